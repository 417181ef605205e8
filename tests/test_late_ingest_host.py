"""CPU: the host side of the token hand-over at ingest (sc_encoder_embed_tokens_into) -- the plan rule for keep flags through
sc_diag_encoder_plan_keep against a NumPy restatement, the ABI additions, and the store's choice between the hand-over and the path
through the host.  No device, no encoder."""
import re
from pathlib import Path

import numpy as np
import pytest

from semcode_amd import _native as nv

ROOT = Path(__file__).resolve().parent.parent
LENS = (1, 2, 15, 16, 17, 31, 32, 33, 180, 1100)  # 1 600 packed rows: the batch crosses six 256-row boundaries
PATTERNS = ("null", "ones", "none", "first", "last", "alternating", "random70")


def keep_pattern(name: str, lens, seed: int = 0) -> "np.ndarray | None":
    """One byte per token of the flattened batch (None: the NULL pointer).  random70: seeded, 70 % kept, so that dropped rows fall inside,
    at the start and at the end of a 16-row tile."""
    total = int(np.sum(lens))
    off = np.concatenate(([0], np.cumsum(lens)))
    if name == "null":
        return None
    if name == "ones":
        return np.ones(total, np.uint8)
    keep = np.zeros(total, np.uint8)
    if name == "first":
        keep[off[:-1]] = 1
    elif name == "last":
        keep[off[1:] - 1] = 7  # (any value but 0 keeps)
    elif name == "alternating":
        keep[::2] = 1
    elif name == "random70":
        keep[:] = np.random.default_rng(700 + seed).random(total) < 0.7
    elif name != "none":
        raise ValueError(name)
    return keep


def plan_ref(lens, keep):
    """dst [M], counts [B]: text i owns the rows [start_i, start_i + ceil32(len_i)); a kept token's row takes the next number."""
    lens = np.asarray(lens, np.int64)
    spans = (lens + 31) // 32 * 32
    rows = int(spans.sum())
    M = (rows + 255) // 256 * 256
    dst = np.full(M, -1, np.int32)
    flags = np.ones(int(lens.sum()), bool) if keep is None else np.asarray(keep) != 0
    counts, at, tok, start = [], 0, 0, 0
    for n, span in zip(lens.tolist(), spans.tolist()):
        k = flags[tok:tok + n]
        dst[start:start + n][k] = np.arange(at, at + int(k.sum()))
        counts.append(int(k.sum()))
        at, tok, start = at + int(k.sum()), tok + n, start + span
    return dst, np.asarray(counts, np.int32), rows, M


@pytest.mark.parametrize("pattern", PATTERNS)
def test_keep_flags_enter_the_plan(pattern):
    for lens in (LENS, LENS[::-1], (1,), (33,), (180,) * 3):
        keep = keep_pattern(pattern, lens)
        ids = np.arange(3, 3 + int(np.sum(lens)), dtype=np.int32) % 30000
        off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        got = nv.diag_encoder_plan_keep(ids, off, keep)
        dst, counts, rows, M = plan_ref(lens, keep)
        assert int(got["rows"][0]) == rows and int(got["M"][0]) == M and int(got["nrows"][0]) == int(np.sum(lens))
        assert np.array_equal(got["counts"], counts) and int(got["kept"][0]) == int(counts.sum())
        assert np.array_equal(got["dst"], dst), (pattern, lens)
        # -1 exactly on dropped, alignment and tail rows; the kept rows are 0 .. kept - 1 in row order
        kept_rows = got["dst"][got["dst"] >= 0]
        assert np.array_equal(kept_rows, np.arange(int(counts.sum())))
        # everything but dst is the plan of the plain document call: a dropped token is still a row of the forward
        plain = nv.diag_encoder_plan(ids, off, kind="tokens", expand_id=-1)
        for name in ("ids", "pos", "starts", "lens"):
            assert np.array_equal(got[name], plain[name]), name
        if pattern in ("null", "ones"):
            assert np.array_equal(got["dst"], plain["dst"])


def test_the_plan_entry_keeps_the_refusals_of_a_document_token_call():
    ids = np.zeros(600, np.int32)
    for off, kw, needle in (([3, 8], {}, "offsets[0] must be 0"), ([0, 4, 4], {}, "has length 0"), ([0, 513], dict(max_pos=512), "more than 512"),
                            ([0, 2049], dict(pos_type=1), "more than 2048")):
        with pytest.raises(nv.ScError, match=re.escape("sc_diag_encoder_plan_keep: ")) as e:
            nv.diag_encoder_plan_keep(np.zeros(off[-1], np.int32), np.asarray(off, np.int64), None, **kw)
        assert needle in str(e.value)
    with pytest.raises(ValueError, match="one flag per token"):
        nv.diag_encoder_plan_keep(ids, np.array([0, 600], np.int64), np.ones(599, np.uint8))
    # sc_diag_encoder_plan itself is as it was: same signature, no flags
    assert len(nv.SIGNATURES["sc_diag_encoder_plan"][1]) == 17


def test_abi_additions_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "semcode_hip.h").read_text(), flags=re.S)
    lib = nv.lib()
    for name, nargs in (("sc_encoder_embed_tokens_into", 9), ("sc_index_put_tokens_dev", 8), ("sc_diag_encoder_plan_keep", 10)):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and len(nv.SIGNATURES[name][1]) == nargs
    assert callable(nv.Encoder.embed_tokens_into) and callable(nv.Index.put_tokens_dev)


class Ix:
    """A stand-in vector index: remembers what it is handed."""

    def __init__(self, **k):
        self.n, self.tokens, self.rt = 0, {}, "runtime"

    def put_rows(self, vectors, rows):
        self.n = max(self.n, int(rows.max()) + 1)

    def __len__(self):
        return self.n

    def put_tokens(self, rows, toks, fmt="f32"):
        for r, t in zip(rows.tolist(), toks):
            self.tokens[r] = ("host", fmt, t.shape)


class HostOnlyLate:
    """A late object of before the hand-over: no store_document_tokens."""

    def __init__(self):
        self.embedded = 0

    def embed_document_tokens(self, texts, kept_only=False):
        assert kept_only
        self.embedded += 1
        return [np.full((len(t), 16), i, np.float32) for i, t in enumerate(texts)]


class HandoverLate(HostOnlyLate):
    def __init__(self, shares=True):
        super().__init__()
        self.stored, self.shares = 0, shares

    def shares_runtime(self, index):
        return self.shares

    def store_document_tokens(self, texts, index, rows, fmt="f32"):
        self.stored += 1
        for r, t in zip(np.asarray(rows).tolist(), texts):
            index.tokens[r] = ("device", fmt, (len(t), 16))
        return np.asarray([len(t) for t in texts], np.int32)


def test_store_takes_the_handover_only_where_it_can(monkeypatch):
    from semcode_amd.settings import Settings
    from semcode_amd.storage import MilvusVectorStore

    def run(late, **k):
        s = MilvusVectorStore(dim=2, index_factory=Ix, late=late, late_format="bf16", **k)
        s.connect()
        s.upsert_arrays(["a", "b"], np.zeros((2, 2), np.float32), ["xx", "yyy"], [{}, {}])
        return s

    old = HostOnlyLate()  # a late object without the method: the path of before
    s = run(old)
    assert s._collection.tokens == {0: ("host", "bf16", (2, 16)), 1: ("host", "bf16", (3, 16))} and old.embedded == 1
    new = HandoverLate()
    s = run(new)
    assert s.late_handover and s._collection.tokens == {0: ("device", "bf16", (2, 16)), 1: ("device", "bf16", (3, 16))} and (new.stored, new.embedded) == (1, 0)
    # token_vectors= handed through: always the host path, whatever the reranker can do
    s.upsert_arrays(["b"], np.zeros((1, 2), np.float32), ["zzzz"], [{}], token_vectors=[np.ones((7, 16), np.float32)])
    assert s._collection.tokens[1] == ("host", "bf16", (7, 16)) and (new.stored, new.embedded) == (1, 0)
    # another runtime, the constructor switch, the setting: the host path
    other = HandoverLate(shares=False)
    assert run(other)._collection.tokens[0][0] == "host" and (other.stored, other.embedded) == (0, 1)
    off = HandoverLate()
    assert run(off, late_handover=False)._collection.tokens[0][0] == "host" and (off.stored, off.embedded) == (0, 1)
    assert Settings().mi355x_late_handover is True
    monkeypatch.setenv("SEMCODE_MI355X_LATE_HANDOVER", "0")
    assert Settings().mi355x_late_handover is False
    import semcode_amd.storage.milvus_store as ms

    monkeypatch.setattr(ms, "_resolve_settings", lambda: Settings())
    env = HandoverLate()
    s = run(env)
    assert not s.late_handover and s._collection.tokens[0][0] == "host" and (env.stored, env.embedded) == (0, 1)


def test_reranker_shares_a_runtime_only_with_an_index_of_its_own():
    from semcode_amd.embeddings.late import MI355XLateReranker

    class Tok:
        vocab = {"[MASK]": 3, "[unused0]": 4, "[unused1]": 5, ".": 6}

        def encode(self, text, max_tokens):
            return [1] + [12 + len(w) for w in text.split()][: max_tokens - 2] + [2]

    class Enc:  # a stand-in encoder: no runtime, so nothing to share
        def packed_rows(self, offsets):
            return 256

    meta = dict(query_marker="[unused0]", document_marker="[unused1]", document_length=64, skiplist=["."])
    r = MI355XLateReranker(cfg=dict(max_pos=512), tokenizer=Tok(), meta=meta, encoder=Enc())
    assert hasattr(r, "store_document_tokens") and not r.shares_runtime(Ix())
    enc = Enc()
    enc.rt, enc.embed_tokens_into = object(), lambda *a: None
    r2 = MI355XLateReranker(cfg=dict(max_pos=512), tokenizer=Tok(), meta=meta, encoder=enc)
    assert not r2.shares_runtime(Ix())  # another runtime
    ix = Ix()
    ix.rt = enc.rt
    assert r2.shares_runtime(ix)
