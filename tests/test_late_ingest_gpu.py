"""GPU: the token hand-over at ingest.  sc_encoder_embed_tokens_into (the token head writes into the index's token pool) and
sc_index_put_tokens_dev (late_install_kernel) against today's path through the host -- sc_encoder_embed_tokens, the keep mask on the
host, sc_index_put_tokens -- bit for bit: stored vectors, counts, statistics, rerank and search results, the files of a saved store.
The models are the seeded ones of tests/golden/late_golden.json."""
import ctypes as C
import json

import numpy as np
import pytest

import late_ref as lr
import late_store_ref as ls
from semcode_amd import _native
from test_late_ingest_host import PATTERNS, keep_pattern

pytestmark = pytest.mark.gpu

DIM = 16
LENS = (1, 2, 15, 16, 17, 31, 32, 33, 180)  # 480 packed rows: the batch crosses a 256-row boundary; + 1 100 where max_pos allows
FORMATS = ("f32", "bf16")
CASE_NAMES = ("bert128", "bert384", "bert768", "mb256")
INVALID, UNSUPPORTED = -1, -4


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error():
    buf = C.create_string_buffer(1024)
    _native.lib().sc_last_error(buf, 1024)
    return buf.value.decode()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Model:
    def __init__(self, rt, name, meta):
        self.name, self.case = name, lr.CASES[name]
        self.cfg, self.W = self.case["cfg"], self.case["W"]
        self.blob = lr.make_weights(self.case, meta[name]["seed"], meta[name]["scale"])
        self.proj = lr.make_proj(self.case, meta[name]["seed"])
        self.enc = _native.Encoder(rt, self.cfg, weights=self.blob)
        self.enc.set_token_head(self.proj)
        self.lens = LENS + ((1100,) if self.cfg["max_pos"] >= 1100 else ())
        rng = np.random.default_rng(len(name))
        self.texts = [np.concatenate(([lr.CLS_ID], rng.integers(lr.FIRST_WORD, self.cfg["vocab"], n - 1))).astype(np.int32) for n in self.lens]
        self.ids, self.off = lr.pack(self.texts)
        self._vec = None

    def vectors(self):
        """What sc_encoder_embed_tokens returns for the texts, computed once: one [len_i, W] array per text."""
        if self._vec is None:
            vec, counts = self.enc.embed_tokens(self.ids, self.off)
            assert counts.tolist() == list(self.lens)
            self._vec = np.split(vec, np.cumsum(counts)[:-1])
        return self._vec


@pytest.fixture(scope="module")
def models(rt, golden):
    meta = json.loads((golden / "late_golden.json").read_text())
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(rt, name, meta)
        return made[name]

    yield get
    for m in made.values():
        m.enc.close()


def new_index(rt, n, seed=0):
    ix = _native.Index(rt, DIM, metric="IP")
    ix.add(ls.unit_rows(np.random.default_rng(seed), n, DIM))
    return ix


def host_put(ix, enc, ids, off, keep, rows, fmt, vecs=None):
    """Today's path: download, one boolean mask per text, upload."""
    if vecs is None:
        vec, counts = enc.embed_tokens(ids, off)
        vecs = np.split(vec, np.cumsum(counts)[:-1])
    if keep is not None:
        vecs = [v[keep[off[i]:off[i + 1]] != 0] for i, v in enumerate(vecs)]
    ix.put_tokens(rows, vecs, fmt=fmt)
    return np.asarray([len(v) for v in vecs], np.int32)


def assert_same_store(a, b, n, what):
    sa, sb = a.token_stats(), b.token_stats()
    assert {k: sa[k] for k in ("rows_with_tokens", "live", "dead", "W", "fmt")} == {k: sb[k] for k in ("rows_with_tokens", "live", "dead", "W", "fmt")}, (what, sa, sb)
    ca, va = a.get_tokens(np.arange(n))
    cb, vb = b.get_tokens(np.arange(n))
    assert np.array_equal(ca, cb) and np.array_equal(bits(va), bits(vb)), what
    return ca, va


# ---------------------------------------------------------------- 1. the same bits as the host path
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_handover_stores_the_bits_of_the_host_path(rt, models, name, fmt):
    m = models(name)
    n = len(m.texts)
    rows = np.arange(n)
    A, B = new_index(rt, n + 1), new_index(rt, n + 1)
    rng = np.random.default_rng(3)
    three = ls.unit_rows(rng, 3, m.W)
    for ix in (A, B):  # used is not a multiple of 16 when the hand-over writes
        ix.put_tokens([n], [three], fmt=fmt)
    questions = [ls.unit_rows(rng, 5, m.W), ls.unit_rows(rng, 32, m.W)]
    allow = rng.random(n + 1) < 0.6
    cand = np.tile(np.arange(n + 1), (2, 1))
    for pattern in PATTERNS:
        keep = keep_pattern(pattern, m.lens, seed=len(name))
        want = host_put(A, m.enc, m.ids, m.off, keep, rows, fmt, vecs=m.vectors())
        got = m.enc.embed_tokens_into(m.ids, m.off, keep, B, rows, fmt)
        assert np.array_equal(got, want), pattern
        counts, vecs = assert_same_store(A, B, n + 1, (name, fmt, pattern))
        assert counts[:n].tolist() == want.tolist() and counts[n] == 3
        if pattern == "none":
            assert counts[:n].sum() == 0 and B.token_stats()["rows_with_tokens"] == 1
        if fmt == "bf16":
            assert (bits(vecs) & 0xFFFF == 0).all()
        assert np.array_equal(bits(A.rerank_late(questions, cand)), bits(B.rerank_late(questions, cand))), pattern
        for al in (None, allow):
            sa, ra = A.search_late(questions, k=10, allow=al)
            sb, rb = B.search_late(questions, k=10, allow=al)
            assert np.array_equal(ra, rb) and np.array_equal(bits(sa), bits(sb)), pattern
    A.close()
    B.close()


# ---------------------------------------------------------------- 2. a text's stored vectors do not depend on its batch-mates
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stored_vectors_do_not_depend_on_the_batch(rt, models, name, fmt):
    m = models(name)
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 120, 24)
    lens[5] = 77
    texts = [np.concatenate(([lr.CLS_ID], rng.integers(lr.FIRST_WORD, m.cfg["vocab"], n - 1))).astype(np.int32) for n in lens]
    flags = [(rng.random(n) < 0.7).astype(np.uint8) for n in lens]
    flags[5][[0, 15, 16, 76]] = (0, 1, 0, 1)
    ix = new_index(rt, 3 * 24)
    one_ids, one_off = lr.pack([texts[5]])
    m.enc.embed_tokens_into(one_ids, one_off, flags[5], ix, [0], fmt)
    ids, off = lr.pack(texts)
    m.enc.embed_tokens_into(ids, off, np.concatenate(flags), ix, np.arange(24, 48), fmt)
    ids, off = lr.pack(texts[::-1])
    m.enc.embed_tokens_into(ids, off, np.concatenate(flags[::-1]), ix, np.arange(48, 72), fmt)
    (c0, v0), (c1, v1), (c2, v2) = ix.get_tokens([0]), ix.get_tokens([24 + 5]), ix.get_tokens([48 + 23 - 5])
    assert c0[0] == c1[0] == c2[0] == int(flags[5].sum()) > 0
    assert np.array_equal(bits(v0), bits(v1)) and np.array_equal(bits(v0), bits(v2))
    ix.close()


# ---------------------------------------------------------------- 3. sc_index_put_tokens_dev against sc_index_put_tokens
def crafted_values():
    """f32 bit patterns whose bf16 rounding has a rule of its own: zeros, denormals, ties, overflow, infinities, NaNs."""
    u = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,
                  0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF,
                  0xFF80FFFF, 0x7FFFFFFF, 0x7F810000, 0x3F800000, 0x33800000, 0x0000FFFF, 0x00010000, 0x80008000, 0x7FFF8000], np.uint32)
    return u.view(np.float32)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W", [16, 96, 128])
def test_put_tokens_dev_equals_put_tokens(rt, W, fmt):
    import torch

    rng = np.random.default_rng(W)
    counts = np.array([1, 0, 17, 16, 33, 2, 200, 15], np.int32)
    T = int(counts.sum()) + 40  # the device array holds more tokens than are stored
    vecs = ls.unit_rows(rng, T, W)
    special = crafted_values()
    vecs[:2, :] = np.resize(special, 2 * W).reshape(2, W)  # (W = 16: all 32 of them; wider: repeated)
    dev = torch.from_numpy(vecs).cuda()
    torch.cuda.synchronize()
    rows = np.array([7, 3, 0, 5, 9, 1, 2, 8])
    total = int(counts.sum())
    A, B = new_index(rt, 10), new_index(rt, 10)
    three = ls.unit_rows(rng, 3, W)
    for ix in (A, B):
        ix.put_tokens([4], [three], fmt=fmt)
    # without a list: the first sum(counts) tokens in order
    A.put_tokens(rows, (counts, vecs[:total]), fmt=fmt)
    B.put_tokens_dev(rows, counts, dev.data_ptr(), None, W, fmt)
    _, stored = assert_same_store(A, B, 10, "in order")
    first = B.get_tokens([7])[1]  # row 7 holds token 0: the crafted values
    want = vecs[:1] if fmt == "f32" else _native.diag_round_bf16(vecs[:1])
    assert np.array_equal(bits(first), bits(want))
    # a gather list: a permutation with gaps; the rows' old tokens become dead
    src = rng.permutation(T)[:total].astype(np.int32)
    src[:2] = (1, 0)
    A.put_tokens(rows, (counts, vecs[src]), fmt=fmt)
    B.put_tokens_dev(rows, counts, dev.data_ptr(), src, W, fmt)
    assert_same_store(A, B, 10, "gathered")
    got = B.get_tokens(rows)[1]
    assert np.array_equal(bits(got), bits(vecs[src] if fmt == "f32" else _native.diag_round_bf16(vecs[src])))
    if fmt == "bf16":  # the crafted values, one by one, against the rounding rule of the store
        r = _native.diag_round_bf16(special)
        on_device = np.concatenate([got[1], got[0]])[: len(special)]  # (stored tokens 0 and 1 are source tokens 1 and 0: the crafted values)
        assert np.array_equal(bits(on_device), bits(r))
        by_hand = {0x3F808000: 0x3F800000, 0x3F818000: 0x3F820000, 0x7F7FFFFF: 0x7F800000, 0xFF7FFFFF: 0xFF800000, 0x00000001: 0x00000000, 0x80000001: 0x80000000,
                   0x00008000: 0x00000000, 0x00018000: 0x00020000, 0x7F800000: 0x7F800000, 0xFF800000: 0xFF800000, 0x00000000: 0x00000000, 0x80000000: 0x80000000}
        for src_bits, want_bits in by_hand.items():
            assert int(bits(r)[list(bits(special)).index(src_bits)]) == want_bits, hex(src_bits)
        nan_in = np.isnan(special)
        assert nan_in.sum() >= 6 and np.isnan(r[nan_in]).all() and not np.isnan(r[~nan_in]).any()
    # counts of zero alone: the rows lose their tokens, no vector is read
    A.put_tokens([0, 2], (np.zeros(2, np.int32), np.empty((0, W), np.float32)), fmt=fmt)
    B.put_tokens_dev([0, 2], np.zeros(2, np.int32), 0, None, W, fmt)
    assert_same_store(A, B, 10, "removed")
    A.close()
    B.close()


# ---------------------------------------------------------------- 4. accounting under mutation
@pytest.mark.parametrize("fmt", FORMATS)
def test_accounting_under_mutation_equals_the_host_path(rt, models, fmt):
    m = models("bert128")
    rng = np.random.default_rng(2024)
    N = 30
    A, B = new_index(rt, N), new_index(rt, N)
    n = N
    autos = 0

    def texts_for(k, lo, hi):
        lens = rng.integers(lo, hi, k)
        return [np.concatenate(([lr.CLS_ID], rng.integers(lr.FIRST_WORD, m.cfg["vocab"], x - 1))).astype(np.int32) for x in lens]

    def into(rows, texts, pattern):
        nonlocal autos
        ids, off = lr.pack(texts)
        keep = keep_pattern(pattern, [len(t) for t in texts], seed=len(rows))
        dead_before = B.token_stats()["dead"]
        replaced = int(B.token_counts(rows).sum())
        host_put(A, m.enc, ids, off, keep, rows, fmt)
        m.enc.embed_tokens_into(ids, off, keep, B, rows, fmt)
        autos += B.token_stats()["dead"] == 0 and dead_before + replaced > 0

    steps = [
        lambda: into(np.arange(0, 20), texts_for(20, 20, 60), "ones"),                           # rows without tokens
        lambda: into(rng.choice(n, 8, replace=False), texts_for(8, 1, 40), "random70"),          # rows with and without
        lambda: (A.delete_rows([1, 4, 25]), B.delete_rows([1, 4, 25])),
        lambda: into(rng.choice(n, 10, replace=False), texts_for(10, 5, 50), "alternating"),
        lambda: (A.compact_tokens(), B.compact_tokens()),
        lambda: into(np.arange(n), texts_for(n, 30, 60), "null"),                                # every row replaced
        lambda: into(np.arange(n), texts_for(n, 30, 60), "first"),                               # 1 live against 30 .. 59 dead per row -> automatic
        lambda: into(rng.choice(n, 5, replace=False), texts_for(5, 2, 30), "none"),              # tokens removed
        lambda: (A.delete_rows(np.arange(0, n, 5)), B.delete_rows(np.arange(0, n, 5))),
        lambda: into(rng.choice(n, 6, replace=False), texts_for(6, 17, 34), "last"),
        lambda: into(rng.choice(n, 12, replace=False), texts_for(12, 1, 20), "random70"),
        lambda: (A.compact_tokens(), B.compact_tokens()),
    ]
    assert len(steps) == 12
    for i, step in enumerate(steps):
        step()
        n = len(B)
        assert len(A) == n
        sa, sb = A.token_stats(), B.token_stats()
        assert (sa["rows_with_tokens"], sa["live"], sa["dead"]) == (sb["rows_with_tokens"], sb["live"], sb["dead"]), (i, sa, sb)
    assert autos >= 1
    assert_same_store(A, B, n, "after the sequence")
    A.close()
    B.close()


# ---------------------------------------------------------------- 5. refusals change nothing
def test_refusals_change_nothing(rt, models):
    lib = _native.lib()
    m = models("bert128")
    W = m.W
    ix = new_index(rt, 12)
    texts = m.texts[2:6]
    ids, off = lr.pack(texts)
    keep = keep_pattern("random70", [len(t) for t in texts])
    m.enc.embed_tokens_into(ids, off, keep, ix, [0, 1, 2, 3], "f32")
    st0 = ix.token_stats()
    tok0 = ix.get_tokens([0, 1, 3])
    rows = np.array([4, 5, 6, 7], np.int64)
    counts = np.zeros(4, np.int32)

    def unchanged(what):
        assert ix.token_stats() == st0, what
        c, v = ix.get_tokens([0, 1, 3])
        assert np.array_equal(c, tok0[0]) and np.array_equal(bits(v), bits(tok0[1])), what

    def into_rc(**k):
        a = dict(enc=m.enc.handle, ids=ids, off=off, B=4, keep=keep, ix=ix.handle, rows=rows, fmt=0, counts=counts)
        a.update(k)
        return lib.sc_encoder_embed_tokens_into(a["enc"], _p(a["ids"]), _p(a["off"]), a["B"], _p(a["keep"]), a["ix"], _p(a["rows"]), a["fmt"], _p(a["counts"]))

    rt2 = _native.Runtime(device=0)
    other = _native.Index(rt2, DIM, metric="IP")
    other.add(ls.unit_rows(np.random.default_rng(1), 12, DIM))
    wide = models("bert384")  # a head of another W
    q2 = _native.Encoder(rt, dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0, hidden=128, heads=2,
                                  kv_heads=1, ffn=256, layers=1), synth_seed=2)
    big = np.full(512 * 1025, lr.FIRST_WORD, np.int32)  # 1 025 texts of max_pos tokens: more rows than one packed call may have
    big_off = np.arange(1026, dtype=np.int64) * 512
    cases = [
        (dict(enc=None), INVALID, "NULL"), (dict(ids=None), INVALID, "NULL"), (dict(off=None), INVALID, "NULL"), (dict(ix=None), INVALID, "NULL"),
        (dict(rows=None), INVALID, "NULL"),
        (dict(fmt=2), INVALID, "fmt must be"), (dict(fmt=-1), INVALID, "fmt must be"),
        (dict(fmt=1), INVALID, "holds tokens of W=32 fmt=0"), (dict(enc=wide.enc.handle), INVALID, "holds tokens of W=32"),
        (dict(ix=other.handle), INVALID, "different runtimes"),
        (dict(rows=np.array([4, 5, 6, 12], np.int64)), INVALID, "out of range"), (dict(rows=np.array([-1, 5, 6, 7], np.int64)), INVALID, "out of range"),
        (dict(rows=np.array([4, 5, 5, 7], np.int64)), INVALID, "distinct"),
        (dict(off=off + 1), INVALID, "offsets[0]"), (dict(off=np.array([0, 3, 3, 5, 9], np.int64)), INVALID, "length 0"),
        (dict(ids=np.full(513, lr.FIRST_WORD, np.int32), off=np.array([0, 513], np.int64), B=1, keep=None, rows=rows[:1]), INVALID, "more than 512"),
        (dict(B=0), INVALID, "batch 0"),
        (dict(enc=q2.handle), UNSUPPORTED, "arch 2"),
        (dict(ids=big, off=big_off, B=1025, keep=None, rows=np.arange(1025, dtype=np.int64)), UNSUPPORTED, "SC_ENCODER_PACKED_MAX_ROWS"),
    ]
    for kw, code, needle in cases:
        rc = into_rc(**kw)
        assert rc == code and "sc_encoder_embed_tokens_into" in last_error() and needle in last_error(), (list(kw), rc, last_error())
        unchanged(list(kw))
    m.enc.set_token_head(None)
    assert into_rc() == INVALID and "no token head" in last_error()
    unchanged("no head")
    m.enc.set_token_head(m.proj)
    assert other.token_stats()["W"] == 0  # (the refused call created no store on the other index either)

    # sc_index_put_tokens_dev: the refusals of sc_index_put_tokens, and its own
    import torch

    dev = torch.from_numpy(ls.unit_rows(np.random.default_rng(2), 8, W)).cuda()
    torch.cuda.synchronize()
    cnt = np.array([1, 2, 0, 3], np.int32)

    def dev_rc(**k):
        a = dict(rows=rows, n=4, counts=cnt, vecs=dev.data_ptr(), src=None, W=W, fmt=0)
        a.update(k)
        return lib.sc_index_put_tokens_dev(ix.handle, _p(a["rows"]), a["n"], _p(a["counts"]), C.c_void_p(a["vecs"]) if a["vecs"] else None, _p(a["src"]), a["W"], a["fmt"])

    for kw, needle in ((dict(rows=None), "bad argument"), (dict(counts=None), "bad argument"), (dict(n=-1), "bad argument"), (dict(vecs=0), "vecs_dev is NULL"),
                       (dict(W=24), "multiple of 16"), (dict(W=16), "holds tokens of W=32"), (dict(fmt=1), "holds tokens of W=32"), (dict(fmt=2), "fmt must be"),
                       (dict(counts=np.array([1, 2049, 0, 0], np.int32)), "outside 0 .. 2048"), (dict(counts=np.array([-1, 1, 0, 0], np.int32)), "outside 0 .. 2048"),
                       (dict(rows=np.array([4, 5, 6, 12], np.int64)), "out of range"), (dict(rows=np.array([4, 4, 6, 7], np.int64)), "distinct"),
                       (dict(src=np.array([0, 1, 2, 3, -1, 5], np.int32)), "src[4] = -1")):
        assert dev_rc(**kw) == INVALID and "sc_index_put_tokens_dev" in last_error() and needle in last_error(), (list(kw), last_error())
        unchanged(list(kw))
    # ... and the accepted forms of both still work on this store afterwards
    assert dev_rc(src=np.array([7, 6, 5, 4, 3, 2], np.int32)) == 0 and into_rc(rows=np.array([8, 9, 10, 11], np.int64)) == 0
    assert counts.tolist() == [int(keep[off[i]:off[i + 1]].sum()) for i in range(4)]
    assert ix.token_stats()["live"] == st0["live"] + 6 + int(counts.sum())
    for h in (q2, other, ix):
        h.close()
    rt2.close()


# ---------------------------------------------------------------- 6. through the store
class Spy:
    """Counts what an ingest with the hand-over may not do: embed_document_tokens, and Encoder.embed_tokens for documents."""

    def __init__(self, reranker):
        self.embed_document_tokens = self.embed_tokens_docs = self.stored = 0
        enc = reranker._encoder
        edt, et, sdt = reranker.embed_document_tokens, enc.embed_tokens, reranker.store_document_tokens

        def counted_edt(*a, **k):
            self.embed_document_tokens += 1
            return edt(*a, **k)

        def counted_et(ids, off, expand_id=-1, **k):
            self.embed_tokens_docs += expand_id < 0
            return et(ids, off, expand_id=expand_id, **k)

        def counted_sdt(*a, **k):
            self.stored += 1
            return sdt(*a, **k)

        reranker.embed_document_tokens, enc.embed_tokens, reranker.store_document_tokens = counted_edt, counted_et, counted_sdt

    def take(self):
        got = (self.embed_document_tokens, self.embed_tokens_docs, self.stored)
        self.embed_document_tokens = self.embed_tokens_docs = self.stored = 0
        return got


@pytest.mark.parametrize("fmt", FORMATS)
def test_through_the_store(rt, golden, tmp_path, monkeypatch, fmt):
    from pathlib import Path

    from semcode_amd.embeddings.late import MI355XLateReranker
    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from semcode_amd.services import Retriever, ingest_chunks
    from semcode_amd.settings import settings
    from semcode_amd.storage import MilvusVectorStore
    from test_seams_gpu import Chunk

    meta = json.loads((golden / "late_golden.json").read_text())["bert128"]
    case = lr.CASES["bert128"]
    cfg = case["cfg"]
    blob, proj = lr.make_weights(case, meta["seed"], meta["scale"]), lr.make_proj(case, meta["seed"])
    monkeypatch.setattr(settings, "rag_max_context_sources", 5)
    monkeypatch.setattr(settings, "milvus_upsert_batch_size", 16)
    monkeypatch.setattr(settings, "mi355x_ingest_batch", 16, raising=False)
    vocab = {w: i for i, w in enumerate(lr.vocab_lines(cfg))}
    emb = MI355XEmbeddings(cfg=dict(cfg), vocab=vocab, runtime=rt, synth_seed=3, allow_synthetic=True)
    reranker = MI355XLateReranker(lr.write_pylate_dir(tmp_path / "m", case, blob, proj), runtime=rt, rows_budget=512)  # (several hand-over calls per commit)
    spy = Spy(reranker)
    rng = np.random.default_rng(21)
    root = Path("/w/demo")
    N = 40
    texts = [f"w{20 + i} . " + " , ".join(f"w{int(j)}" for j in rng.integers(40, 400, int(rng.integers(5, 50)))) for i in range(N)]
    texts[7] = ". , ! ?"  # nothing but punctuation between the markers: [CLS], the marker and [SEP] are what is kept
    chunks = [Chunk(t, root / ("pkg" if i % 2 else "lib") / f"k{i}.py", "python" if i % 3 else "go", 1, 3) for i, t in enumerate(texts)]
    vectors = emb.embed_documents_array(texts)
    ids = [f"k{i}" for i in range(N)]
    metas = [{"repo": "demo", "path": f"k{i}.py", "language": "python"} for i in range(N)]

    def make_store(name, handover):
        s = MilvusVectorStore(collection_name=name, dim=cfg["hidden"], metric="COSINE", index_type="FLAT", runtime=rt, late=reranker, late_format=fmt, late_handover=handover)
        s.connect()
        return s

    saved = {}
    for how in ("arrays", "ingest"):
        for handover in (True, False):
            s = make_store(f"{how}{handover}", handover)
            spy.take()
            if how == "arrays":
                s.upsert_arrays(ids, vectors, texts, metas)
                s.upsert_arrays(ids[3:9], vectors[3:9], texts[10:16], metas[3:9])  # replaced keys: their rows' tokens are replaced
            else:
                assert ingest_chunks("demo", root, chunks, emb, s) == N
            edt, et, stored = spy.take()
            if handover:
                assert (edt, et) == (0, 0) and stored >= 3
            else:
                assert stored == 0 and edt >= 3 and et >= edt
            st = s._collection.token_stats()
            assert st["fmt"] == fmt and st["W"] == case["W"] and st["rows_with_tokens"] == N
            s.save(tmp_path / f"{how}{handover}")
            saved[(how, handover)] = s
        a, b = tmp_path / f"{how}True", tmp_path / f"{how}False"
        for f in (f"tokens.{fmt}", "token_counts.i32"):
            assert (a / f).read_bytes() == (b / f).read_bytes() and (a / f).stat().st_size > 0, (how, f)
        on, off_ = saved[(how, True)], saved[(how, False)]
        questions = ["w25 w26", "w40 , w77 w300", "w21"]
        r_on, r_off = Retriever(emb, on, reranker=reranker), Retriever(emb, off_, reranker=reranker)
        for q in questions:
            for kw in (dict(rerank=True, fetch_k=40), dict(late=True)):
                got, want = r_on.retrieve(q, **kw), r_off.retrieve(q, **kw)
                assert r_on.last_error is None and r_off.last_error is None and len(want) == 5
                assert [(d["path"], np.float32(d["score"]).view(np.uint32)) for d in got] == [(d["path"], np.float32(d["score"]).view(np.uint32)) for d in want], (how, q, kw)
    for s in saved.values():
        s.close()
    reranker.close()
    emb.close()
