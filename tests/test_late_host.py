"""CPU: the late-interaction reranker without a GPU -- the MaxSim rule (sc_diag_maxsim_host, the header the kernel compiles) against
tests/late_ref.maxsim_rule bit for bit, the two directory layouts through load_late_dir with every refusal, the batching and dedup of
MI355XLateReranker.score_pairs against a fake encoder, and the settings switch."""
import ctypes as C

import numpy as np
import pytest

import late_ref as lr
from semcode_amd import _native
from semcode_amd.embeddings import late
from semcode_amd.embeddings.tokenizer import WordPieceTokenizer


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error():
    buf = C.create_string_buffer(1024)
    _native.lib().sc_last_error(buf, 1024)
    return buf.value.decode()


def maxsim_host(Q, q_off, D, d_off, keep, pq, pd, W):
    out = np.full(len(pq), np.nan, np.float32)
    _native._check(_native.lib().sc_diag_maxsim_host(_p(Q), _p(q_off), len(q_off) - 1, _p(D), _p(d_off), len(d_off) - 1, _p(keep), _p(pq), _p(pd), len(pq), W, _p(out)))
    return out


def make_case(rng, W, nqs, nds, grid=None):
    """Queries of nqs tokens, documents of nds tokens, every pair; grid: values k / grid (ties happen) instead of normals."""
    draw = (lambda *s: rng.standard_normal(s).astype(np.float32)) if grid is None else (lambda *s: (rng.integers(-grid, grid + 1, s) / np.float32(grid)).astype(np.float32))
    q_off = np.concatenate(([0], np.cumsum(nqs))).astype(np.int32)
    d_off = np.concatenate(([0], np.cumsum(nds))).astype(np.int32)
    Q, D = draw(int(q_off[-1]), W), draw(int(d_off[-1]), W)
    pq, pd = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(len(nqs)), np.arange(len(nds)), indexing="ij"))
    return Q, q_off, D, d_off, pq, pd


def expected(Q, q_off, D, d_off, keep, pq, pd):
    return np.array([lr.maxsim_rule(Q[q_off[a]:q_off[a + 1]], D[d_off[b]:d_off[b + 1]], None if keep is None else keep[d_off[b]:d_off[b + 1]]) for a, b in zip(pq, pd)],
                    np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# (W, query lengths, document lengths): W 16 / 96 / 128; nq 1, 17, 32, 128; nd 1, 15, 16, 17, 300
SHAPES = [(16, (1, 17, 32, 128), (1, 15, 16, 17, 300)), (96, (1, 17, 32), (1, 15, 16, 17)), (128, (17, 128), (16, 17, 300))]


@pytest.mark.parametrize("W,nqs,nds", SHAPES)
def test_host_rule_equals_the_restatement(W, nqs, nds):
    rng = np.random.default_rng(W)
    Q, q_off, D, d_off, pq, pd = make_case(rng, W, nqs, nds)
    assert same_bits(maxsim_host(Q, q_off, D, d_off, None, pq, pd, W), expected(Q, q_off, D, d_off, None, pq, pd))
    keep = (rng.random(int(d_off[-1])) < 0.6).astype(np.uint8)
    keep[d_off[:-1]] = 1  # every document keeps a token
    assert same_bits(maxsim_host(Q, q_off, D, d_off, keep, pq, pd, W), expected(Q, q_off, D, d_off, keep, pq, pd))


def test_host_rule_on_ties_zeros_and_negative_documents():
    rng = np.random.default_rng(5)
    Q, q_off, D, d_off, pq, pd = make_case(rng, 16, (1, 17, 32), (1, 15, 16, 17), grid=2)  # a coarse grid: equal dots, exact zeros
    D[d_off[1]:d_off[2]] = -np.abs(D[d_off[1]:d_off[2]])
    Q[:] = np.where(Q == 0, np.float32(-0.0), Q)  # -0 among the operands
    got = maxsim_host(Q, q_off, D, d_off, None, pq, pd, 16)
    assert same_bits(got, expected(Q, q_off, D, d_off, None, pq, pd))
    # the order of a document's tokens does not matter
    Dr = D.copy()
    for i in range(len(d_off) - 1):
        Dr[d_off[i]:d_off[i + 1]] = D[d_off[i]:d_off[i + 1]][::-1]
    assert same_bits(maxsim_host(Q, q_off, Dr, d_off, None, pq, pd, 16), got)
    # a document of negative dots only: the maximum is the least negative one, never a 0 from a masked or missing token
    q = np.zeros((1, 16), np.float32)
    q[0, 0] = 1
    d = np.zeros((17, 16), np.float32)
    d[:, 0] = -np.arange(2, 19)
    one = np.array([0], np.int32)
    out = maxsim_host(q, np.array([0, 1], np.int32), d, np.array([0, 17], np.int32), None, one, one, 16)
    assert out[0] == -2.0
    keep = np.ones(17, np.uint8)
    keep[0] = 0
    assert maxsim_host(q, np.array([0, 1], np.int32), d, np.array([0, 17], np.int32), keep, one, one, 16)[0] == -3.0
    # -0 < +0 under the key order: a maximum over {-0, +0} is +0 wherever it stands; the chain itself starts from +0
    assert lr._unkey(max(lr._key(np.float32(-0.0)), lr._key(np.float32(0.0)))).view(np.uint32) == 0


def test_host_rule_refusals():
    rng = np.random.default_rng(1)
    Q, q_off, D, d_off, pq, pd = make_case(rng, 16, (3,), (5,))
    out = np.zeros(1, np.float32)
    f = _native.lib().sc_diag_maxsim_host
    ok = lambda **k: f(*[_p(k.get(n, v)) if isinstance(k.get(n, v), np.ndarray) or k.get(n, v) is None else k.get(n, v) for n, v in  # noqa: E731
                         (("Q", Q), ("q_off", q_off), ("Bq", 1), ("D", D), ("d_off", d_off), ("Bd", 1), ("keep", None), ("pq", pq), ("pd", pd), ("P", 1), ("W", 16),
                          ("out", out))])
    assert ok() == 0
    for bad in (dict(W=24), dict(W=144), dict(P=0), dict(pq=np.array([1], np.int32)), dict(pd=np.array([-1], np.int32)), dict(q_off=np.array([1, 3], np.int32)),
                dict(q_off=np.array([0, 129], np.int32)), dict(d_off=np.array([0, 0], np.int32)), dict(Q=None)):
        assert ok(**bad) == -1, bad
        assert "sc_diag_maxsim_host" in last_error()


# ---------------------------------------------------------------- the two directory layouts
CASE = lr.CASES["bert128"]


@pytest.fixture(scope="module")
def model():
    blob, proj = lr.make_weights(CASE, 41, 4.0), lr.make_proj(CASE, 41)
    return blob, proj


@pytest.mark.parametrize("layout", ["pylate", "stanford"])
def test_directory_round_trip(tmp_path, model, layout):
    blob, proj = model
    write = lr.write_pylate_dir if layout == "pylate" else lr.write_stanford_dir
    cfg, got_blob, got_proj, meta = late.load_late_dir(write(tmp_path / "m", CASE, blob, proj))
    assert np.array_equal(got_blob, blob) and np.array_equal(got_proj, proj)
    assert {k: cfg[k] for k in ("vocab", "hidden", "layers", "heads", "ffn", "max_pos", "type_vocab")} == {k: CASE["cfg"][k] for k in
                                                                                                            ("vocab", "hidden", "layers", "heads", "ffn", "max_pos", "type_vocab")}
    assert meta["layout"] == layout and meta["query_length"] == 32 and meta["document_length"] == 300
    assert (meta["query_marker"], meta["document_marker"]) == ("[unused0]", "[unused1]")
    assert "." in meta["skiplist"] and late.is_late_dir(tmp_path / "m")


def test_modernbert_directory_round_trip(tmp_path):
    case = lr.CASES["mb256"]
    blob, proj = lr.make_weights(case, 41, 4.0), lr.make_proj(case, 41)
    cfg, got_blob, got_proj, _ = late.load_late_dir(lr.write_pylate_dir(tmp_path / "m", case, blob, proj))
    W, G = lr.mb.unpack(case["cfg"], blob), lr.mb.unpack(case["cfg"], got_blob)
    for k in W:  # (layer 0's attn_norm is not a tensor of the family: its slot comes back as ones)
        assert k == "l0.ln1_g" or np.array_equal(W[k], G[k]), k
    assert cfg["modernbert"] and cfg["local_window"] == 16 and cfg["global_every"] == 3 and np.array_equal(got_proj, proj)


@pytest.mark.parametrize("layout,override,needle", [
    ("pylate", dict(attend_to_expansion_tokens=True), "attend_to_expansion_tokens"), ("stanford", dict(attend_to_mask_tokens=True), "attend_to_mask_tokens"),
    ("pylate", dict(query_length=48), "query length"), ("stanford", dict(query_maxlen=64), "query length"), ("pylate", dict(bias=True), "bias"),
    ("stanford", dict(bias=True), "bias"), ("stanford", dict(dim=64), "dim")])
def test_directory_refusals(tmp_path, model, layout, override, needle):
    write = lr.write_pylate_dir if layout == "pylate" else lr.write_stanford_dir
    with pytest.raises(ValueError, match=needle):
        late.load_late_dir(write(tmp_path / "m", CASE, *model, **override))


def test_directory_without_a_config_file_or_a_projection(tmp_path, model):
    d = lr.write_pylate_dir(tmp_path / "a", CASE, *model)
    (d / "config_sentence_transformers.json").unlink()
    assert not late.is_late_dir(d)
    with pytest.raises(FileNotFoundError, match="artifact.metadata"):
        late.load_late_dir(d)
    d = lr.write_pylate_dir(tmp_path / "b", CASE, *model)
    (d / "1_Dense" / "model.safetensors").unlink()
    with pytest.raises(FileNotFoundError, match="1_Dense"):
        late.load_late_dir(d)


# ---------------------------------------------------------------- batching and dedup against a fake encoder
class FakeEncoder:
    """Records every score_late call; a pair's score is (first word of the question) * 1000 + (document length)."""

    def __init__(self):
        self.calls = []

    def packed_rows(self, offsets):
        return int((((np.diff(offsets) + 31) // 32 * 32).sum() + 255) // 256 * 256)

    def score_late(self, q_ids, q_off, d_ids, d_off, pair_q, pair_d, expand_id=-1, d_keep=None):
        self.calls.append(dict(q_ids=q_ids.copy(), q_off=q_off.copy(), d_ids=d_ids.copy(), d_off=d_off.copy(), pair_q=pair_q.copy(), pair_d=pair_d.copy(),
                               expand_id=expand_id, d_keep=d_keep.copy()))
        return np.array([q_ids[q_off[a] + 2] * 1000.0 + (d_off[b + 1] - d_off[b]) for a, b in zip(pair_q, pair_d)], np.float32)


def fake_reranker(rows_budget):
    cfg = CASE["cfg"]
    tok = WordPieceTokenizer({t: i for i, t in enumerate(lr.vocab_lines(cfg))})
    meta = dict(query_marker="[unused0]", document_marker="[unused1]", query_length=32, document_length=300, skiplist=[".", ",", "!", "?", "#"])
    enc = FakeEncoder()
    return late.MI355XLateReranker(cfg=cfg, tokenizer=tok, meta=meta, encoder=enc, rows_budget=rows_budget), enc


def test_score_pairs_batches_and_dedupes():
    rr, enc = fake_reranker(rows_budget=512)
    qs = ["w20 w21", "w30 w31 w32", "w40"]
    ps = [" ".join(f"w{50 + (i * 7 + j) % 300}" for j in range(n)) + " ." for i, n in enumerate((5, 60, 200, 280, 33, 90, 150))]
    questions = [qs[i % 3] for i in range(14)]
    passages = [ps[i % 7] for i in range(14)]
    got = rr.score_pairs(questions, passages)
    want = np.array([float(q.split()[0][1:]) * 1000 + min(300, len(p.split()) + 3) for q, p in zip(questions, passages)], np.float32)
    assert np.array_equal(got, want)
    assert len(enc.calls) > 1  # the budget of 512 rows cuts the seven passages into several batches
    seen_docs = 0
    for c in enc.calls:
        assert enc.packed_rows(c["d_off"]) <= 512 and c["expand_id"] == lr.MASK_ID
        nd, nq = len(c["d_off"]) - 1, len(c["q_off"]) - 1
        seen_docs += nd
        assert set(c["pair_d"]) == set(range(nd)) and set(c["pair_q"]) == set(range(nq))  # only what the batch pairs, each text once
        first = c["q_ids"][c["q_off"][:-1] + 2]
        assert len(set(first.tolist())) == nq
        assert (c["q_ids"][c["q_off"][:-1] + 1] == lr.Q_ID).all() and (c["d_ids"][c["d_off"][:-1] + 1] == lr.D_ID).all()
        assert (np.diff(c["q_off"]) <= 32).all() and (np.diff(c["d_off"]) <= 300).all()
        assert np.array_equal(c["d_keep"], (~np.isin(c["d_ids"], lr.SKIP_IDS)).astype(np.uint8)) and (c["d_keep"] == 0).any()
    assert seen_docs == len(ps)  # every distinct passage is encoded once in all
    assert rr.score_pairs([], []).shape == (0,)
    order, scores = rr.rerank(qs[0], ps, top_k=3)
    assert list(order) == [3, 2, 6] and np.array_equal(scores, np.array([20284, 20204, 20154], np.float32))  # [CLS] [D] words . [SEP]


def test_long_texts_are_cut():
    rr, _ = fake_reranker(rows_budget=65536)
    long_q = " ".join(f"w{20 + i}" for i in range(60))
    q = rr.query_ids(long_q)
    assert len(q) == 32 and q[:2] == [lr.CLS_ID, lr.Q_ID] and q[-1] == lr.SEP_ID
    d = rr.document_ids(" ".join(f"w{20 + i % 300}" for i in range(500)))
    assert len(d) == 300 and d[:2] == [lr.CLS_ID, lr.D_ID] and d[-1] == lr.SEP_ID


# ---------------------------------------------------------------- the settings switch
def test_settings_switch(tmp_path, model, monkeypatch):
    from semcode_amd.embeddings import providers, reranker
    from semcode_amd.settings import settings

    made = []
    monkeypatch.setattr(late, "MI355XLateReranker", lambda path, **k: made.append(("late", str(path))) or "late")
    monkeypatch.setattr(reranker, "MI355XReranker", lambda path, **k: made.append(("cross", str(path))) or "cross")
    late_dir = lr.write_pylate_dir(tmp_path / "late", CASE, *model)
    plain_dir = tmp_path / "plain"
    plain_dir.mkdir()
    assert settings.mi355x_reranker_kind == "auto"
    assert providers.create_reranker(str(late_dir)) == "late"
    assert providers.create_reranker(str(plain_dir)) == "cross"
    assert providers.create_reranker(str(tmp_path / "x.safetensors")) == "cross"
    monkeypatch.setattr(settings, "mi355x_reranker_kind", "cross")
    assert providers.create_reranker(str(late_dir)) == "cross"
    monkeypatch.setattr(settings, "mi355x_reranker_kind", "late")
    assert providers.create_reranker(str(plain_dir)) == "late"
    monkeypatch.setattr(settings, "mi355x_reranker_kind", "both")
    with pytest.raises(ValueError, match="mi355x_reranker_kind"):
        providers.create_reranker(str(late_dir))
    monkeypatch.setattr(settings, "mi355x_reranker_path", None)
    assert providers.create_reranker() is None
