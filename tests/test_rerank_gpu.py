"""GPU: the reranker path (sc_encoder_score_pairs, sc_diag_pair_head, sc_diag_embed_pairs) through the C ABI.

Bounds.
  pair_head_kernel against float64 on the same f32 inputs.  A dot product of H f32 terms accumulated in f32, in any order, is off by at
  most gamma_H sum|a_k w_k| with gamma_H <= 2 H 2^-24 (every partial sum is rounded once, relative error 2^-24 each, first order doubled
  for the higher ones), so a value is held to  2 H 2^-24 sum_k |a_k w_k| + 2^-21  (the constant covers the bias add and the final
  rounding of values near zero).  With a pooler the bound is applied twice: the pre-activation a_n has error E_n by that formula, tanh is
  monotone, so p_n is off by at most max|tanh(a_n +- E_n) - tanh(a_n)| + 2^-22 (the device tanh is good to 2 ulp of a value <= 1), and
  the logit is off by sum_n |Wc_n| dp_n plus the formula over the terms Wc_n p_n.
  Typed embedding: the project's 2^-8 of the output scale (tests/test_encoder_gpu.py header).
  Whole path: T_logit / T_cls of tests/golden/rerank_golden.json -- twice what transformers' own bf16 forward misses its fp32 forward by
  (scripts/gen_rerank_fixtures.py) -- and the project's cos >= 0.999 for the [CLS] rows.
"""
import ctypes as C
import json

import numpy as np
import pytest

import fold_ref as fr
import rerank_ref as rr
from semcode_amd import _native

pytestmark = pytest.mark.gpu

lib = _native.lib
U24 = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error():
    buf = C.create_string_buffer(1024)
    lib().sc_last_error(buf, 1024)
    return buf.value.decode()


# ------------------------------------------------------------------ pair_head_kernel alone
def head_case(B, H, nl, pooler, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    cls = f(B, H)
    wp, bp = (f(H, H) / np.float32(np.sqrt(H)), np.float32(0.1) * f(H)) if pooler else (None, None)
    if pooler:  # saturation: pre-activations of +-1e4 (row 1), of +-3e38 (rows 2, 3: one term each, no inf - inf), far negative bias (row 4)
        wp[1] *= np.float32(1e4)
        wp[2] = 0
        wp[2, 5] = 3e38
        wp[3] = 0
        wp[3, 7] = -3e38
        cls[:, 5] = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
        cls[:, 7] = 1.0
        bp[4] = -1e30
    return cls, wp, bp, f(nl, H), f(nl)


def head_ref(cls, wp, bp, wc, bc):
    """(logits, bound per logit) in float64."""
    H = cls.shape[1]
    x, wc64, g = cls.astype(np.float64), wc.astype(np.float64), 2.0 * H * U24
    if wp is None:
        pv, dp = x, np.zeros_like(x)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            w64, b64 = wp.astype(np.float64), bp.astype(np.float64)
            a = x @ w64.T + b64
            E = g * (np.abs(x) @ np.abs(w64).T + np.abs(b64)) + 2.0 ** -21
            pv = np.tanh(a)
            dp = np.maximum(np.abs(np.tanh(a + E) - pv), np.abs(np.tanh(a - E) - pv)) + 2.0 ** -22
    logits = pv @ wc64.T + bc.astype(np.float64)
    bound = dp @ np.abs(wc64).T + g * (np.abs(pv) @ np.abs(wc64).T + np.abs(bc.astype(np.float64))) + 2.0 ** -21
    return logits, bound


@pytest.mark.parametrize("pooler", [True, False])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("H", [128, 768, 1024])
@pytest.mark.parametrize("B", [1, 16, 17, 100])
def test_pair_head_kernel(rt, B, H, nl, pooler):
    cls, wp, bp, wc, bc = head_case(B, H, nl, pooler, seed=B * 7 + H + nl)
    got = _native.diag_pair_head(rt, cls, wc, bc, wp, bp)
    again = _native.diag_pair_head(rt, cls, wc, bc, wp, bp)
    ref, bound = head_ref(cls, wp, bp, wc, bc)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"pair_head B={B} H={H} labels={nl} pooler={pooler}: max err {err.max():.3e}, worst err/bound {np.max(err / bound):.3f}")
    assert got.shape == (B, nl) and np.isfinite(got).all()  # tanh saturated, no NaN from the +-3e38 pre-activations
    assert (err <= bound).all(), (err.max(), np.unravel_index(np.argmax(err / bound), err.shape))
    assert np.array_equal(bits(got), bits(again))


def test_pair_head_saturates_exactly(rt):
    """One pooler output per pair feeds the logit: tanh of +-3e38, +-1e4, +-20.5 is exactly +-1, of 0 exactly 0."""
    H, vals = 128, np.array([3e38, -3e38, 1e4, -1e4, 20.5, -20.5, 0.0], np.float32)
    cls = np.zeros((len(vals), H), np.float32)
    cls[:, 0] = 1.0
    wp = np.zeros((H, H), np.float32)
    wp[3, 0] = 1.0
    cls[:, 0] = vals  # pre-activation of pooler output 3 = vals[b]
    wc = np.zeros((1, H), np.float32)
    wc[0, 3] = 1.0
    got = _native.diag_pair_head(rt, cls, wc, np.zeros(1, np.float32), wp, np.zeros(H, np.float32))
    assert got[:, 0].tolist() == [1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 0.0]


# ------------------------------------------------------------------ typed embedding
def embed_sum_typed(ids, pos, types, wemb, pemb, temb, max_pos, dtype=np.float64):
    """fold_ref.embed_sum with a position and a segment id per row: (word + position) + type_emb[type], everything clamped into its table."""
    zero = fr.embed_sum(np.asarray(ids).reshape(1, -1), wemb, None, np.zeros_like(temb[:1]), max_pos, dtype)  # the clamped word rows
    x = zero + np.asarray(pemb, dtype)[np.minimum(pos, max_pos - 1)]
    return x + np.asarray(temb, dtype)[np.clip(types, 0, len(temb) - 1)]


@pytest.mark.parametrize("H", [128, 768])
def test_typed_embedding_kernels(rt, H):
    B, S, vocab, max_pos, EPS = 3, 13, 50, 11, 1e-12  # 39 rows: no multiple of the 4 rows of a workgroup; positions 11, 12 clamp to 10
    tokens, tp, slots = B * S, 64, max(1, H // 256)
    rng = np.random.default_rng(H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    wemb, pemb, temb = f(vocab, H), f(max_pos, H), np.float32(4.0) * f(2, H)
    g, b = 1 + np.float32(0.1) * f(H), np.float32(0.1) * f(H)
    ids = rng.integers(-2, vocab + 2, (B, S)).astype(np.int32)
    pos = np.tile(np.arange(S, dtype=np.int32), B)
    zeros = np.zeros(tokens, np.int32)
    # all types 0: the bits of the untyped kernels on the same rows, statistics included
    rows0, stats0 = _native.diag_embed_pairs(rt, ids, pos, zeros, wemb, pemb, temb, max_pos, tokens_pad=tp, slots=slots)
    rows_u, stats_u = _native.diag_embed(rt, ids, wemb, pemb, temb, max_pos, tokens_pad=tp, slots=slots)
    assert np.array_equal(bits(rows0), bits(rows_u)) and np.array_equal(bits(stats0), bits(stats_u))
    ln0 = _native.diag_embed_pairs(rt, ids, pos, zeros, wemb, pemb, temb, max_pos, ln=(g, b, EPS))
    assert np.array_equal(bits(ln0), bits(_native.diag_embed(rt, ids, wemb, pemb, temb, max_pos, ln=(g, b, EPS))))
    # mixed types (5 and -1 are clamped into the table), positions in an order of their own
    types = (np.arange(tokens) % S >= 4).astype(np.int32)
    types[[2, 20]], types[[7, 30]] = 5, -1
    pos2 = rng.integers(0, S, tokens).astype(np.int32)
    want = embed_sum_typed(ids, pos2, types, wemb, pemb, temb, max_pos)
    rows, stats = _native.diag_embed_pairs(rt, ids, pos2, types, wemb, pemb, temb, max_pos, tokens_pad=tp, slots=slots)
    scale = max(1.0, float(np.abs(want).max()))
    err = np.abs(rows[:tokens] - want).max()
    print(f"embed_raw_pairs H={H}: max err {err:.3e} of scale {scale:.2f} (bound {scale * 2.0 ** -8:.3e})")
    assert err <= scale * 2.0 ** -8
    assert not np.array_equal(rows[:tokens], rows0[:tokens])  # the types were read
    assert not rows[tokens:].any() and not stats[:, tokens:].any() and not stats[1:].any()  # tail rows: zeros, statistics (0, 0)
    ref_stats = fr.embed_slot_stats(rows[:tokens], 1)[0]
    serr = np.abs(stats[0, :tokens] - ref_stats)
    sbound = 2 * H * U24 * np.stack([np.abs(rows[:tokens]).astype(np.float64).sum(1), ref_stats[:, 1]], axis=1) + 2.0 ** -21
    assert (serr <= sbound).all(), float(np.max(serr / sbound))
    ln = _native.diag_embed_pairs(rt, ids, pos2, types, wemb, pemb, temb, max_pos, ln=(g, b, EPS))
    ref = fr.layernorm(want, g, b, EPS)
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(ln - ref).max()
    print(f"embed_ln_pairs H={H}: max err {err:.3e} of scale {scale:.2f}")
    assert ln.shape == (tokens, H) and err <= scale * 2.0 ** -8


# ------------------------------------------------------------------ the whole path against the golden
@pytest.fixture(scope="module")
def golden_pairs(golden):
    return np.load(golden / "rerank_golden.npz"), json.loads((golden / "rerank_golden.json").read_text())


class Model:
    """One golden model: its pairs, references and (lazily, cached) encoders with the head installed."""

    def __init__(self, rt, data, meta, name):
        m = meta[name]
        self.rt, self.name, self.cfg, self.meta = rt, name, m["cfg"], m
        self.ids = data[f"{name}_ids"].astype(np.int32)
        self.offsets = data[f"{name}_offsets"].astype(np.int64)
        self.first = data[f"{name}_first_lens"].astype(np.int32)
        self.cls, self.logits = data[f"{name}_cls"], data[f"{name}_logits"]
        self.blob = rr.make_weights(self.cfg, m["seed"], m["vo_scale"])
        self.head = rr.make_head(self.cfg, m["seed"], m["num_labels"], m["pooler"])
        self.paths = ["small", "batch"] if rr.FOLDS[name] else ["small"]
        self._enc = {}

    def encoder(self, normalize=False, head=True):
        key = (normalize, head)
        if key not in self._enc:
            enc = _native.Encoder(self.rt, self.cfg, weights=self.blob, normalize=normalize)
            if head:
                enc.set_pair_head(self.head["cls_w"], self.head["cls_b"], self.head["pooler_w"], self.head["pooler_b"])
            self._enc[key] = enc
        return self._enc[key]

    def close(self):
        for enc in self._enc.values():
            enc.close()


@pytest.fixture(scope="module")
def models(rt, golden_pairs):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(rt, *golden_pairs, name)
        return made[name]

    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("name", ["small", "mid", "base"])
def test_pairs_against_transformers(models, name):
    m = models(name)
    T_logit, T_cls = m.meta["T_logit"], m.meta["T_cls"]
    want_scores = rr.scores(m.logits).reshape(rr.N_QUESTIONS, rr.N_PASSAGES)
    for path in m.paths:
        results = []
        for normalize in (False, True):
            enc = m.encoder(normalize)
            enc.set_path(path)
            logits, cls = enc.score_pairs(m.ids, m.offsets, m.first, want_cls=True)
            enc.set_path("auto")
            results.append((logits, cls))
        logits, cls = results[0]
        dl, dc = np.abs(logits - m.logits).max(), np.abs(cls - m.cls).max()
        cos = (cls * m.cls).sum(1) / (np.linalg.norm(cls, axis=1) * np.linalg.norm(m.cls, axis=1))
        print(f"{name} / {path}: logits max|d| {dl:.4f} (T_logit {T_logit:.4f}), cls max|d| {dc:.4f} (T_cls {T_cls:.4f}), cos min {cos.min():.6f}")
        assert np.isfinite(logits).all() and logits.shape == m.logits.shape
        assert dl <= T_logit and dc <= T_cls and cos.min() >= 0.999
        got_scores = rr.scores(logits).reshape(rr.N_QUESTIONS, rr.N_PASSAGES)
        checked = 0
        for q in range(rr.N_QUESTIONS):
            for i, j in rr.ordered_pairs(want_scores[q], 2.0 * T_logit):
                assert got_scores[q, i] > got_scores[q, j], (path, q, i, j)
                checked += 1
        total = rr.N_QUESTIONS * rr.N_PASSAGES * (rr.N_PASSAGES - 1) // 2
        assert checked >= total / 2, (checked, total)  # the ranking check skipped at most half of the passage pairs
        # cfg.normalize does not reach the pair path: the same bits
        assert np.array_equal(bits(results[1][0]), bits(logits)) and np.array_equal(bits(results[1][1]), bits(cls))


@pytest.mark.parametrize("name", ["small", "mid"])
def test_order_independence(models, name):
    m = models(name)
    enc = m.encoder()
    oids, ooff, ofirst = rr.make_pairs(m.cfg, m.meta["seed"] + 100)  # other pairs to mix in
    B = len(m.first)
    rng = np.random.default_rng(3)
    pool = [(m.ids[m.offsets[i]:m.offsets[i + 1]], m.first[i], i) for i in range(B)] + \
           [(oids[ooff[i]:ooff[i + 1]], ofirst[i], -1) for i in range(len(ofirst))]
    order = rng.permutation(len(pool))
    ids = np.concatenate([pool[k][0] for k in order])
    offsets = np.concatenate(([0], np.cumsum([len(pool[k][0]) for k in order]))).astype(np.int64)
    first = np.array([pool[k][1] for k in order], np.int32)
    where = {pool[k][2]: at for at, k in enumerate(order) if pool[k][2] >= 0}
    for path in m.paths:
        enc.set_path(path)
        base = enc.score_pairs(m.ids, m.offsets, m.first)
        mixed = enc.score_pairs(ids, offsets, first)
        enc.set_path("auto")
        back = np.stack([mixed[where[i]] for i in range(B)])
        same = np.array_equal(bits(back), bits(base))
        print(f"{name} / {path}: permuted and mixed into {len(pool)} pairs: max|d| {np.abs(back - base).max():.3e}, bit-identical: {same}")
        assert np.abs(back - base).max() <= m.meta["T_logit"]


def test_no_side_effect_on_embeds(models):
    m = models("mid")
    enc = _native.Encoder(m.rt, m.cfg, weights=m.blob)
    for path in m.paths:
        enc.set_path(path)
        before = enc.embed_packed(m.ids, m.offsets)
        enc.set_pair_head(m.head["cls_w"], m.head["cls_b"], m.head["pooler_w"], m.head["pooler_b"])
        enc.score_pairs(m.ids, m.offsets, m.first)
        after = enc.embed_packed(m.ids, m.offsets)
        enc.set_pair_head(None, None)
        assert np.array_equal(bits(before), bits(after)), path
    enc.close()


def test_errors_leave_results_unchanged(models, rt):
    m = models("small")
    enc, H = m.encoder(), m.cfg["hidden"]
    B = len(m.first)
    want = enc.score_pairs(m.ids, m.offsets, m.first)
    out, cls = np.full((B, 2), 7.0, np.float32), np.full((B, H), 7.0, np.float32)

    def rejected(ids, offsets, first, n, logits=out, needle=None, handle=enc.handle, code=-1):
        rc = lib().sc_encoder_score_pairs(handle, p(ids), p(offsets), p(first), n, p(logits), p(cls))
        assert rc == code and "sc_encoder_score_pairs" in last_error(), (rc, last_error())
        if needle is not None:
            assert needle in last_error(), last_error()
        assert (out == 7.0).all() and (cls == 7.0).all()  # nothing written
        assert np.array_equal(bits(enc.score_pairs(m.ids, m.offsets, m.first)), bits(want))  # nothing changed

    off = lambda *lens: np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    big = np.ones(600, np.int32)
    one = np.array([1], np.int32)
    rejected(None, m.offsets, m.first, B)
    rejected(m.ids, None, m.first, B)
    rejected(m.ids, m.offsets, None, B)
    rejected(m.ids, m.offsets, m.first, B, logits=None)
    rejected(m.ids, m.offsets, m.first, 0, needle="0")
    rejected(m.ids, m.offsets, m.first, 65537, needle="65537")
    rejected(big, off(1), one, 1, needle="1 token")                    # shorter than 2
    rejected(big, off(513), one, 1, needle="513")                      # longer than max_pos = 512
    rejected(big, off(40), np.array([0], np.int32), 1, needle="= 0")   # first_lens outside 1 .. len
    rejected(big, off(40), np.array([41], np.int32), 1, needle="= 41")
    rejected(big, off(10, 40), np.array([10, 41], np.int32), 2, needle="first_lens[1]")
    wrong0 = m.offsets.copy()
    wrong0[0] = 1
    rejected(m.ids, wrong0, m.first, B, needle="offsets[0]")
    rejected(big, off(*([512] * 1025)), np.ones(1025, np.int32), 1025, needle="SC_ENCODER_PACKED_MAX_ROWS", code=-4)  # unsupported, by the planner alone
    # no head installed
    bare = m.encoder(head=False)
    rejected(m.ids, m.offsets, m.first, B, handle=bare.handle, needle="no pair head")
    # a second segment on a model with one type row; a pair that is all segment 0 runs
    mono = _native.Encoder(rt, dict(m.cfg, type_vocab=1), synth_seed=2)
    mono.set_pair_head(m.head["cls_w"], m.head["cls_b"], m.head["pooler_w"], m.head["pooler_b"])
    rejected(big, off(40), np.array([39], np.int32), 1, handle=mono.handle, needle="type_vocab")
    assert np.isfinite(mono.score_pairs(big[:40], off(40), np.array([40], np.int32))).all()
    # no position table (ALiBi): 2 048 tokens bound a pair whatever max_pos says; a pair of exactly 2 048 runs
    ali = _native.Encoder(rt, dict(m.cfg, alibi=True, type_vocab=2), synth_seed=2)
    ali.set_pair_head(m.head["cls_w"], m.head["cls_b"], m.head["pooler_w"], m.head["pooler_b"])
    huge = np.ones(2049, np.int32)
    rejected(huge, off(2049), np.array([10], np.int32), 1, handle=ali.handle, needle="2048")
    rejected(huge, off(40, 2049), np.array([10, 10], np.int32), 2, handle=ali.handle, needle="2049")
    long_logits = ali.score_pairs(huge[:2048], off(2048), np.array([10], np.int32))
    assert long_logits.shape == (1, m.meta["num_labels"]) and np.isfinite(long_logits).all()
    assert np.array_equal(bits(ali.score_pairs(huge[:2048], off(2048), np.array([10], np.int32))), bits(long_logits))
    ali.close()
    # num_labels outside 1 .. 2, NULL bias: the installed head stays
    w3 = np.zeros((3, H), np.float32)
    for nl in (0, 3):
        assert lib().sc_encoder_set_pair_head(enc.handle, None, None, p(w3), p(w3), nl) == -1 and str(nl) in last_error()
    assert lib().sc_encoder_set_pair_head(enc.handle, None, None, p(w3), None, 1) == -1
    assert lib().sc_encoder_set_pair_head(enc.handle, p(w3), None, p(w3), p(w3), 1) == -1
    assert np.array_equal(bits(enc.score_pairs(m.ids, m.offsets, m.first)), bits(want))
    mono.close()


# ------------------------------------------------------------------ Retriever on the device seams
def test_retriever_reranks_on_the_device(models, rt, monkeypatch):
    from pathlib import Path

    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from semcode_amd.embeddings.reranker import MI355XReranker
    from semcode_amd.services import Retriever, build_payloads
    from test_seams_gpu import Chunk
    from semcode_amd.settings import settings
    from semcode_amd.storage import MilvusVectorStore

    m = models("small")
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    words = ["[PAD]", "[CLS]", "[SEP]", "[UNK]"] + [f"w{j}" for j in range(300)] + [f"name{j}" for j in range(16)] + ["def", "where", "is", "defined", "(", ")", ":"]
    vocab = {w: i for i, w in enumerate(words)}
    assert vocab["[CLS]"] == rr.CLS_ID and vocab["[SEP]"] == rr.SEP_ID and len(words) <= m.cfg["vocab"]
    emb = MI355XEmbeddings(cfg=dict(m.cfg), vocab=vocab, runtime=rt, synth_seed=3, allow_synthetic=True)
    reranker = MI355XReranker(weights=m.blob, head=m.head, cfg=dict(m.cfg), vocab=vocab, runtime=rt)
    rng = np.random.default_rng(11)
    root = Path("/w/demo")
    texts = [f"def name{i} ( w{i} ) : " + " ".join(rng.choice(words[4:304], size=int(rng.integers(10, 60)))) for i in range(16)]
    chunks = [Chunk(t, root / "pkg" / f"k{i}.py", "python", 1, 3) for i, t in enumerate(texts)]
    store = MilvusVectorStore(collection_name="test_rerank", dim=m.cfg["hidden"], metric="COSINE", index_type="FLAT", runtime=rt)
    store.connect()
    store.upsert_embeddings(build_payloads("demo", root, chunks, emb))
    r = Retriever(emb, store, reranker=reranker)
    monkeypatch.setattr(settings, "rag_max_context_sources", 16)
    dense = {i: [d["path"] for d in Retriever(emb, store).retrieve(f"where is name{i} defined")] for i in range(16)}
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    late = [i for i in range(16) if dense[i].index(f"pkg/k{i}.py") >= 5]  # the defining chunk lies at dense rank 5 or later
    assert late, "no question whose defining chunk the dense search ranks 5th or later"
    W = {k: v.astype(np.float64) for k, v in rr.bo.unpack(m.cfg, m.blob).items()}
    T = m.meta["T_logit"] * (2 if m.meta["num_labels"] == 2 else 1)  # a score of two labels is the difference of two logits
    questions = [f"where is name{i} defined" for i in late[:2]]
    plain = [r.retrieve(q) for q in questions]
    assert plain == [Retriever(emb, store).retrieve(q) for q in questions] and all("retrieval_score" not in d for docs in plain for d in docs)
    for q, docs in zip(questions, r.retrieve_batch(questions, rerank=True, fetch_k=12)):
        fetched = dense[int(q.split()[2][4:])][:12]
        snippet = {f"pkg/k{i}.py": texts[i] for i in range(16)}
        ids, offsets, first = reranker.build_pairs([q] * 12, [snippet[pth] for pth in fetched])
        cpu = rr.scores(rr.head_logits(m.head, np.stack([rr.forward_cls(m.cfg, W, ids[offsets[i]:offsets[i + 1]], int(first[i])) for i in range(12)])))
        by_path = dict(zip(fetched, cpu))
        assert len(docs) == 3 and all(d["path"] in by_path for d in docs) and r.last_error is None
        assert all(abs(d["score"] - by_path[d["path"]]) <= T for d in docs), [(d["score"], by_path[d["path"]]) for d in docs]
        assert all(docs[j]["score"] >= docs[j + 1]["score"] for j in range(2))
        # the CPU order, wherever its scores are further apart than the bound can bridge: the returned three beat every chunk left out
        got = [d["path"] for d in docs]
        for a in fetched:
            for b in fetched:
                if by_path[a] - by_path[b] > 2 * T:
                    assert not (b in got and a not in got), (a, b)
                    if a in got and b in got:
                        assert got.index(a) < got.index(b)
        assert docs == r.retrieve(q, rerank=True, fetch_k=12)
    store.close()
    reranker.close()
    emb.close()
