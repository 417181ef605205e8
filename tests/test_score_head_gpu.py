"""GPU: the score heads of the ModernBERT and Qwen2 / Qwen3 rerankers (sc_encoder_set_score_head, sc_encoder_score_seqs, sc_diag_score_head)
through the C ABI.

Bounds.
  Linear head (kind 2, score_linear_kernel) against float64 on the same f32 inputs: tests/test_rerank_gpu.py's dot-product bound.  A sum of
  H f32 products accumulated in f32, in any order, is off by at most 2 H 2^-24 sum_k |r_k w_k|; the bias is one more term and 2^-21 covers
  the final rounding of values near zero (rerank_heads_ref.head_bound).
  Prediction head (kind 1, score_head_kernel).  The same analysis can be carried on -- the dense layer's error through GELU's Lipschitz
  constant 1.13 plus the 2.5e-7 of gelu_erf_fast2, then through the LayerNorm at the row's rstd (d mean <= mean |dg|, d var <= 2 sqrt(var)
  |dc| + |dc|^2, d rstd <= rstd^3 d var / 2), then through sum |cls_w| -- but the closed form does not hold up: every stage takes the worst
  case of the one before, the result grows like H^2.5 2^-24 and was evaluated on these very inputs at a median of 0.06 per logit for H = 128,
  5.2 for H = 768 and 62 for H = 2 048, against logits of +-20 .. +-130: from H = 768 on it would pass a kernel that drops whole column tiles.
  On the rows of equal values its first-order expansion of rsqrt is not even valid (d var is not small against var + eps = 1e-5).  So the
  bound is the stated fallback: T = 4 x the largest miss of a plain numpy float32 evaluation in the stated order
  (rerank_heads_ref.head_f32: the header's stage, lane and wave orders, gelu_erf_fast2's polynomial, fused multiply-adds as multiply + add)
  against float64 (exact erf) on the same inputs.  Two yardsticks per shape, each the largest miss over its rows of the 33 (every B under
  test is a prefix), so that neither hangs on the one or two logits of a single row: one over the nine rows of equal values behind the
  dense layer (kernel_case's rows 1 .. 9), whose last-bit noise the LayerNorm multiplies by 1 / sqrt(1e-5) = 316, and one over the 24
  ordinary rows (the row at GELU's tails among them) -- a bound shared with the rows of equal values would hold an ordinary row to a
  hundred times its own f32 error and pass, say, a variance over H - 1 at H = 2 048 (0.01 on a logit).  Measured (the largest of the four
  label / bias variants of a width), rows of equal values: 2.1e-3 at H = 128, 8.8e-3 at 384, 1.4e-2 at 768, 2.2e-2 at 1 024, 4.0e-2 at
  2 048; ordinary rows: 5.5e-5, 1.8e-4, 2.2e-4, 2.6e-4, 4.4e-4 (logits of +-20 .. +-130).  It is never a bound taken from the kernel's
  own output.
  Whole path: T_logit / T_row of tests/golden/rerank_heads_golden.json -- twice what transformers' own bf16 forward misses its fp32 forward
  by (scripts/gen_rerank_heads_fixtures.py) -- and the project's cos >= 0.999 for the rows.
"""
import ctypes as C
import json

import numpy as np
import pytest

import rerank_heads_ref as hr
from semcode_amd import _native

pytestmark = pytest.mark.gpu

lib = _native.lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error():
    buf = C.create_string_buffer(1024)
    lib().sc_last_error(buf, 1024)
    return buf.value.decode()


# ------------------------------------------------------------------ the head kernels alone
@pytest.mark.parametrize("biases", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("H", [128, 384, 768, 1024, 2048])
def test_score_head_kernels(rt, H, kind, nl, biases):
    rows, head = hr.kernel_case(33, H, kind, nl, biases, seed=1000 * H + 10 * nl + biases)
    if kind == 2:
        ref, bound = hr.head_bound(head, rows)
    else:
        ref = hr.head_logits(head, rows)
        miss = np.abs(hr.head_f32(head, rows) - ref).max(1)
        equal = np.zeros(33, bool)
        equal[1:10] = True  # kernel_case's rows of equal values behind the dense layer
        yard = (float(miss[~equal].max()), float(miss[equal].max()))  # one yardstick for the ordinary rows, one for the rows of equal values
        bound = np.repeat(4.0 * np.where(equal, yard[1], yard[0])[:, None], nl, axis=1)
    full = _native.diag_score_head(rt, rows, head)
    for B in (1, 15, 16, 17, 33):
        got = _native.diag_score_head(rt, rows[:B], head)
        err = np.abs(got.astype(np.float64) - ref[:B])
        print(f"score_head kind={kind} B={B} H={H} labels={nl} biases={biases}: max err {err.max():.3e}, worst err/bound {np.max(err / bound[:B]):.3f}"
              + (f" (numpy f32 in the stated order misses by {yard[0]:.3e} on the ordinary rows, {yard[1]:.3e} on the rows of equal values)" if kind == 1 else ""))
        assert got.shape == (B, nl) and np.isfinite(got).all()
        assert (err <= bound[:B]).all(), (B, err.max(), np.unravel_index(np.argmax(err / bound[:B]), err.shape))
        assert np.array_equal(bits(got), bits(_native.diag_score_head(rt, rows[:B], head)))  # run to run
        assert np.array_equal(bits(got), bits(full[:B]))  # a row's logits do not depend on how many rows stand behind it


def test_score_head_rows_are_position_independent(rt):
    """A row gives the same bits as row 0, as the last row of a workgroup, as the first of the next and alone."""
    for kind in (1, 2):
        rows, head = hr.kernel_case(33, 384, kind, 2, True, seed=5)
        base = _native.diag_score_head(rt, rows, head)
        order = np.random.default_rng(1).permutation(33)
        mixed = _native.diag_score_head(rt, rows[order], head)
        assert np.array_equal(bits(mixed), bits(base[order]))
        for i in (0, 15, 16, 32):
            assert np.array_equal(bits(_native.diag_score_head(rt, rows[i:i + 1], head)[0]), bits(base[i]))


def test_diag_refusals(rt):
    rows, head = hr.kernel_case(4, 128, 1, 1, True, seed=9)
    for change, word in ((dict(kind=3), "kind 3"), (dict(num_labels=3), "num_labels 3"), (dict(num_labels=0), "num_labels 0"), (dict(norm_eps=0.0), "norm_eps"),
                         (dict(dense_w=None), "dense_w"), (dict(norm_g=None), "norm_g"), (dict(cls_w=None, num_labels=1), "cls_w"),
                         (dict(kind=2), "must be NULL on kind 2")):
        with pytest.raises(_native.ScError) as err:
            _native.diag_score_head(rt, rows, dict(head, **change))
        assert "sc_diag_score_head" in str(err.value) and word in str(err.value), str(err.value)
    with pytest.raises(_native.ScError) as err:
        _native.diag_score_head(rt, np.zeros((2, 72), np.float32), dict(kind=2, cls_w=np.zeros((1, 72), np.float32)))
    assert "72" in str(err.value)


# ------------------------------------------------------------------ the whole path against the golden
@pytest.fixture(scope="module")
def golden_heads(golden):
    return np.load(golden / "rerank_heads_golden.npz"), json.loads((golden / "rerank_heads_golden.json").read_text())


class Model:
    """One golden case: its pairs, references and (lazily, cached) encoders with the head installed."""

    def __init__(self, rt, data, meta, name):
        m = meta[name]
        self.rt, self.name, self.case, self.cfg, self.meta = rt, name, hr.CASES[name], m["cfg"], m
        assert self.case["cfg"] == m["cfg"]
        self.ids = data[f"{name}_ids"].astype(np.int32)
        self.offsets = data[f"{name}_offsets"].astype(np.int64)
        self.rows, self.logits = data[f"{name}_rows"], data[f"{name}_logits"]
        self.blob = hr.make_weights(self.case, m["seed"])
        self.head = hr.make_head(self.case, m["seed"], self.blob, m["head_scale"])
        self._enc = {}

    def encoder(self, normalize=False, head=True):
        key = (normalize, head)
        if key not in self._enc:
            enc = _native.Encoder(self.rt, self.cfg, weights=self.blob, normalize=normalize)
            if head:
                enc.set_score_head(self.head)
            self._enc[key] = enc
        return self._enc[key]

    def pair(self, i):
        return self.ids[self.offsets[i]:self.offsets[i + 1]]

    def close(self):
        for enc in self._enc.values():
            enc.close()


@pytest.fixture(scope="module")
def models(rt, golden_heads):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(rt, *golden_heads, name)
        return made[name]

    yield get
    for m in made.values():
        m.close()


def packed(texts):
    return np.concatenate(texts).astype(np.int32), np.concatenate(([0], np.cumsum([len(t) for t in texts]))).astype(np.int64)


@pytest.mark.parametrize("name", list(hr.CASES))
def test_seqs_against_transformers(models, name):
    m = models(name)
    T_logit, T_row = m.meta["T_logit"], m.meta["T_row"]
    want_scores = hr.scores(m.logits)[hr.N_SHAPE_PAIRS:].reshape(hr.N_QUESTIONS, hr.N_PASSAGES)
    enc = m.encoder()
    for path in ("small", "batch"):
        enc.set_path(path)
        logits, rows = enc.score_seqs(m.ids, m.offsets, want_rows=True)
        enc.set_path("auto")
        dl, dr = np.abs(logits - m.logits).max(), np.abs(rows - m.rows).max()
        cos = (rows * m.rows).sum(1) / (np.linalg.norm(rows, axis=1) * np.linalg.norm(m.rows, axis=1))
        print(f"{name} / {path}: logits max|d| {dl:.4f} (T_logit {T_logit:.4f}), rows max|d| {dr:.4f} (T_row {T_row:.4f}), cos min {cos.min():.6f}")
        assert np.isfinite(logits).all() and logits.shape == m.logits.shape
        assert dl <= T_logit and dr <= T_row and cos.min() >= 0.999
        got_scores = hr.scores(logits)[hr.N_SHAPE_PAIRS:].reshape(hr.N_QUESTIONS, hr.N_PASSAGES)
        checked = 0
        for q in range(hr.N_QUESTIONS):
            for i, j in hr.ordered_pairs(want_scores[q], 2.0 * T_logit):
                assert got_scores[q, i] > got_scores[q, j], (path, q, i, j)
                checked += 1
        total = hr.N_QUESTIONS * hr.N_PASSAGES * (hr.N_PASSAGES - 1) // 2
        assert checked >= total / 2, (checked, total)  # the ranking check skipped at most half of the passage pairs


@pytest.mark.parametrize("name", ["mb_mean2", "q3_score"])
def test_a_pair_does_not_depend_on_its_batch(models, name):
    """Alone, first in a batch, last in a batch and behind the 600-token pair: the same logit bits, on every set_path setting.  The head adds
    nothing batch-dependent (test_score_head_kernels, test_score_head_rows_are_position_independent), and a scored call's forward never takes
    the split-K GEMMs, whose use and factor follow the call's row count: every GEMM is the 256-tile kernel whatever the batch."""
    m = models(name)
    enc = m.encoder()
    long_ = int(np.argmax(np.diff(m.offsets)))
    assert len(m.pair(long_)) == 600
    paths = []
    for path in ("batch", "auto", "small"):
        enc.set_path(path)
        base = enc.score_seqs(m.ids, m.offsets)
        assert np.array_equal(bits(enc.score_seqs(m.ids, m.offsets)), bits(base))  # run to run
        for i in (0, 2, 4, 9):  # the shortest pair, 32 tokens, 65 tokens, a ranking pair
            alone = enc.score_seqs(*packed([m.pair(i)]))
            first = enc.score_seqs(*packed([m.pair(i), m.pair(3), m.pair(5)]))
            last = enc.score_seqs(*packed([m.pair(5), m.pair(3), m.pair(i)]))
            behind = enc.score_seqs(*packed([m.pair(long_), m.pair(i)]))
            for what, got in (("alone", alone[0]), ("first", first[0]), ("last", last[2]), ("behind 600", behind[1])):
                assert np.array_equal(bits(got), bits(base[i])), (path, i, what, got, base[i])
        paths.append(base)
    enc.set_path("auto")
    assert np.array_equal(bits(paths[1]), bits(paths[0])) and np.array_equal(bits(paths[2]), bits(paths[0]))  # set_path leaves the logits alone


@pytest.mark.parametrize("name", ["mb_cls", "mb_mean2", "q2_tied"])
def test_heads_and_embeds_leave_each_other_alone(models, name):
    m = models(name)
    plain = _native.Encoder(m.rt, m.cfg, weights=m.blob)
    enc, norm = m.encoder(), m.encoder(normalize=True)
    poolings = ("mean", "cls") if hr.kind_of(m.case) == 1 else ("mean", "last")
    try:
        want = enc.score_seqs(m.ids, m.offsets, want_rows=True)
        for pooling in poolings:
            plain.pooling = enc.pooling = norm.pooling = pooling
            before = plain.embed_packed(m.ids, m.offsets)
            plain.set_score_head(m.head)
            plain.score_seqs(m.ids, m.offsets)
            assert np.array_equal(bits(plain.embed_packed(m.ids, m.offsets)), bits(before)), pooling  # an installed head leaves embeds alone
            assert np.array_equal(bits(enc.embed_packed(m.ids, m.offsets)), bits(before)), pooling
            plain.set_score_head(None)
            assert np.array_equal(bits(plain.embed_packed(m.ids, m.offsets)), bits(before)), pooling
            for e in (enc, norm):  # set_pooling / normalize leave logits and rows alone
                got = e.score_seqs(m.ids, m.offsets, want_rows=True)
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), pooling
        emb_n = norm.embed_packed(m.ids, m.offsets)
        assert np.allclose(np.linalg.norm(emb_n, axis=1), 1.0, atol=1e-3)  # ... while the embeds of that encoder are normalised
    finally:
        enc.pooling = norm.pooling = "mean"
        plain.close()


def test_refusals_leave_results_unchanged(models, rt):
    m = models("mb_cls")
    enc, H = m.encoder(), m.cfg["hidden"]
    B = len(m.offsets) - 1
    want = enc.score_seqs(m.ids, m.offsets)
    out, rows = np.full((B, 2), 7.0, np.float32), np.full((B, H), 7.0, np.float32)

    def unchanged():
        assert np.array_equal(bits(enc.score_seqs(m.ids, m.offsets)), bits(want))

    def rejected(ids, offsets, n, logits=out, needle=None, handle=enc.handle, code=-1):
        rc = lib().sc_encoder_score_seqs(handle, p(ids), p(offsets), n, p(logits), p(rows))
        assert rc == code and "sc_encoder_score_seqs" in last_error(), (rc, last_error())
        if needle is not None:
            assert needle in last_error(), last_error()
        assert (out == 7.0).all() and (rows == 7.0).all()  # nothing written
        unchanged()

    off = lambda *lens: np.concatenate(([0], np.cumsum(lens))).astype(np.int64)  # noqa: E731
    big = np.ones(3000, np.int32)
    rejected(None, m.offsets, B)
    rejected(m.ids, None, B)
    rejected(m.ids, m.offsets, B, logits=None)
    rejected(m.ids, m.offsets, 0, needle="0")
    rejected(m.ids, m.offsets, 65537, needle="65537")
    rejected(big, off(5, 0), 2, needle="text 1")                       # shorter than 1 token
    rejected(big, off(2049), 1, needle="2049")                         # longer than 2 048 tokens (= max_pos here)
    wrong0 = m.offsets.copy()
    wrong0[0] = 1
    rejected(m.ids, wrong0, B, needle="offsets[0]")
    rejected(np.ones(1025 * 512, np.int32), off(*([512] * 1025)), 1025, needle="SC_ENCODER_PACKED_MAX_ROWS", code=-4)
    short = _native.Encoder(rt, dict(m.cfg, max_pos=64), synth_seed=2)  # max_pos below 2 048 bounds a text
    short.set_score_head(m.head)
    rejected(big, off(65), 1, handle=short.handle, needle="65")
    assert np.isfinite(short.score_seqs(big[:64], off(64))).all()
    short.close()
    bare = m.encoder(head=False)
    rejected(m.ids, m.offsets, B, handle=bare.handle, needle="no score head")
    # an arch 0 encoder: both calls are refused by name and point at the pair head
    bert = _native.Encoder(rt, dict(_native.BERT_BASE, vocab=64, layers=1, hidden=128, heads=2, ffn=256), synth_seed=1)
    rejected(m.ids, m.offsets, B, handle=bert.handle, needle="sc_encoder_score_pairs", code=-4)
    st, keep = _native.score_head_struct(m.head, H)
    assert lib().sc_encoder_set_score_head(bert.handle, C.byref(st)) == -4 and "sc_encoder_set_pair_head" in last_error()
    bert.close()
    # set_score_head: every refusal leaves the installed head in place
    causal = _native.Encoder(rt, dict(hr.CASES["q2_tied"]["cfg"], layers=1), synth_seed=3)
    lin = dict(kind=2, pooling="last", cls_w=np.ones((1, H), np.float32), cls_b=None)

    def refused(handle, head, word, code=-1):
        st, keep = _native.score_head_struct(head, H)
        assert lib().sc_encoder_set_score_head(handle, C.byref(st)) == code, last_error()
        assert "sc_encoder_set_score_head" in last_error() and word in last_error(), last_error()
        unchanged()

    refused(enc.handle, lin, "kind 2")                                       # a linear head on an arch 1 encoder
    refused(causal.handle, m.head, "kind 1")                                 # a prediction head on an arch 2 encoder
    refused(enc.handle, dict(m.head, pooling=2), "pooling 2")
    refused(causal.handle, dict(lin, pooling=0), "pooling 0")
    refused(causal.handle, dict(lin, dense_w=np.zeros((H, H), np.float32)), "must be NULL on kind 2")
    for nl in (0, 3):
        refused(enc.handle, dict(m.head, num_labels=nl), f"num_labels {nl}")
    refused(enc.handle, dict(m.head, dense_w=None), "dense_w")
    refused(enc.handle, dict(m.head, norm_g=None), "norm_g")
    refused(enc.handle, dict(m.head, cls_w=None, num_labels=1), "cls_w")
    refused(enc.handle, dict(m.head, norm_eps=0.0), "norm_eps")
    refused(enc.handle, dict(m.head, kind=0), "kind 0")
    causal.set_score_head(lin)  # ... and a good head on the causal encoder runs, is replaced and removed
    one = causal.score_seqs(big[:40], off(40))
    causal.set_score_head(dict(lin, cls_w=2 * np.ones((1, H), np.float32)))
    assert np.array_equal(bits(causal.score_seqs(big[:40], off(40))), bits(2 * one))
    causal.set_score_head(None)
    with pytest.raises(_native.ScError, match="no score head"):
        causal.score_seqs(big[:40], off(40))
    causal.close()
    unchanged()


def test_score_pairs_still_refuses_these_encoders(models):
    """The pair entry point keeps its refusals, words included, with a score head installed."""
    for name, words in (("mb_cls", "arch 1 (pre-LN) models have no pair head: their classifier is not pooler + linear"),
                        ("q2_tied", "arch 2 (causal decoder) models do not score pairs: the family has no [CLS] row and no pair head")):
        enc = models(name).encoder()
        with pytest.raises(_native.ScError) as err:
            enc.score_pairs(np.arange(1, 9, dtype=np.int32), np.array([0, 8], np.int64), np.array([4], np.int32))
        assert "sc_encoder_score_pairs: " + words in str(err.value), str(err.value)


# ------------------------------------------------------------------ a decoder reranker through MI355XReranker
def test_causal_reranker_scores_prompts(models, rt):
    """A causal-LM reranker given as blob + head: prompts built from a template, cut to max_pair_tokens with prefix and suffix whole, scored
    as logit(true row) - logit(false row), against the restatement within 2 T_logit (a difference of two logits)."""
    from semcode_amd.embeddings.reranker import MI355XReranker

    m = models("q2_tied")

    class Tok:
        pad_id = 0

        def encode_plain(self, text):
            return [hr.FIRST_WORD + sum(w.encode()) % 300 for w in text.split()]

    template = dict(prefix="sys judge this", body="I: {instruction} Q: {query} D: {document}", suffix="as sist ant", instruction="find the definition")
    r = MI355XReranker(weights=m.blob, head=m.head, cfg=dict(m.cfg), tokenizer=Tok(), runtime=rt, template=template, max_pair_tokens=40)
    try:
        assert r.family == "causal" and r.num_labels == 2 and r.max_len == 40
        rng = np.random.default_rng(5)
        texts = [" ".join(f"w{j}" for j in rng.integers(0, 500, size=n)) for n in (3, 12, 60, 0, 25, 31)]  # one longer than the room, one empty
        qs = ["where is foo defined"] * len(texts)
        ids, offsets = r.build_pairs(qs, texts)
        lens = np.diff(offsets)
        tok = Tok()
        assert lens.max() == 40 and lens[3] == len(tok.encode_plain("sys judge this I: find the definition Q: where is foo defined D: as sist ant"))
        for i in range(len(texts)):
            row = ids[offsets[i]:offsets[i + 1]].tolist()
            assert row[:3] == tok.encode_plain("sys judge this") and row[-3:] == tok.encode_plain("as sist ant")
        want = hr.scores(hr.forward(m.case, m.blob, m.head, ids, offsets)[1])
        got = r.score_pairs(qs, texts)
        print(f"causal reranker: scores max|d| {np.abs(got - want).max():.4f} (2 T_logit {2 * m.meta['T_logit']:.4f}), spread {np.ptp(want):.2f}")
        assert got.shape == (len(texts),) and np.abs(got - want).max() <= 2 * m.meta["T_logit"]
        order, scores = r.rerank(qs[0], texts, top_k=3)
        assert len(order) == 3 and np.array_equal(scores, got[order]) and (np.diff(scores) <= 0).all()
        assert np.array_equal(r.score_pairs([], []), np.empty(0, np.float32))
    finally:
        r.close()


# ------------------------------------------------------------------ Retriever on the device seams
def test_retriever_reranks_with_a_directory_model(models, rt, monkeypatch, tmp_path):
    from pathlib import Path

    from safetensors.numpy import save_file
    from tokenizers import Tokenizer, models as tk_models, pre_tokenizers, processors

    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from semcode_amd.embeddings.reranker import MI355XReranker
    from semcode_amd.services import Retriever, build_payloads
    from semcode_amd.settings import settings
    from semcode_amd.storage import MilvusVectorStore
    from test_seams_gpu import Chunk

    m = models("mb_cls")
    words = ["[PAD]", "[CLS]", "[SEP]", "[UNK]"] + [f"w{j}" for j in range(300)] + [f"name{j}" for j in range(16)] + ["def", "where", "is", "defined", "(", ")", ":"]
    vocab = {w: i for i, w in enumerate(words)}
    assert vocab["[CLS]"] == hr.CLS_ID and vocab["[SEP]"] == hr.SEP_ID and len(words) <= m.cfg["vocab"]
    # the directory: config.json, model.safetensors, tokenizer.json (word level, [CLS] text [SEP])
    d = tmp_path / "reranker"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(hr.hf_config(m.case)))
    save_file(hr.to_hf_state_dict(m.case, m.blob, m.head, m.meta["seed"], m.meta["head_scale"]), str(d / "model.safetensors"))
    tok = Tokenizer(tk_models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    tok.save(str(d / "tokenizer.json"))

    emb_cfg = dict(_native.BERT_BASE, vocab=400, hidden=128, layers=2, heads=2, ffn=256, max_pos=512)
    emb = MI355XEmbeddings(cfg=emb_cfg, vocab=vocab, runtime=rt, synth_seed=3, allow_synthetic=True)
    reranker = MI355XReranker(d, runtime=rt)
    assert reranker.family == "modernbert" and reranker.num_labels == 1 and reranker.max_len == 512
    rng = np.random.default_rng(11)
    root = Path("/w/demo")
    texts = [f"def name{i} ( w{i} ) : " + " ".join(rng.choice(words[4:304], size=int(rng.integers(10, 60)))) for i in range(16)]
    chunks = [Chunk(t, root / "pkg" / f"k{i}.py", "python", 1, 3) for i, t in enumerate(texts)]
    store = MilvusVectorStore(collection_name="test_score_head", dim=128, metric="COSINE", index_type="FLAT", runtime=rt)
    store.connect()
    store.upsert_embeddings(build_payloads("demo", root, chunks, emb))
    monkeypatch.setattr(settings, "rag_max_context_sources", 12)
    dense = {i: [doc["path"] for doc in Retriever(emb, store).retrieve(f"where is name{i} defined")] for i in range(2)}
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    r = Retriever(emb, store, reranker=reranker)
    T = m.meta["T_logit"]
    snippet = {f"pkg/k{i}.py": texts[i] for i in range(16)}
    questions = [f"where is name{i} defined" for i in range(2)]
    for q, docs in zip(questions, r.retrieve_batch(questions, rerank=True, fetch_k=12)):
        fetched = dense[int(q.split()[2][4:])]
        ids, offsets = reranker.build_pairs([q] * 12, [snippet[pth] for pth in fetched])
        assert ids[0] == hr.CLS_ID and (ids == hr.SEP_ID).sum() == 24
        cpu = hr.scores(hr.forward(m.case, m.blob, m.head, ids, offsets)[1])
        by_path = dict(zip(fetched, cpu))
        assert len(docs) == 3 and all(doc["path"] in by_path for doc in docs) and r.last_error is None
        assert all(abs(doc["score"] - by_path[doc["path"]]) <= T for doc in docs), [(doc["score"], by_path[doc["path"]]) for doc in docs]
        assert all(docs[j]["score"] >= docs[j + 1]["score"] for j in range(2))
        got = [doc["path"] for doc in docs]
        for a in fetched:  # the CPU order, wherever its scores are further apart than the bound can bridge
            for b in fetched:
                if by_path[a] - by_path[b] > 2 * T:
                    assert not (b in got and a not in got), (a, b)
                    if a in got and b in got:
                        assert got.index(a) < got.index(b)
    store.close()
    reranker.close()
    emb.close()
