"""The shared recipe of the score-head tests: seeded rerankers on the ModernBERT and the Qwen2 / Qwen3 backbones, their pairs, and a float64
restatement of what sc_encoder_score_seqs computes.  TEST INFRASTRUCTURE ONLY (tests/test_score_head_*.py,
scripts/gen_rerank_heads_fixtures.py).

The backbones are those of tests/modernbert_ref.py, tests/qwen2_ref.py and tests/qwen3_ref.py, run up to the last hidden state -- last_hidden
calls their forward for one text and keeps what its final norm was given and what it returned, so nothing of the three forwards is restated
here -- and the two heads are added on top:

  prediction head (ModernBertForSequenceClassification): r = final_norm row 0 ("cls") or the mean of the final_norm rows over the real
      tokens ("mean");  g = gelu_erf(dense_w r + dense_b);  p = LayerNorm(g; norm_g, norm_b, norm_eps);  logits = cls_w p + cls_b.
  linear head on the last token: r = RMS_final of row len - 1;  logits = cls_w r.  cls_w is the `score` layer of a
      Qwen3ForSequenceClassification, or the rows (false token, true token) of the vocabulary projection of a Qwen2ForCausalLM /
      Qwen3ForCausalLM -- lm_head, or the embedding table when the two are tied.

tests/golden/rerank_heads_golden.{npz,json} stores ids, offsets and what transformers (fp32, CPU) computes for them -- not the weights:
make_weights / make_head rebuild those from the case and its seed.

DEVIATIONS: one deliberate mix-up each, so that the generator and the tests can show that the fixtures tell it apart.  Two of them read rows
the model does not have: "mean_ceil32" and "last_of_block" run the backbone on the text padded with token 0 to the next multiple of 32, the
padding taken for real tokens -- a stand-in for a kernel that reads the alignment rows of the packed layout.
"""
from __future__ import annotations

import zlib
from contextlib import contextmanager

import numpy as np

import modernbert_ref as mb
import qwen2_ref as q2
import qwen3_ref as q3

MB_COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True, rope_theta=160000.0, rope_theta_local=10000.0,
                 local_window=32, global_every=3)
QW_COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0)
MB_SCALES = (8.0, 3.0, 3.0, 0.6)                          # modernbert_ref.make_weights: the golden cases' (qk, vo, mlp, global_qk)
Q2_SCALES = (2.0, 2.0, 3.0, 3.0, 5.0, 0.3, 0)             # qwen2_ref.make_weights: qwen2_golden's
Q3_SCALES = (1.0, 0.4, 2.0, 3.0, 5.0, 0.5, 5, 1.1)        # qwen3_ref.make_weights: the entry qwen3_golden uses for its long text (bias_first 5)
# name: backbone cfg, architecture (the transformers class that pins it), head: kind of head, pooling, num_labels, optional biases
CASES = {
    "mb_cls": dict(cfg=dict(MB_COMMON, hidden=128, heads=2, ffn=256, layers=4), arch="ModernBertForSequenceClassification", pooling="cls", num_labels=1,
                   dense_bias=False, norm_bias=False),
    "mb_mean2": dict(cfg=dict(MB_COMMON, hidden=128, heads=2, ffn=256, layers=4), arch="ModernBertForSequenceClassification", pooling="mean", num_labels=2,
                     dense_bias=True, norm_bias=True),
    "mb_256": dict(cfg=dict(MB_COMMON, hidden=256, heads=4, ffn=512, layers=4), arch="ModernBertForSequenceClassification", pooling="mean", num_labels=1,
                   dense_bias=False, norm_bias=False),
    "mb_base": dict(cfg=dict(MB_COMMON, hidden=768, heads=12, ffn=1152, layers=2), arch="ModernBertForSequenceClassification", pooling="cls", num_labels=1,
                    dense_bias=False, norm_bias=False),
    "q2_tied": dict(cfg=dict(QW_COMMON, hidden=128, heads=2, kv_heads=1, ffn=256, layers=3), arch="Qwen2ForCausalLM", pooling="last", num_labels=2, tied=True),
    "q3_score": dict(cfg=dict(QW_COMMON, hidden=256, heads=4, kv_heads=2, ffn=512, layers=2, head_dim=128, qk_norm=True), arch="Qwen3ForSequenceClassification",
                     pooling="last", num_labels=1),
    "q3_06b": dict(cfg=dict(QW_COMMON, hidden=1024, heads=16, kv_heads=8, ffn=3072, layers=2, head_dim=128, qk_norm=True), arch="Qwen3ForCausalLM", pooling="last",
                   num_labels=2, tied=False),
}
FALSE_ID, TRUE_ID = 7, 11          # the two vocabulary rows of the causal-LM cases ("no", "yes")
CLS_ID, SEP_ID, FIRST_WORD = 1, 2, 12
SHAPE_LENS = (31, 32, 33, 65, 129, 300, 600)  # behind the shortest pair a family has: 1 token (causal) or 3 ([CLS] [SEP] [SEP])
N_QUESTIONS, N_PASSAGES = 3, 4

MB_DEVIATIONS = ("no_act", "no_norm", "norm_before_act", "pool_swapped", "mean_ceil32", "no_final_norm", "l2_row", "no_head_bias")
CAUSAL_DEVIATIONS = ("last_of_block", "token_before_last", "mean", "no_final_norm", "l2_row", "labels_swapped")
DEVIATIONS = MB_DEVIATIONS + tuple(d for d in CAUSAL_DEVIATIONS if d not in MB_DEVIATIONS)


def family(cfg: dict) -> str:
    return "modernbert" if cfg.get("modernbert") else ("qwen3" if cfg.get("qk_norm") or cfg.get("head_dim") == 128 else "qwen2")


def kind_of(case: dict) -> int:
    return 1 if family(case["cfg"]) == "modernbert" else 2


def deviations_of(case: dict) -> tuple:
    return MB_DEVIATIONS if kind_of(case) == 1 else CAUSAL_DEVIATIONS


def applicable(case: dict, dev: str, n: int) -> bool:
    """Whether a mix-up differs from the model at all for a text of n tokens of this case."""
    if dev == "no_head_bias":
        return bool(case.get("dense_bias") or case.get("norm_bias"))
    if dev == "labels_swapped":
        return case["num_labels"] == 2
    if dev in ("mean_ceil32", "last_of_block"):
        return n % 32 != 0 and (dev == "last_of_block" or case["pooling"] == "mean")
    if dev in ("token_before_last", "mean", "pool_swapped"):
        return n > 1
    return True


def make_weights(case: dict, seed: int) -> np.ndarray:
    cfg = case["cfg"]
    fam = family(cfg)
    if fam == "modernbert":
        return mb.make_weights(cfg, seed, *MB_SCALES)
    return q2.make_weights(cfg, seed, *Q2_SCALES) if fam == "qwen2" else q3.make_weights(cfg, seed, *Q3_SCALES)


def make_lm_head(cfg: dict, seed: int) -> np.ndarray:
    """The vocabulary projection [vocab, H] of an untied causal LM: N(0, 1 / H) x head_scale is applied by make_head to the two rows it takes."""
    rng = np.random.default_rng(66000 + seed)
    return (rng.standard_normal((cfg["vocab"], cfg["hidden"])) / np.sqrt(cfg["hidden"])).astype(np.float32)


def make_head(case: dict, seed: int, blob: "np.ndarray | None" = None, head_scale: float = 1.0) -> dict:
    """The head of a case as the dict _native.Encoder.set_score_head takes.  Prediction head: dense_w = head_scale x N(0, 1 / H) (pre-activations of
    order head_scale: around 1 the GELU bends -- far above it is a ReLU, far below a line, and either commutes with a rescaled row under the
    LayerNorm that follows), dense_b 0.3 x N(0,1), norm_g 1 + 0.3 N(0,1), norm_b 0.1 N(0,1), cls_w 8 x N(0, 1 / H), cls_b 0.1 N(0,1);
    dense_b / norm_b None without the case's dense_bias / norm_bias.  `score` layer: head_scale x N(0, 1 / H), no bias.  Vocabulary rows:
    (FALSE_ID, TRUE_ID) of the embedding table (tied: blob is needed) or of make_lm_head x head_scale."""
    cfg, H, nl = case["cfg"], case["cfg"]["hidden"], case["num_labels"]
    rng = np.random.default_rng(77000 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    if kind_of(case) == 1:
        head = dict(kind=1, pooling=case["pooling"], norm_eps=float(cfg["ln_eps"]), dense_w=np.float32(head_scale) * f(H, H) / np.float32(np.sqrt(H)),
                    dense_b=np.float32(0.3) * f(H), norm_g=1 + np.float32(0.3) * f(H), norm_b=np.float32(0.1) * f(H),
                    cls_w=np.float32(8.0) * f(nl, H) / np.float32(np.sqrt(H)), cls_b=np.float32(0.1) * f(nl))
        if not case.get("dense_bias"):
            head["dense_b"] = None
        if not case.get("norm_bias"):
            head["norm_b"] = None
        return head
    if "tied" not in case:
        cls_w = np.float32(head_scale) * f(nl, H) / np.float32(np.sqrt(H))
    elif case["tied"]:
        cls_w = fam_unpack(cfg, blob)["word_emb"][[FALSE_ID, TRUE_ID]].copy()
    else:
        cls_w = np.float32(head_scale) * make_lm_head(cfg, seed)[[FALSE_ID, TRUE_ID]]
    return dict(kind=2, pooling="last", cls_w=np.ascontiguousarray(cls_w, np.float32), cls_b=None)


def fam_unpack(cfg: dict, blob: np.ndarray) -> dict:
    return {"modernbert": mb, "qwen2": q2, "qwen3": q3}[family(cfg)].unpack(cfg, blob)


def make_pairs(case: dict, seed: int):
    """(ids_flat int32, offsets int64): the shortest pair of the family, the pairs of SHAPE_LENS tokens, then N_QUESTIONS x N_PASSAGES pairs of
    20 .. 32 tokens, question-major, whose passages share the question's 6 .. 10 words.  ModernBERT pairs are [CLS] q [SEP] p [SEP].
    The ranking pairs stay at or below 32 tokens on purpose: the generator's rule (ii) -- every mix-up outside T_logit on EVERY pair longer
    than 32 tokens -- then binds on the five long shape pairs.  A head with one label gives one number per pair, and a wrong number lands
    within T_logit of the right one by chance on about one pair in 25 (2 T_logit / the logits' spread, measured): with twelve more long
    pairs and six mix-ups hardly a seed passes, which says nothing about the fixtures' power to tell a mix-up apart."""
    cfg, k1 = case["cfg"], kind_of(case) == 1
    rng = np.random.default_rng(88000 + seed)
    words = lambda n: rng.integers(FIRST_WORD, cfg["vocab"], max(0, n)).tolist()  # noqa: E731

    def pair(q, n):  # q: the question's words; n tokens in all
        if not k1:
            return (q + words(n - len(q)))[:n]
        body = [CLS_ID] + q + [SEP_ID]
        return body + words(n - len(body) - 1) + [SEP_ID]

    rows = [[CLS_ID, SEP_ID, SEP_ID] if k1 else words(1)]
    rows += [pair(words(6), n) for n in SHAPE_LENS]
    for _ in range(N_QUESTIONS):
        q = words(int(rng.integers(6, 11)))
        rows += [pair(q, int(rng.integers(20, 33))) for _ in range(N_PASSAGES)]
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return np.concatenate([np.asarray(r, np.int32) for r in rows]), offsets


N_SHAPE_PAIRS = 1 + len(SHAPE_LENS)  # the ranking pairs lie behind them


@contextmanager
def _recorded(mod, name):
    """Every call of mod.<name>(x, ...) inside the block, as (x, result)."""
    calls, orig = [], getattr(mod, name)

    def wrap(x, *a, **k):
        y = orig(x, *a, **k)
        calls.append((x, y))
        return y

    setattr(mod, name, wrap)
    try:
        yield calls
    finally:
        setattr(mod, name, orig)


_HIDDEN: dict = {}  # (a checksum of the blob, its size, the text's ids) -> last_hidden's result: the mix-ups of one text share the backbone run


def last_hidden(cfg: dict, blob: np.ndarray, ids: np.ndarray):
    """One text -> (h [n, H] before the final norm, final_norm(h) [n, H]) in float64: the backbone's own forward, its last norm call recorded."""
    key = (zlib.crc32(np.ascontiguousarray(blob[::61]).tobytes()), blob.size, np.asarray(ids, np.int64).tobytes())
    if key not in _HIDDEN:
        if len(_HIDDEN) >= 64 or any(k[:2] != key[:2] for k in _HIDDEN):
            _HIDDEN.clear()
        _HIDDEN[key] = _last_hidden(cfg, blob, ids)
    return _HIDDEN[key]


def _last_hidden(cfg: dict, blob: np.ndarray, ids: np.ndarray):
    ids = np.asarray(ids).reshape(1, -1)
    lens = np.array([ids.shape[1]])
    fam = family(cfg)
    mod, name = {"modernbert": (mb, "_layernorm"), "qwen2": (q2, "_rms"), "qwen3": (q3, "_rms")}[fam]
    with _recorded(mod, name) as calls:
        mod.forward(cfg, blob, ids, lens, "mean")
    raw, normed = calls[-1]
    assert raw.shape == (ids.shape[1], cfg["hidden"]) and normed.shape == raw.shape
    return raw, normed


def _gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps) * g + (0.0 if b is None else b)


def head_logits(head: dict, r: np.ndarray, deviate: "str | None" = None) -> np.ndarray:
    """r [B, H] -> logits [B, num_labels] in float64 (the head arithmetic of include/semcode_hip.h, any order)."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    r = np.asarray(r, np.float64)
    wc, bc = f64(head["cls_w"]).reshape(-1, r.shape[1]), f64(head.get("cls_b"))
    if deviate == "labels_swapped":
        wc = wc[::-1]
    if head["kind"] == 2:
        return r @ wc.T + (0.0 if bc is None else bc)
    db, nb = f64(head.get("dense_b")), f64(head.get("norm_b"))
    if deviate == "no_head_bias":
        db = nb = None
    a = r @ f64(head["dense_w"]).T + (0.0 if db is None else db)
    if deviate == "norm_before_act":
        p = _gelu(_ln(a, f64(head["norm_g"]), nb, head["norm_eps"]))
    else:
        g = a if deviate == "no_act" else _gelu(a)
        p = g if deviate == "no_norm" else _ln(g, f64(head["norm_g"]), nb, head["norm_eps"])
    return p @ wc.T + (0.0 if bc is None else bc)


def pooled_row(case: dict, blob: np.ndarray, ids: np.ndarray, deviate: "str | None" = None) -> np.ndarray:
    """The row [H] (float64) the head of the case reads for one text."""
    cfg, n = case["cfg"], len(ids)
    if deviate in ("mean_ceil32", "last_of_block"):
        ids = np.concatenate([ids, np.zeros((-n) % 32, np.int64)])
    raw, normed = last_hidden(cfg, blob, ids)
    h = raw if deviate == "no_final_norm" else normed
    pooling = case["pooling"]
    if deviate == "pool_swapped":
        pooling = "mean" if pooling == "cls" else "cls"
    if deviate == "mean":
        pooling = "mean"
    if pooling == "cls":
        r = h[0]
    elif pooling == "mean":
        r = h.mean(0) if deviate == "mean_ceil32" else h[:n].mean(0)
    else:
        r = h[-1] if deviate == "last_of_block" else h[n - 2] if deviate == "token_before_last" else h[n - 1]
    return r / max(np.linalg.norm(r), 1e-12) if deviate == "l2_row" else r


def forward(case: dict, blob: np.ndarray, head: dict, ids_flat, offsets, deviate: "str | None" = None, only=None):
    """All texts (or those of `only`) -> (rows [B, H], logits [B, num_labels]) float64."""
    assert deviate is None or deviate in deviations_of(case), deviate
    idx = range(len(offsets) - 1) if only is None else only
    rows = np.stack([pooled_row(case, blob, np.asarray(ids_flat[offsets[i]:offsets[i + 1]], np.int64), deviate) for i in idx])
    return rows, head_logits(head, rows, deviate)


def scores(logits: np.ndarray) -> np.ndarray:
    """1 label: the logit; 2 labels: logit[1] - logit[0] (for a causal LM: true row - false row)."""
    logits = np.asarray(logits)
    return logits[:, 0] if logits.shape[1] == 1 else logits[:, 1] - logits[:, 0]


def ordered_pairs(score_row: np.ndarray, gap: float) -> "list[tuple[int, int]]":
    n = len(score_row)
    return [(i, j) for i in range(n) for j in range(n) if score_row[i] - score_row[j] > gap]


# ------------------------------------------------------------------ transformers' view of a case (names and config only; the generator imports transformers)
def hf_config(case: dict) -> dict:
    cfg = case["cfg"]
    if kind_of(case) == 1:
        out = dict(mb.hf_config(cfg), classifier_pooling=case["pooling"], classifier_bias=bool(case.get("dense_bias")), classifier_activation="gelu",
                   classifier_dropout=0.0, num_labels=case["num_labels"], norm_bias=bool(case.get("norm_bias")), architectures=[case["arch"]])
        return out
    out = dict((q2 if family(cfg) == "qwen2" else q3).hf_config(cfg), architectures=[case["arch"]])
    if case["arch"].endswith("ForSequenceClassification"):
        out["num_labels"] = case["num_labels"]
    else:
        out["tie_word_embeddings"] = bool(case["tied"])
    return out


def to_hf_state_dict(case: dict, blob: np.ndarray, head: dict, seed: int, head_scale: float = 1.0) -> dict:
    """The tensors of a checkpoint of the case's architecture, under transformers' names (numpy arrays)."""
    cfg = case["cfg"]
    if kind_of(case) == 1:
        sd = {"model." + k: v for k, v in mb.to_hf_state_dict(cfg, blob).items()}
        if case.get("norm_bias"):  # norm_bias gives every LayerNorm of the model a bias: the backbone's stay zero (modernbert_ref.make_weights)
            zero = np.zeros(cfg["hidden"], np.float32)
            for k in [k for k in sd if k.endswith("norm.weight")]:
                sd[k[:-6] + "bias"] = zero
        sd.update({"head.dense.weight": head["dense_w"], "head.norm.weight": head["norm_g"], "classifier.weight": head["cls_w"], "classifier.bias": head["cls_b"]})
        if head["dense_b"] is not None:
            sd["head.dense.bias"] = head["dense_b"]
        if head["norm_b"] is not None:
            sd["head.norm.bias"] = head["norm_b"]
        return {k: np.ascontiguousarray(v) for k, v in sd.items()}
    sd = (q2 if family(cfg) == "qwen2" else q3).to_hf_state_dict(cfg, blob, prefix="model.")
    if case["arch"].endswith("ForSequenceClassification"):
        sd["score.weight"] = head["cls_w"]
    elif not case["tied"]:
        sd["lm_head.weight"] = np.float32(head_scale) * make_lm_head(cfg, seed)
    return {k: np.ascontiguousarray(v) for k, v in sd.items()}


# ------------------------------------------------------------------ the head kernels alone: inputs, float64 reference and forward error bound
U24 = 2.0 ** -24


EQ_COLS, EQ_VALS = (3, 7, 11, 19, 23, 29, 31, 37), (2.5, -2.2, 1.9, 2.1, -2.4, 2.3, 1.7, -1.8)


def kernel_case(B: int, H: int, kind: int, num_labels: int, biases: bool, seed: int):
    """(rows [B, H] f32, head) for the single-kernel tests: N(0,1) rows, dense_w ~ N(0, 1 / H), and -- kind 1 -- special rows in front, as far
    as B reaches: row 0 = 10 e_5 with dense_w[:, 5] = +-1 alternating, so the pre-activations sit at GELU's tails +-10; rows 1 .. 8 =
    2 e_k with dense_w[:, k] = (v - dense_b) / 2 for (k, v) of (EQ_COLS, EQ_VALS), so every pre-activation of the row is v up to rounding:
    a row of equal values behind the dense layer, whose variance (0, or 1e-15) is carried by norm_eps and whose last-bit noise the
    LayerNorm multiplies by 1 / sqrt(norm_eps) = 316 (eight of them: the largest of eight such errors is a steadier yardstick than one);
    row 9 = 0 (equal values again: gelu(dense_b) is not, zeros are).  The rows do not depend on B: a smaller B is a prefix."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    rows = f(33, H)
    cls_w, cls_b = f(num_labels, H), (f(num_labels) if biases else None)
    if kind == 2:
        return rows[:B].copy(), dict(kind=2, pooling="last", cls_w=cls_w, cls_b=cls_b)
    head = dict(kind=1, pooling="cls", norm_eps=1e-5, dense_w=f(H, H) / np.float32(np.sqrt(H)), dense_b=(np.float32(0.3) * f(H) if biases else None),
                norm_g=1 + np.float32(0.3) * f(H), norm_b=(np.float32(0.1) * f(H) if biases else None), cls_w=cls_w, cls_b=cls_b)
    db = head["dense_b"] if biases else np.zeros(H, np.float32)
    head["dense_w"][:, 5] = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    rows[:10] = 0
    rows[0, 5] = 10.0
    for i, (k, v) in enumerate(zip(EQ_COLS, EQ_VALS)):
        head["dense_w"][:, k] = (np.float32(v) - db) / np.float32(2.0)
        rows[1 + i, k] = 2.0
    return rows[:B].copy(), head


def head_bound(head: dict, rows: np.ndarray):
    """The linear head (kind 2): (logits, bound per logit) in float64 for an f32 evaluation on the same f32 inputs in ANY summation order --
    tests/test_rerank_gpu.py's dot-product bound 2 H 2^-24 sum_k |r_k w_k| + 2^-21, the bias among the terms."""
    assert head["kind"] == 2
    x = np.asarray(rows, np.float64)
    H = x.shape[1]
    wc = np.asarray(head["cls_w"], np.float64).reshape(-1, H)
    bc = np.zeros(wc.shape[0]) if head.get("cls_b") is None else np.asarray(head["cls_b"], np.float64)
    return x @ wc.T + bc, 2.0 * H * U24 * (np.abs(x) @ np.abs(wc).T + np.abs(bc)) + 2.0 ** -21


def _gelu_f32(x: np.ndarray) -> np.ndarray:
    """gemm_tile.h's gelu_erf_fast2 in numpy float32: gelu(x) = (h + |h|) - |h| 2^Q(|h|), h = x / 2, the same degree-7 polynomial, every fused
    multiply-add evaluated as a multiply, then an add."""
    f = np.float32
    h = x * f(0.5)
    ah = np.abs(h)
    q = ah * f(-0.000139362935) + f(0.00303643686)
    for coef in (-0.0268522501, 0.131913051, -0.428876668, -1.83460581, -2.30246782, 9.69476332e-06):
        q = q * ah + f(coef)
    return (-ah) * np.exp2(q) + (h + ah)


def head_f32(head: dict, rows: np.ndarray) -> np.ndarray:
    """A plain numpy float32 evaluation of the head in the order include/semcode_hip.h states (H a multiple of 64; fused multiply-adds as a
    multiply, then an add): the yardstick of what f32 arithmetic in that order costs, never the kernel's own output.
    kind 1: the dense layer in 16-wide stages, k = 16 st + 4 j + c in (c, j) order, even and odd stages in two chains; the three sums over n
    per lane (w, j) in (t, c) order over n = 64 t + 16 w + 4 j + c, then the 16 lanes in (w, j) order.  kind 2: 64 chains over the 4-element
    pieces j, j + 64, ..., added by the xor butterfly 32 .. 1."""
    f = np.float32
    x = np.asarray(rows, f)
    B, H = x.shape
    wc = np.asarray(head["cls_w"], f).reshape(-1, H)
    nl = wc.shape[0]
    bc = None if head.get("cls_b") is None else np.asarray(head["cls_b"], f)
    if head["kind"] == 2:
        P = -(-(H // 4) // 64) * 64  # pieces, padded to whole rounds of 64 lanes with zeros (a lane without a piece adds nothing)
        xp, wp = np.zeros((B, P * 4), f), np.zeros((nl, P * 4), f)
        xp[:, :H], wp[:, :H] = x, wc
        xp, wp = xp.reshape(B, P // 64, 64, 4), wp.reshape(nl, P // 64, 64, 4)
        lg = np.zeros((B, nl, 64), f)
        for rnd in range(P // 64):
            for c in range(4):
                lg = lg + wp[None, :, rnd, :, c] * xp[:, None, rnd, :, c]
        for off in (32, 16, 8, 4, 2, 1):
            lg = lg + lg[:, :, np.arange(64) ^ off]
        out = lg[:, :, 0]
        return out if bc is None else out + bc
    assert H % 64 == 0
    W = np.asarray(head["dense_w"], f)
    acc = [np.zeros((B, H), f), np.zeros((B, H), f)]
    for st in range(H // 16):
        for c in range(4):
            for j in range(4):
                k = 16 * st + 4 * j + c
                acc[st & 1] = acc[st & 1] + W[None, :, k] * x[:, k:k + 1]
    a = acc[0] + acc[1]
    if head.get("dense_b") is not None:
        a = a + np.asarray(head["dense_b"], f)
    T = H // 64
    G = _gelu_f32(a).reshape(B, T, 4, 4, 4)  # [row, t, w, j, c]

    def lanes_then_rows(terms):  # terms [B, T, 4, 4, 4] -> [B]: per lane in (t, c) order, then the lanes in (w, j) order
        lane = np.zeros((B, 4, 4), f)
        for t in range(T):
            for c in range(4):
                lane = lane + terms[:, t, :, :, c]
        tot = np.zeros(B, f)
        for w in range(4):
            for j in range(4):
                tot = tot + lane[:, w, j]
        return tot

    mean = (lanes_then_rows(G) / f(H)).reshape(B, 1, 1, 1, 1)
    dv = G - mean
    rstd = (f(1.0) / np.sqrt(lanes_then_rows(dv * dv) / f(H) + f(head["norm_eps"]))).reshape(B, 1, 1, 1, 1)
    p = dv * rstd * np.asarray(head["norm_g"], f).reshape(1, T, 4, 4, 4)
    if head.get("norm_b") is not None:
        p = p + np.asarray(head["norm_b"], f).reshape(1, T, 4, 4, 4)
    out = np.stack([lanes_then_rows(wc[l].reshape(1, T, 4, 4, 4) * p) for l in range(nl)], axis=1)
    return out if bc is None else out + bc
