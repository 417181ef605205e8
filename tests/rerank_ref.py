"""The shared recipe of the reranker tests: seeded cross-encoder weights, pairs, and a float64 restatement of the pair forward.
TEST INFRASTRUCTURE ONLY (tests/test_rerank_*.py, scripts/gen_rerank_fixtures.py).

tests/golden/rerank_golden.{npz,json} stores ids, offsets, first_lens and what transformers' BertForSequenceClassification (fp32, CPU)
computes for them -- not the weights: make_weights / make_head rebuild those from (cfg, seed).  The encoder blob is
oracle.bert_oracle.make_blob(cfg, seed, "test") with type_emb x 8, Wq / Wk x 4 and Wv / Wo x vo_scale (4 .. 8), the classifier
weight is drawn x 8: with the 0.02-scale weights of make_blob alone, segment ids and attention move the logits by less than bf16
rounding does, and a forward that ignores them would pass.  The method is scripts/gen_nomic_fixtures.py's; the generator checks that
three wrong segment conventions (DEVIATIONS) fall outside the logit bound before it writes anything.
"""
from __future__ import annotations

import numpy as np

from oracle import bert_oracle as bo

COMMON = dict(vocab=400, layers=2, max_pos=512, type_vocab=2, ln_eps=1e-12)
MODELS = {"small": dict(hidden=128, heads=2, ffn=512), "mid": dict(hidden=256, heads=4, ffn=1024), "base": dict(hidden=768, heads=12, ffn=3072)}
# what the head of each model looks like: every combination the kernel has a path for appears once
HEADS = {"small": dict(num_labels=2, pooler=True), "mid": dict(num_labels=1, pooler=False), "base": dict(num_labels=1, pooler=True)}
VO_SCALE = {"small": 8.0, "mid": 6.0, "base": 4.0}
FOLDS = {"small": False, "mid": True, "base": True}  # shapes the LayerNorm-folded batch pipeline takes (every GEMM dimension % 256)
CLS_ID, SEP_ID, FIRST_WORD = 1, 2, 3
N_QUESTIONS, N_PASSAGES = 4, 8
DEVIATIONS = ("types0", "flipped", "sep1")


def model_cfg(name: str) -> dict:
    return dict(COMMON, **MODELS[name])


def make_weights(cfg: dict, seed: int, vo_scale: float) -> np.ndarray:
    blob = bo.make_blob(cfg, seed, "test").copy()
    W = bo.unpack(cfg, blob)  # views into blob
    W["type_emb"] *= 8.0
    for l in range(cfg["layers"]):
        for n, s in (("wq", 4.0), ("wk", 4.0), ("wv", vo_scale), ("wo", vo_scale)):
            W[f"l{l}.{n}"] *= s
    return blob


def make_head(cfg: dict, seed: int, num_labels: int, pooler: bool) -> dict:
    """Pooler ~ N(0, 1 / H) (pre-activations of order one, so tanh bends), classifier 8 x N(0, 1 / H), biases 0.1 x N(0, 1)."""
    H = cfg["hidden"]
    rng = np.random.default_rng(77000 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    head = dict(pooler_w=f(H, H) / np.float32(np.sqrt(H)), pooler_b=np.float32(0.1) * f(H), cls_w=np.float32(8.0) * f(num_labels, H) / np.float32(np.sqrt(H)),
                cls_b=np.float32(0.1) * f(num_labels))
    if not pooler:
        head["pooler_w"] = head["pooler_b"] = None
    return head


def make_pairs(cfg: dict, seed: int):
    """N_QUESTIONS x N_PASSAGES pairs, question-major: (ids_flat int32, offsets int64, first_lens int32).  Question part 5 .. 20 tokens
    ([CLS] .. [SEP]), pair 30 .. 96 tokens; pair (0, 0) has 333 tokens (attention class 0), pair (1, 1) max_pos = 512, the passage of
    pair (2, 2) is a single token."""
    rng = np.random.default_rng(88000 + seed)
    rows, first = [], []
    for q in range(N_QUESTIONS):
        lq = int(rng.integers(5, 21))
        qids = [CLS_ID] + rng.integers(FIRST_WORD, cfg["vocab"], lq - 2).tolist() + [SEP_ID]
        for p in range(N_PASSAGES):
            total = int(rng.integers(30, 97))
            if (q, p) == (0, 0):
                total = 333
            elif (q, p) == (1, 1):
                total = cfg["max_pos"]
            elif (q, p) == (2, 2):
                total = lq + 2
            rows.append(qids + rng.integers(FIRST_WORD, cfg["vocab"], total - lq - 1).tolist() + [SEP_ID])
            first.append(lq)
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return np.concatenate([np.asarray(r, np.int32) for r in rows]), offsets, np.asarray(first, np.int32)


def segment_ids(n: int, first_len: int, deviate: "str | None" = None) -> np.ndarray:
    t = (np.arange(n) >= first_len).astype(np.int64)
    if deviate == "types0":
        t[:] = 0
    elif deviate == "flipped":
        t = 1 - t
    elif deviate == "sep1":  # the question's [SEP] counted to the passage
        t[first_len - 1] = 1
    elif deviate is not None:
        raise ValueError(deviate)
    return t


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps) * g + b


def _gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def forward_cls(cfg: dict, W: dict, ids: np.ndarray, first_len: int, deviate: "str | None" = None) -> np.ndarray:
    """One pair, unpadded, float64: the last hidden state of its [CLS] row.  W = {name: float64 array} of bert_oracle.unpack."""
    n, H, nh = len(ids), cfg["hidden"], cfg["heads"]
    x = W["word_emb"][ids] + W["pos_emb"][np.arange(n)] + W["type_emb"][segment_ids(n, first_len, deviate)]
    x = _ln(x, W["emb_ln_g"], W["emb_ln_b"], cfg["ln_eps"])
    sp = lambda t: t.reshape(n, nh, 64).transpose(1, 0, 2)
    for l in range(cfg["layers"]):
        p = f"l{l}."
        q, k, v = (x @ W[p + "w" + c].T + W[p + "b" + c] for c in "qkv")
        s = sp(q) @ sp(k).transpose(0, 2, 1) / 8.0
        e = np.exp(s - s.max(-1, keepdims=True))
        ctx = ((e / e.sum(-1, keepdims=True)) @ sp(v)).transpose(1, 0, 2).reshape(n, H)
        x = _ln(ctx @ W[p + "wo"].T + W[p + "bo"] + x, W[p + "ln1_g"], W[p + "ln1_b"], cfg["ln_eps"])
        x = _ln(_gelu(x @ W[p + "w1"].T + W[p + "b1"]) @ W[p + "w2"].T + W[p + "b2"] + x, W[p + "ln2_g"], W[p + "ln2_b"], cfg["ln_eps"])
    return x[0]


def head_logits(head: dict, cls: np.ndarray) -> np.ndarray:
    """cls [B, H] -> logits [B, num_labels] in float64: classifier(tanh(pooler(cls))), or classifier(cls) without a pooler."""
    p = np.asarray(cls, np.float64)
    if head["pooler_w"] is not None:
        p = np.tanh(p @ head["pooler_w"].astype(np.float64).T + head["pooler_b"].astype(np.float64))
    return p @ head["cls_w"].astype(np.float64).T + head["cls_b"].astype(np.float64)


def forward(cfg: dict, blob: np.ndarray, head: dict, ids_flat, offsets, first_lens, deviate: "str | None" = None):
    """All pairs -> (cls [B, H], logits [B, num_labels]) float64."""
    W = {k: v.astype(np.float64) for k, v in bo.unpack(cfg, blob).items()}
    cls = np.stack([forward_cls(cfg, W, np.asarray(ids_flat[offsets[i]:offsets[i + 1]]), int(first_lens[i]), deviate) for i in range(len(first_lens))])
    return cls, head_logits(head, cls)


def scores(logits: np.ndarray) -> np.ndarray:
    """1 label: the logit; 2 labels: logit[1] - logit[0]."""
    logits = np.asarray(logits)
    return logits[:, 0] if logits.shape[1] == 1 else logits[:, 1] - logits[:, 0]


def ordered_pairs(score_row: np.ndarray, gap: float) -> "list[tuple[int, int]]":
    """Passage pairs (i, j) of one question whose reference scores differ by more than gap, i the better one."""
    n = len(score_row)
    return [(i, j) for i in range(n) for j in range(n) if score_row[i] - score_row[j] > gap]


def to_hf_state_dict(cfg: dict, blob: np.ndarray, head: dict) -> dict:
    """BertForSequenceClassification names (numpy arrays): bert.*, bert.pooler.dense.* when the head has a pooler, classifier.*."""
    sd = {"bert." + k: v.numpy() for k, v in bo.to_hf_state_dict(cfg, blob).items()}
    if head["pooler_w"] is not None:
        sd["bert.pooler.dense.weight"], sd["bert.pooler.dense.bias"] = head["pooler_w"], head["pooler_b"]
    sd["classifier.weight"], sd["classifier.bias"] = head["cls_w"], head["cls_b"]
    return sd
