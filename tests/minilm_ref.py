"""The shared recipe of the head-dimension-32 tests: seeded MiniLM-shaped weights and inputs.  TEST INFRASTRUCTURE ONLY
(tests/test_headdim32_*.py, scripts/gen_minilm_fixtures.py).

tests/golden/minilm_golden.{npz,json} stores ids, lengths and what transformers' BertModel / BertForSequenceClassification (fp32, CPU)
compute for them -- not the weights: make_weights rebuilds those from (cfg, seed).  The blob is oracle.bert_oracle.make_blob(cfg, seed,
"test") with Wq, Wk, Wv, Wo x 8: with the 0.02-scale weights of make_blob alone, attention moves the pooled vector by less than bf16
rounding does, and a forward that split the hidden size into half as many heads of 64 would pass.  The generator checks that this wrong
split falls outside the bound in every sequence before it writes anything.
"""
from __future__ import annotations

import numpy as np

from oracle import bert_oracle as bo

COMMON = dict(vocab=400, layers=2, max_pos=512, type_vocab=2, ln_eps=1e-12)
# every head is 32 wide.  h384: the MiniLM width, 6 head pairs, not foldable (384 % 256); h128: two pairs; h256: the LayerNorm-folded
# batch pipeline (every GEMM dimension % 256 == 0)
SHAPES = {"h384": dict(hidden=384, heads=12, ffn=1536), "h128": dict(hidden=128, heads=4, ffn=256), "h256": dict(hidden=256, heads=8, ffn=512)}
FOLDS = {"h384": False, "h128": False, "h256": True}
LENS = (128, 77, 33, 2, 5, 100)  # token lengths of the batch at S = 128
LONG = 512                       # and one text of max_pos tokens
QKVO_SCALE = 8.0
PAIR_SHAPE = "h384"              # the cross-encoder: 1 label, pooler (the ms-marco-MiniLM head)
TYPE_SCALE = 8.0                 # its segment embeddings, as tests/rerank_ref.py scales them


def model_cfg(name: str) -> dict:
    return dict(COMMON, **SHAPES[name])


def make_weights(cfg: dict, seed: int, type_scale: float = 1.0) -> np.ndarray:
    blob = bo.make_blob(cfg, seed, "test").copy()
    W = bo.unpack(cfg, blob)  # views into blob
    W["type_emb"] *= np.float32(type_scale)
    for l in range(cfg["layers"]):
        for n in ("wq", "wk", "wv", "wo"):
            W[f"l{l}.{n}"] *= np.float32(QKVO_SCALE)
    return blob


def make_inputs(cfg: dict, seed: int):
    """(ids [6, 128] int32 zero-padded, lens [6] int32, long_ids [1, 512] int32)."""
    rng = np.random.default_rng(99000 + seed)
    lens = np.asarray(LENS, np.int32)
    ids = np.zeros((len(LENS), 128), np.int32)
    for i, n in enumerate(LENS):
        ids[i, :n] = rng.integers(1, cfg["vocab"], n)
    return ids, lens, rng.integers(1, cfg["vocab"], (1, LONG)).astype(np.int32)


def attention_ref(qkv: np.ndarray, lens, S: int, heads: int, head_dim: int) -> np.ndarray:
    """float64 softmax attention of qkv [B*S, 3H] (Q | K | V, head h at columns h * head_dim of each third; the caller rounds the inputs
    to bf16) over the first lens[b] keys of every sequence -> [B*S, H]."""
    H = heads * head_dim
    q, k, v = (qkv[:, i * H:(i + 1) * H].astype(np.float64).reshape(-1, S, heads, head_dim).transpose(0, 2, 1, 3) for i in range(3))
    out = np.empty_like(q)
    for b, n in enumerate(lens):
        n = max(1, min(int(n), S))
        s = q[b] @ k[b, :, :n].transpose(0, 2, 1) / np.sqrt(head_dim)
        e = np.exp(s - s.max(-1, keepdims=True))
        out[b] = (e / e.sum(-1, keepdims=True)) @ v[b, :, :n]
    return out.transpose(0, 2, 1, 3).reshape(-1, H)
