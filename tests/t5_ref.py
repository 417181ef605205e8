"""CPU restatement (numpy float64) of the T5 ENCODER as an embedding model.  TEST INFRASTRUCTURE ONLY.

T5 (CodeT5+, GTR, sentence-T5) is a PRE-norm bidirectional encoder: h = tok_emb[id]; per layer h += Wo Attn(RMS(h)), h += W2 act(W1 RMS(h));
RMS_final before pooling.  No embedding norm, no position and no type table, no biases.  RMS(x) = x * rsqrt(mean(x^2) + eps) * gamma.
Scores are q.k + bias[head][bucket(j - i)] over the real keys, WITHOUT 1/sqrt(d); one learned [buckets, heads] table for all layers.
act = ReLU ("relu", T5 v1.0) or the tanh-GELU gate gelu_new(wi_0 m) * (wi_1 m) ("gated-gelu", v1.1).  The vector of a text is the row of
its first token ("first") or the mean over its real tokens ("mean").
Pinned to transformers' T5EncoderModel (fp32, eager) by tests/golden/t5_golden.npz, written by scripts/gen_t5_fixtures.py.

Blob layout = arch 3 of include/semcode_hip.h, AW = heads * 64: word_emb, rel_bias [buckets, heads], per layer Wq [AW,H] bq Wk bk Wv bv
Wo [H,AW] bo ln1 W1 ([F,H], or [2F,H] = wi_0 then wi_1) b1 W2 b2 ln2, then final_norm gamma / beta.  Bias and beta slots stay, as zeros.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import sc_oracle as orc

DEVIATIONS = ("no_bias", "mirrored", "unidirectional_buckets", "scores/8", "bias_layer0_only", "layernorm_stats", "relu<->gelu",
              "gate_halves_swapped", "erf_gelu", "pooling_swapped")
PROJ_DEVIATIONS = ("proj_skipped", "normalise_before_proj")  # of the projection behind the pooling (project below)


def make_proj(hidden: int, E: int, seed: int, bias: bool):
    """The fixtures' projection: W [E, hidden] = N(0,1) / sqrt(hidden), b [E] = 0.1 * N(0,1) or None (the oracle's generator, its own seed)."""
    unit = orc.synth(E * hidden + E, 1, seed + 7000).reshape(-1).astype(np.float32)
    W = (unit[:E * hidden].reshape(E, hidden) / np.float32(np.sqrt(hidden))).astype(np.float32)
    return W, ((np.float32(0.1) * unit[E * hidden:]).astype(np.float32) if bias else None)


def project(pooled: np.ndarray, W: np.ndarray, b, deviate: "str | None" = None) -> np.ndarray:
    """pooled [B, H] (un-normalised) -> L2-normalised W pooled + b, float64 inside.  deviate: "proj_skipped" (the normalised pooled row itself;
    comparable where E == H only) | "normalise_before_proj" (the pooled row normalised first: shows where there is a bias)."""
    assert deviate is None or deviate in PROJ_DEVIATIONS, deviate
    x = pooled.astype(np.float64)
    if deviate == "normalise_before_proj":
        x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    y = x if deviate == "proj_skipped" else x @ W.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
    return (y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-12)).astype(np.float32)


def gated(cfg: dict) -> bool:
    return cfg["t5_ffn"] == "gated-gelu"


def attn_width(cfg: dict) -> int:
    return cfg["heads"] * 64 if cfg.get("head_dim") else cfg["hidden"]


def blob_layout(cfg: dict) -> list:
    H, F, AW = cfg["hidden"], cfg["ffn"], attn_width(cfg)
    F1 = 2 * F if gated(cfg) else F
    out = [("word_emb", (cfg["vocab"], H)), ("rel_bias", (cfg["rel_buckets"], cfg["heads"]))]
    for l in range(cfg["layers"]):
        p = f"l{l}."
        out += [(p + "wq", (AW, H)), (p + "bq", (AW,)), (p + "wk", (AW, H)), (p + "bk", (AW,)), (p + "wv", (AW, H)), (p + "bv", (AW,)),
                (p + "wo", (H, AW)), (p + "bo", (H,)), (p + "ln1_g", (H,)), (p + "ln1_b", (H,)),
                (p + "w1", (F1, H)), (p + "b1", (F1,)), (p + "w2", (H, F)), (p + "b2", (H,)), (p + "ln2_g", (H,)), (p + "ln2_b", (H,))]
    return out + [("final_g", (H,)), ("final_b", (H,))]


def blob_size(cfg: dict) -> int:
    return int(sum(int(np.prod(s)) for _, s in blob_layout(cfg)))


def unpack(cfg: dict, blob: np.ndarray) -> dict:
    blob = np.asarray(blob, dtype=np.float32).reshape(-1)
    assert blob.size == blob_size(cfg), (blob.size, blob_size(cfg))
    out, off = {}, 0
    for name, shape in blob_layout(cfg):
        n = int(np.prod(shape))
        out[name] = blob[off:off + n].reshape(shape)
        off += n
    return out


def make_weights(cfg: dict, seed: int, qk_scale: float = 2.0, bias_sigma: float = 1.0, vo_scale: float = 3.0, mlp_scale: float = 3.0,
                 emb_scale: float = 5.0, norm_sigma: float = 0.3) -> np.ndarray:
    """The fixtures' weight rule: every tensor 0.02 * N(0,1) (the integer-hash generator of the oracle), then Wq and Wk times qk_scale, Wv
    and Wo times vo_scale, W1 and W2 times mlp_scale (stated for hidden 128, all shrinking with sqrt(128 / hidden)), the embedding table
    times emb_scale, RMSNorm gammas 1 + norm_sigma * N(0,1), every bias and beta slot zero (the family has none) and the relative bias
    table RE-DRAWN as bias_sigma * N(0,1): at the default initialisation it is too small against the scores to pin anything."""
    unit = orc.synth(blob_size(cfg), 1, seed).reshape(-1).astype(np.float32)  # N(0,1)
    blob = (np.float32(0.02) * unit).astype(np.float32)
    u, n = unpack(cfg, blob), unpack(cfg, unit)  # views
    for name, seg in u.items():
        leaf = name.split(".")[-1]
        if leaf.endswith("_g"):
            seg[:] = 1.0 + np.float32(norm_sigma) * n[name]
        elif leaf.endswith("_b") or leaf in ("bq", "bk", "bv", "bo", "b1", "b2"):
            seg[:] = 0.0
    u["word_emb"][:] *= np.float32(emb_scale)
    u["rel_bias"][:] = np.float32(bias_sigma) * n["rel_bias"]
    width = np.sqrt(128.0 / cfg["hidden"])
    for l in range(cfg["layers"]):
        for name, sc in (("wq", qk_scale), ("wk", qk_scale), ("wv", vo_scale), ("wo", vo_scale), ("w1", mlp_scale), ("w2", mlp_scale)):
            u[f"l{l}.{name}"][:] *= np.float32(sc * width)
    return blob


def buckets(rel: np.ndarray, nbuckets: int, max_distance: int, bidirectional: bool = True) -> np.ndarray:
    """transformers' _relative_position_bucket on rel = key - query, the logarithmic arm in float32 as there."""
    rel = np.asarray(rel, np.int64)
    nb = nbuckets
    out = np.zeros_like(rel)
    if bidirectional:
        nb //= 2
        out += (rel > 0) * nb
        n = np.abs(rel)
    else:
        n = -np.minimum(rel, 0)
    me = nb // 2
    ratio = np.log(np.maximum(n, 1).astype(np.float32) / np.float32(me)) / np.float32(math.log(max_distance / me))  # (n = 0 takes the exact arm)
    large = me + (ratio.astype(np.float32) * np.float32(nb - me)).astype(np.int64)
    large = np.minimum(large, nb - 1)
    return out + np.where(n < me, n, large)


def _rms(x, g, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * g


def _layernorm(x, g, eps):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps) * g


def gelu_new(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf(x):
    erf = np.vectorize(math.erf, otypes=[np.float64])
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def forward(cfg: dict, blob: np.ndarray, ids: np.ndarray, lens: np.ndarray, pooling: str = "mean", deviate: "str | None" = None) -> np.ndarray:
    """ids [B, S] int, lens [B] -> [B, H] f32: RMS_final of the first token's row ("first") or its mean over the real tokens ("mean").
    deviate: one deliberate departure from the model (DEVIATIONS): "no_bias" | "mirrored" (the bias of query - key) |
    "unidirectional_buckets" | "scores/8" | "bias_layer0_only" | "layernorm_stats" | "relu<->gelu" (the other activation; on a gated model
    a ReLU gate) | "gate_halves_swapped" | "erf_gelu" (gated models) | "pooling_swapped"."""
    assert deviate is None or deviate in DEVIATIONS, deviate
    assert pooling in ("first", "mean"), pooling
    if deviate == "pooling_swapped":
        pooling = "mean" if pooling == "first" else "first"
    W = {k: v.astype(np.float64) for k, v in unpack(cfg, blob).items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    lens = np.clip(np.asarray(lens), 1, S)
    H, nh, F, eps, AW = cfg["hidden"], cfg["heads"], cfg["ffn"], cfg["ln_eps"], attn_width(cfg)
    norm = _layernorm if deviate == "layernorm_stats" else _rms
    out = np.empty((B, H), np.float64)
    for b in range(B):  # rows at or beyond len never reach a real row (a real query's keys are real): leave them out
        n = int(lens[b])
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        rel = (i - j) if deviate == "mirrored" else (j - i)
        bk = buckets(rel, cfg["rel_buckets"], cfg["rel_max_distance"], bidirectional=deviate != "unidirectional_buckets")
        bias = W["rel_bias"][bk].transpose(2, 0, 1)  # [heads, n, n]
        if deviate == "no_bias":
            bias = np.zeros_like(bias)
        h = W["word_emb"][ids[b, :n]]
        for l in range(cfg["layers"]):
            p = f"l{l}."
            a = norm(h, W[p + "ln1_g"], eps)
            q = (a @ W[p + "wq"].T + W[p + "bq"]).reshape(n, nh, 64).transpose(1, 0, 2)
            k = (a @ W[p + "wk"].T + W[p + "bk"]).reshape(n, nh, 64).transpose(1, 0, 2)
            v = (a @ W[p + "wv"].T + W[p + "bv"]).reshape(n, nh, 64).transpose(1, 0, 2)
            s = q @ k.transpose(0, 2, 1)
            if deviate == "scores/8":
                s = s / 8.0
            if not (deviate == "bias_layer0_only" and l > 0):
                s = s + bias
            e = np.exp(s - s.max(-1, keepdims=True))
            ctx = ((e / e.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(n, AW)
            h = ctx @ W[p + "wo"].T + W[p + "bo"] + h
            m = norm(h, W[p + "ln2_g"], eps)
            u = m @ W[p + "w1"].T + W[p + "b1"]
            if gated(cfg):
                gate, up = (u[:, F:], u[:, :F]) if deviate == "gate_halves_swapped" else (u[:, :F], u[:, F:])
                act = np.maximum(gate, 0.0) if deviate == "relu<->gelu" else gelu_erf(gate) if deviate == "erf_gelu" else gelu_new(gate)
                mid = act * up
            else:
                mid = gelu_new(u) if deviate == "relu<->gelu" else np.maximum(u, 0.0)
            h = mid @ W[p + "w2"].T + W[p + "b2"] + h
        h = norm(h, W["final_g"], eps)
        out[b] = h[0] if pooling == "first" else h.mean(0)
    return out.astype(np.float32)


def hf_config(cfg: dict) -> dict:
    """The config.json of transformers' T5EncoderModel for cfg (the keys the loader reads, in the released checkpoints' spelling)."""
    return {"model_type": "t5", "vocab_size": cfg["vocab"], "d_model": cfg["hidden"], "d_kv": 64, "num_heads": cfg["heads"],
            "num_layers": cfg["layers"], "d_ff": cfg["ffn"], "relative_attention_num_buckets": cfg["rel_buckets"],
            "relative_attention_max_distance": cfg["rel_max_distance"], "layer_norm_epsilon": cfg["ln_eps"],
            "feed_forward_proj": cfg["t5_ffn"], "dropout_rate": 0.0, "is_encoder_decoder": False, "use_cache": False}


def to_hf_state_dict(cfg: dict, blob: np.ndarray, prefix: str = "") -> dict:
    """Blob -> transformers T5EncoderModel state_dict names (numpy arrays)."""
    W = unpack(cfg, blob)
    F = cfg["ffn"]
    sd = {"shared.weight": W["word_emb"], "encoder.embed_tokens.weight": W["word_emb"], "encoder.final_layer_norm.weight": W["final_g"],
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": W["rel_bias"]}
    for l in range(cfg["layers"]):
        p, q = f"l{l}.", f"encoder.block.{l}.layer."
        sd.update({q + "0.SelfAttention.q.weight": W[p + "wq"], q + "0.SelfAttention.k.weight": W[p + "wk"], q + "0.SelfAttention.v.weight": W[p + "wv"],
                   q + "0.SelfAttention.o.weight": W[p + "wo"], q + "0.layer_norm.weight": W[p + "ln1_g"], q + "1.layer_norm.weight": W[p + "ln2_g"],
                   q + "1.DenseReluDense.wo.weight": W[p + "w2"]})
        if gated(cfg):
            sd.update({q + "1.DenseReluDense.wi_0.weight": W[p + "w1"][:F], q + "1.DenseReluDense.wi_1.weight": W[p + "w1"][F:]})
        else:
            sd[q + "1.DenseReluDense.wi.weight"] = W[p + "w1"]
    return {prefix + k: np.ascontiguousarray(v) for k, v in sd.items()}
