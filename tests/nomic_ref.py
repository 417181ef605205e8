"""CPU restatement (numpy float64) of the nomic-bert forward.  TEST INFRASTRUCTURE ONLY.

nomic-bert (nomic-embed-text-v1 / v1.5) is a post-LN BERT without a position table: rotary position embedding on Q and K
("rotate-half" pairing (j, j + 32) of a 64-wide head, angle p * theta^(-2j/64)), a SwiGLU feed-forward silu(Wg y) * (Wu y), no
bias on any Linear layer, LayerNorms with gamma and beta, masked mean pooling.  Pinned to transformers' NomicBertModel (fp32,
eager attention) by tests/golden/nomic_golden.npz, written by scripts/gen_nomic_fixtures.py.

Blob layout = rotary + SwiGLU of include/semcode_hip.h: no position table, W1 = [2 ffn, H] (gate rows, then up rows), bias slots
kept (zeros).  That is exactly oracle.bert_oracle's layout for alibi + geglu, reused here for the layout alone.
"""
from __future__ import annotations

import numpy as np

from oracle import bert_oracle as bo


def layout_cfg(cfg: dict) -> dict:
    """cfg as oracle.bert_oracle must see it to lay a rotary + SwiGLU blob out (no position table, W1 = [2F, H])."""
    c = {k: v for k, v in cfg.items() if k not in ("rotary", "swiglu", "rope_theta")}
    return dict(c, alibi=True, geglu=True)


def make_weights(cfg: dict, seed: int, qk_scale: float = 4.0) -> np.ndarray:
    """The fixtures' weight rule: make_blob(style="test") tensors, Linear biases zeroed (the family has none), Wq and Wk times
    qk_scale.  Without the scale the first layer's attention scores have a standard deviation of 0.1-0.3, the softmax is nearly
    uniform and a forward WITHOUT any rotation passes the pooled-vector tolerance; at 4 every convention mix-up fails it."""
    lc = layout_cfg(cfg)
    blob = bo.make_blob(lc, seed, "test")
    u = bo.unpack(lc, blob)  # views into blob
    for l in range(cfg["layers"]):
        for b in ("bq", "bk", "bv", "bo", "b1", "b2"):
            u[f"l{l}.{b}"][:] = 0.0
        u[f"l{l}.wq"][:] *= np.float32(qk_scale)
        u[f"l{l}.wk"][:] *= np.float32(qk_scale)
    return blob


def rope_tables(S: int, theta: float, dh: int = 64):
    f = float(theta) ** (-2.0 * np.arange(dh // 2, dtype=np.float64) / dh)
    ang = np.arange(S, dtype=np.float64)[:, None] * f[None, :]
    return np.cos(ang), np.sin(ang)


def rotate_half(t: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    """t [..., S, dh]; pairs (j, j + dh/2)."""
    h = t.shape[-1] // 2
    a, b = t[..., :h], t[..., h:]
    return np.concatenate([a * cos - b * sin, b * cos + a * sin], axis=-1)


def rotate_interleaved(t: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    """The OTHER convention (pairs (2j, 2j + 1)); only the fixture generator's sensitivity check uses it."""
    a, b = t[..., 0::2], t[..., 1::2]
    out = np.empty_like(t)
    out[..., 0::2] = a * cos - b * sin
    out[..., 1::2] = b * cos + a * sin
    return out


def _layernorm(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def _gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def forward(cfg: dict, blob: np.ndarray, ids: np.ndarray, lens: np.ndarray, theta: float, deviate: "str | None" = None) -> np.ndarray:
    """ids [B, S] int, lens [B] -> pooled [B, H] f32.  deviate: one deliberate departure from the model, for the fixture generator's
    check that the fixtures can tell it apart: "no_rope" | "interleaved" | "theta" (10000 <-> 1000) | "gelu" | "swap"."""
    lc = layout_cfg(cfg)
    W = {k: v.astype(np.float64) for k, v in bo.unpack(lc, blob).items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    lens = np.clip(np.asarray(lens), 1, S)
    H, nh, F, eps = cfg["hidden"], cfg["heads"], cfg["ffn"], cfg["ln_eps"]
    dh = H // nh
    if deviate == "theta":
        theta = 10000.0 if float(theta) != 10000.0 else 1000.0
    cos, sin = rope_tables(S, theta, dh)
    rot = {None: rotate_half, "interleaved": rotate_interleaved}.get(deviate, rotate_half)
    out = np.empty((B, H), np.float64)
    for b in range(B):  # one chunk at a time: a [heads, 2048, 2048] f64 score tensor is large enough
        n = int(lens[b])
        x = _layernorm(W["word_emb"][ids[b]] + W["type_emb"][0][None], W["emb_ln_g"], W["emb_ln_b"], eps)
        for l in range(cfg["layers"]):
            p = f"l{l}."
            sp = lambda t: t.reshape(S, nh, dh).transpose(1, 0, 2)
            q, k, v = sp(x @ W[p + "wq"].T + W[p + "bq"]), sp(x @ W[p + "wk"].T + W[p + "bk"]), sp(x @ W[p + "wv"].T + W[p + "bv"])
            if deviate != "no_rope":
                q, k = rot(q, cos, sin), rot(k, cos, sin)
            s = q @ k[:, :n].transpose(0, 2, 1) / np.sqrt(dh)  # keys >= len masked = left out
            e = np.exp(s - s.max(-1, keepdims=True))
            ctx = ((e / e.sum(-1, keepdims=True)) @ v[:, :n]).transpose(1, 0, 2).reshape(S, H)
            x = _layernorm(ctx @ W[p + "wo"].T + W[p + "bo"] + x, W[p + "ln1_g"], W[p + "ln1_b"], eps)
            h = x @ W[p + "w1"].T + W[p + "b1"]
            gate, up = (h[:, F:], h[:, :F]) if deviate == "swap" else (h[:, :F], h[:, F:])
            act = _gelu(gate) if deviate == "gelu" else gate / (1.0 + np.exp(-gate))
            x = _layernorm((act * up) @ W[p + "w2"].T + W[p + "b2"] + x, W[p + "ln2_g"], W[p + "ln2_b"], eps)
        out[b] = x[:n].mean(0)
    return out.astype(np.float32)


def to_hf_state_dict(cfg: dict, blob: np.ndarray) -> dict:
    """Blob -> transformers NomicBertModel(add_pooling_layer=False) state_dict names (numpy arrays)."""
    W = bo.unpack(layout_cfg(cfg), blob)
    F = cfg["ffn"]
    sd = {"embeddings.word_embeddings.weight": W["word_emb"], "embeddings.token_type_embeddings.weight": W["type_emb"],
          "embeddings.LayerNorm.weight": W["emb_ln_g"], "embeddings.LayerNorm.bias": W["emb_ln_b"]}
    for l in range(cfg["layers"]):
        p, q = f"l{l}.", f"layers.{l}."
        sd.update({q + "self_attn.q_proj.weight": W[p + "wq"], q + "self_attn.k_proj.weight": W[p + "wk"],
                   q + "self_attn.v_proj.weight": W[p + "wv"], q + "self_attn.o_proj.weight": W[p + "wo"],
                   q + "post_attention_layernorm.weight": W[p + "ln1_g"], q + "post_attention_layernorm.bias": W[p + "ln1_b"],
                   q + "mlp.gate_proj.weight": W[p + "w1"][:F], q + "mlp.up_proj.weight": W[p + "w1"][F:],
                   q + "mlp.down_proj.weight": W[p + "w2"],
                   q + "post_mlp_layernorm.weight": W[p + "ln2_g"], q + "post_mlp_layernorm.bias": W[p + "ln2_b"]})
    return {k: np.ascontiguousarray(v) for k, v in sd.items()}
