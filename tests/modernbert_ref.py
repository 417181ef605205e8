"""CPU restatement (numpy float64) of the ModernBERT forward.  TEST INFRASTRUCTURE ONLY.

ModernBERT (answerdotai/ModernBERT-base, gte-modernbert-base, modernbert-embed-base) is a PRE-norm encoder:
h = LN(tok_emb[id]); per layer h += Attn(attn_norm(h)), h += MLP(mlp_norm(h)), attn_norm of layer 0 the identity; final_norm before
pooling.  No position and no type table, LayerNorms without bias, no bias on any Linear.  Rotary positions ("rotate-half" pairs
(j, j + 32) of a 64-wide head) with two bases: the global layers (l % global_every == 0) use rope_theta, the others rope_theta_local
and see only the real keys with |i - j| <= local_window / 2.  MLP = Wo (gelu(Wi[:F] m) * (Wi[F:] m)).
Pinned to transformers' ModernBertModel (fp32, eager attention) by tests/golden/modernbert_golden.npz, written by
scripts/gen_modernbert_fixtures.py.

Blob layout = arch 1 of include/semcode_hip.h: word_emb, emb_ln gamma / beta, per layer Wq bq Wk bk Wv bv Wo bo ln1 (= attn_norm; layer
0's slot present and ignored) W1 (= Wi: gate rows first) b1 W2 b2 ln2 (= mlp_norm), then final_norm gamma / beta.  Bias and beta slots
stay (zeros here: the family has none).
"""
from __future__ import annotations

import numpy as np

from oracle import sc_oracle as orc

DEVIATIONS = ("no_window", "window_m2", "local_base", "global_base", "post_norm", "attn_norm0", "swap")


def blob_layout(cfg: dict) -> list:
    H, F = cfg["hidden"], cfg["ffn"]
    out = [("word_emb", (cfg["vocab"], H)), ("emb_ln_g", (H,)), ("emb_ln_b", (H,))]
    for l in range(cfg["layers"]):
        p = f"l{l}."
        out += [(p + "wq", (H, H)), (p + "bq", (H,)), (p + "wk", (H, H)), (p + "bk", (H,)), (p + "wv", (H, H)), (p + "bv", (H,)),
                (p + "wo", (H, H)), (p + "bo", (H,)), (p + "ln1_g", (H,)), (p + "ln1_b", (H,)),
                (p + "w1", (2 * F, H)), (p + "b1", (2 * F,)), (p + "w2", (H, F)), (p + "b2", (H,)), (p + "ln2_g", (H,)), (p + "ln2_b", (H,))]
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


def make_weights(cfg: dict, seed: int, qk_scale: float = 8.0, vo_scale: float = 3.0, mlp_scale: float = 3.0, global_qk: float = 0.6) -> np.ndarray:
    """The fixtures' weight rule: every tensor 0.02 * N(0,1) (the integer-hash generator of the oracle), LayerNorm gamma = 1 + 5x,
    every beta and bias 0 (the family has none), Wq and Wk times qk_scale, Wv and the attention's Wo times vo_scale, Wi and the MLP's
    Wo times mlp_scale -- the scales are stated for hidden 128 and shrink with sqrt(128 / hidden), so that scores and branch sizes stay
    put as the model widens.  Layer 0's attn_norm slot holds a gamma around 2 instead of 1: the model never reads it, a forward that does
    shows.  With plain 0.02 weights the softmax is nearly uniform and the attention branch small next to the residual
    stream: a forward without any window, or with the wrong rotary base, then moves the pooled vector by less than the model's own
    bf16 error (scripts/gen_modernbert_fixtures.py measures both and refuses fixtures that cannot tell)."""
    blob = (np.float32(0.02) * orc.synth(blob_size(cfg), 1, seed).reshape(-1)).astype(np.float32)
    u = unpack(cfg, blob)  # views into blob
    for name, seg in u.items():
        leaf = name.split(".")[-1]
        if leaf.endswith("_g"):
            seg[:] = 1.0 + 5.0 * seg
        elif leaf.endswith("_b") or leaf in ("bq", "bk", "bv", "bo", "b1", "b2"):
            seg[:] = 0.0
    u["l0.ln1_g"][:] += 1.0  # (around 2: see above)
    width = np.sqrt(128.0 / cfg["hidden"])
    qk_scale, vo_scale, mlp_scale = qk_scale * width, vo_scale * width, mlp_scale * width
    for l in range(cfg["layers"]):
        # the global layers' scores are softer by global_qk: a sharp softmax over a thousand keys is where the model's own bf16 forward
        # loses the [CLS] row of a long text, and the window and the local base live in the local layers
        sharp = qk_scale * (global_qk if is_global(cfg, l) else 1.0)
        u[f"l{l}.wq"][:] *= np.float32(sharp)
        u[f"l{l}.wk"][:] *= np.float32(sharp)
        u[f"l{l}.wv"][:] *= np.float32(vo_scale)
        u[f"l{l}.wo"][:] *= np.float32(vo_scale)
        u[f"l{l}.w1"][:] *= np.float32(mlp_scale)
        u[f"l{l}.w2"][:] *= np.float32(mlp_scale)
    return blob


def rope_tables(S: int, theta: float, dh: int = 64):
    f = float(theta) ** (-2.0 * np.arange(dh // 2, dtype=np.float64) / dh)
    ang = np.arange(S, dtype=np.float64)[:, None] * f[None, :]
    return np.cos(ang), np.sin(ang)


def rotate_half(t: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    h = t.shape[-1] // 2
    a, b = t[..., :h], t[..., h:]
    return np.concatenate([a * cos - b * sin, b * cos + a * sin], axis=-1)


def _layernorm(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def _gelu(x):
    from scipy.special import erf

    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def is_global(cfg: dict, l: int) -> bool:
    return l % int(cfg.get("global_every") or 1) == 0


def forward(cfg: dict, blob: np.ndarray, ids: np.ndarray, lens: np.ndarray, pooling: str = "mean", deviate: "str | None" = None) -> np.ndarray:
    """ids [B, S] int, lens [B] -> [B, H] f32: the masked mean of the last hidden state, or (pooling "cls") its first row.
    deviate: one deliberate departure from the model, so that the fixture generator and the tests can show that the fixtures tell
    it apart: "no_window" (every layer attends globally; the bases stay) | "window_m2" (local_window - 2) | "local_base" / "global_base"
    (that rotary base in every layer) | "post_norm" (h = LN(h + sublayer(h))) | "attn_norm0" (layer 0's attn_norm applied) |
    "swap" (the other half of Wi activated)."""
    assert deviate is None or deviate in DEVIATIONS, deviate
    W = {k: v.astype(np.float64) for k, v in unpack(cfg, blob).items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    lens = np.clip(np.asarray(lens), 1, S)
    H, nh, F, eps = cfg["hidden"], cfg["heads"], cfg["ffn"], cfg["ln_eps"]
    dh = H // nh
    th_g, th_l = float(cfg.get("rope_theta") or 10000.0), float(cfg.get("rope_theta_local") or 10000.0)
    if deviate == "local_base":
        th_g = th_l
    if deviate == "global_base":
        th_l = th_g
    half = (int(cfg["local_window"]) - (2 if deviate == "window_m2" else 0)) // 2
    out = np.empty((B, H), np.float64)
    for b in range(B):  # rows at or beyond len never reach a real row (keys masked, everything else is row-wise): leave them out
        n = int(lens[b])
        tabs = {True: rope_tables(n, th_g, dh), False: rope_tables(n, th_l, dh)}
        dist = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
        band = np.where(dist <= half, 0.0, -np.inf)[None]
        h = _layernorm(W["word_emb"][ids[b, :n]], W["emb_ln_g"], W["emb_ln_b"], eps)
        for l in range(cfg["layers"]):
            p = f"l{l}."
            glob = is_global(cfg, l)
            sp = lambda t: t.reshape(n, nh, dh).transpose(1, 0, 2)
            if deviate == "post_norm":
                a = h
            elif l == 0 and deviate != "attn_norm0":
                a = h
            else:
                a = _layernorm(h, W[p + "ln1_g"], W[p + "ln1_b"], eps)
            q, k, v = sp(a @ W[p + "wq"].T + W[p + "bq"]), sp(a @ W[p + "wk"].T + W[p + "bk"]), sp(a @ W[p + "wv"].T + W[p + "bv"])
            cos, sin = tabs[glob]
            q, k = rotate_half(q, cos, sin), rotate_half(k, cos, sin)
            s = q @ k.transpose(0, 2, 1) / np.sqrt(dh)
            if not glob and deviate != "no_window":
                s = s + band
            e = np.exp(s - s.max(-1, keepdims=True))
            ctx = ((e / e.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(n, H)
            h = ctx @ W[p + "wo"].T + W[p + "bo"] + h
            if deviate == "post_norm":
                h = _layernorm(h, W[p + "ln1_g"], W[p + "ln1_b"], eps)
            m = h if deviate == "post_norm" else _layernorm(h, W[p + "ln2_g"], W[p + "ln2_b"], eps)
            u = m @ W[p + "w1"].T + W[p + "b1"]
            gate, up = (u[:, F:], u[:, :F]) if deviate == "swap" else (u[:, :F], u[:, F:])
            h = (_gelu(gate) * up) @ W[p + "w2"].T + W[p + "b2"] + h
            if deviate == "post_norm":
                h = _layernorm(h, W[p + "ln2_g"], W[p + "ln2_b"], eps)
        h = _layernorm(h, W["final_g"], W["final_b"], eps)
        out[b] = h[0] if pooling == "cls" else h.mean(0)
    return out.astype(np.float32)


def hf_config(cfg: dict) -> dict:
    """The config.json of transformers' ModernBertModel for cfg (the keys the loader reads, in the released checkpoints' spelling)."""
    return {"model_type": "modernbert", "vocab_size": cfg["vocab"], "hidden_size": cfg["hidden"], "num_hidden_layers": cfg["layers"],
            "num_attention_heads": cfg["heads"], "intermediate_size": cfg["ffn"], "max_position_embeddings": cfg["max_pos"], "norm_eps": cfg["ln_eps"],
            "local_attention": cfg["local_window"], "global_attn_every_n_layers": cfg["global_every"], "global_rope_theta": float(cfg["rope_theta"]),
            "local_rope_theta": float(cfg["rope_theta_local"]), "norm_bias": False, "attention_bias": False, "mlp_bias": False,
            "hidden_activation": "gelu", "pad_token_id": 0}


def to_hf_state_dict(cfg: dict, blob: np.ndarray) -> dict:
    """Blob -> transformers ModernBertModel state_dict names (numpy arrays): Wqkv = [Wq; Wk; Wv], Wi = W1 (activated half first)."""
    W = unpack(cfg, blob)
    sd = {"embeddings.tok_embeddings.weight": W["word_emb"], "embeddings.norm.weight": W["emb_ln_g"], "final_norm.weight": W["final_g"]}
    for l in range(cfg["layers"]):
        p, q = f"l{l}.", f"layers.{l}."
        if l > 0:
            sd[q + "attn_norm.weight"] = W[p + "ln1_g"]
        sd.update({q + "attn.Wqkv.weight": np.concatenate([W[p + "wq"], W[p + "wk"], W[p + "wv"]], 0), q + "attn.Wo.weight": W[p + "wo"],
                   q + "mlp_norm.weight": W[p + "ln2_g"], q + "mlp.Wi.weight": W[p + "w1"], q + "mlp.Wo.weight": W[p + "w2"]})
    return {k: np.ascontiguousarray(v) for k, v in sd.items()}
