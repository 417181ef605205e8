"""CPU restatement (numpy float64) of the causal decoder forward at a STATED head dimension, with or without QK-norm: Qwen3-Embedding
(heads of 128, a per-head RMSNorm on Q and on K before the rotation, no q / k / v bias, attention width heads * 128 that need not equal
hidden) and Qwen2.5-1.5B (heads of 128, biases, no QK-norm).  TEST INFRASTRUCTURE ONLY.

The model is tests/qwen2_ref's with three changes: q = a Wq^T (+ bq) has AW = heads * head_dim columns and o_proj is [H, AW]; with
cfg["qk_norm"], q and k become x * rsqrt(mean(x^2) + eps) * gamma over each head's head_dim values (gamma_q / gamma_k [head_dim] per
layer) BEFORE the rotation; the rotation pairs (j, j + head_dim / 2) with the angle p * theta^(-2j / head_dim) and the scores are
q.k / sqrt(head_dim).
Pinned to transformers' Qwen3Model (qk_norm) and Qwen2Model (biases) -- fp32, eager attention -- by tests/golden/qwen3_golden.npz, written
by scripts/gen_qwen3_fixtures.py.

Blob layout = arch 2 of include/semcode_hip.h with head_dim stated, AW = heads * head_dim, KV = kv_heads * head_dim: word_emb, per layer
Wq [AW,H] bq [AW] Wk [KV,H] bk [KV] Wv [KV,H] bv [KV] Wo [H,AW] bo ln1 W1 b1 W2 b2 ln2 (gamma, beta), then with qk_norm q_norm_gamma
[head_dim], k_norm_gamma [head_dim]; at the end final_norm gamma / beta.
"""
from __future__ import annotations

import numpy as np

from oracle import sc_oracle as orc
from qwen2_ref import _rms, _silu, rope_tables, rotate_half

DEVIATIONS = ("no_qk_norm", "norm_after_rope", "gammas_swapped", "norm_whole_row", "pairs_in_halves", "scale_64", "halves_swapped",
              "kv_interleaved", "no_mask", "mask_p1")
NORM_DEVIATIONS = DEVIATIONS[:4]  # exist with qk_norm only


def kv_heads(cfg: dict) -> int:
    return int(cfg.get("kv_heads") or cfg["heads"])


def head_dim(cfg: dict) -> int:
    return int(cfg.get("head_dim") or 64)


def applicable(cfg: dict, dev: str) -> bool:
    """Whether a deviation differs from the model at all for cfg."""
    if dev in NORM_DEVIATIONS:
        return bool(cfg.get("qk_norm"))
    if dev == "kv_interleaved":
        return kv_heads(cfg) not in (1, cfg["heads"])
    return True


def blob_layout(cfg: dict) -> list:
    H, F, hd = cfg["hidden"], cfg["ffn"], head_dim(cfg)
    AW, KV = cfg["heads"] * hd, kv_heads(cfg) * hd
    out = [("word_emb", (cfg["vocab"], H))]
    for l in range(cfg["layers"]):
        p = f"l{l}."
        out += [(p + "wq", (AW, H)), (p + "bq", (AW,)), (p + "wk", (KV, H)), (p + "bk", (KV,)), (p + "wv", (KV, H)), (p + "bv", (KV,)),
                (p + "wo", (H, AW)), (p + "bo", (H,)), (p + "ln1_g", (H,)), (p + "ln1_b", (H,)),
                (p + "w1", (2 * F, H)), (p + "b1", (2 * F,)), (p + "w2", (H, F)), (p + "b2", (H,)), (p + "ln2_g", (H,)), (p + "ln2_b", (H,))]
        if cfg.get("qk_norm"):
            out += [(p + "qn_g", (hd,)), (p + "kn_g", (hd,))]
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


def make_weights(cfg: dict, seed: int, qk_scale: float = 1.0, bias_sigma: float = 2.0, vo_scale: float = 3.0, mlp_scale: float = 3.0,
                 emb_scale: float = 5.0, norm_sigma: float = 0.3, bias_first: int = 0, qk_gamma: float = 1.0) -> np.ndarray:
    """The fixtures' weight rule, tests/qwen2_ref.make_weights restated for a stated head width: every tensor 0.02 * N(0,1), Wq / Wk times
    qk_scale, Wv / Wo times vo_scale, W1 / W2 times mlp_scale (all shrinking with sqrt(128 / hidden)), the embedding table times emb_scale,
    RMSNorm gammas 1 + norm_sigma * N(0,1), beta slots and bo / b1 / b2 zero.

    The structure that makes the causal mask visible at the last token is qwen2_ref's: a K head and the query heads that read it share ONE
    vector b = bias_sigma on the columns bias_first .. bias_first + 15 of the head (sixteen of the fastest rotary pairs), the K head's copy
    turned back by one position, so that q_i . k_j peaks at the key ONE AHEAD of the query.
      without qk_norm (Qwen2.5-1.5B: biases): b is the q / k bias, as there; the v bias is 0.02 * N(0,1).
      with qk_norm (Qwen3: no q / k / v bias): the same b rides on ONE embedding direction.  Column 0 of the embedding table is the constant
        1 for every token, and row 0 of every Wo and W2 is zero, so h[:, 0] = 1 in every layer and a = RMS_in(h) has a[:, 0] =
        gamma_in[0] / rms(h) > 0 (gamma_in[0] is set to 1).  Column 0 of Wq holds b and of Wk R(-1) b, the latter divided elementwise
        by k_norm's gamma, the former by q_norm's: after the per-head norm -- which removes the token's 1 / rms(h) -- and its gamma the
        structured part of q is c_q b and of k c_k R(-1) b with scalars c, the rotation-friendly form again.  The q / k norm gammas are
        qk_gamma * (1 + norm_sigma * N(0,1)), clipped to at least 0.3 * qk_gamma: they vary across the pair dimension (a norm with a
        constant gamma commutes with the rotation: norm_after_rope would be invisible), and qk_gamma sets the softmax's sharpness.
        Head h of Wq and of Wk is scaled by 1 + h % 4: the per-head norm removes that, one norm over the whole row does not."""
    unit = orc.synth(blob_size(cfg), 1, seed).reshape(-1).astype(np.float32)  # N(0,1)
    blob = (np.float32(0.02) * unit).astype(np.float32)
    u, n = unpack(cfg, blob), unpack(cfg, unit)  # views
    hd, qkn = head_dim(cfg), bool(cfg.get("qk_norm"))
    for name, seg in u.items():
        leaf = name.split(".")[-1]
        if leaf in ("qn_g", "kn_g"):
            seg[:] = np.float32(qk_gamma) * np.maximum(1.0 + np.float32(norm_sigma) * n[name], np.float32(0.3))
        elif leaf.endswith("_g"):
            seg[:] = 1.0 + np.float32(norm_sigma) * n[name]
        elif leaf.endswith("_b") or leaf in ("bo", "b1", "b2") or (qkn and leaf in ("bq", "bk", "bv")):
            seg[:] = 0.0
    u["word_emb"][:] *= np.float32(emb_scale)
    nh, nkv = cfg["heads"], kv_heads(cfg)
    width = np.sqrt(128.0 / cfg["hidden"])
    cos1, sin1 = rope_tables(2, float(cfg.get("rope_theta") or 10000.0), hd)
    b = np.where((np.arange(hd) >= bias_first) & (np.arange(hd) < bias_first + 16), np.float32(bias_sigma), np.float32(0.0)).astype(np.float32)
    bk_vec = rotate_half(b.astype(np.float64), cos1[1], -sin1[1]).astype(np.float32)  # R(-1) b: q_i . k_j peaks at j = i + 1
    if qkn:
        u["word_emb"][:, 0] = 1.0
    for l in range(cfg["layers"]):
        for name, sc in (("wq", qk_scale), ("wk", qk_scale), ("wv", vo_scale), ("wo", vo_scale), ("w1", mlp_scale), ("w2", mlp_scale)):
            u[f"l{l}.{name}"][:] *= np.float32(sc * width)
        if qkn:
            u[f"l{l}.wo"][0, :] = 0.0
            u[f"l{l}.w2"][0, :] = 0.0
            u[f"l{l}.ln1_g"][0] = 1.0
            wq, wk = u[f"l{l}.wq"].reshape(nh, hd, -1), u[f"l{l}.wk"].reshape(nkv, hd, -1)
            wq[:, :, 0] = b / u[f"l{l}.qn_g"]
            wk[:, :, 0] = bk_vec / u[f"l{l}.kn_g"]
            wq *= (1.0 + np.arange(nh) % 4).astype(np.float32)[:, None, None]  # heads of different length: one norm over the whole row
            wk *= (1.0 + np.arange(nkv) % 4).astype(np.float32)[:, None, None]  # (norm_whole_row) is not the norm per head
        else:
            bq, bk = u[f"l{l}.bq"].reshape(nh, hd), u[f"l{l}.bk"].reshape(nkv, hd)
            bq[:] = b
            bk[:] = bk_vec
    return blob


def _swap_halves(t, hd):
    return np.concatenate([t[..., hd // 2:], t[..., :hd // 2]], axis=-1)


def _rope_in_halves(t, cos, sin, hd):
    """the 64-wide kernels' pairing inside each 64-column half of a 128-wide head: pairs (j, j + 32), the angle of pair index j of a head
    of 64 -- what rope_qk_kernel would do to the head's two blocks"""
    q = hd // 4
    lo, hi = t[..., :hd // 2], t[..., hd // 2:]
    return np.concatenate([rotate_half(lo, cos[..., :q], sin[..., :q]), rotate_half(hi, cos[..., :q], sin[..., :q])], axis=-1)


def forward(cfg: dict, blob: np.ndarray, ids: np.ndarray, lens: np.ndarray, pooling: str = "last", deviate: "str | None" = None) -> np.ndarray:
    """ids [B, S] int, lens [B] -> [B, H] f32: RMS_final of the last real token's row ("last") or its mean over the real tokens ("mean").
    deviate: one deliberate departure from the model:
      "no_qk_norm" | "norm_after_rope" (the per-head norm applied to the rotated q, k) | "gammas_swapped" (q gets k_norm's gamma and k
      q_norm's) | "norm_whole_row" (one RMS over all heads of the row instead of one per head) | "pairs_in_halves" (rotary pairs (j, j + 32)
      inside each 64-column half, with a 64-wide head's angles, instead of (j, j + 64)) | "scale_64" (scores / 8) | "halves_swapped" (the
      two 64-column halves of every q and k head exchanged before the rotation) | "kv_interleaved" (query head h reads K / V head
      h % kv_heads) | "no_mask" | "mask_p1" (the mask one key too wide)."""
    assert deviate is None or deviate in DEVIATIONS, deviate
    assert pooling in ("last", "mean"), pooling
    W = {k: v.astype(np.float64) for k, v in unpack(cfg, blob).items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    lens = np.clip(np.asarray(lens), 1, S)
    H, nh, nkv, F, eps, hd = cfg["hidden"], cfg["heads"], kv_heads(cfg), cfg["ffn"], cfg["ln_eps"], head_dim(cfg)
    AW = nh * hd
    qkn = bool(cfg.get("qk_norm")) and deviate != "no_qk_norm"
    theta = float(cfg.get("rope_theta") or 10000.0)
    group = nh // nkv
    kv_of = [(h % nkv) if deviate == "kv_interleaved" else (h // group) for h in range(nh)]
    out = np.empty((B, H), np.float64)

    def head_norm(t, g):  # t [heads, n, hd]
        if deviate == "norm_whole_row":
            return t / np.sqrt((t * t).mean(axis=(0, 2), keepdims=True) + eps) * g
        return _rms(t, g, eps)

    for b in range(B):
        n = int(lens[b])
        if deviate == "pairs_in_halves":
            cos, sin = rope_tables(n, theta, hd // 2)
            rot = lambda t: _rope_in_halves(t, cos, sin, hd)  # noqa: E731
        else:
            cos, sin = rope_tables(n, theta, hd)
            rot = lambda t: rotate_half(t, cos, sin)  # noqa: E731
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        mask = np.zeros((n, n)) if deviate == "no_mask" else np.where(j <= i + (1 if deviate == "mask_p1" else 0), 0.0, -np.inf)
        h = W["word_emb"][ids[b, :n]]
        for l in range(cfg["layers"]):
            p = f"l{l}."
            a = _rms(h, W[p + "ln1_g"], eps)
            q = (a @ W[p + "wq"].T + W[p + "bq"]).reshape(n, nh, hd).transpose(1, 0, 2)
            k = (a @ W[p + "wk"].T + W[p + "bk"]).reshape(n, nkv, hd).transpose(1, 0, 2)
            v = (a @ W[p + "wv"].T + W[p + "bv"]).reshape(n, nkv, hd).transpose(1, 0, 2)
            if deviate == "halves_swapped":
                q, k = _swap_halves(q, hd), _swap_halves(k, hd)
            if qkn:
                gq, gk = (W[p + "kn_g"], W[p + "qn_g"]) if deviate == "gammas_swapped" else (W[p + "qn_g"], W[p + "kn_g"])
                if deviate == "norm_after_rope":
                    q, k = head_norm(rot(q), gq), head_norm(rot(k), gk)
                else:
                    q, k = rot(head_norm(q, gq)), rot(head_norm(k, gk))
            else:
                q, k = rot(q), rot(k)
            k, v = k[kv_of], v[kv_of]
            s = q @ k.transpose(0, 2, 1) / (8.0 if deviate == "scale_64" else np.sqrt(hd)) + mask[None]
            e = np.exp(s - s.max(-1, keepdims=True))
            ctx = ((e / e.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(n, AW)
            h = ctx @ W[p + "wo"].T + W[p + "bo"] + h
            m = _rms(h, W[p + "ln2_g"], eps)
            u = m @ W[p + "w1"].T + W[p + "b1"]
            h = (_silu(u[:, :F]) * u[:, F:]) @ W[p + "w2"].T + W[p + "b2"] + h
        h = _rms(h, W["final_g"], eps)
        out[b] = h[n - 1] if pooling == "last" else h.mean(0)
    return out.astype(np.float32)


def hf_config(cfg: dict) -> dict:
    """The config.json of transformers' Qwen3Model (qk_norm) or Qwen2Model for cfg, in the released checkpoints' spelling.  Qwen2Model
    derives its head width from hidden_size / num_attention_heads: such a cfg must have hidden == heads * head_dim."""
    hd = head_dim(cfg)
    out = {"model_type": "qwen3" if cfg.get("qk_norm") else "qwen2", "vocab_size": cfg["vocab"], "hidden_size": cfg["hidden"],
           "num_hidden_layers": cfg["layers"], "num_attention_heads": cfg["heads"], "num_key_value_heads": kv_heads(cfg),
           "intermediate_size": cfg["ffn"], "max_position_embeddings": cfg["max_pos"], "rms_norm_eps": cfg["ln_eps"],
           "rope_theta": float(cfg.get("rope_theta") or 10000.0), "hidden_act": "silu", "use_sliding_window": False, "tie_word_embeddings": True,
           "attention_dropout": 0.0}
    if cfg.get("qk_norm"):
        out.update(head_dim=hd, attention_bias=False)
    else:
        assert cfg["hidden"] == cfg["heads"] * hd, "Qwen2Model has no head_dim of its own"
    return out


def to_hf_state_dict(cfg: dict, blob: np.ndarray, prefix: str = "") -> dict:
    """Blob -> transformers Qwen3Model / Qwen2Model state_dict names (numpy arrays); Qwen3 has no q / k / v bias tensors."""
    W = unpack(cfg, blob)
    F = cfg["ffn"]
    sd = {"embed_tokens.weight": W["word_emb"], "norm.weight": W["final_g"]}
    for l in range(cfg["layers"]):
        p, q = f"l{l}.", f"layers.{l}."
        sd.update({q + "self_attn.q_proj.weight": W[p + "wq"], q + "self_attn.k_proj.weight": W[p + "wk"], q + "self_attn.v_proj.weight": W[p + "wv"],
                   q + "self_attn.o_proj.weight": W[p + "wo"], q + "input_layernorm.weight": W[p + "ln1_g"],
                   q + "post_attention_layernorm.weight": W[p + "ln2_g"], q + "mlp.gate_proj.weight": W[p + "w1"][:F],
                   q + "mlp.up_proj.weight": W[p + "w1"][F:], q + "mlp.down_proj.weight": W[p + "w2"]})
        if cfg.get("qk_norm"):
            sd.update({q + "self_attn.q_norm.weight": W[p + "qn_g"], q + "self_attn.k_norm.weight": W[p + "kn_g"]})
        else:
            sd.update({q + "self_attn.q_proj.bias": W[p + "bq"], q + "self_attn.k_proj.bias": W[p + "bk"], q + "self_attn.v_proj.bias": W[p + "bv"]})
    return {prefix + k: np.ascontiguousarray(v) for k, v in sd.items()}
