"""CPU restatement (numpy float64) of the Qwen2 forward as an embedding model.  TEST INFRASTRUCTURE ONLY.

Qwen2 / Qwen2.5 (the 0.5B backbone of jina-code-embeddings-0.5b, gte-Qwen2, KaLM-mini) is a PRE-norm CAUSAL decoder:
h = tok_emb[id]; per layer h += Attn(RMS_in(h)), h += MLP(RMS_post(h)); RMS_final before pooling.  No embedding norm, no position and no
type table.  RMS(x) = x * rsqrt(mean(x^2) + eps) * gamma (no beta).  Biases on the q, k, v projections only.  Rotary positions
("rotate-half" pairs (j, j + 32) of a 64-wide head) with one base.  Scores q.k / 8 over the keys j <= i.  Grouped-query attention: query
head h reads K / V head h // (heads // kv_heads).  MLP = down (silu(gate m) * (up m)).  The vector of a text is the row of its last real
token ("last") or the mean over its real tokens ("mean").
Pinned to transformers' Qwen2Model (fp32, eager attention) by tests/golden/qwen2_golden.npz, written by scripts/gen_qwen2_fixtures.py.

Blob layout = arch 2 of include/semcode_hip.h, KV = kv_heads * 64: word_emb, per layer Wq [H,H] bq Wk [KV,H] bk Wv [KV,H] bv Wo bo ln1
(= input_layernorm) W1 (= [gate_proj; up_proj]) b1 W2 (= down_proj) b2 ln2 (= post_attention_layernorm), then final_norm gamma / beta.
Beta slots and the slots of the biases the family lacks (bo, b1, b2) stay, as zeros.
"""
from __future__ import annotations

import numpy as np

from oracle import sc_oracle as orc

DEVIATIONS = ("no_mask", "mask_p1", "kv_interleaved", "layernorm", "base_10000", "k_unrotated", "swap", "emb_ln")


def kv_heads(cfg: dict) -> int:
    return int(cfg.get("kv_heads") or cfg["heads"])


def blob_layout(cfg: dict) -> list:
    H, F, KV = cfg["hidden"], cfg["ffn"], kv_heads(cfg) * 64
    out = [("word_emb", (cfg["vocab"], H))]
    for l in range(cfg["layers"]):
        p = f"l{l}."
        out += [(p + "wq", (H, H)), (p + "bq", (H,)), (p + "wk", (KV, H)), (p + "bk", (KV,)), (p + "wv", (KV, H)), (p + "bv", (KV,)),
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


def make_weights(cfg: dict, seed: int, qk_scale: float = 2.0, bias_sigma: float = 2.0, vo_scale: float = 3.0, mlp_scale: float = 3.0,
                 emb_scale: float = 5.0, norm_sigma: float = 0.3, bias_first: int = 0) -> np.ndarray:
    """The fixtures' weight rule: every tensor 0.02 * N(0,1) (the integer-hash generator of the oracle) = transformers' default
    initialisation, then: Wq and Wk times qk_scale, Wv and Wo times vo_scale, W1 and W2 times mlp_scale (stated for hidden 128, all
    shrinking with sqrt(128 / hidden)), the embedding table times emb_scale, RMSNorm gammas 1 + norm_sigma * N(0,1), the v bias
    0.02 * N(0,1), every beta slot and the bo / b1 / b2 slots zero (the family has none), and the q / k biases as follows.

    A K head and the query heads that read it share ONE bias vector b = bias_sigma on the columns bias_first .. bias_first + 15 of the
    head (sixteen of the fastest rotary pairs; zero elsewhere), the K head's copy turned back by one position.  (bias_first > 0 leaves
    the very fastest pairs out: at position 1 100 their angle is a float32 of 1e-4 resolution, and a large bias there shows in
    transformers' own fp32 forward.)  Rotated by position, the bias term of a
    score is bias_sigma^2 sum_f cos((j - i - 1) theta_f): it peaks at the key ONE AHEAD of the query and falls off within a few
    positions (sixteen equal pairs keep the side lobes of a 2 048-token text at a sixth of the peak).  Under the causal mask a token then attends mostly to itself and its last few predecessors; with the mask one key too
    wide or missing, the favoured key becomes visible and takes the largest share; with another base or an unrotated K the peak
    is gone.  With plain 0.02 weights and independent biases the softmax is nearly uniform and the attention branch a near-constant:
    each of those then moves the last token's vector by less than the model's own bf16 error (scripts/gen_qwen2_fixtures.py measures
    both and refuses fixtures that cannot tell)."""
    unit = orc.synth(blob_size(cfg), 1, seed).reshape(-1).astype(np.float32)  # N(0,1)
    blob = (np.float32(0.02) * unit).astype(np.float32)
    u, n = unpack(cfg, blob), unpack(cfg, unit)  # views
    for name, seg in u.items():
        leaf = name.split(".")[-1]
        if leaf.endswith("_g"):
            seg[:] = 1.0 + np.float32(norm_sigma) * n[name]
        elif leaf.endswith("_b") or leaf in ("bo", "b1", "b2"):
            seg[:] = 0.0
    u["word_emb"][:] *= np.float32(emb_scale)
    nh, nkv = cfg["heads"], kv_heads(cfg)
    width = np.sqrt(128.0 / cfg["hidden"])
    cos1, sin1 = rope_tables(2, float(cfg.get("rope_theta") or 10000.0))
    b = np.where((np.arange(64) >= bias_first) & (np.arange(64) < bias_first + 16), np.float32(bias_sigma), np.float32(0.0)).astype(np.float32)
    for l in range(cfg["layers"]):
        for name, sc in (("wq", qk_scale), ("wk", qk_scale), ("wv", vo_scale), ("wo", vo_scale), ("w1", mlp_scale), ("w2", mlp_scale)):
            u[f"l{l}.{name}"][:] *= np.float32(sc * width)
        bq, bk = u[f"l{l}.bq"].reshape(nh, 64), u[f"l{l}.bk"].reshape(nkv, 64)
        for g in range(nkv):
            bq[g * (nh // nkv):(g + 1) * (nh // nkv)] = b
            bk[g] = rotate_half(b.astype(np.float64), cos1[1], -sin1[1]).astype(np.float32)  # R(-1) b: q_i . k_j peaks at j = i + 1
    return blob


def rope_tables(S: int, theta: float, dh: int = 64):
    f = float(theta) ** (-2.0 * np.arange(dh // 2, dtype=np.float64) / dh)
    ang = np.arange(S, dtype=np.float64)[:, None] * f[None, :]
    return np.cos(ang), np.sin(ang)


def rotate_half(t: np.ndarray, cos: np.ndarray, sin: np.ndarray) -> np.ndarray:
    h = t.shape[-1] // 2
    a, b = t[..., :h], t[..., h:]
    return np.concatenate([a * cos - b * sin, b * cos + a * sin], axis=-1)


def _rms(x, g, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * g


def _layernorm(x, g, eps):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps) * g


def _silu(x):
    return x / (1.0 + np.exp(-x))


def forward(cfg: dict, blob: np.ndarray, ids: np.ndarray, lens: np.ndarray, pooling: str = "last", deviate: "str | None" = None) -> np.ndarray:
    """ids [B, S] int, lens [B] -> [B, H] f32: RMS_final of the last real token's row ("last") or its mean over the real tokens ("mean").
    deviate: one deliberate departure from the model, so that the fixture generator and the tests can show that the fixtures tell it
    apart: "no_mask" (every token sees every real key) | "mask_p1" (the mask one key too wide: j <= i + 1) | "kv_interleaved" (query head
    h reads K / V head h % kv_heads) | "layernorm" (LayerNorm statistics instead of RMS) | "base_10000" (that rotary base instead of the
    model's) | "k_unrotated" | "swap" (the other half of W1 activated) | "emb_ln" (a LayerNorm applied to the embeddings)."""
    assert deviate is None or deviate in DEVIATIONS, deviate
    assert pooling in ("last", "mean"), pooling
    W = {k: v.astype(np.float64) for k, v in unpack(cfg, blob).items()}
    ids = np.asarray(ids)
    B, S = ids.shape
    lens = np.clip(np.asarray(lens), 1, S)
    H, nh, nkv, F, eps = cfg["hidden"], cfg["heads"], kv_heads(cfg), cfg["ffn"], cfg["ln_eps"]
    dh = H // nh
    theta = 10000.0 if deviate == "base_10000" else float(cfg.get("rope_theta") or 10000.0)
    norm = _layernorm if deviate == "layernorm" else _rms
    group = nh // nkv
    kv_of = [(h % nkv) if deviate == "kv_interleaved" else (h // group) for h in range(nh)]
    out = np.empty((B, H), np.float64)
    for b in range(B):  # rows at or beyond len never reach a real row (a real query's keys are real): leave them out
        n = int(lens[b])
        cos, sin = rope_tables(n, theta, dh)
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        if deviate == "no_mask":
            mask = np.zeros((n, n))
        else:
            mask = np.where(j <= i + (1 if deviate == "mask_p1" else 0), 0.0, -np.inf)
        h = W["word_emb"][ids[b, :n]]
        if deviate == "emb_ln":
            h = _layernorm(h, 1.0, eps)
        for l in range(cfg["layers"]):
            p = f"l{l}."
            a = norm(h, W[p + "ln1_g"], eps)
            q = (a @ W[p + "wq"].T + W[p + "bq"]).reshape(n, nh, dh).transpose(1, 0, 2)
            k = (a @ W[p + "wk"].T + W[p + "bk"]).reshape(n, nkv, dh).transpose(1, 0, 2)
            v = (a @ W[p + "wv"].T + W[p + "bv"]).reshape(n, nkv, dh).transpose(1, 0, 2)
            q = rotate_half(q, cos, sin)
            if deviate != "k_unrotated":
                k = rotate_half(k, cos, sin)
            k, v = k[kv_of], v[kv_of]
            s = q @ k.transpose(0, 2, 1) / np.sqrt(dh) + mask[None]
            e = np.exp(s - s.max(-1, keepdims=True))
            ctx = ((e / e.sum(-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(n, H)
            h = ctx @ W[p + "wo"].T + W[p + "bo"] + h
            m = norm(h, W[p + "ln2_g"], eps)
            u = m @ W[p + "w1"].T + W[p + "b1"]
            gate, up = (u[:, F:], u[:, :F]) if deviate == "swap" else (u[:, :F], u[:, F:])
            h = (_silu(gate) * up) @ W[p + "w2"].T + W[p + "b2"] + h
        h = norm(h, W["final_g"], eps)
        out[b] = h[n - 1] if pooling == "last" else h.mean(0)
    return out.astype(np.float32)


def hf_config(cfg: dict) -> dict:
    """The config.json of transformers' Qwen2Model for cfg (the keys the loader reads, in the released checkpoints' spelling)."""
    return {"model_type": "qwen2", "vocab_size": cfg["vocab"], "hidden_size": cfg["hidden"], "num_hidden_layers": cfg["layers"],
            "num_attention_heads": cfg["heads"], "num_key_value_heads": kv_heads(cfg), "intermediate_size": cfg["ffn"],
            "max_position_embeddings": cfg["max_pos"], "rms_norm_eps": cfg["ln_eps"], "rope_theta": float(cfg.get("rope_theta") or 10000.0),
            "hidden_act": "silu", "use_sliding_window": False, "tie_word_embeddings": True, "attention_dropout": 0.0}


def to_hf_state_dict(cfg: dict, blob: np.ndarray, prefix: str = "") -> dict:
    """Blob -> transformers Qwen2Model state_dict names (numpy arrays); prefix "model." gives the names of a Qwen2ForCausalLM file."""
    W = unpack(cfg, blob)
    F = cfg["ffn"]
    sd = {"embed_tokens.weight": W["word_emb"], "norm.weight": W["final_g"]}
    for l in range(cfg["layers"]):
        p, q = f"l{l}.", f"layers.{l}."
        sd.update({q + "self_attn.q_proj.weight": W[p + "wq"], q + "self_attn.q_proj.bias": W[p + "bq"],
                   q + "self_attn.k_proj.weight": W[p + "wk"], q + "self_attn.k_proj.bias": W[p + "bk"],
                   q + "self_attn.v_proj.weight": W[p + "wv"], q + "self_attn.v_proj.bias": W[p + "bv"],
                   q + "self_attn.o_proj.weight": W[p + "wo"], q + "input_layernorm.weight": W[p + "ln1_g"],
                   q + "post_attention_layernorm.weight": W[p + "ln2_g"], q + "mlp.gate_proj.weight": W[p + "w1"][:F],
                   q + "mlp.up_proj.weight": W[p + "w1"][F:], q + "mlp.down_proj.weight": W[p + "w2"]})
    return {prefix + k: np.ascontiguousarray(v) for k, v in sd.items()}
