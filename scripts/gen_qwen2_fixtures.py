"""Writes tests/golden/qwen2_golden.{npz,json}: last-token and mean-pooled vectors of transformers' Qwen2Model (fp32, eager attention,
CPU) for seeded weights.  Run by hand (CPU, a few minutes); no test runs it.

The files hold ids, lens, the two vectors per text, cfg, seed, the weight rule and the tolerances -- not the weights: tests regenerate
them with tests/qwen2_ref.make_weights(cfg, seed, qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma, bias_first).

T per case and pooling = 2 x max|vector_bf16 - vector_fp32| over the texts of the case, transformers' own bf16 forward of that model
against its fp32 forward (T_last, T_mean): the rule of the other golden files, measured against the reference, never against the code
under test.  Users add the floor cos >= 0.999.

Before writing, the generator checks in every case that
  (i)   tests/qwen2_ref.forward lands within 1e-5 of transformers, both poolings,
  (ii)  the model's own bf16 forward keeps cos >= 0.99975 for both poolings (an error twice that size then still keeps 0.999: 1 - cos
        grows with the square of the error), and
  (iii) each of eight mix-ups -- no causal mask, the mask one key too wide, interleaved K/V head mapping, LayerNorm statistics instead
        of RMS, rotary base 10 000, K left unrotated, gate halves swapped, an embedding LayerNorm -- puts the LAST-token vector of EVERY
        text longer than 32 tokens outside (T_last, cos >= 0.999); the K/V mix-up is skipped where kv_heads is 1 or equals heads (there
        the two mappings coincide),
and refuses to write otherwise: fixtures that cannot tell those apart pin nothing.  The weight scales are not constants: with
default-initialised weights the 896-wide shape misses (ii) at some scales and holds it at others, so each case takes the first entry of
SCALES that passes (i) - (iii), and the files record which.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import qwen2_ref as qr  # noqa: E402

# (qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma, bias_first), tried in this order
SCALES = [(2.0, 2.0, 3.0, 3.0, 5.0, 0.3, 0), (2.0, 1.7, 3.0, 3.0, 5.0, 0.3, 0), (1.0, 2.0, 4.0, 3.0, 5.0, 0.3, 0),
          # texts beyond a thousand tokens: without the fastest pairs, or transformers' fp32 forward itself leaves (i)
          (1.0, 2.5, 2.0, 3.0, 5.0, 0.3, 5), (1.0, 2.6, 1.7, 3.0, 5.0, 0.3, 5), (1.0, 2.4, 2.0, 3.0, 5.0, 0.3, 5), (1.0, 2.7, 1.5, 3.0, 5.0, 0.3, 5)]
COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0)
SHAPES = {"s128": dict(hidden=128, heads=2, kv_heads=1, ffn=256), "s128_mha": dict(hidden=128, heads=2, kv_heads=2, ffn=256),
          "s256": dict(hidden=256, heads=4, kv_heads=2, ffn=512), "s256_mqa": dict(hidden=256, heads=4, kv_heads=1, ffn=512),
          "s896": dict(hidden=896, heads=14, kv_heads=2, ffn=4864)}
# name: (shape, layers, S, lens, seed)
CASES = {
    "g2_s64": ("s128", 3, 64, [64, 33, 32, 1], 21),
    "mha_s128": ("s128_mha", 2, 128, [128, 65], 22),
    "g2_s256": ("s256", 2, 256, [256, 129, 65], 23),
    "mqa_s128": ("s256_mqa", 2, 128, [128, 31], 24),
    "g2_s1024": ("s128", 2, 1024, [600, 513], 25),
    "g2_s2048": ("s128", 2, 2048, [1100], 26),
    "half_b": ("s896", 2, 128, [128, 70], 27),
}
BF16_COS, COS_FLOOR = 0.99975, 0.999


def miss(got, want):
    """per text: (max|d|, cos)"""
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


def transformers_vectors(cfg, blob, ids, lens, dtype="float32"):
    import torch
    from transformers import Qwen2Config, Qwen2Model

    hc = Qwen2Config(**{k: v for k, v in qr.hf_config(cfg).items() if k != "model_type"})
    hc._attn_implementation = "eager"
    model = Qwen2Model(hc).eval()
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in qr.to_hf_state_dict(cfg, blob).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if dtype == "bfloat16":
        model = model.to(torch.bfloat16)
    S = ids.shape[1]
    mask = np.arange(S)[None, :] < lens[:, None]
    last = np.empty((len(lens), cfg["hidden"]), np.float32)
    mean = np.empty_like(last)
    with torch.no_grad():
        for b in range(len(lens)):  # one text at a time keeps the S = 2048 score tensors small
            h = model(input_ids=torch.from_numpy(ids[b:b + 1].astype(np.int64)), attention_mask=torch.from_numpy(mask[b:b + 1].astype(np.int64))).last_hidden_state
            last[b] = h[0, lens[b] - 1].float().numpy()
            mean[b] = h[0, : lens[b]].double().mean(0).float().numpy()
    return last, mean


def try_scales(name, cfg, seed, ids, lens, scales):
    """One case at one entry of SCALES: transformers fp32 and bf16, the restatement, the eight mix-ups.  -> (ok, arrays, meta)"""
    blob = qr.make_weights(cfg, seed, *scales)
    want, want_mean = transformers_vectors(cfg, blob, ids, lens)
    low, low_mean = transformers_vectors(cfg, blob, ids, lens, "bfloat16")
    T_last, T_mean = 2.0 * float(np.abs(low - want).max()), 2.0 * float(np.abs(low_mean - want_mean).max())
    bcos = float(min(miss(low, want)[1].min(), miss(low_mean, want_mean)[1].min()))
    d = max(float(np.abs(qr.forward(cfg, blob, ids, lens, "last") - want).max()), float(np.abs(qr.forward(cfg, blob, ids, lens, "mean") - want_mean).max()))
    print(f"{name} (seed {seed}) scales {scales}: qwen2_ref vs transformers max|d| = {d:.2e}; T_last = {T_last:.4f}, T_mean = {T_mean:.4f}, bf16 cos >= {bcos:.5f}", flush=True)
    ok = d <= 1e-5 and bcos >= BF16_COS
    if not ok:
        return False, None, None
    long_ = lens > 32
    dev_miss = {}
    for dev in qr.DEVIATIONS:
        if dev == "kv_interleaved" and qr.kv_heads(cfg) in (1, cfg["heads"]):
            continue
        dd, cos = miss(qr.forward(cfg, blob, ids, lens, "last", deviate=dev), want)
        outside = (dd > T_last) | (cos < COS_FLOOR)
        good = bool(outside[long_].all())
        dev_miss[dev] = float(dd[long_].min()) if long_.any() else None
        print(f"  {dev:14s} max|d| per text = {np.array2string(dd, precision=4)}  {'outside' if good else 'INSIDE the tolerance'}", flush=True)
        ok &= good
    arrays = {f"{name}_ids": ids.astype(np.int16), f"{name}_lens": lens, f"{name}_last": want, f"{name}_mean": want_mean}
    meta = dict(cfg=cfg, seed=seed, S=int(ids.shape[1]), qk_scale=scales[0], bias_sigma=scales[1], vo_scale=scales[2], mlp_scale=scales[3], emb_scale=scales[4], norm_sigma=scales[5], bias_first=scales[6], T_last=T_last,
                T_mean=T_mean, bf16_cos=bcos, deviation_min_miss=dev_miss, weights="tests/qwen2_ref.make_weights(cfg, seed, qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma, bias_first)")
    return ok, arrays, meta


def run_case(name, data, meta) -> bool:
    shape, layers, S, lens, seed = CASES[name]
    cfg = dict(COMMON, **SHAPES[shape], layers=layers)
    rng = np.random.default_rng(3000 + seed)
    lens = np.asarray(lens, np.int32)
    ids = rng.integers(1, cfg["vocab"], size=(len(lens), S)).astype(np.int32)
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0  # padding (never read by a real row)
    for scales in SCALES:
        ok, arrays, m = try_scales(name, cfg, seed, ids, lens, scales)
        if ok:
            data.update(arrays)
            meta[name] = m
            return True
    print(f"{name}: no entry of SCALES passes the checks")
    return False


def main() -> int:
    data, meta, ok = {}, {}, True
    only = sys.argv[1:]  # (trying a case: a partial run never writes)
    for name in CASES:
        if not only or name in only:
            ok &= run_case(name, data, meta)
    if not ok or only:
        print("REFUSED: a check failed (or a partial run), nothing written")
        return 1
    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "qwen2_golden.npz", **data)
    (out / "qwen2_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "qwen2_golden.npz", (out / "qwen2_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
