"""Writes tests/golden/modernbert_golden.{npz,json}: mean-pooled and [CLS] vectors of transformers' ModernBertModel (fp32, eager
attention, CPU) for seeded weights.  Run by hand (CPU, several minutes); no test runs it.

The files hold ids, lens, the two vectors per text, cfg, seed, the weight rule and the tolerance -- not the weights: tests regenerate
them with tests/modernbert_ref.make_weights(cfg, seed, qk_scale, vo_scale, mlp_scale, global_qk).  One case also carries the vectors of the same weights
with EVERY layer global (global_every = 1), for the test that an encoder created that way does not window; those come from
tests/modernbert_ref.forward, which (i) below has just pinned: transformers cannot build a ModernBertConfig without a sliding layer.

T per case = 2 x max|vector_bf16 - vector_fp32| over the texts of the case, transformers' own bf16 forward of that model against its
fp32 forward (T for the mean, T_cls for [CLS]): the rule of minilm_golden.json and cls_golden.json, measured against the reference,
never against the code under test.  Users add the floor cos >= 0.999.

Before writing, the generator checks in every case that
  (i)  tests/modernbert_ref.forward lands within 1e-5 of transformers, both poolings, and
  (ii) each of seven mix-ups -- no window, window off by one (local_window - 2), the local rotary base everywhere, the global base
       everywhere, post-norm instead of pre-norm, attn_norm applied in layer 0, gate halves swapped -- puts the mean-pooled vector
       of EVERY text longer than the window outside (T, cos >= 0.999),
and refuses to write otherwise: fixtures that cannot tell those apart pin nothing.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import modernbert_ref as mr  # noqa: E402

QK_SCALE, VO_SCALE, MLP_SCALE, GLOBAL_QK = 8.0, 3.0, 3.0, 0.6
COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True, rope_theta=160000.0, rope_theta_local=10000.0)
SHAPES = {"s128": dict(hidden=128, heads=2, ffn=256), "s256": dict(hidden=256, heads=4, ffn=512), "s768": dict(hidden=768, heads=12, ffn=1152)}
# name: (shape, layers, global_every, local_window, S, lens, seed)
CASES = {
    "w128": ("s128", 4, 3, 128, 512, [300, 200, 257], 11),
    "w128_short": ("s128", 4, 3, 128, 128, [128, 70, 3], 18),
    "w32": ("s128", 4, 3, 32, 1024, [600, 513, 300], 12),
    "w32_s128": ("s128", 4, 3, 32, 128, [128, 66, 65, 33], 19),
    "w16_s64": ("s256", 4, 3, 16, 64, [64, 33, 17, 3], 13),
    "w32_l7": ("s128", 7, 3, 32, 256, [256, 129, 66], 14),
    "w128_ge2": ("s256", 4, 2, 128, 2048, [1100, 600], 15),
    "base_w128": ("s768", 4, 3, 128, 512, [300, 200], 16),
    "w32_s32": ("s128", 4, 3, 32, 32, [32, 3], 17),
}
GE1_CASE = "w32"  # also stored with every layer global


def miss(got, want):
    """per text: (max|d|, cos)"""
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


def transformers_vectors(cfg, blob, ids, lens, dtype="float32"):
    import torch
    from transformers import ModernBertConfig, ModernBertModel

    hc = ModernBertConfig(**{k: v for k, v in mr.hf_config(cfg).items() if k != "model_type"})
    hc._attn_implementation = "eager"
    model = ModernBertModel(hc).eval()
    missing = model.load_state_dict({k: torch.from_numpy(v) for k, v in mr.to_hf_state_dict(cfg, blob).items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    if dtype == "bfloat16":
        model = model.to(torch.bfloat16)
    S = ids.shape[1]
    mask = np.arange(S)[None, :] < lens[:, None]
    mean = np.empty((len(lens), cfg["hidden"]), np.float32)
    cls = np.empty_like(mean)
    with torch.no_grad():
        for b in range(len(lens)):  # one text at a time keeps the S = 2048 score tensors small
            h = model(input_ids=torch.from_numpy(ids[b:b + 1].astype(np.int64)), attention_mask=torch.from_numpy(mask[b:b + 1].astype(np.int64))).last_hidden_state
            mean[b] = h[0, : lens[b]].double().mean(0).float().numpy()
            cls[b] = h[0, 0].float().numpy()
    return mean, cls


def run_case(name, seed, data, meta) -> bool:
    """One case: transformers fp32 and bf16, the restatement, the seven mix-ups.  Fills data / meta; False = a check failed."""
    shape, layers, ge, lw, S, lens, _ = CASES[name]
    ok = True
    cfg = dict(COMMON, **SHAPES[shape], layers=layers, global_every=ge, local_window=lw)
    blob = mr.make_weights(cfg, seed, QK_SCALE, VO_SCALE, MLP_SCALE, GLOBAL_QK)
    rng = np.random.default_rng(2000 + seed)
    lens = np.asarray(lens, np.int32)
    ids = rng.integers(1, cfg["vocab"], size=(len(lens), S)).astype(np.int32)
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0  # padding: the pad token (never read by a real row)
    want, want_cls = transformers_vectors(cfg, blob, ids, lens)
    low, low_cls = transformers_vectors(cfg, blob, ids, lens, "bfloat16")
    T, T_cls = 2.0 * float(np.abs(low - want).max()), 2.0 * float(np.abs(low_cls - want_cls).max())
    bcos = float(min(miss(low, want)[1].min(), miss(low_cls, want_cls)[1].min()))
    d = max(float(np.abs(mr.forward(cfg, blob, ids, lens) - want).max()), float(np.abs(mr.forward(cfg, blob, ids, lens, "cls") - want_cls).max()))
    print(f"{name} (seed {seed}): modernbert_ref vs transformers max|d| = {d:.2e}; T = {T:.4f}, T_cls = {T_cls:.4f}, bf16 cos >= {bcos:.5f}")
    ok &= d <= 1e-5 and bcos >= 0.999  # (a model whose own bf16 forward leaves the cos floor cannot be asked to keep it)
    long_ = lens > lw
    dev_miss = {}
    for dev in mr.DEVIATIONS:
        dd, cos = miss(mr.forward(cfg, blob, ids, lens, deviate=dev), want)
        outside = (dd > T) | (cos < 0.999)
        good = bool(outside[long_].all())
        dev_miss[dev] = float(dd[long_].min()) if long_.any() else None
        print(f"  {dev:12s} max|d| per text = {np.array2string(dd, precision=4)}  {'outside' if good else 'INSIDE the tolerance'}", flush=True)
        ok &= good
    data[f"{name}_ids"], data[f"{name}_lens"], data[f"{name}_mean"], data[f"{name}_cls"] = ids.astype(np.int16), lens, want, want_cls
    meta[name] = dict(cfg=cfg, seed=seed, S=S, qk_scale=QK_SCALE, vo_scale=VO_SCALE, mlp_scale=MLP_SCALE, global_qk=GLOBAL_QK, T=T, T_cls=T_cls, deviation_min_miss=dev_miss,
                      weights="tests/modernbert_ref.make_weights(cfg, seed, qk_scale, vo_scale, mlp_scale, global_qk)")
    if name == GE1_CASE:
        g1 = dict(cfg, global_every=1)
        m1, c1 = mr.forward(g1, blob, ids, lens), mr.forward(g1, blob, ids, lens, "cls")
        dd, cos = miss(m1, want)
        apart = bool(((dd > T) | (cos < 0.999))[long_].all())
        print(f"  every layer global (modernbert_ref): against the windowed vectors {np.array2string(dd, precision=4)} {'outside' if apart else 'INSIDE'}")
        ok &= apart
        data[f"{name}_ge1_mean"], data[f"{name}_ge1_cls"] = m1, c1
    return ok


def main() -> int:
    data, meta, ok = {}, {}, True
    only = sys.argv[1:]  # (trying a case: a partial run never writes)
    for name in CASES:
        if not only or name in only:
            ok &= run_case(name, CASES[name][-1], data, meta)
    if not ok or only:
        print("REFUSED: a check failed (or a partial run), nothing written")
        return 1
    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "modernbert_golden.npz", **data)
    (out / "modernbert_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "modernbert_golden.npz", (out / "modernbert_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
