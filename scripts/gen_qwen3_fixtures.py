"""Writes tests/golden/qwen3_golden.{npz,json}: last-token and mean-pooled vectors of transformers' Qwen3Model (the QK-norm cases) and
Qwen2Model (heads of 128 with biases, no QK-norm) -- fp32, eager attention, CPU -- for seeded weights.  Run by hand (CPU, a few minutes);
no test runs it.

The files hold ids, lens, the two vectors per text, cfg, seed, the weight rule and the tolerances -- not the weights: tests regenerate
them with tests/qwen3_ref.make_weights(cfg, seed, *scales).

T per case and pooling = 2 x max|vector_bf16 - vector_fp32| over the texts of the case, transformers' own bf16 forward of that model
against its fp32 forward (T_last, T_mean): the rule of the other golden files, measured against the reference, never against the code
under test.  Users add the floor cos >= 0.999.

Before writing, the generator checks in every case that
  (i)   tests/qwen3_ref.forward lands within 1e-5 of transformers, both poolings,
  (ii)  the model's own bf16 forward keeps cos >= 0.99975 for both poolings, and
  (iii) each mix-up of qwen3_ref.DEVIATIONS that applies to the case (the four norm mix-ups need qk_norm; interleaved K/V heads need
        1 < kv_heads < heads) puts the LAST-token vector of EVERY text longer than 32 tokens outside (T_last, cos >= 0.999),
and refuses to write otherwise.  Each case takes the first entry of SCALES that passes (i) - (iii); the files record which, and the
smallest miss of every mix-up over the case's long texts.  A mix-up listed in DROPPED for a case is measured and recorded but does not
refuse the case; the reason stands there and in DESIGN.md.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import qwen3_ref as q3  # noqa: E402

# (qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma, bias_first, qk_gamma), tried in this order
SCALES_NORM = [(1.0, 0.3, 2.0, 3.0, 5.0, 0.3, 0, 1.2), (1.0, 0.2, 3.0, 3.0, 5.0, 0.3, 0, 1.0), (1.0, 0.3, 2.0, 3.0, 5.0, 0.3, 0, 1.5),
               # a text beyond a thousand tokens: without the fastest pairs (tests/qwen2_ref.make_weights says why), sharper, a quieter V path
               (1.0, 0.4, 2.0, 3.0, 5.0, 0.5, 5, 1.1), (1.0, 0.4, 2.0, 3.0, 5.0, 0.5, 5, 1.3), (1.0, 0.4, 2.5, 3.0, 5.0, 0.5, 5, 1.2), (1.0, 0.4, 1.5, 3.0, 5.0, 0.5, 5, 1.0)]
SCALES_BIAS = [(1.0, 2.0, 3.0, 3.0, 5.0, 0.3, 0, 1.0), (2.0, 2.0, 3.0, 3.0, 5.0, 0.3, 0, 1.0), (1.0, 2.5, 2.0, 3.0, 5.0, 0.3, 0, 1.0), (1.0, 1.7, 4.0, 3.0, 5.0, 0.3, 0, 1.0)]
COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0, head_dim=128)
# name: (hidden, heads, kv_heads, ffn, qk_norm, layers, S, lens, seed)
CASES = {
    "n_aw2h": (128, 2, 1, 256, True, 3, 512, [300, 129, 65, 33, 32, 31, 1], 31),  # AW = 2 hidden
    "n_g2": (256, 4, 2, 512, True, 2, 256, [256, 129, 65], 32),
    "b_mha": (256, 2, 2, 512, False, 2, 128, [128, 65], 33),                       # Qwen2 biases, AW = hidden
    "n_s2048": (256, 2, 1, 512, True, 4, 2048, [1100, 40, 7], 34),                 # a long text among short batch-mates
    "n_06b": (1024, 16, 8, 3072, True, 2, 64, [64, 33], 35),                       # the 0.6B width
    "b_15b": (1536, 12, 2, 8960, False, 1, 64, [64, 40], 36),                      # the 1.5B width
}
ONE_LAYER = "one layer: the last token's row reads K / V of the embeddings only, and no later key exists for it -- no mask changes it (the miss is 0)"
LONG_TEXT = ("the 1 100-token text: among that many keys one more visible key moves the last token's vector by less than the model's own bf16 error there; "
             "every weight scale tried that sharpens the softmax enough leaves rule (i) or (ii) first.  no_mask is told apart; the mask at this length is "
             "pinned on the kernel itself (tests/test_qwen3_gpu.py, float64 reference with the mask one key wider)")
DROPPED: dict = {"b_15b": {"no_mask": ONE_LAYER, "mask_p1": ONE_LAYER}, "n_s2048": {"mask_p1": LONG_TEXT}}  # case -> {deviation: reason}
BF16_COS, COS_FLOOR = 0.99975, 0.999


def miss(got, want):
    """per text: (max|d|, cos)"""
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


def transformers_vectors(cfg, blob, ids, lens, dtype="float32"):
    import torch
    from transformers import Qwen2Config, Qwen2Model, Qwen3Config, Qwen3Model

    kw = {k: v for k, v in q3.hf_config(cfg).items() if k != "model_type"}
    hc = Qwen3Config(**kw) if cfg.get("qk_norm") else Qwen2Config(**kw)
    hc._attn_implementation = "eager"
    model = (Qwen3Model if cfg.get("qk_norm") else Qwen2Model)(hc).eval()
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in q3.to_hf_state_dict(cfg, blob).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if dtype == "bfloat16":
        model = model.to(torch.bfloat16)
    S = ids.shape[1]
    mask = np.arange(S)[None, :] < lens[:, None]
    last = np.empty((len(lens), cfg["hidden"]), np.float32)
    mean = np.empty_like(last)
    with torch.no_grad():
        for b in range(len(lens)):  # one text at a time, cut to its length: keeps the S = 2048 score tensors small
            n = int(lens[b])
            h = model(input_ids=torch.from_numpy(ids[b:b + 1, :n].astype(np.int64)), attention_mask=torch.from_numpy(mask[b:b + 1, :n].astype(np.int64))).last_hidden_state
            last[b] = h[0, n - 1].float().numpy()
            mean[b] = h[0, :n].double().mean(0).float().numpy()
    return last, mean


def try_scales(name, cfg, seed, ids, lens, scales):
    """One case at one entry of SCALES: transformers fp32 and bf16, the restatement, the mix-ups.  -> (ok, arrays, meta)"""
    blob = q3.make_weights(cfg, seed, *scales)
    want, want_mean = transformers_vectors(cfg, blob, ids, lens)
    low, low_mean = transformers_vectors(cfg, blob, ids, lens, "bfloat16")
    T_last, T_mean = 2.0 * float(np.abs(low - want).max()), 2.0 * float(np.abs(low_mean - want_mean).max())
    bcos = float(min(miss(low, want)[1].min(), miss(low_mean, want_mean)[1].min()))
    d = max(float(np.abs(q3.forward(cfg, blob, ids, lens, "last") - want).max()), float(np.abs(q3.forward(cfg, blob, ids, lens, "mean") - want_mean).max()))
    print(f"{name} (seed {seed}) scales {scales}: qwen3_ref vs transformers max|d| = {d:.2e}; T_last = {T_last:.4f}, T_mean = {T_mean:.4f}, bf16 cos >= {bcos:.5f}", flush=True)
    ok = d <= 1e-5 and bcos >= BF16_COS
    if not ok:
        return False, None, None
    long_ = lens > 32
    dev_miss, dev_cos = {}, {}
    for dev in q3.DEVIATIONS:
        if not q3.applicable(cfg, dev):
            continue
        dd, cos = miss(q3.forward(cfg, blob, ids, lens, "last", deviate=dev), want)
        outside = (dd > T_last) | (cos < COS_FLOOR)
        good = bool(outside[long_].all())
        dev_miss[dev], dev_cos[dev] = float(dd[long_].min()), float(cos[long_].max())
        dropped = dev in DROPPED.get(name, {})
        print(f"  {dev:16s} max|d| per text = {np.array2string(dd, precision=4)}  {'outside' if good else 'INSIDE the tolerance'}{' (dropped for this case)' if dropped else ''}", flush=True)
        ok &= good or dropped
    arrays = {f"{name}_ids": ids.astype(np.int16), f"{name}_lens": lens, f"{name}_last": want, f"{name}_mean": want_mean}
    meta = dict(cfg=cfg, seed=seed, S=int(ids.shape[1]), scales=list(scales), T_last=T_last, T_mean=T_mean, bf16_cos=bcos, deviation_min_miss=dev_miss,
                deviation_max_cos=dev_cos, dropped=DROPPED.get(name, {}),
                weights="tests/qwen3_ref.make_weights(cfg, seed, *scales): (qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma, bias_first, qk_gamma)")
    return ok, arrays, meta


def run_case(name, data, meta) -> bool:
    hidden, heads, kvh, ffn, qkn, layers, S, lens, seed = CASES[name]
    cfg = dict(COMMON, hidden=hidden, heads=heads, kv_heads=kvh, ffn=ffn, layers=layers, qk_norm=qkn)
    rng = np.random.default_rng(3000 + seed)
    lens = np.asarray(lens, np.int32)
    ids = rng.integers(1, cfg["vocab"], size=(len(lens), S)).astype(np.int32)
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0  # padding (never read by a real row)
    for scales in (SCALES_NORM if qkn else SCALES_BIAS):
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
    np.savez_compressed(out / "qwen3_golden.npz", **data)
    (out / "qwen3_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "qwen3_golden.npz", (out / "qwen3_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
