"""Writes tests/golden/t5_golden.{npz,json}: first-token and mean-pooled vectors of transformers' T5EncoderModel (fp32, eager, CPU) for
seeded weights, and transformers' own bucket tables.  Run by hand (CPU, a few minutes); no test runs it.

The files hold ids, lens, the two vectors per text, cfg, seed, the weight rule and the tolerances -- not the weights: tests regenerate
them with tests/t5_ref.make_weights(cfg, seed, qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma) -- and
T5Attention._relative_position_bucket for the distances -2047 .. 2047 at (buckets, max_distance) = (32, 128), (16, 32), (32, 64).

T per case and pooling = 2 x max|vector_bf16 - vector_fp32| over the texts of the case, transformers' own bf16 forward of that model
against its fp32 forward (T_first, T_mean): the rule of the other golden files, measured against the reference, never against the code
under test.  Users add the floor cos >= 0.999.

Before writing, the generator checks in every case that
  (i)   tests/t5_ref.forward lands within 1e-5 of transformers, both poolings,
  (ii)  the model's own bf16 forward keeps cos >= 0.99975 for both poolings, and
  (iii) the mix-ups of t5_ref.DEVIATIONS put every text longer than 32 tokens outside (T, cos >= 0.999) in the mean-pooled or in the
        first-token vector.  "no_bias", "mirrored" and "scores/8" must be caught in every case; any other (case, mix-up) pair that is
        not caught is recorded with its measured miss ("dropped" in the json) instead of refusing the case; every mix-up except
        "erf_gelu" (expected to vanish in whole-model vectors: the single-kernel test pins it) must be caught in at least one case.
  (iv)  where a case has a projection behind the pooling (torch's Linear + normalize on transformers' pooled rows; T_proj by the rule of
        T), tests/t5_ref.project is within 1e-5, and "proj_skipped" (where E = hidden) and "normalise_before_proj" are caught or recorded.
Each case takes the first entry of SCALES that passes, and the files record which.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import t5_ref as tr  # noqa: E402

# (qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma), tried in this order
SCALES = [(2.0, 1.0, 3.0, 3.0, 5.0, 0.3), (1.5, 1.0, 3.0, 3.0, 5.0, 0.3), (1.0, 1.0, 3.0, 3.0, 5.0, 0.3), (2.0, 1.5, 2.0, 3.0, 5.0, 0.3),
          (1.0, 1.0, 2.0, 2.0, 5.0, 0.3), (1.0, 1.0, 1.0, 1.0, 5.0, 0.3)]
COMMON = dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-6, t5=True, rel_buckets=32, rel_max_distance=128)
SHAPES = {"s128": dict(hidden=128, heads=2, ffn=256, t5_ffn="relu"), "s128_b16": dict(hidden=128, heads=2, ffn=256, t5_ffn="relu", rel_buckets=16, rel_max_distance=32),
          "s256": dict(hidden=256, heads=4, ffn=512, t5_ffn="gated-gelu"), "s256_aw128": dict(hidden=256, heads=2, head_dim=64, ffn=512, t5_ffn="gated-gelu"),
          "s768": dict(hidden=768, heads=12, ffn=3072, t5_ffn="relu")}
# name: (shape, layers, S, lens, seed[, (E, bias, pooling) of the projection behind the pooling])
CASES = {
    "relu_s64": ("s128", 3, 64, [64, 33, 32, 1], 41),
    "b16_s128": ("s128_b16", 3, 128, [128, 65], 42),
    "gated_s512": ("s256", 2, 512, [300, 129, 65], 43),
    "aw128_s128": ("s256_aw128", 2, 128, [128, 31], 44),
    "relu_s1024": ("s128", 2, 1024, [600, 513], 45),
    "relu_s2048": ("s128", 2, 2048, [1100], 46),
    "base_relu": ("s768", 1, 128, [128, 70], 47, (256, True, "first")),  # the CodeT5+ form: first token -> Linear(768, 256) with bias -> L2
    "dense_mean": ("s256", 2, 128, [128, 70], 48, (256, False, "mean")),   # the sentence-T5 form: mean -> Dense(256, 256) without bias -> L2
}
BUCKET_TABLES = [(32, 128), (16, 32), (32, 64)]
NEVER_DROPPED = ("no_bias", "mirrored", "scores/8")
BF16_COS, COS_FLOOR = 0.99975, 0.999


def miss(got, want):
    """per text: (max|d|, cos)"""
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


def transformers_projection(pooled, W, b, dtype="float32"):
    """torch's Linear + normalize on transformers' pooled rows, in the model's own precision"""
    import torch

    t = torch.float32 if dtype == "float32" else torch.bfloat16
    y = torch.nn.functional.linear(torch.from_numpy(pooled).to(t), torch.from_numpy(W).to(t), None if b is None else torch.from_numpy(b).to(t))
    return torch.nn.functional.normalize(y, dim=1).float().numpy()


def transformers_vectors(cfg, blob, ids, lens, dtype="float32"):
    import torch
    from transformers import T5Config, T5EncoderModel

    hc = T5Config(**{k: v for k, v in tr.hf_config(cfg).items() if k != "model_type"})
    model = T5EncoderModel(hc).eval()
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in tr.to_hf_state_dict(cfg, blob).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    if dtype == "bfloat16":
        model = model.to(torch.bfloat16)
    S = ids.shape[1]
    mask = np.arange(S)[None, :] < lens[:, None]
    first = np.empty((len(lens), cfg["hidden"]), np.float32)
    mean = np.empty_like(first)
    with torch.no_grad():
        for b in range(len(lens)):  # one text at a time keeps the S = 2048 score tensors small
            h = model(input_ids=torch.from_numpy(ids[b:b + 1].astype(np.int64)), attention_mask=torch.from_numpy(mask[b:b + 1].astype(np.int64))).last_hidden_state
            first[b] = h[0, 0].float().numpy()
            mean[b] = h[0, : lens[b]].double().mean(0).float().numpy()
    return first, mean


def applies(dev, cfg):
    return not (dev in ("gate_halves_swapped", "erf_gelu") and not tr.gated(cfg))


def try_scales(name, cfg, seed, ids, lens, scales, proj=None):
    """One case at one entry of SCALES: transformers fp32 and bf16, the restatement, the mix-ups.  -> (ok, arrays, meta)"""
    blob = tr.make_weights(cfg, seed, *scales)
    want = dict(zip(("first", "mean"), transformers_vectors(cfg, blob, ids, lens)))
    low = dict(zip(("first", "mean"), transformers_vectors(cfg, blob, ids, lens, "bfloat16")))
    T = {p: 2.0 * float(np.abs(low[p] - want[p]).max()) for p in want}
    bcos = float(min(miss(low[p], want[p])[1].min() for p in want))
    d = max(float(np.abs(tr.forward(cfg, blob, ids, lens, p) - want[p]).max()) for p in want)
    print(f"{name} (seed {seed}) scales {scales}: t5_ref vs transformers max|d| = {d:.2e}; T_first = {T['first']:.4f}, T_mean = {T['mean']:.4f}, bf16 cos >= {bcos:.5f}", flush=True)
    if not (d <= 1e-5 and bcos >= BF16_COS):
        return False, None, None
    long_ = lens > 32
    caught, dropped, ok = {}, {}, True
    for dev in tr.DEVIATIONS:
        if not applies(dev, cfg):
            continue
        by, least = [], {}
        for p in ("first", "mean"):
            dd, cos = miss(tr.forward(cfg, blob, ids, lens, p, deviate=dev), want[p])
            outside = (dd > T[p]) | (cos < COS_FLOOR)
            least[p] = float(dd[long_].min())
            if bool(outside[long_].all()):
                by.append(p)
        print(f"  {dev:24s} least max|d| over the long texts: first {least['first']:.4f}, mean {least['mean']:.4f}  caught by {by or 'NOTHING'}", flush=True)
        if by:
            caught[dev] = by
        elif dev in NEVER_DROPPED:
            ok = False
        else:
            dropped[dev] = least
    extra_arrays, extra_meta = {}, {}
    if proj:  # the projection behind the pooling: T_proj by the same rule, its two mix-ups
        E, with_bias, pooling = proj
        W, b = tr.make_proj(cfg["hidden"], E, seed, with_bias)
        pw, pl = transformers_projection(want[pooling], W, b), transformers_projection(low[pooling], W, b, "bfloat16")
        T_proj = 2.0 * float(np.abs(pl - pw).max())
        dp = float(np.abs(tr.project(want[pooling], W, b) - pw).max())
        pcos = float(miss(pl, pw)[1].min())
        print(f"  projection E {E} bias {with_bias} on {pooling}: t5_ref.project vs torch max|d| = {dp:.2e}; T_proj = {T_proj:.5f}, bf16 cos >= {pcos:.5f}", flush=True)
        ok &= dp <= 1e-5 and pcos >= BF16_COS
        for dev in tr.PROJ_DEVIATIONS:
            if dev == "proj_skipped" and E != cfg["hidden"]:
                continue  # another width: not comparable, and no test could mistake it
            dd, cos = miss(tr.project(want[pooling], W, b, deviate=dev), pw)
            good = bool(((dd > T_proj) | (cos < COS_FLOOR))[long_].all())
            print(f"  {dev:24s} least max|d| over the long texts: {float(dd[long_].min()):.5f}  {'caught' if good else 'NOT caught'}", flush=True)
            if good:
                caught[dev] = [pooling]
            else:
                dropped[dev] = {pooling: float(dd[long_].min())}
        extra_arrays = {f"{name}_proj": pw}
        extra_meta = dict(proj=dict(E=E, bias=with_bias, pooling=pooling, T_proj=T_proj, bf16_cos=pcos, weights="tests/t5_ref.make_proj(hidden, E, seed, bias)"))
    arrays = {f"{name}_ids": ids.astype(np.int16), f"{name}_lens": lens, f"{name}_first": want["first"], f"{name}_mean": want["mean"]}
    meta = dict(cfg=cfg, seed=seed, S=int(ids.shape[1]), scales=list(scales), T_first=T["first"], T_mean=T["mean"], bf16_cos=bcos, caught=caught, dropped=dropped,
                weights="tests/t5_ref.make_weights(cfg, seed, *scales): qk_scale, bias_sigma, vo_scale, mlp_scale, emb_scale, norm_sigma")
    arrays.update(extra_arrays)
    meta.update(extra_meta)
    return ok, arrays, meta


def run_case(name, data, meta) -> bool:
    shape, layers, S, lens, seed = CASES[name][:5]
    proj = CASES[name][5] if len(CASES[name]) > 5 else None
    cfg = dict(COMMON, **SHAPES[shape], layers=layers)
    rng = np.random.default_rng(5000 + seed)
    lens = np.asarray(lens, np.int32)
    ids = rng.integers(1, cfg["vocab"], size=(len(lens), S)).astype(np.int32)
    ids[np.arange(S)[None, :] >= lens[:, None]] = 0  # padding (never read by a real row)
    for scales in SCALES:
        ok, arrays, m = try_scales(name, cfg, seed, ids, lens, scales, proj)
        if ok:
            data.update(arrays)
            meta[name] = m
            return True
    print(f"{name}: no entry of SCALES passes the checks")
    return False


def bucket_tables(data):
    import torch
    from transformers.models.t5.modeling_t5 import T5Attention

    rel = torch.arange(-2047, 2048)
    for nb, md in BUCKET_TABLES:
        ref = T5Attention._relative_position_bucket(rel, bidirectional=True, num_buckets=nb, max_distance=md).numpy()
        assert np.array_equal(ref, tr.buckets(rel.numpy(), nb, md)), (nb, md)  # the restatement agrees bin edge by bin edge
        data[f"buckets_{nb}_{md}"] = ref.astype(np.int16)


def main() -> int:
    data, meta, ok = {}, {}, True
    only = sys.argv[1:]  # (trying a case: a partial run never writes)
    bucket_tables(data)
    for name in CASES:
        if not only or name in only:
            ok &= run_case(name, data, meta)
    everywhere = {d for m in meta.values() for d in m["caught"]}
    lost = [d for d in tr.DEVIATIONS + tr.PROJ_DEVIATIONS if d != "erf_gelu" and d not in everywhere]
    if lost and not only:
        print("mix-ups no case catches:", lost)
        ok = False
    if not ok or only:
        print("REFUSED: a check failed (or a partial run), nothing written")
        return 1
    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "t5_golden.npz", **data)
    (out / "t5_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "t5_golden.npz", (out / "t5_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
