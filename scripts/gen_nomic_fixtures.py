"""Writes tests/golden/nomic_golden.{npz,json}: pooled vectors of transformers' NomicBertModel (fp32, eager attention, CPU) for
seeded weights.  Run by hand (CPU, a few minutes); no test runs it.

The file holds ids, lens, pooled vectors, cfg, seed, theta and the weight rule -- not the weights: tests regenerate them with
tests/nomic_ref.make_weights (make_blob style "test", Linear biases zeroed, Wq / Wk times qk_scale).

Before writing, the generator checks with the project's pooled-vector tolerance (cos >= 0.999, max|d| <= 2e-2) that
  (i)  tests/nomic_ref.forward lands within 1e-5 of the transformers output in every case, and
  (ii) in each BASE case every one of five convention mix-ups -- no rotation, interleaved pairing, theta 10000 for 1000, GELU for
       SiLU, gate and up halves swapped -- falls OUTSIDE the tolerance,
and refuses to write the file otherwise: fixtures that cannot tell those apart pin nothing.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import nomic_ref as nr  # noqa: E402

QK_SCALE = 4.0
COMMON = dict(vocab=400, layers=2, max_pos=2048, type_vocab=2, ln_eps=1e-12, rotary=True, swiglu=True)
SHAPES = {"s128": dict(hidden=128, heads=2, ffn=256), "s256": dict(hidden=256, heads=4, ffn=512), "s768": dict(hidden=768, heads=12, ffn=3072)}
# name: (shape, S, lens, theta, seed, base?)
CASES = {
    "tiny": ("s128", 32, [32, 17, 3, 31], 1000.0, 5, False),
    "mid": ("s256", 256, [256, 129, 3, 255, 17], 1000.0, 6, False),
    "long": ("s128", 2048, [2048, 1500, 3], 1000.0, 7, False),
    "mid_theta10000": ("s256", 64, [64, 33, 3, 63, 17], 10000.0, 8, False),
    "base": ("s768", 128, [128, 77, 40], 1000.0, 5, True),
    "base_long": ("s768", 2048, [2048, 1100], 1000.0, 9, True),
}
DEVIATIONS = ("no_rope", "interleaved", "theta", "gelu", "swap")


def inside(got, want) -> bool:
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return bool(cos.min() >= 0.999 and np.abs(got - want).max() <= 2e-2)


def transformers_pooled(cfg, blob, ids, lens, theta):
    import torch
    from transformers import NomicBertConfig, NomicBertModel

    hc = NomicBertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                         intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], type_vocab_size=cfg["type_vocab"],
                         layer_norm_eps=cfg["ln_eps"], hidden_act="silu", rope_parameters={"rope_type": "default", "rope_theta": float(theta)})
    hc._attn_implementation = "eager"
    model = NomicBertModel(hc, add_pooling_layer=False).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in nr.to_hf_state_dict(cfg, blob).items()}, strict=True)
    S = ids.shape[1]
    mask = (np.arange(S)[None, :] < lens[:, None])
    out = np.empty((len(lens), cfg["hidden"]), np.float32)
    with torch.no_grad():
        for b in range(len(lens)):  # one chunk at a time keeps the S = 2048 score tensors small
            h = model(input_ids=torch.from_numpy(ids[b:b + 1].astype(np.int64)), attention_mask=torch.from_numpy(mask[b:b + 1].astype(np.int64))).last_hidden_state
            out[b] = h[0, : lens[b]].double().mean(0).float().numpy()
    return out


def main() -> int:
    data, meta, ok = {}, {}, True
    for name, (shape, S, lens, theta, seed, base) in CASES.items():
        cfg = dict(COMMON, **SHAPES[shape])
        blob = nr.make_weights(cfg, seed, QK_SCALE)
        rng = np.random.default_rng(1000 + seed)
        ids = rng.integers(1, cfg["vocab"], size=(len(lens), S)).astype(np.int32)
        lens = np.asarray(lens, np.int32)
        want = transformers_pooled(cfg, blob, ids, lens, theta)
        ref = nr.forward(cfg, blob, ids, lens, theta)
        d = float(np.abs(ref - want).max())
        print(f"{name}: nomic_ref vs transformers max|d| = {d:.2e}")
        ok &= d <= 1e-5
        if base:
            for dev in DEVIATIONS:
                got = nr.forward(cfg, blob, ids, lens, theta, deviate=dev)
                dd, ins = float(np.abs(got - want).max()), inside(got, want)
                print(f"  {dev:12s} max|d| = {dd:.3f}  {'INSIDE the tolerance' if ins else 'outside'}")
                ok &= not ins
        data[f"{name}_ids"], data[f"{name}_lens"], data[f"{name}_pooled"] = ids.astype(np.int16), lens, want
        meta[name] = dict(cfg=cfg, seed=seed, theta=theta, S=S, qk_scale=QK_SCALE, base=base,
                          weights="tests/nomic_ref.make_weights(cfg, seed, qk_scale): make_blob style 'test', Linear biases 0, Wq and Wk * qk_scale")
    if not ok:
        print("REFUSED: a check failed, nothing written")
        return 1
    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "nomic_golden.npz", **data)
    (out / "nomic_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "nomic_golden.npz", (out / "nomic_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
