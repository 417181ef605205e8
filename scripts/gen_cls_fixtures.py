"""Writes tests/golden/cls_golden.{npz,json}: the [CLS] vector -- last_hidden_state[0, 0] -- that transformers' BertModel(add_pooling_layer=False)
computes (fp32, eager attention, CPU, one unpadded sequence at a time) for seeded models, the reference of tests/test_cls_pooling_gpu.py.
Run by hand (CPU, a minute or two); no test runs it.

Models: the three head-dimension-32 shapes of tests/minilm_ref.py (128 / 4 heads, 256 / 8, 384 / 12; 2 layers), two with heads of 64 -- 256 / 4
with 2 layers and 128 / 2 with ONE layer (the pruned last layer then takes its residual from the embedding LayerNorm) -- and the 384 / 12 shape
once more at S = 256.  Weights: tests/minilm_ref.make_weights(cfg, seed).  Eight sequences per model, lengths 1, 2 and S among them.

The file holds ids, lengths, the fp32 vectors (plain and L2-normalised), cfg, seed and the bounds -- not the weights.

Bounds, measured against the reference alone (the project's convention, scripts/gen_minilm_fixtures.py): the same transformers model cast to
torch.bfloat16 on the CPU; T = 2 x max|cls_bf16 - cls_fp32| over the sequences of a model, T_norm the same of the L2-normalised vectors.

Before writing, per model, the generator checks that the fp32 MEAN-pooled vector misses the [CLS] vector by more than T in every sequence
longer than one token, and refuses to write otherwise (the next seed is tried): a fixture that cannot tell the two poolings apart pins nothing.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import bert_oracle as bo  # noqa: E402
from scripts.gen_minilm_fixtures import hf_config  # noqa: E402
from tests import minilm_ref as mr  # noqa: E402

SEEDS = range(3, 11)
LENS64 = (64, 1, 2, 37, 50, 9, 33, 21)
LENS256 = (256, 1, 2, 200, 129, 77, 255, 31)
# name -> (cfg, S, lengths)
MODELS = {
    "h128": (mr.model_cfg("h128"), 64, LENS64),
    "h256": (mr.model_cfg("h256"), 64, LENS64),
    "h384": (mr.model_cfg("h384"), 64, LENS64),
    "h384_s256": (mr.model_cfg("h384"), 256, LENS256),
    "h256_hd64": (dict(mr.COMMON, hidden=256, heads=4, ffn=512), 64, LENS64),
    "h128_hd64_l1": (dict(mr.COMMON, hidden=128, heads=2, ffn=256, layers=1), 64, LENS64),
}


def make_inputs(cfg: dict, seed: int, S: int, lens) -> "tuple[np.ndarray, np.ndarray]":
    rng = np.random.default_rng(77000 + seed)
    ids = np.zeros((len(lens), S), np.int32)
    for i, n in enumerate(lens):
        ids[i, :n] = rng.integers(1, cfg["vocab"], n)
    return ids, np.asarray(lens, np.int32)


def hidden_states(cfg, blob, seqs, dtype):
    """([len(seqs), hidden] [CLS] rows, [len(seqs), hidden] token means) of BertModel's last hidden state, f32."""
    import torch
    from transformers import BertModel

    model = BertModel(hf_config(cfg, cfg["heads"]), add_pooling_layer=False).eval()
    missing = model.load_state_dict(bo.to_hf_state_dict(cfg, blob), strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    model = model.to(dtype)
    cls, mean = np.empty((len(seqs), cfg["hidden"]), np.float32), np.empty((len(seqs), cfg["hidden"]), np.float32)
    with torch.no_grad():
        for i, s in enumerate(seqs):
            h = model(input_ids=torch.from_numpy(np.asarray(s, np.int64))[None]).last_hidden_state[0].float()
            cls[i], mean[i] = h[0].numpy(), h.mean(0).numpy()
    return cls, mean


def l2(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)


def main() -> int:
    import torch

    data, meta = {}, {}
    for name, (cfg, S, lens) in MODELS.items():
        chosen = None
        for seed in SEEDS:
            blob = mr.make_weights(cfg, seed)
            ids, lens_a = make_inputs(cfg, seed, S, lens)
            seqs = [ids[i, :n] for i, n in enumerate(lens_a)]
            c32, m32 = hidden_states(cfg, blob, seqs, torch.float32)
            c16, _ = hidden_states(cfg, blob, seqs, torch.bfloat16)
            T = 2.0 * float(np.abs(c16 - c32).max())
            T_norm = 2.0 * float(np.abs(l2(c16) - l2(c32)).max())
            miss = np.abs(m32 - c32).max(1)[lens_a > 1]
            print(f"{name} seed {seed}: T {T:.4f}  T_norm {T_norm:.5f} (scale {np.abs(c32).max():.2f}); the mean misses [CLS] by {miss.min():.3f} .. {miss.max():.3f}")
            if miss.min() > T:
                chosen = seed
                break
        if chosen is None:
            print(f"REFUSED: no seed of {list(SEEDS)} lets {name} tell mean pooling from [CLS] pooling in every sequence")
            return 1
        data[f"{name}_ids"], data[f"{name}_lens"] = ids.astype(np.int16), lens_a
        data[f"{name}_cls"], data[f"{name}_cls_norm"] = c32, l2(c32).astype(np.float32)
        meta[name] = dict(cfg=cfg, seed=chosen, S=S, T=T, T_norm=T_norm, mean_min_miss=float(miss.min()), weights="tests/minilm_ref.make_weights(cfg, seed)")

    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "cls_golden.npz", **data)
    (out / "cls_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "cls_golden.npz", (out / "cls_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
