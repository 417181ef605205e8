"""[CLS] pooling throughput: mean pooling, [CLS] with the full last layer (cls_prune 0) and [CLS] with the last layer on the [CLS] rows only
(cls_prune 1), alternating in one process, synthetic weights.

    python scripts/bench_cls.py [--texts 4096] [--passes 3] [--models bge-small,bge-base,bge-large,minilm-l6] >> profiles/cls_bench.log

Input: --texts texts of 256 tokens as padded rectangles of 256 texts (Encoder.embed_ids) and packed (flatten_ids + Encoder.embed_packed, 65 536
rows a call).  Per model and form, --passes rounds of (mean, cls_prune 0, cls_prune 1), one timed pass each per round: texts/s of every pass,
the best per mode, and the spread (max / min - 1) of a mode's passes -- the yardstick is the mean-pooled rate, the parent's code.  Ratios are
printed next to the FLOP-count ceiling 1 / (1 - 0.75 / layers) of the GEMM time (out-projection and feed-forward of the last layer are 18 / 24
of its GEMM work).  attention_cls_kernel: from two passes with every launch bracketed by events (sc_runtime_set_profiling(1), class 3 =
attention), the time of the attention class with cls_prune 1 minus (layers - 1) / layers of that with cls_prune 0, per launch, next to the
K / V bytes a launch streams (tokens x 2 H x 2) and the rate the two give.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semcode_amd import _native  # noqa: E402
from semcode_amd.embeddings.providers import flatten_ids  # noqa: E402

MODELS = {
    "bge-small": dict(_native.BERT_BASE, hidden=384, heads=12, layers=12, ffn=1536),
    "bge-base": dict(_native.BERT_BASE, hidden=768, heads=12, layers=12, ffn=3072),
    "bge-large": dict(_native.BERT_BASE, hidden=1024, heads=16, layers=24, ffn=4096),
    "minilm-l6": dict(_native.BERT_BASE, hidden=384, heads=12, layers=6, ffn=1536),
}
MODES = (("mean", "mean", -1), ("cls_prune 0", "cls", 0), ("cls_prune 1", "cls", 1))
BATCH, TOKENS = 256, 256


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--models", default=",".join(MODELS))
    args = ap.parse_args()
    rt = _native.Runtime(device=0)
    rng = np.random.default_rng(23)
    lens = np.full(BATCH, TOKENS, np.int32)
    batches = [rng.integers(1, 30000, size=(BATCH, TOKENS)).astype(np.int32) for _ in range(max(1, args.texts // BATCH))]
    flats = [flatten_ids(ids, lens) for ids in batches]
    texts = len(batches) * BATCH
    print(f"# bench_cls: {texts} texts of {TOKENS} tokens, batches of {BATCH}, {args.passes} alternating rounds, {_native.lib().sc_version().decode()}")
    for mname in args.models.split(","):
        cfg = MODELS[mname]
        L, H = cfg["layers"], cfg["hidden"]
        enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)

        def padded():
            for ids in batches:
                enc.embed_ids(ids, lens)

        def packed():
            for f in flats:
                enc.embed_packed(*f)

        def select(pooling, prune):
            enc.pooling = pooling
            _native.diag_set_option("cls_prune", prune)

        print(f"{mname}: hidden {H}, {cfg['heads']} heads, {L} layers, ffn {cfg['ffn']}; GEMM-time ceiling of cls_prune 1 / cls_prune 0: {1 / (1 - 0.75 / L):.3f}")
        for form, fn in (("padded", padded), ("packed", packed)):
            for _, pooling, prune in MODES:  # warm-up: workspace, first touch, split-K scratch
                select(pooling, prune)
                fn()
            rates = {m[0]: [] for m in MODES}
            for _ in range(args.passes):
                for mode, pooling, prune in MODES:
                    select(pooling, prune)
                    t0 = time.perf_counter()
                    fn()
                    rates[mode].append(texts / (time.perf_counter() - t0))
            best = {m: max(r) for m, r in rates.items()}
            spread = max(max(r) / min(r) - 1 for r in rates.values())
            for mode, r in rates.items():
                print(f"  {form} {mode:12s}: best {best[mode]:9.0f} texts/s   passes {' '.join(f'{x:.0f}' for x in r)}   spread {100 * (max(r) / min(r) - 1):.2f} %")
            print(f"  {form} ratios: cls_prune 0 / mean {best['cls_prune 0'] / best['mean']:.4f}   cls_prune 1 / mean {best['cls_prune 1'] / best['mean']:.4f}   "
                  f"cls_prune 1 / cls_prune 0 {best['cls_prune 1'] / best['cls_prune 0']:.4f}   (largest spread {100 * spread:.2f} %)", flush=True)
            attn = {}
            for prune in (0, 1):
                select("cls", prune)
                rt.set_profiling(1)
                rt.profile_reset()
                fn()
                attn[prune] = rt.profile_read(3)
                rt.set_profiling(0)
            launches = len(batches)
            t_cls = (attn[1][0] - attn[0][0] * (L - 1) / L) / launches
            kv = BATCH * TOKENS * 2 * H * 2
            print(f"  {form} attention class: cls_prune 0 {attn[0][0]:.2f} ms in {attn[0][1]} launches, cls_prune 1 {attn[1][0]:.2f} ms in {attn[1][1]}; "
                  f"attention_cls_kernel ~ {1e3 * t_cls:.1f} us a launch for {kv / 1e6:.1f} MB of K / V ({kv / max(t_cls, 1e-9) / 1e9:.2f} TB/s)", flush=True)
        _native.diag_set_option("cls_prune", -1)
        enc.close()
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
