"""MiniLM-L6 throughput (head dimension 32) next to the same shape with heads of 64, same process, synthetic weights.

    python scripts/bench_minilm.py [--texts 4096] [--passes 3] >> profiles/headdim32_bench.log

Two encoders of 384 hidden / 6 layers / 1536 ffn / 512 positions: 12 heads of 32 (all-MiniLM-L6-v2's shape) and 6 heads of 64.  Their GEMMs
are identical; only the attention kernels differ (attention_kernel / attention_packed_kernel on Head32 against Head64, attention_core.h).  Input: --texts
texts of 256 tokens, as padded rectangles of 256 texts (Encoder.embed_ids) and packed (flatten_ids + Encoder.embed_packed, 65 536 rows a
call).  Per model and path: texts/s (best of --passes timed passes after a warm-up) and, from a separate pass with every launch
bracketed by events (sc_runtime_set_profiling(1), sc_runtime_profile_read(which=3)), the time inside the attention class.  The d32 / d64
ratio of that time is reported, not gated: the same QK^T and PV flops, twice the exponentials and half-filled score MFMAs put it
between 1 and 2.
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

SHAPE = dict(_native.BERT_BASE, hidden=384, layers=6, ffn=1536, max_pos=512)
MODELS = {"d32 (12 heads)": dict(SHAPE, heads=12), "d64 (6 heads)": dict(SHAPE, heads=6)}
BATCH, TOKENS = 256, 256


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    rt = _native.Runtime(device=0)
    rng = np.random.default_rng(23)
    lens = np.full(BATCH, TOKENS, np.int32)
    batches = [rng.integers(1, SHAPE["vocab"], size=(BATCH, TOKENS)).astype(np.int32) for _ in range(max(1, args.texts // BATCH))]
    texts = len(batches) * BATCH
    print(f"# bench_minilm: {texts} texts of {TOKENS} tokens, batches of {BATCH}, best of {args.passes} passes, {_native.lib().sc_version().decode()}")
    attn = {}
    for mname, cfg in MODELS.items():
        enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)

        def padded():
            for ids in batches:
                enc.embed_ids(ids, lens)

        def packed():
            for ids in batches:
                enc.embed_packed(*flatten_ids(ids, lens))

        for path, fn in (("padded", padded), ("packed", packed)):
            fn()  # warm-up: workspace, first touch
            best = None
            for _ in range(args.passes):
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            rt.set_profiling(1)
            rt.profile_reset()
            fn()
            gemm_ms, _ = rt.profile_read(2)
            attn_ms, launches = rt.profile_read(3)
            rt.set_profiling(0)
            attn[(mname, path)] = attn_ms
            print(f"{mname:15s} {path}: {texts / best:9.0f} texts/s  {texts * TOKENS / best / 1e6:7.3f} M tokens/s  {best:.3f} s;  profiled pass: attention "
                  f"{attn_ms:8.2f} ms in {launches} launches, GEMMs {gemm_ms:8.2f} ms", flush=True)
        enc.close()
    for path in ("padded", "packed"):
        a, b = attn[("d32 (12 heads)", path)], attn[("d64 (6 heads)", path)]
        print(f"attention time d32 / d64, {path}: {a / b:.3f}")
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
