"""Qwen3-Embedding-0.6B and Qwen2.5-1.5B shapes on the device (sc_encoder_cfg.arch 2 with head_dim 128): texts/s with last-token pooling,
padded and packed, next to the Qwen2.5-0.5B shape (heads of 64) and BERT-base in the same process; time per launch of the 128-wide causal
kernel against the 64-wide one at equal FLOPs and equal K / V bytes; time per launch of qknorm_rope_kernel against rope_qk_kernel on the
same bytes.  Synthetic weights.

    python scripts/bench_qwen3.py [--iters 3]                                   # texts/s and attention time per launch
    rocprofv3 --kernel-trace --stats -d DIR -o q3 --output-format csv -- python scripts/bench_qwen3.py --kernels
    python scripts/bench_qwen3.py --stats DIR/.../q3_kernel_stats.csv           # the rotation kernels' lines of that run

On the GPU machine every step runs under its own time limit and the steps are chained:
    timeout -k 10 500 python scripts/bench_qwen3.py > q3.log && timeout -k 10 200 rocprofv3 ... -- python scripts/bench_qwen3.py --kernels && ...

Shapes: 0.6B = 28 layers, hidden 1 024, 16 query / 8 K/V heads of 128 (attention width 2 048), SwiGLU 3 072, QK-norm, vocab 151 669;
1.5B = 28 layers, hidden 1 536, 12 / 2 heads of 128, SwiGLU 8 960, biases, vocab 151 936; 0.5B = bench_qwen2.py's.  Every text is S tokens
long (S = 256, 1 024, 2 048; about 32k tokens per batch).  Wall-clock per synchronous call (upload of the ids and download of the vectors
included), median of --iters after 2 warm-up calls.

Attention time per launch comes from the runtime's profiling class 3 in a separate, bracketed pass (every launch synchronises: those
passes are not the ones timed), on 2-layer models: W128 = hidden 1 024, 16 / 8 heads of 128; W64 = hidden 2 048, 32 / 16 heads of 64 --
the same (query, key) pairs x width, i.e. the same MFMA FLOPs, and the same K / V bytes; same B and S.  MFMA work = S/32 (S/32 + 1) / 2
(query block, key tile) pairs per (text, head) x 32 x 32 x head_dim x 4 FLOP.
--kernels runs one padded and one packed call of W128 with QK-norm (qknorm_rope_kernel<128, true>), of W128 without, and of a 2-layer
hidden-2 048 model of 32 / 16 heads of 64 (rope_qk_kernel: (32 + 16) x 64 = the same rotated bytes as (16 + 8) x 128) at B x S = 16 x 2 048.
"""
from __future__ import annotations

import argparse
import csv
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semcode_amd import _native  # noqa: E402

COMMON = dict(max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0)
Q06 = dict(COMMON, vocab=151669, hidden=1024, layers=28, heads=16, kv_heads=8, ffn=3072, head_dim=128, qk_norm=True)
Q15 = dict(COMMON, vocab=151936, hidden=1536, layers=28, heads=12, kv_heads=2, ffn=8960, head_dim=128)
Q05 = dict(COMMON, vocab=151936, hidden=896, layers=24, heads=14, kv_heads=2, ffn=4864)
W128 = dict(COMMON, vocab=1024, hidden=1024, layers=2, heads=16, kv_heads=8, ffn=3072, head_dim=128, qk_norm=True)
W64 = dict(COMMON, vocab=1024, hidden=2048, layers=2, heads=32, kv_heads=16, ffn=3072)
BERT = dict(_native.BERT_BASE)


def timed(fn, iters):
    for _ in range(2):
        fn()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def attention_profile(rt, fn):
    rt.set_profiling(1)
    rt.profile_reset()
    fn()
    ms, n = rt.profile_read(3)
    rt.set_profiling(0)
    return ms, n


def forms(enc, ids, lens):
    B, S = ids.shape
    flat, offsets = ids.reshape(-1), (np.arange(B + 1) * S).astype(np.int64)
    return (("padded", lambda: enc.embed_ids(ids, lens)), ("packed", lambda: enc.embed_packed(flat, offsets)))


def kernels_mode(rt):
    rng = np.random.default_rng(0)
    ids = rng.integers(1, 1024, size=(16, 2048)).astype(np.int32)
    lens = np.full(16, 2048, np.int32)
    for cfg in (W128, dict(W128, qk_norm=False), W64):
        enc = _native.Encoder(rt, cfg, synth_seed=1, pooling="last")
        for _, call in forms(enc, ids, lens):
            call()
        enc.close()


def stats_mode(path):
    M, nblk = 16 * 2048, (16 + 8) * 2  # rows; 64-column blocks read and written
    print(f"# rotation kernels at B x S = 16 x 2048 ({M} rows, {nblk} blocks of 64 columns: {2 * M * nblk * 128 / 1e6:.1f} MB read + written a launch), from {Path(path).name}")
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "rope" in name or "attention_causal" in name:
            avg = float(row["AverageNs"])
            tb = f", {2 * M * nblk * 128 / avg / 1e3:.2f} TB/s" if "rope" in name else ""
            print(f"{name.split('(')[0]}: {row['Calls']} calls, average {avg / 1e3:.1f} us{tb}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        return stats_mode(a.stats)
    rt = _native.Runtime(device=0)
    if a.kernels:
        kernels_mode(rt)
        rt.close()
        return
    rng = np.random.default_rng(0)
    print(f"# last-token pooling, synthetic weights; median (min .. max) of {a.iters} calls")
    for name, cfg in (("qwen3-0.6b", Q06), ("qwen2.5-1.5b", Q15), ("qwen2.5-0.5b", Q05)):
        enc = _native.Encoder(rt, cfg, synth_seed=1, pooling="last")
        for S in (256, 1024, 2048):
            B = 32768 // S
            ids = rng.integers(1, 30000, size=(B, S)).astype(np.int32)
            for form, call in forms(enc, ids, np.full(B, S, np.int32)):
                med, lo, hi = timed(call, a.iters)
                print(f"S={S} B={B} {form:6s} {name}: {B / med:9.1f} texts/s  ({B / hi:.1f} .. {B / lo:.1f}), {B * S / med / 1e3:.1f}k tokens/s", flush=True)
        enc.close()
    bert = _native.Encoder(rt, BERT, synth_seed=1)
    bids = rng.integers(1, 30000, size=(128, 256)).astype(np.int32)
    med, lo, hi = timed(lambda: bert.embed_ids(bids, np.full(128, 256, np.int32)), a.iters)
    print(f"S=256 B=128 padded BERT-base (12 layers, 768 / 3072): {128 / med:9.1f} texts/s  ({128 / hi:.1f} .. {128 / lo:.1f})")
    bert.close()
    w128, w64 = _native.Encoder(rt, W128, synth_seed=1, pooling="last"), _native.Encoder(rt, W64, synth_seed=1, pooling="last")
    for S in (128, 256, 1024, 2048):
        B = 32768 // S
        ids = rng.integers(1, 1024, size=(B, S)).astype(np.int32)
        lens = np.full(B, S, np.int32)
        for (form, c128), (_, c64) in zip(forms(w128, ids, lens), forms(w64, ids, lens)):
            ms_a, n_a = attention_profile(rt, c128)
            ms_b, n_b = attention_profile(rt, c64)
            t_a, t_b = ms_a / max(n_a, 1), ms_b / max(n_b, 1)
            flop = (S // 32) * (S // 32 + 1) // 2 * 32 * 32 * 128 * 4 * B * 16
            print(f"S={S} B={B} {form:6s} causal attention per launch: 16/8 heads of 128 {t_a * 1e3:.1f} us ({n_a} launches), 32/16 heads of 64 {t_b * 1e3:.1f} us "
                  f"({n_b} launches), 128 / 64 = {t_a / t_b:.3f}; MFMA work {flop / 1e9:.2f} GFLOP -> {flop / (t_a * 1e-3) / 1e12:.1f} TFLOP/s at 128")
    w128.close()
    w64.close()
    rt.close()


if __name__ == "__main__":
    main()
