"""Qwen2.5-0.5B shape on the device (sc_encoder_cfg.arch 2): texts/s with last-token pooling, padded and packed; attention time per
launch of the causal kernel next to the global kernel on the same number of query heads; BERT-base as the yardstick.  One process,
synthetic weights.

    python scripts/bench_qwen2.py [--iters 5] > profiles/qwen2_bench.log

Shape: 24 layers, hidden 896, 14 query heads and 2 K/V heads of 64, SwiGLU 4 864, vocab 151 936, rope_theta 1e6.
Every text is S tokens long (S = 256, 1 024, 2 048; about 32k tokens per batch), embedded as a [B, S] rectangle and as packed rows.
Wall-clock per synchronous call (upload of the ids and download of the vectors included), median of --iters after 2 warm-up calls.

Attention time per launch comes from the runtime's profiling class 3 in a separate, bracketed pass (every launch synchronises: those
passes are not the ones timed).  The global kernel is measured on a 2-layer post-LN rotary model of the same width and head count
(hidden 896, 14 heads: attention_kernel / attention_long_kernel with 14 K/V heads), same B and S, same process.  MFMA work of the causal
kernel = the (query block, key tile) pairs it multiplies -- S/32 (S/32 + 1) / 2 per (text, head) -- x 32 x 32 x 64 x 4 FLOP.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semcode_amd import _native  # noqa: E402

QWEN = dict(vocab=151936, hidden=896, layers=24, heads=14, kv_heads=2, ffn=4864, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True,
            rope_theta=1000000.0)
GLOBAL14 = dict(vocab=1024, hidden=896, layers=2, heads=14, ffn=4864, max_pos=2048, type_vocab=2, ln_eps=1e-6, rotary=True, swiglu=True, rope_theta=1000000.0)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    rt = _native.Runtime(device=0)
    qw = _native.Encoder(rt, QWEN, synth_seed=1, pooling="last")
    glo = _native.Encoder(rt, GLOBAL14, synth_seed=1)
    bert = _native.Encoder(rt, BERT, synth_seed=1)
    rng = np.random.default_rng(0)
    print(f"# Qwen2.5-0.5B shape, {QWEN['layers']} layers, {QWEN['heads']} query / {QWEN['kv_heads']} K/V heads, last-token pooling; median (min .. max) of {a.iters} calls")
    for S in (128, 256, 1024, 2048):
        B = 32768 // S
        ids = rng.integers(1, 30000, size=(B, S)).astype(np.int32)
        gids = ids % GLOBAL14["vocab"]
        lens = np.full(B, S, np.int32)
        flat, offsets = ids.reshape(-1), (np.arange(B + 1) * S).astype(np.int64)
        gflat = gids.reshape(-1)
        for form, call, gcall in (("padded", lambda: qw.embed_ids(ids, lens), lambda: glo.embed_ids(gids, lens)),
                                  ("packed", lambda: qw.embed_packed(flat, offsets), lambda: glo.embed_packed(gflat, offsets))):
            if S >= 256:
                med, lo, hi = timed(call, a.iters)
                print(f"S={S} B={B} {form:6s} qwen2-0.5b: {B / med:9.1f} texts/s  ({B / hi:.1f} .. {B / lo:.1f}), {B * S / med / 1e3:.1f}k tokens/s")
            ms_c, n_c = attention_profile(rt, call)
            ms_g, n_g = attention_profile(rt, gcall)
            t_c, t_g = ms_c / max(n_c, 1), ms_g / max(n_g, 1)
            pairs = (S // 32) * (S // 32 + 1) // 2
            flop = pairs * 32 * 32 * 64 * 4 * B * QWEN["heads"]
            print(f"S={S} B={B} {form:6s} attention per launch: causal {t_c * 1e3:.1f} us ({n_c} launches), global {t_g * 1e3:.1f} us ({n_g} launches), "
                  f"causal / global = {t_c / t_g:.3f}; causal MFMA work {flop / 1e9:.2f} GFLOP -> {flop / (t_c * 1e-3) / 1e12:.1f} TFLOP/s")
        if S == 256:
            bids = rng.integers(1, 30000, size=(B, S)).astype(np.int32)
            med, lo, hi = timed(lambda: bert.embed_ids(bids, lens), a.iters)
            print(f"S={S} B={B} padded BERT-base (12 layers, 768 / 3072): {B / med:9.1f} texts/s  ({B / hi:.1f} .. {B / lo:.1f})")
    for e in (qw, glo, bert):
        e.close()
    rt.close()


if __name__ == "__main__":
    main()
