"""ModernBERT-base shape on the device: texts/s of the windowed model against the same model with every layer global, and against
BERT-base; attention time per launch of the windowed and the global kernels.  One process, synthetic weights.

    python scripts/bench_modernbert.py [--iters 5] > profiles/modernbert_bench.log

Shape: 22 layers, hidden 768, 12 heads, ffn 1 152, vocab 50 368, local_window 128, global_every 3 (8 global + 14 local layers).
Every text is S tokens long (S = 256, 1 024, 2 048; about 32k tokens per batch), embedded as a [B, S] rectangle and as packed rows.
Wall-clock per synchronous call (upload of the ids and download of the vectors included), median of --iters after 2 warm-up calls.

Attention time per launch comes from the runtime's profiling class 3 in a separate, bracketed pass (every launch synchronises: those
passes are not the ones timed).  The class does not tell kernels apart, so: t_global = the all-global model's time per launch;
t_window = (the windowed model's class total - its 8 global launches x t_global) / its 14 windowed launches.  K/V bytes per second of
the windowed kernel = what its workgroups stage (per sequence and head: for every group of 8 query blocks the tiles
max(0, qb0 - 2) .. min(S / 32, qb0 + 10), 32 rows x 128 B each, K and V) / t_window.
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

BASE = dict(vocab=50368, hidden=768, layers=22, heads=12, ffn=1152, max_pos=8192, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True,
            local_window=128, global_every=3, rope_theta=160000.0, rope_theta_local=10000.0)
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


def staged_bytes(S, B, heads):
    tiles = sum(min(S // 32, qb0 + 10) - max(0, qb0 - 2) for qb0 in range(0, S // 32, 8))
    return tiles * 32 * 128 * 2 * B * heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    rt = _native.Runtime(device=0)
    win = _native.Encoder(rt, BASE, synth_seed=1)
    glo = _native.Encoder(rt, dict(BASE, global_every=1), synth_seed=1)
    bert = _native.Encoder(rt, BERT, synth_seed=1)
    n_local = sum(1 for l in range(BASE["layers"]) if l % BASE["global_every"])
    n_global = BASE["layers"] - n_local
    rng = np.random.default_rng(0)
    print(f"# ModernBERT-base shape, {n_global} global + {n_local} local layers; median (min .. max) of {a.iters} calls")
    for S in (256, 1024, 2048):
        B = 32768 // S
        ids = rng.integers(1, 30000, size=(B, S)).astype(np.int32)
        lens = np.full(B, S, np.int32)
        flat, offsets = ids.reshape(-1), (np.arange(B + 1) * S).astype(np.int64)
        res = {}
        for form, call in (("padded", lambda e: e.embed_ids(ids, lens)), ("packed", lambda e: e.embed_packed(flat, offsets))):
            for name, enc in (("windowed", win), ("all-global", glo)):
                med, lo, hi = timed(lambda: call(enc), a.iters)
                res[form, name] = med
                print(f"S={S} B={B} {form:6s} {name:10s}: {B / med:9.1f} texts/s  ({B / hi:.1f} .. {B / lo:.1f})")
            print(f"S={S} {form}: windowed / all-global = {res[form, 'all-global'] / res[form, 'windowed']:.3f}x")
            ms_g, n_g = attention_profile(rt, lambda: call(glo))
            ms_w, n_w = attention_profile(rt, lambda: call(win))
            t_g = ms_g / max(n_g, 1)
            launches_per_layer = n_g // BASE["layers"]  # packed rows: one launch per class in use
            t_w = (ms_w - n_global * launches_per_layer * t_g) / max(n_w - n_global * launches_per_layer, 1)
            print(f"S={S} {form}: attention per launch: global {t_g * 1e3:.1f} us ({n_g} launches), windowed {t_w * 1e3:.1f} us "
                  f"({n_w - n_global * launches_per_layer} launches), windowed / global = {t_w / t_g:.3f}; windowed K/V staged {staged_bytes(S, B, BASE['heads']) / 1e6:.1f} MB "
                  f"-> {staged_bytes(S, B, BASE['heads']) / (t_w * 1e-3) / 1e12:.2f} TB/s")
        if S == 256:
            bids = rng.integers(1, 30000, size=(B, S)).astype(np.int32)
            med, lo, hi = timed(lambda: bert.embed_ids(bids, lens), a.iters)
            print(f"S={S} B={B} padded BERT-base (12 layers, ffn 3072): {B / med:9.1f} texts/s  ({B / hi:.1f} .. {B / lo:.1f})")
    for e in (win, glo, bert):
        e.close()
    rt.close()


if __name__ == "__main__":
    main()
