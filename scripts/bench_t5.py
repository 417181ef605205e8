"""T5 encoder shapes on the device (sc_encoder_cfg.arch 3): texts/s padded and packed, next to BERT-base in the same process; time per
launch of the bias attention (Head64Rel) against the plain (Head64<false>) and the ALiBi (Head64<true>) kernels on the same shapes; time per
launch of output_proj_kernel.  Synthetic weights.

    python scripts/bench_t5.py [--iters 3]                                      # texts/s and attention time per launch
    rocprofv3 --kernel-trace -d DIR -o t5 --output-format csv -- python scripts/bench_t5.py --kernels
    python scripts/bench_t5.py --trace DIR/.../t5_kernel_trace.csv              # output_proj_kernel's launches of that run

On the GPU machine every step runs under a time limit of its own and the steps are chained:
    timeout -k 10 500 python scripts/bench_t5.py > t5.log && timeout -k 10 200 rocprofv3 ... -- python scripts/bench_t5.py --kernels && ...

Shapes: codet5p-110m = 12 layers, 768 / 12 heads / ffn 3 072 ReLU, vocab 32 100, first-token pooling, output projection 768 -> 256 with
bias; sentence-t5-base = the same width with the tanh-GELU gate, ffn 2 048, mean pooling, output projection 768 -> 768 without bias.  The
projections are installed (sc_encoder_set_output_proj): the vectors timed are the projected, normalised ones.  Every text is S tokens long (S = 256, 1 024, 2 048; about 32k tokens per batch).  Wall-clock per synchronous call (upload of the
ids and download of the vectors included), median of --iters after 2 warm-up calls.

Attention time per launch comes from the runtime's profiling class 3 in a separate, bracketed pass (every launch synchronises: those
passes are not the ones timed), on 2-layer models of 768 / 12 heads: T5 (bias table), BERT with learned positions (plain scores) and BERT
with ALiBi -- the same (query, key) pairs, the same K / V bytes, same B and S.
--kernels launches output_proj_kernel alone (sc_diag_output_proj) PROJ_REPEAT times for each of PROJ_SHAPES, in that order; --trace reads
the kernel trace of such a run and prints the median of each group without its first launch.
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

T5 = dict(max_pos=2048, type_vocab=1, ln_eps=1e-6, t5=True, rel_buckets=32, rel_max_distance=128, vocab=32100, hidden=768, heads=12)
CODET5P = dict(T5, layers=12, ffn=3072, t5_ffn="relu")
ST5 = dict(T5, layers=12, ffn=2048, t5_ffn="gated-gelu")
BERT = dict(_native.BERT_BASE)
A_REL = dict(T5, vocab=1024, layers=2, ffn=3072, t5_ffn="relu")
A_PLAIN = dict(_native.BERT_BASE, vocab=1024, layers=2, max_pos=2048)
A_ALIBI = dict(A_PLAIN, alibi=True)
# (B, H, E, bias): the batches of the throughput lines at both output widths, and one row
PROJ_SHAPES = [(B, 768, E, E == 256) for E in (256, 768) for B in (128, 32, 16, 1)]
PROJ_REPEAT = 6


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
    return ms / max(n, 1), n


def forms(enc, ids, lens):
    B, S = ids.shape
    flat, offsets = ids.reshape(-1), (np.arange(B + 1) * S).astype(np.int64)
    return (("padded", lambda: enc.embed_ids(ids, lens)), ("packed", lambda: enc.embed_packed(flat, offsets)))


def proj_weights(rng, H, E, bias):
    return (rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float32), (rng.standard_normal(E).astype(np.float32) * 0.1 if bias else None)


def kernels_mode(rt):
    rng = np.random.default_rng(0)
    for B, H, E, bias in PROJ_SHAPES:
        W, b = proj_weights(rng, H, E, bias)
        x = rng.standard_normal((B, H)).astype(np.float32)
        for _ in range(PROJ_REPEAT):
            _native.diag_output_proj(rt, x, W, b)


def trace_mode(path):
    rows = [r for r in csv.DictReader(open(path)) if "output_proj_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(PROJ_SHAPES) * PROJ_REPEAT:
        sys.exit(f"{path}: {len(rows)} launches of output_proj_kernel, expected {len(PROJ_SHAPES) * PROJ_REPEAT}")
    print(f"# output_proj_kernel alone, f32 rows in, normalised rows out; median (min .. max) of {PROJ_REPEAT - 1} launches, from {Path(path).name}")
    for i, (B, H, E, bias) in enumerate(PROJ_SHAPES):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[i * PROJ_REPEAT + 1:(i + 1) * PROJ_REPEAT]]
        print(f"B={B} H={H} E={E} {'bias' if bias else 'no bias'}: output_proj_kernel {statistics.median(us):.1f} us a launch  ({min(us):.1f} .. {max(us):.1f}), "
              f"{(B + 15) // 16} workgroups")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--trace")
    a = ap.parse_args()
    if a.trace:
        return trace_mode(a.trace)
    rt = _native.Runtime(device=0)
    if a.kernels:
        kernels_mode(rt)
        rt.close()
        return
    rng = np.random.default_rng(0)
    print(f"# synthetic weights; median (min .. max) of {a.iters} calls")
    for name, cfg, pooling, E, bias in (("codet5p-110m (first token, E 256)", CODET5P, "first", 256, True), ("sentence-t5-base (mean, E 768)", ST5, "mean", 768, False)):
        enc = _native.Encoder(rt, cfg, synth_seed=1, pooling=pooling)
        enc.set_output_proj(*proj_weights(rng, cfg["hidden"], E, bias))
        assert enc.out_dim == E
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
    encs = [("bias table", _native.Encoder(rt, A_REL, synth_seed=1)), ("plain", _native.Encoder(rt, A_PLAIN, synth_seed=1)), ("ALiBi", _native.Encoder(rt, A_ALIBI, synth_seed=1))]
    for S in (128, 256, 512, 1024, 2048):
        B = 32768 // S
        ids = rng.integers(1, 1024, size=(B, S)).astype(np.int32)
        lens = np.full(B, S, np.int32)
        for i, form in enumerate(("padded", "packed")):
            t = {}
            for name, enc in encs:
                enc.set_path("small")  # the stand-alone pipeline for all three: the attention launches are what is read
                call = forms(enc, ids, lens)[i][1]
                call()
                t[name], n = attention_profile(rt, call)
            print(f"S={S} B={B} {form:6s} attention per launch, 12 heads of 64: bias table {t['bias table'] * 1e3:.1f} us, plain {t['plain'] * 1e3:.1f} us, "
                  f"ALiBi {t['ALiBi'] * 1e3:.1f} us; bias / plain = {t['bias table'] / t['plain']:.3f}, bias / ALiBi = {t['bias table'] / t['ALiBi']:.3f}", flush=True)
    for _, enc in encs:
        enc.close()
    rt.close()


if __name__ == "__main__":
    main()
