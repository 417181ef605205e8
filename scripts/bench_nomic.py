"""Encoder throughput of the three model families at the ingest shape (256 chunks x 256 tokens, 12 layers, base size, synthetic
weights on device), and the A/B that decides how the batch pipeline of a rotary model rotates Q and K:

    python scripts/bench_nomic.py [--steps 20] [--warmup 3] [--reps 3]

Per repetition, in the same order each time: BERT-base (orientation: nomic does 1.33x its GEMM FLOPs per layer), jina-v2 base
shape (alibi + geglu: THE YARDSTICK -- the same GEMM shapes and the same unfused gate kernel, ALiBi in place of rotary), nomic
with rope_fused 0 (stand-alone rope_qk_kernel) and rope_fused 1 (rotation in the QKV epilogue).  Timing as bench.py's embed leg:
device-resident ids, `steps` forwards between two synchronisations, after `warmup` forwards.

Decision rule (no number fixed in advance): the fused epilogue becomes the default only if it beats the stand-alone kernel by
more than the run-to-run spread of the repetitions; otherwise the stand-alone kernel stays and the fused form remains an option."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=256)
    ap.add_argument("--only", default="", help="comma list of legs (bert,jina,nomic_rope0,nomic_rope1): e.g. for a kernel trace")
    args = ap.parse_args()
    import torch

    from semcode_amd import _native

    rt = _native.Runtime(device=0)
    B, S = args.batch, args.seq
    base = dict(_native.BERT_BASE)
    nomic = dict(base, max_pos=2048, rotary=True, swiglu=True, rope_theta=1000.0)
    legs = [("bert", base, -1), ("jina", dict(base, alibi=True, geglu=True), -1), ("nomic_rope0", nomic, 0), ("nomic_rope1", nomic, 1)]
    if args.only:
        legs = [l for l in legs if l[0] in args.only.split(",")]
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(1000, 30000, (B, S), generator=g, dtype=torch.int32).to("cuda:0")
    lens = torch.full((B,), S, dtype=torch.int32, device="cuda:0")
    out = torch.empty((B, 768), dtype=torch.float32, device="cuda:0")
    encs = {}
    for name, cfg, _ in legs:
        if id(cfg) not in encs:
            encs[id(cfg)] = _native.Encoder(rt, cfg, weights=None, synth_seed=0)
    rate = {name: [] for name, _, _ in legs}
    for rep in range(args.reps):
        for name, cfg, fused in legs:
            enc = encs[id(cfg)]
            _native.diag_set_option("rope_fused", fused)
            step = lambda: enc.embed_ids_dev(ids.data_ptr(), lens.data_ptr(), B, S, out.data_ptr())
            for _ in range(args.warmup):
                step()
            rt.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            rt.synchronize()
            dt = time.perf_counter() - t0
            assert bool(torch.isfinite(out).all()), f"{name}: non-finite output"
            rate[name].append(B * args.steps / dt)
            print(f"rep {rep} {name:12s} {1e3 * dt / args.steps:8.3f} ms/step  {rate[name][-1]:10.1f} chunks/s", flush=True)
    _native.diag_set_option("rope_fused", -1)
    med = {n: sorted(v)[len(v) // 2] for n, v in rate.items()}
    spread = {n: (max(v) - min(v)) / med[n] for n, v in rate.items()}
    for n in rate:
        print(f"{n:12s} median {med[n]:10.1f} chunks/s  spread {100 * spread[n]:.2f} % of {len(rate[n])} repetitions")
    if "nomic_rope0" in med and "nomic_rope1" in med:
        gain = med["nomic_rope1"] / med["nomic_rope0"] - 1.0
        noise = max(spread["nomic_rope0"], spread["nomic_rope1"])
        print(f"fused over stand-alone: {100 * gain:+.2f} %  (run-to-run spread {100 * noise:.2f} %)")
        print("decision: " + ("fused epilogue is faster beyond the spread -> default" if gain > noise else
                              "not faster beyond the spread -> the stand-alone kernel is the default, the fused epilogue stays behind the option"))
        if "jina" in med:
            for n in ("nomic_rope0", "nomic_rope1"):
                print(f"{n} / jina = {med[n] / med['jina']:.4f}")
    if "bert" in med and "jina" in med:
        print(f"jina / bert = {med['jina'] / med['bert']:.4f}")
    for e in encs.values():
        e.close()
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
