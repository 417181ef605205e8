"""Strip lengths of the QKV / FFN1 GEMMs on the encoder step, interleaved in ONE process (profiles/strip_ab.log).

    python scripts/strip_sweep.py [--batch 256] [--seq 256] [--steps 40] [--rounds 7] [--qkv 3,9] [--ffn 3,4,6,12]

Every candidate forces L on the launches of one shape only ("gemm_strip_n" = N, "gemm_strip" = L; every other launch runs
per tile); "off" runs the per-tile kernel everywhere, "auto" the shape rule.  The pooled outputs of every
candidate are compared with "off" bit for bit first.  Then ROUNDS rounds visit the candidates in turn, STEPS synchronised steps each,
wall clock.  The gate per candidate (the one scripts/ab_encoder.sh's runs are held to): its slowest round beats the fastest "off"
round, and its median gain is at least twice the larger of the two spreads (max - min)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semcode_amd import _native as nv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--seq", type=int, default=256)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--qkv", default="3,9")
ap.add_argument("--ffn", default="3,4,6,12")
args = ap.parse_args()

rt = nv.Runtime(0)
B, S = args.batch, args.seq
enc = nv.Encoder(rt, dict(nv.BERT_BASE), weights=None, synth_seed=0)
g = torch.Generator(device="cpu").manual_seed(1)
ids = torch.randint(1000, 30000, (B, S), generator=g, dtype=torch.int32).cuda()
lens = torch.full((B,), S, dtype=torch.int32, device="cuda")
out = torch.empty((B, 768), dtype=torch.float32, device="cuda")
configs = [("off", 0, 0), ("auto", 0, -1)]
configs += [(f"qkv{L}", 2304, int(L)) for L in args.qkv.split(",") if L]
configs += [(f"ffn{L}", 3072, int(L)) for L in args.ffn.split(",") if L]


def select(c):
    nv.diag_set_option("gemm_strip_n", c[1])
    nv.diag_set_option("gemm_strip", c[2])


def step():
    enc.embed_ids_dev(ids.data_ptr(), lens.data_ptr(), B, S, out.data_ptr())


print(f"{B} chunks x {S} tokens (M = {B * S}); shape rule here: QKV {nv.diag_gemm_strip(B * S, 2304, 768)}, FFN1 {nv.diag_gemm_strip(B * S, 3072, 768)} tiles per strip")
ref = None
for c in configs:
    select(c)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    o = out.cpu().numpy().tobytes()
    ref = o if ref is None else ref
    print(f"{c[0]:8s} output {'bit-identical to off' if o == ref else 'DIFFERENT'}", flush=True)
    if o != ref:
        sys.exit(3)
res = {c[0]: [] for c in configs}
for r in range(args.rounds):
    for c in configs:
        select(c)
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        res[c[0]].append(1e3 * (time.perf_counter() - t0) / args.steps)
off = np.array(res["off"])
print(f"ms per step, {args.rounds} interleaved rounds of {args.steps} steps")
for k, v in res.items():
    v = np.array(v)
    gain = np.median(off) - np.median(v)
    spread = max(v.max() - v.min(), off.max() - off.min())
    gate = "" if k == "off" else ("  gate: pass" if v.max() < off.min() and gain >= 2 * spread else "  gate: no")
    print(f"{k:8s} median {np.median(v):7.3f}  min {v.min():7.3f}  max {v.max():7.3f}  vs off {100 * (np.median(v) / np.median(off) - 1):+6.2f} %{gate}   rounds: "
          + " ".join(f"{x:.3f}" for x in v), flush=True)
select(("", 0, -1))
enc.close()
rt.close()
