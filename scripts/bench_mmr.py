"""What an MMR search costs (sc_index_search_mmr_dev: the planner at width fetch_k + the candidate x candidate score matrix + the greedy
selection; on a trained IVF_FLAT index also the inverse position map), next to the plain top-fetch_k search it contains and to the
host way -- plain top-fetch_k, the candidates' vectors gathered and copied to the host, maximal marginal relevance in numpy (what
the LangChain vector stores do with fetch_k embeddings).

    python scripts/bench_mmr.py [--rows 10000000] [--dim 768] [--reps 20] [--queries 1,16,256,1024] [--fetch 32,128] [--kinds FLAT,IVF_FLAT]

L2, synthetic fill, k = 10, lambda = 0.5.  Per index kind, fetch_k and Q, alternating in one process on one index: the MMR call; the
plain search (default planner, exhaustive: nprobe = nlist) at fetch_k; the host way.  The host way needs the vectors by row id: it
gathers them on the device from a second copy of the corpus in row order (torch.index_select; rows * ld * 4 bytes more HBM -- lower
--rows where that does not fit), copies [Q, fetch_k, dim] to the host and runs one matrix product and k - 1 greedy steps per query.
A timed device call lies between two events on the runtime's stream; the host way is timed with the wall clock around everything it
does.  Median and min .. max of --reps calls after 3 warm-ups (the host way: --host-reps).  Reported: MMR minus plain top-fetch_k (what
the feature adds on the device) and host way minus plain top-fetch_k (what the host way adds), and whether both pick the same rows.
The inverse position map has no entry point of its own: its cost on IVF_FLAT shows as the difference of the added time between the
two kinds here, and as mmr_inverse_kernel in a rocprofv3 --kernel-trace --stats run of one batch (--one-batch Q runs exactly one MMR
call per kind at fetch_k = max of --fetch and exits).  One JSON line per case; the text above it is for reading.
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from semcode_amd import _native


def med(v):
    return round(statistics.median(v), 4)


def numpy_mmr(qv, V, k, lam):
    """One query, L2: V [F, dim] best first.  Indices of the picks."""
    vn = (V * V).sum(1)
    rel = -(vn - 2.0 * (V @ qv) + qv @ qv)
    red = -(vn[:, None] + vn[None, :] - 2.0 * (V @ V.T))
    picked = [0]
    m = np.full(len(V), -np.inf, dtype=np.float32)
    taken = np.zeros(len(V), dtype=bool)
    taken[0] = True
    for _ in range(1, min(k, len(V))):
        m = np.maximum(m, red[:, picked[-1]])
        v = np.where(taken, -np.inf, np.float32(lam) * rel - np.float32(1.0 - lam) * m)
        picked.append(int(np.argmax(v)))
        taken[picked[-1]] = True
    return picked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--queries", default="1,16,256,1024")
    ap.add_argument("--fetch", default="32,128")
    ap.add_argument("--kinds", default="FLAT,IVF_FLAT")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--one-batch", type=int, default=0)
    a = ap.parse_args()
    rows, dim, k, lam = a.rows, a.dim, a.k, a.lam
    queries = [int(q) for q in a.queries.split(",")]
    fetches = [int(f) for f in a.fetch.split(",")]
    stream = torch.cuda.Stream()
    rt = _native.Runtime(device=0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)
    maxq = max(queries + [a.one_batch])
    qs = _native.Index(rt, dim, metric="L2")
    qs.fill_synthetic(maxq, seed=1, first_row=rows + 777)
    allq = qs.get_rows(0, maxq)
    ld = qs.info()["ld"]
    qs.close()
    print(json.dumps({"device": rt.device_info(), "rows": rows, "dim": dim, "ld": ld, "k": k, "lambda": lam, "reps": a.reps, "host_reps": a.host_reps}), flush=True)
    od = torch.empty((maxq, max(fetches)), dtype=torch.float32, device=dev)
    orow = torch.empty((maxq, max(fetches)), dtype=torch.int64, device=dev)

    def timed(call):
        rt.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    copy = None
    if not a.one_batch:  # the host way's vectors by row id
        copy = torch.empty((rows, ld), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        rt.synth_fill_dev(copy.data_ptr(), rows, dim, ld, 0, 0)
        rt.synchronize()

    for kind in a.kinds.split(","):
        ix = _native.Index(rt, dim, metric="L2", kind=kind, nlist=a.nlist)
        ix.fill_synthetic(rows, seed=0)
        if kind == "IVF_FLAT":
            t0 = time.perf_counter()
            ix.train(niter=4, seed=0)
            print(f"[{kind}] trained {a.nlist} lists in {time.perf_counter() - t0:.1f} s", flush=True)
        if a.one_batch:
            Q, F = a.one_batch, max(fetches)
            qdev = torch.from_numpy(allq[:Q].copy()).to(dev)
            ix.search_mmr_dev(qdev.data_ptr(), Q, k, F, lam, 0, 0, od.data_ptr(), orow.data_ptr())
            rt.synchronize()
            print(json.dumps({"kind": kind, "one_batch": Q, "fetch_k": F, "mmr_stats": ix.last_mmr_stats()}), flush=True)
            ix.close()
            continue
        for F in fetches:
            for Q in queries:
                qdev = torch.from_numpy(allq[:Q].copy()).to(dev)

                def mmr():
                    ix.search_mmr_dev(qdev.data_ptr(), Q, k, F, lam, 0, 0, od.data_ptr(), orow.data_ptr())

                def plain():
                    ix.search_dev(qdev.data_ptr(), Q, F, od.data_ptr(), orow.data_ptr(), nprobe=a.nlist)

                def host_way():
                    rt.synchronize()
                    t0 = time.perf_counter()
                    plain()
                    rt.synchronize()
                    t1 = time.perf_counter()
                    r = orow.view(-1)[: Q * F].view(Q, F)
                    vec = copy.index_select(0, r.reshape(-1))[:, :dim].reshape(Q, F, dim).cpu().numpy()
                    rh = r.cpu().numpy()
                    t2 = time.perf_counter()
                    kept = np.stack([rh[i][numpy_mmr(allq[i], vec[i], k, lam)] for i in range(Q)])
                    t3 = time.perf_counter()
                    return (t3 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, kept

                mmr()
                rt.synchronize()
                mmr_rows = orow.view(-1)[: Q * k].view(Q, k).cpu().numpy().copy()
                stats = ix.last_mmr_stats()
                t_m, t_p, t_h, t_copy, t_np = [], [], [], [], []
                for rep in range(a.reps + 3):
                    if rep < a.host_reps + 3:  # first: it leaves the GPU idle while Python works, and the call after an idle gap runs slower
                        th, tc, tn, kept = host_way()
                    tp0 = timed(plain)  # (not recorded: both calls that are compared follow a busy GPU)
                    tm = timed(mmr)
                    tp = timed(plain)
                    path = ix.last_search_stats()["path"]
                    if rep >= 3:
                        t_m.append(tm); t_p.append(tp)
                        if rep < a.host_reps + 3:
                            t_h.append(th); t_copy.append(tc); t_np.append(tn)
                agree = sum(int(np.array_equal(x, g)) for x, g in zip(kept, mmr_rows))
                out = {"kind": kind, "Q": Q, "k": k, "fetch_k": F, "mmr_stats": stats, "mmr_ms": med(t_m), "mmr_ms_min_max": [round(min(t_m), 4), round(max(t_m), 4)],
                       "plain_fetch_ms": med(t_p), "plain_fetch_ms_min_max": [round(min(t_p), 4), round(max(t_p), 4)], "plain_fetch_path": path,
                       "mmr_minus_plain_ms": round(statistics.median(t_m) - statistics.median(t_p), 4),
                       "host_way_ms": med(t_h), "host_way_gather_copy_ms": med(t_copy), "host_way_numpy_ms": med(t_np),
                       "host_way_minus_plain_ms": round(statistics.median(t_h) - statistics.median(t_p), 4), "host_way_queries_equal_to_mmr": agree}
                print(f"[{kind} fetch_k={F} Q={Q}] mmr {out['mmr_ms']:.3f} ms ({min(t_m):.3f} .. {max(t_m):.3f}); plain top-{F} ({path}) {out['plain_fetch_ms']:.3f} ms "
                      f"({min(t_p):.3f} .. {max(t_p):.3f}): mmr - plain = {out['mmr_minus_plain_ms']:.3f} ms; host way {out['host_way_ms']:.3f} ms (gather + copy "
                      f"{out['host_way_gather_copy_ms']:.3f}, numpy {out['host_way_numpy_ms']:.3f}): host way - plain = {out['host_way_minus_plain_ms']:.3f} ms; "
                      f"{agree} of {Q} queries pick the same rows (the host way rounds differently)", flush=True)
                print(json.dumps(out), flush=True)
        ix.close()
    rt.close()


if __name__ == "__main__":
    main()
