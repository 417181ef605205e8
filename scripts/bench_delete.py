"""What a delete costs (sc_index_delete_rows: in-place compaction) next to the only alternative without it -- rebuilding the
collection from its survivors through the public API -- and what the first search after a delete pays.

    python scripts/bench_delete.py [--rows 10000000] [--dim 768] [--nlist 128] [--reps 5] [--no-rebuild]

FLAT and trained IVF_FLAT, every shadow built before each delete (a search in every mode that owns one).  Two delete sets:
1 % of the rows as 50 contiguous runs (a repository's worth of chunks) and a random 30 %.  Each delete is timed with device
events on the runtime's stream around the call (the call ends in a stream synchronise, so this is its wall time on the device
clock) and by the host clock; median of --reps after one warm-up, the index re-filled (and its lists re-installed) between
repetitions.  bytes_moved comes from sc_index_last_delete_stats; every moved byte is read once and written once, so the
achieved rate is 2 x bytes_moved / time, reported as a share of the 6.3 TB/s of achievable HBM streaming.
One JSON line per (index kind, delete set) at the end of its block; the text above it is for reading.
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

HBM_STREAM = 6.3e12  # bytes/s, achievable streaming rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=128)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--niter", type=int, default=4)
    ap.add_argument("--kinds", default="FLAT,IVF_FLAT")
    ap.add_argument("--no-rebuild", action="store_true")
    a = ap.parse_args()
    rows, dim, k = a.rows, a.dim, 10
    stream = torch.cuda.Stream()
    rt = _native.Runtime(device=0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)
    print(json.dumps({"device": rt.device_info(), "rows": rows, "dim": dim, "nlist": a.nlist, "nprobe": a.nprobe, "reps": a.reps}), flush=True)
    qs = _native.Index(rt, dim, metric="L2")
    qs.fill_synthetic_clustered(1024, seed=0, nclusters=1024, spread=0.5, first_row=rows + 777)
    allq = qs.get_rows(0, 1024)
    qs.close()
    qdev = {Q: torch.from_numpy(allq[:Q].copy()).to(dev) for Q in (1, 1024)}
    od = torch.empty((1024, k), dtype=torch.float32, device=dev)
    orow = torch.empty((1024, k), dtype=torch.int64, device=dev)

    def search(ix, Q):
        rt.synchronize()
        t0 = time.perf_counter()
        ix.search_dev(qdev[Q].data_ptr(), Q, k, od.data_ptr(), orow.data_ptr(), nprobe=a.nprobe)
        rt.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rng = np.random.default_rng(0)
    run_len = max(1, rows // 100 // 50)
    starts = (np.arange(50, dtype=np.int64) * (rows // 50)) + rows // 200
    sets = {
        "1pct_50runs": np.concatenate([np.arange(s, s + run_len, dtype=np.int64) for s in starts]),
        "random_30pct": np.sort(rng.choice(rows, size=(3 * rows) // 10, replace=False)).astype(np.int64),
    }

    for kind in a.kinds.split(","):
        ix = _native.Index(rt, dim, metric="L2", kind=kind, nlist=a.nlist)
        cent = assign = None

        def refill():
            ix.fill_synthetic_clustered(rows, seed=0, nclusters=1024, spread=0.5)
            if kind == "IVF_FLAT":
                ix.set_ivf(cent, assign)
            # every shadow: bf16 and int8 of the exhaustive path, the centred int8 of the list probe
            for mode, bits in (("batched", 16), ("batched", 8)) + ((("ivf_coarse", 0),) if kind == "IVF_FLAT" else ()):
                ix.set_search_mode(mode)
                ix.set_coarse_stage(bits)
                search(ix, 1024)
            ix.set_search_mode("auto")
            ix.set_coarse_stage(0)
            for Q in (1, 1024):
                search(ix, Q)

        ix.fill_synthetic_clustered(rows, seed=0, nclusters=1024, spread=0.5)
        if kind == "IVF_FLAT":
            t0 = time.perf_counter()
            ix.train(niter=a.niter)
            cent, assign = ix.ivf_info()["centroids"].copy(), ix.ivf_assignments().copy()
            print(f"[{kind}] k-means + list build: {time.perf_counter() - t0:.1f} s", flush=True)
        refill()
        steady_full = {Q: statistics.median(search(ix, Q) for _ in range(5)) for Q in (1, 1024)}
        print(f"[{kind}] steady search on {rows} rows: Q=1 {steady_full[1]:.3f} ms, Q=1024 {steady_full[1024]:.3f} ms ({ix.last_search_stats()['path']})", flush=True)

        for name, dele in sets.items():
            t_dev, t_host, first, steady, stats = [], [], {1: [], 1024: []}, {1: [], 1024: []}, None
            for rep in range(a.reps + 1):
                if rep or name != next(iter(sets)):
                    refill()
                rt.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                t0 = time.perf_counter()
                ix.delete_rows(dele)
                e1.record(stream)
                e1.synchronize()
                th = (time.perf_counter() - t0) * 1e3
                td = e0.elapsed_time(e1)
                stats = ix.last_delete_stats()
                Q = 1024 if rep % 2 else 1
                f = search(ix, Q)
                path = ix.last_search_stats()["path"]
                s = statistics.median(search(ix, Q) for _ in range(3))
                tag = "warm-up" if rep == 0 else f"rep {rep}"
                print(f"[{kind}] {name} {tag}: delete {td:.2f} ms (host clock {th:.2f}), first search Q={Q} {f:.3f} ms, steady {s:.3f} ms ({path}), {stats}", flush=True)
                assert stats["shadows_dropped"] == 0, stats
                if rep:
                    t_dev.append(td)
                    t_host.append(th)
                    first[Q].append(f)
                    steady[Q].append(s)
            med = statistics.median(t_dev)
            rate = 2.0 * stats["bytes_moved"] / (med * 1e-3)
            out = {"kind": kind, "delete_set": name, "rows": rows, "dim": dim, "deleted": int(len(dele)), "delete_ms_median": round(med, 3),
                   "delete_ms_all": [round(t, 3) for t in t_dev], "delete_ms_host_clock_median": round(statistics.median(t_host), 3),
                   "rows_moved": stats["rows_moved"], "bytes_moved": stats["bytes_moved"], "achieved_bytes_per_s": round(rate, 1),
                   "share_of_6.3TBps": round(rate / HBM_STREAM, 4), "shadows_kept": stats["shadows_kept"], "shadows_dropped": stats["shadows_dropped"]}
            for Q in (1, 1024):
                if first[Q]:
                    out[f"first_search_q{Q}_ms"] = round(statistics.median(first[Q]), 3)
                    out[f"steady_search_q{Q}_ms"] = round(statistics.median(steady[Q]), 3)
                    out[f"first_search_q{Q}_samples"] = len(first[Q])
            if not a.no_rebuild:
                # the alternative without a delete: survivors out through get_rows, into a new index, lists re-installed, first search
                # (which builds every shadow it needs again).  The index at hand holds exactly the survivors: read them from it.
                n2 = len(ix)
                a2 = ix.ivf_assignments().copy() if kind == "IVF_FLAT" else None
                rt.synchronize()
                t0 = time.perf_counter()
                nx = _native.Index(rt, dim, metric="L2", kind=kind, nlist=a.nlist)
                nx.reserve(n2)
                step = 1 << 20
                for r0 in range(0, n2, step):
                    nx.add(ix.get_rows(r0, min(step, n2 - r0)))
                t_copy = time.perf_counter() - t0
                if kind == "IVF_FLAT":
                    nx.set_ivf(cent, a2)
                t_lists = time.perf_counter() - t0 - t_copy
                f2 = search(nx, 1024)
                t_all = (time.perf_counter() - t0) * 1e3
                nx.close()
                mine = med + out.get("first_search_q1024_ms", 0.0)
                out.update(rebuild_ms=round(t_all, 1), rebuild_copy_ms=round(t_copy * 1e3, 1), rebuild_lists_ms=round(t_lists * 1e3, 1), rebuild_first_search_q1024_ms=round(f2, 3),
                           delete_plus_first_search_q1024_ms=round(mine, 3), rebuild_over_delete=round(t_all / mine, 1))
                print(f"[{kind}] {name}: rebuild from the survivors {t_all:.0f} ms (rows out and in {t_copy * 1e3:.0f}, lists {t_lists * 1e3:.0f}, first search {f2:.1f}) "
                      f"against delete + first search {mine:.2f} ms: {t_all / mine:.0f}x", flush=True)
            print(json.dumps(out), flush=True)
        ix.close()
    rt.close()


if __name__ == "__main__":
    main()
