"""What a grouped search costs (sc_index_search_grouped_dev: the planner at width W0 + selection kernel, exclusion rounds where W0
candidates do not hold k labels), next to the plain searches it is built on and to the host way (a wider top-k, repeats dropped in Python).

    python scripts/bench_grouped.py [--rows 10000000] [--dim 768] [--reps 20] [--queries 1,16,1024] [--masked-widths 10,64,256,1024]

FLAT, L2, synthetic fill, k = 10.  Two label sets:
  files     runs of consecutive rows with geometric sizes around 20 (the chunks of a file are neighbours);
  dominant  the same, but the 5 % of rows nearest query 0 share one label (one huge file holds everything that query likes best).
Per label set and Q, alternating in one process: the grouped call; the plain search (default planner) at k and at W0; the host way --
plain top-W0 to the host, first row of every label kept in Python -- with how many of the k sources it is left with.  For `dominant`
also the masked search of one query over the rows outside the dominant label at the widths of --masked-widths: what the scan of an
exclusion round costs on its own, by width.  A timed call lies between two events on the runtime's stream (every call ends its device work before the second event);
median and min .. max of --reps calls after 3 warm-ups.  The one-off label upload (sc_index_set_groups, host to device) is timed
with the wall clock.  One JSON line per case; the text above it is for reading.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", default="1,16,1024")
    ap.add_argument("--masked-widths", default="10,64,256,1024")
    a = ap.parse_args()
    rows, dim, k = a.rows, a.dim, a.k
    queries = [int(q) for q in a.queries.split(",")]
    stream = torch.cuda.Stream()
    rt = _native.Runtime(device=0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)
    ix = _native.Index(rt, dim, metric="L2")
    ix.fill_synthetic(rows, seed=0)
    ld = ix.info()["ld"]
    print(json.dumps({"device": rt.device_info(), "rows": rows, "dim": dim, "ld": ld, "k": k, "reps": a.reps}), flush=True)
    maxq = max(queries)
    qs = _native.Index(rt, dim, metric="L2")
    qs.fill_synthetic(maxq, seed=1, first_row=rows + 777)
    allq = qs.get_rows(0, maxq)
    qs.close()

    # label sets
    rng = np.random.default_rng(0)
    sizes = rng.geometric(1.0 / 20.0, size=rows // 10 + 1000)
    files = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)[:rows]
    assert len(files) == rows
    # squared distances of query 0 to every row, from the same generator that filled the index, a chunk at a time
    q0 = torch.from_numpy(allq[0]).to(dev)
    dist0 = torch.empty(rows, dtype=torch.float32, device=dev)
    chunk = 500_000
    buf = torch.empty((chunk, ld), dtype=torch.float32, device=dev)
    for first in range(0, rows, chunk):
        m = min(chunk, rows - first)
        torch.cuda.synchronize()
        rt.synth_fill_dev(buf.data_ptr(), m, dim, ld, 0, first)
        rt.synchronize()
        dist0[first:first + m] = ((buf[:m, :dim] - q0) ** 2).sum(1)
    del buf
    near = torch.topk(dist0, rows // 20, largest=False).indices.cpu().numpy()
    del dist0
    dominant = files.copy()
    dominant[near] = -1
    label_sets = {"files": files, "dominant": dominant}

    words_n = (rows + 31) // 32
    maxw = 1024
    od = torch.empty((maxq, maxw), dtype=torch.float32, device=dev)
    orow = torch.empty((maxq, maxw), dtype=torch.int64, device=dev)

    def timed(call):
        rt.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for name, labels in label_sets.items():
        t_up = []
        for _ in range(3):
            t0 = time.perf_counter()
            ix.set_groups(labels)
            t_up.append((time.perf_counter() - t0) * 1e3)
        print(f"[{name}] {len(np.unique(labels))} labels over {rows} rows; label upload (sc_index_set_groups, {rows * 4 / 1e6:.0f} MB) {min(t_up):.2f} ms best of 3", flush=True)
        print(json.dumps({"labels": name, "distinct_labels": int(len(np.unique(labels))), "upload_ms_best_of_3": round(min(t_up), 3)}), flush=True)
        outside = torch.from_numpy(_native.pack_allow(labels != -1, rows).view(np.int32).copy()).to(dev) if name == "dominant" else None
        for Q in queries:
            qdev = torch.from_numpy(allq[:Q].copy()).to(dev)
            ix.search_grouped_dev(qdev.data_ptr(), Q, k, 0, 0, od.data_ptr(), orow.data_ptr())
            rt.synchronize()
            W0 = ix.last_group_stats()["first_width"]
            grouped_rows = orow.view(-1)[: Q * k].view(Q, k).cpu().numpy().copy()

            def grouped():
                ix.search_grouped_dev(qdev.data_ptr(), Q, k, 0, 0, od.data_ptr(), orow.data_ptr())

            def plain_k():
                ix.search_dev(qdev.data_ptr(), Q, k, od.data_ptr(), orow.data_ptr())

            def plain_w0():
                ix.search_dev(qdev.data_ptr(), Q, W0, od.data_ptr(), orow.data_ptr())

            def host_way():
                rt.synchronize()
                t0 = time.perf_counter()
                plain_w0()
                rt.synchronize()
                r = orow.view(-1)[: Q * W0].view(Q, W0).cpu().numpy()
                kept = []
                for row in r:
                    _, first = np.unique(labels[row[row >= 0]], return_index=True)
                    kept.append(row[np.sort(first)[:k]])
                return (time.perf_counter() - t0) * 1e3, kept

            t_g, t_k, t_w, t_h = [], [], [], []
            for rep in range(a.reps + 3):
                th, kept = host_way()  # first: it leaves the GPU idle while Python works, and the call after an idle gap runs slower
                tk = timed(plain_k)
                tg = timed(grouped)  # ... so that the two calls that are compared both follow a busy GPU
                stats = ix.last_group_stats()
                tw = timed(plain_w0)
                path_w0 = ix.last_search_stats()["path"]
                if rep >= 3:
                    t_g.append(tg); t_k.append(tk); t_w.append(tw); t_h.append(th)
            left = [len(x) for x in kept]
            agree = sum(int(len(x) == k and np.array_equal(x, g)) for x, g in zip(kept, grouped_rows))
            out = {"labels": name, "Q": Q, "k": k, "W0": W0, "group_stats": stats, "grouped_ms": med(t_g), "grouped_ms_min_max": [round(min(t_g), 4), round(max(t_g), 4)],
                   "plain_k_ms": med(t_k), "plain_W0_ms": med(t_w), "plain_W0_ms_min_max": [round(min(t_w), 4), round(max(t_w), 4)], "plain_W0_path": path_w0,
                   "grouped_minus_plain_W0_ms": round(statistics.median(t_g) - statistics.median(t_w), 4),
                   "host_way_ms": med(t_h), "host_way_sources_left_mean": round(sum(left) / Q, 2), "host_way_sources_left_min": min(left),
                   "host_way_queries_equal_to_grouped": agree}
            line = (f"[{name} Q={Q}] grouped {out['grouped_ms']:.3f} ms ({min(t_g):.3f} .. {max(t_g):.3f}), {stats['queries_continued']} queries continued, {stats['rounds']} exclusion rounds; "
                    f"plain top-{k} {out['plain_k_ms']:.3f} ms, plain top-{W0} ({path_w0}) {out['plain_W0_ms']:.3f} ms ({min(t_w):.3f} .. {max(t_w):.3f}): grouped - plain top-{W0} = "
                    f"{out['grouped_minus_plain_W0_ms']:.3f} ms; host way {out['host_way_ms']:.3f} ms, {out['host_way_sources_left_mean']:.1f} of {k} sources left (min {min(left)}), "
                    f"{agree} of {Q} queries equal to the grouped answer")
            print(line, flush=True)
            print(json.dumps(out), flush=True)
        if outside is not None:  # the scan of an exclusion round on its own: one query over the rows outside the dominant label, by width
            qdev = torch.from_numpy(allq[:1].copy()).to(dev)
            m = int((labels != -1).sum())
            for W in [int(w) for w in a.masked_widths.split(",")]:
                t_m = [timed(lambda: ix.search_masked_dev(qdev.data_ptr(), 1, W, outside.data_ptr(), words_n, od.data_ptr(), orow.data_ptr())) for _ in range(a.reps + 3)][3:]
                print(f"[{name}] masked top-{W} of one query over the {m} rows outside the dominant label: {med(t_m):.3f} ms ({min(t_m):.3f} .. {max(t_m):.3f})", flush=True)
                print(json.dumps({"labels": name, "masked_width": W, "masked_rows": m, "masked_ms": med(t_m), "masked_ms_min_max": [round(min(t_m), 4), round(max(t_m), 4)]}), flush=True)
    ix.close()
    rt.close()


if __name__ == "__main__":
    main()
