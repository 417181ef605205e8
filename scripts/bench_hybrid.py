"""What the lexical scan and a hybrid search cost (sc_index_search_lexical_dev, sc_index_search_hybrid_dev), next to the plain dense
top-fetch_k search a hybrid call contains, and what a mutation of the term rows costs.

    python scripts/bench_hybrid.py [--rows 10000000] [--dim 768] [--slots 128] [--reps 10] [--queries 1,16,256] [--k 10] [--fetch 40] > profiles/hybrid_bench_10Mx768.log

IP, synthetic fill.  The term rows are synthetic: a block of 262 144 rows drawn from a Zipf(1) vocabulary of 20 000 terms with lengths
uniform in [slots / 4, slots], sorted, uploaded over and over in ranges of that many rows until every row has one (the scan's cost does
not depend on the repetition; the upload is timed).  A query has 8 terms; "mixed": half of them among the 200 most common, so that nearly every row holds one and takes the scan's
slow path; "rare": none of them.  The weights are the IDF from sc_index_lex_stats.  Timed device calls lie between two events on the runtime's stream; median and min .. max of --reps
calls after 3 warm-ups.  The scan's rate is rows * 2 * slots bytes * passes / time of the whole call (prep, scan and merge kernels), so
it understates the scan kernel alone; a pass serves 16 queries.  One JSON line per case; the text above it is for reading."""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from semcode_amd import _native

BLOCK = 262144


def med(v):
    return round(statistics.median(v), 4)


def zipf_block(rng, rows, slots, vocab):
    p = 1.0 / np.arange(1, vocab.size + 1)
    p /= p.sum()
    terms = vocab[rng.choice(vocab.size, size=(rows, slots), p=p)]
    dl = rng.integers(slots // 4, slots + 1, size=rows)
    terms[np.arange(slots)[None, :] >= dl[:, None]] = 0xFFFF
    terms.sort(axis=1)
    return terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", default="1,16,256")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch", type=int, default=40)
    a = ap.parse_args()
    rows, dim, T, k, F = a.rows, a.dim, a.slots, a.k, a.fetch
    queries = [int(q) for q in a.queries.split(",")]
    stream = torch.cuda.Stream()
    rt = _native.Runtime(device=0, stream=stream.cuda_stream)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    vocab = np.sort(rng.choice(0xFFFF, size=20000, replace=False)).astype(np.uint16)
    ix = _native.Index(rt, dim, metric="IP")
    ix.fill_synthetic(rows, seed=0)
    print(json.dumps({"device": rt.device_info(), "rows": rows, "dim": dim, "slots": T, "k": k, "fetch_k": F, "reps": a.reps}), flush=True)

    # ---- term rows, uploaded in ranges
    block = zipf_block(rng, min(BLOCK, rows), T, vocab)
    t_up = []
    for first in range(0, rows, BLOCK):
        n = min(BLOCK, rows - first)
        t0 = time.perf_counter()
        ix.set_terms(block[:n], first_row=first)
        t_up.append((time.perf_counter() - t0) * 1e3 / n * BLOCK)
    print(f"[upload] {rows} term rows of {T} slots in ranges of {BLOCK}: median {med(t_up):.2f} ms per {BLOCK} rows "
          f"({BLOCK * 2 * T / statistics.median(t_up) / 1e6:.2f} GB/s, host wall clock, first range includes the allocation)", flush=True)
    t0 = time.perf_counter()
    st = ix.lex_stats()
    t_stats = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ix.lex_stats()
    t_cached = (time.perf_counter() - t0) * 1e3
    n_rows, df = st["rows"], st["df"].astype(np.float64)
    idf = np.log(1.0 + (n_rows - df + 0.5) / (df + 0.5)).astype(np.float32)
    avgdl = float(np.float32(st["sum_dl"] / n_rows))
    print(json.dumps({"case": "upload", "ms_per_block": med(t_up), "block_rows": BLOCK, "lex_stats_first_ms": round(t_stats, 3), "lex_stats_cached_ms": round(t_cached, 3),
                      "sum_dl": st["sum_dl"], "avgdl": avgdl}), flush=True)
    # ---- a mutation: 128 rows overwritten (an upsert batch), then the statistics again
    t_mut, t_restat = [], []
    for rep in range(5):
        first = int(rng.integers(0, rows - 128))
        t0 = time.perf_counter()
        ix.set_terms(block[rep * 128:rep * 128 + 128], first_row=first)
        t1 = time.perf_counter()
        ix.lex_stats()
        t_restat.append((time.perf_counter() - t1) * 1e3)
        t_mut.append((t1 - t0) * 1e3)
    print(f"[mutation] 128 term rows overwritten: {med(t_mut):.3f} ms; the statistics after it: {med(t_restat):.2f} ms (host wall clock)", flush=True)
    print(json.dumps({"case": "mutation", "set_terms_128_rows_ms": med(t_mut), "lex_stats_after_ms": med(t_restat)}), flush=True)

    # ---- queries: "mixed" = 4 of the 8 terms among the 200 most common (nearly every row holds one: the scan's slow path), "rare" = none
    maxq = max(queries)
    qsets = {}
    for mix in ("mixed", "rare"):
        qt = np.full((maxq, 32), 0xFFFF, dtype=np.uint16)
        qw = np.zeros((maxq, 32), dtype=np.float32)
        for q in range(maxq):
            common = rng.choice(vocab[:200], 4, replace=False) if mix == "mixed" else rng.choice(vocab[2000:], 4, replace=False)
            ts = np.unique(np.concatenate([common, rng.choice(vocab[200:2000], 4, replace=False)]))
            qt[q, :8], qw[q, :8] = ts, idf[ts]
        qsets[mix] = (qt, qw)
    nt = np.full(maxq, 8, dtype=np.int32)
    qs = _native.Index(rt, dim, metric="IP")
    qs.fill_synthetic(maxq, seed=1, first_row=rows + 777)
    allq = torch.from_numpy(qs.get_rows(0, maxq)).to(dev)
    qs.close()
    tn = torch.from_numpy(nt).to(dev)
    dsets = {mix: (torch.from_numpy(qt.view(np.int16)).to(dev), torch.from_numpy(qw).to(dev)) for mix, (qt, qw) in qsets.items()}
    od = torch.empty((maxq, max(F, k)), dtype=torch.float32, device=dev)
    orow = torch.empty((maxq, max(F, k)), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def timed(call):
        rt.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for mix, Q in [(m, q) for m in dsets for q in queries]:
        tt, tw = dsets[mix]

        def lexical(width=k):
            ix.search_lexical_dev(Q, width, tt.data_ptr(), tw.data_ptr(), tn.data_ptr(), 1.2, 0.75, avgdl, 0, 0, od.data_ptr(), orow.data_ptr())

        def hybrid():
            ix.search_hybrid_dev(allq.data_ptr(), Q, k, F, tt.data_ptr(), tw.data_ptr(), tn.data_ptr(), 1.2, 0.75, avgdl, 60, 1.0, 1.0, 0, 0, od.data_ptr(), orow.data_ptr())

        def plain():
            ix.search_dev(allq.data_ptr(), Q, F, od.data_ptr(), orow.data_ptr())

        t_l, t_lf, t_h, t_p = [], [], [], []
        for rep in range(a.reps + 3):
            tl, tlf, th, tp = timed(lexical), timed(lambda: lexical(F)), timed(hybrid), timed(plain)
            path = ix.last_search_stats()["path"]
            if rep >= 3:
                t_l.append(tl); t_lf.append(tlf); t_h.append(th); t_p.append(tp)
        lexical()
        ls = ix.last_lex_stats()
        passes = ls["passes"]
        gbs = ls["bytes_per_pass"] * passes / statistics.median(t_l) / 1e6
        out = {"case": "search", "terms": mix, "Q": Q, "k": k, "fetch_k": F, "lex_stats": ls, "lexical_ms": med(t_l), "lexical_ms_min_max": [round(min(t_l), 4), round(max(t_l), 4)],
               "lexical_GBps_on_rows_x_2T": round(gbs, 1), "lexical_fraction_of_8TBps": round(gbs / 8000.0, 3), "lexical_at_fetch_k_ms": med(t_lf),
               "hybrid_ms": med(t_h), "hybrid_ms_min_max": [round(min(t_h), 4), round(max(t_h), 4)], "plain_fetch_ms": med(t_p),
               "plain_fetch_path": path, "hybrid_minus_plain_ms": round(statistics.median(t_h) - statistics.median(t_p), 4)}
        print(f"[{mix} Q={Q}] lexical top-{k}: {out['lexical_ms']:.3f} ms ({min(t_l):.3f} .. {max(t_l):.3f}) in {passes} pass(es) = {gbs:.0f} GB/s on rows x 2T "
              f"({gbs / 8000.0:.2f} of 8 TB/s); at width {F}: {out['lexical_at_fetch_k_ms']:.3f} ms; hybrid {out['hybrid_ms']:.3f} ms, plain dense top-{F} "
              f"{out['plain_fetch_ms']:.3f} ms: hybrid - plain = {out['hybrid_minus_plain_ms']:.3f} ms", flush=True)
        print(json.dumps(out), flush=True)
    ix.close()
    rt.close()


if __name__ == "__main__":
    main()
