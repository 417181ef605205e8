"""What the token vectors' trip through the host costs a late-store ingest: today's path (sc_encoder_embed_tokens, one boolean mask per
chunk, sc_index_put_tokens) against the hand-over (sc_encoder_embed_tokens_into: the token head writes into the index's token pool), in
one process, alternating, at both storage formats.

    python scripts/bench_late_ingest.py [--passages 4096] [--runs 3] [--budget 65536] > profiles/late_ingest_bench.log

Setup.  A BERT-base-shaped ColBERT (12 layers, synthetic weights, W = 128); --passages passages of log-uniform 40 .. 500 tokens, a seeded
10 % of the token positions dropped by keep flags; batches cut by cut_packed under --budget token rows, as MI355XLateReranker cuts them;
an index of that many rows with its token pool reserved in advance, fresh for every run.  What is timed is everything behind the tokenizer
(the ids and flags of every batch are made before): per batch the forward, the vectors' way into the store and the Python between the
two -- for the host path the statements of MI355XLateReranker.embed_document_tokens(kept_only=True) and Index.put_tokens.  A run ends in a
device synchronise (both paths' last call does).  After one warm-up run of each path and format the two paths alternate --runs times
each; every path is reported with its own spread (min .. max over its runs), and the stored bits of the two paths are compared once.

Ceiling.  Encoder.embed_packed over the same batches in the same process: the forward with its pooled rows downloaded, no token head.

The one synchronisation.  sc_encoder_embed_tokens_into waits for the stream once, at its end.  Its share of a call is reported as the
call's wall time minus the host's time to ENQUEUE the same forward (Encoder.embed_packed_into(..., wait=False) on the same batch: plan,
upload and every launch of the 12 layers, no wait): the time the host sits in the wait, which an asynchronous form could hand back.
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
from semcode_amd.embeddings.providers import cut_packed  # noqa: E402

W = 128


def make_batches(enc, n, budget, seed):
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(40), np.log(500), size=n)).astype(np.int64).clip(40, 500)
    rows_of = lambda l: enc.packed_rows(np.concatenate(([0], np.cumsum(l))))  # noqa: E731
    batches = []
    for a, b in cut_packed(lens, budget, rows_of):
        off = np.concatenate(([0], np.cumsum(lens[a:b]))).astype(np.int64)
        ids = rng.integers(1000, 30000, size=int(off[-1])).astype(np.int32)
        keep = (rng.random(int(off[-1])) >= 0.10).astype(np.uint8)
        batches.append(dict(rows=np.arange(a, b, dtype=np.int64), ids=ids, off=off, keep=keep))
    return lens, batches


def host_path(enc, ix, batches, fmt):
    for c in batches:
        ids, off = c["ids"], c["off"]
        vec, counts = enc.embed_tokens(ids, off, expand_id=-1)
        parts = np.split(vec, np.cumsum(counts)[:-1])
        keep = c["keep"].astype(bool)
        parts = [p[keep[off[i]:off[i + 1]]] for i, p in enumerate(parts)]
        ix.put_tokens(c["rows"], list(parts), fmt=fmt)


def handover(enc, ix, batches, fmt):
    for c in batches:
        enc.embed_tokens_into(c["ids"], c["off"], c["keep"], ix, c["rows"], fmt)


def fresh_index(rt, hidden, n, tokens):
    ix = _native.Index(rt, hidden, metric="IP")
    ix.fill_synthetic(n, seed=0)
    ix.reserve_tokens(tokens)
    return ix


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--budget", type=int, default=65536)
    ap.add_argument("--layers", type=int, default=12)
    a = ap.parse_args()
    rt = _native.Runtime(device=0)
    print(f"# bench_late_ingest: {_native.lib().sc_version().decode()}, {rt.device_info()}", flush=True)
    cfg = dict(_native.BERT_BASE, max_pos=512, layers=a.layers)
    enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)
    rng = np.random.default_rng(29)
    enc.set_token_head((rng.standard_normal((W, cfg["hidden"])) / np.sqrt(cfg["hidden"])).astype(np.float32))
    n = a.passages
    lens, batches = make_batches(enc, n, a.budget, seed=31)
    tokens = int(lens.sum())
    kept = int(sum(int(c["keep"].sum()) for c in batches))
    print(f"[setup] {n} passages, {tokens} tokens (log-uniform 40..500), {kept} kept ({kept / tokens:.3f}), {len(batches)} batches under {a.budget} rows, "
          f"{cfg['layers']} layers, hidden {cfg['hidden']}, W = {W}; f32 vectors through the host: {tokens * W * 4 / 2**20:.0f} MiB down, {kept * W * 4 / 2**20:.0f} MiB up", flush=True)
    paths = (("host", host_path), ("handover", handover))

    def one_run(fn, fmt, keep_index=False):
        ix = fresh_index(rt, cfg["hidden"], n, kept + 1024)
        t0 = time.perf_counter()
        fn(enc, ix, batches, fmt)
        dt = time.perf_counter() - t0
        if keep_index:
            return dt, ix
        ix.close()
        return dt, None

    for fmt in ("f32", "bf16"):
        stored = {}
        for name, fn in paths:  # warm-up, and the stored bits of the two paths
            _, ix = one_run(fn, fmt, keep_index=True)
            stored[name] = ix.get_tokens(np.arange(n))
            assert ix.token_stats()["live"] == kept and ix.token_stats()["dead"] == 0
            ix.close()
        same = np.array_equal(stored["host"][0], stored["handover"][0]) and np.array_equal(stored["host"][1].view(np.uint32), stored["handover"][1].view(np.uint32))
        print(f"[{fmt}] stored counts and bits of the two paths identical: {same}", flush=True)
        del stored
        times = {name: [] for name, _ in paths}
        for _ in range(a.runs):  # alternating
            for name, fn in paths:
                times[name].append(one_run(fn, fmt)[0])
        for name, _ in paths:
            t = times[name]
            med = statistics.median(t)
            print(f"[{fmt}] {name:8s}: median {med:.3f} s = {n / med:.0f} passages/s, {tokens / med / 1e6:.2f} M tokens/s; runs "
                  + ", ".join(f"{x:.3f}" for x in t) + f" s (min {n / max(t):.0f} .. max {n / min(t):.0f} passages/s)", flush=True)
        h, d = times["host"], times["handover"]
        print(f"[{fmt}] hand-over over host path: {statistics.median(h) / statistics.median(d):.2f} x by the medians; slowest hand-over run {max(d):.3f} s against fastest "
              f"host run {min(h):.3f} s -> beyond the host path's own spread ({min(h):.3f} .. {max(h):.3f} s): {max(d) < min(h)}", flush=True)

    # ---- the ceiling: the dense forward over the same batches
    def dense():
        for c in batches:
            enc.embed_packed(c["ids"], c["off"])

    dense()
    t = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        dense()
        t.append(time.perf_counter() - t0)
    med = statistics.median(t)
    print(f"[ceiling] embed_packed over the same batches: median {med:.3f} s = {n / med:.0f} passages/s; runs " + ", ".join(f"{x:.3f}" for x in t) + " s", flush=True)

    # ---- the one synchronisation per call: wall time of a call against the enqueue time of the same forward
    ix = fresh_index(rt, cfg["hidden"], n, 2 * kept + 1024)
    handover(enc, ix, batches, "bf16")
    wall, enq = [], []
    for c in batches:
        t0 = time.perf_counter()
        enc.embed_tokens_into(c["ids"], c["off"], c["keep"], ix, c["rows"], "bf16")
        wall.append(time.perf_counter() - t0)
    for c in batches:
        enc.wait()
        rt_sync = time.perf_counter()
        enc.embed_packed_into(c["ids"], c["off"], ix, c["rows"], wait=False)
        enq.append(time.perf_counter() - rt_sync)
        enc.wait()
    w, e = statistics.median(wall) * 1e3, statistics.median(enq) * 1e3
    print(f"[sync] per call of {len(batches[0]['rows'])} passages (median over {len(batches)} calls): embed_tokens_into {w:.2f} ms wall; the same forward enqueued without a wait "
          f"(embed_packed_into, wait=False) {e:.2f} ms; the host waits {w - e:.2f} ms = {100 * (w - e) / w:.0f} % of the call in the one synchronisation", flush=True)
    ix.close()
    enc.close()
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
