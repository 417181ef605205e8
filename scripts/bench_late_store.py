"""What the token store of an index costs and buys: the exhaustive MaxSim search against its two roofs, the rerank from stored token
vectors against sc_encoder_score_late over the same pairs, the ingest rate of put_tokens and one compaction.

    python scripts/bench_late_store.py [--rows 200000] [--reps 5] [--questions 1024] [--passages 40] [--skip-rerank] > profiles/late_store_bench.log

(1) Search.  --rows rows of log-uniform 40 .. 500 tokens, W = 128, unit-norm random token vectors: one block of 8 192 rows is drawn and
stored over and over in row ranges of that size until every row has tokens (the scan's cost does not depend on the repetition; the puts
are timed: rows/s and tokens/s, host rounding and the copy over the host link included).  Both formats.  search_late with one question
of nq = 32 and of nq = 128 vectors, k = 10: wall time of the whole host call (upload of the question, scan, merge, download), median
and min .. max of --reps calls after 2 warm-ups.  Against the roofs, by calculation: HBM at 6.3 TB/s achievable over 4 W (f32) or 2 W
(bf16) bytes per token; f32 MFMA at 155 TF measured over 2 nq W FLOP per token.  No fraction is promised.
(2) Compaction.  One block of rows gets its tokens again (as many dead tokens), then sc_index_compact_tokens, timed.
(3) Rerank.  --questions questions of 8 .. 32 tokens with --passages passages each (log-uniform 40 .. 500 tokens) on a BERT-base shape
with synthetic weights, as scripts/bench_late.py: Encoder.score_late over all pairs in calls of <= 65 536 passage token rows (both
forwards + MaxSim) against the store path over the same pairs in the same process -- the passages' token vectors stored once, then
per pass the questions' forward (Encoder.embed_tokens) + one Index.rerank_late.  The scores of the two paths are compared bit for bit.
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
from semcode_amd.embeddings.reranker import cut_pair_batches  # noqa: E402

W, BLOCK, MASK, BUDGET = 128, 8192, 103, 65536
HBM_BYTES_S, MFMA_F32_FLOPS = 6.3e12, 155e12


def unit(rng, n):
    v = rng.standard_normal((n, W), dtype=np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def search_part(rt, rows, reps):
    rng = np.random.default_rng(7)
    counts = np.exp(rng.uniform(np.log(40), np.log(500), size=min(BLOCK, rows))).astype(np.int32).clip(40, 500)
    vecs = unit(rng, int(counts.sum()))
    off = np.concatenate(([0], np.cumsum(counts, dtype=np.int64)))
    questions = {nq: [unit(rng, nq)] for nq in (32, 128)}
    for fmt in ("f32", "bf16"):
        ix = _native.Index(rt, 64, metric="IP")
        ix.fill_synthetic(rows, seed=0)
        t0 = time.perf_counter()
        for first in range(0, rows, BLOCK):
            n = min(BLOCK, rows - first)
            ix.put_tokens(np.arange(first, first + n), (counts[:n], vecs[: off[n]]), fmt=fmt)
        t_put = time.perf_counter() - t0
        st = ix.token_stats()
        tokens, elt = st["live"], (4 if fmt == "f32" else 2)
        print(f"[put_tokens {fmt}] {rows} rows, {tokens} tokens (log-uniform 40..500, W = {W}) in ranges of {BLOCK} rows: {t_put:.2f} s = {rows / t_put:.0f} rows/s, "
              f"{tokens / t_put / 1e6:.2f} M tokens/s; pool {st['pool_bytes'] / 2**30:.2f} GiB", flush=True)
        for nq, q in questions.items():
            med, lo, hi = timed(lambda: ix.search_late(q, k=10), reps)
            rate = tokens / (med * 1e-3)
            hbm, mfma = HBM_BYTES_S / (elt * W), MFMA_F32_FLOPS / (2.0 * nq * W)
            print(f"[search_late {fmt} nq={nq}] {med:.3f} ms per question (min {lo:.3f} .. max {hi:.3f}, {reps} calls): {rate / 1e9:.3f} G tokens/s = "
                  f"{rate * elt * W / 1e12:.3f} TB/s, {rate * 2 * nq * W / 1e12:.1f} TF; HBM roof {hbm / 1e9:.2f} G tokens/s -> {rate / hbm:.3f}, f32 MFMA roof "
                  f"{mfma / 1e9:.3f} G tokens/s -> {rate / mfma:.3f}", flush=True)
        n = min(BLOCK, rows)
        ix.put_tokens(np.arange(n), (counts[:n], vecs[: off[n]]), fmt=fmt)
        dead = ix.token_stats()["dead"]
        t0 = time.perf_counter()
        ix.compact_tokens()
        t_c = time.perf_counter() - t0
        assert ix.token_stats()["dead"] == 0
        print(f"[compact_tokens {fmt}] {dead} dead of {tokens + dead} tokens: {t_c * 1e3:.1f} ms = {tokens * elt * W / t_c / 1e12:.3f} TB/s of live tokens gathered "
              f"(read + written once each, allocation included)", flush=True)
        ix.close()


def rerank_part(rt, nq, per, passes):
    n = nq * per
    rng = np.random.default_rng(29)
    cfg = dict(_native.BERT_BASE, max_pos=512)
    plens = np.exp(rng.uniform(np.log(40), np.log(500), size=n)).astype(np.int64).clip(40, 500)
    qlens = rng.integers(8, 33, size=nq).astype(np.int64)
    p_off = np.concatenate(([0], np.cumsum(plens))).astype(np.int64)
    q_off = np.concatenate(([0], np.cumsum(qlens))).astype(np.int64)
    p_ids = rng.integers(1000, cfg["vocab"], size=int(p_off[-1])).astype(np.int32)
    q_ids = rng.integers(1000, cfg["vocab"], size=int(q_off[-1])).astype(np.int32)
    enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)
    enc.set_token_head((rng.standard_normal((W, cfg["hidden"])) / np.sqrt(cfg["hidden"])).astype(np.float32))
    calls = []
    for a, b in cut_pair_batches(enc, plens, BUDGET):  # passage p belongs to question p // per
        qa, qb = a // per, (b - 1) // per + 1
        calls.append(dict(a=a, b=b, q_ids=q_ids[q_off[qa]:q_off[qb]], q_off=q_off[qa:qb + 1] - q_off[qa], d_ids=p_ids[p_off[a]:p_off[b]], d_off=p_off[a:b + 1] - p_off[a],
                          pair_q=((np.arange(a, b) // per) - qa).astype(np.int32), pair_d=np.arange(b - a, dtype=np.int32)))

    def late():
        return np.concatenate([enc.score_late(c["q_ids"], c["q_off"], c["d_ids"], c["d_off"], c["pair_q"], c["pair_d"], expand_id=MASK) for c in calls])

    ix = _native.Index(rt, 64, metric="IP")
    ix.fill_synthetic(n, seed=0)
    t0 = time.perf_counter()
    for c in calls:  # ingest: the passages' forward once, their vectors through the host into the store
        vec, counts = enc.embed_tokens(c["d_ids"], c["d_off"])
        ix.put_tokens(np.arange(c["a"], c["b"]), (counts, vec))
    t_ingest = time.perf_counter() - t0
    cand = np.arange(n, dtype=np.int64).reshape(nq, per)

    def from_store():
        qv, qc = enc.embed_tokens(q_ids, q_off, expand_id=MASK)
        return ix.rerank_late((qv, np.concatenate(([0], np.cumsum(qc))).astype(np.int32)), cand).reshape(-1)

    def best_of(fn):
        out = fn()
        t = min(timed(fn, passes, warm=0)[1:2])
        return out, t * 1e-3

    s_late, t_late = best_of(late)
    s_store, t_store = best_of(from_store)
    same = np.array_equal(s_late.view(np.uint32), s_store.view(np.uint32))
    print(f"[rerank] {nq} questions x {per} passages = {n} pairs, {int(plens.sum())} passage tokens, BERT-base shape, W = {W}, best of {passes} passes; ingest "
          f"(forward + put_tokens, once) {t_ingest:.2f} s")
    print(f"[rerank] score_late (both forwards + MaxSim)          : {t_late:.3f} s = {n / t_late:.0f} pairs/s")
    print(f"[rerank] questions' forward + rerank_late from store  : {t_store:.3f} s = {n / t_store:.0f} pairs/s")
    print(f"[rerank] ratio {t_late / t_store:.1f} x; scores bit-identical: {same}", flush=True)
    ix.close()
    enc.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--questions", type=int, default=1024)
    ap.add_argument("--passages", type=int, default=40)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--skip-rerank", action="store_true")
    a = ap.parse_args()
    rt = _native.Runtime(device=0)
    print(f"# bench_late_store: {_native.lib().sc_version().decode()}, {rt.device_info()}", flush=True)
    search_part(rt, a.rows, a.reps)
    if not a.skip_rerank:
        rerank_part(rt, a.questions, a.passages, a.passes)
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
