"""Reranker throughput against the embedding forward over the SAME token rows, same process, same encoder, synthetic weights.

    python scripts/bench_rerank.py [--questions 1024] [--passages 40] [--passes 2] > profiles/rerank_bench.log

A BERT-base-shaped cross-encoder (12 layers, 768, 512 positions, pooler + 1 label) scores --questions x --passages pairs whose lengths
are log-uniform between 40 and 500 tokens (fixed seed), the question part 8 .. 32 of them, in packed calls of at most 65 536 token
rows (cut_pair_batches, as MI355XReranker.score_packed cuts them).  The same flat ids and offsets then go through Encoder.embed_packed --
what the encoder could do before it had a pair path: same plan, same GEMMs, same attention; no segment ids, a masked mean instead
of the [CLS] row, no head.  Reported: pairs/s, texts/s, their ratio.  The expectation is a ratio of about 1 (the typed embedding and
the head are a few launches next to 12 layers); no threshold is fixed.  Tokenisation and pair stitching are host work and not part of
either number.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semcode_amd import _native  # noqa: E402
from semcode_amd.embeddings.reranker import cut_pair_batches  # noqa: E402

BUDGET = 65536


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=1024)
    ap.add_argument("--passages", type=int, default=40)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    cfg = dict(_native.BERT_BASE, max_pos=512)
    H, n = cfg["hidden"], args.questions * args.passages
    rng = np.random.default_rng(29)
    lens = np.exp(rng.uniform(np.log(40), np.log(500), size=n)).astype(np.int64).clip(40, 500)
    first = np.repeat(rng.integers(8, 33, size=args.questions), args.passages).astype(np.int32)
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    ids = rng.integers(1, cfg["vocab"], size=int(offsets[-1])).astype(np.int32)
    rt = _native.Runtime(device=0)
    enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32) / np.float32(np.sqrt(H))
    enc.set_pair_head(f(1, H), np.zeros(1, np.float32), f(H, H), np.zeros(H, np.float32))
    groups = cut_pair_batches(enc, lens, BUDGET)
    calls = [(ids[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a], first[a:b]) for a, b in groups]
    rows = sum(enc.packed_rows(o) for _, o, _ in calls)

    def score():
        return [enc.score_pairs(i, o, fl) for i, o, fl in calls]

    def embed():
        return [enc.embed_packed(i, o) for i, o, _ in calls]

    print(f"# bench_rerank: {args.questions} questions x {args.passages} passages = {n} pairs, {int(lens.sum())} tokens (log-uniform 40..500), "
          f"{rows} token rows in {len(calls)} calls of <= {BUDGET}, best of {args.passes} passes, {_native.lib().sc_version().decode()}")
    best = {}
    for name, fn in (("score_pairs", score), ("embed_packed", embed), ("score_pairs again", score)):
        out = fn()  # warm-up: workspace, first touch
        assert all(np.isfinite(o).all() for o in out)
        t = None
        for _ in range(args.passes):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            t = dt if t is None else min(t, dt)
        best[name] = t
        print(f"{name:18s}: {n / t:9.0f} pairs/s  {lens.sum() / t / 1e6:7.3f} M tokens/s  {t:.3f} s", flush=True)
    print(f"score_pairs / embed_packed = {best['embed_packed'] / min(best['score_pairs'], best['score_pairs again']):.3f} (pairs/s over texts/s, same rows)")
    enc.close()
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
