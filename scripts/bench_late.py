"""Late-interaction reranker throughput against the embedding forward over the SAME passage rows, same process, same encoder, synthetic
weights.

    python scripts/bench_late.py [--questions 1024] [--passages 40] [--passes 2] [--models bert modernbert] >> profiles/late_bench.log

--questions x --passages (question, passage) pairs: every question has 8 .. 32 tokens and its own --passages passages of log-uniform
40 .. 500 tokens (fixed seed), W = 128, on a BERT-base shape (12 layers, 768, 512 positions) and a ModernBERT-base shape (22 layers, 768,
GEGLU 1152, window 128, every third layer global).  A call of Encoder.score_late holds consecutive passages within 65 536 token rows and
the questions they pair with (what MI355XLateReranker.score_pairs sends).  The same passage ids and offsets then go through
Encoder.embed_packed: same plan, same GEMMs, same attention, a pooling kernel instead of the token head, no question forward, no MaxSim.

Reported: pairs/s and unique passages/s of score_late, passages/s of embed_packed, their ratio, and the time per launch of the two new
kernels, measured by difference in the same process: maxsim = score_late with every pair minus score_late with ONE pair per call;
token head = (score_late with one pair per call minus embed_packed over the rows of both sides), halved: two launches per call (the figure
includes what a pooling kernel would have cost with the opposite sign).  No target is fixed in advance.  Tokenisation is host work and not
part of any number.
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

BUDGET, W, MASK = 65536, 128, 103
SHAPES = {
    "bert": dict(_native.BERT_BASE, max_pos=512),
    "modernbert": dict(vocab=50368, hidden=768, layers=22, heads=12, ffn=1152, max_pos=8192, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True,
                       rope_theta=160000.0, rope_theta_local=10000.0, local_window=128, global_every=3),
}


def best_of(fn, passes):
    fn()  # warm-up: workspace, token buffers, first touch
    t = None
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        t = dt if t is None else min(t, dt)
    return t


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=1024)
    ap.add_argument("--passages", type=int, default=40)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--models", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    args = ap.parse_args()
    nq, per, n = args.questions, args.passages, args.questions * args.passages
    rng = np.random.default_rng(29)
    plens = np.exp(rng.uniform(np.log(40), np.log(500), size=n)).astype(np.int64).clip(40, 500)
    qlens = rng.integers(8, 33, size=nq).astype(np.int64)
    rt = _native.Runtime(device=0)
    for name in args.models:
        cfg = SHAPES[name]
        p_off = np.concatenate(([0], np.cumsum(plens))).astype(np.int64)
        q_off = np.concatenate(([0], np.cumsum(qlens))).astype(np.int64)
        p_ids = rng.integers(1000, cfg["vocab"], size=int(p_off[-1])).astype(np.int32)
        q_ids = rng.integers(1000, cfg["vocab"], size=int(q_off[-1])).astype(np.int32)
        enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)
        enc.set_token_head((rng.standard_normal((W, cfg["hidden"])) / np.sqrt(cfg["hidden"])).astype(np.float32))
        calls = []
        for a, b in cut_pair_batches(enc, plens, BUDGET):  # passage p belongs to question p // per
            qa, qb = a // per, (b - 1) // per + 1
            pair_d = np.arange(b - a, dtype=np.int32)
            pair_q = ((np.arange(a, b) // per) - qa).astype(np.int32)
            calls.append(dict(q_ids=q_ids[q_off[qa]:q_off[qb]], q_off=q_off[qa:qb + 1] - q_off[qa], d_ids=p_ids[p_off[a]:p_off[b]], d_off=p_off[a:b + 1] - p_off[a],
                              pair_q=pair_q, pair_d=pair_d))
        rows = sum(enc.packed_rows(c["d_off"]) for c in calls)

        def late(one_pair=False):
            return [enc.score_late(c["q_ids"], c["q_off"], c["d_ids"], c["d_off"], c["pair_q"][:1] if one_pair else c["pair_q"],
                                   c["pair_d"][:1] if one_pair else c["pair_d"], expand_id=MASK) for c in calls]

        def embed(both=False):
            out = [enc.embed_packed(c["d_ids"], c["d_off"]) for c in calls]
            if both:
                out += [enc.embed_packed(c["q_ids"], c["q_off"]) for c in calls]
            return out

        assert all(np.isfinite(o).all() for o in late())
        print(f"# bench_late {name}: {nq} questions x {per} passages = {n} pairs, {int(plens.sum())} passage tokens (log-uniform 40..500), {rows} passage token rows in "
              f"{len(calls)} calls of <= {BUDGET}, W = {W}, best of {args.passes} passes, {_native.lib().sc_version().decode()}", flush=True)
        t_late = best_of(late, args.passes)
        t_embed = best_of(embed, args.passes)
        t_one = best_of(lambda: late(True), args.passes)
        t_both = best_of(lambda: embed(True), args.passes)
        print(f"score_late        : {n / t_late:9.0f} pairs/s  {n / t_late:9.0f} unique passages/s  {t_late:.3f} s")
        print(f"embed_packed      : {n / t_embed:9.0f} passages/s (the same passage rows)  {t_embed:.3f} s")
        print(f"score_late / embed_packed = {t_embed / t_late:.3f} (unique passages/s over passages/s; the late call also runs the questions' forward)")
        print(f"maxsim_kernel     : {(t_late - t_one) / len(calls) * 1e3:8.3f} ms per launch of {n // len(calls)} pairs (by difference)")
        print(f"token_head_kernel : {(t_one - t_both) / (2 * len(calls)) * 1e3:8.3f} ms per launch (by difference against embed_packed over both sides' rows)", flush=True)
        enc.close()
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
