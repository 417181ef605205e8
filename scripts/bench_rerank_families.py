"""Reranker throughput of the ModernBERT and Qwen3 families against the embedding forward over the SAME token rows, same process, same
encoder, synthetic weights -- scripts/bench_rerank.py's rule for sc_encoder_score_seqs.

    python scripts/bench_rerank_families.py [--questions 1024] [--passages 40] [--passes 2] [--models modernbert,qwen3] > profiles/rerank_families_bench.log

Two shapes: gte-reranker-modernbert-base (22 layers, 768 / 12 heads / 1 152, window 128, global every 3rd layer, prediction head on the [CLS]
row, 1 label) and Qwen3-Reranker-0.6B (28 layers, 1 024, 16 / 8 heads of 128, 3 072, QK-norm, a 2-label head of two vocabulary rows on the
last token); the vocabulary is cut to 4 096 rows (the embedding table does not enter the forward's cost).  Each scores --questions x
--passages sequences whose lengths are log-uniform between 40 and 500 tokens (fixed seed), in packed calls of at most 65 536 token rows
(cut_pair_batches, as MI355XReranker.score_packed cuts them).  The same flat ids and offsets then go through Encoder.embed_packed with the
pooling the head reads ([CLS] / last token): same plan, same GEMMs, same attention, no head.  Reported: pairs/s, texts/s, their ratio and
the run-to-run spread of the passes.  The expectation is a ratio of 1.0 within that spread (the head is about 1 GFLOP per call next to
teraflops of forward); a lower ratio is a finding to explain, no threshold is fixed.  Tokenisation and prompt building are host work and
not part of either number.

Also reported for the causal prompts: the share of token rows that are the per-question shared prefix (the template's system turn and
instruction line, counted by hand at --prompt-prefix tokens because no tokenizer exists offline, plus the question, 8 .. 32 tokens): what
sharing the prefix's K / V across a question's pairs could save.  The head kernels' time per launch comes from a kernel trace of a short
run of this script (rocprofv3 --kernel-trace --stats), appended to the log by hand.

Small calls: a scored call never takes the split-K GEMMs that an embedding call of up to 1 024 token rows takes (a pair's logits must not
depend on its batch-mates, and the split follows the row count), so it is timed against embed_packed over the same rows at 256, 512 and
1 024 rows (2, 4 and 8 texts of 128 tokens; the median of --small-reps calls): what the bit-identity costs where it costs anything.
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
VOCAB = 4096
MODELS = {
    "modernbert": dict(cfg=dict(vocab=VOCAB, hidden=768, layers=22, heads=12, ffn=1152, max_pos=2048, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True,
                                modernbert=True, local_window=128, global_every=3, rope_theta=160000.0, rope_theta_local=10000.0),
                       kind=1, pooling="cls", labels=1),
    "qwen3": dict(cfg=dict(vocab=VOCAB, hidden=1024, layers=28, heads=16, kv_heads=8, ffn=3072, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True,
                           qwen2=True, rope_theta=1000000.0, head_dim=128, qk_norm=True),
                  kind=2, pooling="last", labels=2),
}


def head_of(model: dict, rng) -> dict:
    H, nl = model["cfg"]["hidden"], model["labels"]
    f = lambda *s: rng.standard_normal(s).astype(np.float32) / np.float32(np.sqrt(H))  # noqa: E731
    if model["kind"] == 2:
        return dict(kind=2, pooling="last", cls_w=f(nl, H), cls_b=None)
    return dict(kind=1, pooling=model["pooling"], norm_eps=1e-5, dense_w=f(H, H), dense_b=None, norm_g=np.ones(H, np.float32), norm_b=None, cls_w=f(nl, H),
                cls_b=np.zeros(nl, np.float32))


def best_of(fn, passes: int) -> "tuple[float, float]":
    """(best, worst) wall time of `passes` runs after one warm-up"""
    out = fn()  # warm-up: workspace, first touch
    assert all(np.isfinite(o).all() for o in out)
    times = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times), max(times)


def small_calls(enc, rng, reps: int) -> None:
    for texts in (2, 4, 8):
        offsets = (128 * np.arange(texts + 1)).astype(np.int64)
        ids = rng.integers(1, VOCAB, size=int(offsets[-1])).astype(np.int32)
        med = {}
        for what, fn in (("score_seqs", enc.score_seqs), ("embed_packed", enc.embed_packed)):
            for _ in range(3):
                fn(ids, offsets)
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn(ids, offsets)
                times.append(time.perf_counter() - t0)
            med[what] = float(np.median(times))
        print(f"small call, {texts} texts of 128 tokens ({enc.packed_rows(offsets)} token rows): score_seqs (256-tile GEMMs) {1e3 * med['score_seqs']:.3f} ms, "
              f"embed_packed (split-K GEMMs) {1e3 * med['embed_packed']:.3f} ms, ratio {med['score_seqs'] / med['embed_packed']:.2f}", flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=1024)
    ap.add_argument("--passages", type=int, default=40)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--models", default="modernbert,qwen3")
    ap.add_argument("--small-reps", type=int, default=20, help="timed calls per small-call figure (0: skip them)")
    ap.add_argument("--prompt-prefix", type=int, default=63, help="tokens of the causal template in front of the question (counted by hand)")
    args = ap.parse_args()
    n = args.questions * args.passages
    rng = np.random.default_rng(29)
    lens = np.exp(rng.uniform(np.log(40), np.log(500), size=n)).astype(np.int64).clip(40, 500)
    q_len = np.repeat(rng.integers(8, 33, size=args.questions), args.passages)
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    ids = rng.integers(1, VOCAB, size=int(offsets[-1])).astype(np.int32)
    rt = _native.Runtime(device=0)
    print(f"# bench_rerank_families: {args.questions} questions x {args.passages} passages = {n} pairs, {int(lens.sum())} tokens (log-uniform 40..500), "
          f"calls of <= {BUDGET} token rows, best of {args.passes} passes, {_native.lib().sc_version().decode()}")
    for name in args.models.split(","):
        model = MODELS[name]
        enc = _native.Encoder(rt, model["cfg"], weights=None, synth_seed=1, pooling=model["pooling"])
        enc.set_score_head(head_of(model, rng))
        groups = cut_pair_batches(enc, lens, BUDGET)
        calls = [(ids[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a]) for a, b in groups]
        rows = sum(enc.packed_rows(o) for _, o in calls)
        score = lambda: [enc.score_seqs(i, o) for i, o in calls]  # noqa: E731
        embed = lambda: [enc.embed_packed(i, o) for i, o in calls]  # noqa: E731
        c = model["cfg"]
        print(f"## {name}: {c['layers']} layers, hidden {c['hidden']}, ffn {c['ffn']}, head kind {model['kind']} ({model['pooling']}, {model['labels']} label(s)); "
              f"{rows} token rows in {len(calls)} calls")
        best = {}
        for what, fn in (("score_seqs", score), ("embed_packed", embed), ("score_seqs again", score), ("embed_packed again", embed)):
            lo, hi = best_of(fn, args.passes)
            best[what] = (lo, hi)
            print(f"{what:19s}: {n / lo:9.0f} pairs/s  {lens.sum() / lo / 1e6:7.3f} M tokens/s  best {lo:.3f} s, worst {hi:.3f} s", flush=True)
        s = min(best["score_seqs"][0], best["score_seqs again"][0])
        e = min(best["embed_packed"][0], best["embed_packed again"][0])
        spread = max(hi / lo - 1.0 for lo, hi in best.values())
        again = max(abs(best["score_seqs"][0] / best["score_seqs again"][0] - 1.0), abs(best["embed_packed"][0] / best["embed_packed again"][0] - 1.0))
        print(f"score_seqs / embed_packed = {e / s:.3f} (pairs/s over texts/s, same rows); run-to-run spread: {100 * spread:.1f} % inside a measurement, "
              f"{100 * again:.1f} % between the two measurements of one call")
        if model["kind"] == 2:
            shared = np.minimum(args.prompt_prefix + q_len, lens - 1)
            print(f"shared prompt prefix ({args.prompt_prefix} template tokens + the question, 8..32): {100 * shared.sum() / lens.sum():.1f} % of the tokens, "
                  f"{100 * (np.ceil(shared / 32) * 32).sum() / (np.ceil(lens / 32) * 32).sum():.1f} % of the 32-row blocks")
        if args.small_reps > 0:
            small_calls(enc, rng, args.small_reps)
        enc.close()
    rt.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
