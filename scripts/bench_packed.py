"""Packed variable-length batches against padded rectangles, same process, same encoder, synthetic weights.

    python scripts/bench_packed.py [--texts 4096] [--passes 2] > profiles/packed_bench.log

Two models (BERT-base with 512 positions; nomic-bert: rotary + SwiGLU, 2 048 positions), three inputs of --texts synthetic texts:
  (a) uniform        : 256 tokens each
  (b) log-uniform    : lengths log-uniform between 16 and the model's maximum, fixed seed
  (c) short+outliers : 200 +- 50 tokens, one maximum-length text in every 256
The padded path is the provider's batching as it stands: 256 consecutive texts, padded to the bucket of the longest
(MI355XEmbeddings.tokenize -> Encoder.embed_ids).  The packed path is the provider's with packed=True: the same 256 texts, flattened and
cut into calls of at most 65 536 token rows (flatten_ids + cut_packed + Encoder.embed_packed; the flattening is inside the timed region).
Per path: texts/s, real tokens/s, token rows run per step (mean over the calls).  Gate: packed must beat padded in texts/s on (b) and
(c) for both models; (a) is reported only (packed rotates Q and K with the stand-alone kernel and has no S = 256 attention
specialisation).  Exit status 1 if the gate fails.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from semcode_amd import _native  # noqa: E402
from semcode_amd.embeddings.providers import cut_packed, flatten_ids  # noqa: E402
from semcode_amd.embeddings.tokenizer import bucket_for  # noqa: E402

MODELS = {
    "bert-base": dict(_native.BERT_BASE, max_pos=512),
    "nomic-bert": dict(_native.BERT_BASE, max_pos=2048, rotary=True, swiglu=True, rope_theta=1000.0),
}
BATCH, BUDGET = 256, 65536


def make_lens(kind: str, n: int, max_len: int) -> np.ndarray:
    rng = np.random.default_rng(17)
    if kind == "a":
        return np.full(n, 256, np.int32)
    if kind == "b":
        return np.exp(rng.uniform(np.log(16), np.log(max_len), size=n)).astype(np.int32).clip(16, max_len)
    lens = rng.normal(200, 50, size=n).round().astype(np.int32).clip(8, max_len)
    lens[::256] = max_len
    return lens


def run(enc, lens: np.ndarray, vocab: int, max_len: int, passes: int):
    rng = np.random.default_rng(23)
    batches = []
    for start in range(0, len(lens), BATCH):
        bl = lens[start:start + BATCH]
        S = bucket_for(int(bl.max()), max_len)
        ids = rng.integers(1, vocab, size=(len(bl), S)).astype(np.int32)
        ids[np.arange(S)[None, :] >= bl[:, None]] = 0
        batches.append((ids, bl))
    rows_of = lambda l: enc.packed_rows(np.concatenate(([0], np.cumsum(l))))

    def padded():
        rows = []
        for ids, bl in batches:
            enc.embed_ids(ids, bl)
            rows.append((ids.size + 255) // 256 * 256)
        return rows

    def packed():
        rows = []
        for ids, bl in batches:
            for a, b in cut_packed(bl, BUDGET, rows_of):
                flat, offsets = flatten_ids(ids[a:b], bl[a:b])
                enc.embed_packed(flat, offsets)
                rows.append(enc.packed_rows(offsets))
        return rows

    out = {}
    for name, fn in (("padded", padded), ("packed", packed)):
        fn()  # warm-up: workspace, first touch
        best, rows = None, None
        for _ in range(passes):
            t0 = time.perf_counter()
            rows = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[name] = dict(seconds=best, texts_s=len(lens) / best, tokens_s=float(lens.sum()) / best, rows_step=float(np.mean(rows)), steps=len(rows),
                         rows_total=int(np.sum(rows)))
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=2)
    args = ap.parse_args()
    rt = _native.Runtime(device=0)
    ok = True
    print(f"# bench_packed: {args.texts} texts, batches of {BATCH}, packed budget {BUDGET} rows, best of {args.passes} passes, {_native.lib().sc_version().decode()}")
    for mname, cfg in MODELS.items():
        enc = _native.Encoder(rt, cfg, weights=None, synth_seed=1)
        for kind, label in (("a", "uniform 256"), ("b", "log-uniform 16..max"), ("c", "200+-50, one max per 256")):
            lens = make_lens(kind, args.texts, cfg["max_pos"])
            r = run(enc, lens, cfg["vocab"], cfg["max_pos"], args.passes)
            ratio = r["packed"]["texts_s"] / r["padded"]["texts_s"]
            for path in ("padded", "packed"):
                p = r[path]
                print(f"{mname:10s} ({kind}) {label:26s} {path}: {p['texts_s']:9.0f} texts/s  {p['tokens_s'] / 1e6:7.3f} M real tokens/s  "
                      f"{p['rows_step']:9.0f} rows/step x {p['steps']:3d} steps ({p['rows_total']} rows)  {p['seconds']:.3f} s", flush=True)
            gate = "" if kind == "a" else ("  GATE PASS" if ratio > 1.0 else "  GATE FAIL")
            ok = ok and (kind == "a" or ratio > 1.0)
            print(f"{mname:10s} ({kind}) packed / padded = {ratio:.3f} texts/s, {r['padded']['rows_total'] / r['packed']['rows_total']:.2f}x fewer rows{gate}", flush=True)
        enc.close()
    rt.close()
    print("# gate:", "PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
