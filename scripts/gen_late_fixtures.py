"""Writes tests/golden/late_golden.{npz,json}: token vectors and MaxSim scores of transformers' BertModel / ModernBertModel (fp32, eager
attention, CPU) + Linear(H, W, bias=False) + L2 normalisation for the seeded late-interaction models of tests/late_ref.py.  Run by hand
(CPU, a few minutes); no test runs it.

Reference: every question is run with [MASK] ids on its expansion positions and attention_mask 0 there; every passage as it is; the
score is MaxSim over the passage tokens outside the skiplist.  The files hold the ids, the fp32 scores, the question vectors, the passage
vectors of late_ref.stored_rows, cfg, seed, scale and the bounds -- not the weights.

Bounds, measured against the reference alone: the same transformers model (and projection) cast to torch.bfloat16, on the CPU, thread count
pinned.  T_vec = 2 x max|v_bf16 - v_fp32| over every token vector, T_score = 2 x max|s_bf16 - s_fp32| over every pair.

Before writing, per case, the generator checks that
  (i)   tests/late_ref.forward lands within 1e-4 of transformers, vectors and scores;
  (ii)  every mix-up of late_ref.DEVIATIONS misses the scores by MORE than T_score on every pair it applies to.  A (case, mix-up) in DROPPED
        is measured and recorded with its reason, and does not refuse the case -- provided that, where the mix-up changes token vectors, it
        misses T_vec on every text it changes (the GPU test compares the vectors row by row);
  (iii) for every question at least half of its passage pairs have fp32 scores more than 2 T_score apart (the ranking check of the GPU test
        may skip the others)
for the case's (seed, scale) of CHOSEN, and refuses to write otherwise.  `--search CASE ...` walks TRIES for the named cases and prints the
first entry that passes; it writes nothing, CHOSEN is edited by hand.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import late_ref as lr  # noqa: E402

THREADS = 1
CHOSEN = {"bert128": (41, 4.0), "bert384": (41, 4.0), "bert768": (41, 4.0), "mb256": (41, 2.0)}  # case -> (seed, scale), found with --search
TRIES = [(seed, scale) for seed in range(41, 53) for scale in (4.0, 8.0, 2.0)]
VECTOR_DEVIATIONS = ("unnormalised", "expansion_attended", "expansion_token0", "markers_swapped", "pre_norm_rows")  # mix-ups that change token vectors
# case -> {deviation: reason}.  MaxSim is a sum of maxima over many passage tokens: a changed question row finds another passage token with a
# similar dot, so the SCORE of some pair moves by less than the bf16 model's own error for the mix-ups below on every seed of TRIES (the
# search log has the figures).  Each of them that changes token vectors must then miss T_vec on every text it changes (checked below); the
# skiplist changes a score only where a skiplist token would win a maximum, and its smallest miss is 0 on pairs where none does.
_WEAK = {"expansion_attended": "a sum of up to 29 maxima concentrates; caught in the expansion rows' vectors",
         "expansion_token0": "a sum of up to 29 maxima concentrates; caught in the expansion rows' vectors",
         "markers_swapped": "the marker is one row of the text and reaches the others through attention only; caught in the vectors",
         "pre_norm_rows": "one affine map per column in front of a random projection, then L2 normalisation; caught in the vectors",
         "skiplist_ignored": "changes a score only where a skiplist token would win a maximum: miss 0 on the pairs where none does"}
DROPPED: dict = {name: {k: v for k, v in _WEAK.items() if k != "pre_norm_rows"} for name in ("bert128", "bert384", "bert768")}
# the pre-norm case's questions keep 24 tokens or more (late_ref.Q_LENS): 0 .. 8 expansion rows, whose maxima are a small part of the score;
# a missing expansion row is caught by the counts and the layout, which the GPU test compares exactly
DROPPED["mb256"] = dict(_WEAK, no_expansion="0 .. 8 expansion rows per question; a missing row is caught by the exact count and layout check")


def transformers_outputs(case, blob, proj, questions, passages, dtype):
    import torch
    import transformers

    hc = lr.hf_model_config(case)
    if lr.arch_of(case) == 1:
        conf = transformers.ModernBertConfig(**{k: v for k, v in hc.items() if k != "model_type"})
        conf._attn_implementation = "eager"
        model = transformers.ModernBertModel(conf)
    else:
        conf = transformers.BertConfig(**{k: v for k, v in hc.items() if k != "model_type"})
        conf._attn_implementation = "eager"
        model = transformers.BertModel(conf, add_pooling_layer=False)
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in lr.hf_state_dict(case, blob).items()}, strict=False)
    assert not res.unexpected_keys and not res.missing_keys, res
    model = model.eval().to(dtype)
    lin = torch.nn.Linear(case["cfg"]["hidden"], case["W"], bias=False)
    lin.weight.data = torch.from_numpy(proj.copy())
    lin = lin.to(dtype)

    def vectors(ids, n_real):
        t = torch.from_numpy(np.asarray(ids, np.int64))[None]
        mask = (torch.arange(t.shape[1]) < n_real).long()[None]
        with torch.no_grad():
            h = model(input_ids=t, attention_mask=mask).last_hidden_state[0]
            return torch.nn.functional.normalize(lin(h), p=2, dim=-1).float().numpy()

    qv = [vectors(lr.expand(q), len(q)) for q in questions]
    dv = [vectors(p, len(p)) for p in passages]
    sc = np.array([[(a @ b[lr.keep_flags(p).astype(bool)].T).max(1).sum() for b, p in zip(dv, passages)] for a in qv], np.float32)
    return qv, dv, sc


def try_case(name, case, seed, scale):
    import torch

    torch.set_num_threads(THREADS)
    blob, proj = lr.make_weights(case, seed, scale), lr.make_proj(case, seed)
    questions, passages = lr.make_texts(case, seed)
    q32, d32, s32 = transformers_outputs(case, blob, proj, questions, passages, torch.float32)
    q16, d16, s16 = transformers_outputs(case, blob, proj, questions, passages, torch.bfloat16)
    t_vec = 2.0 * max(float(np.abs(a - b).max()) for a, b in zip(q32 + d32, q16 + d16))
    t_score = 2.0 * float(np.abs(s16 - s32).max())
    per_q = [len(lr.ordered_pairs(row, 2.0 * t_score)) for row in s32]
    need = lr.N_PASSAGES * (lr.N_PASSAGES - 1) // 2 / 2
    print(f"{name} seed {seed} scale {scale}: T_vec {t_vec:.4f}  T_score {t_score:.4f}  score spread {np.ptp(s32):.2f}  passage pairs with a gap per question {per_q} "
          f"(need {need:.0f})", flush=True)
    if min(per_q) < need:
        return None
    rq, rd, rs = lr.forward(case, blob, proj, questions, passages)
    d_vec = max(float(np.abs(a - b).max()) for a, b in zip(q32 + d32, rq + rd))
    d_sc = float(np.abs(rs - s32).max())
    print(f"  late_ref vs transformers: vectors max|d| = {d_vec:.2e}, scores max|d| = {d_sc:.2e}", flush=True)
    ok = d_vec <= 1e-4 and d_sc <= 1e-4
    dev_miss, dev_vec_miss = {}, {}
    expanded = [i for i, q in enumerate(questions) if len(q) % lr.QUERY_LEN]
    for dev in lr.DEVIATIONS:
        wq, wd, ws = lr.forward(case, blob, proj, questions, passages, deviate=dev)
        at = np.array([[lr.applicable(dev, q, p) for p in passages] for q in questions])
        if not at.any():
            continue
        miss = np.abs(ws - s32)[at]
        good = bool((miss > t_score).all())
        dropped = dev in DROPPED.get(name, {})
        dev_miss[dev] = float(miss.min())
        # a mix-up that changes token vectors is also measured there: its smallest max|dv| over the texts it changes, against T_vec.
        # A dropped (case, mix-up) must at least show in the vectors, which the GPU test checks row by row.
        vec_good = True
        if dev in VECTOR_DEVIATIONS:
            texts = [(wq[i], q32[i]) for i in (expanded if dev.startswith("expansion") else range(len(questions)))]
            texts += [] if dev.startswith("expansion") else list(zip(wd, d32))
            vmiss = min(float(np.abs(a - b).max()) for a, b in texts)
            dev_vec_miss[dev] = vmiss
            vec_good = vmiss > t_vec
        print(f"  {dev:20s} smallest miss over {int(at.sum())} pairs {miss.min():.4f}  {'outside' if good else 'INSIDE the bound'}"
              + (f"; vectors {dev_vec_miss[dev]:.4f} {'outside' if vec_good else 'INSIDE'} T_vec" if dev in dev_vec_miss else "")
              + (" (dropped for this case)" if dropped else ""), flush=True)
        ok &= good or (dropped and vec_good)
    if not ok:
        return None
    q_ids, q_off = lr.pack(questions)
    p_ids, p_off = lr.pack(passages)
    arrays = {f"{name}_q_ids": q_ids.astype(np.int16), f"{name}_q_off": q_off.astype(np.int32), f"{name}_p_ids": p_ids.astype(np.int16),
              f"{name}_p_off": p_off.astype(np.int32), f"{name}_scores": s32, f"{name}_qvec": np.concatenate(q32),
              f"{name}_dvec": np.concatenate([v[lr.stored_rows(len(v))] for v in d32])}
    meta = dict(cfg=case["cfg"], W=case["W"], seed=seed, scale=scale, T_vec=t_vec, T_score=t_score, gap_pairs_per_question=per_q, deviation_min_miss=dev_miss, deviation_min_vector_miss=dev_vec_miss,
                dropped=DROPPED.get(name, {}), bf16_reference=dict(torch=torch.__version__, threads=torch.get_num_threads()),
                weights="tests/late_ref.make_weights(case, seed, scale) + make_proj(case, seed) + make_texts(case, seed)")
    return arrays, meta


def main() -> int:
    data, meta, ok = {}, {}, True
    search = sys.argv[1:2] == ["--search"]
    only = sys.argv[2:] if search else sys.argv[1:]  # (trying a case: a search or a partial run never writes)
    for name, case in lr.CASES.items():
        if only and name not in only:
            continue
        for seed, scale in TRIES if search else [CHOSEN[name]]:
            got = try_case(name, case, seed, scale)
            if got:
                data.update(got[0])
                meta[name] = got[1]
                print(f"{name}: (seed, scale) = {(seed, scale)} passes", flush=True)
                break
        else:
            print(f"{name}: {'no entry of TRIES' if search else f'CHOSEN {CHOSEN[name]} no longer'} passes the checks")
            ok = False
    if not ok or only or search:
        print("REFUSED: a check failed (or a search or a partial run), nothing written")
        return 1
    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "late_golden.npz", **data)
    (out / "late_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "late_golden.npz", (out / "late_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
