"""Writes tests/golden/rerank_golden.{npz,json}: [CLS] rows and logits of transformers' BertForSequenceClassification (fp32, eager
attention, CPU) for the seeded cross-encoders of tests/rerank_ref.py.  Run by hand (CPU, a minute); no test runs it.

The file holds ids, offsets, first_lens, the fp32 [CLS] rows and logits, cfg, seed, the head's shape and the bounds -- not the weights
(tests/rerank_ref.make_weights / make_head rebuild them).

Bounds: nothing derives how far a bf16 forward of two scaled layers may land from fp32, so the bounds are measured against the reference
alone: the same transformers model cast to torch.bfloat16, on the CPU.  T_logit = 2 x max|logit_bf16 - logit_fp32|, T_cls likewise over
the [CLS] rows (the factor 2: the device rounds at other points than torch does; it accumulates in f32, so it should sit inside).

Before writing, per model, the generator checks that
  (i)   tests/rerank_ref.forward lands within 1e-4 of the transformers logits;
  (ii)  each of three wrong segment conventions -- all types 0, types flipped, the question's [SEP] counted to segment 1 -- misses the
        logits by MORE than T_logit;
  (iii) at least half of the passage pairs of the questions have fp32 scores more than 2 T_logit apart (the ranking check of the GPU
        test may skip the others); seeds are tried in order until one satisfies it
and refuses to write the file otherwise: fixtures that cannot tell those apart pin nothing.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import rerank_ref as rr  # noqa: E402

SEEDS = range(3, 11)


def transformers_outputs(cfg, blob, head, ids_flat, offsets, first_lens, dtype):
    import torch
    from transformers import BertConfig, BertForSequenceClassification

    nl = head["cls_w"].shape[0]
    hc = BertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                    intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], type_vocab_size=cfg["type_vocab"], layer_norm_eps=cfg["ln_eps"],
                    hidden_act="gelu", num_labels=nl, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, classifier_dropout=0.0)
    hc._attn_implementation = "eager"
    model = BertForSequenceClassification(hc).eval()
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rr.to_hf_state_dict(cfg, blob, head).items()}
    missing = model.load_state_dict(sd, strict=False)
    has_pooler = head["pooler_w"] is not None
    assert not missing.unexpected_keys and all(k.startswith("bert.pooler.") and not has_pooler for k in missing.missing_keys), missing
    model = model.to(dtype)
    B = len(first_lens)
    cls, logits = np.empty((B, cfg["hidden"]), np.float32), np.empty((B, nl), np.float32)
    with torch.no_grad():
        for i in range(B):  # one pair at a time: no padding, no mask
            ids = torch.from_numpy(np.asarray(ids_flat[offsets[i]:offsets[i + 1]], np.int64))[None]
            types = torch.from_numpy(rr.segment_ids(ids.shape[1], int(first_lens[i])))[None]
            if has_pooler:
                out = model(input_ids=ids, token_type_ids=types, output_hidden_states=True)
                row, lg = out.hidden_states[-1][0, 0], out.logits[0]
            else:  # the model's encoder and its classifier module, the pooler left out
                row = model.bert(input_ids=ids, token_type_ids=types).last_hidden_state[0, 0]
                lg = model.classifier(row)
            cls[i], logits[i] = row.float().numpy(), lg.float().numpy()
    return cls, logits


def gap_fraction(score, gap):
    per_q = score.reshape(rr.N_QUESTIONS, rr.N_PASSAGES)
    total = rr.N_QUESTIONS * rr.N_PASSAGES * (rr.N_PASSAGES - 1) // 2
    return sum(len(rr.ordered_pairs(row, gap)) for row in per_q) / total


def main() -> int:
    import torch

    data, meta, ok = {}, {}, True
    for name in rr.MODELS:
        cfg, hd, vo = rr.model_cfg(name), rr.HEADS[name], rr.VO_SCALE[name]
        chosen = None
        for seed in SEEDS:
            blob, head = rr.make_weights(cfg, seed, vo), rr.make_head(cfg, seed, hd["num_labels"], hd["pooler"])
            ids, offsets, first = rr.make_pairs(cfg, seed)
            cls32, lg32 = transformers_outputs(cfg, blob, head, ids, offsets, first, torch.float32)
            cls16, lg16 = transformers_outputs(cfg, blob, head, ids, offsets, first, torch.bfloat16)
            t_logit, t_cls = 2.0 * float(np.abs(lg16 - lg32).max()), 2.0 * float(np.abs(cls16 - cls32).max())
            frac = gap_fraction(rr.scores(lg32), 2.0 * t_logit)
            print(f"{name} seed {seed}: T_logit {t_logit:.4f}  T_cls {t_cls:.4f}  pairs with a gap {frac:.2f}")
            if frac >= 0.5:
                chosen = seed
                break
        if chosen is None:
            print(f"REFUSED: no seed of {list(SEEDS)} gives {name} a ranking gap on half of the passage pairs")
            return 1
        rcls, rlg = rr.forward(cfg, blob, head, ids, offsets, first)
        d = float(np.abs(rlg - lg32).max())
        print(f"  rerank_ref vs transformers: logits max|d| = {d:.2e}, cls max|d| = {np.abs(rcls - cls32).max():.2e}")
        ok &= d <= 1e-4
        for dev in rr.DEVIATIONS:
            _, wl = rr.forward(cfg, blob, head, ids, offsets, first, deviate=dev)
            miss = float(np.abs(wl - lg32).max())
            print(f"  {dev:8s} misses the logits by {miss:.3f}  {'outside' if miss > t_logit else 'INSIDE the bound'}")
            ok &= miss > t_logit
        data[f"{name}_ids"], data[f"{name}_offsets"], data[f"{name}_first_lens"] = ids.astype(np.int16), offsets.astype(np.int32), first
        data[f"{name}_cls"], data[f"{name}_logits"] = cls32, lg32
        meta[name] = dict(cfg=cfg, seed=chosen, vo_scale=vo, num_labels=hd["num_labels"], pooler=hd["pooler"], T_logit=t_logit, T_cls=t_cls, gap_fraction=frac,
                          weights="tests/rerank_ref.make_weights(cfg, seed, vo_scale) + make_head(cfg, seed, num_labels, pooler)")
    if not ok:
        print("REFUSED: a check failed, nothing written")
        return 1
    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "rerank_golden.npz", **data)
    (out / "rerank_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "rerank_golden.npz", (out / "rerank_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
