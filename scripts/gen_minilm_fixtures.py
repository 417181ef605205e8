"""Writes tests/golden/minilm_golden.{npz,json}: what transformers computes (fp32, eager attention, CPU, one sequence at a time) for the
seeded head-dimension-32 models of tests/minilm_ref.py -- mean-pooled BertModel vectors of three shapes, and the [CLS] rows and logits of
one BertForSequenceClassification cross-encoder.  Run by hand (CPU, a minute or two); no test runs it.

The file holds ids, lengths, the fp32 outputs, cfg, seed and the bounds -- not the weights (tests/minilm_ref.make_weights and
tests/rerank_ref.make_head rebuild them).

Bounds: measured against the reference alone, as scripts/gen_rerank_fixtures.py does: the same transformers model cast to torch.bfloat16
on the CPU.  T = 2 x max|vector_bf16 - vector_fp32| over all sequences of a shape; T_logit and T_cls likewise over the pairs (the factor
2: the device rounds at other points than torch does; it accumulates in f32, so it should sit inside).

Before writing, per model, the generator checks that a forward which splits the SAME weights into heads / 2 heads of 64 -- what a loader
that derived heads = hidden // 64 would build -- misses the fp32 result by MORE than the bound in EVERY sequence (for the cross-encoder:
the [CLS] row of every pair by more than T_cls), and refuses to write otherwise: a fixture that cannot tell the two apart pins nothing.
Seeds are tried in order until one satisfies it.  With plain 0.02-scale weights the wrong split moves a pooled vector by 0.001 .. 0.015,
less than the bf16 error; hence Wq, Wk, Wv, Wo x 8 in make_weights.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import bert_oracle as bo  # noqa: E402
from tests import minilm_ref as mr  # noqa: E402
from tests import rerank_ref as rr  # noqa: E402

SEEDS = range(3, 11)


def hf_config(cfg, heads, **kw):
    from transformers import BertConfig

    hc = BertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=heads,
                    intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], type_vocab_size=cfg["type_vocab"], layer_norm_eps=cfg["ln_eps"],
                    hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **kw)
    hc._attn_implementation = "eager"
    return hc


def pooled_vectors(cfg, blob, heads, seqs, dtype):
    """Mean over the tokens of BertModel's last hidden state, one unpadded sequence at a time -> [len(seqs), hidden] f32."""
    import torch
    from transformers import BertModel

    model = BertModel(hf_config(cfg, heads), add_pooling_layer=False).eval()
    missing = model.load_state_dict(bo.to_hf_state_dict(cfg, blob), strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    model = model.to(dtype)
    out = np.empty((len(seqs), cfg["hidden"]), np.float32)
    with torch.no_grad():
        for i, s in enumerate(seqs):
            h = model(input_ids=torch.from_numpy(np.asarray(s, np.int64))[None]).last_hidden_state[0]
            out[i] = h.float().mean(0).numpy()
    return out


def pair_outputs(cfg, blob, head, heads, ids_flat, offsets, first_lens, dtype):
    import torch
    from transformers import BertForSequenceClassification

    model = BertForSequenceClassification(hf_config(cfg, heads, num_labels=head["cls_w"].shape[0], classifier_dropout=0.0)).eval()
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rr.to_hf_state_dict(cfg, blob, head).items()}
    missing = model.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    model = model.to(dtype)
    B = len(first_lens)
    cls, logits = np.empty((B, cfg["hidden"]), np.float32), np.empty((B, head["cls_w"].shape[0]), np.float32)
    with torch.no_grad():
        for i in range(B):  # one pair at a time: no padding, no mask
            ids = torch.from_numpy(np.asarray(ids_flat[offsets[i]:offsets[i + 1]], np.int64))[None]
            types = torch.from_numpy(rr.segment_ids(ids.shape[1], int(first_lens[i])))[None]
            o = model(input_ids=ids, token_type_ids=types, output_hidden_states=True)
            cls[i], logits[i] = o.hidden_states[-1][0, 0].float().numpy(), o.logits[0].float().numpy()
    return cls, logits


def main() -> int:
    import torch

    data, meta = {}, {}
    for name in mr.SHAPES:
        cfg = mr.model_cfg(name)
        chosen = None
        for seed in SEEDS:
            blob = mr.make_weights(cfg, seed)
            ids, lens, long_ids = mr.make_inputs(cfg, seed)
            seqs = [ids[i, :n] for i, n in enumerate(lens)] + [long_ids[0]]
            v32 = pooled_vectors(cfg, blob, cfg["heads"], seqs, torch.float32)
            v16 = pooled_vectors(cfg, blob, cfg["heads"], seqs, torch.bfloat16)
            T = 2.0 * float(np.abs(v16 - v32).max())
            miss = np.abs(pooled_vectors(cfg, blob, cfg["heads"] // 2, seqs, torch.float32) - v32).max(1)
            print(f"{name} seed {seed}: T {T:.4f} (scale {np.abs(v32).max():.2f}); heads of 64 miss each sequence by {np.array2string(miss, precision=3)}")
            if miss.min() > T:
                chosen = seed
                break
        if chosen is None:
            print(f"REFUSED: no seed of {list(SEEDS)} lets {name} tell heads of 32 from heads of 64 in every sequence")
            return 1
        d = float(np.abs(bo.forward(cfg, blob, ids, lens) - v32[:-1]).max())
        print(f"  bert_oracle.forward vs transformers: max|d| = {d:.2e}")
        if d > 1e-4:
            print("REFUSED: the numpy restatement and transformers disagree")
            return 1
        data[f"{name}_ids"], data[f"{name}_lens"], data[f"{name}_long_ids"] = ids.astype(np.int16), lens, long_ids.astype(np.int16)
        data[f"{name}_out"], data[f"{name}_long_out"] = v32[:-1], v32[-1:]
        meta[name] = dict(cfg=cfg, seed=chosen, T=T, wrong_split_min_miss=float(miss.min()), weights="tests/minilm_ref.make_weights(cfg, seed)")

    cfg = mr.model_cfg(mr.PAIR_SHAPE)
    chosen = None
    for seed in SEEDS:
        blob, head = mr.make_weights(cfg, seed, mr.TYPE_SCALE), rr.make_head(cfg, seed, 1, True)
        ids, offsets, first = rr.make_pairs(cfg, seed)
        cls32, lg32 = pair_outputs(cfg, blob, head, cfg["heads"], ids, offsets, first, torch.float32)
        cls16, lg16 = pair_outputs(cfg, blob, head, cfg["heads"], ids, offsets, first, torch.bfloat16)
        t_logit, t_cls = 2.0 * float(np.abs(lg16 - lg32).max()), 2.0 * float(np.abs(cls16 - cls32).max())
        wcls, wlg = pair_outputs(cfg, blob, head, cfg["heads"] // 2, ids, offsets, first, torch.float32)
        miss = np.abs(wcls - cls32).max(1)
        print(f"pair seed {seed}: T_logit {t_logit:.4f}  T_cls {t_cls:.4f}; heads of 64 miss the [CLS] rows by {miss.min():.3f} .. {miss.max():.3f}, "
              f"the logits by up to {np.abs(wlg - lg32).max():.3f}")
        if miss.min() > t_cls:
            chosen = seed
            break
    if chosen is None:
        print(f"REFUSED: no seed of {list(SEEDS)} lets the cross-encoder tell heads of 32 from heads of 64 in every pair")
        return 1
    data["pair_ids"], data["pair_offsets"], data["pair_first_lens"] = ids.astype(np.int16), offsets.astype(np.int32), first
    data["pair_cls"], data["pair_logits"] = cls32, lg32
    meta["pair"] = dict(cfg=cfg, seed=chosen, num_labels=1, pooler=True, T_logit=t_logit, T_cls=t_cls, wrong_split_min_miss=float(miss.min()),
                        weights="tests/minilm_ref.make_weights(cfg, seed, TYPE_SCALE) + tests/rerank_ref.make_head(cfg, seed, 1, True)")

    out = ROOT / "tests" / "golden"
    np.savez_compressed(out / "minilm_golden.npz", **data)
    (out / "minilm_golden.json").write_text(json.dumps(meta, indent=1) + "\n")
    print("wrote", out / "minilm_golden.npz", (out / "minilm_golden.npz").stat().st_size, "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
