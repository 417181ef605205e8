"""GPU: head dimension 32 (Head32 / attention_qblock_core32 of attention_core.h as the policy of the attention kernels, the create rules of sc_encoder_model.cpp) through the C ABI.

Bounds.
  Single kernels against float64 numpy over bf16-rounded inputs with scale 1/sqrt(32): max <= 3e-2, median <= 3e-3, the bounds of
  tests/test_encoder_gpu.py::test_attention_kernel and tests/test_packed_gpu.py::test_attention_packed_kernel -- the rounding points (P
  and O to bf16) are the same as at head dimension 64.
  Whole path: T (T_logit / T_cls for the pairs) of tests/golden/minilm_golden.json -- twice what transformers' own bf16 forward misses its
  fp32 forward by (scripts/gen_minilm_fixtures.py) -- and the project's cos >= 0.999.  The generator has checked that a forward which
  splits the same weights into half as many heads of 64 misses every sequence by more than that.
"""
import json

import numpy as np
import pytest

import minilm_ref as mr
import rerank_ref as rr
from semcode_amd import _native

pytestmark = pytest.mark.gpu

HD = 32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------ 1. single-kernel parity
@pytest.mark.parametrize("S", [32, 64, 128, 256, 512, 1024])  # 1024: keys streamed through the LDS in segments of 512
def test_attention_kernel_d32(rt, S):
    B, heads = 3 if S <= 512 else 4, 4  # two head pairs: a wrong pair stride cannot pass with one
    H = heads * HD
    rng = np.random.default_rng(3200 + S)
    qkv = bf16_round(rng.standard_normal((B * S, 3 * H)).astype(np.float32) * np.r_[np.full(H, 2.0), np.ones(2 * H)].astype(np.float32))  # sharper softmax
    lens = np.array([S, S // 2 + 3, 1] + ([S - 517] if S > 512 else []), np.int32)  # (S - 517: a ragged last segment)
    ref = mr.attention_ref(qkv, lens, S, heads, HD)
    row = _native.diag_attention(rt, qkv, lens, B, S, heads, head_dim=HD)
    blk = _native.diag_attention(rt, qkv, lens, B, S, heads, head_dim=HD, blocked_rows=B * S + 256)
    assert row.shape == (B * S, H) and np.isfinite(row).all()
    assert np.array_equal(bits(blk), bits(row)), int((bits(blk) != bits(row)).sum())  # the layouts hold the same numbers
    err = np.abs(row - ref)
    print(f"attention d32 S={S}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2, (err.max(), np.unravel_index(err.argmax(), err.shape))  # P and O are rounded to bf16
    assert np.median(err) <= 3e-3


# ------------------------------------------------------------------ 2. head-pair isolation
@pytest.mark.parametrize("victim", [0, 1])
def test_a_head_reads_nothing_of_its_pair_partner(rt, victim):
    """The two heads of a 64-column block share every LDS row and every Q fragment register.  Whatever the partner's columns hold --
    zeros or +-1e30, which overflows its scores -- the other head's output keeps its bits."""
    B, S, heads = 2, 128, 2
    H = heads * HD
    rng = np.random.default_rng(41 + victim)
    qkv = rng.standard_normal((B * S, 3 * H)).astype(np.float32)
    lens = np.array([S, 77], np.int32)
    partner = 1 - victim
    cols = np.concatenate([np.arange(partner * HD, (partner + 1) * HD) + third * H for third in range(3)])
    keep = slice(victim * HD, (victim + 1) * HD)
    outs = []
    for fill in (0.0, 1e30):
        x = qkv.copy()
        x[:, cols] = fill * np.where(rng.random((B * S, len(cols))) < 0.5, -1.0, 1.0).astype(np.float32)
        for blocked in (0, B * S):
            outs.append(_native.diag_attention(rt, x, lens, B, S, heads, head_dim=HD, blocked_rows=blocked)[:, keep])
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0.1
    for o in outs[1:]:
        assert np.array_equal(bits(o), bits(outs[0]))


# ------------------------------------------------------------------ 3. segmented equals resident
def test_long_attention_d32_equals_the_resident_kernel_on_short_sequences(rt):
    """A sequence of <= 512 real tokens padded to 1 024 goes through the segmented kernel with ONE segment: same arithmetic per
    (query, key), so the real rows carry the bits the S = 512 kernel writes."""
    B, heads = 2, 4
    H = heads * HD
    rng = np.random.default_rng(5)
    qkv = rng.standard_normal((B * 512, 3 * H)).astype(np.float32)
    lens = np.array([512, 301], np.int32)
    short = _native.diag_attention(rt, qkv, lens, B, 512, heads, head_dim=HD).reshape(B, 512, H)
    pad = np.zeros((B, 1024, 3 * H), np.float32)
    pad[:, :512] = qkv.reshape(B, 512, 3 * H)
    long = _native.diag_attention(rt, pad.reshape(B * 1024, 3 * H), lens, B, 1024, heads, head_dim=HD).reshape(B, 1024, H)
    for b in range(B):
        assert np.isfinite(short[b, : lens[b]]).all()
        assert np.array_equal(bits(long[b, : lens[b]]), bits(short[b, : lens[b]]))


# ------------------------------------------------------------------ 4. packed kernel
def test_attention_packed_kernel_d32(rt):
    heads = 4
    H = heads * HD
    lens = np.array([1, 31, 32, 33, 128, 129, 256, 257, 512, 700], np.int32)  # every launch class and both sides of each threshold
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    end = int(span.sum())
    R = (end + 255) // 256 * 256
    assert R > end  # rows beyond the last sequence exist
    rng = np.random.default_rng(32)
    qkv = bf16_round(rng.standard_normal((R, 3 * H)).astype(np.float32) * np.r_[np.full(H, 2.0), np.ones(2 * H)].astype(np.float32))
    row = _native.diag_attention_packed(rt, qkv, starts, lens, heads, head_dim=HD)
    Rb = R + 256
    pad = np.zeros((Rb, 3 * H), np.float32)
    pad[:R] = qkv
    blk = _native.diag_attention_packed(rt, pad, starts, lens, heads, blocked_rows=Rb, head_dim=HD)
    assert row.shape == (R, H)
    assert np.array_equal(bits(blk[:R]), bits(row)), int((bits(blk[:R]) != bits(row)).sum())
    assert np.isnan(row[end:]).all() and np.isnan(blk[end:]).all()  # rows of no sequence: untouched
    assert np.isfinite(row[:end]).all()                             # alignment rows included
    for s, n, sp in zip(starts, lens, span):
        ref = mr.attention_ref(qkv[s:s + sp], [n], int(sp), heads, HD)
        err = np.abs(row[s:s + n] - ref[:n])
        print(f"packed attention d32 len={n}: max err {err.max():.3e}, median {np.median(err):.3e}")
        assert err.max() <= 3e-2, (n, err.max(), np.unravel_index(err.argmax(), err.shape))
        assert np.median(err) <= 3e-3, n


# ------------------------------------------------------------------ 5. end to end against transformers
@pytest.fixture(scope="module")
def minilm_golden(golden):
    return np.load(golden / "minilm_golden.npz"), json.loads((golden / "minilm_golden.json").read_text())


@pytest.mark.parametrize("name", ["h384", "h128", "h256"])
def test_embeddings_against_transformers(rt, minilm_golden, name):
    data, meta = minilm_golden
    m = meta[name]
    cfg, T = m["cfg"], m["T"]
    assert cfg["hidden"] == cfg["heads"] * HD and ((cfg["hidden"] % 256 == 0) == mr.FOLDS[name])
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    long_ids = data[f"{name}_long_ids"].astype(np.int32)
    want = np.concatenate([data[f"{name}_out"], data[f"{name}_long_out"]])
    flat = np.concatenate([ids[i, :n] for i, n in enumerate(lens)] + [long_ids[0]])
    offsets = np.concatenate([[0], np.cumsum(np.r_[lens, long_ids.shape[1]])]).astype(np.int64)
    enc = _native.Encoder(rt, cfg, weights=mr.make_weights(cfg, m["seed"]))
    try:
        for path in ("batch", "small"):  # sc_encoder_set_path 1 and 2; a shape that cannot fold runs the unfolded pipeline under both
            enc.set_path(path)
            rect = np.concatenate([enc.embed_ids(ids, lens), enc.embed_ids(long_ids, np.array([long_ids.shape[1]], np.int32))])
            packed = enc.embed_packed(flat, offsets)
            for form, got in (("rectangle", rect), ("packed", packed)):
                d = np.abs(got - want)
                cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
                print(f"{name} / {path} / {form}: max|d| {d.max():.4f} (T {T:.4f}), cos min {cos.min():.6f}")
                assert np.isfinite(got).all() and got.shape == want.shape
                assert d.max() <= T, (path, form, np.unravel_index(d.argmax(), d.shape))
                assert cos.min() >= 0.999, (path, form)
    finally:
        enc.close()


# ------------------------------------------------------------------ 6. reranker
def test_pairs_d32_against_transformers(rt, minilm_golden):
    data, meta = minilm_golden
    m = meta["pair"]
    cfg = m["cfg"]
    assert cfg["hidden"] == cfg["heads"] * HD and m["num_labels"] == 1 and m["pooler"]
    ids, offsets, first = data["pair_ids"].astype(np.int32), data["pair_offsets"].astype(np.int64), data["pair_first_lens"].astype(np.int32)
    want_ids, want_off, want_first = rr.make_pairs(cfg, m["seed"])
    assert np.array_equal(ids, want_ids) and np.array_equal(offsets, want_off) and np.array_equal(first, want_first)
    head = rr.make_head(cfg, m["seed"], 1, True)
    enc = _native.Encoder(rt, cfg, weights=mr.make_weights(cfg, m["seed"], mr.TYPE_SCALE))
    try:
        enc.set_pair_head(head["cls_w"], head["cls_b"], head["pooler_w"], head["pooler_b"])
        logits, cls = enc.score_pairs(ids, offsets, first, want_cls=True)
        dl, dc = np.abs(logits - data["pair_logits"]).max(), np.abs(cls - data["pair_cls"]).max()
        print(f"pairs d32: logits max|d| {dl:.4f} (T_logit {m['T_logit']:.4f}), cls max|d| {dc:.4f} (T_cls {m['T_cls']:.4f})")
        assert np.isfinite(logits).all() and logits.shape == data["pair_logits"].shape
        assert dl <= m["T_logit"] and dc <= m["T_cls"]
    finally:
        enc.close()


# ------------------------------------------------------------------ 7. create rules
def test_create_rules(rt):
    base = dict(mr.COMMON, hidden=256, heads=8, ffn=512)
    for scheme, word in (("alibi", "ALiBi"), ("rotary", "rotary")):
        with pytest.raises(_native.ScError) as err:
            _native.Encoder(rt, dict(base, **{scheme: True}), synth_seed=1)
        msg = str(err.value)
        assert "head dimension 32" in msg and word in msg and "pos_type" in msg, msg
    with pytest.raises(_native.ScError) as err:
        _native.Encoder(rt, dict(mr.COMMON, hidden=192, heads=4, ffn=512), synth_seed=1)  # head dimension 48
    assert "head dimension" in str(err.value)
    enc = _native.Encoder(rt, base, synth_seed=1)
    try:
        ids = np.random.default_rng(0).integers(1, base["vocab"], size=(3, 32)).astype(np.int32)
        out = enc.embed_ids(ids, np.array([32, 9, 1], np.int32))
        assert out.shape == (3, 256) and np.isfinite(out).all() and np.abs(out).max() > 0
    finally:
        enc.close()
