"""GPU: [CLS] pooling (sc_encoder_set_pooling, encoder_cls.hip) and the last layer on the [CLS] rows only ("cls_prune"), through the C ABI.

Bounds.
  Whole path: T (T_norm for L2-normalised output) of tests/golden/cls_golden.json -- twice what transformers' own bf16 forward misses its
  fp32 forward by on the [CLS] row (scripts/gen_cls_fixtures.py).  The generator has checked that the fp32 MEAN-pooled vector misses every
  [CLS] vector of a sequence longer than one token by more than T: an encoder that kept pooling by mean cannot pass.
  Pruned against unpruned on batches without a golden vector: both sit within T of the same exact result, T of the fixture model with
  that shape -- the two differ by bf16 rounding (other GEMM tile / split-K orders, the last LayerNorm in f32), far inside it.
  attention_cls_kernel against float64 numpy over bf16-rounded inputs, and against row 0 of the full attention kernels: max <= 3e-2,
  median <= 3e-3, the bar of tests/test_headdim32_gpu.py and tests/test_fold_kernels_gpu.py for the attention diagnostics.
"""
import json

import numpy as np
import pytest

import minilm_ref as mr
import rerank_ref as rr
from oracle import bert_oracle as bo
from semcode_amd import _native

pytestmark = pytest.mark.gpu

MODELS = ["h128", "h256", "h384", "h384_s256", "h256_hd64", "h128_hd64_l1"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def flatten(ids, lens):
    flat = np.concatenate([ids[i, :n] for i, n in enumerate(lens)]).astype(np.int32)
    return flat, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.fixture(scope="module")
def cls_golden(golden):
    return np.load(golden / "cls_golden.npz"), json.loads((golden / "cls_golden.json").read_text())


@pytest.fixture()
def prune():
    yield lambda v: _native.diag_set_option("cls_prune", v)
    _native.diag_set_option("cls_prune", -1)


@pytest.fixture(scope="module")
def encoders(rt, cls_golden):
    """One encoder per (fixture model, normalize), built on first use and shared by the tests of this module."""
    _, meta = cls_golden
    cache = {}

    def get(name, normalize=False, pooling="cls"):
        key = (name, bool(normalize))
        if key not in cache:
            m = meta[name]
            cache[key] = _native.Encoder(rt, m["cfg"], weights=mr.make_weights(m["cfg"], m["seed"]), normalize=bool(normalize))
        enc = cache[key]
        enc.set_path("auto")
        enc.pooling = pooling
        return enc

    yield get
    for enc in cache.values():
        enc.close()


# ------------------------------------------------------------------ 1. golden parity
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", MODELS)
def test_cls_vectors_against_transformers(cls_golden, encoders, prune, name, normalize):
    data, meta = cls_golden
    m = meta[name]
    T = m["T_norm"] if normalize else m["T"]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    assert ids.shape == (8, m["S"]) and {1, 2, m["S"]} <= set(lens.tolist())
    want = data[f"{name}_cls_norm"] if normalize else data[f"{name}_cls"]
    flat, offsets = flatten(ids, lens)
    enc = encoders(name, normalize)
    assert enc.pooling == "cls"
    for path in ("batch", "small"):
        enc.set_path(path)
        for pr in (0, 1):
            prune(pr)
            for form, got in (("rectangle", enc.embed_ids(ids, lens)), ("packed", enc.embed_packed(flat, offsets))):
                d = np.abs(got - want)
                print(f"{name} norm={int(normalize)} / {path} / cls_prune {pr} / {form}: max|d| {d.max():.4f} (T {T:.4f})")
                assert got.shape == want.shape and np.isfinite(got).all()
                assert d.max() <= T, (path, pr, form, np.unravel_index(d.argmax(), d.shape))


# ------------------------------------------------------------------ 2. the mean path does not move
@pytest.mark.parametrize("name", ["h256", "h384"])
def test_mean_pooling_survives_a_round_trip(rt, cls_golden, encoders, name):
    data, meta = cls_golden
    m = meta[name]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    flat, offsets = flatten(ids, lens)
    fresh = _native.Encoder(rt, m["cfg"], weights=mr.make_weights(m["cfg"], m["seed"]))
    try:
        assert fresh.pooling == "mean"
        enc = encoders(name, pooling="mean")
        for path in ("batch", "small"):
            fresh.set_path(path)
            enc.set_path(path)
            want = (fresh.embed_ids(ids, lens), fresh.embed_packed(flat, offsets))
            before = (enc.embed_ids(ids, lens), enc.embed_packed(flat, offsets))
            enc.pooling = "cls"
            cls = enc.embed_ids(ids, lens)
            enc.pooling = "mean"
            after = (enc.embed_ids(ids, lens), enc.embed_packed(flat, offsets))
            assert np.abs(cls - want[0])[lens > 1].max() > m["T"]  # the mode did switch in between
            for w, b, a in zip(want, before, after):
                assert np.array_equal(bits(b), bits(w)) and np.array_equal(bits(a), bits(w)), path
    finally:
        fresh.close()


# ------------------------------------------------------------------ 3. a text's vector does not depend on its batch-mates' order
@pytest.mark.parametrize("name", ["h256", "h384", "h128_hd64_l1"])
def test_pruned_rows_follow_a_permutation(cls_golden, encoders, prune, name):
    data, _ = cls_golden
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    perm = np.array([5, 0, 7, 2, 1, 6, 3, 4])
    enc = encoders(name)
    prune(1)
    for path in ("batch", "small"):
        enc.set_path(path)
        a, b = enc.embed_ids(ids, lens), enc.embed_ids(ids[perm], lens[perm])
        assert np.isfinite(a).all() and np.array_equal(bits(b), bits(a[perm])), path
        pa, pb = enc.embed_packed(*flatten(ids, lens)), enc.embed_packed(*flatten(ids[perm], lens[perm]))
        assert np.isfinite(pa).all() and np.array_equal(bits(pb), bits(pa[perm])), path


# ------------------------------------------------------------------ 4. the compact GEMMs at other batch sizes
@pytest.mark.parametrize("B", [3, 257, 1025])  # 257: two row tiles of compact rows, split-K; 1025: Mc = 1280, above the split-K limit
@pytest.mark.parametrize("name", ["h256", "h384"])
def test_pruned_equals_unpruned_at_batch_sizes(cls_golden, encoders, prune, name, B):
    _, meta = cls_golden
    m = meta[name]
    S = 32
    rng = np.random.default_rng(1000 + B)
    lens = rng.integers(1, S + 1, B).astype(np.int32)
    lens[:3] = (S, 1, 2)
    ids = np.where(np.arange(S)[None, :] < lens[:, None], rng.integers(1, m["cfg"]["vocab"], (B, S)), 0).astype(np.int32)
    enc = encoders(name)
    outs = {}
    for pr in (0, 1):
        prune(pr)
        outs[pr] = (enc.embed_ids(ids, lens), enc.embed_packed(*flatten(ids, lens)))
    for form, full, pruned in zip(("rectangle", "packed"), outs[0], outs[1]):
        d = np.abs(pruned - full)
        print(f"{name} B={B} S={S} {form}: cls_prune 1 vs 0 max|d| {d.max():.4f} (T {m['T']:.4f})")
        assert pruned.shape == (B, m["cfg"]["hidden"]) and np.isfinite(pruned).all() and np.isfinite(full).all()
        assert d.max() <= m["T"], (form, np.unravel_index(d.argmax(), d.shape))


# ------------------------------------------------------------------ 5. attention_cls_kernel on its own
def attention_cls_ref(qkv, lens, S, heads, hd, slopes=None):
    """float64: softmax(q_0 K^T / sqrt(hd) - slope_h j) V of each text's first row -> [B, heads * hd]."""
    H = heads * hd
    B = len(lens)
    q, k, v = (qkv[:, i * H:(i + 1) * H].astype(np.float64).reshape(B, S, heads, hd) for i in range(3))
    out = np.empty((B, heads, hd))
    for b, n in enumerate(lens):
        n = max(1, min(int(n), S))
        for h in range(heads):
            s = k[b, :n, h] @ q[b, 0, h] / np.sqrt(hd)
            if slopes is not None:
                s = s - float(slopes[h]) * np.arange(n)
            e = np.exp(s - s.max())
            out[b, h] = (e / e.sum()) @ v[b, :n, h]
    return out.reshape(B, H)


@pytest.mark.parametrize("alibi", [False, True])
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("S", [64, 2048])
def test_attention_cls_kernel(rt, S, hd, alibi):
    heads = 4 if hd == 32 else 3  # two head pairs; an odd number of 64-wide heads
    H = heads * hd
    lens = np.array([1, 2, 31, 32, 33, S], np.int32)
    B = len(lens)
    rng = np.random.default_rng(S + hd + int(alibi))
    qkv = bf16_round(rng.standard_normal((B * S, 3 * H)).astype(np.float32) * np.r_[np.full(H, 2.0), np.ones(2 * H)].astype(np.float32))
    slopes = bo.alibi_slopes(heads).astype(np.float32) if alibi else None
    ref = attention_cls_ref(qkv, lens, S, heads, hd, slopes)
    if alibi:  # the bias matters on this data
        assert np.abs(ref - attention_cls_ref(qkv, lens, S, heads, hd)).max() > 0.1
    got = _native.diag_attention_cls(rt, qkv, lens, B, S, heads, head_dim=hd, slopes=slopes)
    assert got.shape == (B, H) and np.isfinite(got).all()
    err = np.abs(got - ref)
    print(f"attention_cls S={S} hd={hd} alibi={int(alibi)}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2, (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 3e-3
    if alibi and hd == 32:
        return  # the full kernels have no ALiBi form at head dimension 32
    full = _native.diag_attention_ex(rt, qkv, lens, B, S, heads, slopes=slopes, head_dim=hd)
    err = np.abs(got - full.reshape(B, S, H)[:, 0])
    print(f"  against row 0 of the full kernel: max {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2 and np.median(err) <= 3e-3


# ------------------------------------------------------------------ 6. fused ingest, pairs, invalid values
def test_embed_into_writes_the_cls_vectors(rt, cls_golden, encoders):
    data, meta = cls_golden
    name = "h256"
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    B = len(lens)
    enc = encoders(name)
    want = enc.embed_ids(ids, lens)
    assert np.abs(want - data[f"{name}_cls"]).max() <= meta[name]["T"]
    rows = np.arange(B, dtype=np.int64)
    ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
    got = enc.embed_ids_into(ids, lens, ix, rows, want_host=True)
    assert np.array_equal(bits(got), bits(want)) and len(ix) == B and ix.get_rows(0, B).tobytes() == want.tobytes()
    ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
    assert enc.embed_ids_into(ids, lens, ix, rows, wait=False) is None
    enc.wait()
    assert ix.get_rows(0, B).tobytes() == want.tobytes()
    flat, offsets = flatten(ids, lens)
    wantp = enc.embed_packed(flat, offsets)
    ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
    assert np.array_equal(bits(enc.embed_packed_into(flat, offsets, ix, rows, want_host=True)), bits(wantp))
    assert ix.get_rows(0, B).tobytes() == wantp.tobytes()
    ix = _native.Index(rt, 256, metric="IP", kind="FLAT")
    assert enc.embed_packed_into(flat, offsets, ix, rows, wait=False) is None
    enc.wait()
    assert ix.get_rows(0, B).tobytes() == wantp.tobytes()


def test_score_pairs_does_not_read_the_pooling_mode(rt, golden):
    m = json.loads((golden / "minilm_golden.json").read_text())["pair"]
    cfg = m["cfg"]
    ids, offsets, first = rr.make_pairs(cfg, m["seed"])
    head = rr.make_head(cfg, m["seed"], 1, True)
    enc = _native.Encoder(rt, cfg, weights=mr.make_weights(cfg, m["seed"], mr.TYPE_SCALE))
    try:
        enc.set_pair_head(head["cls_w"], head["cls_b"], head["pooler_w"], head["pooler_b"])
        for path in ("batch", "small"):
            enc.set_path(path)
            enc.pooling = "mean"
            l0, c0 = enc.score_pairs(ids, offsets, first, want_cls=True)
            enc.pooling = "cls"
            l1, c1 = enc.score_pairs(ids, offsets, first, want_cls=True)
            assert np.isfinite(l0).all() and np.array_equal(bits(l1), bits(l0)) and np.array_equal(bits(c1), bits(c0)), path
    finally:
        enc.close()


def test_invalid_pooling_values_change_nothing(cls_golden, encoders):
    data, _ = cls_golden
    ids, lens = data["h128_ids"].astype(np.int32), data["h128_lens"].astype(np.int32)
    enc = encoders("h128")
    want = enc.embed_ids(ids, lens)
    for bad in (2, -1, 7):
        assert _native.lib().sc_encoder_set_pooling(enc.handle, bad) == -1  # SC_ERR_INVALID
        assert enc.pooling == "cls"
        assert np.array_equal(bits(enc.embed_ids(ids, lens)), bits(want))
    with pytest.raises(ValueError):
        enc.pooling = "last"
    with pytest.raises(ValueError):
        _native.Encoder(None, pooling="max")
