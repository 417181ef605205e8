"""GPU: heads of 128 and QK-norm on the causal decoder pipeline (sc_encoder_cfg.arch 2 with head_dim / qk_norm: Qwen3-Embedding, Qwen2.5-1.5B)
through the C ABI -- attention_causal_kernel<2, ..> and qknorm_rope_kernel of encoder_causal.hip on their own, the whole forward against
transformers, its properties and its refusals.

Bounds.
  Attention against float64 numpy over bf16-rounded q, k, v (q times 2: scores of standard deviation 2, a sharp softmax, as the 64-wide
  test): max <= 3e-2, median <= 3e-3, the bounds tests/test_qwen2_gpu.py and tests/test_encoder_gpu.py::test_attention_kernel put on the
  64-wide kernels, restated for a 128-term product.  An output is o = sum_j p_j v_j / l with sum p / l = 1 and |v| <= 4.5 here.  (a) P is
  rounded to bf16 before P V: relative 2^-9 per term, at most 2^-9 * max|v| = 8.8e-3; (b) l sums the unrounded p: the same 2^-9 relative on
  o, at most 8.8e-3; (c) O is rounded to bf16 once: half an ulp of |o| <= 4.5, 7.8e-3: 2.5e-2 <= 3e-2 when all three align, a tenth of it
  typically (the median).  None of these depends on the head width.  What does is the score: a 128-term instead of a 64-term product of
  bf16 values accumulated in f32 -- products exact, at most 128 roundings of 2^-24 relative to sum |q_i k_i| ~ 128 * 2 * 0.64 = 164, i.e.
  1.3e-3 on the raw score, 1.1e-4 after the 1/sqrt(128) scale (64-wide: 64 * 2^-24 * 82 / 8 = 4e-5): a relative 1.1e-4 on p, a twentieth
  of (a).  The f32 accumulation of P V runs over the keys, not the width.  So the 64-wide bounds hold unchanged.  The same numpy without a
  mask, with the mask one key wider, or with interleaved K/V heads must exceed them on every sequence of at least 33 tokens.
  qknorm_rope against float64: one rounding to bf16 -- half a bf16 ulp of the reference -- plus twice the kernel's f32 term: the sum of
  squares is a chain of 16 fused multiply-adds per lane and up to 3 shuffle levels (depth 19, all terms positive), rsqrt, the division, eps
  and the 1/HD factor 4 more roundings, entering by half; x * rs * gamma rounds twice; the table entry is a rounded cosine or sine (1), the
  rotation a product and a fused multiply-add (2): (23 / 2 + 5) * 2^-24 relative to |a cos| + |b sin| of the normalised pair (5 without
  the norm).
  Whole path: T_last / T_mean of tests/golden/qwen3_golden.json -- twice what transformers' own bf16 forward of that model misses its fp32
  forward by (scripts/gen_qwen3_fixtures.py) -- and the project's cos >= 0.999.
"""
import json

import numpy as np
import pytest

import fold_ref as fr
import qwen3_ref as q3
from semcode_amd import _native

pytestmark = pytest.mark.gpu

HD = 128


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def make_qkv(rows, heads, kvh, seed):
    rng = np.random.default_rng(seed)
    scale = np.r_[np.full(heads * HD, 2.0), np.ones(2 * kvh * HD)].astype(np.float32)
    return bf16_round(rng.standard_normal((rows, (heads + 2 * kvh) * HD)).astype(np.float32) * scale)


class SeqRef:
    """float64 attention of one sequence's real rows at head dimension 128: out(mask_extra, no_mask, interleaved)."""

    def __init__(self, qkv_rows, n, heads, kvh):
        x = qkv_rows[:n].astype(np.float64)
        AW, KV = heads * HD, kvh * HD
        self.n, self.heads, self.kvh = n, heads, kvh
        self.q = x[:, :AW].reshape(n, heads, HD).transpose(1, 0, 2)
        self.k = x[:, AW:AW + KV].reshape(n, kvh, HD).transpose(1, 0, 2)
        self.v = x[:, AW + KV:].reshape(n, kvh, HD).transpose(1, 0, 2)

    def out(self, extra=0, no_mask=False, interleaved=False):
        n, heads, kvh = self.n, self.heads, self.kvh
        of = [(h % kvh) if interleaved else h // (heads // kvh) for h in range(heads)]
        s = self.q @ self.k[of].transpose(0, 2, 1) / np.sqrt(HD)
        if not no_mask:
            s = np.where((np.arange(n)[None, :] <= np.arange(n)[:, None] + extra)[None], s, -np.inf)
        e = np.exp(s - s.max(-1, keepdims=True))
        return ((e / e.sum(-1, keepdims=True)) @ self.v[of]).transpose(1, 0, 2).reshape(n, heads * HD)


def check_causal(got, ref: SeqRef, what):
    """got: the kernel's rows of the sequence's real tokens"""
    err = np.abs(got - ref.out())
    print(f"{what} heads {ref.heads}/{ref.kvh} len {ref.n}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2, (what, ref.n, err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 3e-3, (what, ref.n)
    if ref.n >= 33:  # the inputs can tell: numpy with another mask or another head mapping must not pass
        wrong = [("no mask", ref.out(no_mask=True)), ("mask one key wider", ref.out(extra=1))]
        if ref.kvh not in (1, ref.heads):
            wrong.append(("interleaved K/V heads", ref.out(interleaved=True)))
        for name, w in wrong:
            e2 = np.abs(got - w)
            assert e2.max() > 3e-2, (what, name, ref.n, e2.max())


# Segments are 4 key tiles (S <= 128, texts up to 128 tokens) or 8 (beyond); the packed classes change at 128 and 256 tokens: one below, at
# and one above each, the four small lengths, a third segment (513) and a text of 1 100 tokens in S = 2 048.
RECT_LENS = {32: [32, 1, 31], 64: [64, 33], 128: [128, 127], 256: [256, 129, 255], 512: [512, 257], 2048: [1100]}
RECT_FORMS = {32: [(1, 1), (2, 1)], 64: [(2, 1), (4, 2)], 128: [(1, 1), (4, 2)], 256: [(2, 1), (16, 8)], 512: [(4, 2)], 2048: [(2, 1)]}


# ------------------------------------------------------------------ 1. the causal kernel at head dimension 128
@pytest.mark.parametrize("S", sorted(RECT_LENS))
def test_attention_causal128_kernel(rt, S):
    lens = np.array(RECT_LENS[S], np.int32)
    B = len(lens)
    for heads, kvh in RECT_FORMS[S]:
        AW = heads * HD
        qkv = make_qkv(B * S, heads, kvh, 8400 + S + heads)
        row = _native.diag_attention_causal(rt, qkv, lens, heads, kvh, S=S, head_dim=HD)
        assert row.shape == (B * S, AW) and np.isfinite(row).all()  # padding rows are queries too: they see key 0 at least
        if (heads, kvh) == RECT_FORMS[S][-1]:
            pad = np.zeros((B * S + 256, qkv.shape[1]), np.float32)
            pad[:B * S] = qkv
            blk = _native.diag_attention_causal(rt, pad, lens, heads, kvh, S=S, blocked_rows=B * S + 256, head_dim=HD)
            assert np.array_equal(bits(blk), bits(row)), int((bits(blk) != bits(row)).sum())  # the layouts hold the same numbers
        for b, n in enumerate(np.minimum(lens, S)):
            check_causal(row[b * S:b * S + n], SeqRef(qkv[b * S:(b + 1) * S], int(n), heads, kvh), f"rect S={S}")


PACKED_LENS = np.array([1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513, 1100], np.int32)  # every launch class, both sides of each threshold


def packed_layout(lens):
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    end = int(span.sum())
    return span, starts, end, (end + 255) // 256 * 256


@pytest.mark.parametrize("heads,kvh", [(1, 1), (2, 1), (4, 2), (16, 8)])
def test_attention_causal128_packed_kernel(rt, heads, kvh):
    lens = PACKED_LENS if (heads, kvh) == (2, 1) else PACKED_LENS[[0, 3, 5, 6, 8, 9]] if heads <= 4 else PACKED_LENS[[0, 3, 6, 9]]
    span, starts, end, R = packed_layout(lens)
    qkv = make_qkv(R, heads, kvh, 8500 + heads + kvh)
    row = _native.diag_attention_causal(rt, qkv, lens, heads, kvh, starts=starts, head_dim=HD)
    assert row.shape == (R, heads * HD)
    assert np.isnan(row[end:]).all()    # rows of no sequence (where the layout leaves any): untouched
    assert np.isfinite(row[:end]).all()  # alignment rows included
    if (heads, kvh) == (4, 2):
        pad = np.zeros((R + 256, qkv.shape[1]), np.float32)
        pad[:R] = qkv
        blk = _native.diag_attention_causal(rt, pad, lens, heads, kvh, starts=starts, blocked_rows=R + 256, head_dim=HD)
        assert np.array_equal(bits(blk[:end]), bits(row[:end])) and np.isnan(blk[end:]).all()
    for s, n in zip(starts, lens):
        check_causal(row[s:s + n], SeqRef(qkv[s:s + n], int(n), heads, kvh), "packed")


@pytest.mark.parametrize("heads,kvh", [(2, 1), (4, 2)])
def test_causal128_kernel_packed_and_rectangle_agree_bit_for_bit(rt, heads, kvh):
    """Keys are folded in groups of four tiles from key 0 whatever the segment size, and a query block's tiles depend on its own position
    and the text's length only: a text's rows are the same bits in rectangles of two S, in packed rows alone and among batch-mates."""
    lens = np.array([1100, 257, 129, 33, 1], np.int32)
    S = 2048
    qkv = make_qkv(len(lens) * S, heads, kvh, 8600 + heads)
    rect = _native.diag_attention_causal(rt, qkv, lens, heads, kvh, S=S, head_dim=HD)
    span, starts, end, R = packed_layout(lens)
    pk = np.zeros((R, qkv.shape[1]), np.float32)
    for b, (s, sp) in enumerate(zip(starts, span)):
        pk[s:s + sp] = qkv[b * S:b * S + sp]
    got = _native.diag_attention_causal(rt, pk, lens, heads, kvh, starts=starts, head_dim=HD)
    for b, (s, n) in enumerate(zip(starts, lens)):
        assert np.array_equal(bits(got[s:s + n]), bits(rect[b * S:b * S + n])), b
    for b, Ss in ((2, 256), (3, 64), (3, 128)):  # the 129- and the 33-token text in rectangles of their own: 8-tile and 4-tile segments
        small = _native.diag_attention_causal(rt, qkv[b * S:b * S + Ss], lens[b:b + 1], heads, kvh, S=Ss, head_dim=HD)
        assert np.array_equal(bits(small[:lens[b]]), bits(rect[b * S:b * S + lens[b]])), (b, Ss)
    alone = np.zeros((256, qkv.shape[1]), np.float32)  # the 129-token text alone in packed rows
    alone[:160] = qkv[2 * S:2 * S + 160]
    one = _native.diag_attention_causal(rt, alone, lens[2:3], heads, kvh, starts=np.zeros(1, np.int32), head_dim=HD)
    assert np.array_equal(bits(one[:129]), bits(rect[2 * S:2 * S + 129]))


def test_causal_widths_agree_on_a_zero_padded_head(rt):
    """One fold, one body and one launch path serve both widths, told apart by the number of 64-column blocks of a head: this pins the
    width-dependent strides, image offsets, fragment and tile counts against each other.  A 129-token text (second segment of the 8-tile
    class, first of the 16-tile class), 4 / 2 heads, in a rectangle of S = 256 and as a packed item.  The 128-wide input is the 64-wide
    one with 64 zero columns appended to every head; its Q is rounded to bf16 from sqrt(2) times the unrounded values the 64-wide Q is
    rounded from, so that q . k / sqrt(128) is the 64-wide q . k / sqrt(64) up to the two roundings of q and of the scale constant.  The
    float64 reference is the 64-wide one, from the 64-wide Q, K, V as they are; each width is held against it by the kernel bound of this
    file (max 3e-2, median 3e-3).  The extra rounding of the 128-wide Q moves a score by at most 2^-8 relative per term with random signs:
    about 2^-8 / sqrt(3) * sqrt(64) * 2 * 0.8 / 8 = 3.6e-3 on a score of standard deviation 2, the size of term (a) above.  The appended
    columns see V = 0 only: exactly zero."""
    heads, kvh, n, S = 4, 2, 129, 256
    rng = np.random.default_rng(8700)
    raw = rng.standard_normal((S, heads + 2 * kvh, 64)).astype(np.float32)
    raw[:, :heads] *= 2.0  # scores of standard deviation 2, as make_qkv
    x64 = bf16_round(raw)
    x128 = np.zeros((S, heads + 2 * kvh, HD), np.float32)
    x128[:, :, :64] = x64
    x128[:, :heads, :64] = bf16_round(raw[:, :heads] * np.float32(np.sqrt(2.0)))
    x64, x128 = x64.reshape(S, -1), x128.reshape(S, -1)
    lens, zero = np.array([n], np.int32), np.zeros(1, np.int32)
    q, k, v = (x64[:n].astype(np.float64).reshape(n, -1, 64)[:, a:b].transpose(1, 0, 2) for a, b in ((0, heads), (heads, heads + kvh), (heads + kvh, heads + 2 * kvh)))
    of = [h // (heads // kvh) for h in range(heads)]
    s = np.where((np.arange(n)[None, :] <= np.arange(n)[:, None])[None], q @ k[of].transpose(0, 2, 1) / 8.0, -np.inf)
    e = np.exp(s - s.max(-1, keepdims=True))
    ref = ((e / e.sum(-1, keepdims=True)) @ v[of]).transpose(1, 0, 2)  # [n, heads, 64]
    for form, kw in (("rect", dict(S=S)), ("packed", dict(starts=zero))):
        o64 = _native.diag_attention_causal(rt, x64, lens, heads, kvh, **kw)[:n].reshape(n, heads, 64)
        o128 = _native.diag_attention_causal(rt, x128, lens, heads, kvh, head_dim=HD, **kw)[:n].reshape(n, heads, HD)
        e64, e128 = np.abs(o64 - ref), np.abs(o128[:, :, :64] - ref)
        print(f"{form}: 64-wide max err {e64.max():.3e} median {np.median(e64):.3e}; 128-wide max err {e128.max():.3e} median {np.median(e128):.3e}; "
              f"128 against 64 max {np.abs(o128[:, :, :64] - o64).max():.3e}")
        assert e64.max() <= 3e-2 and np.median(e64) <= 3e-3, (form, e64.max(), np.median(e64))
        assert e128.max() <= 3e-2 and np.median(e128) <= 3e-3, (form, e128.max(), np.median(e128))
        assert (o128[:, :, 64:] == 0).all(), form


# ------------------------------------------------------------------ 2. QK-norm + rotation
U = 2.0 ** -24
EPS = 1e-6
THETA = 1000000.0


def qknorm_rope_ref(x, pos, heads, kvh, hd, gq, gk):
    """float64: (reference, magnitude |a cos| + |b sin| per output) of the Q and K columns; V columns as they are."""
    rows = x.shape[0]
    nqk = heads + kvh
    t = x[:, :nqk * hd].astype(np.float64).reshape(rows, nqk, hd)
    if gq is not None:
        g = np.stack([gq.astype(np.float64)] * heads + [gk.astype(np.float64)] * kvh)
        t = t / np.sqrt((t * t).mean(-1, keepdims=True) + EPS) * g[None]
    f = THETA ** (-2.0 * np.arange(hd // 2, dtype=np.float64) / hd)
    ang = pos.astype(np.float64)[:, None] * f[None, :]
    cos, sin = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    a, b = t[..., :hd // 2], t[..., hd // 2:]
    ref = np.concatenate([a * cos - b * sin, b * cos + a * sin], -1)
    mag = np.concatenate([np.abs(a * cos) + np.abs(b * sin), np.abs(b * cos) + np.abs(a * sin)], -1)
    return ref.reshape(rows, nqk * hd), mag.reshape(rows, nqk * hd)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_qknorm_rope_kernel(rt, hd, norm, packed):
    """Rectangle positions row % 2048 (rows 0, 1, 2047 and the wrap to 0, 1 among them) or an explicit position per row (0, 1, 2047 and random
    ones); rows of unit scale, rows 100 times larger and all-zero rows; heads 3 / kv_heads 1: an odd number of Q heads in front of the K head."""
    heads, kvh = 3, 1
    rng = np.random.default_rng(900 + hd + 2 * norm + packed)
    rows = 300 if packed else 2050
    x = rng.standard_normal((rows, (heads + 2 * kvh) * hd))
    r = np.arange(rows)
    x[r % 5 == 2] *= 100.0
    x[r % 11 == 3] = 0.0
    x = bf16_round(x.astype(np.float32))
    gq = (1.0 + 0.3 * rng.standard_normal(hd)).astype(np.float32) if norm else None
    gk = (1.0 + 0.3 * rng.standard_normal(hd)).astype(np.float32) if norm else None
    if packed:
        pos = rng.integers(0, 2048, size=rows).astype(np.int32)
        pos[:3] = (0, 1, 2047)
        got = _native.diag_qknorm_rope(rt, x, heads, kvh, hd, 2048, THETA, pos=pos, gamma_q=gq, gamma_k=gk, eps=EPS)
    else:
        pos = (r % 2048).astype(np.int32)
        got = _native.diag_qknorm_rope(rt, x, heads, kvh, hd, 2048, THETA, gamma_q=gq, gamma_k=gk, eps=EPS)
    nqk = (heads + kvh) * hd
    assert np.array_equal(bits(got[:, nqk:]), bits(x[:, nqk:]))  # V blocks come back bit-unchanged
    assert np.isfinite(got).all()
    assert not got[~x.any(1)].any()  # zero rows stay zero
    ref, mag = qknorm_rope_ref(x, pos, heads, kvh, hd, gq, gk)
    f32term = ((23 / 2 if norm else 0) + 5) * U * mag
    err = np.abs(got[:, :nqk] - ref)
    bar = 0.5 * fr.bf16_ulp(ref) + 2 * f32term
    print(f"qknorm_rope hd={hd} norm={norm} packed={packed}: err/bar max {float((err / np.maximum(bar, 1e-300)).max()):.4f}")
    assert np.all(err <= bar), (float((err / np.maximum(bar, 1e-300)).max()), np.unravel_index((err - bar).argmax(), err.shape))
    assert np.abs(got[3:, :nqk] - x[3:, :nqk]).max() > 0.5  # (it did rotate)


# ------------------------------------------------------------------ 3. whole path against transformers
@pytest.fixture(scope="module")
def q3_golden(golden):
    return np.load(golden / "qwen3_golden.npz"), json.loads((golden / "qwen3_golden.json").read_text())


def weights_of(m):
    return q3.make_weights(m["cfg"], m["seed"], *m["scales"])


def packed_of(ids, lens):
    flat = np.concatenate([ids[i, :n] for i, n in enumerate(lens)]).astype(np.int32)
    return flat, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


CASES = ["n_aw2h", "n_g2", "b_mha", "n_s2048", "n_06b", "b_15b"]


@pytest.mark.parametrize("name", CASES)
def test_embeddings_against_transformers(rt, q3_golden, name):
    data, meta = q3_golden
    m = meta[name]
    cfg = m["cfg"]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    flat, offsets = packed_of(ids, lens)
    enc = _native.Encoder(rt, cfg, weights=weights_of(m))
    try:
        for path in ("small", "batch"):  # split-K GEMMs up to 1 024 rows, or the 256-tile GEMMs for every size
            enc.set_path(path)
            for pooling, T, want in (("last", m["T_last"], data[f"{name}_last"]), ("mean", m["T_mean"], data[f"{name}_mean"])):
                enc.pooling = pooling
                for form, got in (("rectangle", enc.embed_ids(ids, lens)), ("packed", enc.embed_packed(flat, offsets))):
                    d, cos = miss(got, want)
                    print(f"{name} / {path} / {pooling} / {form}: max|d| {d.max():.4f} (T {T:.4f}), cos min {cos.min():.6f}")
                    assert np.isfinite(got).all() and got.shape == want.shape
                    assert d.max() <= T, (path, pooling, form, d)
                    assert cos.min() >= 0.999, (path, pooling, form, cos)
    finally:
        enc.close()


# ------------------------------------------------------------------ 4. properties
def test_a_text_does_not_depend_on_its_batch_mates(rt, q3_golden):
    data, meta = q3_golden
    m = meta["n_g2"]
    cfg = m["cfg"]
    ids, lens = data["n_g2_ids"].astype(np.int32), data["n_g2_lens"].astype(np.int32)
    enc = _native.Encoder(rt, cfg, weights=weights_of(m))
    try:
        for pooling in ("last", "mean"):
            enc.pooling = pooling
            both = enc.embed_ids(ids, lens)
            assert np.array_equal(bits(enc.embed_ids(ids, lens)), bits(both))  # run to run
            flat, offsets = packed_of(ids, lens)
            pboth = enc.embed_packed(flat, offsets)
            assert np.array_equal(bits(enc.embed_packed(flat, offsets)), bits(pboth))
            for i in (0, 2):  # 256 and 65 tokens: alone, and (packed) behind another text
                alone = enc.embed_ids(ids[i:i + 1], lens[i:i + 1])
                assert np.array_equal(bits(alone[0]), bits(both[i])), (pooling, i)
                f1, o1 = packed_of(ids[i:i + 1], lens[i:i + 1])
                assert np.array_equal(bits(enc.embed_packed(f1, o1)[0]), bits(pboth[i])), (pooling, i)
                j = (i + 1) % len(lens)
                f2, o2 = packed_of(ids[[j, i]], lens[[j, i]])
                assert np.array_equal(bits(enc.embed_packed(f2, o2)[1]), bits(pboth[i])), (pooling, i)
    finally:
        enc.close()


# ------------------------------------------------------------------ 5. refusals and the ABI's new fields
def test_create_rules_pooling_and_info(rt, q3_golden):
    _, meta = q3_golden
    base = dict(meta["n_g2"]["cfg"], vocab=64, layers=2)
    for change, words in ((dict(head_dim=96), ("head_dim", "96")), (dict(heads=17, kv_heads=17), ("head_dim 128", "2048")), (dict(qk_norm=2), ("qk_norm",)),
                          (dict(kv_heads=3), ("kv_heads", "3")), (dict(head_dim=0, heads=2, kv_heads=1), ("head dimension",))):
        c = _native.encoder_cfg(dict(base, **change))
        if "qk_norm" in change:
            c.qk_norm = change["qk_norm"]
        out = _native.C.c_void_p()
        assert _native.lib().sc_encoder_create(rt.handle, _native.C.byref(c), None, 0, _native.C.byref(out)) != 0 and not out.value
        buf = _native.C.create_string_buffer(512)
        _native.lib().sc_last_error(buf, 512)
        assert all(w in buf.value.decode() for w in words), (change, buf.value.decode())
    for field in ("head_dim", "qk_norm"):  # on a BERT encoder
        with pytest.raises(_native.ScError) as err:
            _native.Encoder(rt, dict(_native.BERT_BASE, vocab=64, layers=1, **{field: 128 if field == "head_dim" else True}), synth_seed=1)
        assert field in str(err.value) and "arch 2" in str(err.value)
    for heads, kvh, hd in ((3, 2, 128), (2, 3, 128), (2, 0, 128), (17, 1, 128), (2, 1, 96)):  # the support predicate
        with pytest.raises(_native.ScError) as err:
            _native.diag_attention_causal(rt, np.zeros((32, (heads + 2 * kvh) * hd), np.float32), np.array([32], np.int32), heads, kvh, S=32, head_dim=hd)
        assert "kv_heads" in str(err.value) and "head_dim" in str(err.value)
    enc = _native.Encoder(rt, base, synth_seed=1)
    try:
        info = _native.EncoderCfg()
        assert _native.lib().sc_encoder_info(enc.handle, _native.C.byref(info)) == 0
        assert (info.arch, info.heads, info.kv_heads, info.head_dim, info.qk_norm, info.hidden) == (2, 4, 2, 128, 1, 256)
        lib = _native.lib()
        assert lib.sc_encoder_set_pooling(enc.handle, 1) != 0 and enc.pooling == "mean"  # [CLS] is refused on arch 2 and changes nothing
        with pytest.raises(ValueError):
            enc.pooling = "cls"
        ids = np.random.default_rng(0).integers(1, 64, size=(3, 64)).astype(np.int32)
        out = enc.embed_ids(ids, np.array([64, 9, 1], np.int32))
        assert out.shape == (3, 256) and np.isfinite(out).all() and np.abs(out).max() > 0
        with pytest.raises(_native.ScError) as err:
            enc.score_pairs(np.arange(1, 9, dtype=np.int32), np.array([0, 8], np.int64), np.array([4], np.int32))
        assert "arch 2" in str(err.value) and "pairs" in str(err.value)
    finally:
        enc.close()


def test_head_dim_zero_and_64_stated_are_the_same_encoder(rt):
    """A Qwen2 0.5B-shaped encoder: head_dim 0 (hidden / heads) and head_dim 64 stated give the same bits, and report 64."""
    cfg = dict(vocab=300, hidden=896, layers=2, heads=14, kv_heads=2, ffn=4864, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True,
               rope_theta=1000000.0)
    ids = np.random.default_rng(1).integers(1, 300, size=(3, 128)).astype(np.int32)
    lens = np.array([128, 70, 1], np.int32)
    outs = []
    for hd in (0, 64):
        enc = _native.Encoder(rt, dict(cfg, head_dim=hd), synth_seed=5, pooling="last")
        try:
            info = _native.EncoderCfg()
            assert _native.lib().sc_encoder_info(enc.handle, _native.C.byref(info)) == 0
            assert (info.head_dim, info.qk_norm, info.kv_heads) == (64, 0, 2)
            outs.append(enc.embed_ids(ids, lens))
        finally:
            enc.close()
    assert np.isfinite(outs[0]).all() and np.array_equal(bits(outs[0]), bits(outs[1]))


def test_qk_norm_at_head_dimension_64(rt):
    """qk_norm is allowed at heads of 64 (qknorm_rope_kernel<64, true> in the forward): against the numpy restatement with the project's
    floor cos >= 0.999, on texts the restatement WITHOUT the norm misses that floor on (so the floor can tell), rectangle and packed."""
    cfg = dict(vocab=200, hidden=128, layers=2, heads=2, kv_heads=1, ffn=256, max_pos=512, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True,
               rope_theta=1000000.0, head_dim=64, qk_norm=True)
    blob = q3.make_weights(cfg, 41, 1.0, 0.3, 2.0, 3.0, 5.0, 0.3, 0, 1.0)
    ids = np.random.default_rng(2).integers(1, 200, size=(3, 256)).astype(np.int32)
    lens = np.array([200, 65, 9], np.int32)
    want = q3.forward(cfg, blob, ids, lens, "last")
    _, wrong_cos = miss(q3.forward(cfg, blob, ids, lens, "last", deviate="no_qk_norm"), want)
    assert (wrong_cos[lens > 32] < 0.999).all(), wrong_cos
    enc = _native.Encoder(rt, cfg, weights=blob, pooling="last")
    try:
        flat, offsets = packed_of(ids, lens)
        for got in (enc.embed_ids(ids, lens), enc.embed_packed(flat, offsets)):
            d, cos = miss(got, want)
            print(f"qk_norm at 64: max|d| {d.max():.4f}, cos min {cos.min():.6f}")
            assert np.isfinite(got).all() and cos.min() >= 0.999, (d, cos)
    finally:
        enc.close()
