"""GPU: the T5 encoder (sc_encoder_cfg.arch 3) through the C ABI -- the bias attention (Head64Rel of attention_core.h) in the rectangle
and packed kernels, the ReLU pass and the tanh-GELU gate on their own, the whole forward against transformers, its refusals.

Bounds.
  Attention against float64 numpy over bf16-rounded q, k, v: max <= 3e-2, median <= 3e-3, the project's bounds for P and O rounded to
  bf16 (tests/test_qwen2_gpu.py).  q is scaled by 1/4 so that the logits' standard deviation is that test's 2 (nothing divides by 8
  here); the arithmetic behind the logits is unchanged, the bias adds one f32 fma.  On every sequence of at least 33 tokens the same numpy
  without the bias, with the mirrored bias or with scores / 8 must exceed the bounds, from 129 tokens on also with max_distance 64.
  ReLU: bit-exact.
  tanh-GELU gate against float64: half a bf16 ulp of the reference plus twice the kernel's f32 term (check_one_bf16_rounding's rule).
  The term, relative, U = 2^-24: the exponent's argument a = -2 log2(e) u carries six roundings (g^2, g^3, the product with 0.044715, the
  sum -- both terms of one sign --, the two constants): 3 U, which exp2 turns into |a| ln2 3 U = 6 |u| U; v_exp_f32 and v_rcp_f32 one ulp
  (2 U) each; 1 + e, g * and * up half an ulp (U / 2) each: (6 |u| + 5.5) U, taken as (6 |u| + 6) U.
  Output projection against float64: |d| <= 2 H 2^-24 sum_k |W_ek x_k| plus one f32 ulp of the result (the f32 MFMA chain of H terms), and
  the normalised form that bound divided by the float64 norm plus three f32 ulps of the result (sum of squares, sqrt / reciprocal, the scale).
  Whole path: T_first / T_mean of tests/golden/t5_golden.json -- twice what transformers' own bf16 forward of that model misses its fp32
  forward by (scripts/gen_t5_fixtures.py) -- and the project's cos >= 0.999.
"""
import json
import math

import numpy as np
import pytest

import fold_ref as fr
import t5_ref as tr
from semcode_amd import _native

pytestmark = pytest.mark.gpu
C = _native.C


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def make_qkv(rows, heads, seed):
    rng = np.random.default_rng(seed)
    scale = np.r_[np.full(heads * 64, 0.25), np.ones(2 * heads * 64)].astype(np.float32)
    return bf16_round(rng.standard_normal((rows, 3 * heads * 64)).astype(np.float32) * scale)


def make_bias(heads, seed, buckets=32):
    return np.random.default_rng(seed).standard_normal((buckets, heads)).astype(np.float32)


class SeqRef:
    """float64 bias attention of one sequence's real rows"""

    def __init__(self, qkv_rows, n, heads, rel_bias, max_distance):
        x = qkv_rows[:n].astype(np.float64)
        H = heads * 64
        self.n, self.heads, self.rb, self.md = n, heads, rel_bias.astype(np.float64), max_distance
        self.q, self.k, self.v = (x[:, i * H:(i + 1) * H].reshape(n, heads, 64).transpose(1, 0, 2) for i in range(3))

    def out(self, bias="model", scale=1.0, max_distance=None):
        n = self.n
        s = self.q @ self.k.transpose(0, 2, 1) * scale
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        if bias != "none":
            bk = tr.buckets((i - j) if bias == "mirrored" else (j - i), self.rb.shape[0], max_distance or self.md)
            s = s + self.rb[bk].transpose(2, 0, 1)
        e = np.exp(s - s.max(-1, keepdims=True))
        return ((e / e.sum(-1, keepdims=True)) @ self.v).transpose(1, 0, 2).reshape(n, self.heads * 64)


def check_bias_attention(got, ref: SeqRef, what):
    err = np.abs(got - ref.out())
    print(f"{what} heads {ref.heads} len {ref.n}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert err.max() <= 3e-2, (what, ref.n, err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 3e-3, (what, ref.n)
    if ref.n >= 33:  # the inputs can tell
        wrong = [("no bias", ref.out(bias="none")), ("mirrored bias", ref.out(bias="mirrored")), ("scores / 8", ref.out(scale=0.125))]
        if ref.n >= 129:
            wrong.append(("max_distance 64", ref.out(max_distance=64)))
        for name, w in wrong:
            e2 = np.abs(got - w)
            assert e2.max() > 3e-2, (what, name, ref.n, e2.max())


RECT_LENS = {32: [32, 1, 31], 64: [64, 33, 1], 256: [256, 129, 65, 33], 1024: [1024, 513, 257, 1], 2048: [2048, 1100, 513]}  # tests/test_qwen2_gpu.py's
RECT_HEADS = {32: [2], 64: [2, 4], 256: [2, 4, 12], 1024: [2, 4], 2048: [2]}
PACKED_LENS = np.array([1, 31, 32, 33, 65, 129, 257, 513, 1100, 2048, 128, 256], np.int32)  # every launch class, both sides of each threshold


# ------------------------------------------------------------------ 1. bias attention
@pytest.mark.parametrize("S", sorted(RECT_LENS))
def test_bias_attention_kernel(rt, S):
    lens = np.array(RECT_LENS[S], np.int32)
    B = len(lens)
    for heads in RECT_HEADS[S]:
        qkv, rb = make_qkv(B * S, heads, 8400 + S + heads), make_bias(heads, 8450 + S + heads)
        row = _native.diag_attention_bias(rt, qkv, lens, B, S, heads, rb, 128)
        assert row.shape == (B * S, heads * 64) and np.isfinite(row).all()  # padding rows are queries too
        if heads == RECT_HEADS[S][-1]:
            blk = _native.diag_attention_bias(rt, qkv, lens, B, S, heads, rb, 128, blocked_rows=B * S + 256)
            assert np.array_equal(bits(blk), bits(row)), int((bits(blk) != bits(row)).sum())  # the layouts hold the same numbers
        for b, n in enumerate(np.minimum(lens, S)):
            check_bias_attention(row[b * S:b * S + n], SeqRef(qkv[b * S:(b + 1) * S], int(n), heads, rb, 128), f"rect S={S}")


def packed_layout(lens):
    span = (lens + 31) // 32 * 32
    starts = (np.cumsum(span) - span).astype(np.int32)
    end = int(span.sum())
    return span, starts, end, (end + 255) // 256 * 256


@pytest.mark.parametrize("heads", [2, 4, 12])
def test_bias_attention_packed_kernel(rt, heads):
    lens = PACKED_LENS if heads <= 4 else PACKED_LENS[[0, 3, 5, 6, 7]]  # 12 heads: one text of every class
    span, starts, end, R = packed_layout(lens)
    assert R > end  # rows beyond the last sequence exist
    qkv, rb = make_qkv(R, heads, 8500 + heads), make_bias(heads, 8550 + heads)
    row = _native.diag_attention_bias_packed(rt, qkv, starts, lens, heads, rb, 128)
    assert row.shape == (R, heads * 64)
    assert np.isnan(row[end:]).all()    # rows of no sequence: untouched
    assert np.isfinite(row[:end]).all()  # alignment rows included
    if heads == 4:
        pad = np.zeros((R + 256, qkv.shape[1]), np.float32)
        pad[:R] = qkv
        blk = _native.diag_attention_bias_packed(rt, pad, starts, lens, heads, rb, 128, blocked_rows=R + 256)
        assert np.array_equal(bits(blk[:R]), bits(row)) and np.isnan(blk[end:]).all()
    for s, n in zip(starts, lens):
        check_bias_attention(row[s:s + n], SeqRef(qkv[s:s + n], int(n), heads, rb, 128), "packed")


def test_bias_attention_other_bucket_counts(rt):
    """(16, 32) and (32, 64): the table is built by the bucket rule, not for the released pair only."""
    lens = np.array([256, 129], np.int32)
    for buckets, md in ((16, 32), (32, 64)):
        qkv, rb = make_qkv(2 * 256, 2, 8600 + buckets), make_bias(2, 8650 + md, buckets)
        row = _native.diag_attention_bias(rt, qkv, lens, 2, 256, 2, rb, md)
        for b, n in enumerate(lens):
            err = np.abs(row[b * 256:b * 256 + n] - SeqRef(qkv[b * 256:(b + 1) * 256], int(n), 2, rb, md).out())
            assert err.max() <= 3e-2 and np.median(err) <= 3e-3, (buckets, md, err.max())


# ------------------------------------------------------------------ 2. ReLU, 3. the tanh-GELU gate
def test_relu_is_bit_exact(rt):
    rng = np.random.default_rng(8700)
    x = bf16_round((rng.standard_normal((37, 136)) * 3).astype(np.float32))
    x[0, :6] = [0.0, -0.0, np.inf, -np.inf, 2.0 ** -130, -(2.0 ** -130)]
    got = _native.diag_ffn_act(rt, 3, x)
    want = np.maximum(x, np.float32(0.0))
    assert np.array_equal(got, want) and not np.signbit(got).any()


U = 2.0 ** -24


def test_tanh_gelu_gate(rt):
    rng = np.random.default_rng(8800)
    rows, F = 67, 264
    gate = rng.uniform(-6.0, 6.0, (rows, F))
    gate[:, :96] = rng.uniform(-4.0, -2.0, (rows, 96))  # where the erf form is ~10 % off: gelu_new(-3) = -0.00364, erf form -0.00405
    up = rng.standard_normal((rows, F))
    up[np.abs(up) < 0.25] = 0.25  # (a factor near zero would hide the activation)
    h = bf16_round(np.concatenate([gate, up], 1).astype(np.float32))
    got = _native.diag_ffn_act(rt, 4, h)
    g, u_ = h[:, :F].astype(np.float64), h[:, F:].astype(np.float64)
    ref = tr.gelu_new(g) * u_
    arg = math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)
    f32term = (6.0 * np.abs(arg) + 6.0) * U * np.abs(ref)
    bar = 0.5 * fr.bf16_ulp(ref) + 2 * f32term
    err = np.abs(got - ref)
    print(f"tanh-GELU gate: err/bar max {float((err / bar).max()):.4f}")
    assert np.isfinite(got).all() and np.all(err <= bar), (float((err / bar).max()), np.unravel_index((err / bar).argmax(), err.shape))
    erf = np.abs(got[:, :96] - (tr.gelu_erf(g) * u_)[:, :96])
    assert np.mean(erf > bar[:, :96]) > 0.9  # the erf form fails the bound there


# ------------------------------------------------------------------ 4. the output projection
def f32_ulp(a):
    a = np.abs(np.asarray(a, np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 23)


@pytest.mark.parametrize("H,E,bias", [(768, 256, True), (256, 256, False), (128, 2048, True), (2048, 16, False), (144, 48, True)])
def test_output_projection_kernel(rt, H, E, bias):
    rng = np.random.default_rng(8900 + H + E)
    B = 37  # two full blocks of 16 rows and a partial one
    x = (rng.standard_normal((B, H)) * rng.uniform(0.1, 10.0, (B, 1))).astype(np.float32)
    x[5] = 0.0  # a zero row: the 1e-12 rule
    W = (rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(E)).astype(np.float32) if bias else None
    x64, W64 = x.astype(np.float64), W.astype(np.float64)
    ref = x64 @ W64.T + (0.0 if b is None else b.astype(np.float64))
    bar = 2.0 * H * U * (np.abs(x64) @ np.abs(W64).T) + f32_ulp(ref)
    raw = _native.diag_output_proj(rt, x, W, b, normalize=False)
    err = np.abs(raw - ref)
    print(f"projection {H} -> {E}: err/bar max {float((err / bar).max()):.4f}")
    assert np.isfinite(raw).all() and np.all(err <= bar), float((err / bar).max())
    got = _native.diag_output_proj(rt, x, W, b, normalize=True)
    nrm = np.maximum(np.linalg.norm(ref, axis=1, keepdims=True), 1e-12)
    refn = ref / nrm
    barn = bar / nrm + 3 * f32_ulp(refn) + np.abs(refn) * (np.linalg.norm(bar, axis=1, keepdims=True) / nrm)  # (the norm's own share of the error)
    errn = np.abs(got - refn)
    assert np.isfinite(got).all() and np.all(errn <= barn), float((errn / barn).max())
    if not bias:
        assert not got[5].any()  # the zero row stays zero


def test_projected_row_does_not_depend_on_its_batch_mates(rt):
    rng = np.random.default_rng(8950)
    H, E = 768, 256
    x = rng.standard_normal((300, H)).astype(np.float32)
    W, b = (rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float32), rng.standard_normal(E).astype(np.float32)
    for normalize in (False, True):
        alone = _native.diag_output_proj(rt, x[:1], W, b, normalize)
        some = _native.diag_output_proj(rt, np.concatenate([x[1:17], x[:1]]), W, b, normalize)  # B = 17: row 0 of a second block
        many = _native.diag_output_proj(rt, x[::-1].copy(), W, b, normalize)                      # B = 300: the last row, another lane of its block
        assert np.array_equal(bits(alone[0]), bits(some[16])) and np.array_equal(bits(alone[0]), bits(many[299]))


# ------------------------------------------------------------------ 5. whole path against transformers
@pytest.fixture(scope="module")
def t5_golden(golden):
    return np.load(golden / "t5_golden.npz"), json.loads((golden / "t5_golden.json").read_text())


def packed_of(ids, lens):
    flat = np.concatenate([ids[i, :n] for i, n in enumerate(lens)]).astype(np.int32)
    return flat, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


CASES = ["relu_s64", "b16_s128", "gated_s512", "aw128_s128", "relu_s1024", "relu_s2048", "base_relu", "dense_mean"]


@pytest.mark.parametrize("name", CASES)
def test_embeddings_against_transformers(rt, t5_golden, name):
    data, meta = t5_golden
    m = meta[name]
    cfg = m["cfg"]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    flat, offsets = packed_of(ids, lens)
    enc = _native.Encoder(rt, cfg, weights=tr.make_weights(cfg, m["seed"], *m["scales"]))
    try:
        assert enc.pooling == "mean" and enc.cfg.arch == 3
        for path in ("small", "batch"):  # split-K and large-tile GEMMs
            enc.set_path(path)
            for pooling in ("first", "mean"):
                enc.pooling = pooling
                T, want = m[f"T_{pooling}"], data[f"{name}_{pooling}"]
                for form, got in (("rectangle", enc.embed_ids(ids, lens)), ("packed", enc.embed_packed(flat, offsets))):
                    d, cos = miss(got, want)
                    print(f"{name} / {path} / {pooling} / {form}: max|d| {d.max():.4f} (T {T:.4f}), cos min {cos.min():.6f}")
                    assert np.isfinite(got).all() and got.shape == want.shape
                    assert d.max() <= T, (path, pooling, form, d)
                    assert cos.min() >= 0.999, (path, pooling, form, cos)
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["base_relu", "dense_mean"])
def test_projected_embeddings_against_transformers(rt, t5_golden, name):
    """The CodeT5+ form (first token -> Linear(768, 256) with bias -> L2) and the sentence-T5 form (mean -> Dense without bias -> L2): every
    embedding entry point returns [B, E] within T_proj of torch's Linear + normalize on transformers' pooled rows."""
    data, meta = t5_golden
    m = meta[name]
    cfg, p = m["cfg"], m["proj"]
    H, E = cfg["hidden"], p["E"]
    ids, lens = data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"].astype(np.int32)
    flat, offsets = packed_of(ids, lens)
    W, b = tr.make_proj(H, E, m["seed"], p["bias"])
    want, T = data[f"{name}_proj"], p["T_proj"]
    enc = _native.Encoder(rt, cfg, weights=tr.make_weights(cfg, m["seed"], *m["scales"]), normalize=True, pooling=p["pooling"])
    try:
        assert enc.out_dim == H
        plain = enc.embed_ids(ids, lens)
        enc.set_output_proj(W, b)
        assert enc.out_dim == E
        for path in ("small", "batch"):
            enc.set_path(path)
            for form, got in (("rectangle", enc.embed_ids(ids, lens)), ("packed", enc.embed_packed(flat, offsets))):
                d, cos = miss(got, want)
                print(f"{name} projected / {path} / {form}: max|d| {d.max():.5f} (T {T:.5f}), cos min {cos.min():.6f}")
                assert got.shape == (len(lens), E) and np.isfinite(got).all()
                assert d.max() <= T, (path, form, d)
                assert cos.min() >= 0.999, (path, form, cos)
                assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-5
        enc.set_path("auto")
        # the _into forms: an index of width E takes the rows, one of width H != E is refused
        rows = np.arange(len(lens), dtype=np.int64)
        ix = _native.Index(rt, E, metric="IP")
        host = enc.embed_ids_into(ids, lens, ix, rows, want_host=True)
        assert len(ix) == len(lens) and np.array_equal(bits(ix.get_rows(0, len(lens))), bits(host)) and miss(host, want)[0].max() <= T
        back = enc.embed_packed_into(flat, offsets, ix, rows, want_host=True)
        assert np.array_equal(bits(ix.get_rows(0, len(lens))), bits(back)) and miss(back, want)[0].max() <= T
        ix.close()
        if H != E:
            wide = _native.Index(rt, H, metric="IP")
            for call in (lambda: enc.embed_ids_into(ids, lens, wide, rows), lambda: enc.embed_packed_into(flat, offsets, wide, rows)):
                with pytest.raises(_native.ScError, match="output projection width"):
                    call()
            wide.close()
        enc.set_output_proj(None)  # cleared: the pooled rows again, the same bits as before
        assert enc.out_dim == H and np.array_equal(bits(enc.embed_ids(ids, lens)), bits(plain))
    finally:
        enc.close()


# ------------------------------------------------------------------ 6. refusals
def test_heads_and_last_token_pooling_are_refused(rt, t5_golden):
    _, meta = t5_golden
    cfg = dict(meta["relu_s64"]["cfg"], vocab=64, layers=1)
    enc = _native.Encoder(rt, cfg, synth_seed=1)
    lib = _native.lib()
    try:
        with pytest.raises(ValueError):
            enc.pooling = "last"
        assert lib.sc_encoder_set_pooling(enc.handle, 2) != 0 and enc.pooling == "mean"
        w = np.zeros((16, cfg["hidden"]), np.float32)
        head = _native.ScoreHead(kind=1, pooling=0, num_labels=1, norm_eps=1e-5)
        ids, off, fl, out = np.ones(32, np.int32), np.array([0, 32], np.int64), np.array([16], np.int32), np.zeros(8, np.float32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        for st in (lib.sc_encoder_set_token_head(enc.handle, p(w), 16), lib.sc_encoder_set_score_head(enc.handle, C.byref(head)),
                   lib.sc_encoder_score_seqs(enc.handle, p(ids), p(off), 1, p(out), None), lib.sc_encoder_score_pairs(enc.handle, p(ids), p(off), p(fl), 1, p(out), None)):
            with pytest.raises(_native.ScError) as err:
                _native._check(st)
            assert "arch 3" in str(err.value)
        info = _native.EncoderCfg()
        assert lib.sc_encoder_info(enc.handle, C.byref(info)) == 0
        assert (info.arch, info.pos_type, info.ffn_type, info.rel_buckets, info.rel_max_distance) == (3, 3, 3, 32, 128)
        assert np.isfinite(enc.embed_ids(np.ones((1, 32), np.int32), np.array([32], np.int32))).all()
    finally:
        enc.close()
    for change, words in ((dict(rel_buckets=31), ("rel_buckets",)), (dict(heads=4), ("head dimension",)), (dict(head_dim=128), ("head_dim",)),
                          (dict(head_dim=64, heads=3), ("attention width",)), (dict(max_pos=4096), ("max_pos",))):
        with pytest.raises(_native.ScError) as err:
            _native.Encoder(rt, dict(cfg, **change), synth_seed=1)
        assert all(w_ in str(err.value) for w_ in words), (change, str(err.value))


def test_output_projection_on_arch_0_and_its_rules(rt):
    """Accepted on every arch: a BERT-shaped encoder returns [B, E] = normalise(W mean + b); clearing restores out_dim and the bits."""
    cfg = dict(_native.BERT_BASE, vocab=64, layers=1, hidden=128, heads=2, ffn=256, max_pos=64)
    rng = np.random.default_rng(9000)
    ids, lens = rng.integers(1, 64, size=(3, 32)).astype(np.int32), np.array([32, 7, 1], np.int32)
    W, b = rng.standard_normal((48, 128)).astype(np.float32), rng.standard_normal(48).astype(np.float32)
    raw_enc = _native.Encoder(rt, cfg, synth_seed=3)             # un-normalised pooled rows: what the projection reads
    enc = _native.Encoder(rt, cfg, synth_seed=3, normalize=True)
    try:
        pooled, before = raw_enc.embed_ids(ids, lens), enc.embed_ids(ids, lens)
        assert enc.out_dim == 128
        enc.set_output_proj(W, b)
        assert enc.out_dim == 48
        got = enc.embed_ids(ids, lens)
        assert got.shape == (3, 48) and np.abs(got - tr.project(pooled, W, b)).max() <= 1e-5
        enc.pooling = "cls"
        raw_enc.pooling = "cls"
        assert np.abs(enc.embed_ids(ids, lens) - tr.project(raw_enc.embed_ids(ids, lens), W, b)).max() <= 1e-5
        enc.pooling = "mean"
        lib = _native.lib()
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        for E in (0, 8, 40, 2064):
            assert lib.sc_encoder_set_output_proj(enc.handle, p(W), p(b), E) != 0 and enc.out_dim == 48  # refused, the installed one stays
        enc.set_output_proj(None)
        assert enc.out_dim == 128 and np.array_equal(bits(enc.embed_ids(ids, lens)), bits(before))
    finally:
        enc.close()
        raw_enc.close()


def test_embeddings_client_reads_a_t5_directory(rt, tmp_path):
    """MI355XEmbeddings(weights=<directory>): config.json, weights, proj.* of a CodeT5+-style directory, first-token pooling and tokenizer.json
    are wired up; the client reports the projection's width and returns the vectors the numpy restatement gives for the same ids."""
    from safetensors.numpy import save_file
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace

    from semcode_amd.embeddings.providers import MI355XEmbeddings

    words = ["<pad>", "<unk>"] + [f"w{i}" for i in range(62)]
    cfg = dict(vocab=64, hidden=128, layers=2, heads=2, ffn=256, max_pos=2048, type_vocab=1, ln_eps=1e-6, t5=True, t5_ffn="relu", rel_buckets=32, rel_max_distance=128)
    blob = tr.make_weights(cfg, 9)
    W, b = tr.make_proj(128, 48, 9, True)
    d = tmp_path / "codet5p"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(tr.hf_config(cfg), model_type="codet5p_embedding", embed_dim=48)))
    save_file(dict(tr.to_hf_state_dict(cfg, blob), **{"proj.weight": W, "proj.bias": b}), str(d / "model.safetensors"))
    tok = Tokenizer(WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    tok.save(str(d / "tokenizer.json"))
    texts = [" ".join(f"w{(7 * i + j) % 62}" for j in range(n)) for i, n in enumerate((40, 5, 1))]
    client = MI355XEmbeddings(weights=d, runtime=rt, normalize=True, max_tokens=64)
    try:
        assert client.pooling == "first" and client.dimension == 48
        got = client.embed_documents_array(texts)
        ids = np.zeros((3, 64), np.int32)
        lens = np.array([40, 5, 1], np.int32)
        for i, t in enumerate(texts):
            ids[i, :lens[i]] = tok.encode(t).ids
        want = tr.project(tr.forward(cfg, blob, ids, lens, "first"), W, b)
        d_, cos = miss(got, want)
        print(f"client on a T5 directory: max|d| {d_.max():.5f}, cos min {cos.min():.6f}")
        assert got.shape == (3, 48) and cos.min() >= 0.999, (d_, cos)  # the project's floor (no T exists for this ad-hoc model: the golden cases carry those)
    finally:
        client.close()
