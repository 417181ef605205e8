"""GPU: single-kernel parity of the LayerNorm-folded batch pipeline and of the stand-alone encoder kernels.

Every kernel runs ONCE through the product's own launcher (sc_diag_* of include/semcode_hip.h) on host data and is held against the
float64 stage of tests/fold_ref.py on the same bf16-rounded inputs; the stages chained reproduce oracle.bert_oracle.forward
(tests/test_fold_reference.py, CPU).  u = 2^-24 is the unit roundoff of f32 throughout; a summation of f32 terms t_i along any tree of
depth d is off by at most d u sum |t_i| (first order), which is where every "derived" bound below comes from.

Kernels launched by forward_locked / forward_folded_locked, and the test that names each:

    embed_raw_kernel                                  test_embed_raw_kernel
    embed_ln_kernel                                   test_embed_ln_kernel
    fold_ln_weights_kernel (sc_encoder_create)        test_fold_ln_weights_kernel
    gemm256_bf16_kernel<EPI_LNA_BIAS>                 test_lna_gemm, test_resln_output_feeds_an_lna_gemm
    gemm256_bf16_kernel<EPI_LNA_GELU>                 test_lna_gemm
    gemm256_bf16_kernel<EPI_LNA_BIAS_ROPE>            test_lna_gemm (rotary part)
    gemm256_bf16_kernel<EPI_RESLN_STATS>              test_resln_gemm, test_resln_output_feeds_an_lna_gemm
      cblock / ablock / nt stores / one-barrier loop  test_lna_gemm, test_resln_gemm (bit-identity of the variants)
    gemm256_bf16_kernel<EPI_BIAS|_GELU|_RES>          test_gemm_plain_gpu.py::test_256_tile_dense_and_blocked (cblock / ablock),
                                                      test_256_tile_switches (nt stores, both main loops and residual hooks),
                                                      test_walk_orders (tile_coords256), test_128_tile_against_256_tile;
                                                      test_encoder_gpu.py::test_gemm_kernel, test_gelu_epilogue_accuracy
    gemm_bf16_kernel (128-tile)                       test_gemm_plain_gpu.py::test_128_tile_dense_and_blocked_c,
                                                      test_128_tile_against_256_tile; test_encoder_gpu.py::test_gemm_kernel
    gemm256_splitk_kernel + gemm_splitk_reduce_kernel test_gemm_plain_gpu.py::test_splitk; test_encoder_gpu.py::test_gemm_kernel
    gemm256_i8_diag_kernel (the int8 tile loop)       test_gemm_plain_gpu.py::test_int8_tile_loop_is_exact
    attention_kernel / attention_long_kernel          test_encoder_gpu.py::test_attention_kernel (row-major, no bias);
                                                      test_attention_blocked_layout, test_attention_alibi (as the pipelines call it)
    rope_qk_kernel, glu_kernel<ActSilu>               test_nomic_gpu.py::test_rope_kernel, test_swiglu_kernel
    glu_kernel<ActGelu>                               test_geglu_kernel
    layernorm_kernel<3|4|8>                           test_layernorm_kernel
    mean_pool_kernel, mean_pool_sliced_kernel         test_mean_pool_kernels
    mean_pool_ln_kernel                               test_mean_pool_ln_kernel
    add_vectors_kernel (b + beta at create time)      one f32 add per element; covered end to end only
"""
import numpy as np
import pytest

import fold_ref as fr
from fold_ref import LARGE_MEAN, ORDINARY, TINY_VAR, UNEVEN, ZERO, U, bf16_round
from oracle import bert_oracle as bo
from semcode_amd import _native

pytestmark = pytest.mark.gpu

EPS = 1e-12  # BERT's LayerNorm epsilon: the value that lets rs reach 1e6 on a zero row


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def gemm_options():
    """Hands out a setter of the process-wide GEMM switches and puts the defaults back afterwards."""
    def set_(nt=-1, pp=-1):
        _native.diag_set_option("gemm_nt", nt)
        _native.diag_set_option("gemm_pp", pp)
    yield set_
    set_()


def f32_stats(A):
    """The statistics a caller supplies: float64 partial sums of the bf16 rows per 256-column slot, rounded to f32."""
    return fr.slot_stats(A).astype(np.float32)


def fin_bounds(stats32, K, eps):
    """(mu, rs) in float64 of the SUPPLIED f32 statistics, and bounds on what gemm256_epilogue_lna may publish instead.

    The kernel adds the `slots` partial sums sequentially in f32 (slots - 1 roundings), multiplies by an f32 1/K (its rounding + the
    product's: 2 more), so |d mu| <= (slots + 1) u sum_t |s1_t| / K, and the same factor on E[y^2] = sum_t s2_t / K.  The variance is
    fma(-mu, mu, E[y^2]) -- one rounding, u |var| <= u (E[y^2] + mu^2) -- and inherits 2 |mu| |d mu| + |d mu|^2 from mu: this is the
    E[y^2] - mu^2 cancellation, relative to var it grows as (mu / sigma)^2.  max(., 0) + eps rounds once more (u), v_rsq_f32 is good to
    1 ulp (2^-23 relative): rs lies between 1 / sqrt(var + dvar + eps) and 1 / sqrt(max(var - dvar, 0) + eps), widened by 4 u."""
    s = np.asarray(stats32, np.float64)
    slots = s.shape[0]
    fin = fr.finalise(s, K, eps)
    mu, rs = fin[:, 0], fin[:, 1]
    dmu = (slots + 1) * U * np.abs(s[:, :, 0]).sum(0) / K
    e2 = s[:, :, 1].sum(0) / K
    var = np.maximum(e2 - mu * mu, 0.0)
    dvar = (slots + 1) * U * e2 + U * (e2 + mu * mu) + 2 * np.abs(mu) * dmu + dmu * dmu
    rs_hi = (1 + 4 * U) / np.sqrt(np.maximum(var - dvar, 0.0) + eps)
    rs_lo = (1 - 4 * U) / np.sqrt(var + dvar + eps)
    return mu, rs, dmu, rs_lo, rs_hi


def lna_extra_bound(A, Wf, c1, c2, ref_lin, stats32, eps):
    """What f32 adds to an EPI_LNA_* output beyond the ordinary bar, per element, for rows whose mean is not small.

    The kernel forms v = rs acc + (c2 - rs mu c1) from acc = sum_k a_k w'_k (MFMA, f32 accumulate).  With T = sum_k |a_k w'_k|:
      * acc is off by at most 2 K u T (K additions; the factor 2 allows for an accumulator that truncates instead of rounding),
        scaled by rs;
      * the two FMAs and the product rs mu round three times on numbers of size |rs mu c1|, |c2| and |v|:
        u (3 rs |mu c1| + |c2| + |v|);
      * these two are the cancellation the issue names: for a row with mean mu, rs acc and rs mu c1 are both ~ rs |mu c1| and their
        difference is the O(1) result;
      * mu itself is off by d mu (fin_bounds): rs |c1| d mu;
      * rs is off by the relative amount fin_bounds allows, which scales the normalised part v - c2."""
    mu, rs, dmu, rs_lo, rs_hi = fin_bounds(stats32, A.shape[1], eps)
    T = np.abs(A).astype(np.float64) @ np.abs(Wf).astype(np.float64).T
    rel_rs = np.maximum(rs_hi / rs - 1.0, 1.0 - rs_lo / rs)
    c1a, c2a = np.abs(c1).astype(np.float64), np.abs(c2).astype(np.float64)
    return (rs[:, None] * 2 * A.shape[1] * U * T + U * (3 * (rs * np.abs(mu))[:, None] * c1a + c2a + np.abs(ref_lin))
            + (rs * dmu)[:, None] * c1a + rel_rs[:, None] * np.abs(ref_lin - c2.astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("N,K,with_bias", [(256, 256, True), (770, 768, True), (3, 1024, False), (261, 2048, True), (1, 768, False)])
def test_fold_ln_weights_kernel(rt, N, K, with_bias):
    """W' bit-exact against bf16(f32(W) * f32(gamma)).  c1 = sum_k W'[n,k] and c2 = b + sum_k beta_k W[n,k] are f32 sums of K terms
    taken as K/256 sequential steps of 4 per lane, then a 6-level wave reduction: any path has at most K/64 + 6 additions, the FMA
    products of c2 round once each and the bias add once, so
        |c1 - ref| <= (K/64 + 6) u sum_k |W'[n,k]|,      |c2 - ref| <= (K/64 + 8) u (sum_k |beta_k W[n,k]| + |b_n|).
    N values that are not a multiple of the 4 rows of a workgroup, and no bias, are among the cases.
    Observed on an MI355X (2026-10-17): c1 at most 0.021 of its bound, c2 at most 0.032."""
    rng = np.random.default_rng(N + K)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    g, be = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) if with_bias else None
    Wf, c1, c2 = _native.diag_fold_ln(rt, W, g, be, b)
    assert np.array_equal(bits(Wf), bits(bf16_round(W * g[None, :])))
    Wd, W64 = Wf.astype(np.float64), W.astype(np.float64)
    d = K // 64 + 6
    b1 = d * U * np.abs(Wd).sum(1)
    terms = W64 * be.astype(np.float64)
    b2 = (d + 2) * U * (np.abs(terms).sum(1) + (np.abs(b) if with_bias else 0.0))
    e1 = np.abs(c1 - Wd.sum(1))
    e2 = np.abs(c2 - (terms.sum(1) + (b.astype(np.float64) if with_bias else 0.0)))
    print(f"fold N={N} K={K}: c1 err/bound {np.max(e1 / b1):.3f}, c2 err/bound {np.max(e2 / b2):.3f}")
    assert np.all(e1 <= b1), (e1 / b1).max()
    assert np.all(e2 <= b2), (e2 / b2).max()


# ----------------------------------------------------------------------------------------------------------- LNA GEMMs
def lna_inputs(rt, M, N, K, seed):
    rng = np.random.default_rng(seed)
    A, kind = fr.make_rows(rng, M, K)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    g, be = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    Wf, c1, c2 = _native.diag_fold_ln(rt, W, g, be, b)  # the device's own W': the fold's rounding is not charged to the GEMM
    c2_ref = b.astype(np.float64) + W.astype(np.float64) @ be.astype(np.float64)  # ... but a c2 that lost beta or b would be
    return A, kind, Wf, c1, c2, c2_ref


def check_fin(fin, stats32, K, eps, tag):
    """fin must hold (mu, rs) of EVERY row (the buffer starts as NaN; only the n0 == 0 column tiles write it)."""
    mu, rs, dmu, rs_lo, rs_hi = fin_bounds(stats32, K, eps)
    assert np.isfinite(fin).all(), (tag, "fin rows never written", np.nonzero(~np.isfinite(fin).all(1))[0][:8])
    emu = np.abs(fin[:, 0] - mu)
    worst = float(np.max(emu / np.maximum(dmu, 1e-300) * (emu > 0)))
    wrs = float(np.max(np.maximum(fin[:, 1] / rs_hi, rs_lo / fin[:, 1])))
    print(f"{tag}: fin mu err/bound {worst:.3f}; rs max rel err {np.max(np.abs(fin[:, 1] / rs - 1)):.2e} (inside its interval by {1 - wrs:+.2e})")
    assert np.all(emu <= dmu), (tag, worst)
    assert np.all((fin[:, 1] >= rs_lo) & (fin[:, 1] <= rs_hi)), (tag, wrs)


def rope_extra(extra, lin, ncols):
    """A rotated value x cos - y sin mixes columns j and j + 32 of a head with |cos| + |sin| <= sqrt 2, in two more roundings on f32
    table entries: sqrt 2 max(extra_j, extra_j+32) + 4 u (|x| + |y|)."""
    ex = np.array(extra)
    for h0 in range(0, ncols, 64):
        a, b = slice(h0, h0 + 32), slice(h0 + 32, h0 + 64)
        m = np.sqrt(2.0) * np.maximum(extra[:, a], extra[:, b]) + 4 * U * (np.abs(lin[:, a]) + np.abs(lin[:, b]))
        ex[:, a] = m
        ex[:, b] = m
    return ex


def check_lna_output(got, ref, extra, kind, tag, ulps=0.5, floor=0.0):
    """Ordinary rows: test_gemm_kernel's bar, scale 2^-8 + 1e-3 (one bf16 output rounding of the output scale + accumulation noise).
    Rows with a mean (LARGE_MEAN, TINY_VAR, UNEVEN) add the f32 term `extra` (lna_extra_bound / resln_extra_bound).
    Since every element's error is at most `ulps` bf16 ulp (half an ulp <= 2^-9 |ref|; test_gelu_epilogue_accuracy's 0.64 ulp + 1e-6
    where the fast GELU sits in front of the rounding) plus that f32 term, the RMS error over the ordinary rows is at most
    2 ulps 2^-9 RMS(ref) + floor + RMS(extra): a relative bar the scale-wide one cannot give."""
    assert np.isfinite(got).all(), (tag, "non-finite output")
    scale = max(1.0, float(np.abs(ref).max()))
    bar = np.full(ref.shape, scale * 2.0 ** -8 + 1e-3)
    special = np.isin(kind, (LARGE_MEAN, TINY_VAR, UNEVEN))
    bar[special] += extra[special]
    err = np.abs(got - ref)
    o = kind == ORDINARY
    rms_err = np.sqrt((err[o] ** 2).mean())
    rms_bar = 2 * ulps * 2.0 ** -9 * np.sqrt((ref[o] ** 2).mean()) + floor + np.sqrt((extra[o] ** 2).mean())
    names = ("ordinary", "large-mean", "tiny-variance", "zero", "uneven")
    per = {names[k]: round(float((err[kind == k] / bar[kind == k]).max()), 3) for k in range(5) if (kind == k).any()}
    ext = {names[k]: float(f"{extra[kind == k].max():.2e}") for k in (LARGE_MEAN, TINY_VAR, UNEVEN) if (kind == k).any()}
    print(f"{tag}: max err/bar {per}; ordinary rms err/bar {rms_err / rms_bar:.3f}; largest f32 term {ext}")
    assert np.all(err <= bar), (tag, float((err / bar).max()), np.unravel_index((err / bar).argmax(), err.shape))
    assert rms_err <= rms_bar, (tag, rms_err, rms_bar)


LNA_SHAPES = [(256, 256, 256), (512, 768, 768), (1280, 2304, 768), (256, 3072, 1024), (512, 768, 2048), (1280, 3072, 2048)]


@pytest.mark.parametrize("M,N,K", LNA_SHAPES)
def test_lna_gemm(rt, gemm_options, M, N, K):
    """EPI_LNA_BIAS, EPI_LNA_GELU and EPI_LNA_BIAS_ROPE against LayerNorm(bf16 A) W'^T + c2 computed the plain way (normalise every
    row with its own mean and variance, then multiply) -- 1, 3, 4 and 8 statistics slots, both tile-walk orders (N K 2 > 8 MiB at
    3072 x 2048), five row populations in one matrix (fold_ref.make_rows), N(0,1) gamma / beta / bias.
    Bars: check_lna_output, check_fin (derivations there).  All-zero rows: finite and exactly bf16(c2) (rs = 1e6 multiplies an exact
    0), gelu(c2) within the ordinary bar.  Variants -- C in 64-column blocks, non-temporal stores, the one-barrier main loop, all three
    together -- must repeat C and fin bit for bit.  Rotary form: Q / K columns against the float64 rotation of the reference before
    its one rounding, V columns bit-identical to EPI_LNA_BIAS, S in {32, 512, 2048} x theta in {1000, 10000}.
    TINY_VAR rows (|mu| / sigma ~ 140, sigma ~ 2^-6, rs ~ 45): the one-pass variance E[y^2] - mu^2 in f32 loses (mu / sigma)^2 u of rs
    by construction -- 1.4e-3 relative observed, inside fin_bounds -- and rs scales the accumulator's worst-case error, so the derived
    term is large there (0.07 at K = 256, 1.6 at K = 2048); the kernel uses 1.5 % - 21 % of it and would in fact meet the ordinary bar.
    These rows stay in contract with the derived bar ("LayerNorm folded into the GEMMs").
    Observed on an MI355X (2026-10-17), largest err / bar over all shapes and epilogues: ordinary 0.87, large-mean 0.70, tiny-variance
    0.21, zero 0.51, uneven 0.75; ordinary-row RMS error at most 0.79 of its bar; fin: mu at most 0.60 of its bound, rs off by at most
    1.4e-3 relative (the tiny-variance rows; 1.3e-7 on all others), every variant bit-identical."""
    A, kind, Wf, c1, c2, c2_ref = lna_inputs(rt, M, N, K, M + N + K)
    st = f32_stats(A)
    lin = fr.lna_with_folded_weight(A, Wf, c2_ref, EPS)
    extra = lna_extra_bound(A, Wf, c1, c2, lin, st, EPS)
    zero = kind == ZERO
    ncols = (2 * N // 3) // 64 * 64
    rope_cfg = {256: (32, 1000.0), 768: (512, 10000.0), 2304: (2048, 10000.0), 3072: (2048, 1000.0)}[N]
    base = {}
    for epi, name in ((3, "bias"), (4, "gelu"), (6, "rope")):
        tag = f"lna {name} {M}x{N}x{K}"
        rope = dict(rope_S=rope_cfg[0], rope_theta=rope_cfg[1], rope_ncols=ncols) if epi == 6 else {}
        gemm_options(nt=0, pp=-1)
        got, fin = _native.diag_gemm_lna(rt, epi, A, Wf, c1, c2, st, EPS, **rope)
        base[epi] = got
        check_fin(fin, st, K, EPS, tag)
        kw = {}
        if epi == 3:
            ref, ex = lin, extra
            assert np.array_equal(bits(got[zero]), bits(np.broadcast_to(bf16_round(c2), (M, N))[zero])), tag
        elif epi == 4:
            ref, ex = fr.gelu(lin), 1.13 * extra  # |gelu'| <= 1.13: the f32 term passes through at most that much larger
            kw = dict(ulps=0.64, floor=1e-6)
            assert np.all(bits(got[zero]) == bits(got[zero][0])), tag
        else:
            ref, ex = fr.rope_rotate(lin, rope_cfg[0], rope_cfg[1], ncols), rope_extra(extra, lin, ncols)
            assert np.array_equal(bits(got[:, ncols:]), bits(base[3][:, ncols:])), (tag, "V columns differ from EPI_LNA_BIAS")
            assert np.abs(got[:, :ncols] - base[3][:, :ncols]).max() > 0.1, (tag, "nothing was rotated")
        check_lna_output(got, ref, ex, kind, tag, **kw)
        for blocked, nt, pp in ((True, 0, -1), (False, 1, -1), (False, 0, 0), (True, 1, 0)):
            gemm_options(nt=nt, pp=pp)
            g2, f2 = _native.diag_gemm_lna(rt, epi, A, Wf, c1, c2, st, EPS, blocked=blocked, **rope)
            assert np.array_equal(bits(g2), bits(got)) and np.array_equal(bits(f2), bits(fin)), (tag, blocked, nt, pp, int((bits(g2) != bits(got)).sum()))
    if N == 2304 or N == 256:  # the other sequence lengths and theta on one wide and one narrow shape
        for S, theta in ((32, 10000.0), (512, 1000.0), (2048, 1000.0)):
            gemm_options(nt=0, pp=-1)
            got, _ = _native.diag_gemm_lna(rt, 6, A, Wf, c1, c2, st, EPS, blocked=True, rope_S=S, rope_theta=theta, rope_ncols=ncols)
            ref = fr.rope_rotate(lin, S, theta, ncols)
            check_lna_output(got, ref, rope_extra(extra, lin, ncols), kind, f"lna rope S={S} theta={theta:g} {M}x{N}x{K}")
            assert np.array_equal(bits(got[:, ncols:]), bits(base[3][:, ncols:]))


def test_lna_gemm_rejects_what_the_kernel_cannot_take(rt):
    A = np.zeros((256, 256), np.float32)
    v = np.zeros(256, np.float32)
    st = np.zeros((1, 256, 2), np.float32)
    with pytest.raises(_native.ScError):
        _native.diag_gemm_lna(rt, 5, A, A, v, v, st, EPS)  # not an LNA epilogue
    with pytest.raises(_native.ScError):
        _native.diag_gemm_lna(rt, 6, A, A, v, v, st, EPS, rope_S=48, rope_ncols=128)  # S not a power of two
    with pytest.raises(_native.ScError):
        _native.diag_gemm_lna(rt, 3, A[:128], A, v, v, st[:, :128], EPS)  # M not a multiple of 256
    with pytest.raises(_native.ScError):
        _native.diag_set_option("gemm_no_such_option", 1)


# ---------------------------------------------------------------------------------------------------------- RESLN GEMM
def resln_extra_bound(A, W, bias, gam, R, fin32, ref):
    """f32 terms of EPI_RESLN_STATS beyond the ordinary bar: acc off by 2 K u T (as in lna_extra_bound); (r - mu) is exact or rounds
    once, rs gam rounds once, the FMA once, acc + bias once: u (3 |r - mu| rs |gam| + |acc + bias| + |ref|); and the supplied f32
    (mu, rs) are the float64 values rounded: u |mu| rs |gam| + u |r - mu| rs |gam|."""
    K = A.shape[1]
    T = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    mu, rs = fin32[:, 0:1].astype(np.float64), fin32[:, 1:2].astype(np.float64)
    res = np.abs(R.astype(np.float64) - mu) * rs * np.abs(gam).astype(np.float64)
    return 2 * K * U * T + U * (4 * res + T + np.abs(bias).astype(np.float64) + np.abs(ref) + np.abs(mu) * rs * np.abs(gam).astype(np.float64))


def check_stats_out(stats, C, tag):
    """stats_out against sums of the device's own C (bf16 values: exactly representable, so float64 sums of them are exact): per row
    and 256-column tile, 256 terms x u = 2^-16 of sum |C| (and of sum C^2: the squares are FMA'd, one rounding each, same count).
    Isolates the reduction -- lane, __shfl_xor over the 4 k-groups, four waves through LDS -- from the GEMM."""
    want = fr.slot_stats(C)
    babs = 2.0 ** -16 * np.stack([fr.slot_stats(np.abs(C))[:, :, 0], want[:, :, 1]], axis=-1)
    assert np.isfinite(stats).all(), (tag, "stats_out not fully written")
    err = np.abs(stats - want)
    print(f"{tag}: stats_out err/bound max {np.max(err / np.maximum(babs, 1e-300) * (err > 0)):.3f}")
    assert np.all(err <= babs), (tag, np.unravel_index((err - babs).argmax(), err.shape))


RESLN_SHAPES = [(256, 256, 256, False), (512, 768, 768, False), (1280, 768, 3072, False), (1280, 768, 3072, True), (512, 1024, 768, False),
                (256, 1024, 3072, True)]


@pytest.mark.parametrize("M,N,K,a_blocked", RESLN_SHAPES)
def test_resln_gemm(rt, gemm_options, M, N, K, a_blocked):
    """EPI_RESLN_STATS against A W^T + (b + beta) + normalise(R) gam in float64 (R carries the five row populations, (mu, rs) are
    supplied from float64, gam / bias N(0,1)); C: the LNA GEMMs' bar (check_lna_output) with resln_extra_bound; stats_out:
    check_stats_out.  K = 3072 also reads A in 64-column blocks, as FFN2 reads the FFN hidden tensor -- bit-identical to row-major A.
    Non-temporal stores and the one-barrier main loop (its *TailHook fetches the residual tile and the statistics instead of the
    default *CoopHook) must repeat C and the statistics bit for bit.
    Observed on an MI355X (2026-10-17): C err / bar at most 0.72, ordinary-row RMS at most 0.77 of its bar; stats_out at most 0.011 of its
    bound; every variant bit-identical."""
    rng = np.random.default_rng(M + N + K)
    A = bf16_round(rng.standard_normal((M, K)).astype(np.float32))
    W = bf16_round((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
    bias, gam = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    R, kind = fr.make_rows(rng, M, N)
    fin = fr.finalise(fr.slot_stats(R), N, EPS).astype(np.float32)
    ref = fr.resln(A, W, bias, gam, R, EPS)
    tag = f"resln {M}x{N}x{K}{' A blocked' if a_blocked else ''}"
    gemm_options(nt=0, pp=-1)
    C, st = _native.diag_gemm_resln(rt, A, W, bias, gam, R, fin, EPS, a_blocked=a_blocked)
    check_lna_output(C, ref, resln_extra_bound(A, W, bias, gam, R, fin, ref), kind, tag)
    check_stats_out(st, C, tag)
    for ab, nt, pp in ((a_blocked, 1, -1), (a_blocked, 0, 0), (a_blocked, 1, 0), (not a_blocked, 0, -1)):
        gemm_options(nt=nt, pp=pp)
        C2, st2 = _native.diag_gemm_resln(rt, A, W, bias, gam, R, fin, EPS, a_blocked=ab)
        assert np.array_equal(bits(C2), bits(C)) and np.array_equal(bits(st2), bits(st)), (tag, ab, nt, pp, int((bits(C2) != bits(C)).sum()))


def test_resln_output_feeds_an_lna_gemm(rt, gemm_options):
    """The real hand-over on device-produced numbers: EPI_RESLN_STATS leaves y [512, 768] and its partial statistics in 3 slots; an
    EPI_LNA_BIAS GEMM with K = 768 consumes both.  Reference: float64 LayerNorm of the producer's RETURNED y (bf16, exact), times W'.
    Observed on an MI355X (2026-10-17): err / bar at most 0.79; fin mu at most 0.41 of its bound."""
    M, N, K = 512, 768, 768
    rng = np.random.default_rng(77)
    A = bf16_round(rng.standard_normal((M, K)).astype(np.float32))
    W = bf16_round((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
    bias, gam = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    R, kind = fr.make_rows(rng, M, N)
    fin = fr.finalise(fr.slot_stats(R), N, EPS).astype(np.float32)
    gemm_options()
    y, st = _native.diag_gemm_resln(rt, A, W, bias, gam, R, fin, EPS)
    N2 = 1024
    W2 = (rng.standard_normal((N2, N)) / np.sqrt(N)).astype(np.float32)
    g2, be2, b2 = (rng.standard_normal(n).astype(np.float32) for n in (N, N, N2))
    Wf, c1, c2 = _native.diag_fold_ln(rt, W2, g2, be2, b2)
    c2_ref = b2.astype(np.float64) + W2.astype(np.float64) @ be2.astype(np.float64)
    got, fin2 = _native.diag_gemm_lna(rt, 3, y, Wf, c1, c2, st, EPS, blocked=True)
    check_fin(fin2, st, N, EPS, "handover")
    # the producer's statistics are sums of the rows it returned: fin is also the moments of y itself
    true = fr.finalise(fr.slot_stats(y), N, EPS)
    assert np.abs(fin2[:, 0] - true[:, 0]).max() <= 1e-5 and np.abs(fin2[:, 1] / true[:, 1] - 1).max() <= 1e-3
    lin = fr.lna_with_folded_weight(y, Wf, c2_ref, EPS)
    extra = lna_extra_bound(y, Wf, c1, c2, lin, st, EPS)
    check_lna_output(got, lin, extra, np.where(kind == ORDINARY, ORDINARY, LARGE_MEAN), "handover")


# ------------------------------------------------------------------------------------------------------ embedding kernels
def embed_tables(rng, vocab, max_pos, H):
    return (rng.standard_normal((vocab, H)).astype(np.float32), rng.standard_normal((max_pos, H)).astype(np.float32),
            rng.standard_normal((2, H)).astype(np.float32))


def embed_ids(rng, B, S, vocab):
    ids = rng.integers(0, vocab, (B, S)).astype(np.int32)
    ids[0, :6] = [-1, -2 ** 31, vocab, vocab + 7, 2 ** 31 - 1, 0]  # out of range on both sides: must clamp
    return ids


@pytest.mark.parametrize("H", [128, 384, 768, 1024, 2048])
@pytest.mark.parametrize("with_pos", [True, False])
def test_embed_raw_kernel(rt, H, with_pos):
    """Rows bit-exact against bf16 of the f32 sum in the kernel's documented order (word + position) + type; ids < 0 and >= vocab clamp,
    positions >= max_pos clamp (S = 32 > max_pos = 20); 3 x 32 + padding: tokens = 96 is not what tokens_pad = 131 is, and 131 is not a
    multiple of the 4 rows of a workgroup.  Padding rows are zero with zero statistics, slots 1.. are exactly 0, slot 0 holds the sums
    of the RETURNED rows: a lane adds its <= 32 values sequentially, the wave reduces in 6 levels, so
    |sum - ref| <= 38 u sum |y| and likewise for the squares.
    Observed on an MI355X (2026-10-17): rows bit-exact; statistics at most 0.052 of the bound."""
    rng = np.random.default_rng(H)
    vocab, max_pos, B, S, tp, slots = 50, 20, 3, 32, 131, max(1, H // 256)
    wemb, pemb, temb = embed_tables(rng, vocab, max_pos, H)
    ids = embed_ids(rng, B, S, vocab)
    rows, stats = _native.diag_embed(rt, ids, wemb, pemb if with_pos else None, temb, max_pos, tokens_pad=tp, slots=slots)
    want = bf16_round(fr.embed_sum(ids, wemb, pemb if with_pos else None, temb, max_pos, dtype=np.float32))
    assert np.array_equal(bits(rows[: B * S]), bits(want))
    assert not rows[B * S:].any() and not stats[:, B * S:].any() and not stats[1:].any()
    ref = fr.embed_slot_stats(rows[: B * S], 1)[0]
    bound = 38 * U * np.stack([np.abs(rows[: B * S]).astype(np.float64).sum(1), ref[:, 1]], axis=1)
    err = np.abs(stats[0, : B * S] - ref)
    print(f"embed_raw H={H}: stats err/bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


def ln_f32_term(x, g, ref, depth):
    """f32 term of a LayerNorm kernel that subtracts the mean first: the mean is a `depth`-deep sum, |d mu| <= depth u mean |x|, which
    moves every output by rs |g| d mu; the centred sum of squares is as deep and enters rs by half its relative error,
    (depth + 4) u / 2 with the division, square root and epsilon, plus what the shifted mean does to the centred squares
    (2 |d mu| mean |x - mu| + d mu^2, second order except on near-constant rows); (x - mu) rs g rounds three times and + b once."""
    x = np.asarray(x, np.float64)
    mu, var = fr.row_moments(x)
    rs = 1.0 / np.sqrt(var + EPS)
    xh = np.abs(x - mu) * rs * np.abs(g)
    dmu = depth * U * np.abs(x).mean(-1, keepdims=True)
    rel_rs = (depth + 4) * U / 2 + (2 * dmu * np.abs(x - mu).mean(-1, keepdims=True) + dmu * dmu) / (2 * (var + EPS))
    return rs * np.abs(g) * dmu + (rel_rs + 3 * U) * xh + U * np.abs(ref)


def check_one_bf16_rounding(got, ref, f32term, tag):
    """Half a bf16 ulp of the reference plus the kernel's f32 term (which may also carry the value across a rounding boundary: counted
    twice)."""
    err = np.abs(got - ref)
    bar = 0.5 * fr.bf16_ulp(ref) + 2 * f32term
    print(f"{tag}: err/bar max {float((err / bar).max()):.4f}; median bar {float(np.median(bar / fr.bf16_ulp(ref))):.4f} bf16 ulp")
    assert np.isfinite(got).all(), tag
    assert np.all(err <= bar), (tag, float((err / bar).max()), np.unravel_index((err / bar).argmax(), err.shape))


@pytest.mark.parametrize("H", [128, 384, 768, 1024, 2048])
@pytest.mark.parametrize("with_pos", [True, False])
def test_embed_ln_kernel(rt, H, with_pos):
    """LayerNorm of the same f32 sum, one wave per row (a lane adds <= 32 values, 6 reduction levels: depth 38), one bf16 rounding:
    check_one_bf16_rounding with ln_f32_term.  99 tokens: not a multiple of 4.
    Observed on an MI355X (2026-10-17): largest err / bar 1.000 to three decimals, never above 1 (errors reach half an ulp, as those of a
    correctly rounded result do)."""
    rng = np.random.default_rng(H + 1)
    vocab, max_pos, B, S = 50, 20, 3, 33
    wemb, pemb, temb = embed_tables(rng, vocab, max_pos, H)
    ids = embed_ids(rng, B, S, vocab)
    g, b = rng.standard_normal(H).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    got = _native.diag_embed(rt, ids, wemb, pemb if with_pos else None, temb, max_pos, ln=(g, b, EPS))
    x = fr.embed_sum(ids, wemb, pemb if with_pos else None, temb, max_pos, dtype=np.float32)
    ref = fr.layernorm(x, g, b, EPS)
    check_one_bf16_rounding(got, ref, ln_f32_term(x, g.astype(np.float64), ref, 38), f"embed_ln H={H}")


# -------------------------------------------------------------------------------------------------------------- LayerNorm
LN_CASES = [(H, t) for H in (128, 384, 768, 1024, 2048) for t in (1, 2, 7, 8, 9, 4095)] + [(128, 16385), (768, 16385), (2048, 16385), (128, 70001), (768, 70001)]


@pytest.mark.parametrize("H,tokens", LN_CASES)
def test_layernorm_kernel(rt, H, tokens):
    """layernorm_kernel<3> (H <= 768), <4> (1024), <8> (2048) with the `k0 < H` guards of H = 128 / 384; token counts around the 8 rows
    of a workgroup sweep, odd ones (the second half-wave idles), and beyond one grid sweep of 2048 workgroups x 8 rows (16385, 70001:
    the grid-stride loop and its next-row prefetch).  Rows: zero-mean, means up to 8 sigma and 100 sigma -- this kernel subtracts
    the mean first -- and all-zero rows.  Half a wave per row: 8 values per chunk in a 3-level tree, <= 8 chunks, 5 shuffle levels:
    depth 16.  Bar: check_one_bf16_rounding with ln_f32_term.
    Observed on an MI355X (2026-10-17): largest err / bar 1.000 to three decimals, never above 1 (errors reach half an ulp, as those of a
    correctly rounded result do)."""
    rng = np.random.default_rng(H * 7 + tokens)
    x = rng.standard_normal((tokens, H))
    r = np.arange(tokens)
    x[r % 5 == 1] += rng.uniform(-8, 8, ((r % 5 == 1).sum(), 1))
    x[r % 5 == 2] += rng.uniform(-100, 100, ((r % 5 == 2).sum(), 1))
    x[r % 11 == 3] = 0.0
    x = bf16_round(x.astype(np.float32))
    g, b = rng.standard_normal(H).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    got = _native.diag_layernorm(rt, x, g, b, EPS)
    ref = fr.layernorm(x, g, b, EPS)
    zero = ~x.any(1)
    assert np.array_equal(bits(got[zero]), bits(np.broadcast_to(bf16_round(b), x.shape)[zero]))
    check_one_bf16_rounding(got, ref, ln_f32_term(x, g.astype(np.float64), ref, 16), f"layernorm H={H} tokens={tokens}")


# ---------------------------------------------------------------------------------------------------------------- pooling
def pool_lens(S):
    return np.array([1, 2, 7, 8, 9, S - 1, S, 0, S + 5], np.int32)  # 0 and S + 5 clamp to 1 and S


@pytest.mark.parametrize("S", [32, 512, 2048])
@pytest.mark.parametrize("H", [128, 768, 1024])
def test_mean_pool_kernels(rt, S, H):
    """mean_pool_sliced_kernel (normalize off) and mean_pool_kernel (on) on f32 outputs.  The sliced kernel adds the rows rg, rg + 8, ..
    sequentially and the 8 row groups after that, the other one all len rows sequentially: depth <= len + 8, then one multiply, so
        |pooled - ref| <= (len + 9) u mean_t |x_t|.
    Normalised: out = p / |p|; the sum of squares is 4 products per step, <= 2 steps, an 8-level tree: 16 u relative, half of it in the
    norm, plus the pooled errors d: |d_i| / |p| + |out_i| (|d| / |p| + 12 u).  The test asserts the bound itself stays below 2e-4,
    100 x under the 2e-2 end-to-end bar.
    Observed on an MI355X (2026-10-17): sliced at most 0.107 of the bound, normalised 0.089; largest bound 1.48e-4."""
    rng = np.random.default_rng(S + H)
    lens = pool_lens(S)
    B = lens.size
    x = bf16_round((rng.standard_normal((B * S, H)) + rng.uniform(-1, 1, (1, H))).astype(np.float32))
    ln = np.clip(lens, 1, S)
    absmean = np.stack([np.abs(x[b * S: b * S + ln[b]]).astype(np.float64).mean(0) for b in range(B)])
    d = (ln[:, None] + 9) * U * absmean
    got = _native.diag_mean_pool(rt, x, lens, S, normalize=False)
    ref = fr.mean_pool(x, lens, S)
    err = np.abs(got - ref)
    print(f"mean_pool_sliced S={S} H={H}: err/bound {float((err / d).max()):.3f}, largest bound {d.max():.2e}")
    assert d.max() <= 2e-4 and np.all(err <= d)
    gotn = _native.diag_mean_pool(rt, x, lens, S, normalize=True)
    refn = fr.mean_pool(x, lens, S, normalize=True)
    nrm = np.linalg.norm(ref, axis=1, keepdims=True)
    dn = d / nrm + np.abs(refn) * (np.linalg.norm(d, axis=1, keepdims=True) / nrm + 12 * U)
    errn = np.abs(gotn - refn)
    print(f"mean_pool normalised S={S} H={H}: err/bound {float((errn / dn).max()):.3f}, largest bound {dn.max():.2e}")
    assert dn.max() <= 2e-4 and np.all(errn <= dn)


@pytest.mark.parametrize("S", [32, 512, 2048])
@pytest.mark.parametrize("H", [256, 768, 1024])
def test_mean_pool_ln_kernel(rt, S, H):
    """mean_pool_ln_kernel: gamma (sum_t rs_t y_t - sum_t rs_t mu_t) / len + beta from raw rows and caller-supplied statistics in 1, 3
    and 4 slots (tokens_pad > B S: the slot stride is tokens_pad).  Per token (mu, rs) carry fin_bounds' errors (sequential slot sums,
    one-pass variance; sqrtf and the division are correctly rounded, inside the 4 u); the two sums run over rows rg, rg + 8, ... then
    over the 8 row groups (depth len / 8 + 8) on terms rs |y| and rs |mu|, then (t - m) / len gamma + beta round 4 times:
        |out - ref| <= |gamma| / len sum_t [ (len / 8 + 10) u rs_t (|y_t| + |mu_t|) + |d rs_t| |y_t - mu_t| + rs_t |d mu_t| ] + 4 u |ref|.
    Means up to 2 sigma, gamma = 1 + 0.3 N(0,1): the bound stays below 2e-4 (asserted), 100 x under the end-to-end bar.
    Observed on an MI355X (2026-10-17): at most 0.18 of the bound; largest bound 7.7e-5."""
    rng = np.random.default_rng(S * 3 + H)
    lens = pool_lens(S)
    B = lens.size
    tp = B * S + 57
    y = bf16_round((rng.standard_normal((tp, H)) + rng.uniform(-2, 2, (tp, 1))).astype(np.float32))
    st = f32_stats(y)
    g, b = (1 + 0.3 * rng.standard_normal(H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    got = _native.diag_mean_pool_ln(rt, y, st, g, b, EPS, lens, S)
    ref = fr.mean_pool_ln(y[: B * S], g, b, EPS, lens, S)
    mu, rs, dmu, rs_lo, rs_hi = fin_bounds(st, H, EPS)
    drs = np.maximum(rs_hi - rs, rs - rs_lo)
    y64 = y.astype(np.float64)
    ln = np.clip(lens, 1, S)
    bound = np.empty_like(ref)
    for i in range(B):
        t = slice(i * S, i * S + ln[i])
        per = ((ln[i] / 8 + 10) * U * rs[t, None] * (np.abs(y64[t]) + np.abs(mu[t, None])) + drs[t, None] * np.abs(y64[t] - mu[t, None])
               + (rs[t] * dmu[t])[:, None])
        bound[i] = np.abs(g) / ln[i] * per.sum(0) + 4 * U * np.abs(ref[i])
    err = np.abs(got - ref)
    print(f"mean_pool_ln S={S} H={H}: err/bound {float((err / bound).max()):.3f}, largest bound {bound.max():.2e}")
    assert bound.max() <= 2e-4 and np.all(err <= bound)


# ------------------------------------------------------------------------------------------------------------------ GEGLU
def test_geglu_kernel(rt):
    """glu_kernel<ActGelu>: the form and bar of test_nomic_gpu.py::test_swiglu_kernel with erf-GELU as the activation -- gates over
    [-16, 16] and N(0, 2), |err| <= scale 2^-8; saturated tails finite (gelu(-inf side) = 0, gelu(g) = g for large g).
    Observed on an MI355X (2026-10-17): max err 0.125 at scale 44.4 (bar 0.173)."""
    rows, F = 64, 512
    rng = np.random.default_rng(13)
    n = rows * F
    g = np.concatenate([np.linspace(-16.0, 16.0, n // 2), rng.standard_normal(n - n // 2) * 2.0]).astype(np.float32).reshape(rows, F)
    u = rng.standard_normal((rows, F)).astype(np.float32)
    h = bf16_round(np.concatenate([g, u], axis=1))
    got = _native.diag_geglu(rt, h).astype(np.float64)
    ref = fr.geglu(h)
    err = np.abs(got - ref)
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"geglu: max err {err.max():.3e} (scale {scale:.2f})")
    assert np.isfinite(got).all()
    assert err.max() <= scale * 2.0 ** -8, (err.max(), scale)
    gt = np.array([-3.0e38, -1.0e4, -200.0, -100.0, -89.0, -88.0, -30.0, 30.0, 100.0, 1.0e4, 0.0] + [0.0] * 5, np.float32)
    ht = bf16_round(np.concatenate([np.tile(gt, (2, 1)), np.stack([np.full(16, 1.5, np.float32), np.full(16, -2.0, np.float32)])], axis=1))
    out = _native.diag_geglu(rt, ht)
    assert not np.isnan(out).any(), out
    assert np.all(np.abs(out[:, :7]) < 1e-8), out[:, :7]
    assert np.allclose(out[:, 7:10], bf16_round(ht[:, 7:10] * ht[:, 16 + 7:16 + 10]), rtol=2.0 ** -7)


# -------------------------------------------------------------------------------------------------------------- attention
def attention_case(S, heads):
    B = 3 if S <= 512 else 4
    H = heads * 64
    rng = np.random.default_rng(S)
    qkv = rng.standard_normal((B * S, 3 * H)).astype(np.float32)
    qkv[:, :H] *= 2.0  # sharper softmax
    lens = np.array([S, max(1, S // 2 + 3), 1] + ([S - 517] if S > 512 else []), np.int32)
    return B, qkv, lens


def check_attention(got, ref, lens, B, S, tag):
    """test_attention_kernel's bar: max 3e-2, median 3e-3 (P and O are rounded to bf16)."""
    err = np.abs(got - ref)
    print(f"{tag}: max err {err.max():.3e}, median {np.median(err):.3e}")
    assert np.isfinite(got).all(), tag
    assert err.max() <= 3e-2, (tag, err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 3e-3, tag


@pytest.mark.parametrize("S", [32, 64, 128, 256, 512, 1024, 2048])
def test_attention_blocked_layout(rt, S):
    """test_attention_kernel's cases through the layout both pipelines use -- sc_launch_attention(..., blocked = M) on the
    [3 heads][M][64] buffer of the QKV epilogue, M = the token count padded to the GEMM's 256 rows (and once more, so that M differs
    from B S even where B S is a multiple of 256): same arithmetic at other addresses, so bit-identical to the row-major launch, which
    in turn meets the float64 bar.
    Observed on an MI355X (2026-10-17): bit-identical everywhere; max err 7.7e-3, median at most 2.0e-4."""
    heads = 2
    B, qkv, lens = attention_case(S, heads)
    row = _native.diag_attention_ex(rt, qkv, lens, B, S, heads)
    assert np.array_equal(bits(row), bits(_native.diag_attention(rt, qkv, lens, B, S, heads)))
    M = (B * S + 255) // 256 * 256 + 256
    blk = _native.diag_attention_ex(rt, qkv, lens, B, S, heads, blocked_rows=M)
    assert np.array_equal(bits(blk), bits(row)), int((bits(blk) != bits(row)).sum())
    check_attention(blk, fr.attention(bf16_round(qkv), lens, B, S, heads), lens, B, S, f"attention blocked S={S}")


@pytest.mark.parametrize("S", [32, 256, 512, 1024, 2048])
@pytest.mark.parametrize("heads", [2, 12])
def test_attention_alibi(rt, S, heads):
    """The ALiBi bias -slope_h |i - j| with oracle.bert_oracle.alibi_slopes (12 heads: the non-power-of-two ladder), blocked layout,
    the same ragged lens; S = 1024 / 2048 carry the bias across the 512-key segments of attention_long_kernel.  Same bar.
    Observed on an MI355X (2026-10-17): max err 1.11e-2 (12 heads, S = 1024), median at most 2.1e-4."""
    B, qkv, lens = attention_case(S, heads)
    slopes = bo.alibi_slopes(heads)
    M = (B * S + 255) // 256 * 256
    got = _native.diag_attention_ex(rt, qkv, lens, B, S, heads, blocked_rows=M, slopes=slopes)
    ref = fr.attention(bf16_round(qkv), lens, B, S, heads, slopes)
    if S <= 512:  # the bias matters on this data: leaving it out cannot pass
        assert np.abs(ref - fr.attention(bf16_round(qkv), lens, B, S, heads)).max() > 0.1
    check_attention(got, ref, lens, B, S, f"attention alibi S={S} heads={heads}")
    assert np.array_equal(bits(got), bits(_native.diag_attention_ex(rt, qkv, lens, B, S, heads, slopes=slopes)))  # row-major twin
