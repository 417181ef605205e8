"""GPU: single-kernel parity of the plain encoder GEMMs (sc_launch_gemm_bf16) in every layout, tile and split-K form the forward passes
launch: gemm_bf16_kernel (128-tile), gemm256_bf16_kernel<EPI_BIAS | EPI_BIAS_GELU | EPI_BIAS_RES> (256-tile; both main loops, both
residual hooks, every walk order), gemm256_splitk_kernel + gemm_splitk_reduce_kernel, and the int8 tile loop (gemm256_i8_diag_kernel).

Every launch goes ONCE through the product's launcher (sc_diag_gemm_bf16_ex) and reports the kernel it ran -- tile, K slices, walk order,
ring depth, non-temporal stores -- which every test asserts: no case passes by running another kernel than the one it names.  The output
buffer starts as NaN, so an element no workgroup writes fails the finiteness check.

Reference: float64 on the bf16-rounded operands, lin = A W^T + bias, then erf-GELU(lin) or lin + bf16(R).

Bar, per element (u = 2^-24, T = |A| |W|^T, the idiom of test_fold_kernels_gpu.py):
  * one bf16 rounding of the result: half an ulp of |ref|;
  * the f32 accumulation: 2 K u T (K additions of f32 terms are off by at most K u sum |t_i|; the factor 2 allows for an accumulator
    that truncates instead of rounding, as lna_extra_bound does);
  * the epilogue's adds, each rounding once on a number no larger than the sum of its parts: u (|bias| + |R| + |ref|);
  * split-K: the reduce kernel adds the d slices one after the other in f32, d more roundings on partial sums bounded by T: + d u T.
  * GELU: the bars of test_gelu_epilogue_accuracy (rounding + the approximation of gelu_erf_fast2: 0.515 ulp where |gelu| > 1e-3, 0.64 ulp
    down to 1e-5, 1e-6 absolute below) and the f32 term of lin = A W^T + bias passed through |gelu'| <= 1.13.

Operands are asymmetric so that a transposed, permuted or misplaced tile cannot pass: A ~ N(0,1) and R ~ N(0,1) with row ramps of
different slope (x 1..3 and x 0.5..3.5), W ~ N(0,1) / sqrt K, bias ~ N(0,1).

Bit identity.  A blocked layout changes addresses only, the walk order which workgroup computes a tile, nt the store's cache policy, and
both main loops feed every accumulator its K-steps in ascending order: all of these must repeat the dense result bit for bit.  So must
the 128-tile kernel against the 256-tile kernel: gemm_tile_mainloop and gemm_tile256_mainloop(_pp) both issue one
v_mfma_f32_16x16x32_bf16 per accumulator and 32-deep K-step, K-step after K-step, and the epilogues apply the same f32 operations in the
same order ((acc + bias), then GELU by gelu_erf_fast2 or + R).  Split-K sums K in another order and is held to the bar only.

Found while writing these tests: the 128-tile kernel computed its GELU as 0.5 x (1 + erff(x / sqrt 2)); in f32 the sum 1 + erf cancels
for x < -3.4 (|gelu| < 1e-3) and its rounding alone reaches 1.1 bf16 ulp at |gelu| ~ 1e-5 .. 1e-4 -- outside the bars the 256-tile kernel
meets in test_gelu_epilogue_accuracy, though far inside the bar above, whose f32 term is absolute (both forms give the same err / bar
on the random shapes).  test_gelu_epilogue_accuracy_of_the_128_tile_kernel, with an exact accumulator, shows it; the kernel now uses
gelu_erf_fast2 like the other two, which is also what makes the GELU results of the two tile sizes bit-identical.

Observed on an MI355X (2026-10-21), largest err / bar per family (epi 0 / 1 / 2) -- close to 1 by construction, since the rounding of
some element among 10^5 comes within a percent of half an ulp and the f32 term is small against it at small K:
128-tile 0.986 / 0.954 / 0.992, 256-tile layouts 0.995 / 0.965 / 0.996, split-K 0.913 / 0.855 / 0.924, switches 0.988 / 0.960 / 0.992,
walk orders 0.997 / 0.969 / 0.997, 128-tile forced 0.995 / 0.965 / 0.996 (equal to the 256-tile figures: same bits); at K = 4864 the f32
term dominates and the kernel uses 0.39 / 0.34 / 0.45 of the bar.  Every blocked, nt, main-loop, order and tile-size variant bit-identical.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import fold_ref as fr
from fold_ref import U, bf16_round, bf16_ulp
from semcode_amd import _native

pytestmark = pytest.mark.gpu

EPIS = [0, 1, 2]
TILE128 = dict(tile=128, splitk=1, order=0, pp=0, nt=0)


def tile256(K, order=0, pp=-1, nt=0):
    """The path of a per-tile 256-tile launch: the ring needs two K-tiles."""
    return dict(tile=256, splitk=1, order=order, pp=4 if pp != 0 and K >= 128 else 0, nt=nt)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def gemm_options():
    """Hands out a setter of the process-wide GEMM switches and puts the defaults back afterwards."""
    def set_(nt=-1, pp=-1, order=-1):
        _native.diag_set_option("gemm_nt", nt)
        _native.diag_set_option("gemm_pp", pp)
        _native.diag_set_option("gemm_order", order)
    set_()
    yield set_
    set_()


@functools.lru_cache(maxsize=None)
def case(M, N, K):
    """Operands (bf16-representable f32), float64 references per epilogue and T = |A| |W|^T of one shape: computed once, read-only."""
    rng = np.random.default_rng([M, N, K])
    ramp = np.arange(M) / M
    A = bf16_round((rng.standard_normal((M, K)) * (1.0 + 2.0 * ramp)[:, None]).astype(np.float32))
    W = bf16_round((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32))
    bias = rng.standard_normal(N).astype(np.float32)
    R = bf16_round((rng.standard_normal((M, N)) * (0.5 + 3.0 * ramp)[:, None]).astype(np.float32))
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    lin = A64 @ W64.T + bias.astype(np.float64)
    T = np.abs(A64) @ np.abs(W64).T
    c = SimpleNamespace(M=M, N=N, K=K, A=A, W=W, bias=bias, R=R, lin=lin, T=T, ref=(lin, fr.gelu(lin), lin + R.astype(np.float64)))
    for a in (A, W, bias, R, lin, T) + c.ref:
        a.setflags(write=False)
    return c


def bar(c, epi, splitk=1):
    """The per-element bar of the module docstring."""
    ref, absb = c.ref[epi], np.abs(c.bias).astype(np.float64)[None, :]
    f32 = 2 * c.K * U * c.T + U * (absb + np.abs(c.lin))
    if epi == 2:
        f32 = 2 * c.K * U * c.T + U * (absb + np.abs(c.R) + np.abs(ref))
    if splitk > 1:
        f32 = f32 + splitk * U * c.T
    if epi != 1:
        return 0.5 * bf16_ulp(ref) + f32
    a, ulp = np.abs(ref), bf16_ulp(ref)
    return np.where(a > 1e-3, 0.515 * ulp, np.where(a > 1e-5, 0.64 * ulp, 1e-6)) + 1.13 * f32


def run(rt, c, epi, **form):
    return _native.diag_gemm_bf16_ex(rt, c.A, c.W, c.bias, c.R if epi == 2 else None, epi=epi, **form)


def check(got, c, epi, tag, splitk=1):
    assert np.isfinite(got).all(), (tag, "elements never written / not finite", np.argwhere(~np.isfinite(got))[:4])
    q = np.abs(got - c.ref[epi]) / bar(c, epi, splitk)
    print(f"{tag} epi {epi}: max err/bar {q.max():.3f}")
    assert q.max() <= 1.0, (tag, epi, float(q.max()), np.unravel_index(q.argmax(), q.shape))


def same(got, base, tag):
    assert np.array_equal(bits(got), bits(base)), (tag, int((bits(got) != bits(base)).sum()), np.argwhere(bits(got) != bits(base))[:4])


# ------------------------------------------------------------------------------------------------------- layouts x kernels
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(256, 1152, 384), (256, 1152, 896), (256, 896, 4864), (128, 384, 128)])
def test_128_tile_dense_and_blocked_c(rt, gemm_options, M, N, K, epi):
    """gemm_bf16_kernel: the QKV widths that are no multiple of 256 (MiniLM 1152 x 384, Qwen2-0.5B 1152 x 896), a deep K and one tile
    row; C row-major and in 64-column blocks (c_index), the layout attention reads."""
    c = case(M, N, K)
    got, path = run(rt, c, epi)
    assert path == TILE128, path
    check(got, c, epi, f"128-tile {M}x{N}x{K}")
    blocked, path = run(rt, c, epi, c_blocked=True)
    assert path == TILE128, path
    same(blocked, got, "C in blocks")


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(256, 768, 768), (512, 768, 3072), (256, 1024, 2048), (256, 256, 64), (256, 256, 128), (512, 512, 192)])
def test_256_tile_dense_and_blocked(rt, gemm_options, M, N, K, epi):
    """gemm256_bf16_kernel with the plain epilogues: dense, C in blocks (QKV of forward_locked, FFN1 with ffn_blocked), A in blocks (FFN2
    with ffn_blocked: a_kstep = M * 64, with EPI_BIAS_RES and the cooperative residual hook) and both."""
    c = case(M, N, K)
    got, path = run(rt, c, epi)
    assert path == tile256(K), path
    check(got, c, epi, f"256-tile {M}x{N}x{K}")
    for form in (dict(c_blocked=True), dict(a_blocked=True), dict(a_blocked=True, c_blocked=True)):
        g2, path = run(rt, c, epi, **form)
        assert path == tile256(K), (form, path)
        same(g2, got, form)


# ---------------------------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (256, 768, 3072), (256, 1024, 2048), (256, 256, 64)])
def test_splitk(rt, gemm_options, M, N, K, epi):
    """gemm256_splitk_kernel + gemm_splitk_reduce_kernel (a single query's projections; the reduce kernel writes through c_index).  The
    factor is the rule's for this device's CU count and is read back from the launch; (256, 256, 64) -- one K-tile -- must be left on the
    per-tile kernel."""
    c = case(M, N, K)
    want = _native.diag_gemm_splitk(M, N, K)
    if K == 64:
        assert want == 1
        got, path = run(rt, c, epi, splitk=True)
        assert path == tile256(K), path
        base, _ = run(rt, c, epi)
        same(got, base, "scratch offered, not used")
        return
    if want <= 1:
        pytest.skip(f"the split-K rule leaves {M}x{N}x{K} alone on this device ({_native.diag_gemm_path(M, N, K)}): too few CUs")
    got, path = run(rt, c, epi, splitk=True)
    assert path == dict(tile=256, splitk=want, order=1, pp=0, nt=0), (path, want)
    check(got, c, epi, f"split-K x{want} {M}x{N}x{K}", splitk=want)
    blocked, path = run(rt, c, epi, splitk=True, c_blocked=True)
    assert path["splitk"] == want and path["tile"] == 256, path
    same(blocked, got, "C in blocks")


# ------------------------------------------------------------------------------------------- switches of the 256-tile kernel
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 512, 192), (256, 768, 448)])
def test_256_tile_switches(rt, gemm_options, M, N, K, epi):
    """gemm_nt 0 / 1 x gemm_pp 0 / -1: the store's cache policy and the main loop (one barrier per K-tile with ResidualTailHook, the
    ping-pong ring with ResidualCoopHook) change no bit.  K = 128 is the ring with exactly two K-tiles, 192 and 448 are odd counts."""
    c = case(M, N, K)
    base = None
    for nt, pp in ((0, -1), (1, -1), (0, 0), (1, 0)):
        gemm_options(nt=nt, pp=pp)
        got, path = run(rt, c, epi)
        assert path == tile256(K, pp=pp, nt=nt), (nt, pp, path)
        if base is None:
            base = got
            check(got, c, epi, f"switches {M}x{N}x{K}")
        same(got, base, (nt, pp))
    got, path = run(rt, c, epi, a_blocked=True, c_blocked=True)  # still nt 1, pp 0
    assert path == tile256(K, pp=0, nt=1), path
    same(got, base, "nt 1, pp 0, A and C in blocks")


# ------------------------------------------------------------------------------------------------------------ walk orders
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(2816, 512, 128), (1280, 768, 64)])
def test_walk_orders(rt, gemm_options, M, N, K, epi):
    """tile_coords256: order 0 (row panel by row panel, XCD remap), 1 (no remap), 16 (column-major inside groups of 8 row panels, remap)
    and 17 (the same without).  2816 rows are 11 panels -- a full group of 8 and a short one of 3, 22 tiles, no multiple of 8 -- and
    1280 rows a single short group of 5.  Every order must write every tile once, with the bits of order 0."""
    c = case(M, N, K)
    base = None
    for order in (0, 1, 16, 17):
        gemm_options(order=order)
        got, path = run(rt, c, epi)
        assert path == tile256(K, order=order), (order, path)
        if base is None:
            base = got
            check(got, c, epi, f"orders {M}x{N}x{K}")
        assert np.isfinite(got).all(), (order, "tiles never written", np.argwhere(~np.isfinite(got))[:4])
        same(got, base, f"order {order}")
    got, path = run(rt, c, epi, c_blocked=True)  # order 17
    assert path == tile256(K, order=17), path
    same(got, base, "order 17, C in blocks")


# ------------------------------------------------------------------------------------------------- 128-tile against 256-tile
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,N,K", [(256, 768, 768), (512, 512, 192), (256, 256, 64)])
def test_128_tile_against_256_tile(rt, gemm_options, M, N, K, epi):
    """The same shape on both kernels (sc_gemm_force_tile128 through the harness): both within the bar and, since both main loops feed
    an accumulator its K-steps in the same order and the epilogues compute alike (module docstring), bit for bit the same."""
    c = case(M, N, K)
    big, path = run(rt, c, epi)
    assert path == tile256(K), path
    small, path = run(rt, c, epi, tile128=True)
    assert path == TILE128, path
    check(big, c, epi, f"256-tile {M}x{N}x{K}")
    check(small, c, epi, f"128-tile forced {M}x{N}x{K}")
    same(small, big, "128-tile against 256-tile")
    after, path = run(rt, c, epi)  # the force does not outlive its call
    assert path == tile256(K), path


def test_gelu_epilogue_accuracy_of_the_128_tile_kernel(rt, gemm_options):
    """test_encoder_gpu.py::test_gelu_epilogue_accuracy on the 128-tile kernel: W = identity and bias 0 pass the bf16 inputs through the
    accumulator exactly (T's term of the bar is zero), so out = bf16(gelu(x)) for x over [-16, 16] with both tails, within that test's
    bars -- 0.515 ulp where |gelu| > 1e-3, 0.64 ulp down to 1e-5, 1e-6 below -- and with the bits of the 256-tile kernel.
    The kernel's earlier form 0.5 x (1 + erff(x / sqrt 2)) cancels for x < -3.4: evaluated in f32 on the host with a correctly rounded
    erff it is off by up to 1.1 ulp at |gelu| ~ 1e-5 .. 1e-4 before the output rounding adds its half."""
    M = N = K = 256
    rng = np.random.default_rng(11)
    x = np.concatenate([np.linspace(-16.0, 16.0, M * K // 2), rng.standard_normal(M * K // 2) * 2.0]).astype(np.float32)
    A, W, zero = bf16_round(x.reshape(M, K)), np.eye(N, K, dtype=np.float32), np.zeros(N, np.float32)
    got, path = _native.diag_gemm_bf16_ex(rt, A, W, zero, epi=1, tile128=True)
    assert path == TILE128, path
    big, path = _native.diag_gemm_bf16_ex(rt, A, W, zero, epi=1)
    assert path == tile256(K), path
    ref = fr.gelu(A.astype(np.float64))
    q = np.abs(got - ref) / bf16_ulp(ref)
    a = np.abs(ref)
    print(f"128-tile GELU: err in ulp {q[a > 1e-3].max():.3f} (|gelu| > 1e-3), {q[a > 1e-5].max():.3f} (> 1e-5), abs {np.abs(got - ref)[a <= 1e-5].max():.2e} below")
    assert q[a > 1e-3].max() <= 0.515 and q[a > 1e-5].max() <= 0.64 and np.abs(got - ref)[a <= 1e-5].max() <= 1e-6
    assert np.all(got[A > 12] == A[A > 12]) and np.all(np.abs(got[A < -12]) < 1e-30)  # saturated tails, no NaN
    same(got, big, "128-tile against 256-tile")


# ------------------------------------------------------------------------------------------------------------------- int8
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 768, 768), (256, 256, 1024)])
def test_int8_tile_loop_is_exact(rt, M, N, K):
    """The int8 tile loop of the batched scan (sc_diag_gemm_i8): exact integers.  Operands over the whole range -127 .. 127; rows of all
    +127 against rows of all -127 and +127 reach the extreme accumulator values -+ 127^2 K."""
    rng = np.random.default_rng([M, N, K, 8])
    A = rng.integers(-127, 128, (M, K)).astype(np.int8)
    W = rng.integers(-127, 128, (N, K)).astype(np.int8)
    A[0], A[1], A[M - 1] = 127, -127, 127
    W[0], W[1], W[N - 1] = -127, 127, -127
    A[2, ::2], A[2, 1::2] = 127, -127  # alternating signs against a constant row: cancels to 0 through extreme partial sums
    want = A.astype(np.int64) @ W.astype(np.int64).T
    assert want.min() == -127 * 127 * K and want.max() == 127 * 127 * K and {-127, 127} <= set(np.unique(A)) & set(np.unique(W))
    got = _native.diag_gemm_i8(rt, A, W)
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want), np.argwhere(got != want)[:4]


# ------------------------------------------------------------------------------------------------------------ the harness
def test_bench_leaves_the_walk_order_by_shape(rt, gemm_options):
    """sc_diag_gemm_bench forces an order while it times; afterwards the launcher decides by shape again: order 0 for a small N K."""
    c = case(256, 256, 64)
    _native.diag_gemm_bench(rt, 256, 256, 64, iters=1)
    got, path = run(rt, c, 0)
    assert path == tile256(64, order=0), path
    assert _native.diag_gemm_path() == path
    assert _native.diag_gemm_path(256, 6144, 1024)["order"] == 16 and _native.diag_gemm_path(256, 768, 768)["order"] == 0
    check(got, c, 0, "after the bench")


def test_refused_forms_launch_nothing(rt, gemm_options):
    """Blocked A outside the per-tile 256-tile kernel is refused by the harness (the launcher's contract), and the next call runs."""
    c = case(256, 256, 128)
    for form in (dict(a_blocked=True, splitk=True), dict(a_blocked=True, tile128=True)):
        with pytest.raises(_native.ScError, match="blocked A"):
            run(rt, c, 0, **form)
    c128 = case(128, 384, 128)
    with pytest.raises(_native.ScError, match="blocked A"):
        run(rt, c128, 0, a_blocked=True)
    got, path = run(rt, c, 2, a_blocked=True)
    assert path == tile256(128), path
    check(got, c, 2, "after the refusals")
