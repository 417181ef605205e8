"""GPU: the strip walk of the EPI_LNA_* GEMMs (gemm256_strip_kernel) against the per-tile kernel, bit for bit.

A strip kernel workgroup takes L consecutive column tiles of one row panel, finalises the row statistics once, and prefetches the
next tile's first two K-tiles under the last phases of the current one; none of that may change a bit of C or of the published
(mu, rs).  Both kernels run through the product's launcher (sc_diag_gemm_lna) with "gemm_strip" forced: 0 = per-tile, L = tiles per
strip.  The per-tile kernel itself is held against the float64 reference in tests/test_fold_kernels_gpu.py::test_lna_gemm.

Shapes: K = 256 is four K-tiles, the shortest loop (the prefetched K-tile 0 and the last two K-tiles of the loop sit next to each
other); N = 768 with L = 2 gives a full strip and a short one, N = 1024 with L = 4 first, middle and last tiles in one strip, L = 1
the strip kernel without any prefetch; M = 768 puts several panels on one launch.  Rows: the five populations of fold_ref.make_rows
(all-zero rows among them).
"""
import numpy as np
import pytest

import fold_ref as fr
from semcode_amd import _native

pytestmark = pytest.mark.gpu

EPS = 1e-12
EPIS = ((3, "bias"), (4, "gelu"), (6, "rope"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture
def strip_options():
    def set_(strip=-1, nt=-1):
        _native.diag_set_option("gemm_strip_n", 0)
        _native.diag_set_option("gemm_strip", strip)
        _native.diag_set_option("gemm_nt", nt)
    yield set_
    set_()


def inputs(rt, M, N, K):
    rng = np.random.default_rng(7 * M + 3 * N + K)
    A, kind = fr.make_rows(rng, M, K)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    g, be = rng.standard_normal(K).astype(np.float32), rng.standard_normal(K).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    Wf, c1, c2 = _native.diag_fold_ln(rt, W, g, be, b)
    return A, kind, Wf, c1, c2, fr.slot_stats(A).astype(np.float32)


def rope_kw(epi, N):
    return dict(rope_S=32, rope_theta=10000.0, rope_ncols=(2 * N // 3) // 64 * 64) if epi == 6 else {}


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("N", [768, 1024])
@pytest.mark.parametrize("M", [256, 768])
def test_strip_kernel_repeats_the_per_tile_kernel(rt, strip_options, M, N, K):
    """C and fin of gemm_strip = L, L in {1, 2, 3, 4}, equal those of gemm_strip = 0 bit for bit: three epilogues x blocked / row-major
    C x plain / non-temporal stores."""
    A, kind, Wf, c1, c2, st = inputs(rt, M, N, K)
    assert (kind == fr.ZERO).any() and (kind == fr.TINY_VAR).any() and (kind == fr.UNEVEN).any()
    for epi, name in EPIS:
        for blocked in (False, True):
            for nt in (0, 1):
                strip_options(strip=0, nt=nt)
                want, fin = _native.diag_gemm_lna(rt, epi, A, Wf, c1, c2, st, EPS, blocked=blocked, **rope_kw(epi, N))
                assert _native.diag_gemm_strip() == 0, "the reference launch must be the per-tile kernel"
                assert np.isfinite(want).all() and np.isfinite(fin).all()
                for L in (1, 2, 3, 4):
                    strip_options(strip=L, nt=nt)
                    got, f2 = _native.diag_gemm_lna(rt, epi, A, Wf, c1, c2, st, EPS, blocked=blocked, **rope_kw(epi, N))
                    tag = (name, M, N, K, "blocked" if blocked else "row-major", f"nt={nt}", f"L={L}")
                    assert _native.diag_gemm_strip() == min(L, N // 256), (tag, "the launch did not run as strips of L tiles")
                    diff = bits(got) != bits(want)
                    assert not diff.any(), (tag, int(diff.sum()), "first at", tuple(int(v) for v in np.argwhere(diff)[0]))
                    assert np.array_equal(bits(f2), bits(fin)), (tag, "fin differs")


def test_strip_launch_is_reproducible(rt, strip_options):
    """The same strip launch twice: same bits (a prefetch read too early would show as rare wrong tiles that come and go)."""
    M, N, K = 768, 1024, 256
    A, _, Wf, c1, c2, st = inputs(rt, M, N, K)
    for epi, _name in EPIS:
        for L in (2, 4):
            strip_options(strip=L, nt=1)
            a1, f1 = _native.diag_gemm_lna(rt, epi, A, Wf, c1, c2, st, EPS, blocked=True, **rope_kw(epi, N))
            a2, f2 = _native.diag_gemm_lna(rt, epi, A, Wf, c1, c2, st, EPS, blocked=True, **rope_kw(epi, N))
            assert _native.diag_gemm_strip() == L
            assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(f1), bits(f2)), (epi, L)


def test_strip_option_is_clamped_and_filtered(rt, strip_options):
    """A strip longer than a row panel's tiles is clamped to them (one strip per panel); with "gemm_strip_n" set, a launch with
    another N runs one workgroup per tile."""
    M, N, K = 256, 768, 256
    A, _, Wf, c1, c2, st = inputs(rt, M, N, K)
    strip_options(strip=0, nt=0)
    want, fin = _native.diag_gemm_lna(rt, 3, A, Wf, c1, c2, st, EPS)
    assert _native.diag_gemm_strip() == 0
    strip_options(strip=64, nt=0)
    got, f2 = _native.diag_gemm_lna(rt, 3, A, Wf, c1, c2, st, EPS)
    assert _native.diag_gemm_strip() == 3
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(f2), bits(fin))
    _native.diag_set_option("gemm_strip_n", 1024)
    _native.diag_gemm_lna(rt, 3, A, Wf, c1, c2, st, EPS)
    assert _native.diag_gemm_strip() == 0


def test_default_batch_step_runs_strips_and_repeats_the_per_tile_step(rt, strip_options):
    """The product path with nothing forced: one BERT-base layer on 256 chunks x 256 tokens (M = 65536, the shape the rule was
    measured at).  The shape rule must pick strips there (FFN1, the last EPI_LNA_* launch of a forward: 6 tiles; QKV: 3), and the
    pooled vectors must equal those of the same forward with strips switched off, bit for bit."""
    B, S = 256, 256
    enc = _native.Encoder(rt, dict(_native.BERT_BASE, layers=1), weights=None, synth_seed=3)
    try:
        rng = np.random.default_rng(11)
        ids = rng.integers(1000, 30000, size=(B, S)).astype(np.int32)
        lens = np.full(B, S, np.int32)
        strip_options(strip=0)
        want = enc.embed_ids(ids, lens)
        assert _native.diag_gemm_strip() == 0
        strip_options(strip=-1)
        assert _native.diag_gemm_strip(B * S, 2304, 768) == 3 and _native.diag_gemm_strip(B * S, 3072, 768) == 6
        got = enc.embed_ids(ids, lens)
        assert _native.diag_gemm_strip() == 6, "the default batch step did not take the strip kernel"
        assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want))
    finally:
        enc.close()
