"""CPU preconditions of tests/test_degenerate_values_gpu.py: conditions on the INPUTS of tests/degenerate_data.py, checked against
the oracle alone, so that the GPU comparisons cannot become vacuous -- the ties are there, the oracle obeys the scaling law the
device is held to, and it follows the zero-norm rule (include/semcode_hip.h: under COSINE a row or query with |v|^2 == 0 scores
exactly +0.0) without moving a bit of any other score (the committed golden files still reproduce)."""
import numpy as np
import pytest

import degenerate_data as dd
from oracle import sc_oracle as orc
from oracle.ivf_oracle import IvfOracle

METRICS = ["IP", "L2", "COSINE"]
bits = dd.bits


# depth: the oracle's top-`depth` the ties are counted in (degenerate_data.tie_counts) -- beyond the bound asserted
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name,depth,floor", [("copies1500", 128, 64), ("copies100", 600, 513), ("copies12", 4200, 4097)])
def test_copies_tie_with_the_tenth_score_beyond_each_candidate_set(name, depth, floor, metric):
    X, Q = dd.family(name)
    t = dd.tie_counts(X, Q[:40], metric, depth)
    print(name, metric, "ties with the 10th score inside the top", depth, ": min", t.min(), "max", t.max())
    assert t.min() >= floor, (name, metric, t)


@pytest.mark.parametrize("name,metric", [("ternary", "IP"), ("ternary", "L2"), ("offset", "L2"), ("offset", "COSINE")])
def test_ternary_and_offset_scores_tie_by_the_dozen(name, metric):
    X, Q = dd.family(name)
    t = dd.tie_counts(X, Q[:40], metric, 512)
    print(name, metric, "ties with the 10th score: min", t.min(), "median", np.median(t), "max", t.max())
    assert np.median(t) >= 5, (name, metric, t)  # (a count cut off at the depth is a lower bound: the median can only be larger)


@pytest.fixture(scope="module")
def scaled0():
    X, Q = dd.scaled(0)
    return {m: orc.search(X, Q[:40], 10, m) for m in METRICS}


@pytest.mark.parametrize("s", [s for s in dd.SCALES if s != 0])
def test_oracle_scaling_law(scaled0, s):
    """scaled(s) = scaled(0) * 2^s, exact in f32: the same rows; IP and L2 distances times 2^(2 s) bit for bit, COSINE unchanged."""
    X, Q = dd.scaled(s)
    X0, Q0 = dd.scaled(0)
    assert np.array_equal(X, np.ldexp(X0, s)) and np.array_equal(Q, np.ldexp(Q0, s))
    for metric in METRICS:
        d0, r0 = scaled0[metric]
        d, r = orc.search(X, Q[:40], 10, metric)
        assert np.array_equal(r, r0), (s, metric)
        want = d0 if metric == "COSINE" else np.ldexp(d0, 2 * s)
        assert np.isfinite(want).all() and (want != 0).all()
        assert np.array_equal(bits(d), bits(want)), (s, metric)


def test_zero_norm_rule_on_the_oracle():
    lib = orc.lib()
    pz = np.float32(0.0).view(np.uint32)
    z = np.zeros(64, np.float32)
    assert np.float32(orc.dot(z, -np.ones(64, np.float32))).view(np.uint32) == pz  # the dot of a zero vector is +0.0, whatever the signs
    for xn, qn in ((0.0, 4.0), (4.0, 0.0), (0.0, 0.0)):
        assert np.float32(lib.sc_oracle_score(2, 0.0, xn, qn)).view(np.uint32) == pz  # +0.0: neither NaN nor -0.0
    assert lib.sc_oracle_score(2, 2.0, 4.0, 4.0) == 0.5
    X, Q = dd.family("zero_norm")
    n, k = len(X), 10
    d, r = orc.search(X, Q, k, "COSINE")
    # (a score of +0.0 is REPORTED as -0.0 under IP and COSINE: results are read back from the sort key, which holds -score with
    # -0 folded into +0 -- as for every inner product of exactly 0 before the rule; the device reads its keys back the same way)
    nz = np.float32(-0.0).view(np.uint32)
    for q in dd.ZERO_QUERIES:  # every score +0.0: ties to the lower row
        assert np.array_equal(r[q], np.arange(k)) and (bits(d[q]) == nz).all()
    assert not np.isnan(d).any()
    # a zero row against a non-zero query: exactly +0.0, wherever it sorts
    rows = np.ascontiguousarray(dd.ZERO_ROWS)
    dz, rz = orc.search_rows(X, Q[0], rows, len(rows), "COSINE")
    assert np.array_equal(rz, np.sort(rows)) and (bits(dz) == nz).all()
    # IP: zero rows score 0; L2: they score |q|^2, and a zero query returns the smallest-norm rows (the zero rows first, in row order)
    dz, _ = orc.search_rows(X, Q[0], rows, len(rows), "IP")
    assert (bits(dz) == nz).all()
    dz, _ = orc.search_rows(X, Q[0], rows, len(rows), "L2")
    qn = np.float32(orc.sqnorm(orc.padded(Q[:1])[0]))
    assert (bits(dz) == qn.view(np.uint32)).all()
    d2, r2 = orc.search(X, Q[list(dd.ZERO_QUERIES)], k, "L2")
    assert np.array_equal(r2[0], np.sort(rows)[:k]) and (bits(d2) == pz).all()
    assert n == dd.N


def test_small_corpus_of_zero_rows_pads_nothing():
    X, Q = dd.zero_norm_small()
    d, r = orc.search(X, Q, 10, "COSINE")
    zero = np.flatnonzero(~X.any(axis=1))
    assert len(zero) == 295
    for q in range(len(Q)):
        # ten real rows, no padding: the rows with a positive cosine lead, then zero rows at +0.0 in row order (the rows with a negative
        # cosine sort behind all 295 of them)
        iz = np.isin(r[q], zero)
        npos = int((~iz).sum())
        assert (r[q] >= 0).all() and not iz[:npos].any() and (d[q, :npos] > 0).all()
        assert np.array_equal(r[q, npos:], zero[:10 - npos]) and (bits(d[q, npos:]) == 0x80000000).all()  # (+0.0 read back from the key: -0.0)


def test_golden_files_still_reproduce(golden):
    """The rule changes no score of a non-zero vector: both committed fixtures reproduce bit for bit."""
    knn = np.load(golden / "knn_4096x64.npz")
    g = np.load(golden / "ivf_4096x64.npz")
    for metric in METRICS:
        dist, rows = orc.search(knn["X"], knn["Q"], 10, metric)
        assert np.array_equal(rows, knn[f"{metric}_rows"]) and np.array_equal(bits(dist), bits(knn[f"{metric}_dist"]))
        o = IvfOracle(knn["X"], metric, nlist=16, niter=6)
        assert np.array_equal(bits(o.centroids), bits(g[f"{metric}_centroids"])) and np.array_equal(o.assign, g[f"{metric}_assign"])
        dist, rows = o.search(knn["Q"], 10, 4)
        assert np.array_equal(rows, g[f"{metric}_rows"]) and np.array_equal(bits(dist), bits(g[f"{metric}_dist"]))
