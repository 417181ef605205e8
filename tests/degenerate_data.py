"""Corpora of degenerate VALUES for the search parity tests (tests/test_degenerate_values_host.py, ..._gpu.py).  No test in here.

The shapes of the suite are swept elsewhere; these sweep what the certificate arithmetic of the batched path (certificate_eps,
fast_threshold, the per-row int8 scale, the strict `<` against the threshold) sees: ties by the thousand, zero norms, norms that
differ by orders of magnitude, a large common offset, powers of two far from 1.  Every family is one function -> (X, Q), float32,
fixed seeds; n = 140 000 rows (above the 131 072 from which the persistent int8 kernel keeps per-wave hit lists and the 65 536 /
32 768 limits of the narrow kernel and the bf16 stage), dim = 64, 200 queries unless stated.  The tests slice the queries.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

N, DIM, NQ = 140_000, 64, 200

ZERO_ROWS = np.concatenate([[0, N - 1, 1000], np.arange(4096, 4352), [70_001, 70_002, 70_003]]).astype(np.int64)  # (4096..4351: one whole 256-row tile)
ZERO_QUERIES = (3, 150)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def copies(distinct: int, n: int = N):
    """n rows drawn from `distinct` base vectors: identical rows score identically in every metric, so the k-th score is shared
    by n / distinct rows (1500: below the 128 candidates of the bf16 stage; 100: above the 512 of the int8 stage and below the
    4096-entry survivor cap; 12: above that cap)."""
    rng = np.random.default_rng(1000 + distinct)
    base = _f32(rng.standard_normal((distinct, DIM)))
    X = base[rng.integers(0, distinct, n)]
    Q = _f32(base[rng.integers(0, distinct, NQ)] + 0.1 * rng.standard_normal((NQ, DIM)))
    return _f32(X), Q


def ternary(dim: int = 16, n: int = N):
    """Entries +-1 with probability 1/2, else 0 (index dim 16: rows padded to the stride of 64).  bf16 and int8 hold them exactly
    (residual 0): eps sits at its floor and scores tie by the dozen; a few rows come out all zero."""
    rng = np.random.default_rng(2001)
    X = _f32(rng.choice(np.array([-1.0, 0.0, 0.0, 1.0], np.float32), size=(n, dim)))
    Q = _f32(rng.choice(np.array([-1.0, 0.0, 0.0, 1.0], np.float32), size=(NQ, dim)))
    Q[~Q.any(axis=1), 0] = 1.0
    return X, Q


def offset(scale: float = 1000.0, n: int = N):
    """A common offset c = scale * N(0,1) under unit noise (un-normalised mean-pooled vectors): |x|^2 ~ 6e7, an L2 score is a
    multiple of 4 or 8, cosines crowd against 1."""
    rng = np.random.default_rng(3001)
    c = scale * rng.standard_normal(DIM)
    return _f32(c + rng.standard_normal((n, DIM))), _f32(c + rng.standard_normal((NQ, DIM)))


def mixed_magnitude(n: int = N):
    """N(0,1) rows times 2^e, e uniform in [-10, 10] per row; queries likewise: one int8 query scale for the whole batch, row norms
    over 2^40 of range."""
    rng = np.random.default_rng(4001)
    X = rng.standard_normal((n, DIM)) * np.exp2(rng.integers(-10, 11, n))[:, None]
    Q = rng.standard_normal((NQ, DIM)) * np.exp2(rng.integers(-10, 11, NQ))[:, None]
    return _f32(X), _f32(Q)


def scaled(s: int, n: int = N):
    """One N(0,1) corpus and query set times 2^s (exact in f32): |x|^2 = 64 * 2^(2 s), nothing under- or overflows for |s| <= 40."""
    rng = np.random.default_rng(5001)
    X, Q = _f32(rng.standard_normal((n, DIM))), _f32(rng.standard_normal((NQ, DIM)))
    return _f32(np.ldexp(X, s)), _f32(np.ldexp(Q, s))


def zero_norm(n: int = N):
    """An N(0,1) corpus with ZERO_ROWS all zero (first row, last row, a lone row, a whole 256-row tile, three in a row) and the
    queries ZERO_QUERIES all zero."""
    rng = np.random.default_rng(6001)
    X, Q = _f32(rng.standard_normal((n, DIM))), _f32(rng.standard_normal((NQ, DIM)))
    X[ZERO_ROWS[ZERO_ROWS < n]] = 0.0
    Q[list(ZERO_QUERIES)] = 0.0
    return X, Q


def zero_norm_small():
    """300 rows, 295 of them zero: fewer non-zero rows than k = 10."""
    rng = np.random.default_rng(6002)
    X = np.zeros((300, DIM), np.float32)
    keep = np.array([7, 64, 128, 255, 299])
    X[keep] = _f32(rng.standard_normal((5, DIM)))
    return X, _f32(rng.standard_normal((40, DIM)))


def outlier_columns(n: int = N):
    """Two constant columns of 300 in an N(0,1) corpus (every row's int8 step is 300 / 127: the informative columns round to 0 or
    +-1), queries zero there: the corpus of test_int8_stage_hands_hard_queries_on_and_switches_itself_off at dim 64."""
    rng = np.random.default_rng(7001)
    X, Q = _f32(rng.standard_normal((n, DIM))), _f32(rng.standard_normal((NQ, DIM)))
    X[:, :2] = 300.0
    Q[:, :2] = 0.0
    return X, Q


SCALES = (-40, -12, 0, 12, 40)
FAMILIES = {
    "copies1500": lambda: copies(1500),
    "copies100": lambda: copies(100),
    "copies12": lambda: copies(12),
    "ternary": ternary,
    "offset": offset,
    "mixed_magnitude": mixed_magnitude,
    **{f"scaled{s:+d}": (lambda s=s: scaled(s)) for s in SCALES},
    "zero_norm": zero_norm,
    "outlier_columns": outlier_columns,
}


@lru_cache(maxsize=2)
def family(name: str):
    """(X, Q) of FAMILIES[name], read-only (shared between the cases that use it)."""
    X, Q = FAMILIES[name]()
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tie_counts(X, Q, metric: str, depth: int, k: int = 10):
    """Rows of X whose oracle score has the bits of the k-th best, per query, counted inside the oracle's top-`depth` (the oracle
    has no call that returns every score): exact where the ties end before `depth`, i.e. a count below depth - k + 1, and a lower
    bound otherwise."""
    from oracle import sc_oracle as orc

    d, _ = orc.search(X, Q, depth, metric)
    return (bits(d) == bits(d[:, k - 1:k])).sum(axis=1)
