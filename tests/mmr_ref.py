"""The reference of the MMR search (include/semcode_hip.h, sc_index_search_mmr), shared by tests/test_mmr_host.py and
tests/test_mmr_gpu.py: candidates and the candidate x candidate score matrix from the CPU oracle, the greedy selection in numpy
float32 -- one correctly rounded operation at a time, no fused multiply-add (np.float32 products and differences are exactly
that; nothing goes through float64)."""
import numpy as np

from oracle import sc_oracle as orc


def select(rel, G, k, lam):
    """rel [C] f32, G [C, >= C] f32 (oriented scores, larger is better) -> candidate indices in selection order."""
    rel = np.asarray(rel, dtype=np.float32)
    G = np.asarray(G, dtype=np.float32)
    C = len(rel)
    steps = min(int(k), C)
    if steps < 1:
        return []
    lam = np.float32(lam)
    mu = np.float32(1.0) - lam
    assert mu.dtype == np.float32
    picked = [0]
    taken = np.zeros(C, dtype=bool)
    taken[0] = True
    m = np.full(C, -np.inf, dtype=np.float32)
    for _ in range(1, steps):
        m = np.maximum(m, G[:C, picked[-1]])  # f32 max: exact (a column of a symmetric matrix = its row)
        a = lam * rel
        b = mu * m
        v = a - b
        assert a.dtype == b.dtype == v.dtype == np.float32
        left = np.flatnonzero(~taken)
        best = int(left[np.argmax(v[left])])  # argmax returns the first maximum: equal values keep the smaller index
        picked.append(best)
        taken[best] = True
    return picked


def candidates(X, Q, fetch_k, metric, allowed=None):
    """Per query (cand_dist [C], local rows [C], G [C, C]): the exact top-fetch_k of the allowed rows, best first, ties by lower row,
    and their score matrix (plain metric scores, not oriented).  X [n, dim] tight, allowed: bool [n] or None.  Shared between the
    tests that vary only k and lambda."""
    idx = np.arange(len(X)) if allowed is None else np.flatnonzero(allowed)
    C = min(fetch_k, len(idx))
    out = []
    if C == 0:
        return [(np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 0), np.float32)) for _ in Q]
    cd, cr = orc.search(X[idx], Q, C, metric)
    for i in range(len(Q)):
        cand = idx[cr[i]]  # idx is ascending: ties by lower local row survive the mapping
        gd, gr = orc.search(X[cand], X[cand], C, metric)
        G = np.empty((C, C), dtype=np.float32)
        np.put_along_axis(G, gr, gd, axis=1)
        assert np.array_equal(G.view(np.uint32), G.T.copy().view(np.uint32)), "the canonical score is not bitwise symmetric"
        out.append((cd[i].copy(), cand, G))
    return out


def answer(cands, k, lam, metric, row_base=0):
    """(dist [Q, k] f32, rows [Q, k] i64) of the definition from candidates()."""
    pad = np.float32(np.inf if metric == "L2" else -np.inf)
    sign = np.float32(-1.0 if metric == "L2" else 1.0)
    dist = np.full((len(cands), k), pad, dtype=np.float32)
    rows = np.full((len(cands), k), -1, dtype=np.int64)
    for i, (cd, cand, G) in enumerate(cands):
        picked = select(sign * cd, sign * G, k, lam)
        dist[i, : len(picked)] = cd[picked]
        rows[i, : len(picked)] = row_base + cand[picked]
    return dist, rows


def reference_batch(X, Q, k, fetch_k, lam, metric, allowed=None, row_base=0):
    return answer(candidates(X, Q, fetch_k, metric, allowed), k, lam, metric, row_base)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))
