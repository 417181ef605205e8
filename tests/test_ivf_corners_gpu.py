"""GPU: three corners of the IVF planner that the differential sweep cannot reach or used to hide.

1. More trained lists than the handle was created for (set_ivf / assign_lists install any number; a collection saved with one nlist
   and loaded into a store configured with another): the coarse stage's per-list statistics are sized and indexed by the TRAINED
   count, also when lists are installed again on a handle that already searched.
2. Queries the coarse stage cannot certify where the list-major probe has no plan (nprobe * k > 8192): per-query probing answers
   them; nothing is refused, and every query of the batch is answered under probe semantics.
3. Fallbacks of the coarse stage while rows lie behind the lists as a tail: the tail is scanned once, whatever answers the lists, and
   an allocation failure on a later 4 096-query chunk does not fail the call.

Every result is compared as ids and f32 bits with a reference that does not run the path under test: the CPU restatement
(oracle/ivf_oracle.py) where the centroids are its own, per-query probing of the same index asked right after otherwise."""
import functools

import numpy as np
import pytest

from oracle.ivf_oracle import IvfOracle
from semcode_amd import _native

pytestmark = pytest.mark.gpu
DIM = 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clustered(n, d, ncl, seed, spread=0.35):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((ncl, d)).astype(np.float32)
    lab = rng.integers(0, ncl, size=n)
    return (centers[lab] + spread * rng.standard_normal((n, d))).astype(np.float32), centers


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))


def search(ix, mode, Q, k, nprobe):
    ix.set_search_mode(mode)
    d, r = ix.search(Q, k=k, nprobe=nprobe)
    return (d, r), ix.last_search_stats()


# ---- 1. trained list count != the handle's ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mismatch_data():
    X, centers = clustered(20_000, DIM, 40, seed=101)
    rng = np.random.default_rng(102)
    Q = (centers[rng.integers(0, 40, size=40)] + 0.3 * rng.standard_normal((40, DIM))).astype(np.float32)
    X.setflags(write=False)
    Q.setflags(write=False)
    return X, Q


@functools.lru_cache(maxsize=None)
def mismatch_ref(metric, nlist):
    """The oracle's own centroids and lists, and its answers at nprobe = 8 for k = 10 and 100 (computed once per metric)."""
    X, Q = mismatch_data()
    ref = IvfOracle(X, metric, nlist=nlist, niter=3)
    return ref, {k: ref.search(Q, k, 8) for k in (10, 100)}


def install(ix, ref, how):
    if how == "set_ivf":
        ix.set_ivf(ref.centroids, ref.assign)
    else:
        ix.assign_lists(ref.centroids)
        assert np.array_equal(ix.ivf_assignments(), ref.assign)
    assert ix.ivf_info()["nlist"] == ref.nlist


@pytest.mark.parametrize("how", ["set_ivf", "assign_lists"])
@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_more_trained_lists_than_the_handle_was_created_for(rt, metric, how):
    """96 lists installed on a handle created with nlist = 16: the coarse stage answers as the oracle does, and certifies as many
    queries as on a twin handle created with nlist = 96 (statistics of list 16 and up, and max |x|^2 behind them, all in bounds)."""
    X, Q = mismatch_data()
    ref, want = mismatch_ref(metric, 96)
    ix = _native.Index(rt, DIM, metric=metric, kind="IVF_FLAT", nlist=16)
    twin = _native.Index(rt, DIM, metric=metric, kind="IVF_FLAT", nlist=96)
    try:
        for h in (ix, twin):
            h.add(X)
            install(h, ref, how)
        for k in (10, 100):
            got, st = search(ix, "ivf_coarse", Q, k, 8)
            got2, st2 = search(twin, "ivf_coarse", Q, k, 8)
            assert st["path"] == "ivf_coarse" and st2["path"] == "ivf_coarse", (st, st2)
            assert same(got, want[k]) and same(got2, want[k]), (metric, how, k, st)
            assert st["uncertified"] <= st2["uncertified"], (st, st2)
    finally:
        ix.close(); twin.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_per_list_statistics_follow_every_install_on_one_handle(rt, metric):
    """16 lists, a search (the statistics exist now), 96 lists, a search, train() back to 16, a search: each equals the oracle."""
    X, Q = mismatch_data()
    ref16, want16 = mismatch_ref(metric, 16)
    ref96, want96 = mismatch_ref(metric, 96)
    ix = _native.Index(rt, DIM, metric=metric, kind="IVF_FLAT", nlist=16)
    try:
        ix.add(X)
        for step, (ref, want) in enumerate(((ref16, want16), (ref96, want96), (None, want16))):
            if ref is None:
                ix.train(niter=3)  # the deterministic build the oracle restates: ref16's centroids and lists
                assert np.array_equal(bits(ix.ivf_info()["centroids"]), bits(ref16.centroids))
            else:
                install(ix, ref, "set_ivf")
            for k in (10, 100):
                got, st = search(ix, "ivf_coarse", Q, k, 8)
                assert st["path"] == "ivf_coarse", st
                assert same(got, want[k]), (metric, step, k, st)
    finally:
        ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_fewer_trained_lists_than_the_handle_was_created_for(rt, metric):
    """40 rows in a handle created with nlist = 64: train() builds 40 lists."""
    X, _ = mismatch_data()
    X40 = np.ascontiguousarray(X[:4000:100])
    Q = np.ascontiguousarray(X40[::7] * np.float32(1.01))
    ref = IvfOracle(X40, metric, nlist=64, niter=3)
    assert ref.nlist == 40
    ix = _native.Index(rt, DIM, metric=metric, kind="IVF_FLAT", nlist=64)
    try:
        ix.add(X40)
        ix.train(niter=3)
        assert ix.ivf_info()["nlist"] == 40
        got, st = search(ix, "ivf_coarse", Q, 5, 8)
        assert st["path"] == "ivf_coarse", st
        assert same(got, ref.search(Q, 5, 8)), (metric, st)
    finally:
        ix.close()


# ---- 2. the exact re-probe of uncertified queries where list-major has no plan -----------------------------------------------------------

NDUP, NGRP, GRP = 700, 10, 300


@functools.lru_cache(maxsize=None)
def dup_data(n):
    """n rows in 40 clusters; the last 700 of them near-duplicates of row 123 (gaps far below any int8 bound: a query among them has
    all 700 within reach of its k-th distance, 512 are re-scored for the bound, and a refine step limited to 8 rows cannot take the
    rest: uncertified); before them ten tight groups of 300 rows far from every cluster and from each other (a query inside one has
    its k <= 256 neighbours, and nothing else, within reach: all among the 512 re-scored for the bound, the refine step takes on
    none: certified).  Queries: duplicates, and fresh points inside the groups."""
    X, _ = clustered(n, DIM, 40, seed=111)
    rng = np.random.default_rng(112)
    X[n - NDUP:] = X[123][None, :] + np.float32(1e-4) * rng.standard_normal((NDUP, DIM)).astype(np.float32)
    gc = (3.0 * rng.standard_normal((NGRP, DIM))).astype(np.float32)
    g0 = n - NDUP - NGRP * GRP
    X[g0:n - NDUP] = np.repeat(gc, GRP, axis=0) + (0.05 * rng.standard_normal((NGRP * GRP, DIM))).astype(np.float32)
    plain = (gc[np.arange(100) % NGRP] + 0.05 * rng.standard_normal((100, DIM))).astype(np.float32)
    dups = X[n - NDUP:n - NDUP + 24].copy()
    X.setflags(write=False)
    return X, dups, plain


def check_fallback(rt, n, mode):
    X, dups, plain = dup_data(n)
    one = np.concatenate([plain[:5], dups[:1], plain[5:8]])   # exactly one query for the exact re-probe
    many = np.concatenate([dups, plain[:76]])                 # 24 of 100: at least twenty, and below the quarter that switches the stage off
    ix = _native.Index(rt, DIM, metric="L2", kind="IVF_FLAT", nlist=128)
    try:
        ix.add(X)
        ix.train(niter=3)
        _native.diag_set_option("ivf_refine_cap", 8)
        for k in (128, 129, 200, 256):  # 64 * 128 = 8192: the last k with a list-major plan
            for Q, lo, hi in ((one, 1, 1), (many, 20, 25)):
                got, st = search(ix, mode, Q, k, 64)
                print(f"n {n} mode {mode} k {k} Q {len(Q)}: {st}")
                assert st["path"] == "ivf_coarse", (k, st)
                assert lo <= st["uncertified"] <= hi, (k, st)
                want, rst = search(ix, "ivf", Q, k, 64)
                assert rst["path"] == "ivf", rst
                assert same(got, want), (mode, k, len(Q), st)
    finally:
        _native.diag_set_option("ivf_refine_cap", -1)
        ix.close()


def test_uncertified_queries_without_a_listmajor_plan_are_probed_per_query(rt):
    check_fallback(rt, 30_000, "ivf_coarse")


def test_uncertified_queries_without_a_listmajor_plan_in_auto_mode(rt):
    check_fallback(rt, 100_000, "auto")  # (the coarse stage takes an auto-mode batch from 100 000 rows on)


# ---- 3. fallbacks with a tail behind the lists ----------------------------------------------------------------------------------------------

TAIL_CASES = [(129, 64), (10, 6)]  # no list-major plan (64 * 129 > 8192: per-query probing must answer the lists) | list-major serves


def check_tail_fallback(rt, n, mode, nq, k, nprobe):
    """The appended rows are the queries scaled by 1.0001: each leads its query's top-k, so a tail that enters the merge twice shows
    as a repeated row id at once.  (One case per index: in auto mode the stage stays off once it ran out of memory.)"""
    X, centers = clustered(n, DIM, 40, seed=121)
    rng = np.random.default_rng(122)
    Qall = (centers[rng.integers(0, 40, size=400)] + 0.3 * rng.standard_normal((400, DIM))).astype(np.float32)
    Q = Qall[:nq]
    ix = _native.Index(rt, DIM, metric="L2", kind="IVF_FLAT", nlist=128)
    try:
        ix.add(X)
        ix.train(niter=3)
        ix.add(Qall * np.float32(1.0001))
        before, st0 = search(ix, "ivf", Q, k, nprobe)
        assert st0["path"] == "ivf" and st0["tail_rows"] == 400, st0
        assert np.array_equal(before[1][:, 0], n + np.arange(nq))
        _native.diag_set_option("ivf_coarse_nomem", 1)
        got, st = search(ix, mode, Q, k, nprobe)
        _native.diag_set_option("ivf_coarse_nomem", 0)
        print(f"n {n} mode {mode} k {k} nprobe {nprobe}: {st}")
        twice = [(i, int(v)) for i, row in enumerate(got[1]) for v, c in zip(*np.unique(row[row >= 0], return_counts=True)) if c > 1]
        assert not twice, (k, nprobe, st, twice[:8])
        # list-major serves where it has a plan, as it did; per-query probing where not; the tail stays a tail
        assert st["path"] == ("ivf_listmajor" if nprobe * k <= 8192 else "ivf") and st["tail_rows"] == 400, st
        after, st1 = search(ix, "ivf", Q, k, nprobe)
        assert st1["path"] == "ivf" and st1["tail_rows"] == 400, st1
        assert same(before, after) and same(got, after), (mode, k, nprobe, st)
    finally:
        _native.diag_set_option("ivf_coarse_nomem", 0)
        ix.close()


@pytest.mark.parametrize("k,nprobe", TAIL_CASES)
def test_coarse_stage_out_of_memory_with_a_tail_scans_the_tail_once(rt, k, nprobe):
    check_tail_fallback(rt, 30_000, "ivf_coarse", 400, k, nprobe)


@pytest.mark.parametrize("k,nprobe", TAIL_CASES)
def test_coarse_stage_out_of_memory_with_a_tail_in_auto_mode(rt, k, nprobe):
    check_tail_fallback(rt, 100_000, "auto", 8, k, nprobe)


def test_out_of_memory_on_a_later_chunk_leaves_the_rest_to_the_exact_probe(rt):
    """4 100 queries go through the coarse stage in chunks of 4 096; the second chunk runs out of memory: the call succeeds, the first
    chunk keeps its results and the other four queries are probed list-major -- the same bits as list-major probing of them all."""
    X, centers = clustered(20_000, DIM, 40, seed=131)
    rng = np.random.default_rng(132)
    Q = (centers[rng.integers(0, 40, size=4100)] + 0.3 * rng.standard_normal((4100, DIM))).astype(np.float32)
    ix = _native.Index(rt, DIM, metric="L2", kind="IVF_FLAT", nlist=32)
    try:
        ix.add(X)
        ix.train(niter=3)
        want, st4 = search(ix, "ivf_listmajor", Q, 10, 6)
        assert st4["path"] == "ivf_listmajor", st4
        whole, st5 = search(ix, "ivf_coarse", Q, 10, 6)
        assert st5["path"] == "ivf_coarse" and same(whole, want), st5
        _native.diag_set_option("ivf_coarse_nomem", 2)
        got, st = search(ix, "ivf_coarse", Q, 10, 6)
        assert same(got, want), st
    finally:
        _native.diag_set_option("ivf_coarse_nomem", 0)
        ix.close()
