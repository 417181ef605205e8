"""GPU: the grouped search (sc_index_set_groups + sc_index_search_grouped*: selection and exclusion kernels around the exact scans)
against the CPU oracle.

Bar: for every query the answer is the walk over the FULL canonical order of the allowed rows -- orc.search(X[allowed], Q,
k=len(allowed), metric), indices mapped back through `allowed` as in tests/test_masked_gpu.py::reference -- keeping a row when no
earlier row had its label, cut and padded to k.  Ids compared with np.array_equal, distances by their uint32 view.  The shapes are
the smallest that reach every branch: 3 001 rows (a ragged tile and a ragged bitset word), so the full order costs milliseconds.
"""
import numpy as np
import pytest

from oracle import sc_oracle as orc
from semcode_amd import _native
from semcode_amd.storage import MilvusVectorStore

pytestmark = pytest.mark.gpu

METRICS = ["IP", "L2", "COSINE"]
N = 3001


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def full_order(X, Q, metric, allowed=None):
    """(dist [Q, m], local rows [Q, m]): every allowed row, best first, ties by lower row id."""
    idx = np.arange(len(X)) if allowed is None else np.flatnonzero(allowed)
    if idx.size == 0:
        return np.zeros((len(Q), 0), np.float32), np.zeros((len(Q), 0), np.int64)
    od, orow = orc.search(X[idx], Q, int(idx.size), metric)
    assert (orow >= 0).all()
    return od, idx[orow]


def dedup(order, labels, k, metric, row_base=0):
    """The host way over the full order: first row of every label, cut and padded to k."""
    od, orow = order
    nq = len(od)
    dist = np.full((nq, k), np.inf if metric == "L2" else -np.inf, np.float32)
    rows = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        _, first = np.unique(labels[orow[q]], return_index=True)
        first = np.sort(first)[:k]
        dist[q, : first.size] = od[q, first]
        rows[q, : first.size] = orow[q, first] + row_base
    return dist, rows


def check_grouped(ix, Q, order, labels, k, metric, allow=None, row_base=0, what="", nq=None):
    """order: full_order(...) for (at least the first nq of) these queries and this mask; nq: use the first nq queries."""
    od, orow = order
    nq = len(od) if nq is None else nq
    d, r = ix.search_grouped(Q[:nq], k=k, allow=allow)
    wd, wr = dedup((od[:nq], orow[:nq]), labels, k, metric, row_base)
    assert np.array_equal(r, wr), f"{metric} {what}: row ids / order differ"
    assert np.array_equal(bits(d), bits(wd)), f"{metric} {what}: distances not bit-exact"
    assert ix.last_search_stats()["path"] == "grouped", what
    return d, r


def run_labels(n, lo, hi, seed):
    """Runs of lo..hi consecutive rows share a label (the chunks of one file)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, n)
    return np.repeat(np.arange(n, dtype=np.int32), sizes)[:n].astype(np.int32)


def scattered_labels(n, groups, seed):
    """Labels scattered at random over the rows; the values are negative and huge (opaque: compared for equality only)."""
    rng = np.random.default_rng(seed)
    values = np.unique(np.concatenate([rng.integers(-2**31, 2**31, groups), [-2**31, 2**31 - 1, -1, 0]])).astype(np.int64)
    return values[rng.integers(0, len(values), n)].astype(np.int32)


@pytest.fixture(scope="module")
def corpora():
    """Per dim: X, 17 queries, and per metric the full canonical order of all rows for these queries (computed once, read only)."""
    out = {}
    for dim in (64, 100):
        X = orc.synth(N, dim, seed=81)
        Q = orc.synth(17, dim, seed=82)
        out[dim] = (X, Q, {m: full_order(X, Q, m) for m in METRICS})
    return out


@pytest.fixture(autouse=True)
def default_widths():
    yield
    _native.diag_set_option("group_width0", -1)
    _native.diag_set_option("group_width1", -1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [64, 100])
def test_random_labels(rt, corpora, metric, dim):
    X, Q, orders = corpora[dim]
    ix = _native.Index(rt, dim, metric=metric)
    ix.add(X)
    runs = run_labels(N, 1, 40, 7)
    ix.set_groups(runs)
    for nq in (1, 3, 17):
        for k in (1, 10, 128):
            check_grouped(ix, Q, orders[metric], runs, k, metric, nq=nq, what=f"runs Q={nq} k={k}")
            if k <= 10:  # the 32 / 40 candidates of round 0 hold 10 of these ~150 labels for every query: it answers
                st = ix.last_group_stats()
                assert st["rounds"] == 0 and st["queries_continued"] == 0 and st["first_width"] == max(32, 4 * k) and st["rows_scanned"] == N, (nq, k, st)
    scattered = scattered_labels(N, 300, 8)
    ix.set_groups(scattered)  # replaces the earlier set
    for nq, k in ((1, 10), (3, 128), (17, 1), (17, 10)):
        check_grouped(ix, Q, orders[metric], scattered, k, metric, nq=nq, what=f"scattered Q={nq} k={k}")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_extreme_labellings(rt, corpora, metric):
    X, Q, orders = corpora[100]
    ix = _native.Index(rt, 100, metric=metric)
    ix.add(X)
    # all distinct: the plain exact search, bit for bit
    distinct = np.random.default_rng(9).permutation(N).astype(np.int32) - 1500
    ix.set_groups(distinct)
    for k in (1, 10, 128):
        d, r = check_grouped(ix, Q, orders[metric], distinct, k, metric, what=f"distinct k={k}")
        assert ix.last_group_stats()["rounds"] == 0
        d0, r0 = ix.search(Q, k=k)
        assert np.array_equal(r, r0) and np.array_equal(bits(d), bits(d0))
    # all equal: one hit plus padding (one exclusion round per query shows that nothing is left)
    same = np.full(N, -7, np.int32)
    ix.set_groups(same)
    d, r = check_grouped(ix, Q, orders[metric], same, 10, metric, what="all equal")
    assert (r[:, 0] >= 0).all() and (r[:, 1:] == -1).all() and np.isinf(d[:, 1:]).all() and (d[:, 1:] > 0).all() == (metric == "L2")
    d1, r1 = ix.search(Q, k=1)
    assert np.array_equal(r[:, :1], r1) and np.array_equal(bits(d[:, :1]), bits(d1))
    check_grouped(ix, Q, orders[metric], same, 1, metric, what="all equal k=1")
    assert ix.last_group_stats()["rounds"] == 0  # k labels found in round 0
    # fewer labels than k
    few = (np.arange(N) % 7).astype(np.int32)
    ix.set_groups(few)
    for k in (10, 128):
        d, r = check_grouped(ix, Q, orders[metric], few, k, metric, what=f"7 labels k={k}")
        assert (r[:, :7] >= 0).all() and (r[:, 7:] == -1).all()
        assert sorted(few[r[0, :7]].tolist()) == list(range(7))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_dominating_label_takes_exclusion_rounds(rt, corpora, metric):
    """The 1 500 rows closest to a query share one label: its first 1 500 candidates are one hit.  Round 0 cannot answer it, one
    exclusion round (64 candidates over the rows of every other label, which lie in runs of about 20) does."""
    X, Q, orders = corpora[64]
    od, orow = orders[metric]
    labels = run_labels(N, 1, 40, 10) + 1
    labels[orow[0, :1500]] = 0
    ix = _native.Index(rt, 64, metric=metric)
    ix.add(X)
    ix.set_groups(labels)
    check_grouped(ix, Q, orders[metric], labels, 10, metric, nq=1, what="dominant")
    st = ix.last_group_stats()
    assert st["queries_continued"] == 1 and st["rounds"] == 1 and st["rows_scanned"] == N + int((labels != 0).sum()), st
    check_grouped(ix, Q, orders[metric], labels, 10, metric, what="dominant, 17 queries")  # the other queries see that label often, too
    st = ix.last_group_stats()
    assert 1 <= st["queries_continued"] <= 17 and st["rounds"] >= st["queries_continued"], st
    check_grouped(ix, Q, orders[metric], labels, 128, metric, nq=3, what="dominant k=128")
    assert ix.last_group_stats()["rounds"] >= 1
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_forced_narrow_widths_give_the_same_answers(rt, corpora, metric):
    """Widths of 16 on the same inputs: many rounds, the same bits.  `staircase` puts the rows of query 0, best first, into groups of
    100: every list of 16 candidates holds one new label, so top-10 takes round 0 and nine exclusion rounds."""
    X, Q, orders = corpora[100]
    runs = run_labels(N, 1, 40, 11)
    od, orow = orders[metric]
    staircase = np.empty(N, np.int32)
    staircase[orow[0]] = np.arange(N) // 100 - 15
    ix = _native.Index(rt, 100, metric=metric)
    ix.add(X)
    for name, labels in (("runs", runs), ("staircase", staircase)):
        ix.set_groups(labels)
        wide = {(nq, k): check_grouped(ix, Q, orders[metric], labels, k, metric, nq=nq, what=f"{name} default") for nq, k in ((1, 10), (3, 128), (17, 10))}
        _native.diag_set_option("group_width0", 16)
        _native.diag_set_option("group_width1", 16)
        for (nq, k), (d0, r0) in wide.items():
            d, r = check_grouped(ix, Q, orders[metric], labels, k, metric, nq=nq, what=f"{name} narrow Q={nq} k={k}")
            st = ix.last_group_stats()
            assert st["first_width"] == max(16, k), (name, nq, k, st)
            if name == "staircase" or k == 128:  # (16 candidates of `runs` hold 10 labels: round 0 answers top-10 there)
                assert st["queries_continued"] >= 1 and st["rounds"] >= 2, (name, nq, k, st)
            if name == "staircase" and (nq, k) == (1, 10):
                assert st["rounds"] == 9 and st["queries_continued"] == 1, st
            assert np.array_equal(r, r0) and np.array_equal(bits(d), bits(d0))
        _native.diag_set_option("group_width0", -1)
        _native.diag_set_option("group_width1", -1)
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lowest_row(rt, metric):
    base = orc.synth(700, 64, seed=83)
    X = np.tile(base, (4, 1))  # vector v occurs at rows v, v + 700, v + 1400, v + 2100: four equal scores
    Q = orc.synth(3, 64, seed=84)
    order = full_order(X, Q, metric)
    ix = _native.Index(rt, 64, metric=metric)
    ix.add(X)
    n = len(X)
    # (a) the copies of a vector in four labels: four hits with one distance, ids ascending
    by_copy = (np.arange(n) // 700 * 1000 + np.arange(n) % 700 // 5).astype(np.int32)
    # (b) the copies of a vector within one label: the group is represented by its lowest copy
    by_vector = (np.arange(n) % 700 // 5).astype(np.int32)
    # (c) copies 0 and 2 in one label, 1 and 3 in another
    mixed = (np.arange(n) // 700 % 2 * 1000 + np.arange(n) % 700 // 5).astype(np.int32)
    for name, labels in (("across", by_copy), ("within", by_vector), ("mixed", mixed)):
        ix.set_groups(labels)
        for k in (10, 128):
            d, r = check_grouped(ix, Q, order, labels, k, metric, what=f"{name} k={k}")
            same = (bits(d)[:, 1:] == bits(d)[:, :-1]) & (r[:, 1:] >= 0)
            assert (np.diff(r, axis=1)[same] > 0).all()
            if name == "within":
                assert (r[r >= 0] < 700).all()
            if name == "mixed":
                assert (r[r >= 0] < 1400).all() and same.any()
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_with_an_allow_mask(rt, corpora, metric):
    X, Q, orders = corpora[100]
    labels = run_labels(N, 1, 40, 12)
    ix = _native.Index(rt, 100, metric=metric)
    ix.add(X)
    ix.set_groups(labels)
    rng = np.random.default_rng(13)
    half = rng.random(N) < 0.5
    for k in (10, 128):
        check_grouped(ix, Q, full_order(X, Q, metric, half), labels, k, metric, allow=half, what=f"50% k={k}")
    # word form with every padding bit beyond n set: ignored
    words = _native.pack_allow(half, N).copy()
    words[-1] |= np.uint32((0xFFFFFFFF << (N % 32)) & 0xFFFFFFFF)
    check_grouped(ix, Q, full_order(X, Q, metric, half), labels, 10, metric, allow=words, what="words")
    # narrow widths with a mask: the exclusion kernel ANDs the user's bits
    _native.diag_set_option("group_width0", 16)
    _native.diag_set_option("group_width1", 16)
    check_grouped(ix, Q, full_order(X, Q[:3], metric, half), labels, 128, metric, allow=half, nq=3, what="50% narrow")
    assert ix.last_group_stats()["rounds"] >= 2
    _native.diag_set_option("group_width0", -1)
    _native.diag_set_option("group_width1", -1)
    # one row, no row, every row
    one = np.arange(N) == 1234
    d, r = check_grouped(ix, Q, full_order(X, Q, metric, one), labels, 10, metric, allow=one, what="one row")
    assert (r[:, 0] == 1234).all() and (r[:, 1:] == -1).all()
    none = np.zeros(N, bool)
    d, r = check_grouped(ix, Q, full_order(X, Q, metric, none), labels, 10, metric, allow=none, what="empty")
    assert (r == -1).all() and np.isinf(d).all() and (d > 0).all() == (metric == "L2")
    d, r = check_grouped(ix, Q, orders[metric], labels, 10, metric, allow=np.ones(N, bool), what="full mask")
    # a group whose best rows are disallowed is represented by its best allowed row
    od, orow = orders[metric]
    best = orow[0, 0]
    big = labels.copy()
    big[orow[0, :50]] = labels[best]  # the 50 best rows of query 0 in one group ...
    ix.set_groups(big)
    allow = np.ones(N, bool)
    allow[orow[0, :49]] = False  # ... of which only the 50th is allowed
    d, r = check_grouped(ix, Q, full_order(X, Q, metric, allow), big, 10, metric, allow=allow, what="best rows disallowed")
    assert r[0, 0] == orow[0, 49] and big[r[0, 0]] == labels[best]
    ix.close()


def ivf_state(ix):
    info = ix.ivf_info()
    return info["nlist"], info["list_sizes"].tolist(), bits(info["centroids"]).tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_trained_ivf_is_scanned_as_it_lies(rt, metric):
    """A trained IVF_FLAT index with an appended tail and overwritten rows (tests/test_masked_gpu.py::
    test_trained_ivf_is_scanned_where_its_rows_lie): grouped searches with and without a mask answer over the current vectors;
    afterwards the lists are what they are in a twin that never ran a grouped search, and an unmasked exact search returns the
    same bits as the twin's and the oracle's."""
    n, dim = 6000, 64
    X = orc.synth(n, dim, seed=85)
    Q = orc.synth(5, dim, seed=86)
    ix, twin = (_native.Index(rt, dim, metric=metric, kind="IVF_FLAT", nlist=8) for _ in range(2))
    rng = np.random.default_rng(14)
    new = orc.synth(300, dim, seed=87)
    rows = rng.choice(n, 200, replace=False)
    over = orc.synth(200, dim, seed=88)
    for i in (ix, twin):
        i.add(X)
        i.train(niter=4, seed=3)
        i.add(new)
        i.overwrite(over, rows)
    X = np.concatenate([X, new])
    X[rows] = over
    labels = run_labels(len(X), 1, 40, 15)
    ix.set_groups(labels)
    order = full_order(X, Q, metric)
    check_grouped(ix, Q, order, labels, 10, metric, what="trained, unmasked")
    _native.diag_set_option("group_width0", 16)
    _native.diag_set_option("group_width1", 16)
    check_grouped(ix, Q, order, labels, 100, metric, what="trained, narrow")
    assert ix.last_group_stats()["rounds"] >= 2
    _native.diag_set_option("group_width0", -1)
    _native.diag_set_option("group_width1", -1)
    allowed = rng.random(len(X)) < 0.3
    check_grouped(ix, Q, full_order(X, Q, metric, allowed), labels, 10, metric, allow=allowed, what="trained, masked")
    for i in (ix, twin):
        i.set_search_mode("exact")
    d, r = ix.search(Q, k=10)
    d2, r2 = twin.search(Q, k=10)
    assert np.array_equal(r, order[1][:, :10]) and np.array_equal(bits(d), bits(order[0][:, :10]))
    assert np.array_equal(r, r2) and np.array_equal(bits(d), bits(d2))
    state = ivf_state(ix)
    assert state == ivf_state(twin) and state[0] == 8 and sum(state[1]) == len(X)
    ix.close()
    twin.close()


def test_larger_corpus_takes_the_batched_path_in_round_0(rt):
    n, dim, nq = 70_000, 64, 40
    ix = _native.Index(rt, dim, metric="L2")
    ix.fill_synthetic(n, seed=89)
    Q = orc.synth(nq, dim, seed=90)
    labels = run_labels(n, 1, 40, 16)
    ix.set_groups(labels)
    ix.set_search_mode("exact")
    d1, r1 = ix.search_grouped(Q, k=10)
    ix.search(Q, k=40)
    assert ix.last_search_stats()["path"] == "exact"
    ix.set_search_mode("auto")
    d0, r0 = ix.search_grouped(Q, k=10)
    assert ix.last_search_stats()["path"] == "grouped" and ix.last_group_stats()["first_width"] == 40
    ix.search(Q, k=40)  # what round 0 ran
    assert ix.last_search_stats()["path"] == "batched"
    assert np.array_equal(r0, r1) and np.array_equal(bits(d0), bits(d1))
    assert (r0 >= 0).all() and all(len(set(labels[r].tolist())) == 10 for r in r0)
    # ... and equal to the host way over a wide plain search (every query has 10 labels among its 400 best rows)
    dw, rw = ix.search(Q, k=400)
    wd, wr = dedup((dw, rw), labels, 10, "L2")
    assert np.array_equal(r0, wr) and np.array_equal(bits(d0), bits(wd))
    ix.close()


def test_device_pointer_variant_and_row_base(rt, corpora):
    import torch

    X, Q, orders = corpora[100]
    nq, k, base = 5, 10, 500
    labels = run_labels(N, 1, 40, 17)
    ix = _native.Index(rt, 100, metric="IP", row_base=base)
    ix.add(X)
    ix.set_groups(labels)
    d0, r0 = check_grouped(ix, Q, orders["IP"], labels, k, "IP", row_base=base, nq=nq, what="row_base")
    assert r0.min() >= base
    q = torch.from_numpy(Q[:nq]).cuda()
    d = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    r = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.search_grouped_dev(q.data_ptr(), nq, k, 0, 0, d.data_ptr(), r.data_ptr())
    rt.synchronize()
    assert np.array_equal(r.cpu().numpy(), r0) and np.array_equal(bits(d.cpu().numpy()), bits(d0))
    # with a mask, and narrow widths: rounds on device pointers
    allowed = np.random.default_rng(18).random(N) < 0.5
    words = _native.pack_allow(allowed, N)
    w = torch.from_numpy(words.view(np.int32).copy()).cuda()
    _native.diag_set_option("group_width0", 16)
    _native.diag_set_option("group_width1", 16)
    torch.cuda.synchronize()
    ix.search_grouped_dev(q.data_ptr(), nq, k, w.data_ptr(), words.size, d.data_ptr(), r.data_ptr())
    rt.synchronize()
    wd, wr = dedup(full_order(X, Q[:nq], "IP", allowed), labels, k, "IP", base)
    assert np.array_equal(r.cpu().numpy(), wr) and np.array_equal(bits(d.cpu().numpy()), bits(wd))
    ix.close()


def test_label_lifetime_and_invalid_arguments(rt, corpora):
    X, Q, orders = corpora[64]
    Q3 = Q[:3]
    ix = _native.Index(rt, 64, metric="L2")
    ix.add(X)
    d0, r0 = ix.search(Q3, k=10)
    stats = ix.last_search_stats()

    def refused(match, **kw):
        with pytest.raises(_native.ScError, match=match) as e:
            ix.search_grouped(kw.pop("q", Q3), **kw)
        assert e.value.status == -1  # SC_ERR_INVALID
        assert ix.last_search_stats() == stats and len(ix) == len(X)

    refused(rf"-1.*{N}", k=10)  # before set_groups: both counts are named
    labels = run_labels(N, 1, 40, 19)
    for bad in (labels[:-1], np.concatenate([labels, labels[:1]]), labels[:0]):
        with pytest.raises(_native.ScError) as e:
            ix.set_groups(bad)
        assert e.value.status == -1
    refused(rf"-1.*{N}", k=10)  # a refused install installs nothing
    ix.set_groups(labels)
    check_grouped(ix, Q, orders["L2"], labels, 10, "L2", nq=3, what="installed")
    d0, r0 = ix.search(Q3, k=10)
    stats = ix.last_search_stats()
    words = _native.pack_allow(np.ones(N, bool), N)
    refused("top_k", k=0)
    refused("top_k", k=129)
    refused("allow_words", k=10, allow=words[:-1])
    refused("Q=0|NULL", k=10, q=np.zeros((0, 64), np.float32))
    ix.release_scratch()  # the labels are not scratch
    check_grouped(ix, Q, orders["L2"], labels, 10, "L2", nq=3, what="after release_scratch")
    # an append outdates the labels
    extra = orc.synth(5, 64, seed=91)
    ix.add(extra)
    X = np.concatenate([X, extra])
    ix.search(Q3, k=10)
    stats = ix.last_search_stats()
    refused(rf"{N}.*{N + 5}", k=10)
    labels = np.concatenate([labels, np.full(5, labels[0], np.int32)])
    ix.set_groups(labels)
    order = full_order(X, Q3, "L2")
    check_grouped(ix, Q, order, labels, 10, "L2", what="re-installed after the append")
    # delete_rows drops them, even when the count is restored afterwards
    gone = np.array([0, 17, N + 4])
    ix.delete_rows(gone)
    X = np.delete(X, gone, axis=0)
    ix.add(orc.synth(3, 64, seed=92))
    X = np.concatenate([X, orc.synth(3, 64, seed=92)])
    assert len(ix) == N + 5
    ix.search(Q3, k=10)
    stats = ix.last_search_stats()
    refused(rf"-1.*{N + 5}", k=10)
    labels = np.concatenate([np.delete(labels, gone), np.array([5, 6, 7], np.int32)])
    ix.set_groups(labels)
    check_grouped(ix, Q, full_order(X, Q3, "L2"), labels, 10, "L2", what="re-installed after the delete")
    ix.close()
    # an empty index: zero labels are valid labels
    empty = _native.Index(rt, 64, metric="IP")
    empty.set_groups(np.zeros(0, np.int32))
    d, r = empty.search_grouped(Q3, k=5)
    assert (r == -1).all() and np.isneginf(d).all()
    empty.close()


@pytest.mark.parametrize("index_type", ["FLAT", "IVF_FLAT"])
def test_store_groups_on_the_real_index(rt, index_type, tmp_path):
    n, dim = 3000, 64
    X = orc.synth(n, dim, seed=93)
    repos = ["a", "b", "c"]
    sizes = np.random.default_rng(20).integers(1, 30, n)
    file_of = np.repeat(np.arange(n), sizes)[:n]
    meta = [{"repo": repos[int(f) % 3], "path": f"f{int(f) // 3}", "language": "py"} for f in file_of]
    s = MilvusVectorStore(dim=dim, metric="IP", index_type=index_type, nlist=8, nprobe=8, runtime=rt)
    s.connect()
    s.upsert_arrays([f"id{i}" for i in range(n)], X, [f"t{i}" for i in range(n)], meta)
    v = orc.synth(1, dim, seed=94)

    def check(store, X, group_by, top_k=5, **kw):
        keys = list(zip(store._repos, store._paths)) if group_by == "path" else list(store._repos)
        codes = {}
        labels = np.array([codes.setdefault(key, len(codes)) for key in keys], np.int32)
        allowed = np.array([kw.get("repos") is None or r in kw["repos"] for r in store._repos])
        hits = next(iter(store.search(v[0].tolist(), top_k=top_k, group_by=group_by, **kw)))
        wd, wr = dedup(full_order(X, v, "IP", allowed), labels, top_k, "IP")
        want = wr[0][wr[0] >= 0]
        assert [h.row for h in hits] == want.tolist() and np.array_equal(bits([h.distance for h in hits]), bits(wd[0][: len(want)]))
        assert len({keys[h.row] for h in hits}) == len(hits) and all(allowed[h.row] for h in hits)
        assert store._collection.last_search_stats()["path"] == "grouped"
        return hits

    check(s, X, "path")
    assert len(check(s, X, "repo")) == 3
    check(s, X, "path", repos=["b", "c"])
    assert len(check(s, X, "repo", repos=["b"])) == 1
    plain = next(iter(s.search(v[0].tolist(), top_k=5)))
    assert s._collection.last_search_stats()["path"] != "grouped" and len(plain) == 5
    # mutations: the labels on the device must not be reused -- rows move up after the delete, new rows arrive
    assert s.delete_where(repo="a") == int(sum(m["repo"] == "a" for m in meta))
    X = X[np.array([m["repo"] != "a" for m in meta])]
    check(s, X, "path")
    new = orc.synth(50, dim, seed=95)
    s.upsert_arrays([f"new{i}" for i in range(50)], new, ["t"] * 50, [{"repo": "b", "path": f"p{i // 10}", "language": "py"} for i in range(50)])
    X = np.concatenate([X, new])
    check(s, X, "path", top_k=20)
    check(s, X, "repo")
    check(s, X, "path", repos=["b"])
    # save -> load
    s.save(tmp_path / "c")
    t = MilvusVectorStore(dim=dim, metric="IP", index_type=index_type, nlist=8, nprobe=8, runtime=rt)
    t.connect()
    t.load(tmp_path / "c")
    a, b = check(s, X, "path", top_k=20), check(t, X, "path", top_k=20)
    assert [(h.id, h.distance) for h in a] == [(h.id, h.distance) for h in b]
    check(t, X, "repo", repos=["c", "b"])
    s.close()
    t.close()
