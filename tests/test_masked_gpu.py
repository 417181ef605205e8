"""GPU: the masked search (sc_index_search_masked*: mask compaction + gathered exact scan) against the CPU oracle.

Bar: a masked search returns, bit for bit, the exhaustive answer over the index that holds only the allowed rows -- reference
orc.search(X[allowed], Q, k, metric) with its indices mapped back through `allowed` (ascending, so the tie rule carries over) and
row_base added; ids and the uint32 view of the distances compared with np.array_equal, as in tests/test_scan_gpu.py.
"""
import numpy as np
import pytest

from oracle import sc_oracle as orc
from semcode_amd import _native
from semcode_amd.storage import MilvusVectorStore

pytestmark = pytest.mark.gpu

METRICS = ["IP", "L2", "COSINE"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reference(X, Q, k, metric, allowed, row_base=0):
    idx = np.flatnonzero(allowed)
    if idx.size == 0:
        return np.full((len(Q), k), np.inf if metric == "L2" else -np.inf, np.float32), np.full((len(Q), k), -1, np.int64)
    od, orow = orc.search(X[idx], Q, k, metric)
    return od, np.where(orow >= 0, idx[np.clip(orow, 0, None)] + row_base, -1)


def check_masked(ix, X, Q, k, metric, allowed, row_base=0, what=""):
    d, r = ix.search_masked(Q, allowed, k=k)
    od, orow = reference(X, Q, k, metric, allowed, row_base)
    assert np.array_equal(r, orow), f"{metric} {what}: row ids / order differ"
    assert np.array_equal(bits(d), bits(od)), f"{metric} {what}: distances not bit-exact"
    st = ix.last_mask_stats()
    assert st["allowed_rows"] == int(np.count_nonzero(allowed)), what
    return d, r


def random_mask(n, m, seed):
    a = np.zeros(n, bool)
    a[np.random.default_rng(seed).choice(n, m, replace=False)] = True
    return a


def mask_shapes(n):
    rng = np.random.default_rng(5)
    out = {f"m={m}": random_mask(n, m, 100 + m) for m in (1, 15, 16, 17, 63, 64, 65)}
    out["row 0"] = np.arange(n) == 0
    out["row n-1"] = np.arange(n) == n - 1
    out["last 5"] = np.arange(n) >= n - 5
    out["range"] = (np.arange(n) >= 1000) & (np.arange(n) < 2500)
    out["50%"] = rng.random(n) < 0.5
    out["1%"] = rng.random(n) < 0.01
    return out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [64, 100, 768])
def test_mask_shapes(rt, metric, dim):
    n = 4133
    X = orc.synth(n, dim, seed=51)
    Q = orc.synth(3, dim, seed=52)
    ix = _native.Index(rt, dim, metric=metric)
    ix.add(X)
    for name, allowed in mask_shapes(n).items():
        check_masked(ix, X, Q, 10, metric, allowed, what=name)
        assert ix.last_search_stats()["path"] == "masked" and ix.last_mask_stats()["gathered"], name
    # word form, every padding bit beyond n set (and a spare word of ones): ignored
    allowed = random_mask(n, 300, 7)
    words = _native.pack_allow(allowed, n).copy()
    words[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    words = np.concatenate([words, np.array([0xFFFFFFFF], np.uint32)])
    d, r = ix.search_masked(Q, words, k=10)
    od, orow = reference(X, Q, 10, metric, allowed)
    assert np.array_equal(r, orow) and np.array_equal(bits(d), bits(od))
    assert ix.last_mask_stats() == {"allowed_rows": 300, "scanned_rows": 300, "gathered": True}
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_fewer_allowed_rows_than_k(rt, metric):
    n = 4133
    X = orc.synth(n, 100, seed=53)
    Q = orc.synth(3, 100, seed=54)
    ix = _native.Index(rt, 100, metric=metric)
    ix.add(X)
    allowed = random_mask(n, 7, 8)
    for k in (10, 100):
        d, r = check_masked(ix, X, Q, k, metric, allowed, what=f"k={k}")
        assert (r[:, 7:] == -1).all() and (r[:, :7] >= 0).all() and np.isinf(d[:, 7:]).all()
    d, r = check_masked(ix, X, Q, 10, metric, np.zeros(n, bool), what="m=0")
    assert (r == -1).all() and np.isinf(d).all() and (d > 0).all() == (metric == "L2")
    assert ix.last_mask_stats() == {"allowed_rows": 0, "scanned_rows": 0, "gathered": False}
    ix.close()
    empty = _native.Index(rt, 100, metric=metric)
    d, r = empty.search_masked(Q, np.zeros(0, bool), k=5)
    assert (r == -1).all() and np.isinf(d).all() and empty.last_mask_stats()["scanned_rows"] == 0
    empty.close()


@pytest.fixture(scope="module")
def corpus_20k():
    return orc.synth(20_001, 128, seed=55)


@pytest.mark.parametrize("nq", [1, 16, 17, 33])
def test_query_groups(rt, corpus_20k, nq):
    X = corpus_20k
    Q = orc.synth(nq, 128, seed=56 + nq)
    allowed = np.random.default_rng(9).random(len(X)) < 0.3
    ix = _native.Index(rt, 128, metric="L2")
    ix.add(X)
    check_masked(ix, X, Q, 10, "L2", allowed)
    ix.close()


@pytest.mark.parametrize("k", [1, 2, 48, 49, 100, 257, 1024])
def test_k_range(rt, corpus_20k, k):
    X = corpus_20k
    Q = orc.synth(4, 128, seed=57)
    allowed = np.random.default_rng(10).random(len(X)) < 0.4
    ix = _native.Index(rt, 128, metric="IP")
    ix.add(X)
    check_masked(ix, X, Q, k, "IP", allowed)
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_long_rows_take_more_passes(rt, metric):
    """3 072-d rows leave LDS room for 6 resident queries: 16 queries are three groups of the gathered scan (there is no streamed
    variant of it), 17 a partial last group."""
    X = orc.synth(3_001, 3072, seed=77)
    allowed = np.random.default_rng(17).random(len(X)) < 0.3
    ix = _native.Index(rt, 3072, metric=metric)
    ix.add(X)
    for nq in (16, 17):
        check_masked(ix, X, orc.synth(nq, 3072, seed=78 + nq), 10, metric, allowed, what=f"Q={nq}")
    ix.close()


@pytest.mark.parametrize("n", [17, 4097, 20_001])
def test_full_mask(rt, n):
    X = orc.synth(n, 128, seed=58)
    Q = orc.synth(5, 128, seed=59)
    ix = _native.Index(rt, 128, metric="COSINE")
    ix.add(X)
    ix.set_search_mode("exact")
    k = min(10, n)
    d0, r0 = ix.search(Q, k=k)
    ones = np.ones(n, bool)
    try:
        _native.diag_set_option("mask_gather", 1)
        d1, r1 = check_masked(ix, X, Q, k, "COSINE", ones, what="forced gather")
        assert ix.last_search_stats()["path"] == "masked" and ix.last_mask_stats() == {"allowed_rows": n, "scanned_rows": n, "gathered": True}
    finally:
        _native.diag_set_option("mask_gather", 0)
    d2, r2 = check_masked(ix, X, Q, k, "COSINE", ones, what="planner")
    assert ix.last_search_stats()["path"] != "masked" and ix.last_mask_stats() == {"allowed_rows": n, "scanned_rows": n, "gathered": False}
    for d, r in ((d1, r1), (d2, r2)):
        assert np.array_equal(r, r0) and np.array_equal(bits(d), bits(d0))
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lowest_allowed_copy(rt, metric):
    base = orc.synth(700, 64, seed=60)
    X = np.tile(base, (4, 1))  # vector v occurs at rows v, v + 700, v + 1400, v + 2100
    Q = orc.synth(3, 64, seed=61)
    rng = np.random.default_rng(11)
    allowed = rng.random(2800) < 0.5  # a varying subset of every set of copies (some sets empty, some whole)
    ix = _native.Index(rt, 64, metric=metric)
    ix.add(X)
    d, r = check_masked(ix, X, Q, 40, metric, allowed)
    same = bits(d)[:, 1:] == bits(d)[:, :-1]  # equal distances come in runs, ids ascending inside a run
    assert same.any() and (np.diff(r, axis=1)[same] > 0).all()
    ix.close()


def test_row_base(rt):
    n = 4133
    X = orc.synth(n, 100, seed=62)
    Q = orc.synth(3, 100, seed=63)
    ix = _native.Index(rt, 100, metric="L2", row_base=500)
    ix.add(X)
    allowed = random_mask(n, 333, 12)
    d, r = check_masked(ix, X, Q, 10, "L2", allowed, row_base=500)
    assert r.min() >= 500 and allowed[r - 500].all()
    ix.close()


def ivf_state(ix):
    info = ix.ivf_info()
    return info["nlist"], info["list_sizes"].tolist(), bits(info["centroids"]).tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_trained_ivf_is_scanned_where_its_rows_lie(rt, metric):
    """Masked searches of a trained IVF_FLAT index right after train, with a pending tail, with pending overwritten rows and with
    both.  After each: the oracle's answer over the store's current vectors, and the index is left as it was -- no refresh, no
    re-layout, no k-means.  sc_index_ivf_info cannot show the state BEFORE a masked search with rows pending (the call itself folds
    pending rows into the lists), so `ix` is compared with a twin that goes through the same upserts WITHOUT the masked searches:
    the same nlist, list sizes and centroid bits at every step; and a probe right after the masked search still finds the
    appended rows behind the lists (tail_rows), i.e. the masked search folded nothing in."""
    n, dim = 20_000, 64
    X = orc.synth(n, dim, seed=64)
    Q = orc.synth(5, dim, seed=65)
    ix, twin = (_native.Index(rt, dim, metric=metric, kind="IVF_FLAT", nlist=16) for _ in range(2))
    for i in (ix, twin):
        i.add(X)
        i.train(niter=4, seed=3)
    trained = ivf_state(ix)
    assert trained[0] == 16 and trained == ivf_state(twin)
    rng = np.random.default_rng(13)

    def step(name, mutate, tail):
        nonlocal X
        X = mutate(X)
        allowed = rng.random(len(X)) < 0.3
        allowed[-1] = True
        check_masked(ix, X, Q, 10, metric, allowed, what=name)
        assert ix.last_search_stats()["path"] == "masked"
        if tail:  # an approximate probe next: it answers from the lists AND the tail, which the masked search left pending
            ix.set_search_mode("auto")
            ix.search(Q[:1], k=10, nprobe=2)
            stats = ix.last_search_stats()
            assert stats["path"].startswith("ivf") and stats["tail_rows"] == tail, (name, stats)
        ix.set_search_mode("exact")
        d, r = ix.search(Q, k=10)
        od, orow = orc.search(X, Q, 10, metric)
        assert np.array_equal(r, orow) and np.array_equal(bits(d), bits(od)), name
        state = ivf_state(ix)
        assert state == ivf_state(twin), name
        assert state[0] == 16 and sum(state[1]) == len(X) and state[2] == trained[2], name

    def append(X):
        new = orc.synth(300, dim, seed=66 + len(X))
        for i in (ix, twin):
            i.add(new)
        return np.concatenate([X, new])

    def overwrite(X):
        rows = rng.choice(n, 200, replace=False)
        new = orc.synth(200, dim, seed=67 + len(X))
        for i in (ix, twin):
            i.overwrite(new, rows)
        X = X.copy()
        X[rows] = new
        return X

    step("after train", lambda X: X, 0)
    step("tail", append, 300)
    step("overwritten", overwrite, 0)
    step("both", lambda X: overwrite(append(X)), 0)
    ix.close()
    twin.close()


@pytest.mark.parametrize("kind", ["FLAT", "IVF_FLAT"])
def test_after_delete_rows(rt, kind):
    n, dim = 20_000, 64
    X = orc.synth(n, dim, seed=68)
    Q = orc.synth(4, dim, seed=69)
    ix = _native.Index(rt, dim, metric="L2", kind=kind, nlist=16)
    ix.add(X)
    if kind == "IVF_FLAT":
        ix.train(niter=4, seed=3)
    rng = np.random.default_rng(14)
    gone = np.sort(rng.choice(n, n // 10, replace=False))
    ix.delete_rows(gone)
    X = np.delete(X, gone, axis=0)
    assert len(ix) == len(X)
    for frac in (0.3, 0.002):
        check_masked(ix, X, Q, 10, "L2", rng.random(len(X)) < frac, what=f"{kind} {frac}")  # a mask in the new numbering
    ix.close()


def test_device_pointer_variant(rt):
    import torch

    n, dim, nq, k = 20_001, 128, 5, 10
    X = orc.synth(n, dim, seed=70)
    Q = orc.synth(nq, dim, seed=71)
    allowed = np.random.default_rng(15).random(n) < 0.2
    ix = _native.Index(rt, dim, metric="IP")
    ix.add(X)
    d0, r0 = check_masked(ix, X, Q, k, "IP", allowed)
    words = _native.pack_allow(allowed, n)
    q = torch.from_numpy(Q).cuda()
    w = torch.from_numpy(words.view(np.int32).copy()).cuda()
    d = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    r = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.search_masked_dev(q.data_ptr(), nq, k, w.data_ptr(), words.size, d.data_ptr(), r.data_ptr())
    rt.synchronize()
    assert np.array_equal(r.cpu().numpy(), r0) and np.array_equal(bits(d.cpu().numpy()), bits(d0))
    assert ix.last_mask_stats()["allowed_rows"] == int(allowed.sum())
    ix.close()


def test_invalid_arguments_change_nothing(rt):
    n = 4133
    X = orc.synth(n, 64, seed=72)
    Q = orc.synth(3, 64, seed=73)
    ix = _native.Index(rt, 64, metric="L2")
    ix.add(X)
    d0, r0 = ix.search(Q, k=10)
    stats = ix.last_search_stats()
    words = _native.pack_allow(random_mask(n, 50, 16), n)
    for q, allow, k in ((Q, words[:-1], 10), (Q, words, 0), (Q, words, 1025), (np.zeros((0, 64), np.float32), words, 10)):
        with pytest.raises(_native.ScError) as e:
            ix.search_masked(q, allow, k=k)
        assert e.value.status == -1  # SC_ERR_INVALID
        assert ix.last_search_stats() == stats
    d1, r1 = ix.search(Q, k=10)
    assert np.array_equal(r1, r0) and np.array_equal(bits(d1), bits(d0))
    ix.close()


@pytest.mark.parametrize("index_type", ["FLAT", "IVF_FLAT"])
def test_store_filters_on_the_real_index(rt, index_type):
    n, dim = 3000, 64
    X = orc.synth(n, dim, seed=74)
    repos, langs = ["a", "b", "c"], ["py", "go"]
    meta = [{"repo": repos[i % 3], "path": f"f{i}", "language": langs[(i // 3) % 2]} for i in range(n)]
    s = MilvusVectorStore(dim=dim, metric="IP", index_type=index_type, nlist=8, nprobe=8, runtime=rt)
    s.connect()
    s.upsert_arrays([f"id{i}" for i in range(n)], X, [f"t{i}" for i in range(n)], meta)
    v = orc.synth(1, dim, seed=75)

    def check(X, **kw):
        cols = list(zip(s._repos, s._languages))
        allowed = np.array([(kw.get("repos") is None or r in kw["repos"]) and (kw.get("languages") is None or l in kw["languages"]) for r, l in cols])
        hits = next(iter(s.search(v[0].tolist(), top_k=5, **kw)))
        od, orow = reference(X, v, 5, "IP", allowed)
        assert [h.row for h in hits] == orow[0].tolist() and np.array_equal(bits([h.distance for h in hits]), bits(od[0]))
        assert all(allowed[h.row] for h in hits)
        assert s._collection.last_search_stats()["path"] == "masked"

    check(X, repos=["b"], languages={"py"})
    assert list(next(iter(s.search(v[0].tolist(), top_k=5, repos=[])))) == []
    plain = next(iter(s.search(v[0].tolist(), top_k=5)))
    every = next(iter(s.search(v[0].tolist(), top_k=5, repos=["a", "b", "c"])))
    assert s._collection.last_search_stats()["path"] != "masked"
    assert [(h.id, h.distance) for h in every] == [(h.id, h.distance) for h in plain]
    # mutations: the cached bitset must not be reused -- rows move up after the delete, new rows arrive
    assert s.delete_where(repo="a") == 1000
    X = X[np.arange(n) % 3 != 0]
    new = orc.synth(50, dim, seed=76)
    s.upsert_arrays([f"new{i}" for i in range(50)], new, ["t"] * 50, [{"repo": "b", "path": "p", "language": "py"}] * 50)
    X = np.concatenate([X, new])
    check(X, repos=["b"], languages={"py"})
    check(X, languages=["go"])
    s.close()
