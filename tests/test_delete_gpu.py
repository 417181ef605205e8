"""GPU: sc_index_delete_rows -- in-place compaction of the collection -- through the C ABI, and the store / ingest layers on top.

The yardstick is the twin: an index into which only the surviving vectors were put, in their order.  For FLAT indexes the
twin's answer is the oracle's over X[survivors] (ids and f32 distance bits, ties to the lower row id); for trained IVF_FLAT
indexes a second device index built from add(X[survivors]) + set_ivf(centroids, assign[survivors]), and oracle/ivf_oracle.py
for the probe of the survivors' lists.  Where a search mode is forced the path that answered is asserted, so no case passes by
falling back to the exact scan.
"""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import sc_oracle as orc
from oracle.ivf_oracle import IvfOracle, _assign_metric, _nearest
from semcode_amd import _native
from semcode_amd.embeddings import EmbeddingPayload
from semcode_amd.storage import MilvusVectorStore

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    r = _native.Runtime(device=0)
    yield r
    r.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def corpus(n, dim, seed):
    """Gaussian rows with duplicated vectors spread over the row range (ties across deleted rows)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if n >= 512:
        for group in ((0, 7, n // 2), (1, n // 3, n - 1), (255, 256, 257, n - 2), (300, n // 2 + 1)):
            X[list(group[1:])] = X[group[0]]
    return X


def queries(X, Q, seed):
    """Half of the queries are stored rows (the duplicated ones first), the rest random."""
    rng = np.random.default_rng(seed)
    n = len(X)
    q = rng.standard_normal((Q, X.shape[1])).astype(np.float32)
    own = [r for r in (0, 255, 1, 300) if r < n][: max(1, Q // 2)]
    own += rng.integers(0, n, size=max(0, Q // 2 - len(own))).tolist()
    q[: len(own)] = X[own]
    return q


def delete_set(name, n, seed):
    rng = np.random.default_rng(seed)
    if name == "first":
        return np.array([0])
    if name == "last":
        return np.array([n - 1])
    if name == "block":  # contiguous, across a 256-row boundary
        return np.arange(200, 330)
    if name == "random30":
        return rng.permutation(n)[: (3 * n) // 10]  # (unsorted on purpose)
    if name == "all_but_one":
        return np.delete(np.arange(n), n // 2)
    if name == "all":
        return rng.permutation(n)
    raise KeyError(name)


FLAT_PATHS = {  # name -> (search mode, coarse stage, path reported)
    "exact": ("exact", 0, "exact"),
    "batched8": ("batched", 8, "batched"),
    "batched16": ("batched", 16, "batched"),
}


def flat_search(ix, path, q, k):
    mode, coarse, want = FLAT_PATHS[path]
    ix.set_search_mode(mode)
    ix.set_coarse_stage(coarse)
    d, r = ix.search(q, k=k)
    st = ix.last_search_stats()
    assert st["path"] == want, (path, st)
    if coarse:
        assert st["coarse_bits"] == coarse, (path, st)
    return d, r


def check_flat(ix, Xs, metric, plan, seed):
    """plan: (path, Q, k) triples; bit-exact against the oracle over the surviving matrix."""
    n = len(Xs)
    for path, Q, k in plan:
        q = queries(Xs, Q, seed + Q + k)
        d, r = flat_search(ix, path, q, k)
        kk = min(k, n)
        wd, wr = orc.search(Xs, q, kk, metric)
        assert np.array_equal(r[:, :kk], wr) and np.array_equal(bits(d[:, :kk]), bits(wd)), (path, Q, k, n)
        assert (r[:, kk:] == -1).all()
    ix.set_search_mode("auto")
    ix.set_coarse_stage(0)


# every delete set meets every path; every metric, shape, Q and k occurs; batched16 serves k <= 64 only (existing behaviour:
# beyond that only the int8 stage has the candidates)
FLAT_CASES = [
    # set,       n,      dim, metric,   (path, Q, k) ...
    ("first",    5_000,  64,  "L2",     (("exact", 16, 128), ("batched8", 200, 10), ("batched16", 1, 1))),
    ("last",     5_000,  200, "IP",     (("exact", 1, 10), ("batched8", 16, 128), ("batched16", 200, 10))),
    ("block",    5_000,  64,  "COSINE", (("exact", 200, 1), ("batched8", 1, 10), ("batched16", 16, 10))),
    ("random30", 70_001, 200, "L2",     (("exact", 16, 10), ("batched8", 200, 128), ("batched16", 200, 1))),
    ("random30", 5_000,  64,  "IP",     (("exact", 200, 128), ("batched8", 16, 1), ("batched16", 1, 10))),
    ("block",    70_001, 64,  "COSINE", (("exact", 1, 1), ("batched8", 200, 10), ("batched16", 16, 10))),
]


@pytest.mark.parametrize("prebuilt", [True, False], ids=["shadows", "noshadows"])
@pytest.mark.parametrize("case", FLAT_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def test_flat_delete_matches_oracle(rt, case, prebuilt):
    name, n, dim, metric, plan = case
    X = corpus(n, dim, seed=n + dim)
    ix = _native.Index(rt, dim, metric=metric, kind="FLAT")
    ix.add(X)
    if prebuilt:  # search first in every mode: both shadows exist and are valid at the delete
        for path, Q, k in plan:
            flat_search(ix, path, queries(X, Q, 5), k)
    dele = delete_set(name, n, seed=3)
    ix.delete_rows(dele)
    keep = np.ones(n, bool)
    keep[dele] = False
    Xs = X[keep]
    assert len(ix) == len(Xs)
    st = ix.last_delete_stats()
    print(name, n, dim, metric, "prebuilt" if prebuilt else "bare", st)
    assert st["shadows_dropped"] == 0
    assert st["shadows_kept"] == (3 if prebuilt else 0)  # bf16 | int8: moved, not rebuilt
    assert st["rows_moved"] == (n - int(dele.min())) - len(dele)  # the survivors above the first deleted position
    assert np.array_equal(bits(ix.get_rows(0, len(Xs))), bits(Xs))
    check_flat(ix, Xs, metric, plan, seed=11)
    # the collection goes on living: append, overwrite, delete again
    more = corpus(300, dim, seed=9)
    ix.add(more)
    ix.overwrite(more[:5], np.arange(5))
    Xs = np.vstack([Xs, more])
    Xs[:5] = more[:5]
    ix.delete_rows([2, len(Xs) - 1])
    Xs = np.delete(Xs, [2, len(Xs) - 1], axis=0)
    assert ix.last_delete_stats()["shadows_dropped"] == 0
    check_flat(ix, Xs, metric, plan[:2], seed=12)
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("name", ["all_but_one", "all"])
def test_flat_delete_degenerate(rt, name, metric):
    n, dim = 5_000, 64
    X = corpus(n, dim, seed=4)
    ix = _native.Index(rt, dim, metric=metric, kind="FLAT")
    ix.add(X)
    flat_search(ix, "batched8", queries(X, 16, 5), 10)
    flat_search(ix, "batched16", queries(X, 16, 5), 10)
    ix.set_search_mode("auto")
    ix.set_coarse_stage(0)
    dele = delete_set(name, n, seed=3)
    ix.delete_rows(dele)
    st = ix.last_delete_stats()
    q = queries(X, 16, 6)
    d, r = ix.search(q, k=10)
    sentinel = np.float32(np.inf if metric == "L2" else -np.inf)
    if name == "all":
        assert len(ix) == 0 and st["shadows_dropped"] == 3 and st["shadows_kept"] == 0
        assert (r == -1).all() and (d == sentinel).all()
        ix.add(X[:700])  # rows can be added again
        Xs = X[:700]
    else:
        assert len(ix) == 1 and st["shadows_dropped"] == 0 and st["shadows_kept"] == 3
        Xs = X[n // 2: n // 2 + 1]
        wd, wr = orc.search(Xs, q, 1, metric)
        assert np.array_equal(r[:, :1], wr) and np.array_equal(bits(d[:, :1]), bits(wd))
        assert (r[:, 1:] == -1).all() and (d[:, 1:] == sentinel).all()
        assert np.array_equal(bits(ix.get_rows(0, 1)), bits(Xs))
        ix.add(X[:700])
        Xs = np.vstack([Xs, X[:700]])
    d, r = ix.search(q, k=10)
    wd, wr = orc.search(Xs, q, 10, metric)
    assert np.array_equal(r, wr) and np.array_equal(bits(d), bits(wd))
    ix.close()


@pytest.mark.parametrize("name", ["random30", "first"])
def test_chunked_path(rt, name):
    """9 chunks over 70 001 rows.  `first` is the hazard case: every row moves by one, so each chunk's destinations overlap its
    own sources and go through the bounce buffer; `random30` starts that way and turns to direct moves once the shift exceeds a chunk."""
    n, dim, metric = 70_001, 64, "L2"
    X = corpus(n, dim, seed=21)
    plan = (("exact", 16, 10), ("batched8", 200, 10), ("batched16", 16, 1))
    ix = _native.Index(rt, dim, metric=metric, kind="FLAT")
    ix.add(X)
    for path, Q, k in plan:
        flat_search(ix, path, queries(X, Q, 5), k)
    dele = delete_set(name, n, seed=8)
    _native.diag_set_option("delete_chunk_rows", 8192)
    try:
        assert (n - int(dele.min()) + 8191) // 8192 >= 5
        ix.delete_rows(dele)
    finally:
        _native.diag_set_option("delete_chunk_rows", 0)
    Xs = np.delete(X, dele, axis=0)
    st = ix.last_delete_stats()
    assert st["shadows_kept"] == 3 and st["shadows_dropped"] == 0 and st["rows_moved"] == (n - int(dele.min())) - len(dele)
    assert np.array_equal(bits(ix.get_rows(0, len(Xs))), bits(Xs))
    check_flat(ix, Xs, metric, plan, seed=13)
    ix.close()


def test_validation_is_atomic(rt):
    n, dim = 5_000, 64
    X = corpus(n, dim, seed=2)
    ix = _native.Index(rt, dim, metric="L2", kind="FLAT")
    ix.add(X)
    q = queries(X, 16, 1)
    before = [flat_search(ix, p, q, 10) for p in FLAT_PATHS]
    for bad in ([n], [-1], [5, 9, 5], [0, n - 1, n]):
        with pytest.raises(_native.ScError) as e:
            ix.delete_rows(bad)
        assert e.value.status == -1, e.value  # SC_ERR_INVALID
        assert len(ix) == n
    assert _native.lib().sc_index_delete_rows(ix.handle, None, 3) == -1 and len(ix) == n
    ix.delete_rows([])  # n == 0: SC_OK, nothing happens
    assert len(ix) == n
    after = [flat_search(ix, p, q, 10) for p in FLAT_PATHS]
    for (d0, r0), (d1, r1) in zip(before, after):
        assert np.array_equal(r0, r1) and np.array_equal(bits(d0), bits(d1))
    assert np.array_equal(bits(ix.get_rows(0, n)), bits(X))
    ix.close()


# ------------------------------------------------------------------ IVF_FLAT

IVF_MODES = (("ivf", 5), ("ivf_listmajor", 70), ("ivf_coarse", 70))  # forced mode, queries


def clustered(n, dim, seed, centers=40):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centers, dim)).astype(np.float32) * 2
    return (c[rng.integers(0, centers, size=n)] + 0.4 * rng.standard_normal((n, dim))).astype(np.float32)


def ivf_compare(ix, twin, X, k, nprobe, seed, oracle=None):
    """every forced probe mode, then the exhaustive modes over the list-major layout: same bits as the twin, the named path on
    both; where the twin refuses a shape, so may the index.  Returns the modes that were compared."""
    compared = []
    for mode, Q in IVF_MODES + (("exact", 16), ("batched", 70)):
        q = queries(X, Q, seed + Q)
        twin.set_search_mode(mode)
        ix.set_search_mode(mode)
        try:
            wd, wr = twin.search(q, k=k, nprobe=nprobe)
        except _native.ScError:
            continue
        d, r = ix.search(q, k=k, nprobe=nprobe)
        assert twin.last_search_stats()["path"] == mode and ix.last_search_stats()["path"] == mode, (mode, ix.last_search_stats())
        assert np.array_equal(r, wr) and np.array_equal(bits(d), bits(wd)), mode
        if oracle is not None and mode.startswith("ivf"):
            od, orow = oracle.search(q, k, nprobe)
            assert np.array_equal(r, orow) and np.array_equal(bits(d), bits(od)), mode
        if mode in ("exact", "batched"):
            od, orow = orc.search(X, q, k, ix.metric)
            assert np.array_equal(r, orow) and np.array_equal(bits(d), bits(od)), mode
        compared.append(mode)
    for x in (ix, twin):
        x.set_search_mode("auto")
    return compared


def oracle_for(Xs, metric, cent, assign):
    o = object.__new__(IvfOracle)
    o.X, o.metric, o.nlist, o.centroids, o.assign = np.ascontiguousarray(Xs), metric, len(cent), cent, assign
    o.lists = [np.nonzero(assign == c)[0] for c in range(len(cent))]
    return o


IVF_CASES = [  # every variant, both nlist, every metric
    ("plain", 16, 64, "L2"), ("plain", 64, 200, "IP"), ("tail", 64, 64, "L2"), ("dirty", 16, 200, "COSINE"), ("mixed", 16, 64, "L2"),
    ("mixed", 64, 64, "IP"), ("empty_list", 16, 64, "L2"), ("empty_list", 64, 64, "COSINE"),
]


@pytest.mark.parametrize("variant,nlist,dim,metric", IVF_CASES)
def test_ivf_delete_matches_rebuilt_twin(rt, nlist, dim, metric, variant):
    n, k, nprobe = 30_000, 10, 4
    X = clustered(n, dim, seed=nlist + dim)
    rng = np.random.default_rng(17)
    ix = _native.Index(rt, dim, metric=metric, kind="IVF_FLAT", nlist=nlist)
    ix.add(X)
    ix.train(niter=3)
    info = ix.ivf_info()
    cent, assign = info["centroids"].copy(), ix.ivf_assignments().copy()
    for mode, Q in IVF_MODES + (("batched", 70),):  # every probe path once: the centred shadow exists at the delete -- and a coarse
        ix.set_search_mode(mode)                     # shadow of the exhaustive path, indexed by stored position like it
        ix.search(queries(X, Q, 5), k=k, nprobe=nprobe)
        assert ix.last_search_stats()["path"] == mode
    ix.set_search_mode("auto")

    tail = clustered(500, dim, seed=99) if variant in ("tail", "mixed") else np.zeros((0, dim), np.float32)
    dirty_rows = np.sort(rng.permutation(n)[:60]) if variant in ("dirty", "mixed") else np.zeros(0, np.int64)
    dirty_vecs = clustered(len(dirty_rows), dim, seed=98)
    if len(tail):
        ix.add(tail)
    if len(dirty_rows):
        ix.overwrite(dirty_vecs, dirty_rows)
    total = n + len(tail)
    if variant == "empty_list":
        big = int(np.argmax(np.bincount(assign, minlength=nlist)))
        dele = np.nonzero(assign == big)[0]
    else:
        dele = rng.permutation(n)[: (3 * n) // 10]
        if len(tail):
            dele = np.concatenate([dele, n + rng.permutation(len(tail))[:150]])
        if len(dirty_rows):
            dele = np.unique(np.concatenate([dele, dirty_rows[::3]]))
    dele = rng.permutation(dele)
    ix.delete_rows(dele)
    st = ix.last_delete_stats()
    print(variant, nlist, dim, metric, st)
    assert st["shadows_dropped"] == 0 and (st["shadows_kept"] & 4) and (st["shadows_kept"] & 3), st  # valid shadows stay
    keep = np.ones(total, bool)
    keep[dele] = False
    assert len(ix) == int(keep.sum())

    # the twin: the same operations over the survivors alone
    Xall = np.vstack([X, tail])
    Xnow = Xall.copy()
    Xnow[dirty_rows] = dirty_vecs
    newid = np.cumsum(keep) - 1
    twin = _native.Index(rt, dim, metric=metric, kind="IVF_FLAT", nlist=nlist)
    twin.add(X[keep[:n]])
    twin.set_ivf(cent, assign[keep[:n]])
    if len(tail):
        twin.add(tail[keep[n:]])
    kept_dirty = keep[dirty_rows] if len(dirty_rows) else np.zeros(0, bool)
    if kept_dirty.any():
        twin.overwrite(dirty_vecs[kept_dirty], newid[dirty_rows[kept_dirty]])
    Xs = Xnow[keep]
    assert np.array_equal(bits(ix.get_rows(0, len(Xs))), bits(Xs))
    modes = ivf_compare(ix, twin, Xs, k, nprobe, seed=23, oracle=oracle_for(Xs, metric, cent, assign[keep]) if variant in ("plain", "empty_list") else None)
    assert modes == ["ivf", "ivf_listmajor", "ivf_coarse", "exact", "batched"], modes  # (these shapes: no path refuses)
    # lists: every survivor kept its list (rows upserted meanwhile are assigned to the same centroids by both), centroid bits unchanged
    a_ix, a_tw = ix.ivf_assignments(), twin.ivf_assignments()
    assert np.array_equal(a_ix, a_tw)
    clean = keep[:n].copy()
    clean[dirty_rows] = False
    assert np.array_equal(a_ix[newid[np.nonzero(clean)[0]]], assign[clean])
    if len(tail):
        want = _nearest(cent, tail[keep[n:]], _assign_metric(metric))
        assert np.array_equal(a_ix[newid[n:][keep[n:]]], want)
    i2, t2 = ix.ivf_info(), twin.ivf_info()
    assert i2["nlist"] == nlist and np.array_equal(bits(i2["centroids"]), bits(cent))
    assert i2["list_sizes"].tolist() == np.bincount(a_ix, minlength=nlist).tolist() == t2["list_sizes"].tolist()
    if variant == "empty_list":
        assert i2["list_sizes"][big] == 0
    ivf_compare(ix, twin, Xs, k, nprobe, seed=29, oracle=oracle_for(Xs, metric, cent, a_ix))  # after the refresh: lists only
    ix.close()
    twin.close()


def test_ivf_delete_every_listed_row_keeps_the_tail(rt):
    """every row of the lists goes, rows appended since stay: empty lists + a tail, answered exactly; the lists take the tail in later"""
    X, tail = clustered(6_000, 64, seed=1), clustered(300, 64, seed=2)
    ix = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=16)
    ix.add(X)
    ix.train(niter=2)
    cent = ix.ivf_info()["centroids"].copy()
    ix.set_search_mode("ivf_coarse")
    ix.search(queries(X, 70, 3), k=5, nprobe=4)
    ix.set_search_mode("auto")
    ix.add(tail)
    ix.delete_rows(np.concatenate([np.arange(6_000), [6_000 + 17]]))
    Xs = np.delete(tail, 17, axis=0)
    assert len(ix) == 299 and ix.last_delete_stats()["shadows_dropped"] == 0
    assert np.array_equal(bits(ix.get_rows(0, 299)), bits(Xs))
    # the probe modes leave the tail a tail: every list is empty and the whole tail is scanned, so the answer is the exact one;
    # the exhaustive mode comes last (it folds the tail into the lists first)
    for mode, Q in (("ivf", 5), ("ivf_listmajor", 70), ("ivf_coarse", 70), ("auto", 1), ("exact", 16)):
        ix.set_search_mode(mode)
        q = queries(Xs, Q, 7)
        d, r = ix.search(q, k=5, nprobe=4)
        wd, wr = orc.search(Xs, q, 5, "L2")
        assert np.array_equal(r, wr) and np.array_equal(bits(d), bits(wd)), mode
        if mode != "exact":
            assert ix.last_search_stats().get("tail_rows") == 299, (mode, ix.last_search_stats())
    ix.set_search_mode("auto")
    assert np.array_equal(ix.ivf_assignments(), _nearest(cent, Xs, _assign_metric("L2")))
    info = ix.ivf_info()
    assert info["nlist"] == 16 and np.array_equal(bits(info["centroids"]), bits(cent)) and int(info["list_sizes"].sum()) == 299
    ix.close()


def test_ivf_delete_all(rt):
    X = clustered(8_000, 64, seed=1)
    ix = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=16)
    ix.add(X)
    ix.train(niter=2)
    ix.search(X[:5], k=5, nprobe=4)
    ix.delete_rows(np.arange(len(X)))
    assert len(ix) == 0 and ix.ivf_info()["nlist"] == 0  # the lists are dropped
    d, r = ix.search(X[:5], k=5, nprobe=4)
    assert (r == -1).all() and np.isinf(d).all()
    ix.add(X[:3000])
    d, r = ix.search(X[:5], k=5, nprobe=4)
    wd, wr = orc.search(X[:3000], X[:5], 5, "L2")
    assert np.array_equal(r, wr) and np.array_equal(bits(d), bits(wd))
    ix.close()


# ------------------------------------------------------------------ the store: random collection operations with deletes

DIM = 64


class Model:
    """Host model of the collection: primary key -> row, columns, f32 matrix; a delete renumbers as the store does."""

    def __init__(self):
        self.ids, self.texts, self.paths, self.X, self.deleted = [], [], [], np.zeros((0, DIM), np.float32), set()

    @property
    def row_of(self):
        return {pk: r for r, pk in enumerate(self.ids)}

    def upsert(self, payloads):
        row_of = self.row_of
        new = []
        for p in payloads:
            v = np.asarray(p.vector, np.float32)
            self.deleted.discard(p.id)
            if p.id in row_of:
                r = row_of[p.id]
                if r < len(self.X):
                    self.X[r] = v
                else:
                    new[r - len(self.X)] = v
                self.texts[r], self.paths[r] = p.text, p.metadata["path"]
            else:
                row_of[p.id] = len(self.ids)
                self.ids.append(p.id)
                self.texts.append(p.text)
                self.paths.append(p.metadata["path"])
                new.append(v)
        if new:
            self.X = np.vstack([self.X, np.asarray(new, np.float32)])

    def delete_rows(self, rows):
        self.deleted.update(self.ids[r] for r in rows)
        keep = np.ones(len(self.ids), bool)
        keep[list(rows)] = False
        self.X = self.X[keep]
        for name in ("ids", "texts", "paths"):
            setattr(self, name, [v for v, kp in zip(getattr(self, name), keep) if kp])
        return len(rows)


def payload(rng, key, gen):
    v = rng.standard_normal(DIM).astype(np.float32)
    return EmbeddingPayload(id=key, text=f"{key}@{gen}", vector=v.tolist(),
                            metadata={"repo": "r", "path": f"src/f{int(key[1:]) % 37}.py", "language": "py", "start_line": 1, "end_line": 2,
                                      "symbol": None})


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("index_type", ["FLAT", "IVF_FLAT"])
def test_random_collection_operations_with_deletes(rt, tmp_path, metric, index_type):
    rng = np.random.default_rng({"L2": 1, "IP": 2, "COSINE": 3}[metric] * 100 + len(index_type))

    def open_store():
        s = MilvusVectorStore(dim=DIM, metric=metric, index_type=index_type, nlist=16, nprobe=4, runtime=rt)
        s.connect()
        return s

    store, model = open_store(), Model()
    next_key = searches = deletes = 0
    after_delete = False
    for step in range(110):
        op = str(rng.choice(["new", "new", "mixed", "known", "search", "search", "build", "saveload", "delete", "delete", "delete_where"]))
        if after_delete and op not in ("search", "saveload"):
            op = "saveload" if rng.random() < 0.3 else "search"  # what follows a delete looks at it
        after_delete = False
        if not model.ids:
            op = "new"
        if op in ("new", "known", "mixed"):
            if op == "new":
                n = int(rng.choice([1, 5, 130, 700, 3000])) if model.ids else 700
                batch = [payload(rng, f"k{next_key + i}", step) for i in range(n)]
                next_key += n
            elif op == "known":
                batch = [payload(rng, model.ids[int(j)], step) for j in rng.integers(0, len(model.ids), size=int(rng.choice([1, 40])))]
            else:
                batch = [payload(rng, model.ids[int(j)], step) for j in rng.integers(0, len(model.ids), size=20)]
                batch += [payload(rng, f"k{next_key + i}", step) for i in range(30)]
                next_key += 30
                batch = [batch[int(j)] for j in rng.permutation(len(batch))]
            store.upsert_embeddings(batch)
            model.upsert(batch)
            assert len(store) == len(model.ids)
            continue
        if op == "build":
            store.build_index(niter=3)
            continue
        if op == "saveload":
            store.save(tmp_path / f"c{step}")
            store.close()
            store = open_store()
            store.load(tmp_path / f"c{step}")
            assert len(store) == len(model.ids) and store._ids == model.ids
            continue
        if op == "delete":
            m = int(rng.choice([1, 3, 50, max(1, len(model.ids) // 3)]))
            keys = [model.ids[int(j)] for j in rng.integers(0, len(model.ids), size=m)]  # (may repeat)
            keys += [f"unknown{step}", f"k{next_key + 5}"] + list(model.deleted)[:2]  # never stored / deleted before
            want = model.delete_rows(sorted({model.row_of[pk] for pk in keys if pk in model.row_of}))
            assert store.delete(keys) == want
        if op == "delete_where":
            path = model.paths[int(rng.integers(0, len(model.ids)))]
            want = model.delete_rows([r for r, p in enumerate(model.paths) if p == path])
            assert want >= 1 and store.delete_where(path=path) == want
            assert store.delete_where(path=path, repo="r") == 0
        if op in ("delete", "delete_where"):
            deletes += 1
            after_delete = True
            assert len(store) == len(model.ids) and store._ids == model.ids and store._texts == model.texts
            assert store._row_of == model.row_of
            continue
        # search
        searches += 1
        n = len(model.ids)
        Q = int(rng.choice([1, 3, 20, 70, 300]))
        k = int(rng.choice([1, 5, 10, 70]))
        own = rng.integers(0, n, size=max(1, Q // 2))
        q = rng.standard_normal((Q, DIM)).astype(np.float32)
        q[: len(own)] = model.X[own]
        dist, rows = store.search_batch(q, top_k=k)
        kk = min(k, n)
        want_d, want_r = orc.search(model.X, q, kk, metric)
        if index_type == "FLAT":
            assert np.array_equal(rows[:, :kk], want_r) and np.array_equal(bits(dist[:, :kk]), bits(want_d)), (step, n, Q, k)
        else:
            for j in range(Q):
                got = rows[j][rows[j] >= 0]
                assert len(set(got.tolist())) == len(got) and len(got) >= 1 and got.max() < n
                d1, r1 = orc.search_rows(model.X, q[j], got, len(got), metric)
                assert np.array_equal(r1, got) and np.array_equal(bits(d1), bits(dist[j][: len(got)])), (step, j)
            if metric != "IP":  # a stored row finds itself
                for j in range(len(own)):
                    assert np.array_equal(model.X[rows[j, 0]], model.X[own[j]]), (step, j)
        hits = next(iter(store.search(q[0].tolist(), top_k=k)))
        d0, r0 = store.search_batch(q[:1], top_k=k)
        assert [h.id for h in hits] == [model.ids[int(r)] for r in r0[0] if r >= 0]
        assert [h.entity.get("text") for h in hits] == [model.texts[int(r)] for r in r0[0] if r >= 0]
        assert not (set(h.id for h in hits) & model.deleted)  # no deleted key is ever returned
        assert not (set(store._ids[int(r)] for r in rows.ravel() if r >= 0) & model.deleted)
    assert searches >= 5 and deletes >= 5
    store.close()


def test_store_save_load_after_delete(rt, tmp_path):
    rng = np.random.default_rng(5)
    store = MilvusVectorStore(dim=DIM, metric="L2", index_type="IVF_FLAT", nlist=16, nprobe=4, runtime=rt)
    store.connect()
    batch = [payload(rng, f"k{i}", 0) for i in range(3000)]
    store.upsert_embeddings(batch)
    store.build_index(niter=3)
    q = rng.standard_normal((20, DIM)).astype(np.float32)
    store.search_batch(q, top_k=5)
    assert store.delete([f"k{i}" for i in range(0, 3000, 3)]) == 1000
    d0, r0 = store.search_batch(q, top_k=5)
    store.save(tmp_path / "c")
    other = MilvusVectorStore(dim=DIM, metric="L2", index_type="IVF_FLAT", nlist=16, nprobe=4, runtime=rt)
    other.connect()
    other.load(tmp_path / "c")
    assert len(other) == 2000 and other._ids == store._ids and not other._needs_train  # the lists travel: no k-means
    d1, r1 = other.search_batch(q, top_k=5)
    assert np.array_equal(r0, r1) and np.array_equal(bits(d0), bits(d1))
    store.close()
    other.close()


# ------------------------------------------------------------------ ingest with prune, through the device seams

SMALL = dict(vocab=2000, hidden=128, layers=2, heads=2, ffn=256, max_pos=128)


def test_ingest_prune_on_device(monkeypatch):
    """Re-index with shifted line numbers: every chunk gets a new primary key.  prune=False keeps both generations (today's
    behaviour, the reference's); prune=True leaves exactly the second one, and the other repository alone."""
    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from semcode_amd.services import ingest_chunks
    from semcode_amd.settings import settings

    monkeypatch.setattr(settings, "mi355x_ingest_batch", 64, raising=False)
    emb = MI355XEmbeddings(cfg=SMALL, synth_seed=3, allow_synthetic=True)
    root = Path("/w/demo")
    texts = [("def f%d(x):\n    return x + %d  # helper number %d " % (i, i, i)) * (1 + i % 5) for i in range(150)]

    def generation(shift, count=150):
        return [SimpleNamespace(content=texts[i], path=root / "src" / f"m{i % 40}.py", language="python", start_line=10 * i + 1 + shift,
                                end_line=10 * i + 9 + shift, symbol=None) for i in range(count)]

    gen1, gen2 = generation(0), generation(2, count=140)  # (ten chunks vanished as well)
    other = [SimpleNamespace(content="x = %d" % i, path=Path("/w/lib") / f"a{i}.py", language="python", start_line=1, end_line=2, symbol=None) for i in range(30)]
    stores = {}
    for prune in (False, True):
        st = MilvusVectorStore(dim=128, metric="COSINE", index_type="FLAT")
        st.connect()
        assert ingest_chunks("demo", root, gen1, emb, st) == 150
        assert ingest_chunks("lib", Path("/w/lib"), other, emb, st) == 30
        assert ingest_chunks("demo", root, gen2, emb, st, prune=prune) == 140
        stores[prune] = st
    keep, pruned = stores[False], stores[True]
    assert len(keep) == 150 + 30 + 140  # both generations searchable: pinned
    assert len(pruned) == 30 + 140
    from semcode_amd.services.indexer import make_chunk_id
    want = {make_chunk_id("demo", c.path, c.start_line, c.end_line) for c in gen2} | {make_chunk_id("lib", c.path, c.start_line, c.end_line) for c in other}
    assert set(pruned._ids) == want and pruned._repos.count("lib") == 30
    # the vectors moved with their rows: each stored row is the embedding of its text, and finds itself
    vec = emb.embed_documents_array([pruned._texts[r] for r in range(60)])
    assert np.array_equal(pruned._collection.get_rows(0, 60), vec)
    q = emb.embed_documents_array(texts[:20])
    d, r = pruned.search_batch(q, top_k=3)
    for j in range(20):
        assert pruned._texts[int(r[j, 0])] == texts[j] and pruned._metadata[int(r[j, 0])]["start_line"] == 10 * j + 3
    for st in stores.values():
        st.close()
