"""GPU: the MMR search (sc_index_search_mmr*: the inverse position map, mmr_gram_kernel and mmr_select_kernel behind the exact
candidate searches) against the reference of tests/mmr_ref.py.

Bar: ids compared with np.array_equal, distances by their uint32 view, for the definition in include/semcode_hip.h: candidates and
the candidate x candidate matrix from the CPU oracle in the canonical summation order, the selection in numpy float32 one rounded
operation at a time.  The shapes are the smallest that reach every branch: 3 001 rows (a ragged 16-row tile and a ragged bitset
word), fetch_k 20 and 33 (ragged matrix tiles), 128 (the limit), 17 queries (two chunks of the forced query chunk).  The candidates
and their matrix are computed once per (corpus, metric, fetch_k, mask) and shared by every k and lambda.
"""
import ctypes as C

import numpy as np
import pytest

import mmr_ref
from oracle import sc_oracle as orc
from semcode_amd import _native
from semcode_amd.storage import MilvusVectorStore

pytestmark = pytest.mark.gpu

METRICS = ["IP", "L2", "COSINE"]
N = 3001
NQ = 17


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, want, what=""):
    (d, r), (wd, wr) = got, want
    assert np.array_equal(r, wr), f"{what}: ids differ, first query {np.flatnonzero((r != wr).any(1))[:1]}"
    assert np.array_equal(bits(d), bits(wd)), f"{what}: distances differ"


@pytest.fixture(scope="module")
def corpora():
    """dim -> (X [N, dim], Q [17, dim], cache of mmr_ref.candidates by (metric, fetch_k))."""
    out = {}
    for dim in (64, 100):
        out[dim] = (orc.synth(N, dim, seed=301 + dim), orc.synth(NQ, dim, seed=401 + dim), {})
    return out


def cands(corpora, dim, metric, fetch_k):
    X, Q, cache = corpora[dim]
    key = (metric, fetch_k)
    if key not in cache:
        cache[key] = mmr_ref.candidates(X, Q, fetch_k, metric)
    return cache[key]


@pytest.fixture(autouse=True)
def default_chunk():
    _native.diag_set_option("mmr_chunk_q", -1)
    yield
    _native.diag_set_option("mmr_chunk_q", -1)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [64, 100])
def test_sweep(rt, corpora, metric, dim):
    X, Q, _ = corpora[dim]
    ix = _native.Index(rt, dim, metric=metric)
    ix.add(X)
    for k, fetch_k in ((1, 1), (5, 20), (10, 32), (10, 33), (128, 128)):
        c = cands(corpora, dim, metric, fetch_k)
        for lam in (0.0, 0.3, 1.0):
            want = mmr_ref.answer(c, k, lam, metric)
            for nq in (1, 3, NQ):
                got = ix.search_mmr(Q[:nq], k=k, fetch_k=fetch_k, lam=lam)
                assert ix.last_search_stats()["path"] == "mmr"
                check(got, (want[0][:nq], want[1][:nq]), f"k={k} fetch_k={fetch_k} lambda={lam} Q={nq}")
                if lam == 1.0:
                    check(got, ix.search(Q[:nq], k=k), f"lambda=1 against the plain search, k={k} fetch_k={fetch_k} Q={nq}")
    # the redundancy term decides: at lambda = 0.5, fetch_k = 32 no query keeps the plain prefix
    want = mmr_ref.answer(cands(corpora, dim, metric, 32), 10, 0.5, metric)
    plain = ix.search(Q, k=10)[1]
    assert all(not np.array_equal(want[1][i], plain[i]) for i in range(NQ))
    got = ix.search_mmr(Q, k=10, fetch_k=32, lam=0.5)
    check(got, want, "lambda=0.5")
    # fetch_k = k: a permutation of the plain top-k; k = 1: the best hit
    d, r = ix.search_mmr(Q, k=10, fetch_k=10, lam=0.2)
    assert np.array_equal(np.sort(r, axis=1), np.sort(plain, axis=1))
    d, r = ix.search_mmr(Q, k=1, fetch_k=40, lam=0.0)
    assert np.array_equal(r[:, 0], plain[:, 0])
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_masks(rt, corpora, metric):
    dim = 100
    X, Q, _ = corpora[dim]
    ix = _native.Index(rt, dim, metric=metric)
    ix.add(X)
    rng = np.random.default_rng(31)
    pad = np.inf if metric == "L2" else -np.inf
    allowed = rng.random(N) < 0.3
    check(ix.search_mmr(Q, k=10, fetch_k=32, lam=0.5, allow=allowed), mmr_ref.reference_batch(X, Q, 10, 32, 0.5, metric, allowed), "30 % allowed")
    st = ix.last_mmr_stats()
    assert st == {"fetch_k": 32, "min_candidates": 32, "rows_scanned": int(allowed.sum())} and ix.last_search_stats()["path"] == "mmr"
    seven = np.zeros(N, bool)
    seven[rng.choice(N - 1, 6, replace=False)] = True
    seven[N - 1] = True  # (the last bit of the ragged word)
    assert seven.sum() == 7
    d, r = ix.search_mmr(Q, k=10, fetch_k=20, lam=0.3, allow=seven)
    check((d, r), mmr_ref.reference_batch(X, Q, 10, 20, 0.3, metric, seven), "7 rows allowed")
    assert (r[:, :7] >= 0).all() and (r[:, 7:] == -1).all() and (d[:, 7:] == pad).all()
    assert ix.last_mmr_stats()["min_candidates"] == 7
    d, r = ix.search_mmr(Q, k=10, fetch_k=20, lam=0.3, allow=np.zeros(N, bool))
    assert (r == -1).all() and (d == pad).all()
    assert ix.last_mmr_stats() == {"fetch_k": 20, "min_candidates": 0, "rows_scanned": 0}  # no scan
    check(ix.search_mmr(Q, k=10, fetch_k=32, lam=0.3, allow=np.ones(N, bool)), mmr_ref.answer(cands(corpora, dim, metric, 32), 10, 0.3, metric), "every row allowed")
    assert ix.last_mmr_stats()["rows_scanned"] == N
    ix.close()
    empty = _native.Index(rt, dim, metric=metric)
    for allow in (None, np.zeros(0, bool)):
        d, r = empty.search_mmr(Q[:3], k=5, fetch_k=20, lam=0.5, allow=allow)
        assert (r == -1).all() and (d == pad).all()
        assert empty.last_mmr_stats() == {"fetch_k": 20, "min_candidates": 0, "rows_scanned": 0}
    empty.close()


def ivf_state(ix):
    info = ix.ivf_info()
    return info["nlist"], info["list_sizes"].tolist(), bits(info["centroids"]).tobytes()


@pytest.mark.parametrize("metric", METRICS)
def test_trained_ivf_is_searched_as_it_lies(rt, metric):
    """A trained IVF_FLAT index with a tail of appended rows and rows overwritten in place: the candidates are row ids, the rows
    lie list-major, so this is the test of the inverse position map.  A twin that never runs an MMR search tells whether anything
    about later searches changed."""
    dim = 64
    X = orc.synth(N, dim, seed=311)
    Q = orc.synth(NQ, dim, seed=312)
    rng = np.random.default_rng(32)
    new = orc.synth(203, dim, seed=313)
    rows = rng.choice(N, 150, replace=False)
    over = orc.synth(150, dim, seed=314)
    ix, twin = (_native.Index(rt, dim, metric=metric, kind="IVF_FLAT", nlist=16) for _ in range(2))
    for i in (ix, twin):
        i.add(X)
        i.train(niter=4, seed=3)
        i.add(new)
        i.overwrite(over, rows)
    X = np.concatenate([X, new])
    X[rows] = over
    allowed = rng.random(len(X)) < 0.3
    allowed[-5:] = True  # (tail rows among the allowed)
    # masked first: the position map does not cover the tail yet
    check(ix.search_mmr(Q, k=10, fetch_k=33, lam=0.3, allow=allowed), mmr_ref.reference_batch(X, Q, 10, 33, 0.3, metric, allowed), "trained, masked")
    c = mmr_ref.candidates(X, Q, 33, metric)
    check(ix.search_mmr(Q, k=10, fetch_k=33, lam=0.3), mmr_ref.answer(c, 10, 0.3, metric), "trained, unmasked")
    check(ix.search_mmr(Q, k=33, fetch_k=33, lam=0.0), mmr_ref.answer(c, 33, 0.0, metric), "trained, unmasked, lambda=0")
    check(ix.search_mmr(Q, k=10, fetch_k=33, lam=0.3, allow=allowed), mmr_ref.reference_batch(X, Q, 10, 33, 0.3, metric, allowed), "trained, masked again")
    for nprobe in (4, 16):
        check(ix.search(Q, k=10, nprobe=nprobe), twin.search(Q, k=10, nprobe=nprobe), f"plain search afterwards, nprobe={nprobe}")
    for i in (ix, twin):
        i.set_search_mode("exact")
    check(ix.search(Q, k=10), orc.search(X, Q, 10, metric), "exact search afterwards")
    check(ix.search(Q, k=10), twin.search(Q, k=10), "exact search afterwards against the twin")
    state = ivf_state(ix)
    assert state == ivf_state(twin) and state[0] == 16 and sum(state[1]) == len(X)
    # ... and once the lists have taken the tail in
    check(ix.search_mmr(Q, k=10, fetch_k=33, lam=0.3), mmr_ref.answer(c, 10, 0.3, metric), "trained, after the refresh")
    ix.close()
    twin.close()


def test_row_base_and_device_pointers(rt, corpora):
    import torch

    dim, metric, base, nq, k, fk, lam = 100, "L2", 500, 5, 10, 33, 0.3
    X, Q, _ = corpora[dim]
    ix = _native.Index(rt, dim, metric=metric, row_base=base)
    ix.add(X)
    want = mmr_ref.answer(cands(corpora, dim, metric, fk), k, lam, metric, row_base=base)
    want = (want[0][:nq], want[1][:nq])
    got = ix.search_mmr(Q[:nq], k=k, fetch_k=fk, lam=lam)
    check(got, want, "row_base")
    assert got[1].min() >= base
    q = torch.from_numpy(Q[:nq]).cuda()
    d = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    r = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.search_mmr_dev(q.data_ptr(), nq, k, fk, lam, 0, 0, d.data_ptr(), r.data_ptr())
    rt.synchronize()
    check((d.cpu().numpy(), r.cpu().numpy()), got, "device pointers")
    assert ix.last_mmr_stats() == {"fetch_k": fk, "min_candidates": fk, "rows_scanned": N}
    allowed = np.random.default_rng(33).random(N) < 0.5
    words = _native.pack_allow(allowed, N)
    w = torch.from_numpy(words.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    ix.search_mmr_dev(q.data_ptr(), nq, k, fk, lam, w.data_ptr(), words.size, d.data_ptr(), r.data_ptr())
    rt.synchronize()
    check((d.cpu().numpy(), r.cpu().numpy()), ix.search_mmr(Q[:nq], k=k, fetch_k=fk, lam=lam, allow=allowed), "device pointers, masked, against the host form")
    check((d.cpu().numpy(), r.cpu().numpy()), mmr_ref.reference_batch(X, Q[:nq], k, fk, lam, metric, allowed, row_base=base), "device pointers, masked")
    ix.close()


def test_long_rows(rt):
    n, dim, nq = 515, 3072, 2
    X = orc.synth(n, dim, seed=321)
    Q = orc.synth(nq, dim, seed=322)
    for metric in METRICS:
        ix = _native.Index(rt, dim, metric=metric)
        ix.add(X)
        check(ix.search_mmr(Q, k=10, fetch_k=33, lam=0.3), mmr_ref.reference_batch(X, Q, 10, 33, 0.3, metric), f"dim 3072, {metric}")
        ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_query_chunks(rt, corpora, metric):
    X, Q, _ = corpora[64]
    ix = _native.Index(rt, 64, metric=metric)
    ix.add(X)
    allowed = np.random.default_rng(34).random(N) < 0.4
    whole = ix.search_mmr(Q, k=10, fetch_k=32, lam=0.3), ix.search_mmr(Q, k=10, fetch_k=32, lam=0.3, allow=allowed)
    _native.diag_set_option("mmr_chunk_q", 4)
    check(ix.search_mmr(Q, k=10, fetch_k=32, lam=0.3), whole[0], "chunks of 4")
    assert ix.last_mmr_stats() == {"fetch_k": 32, "min_candidates": 32, "rows_scanned": 5 * N}
    check(ix.search_mmr(Q, k=10, fetch_k=32, lam=0.3, allow=allowed), whole[1], "chunks of 4, masked")
    check(whole[0], mmr_ref.answer(cands(corpora, 64, metric, 32), 10, 0.3, metric), "the default chunk")
    ix.close()


@pytest.mark.parametrize("metric", METRICS)
def test_duplicates_do_not_take_every_slot(rt, metric):
    """600 vectors, each stored 5 times at scattered rows: a plain top-10 holds 2 distinct sources, MMR holds 10."""
    dim = 64
    src = np.random.default_rng(7).permutation(np.repeat(np.arange(600), 5))
    X = orc.synth(600, dim, seed=77)[src]
    Q = orc.synth(NQ, dim, seed=78)
    ix = _native.Index(rt, dim, metric=metric)
    ix.add(X)
    d, r = ix.search_mmr(Q, k=10, fetch_k=64, lam=0.5)
    check((d, r), mmr_ref.reference_batch(X, Q, 10, 64, 0.5, metric), "duplicates")
    assert [len(set(src[x].tolist())) for x in r] == [10] * NQ
    assert [len(set(src[x].tolist())) for x in ix.search(Q, k=10)[1]] == [2] * NQ
    ix.close()


def test_arguments_and_state(rt, corpora):
    X, Q, _ = corpora[64]
    Q3 = Q[:3]
    ix = _native.Index(rt, 64, metric="L2")
    ix.add(X)
    before = ix.search(Q3, k=10)
    stats = ix.last_search_stats()

    def refused(match, q=Q3, **kw):
        with pytest.raises(_native.ScError, match=match) as e:
            ix.search_mmr(q, **kw)
        assert e.value.status == -1  # SC_ERR_INVALID
        assert ix.last_search_stats() == stats and len(ix) == N

    refused("top_k.*0", k=0, fetch_k=10)
    refused("11.*10", k=11, fetch_k=10)
    refused("129", k=10, fetch_k=129)
    refused("Q=0|NULL", q=np.zeros((0, 64), np.float32), k=5, fetch_k=10)
    refused("lambda.*-0.1", k=5, fetch_k=10, lam=-0.1)
    refused("lambda.*1.5", k=5, fetch_k=10, lam=1.5)
    refused("lambda.*nan", k=5, fetch_k=10, lam=float("nan"))
    refused("allow_words", k=5, fetch_k=10, allow=_native.pack_allow(np.ones(N, bool), N)[:-1])
    lib = _native.lib()
    q = np.ascontiguousarray(Q3)
    d, r = np.empty((3, 5), np.float32), np.empty((3, 5), np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args in ((None, 3, 5, 10, 0.5, None, 0, ptr(d), ptr(r)), (ptr(q), 3, 5, 10, 0.5, None, 0, None, ptr(r)), (ptr(q), 3, 5, 10, 0.5, None, 0, ptr(d), None),
                 (ptr(q), 3, 5, 10, 0.5, None, 94, ptr(d), ptr(r))):
        assert lib.sc_index_search_mmr(ix.handle, *args) == -1
        assert lib.sc_index_search_mmr_dev(ix.handle, *args) == -1
    assert lib.sc_index_search_mmr(None, ptr(q), 3, 5, 10, 0.5, None, 0, ptr(d), ptr(r)) == -1
    assert ix.last_search_stats() == stats
    # ... and the index is as usable as before
    check(ix.search(Q3, k=10), before, "plain search after the refused calls")
    got = ix.search_mmr(Q3, k=10, fetch_k=32, lam=0.3)
    want = mmr_ref.answer(cands(corpora, 64, "L2", 32), 10, 0.3, "L2")
    check(got, (want[0][:3], want[1][:3]), "after the refused calls")
    assert ix.last_search_stats()["path"] == "mmr"
    assert ix.last_mmr_stats() == {"fetch_k": 32, "min_candidates": 32, "rows_scanned": N}
    ix.release_scratch()
    check(ix.search_mmr(Q3, k=10, fetch_k=32, lam=0.3), got, "after release_scratch")
    check(ix.search(Q3, k=10), before, "plain search after the MMR searches")
    assert ix.last_search_stats()["path"] != "mmr"
    # fewer rows than fetch_k
    ix.delete_rows(np.arange(9, N))
    check(ix.search_mmr(Q3, k=10, fetch_k=32, lam=0.3), mmr_ref.reference_batch(X[:9], Q3, 10, 32, 0.3, "L2"), "nine rows")
    assert ix.last_mmr_stats() == {"fetch_k": 32, "min_candidates": 9, "rows_scanned": 9}
    ix.close()


@pytest.mark.parametrize("index_type", ["FLAT", "IVF_FLAT"])
def test_store_level(rt, index_type):
    n, dim = 3000, 64
    X = orc.synth(n, dim, seed=331)
    repos = ["a", "b", "c"]
    meta = [{"repo": repos[(i // 7) % 3], "path": f"f{i // 7}", "language": "py" if i % 2 else "go"} for i in range(n)]
    s = MilvusVectorStore(dim=dim, metric="IP", index_type=index_type, nlist=16, nprobe=8, runtime=rt)
    s.connect()
    s.upsert_arrays([f"id{i}" for i in range(n)], X, [f"t{i}" for i in range(n)], meta)
    Q = orc.synth(4, dim, seed=332)
    s.search_batch(Q, 5)  # (an IVF_FLAT collection trains on its first plain search: the MMR searches below see list-major storage)
    allowed = np.array([m["repo"] == "b" for m in meta])
    hits = next(iter(s.search(Q[0].tolist(), top_k=5, mmr=0.5, repos=["b"])))
    wd, wr = mmr_ref.reference_batch(X, Q, 5, 20, 0.5, "IP", allowed)  # fetch_k defaults to max(20, 4 top_k)
    assert [h.row for h in hits] == wr[0].tolist() and np.array_equal(bits([h.distance for h in hits]), bits(wd[0]))
    assert all(h.entity.get("repo") == "b" for h in hits) and s._collection.last_search_stats()["path"] == "mmr"
    check(s.search_batch(Q, 5, mmr=0.5, repos=["b"]), (wd, wr), "search_batch, one repo")
    both = allowed & np.array([m["language"] == "go" for m in meta])
    check(s.search_batch(Q, 8, mmr=0.25, fetch_k=33, repos="b", languages=["go"]), mmr_ref.reference_batch(X, Q, 8, 33, 0.25, "IP", both), "repo and language")
    check(s.search_batch(Q, 8, mmr=0.25, fetch_k=33), mmr_ref.reference_batch(X, Q, 8, 33, 0.25, "IP"), "no filter")
    plain = s.search_batch(Q, 5)
    assert s._collection.last_search_stats()["path"] != "mmr" and (plain[1] >= 0).all()
    s.close()
