"""GPU: IVF_FLAT build (deterministic k-means + list-major re-ordering) and probe search against the CPU
restatement (oracle/ivf_oracle.py): centroids bit-exact, identical lists, identical results; recall vs brute force."""
import numpy as np
import pytest

from oracle import sc_oracle as orc
from oracle.ivf_oracle import IvfOracle
from semcode_amd import _native

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clustered(n, d, ncl, seed, spread=0.35):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((ncl, d)).astype(np.float32)
    lab = rng.integers(0, ncl, size=n)
    return (centers[lab] + spread * rng.standard_normal((n, d))).astype(np.float32), centers


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_build_and_probe_match_oracle(rt, metric):
    X, centers = clustered(20_000, 64, 40, seed=1)
    rng = np.random.default_rng(2)
    Q = (centers[rng.integers(0, 40, size=5)] + 0.3 * rng.standard_normal((5, 64))).astype(np.float32)
    ix = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=32)
    ix.add(X)
    # before training: exhaustive scan
    d0, r0 = ix.search(Q, k=10, nprobe=4)
    od, orow = orc.search(X, Q, 10, metric)
    assert np.array_equal(r0, orow) and np.array_equal(bits(d0), bits(od)) and ix.last_search_stats()["path"] == "exact"
    ix.train(niter=6)
    ref = IvfOracle(X, metric, nlist=32, niter=6)
    info = ix.ivf_info()
    assert info["nlist"] == 32
    assert np.array_equal(bits(info["centroids"]), bits(ref.centroids)), "centroids differ from the restatement"
    assert info["list_sizes"].tolist() == [len(l) for l in ref.lists]
    assert np.array_equal(ix.get_rows(0, 20_000), X)  # row ids stay insertion-ordered although storage is list-major
    d, r = ix.search(Q, k=10, nprobe=4)
    assert ix.last_search_stats()["path"] == "ivf"
    rd, rr = ref.search(Q, 10, 4)
    assert np.array_equal(r, rr) and np.array_equal(bits(d), bits(rd))
    # more probes than lists: the batch is either probed list-major (same result as per-query probing) or, where the
    # library estimates that to be cheaper, answered exhaustively (exact result)
    Qb = (centers[rng.integers(0, 40, size=64)] + 0.3 * rng.standard_normal((64, 64))).astype(np.float32)
    d, r = ix.search(Qb, k=10, nprobe=4)
    path = ix.last_search_stats()["path"]
    assert path in ("exact", "batched", "ivf_listmajor")
    wd, wr = ref.search(Qb, 10, 4) if path == "ivf_listmajor" else orc.search(X, Qb, 10, metric)
    assert np.array_equal(r, wr) and np.array_equal(bits(d), bits(wd))
    ix.set_search_mode("ivf_listmajor")
    d, r = ix.search(Qb, k=10, nprobe=4)
    rd, rr = ref.search(Qb, 10, 4)
    assert ix.last_search_stats()["path"] == "ivf_listmajor" and np.array_equal(r, rr) and np.array_equal(bits(d), bits(rd))
    ix.set_search_mode("auto")
    # probing every list is the exhaustive scan (exact results)
    d, r = ix.search(Qb, k=10, nprobe=32)
    assert ix.last_search_stats()["path"] in ("exact", "batched")
    od, orow = orc.search(X, Qb, 10, metric)
    assert np.array_equal(r, orow) and np.array_equal(bits(d), bits(od))
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("wide", [True, False])
def test_listmajor_probe_equals_per_query_probe(rt, metric, wide, monkeypatch):
    """List-major probing (every probed list streamed once per group of queries that want it) returns bit for bit what
    per-query probing returns: ragged group sizes, lists wanted by more queries than fit one group, lists nobody wants,
    empty lists, k from 1 to 64, and the CPU restatement agrees.  `wide`: lists wanted by more than 16 queries go to the
    64-query GEMM-style kernel (k <= 48; remainders and k = 64 stay on the 16-query scan) or, with SC_IVF_WIDE=0, everything
    runs on the 16-query scan."""
    if not wide:
        monkeypatch.setenv("SC_IVF_WIDE", "0")
    X, centers = clustered(30_000, 96, 25, seed=11)  # 25 clusters on 64 lists: some lists end up tiny or empty
    rng = np.random.default_rng(12)
    ix = _native.Index(rt, 96, metric=metric, kind="IVF_FLAT", nlist=64)
    ix.add(X)
    ix.train(niter=5)
    ref = IvfOracle(X, metric, nlist=64, niter=5)
    sizes = ix.ivf_info()["list_sizes"]
    for nq, k, nprobe in ((2, 10, 1), (17, 1, 4), (200, 10, 16), (333, 64, 7), (40, 5, 63)):
        Q = (centers[rng.integers(0, 25, size=nq)] + 0.4 * rng.standard_normal((nq, 96))).astype(np.float32)
        ix.set_search_mode("ivf")
        d3, r3 = ix.search(Q, k=k, nprobe=nprobe)
        assert ix.last_search_stats()["path"] == "ivf"
        ix.set_search_mode("ivf_listmajor")
        d4, r4 = ix.search(Q, k=k, nprobe=nprobe)
        assert ix.last_search_stats()["path"] == "ivf_listmajor"
        assert np.array_equal(r3, r4) and np.array_equal(bits(d3), bits(d4)), (nq, k, nprobe, wide)
        rd, rr = ref.search(Q, k, nprobe)
        assert np.array_equal(r4, rr) and np.array_equal(bits(d4), bits(rd)), (nq, k, nprobe)
    assert int((sizes == 0).sum()) >= 0  # informational: empty lists are legal and skipped
    ix.close()


def test_listmajor_probe_with_streamed_queries(rt, monkeypatch):
    """List-major probing on the streamed-query scan variant (the default from ~1 400 dimensions up, forced here at 96 and
    taken by itself at 2 048): groups of up to 16 queries per list part, same bits as per-query probing."""
    monkeypatch.setenv("SC_IVF_WIDE", "0")  # the 16-query classes are what this test is about
    for dim, n, ncl, force in ((96, 30_000, 25, True), (2048, 12_000, 20, False)):
        X, centers = clustered(n, dim, ncl, seed=21)
        rng = np.random.default_rng(22)
        ix = _native.Index(rt, dim, metric="L2", kind="IVF_FLAT", nlist=32)
        ix.add(X)
        ix.train(niter=4)
        for nq, k, nprobe in ((3, 10, 2), (150, 10, 8), (64, 32, 31)):
            Q = (centers[rng.integers(0, ncl, size=nq)] + 0.4 * rng.standard_normal((nq, dim))).astype(np.float32)
            ix.set_search_mode("ivf")
            d3, r3 = ix.search(Q, k=k, nprobe=nprobe)
            if force:
                monkeypatch.setenv("SC_SCAN_QSTREAM", "1")
            ix.set_search_mode("ivf_listmajor")
            d4, r4 = ix.search(Q, k=k, nprobe=nprobe)
            assert ix.last_search_stats()["path"] == "ivf_listmajor"
            if force:
                monkeypatch.delenv("SC_SCAN_QSTREAM")
            assert np.array_equal(r3, r4) and np.array_equal(bits(d3), bits(d4)), (dim, nq, k, nprobe)
        ix.close()


def test_listmajor_wide_groups_long_rows(rt):
    """The 64-query groups at 2 048 dimensions (32 k-chunks per row tile, three-deep ring wrapping many times), list parts that
    are not multiples of 64 rows, groups of 17 .. 64 queries with narrow remainders next to them, k up to the kernel's 48."""
    X, centers = clustered(12_000, 2048, 20, seed=31)
    rng = np.random.default_rng(32)
    ix = _native.Index(rt, 2048, metric="L2", kind="IVF_FLAT", nlist=32)
    ix.add(X)
    ix.train(niter=4)
    for nq, k, nprobe in ((150, 10, 8), (300, 48, 4), (77, 1, 31)):
        Q = (centers[rng.integers(0, 20, size=nq)] + 0.4 * rng.standard_normal((nq, 2048))).astype(np.float32)
        ix.set_search_mode("ivf")
        d3, r3 = ix.search(Q, k=k, nprobe=nprobe)
        ix.set_search_mode("ivf_listmajor")
        d4, r4 = ix.search(Q, k=k, nprobe=nprobe)
        assert ix.last_search_stats()["path"] == "ivf_listmajor"
        assert np.array_equal(r3, r4) and np.array_equal(bits(d3), bits(d4)), (nq, k, nprobe)
    ix.close()


def test_recall_and_forced_probe_on_larger_set(rt):
    X, centers = clustered(300_000, 128, 500, seed=3)
    rng = np.random.default_rng(4)
    Q = (centers[rng.integers(0, 500, size=200)] + 0.35 * rng.standard_normal((200, 128))).astype(np.float32)
    ix = _native.Index(rt, 128, metric="L2", kind="IVF_FLAT", nlist=256)
    ix.add(X)
    ix.train(niter=8)
    ix.set_search_mode("exact")
    de, re_ = ix.search(Q, k=10)
    ix.set_search_mode("ivf")
    for nprobe, floor in ((1, 0.3), (8, 0.85), (32, 0.97)):
        d, r = ix.search(Q, k=10, nprobe=nprobe)
        assert ix.last_search_stats()["path"] == "ivf"
        recall = np.mean([len(set(a) & set(b)) / 10.0 for a, b in zip(r.tolist(), re_.tolist())])
        assert recall >= floor, (nprobe, recall)
        # whatever is returned carries exact distances, best first, and real row ids
        assert (np.diff(d, axis=1) >= 0).all()
        qi = 7
        od, _ = orc.search(X[r[qi]], Q[qi:qi + 1], 10, "L2")
        assert np.array_equal(bits(od[0]), bits(d[qi]))
    ix.close()


def test_upsert_into_trained_index_keeps_lists_without_kmeans(rt):
    """Upsert into an indexed collection (reference milvus_store.py:128) does not retrain: ~1 % new rows and some replaced rows
    are assigned to the EXISTING centroids at the next search.  Lists, stored rows and probe results then equal, bit for bit,
    a from-scratch sc_index_assign_lists of the final corpus with the same centroids."""
    for metric in ("L2", "IP", "COSINE"):
        X, centers = clustered(30_000, 64, 40, seed=5)
        rng = np.random.default_rng(6)
        ix = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=32)
        try:
            ix.add(X)
            ix.train(niter=6)
            cent = ix.ivf_info()["centroids"]
            new = (centers[rng.integers(0, 40, size=300)] + 0.35 * rng.standard_normal((300, 64))).astype(np.float32)
            rep_rows = rng.choice(30_000, size=60, replace=False).astype(np.int64)
            rep = (centers[rng.integers(0, 40, size=60)] + 0.35 * rng.standard_normal((60, 64))).astype(np.float32)  # most change lists
            ix.add(new[:100])
            ix.overwrite(rep[:30], rep_rows[:30])
            # one upsert batch mixing replaced rows and appended rows
            ix.put_rows(np.concatenate([rep[30:], new[100:]]), np.concatenate([rep_rows[30:], np.arange(30_100, 30_300)]))
            X2 = np.concatenate([X, new])
            X2[rep_rows] = rep
            assert len(ix) == 30_300 and np.array_equal(ix.get_rows(0, 30_300), X2)  # readable before any search folds them in
            info = ix.ivf_info()
            assert info["nlist"] == 32 and np.array_equal(bits(info["centroids"]), bits(cent)), "centroids moved: k-means ran"
            ref = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=32)
            try:
                ref.add(X2)
                ref.assign_lists(cent)
                assert np.array_equal(ix.ivf_assignments(), ref.ivf_assignments())
                assert np.array_equal(info["list_sizes"], ref.ivf_info()["list_sizes"]) and int(info["list_sizes"].sum()) == 30_300
                assert np.array_equal(ix.get_rows(0, 30_300), X2)
                Q = (centers[rng.integers(0, 40, size=70)] + 0.3 * rng.standard_normal((70, 64))).astype(np.float32)
                for mode, nq in (("ivf", 5), ("ivf_listmajor", 70)):
                    ix.set_search_mode(mode)
                    ref.set_search_mode(mode)
                    d, r = ix.search(Q[:nq], k=10, nprobe=4)
                    rd, rr = ref.search(Q[:nq], k=10, nprobe=4)
                    assert ix.last_search_stats()["path"] == mode
                    assert np.array_equal(r, rr) and np.array_equal(bits(d), bits(rd)), (metric, mode)
                ix.set_search_mode("exact")
                d, r = ix.search(Q[:4], k=10)
                od, orow = orc.search(X2, Q[:4], 10, metric)
                assert np.array_equal(r, orow) and np.array_equal(bits(d), bits(od))
                # a replaced row that stays in its list moves nothing; an explicit train() still re-runs k-means
                ix.set_search_mode("auto")
                ix.overwrite(X2[7:8] * np.float32(1.0001), np.array([7]))
                assert ix.ivf_info()["nlist"] == 32
                ix.train(niter=3)
                assert not np.array_equal(bits(ix.ivf_info()["centroids"]), bits(cent))
            finally:
                ref.close()
        finally:
            ix.close()


def test_config5_full_size_ivf_flat_10m_x_3072(rt):
    """BASELINE configs[4] at full size: IVF_FLAT nlist 4096 / nprobe 64 over 10M x 3072 (text-embedding-3-large dim), batch 1024,
    k 10 -- the index parameters of reference milvus_store.py:76-83,141-147 at the benchmark's scale.  Size-independent
    properties: the lists hold every row once; list-major probing == per-query probing bit for bit; every returned distance
    is the canonical f32 score of the regenerated row; results are sorted with the tie rule; recall@10 against the exhaustive
    (certified-exact) search of the same index."""
    N, D, NLIST, NPROBE, NQ, K = 10_000_000, 3072, 4096, 64, 1024, 10
    free = rt.device_info()["hbm_bytes"]
    if free < 270 * 2**30:
        pytest.skip("needs the 288 GB of an MI355X")
    ix = _native.Index(rt, D, metric="L2", kind="IVF_FLAT", nlist=NLIST)
    try:
        ix.fill_synthetic_clustered(N, seed=0, nclusters=NLIST, spread=0.5)
        qsrc = _native.Index(rt, D, metric="L2")
        qsrc.fill_synthetic_clustered(NQ, seed=0, nclusters=NLIST, spread=0.5, first_row=N + 12345)  # same distribution, not in the corpus
        Q = qsrc.get_rows(0, NQ)
        qsrc.close()
        assert np.array_equal(bits(Q[:3]), bits(orc.synth_clustered(3, D, 0, NLIST, 0.5, first_row=N + 12345)))
        d_bf, r_bf = ix.search(Q, k=K, nprobe=NLIST)  # untrained: exhaustive, certified exact
        assert ix.last_search_stats()["path"] in ("batched", "exact")
        ix.release_scratch()  # the bf16 shadow (61 GB) makes room for the second corpus copy of the build
        ix.train(niter=10)
        info = ix.ivf_info()
        sizes = info["list_sizes"]
        assert info["nlist"] == NLIST and int(sizes.sum()) == N and int(sizes.max()) < 40 * (N // NLIST)
        ix.set_search_mode("ivf_listmajor")
        d, r = ix.search(Q, k=K, nprobe=NPROBE)
        assert ix.last_search_stats()["path"] == "ivf_listmajor"
        ix.set_search_mode("ivf")
        d3, r3 = ix.search(Q[:48], k=K, nprobe=NPROBE)
        assert np.array_equal(r3, r[:48]) and np.array_equal(bits(d3), bits(d[:48]))
        ix.set_search_mode("auto")
        da, ra = ix.search(Q, k=K, nprobe=NPROBE)  # whatever the planner picks returns the same probe result or the exact one
        sta = ix.last_search_stats()
        path = sta["path"]
        assert path == "ivf_coarse" and sta["uncertified"] <= NQ // 16, sta  # round 3: the int8 coarse stage (bound and refine) answers such a batch
        assert (np.array_equal(ra, r) and np.array_equal(bits(da), bits(d))) if path.startswith("ivf") else np.array_equal(ra, r_bf)
        assert (r >= 0).all() and (r < N).all() and (np.diff(d, axis=1) >= 0).all()
        for qi in range(0, NQ, 41):  # 25 queries: every returned distance bit-exact on the regenerated rows, order = (distance, row)
            rows = orc.synth_clustered_rows(r[qi], D, 0, NLIST, 0.5)
            od, oi = orc.search(rows, Q[qi:qi + 1], K, "L2")
            assert np.array_equal(bits(od[0]), bits(d[qi])) and np.array_equal(r[qi][oi[0]], r[qi]), qi
            rows = orc.synth_clustered_rows(r_bf[qi], D, 0, NLIST, 0.5)
            od, _ = orc.search(rows, Q[qi:qi + 1], K, "L2")
            assert np.array_equal(bits(od[0]), bits(d_bf[qi])), qi
        recall = float(np.mean([len(set(a) & set(b)) / K for a, b in zip(r.tolist(), r_bf.tolist())]))
        assert recall >= 0.99, recall  # published with the bench line: 1.0 on this corpus
    finally:
        ix.close()


def test_train_errors(rt):
    flat = _native.Index(rt, 64, metric="L2", kind="FLAT")
    flat.add(np.zeros((10, 64), np.float32))
    with pytest.raises(_native.ScError):
        flat.train()
    empty = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=8)
    with pytest.raises(_native.ScError):
        empty.train()
    tiny = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=128)
    tiny.add(np.random.default_rng(0).standard_normal((20, 64)).astype(np.float32))
    tiny.train(niter=2)  # nlist clamps to the row count
    assert tiny.ivf_info()["nlist"] == 20
    flat.close(); empty.close(); tiny.close()


def test_clustered_synthetic_fill_matches_restatement(rt):
    ix = _native.Index(rt, 96, metric="L2")
    ix.fill_synthetic_clustered(2000, seed=5, nclusters=37, spread=0.5, first_row=1000)
    got = ix.get_rows(0, 2000)
    want = orc.synth_clustered(2000, 96, seed=5, nclusters=37, spread=0.5, first_row=1000)
    assert np.array_equal(bits(got), bits(want))
    ix.close()


def test_sharded_ivf_with_shared_centroids_equals_one_index(rt):
    """Multi-GPU IVF_FLAT, two logical shards on one device: shard 0 trains, shard 1 builds its lists for
    shard 0's centroids (sc_index_assign_lists = what the other ranks do after the broadcast); the merge of the two shards' probe
    results equals the probe result of ONE index over all rows with the same centroids -- the result does not depend on sharding."""
    X, centers = clustered(24_000, 64, 30, seed=21)
    rng = np.random.default_rng(22)
    Q = (centers[rng.integers(0, 30, size=48)] + 0.3 * rng.standard_normal((48, 64))).astype(np.float32)
    a = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=32, row_base=0)
    b = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=32, row_base=12_000)
    a.add(X[:12_000])
    b.add(X[12_000:])
    a.train(niter=6)
    cent = a.ivf_info()["centroids"]
    b.assign_lists(cent)
    assert np.array_equal(bits(b.ivf_info()["centroids"]), bits(cent))
    whole = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=32)
    whole.add(X)
    whole.assign_lists(cent)
    assert int(whole.ivf_info()["list_sizes"].sum()) == 24_000
    assert np.array_equal(whole.ivf_info()["list_sizes"], a.ivf_info()["list_sizes"] + b.ivf_info()["list_sizes"])
    for mode, nq in (("ivf", 3), ("ivf_listmajor", 48)):
        for ix in (a, b, whole):
            ix.set_search_mode(mode)
        da, ra = a.search(Q[:nq], k=10, nprobe=4)
        db, rb = b.search(Q[:nq], k=10, nprobe=4)
        dw, rw = whole.search(Q[:nq], k=10, nprobe=4)
        md, mr = _native.topk_merge_host("L2", np.stack([da, db]), np.stack([ra, rb]))
        assert np.array_equal(mr, rw) and np.array_equal(bits(md), bits(dw)), mode
    for ix in (a, b, whole):
        ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_gpu_build_matches_committed_build(rt, golden, metric):
    """The device build against the committed lock of the build rule (tests/golden/ivf_4096x64.npz): centroids bit for bit, the
    same list of every row, the same probe results."""
    d = np.load(golden / "knn_4096x64.npz")
    g = np.load(golden / "ivf_4096x64.npz")
    ix = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=16)
    ix.add(d["X"])
    ix.train(niter=6)
    assert np.array_equal(bits(ix.ivf_info()["centroids"]), bits(g[f"{metric}_centroids"]))
    assert np.array_equal(ix.ivf_assignments(), g[f"{metric}_assign"])
    for mode in ("ivf", "ivf_listmajor"):
        ix.set_search_mode(mode)
        dist, rows = ix.search(d["Q"], k=10, nprobe=4)
        assert np.array_equal(rows, g[f"{metric}_rows"]) and np.array_equal(bits(dist), bits(g[f"{metric}_dist"])), mode
    ix.close()


def test_search_survives_a_refresh_that_cannot_get_its_memory(rt):
    """Upserts into a trained index are folded into the lists by a re-layout that needs a second copy of the corpus.  When that
    allocation fails the search used to fail with it (and the store's Retriever then returned [] silently): now the rows upserted
    since the build are covered by the position -> row id map and the query is answered exhaustively -- exact results, appended and
    replaced rows included -- until a refresh succeeds again."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((6000, 64)).astype(np.float32)
    ix = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=16)
    ix.add(X)
    ix.train(niter=4)
    extra = rng.standard_normal((300, 64)).astype(np.float32)
    repl_rows = np.array([5, 999, 4321], np.int64)
    repl = rng.standard_normal((3, 64)).astype(np.float32)
    _native.diag_set_option("ivf_refresh_nomem", 1)
    try:
        ix.add(extra)
        ix.overwrite(repl, repl_rows)
        full = np.concatenate([X, extra])
        full[repl_rows] = repl
        Q = np.concatenate([extra[:5], repl, rng.standard_normal((4, 64)).astype(np.float32)])
        for q in (Q, Q[:1]):
            d, r = ix.search(q, k=8, nprobe=4)
            od, orow = orc.search(full, q, 8, "L2")
            assert np.array_equal(r, orow) and np.array_equal(d.view(np.uint32), od.view(np.uint32))
        assert r[0, 0] == 6000  # an appended row is found
    finally:
        _native.diag_set_option("ivf_refresh_nomem", 0)
    # memory is back: the next search folds the rows into their lists and probes again
    d, r = ix.search(Q, k=8, nprobe=16)
    od, orow = orc.search(full, Q, 8, "L2")
    assert np.array_equal(r, orow) and np.array_equal(d.view(np.uint32), od.view(np.uint32))
    assert ix.last_search_stats()["path"] in ("ivf", "ivf_listmajor", "exact", "batched")
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("dim,n,ncl,nlist", [(96, 30_000, 25, 64), (768, 40_000, 40, 64), (2048, 12_000, 20, 32)])
def test_coarse_stage_probe_equals_exact_listmajor_probe(rt, dim, n, ncl, nlist, metric):
    """List-major probing behind the int8 coarse stage (lists quantised relative to their centroids; L2: one centred query per (query,
    list) pair, IP: the query itself plus the pair's <c, q>, COSINE: that form on unit vectors; coarse scores as bounds of the exact score; bound and refine;
    what it cannot hold probed again exactly) returns bit for bit what the exact list-major probe returns: tight and loose
    clusters, empty lists, lists longer than one row tile and wanted by more queries than one group of 64 slots, k up to 64, few
    workgroups walking many work items."""
    X, centers = clustered(n, dim, ncl, seed=41)
    rng = np.random.default_rng(42)
    ix = _native.Index(rt, dim, metric=metric, kind="IVF_FLAT", nlist=nlist)
    ix.add(X)
    ix.train(niter=5)
    try:
        for nq, k, nprobe, wgs in ((2, 10, 2, 0), (70, 1, 4, 0), (200, 10, 16, 8), (333, 64, 7, 0), (40, 5, nlist - 1, 24), (90, 100, 9, 0)):  # k = 100: 512 re-scored for the bound
            Q = (centers[rng.integers(0, ncl, size=nq)] + 0.4 * rng.standard_normal((nq, dim))).astype(np.float32)
            ix.set_search_mode("ivf_listmajor")
            d4, r4 = ix.search(Q, k=k, nprobe=nprobe)
            _native.diag_set_option("coarse_workgroups", wgs)
            ix.set_search_mode("ivf_coarse")
            for cap in (-1, 8):  # 8: a refine step that takes on 8 rows per query -- most queries go to the exact re-probe
                _native.diag_set_option("ivf_refine_cap", cap)
                d5, r5 = ix.search(Q, k=k, nprobe=nprobe)
                st = ix.last_search_stats()
                assert st["path"] == "ivf_coarse", st
                assert np.array_equal(r4, r5) and np.array_equal(bits(d4), bits(d5)), (metric, dim, nq, k, nprobe, cap, st)
                if cap < 0:
                    assert st["uncertified"] <= max(2, nq // 8), st  # bound and refine answers the bulk of a clustered batch itself
    finally:
        _native.diag_set_option("coarse_workgroups", 0)
        _native.diag_set_option("ivf_refine_cap", -1)
        ix.close()


def test_coarse_stage_follows_a_retrain_and_takes_huge_batches_in_chunks(rt):
    """A second train over the same rows installs other lists: the centred shadow of the coarse stage must be rebuilt (it used to be
    kept while the row count stayed the same).  A batch of 5 000 queries goes through the stage in chunks of 4 096."""
    X, centers = clustered(40_000, 96, 30, seed=71)
    rng = np.random.default_rng(72)
    Q = (centers[rng.integers(0, 30, size=5000)] + 0.4 * rng.standard_normal((5000, 96))).astype(np.float32)
    ix = _native.Index(rt, 96, metric="L2", kind="IVF_FLAT", nlist=48)
    ix.add(X)
    for niter in (2, 6):  # different centroids, same rows
        ix.train(niter=niter)
        ix.set_search_mode("ivf_listmajor")
        d4, r4 = ix.search(Q, k=10, nprobe=6)
        ix.set_search_mode("ivf_coarse")
        d5, r5 = ix.search(Q, k=10, nprobe=6)
        st = ix.last_search_stats()
        assert st["path"] == "ivf_coarse", st
        assert np.array_equal(r4, r5) and np.array_equal(bits(d4), bits(d5)), (niter, st)
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_rows_appended_to_a_trained_index_are_searched_as_a_tail_without_a_relayout(rt, metric):
    """Appends to a trained index do not force a re-layout before the next probe (seconds at 10M rows): up to 65 536 appended rows stay
    behind the lists and every probe also scans them exactly.  Result = best k of (probe of the lists) and (exact search of the tail),
    whichever probe path answers; ivf_info() (or a tail beyond its limit) folds them into the lists as before."""
    X, centers = clustered(120_000, 64, 40, seed=91)
    rng = np.random.default_rng(92)
    Q = (centers[rng.integers(0, 40, size=90)] + 0.3 * rng.standard_normal((90, 64))).astype(np.float32)
    T = (centers[rng.integers(0, 40, size=700)] + 0.3 * rng.standard_normal((700, 64))).astype(np.float32)
    T[:40] = Q[:40] + np.float32(1e-3)  # appended rows that must show up at the top
    modes = (("ivf", 3), ("ivf_listmajor", 90), ("ivf_coarse", 90), ("auto", 90), ("auto", 1))
    ix = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=32)
    tailix = _native.Index(rt, 64, metric=metric, row_base=len(X))
    try:
        ix.add(X)
        ix.train(niter=4)
        lists_only = {}
        for mode, nq in modes:  # the lists alone, before anything is appended
            ix.set_search_mode(mode)
            lists_only[(mode, nq)] = ix.search(Q[:nq], k=10, nprobe=5)
            assert ix.last_search_stats().get("tail_rows", 0) == 0
        ix.add(T)
        tailix.add(T)
        tailix.set_search_mode("exact")
        dt, rt_ = tailix.search(Q, k=10)
        for mode, nq in modes:
            ix.set_search_mode(mode)
            d, r = ix.search(Q[:nq], k=10, nprobe=5)
            st = ix.last_search_stats()
            assert st["path"].startswith("ivf") and st["tail_rows"] == 700, (mode, st)
            dp, rp = lists_only[(mode, nq)]
            for i in range(nq):  # best 10 of the two disjoint sets, order = (score, row id)
                cd = np.concatenate([dp[i], dt[i]])
                cr = np.concatenate([rp[i], rt_[i]])
                keep = cr >= 0
                cd, cr = cd[keep], cr[keep]
                order = np.lexsort((cr, cd if metric == "L2" else -cd))[:10]
                assert np.array_equal(r[i], cr[order]) and np.array_equal(bits(d[i]), bits(cd[order])), (mode, i)
            if nq >= 40 and metric == "L2":
                assert (r[:40, 0] == len(X) + np.arange(40)).all()  # the planted rows lead their queries
        info = ix.ivf_info()  # folds the tail into the lists
        assert int(info["list_sizes"].sum()) == len(X) + 700
        ix.set_search_mode("auto")
        ix.search(Q, k=10, nprobe=5)
        assert ix.last_search_stats()["tail_rows"] == 0
        _native.diag_set_option("ivf_tail_rows", 0)  # no tail allowed: an append is folded in by the very next search
        ix.add(T[:10])
        ix.search(Q, k=10, nprobe=5)
        assert ix.last_search_stats()["tail_rows"] == 0 and int(ix.ivf_info()["list_sizes"].sum()) == len(X) + 710
    finally:
        _native.diag_set_option("ivf_tail_rows", -1)
        ix.close(); tailix.close()


def test_coarse_stage_without_room_for_its_shadow_leaves_the_exact_probe_in_charge(rt):
    """The centred int8 shadow is a quarter of the corpus again; when it cannot be allocated the batch is probed exactly (same
    results), the stage stays off for this index, and a re-train brings it back."""
    X, centers = clustered(40_000, 96, 30, seed=81)
    rng = np.random.default_rng(82)
    Q = (centers[rng.integers(0, 30, size=200)] + 0.4 * rng.standard_normal((200, 96))).astype(np.float32)
    ix = _native.Index(rt, 96, metric="L2", kind="IVF_FLAT", nlist=48)
    ix.add(X)
    ix.train(niter=3)
    ix.set_search_mode("ivf_listmajor")
    d4, r4 = ix.search(Q, k=10, nprobe=6)
    try:
        _native.diag_set_option("ivf_coarse_nomem", 1)
        ix.set_search_mode("ivf_coarse")
        d5, r5 = ix.search(Q, k=10, nprobe=6)
        assert ix.last_search_stats()["path"] == "ivf_listmajor"
        assert np.array_equal(r4, r5) and np.array_equal(bits(d4), bits(d5))
    finally:
        _native.diag_set_option("ivf_coarse_nomem", 0)
    ix.train(niter=3)
    ix.set_search_mode("ivf_coarse")
    d6, r6 = ix.search(Q, k=10, nprobe=6)
    assert ix.last_search_stats()["path"] == "ivf_coarse"
    ix.set_search_mode("ivf_listmajor")
    d7, r7 = ix.search(Q, k=10, nprobe=6)
    assert np.array_equal(r6, r7) and np.array_equal(bits(d6), bits(d7))
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_coarse_stage_with_lists_longer_than_its_survivor_lists(rt, metric):
    """The reference's own index parameters (nlist 128) put tens of thousands of rows into a list: phase A then takes a 4 096-row
    prefix of the nearest list (any subset bounds the k-th score) and the rest of that list joins phase B."""
    X, centers = clustered(90_000, 64, 6, seed=61, spread=0.5)
    rng = np.random.default_rng(62)
    ix = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=6)
    ix.add(X)
    ix.train(niter=4)
    sizes = ix.ivf_info()["list_sizes"]
    assert sizes.max() > 8192, sizes
    Q = (centers[rng.integers(0, 6, size=150)] + 0.5 * rng.standard_normal((150, 64))).astype(np.float32)
    for nprobe, k in ((2, 10), (5, 33)):
        ix.set_search_mode("ivf_listmajor")
        d4, r4 = ix.search(Q, k=k, nprobe=nprobe)
        ix.set_search_mode("ivf_coarse")
        d5, r5 = ix.search(Q, k=k, nprobe=nprobe)
        st = ix.last_search_stats()
        assert st["path"] == "ivf_coarse", st
        assert np.array_equal(r4, r5) and np.array_equal(bits(d4), bits(d5)), (metric, nprobe, k, st)
        assert st["uncertified"] <= 15, st
    ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_coarse_stage_survives_upserts_and_near_duplicates(rt, metric):
    """Rows upserted after the build are folded into the lists (refresh), which rebuilds the centred shadow.  700 near-duplicates of
    one row (gaps far below any int8 bound) all have lower bounds within reach of the k-th distance: the refine step re-scores them
    all; with the step limited to 8 rows, and for 4500 duplicates (more than it takes on), the exact probe answers.  Same bits
    every time."""
    X, centers = clustered(20_000, 128, 30, seed=51)
    rng = np.random.default_rng(52)
    ix = _native.Index(rt, 128, metric=metric, kind="IVF_FLAT", nlist=32)
    ix.add(X)
    ix.train(niter=4)
    dup = (X[123][None, :] + 1e-4 * rng.standard_normal((700, 128))).astype(np.float32)
    ix.add(dup)
    ix.overwrite(rng.standard_normal((2, 128)).astype(np.float32), np.array([7, 19_000], np.int64))
    Q = np.concatenate([dup[:20], (centers[rng.integers(0, 30, size=80)] + 0.4 * rng.standard_normal((80, 128))).astype(np.float32)])
    try:
        ix.set_search_mode("ivf_listmajor")
        d4, r4 = ix.search(Q, k=10, nprobe=8)
        ix.set_search_mode("ivf_coarse")
        d6, r6 = ix.search(Q, k=10, nprobe=8)
        st1 = ix.last_search_stats()
        assert st1["path"] == "ivf_coarse" and st1["uncertified"] == 0, st1
        assert np.array_equal(r4, r6) and np.array_equal(bits(d4), bits(d6))
        _native.diag_set_option("ivf_refine_cap", 8)
        d5, r5 = ix.search(Q, k=10, nprobe=8)
        st0 = ix.last_search_stats()
        assert st0["path"] == "ivf_coarse" and st0["uncertified"] >= 20, st0
        assert np.array_equal(r4, r5) and np.array_equal(bits(d4), bits(d5))
        _native.diag_set_option("ivf_refine_cap", -1)
        # more near-duplicates than the refine step takes on: those queries are probed exactly
        dup2 = (X[123][None, :] + 1e-4 * rng.standard_normal((3800, 128))).astype(np.float32)
        ix.add(dup2)
        ix.ivf_info()  # fold the appended rows into the lists (left alone they would be searched as a tail, outside the coarse stage)
        ix.set_search_mode("ivf_listmajor")
        d7, r7 = ix.search(Q, k=10, nprobe=8)
        ix.set_search_mode("ivf_coarse")
        d8, r8 = ix.search(Q, k=10, nprobe=8)
        st2 = ix.last_search_stats()
        assert st2["path"] == "ivf_coarse" and st2["uncertified"] >= 20, st2
        assert np.array_equal(r7, r8) and np.array_equal(bits(d7), bits(d8))
    finally:
        _native.diag_set_option("ivf_refine_cap", -1)
        ix.close()


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_rows_overwritten_in_their_lists_refresh_their_shadow_rows_only(rt, metric):
    """A re-index of unchanged or slightly changed chunks overwrites rows that stay in their lists: no re-layout, and the shadows the
    coarse stages read (centred int8 of the IVF stage; int8 / bf16 of the exhaustive batched path) re-build the rows that changed, not
    themselves.  Every path must see the NEW vectors: same bits as the per-query probe / the exact scan, and (L2) each query that
    equals an overwritten row finds it first."""
    X, centers = clustered(150_000, 64, 40, seed=131)
    rng = np.random.default_rng(132)
    ix = _native.Index(rt, 64, metric=metric, kind="IVF_FLAT", nlist=32)
    try:
        ix.add(X)
        ix.train(niter=4)
        sizes = ix.ivf_info()["list_sizes"].copy()
        Q0 = (centers[rng.integers(0, 40, size=90)] + 0.3 * rng.standard_normal((90, 64))).astype(np.float32)
        for mode in ("ivf_coarse", "batched"):  # build the shadows on the old rows
            ix.set_search_mode(mode)
            ix.search(Q0, k=10, nprobe=5)
        for rnd in range(3):
            tgt = np.sort(rng.choice(len(X), size=60, replace=False)).astype(np.int64)
            new = (X[tgt] * np.float32(1.0 + 2e-3 * (rnd + 1)) + np.float32(1e-3) * rng.standard_normal((60, 64))).astype(np.float32)  # stays in its list
            ix.overwrite(new, tgt)
            X[tgt] = new
            Q = Q0.copy()
            Q[:60] = new
            ix.set_search_mode("ivf")
            dr, rr = ix.search(Q, k=10, nprobe=5)
            for mode in ("ivf_coarse", "ivf_listmajor", "auto"):
                ix.set_search_mode(mode)
                d, r = ix.search(Q, k=10, nprobe=5)
                assert ix.last_search_stats()["path"].startswith("ivf"), mode
                assert np.array_equal(r, rr) and np.array_equal(bits(d), bits(dr)), (mode, rnd)
            ix.set_search_mode("exact")
            de, re_ = ix.search(Q, k=10)
            ix.set_search_mode("batched")
            d, r = ix.search(Q, k=10)
            assert ix.last_search_stats()["path"] == "batched"
            assert np.array_equal(r, re_) and np.array_equal(bits(d), bits(de)), rnd
            want_d, want_r = orc.search(X, Q[:8], 10, metric)
            assert np.array_equal(re_[:8], want_r) and np.array_equal(bits(de[:8]), bits(want_d))
            if metric == "L2":
                assert (rr[:60, 0] == tgt).all() and (re_[:60, 0] == tgt).all()
        assert np.array_equal(ix.ivf_info()["list_sizes"], sizes)  # nothing moved
        # a re-index: new chunks appended AND known ones overwritten in their lists -- the appended rows stay a tail (no re-layout)
        T = (centers[rng.integers(0, 40, size=300)] + 0.3 * rng.standard_normal((300, 64))).astype(np.float32)
        ix.add(T)
        tgt = np.sort(rng.choice(150_000, size=60, replace=False)).astype(np.int64)
        new = (X[tgt] * np.float32(1.004)).astype(np.float32)
        ix.overwrite(new, tgt)
        X[tgt] = new
        Q = Q0.copy()
        Q[:60] = new
        Q[60:80] = T[:20]
        got = {}
        for mode in ("ivf_coarse", "ivf", "ivf_listmajor"):
            ix.set_search_mode(mode)
            got[mode] = ix.search(Q, k=10, nprobe=5)
            assert ix.last_search_stats()["tail_rows"] == 300, (mode, ix.last_search_stats())
        for mode in ("ivf_coarse", "ivf_listmajor"):
            assert np.array_equal(got[mode][1], got["ivf"][1]) and np.array_equal(bits(got[mode][0]), bits(got["ivf"][0])), mode
        if metric == "L2":
            assert (got["ivf"][1][:60, 0] == tgt).all() and (got["ivf"][1][60:80, 0] == 150_000 + np.arange(20)).all()
    finally:
        ix.close()


def test_search_runs_the_plan_the_host_tests_check(rt):
    """tests/test_ivf_plan_host.py checks the planners through sc_diag_ivf_plan; this ties that entry to the plan a search ran: fed the
    probe table of the same batch (a FLAT search over the centroids under the index metric), the lists' sizes, ld and the CU count,
    it predicts exactly the work the two batched probes report."""
    X, centers = clustered(6000, 64, 24, seed=11)
    rng = np.random.default_rng(12)
    Q = (centers[rng.integers(0, 24, size=80)] + 0.3 * rng.standard_normal((80, 64))).astype(np.float32)
    ix = _native.Index(rt, 64, metric="L2", kind="IVF_FLAT", nlist=32)
    ix.add(X)
    ix.train(niter=6)
    info = ix.ivf_info()
    qz = _native.Index(rt, 64, metric="L2")
    qz.add(info["centroids"])
    probes = qz.search(Q, k=4)[1]
    qz.close()
    list_off = np.concatenate([[0], np.cumsum(info["list_sizes"])])
    for mode, path in (("ivf_listmajor", "listmajor"), ("ivf_coarse", "coarse")):
        plan = _native.diag_ivf_plan(path, probes, list_off, 10, ix.info()["ld"], rt.device_info()["cus"])
        ix.set_search_mode(mode)
        ix.search(Q, k=10, nprobe=4)
        stats = ix.last_search_stats()
        assert stats["path"] == mode and stats["uncertified"] == 0, stats
        want = {name: int(plan[name][0]) for name in ("unique_rows", "streamed_rows", "groups")}
        assert ix.last_probe_stats() == want, (mode, ix.last_probe_stats(), want)
    ix.close()
