"""GPU: the lexical and the hybrid search (sc_index_set_terms, sc_index_lex_stats, sc_index_search_lexical*, sc_index_search_hybrid*:
lex_prep_kernel, lex_scan_kernel, lex_stats_kernel, lex_fuse_kernel) against the reference of tests/lex_ref.py.

Bar: ids compared with np.array_equal, scores by their uint32 view, for the rules in include/semcode_hip.h.  Shapes: 1, 63, 1 000 and
4 099 rows (4 099 is no multiple of the 2, 4 or 16 rows of a wave load nor of a workgroup's share), T = 32 and 128, 1, 3 and 17
queries (17 = two passes of 16), k = 1, 10 and 128.  The term rows hold an empty row, a full row, the term values 0 and 0xFFFE, twenty
identical rows (ties go by row id), a term that only three rows hold (padding appears), and a query term that no row holds.  The
reference is computed once per (T, rows) at k = 128 and shared: the top-k is its prefix."""
import numpy as np
import pytest

import lex_ref
from oracle import sc_oracle as orc
from semcode_amd import _native
from semcode_amd.embeddings.payload import EmbeddingPayload
from semcode_amd.storage import MilvusVectorStore

pytestmark = pytest.mark.gpu

DIM = 64
N = 4099
NQ = 17
ROWS = [1, 63, 1000, 4099]
K1, B = 1.2, 0.75
RARE, ABSENT, TIE = 40000, 50001, 41000  # a term only rows 5, 700 and 4098 hold; a term no row holds; a term only the identical rows hold


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check(got, want, what=""):
    (s, r), (ws, wr) = got, want
    assert np.array_equal(r, wr), f"{what}: ids differ, first query {np.flatnonzero((r != wr).any(1))[:1]}"
    assert np.array_equal(bits(s), bits(ws)), f"{what}: scores differ"


def make_terms(T, seed):
    """[N, T] sorted term rows over a Zipf-like vocabulary of 300 terms that holds 0 and 0xFFFE."""
    rng = np.random.default_rng(seed)
    vocab = np.unique(np.concatenate([[0, 0xFFFE], rng.integers(1, 30000, size=298)])).astype(np.uint16)
    p = 1.0 / np.arange(1, vocab.size + 1)
    p /= p.sum()
    terms = np.full((N, T), 0xFFFF, dtype=np.uint16)
    for r in range(N):
        dl = int(rng.integers(0, T + 1))
        terms[r, :dl] = rng.choice(vocab, size=dl, p=p)
    terms[0] = 0xFFFF  # the only row of the 1-row corpus is empty ...
    terms[1] = rng.choice(vocab, size=T)  # ... a full row
    terms[2, : T // 2] = 0  # term 0, T / 2 times
    terms[2, T // 2:] = 0xFFFE  # (a full row again)
    terms[100:120] = terms[1]  # twenty identical rows, the only ones with TIE (three times)
    terms[100:120, :3] = TIE
    for r in (5, 700, N - 1):
        terms[r, 0] = RARE
    terms.sort(axis=1)
    return terms, vocab


def make_queries(vocab, seed):
    """17 queries: m = 1, m = 32, one with the rare term only (fewer than k hits), one matching nothing, the terms 0 and 0xFFFE."""
    rng = np.random.default_rng(seed)
    qt = np.full((NQ, 32), 0xFFFF, dtype=np.uint16)
    qw = np.zeros((NQ, 32), dtype=np.float32)
    nt = np.zeros(NQ, dtype=np.int32)
    for q in range(NQ):
        m = [1, 32, 1, 1, 2, 0, 1][q] if q < 7 else int(rng.integers(1, 33))
        if q == 2:
            ts = np.array([RARE])
        elif q == 3:
            ts = np.array([ABSENT])
        elif q == 4:
            ts = np.array([0, 0xFFFE])
        elif q == 6:
            ts = np.array([TIE])
        else:
            ts = np.sort(rng.choice(vocab, size=m, replace=False))
        qt[q, :m] = ts
        qw[q, :m] = (rng.random(m) * 8 + 0.05).astype(np.float32)
        nt[q] = m
    return qt, qw, nt


@pytest.fixture(scope="module")
def data():
    """T -> (terms, vocab, queries, cache of references by (rows, allow key))."""
    out = {}
    for T in (32, 128):
        terms, vocab = make_terms(T, 900 + T)
        out[T] = (terms, vocab, make_queries(vocab, 910 + T), {})
    return out


def avgdl_of(terms):
    n = len(terms)
    return float(np.float32((terms != 0xFFFF).sum() / n)) if (terms != 0xFFFF).any() else 1.0


def reference(data, T, n, allow=None, key=None):
    terms, _, (qt, qw, nt), cache = data[T]
    ck = (n, key)
    if ck not in cache:
        cache[ck] = lex_ref.search(terms[:n], qt, qw, nt, 128, K1, B, avgdl_of(terms[:n]), allow)
    return cache[ck]


@pytest.fixture(scope="module")
def X():
    return orc.synth(N, DIM, seed=77)


def index_with_terms(rt, X, terms, n, **kw):
    ix = _native.Index(rt, DIM, **kw)
    if n:
        ix.add(X[:n])
    ix.set_terms(terms[:n])
    return ix


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("T", [32, 128])
def test_lexical_search(rt, data, X, T, n):
    terms, _, (qt, qw, nt), _ = data[T]
    ix = index_with_terms(rt, X, terms, n)
    avgdl = avgdl_of(terms[:n])
    ws, wr = reference(data, T, n)
    for nq in (1, 3, NQ):
        for k in (1, 10, 128):
            got = ix.search_lexical(qt[:nq], qw[:nq], nt[:nq], k=k, k1=K1, b=B, avgdl=avgdl)
            check(got, (ws[:nq, :k], wr[:nq, :k]), f"T={T} rows={n} Q={nq} k={k}")
            assert ix.last_search_stats()["path"] == "lexical"
            assert ix.last_lex_stats() == {"rows_scanned": n, "bytes_per_pass": n * 2 * T, "passes": (nq + 15) // 16}
    s, r = ix.search_lexical(qt, qw, nt, k=10, k1=K1, b=B, avgdl=avgdl)
    assert (r[3] == -1).all() and (s[3] == -np.inf).all() and (r[5] == -1).all()  # the absent term; the query without terms
    if n == N:
        assert sorted(r[2][:3].tolist()) == [5, 700, N - 1] and (r[2][3:] == -1).all()  # the rare term: padding behind three hits
    if n >= 1000:
        s, r = ix.search_lexical(qt, qw, nt, k=128, k1=K1, b=B, avgdl=avgdl)
        assert r[6][:20].tolist() == list(range(100, 120)) and (r[6][20:] == -1).all() and len(set(s[6][:20].tolist())) == 1  # equal scores: by row id
    # allow bitsets: everything, one row, nothing
    for name, allow in (("all", np.ones(n, bool)), ("one", np.arange(n) == min(n - 1, 2)), ("none", np.zeros(n, bool))):
        want = reference(data, T, n, allow, name)
        got = ix.search_lexical(qt, qw, nt, k=10, k1=K1, b=B, avgdl=avgdl, allow=allow)
        check(got, (want[0][:, :10], want[1][:, :10]), f"T={T} rows={n} allow={name}")
        if name == "none":
            assert (got[1] == -1).all()
    # other parameters, and the chunking of many queries does not show
    _native.diag_set_option("lex_chunk_q", 16)
    try:
        got = ix.search_lexical(qt, qw, nt, k=7, k1=0.9, b=0.3, avgdl=11.0)
    finally:
        _native.diag_set_option("lex_chunk_q", -1)
    check(got, lex_ref.search(terms[:n], qt, qw, nt, 7, 0.9, 0.3, 11.0), "k1 = 0.9, b = 0.3, chunks of 16")
    ix.close()


def test_argument_errors(rt, data, X):
    terms, _, (qt, qw, nt), _ = data[32]
    ix = _native.Index(rt, DIM)
    ix.add(X[:63])
    with pytest.raises(_native.ScError, match=r"installed for -1 rows.*63"):
        ix.search_lexical(qt, qw, nt, k=5, avgdl=3.0)
    with pytest.raises(_native.ScError, match="first_row=1 exceeds the 0 term rows held"):
        ix.set_terms(terms[:10], first_row=1)
    with pytest.raises(_native.ScError, match="index of 63 rows"):
        ix.set_terms(terms[:64])
    with pytest.raises(_native.ScError, match="T must be"):
        ix.set_terms(np.zeros((63, 48), np.uint16))
    ix.set_terms(terms[:63])
    with pytest.raises(_native.ScError, match="T=128"):
        ix.set_terms(data[128][0][:63])
    for bad in (dict(k=0), dict(k=129), dict(avgdl=0.0), dict(avgdl=float("nan")), dict(k1=float("inf")), dict(allow=np.zeros(1, np.uint32))):
        with pytest.raises(_native.ScError):
            ix.search_lexical(qt, qw, nt, **{"k": 5, "avgdl": 3.0, **bad})
    unsorted = qt.copy()
    unsorted[1, :2] = unsorted[1, 1::-1]
    with pytest.raises(_native.ScError, match="strictly ascending"):
        ix.search_lexical(unsorted, qw, nt, k=5, avgdl=3.0)
    zero_w = qw.copy()
    zero_w[0, 0] = 0.0
    with pytest.raises(_native.ScError, match="finite and > 0"):
        ix.search_lexical(qt, zero_w, nt, k=5, avgdl=3.0)
    q = orc.synth(NQ, DIM, seed=5)
    for bad in (dict(k=11, fetch_k=10), dict(fetch_k=129), dict(c=0), dict(dense_weight=-1.0), dict(lexical_weight=float("inf"))):
        with pytest.raises(_native.ScError):
            ix.search_hybrid(q, qt, qw, nt, **{"k": 5, "fetch_k": 20, "avgdl": 3.0, **bad})
    ix.drop_terms()
    with pytest.raises(_native.ScError, match=r"installed for -1 rows"):
        ix.lex_stats()
    ix.set_terms(data[128][0][:63])  # after a drop any T installs
    ix.close()


def stats_equal(ix, terms):
    st = ix.lex_stats()
    n, total, df = lex_ref.stats(terms)
    assert (st["rows"], st["sum_dl"]) == (n, total)
    assert np.array_equal(st["df"], df)


def test_statistics_ranges_and_appends(rt, data, X):
    terms, _, (qt, qw, nt), _ = data[128]
    host = terms[:1000].copy()
    ix = index_with_terms(rt, X, host, 1000)
    stats_equal(ix, host)
    stats_equal(ix, host)  # (the cached table)
    # a ranged overwrite
    host[200:263] = terms[3000:3063]
    ix.set_terms(host[200:263], first_row=200)
    stats_equal(ix, host)
    check(ix.search_lexical(qt, qw, nt, k=10, avgdl=20.0), lex_ref.search(host, qt, qw, nt, 10, K1, B, 20.0), "after the overwrite")
    # an append: invalid, naming both counts, until its range is installed
    ix.add(X[1000:1100])
    for call in (ix.lex_stats, lambda: ix.search_lexical(qt, qw, nt, k=10, avgdl=20.0),
                 lambda: ix.search_hybrid(X[:NQ], qt, qw, nt, k=5, fetch_k=10, avgdl=20.0)):
        with pytest.raises(_native.ScError, match=r"installed for 1000 rows.*the index has 1100"):
            call()
    with pytest.raises(_native.ScError, match="first_row=1001 exceeds the 1000"):
        ix.set_terms(terms[1001:1100], first_row=1001)
    host = np.concatenate([host, terms[1000:1100]])
    ix.set_terms(host[1000:], first_row=1000)
    stats_equal(ix, host)
    check(ix.search_lexical(qt, qw, nt, k=10, avgdl=20.0), lex_ref.search(host, qt, qw, nt, 10, K1, B, 20.0), "after the append")
    # release_scratch keeps the term rows
    ix.release_scratch()
    check(ix.search_lexical(qt, qw, nt, k=10, avgdl=20.0), lex_ref.search(host, qt, qw, nt, 10, K1, B, 20.0), "after release_scratch")
    ix.close()


def test_delete_drops_the_terms_and_layout_does_not_matter(rt, data, X):
    terms, _, (qt, qw, nt), _ = data[32]
    avgdl = avgdl_of(terms)
    flat = index_with_terms(rt, X, terms, N)
    ivf = index_with_terms(rt, X, terms, N, kind="IVF_FLAT", nlist=16)
    ivf.train(niter=3)
    assert ivf.ivf_info()["nlist"] == 16
    want = reference(data, 32, N)
    for ix in (flat, ivf):  # term rows are in row-number order wherever the vectors lie
        check(ix.search_lexical(qt, qw, nt, k=128, k1=K1, b=B, avgdl=avgdl), want, "flat / trained")
        stats_equal(ix, terms)
    gone = np.array([0, 5, 100, 101, 4098])
    for ix in (flat, ivf):
        ix.delete_rows(gone)
        with pytest.raises(_native.ScError, match=r"installed for -1 rows.*the index has 4094"):
            ix.search_lexical(qt, qw, nt, k=10, avgdl=avgdl)
        left = np.delete(terms, gone, axis=0)
        ix.set_terms(left)
        check(ix.search_lexical(qt, qw, nt, k=10, k1=K1, b=B, avgdl=avgdl), lex_ref.search(left, qt, qw, nt, 10, K1, B, avgdl), "after the delete")
        ix.close()


def dense_reference(X, Q, F, metric, allow=None):
    """rows [Q, F] of the oracle's exact top-F among the allowed rows, padded with -1."""
    idx = np.arange(len(X)) if allow is None else np.flatnonzero(allow)
    rows = np.full((len(Q), F), -1, dtype=np.int64)
    C = min(F, idx.size)
    if C:
        rows[:, :C] = idx[orc.search(X[idx], Q, C, metric)[1]]
    return rows


@pytest.mark.parametrize("metric", ["IP", "L2", "COSINE"])
def test_hybrid_search(rt, data, X, metric):
    T, n = 128, N
    terms, _, (qt, qw, nt), _ = data[T]
    avgdl = avgdl_of(terms)
    Q = orc.synth(NQ, DIM, seed=78)
    rng = np.random.default_rng(12)
    ix = index_with_terms(rt, X, terms, n, metric=metric)
    masks = {"none": None, "40 %": rng.random(n) < 0.4, "nine rows": np.isin(np.arange(n), rng.choice(n, 9, replace=False))}
    for name, allow in masks.items():
        for k, F in ((10, 40), (1, 1), (128, 128)):
            dense = dense_reference(X, Q, F, metric, allow)
            lex = reference(data, T, n, allow, None if allow is None else "hybrid " + name)[1][:, :F]  # (the top-F is the prefix of the top-128)
            for c, wd, wl in ((60, 1.0, 1.0), (3, 0.25, 1.5)):
                want = [lex_ref.rrf(dense[i], lex[i], k, c, wd, wl) for i in range(NQ)]
                want = (np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
                for nq in (1, NQ):
                    got = ix.search_hybrid(Q[:nq], qt[:nq], qw[:nq], nt[:nq], k=k, fetch_k=F, k1=K1, b=B, avgdl=avgdl, c=c, dense_weight=wd, lexical_weight=wl, allow=allow)
                    check(got, (want[0][:nq], want[1][:nq]), f"{metric} mask={name} k={k} fetch_k={F} c={c} Q={nq}")
            assert ix.last_search_stats()["path"] == "hybrid"
    # wl = 0 and fetch_k = k: the dense order
    s, r = ix.search_hybrid(Q, qt, qw, nt, k=10, fetch_k=10, avgdl=avgdl, lexical_weight=0.0)
    assert np.array_equal(r, ix.search(Q, k=10)[1])
    assert np.array_equal(bits(s), bits(np.tile(np.float32(1.0) / np.arange(60, 70).astype(np.float32), (NQ, 1))))
    ix.close()
    empty = _native.Index(rt, DIM, metric=metric)
    empty.set_terms(np.zeros((0, 128), np.uint16))
    s, r = empty.search_hybrid(Q[:3], qt[:3], qw[:3], nt[:3], k=5, fetch_k=20, avgdl=1.0)
    assert (r == -1).all() and (s == -np.inf).all()
    empty.close()


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_hybrid_on_a_trained_index_with_a_tail(rt, data, X, metric):
    """A trained IVF_FLAT index with 300 rows appended behind its lists: the hybrid search answers as the reference fusion and as a
    FLAT twin, host and device pointers alike, and leaves the tail a tail (the probe that follows still reports it)."""
    import torch

    T, trained, n, k, F = 128, 1000, 1300, 10, 40
    terms, _, (qt, qw, nt), _ = data[T]
    avgdl = avgdl_of(terms[:n])
    Q = orc.synth(NQ, DIM, seed=78)
    ivf = _native.Index(rt, DIM, metric=metric, kind="IVF_FLAT", nlist=16)
    ivf.add(X[:trained])
    ivf.train(niter=3)
    ivf.add(X[trained:n])
    ivf.set_terms(terms[:n])
    twin = index_with_terms(rt, X, terms, n, metric=metric)
    some = np.random.default_rng(14).random(n) < 0.4
    some[-5:] = True
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tq, tt, tw, tn = dev(Q), dev(qt.view(np.int16)), dev(qw), dev(nt)
    for name, allow in (("none", None), ("40 %", some)):
        dense = dense_reference(X[:n], Q, F, metric, allow)
        lex = reference(data, T, n, allow, None if allow is None else "tail " + name)[1][:, :F]
        want = [lex_ref.rrf(dense[i], lex[i], k, 60, 1.0, 1.0) for i in range(NQ)]
        want = (np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
        words = None if allow is None else dev(_native.pack_allow(allow, n).view(np.int32))
        for nq in (NQ, 1):
            what = f"{metric} mask={name} Q={nq}"
            got = ivf.search_hybrid(Q[:nq], qt[:nq], qw[:nq], nt[:nq], k=k, fetch_k=F, k1=K1, b=B, avgdl=avgdl, allow=allow)
            check(got, (want[0][:nq], want[1][:nq]), what)
            assert ivf.last_search_stats()["path"] == "hybrid"
            check(got, twin.search_hybrid(Q[:nq], qt[:nq], qw[:nq], nt[:nq], k=k, fetch_k=F, k1=K1, b=B, avgdl=avgdl, allow=allow), what + ", the FLAT twin")
            score = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            rows = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            ivf.search_hybrid_dev(tq.data_ptr(), nq, k, F, tt.data_ptr(), tw.data_ptr(), tn.data_ptr(), K1, B, avgdl, 60, 1.0, 1.0,
                                  0 if words is None else words.data_ptr(), 0 if words is None else words.numel(), score.data_ptr(), rows.data_ptr())
            rt.synchronize()
            check((score.cpu().numpy(), rows.cpu().numpy()), got, what + ", device pointers")
    ivf.search(Q[:1], k=k, nprobe=4)  # a probe next: it answers from the lists AND the tail, which the hybrid searches left pending
    stats = ivf.last_search_stats()
    assert stats["path"].startswith("ivf") and stats["tail_rows"] == n - trained, stats
    ivf.close()
    twin.close()


def test_hybrid_dev_pointers_report_a_bad_query(rt, data, X):
    import torch

    terms, _, (qt, qw, nt), _ = data[32]
    ix = index_with_terms(rt, X, terms, 1000)
    Q = orc.synth(3, DIM, seed=79)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tq, tt, tw, tn = dev(Q), dev(qt[:3].view(np.int16)), dev(qw[:3]), dev(nt[:3])
    score = torch.empty((3, 10), dtype=torch.float32, device="cuda")
    rows = torch.empty((3, 10), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ix.search_lexical_dev(3, 10, tt.data_ptr(), tw.data_ptr(), tn.data_ptr(), K1, B, 20.0, 0, 0, score.data_ptr(), rows.data_ptr())
    rt.synchronize()
    check((score.cpu().numpy(), rows.cpu().numpy()), lex_ref.search(terms[:1000], qt[:3], qw[:3], nt[:3], 10, K1, B, 20.0), "lexical, device pointers")
    ix.search_hybrid_dev(tq.data_ptr(), 3, 10, 20, tt.data_ptr(), tw.data_ptr(), tn.data_ptr(), K1, B, 20.0, 60, 1.0, 1.0, 0, 0, score.data_ptr(), rows.data_ptr())
    rt.synchronize()
    check((score.cpu().numpy(), rows.cpu().numpy()), ix.search_hybrid(Q, qt[:3], qw[:3], nt[:3], k=10, fetch_k=20, avgdl=20.0), "hybrid, device pointers")
    bad = qt[:3].copy()
    bad[1, :2] = bad[1, 1::-1]  # query 1 (m = 32) descending at its head
    tb = dev(bad.view(np.int16))
    torch.cuda.synchronize()
    with pytest.raises(_native.ScError, match="a query breaks the rules"):
        ix.search_lexical_dev(3, 10, tb.data_ptr(), tw.data_ptr(), tn.data_ptr(), K1, B, 20.0, 0, 0, score.data_ptr(), rows.data_ptr())
    rt.synchronize()
    assert (rows.cpu().numpy()[1] == -1).all()  # ... and was treated as a query without terms
    ix.close()


IDENT = "parse_frobnicate_v2"


@pytest.fixture(scope="module")
def chunks():
    """2 000 synthetic chunks with random vectors; chunk 1234 alone holds IDENT, and its vector is the query's opposite."""
    rng = np.random.default_rng(21)
    words = [f"name{i}" for i in range(400)]
    vec = rng.standard_normal((2000, DIM)).astype(np.float32)
    vec /= np.linalg.norm(vec, axis=1, keepdims=True)
    query = vec[7] + 0.1 * rng.standard_normal(DIM).astype(np.float32)
    vec[1234] = -query / np.linalg.norm(query)
    out = []
    for i in range(2000):
        body = " ".join(rng.choice(words, size=30))
        text = f"def {IDENT}(x): return {body}" if i == 1234 else f"def fn_{i}(x): return {body}"
        out.append(EmbeddingPayload(id=f"c{i}", vector=vec[i].tolist(), text=text, metadata={"repo": f"repo{i % 4}", "path": f"src/f{i // 10}.py", "language": "python"}))
    return out, query


def test_through_the_store(rt, chunks, tmp_path):
    payloads, query = chunks
    question = f"where is {IDENT} defined"
    store = MilvusVectorStore("hyb", DIM, metric="IP", index_type="FLAT", runtime=rt, lexical=True)
    store.connect()
    store.upsert_embeddings(payloads)

    def found(s, **kw):
        plain = [h.id for h in s.search(query, top_k=10, **kw)[0]]
        hybrid = [h.id for h in s.search(query, top_k=10, query_text=question, hybrid=True, **kw)[0]]
        assert "c1234" not in plain, "the dense search alone must miss the chunk"
        assert "c1234" in hybrid[:2], hybrid
        return hybrid

    found(store)
    found(store, repos=["repo2", "repo1"])  # 1234 % 4 == 2
    assert "c1234" not in [h.id for h in store.search(query, top_k=10, query_text=question, hybrid=True, repos=["repo0"])[0]]
    hits = store.search(query, top_k=10, query_text=question, hybrid=True)[0]
    assert hits[0].distance >= hits[1].distance > 0 and all(h.distance <= 2 / 60 for h in hits)  # the fused score
    assert store.delete([f"c{i}" for i in (0, 1, 1000, 1999)]) == 4
    found(store)
    store.save(tmp_path / "hyb")
    again = MilvusVectorStore("hyb", DIM, metric="IP", index_type="FLAT", runtime=rt, lexical=True)
    again.connect()
    again.load(tmp_path / "hyb")
    assert found(again) == found(store)
    # the batch form: one text per query
    d, r = again.search_batch(np.stack([query, query]), 10, query_texts=[question, "nothing of the kind"], hybrid=True)
    assert again._ids[int(r[0][0])] == "c1234" or again._ids[int(r[0][1])] == "c1234"
    assert "c1234" not in [again._ids[int(x)] for x in r[1] if x >= 0]
    store.close()
    again.close()
