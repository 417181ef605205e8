"""CPU: host logic of the MMR search -- the selection rule of semcode_amd/csrc/mmr_rule.h through its host twin
sc_diag_mmr_select_host against the numpy float32 rule of tests/mmr_ref.py (random scores, crafted ties, equal maxima, an input
where a fused multiply-add would pick differently); the mmr / fetch_k keywords of MilvusVectorStore over a stub index that records
its calls; the Retriever's forwarding; the ABI declarations.  The device side is covered by tests/test_mmr_gpu.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import mmr_ref
from semcode_amd import _native
from semcode_amd.services.retrieval import Retriever
from semcode_amd.storage import MilvusVectorStore
from tests.test_grouped_host import Embedder, GroupedIndex, PlainIndex, RecordingStore, payload, unpack

ROOT = Path(__file__).resolve().parent.parent


def host_select(rel, G, k, lam):
    rel = np.ascontiguousarray(rel, dtype=np.float32)
    G = np.ascontiguousarray(G, dtype=np.float32)
    C_, ldg = len(rel), G.shape[1]
    picked = np.full(min(k, C_), -7, dtype=np.int32)
    _native._check(_native.lib().sc_diag_mmr_select_host(rel.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), C_, ldg, int(k), float(lam),
                                                         picked.ctypes.data_as(C.c_void_p)))
    return picked.tolist()


def random_case(C_, seed, ldg=None):
    rng = np.random.default_rng(seed)
    rel = rng.standard_normal(C_).astype(np.float32)
    A = rng.standard_normal((C_, C_)).astype(np.float32)
    G = np.zeros((C_, ldg or C_), dtype=np.float32)
    G[:, :C_] = np.triu(A) + np.triu(A, 1).T  # symmetric, bit for bit
    return rel, G


@pytest.mark.parametrize("C_", [1, 2, 17, 128])
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
def test_host_twin_equals_the_numpy_rule(C_, lam):
    for seed in range(3):
        rel, G = random_case(C_, 100 * C_ + seed, ldg=C_ + (seed % 2) * 5)
        for k in sorted({1, C_}):
            got = host_select(rel, G, k, lam)
            assert got == mmr_ref.select(rel, G, k, lam)
            assert len(got) == k and len(set(got)) == k and got[0] == 0
    # lambda = 1 with a best-first rel: the plain order
    rel = -np.arange(C_, dtype=np.float32)
    assert host_select(rel, random_case(C_, 5)[1], C_, 1.0) == list(range(C_))


def test_equal_values_go_to_the_smaller_index():
    # every candidate equally relevant, equally redundant: v_i is one value, the picks walk up the indices
    C_ = 9
    rel = np.full(C_, 0.25, np.float32)
    G = np.full((C_, C_), 0.5, np.float32)
    for lam in (0.0, 0.3, 1.0):
        assert host_select(rel, G, C_, lam) == list(range(C_)) == mmr_ref.select(rel, G, C_, lam)
    # candidates 2 and 5 tie on top, then 5 must follow 2 only if it still wins
    rel = np.array([9, 1, 4, 1, 1, 4, 1], np.float32)
    G = np.zeros((7, 7), np.float32)
    got = host_select(rel, G, 4, 0.5)
    assert got == [0, 2, 5, 1] == mmr_ref.select(rel, G, 4, 0.5)
    # the same tie, the larger index made redundant with pick 0: the order does not change, then 1 < 3 < 4 < 6
    G[0, 5] = G[5, 0] = 0.0
    G[2, 5] = G[5, 2] = 8.0  # 5 is close to 2: after 2 it falls to 0.5 * 4 - 0.5 * 8 = -2 < 0.5
    assert host_select(rel, G, 7, 0.5) == [0, 2, 1, 3, 4, 6, 5] == mmr_ref.select(rel, G, 7, 0.5)
    # +0 and -0 are equal values
    rel = np.array([1, -0.0, 0.0], np.float32)
    assert host_select(rel, np.zeros((3, 3), np.float32), 3, 1.0) == [0, 1, 2]


def test_equal_maxima_in_g():
    # m_i is a max over the picks: two picks at the same similarity, and a later smaller one, leave it where it was
    rel = np.array([5, 4, 3, 2, 1], np.float32)
    G = np.array([[0, 1, 1, 1, 1],
                  [1, 0, 1, 3, 3],
                  [1, 1, 0, 3, 0.5],
                  [1, 3, 3, 0, 3],
                  [1, 3, 0.5, 3, 0]], np.float32)
    for lam in (0.0, 0.5, 0.75):
        assert host_select(rel, G, 5, lam) == mmr_ref.select(rel, G, 5, lam)
    assert host_select(rel, G, 5, 0.0) == [0, 1, 2, 3, 4]  # all m equal after pick 0 -> 1; then m = (., ., 1, 3, 3) -> 2; then (3, 3) -> 3
    assert host_select(rel, G, 5, 0.5) == [0, 1, 2, 3, 4]


def test_three_roundings_not_a_fused_multiply_add():
    """lambda * rel is rounded before the subtraction.  lambda = 4097 * 2^-13, mu = 4095 * 2^-13 (exact).  Candidate 1: rel = m = 3,
    both products exact, v = 6 * 2^-13 = 3 * 2^-12 however it is computed.  Candidate 2: rel = 4097 * 2^-11, so lambda * rel =
    1 + 2^-11 + 2^-24 exactly, which rounds (to even) to 1 + 2^-11; mu * m = 4095 * 2^-12 for m = 2 is exact; the correctly rounded
    v = 3 * 2^-12: a tie, which goes to candidate 1.  A fused multiply-add keeps the 2^-24 and picks candidate 2."""
    lam = np.float32(4097 * 2.0 ** -13)
    mu = np.float32(1.0) - lam
    assert float(mu) == 4095 * 2.0 ** -13
    rel = np.array([8.0, 3.0, 4097 * 2.0 ** -11], np.float32)
    G = np.zeros((3, 3), np.float32)
    G[0, 1] = G[1, 0] = 3.0
    G[0, 2] = G[2, 0] = 2.0
    v_rounded = [lam * rel[i] - mu * G[i, 0] for i in (1, 2)]
    v_fused = [np.float32(float(lam) * float(rel[i]) - float(mu) * float(G[i, 0])) for i in (1, 2)]  # (every product is exact in float64)
    assert v_rounded[0] == v_rounded[1] == np.float32(3 * 2.0 ** -12)
    assert v_fused[0] == v_rounded[0] and v_fused[1] > v_fused[0]  # the input tells the two apart
    assert mmr_ref.select(rel, G, 2, lam) == [0, 1]
    assert host_select(rel, G, 2, float(lam)) == [0, 1]
    assert host_select(rel, G, 3, float(lam)) == [0, 1, 2]


def test_host_twin_rejects_bad_arguments():
    rel, G = random_case(4, 1)
    lib = _native.lib()
    picked = np.zeros(4, np.int32)
    args = lambda **o: [o.get("rel", rel).ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), o.get("C", 4), o.get("ldg", 4), o.get("k", 2),  # noqa: E731
                        o.get("lam", 0.5), picked.ctypes.data_as(C.c_void_p)]
    assert lib.sc_diag_mmr_select_host(*args()) == 0
    for bad in (dict(C=0), dict(ldg=3), dict(k=0), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan"))):
        assert lib.sc_diag_mmr_select_host(*args(**bad)) == -1, bad
    assert lib.sc_diag_mmr_select_host(None, G.ctypes.data_as(C.c_void_p), 4, 4, 2, 0.5, picked.ctypes.data_as(C.c_void_p)) == -1


# ------------------------------------------------------------------ store keywords

class MmrIndex(GroupedIndex):
    """... plus search_mmr with the native contract over the stub's IP scores."""

    def search_mmr(self, q, k=10, fetch_k=40, lam=0.5, allow=None):
        n = len(self.X)
        assert 1 <= k <= fetch_k <= 128 and 0.0 <= lam <= 1.0
        if allow is not None:
            words = np.asarray(allow)
            assert words.dtype == np.uint32 and words.ndim == 1 and words.size >= (n + 31) // 32
        allowed = np.ones(n, bool) if allow is None else unpack(allow, n)
        self.calls.append(("search_mmr", len(q), k, fetch_k, lam, None if allow is None else allowed.copy()))
        s, order = self._order(np.asarray(q, np.float32), allowed)
        rows = np.full((len(q), k), -1, np.int64)
        dist = np.full((len(q), k), -np.inf, np.float32)
        for i in range(len(q)):
            cand = [r for r in order[i][:fetch_k] if allowed[r]]
            if not cand:
                continue
            G = (self.X[cand] @ self.X[cand].T).astype(np.float32)
            picked = mmr_ref.select(s[i, cand], G, k, lam)
            rows[i, : len(picked)] = np.asarray(cand)[picked]
            dist[i, : len(picked)] = s[i, np.asarray(cand)[picked]]
        return dist, rows


def filled(n=37, cls=MmrIndex):
    s = MilvusVectorStore(dim=2, index_factory=lambda **kw: cls(kw["dim"]))
    s.connect()
    s.upsert_embeddings([payload(i) for i in range(n)])
    return s


def test_fetch_k_defaults_and_what_reaches_the_index():
    s = filled()
    ix = s._collection
    v = [1.0, 0.0]
    for top_k, want in ((1, 20), (5, 20), (6, 24), (10, 40), (32, 128), (50, 128), (128, 128)):
        s.search(v, top_k=top_k, mmr=0.5)
        assert ix.calls[-1][:5] == ("search_mmr", 1, top_k, want, 0.5) and ix.calls[-1][5] is None
    s.search(v, top_k=3, mmr=0, fetch_k=3)
    assert ix.calls[-1][:5] == ("search_mmr", 1, 3, 3, 0.0)
    s.search_batch(np.array([v, v], np.float32), 4, mmr=1, fetch_k=128)
    assert ix.calls[-1][:5] == ("search_mmr", 2, 4, 128, 1.0)
    # with a filter: the same bitset path as the masked search; every row passing: no bitset
    hits = next(iter(s.search(v, top_k=3, mmr=0.5, repos=["b"], languages="go")))
    assert np.array_equal(ix.calls[-1][5], np.array([r == "b" and l == "go" for r, l in zip(s._repos, s._languages)]))
    assert len(hits) == 3 and all(h.entity.get("repo") == "b" and h.entity.get("language") == "go" for h in hits)
    s.search(v, top_k=3, mmr=0.5, repos=["a", "b", "c"])
    assert ix.calls[-1][5] is None
    assert list(next(iter(s.search(v, top_k=3, mmr=0.5, repos=[])))) == []  # nothing passes: no hits
    assert not [c for c in ix.calls if c[0] in ("search", "search_masked", "search_grouped", "set_groups")]
    # lambda = 1 is the plain order; hits come in selection order
    plain = [h.row for h in next(iter(s.search(v, top_k=5)))]
    assert [h.row for h in next(iter(s.search(v, top_k=5, mmr=1.0)))] == plain
    d, r = s.search_batch(np.array([v], np.float32), 5, mmr=0.0)
    assert r[0, 0] == plain[0] and sorted(r[0].tolist()) != sorted(plain) and d.dtype == np.float32


def test_every_value_error():
    s = filled()
    ix = s._collection
    ix.calls.clear()
    v = [1.0, 0.0]
    q = np.zeros((1, 2), np.float32)
    for call in (lambda **kw: s.search(v, **kw), lambda **kw: s.search_batch(q, **kw)):
        with pytest.raises(ValueError, match="group_by"):
            call(top_k=3, mmr=0.5, group_by="path")
        with pytest.raises(ValueError, match="128"):
            call(top_k=129, mmr=0.5)
        with pytest.raises(ValueError, match="128"):
            call(top_k=3, mmr=0.5, fetch_k=129)
        with pytest.raises(ValueError, match="fetch_k"):
            call(top_k=30, mmr=0.5, fetch_k=20)
        for bad in (-0.01, 1.01, float("nan")):
            with pytest.raises(ValueError, match="mmr"):
                call(top_k=3, mmr=bad)
        with pytest.raises(ValueError, match="mmr"):
            call(top_k=3, fetch_k=20)  # a candidate width without an mmr search
    assert ix.calls == []
    with pytest.raises(TypeError):
        s.search(v, 2, None, None, None, 0.5)  # keyword-only


def test_mmr_none_reaches_the_index_through_todays_call_only():
    s = filled()
    ix = s._collection
    ix.calls.clear()
    q = np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32)
    d0, r0 = s.search_batch(q, 3)
    d1, r1 = s.search_batch(q, 3, mmr=None, fetch_k=None)
    s.search([1.0, 0.0], top_k=3, mmr=None)
    s.search([1.0, 0.0], top_k=3)
    assert ix.calls == [("search", 2, 3, s.nprobe)] * 2 + [("search", 1, 3, s.nprobe)] * 2  # exactly the old calls
    assert np.array_equal(r0, r1) and np.array_equal(d0, d1)


def test_index_without_mmr():
    s = filled(cls=PlainIndex)
    with pytest.raises(NotImplementedError, match="PlainIndex.*search_mmr"):
        s.search([1.0, 0.0], top_k=2, mmr=0.5)
    with pytest.raises(NotImplementedError, match="search_mmr"):
        s.search_batch(np.zeros((1, 2), np.float32), 2, mmr=0.5)
    assert len(next(iter(s.search([1.0, 0.0], top_k=2)))) == 2  # served as before


def test_retriever_forwards_mmr_only_when_given():
    store = RecordingStore(filled())
    r = Retriever(Embedder(), store)
    r.retrieve("abc")
    assert store.calls == [("search", 1, {"top_k": 5})]  # the call of today
    docs = r.retrieve("abc", mmr=0.5)
    assert store.calls[-1] == ("search", 1, {"top_k": 5, "mmr": 0.5}) and len(docs) == 5 and r.last_error is None
    r.retrieve("abc", mmr=0.0, fetch_k=30, repos=["a"])
    assert store.calls[-1] == ("search", 1, {"top_k": 5, "repos": ["a"], "mmr": 0.0, "fetch_k": 30})
    store.calls.clear()
    out = r.retrieve_batch(["a", "bcd"])
    assert store.calls == [("search_batch", 1, {"top_k": 5})]
    out = r.retrieve_batch(["a", "bcd"], mmr=0.25, fetch_k=64)
    assert store.calls[-1] == ("search_batch", 1, {"top_k": 5, "mmr": 0.25, "fetch_k": 64}) and [len(o) for o in out] == [5, 5]
    slow = RecordingStore(filled(), batch=False)
    r2 = Retriever(Embedder(), slow)
    r2.retrieve_batch(["a", "bcd"], mmr=0.5)
    assert slow.calls == [("search", 1, {"top_k": 5, "mmr": 0.5})] * 2
    # the failure protocol: a bad value ends as last_error, not as an exception
    assert r.retrieve("abc", mmr=2.0) == [] and isinstance(r.last_error, ValueError)
    assert r.retrieve("abc", mmr=0.5, group_by="path") == [] and isinstance(r.last_error, ValueError)
    assert len(r.retrieve("abc", mmr=0.5)) == 5 and r.last_error is None


# ------------------------------------------------------------------ ABI

def test_mmr_symbols_declared_and_bound():
    header = (ROOT / "include" / "semcode_hip.h").read_text()
    names = (("sc_index_search_mmr", 10), ("sc_index_search_mmr_dev", 10), ("sc_index_last_mmr_stats", 4), ("sc_diag_mmr_select_host", 7))
    for name, nargs in names:
        m = re.search(r"sc_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/semcode_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
    for attr in ("search_mmr", "search_mmr_dev", "last_mmr_stats"):
        assert hasattr(_native.Index, attr)
    assert "mmr_chunk_q" in header and "8 mmr" in header
    for scope in ("nprobe", "fetch_k > 128", "grouping", "sharded", "other than the index metric", "caching the inverse position map"):
        assert scope in header, scope
    handle = _native.lib()  # the built library exports them
    assert all(hasattr(handle, n) for n, _ in names)
    # one copy of the rule: the kernel file and the host twin include the same header
    csrc = ROOT / "semcode_amd" / "csrc"
    assert '#include "mmr_rule.h"' in (csrc / "scan_mmr.hip").read_text() and '#include "mmr_rule.h"' in (csrc / "sc_mmr.cpp").read_text()
