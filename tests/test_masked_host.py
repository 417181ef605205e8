"""CPU: host logic of filtered search -- the bitsets MilvusVectorStore builds for repos / languages filters over a numpy stand-in of
the device index that implements search_masked, their cache, the Retriever's forwarding, and the ABI declarations.  The device side
(mask compaction, gathered scan) is covered by tests/test_masked_gpu.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from semcode_amd import _native
from semcode_amd.embeddings.payload import EmbeddingPayload
from semcode_amd.services.retrieval import Retriever
from semcode_amd.storage import MilvusVectorStore

ROOT = Path(__file__).resolve().parent.parent


class PlainIndex:
    """Stand-in with the upsert / search / delete surface only: an index_factory object that cannot filter."""

    def __init__(self, dim, **_):
        self.dim = dim
        self.X = np.zeros((0, dim), np.float32)
        self.calls = []

    def add(self, v):
        self.X = np.concatenate([self.X, np.asarray(v, np.float32)])

    def put_rows(self, v, rows):
        for vec, r in zip(np.asarray(v, np.float32), [int(r) for r in rows]):
            if r == len(self.X):
                self.X = np.concatenate([self.X, vec[None]])
            else:
                self.X[r] = vec

    def delete_rows(self, rows):
        self.X = np.delete(self.X, [int(r) for r in rows], axis=0)

    def get_rows(self, first, n):
        return self.X[first:first + n].copy()

    def __len__(self):
        return len(self.X)

    def _topk(self, q, k, allowed):
        s = q @ self.X.T
        s[:, ~allowed] = -np.inf
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
        rows = np.full((len(q), k), -1, np.int64)
        dist = np.full((len(q), k), -np.inf, np.float32)
        rows[:, : order.shape[1]] = order
        dist[:, : order.shape[1]] = np.take_along_axis(s, order, 1)
        rows[np.isneginf(dist)] = -1
        return dist, rows

    def search(self, q, k=10, nprobe=16):
        self.calls.append(("search", len(q), k, nprobe))
        return self._topk(q, k, np.ones(len(self.X), bool))


class MaskedIndex(PlainIndex):
    """... plus search_masked with the native contract: uint32 words over row numbers, exact over the allowed rows."""

    def search_masked(self, q, allow, k=10):
        words = np.asarray(allow)
        assert words.dtype == np.uint32 and words.ndim == 1 and words.size >= (len(self.X) + 31) // 32
        self.calls.append(("search_masked", len(q), k, words.copy()))
        return self._topk(q, k, unpack(words, len(self.X)))


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def make_store(cls=MaskedIndex, dim=2):
    s = MilvusVectorStore(dim=dim, index_factory=lambda **kw: cls(kw["dim"]))
    s.connect()
    return s


REPOS = ["a", "b", "c"]
LANGS = ["py", "go"]


def payload(i):
    return EmbeddingPayload(id=f"id{i}", text=f"text {i}", vector=[float(i), 1.0],
                            metadata={"repo": REPOS[i % 3], "path": f"src/f{i}.x", "language": LANGS[(i // 3) % 2], "start_line": i, "end_line": i + 1, "symbol": None})


def filled(n=37, cls=MaskedIndex):  # 37 rows: the last mask word is partial
    s = make_store(cls)
    s.upsert_embeddings([payload(i) for i in range(n)])
    return s


def expected(s, repos=None, languages=None):
    return np.array([(repos is None or r in repos) and (languages is None or l in languages) for r, l in zip(s._repos, s._languages)], bool)


def test_row_filter_builds_the_conjunction_of_disjunctions():
    s = filled()
    n = len(s)
    assert s.row_filter() is None
    for repos, languages in ((["b"], None), (None, ["py"]), (["a", "c"], None), (["b"], {"py"}), (("a", "b"), ["go", "py"]), (["a", "b", "c"], None),
                             (["nope"], None), (["b", "nope"], ["go"]), ([], None), (None, []), (["a"], []), (set(), {"py"})):
        w = s.row_filter(repos=repos, languages=languages)
        assert w.dtype == np.uint32 and w.shape == ((n + 31) // 32,)
        assert np.array_equal(unpack(w, n), expected(s, repos, languages)), (repos, languages)
        assert not unpack(w, 32 * w.size)[n:].any()  # no stray bits in the padding of the last word
    # a string is one name, not a collection of characters
    assert np.array_equal(s.row_filter(repos="b"), s.row_filter(repos=["b"]))
    assert np.array_equal(s.row_filter(languages="py", repos="c"), s.row_filter(repos={"c"}, languages=("py",)))
    with pytest.raises(TypeError):
        s.row_filter(["b"])  # keyword-only


def test_filtered_search_calls_search_masked_and_unfiltered_calls_do_not():
    s = filled()
    ix = s._collection
    ix.calls.clear()
    hits = next(iter(s.search([1.0, 0.0], top_k=4, repos=["b"], languages={"py"})))
    want = [i for i in range(36, -1, -1) if i % 3 == 1 and (i // 3) % 2 == 0][:4]
    assert [h.row for h in hits] == want and all(h.entity.get("repo") == "b" and h.entity.get("language") == "py" for h in hits)
    assert [c[0] for c in ix.calls] == ["search_masked"] and ix.calls[0][1:3] == (1, 4)
    assert np.array_equal(unpack(ix.calls[0][3], len(s)), expected(s, ["b"], ["py"]))
    # no hits: an empty collection of names, unknown names
    for kw in (dict(repos=[]), dict(repos=["nope"]), dict(repos=["a"], languages=["rust"])):
        assert list(next(iter(s.search([1.0, 0.0], top_k=4, **kw)))) == []
    # no keyword, None, or a filter that every row passes: exactly the old call
    ix.calls.clear()
    d0, r0 = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 3)
    d1, r1 = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 3, repos=None, languages=None)
    d2, r2 = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 3, repos=["c", "a", "b"], languages=["go", "py", "zig"])
    s.search([1.0, 0.0], top_k=3)
    assert ix.calls == [("search", 2, 3, s.nprobe)] * 3 + [("search", 1, 3, s.nprobe)]
    assert np.array_equal(r0, r1) and np.array_equal(r0, r2) and np.array_equal(d0, d2)
    # batch form
    d, r = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 2, languages="go")
    assert r.tolist() == [[35, 34], [3, 4]] and ix.calls[-1][0] == "search_masked" and ix.calls[-1][1:3] == (2, 2)


def test_mask_cache_hits_and_is_dropped_by_every_mutation(tmp_path):
    s = filled()
    w = s.row_filter(repos=["b"], languages=["py"])
    assert s.row_filter(repos=("b",), languages={"py"}) is w and s.row_filter(repos="b", languages="py") is w  # one key, one array
    assert s.row_filter(repos=["b"]) is not w
    s.search([1.0, 0.0], top_k=2, repos=["b"], languages=["py"])
    assert s._collection.calls[-1][3].tobytes() == w.tobytes() and len(s._mask_cache) == 2
    # upsert: an existing row changes its repo, a new row arrives
    moved = payload(1)
    moved.metadata = dict(moved.metadata, repo="c")
    s.upsert_embeddings([moved, payload(37)])
    assert s._mask_cache == {}
    w2 = s.row_filter(repos=["b"], languages=["py"])
    assert w2 is not w and np.array_equal(unpack(w2, len(s)), expected(s, ["b"], ["py"])) and not unpack(w2, len(s))[1]
    assert unpack(s.row_filter(repos=["c"]), len(s))[1] and unpack(s.row_filter(repos=["b"]), len(s))[37]
    # delete: the rows behind move up
    assert s.delete_where(repo="a") == 13 and s._mask_cache == {}
    w3 = s.row_filter(repos=["b"], languages=["py"])
    assert w3.shape == ((len(s) + 31) // 32,) and np.array_equal(unpack(w3, len(s)), expected(s, ["b"], ["py"]))
    assert not unpack(s.row_filter(repos=["a"]), len(s)).any()
    hits = next(iter(s.search([1.0, 0.0], top_k=50, repos=["b"])))
    assert len(hits) == int(expected(s, ["b"]).sum()) and all(h.entity.get("repo") == "b" for h in hits)
    # save -> load: the same masks from the string columns (no codes on disk), and load drops what was cached
    s.save(tmp_path / "c")
    assert not any((tmp_path / "c").glob("*code*"))
    t = make_store()
    assert t.row_filter(repos=["b"]).size == 0 and len(t._mask_cache) == 1
    t.load(tmp_path / "c")
    assert t._mask_cache == {}
    for kw in (dict(repos=["b"]), dict(languages=["go"]), dict(repos=["c", "b"], languages=["py"]), dict(repos=["a"])):
        assert np.array_equal(t.row_filter(**kw), s.row_filter(**kw)), kw
    # a loaded collection keeps coding new names
    t.upsert_embeddings([EmbeddingPayload(id="new", text="t", vector=[0.0, 1.0], metadata={"repo": "d", "path": "p", "language": "zig"})])
    assert unpack(t.row_filter(repos=["d"], languages=["zig"]), len(t)).nonzero()[0].tolist() == [len(t) - 1]


def test_index_without_search_masked():
    s = filled(cls=PlainIndex)
    with pytest.raises(NotImplementedError, match="PlainIndex.*search_masked"):
        s.search([1.0, 0.0], top_k=2, repos=["b"])
    with pytest.raises(NotImplementedError, match="search_masked"):
        s.search_batch(np.zeros((1, 2), np.float32), 2, languages=["py"])
    # nothing to filter: served as before
    assert len(next(iter(s.search([1.0, 0.0], top_k=2)))) == 2
    assert len(next(iter(s.search([1.0, 0.0], top_k=2, repos=REPOS)))) == 2
    assert s.row_filter(repos=["b"]) is not None  # the bitset itself needs no device


def test_pack_allow():
    b = np.zeros(37, bool)
    b[[0, 31, 32, 36]] = True
    w = _native.pack_allow(b, 37)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 0x11]
    assert _native.pack_allow(w, 37) is not None and np.array_equal(_native.pack_allow(w, 37), w)
    assert _native.pack_allow(np.zeros(0, bool), 0).size == 0
    for bad in (np.zeros(36, bool), np.zeros(2, np.int64), np.zeros((2, 1), np.uint32)):
        with pytest.raises(ValueError):
            _native.pack_allow(bad, 37)


# ------------------------------------------------------------------ Retriever

class Embedder:
    def embed_query(self, question):
        return [float(len(question)), 0.0]

    def embed_documents_array(self, questions):
        return np.array([[float(len(q)), 0.0] for q in questions], np.float32)


class RecordingStore:
    """The reference's store surface (plus the batch pair), recording how it is called."""

    def __init__(self, inner, batch=True, fail=False):
        self.inner, self.calls, self.fail = inner, [], fail
        if batch:
            self.search_batch = self._search_batch
            self.hits_for = inner.hits_for

    def connect(self):
        pass

    def search(self, *args, **kw):
        self.calls.append(("search", len(args), kw))
        if self.fail:
            raise RuntimeError("device lost")
        return self.inner.search(*args, **kw)

    def _search_batch(self, *args, **kw):
        self.calls.append(("search_batch", len(args), kw))
        if self.fail:
            raise RuntimeError("device lost")
        return self.inner.search_batch(*args, **kw)


def test_retriever_forwards_filters_only_when_given():
    store = RecordingStore(filled())
    r = Retriever(Embedder(), store)
    docs = r.retrieve("abc")
    assert store.calls == [("search", 1, {"top_k": 5})] and len(docs) == 5 and r.last_error is None  # the call of today
    docs = r.retrieve("abc", repos=["b"], languages="py")
    assert store.calls[-1] == ("search", 1, {"top_k": 5, "repos": ["b"], "languages": "py"})
    assert len(docs) == 5 and {(d["repo"], d["language"]) for d in docs} == {("b", "py")}
    r.retrieve("abc", languages=["go"])
    assert store.calls[-1] == ("search", 1, {"top_k": 5, "languages": ["go"]})
    assert r.retrieve("abc", repos=[]) == [] and r.last_error is None  # an empty hit list is a result, as without a filter
    # batch
    store.calls.clear()
    out = r.retrieve_batch(["a", "bcd"])
    assert store.calls == [("search_batch", 1, {"top_k": 5})] and [len(o) for o in out] == [5, 5]
    out = r.retrieve_batch(["a", "bcd"], repos={"c"})
    assert store.calls[-1] == ("search_batch", 1, {"top_k": 5, "repos": {"c"}}) and all(d["repo"] == "c" for o in out for d in o)
    # a store without the batch pair: retrieve per question, the filter with it
    slow = RecordingStore(filled(), batch=False)
    r2 = Retriever(Embedder(), slow)
    out = r2.retrieve_batch(["a", "bcd"], languages="go")
    assert slow.calls == [("search", 1, {"top_k": 5, "languages": "go"})] * 2 and all(d["language"] == "go" for o in out for d in o)
    r2.retrieve_batch(["a"])
    assert slow.calls[-1] == ("search", 1, {"top_k": 5})


def test_retriever_failure_protocol_with_filters():
    r = Retriever(Embedder(), RecordingStore(filled(), fail=True))
    assert r.retrieve("abc", repos=["b"]) == [] and isinstance(r.last_error, RuntimeError)
    r.last_error = None
    assert r.retrieve_batch(["a", "b"], repos=["b"]) == [[], []] and isinstance(r.last_error, RuntimeError)
    # an index that cannot filter: the same protocol
    r = Retriever(Embedder(), filled(cls=PlainIndex))
    assert r.retrieve("abc", repos=["b"]) == [] and isinstance(r.last_error, NotImplementedError)
    assert len(r.retrieve("abc")) == 5 and r.last_error is None


# ------------------------------------------------------------------ ABI

def test_masked_symbols_declared_and_bound():
    header = (ROOT / "include" / "semcode_hip.h").read_text()
    for name, nargs in (("sc_index_search_masked", 8), ("sc_index_search_masked_dev", 8), ("sc_index_last_mask_stats", 4)):
        m = re.search(r"sc_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/semcode_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
    for attr in ("search_masked", "search_masked_dev", "last_mask_stats"):
        assert hasattr(_native.Index, attr)
    assert "mask_gather" in header and "6 masked" in header
    handle = _native.lib()  # the built library exports them
    assert all(hasattr(handle, n) for n in ("sc_index_search_masked", "sc_index_search_masked_dev", "sc_index_last_mask_stats"))
