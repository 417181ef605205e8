"""CPU: host logic of grouped search -- the labels MilvusVectorStore keeps per row for group_by="path" / "repo" and when it hands them to
the index, over a numpy stand-in of the device index that implements set_groups / search_grouped with the native contract; the
Retriever's forwarding; the ABI declarations.  The device side (selection and exclusion kernels, the rounds) is covered by
tests/test_grouped_gpu.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from semcode_amd import _native
from semcode_amd.embeddings.payload import EmbeddingPayload
from semcode_amd.services.retrieval import Retriever
from semcode_amd.storage import MilvusVectorStore

ROOT = Path(__file__).resolve().parent.parent


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


class PlainIndex:
    """Stand-in with the upsert / search / delete surface only: an index_factory object that can neither filter nor group."""

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

    def _order(self, q, allowed):
        s = q @ self.X.T
        s[:, ~allowed] = -np.inf
        return s, np.argsort(-s, axis=1, kind="stable")  # best first, ties by lower row

    def search(self, q, k=10, nprobe=16):
        self.calls.append(("search", len(q), k, nprobe))
        s, order = self._order(q, np.ones(len(self.X), bool))
        rows = np.full((len(q), k), -1, np.int64)
        dist = np.full((len(q), k), -np.inf, np.float32)
        rows[:, : order[:, :k].shape[1]] = order[:, :k]
        dist[:, : order[:, :k].shape[1]] = np.take_along_axis(s, order[:, :k], 1)
        return dist, rows


class GroupedIndex(PlainIndex):
    """... plus the masked and the grouped search with the native contract: labels are valid for the row count they were installed
    for, delete_rows drops them, a grouped search without valid labels is an error."""

    labels = None

    def search_masked(self, q, allow, k=10):
        self.calls.append(("search_masked", len(q), k))
        raise AssertionError("a grouped search must not go through search_masked")

    def delete_rows(self, rows):
        super().delete_rows(rows)
        self.labels = None

    def set_groups(self, labels):
        lab = np.asarray(labels)
        assert lab.dtype == np.int32 and lab.shape == (len(self.X),)
        self.calls.append(("set_groups", lab.copy()))
        self.labels = lab.copy()

    def search_grouped(self, q, k=10, allow=None):
        if self.labels is None or len(self.labels) != len(self.X):
            raise RuntimeError("grouped search: no valid labels")
        n = len(self.X)
        if allow is not None:
            words = np.asarray(allow)
            assert words.dtype == np.uint32 and words.ndim == 1 and words.size >= (n + 31) // 32
        allowed = np.ones(n, bool) if allow is None else unpack(allow, n)
        self.calls.append(("search_grouped", len(q), k, None if allow is None else allowed.copy()))
        s, order = self._order(q, allowed)
        rows = np.full((len(q), k), -1, np.int64)
        dist = np.full((len(q), k), -np.inf, np.float32)
        for i in range(len(q)):
            seen, j = set(), 0
            for r in order[i]:
                if j == k or not allowed[r]:
                    break
                if self.labels[r] not in seen:
                    seen.add(self.labels[r])
                    rows[i, j], dist[i, j] = r, s[i, r]
                    j += 1
        return dist, rows


def make_store(cls=GroupedIndex, dim=2):
    s = MilvusVectorStore(dim=dim, index_factory=lambda **kw: cls(kw["dim"]))
    s.connect()
    return s


REPOS = ["a", "b", "c"]


def payload(i, **over):
    # 4 consecutive chunks per file; the path "src/f0.x" exists in every repo: "path" means the pair (repo, path)
    meta = {"repo": REPOS[(i // 4) % 3], "path": f"src/f{i // 12}.x", "language": "py" if i % 2 else "go", "start_line": i, "end_line": i + 1, "symbol": None}
    meta.update(over)
    return EmbeddingPayload(id=f"id{i}", text=f"text {i}", vector=[float(i), 1.0], metadata=meta)


def filled(n=37, cls=GroupedIndex):
    s = make_store(cls)
    s.upsert_embeddings([payload(i) for i in range(n)])
    return s


def set_groups_calls(s):
    return [c for c in s._collection.calls if c[0] == "set_groups"]


def check_labels(s, labels, group_by):
    """Equal labels <=> equal (repo, path) pairs / repos, over the current rows."""
    keys = list(zip(s._repos, s._paths)) if group_by == "path" else list(s._repos)
    assert labels.dtype == np.int32 and labels.shape == (len(s),)
    seen = {}
    for key, lab in zip(keys, labels.tolist()):
        assert seen.setdefault(key, lab) == lab, (key, lab)
    assert len(set(seen.values())) == len(seen)  # distinct keys, distinct labels


def test_label_codes_are_right():
    s = filled()
    assert next(iter(s.search([1.0, 0.0], top_k=3, group_by="path")))
    calls = set_groups_calls(s)
    assert len(calls) == 1
    check_labels(s, calls[0][1], "path")
    assert len(set(calls[0][1].tolist())) == 10  # 37 rows, 4 per file
    s.search([1.0, 0.0], top_k=3, group_by="repo")
    calls = set_groups_calls(s)
    assert len(calls) == 2
    check_labels(s, calls[1][1], "repo")
    assert len(set(calls[1][1].tolist())) == 3


def test_grouped_hits_one_per_file_and_per_repo():
    s = filled()
    hits = next(iter(s.search([1.0, 0.0], top_k=4, group_by="path")))
    assert [h.row for h in hits] == [36, 35, 31, 27]  # the best chunk of each of the four best files
    assert len({(h.entity.get("repo"), h.entity.get("path")) for h in hits}) == 4
    hits = next(iter(s.search([1.0, 0.0], top_k=5, group_by="repo")))
    assert [h.row for h in hits] == [36, 35, 31] and [h.entity.get("repo") for h in hits] == ["a", "c", "b"]  # three repos: three hits, no padding rows
    # with a filter: through `allow`, a group is represented by its best row that passes
    s._collection.calls.clear()
    hits = next(iter(s.search([1.0, 0.0], top_k=3, group_by="path", repos=["b"], languages="go")))
    assert [h.row for h in hits] == [30, 18, 6]
    call = s._collection.calls[-1]
    assert call[0] == "search_grouped" and call[1:3] == (1, 3)
    assert np.array_equal(call[3], np.array([r == "b" and l == "go" for r, l in zip(s._repos, s._languages)]))
    # a filter that every row passes: no bitset at all
    s.search([1.0, 0.0], top_k=3, group_by="path", repos=REPOS)
    assert s._collection.calls[-1][3] is None
    # a filter that nothing passes: no hits
    assert list(next(iter(s.search([1.0, 0.0], top_k=3, group_by="path", repos=[])))) == []
    # batch form
    d, r = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 2, group_by="repo")
    assert r.tolist() == [[36, 35], [0, 4]] and d.dtype == np.float32
    assert not [c for c in s._collection.calls if c[0] in ("search", "search_masked")]


def test_labels_are_reinstalled_after_every_mutation_and_on_a_switch_and_not_otherwise(tmp_path):
    s = filled()
    v = [1.0, 0.0]
    for _ in range(3):
        s.search(v, top_k=3, group_by="path")
        s.search(v, top_k=2, group_by="path", repos=["a"])  # another filter, the same labels
    assert len(set_groups_calls(s)) == 1
    s.search(v, top_k=3, group_by="repo")
    s.search(v, top_k=3, group_by="repo")
    assert len(set_groups_calls(s)) == 2
    s.search(v, top_k=3, group_by="path")
    assert len(set_groups_calls(s)) == 3
    s.search(v, top_k=3)  # plain and filtered searches in between change nothing
    s.row_filter(repos=["a"])
    s.search(v, top_k=3, group_by="path")
    assert len(set_groups_calls(s)) == 3
    # upsert: an existing row moves to another file, a new row arrives
    s.upsert_embeddings([payload(1, path="other.x"), payload(37)])
    hits = next(iter(s.search(v, top_k=50, group_by="path")))
    calls = set_groups_calls(s)
    assert len(calls) == 4 and len(calls[-1][1]) == 38
    check_labels(s, calls[-1][1], "path")
    assert len(hits) == 11 and 1 in [h.row for h in hits]  # row 1 is now a file of its own
    # delete: the rows behind move up, the index dropped its labels
    assert s.delete_where(repo="a") == 14
    hits = next(iter(s.search(v, top_k=50, group_by="repo")))
    calls = set_groups_calls(s)
    assert len(calls) == 5 and len(calls[-1][1]) == 24 == len(s)
    check_labels(s, calls[-1][1], "repo")
    assert [h.entity.get("repo") for h in hits] == ["c", "b"]
    assert s.delete(["id5", "nope"]) == 1
    s.search(v, top_k=3, group_by="repo")
    assert len(set_groups_calls(s)) == 6
    assert s.delete(["nope"]) == 0  # nothing removed: nothing re-installed
    s.search(v, top_k=3, group_by="repo")
    assert len(set_groups_calls(s)) == 6
    # save -> load: the labels come from the string columns (no codes on disk)
    s.save(tmp_path / "c")
    assert not any((tmp_path / "c").glob("*code*")) and not any((tmp_path / "c").glob("*group*"))
    t = make_store()
    t.load(tmp_path / "c")
    for group_by in ("path", "repo"):
        a = next(iter(s.search(v, top_k=50, group_by=group_by)))
        b = next(iter(t.search(v, top_k=50, group_by=group_by)))
        assert [(h.id, h.distance) for h in a] == [(h.id, h.distance) for h in b] and len(a) > 1
        check_labels(t, set_groups_calls(t)[-1][1], group_by)
    assert len(set_groups_calls(t)) == 2
    # a loaded collection keeps coding new files
    t.upsert_embeddings([EmbeddingPayload(id="new", text="t", vector=[100.0, 1.0], metadata={"repo": "d", "path": "p", "language": "zig"})])
    hits = next(iter(t.search(v, top_k=2, group_by="path")))
    assert hits[0].id == "new" and len(set_groups_calls(t)) == 3
    check_labels(t, set_groups_calls(t)[-1][1], "path")


def test_group_by_none_never_touches_the_new_calls():
    s = filled()
    ix = s._collection
    ix.calls.clear()
    d0, r0 = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 3)
    d1, r1 = s.search_batch(np.array([[1.0, 0.0], [-1.0, 0.0]], np.float32), 3, group_by=None)
    s.search([1.0, 0.0], top_k=3, group_by=None)
    s.search([1.0, 0.0], top_k=3)
    assert ix.calls == [("search", 2, 3, s.nprobe)] * 2 + [("search", 1, 3, s.nprobe)] * 2  # exactly the old calls
    assert np.array_equal(r0, r1) and np.array_equal(d0, d1)
    assert r0[0].tolist() == [36, 35, 34]  # ... which do not group
    s.upsert_embeddings([payload(37)])
    s.delete(["id0"])
    assert not [c for c in ix.calls if c[0] in ("set_groups", "search_grouped")]


def test_index_without_grouping():
    s = filled(cls=PlainIndex)
    with pytest.raises(NotImplementedError, match="PlainIndex.*search_grouped"):
        s.search([1.0, 0.0], top_k=2, group_by="path")
    with pytest.raises(NotImplementedError, match="search_grouped"):
        s.search_batch(np.zeros((1, 2), np.float32), 2, group_by="repo")
    assert len(next(iter(s.search([1.0, 0.0], top_k=2)))) == 2  # ungrouped: served as before


def test_unknown_group_by_is_rejected():
    s = filled()
    s._collection.calls.clear()
    for bad in ("language", "file", "", 3, ("path",)):
        with pytest.raises(ValueError, match="group_by"):
            s.search([1.0, 0.0], top_k=2, group_by=bad)
        with pytest.raises(ValueError, match="group_by"):
            s.search_batch(np.zeros((1, 2), np.float32), 2, group_by=bad)
    assert s._collection.calls == []
    with pytest.raises(TypeError):
        s.search([1.0, 0.0], 2, "path")  # keyword-only


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


def test_retriever_forwards_group_by_only_when_given():
    store = RecordingStore(filled())
    r = Retriever(Embedder(), store)
    docs = r.retrieve("abc")
    assert store.calls == [("search", 1, {"top_k": 5})] and len(docs) == 5 and r.last_error is None  # the call of today
    assert len({(d["repo"], d["path"]) for d in docs}) == 2  # ... whose five sources are two files
    docs = r.retrieve("abc", group_by="path")
    assert store.calls[-1] == ("search", 1, {"top_k": 5, "group_by": "path"})
    assert len(docs) == 5 and len({(d["repo"], d["path"]) for d in docs}) == 5 and r.last_error is None
    docs = r.retrieve("abc", group_by="repo", repos=["a", "b"], languages="py")
    assert store.calls[-1] == ("search", 1, {"top_k": 5, "repos": ["a", "b"], "languages": "py", "group_by": "repo"})
    assert [d["repo"] for d in docs] == ["b", "a"] and all(d["language"] == "py" for d in docs)
    # batch
    store.calls.clear()
    out = r.retrieve_batch(["a", "bcd"])
    assert store.calls == [("search_batch", 1, {"top_k": 5})] and [len(o) for o in out] == [5, 5]
    out = r.retrieve_batch(["a", "bcd"], group_by="path")
    assert store.calls[-1] == ("search_batch", 1, {"top_k": 5, "group_by": "path"})
    assert all(len({(d["repo"], d["path"]) for d in o}) == 5 for o in out)
    # a store without the batch pair: retrieve per question, group_by with it
    slow = RecordingStore(filled(), batch=False)
    r2 = Retriever(Embedder(), slow)
    out = r2.retrieve_batch(["a", "bcd"], group_by="repo")
    assert slow.calls == [("search", 1, {"top_k": 5, "group_by": "repo"})] * 2 and [len(o) for o in out] == [3, 3]
    r2.retrieve_batch(["a"])
    assert slow.calls[-1] == ("search", 1, {"top_k": 5})


def test_retriever_failure_protocol_with_group_by():
    r = Retriever(Embedder(), RecordingStore(filled(), fail=True))
    assert r.retrieve("abc", group_by="path") == [] and isinstance(r.last_error, RuntimeError)
    r.last_error = None
    assert r.retrieve_batch(["a", "b"], group_by="path") == [[], []] and isinstance(r.last_error, RuntimeError)
    # an index that cannot group, an unknown group_by: the same protocol
    r = Retriever(Embedder(), filled(cls=PlainIndex))
    assert r.retrieve("abc", group_by="path") == [] and isinstance(r.last_error, NotImplementedError)
    assert len(r.retrieve("abc")) == 5 and r.last_error is None
    r = Retriever(Embedder(), filled())
    assert r.retrieve("abc", group_by="language") == [] and isinstance(r.last_error, ValueError)
    assert r.retrieve_batch(["abc"], group_by="language") == [[]] and isinstance(r.last_error, ValueError)
    assert len(r.retrieve("abc", group_by="repo")) == 3 and r.last_error is None


# ------------------------------------------------------------------ ABI

def test_grouped_symbols_declared_and_bound():
    header = (ROOT / "include" / "semcode_hip.h").read_text()
    names = (("sc_index_set_groups", 3), ("sc_index_search_grouped", 8), ("sc_index_search_grouped_dev", 8), ("sc_index_last_group_stats", 5))
    for name, nargs in names:
        m = re.search(r"sc_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/semcode_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
    for attr in ("set_groups", "search_grouped", "search_grouped_dev", "last_group_stats"):
        assert hasattr(_native.Index, attr)
    assert "group_width0" in header and "group_width1" in header and "7 grouped" in header
    handle = _native.lib()  # the built library exports them
    assert all(hasattr(handle, n) for n, _ in names)
