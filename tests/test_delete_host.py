"""CPU: host logic of deletes -- MilvusVectorStore.delete / delete_where over a numpy stand-in of the device index that
implements delete_rows, ingest_chunks(prune=...) with a stand-in embedding client, and the ABI declarations.  The device
compaction itself is covered by tests/test_delete_gpu.py."""
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import pytest

from semcode_amd.embeddings.payload import EmbeddingPayload
from semcode_amd.services import ingest_chunks, make_chunk_id
from semcode_amd.settings import settings
from semcode_amd.storage import MilvusVectorStore

ROOT = Path(__file__).resolve().parent.parent


class PlainIndex:
    """Stand-in with the upsert / search surface only: an index_factory object that cannot delete."""

    def __init__(self, dim, **_):
        self.dim = dim
        self.X = np.zeros((0, dim), np.float32)
        self.calls = []

    def add(self, v):
        self.calls.append(("add", len(v)))
        self.X = np.concatenate([self.X, np.asarray(v, np.float32)])

    def put_rows(self, v, rows):
        rows = [int(r) for r in rows]
        self.calls.append(("put_rows", rows))
        for vec, r in zip(np.asarray(v, np.float32), rows):
            if r == len(self.X):
                self.X = np.concatenate([self.X, vec[None]])
            else:
                assert 0 <= r < len(self.X), r
                self.X[r] = vec

    def get_rows(self, first, n):
        return self.X[first:first + n].copy()

    def __len__(self):
        return len(self.X)

    def search(self, q, k=10, nprobe=16):
        s = q @ self.X.T
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
        rows = np.full((len(q), k), -1, np.int64)
        dist = np.full((len(q), k), -np.inf, np.float32)
        rows[:, : order.shape[1]] = order
        dist[:, : order.shape[1]] = np.take_along_axis(s, order, 1)
        return dist, rows


class DeletingIndex(PlainIndex):
    """... plus delete_rows with the native contract: validate first, then remove and renumber densely."""

    fail_delete = False

    def delete_rows(self, rows):
        rows = [int(r) for r in rows]
        self.calls.append(("delete_rows", rows))
        if self.fail_delete:
            raise RuntimeError("device lost")
        if len(set(rows)) != len(rows) or any(r < 0 or r >= len(self.X) for r in rows):
            raise ValueError("bad rows")
        self.X = np.delete(self.X, rows, axis=0)


def make_store(cls=DeletingIndex, dim=2):
    s = MilvusVectorStore(dim=dim, index_factory=lambda **kw: cls(kw["dim"]))
    s.connect()
    return s


def payload(i, repo="demo", path=None, language="python"):
    return EmbeddingPayload(id=f"id{i}", text=f"text {i}", vector=[float(i), 1.0],
                            metadata={"repo": repo, "path": path or f"src/f{i % 3}.py", "language": language, "start_line": i, "end_line": i + 1, "symbol": None})


def filled(cls=DeletingIndex):
    s = make_store(cls)
    s.upsert_embeddings([payload(i, repo="demo" if i < 6 else "lib", language="python" if i % 2 else "go") for i in range(10)])
    return s


def columns(s):
    return list(zip(s._ids, s._texts, s._metadata, s._repos, s._paths, s._languages))


def test_delete_compacts_columns_and_rows():
    s = filled()
    before = columns(s)
    hits = next(iter(s.search([9.0, 0.0], top_k=1)))
    assert hits[0].id == "id9" and hits[0].row == 9
    assert s.delete(["id7", "id2", "nope", "id2", "id0"]) == 3  # unknown and repeated keys are ignored
    assert s._collection.calls[-1] == ("delete_rows", [0, 2, 7])  # one native call, ascending distinct rows
    keep = [1, 3, 4, 5, 6, 8, 9]
    assert len(s) == 7 and columns(s) == [before[r] for r in keep]
    assert s._row_of == {f"id{r}": i for i, r in enumerate(keep)}
    assert np.array_equal(s._collection.X[:, 0], np.array(keep, np.float32))
    hits = next(iter(s.search([9.0, 0.0], top_k=2)))  # Hit.row of the earlier result is stale now: id9 moved to row 6
    assert [(h.id, h.row, h.entity.get("text")) for h in hits] == [("id9", 6, "text 9"), ("id8", 5, "text 8")]
    assert s.delete(["id7", "nope"]) == 0 and s._collection.calls[-1] == ("delete_rows", [0, 2, 7])  # nothing to do: no native call
    # a deleted key can come back: it is appended like any new key
    s.upsert_embeddings([payload(2), payload(9)])
    assert len(s) == 8 and s._row_of["id2"] == 7 and s._row_of["id9"] == 6
    assert s.delete(s._ids[:]) == 8 and len(s) == 0 and s._row_of == {} and len(s._collection) == 0
    s.upsert_embeddings([payload(1)])
    assert len(s) == 1 and s._row_of == {"id1": 0}


def test_delete_where_is_a_conjunction():
    s = filled()
    assert s.keys_where(repo="lib") == ["id6", "id7", "id8", "id9"]
    assert s.delete_where(repo="lib", language="go") == 2 and s._ids == ["id0", "id1", "id2", "id3", "id4", "id5", "id7", "id9"]
    assert s.delete_where(path="src/f0.py") == 3 and s._ids == ["id1", "id2", "id4", "id5", "id7"]
    assert s.delete_where(repo="demo", path="src/f1.py", language="go") == 1 and s._ids == ["id1", "id2", "id5", "id7"]
    assert s.delete_where(repo="other") == 0
    assert s.delete_where(language="python") == 3 and s._ids == ["id2"]
    assert len(s._collection) == 1 and s._row_of == {"id2": 0}
    for call in (lambda: s.delete_where(), lambda: s.keys_where()):
        with pytest.raises(ValueError, match="at least one"):
            call()
    with pytest.raises(TypeError):
        s.delete_where("demo")  # keyword-only: no positional expr
    assert s._ids == ["id2"]


def test_delete_needs_a_connected_store_and_an_index_that_can_delete():
    s = MilvusVectorStore(dim=2, index_factory=lambda **kw: DeletingIndex(kw["dim"]))
    for call in (lambda: s.delete(["x"]), lambda: s.delete_where(repo="r")):
        with pytest.raises(RuntimeError, match="Call connect"):
            call()
    s = filled(PlainIndex)
    before = columns(s)
    for call in (lambda: s.delete(["id1"]), lambda: s.delete([]), lambda: s.delete_where(repo="demo")):
        with pytest.raises(NotImplementedError, match="delete_rows"):
            call()
    assert columns(s) == before and len(s._collection) == 10 and all(c[0] == "put_rows" for c in s._collection.calls)


def test_failed_native_delete_leaves_the_columns():
    s = filled()
    before, row_of = columns(s), dict(s._row_of)
    s._collection.fail_delete = True
    with pytest.raises(RuntimeError, match="device lost"):
        s.delete(["id3"])
    assert columns(s) == before and s._row_of == row_of and len(s._collection) == 10
    s._collection.fail_delete = False
    assert s.delete(["id3"]) == 1 and len(s) == 9


def test_save_load_after_delete(tmp_path):
    s = filled()
    s.delete(["id0", "id4"])
    s.save(tmp_path / "c")
    t = make_store()
    t.load(tmp_path / "c")
    assert columns(t) == columns(s) and t._row_of == s._row_of and np.array_equal(t._collection.X, s._collection.X)


# ------------------------------------------------------------------ ingest_chunks(prune=...)

@dataclass
class Chunk:
    content: str
    path: Path
    language: str
    start_line: int
    end_line: int
    symbol: "str | None" = None


class CountingEmbedding:
    """Stand-in for MI355XEmbeddings on the fused path: tokenize() + embed_ids_into(); vector = [number of characters, first character]."""

    def __init__(self, fail_at=None):
        self.tokenized, self.fail_at, self.pending = [], fail_at, False

    def tokenize(self, texts):
        if self.fail_at is not None and len(self.tokenized) == self.fail_at:
            raise RuntimeError("tokenizer broke")
        self.tokenized.append(len(texts))
        ids = np.zeros((len(texts), 8), np.int32)
        ids[:, 0] = [ord(t[0]) for t in texts]
        return ids, np.array([len(t) for t in texts], np.int32)

    def embed_ids_into(self, store, ids, lens, rows, want_host=False, wait=True):
        store._collection.put_rows(np.stack([lens.astype(np.float32), ids[:, 0].astype(np.float32)], axis=1), rows)
        self.pending = not wait

    def wait(self):
        self.pending = False


def generation(root, shift, count):
    return [Chunk(chr(97 + i % 26) * (i + 1), root / "src" / f"f{i % 7}.py", "python", 10 * i + 1 + shift, 10 * i + 9 + shift) for i in range(count)]


def ids_of(repo, chunks):
    return [make_chunk_id(repo, c.path, c.start_line, c.end_line) for c in chunks]


def test_ingest_prune(monkeypatch):
    monkeypatch.setattr(settings, "mi355x_ingest_batch", 64, raising=False)
    root, lib = Path("/w/demo"), Path("/w/lib")
    gen1, gen2 = generation(root, 0, 130), generation(root, 3, 120)  # a line inserted at the top: every key changes; ten chunks gone
    other = generation(lib, 0, 20)
    for prune in (False, True):
        s, emb, seen = make_store(), CountingEmbedding(), []
        assert ingest_chunks("demo", root, gen1, emb, s) == 130
        assert ingest_chunks("lib", lib, other, emb, s) == 20
        assert ingest_chunks("demo", root, gen2, emb, s, upsert_progress=lambda a, b: seen.append((a, b)), prune=prune) == 120
        assert seen == [(0, 120), (64, 120), (120, 120)] and emb.pending is False  # the protocol and the return value are today's
        if not prune:  # the reference's behaviour, pinned: both generations stay
            assert s._ids == ids_of("demo", gen1) + ids_of("lib", other) + ids_of("demo", gen2)
            assert not any(c[0] == "delete_rows" for c in s._collection.calls)
        else:  # exactly the second generation, the other repository untouched, one native delete after the last batch
            assert s._ids == ids_of("lib", other) + ids_of("demo", gen2)
            assert [c[0] for c in s._collection.calls].count("delete_rows") == 1 and s._collection.calls[-1] == ("delete_rows", list(range(130)))
            assert s._texts == [c.content for c in other + gen2] and len(s._collection) == 140
            assert np.array_equal(s._collection.X[:, 0], [len(c.content) for c in other + gen2])
    # unchanged keys are replaced in place, vanished ones pruned; a re-index of nothing prunes the whole repository
    assert ingest_chunks("demo", root, gen2[:50], emb, s, prune=True) == 50
    assert s._ids == ids_of("lib", other) + ids_of("demo", gen2[:50])
    seen = []
    assert ingest_chunks("demo", root, [], emb, s, upsert_progress=lambda a, b: seen.append((a, b)), prune=True) == 0 and seen == [(0, 0)]
    assert s._ids == ids_of("lib", other)
    assert ingest_chunks("demo", root, [], emb, s) == 0 and len(s) == 20


def test_ingest_that_raises_prunes_nothing(monkeypatch):
    monkeypatch.setattr(settings, "mi355x_ingest_batch", 64, raising=False)
    root = Path("/w/demo")
    gen1, gen2 = generation(root, 0, 130), generation(root, 3, 130)
    s = make_store()
    assert ingest_chunks("demo", root, gen1, CountingEmbedding(), s) == 130
    with pytest.raises(RuntimeError, match="tokenizer broke"):
        ingest_chunks("demo", root, gen2, CountingEmbedding(fail_at=1), s, prune=True)  # the second batch fails
    assert not any(c[0] == "delete_rows" for c in s._collection.calls)
    assert s._ids[:130] == ids_of("demo", gen1) and len(s) == 130 + 64  # the first generation is all there (and one batch of the second)


def test_ingest_prune_needs_an_index_that_can_delete(monkeypatch):
    monkeypatch.setattr(settings, "mi355x_ingest_batch", 64, raising=False)
    root = Path("/w/demo")
    s = make_store(PlainIndex)
    assert ingest_chunks("demo", root, generation(root, 0, 10), CountingEmbedding(), s) == 10
    with pytest.raises(NotImplementedError):
        ingest_chunks("demo", root, generation(root, 3, 10), CountingEmbedding(), s, prune=True)
    assert len(s) == 20  # stored, not pruned


# ------------------------------------------------------------------ ABI

def test_delete_symbols_declared_and_bound():
    from semcode_amd import _native

    header = (ROOT / "include" / "semcode_hip.h").read_text()
    for name, nargs in (("sc_index_delete_rows", 3), ("sc_index_last_delete_stats", 5)):
        m = re.search(r"sc_status\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/semcode_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
    assert "Collection.delete" in header
    assert hasattr(_native.Index, "delete_rows") and hasattr(_native.Index, "last_delete_stats")
