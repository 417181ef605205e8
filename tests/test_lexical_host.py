"""CPU: the host side of the hybrid search -- the term extractor (sc_lex_terms), the score and fusion rules of csrc/lex_rule.h run on
the CPU (sc_diag_lex_score_host, sc_diag_rrf_host) against the independent restatement in tests/lex_ref.py, and the store's and the
Retriever's host logic over a numpy stand-in of the device index that implements set_terms / lex_stats / search_hybrid with the native
contract.  The device side is covered by tests/test_lexical_gpu.py."""
import numpy as np
import pytest

import lex_ref
from semcode_amd import _native
from semcode_amd.embeddings.payload import EmbeddingPayload
from semcode_amd.services.retrieval import Retriever
from semcode_amd.storage import MilvusVectorStore


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def token_folding_to_pad():
    """A token whose folded hash is 0xFFFF (mapped to 0xFFFE), found by search."""
    for i in range(1 << 22):
        tok = b"id%d" % i
        h = 2166136261
        for c in tok:
            h = ((h ^ c) * 16777619) & 0xFFFFFFFF
        if (h ^ (h >> 16)) & 0xFFFF == 0xFFFF:
            return tok.decode()
    raise AssertionError("no such token among 4M candidates")


FIXED = [
    "camelCase",
    "HTTPServer2",
    "snake_case_name",
    "__init__",
    "def parse_frobnicate_v2(self, x2y): return SC_ERR_NOMEM  # ivf_listmajor_plan",
    "größe = naïveÜber_straße + 数据库Name2 λx",
    "a" * 200,
    "Ab" * 100 + "_" + "x9" * 70,
    "",
    "a b c _ 1 __ _x_ y_",
    "\x00\x01 tab\there\nnew.line;semi-colon/slash",
    " ".join(f"tok{i}Word_{i}" for i in range(90)),  # far more than T tokens
]


def test_extractor_equals_the_python_extractor_on_the_fixed_list():
    texts = FIXED + [f"{token_folding_to_pad()} and again {token_folding_to_pad()}"]
    assert lex_ref.term_hash(token_folding_to_pad().encode()) == 0xFFFE
    for T in (32, 64, 128, 256):
        got, dl = _native.lex_terms(texts, T)
        want, wdl = lex_ref.term_rows(texts, T)
        assert got.dtype == np.uint16 and got.shape == (len(texts), T)
        assert np.array_equal(dl, wdl), (T, dl, wdl)
        assert np.array_equal(got, want), (T, np.flatnonzero((got != want).any(1)))
        assert (np.diff(got.astype(np.int32), axis=1) >= 0).all()  # sorted, padding last
    # the split rules, spelled out
    assert lex_ref.tokens("camelCase") == [b"camelcase", b"camel", b"case"]
    assert lex_ref.tokens("HTTPServer2") == [b"httpserver2", b"httpserver"]
    assert lex_ref.tokens("snake_case_name") == [b"snake_case_name", b"snake", b"case", b"name"]
    assert lex_ref.tokens("__init__") == [b"__init__", b"init"]
    assert lex_ref.tokens("a" * 200) == [b"a" * 64]
    got, dl = _native.lex_terms(["", FIXED[-1]], 32)
    assert dl.tolist() == [0, 32] and (got[0] == 0xFFFF).all() and (got[1] != 0xFFFF).all()
    with pytest.raises(_native.ScError):
        _native.lex_terms(["x"], 48)


def random_rows(rng, n, T, vocab):
    """Sorted term rows with repeats: dl anywhere in 0..T, the first row empty, the second full, the third one term T times."""
    terms = np.full((n, T), 0xFFFF, dtype=np.uint16)
    for r in range(n):
        dl = 0 if r == 0 else T if r in (1, 2) else int(rng.integers(0, T + 1))
        row = np.full(dl, vocab[0]) if r == 2 else rng.choice(vocab, size=dl)
        terms[r, :dl] = np.sort(row)
    return terms


@pytest.mark.parametrize("T", [32, 128, 256])
def test_score_rule_is_bit_equal_to_numpy(T):
    rng = np.random.default_rng(T)
    vocab = np.unique(np.concatenate([[0, 0xFFFE], rng.integers(0, 0xFFFF, size=60)])).astype(np.uint16)
    terms = random_rows(rng, 300, T, vocab)
    for m in (1, 5, 32):
        qt = np.sort(rng.choice(vocab, size=m, replace=False)).astype(np.uint16)
        if m == 32:
            qt[0], qt[-1] = 0, 0xFFFE
            qt = np.unique(np.concatenate([qt, vocab]))[:32].astype(np.uint16)
        qw = (rng.random(qt.size) * 9 + 0.01).astype(np.float32)
        for k1, b, avgdl in ((1.2, 0.75, 37.5), (0.9, 0.4, float(T)), (2.0, 1.0, 1.0), (1.2, 0.0, 3.0)):
            got_s, got_h = _native.diag_lex_score_host(terms, qt, qw, k1, b, avgdl)
            want_s, want_h = lex_ref.score_rows(terms, qt, qw, k1, b, avgdl)
            assert np.array_equal(got_h, want_h)
            assert np.array_equal(bits(got_s), bits(want_s)), (m, k1, b, avgdl)
            assert not got_h[0] and got_s[0] == 0  # the empty row is never a hit
    # the query's rules
    for qt, qw in (([5, 5], [1, 1]), ([7, 5], [1, 1]), ([5, 0xFFFF], [1, 1]), ([5], [0.0]), ([5], [np.inf]), ([5], [np.nan]), ([5], [-1.0]), (list(range(33)), [1.0] * 33)):
        with pytest.raises(_native.ScError):
            _native.diag_lex_score_host(terms, qt, qw, 1.2, 0.75, 10.0)


def test_fusion_rule_equals_numpy():
    rng = np.random.default_rng(5)
    cases = []
    for F in (1, 7, 40, 128):
        pool = rng.permutation(4 * F + 5)
        dense = pool[:F].astype(np.int64)
        lex = np.concatenate([pool[F // 2: F // 2 + F // 2], pool[2 * F: 2 * F + F - F // 2]]).astype(np.int64)  # half shared, half its own
        rng.shuffle(lex)
        cases.append((dense, lex))
        short = lex.copy()
        short[F // 3:] = -1  # the lexical list ran out
        cases.append((dense, short))
        cases.append((np.full(F, -1, np.int64), lex))  # no dense hit at all
    # exact ties: a row only in the dense list at rank i and one only in the lexical list at rank i, equal weights -> the lower row first
    cases.append((np.array([9, 4, 7, 2], np.int64), np.array([3, 8, 1, 6], np.int64)))
    cases.append((np.array([-1, -1], np.int64), np.array([-1, -1], np.int64)))
    for dense, lex in cases:
        F = dense.size
        for k in sorted({1, min(3, F), F}):
            for c, wd, wl in ((60, 1.0, 1.0), (1, 0.3, 0.7), (60, 1.0, 0.0), (7, 0.0, 2.5)):
                got = _native.diag_rrf_host(dense, lex, k, c, wd, wl)
                want = lex_ref.rrf(dense, lex, k, c, wd, wl)
                assert np.array_equal(got[1], want[1]), (dense, lex, k, c, wd, wl, got[1], want[1])
                assert np.array_equal(bits(got[0]), bits(want[0]))
    s, r = _native.diag_rrf_host([9, 4, 7, 2], [3, 8, 1, 6], 4)
    assert r.tolist() == [3, 9, 4, 8] and s[0] == s[1] and s[2] == s[3]
    for bad in (dict(c=0), dict(dense_weight=-1.0), dict(lexical_weight=float("nan"))):
        with pytest.raises(_native.ScError):
            _native.diag_rrf_host([1], [2], 1, **bad)
    with pytest.raises(_native.ScError):
        _native.diag_rrf_host([1, 2], [2, 3], 3)


# ---------------------------------------------------------------- store and retriever over a stand-in index
class LexIndex:
    """numpy stand-in of the device index with the native contract of the term rows: installed by range, first_row at most the rows held,
    valid while their count equals the index's, dropped by delete_rows; search_hybrid through tests/lex_ref.py."""

    def __init__(self, dim, **_):
        self.dim = dim
        self.X = np.zeros((0, dim), np.float32)
        self.terms = None
        self.calls = []

    def put_rows(self, v, rows):
        for vec, r in zip(np.asarray(v, np.float32), [int(r) for r in rows]):
            if r == len(self.X):
                self.X = np.concatenate([self.X, vec[None]])
            else:
                self.X[r] = vec

    def add(self, v):
        self.X = np.concatenate([self.X, np.asarray(v, np.float32)])

    def delete_rows(self, rows):
        self.X = np.delete(self.X, [int(r) for r in rows], axis=0)
        self.terms = None

    def get_rows(self, first, n):
        return self.X[first:first + n].copy()

    def __len__(self):
        return len(self.X)

    def search(self, q, k=10, nprobe=16):
        self.calls.append(("search", len(q), k))
        s = q @ self.X.T
        order = np.argsort(-s, axis=1, kind="stable")[:, :k]
        rows = np.full((len(q), k), -1, np.int64)
        dist = np.full((len(q), k), -np.inf, np.float32)
        rows[:, : order.shape[1]] = order
        dist[:, : order.shape[1]] = np.take_along_axis(s, order, 1)
        return dist, rows

    def set_terms(self, terms, first_row=0):
        t = np.asarray(terms)
        assert t.dtype == np.uint16 and t.ndim == 2
        held = 0 if self.terms is None else len(self.terms)
        assert first_row <= held and first_row + len(t) <= len(self.X)
        assert self.terms is None or t.shape[1] == self.terms.shape[1]
        self.calls.append(("set_terms", first_row, len(t)))
        base = np.zeros((0, t.shape[1]), np.uint16) if self.terms is None else self.terms
        self.terms = np.concatenate([base[:first_row], t, base[first_row + len(t):]])

    def drop_terms(self):
        self.terms = None

    def lex_stats(self):
        assert self.terms is not None and len(self.terms) == len(self.X), "no valid term rows"
        self.calls.append(("lex_stats",))
        n, total, df = lex_ref.stats(self.terms)
        return {"rows": n, "sum_dl": total, "df": df}

    def search_hybrid(self, q, qterms, qweights, nterms, k=10, fetch_k=40, k1=1.2, b=0.75, avgdl=1.0, c=60, dense_weight=1.0, lexical_weight=1.0, allow=None):
        assert self.terms is not None and len(self.terms) == len(self.X), "no valid term rows"
        self.calls.append(("search_hybrid", dict(k=k, fetch_k=fetch_k, k1=k1, b=b, avgdl=avgdl, c=c, dense_weight=dense_weight, lexical_weight=lexical_weight,
                                                 allow=None if allow is None else np.asarray(allow).copy(), qterms=np.asarray(qterms).copy(),
                                                 qweights=np.asarray(qweights).copy(), nterms=np.asarray(nterms).copy())))
        n = len(self.X)
        ok = np.ones(n, bool) if allow is None else np.unpackbits(np.ascontiguousarray(allow).view(np.uint8), bitorder="little")[:n].astype(bool)
        s = q @ self.X.T
        s[:, ~ok] = -np.inf
        S, R = np.empty((len(q), k), np.float32), np.empty((len(q), k), np.int64)
        _, lex_rows = lex_ref.search(self.terms, qterms, qweights, nterms, fetch_k, k1, b, avgdl, ok)
        for i in range(len(q)):
            order = np.argsort(-s[i], kind="stable")
            dense = np.full(fetch_k, -1, np.int64)
            good = order[ok[order]][:fetch_k]
            dense[: good.size] = good
            S[i], R[i] = lex_ref.rrf(dense, lex_rows[i], k, c, dense_weight, lexical_weight)
        return S, R


class NoLexIndex(LexIndex):
    set_terms = drop_terms = lex_stats = search_hybrid = None

    def __getattribute__(self, name):
        if name in ("set_terms", "drop_terms", "lex_stats", "search_hybrid"):
            raise AttributeError(name)
        return super().__getattribute__(name)


DIM = 8


def payloads(rng, n, start=0, repo=lambda i: f"r{i % 3}"):
    out = []
    for i in range(start, start + n):
        text = f"def handler_{i % 7}(request): return computeValue{i % 5}(request) + shared_token"
        out.append(EmbeddingPayload(id=f"k{i}", vector=rng.standard_normal(DIM).astype(np.float32).tolist(), text=text,
                                    metadata={"repo": repo(i), "path": f"p{i}.py", "language": "python"}))
    return out


def make_store(factory=LexIndex, **kw):
    store = MilvusVectorStore("t", DIM, metric="IP", index_type="FLAT", index_factory=factory, **kw)
    store.connect()
    return store


def host_matrix(store):
    return store._terms[: len(store)]


def test_store_keeps_the_host_matrix_through_upsert_overwrite_delete_and_load(tmp_path):
    rng = np.random.default_rng(0)
    store = make_store(lexical=True, lex_slots=32)
    ix = store._collection
    store.upsert_embeddings(payloads(rng, 300))
    want = lex_ref.term_rows(store._texts, 32)[0]
    assert np.array_equal(host_matrix(store), want) and np.array_equal(ix.terms, want)
    # appends upload their own range only (batches of 128)
    assert [c[1:] for c in ix.calls if c[0] == "set_terms"] == [(0, 128), (128, 128), (256, 44)]
    # overwrite two rows: the range between them
    ix.calls.clear()
    over = payloads(rng, 1, start=10) + payloads(rng, 1, start=12)
    over[0].text, over[1].text = "renamedIdentifierOne", "renamed_identifier_two"
    store.upsert_embeddings(over)
    assert [c[1:] for c in ix.calls if c[0] == "set_terms"] == [(10, 3)]
    want = lex_ref.term_rows(store._texts, 32)[0]
    assert np.array_equal(host_matrix(store), want) and np.array_equal(ix.terms, want)
    # delete: the same renumbering, then the whole matrix again
    ix.calls.clear()
    assert store.delete(["k0", "k11", "k299"]) == 3
    want = lex_ref.term_rows(store._texts, 32)[0]
    assert len(store) == 297 and np.array_equal(host_matrix(store), want) and np.array_equal(ix.terms, want)
    assert [c[1:] for c in ix.calls if c[0] == "set_terms"] == [(0, 297)]
    # save / load: the on-disk format holds no term rows; they are rebuilt from the texts
    store.save(tmp_path / "c")
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == ["columns.jsonl", "manifest.json", "vectors.f32"]
    again = make_store(lexical=True, lex_slots=32)
    again.load(tmp_path / "c")
    assert np.array_equal(host_matrix(again), want) and np.array_equal(again._collection.terms, want)
    # a store without lexical= keeps nothing and uploads nothing
    plain = make_store()
    plain.upsert_embeddings(payloads(rng, 5))
    assert plain._terms.shape[0] == 0 and plain._collection.terms is None


def test_store_argument_validation_and_conflicts():
    rng = np.random.default_rng(1)
    store = make_store(lexical=True)
    store.upsert_embeddings(payloads(rng, 40))
    q = rng.standard_normal(DIM).astype(np.float32)
    with pytest.raises(ValueError, match="query text"):
        store.search(q, 5, hybrid=True)
    with pytest.raises(ValueError, match="group_by"):
        store.search(q, 5, hybrid=True, query_text="x", group_by="path")
    with pytest.raises(ValueError, match="mmr"):
        store.search(q, 5, hybrid=True, query_text="x", mmr=0.5)
    with pytest.raises(ValueError, match="unknown keys"):
        store.search(q, 5, hybrid={"k": 1}, query_text="x")
    for bad in ({"c": 0}, {"c": 1.5}, {"dense_weight": -1}, {"lexical_weight": float("inf")}):
        with pytest.raises(ValueError, match="hybrid"):
            store.search(q, 5, hybrid=bad, query_text="x")
    with pytest.raises(ValueError, match="hybrid must be"):
        store.search(q, 5, hybrid="yes", query_text="x")
    with pytest.raises(ValueError, match="fetch_k=3 is smaller"):
        store.search(q, 5, hybrid=True, query_text="x", fetch_k=3)
    with pytest.raises(ValueError, match="fetch_k <= 128"):
        store.search(q, 5, hybrid=True, query_text="x", fetch_k=129)
    with pytest.raises(ValueError, match="top_k <= 128"):
        store.search(q, 129, hybrid=True, query_text="x")
    with pytest.raises(ValueError, match="query texts"):
        store.search_batch(np.stack([q, q]), 5, hybrid=True, query_texts=["only one"])
    with pytest.raises(ValueError, match="give mmr as well"):
        store.search(q, 5, fetch_k=20)  # (unchanged: fetch_k alone)
    with pytest.raises(ValueError, match="lex_slots"):
        MilvusVectorStore("t", DIM, lexical=True, lex_slots=100)
    plain = make_store()
    plain.upsert_embeddings(payloads(rng, 5))
    with pytest.raises(ValueError, match="lexical=True"):
        plain.search(q, 5, hybrid=True, query_text="x")
    # hybrid=None / False: today's call, the text is ignored
    store._collection.calls.clear()
    store.search(q, 5, query_text="ignored", hybrid=False)
    assert [c[0] for c in store._collection.calls] == ["search"]
    # an index object without the lexical surface
    bare = make_store(NoLexIndex, lexical=True)
    bare.upsert_embeddings(payloads(rng, 5))
    with pytest.raises(NotImplementedError, match="search_hybrid"):
        bare.search(q, 5, hybrid=True, query_text="x")


def test_store_query_terms_weights_and_forwarding(monkeypatch):
    rng = np.random.default_rng(2)
    store = make_store(lexical=True, lex_slots=64)
    ix = store._collection
    store.upsert_embeddings(payloads(rng, 200))
    n, total, df = lex_ref.stats(ix.terms)
    q = rng.standard_normal((2, DIM)).astype(np.float32)
    texts = ["where is handler_3 defined", " ".join(f"word{i}" for i in range(50)) + " shared_token computeValue2"]
    ix.calls.clear()
    dist, rows = store.search_batch(q, 7, query_texts=texts, hybrid={"c": 10, "lexical_weight": 2.0}, repos=["r0", "r1"])
    call = [c for c in ix.calls if c[0] == "search_hybrid"][0][1]
    assert (call["k"], call["fetch_k"], call["c"], call["dense_weight"], call["lexical_weight"]) == (7, 28, 10, 1.0, 2.0)
    assert (call["k1"], call["b"]) == (1.2, 0.75) and np.float32(call["avgdl"]) == np.float32(total / n)
    allowed = np.unpackbits(call["allow"].view(np.uint8), bitorder="little")[:n].astype(bool)
    assert np.array_equal(allowed, np.isin(np.asarray(store._repos), ["r0", "r1"]))
    for i, text in enumerate(texts):
        qt, qw, m = lex_ref.query_terms(text, df, n, 64)
        assert call["nterms"][i] == m and np.array_equal(call["qterms"][i], qt) and np.array_equal(bits(call["qweights"][i]), bits(qw))
    assert call["nterms"].tolist() == [min(32, len({lex_ref.term_hash(t) for t in lex_ref.tokens(t_)[:64]})) for t_ in texts] and call["nterms"][1] == 32
    # the 32 kept are those of highest idf: every dropped term is at least as common
    kept = set(call["qterms"][1].tolist())
    dropped = {lex_ref.term_hash(t) for t in lex_ref.tokens(texts[1])[:64]} - kept
    assert dropped and max(df[list(kept)]) <= min(df[list(dropped)])
    # results are the stand-in's, hits carry the fused score
    hits = store.search(q[0], 7, query_text=texts[0], hybrid={"c": 10, "lexical_weight": 2.0}, repos=["r0", "r1"])[0]
    assert [h.row for h in hits] == [r for r in rows[0].tolist() if r >= 0] and hits[0].distance == pytest.approx(float(dist[0][0]))
    assert all("handler_3" in h.entity.get("text") for h in hits[:3])
    # the df table is fetched once per mutation
    ix.calls.clear()
    store.search(q[0], 5, query_text="handler_1", hybrid=True)
    assert "lex_stats" not in [c[0] for c in ix.calls]
    store.upsert_embeddings(payloads(rng, 1, start=500))
    store.search(q[0], 5, query_text="handler_1", hybrid=True)
    assert [c[0] for c in ix.calls].count("lex_stats") == 1


class FakeEmbedder:
    def embed_query(self, text):
        return np.ones(DIM, np.float32).tolist()

    def embed_documents_array(self, texts):
        return np.ones((len(texts), DIM), np.float32)


def test_retriever_passes_the_question_text_along():
    rng = np.random.default_rng(3)
    store = make_store(lexical=True)
    store.upsert_embeddings(payloads(rng, 60))
    ix = store._collection
    r = Retriever(FakeEmbedder(), store)
    ix.calls.clear()
    docs = r.retrieve("where is handler_4 defined", hybrid={"lexical_weight": 10.0})  # (every chunk holds "handler": the lexical leg must outweigh the dense one here)
    assert r.last_error is None and docs and "handler_4" in docs[0]["snippet"]
    assert [c[0] for c in ix.calls if c[0].startswith("search")] == ["search_hybrid"]
    ix.calls.clear()
    batch = r.retrieve_batch(["where is handler_4 defined", "computeValue3"], hybrid={"c": 5, "lexical_weight": 10.0})
    assert r.last_error is None and "handler_4" in batch[0][0]["snippet"] and "computeValue3" in batch[1][0]["snippet"]
    call = [c for c in ix.calls if c[0] == "search_hybrid"]
    assert len(call) == 1 and call[0][1]["c"] == 5 and len(call[0][1]["nterms"]) == 2
    # without hybrid the store is called exactly as before
    ix.calls.clear()
    r.retrieve("where is handler_4 defined")
    r.retrieve_batch(["a", "b"])
    assert [c[0] for c in ix.calls] == ["search", "search"]
    # a conflict comes back through the error protocol
    assert r.retrieve("x", hybrid=True, mmr=0.5) == [] and isinstance(r.last_error, ValueError)


def test_settings_switch(monkeypatch):
    from semcode_amd import settings as st

    assert st.Settings().mi355x_lexical is False
    monkeypatch.setenv("SEMCODE_MI355X_LEXICAL", "1")
    assert st.Settings().mi355x_lexical is True
    monkeypatch.setattr(st, "settings", st.Settings())
    assert MilvusVectorStore("t", DIM).lexical is True and MilvusVectorStore("t", DIM, lexical=False).lexical is False
