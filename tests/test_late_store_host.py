"""CPU: the token store without a GPU -- the host search (sc_diag_late_search_host) against a restatement that calls the pairwise host
rule (sc_diag_maxsim_host) and sorts in numpy, the install-time bf16 rounding (sc_diag_round_bf16) against numpy's round-to-nearest-even
on the upper 16 bits, the argument checks of every new entry point, which come back before anything is touched, and the wiring of
Retriever and MilvusVectorStore around the store on fakes (when the stored vectors score, when score_pairs still does, what raises)."""
import ctypes as C

import numpy as np
import pytest

import late_store_ref as ls
from semcode_amd import _native


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error():
    buf = C.create_string_buffer(1024)
    _native.lib().sc_last_error(buf, 1024)
    return buf.value.decode()


def make_docs(rng, n, W, counts=(0, 1, 15, 16, 17, 40), grid=None):
    draw = (lambda m: ls.unit_rows(rng, m, W)) if grid is None else (lambda m: (rng.integers(-grid, grid + 1, (m, W)) / np.float32(grid)).astype(np.float32))
    docs = []
    for _ in range(n):
        m = int(rng.choice(counts))
        docs.append(draw(m) if m else None)
    return docs


@pytest.mark.parametrize("W", [16, 96, 128])
def test_host_search_equals_the_restatement(W):
    rng = np.random.default_rng(W)
    docs = make_docs(rng, 90, W)
    for r in range(5, 90, 9):  # exact duplicates of other rows, spread over the range: ties that only the row number breaks
        docs[r] = None if docs[r - 5] is None else docs[r - 5].copy()
    questions = [ls.unit_rows(rng, nq, W) for nq in (1, 17, 32, 128)]
    scores = ls.pair_scores(questions, docs, W)
    with_tokens = int((~np.isnan(scores[0])).sum())
    assert 0 < with_tokens < 90
    allow = rng.random(90) < 0.5
    for k in (1, 7, 128):  # 128 > rows with tokens: padding
        for a in (None, allow):
            got_s, got_r = _native.diag_late_search_host(questions, docs, k, allow=a)
            want_s, want_r = ls.search_restated(scores, k, a)
            assert np.array_equal(got_r, want_r) and ls.same_bits(got_s, want_s), (W, k, a is not None)
    assert (got_r[:, with_tokens:] == -1).all() and np.isneginf(got_s[:, with_tokens:]).all()
    # a shorter list is the head of a longer one
    s128, r128 = _native.diag_late_search_host(questions, docs, 128)
    s10, r10 = _native.diag_late_search_host(questions, docs, 10)
    assert np.array_equal(r10, r128[:, :10]) and ls.same_bits(s10, s128[:, :10])


def test_host_search_cuts_ties_by_row_number():
    rng = np.random.default_rng(3)
    W = 16
    base = [ls.unit_rows(rng, m, W) for m in (3, 17, 1)]
    docs = [base[i % 3].copy() for i in range(30)]  # ten copies of three documents: tie groups of ten
    docs[4] = None
    docs[11] = None
    questions = [ls.unit_rows(rng, 5, W), ls.unit_rows(rng, 20, W)]
    scores = ls.pair_scores(questions, docs, W)
    for k in (1, 4, 10, 15, 28, 40):  # cuts inside a tie group, at its end, beyond the rows that have tokens
        got_s, got_r = _native.diag_late_search_host(questions, docs, k)
        want_s, want_r = ls.search_restated(scores, k)
        assert np.array_equal(got_r, want_r) and ls.same_bits(got_s, want_s), k
    s, r = _native.diag_late_search_host(questions, docs, 10)
    for q in range(2):
        assert len(set(s[q, :9].tolist())) == 1 and (np.diff(r[q, :9]) > 0).all()  # one tie group (nine rows left of ten), ascending rows
    # one row allowed, none allowed
    one = np.zeros(30, bool)
    one[13] = True
    s, r = _native.diag_late_search_host(questions, docs, 3, allow=one)
    assert r[:, 0].tolist() == [13, 13] and (r[:, 1:] == -1).all() and ls.same_bits(s[:, 0], scores[:, 13])
    s, r = _native.diag_late_search_host(questions, docs, 3, allow=np.zeros(30, bool))
    assert (r == -1).all() and np.isneginf(s).all()
    # documents of zeros of either sign: every chain starts from +0, so both score +0 -- a tie that the row number cuts
    z = [np.zeros((2, W), np.float32), -np.zeros((2, W), np.float32)]
    s, r = _native.diag_late_search_host([np.full((1, W), 1.0, np.float32), np.full((1, W), -1.0, np.float32)], z, 2)
    want_s, want_r = ls.search_restated(ls.pair_scores([np.full((1, W), 1.0, np.float32), np.full((1, W), -1.0, np.float32)], z, W), 2)
    assert np.array_equal(r, want_r) and ls.same_bits(s, want_s)


def numpy_round_bf16(x: np.ndarray) -> np.ndarray:
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def test_round_bf16_is_round_to_nearest_even_on_the_upper_half():
    rng = np.random.default_rng(1)
    special = np.array([0x00000000, 0x80000000,              # +-0
                        0x3F808000, 0x3F818000, 0xBF808000,  # halfway: down to the even 0x3F80, up to the even 0x3F82, the same with a sign
                        0x3F807FFF, 0x3F808001,              # either side of halfway
                        0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001,  # subnormals, halfway ones included
                        0x00800000, 0x7F7F0000, 0x7F7F7FFF,  # smallest normal, large finite values that stay finite
                        0x7F800000, 0xFF800000], np.uint32).view(np.float32)
    x = np.concatenate([special, rng.standard_normal(4096).astype(np.float32), rng.integers(0, 0x7F000000, 4096).astype(np.uint32).view(np.float32),
                        (rng.integers(0, 0x7F00, 2048).astype(np.uint32) << 16 | 0x8000).view(np.float32)])  # many exact halfway cases, all finite
    got = _native.diag_round_bf16(x)
    assert np.array_equal(got.view(np.uint32), numpy_round_bf16(x).view(np.uint32))
    assert (got.view(np.uint32) & 0xFFFF == 0).all()
    assert np.array_equal(_native.diag_round_bf16(got).view(np.uint32), got.view(np.uint32))  # stored values are fixed points
    assert got[0].view(np.uint32) == 0 and got[1].view(np.uint32) == 0x80000000
    assert np.isnan(_native.diag_round_bf16(np.array([np.nan], np.float32))[0])


def test_host_entry_points_refuse_bad_arguments():
    lib = _native.lib()
    W = 16
    Q = np.zeros((4, W), np.float32)
    q_off = np.array([0, 4], np.int32)
    D = np.zeros((3, W), np.float32)
    d_off = np.array([0, 1, 3], np.int64)
    s, r = np.zeros(4, np.float32), np.zeros(4, np.int64)

    def rc(**k):
        a = dict(Q=Q, q_off=q_off, Bq=1, D=D, d_off=d_off, n=2, W=W, k=4, allow=None, words=0, s=s, r=r)
        a.update(k)
        return lib.sc_diag_late_search_host(_p(a["Q"]), _p(a["q_off"]), a["Bq"], _p(a["D"]), _p(a["d_off"]), a["n"], a["W"], a["k"], _p(a["allow"]), a["words"], _p(a["s"]),
                                            _p(a["r"]))

    assert rc() == 0
    for kw, needle in ((dict(Q=None), "NULL"), (dict(W=24), "multiple of 16"), (dict(W=144), "multiple of 16"), (dict(k=0), "top_k"), (dict(k=129), "top_k"),
                       (dict(Bq=0), "Bq"), (dict(q_off=np.array([1, 4], np.int32)), "start at 0"), (dict(q_off=np.array([0, 0], np.int32)), "token vectors"),
                       (dict(q_off=np.array([0, 129], np.int32)), "token vectors"), (dict(d_off=np.array([0, 2, 1], np.int64)), "tokens"),
                       (dict(d_off=np.array([0, 1, 2051], np.int64)), "tokens"), (dict(words=1), "allow_words"), (dict(allow=np.zeros(1, np.uint32), words=0), "allow_words")):
        assert rc(**kw) == -1 and "sc_diag_late_search_host" in last_error() and needle in last_error(), (list(kw), last_error())
    assert lib.sc_diag_round_bf16(None, 3, _p(s)) == -1 and "sc_diag_round_bf16" in last_error()
    assert lib.sc_diag_round_bf16(_p(s), -1, _p(s)) == -1
    # the index entry points check the handle before anything else: a NULL index is refused, nothing is dereferenced
    one = np.zeros(1, np.int64)
    cnt = np.ones(1, np.int32)
    assert lib.sc_index_put_tokens(None, _p(one), 1, _p(cnt), _p(Q), W, 0) == -1
    assert lib.sc_index_reserve_tokens(None, 10) == -1 and lib.sc_index_compact_tokens(None) == -1 and lib.sc_index_drop_tokens(None) == -1
    assert lib.sc_index_get_tokens(None, _p(one), 1, _p(cnt), None, 0) == -1
    assert lib.sc_index_token_stats(None, None, None, None, None, None, None) == -1
    assert lib.sc_index_rerank_late(None, _p(Q), _p(q_off), 1, _p(one), 1, _p(s)) == -1
    assert lib.sc_index_search_late(None, _p(Q), _p(q_off), 1, 4, None, 0, _p(s), _p(r)) == -1


def test_python_packers_refuse_mixed_widths_and_wrong_counts():
    with pytest.raises(ValueError):
        _native.pack_token_lists([np.zeros((2, 16), np.float32), np.zeros((2, 32), np.float32)])
    with pytest.raises(ValueError):
        _native.pack_token_lists((np.array([2, 2], np.int32), np.zeros((3, 16), np.float32)))
    counts, vecs = _native.pack_token_lists([np.zeros((2, 16), np.float32), None, np.zeros((0, 16), np.float32), np.ones((1, 16), np.float32)])
    assert counts.tolist() == [2, 0, 0, 1] and vecs.shape == (3, 16)
    Q, q_off = _native.pack_questions([np.zeros((2, 16), np.float32), np.zeros((5, 16), np.float32)])
    assert q_off.tolist() == [0, 2, 7] and Q.shape == (7, 16)


# ---------------------------------------------------------------- Retriever and the store's wiring, on fakes
class FakeHit:
    def __init__(self, row, score):
        from semcode_amd.storage.milvus_store import _Entity

        self.row, self.score = row, score
        self.entity = _Entity({"repo": "r", "path": f"p{row}", "language": "py", "text": f"text {row}", "metadata": {}})


class FakeStore:
    """search returns rows 0 .. k - 1 with falling scores; rerank_late scores a row by -|row - 3|; rows in `bare` have no tokens."""

    def __init__(self, bare=()):
        self.bare, self.calls = set(bare), []

    def connect(self):
        pass

    def search(self, vector, top_k=10, **kw):
        self.calls.append(("search", top_k, kw))
        return [[FakeHit(r, 1.0 - 0.01 * r) for r in range(top_k)]]

    def has_late_tokens(self, rows):
        return not (set(int(r) for r in rows) & self.bare)

    def rerank_late(self, question_vectors, rows):
        self.calls.append(("rerank_late", np.asarray(rows).shape))
        return -np.abs(np.asarray(rows, np.float32) - 3)

    def search_late(self, question_vectors, top_k=10, **kw):
        self.calls.append(("search_late", top_k, kw))
        return np.tile(np.arange(top_k, 0, -1, dtype=np.float32), (len(question_vectors), 1)), np.tile(np.arange(top_k), (len(question_vectors), 1))

    def hits_for(self, dist, rows):
        return [[FakeHit(int(r), float(d)) for d, r in zip(ds, rs)] for ds, rs in zip(dist, rows)]


class FakeLate:
    def __init__(self):
        self.pairs = self.queries = 0

    def embed_query_tokens(self, texts):
        self.queries += 1
        return [np.zeros((32, 16), np.float32) for _ in texts]

    def score_pairs(self, questions, passages):
        self.pairs += 1
        return np.array([-abs(int(p.split()[1]) - 3) for p in passages], np.float32)


class FakeEmb:
    def embed_query(self, q):
        return [0.0, 1.0]


def test_retriever_scores_from_the_store_only_when_every_candidate_has_tokens(monkeypatch):
    from semcode_amd.services import Retriever
    from semcode_amd.settings import settings

    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    store, late = FakeStore(), FakeLate()
    r = Retriever(FakeEmb(), store, reranker=late)
    docs = r.retrieve("q", rerank=True, fetch_k=8)
    assert [d["path"] for d in docs] == ["p3", "p2", "p4"] and [d["score"] for d in docs] == [0.0, -1.0, -1.0] and r.last_error is None
    assert (late.pairs, late.queries) == (0, 1) and ("rerank_late", (1, 8)) in store.calls
    assert docs[0]["retrieval_score"] == pytest.approx(0.97)
    # one candidate without tokens: score_pairs as before, the same result
    store2, late2 = FakeStore(bare={5}), FakeLate()
    assert Retriever(FakeEmb(), store2, reranker=late2).retrieve("q", rerank=True, fetch_k=8) == docs
    assert (late2.pairs, late2.queries) == (1, 0) and not any(c[0] == "rerank_late" for c in store2.calls)
    # a cross-encoder (no embed_query_tokens) never touches the store's tokens
    class Cross:
        def score_pairs(self, qs, ps):
            return np.zeros(len(ps), np.float32)

    store3 = FakeStore()
    Retriever(FakeEmb(), store3, reranker=Cross()).retrieve("q", rerank=True, fetch_k=8)
    assert not any(c[0] == "rerank_late" for c in store3.calls)
    # late=True: the MaxSim search is the retrieval; filters go along; conflicts raise before anything runs
    store4, late4 = FakeStore(), FakeLate()
    r4 = Retriever(FakeEmb(), store4, reranker=late4)
    docs = r4.retrieve("q", late=True, repos="a")
    assert [d["path"] for d in docs] == ["p0", "p1", "p2"] and store4.calls == [("search_late", 3, {"repos": "a"})] and late4.queries == 1
    assert [[d["path"] for d in ds] for ds in r4.retrieve_batch(["q", "r"], late=True)] == [["p0", "p1", "p2"]] * 2
    n = len(store4.calls)
    for kw in (dict(mmr=0.5), dict(group_by="path"), dict(hybrid=True), dict(rerank=True)):
        with pytest.raises(ValueError, match="late together with"):
            r4.retrieve("q", late=True, **kw)
    with pytest.raises(ValueError, match="late-interaction reranker"):
        Retriever(FakeEmb(), store4, reranker=Cross()).retrieve("q", late=True)
    assert len(store4.calls) == n
    # a failure follows the last_error protocol
    def boom(*a, **k):
        raise RuntimeError("device lost")

    store4.search_late = boom
    assert r4.retrieve("q", late=True) == [] and isinstance(r4.last_error, RuntimeError)


def test_store_hands_token_vectors_to_the_index_and_refuses_what_it_cannot_do(monkeypatch):
    from semcode_amd.settings import Settings
    from semcode_amd.storage import MilvusVectorStore

    class Ix:
        def __init__(self, **k):
            self.n, self.tokens = 0, {}

        def put_rows(self, vectors, rows):
            self.n = max(self.n, int(rows.max()) + 1)

        def __len__(self):
            return self.n

        def put_tokens(self, rows, toks, fmt="f32"):
            for r, t in zip(rows.tolist(), toks):
                self.tokens[r] = (fmt, t)

    class Late:
        def embed_document_tokens(self, texts, kept_only=False):
            assert kept_only
            return [np.full((len(t), 16), i, np.float32) for i, t in enumerate(texts)]

    s = MilvusVectorStore(dim=2, index_factory=Ix, late=Late())  # late given, no format: f32
    assert s.late_format == "f32"
    s.connect()
    s.upsert_arrays(["a", "b"], np.zeros((2, 2), np.float32), ["xx", "yyy"], [{}, {}])
    assert {r: (f, t.shape) for r, (f, t) in s._collection.tokens.items()} == {0: ("f32", (2, 16)), 1: ("f32", (3, 16))}
    s.upsert_arrays(["b"], np.zeros((1, 2), np.float32), ["zzzz"], [{}], token_vectors=[np.ones((7, 16), np.float32)])  # a replaced key, vectors handed in
    assert s._collection.tokens[1][1].shape == (7, 16) and len(s) == 2
    bf = MilvusVectorStore(dim=2, index_factory=Ix, late_format="bf16")  # a format without a reranker: every upsert brings its vectors
    bf.connect()
    with pytest.raises(ValueError, match="token vectors"):
        bf.upsert_arrays(["a"], np.zeros((1, 2), np.float32), ["x"], [{}])
    assert len(bf) == 0  # the columns were not committed
    with pytest.raises(ValueError, match="late_format"):
        MilvusVectorStore(dim=2, late_format="fp8")
    off = MilvusVectorStore(dim=2, index_factory=Ix)
    assert off.late_format is None and not off.has_late_tokens([0])
    off.connect()
    with pytest.raises(ValueError, match="search_late needs the token store"):
        off.search_late([np.zeros((1, 16), np.float32)])
    assert Settings().mi355x_late_store == "off"
    monkeypatch.setenv("SEMCODE_MI355X_LATE_STORE", "bf16")
    assert Settings().mi355x_late_store == "bf16"
