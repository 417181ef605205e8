"""GPU: the token store of an index -- put / get round trip, the rerank from stored vectors against the pairwise host rule and the
existing MaxSim kernel, the exhaustive MaxSim search against sc_diag_late_search_host (FLAT and trained IVF_FLAT, with and without a
bitset), random mutations against a host model with explicit and automatic compaction, bf16 storage against f32 storage under a derived
bound, every refusal, and the store end to end behind MilvusVectorStore and Retriever on a seeded ColBERT model."""
import ctypes as C
import json

import numpy as np
import pytest

import late_store_ref as ls
from semcode_amd import _native

pytestmark = pytest.mark.gpu

DIM = 64
ROW_BASE = 1000
N_ROWS = 3000
NQS = (1, 16, 17, 32, 128)
COUNTS = (1, 15, 16, 17, 63, 64, 65)
HOT = 7                     # the row every question matches token for token: it and its copies lead every result
HOT_COPIES = 12             # a tie group of 13 at the top: k = 1 and k = 10 cut inside it
BIG = 1501                  # the row of 2 048 tokens


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error():
    buf = C.create_string_buffer(1024)
    _native.lib().sc_last_error(buf, 1024)
    return buf.value.decode()


class Corpus:
    """About 3 000 rows of unit-norm token vectors: counts from COUNTS, some rows without tokens, one of 2 048 tokens, a 600-token row
    that holds every question token with 12 copies spread over the rows, and 45 more exact duplicates of other rows."""

    def __init__(self, W: int):
        rng = np.random.default_rng(1000 + W)
        self.W = W
        self.X = ls.unit_rows(rng, N_ROWS, DIM)
        self.questions = [ls.unit_rows(rng, nq, W) for nq in NQS]
        docs = []
        for r in range(N_ROWS):
            docs.append(None if rng.random() < 0.12 else ls.unit_rows(rng, int(rng.choice(COUNTS)), W))
        hot = ls.unit_rows(rng, 600, W)
        hot[: sum(NQS)] = np.concatenate(self.questions)
        docs[HOT] = hot[rng.permutation(600)]
        docs[BIG] = ls.unit_rows(rng, 2048, W)
        self.hot_rows = [HOT] + [int(r) for r in np.linspace(150, N_ROWS - 40, HOT_COPIES).astype(int)]
        for r in self.hot_rows[1:]:
            docs[r] = docs[HOT].copy()
        taken = set(self.hot_rows) | {BIG}
        self.dups = []
        for r in np.linspace(60, N_ROWS - 11, 45).astype(int):
            src = int(rng.integers(0, N_ROWS))
            if int(r) in taken or src in taken or docs[src] is None:
                continue
            docs[int(r)] = docs[src].copy()
            self.dups.append((int(r), src))
        assert len(self.dups) + HOT_COPIES >= 50
        self.docs = docs
        self.allow_half = rng.random(N_ROWS) < 0.5
        self.allow_half[self.hot_rows[::2]] = False  # the bitset cuts into the tie group
        self.allow_half[self.hot_rows[1::2]] = True
        self._stored, self._want, self._ix = {}, {}, {}

    def stored(self, fmt: str):
        """What the store holds at this format: the input bits, or their bf16 rounding."""
        if fmt not in self._stored:
            self._stored[fmt] = self.docs if fmt == "f32" else [None if d is None else _native.diag_round_bf16(d) for d in self.docs]
        return self._stored[fmt]

    def want(self, fmt: str, allow_name: str):
        """The host search of all five questions at k = 128, computed once; shorter lists are its heads (tests/test_late_store_host.py)."""
        key = (fmt, allow_name)
        if key not in self._want:
            self._want[key] = _native.diag_late_search_host(self.questions, self.stored(fmt), 128, allow=self.allow(allow_name))
        return self._want[key]

    def allow(self, name: str):
        if name == "all":
            return None
        if name == "half":
            return self.allow_half
        a = np.zeros(N_ROWS, bool)
        if name == "one":
            a[self.hot_rows[3]] = True
        return a

    def index(self, rt, fmt: str, kind: str = "FLAT"):
        key = (fmt, kind)
        if key not in self._ix:
            ix = _native.Index(rt, DIM, metric="IP", kind=kind, nlist=16, row_base=ROW_BASE)
            ix.add(self.X)
            if kind == "IVF_FLAT":
                ix.train(niter=3, seed=1)
            half = N_ROWS // 2  # two puts, the second in descending row order: the pool is not in row order
            ix.put_tokens(np.arange(half), self.docs[:half], fmt=fmt)
            ix.put_tokens(np.arange(N_ROWS - 1, half - 1, -1), self.docs[:half - 1:-1], fmt=fmt)
            self._ix[key] = ix
        return self._ix[key]

    def close(self):
        for ix in self._ix.values():
            ix.close()


@pytest.fixture(scope="module")
def corpora():
    made = {}

    def get(W):
        if W not in made:
            made[W] = Corpus(W)
        return made[W]

    yield get
    for c in made.values():
        c.close()


WIDTHS = [16, 96, 128]
FORMATS = ["f32", "bf16"]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W", WIDTHS)
def test_put_then_get_returns_the_stored_bits(rt, corpora, W, fmt):
    c = corpora(W)
    ix = c.index(rt, fmt)
    stored = c.stored(fmt)
    st = ix.token_stats()
    live = sum(len(d) for d in stored if d is not None)
    assert st["W"] == W and st["fmt"] == fmt and st["live"] == live and st["dead"] == 0 and st["rows_with_tokens"] == sum(d is not None for d in stored)
    assert st["pool_bytes"] >= live * W * (4 if fmt == "f32" else 2)
    rows = np.random.default_rng(5).permutation(N_ROWS)
    counts, vecs = ix.get_tokens(rows)
    assert counts.tolist() == [0 if stored[r] is None else len(stored[r]) for r in rows]
    assert ls.same_bits(vecs, np.concatenate([stored[r] for r in rows if stored[r] is not None]))
    counts, vecs = ix.get_tokens(np.arange(N_ROWS))
    assert ls.same_bits(vecs, np.concatenate([d for d in stored if d is not None]))
    if fmt == "bf16":
        assert (vecs.view(np.uint32) & 0xFFFF == 0).all() and not ls.same_bits(vecs, np.concatenate([d for d in c.docs if d is not None]))


def maxsim_dev(rt, Q, q_off, D, d_off, pq, pd, W):
    out = np.full(len(pq), np.nan, np.float32)
    _native._check(_native.lib().sc_diag_maxsim(rt.handle, _p(Q), _p(q_off), len(q_off) - 1, _p(D), _p(d_off), len(d_off) - 1, None, _p(pq), _p(pd), len(pq), W, _p(out)))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W", WIDTHS)
def test_rerank_equals_the_host_rule_on_the_stored_values(rt, corpora, W, fmt):
    c = corpora(W)
    ix = c.index(rt, fmt)
    stored = c.stored(fmt)
    rng = np.random.default_rng(W)
    pool = np.concatenate([rng.choice(N_ROWS, 300, replace=False), [HOT, BIG], [r for r in range(N_ROWS) if stored[r] is None][:5]])
    sub = ls.pair_scores(c.questions, [stored[r] for r in pool], W)  # [5, len(pool)], NaN where the row has no tokens
    sub = np.where(np.isnan(sub), np.float32(-np.inf), sub)
    for C_ in (1, 40, 1024):
        pick = rng.integers(0, len(pool), (len(NQS), C_))
        if C_ > 1:
            pick[:, -3:] = len(pool) - 1  # a row without tokens
        cand = pool[pick] + ROW_BASE
        pad = rng.random(cand.shape) < (0.1 if C_ > 1 else 0.0)
        cand[pad] = -1
        got = ix.rerank_late(c.questions, cand)
        want = np.where(pad, np.float32(-np.inf), np.take_along_axis(sub, pick, axis=1))
        assert ls.same_bits(got, want), (W, fmt, C_)
        assert np.isneginf(got[pad]).all()
    one = ix.rerank_late([c.questions[2]], np.array([[HOT + ROW_BASE]]))  # one question, one candidate
    assert ls.same_bits(one, sub[2:3, 300:301])
    if fmt == "f32":  # the existing kernel on the same pairs
        have = [i for i, r in enumerate(pool) if stored[r] is not None][:60]
        Q = np.concatenate(c.questions)
        q_off = np.concatenate(([0], np.cumsum(NQS))).astype(np.int32)
        D = np.concatenate([stored[pool[i]] for i in have])
        d_off = np.concatenate(([0], np.cumsum([len(stored[pool[i]]) for i in have]))).astype(np.int32)
        pq, pd = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(len(NQS)), np.arange(len(have)), indexing="ij"))
        dev = maxsim_dev(rt, Q, q_off, D, d_off, pq, pd, W).reshape(len(NQS), len(have))
        got = ix.rerank_late(c.questions, np.tile(pool[have] + ROW_BASE, (len(NQS), 1)))
        assert ls.same_bits(got, dev)


def check_search(ix, c, fmt, allow_name, ks=(1, 10, 128)):
    want_s, want_r = c.want(fmt, allow_name)
    want_r = np.where(want_r >= 0, want_r + ROW_BASE, -1)
    allow = c.allow(allow_name)
    for k in ks:
        s, r = ix.search_late(c.questions, k=k, allow=allow)  # Bq = 5: nq 1, 16, 17, 32, 128
        assert np.array_equal(r, want_r[:, :k]) and ls.same_bits(s, want_s[:, :k]), (fmt, allow_name, k)
        for q in (0, 2, 4):  # Bq = 1
            s1, r1 = ix.search_late([c.questions[q]], k=k, allow=allow)
            assert np.array_equal(r1, want_r[q:q + 1, :k]) and ls.same_bits(s1, want_s[q:q + 1, :k]), (fmt, allow_name, k, q)
    return want_s, want_r


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W", WIDTHS)
def test_search_equals_the_host_reference(rt, corpora, W, fmt):
    c = corpora(W)
    ix = c.index(rt, fmt)
    want_s, want_r = check_search(ix, c, fmt, "all")
    # the 13 copies of the hot row lead every list in row order with one score: k = 1 and k = 10 cut inside that tie group
    assert (want_r[:, :13] == np.array(c.hot_rows) + ROW_BASE).all() and all(len(set(row.tolist())) == 1 for row in want_s[:, :13])
    assert (want_s[:, 13] < want_s[:, 12]).all()
    rows_with = sum(d is not None for d in c.docs)
    assert rows_with > 128
    want_s, want_r = check_search(ix, c, fmt, "half")
    assert (want_r[:, :6] == np.array(c.hot_rows[1::2]) + ROW_BASE).all()
    want_s, want_r = check_search(ix, c, fmt, "one", ks=(1, 10))
    assert (want_r[:, 0] == c.hot_rows[3] + ROW_BASE).all() and (want_r[:, 1:] == -1).all() and np.isneginf(want_s[:, 1:]).all()
    want_s, want_r = check_search(ix, c, fmt, "none", ks=(1, 10))
    assert (want_r == -1).all() and np.isneginf(want_s).all()
    ix.release_scratch()  # the store is caller data, not scratch
    assert ix.token_stats()["live"] > 0
    check_search(ix, c, fmt, "all", ks=(10,))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W", [16, 128])
def test_search_on_a_trained_ivf_index_gives_the_same_bits(rt, corpora, W, fmt):
    c = corpora(W)
    ivf = c.index(rt, fmt, kind="IVF_FLAT")
    assert ivf.ivf_info()["nlist"] == 16
    ivf.search(c.X[:4], k=5, nprobe=4)  # (a dense search first: the rows lie list-major by now)
    check_search(ivf, c, fmt, "all", ks=(10, 128))
    check_search(ivf, c, fmt, "half", ks=(10,))
    cand = np.array([[HOT, BIG, 3, 4, -1 - ROW_BASE]] * len(NQS)) + ROW_BASE
    assert ls.same_bits(ivf.rerank_late(c.questions, cand), c.index(rt, fmt).rerank_late(c.questions, cand))


@pytest.mark.parametrize("W", WIDTHS)
def test_bf16_storage_moves_a_score_by_at_most_its_derived_bound(rt, corpora, W):
    """|score_bf16 - score_f32| <= nq 2^-9 (1 + 2^-6): for unit-norm vectors one rounding of relative size 2^-9 per document component
    moves a dot product by at most 2^-9 (Cauchy-Schwarz), a maximum by no more, the sum over nq question tokens by nq times that; the
    factor 1 + 2^-6 covers the f32 chains.  Every (question, row) pair of the corpus."""
    c = corpora(W)
    f32, b16 = c.index(rt, "f32"), c.index(rt, "bf16")
    rows = np.array([r for r in range(N_ROWS) if c.docs[r] is not None])
    worst = np.zeros(len(NQS))
    for i in range(0, len(rows), 1024):
        cand = np.tile(rows[i:i + 1024] + ROW_BASE, (len(NQS), 1))
        a, b = f32.rerank_late(c.questions, cand), b16.rerank_late(c.questions, cand)
        worst = np.maximum(worst, np.abs(a.astype(np.float64) - b.astype(np.float64)).max(axis=1))
    bound = np.array(NQS) * 2.0 ** -9 * (1 + 2.0 ** -6)
    print(f"W={W}: max |bf16 - f32| per question {worst.tolist()}, bound {bound.tolist()}")
    assert (worst <= bound).all() and worst.max() > 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_random_mutations_agree_with_a_host_model(rt, fmt):
    W = 16
    rng = np.random.default_rng(77)
    ix = _native.Index(rt, DIM, metric="IP", row_base=ROW_BASE)
    model = ls.StoreModel()
    questions = [ls.unit_rows(rng, 5, W), ls.unit_rows(rng, 33, W)]
    explicit = 0

    def draw(m):
        v = ls.unit_rows(rng, m, W)
        return v if fmt == "f32" else _native.diag_round_bf16(v)  # (already representable: the model holds what the store holds)

    def check(what):
        st = ix.token_stats()
        assert (st["live"], st["dead"], st["rows_with_tokens"]) == (model.live, model.dead, model.rows_with_tokens), (what, st, model.live, model.dead)
        assert len(ix) == len(model.docs)
        if model.live == 0 and st["W"] == 0:
            return
        s, r = ix.search_late(questions, k=10)
        ws, wr = _native.diag_late_search_host(questions, model.docs, 10) if model.docs else (np.full((2, 10), -np.inf, np.float32), np.full((2, 10), -1, np.int64))
        assert np.array_equal(r, np.where(wr >= 0, wr + ROW_BASE, -1)) and ls.same_bits(s, ws), what

    ix.add(ls.unit_rows(rng, 40, DIM))
    model.append(40)
    rows = rng.choice(40, 30, replace=False)
    toks = [draw(int(rng.choice((1, 15, 16, 17, 33)))) for _ in rows]
    ix.put_tokens(rows, toks, fmt=fmt)
    model.put(rows, toks)
    check("first put")
    for step in range(60):
        n = len(model.docs)
        op = rng.choice(["put", "put", "remove", "append", "overwrite", "delete", "compact"]) if n > 8 else "append"
        if op == "put":  # changed counts, rows with and without tokens
            rows = rng.choice(n, int(rng.integers(1, min(n, 12))), replace=False)
            toks = [draw(int(rng.choice((1, 2, 16, 17, 40)))) for _ in rows]
            ix.put_tokens(rows, toks, fmt=fmt)
            model.put(rows, toks)
        elif op == "remove":
            rows = rng.choice(n, int(rng.integers(1, 6)), replace=False)
            ix.put_tokens(rows, [None] * len(rows), fmt=fmt)
            model.put(rows, [None] * len(rows))
        elif op == "append":
            m = int(rng.integers(1, 20))
            ix.add(ls.unit_rows(rng, m, DIM))
            model.append(m)
        elif op == "overwrite":  # the rows' vectors change, their tokens stay
            rows = rng.choice(n, int(rng.integers(1, 6)), replace=False)
            ix.overwrite(ls.unit_rows(rng, len(rows), DIM), rows)
        elif op == "delete":
            rows = rng.choice(n, int(rng.integers(1, max(2, n // 4))), replace=False)
            ix.delete_rows(rows)
            model.delete(rows)
        else:
            before = ix.search_late(questions, k=10) if model.live else None
            ix.compact_tokens()
            model.compact()
            explicit += 1
            assert ix.token_stats()["dead"] == 0
            if before is not None:
                after = ix.search_late(questions, k=10)
                assert np.array_equal(before[1], after[1]) and ls.same_bits(before[0], after[0])
        check(f"step {step}: {op}")
    assert explicit >= 1 and model.auto_compactions >= 1, (explicit, model.auto_compactions)
    # an automatic compaction, seen through the statistics: replacing every row's tokens leaves more dead than live tokens for a moment
    ix.compact_tokens()
    model.compact()
    n = len(model.docs)
    rows = np.arange(n)
    toks = [draw(20) for _ in rows]
    ix.put_tokens(rows, toks, fmt=fmt)
    model.put(rows, toks)
    half = [draw(2) for _ in rows]
    ix.put_tokens(rows, half, fmt=fmt)  # 20 n dead against 2 n live
    autos = model.auto_compactions
    model.put(rows, half)
    assert model.auto_compactions == autos + 1 and ix.token_stats()["dead"] == 0 and ix.token_stats()["live"] == 2 * n
    check("automatic compaction")
    ix.delete_rows(np.arange(n))  # nothing survives
    model.delete(np.arange(n))
    check("everything deleted")
    ix.close()


def test_refusals_change_nothing(rt):
    W = 32
    rng = np.random.default_rng(9)
    lib = _native.lib()
    ix = _native.Index(rt, DIM, metric="IP")
    ix.add(ls.unit_rows(rng, 20, DIM))
    questions = [ls.unit_rows(rng, 4, W)]
    Q, q_off = _native.pack_questions(questions)
    h = ix.handle
    s, r = np.zeros(4, np.float32), np.zeros(4, np.int64)
    # no store yet
    assert lib.sc_index_search_late(h, _p(Q), _p(q_off), 1, 4, None, 0, _p(s), _p(r)) == -1 and "no token vectors" in last_error()
    assert lib.sc_index_rerank_late(h, _p(Q), _p(q_off), 1, _p(r), 4, _p(s)) == -1 and "no token vectors" in last_error()
    assert ix.token_stats() == {"rows_with_tokens": 0, "live": 0, "dead": 0, "W": 0, "fmt": "f32", "pool_bytes": 0}
    ix.reserve_tokens(1000)  # before the first install: remembered
    assert ix.token_stats()["W"] == 0
    docs = [ls.unit_rows(rng, int(m), W) for m in rng.integers(1, 20, 20)]
    ix.put_tokens(np.arange(20), docs)
    st0 = ix.token_stats()
    assert st0["pool_bytes"] >= 1000 * W * 4 and st0["live"] == sum(len(d) for d in docs)
    before = ix.search_late(questions, k=4)

    rows2 = np.array([1, 2], np.int64)
    cnt2 = np.array([1, 1], np.int32)
    vec2 = ls.unit_rows(rng, 2, W)

    def put_rc(**k):
        a = dict(rows=rows2, n=2, counts=cnt2, vecs=vec2, W=W, fmt=0)
        a.update(k)
        return lib.sc_index_put_tokens(h, _p(a["rows"]), a["n"], _p(a["counts"]), _p(a["vecs"]), a["W"], a["fmt"])

    for kw, needle in ((dict(rows=None), "bad argument"), (dict(n=-1), "bad argument"), (dict(vecs=None), "vecs is NULL"), (dict(W=24), "multiple of 16"),
                       (dict(W=16), "holds tokens of W=32"), (dict(fmt=1), "holds tokens of W=32"), (dict(fmt=2), "fmt must be"),
                       (dict(counts=np.array([1, 2049], np.int32)), "outside 0 .. 2048"), (dict(counts=np.array([-1, 1], np.int32)), "outside 0 .. 2048"),
                       (dict(rows=np.array([1, 20], np.int64)), "out of range"), (dict(rows=np.array([-1, 2], np.int64)), "out of range"),
                       (dict(rows=np.array([3, 3], np.int64)), "distinct")):
        assert put_rc(**kw) == -1 and "sc_index_put_tokens" in last_error() and needle in last_error(), (list(kw), last_error())

    def search_rc(**k):
        a = dict(Q=Q, q_off=q_off, Bq=1, k=4, allow=None, words=0, s=s, r=r)
        a.update(k)
        return lib.sc_index_search_late(h, _p(a["Q"]), _p(a["q_off"]), a["Bq"], a["k"], _p(a["allow"]), a["words"], _p(a["s"]), _p(a["r"]))

    for kw, needle in ((dict(Q=None), "NULL"), (dict(s=None), "NULL"), (dict(k=0), "top_k"), (dict(k=129), "top_k"), (dict(Bq=0), "Bq"),
                       (dict(q_off=np.array([1, 4], np.int32)), "q_off[0]"), (dict(q_off=np.array([0, 129], np.int32)), "token vectors"),
                       (dict(q_off=np.array([0, 0], np.int32)), "token vectors"), (dict(words=1), "allow is NULL"), (dict(allow=np.zeros(1, np.uint32), words=0), "allow_words")):
        assert search_rc(**kw) == -1 and "sc_index_search_late" in last_error() and needle in last_error(), (list(kw), last_error())

    cand = np.array([0, 1, -1, 19], np.int64)

    def rerank_rc(**k):
        a = dict(Q=Q, q_off=q_off, Bq=1, cand=cand, C=4, out=s)
        a.update(k)
        return lib.sc_index_rerank_late(h, _p(a["Q"]), _p(a["q_off"]), a["Bq"], _p(a["cand"]), a["C"], _p(a["out"]))

    assert rerank_rc() == 0
    for kw, needle in ((dict(cand=None), "NULL"), (dict(out=None), "NULL"), (dict(C=0), "C must be"), (dict(C=1025), "C must be"),
                       (dict(cand=np.array([0, 1, -2, 19], np.int64)), "neither -1 nor a row"), (dict(cand=np.array([0, 1, 20, 19], np.int64)), "neither -1 nor a row"),
                       (dict(q_off=np.array([0, 200], np.int32)), "token vectors")):
        assert rerank_rc(**kw) == -1 and "sc_index_rerank_late" in last_error() and needle in last_error(), (list(kw), last_error())
    cnt = np.zeros(2, np.int32)
    out = np.zeros((1, W), np.float32)
    assert lib.sc_index_get_tokens(h, _p(np.array([0, 20], np.int64)), 2, _p(cnt), None, 0) == -1 and "out of range" in last_error()
    assert lib.sc_index_get_tokens(h, _p(rows2), 2, _p(cnt), _p(out), 1) == -1 and "room for 1" in last_error()
    assert lib.sc_index_reserve_tokens(h, -1) == -1
    # nothing changed
    assert ix.token_stats() == st0
    after = ix.search_late(questions, k=4)
    assert np.array_equal(before[1], after[1]) and ls.same_bits(before[0], after[0])
    counts, vecs = ix.get_tokens(np.arange(20))
    assert ls.same_bits(vecs, np.concatenate(docs))
    # dropping the store frees it; another format may follow
    ix.drop_tokens()
    assert ix.token_stats()["W"] == 0 and ix.token_stats()["pool_bytes"] == 0
    ix.put_tokens([0], [docs[0][:, :16].copy()], fmt="bf16")
    assert ix.token_stats()["W"] == 16 and ix.token_stats()["fmt"] == "bf16"
    ix.close()


# ---------------------------------------------------------------- end to end: MilvusVectorStore + Retriever on a seeded ColBERT model
class Calls:
    """Counts what a query may not do when the store holds the token vectors: score_pairs, and every document-side encoder call."""

    def __init__(self, reranker):
        self.score_pairs = self.doc_side = 0
        enc, pairs = reranker._encoder, reranker.score_pairs
        embed_tokens, score_late = enc.embed_tokens, enc.score_late

        def counted_pairs(*a, **k):
            self.score_pairs += 1
            return pairs(*a, **k)

        def counted_embed(ids, off, expand_id=-1, **k):
            self.doc_side += expand_id < 0
            return embed_tokens(ids, off, expand_id=expand_id, **k)

        def counted_late(*a, **k):
            self.doc_side += 1
            return score_late(*a, **k)

        reranker.score_pairs, enc.embed_tokens, enc.score_late = counted_pairs, counted_embed, counted_late

    def reset(self):
        self.score_pairs = self.doc_side = 0


def test_store_end_to_end_on_a_seeded_colbert_model(rt, golden, tmp_path, monkeypatch):
    from pathlib import Path

    import late_ref as lr
    from semcode_amd.embeddings.late import MI355XLateReranker
    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from semcode_amd.services import Retriever, build_payloads
    from semcode_amd.settings import settings
    from semcode_amd.storage import MilvusVectorStore
    from test_seams_gpu import Chunk

    meta = json.loads((golden / "late_golden.json").read_text())["bert128"]
    case = lr.CASES["bert128"]
    cfg = case["cfg"]
    blob, proj = lr.make_weights(case, meta["seed"], meta["scale"]), lr.make_proj(case, meta["seed"])
    monkeypatch.setattr(settings, "rag_max_context_sources", 5)
    vocab = {w: i for i, w in enumerate(lr.vocab_lines(cfg))}
    emb = MI355XEmbeddings(cfg=dict(cfg), vocab=vocab, runtime=rt, synth_seed=3, allow_synthetic=True)
    reranker = MI355XLateReranker(lr.write_pylate_dir(tmp_path / "m", case, blob, proj), runtime=rt)
    calls = Calls(reranker)
    rng = np.random.default_rng(21)
    root = Path("/w/demo")
    N = 60
    texts = [f"w{20 + i} . " + " , ".join(f"w{int(j)}" for j in rng.integers(40, 400, int(rng.integers(5, 50)))) for i in range(N)]
    chunks = [Chunk(t, root / ("pkg" if i % 2 else "lib") / f"k{i}.py", "python" if i % 3 else "go", 1, 3) for i, t in enumerate(texts)]
    payloads = build_payloads("demo", root, chunks, emb)

    def make_store(name, **k):
        s = MilvusVectorStore(collection_name=name, dim=cfg["hidden"], metric="COSINE", index_type="FLAT", runtime=rt, **k)
        s.connect()
        return s

    plain = make_store("plain")
    plain.upsert_embeddings(payloads)
    store = make_store("late", late=reranker, late_format="f32")
    store.upsert_embeddings(payloads)
    ix = store._collection
    st = ix.token_stats()
    assert st["rows_with_tokens"] == N and st["fmt"] == "f32" and st["W"] == case["W"] and st["dead"] == 0
    # what is stored: the document's token vectors without those of punctuation
    want_tokens = reranker.embed_document_tokens(texts, kept_only=True)
    all_tokens = reranker.embed_document_tokens(texts)
    assert all(len(k) < len(a) for k, a in zip(want_tokens, all_tokens))  # (every text holds punctuation)
    counts, vecs = ix.get_tokens(np.arange(N))
    assert counts.tolist() == [len(t) for t in want_tokens] and ls.same_bits(vecs, np.concatenate(want_tokens))

    questions = ["w25 w26", "w40 , w77 w300", "w21"]
    parent = Retriever(emb, plain, reranker=reranker)
    r = Retriever(emb, store, reranker=reranker)
    for q in questions:
        want = parent.retrieve(q, rerank=True, fetch_k=40)
        assert len(want) == 5 and parent.last_error is None
        calls.reset()
        got = r.retrieve(q, rerank=True, fetch_k=40)
        assert r.last_error is None and (calls.score_pairs, calls.doc_side) == (0, 0)
        assert [d["path"] for d in got] == [d["path"] for d in want]
        assert ls.same_bits([d["score"] for d in got], [d["score"] for d in want]) and [d["retrieval_score"] for d in got] == [d["retrieval_score"] for d in want]
    want_b = parent.retrieve_batch(questions, rerank=True, fetch_k=40)
    calls.reset()
    got_b = r.retrieve_batch(questions, rerank=True, fetch_k=40)
    assert (calls.score_pairs, calls.doc_side) == (0, 0) and r.last_error is None
    assert [[(d["path"], np.float32(d["score"]).view(np.uint32)) for d in ds] for ds in got_b] == [[(d["path"], np.float32(d["score"]).view(np.uint32)) for d in ds] for ds in want_b]

    # the MaxSim search as the first stage: the host reference's rows
    qv = reranker.embed_query_tokens(questions)
    stored = np.split(vecs, np.cumsum(counts)[:-1])
    ws, wr = _native.diag_late_search_host(qv, stored, 5)
    calls.reset()
    for i, q in enumerate(questions):
        docs = r.retrieve(q, late=True)
        assert r.last_error is None and [d["path"] for d in docs] == [store._paths[int(x)] for x in wr[i]] and ls.same_bits([d["score"] for d in docs], ws[i])
    batch = r.retrieve_batch(questions, late=True)
    assert [[d["path"] for d in ds] for ds in batch] == [[store._paths[int(x)] for x in row] for row in wr]
    assert (calls.score_pairs, calls.doc_side) == (0, 0)
    go = np.array([lang == "go" for lang in store._languages])
    ws_go, wr_go = _native.diag_late_search_host(qv[:1], stored, 5, allow=go)
    docs = r.retrieve(questions[0], late=True, languages="go")
    assert [d["path"] for d in docs] == [store._paths[int(x)] for x in wr_go[0]] and all(d["language"] == "go" for d in docs)
    for kw in (dict(mmr=0.5), dict(group_by="path"), dict(hybrid=True), dict(rerank=True)):
        with pytest.raises(ValueError, match="late together with"):
            r.retrieve(questions[0], late=True, **kw)
        with pytest.raises(ValueError, match="late together with"):
            r.retrieve_batch(questions, late=True, **kw)
    with pytest.raises(ValueError, match="late-interaction reranker"):
        Retriever(emb, store).retrieve(questions[0], late=True)

    # a candidate row without tokens: the rerank falls back to score_pairs, same result
    want = parent.retrieve(questions[0], rerank=True, fetch_k=40)
    top_row = store._row_of[[pk for pk in store._ids if store._paths[store._row_of[pk]] == want[0]["path"]][0]]
    ix.put_tokens([top_row], [None])
    calls.reset()
    got = r.retrieve(questions[0], rerank=True, fetch_k=40)
    assert calls.score_pairs == 1 and [(d["path"], d["score"]) for d in got] == [(d["path"], d["score"]) for d in want]
    ix.put_tokens([top_row], [want_tokens[top_row]])
    assert ix.token_stats()["dead"] == len(want_tokens[top_row])
    ix.compact_tokens()
    assert ix.token_stats()["dead"] == 0 and ix.token_stats()["live"] == sum(len(t) for t in want_tokens)

    # a replaced primary key replaces the row's tokens; a delete renumbers them with the rows
    new_text = "w33 . w34 w35"
    payload = build_payloads("demo", root, [Chunk(new_text, chunks[4].path, "python", 1, 3)], emb)
    store.upsert_embeddings(payload)
    assert len(store) == N and store._texts[4] == new_text
    c4, v4 = ix.get_tokens([4])
    assert ls.same_bits(v4, reranker.embed_document_tokens([new_text], kept_only=True)[0]) and ix.token_stats()["dead"] == len(want_tokens[4])
    assert store.delete([store._ids[0], store._ids[7]]) == 2
    counts2, vecs2 = ix.get_tokens(np.arange(N - 2))
    keep_rows = [i for i in range(N) if i not in (0, 7)]
    assert counts2.tolist() == [len(want_tokens[i]) if i != 4 else int(c4[0]) for i in keep_rows]
    stored2 = np.split(vecs2, np.cumsum(counts2)[:-1])
    ws2, wr2 = _native.diag_late_search_host(qv, stored2, 5)
    docs = r.retrieve_batch(questions, late=True)
    assert [[d["path"] for d in ds] for ds in docs] == [[store._paths[int(x)] for x in row] for row in wr2]

    # save / load: the tokens and the results come back
    store.save(tmp_path / "saved")
    manifest = json.loads((tmp_path / "saved" / "manifest.json").read_text())
    assert manifest["late_format"] == "f32" and manifest["late_width"] == case["W"] and manifest["late_tokens"] == int(counts2.sum())
    again = make_store("again", late=reranker, late_format="f32")
    again.load(tmp_path / "saved")
    c3, v3 = again._collection.get_tokens(np.arange(N - 2))
    assert np.array_equal(c3, counts2) and ls.same_bits(v3, vecs2)
    r2 = Retriever(emb, again, reranker=reranker)
    assert [[(d["path"], d["score"]) for d in ds] for ds in r2.retrieve_batch(questions, late=True)] == [[(d["path"], d["score"]) for d in ds] for ds in docs]
    calls.reset()
    assert r2.retrieve(questions[1], rerank=True, fetch_k=40) == r.retrieve(questions[1], rerank=True, fetch_k=40) and (calls.score_pairs, calls.doc_side) == (0, 0)
    # a bf16 store: the file holds the upper halves, the load brings back the stored bits; a collection saved without tokens loads as before
    half = make_store("half", late_format="bf16")
    half.upsert_embeddings(payloads[:10], token_vectors=want_tokens[:10])
    half.save(tmp_path / "half")
    assert (tmp_path / "half" / "tokens.bf16").stat().st_size == 2 * case["W"] * sum(len(t) for t in want_tokens[:10])
    half2 = make_store("half2")
    half2.load(tmp_path / "half")
    assert half2.late_format == "bf16" and ls.same_bits(half2._collection.get_tokens(np.arange(10))[1], _native.diag_round_bf16(np.concatenate(want_tokens[:10])))
    plain.save(tmp_path / "plain")
    assert "late_format" not in json.loads((tmp_path / "plain" / "manifest.json").read_text()) and not (tmp_path / "plain" / "token_counts.i32").exists()
    plain2 = make_store("plain2")
    plain2.load(tmp_path / "plain")
    assert len(plain2) == N and plain2.late_format is None and plain2._collection.token_stats()["W"] == 0
    for s in (plain, store, again, half, half2, plain2):
        s.close()
    reranker.close()
    emb.close()
