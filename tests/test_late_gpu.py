"""GPU: late interaction on the device -- the MaxSim kernel against the host rule bit for bit (sc_diag_maxsim), token vectors and scores against
tests/golden/late_golden (transformers fp32; bounds = twice the bf16 model's own error, scripts/gen_late_fixtures.py), the bit-identity of
sc_encoder_score_late with the host rule fed the vectors sc_encoder_embed_tokens returns, batch independence, every refusal, and the reranker
class behind Retriever."""
import ctypes as C
import json

import numpy as np
import pytest

import late_ref as lr
from semcode_amd import _native
from test_late_host import SHAPES, last_error, make_case, maxsim_host, same_bits

pytestmark = pytest.mark.gpu


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def maxsim_dev(rt, Q, q_off, D, d_off, keep, pq, pd, W):
    out = np.full(len(pq), np.nan, np.float32)
    _native._check(_native.lib().sc_diag_maxsim(rt.handle, _p(Q), _p(q_off), len(q_off) - 1, _p(D), _p(d_off), len(d_off) - 1, _p(keep), _p(pq), _p(pd), len(pq), W,
                                                _p(out)))
    return out


@pytest.mark.parametrize("W,nqs,nds", SHAPES)
def test_kernel_equals_the_host_rule(rt, W, nqs, nds):
    rng = np.random.default_rng(100 + W)
    Q, q_off, D, d_off, pq, pd = make_case(rng, W, nqs, nds)
    assert same_bits(maxsim_dev(rt, Q, q_off, D, d_off, None, pq, pd, W), maxsim_host(Q, q_off, D, d_off, None, pq, pd, W))
    keep = (rng.random(int(d_off[-1])) < 0.6).astype(np.uint8)
    keep[d_off[:-1]] = 1
    assert same_bits(maxsim_dev(rt, Q, q_off, D, d_off, keep, pq, pd, W), maxsim_host(Q, q_off, D, d_off, keep, pq, pd, W))


def test_kernel_on_ties_zeros_and_negative_documents(rt):
    rng = np.random.default_rng(6)
    Q, q_off, D, d_off, pq, pd = make_case(rng, 16, (1, 17, 32), (1, 15, 16, 17), grid=2)
    D[d_off[1]:d_off[2]] = -np.abs(D[d_off[1]:d_off[2]])  # a document of non-positive values only
    Q[:] = np.where(Q == 0, np.float32(-0.0), Q)
    keep = np.ones(int(d_off[-1]), np.uint8)
    keep[d_off[3] + 1:d_off[4]:2] = 0
    for k in (None, keep):
        assert same_bits(maxsim_dev(rt, Q, q_off, D, d_off, k, pq, pd, 16), maxsim_host(Q, q_off, D, d_off, k, pq, pd, 16))
    order = np.arange(len(pq))[::-1].copy()  # the pair list in another order: the same bits per pair
    assert same_bits(maxsim_dev(rt, Q, q_off, D, d_off, keep, pq[order], pd[order], 16), maxsim_host(Q, q_off, D, d_off, keep, pq, pd, 16)[order])


# ---------------------------------------------------------------- the golden models
@pytest.fixture(scope="module")
def golden_late(golden):
    return np.load(golden / "late_golden.npz"), json.loads((golden / "late_golden.json").read_text())


class Model:
    def __init__(self, rt, name, data, meta):
        self.name, self.case, self.meta = name, lr.CASES[name], meta[name]
        self.cfg, self.W = self.case["cfg"], self.case["W"]
        self.blob = lr.make_weights(self.case, self.meta["seed"], self.meta["scale"])
        self.proj = lr.make_proj(self.case, self.meta["seed"])
        self.questions, self.passages = lr.make_texts(self.case, self.meta["seed"])
        q_ids, q_off = lr.pack(self.questions)
        p_ids, p_off = lr.pack(self.passages)
        assert np.array_equal(q_ids, data[f"{name}_q_ids"]) and np.array_equal(p_ids, data[f"{name}_p_ids"]), "make_texts no longer rebuilds the golden ids"
        self.q_ids, self.q_off, self.p_ids, self.p_off = q_ids, q_off, p_ids, p_off
        self.keep = lr.keep_flags(p_ids)
        self.scores, self.qvec, self.dvec = data[f"{name}_scores"], data[f"{name}_qvec"], data[f"{name}_dvec"]
        self.enc = _native.Encoder(rt, self.cfg, weights=self.blob)
        self.enc.set_token_head(self.proj)
        self.pq, self.pp = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(lr.N_QUESTIONS), np.arange(lr.N_PASSAGES), indexing="ij"))
        self.paths = ("batch", "small") if self.case["fold"] else ("auto",)

    def score_all(self, **k):
        return self.enc.score_late(self.q_ids, self.q_off, self.p_ids, self.p_off, self.pq, self.pp, expand_id=lr.MASK_ID, d_keep=self.keep, **k)


@pytest.fixture(scope="module")
def models(rt, golden_late):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Model(rt, name, *golden_late)
        return made[name]

    yield get
    for m in made.values():
        m.enc.close()


CASE_NAMES = list(lr.CASES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_token_vectors_match_the_golden_model(models, name):
    m = models(name)
    for path in m.paths:
        m.enc.set_path(path)
        qv, qc = m.enc.embed_tokens(m.q_ids, m.q_off, expand_id=lr.MASK_ID)
        dv, dc = m.enc.embed_tokens(m.p_ids, m.p_off)
        # counts and layout exact: 32 rows per question (expansion rows included), len_i rows per passage, text after text
        assert qc.tolist() == [32] * lr.N_QUESTIONS and qv.shape == (32 * lr.N_QUESTIONS, m.W)
        assert dc.tolist() == np.diff(m.p_off).tolist() and dv.shape == (int(m.p_off[-1]), m.W)
        stored = np.concatenate([m.p_off[i] + lr.stored_rows(int(n)) for i, n in enumerate(np.diff(m.p_off))])
        for got, want, what in ((qv, m.qvec, "question"), (dv[stored], m.dvec, "passage")):
            err = float(np.abs(got - want).max())
            cos = float(((got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))).min())
            print(f"{name} path {path} {what} vectors: max|d| = {err:.4f} (T_vec {m.meta['T_vec']:.4f}), cos >= {cos:.5f}")
            assert err <= m.meta["T_vec"] and cos >= 0.999, (name, path, what, err, cos)
        assert np.allclose(np.linalg.norm(dv, axis=1), 1.0, atol=1e-5)
    m.enc.set_path("auto")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_scores_match_the_golden_model_and_rank_alike(models, name):
    m = models(name)
    T = m.meta["T_score"]
    for path in m.paths:
        m.enc.set_path(path)
        got = m.score_all().reshape(lr.N_QUESTIONS, lr.N_PASSAGES)
        err = float(np.abs(got - m.scores).max())
        print(f"{name} path {path} scores: max|d| = {err:.4f} (T_score {T:.4f})")
        assert err <= T, (name, path, err)
        for q in range(lr.N_QUESTIONS):  # the golden order, wherever its scores are further apart than the bound can bridge
            pairs = lr.ordered_pairs(m.scores[q], 2 * T)
            assert len(pairs) >= lr.N_PASSAGES * (lr.N_PASSAGES - 1) // 4
            assert all(got[q, i] > got[q, j] for i, j in pairs)
    m.enc.set_path("auto")


@pytest.mark.parametrize("name", CASE_NAMES)
def test_scores_are_the_host_rule_on_the_returned_vectors(models, name):
    m = models(name)
    for path in m.paths:
        m.enc.set_path(path)
        qv, qc = m.enc.embed_tokens(m.q_ids, m.q_off, expand_id=lr.MASK_ID)
        dv, dc = m.enc.embed_tokens(m.p_ids, m.p_off)
        q_off = np.concatenate(([0], np.cumsum(qc))).astype(np.int32)
        d_off = np.concatenate(([0], np.cumsum(dc))).astype(np.int32)
        assert same_bits(m.score_all(), maxsim_host(qv, q_off, dv, d_off, m.keep, m.pq, m.pp, m.W))
    m.enc.set_path("auto")


@pytest.mark.parametrize("name", ["bert128", "bert768", "mb256"])
def test_a_pair_scores_the_same_bits_alone_in_a_batch_and_reversed(models, name):
    m = models(name)
    full = m.score_all()
    order = np.arange(len(m.pq))[::-1].copy()
    assert same_bits(m.enc.score_late(m.q_ids, m.q_off, m.p_ids, m.p_off, m.pq[order], m.pp[order], expand_id=lr.MASK_ID, d_keep=m.keep), full[order])
    # texts in reversed order as well: every text stands elsewhere in its packed batch
    rq, rp = m.questions[::-1], m.passages[::-1]
    q_ids, q_off = lr.pack(rq)
    p_ids, p_off = lr.pack(rp)
    got = m.enc.score_late(q_ids, q_off, p_ids, p_off, (lr.N_QUESTIONS - 1 - m.pq).astype(np.int32), (lr.N_PASSAGES - 1 - m.pp).astype(np.int32), expand_id=lr.MASK_ID,
                           d_keep=lr.keep_flags(p_ids))
    assert same_bits(got, full)
    one = np.zeros(1, np.int32)
    for q, p in ((0, 0), (1, 3), (3, 5), (2, 4)):  # alone: one question, one passage, one pair
        qi, qo = lr.pack([m.questions[q]])
        pi, po = lr.pack([m.passages[p]])
        alone = m.enc.score_late(qi, qo, pi, po, one, one, expand_id=lr.MASK_ID, d_keep=lr.keep_flags(pi))
        assert same_bits(alone, full[q * lr.N_PASSAGES + p:q * lr.N_PASSAGES + p + 1]), (name, q, p)


def test_refusals_leave_the_head_and_the_next_call_intact(models, rt):
    m = models("bert128")
    lib, h = _native.lib(), m.enc.handle
    before = m.score_all()

    def late_rc(**k):
        a = dict(q_ids=m.q_ids, q_off=m.q_off, Bq=lr.N_QUESTIONS, expand=lr.MASK_ID, d_ids=m.p_ids, d_off=m.p_off, Bd=lr.N_PASSAGES, keep=m.keep, pq=m.pq, pp=m.pp,
                 P=len(m.pq))
        a.update(k)
        out = np.zeros(max(1, len(a["pq"])), np.float32)
        return lib.sc_encoder_score_late(h, _p(a["q_ids"]), _p(a["q_off"]), a["Bq"], a["expand"], _p(a["d_ids"]), _p(a["d_off"]), a["Bd"], _p(a["keep"]), _p(a["pq"]),
                                         _p(a["pp"]), a["P"], _p(out))

    no_keep = m.keep.copy()
    no_keep[m.p_off[2]:m.p_off[3]] = 0
    long_q = np.full(129, lr.FIRST_WORD, np.int32)
    big = np.full(512 * 1025, lr.FIRST_WORD, np.int32)  # 1 025 texts of max_pos = 512 tokens: more rows than one packed call may have
    big_off = (np.arange(1026, dtype=np.int64) * 512)
    m.enc.set_token_head(None)
    assert late_rc() == -1 and "no token head" in last_error()
    m.enc.set_token_head(m.proj)
    for kw, code, needle in ((dict(keep=no_keep), -1, "no kept token"), (dict(pq=np.full_like(m.pq, lr.N_QUESTIONS)), -1, "outside"),
                             (dict(pp=np.full_like(m.pp, -1)), -1, "outside"), (dict(P=0), -1, "P = 0"), (dict(expand=m.cfg["vocab"]), -1, "expand_id"),
                             (dict(q_ids=long_q, q_off=np.array([0, 129], np.int64), Bq=1, pq=np.zeros(1, np.int32), pp=np.zeros(1, np.int32), P=1), -1, "more than 128"),
                             (dict(q_off=np.array([1, 3, 14, 34, 66], np.int64)), -1, "offsets[0]"), (dict(q_ids=None), -1, "NULL"),
                             (dict(d_ids=big, d_off=big_off, Bd=1025, keep=None), -4, "SC_ENCODER_PACKED_MAX_ROWS")):
        rc = late_rc(**kw)
        assert rc == code and "sc_encoder_score_late" in last_error() and needle in last_error(), (kw.keys(), rc, last_error())
    # the token head's own refusals: the installed head stays
    bad = np.zeros((24, m.cfg["hidden"]), np.float32)
    for w in (24, 8, 144):
        assert lib.sc_encoder_set_token_head(h, _p(bad), w) == -1 and "sc_encoder_set_token_head" in last_error()
    counts = np.zeros(1, np.int32)
    out = np.zeros((160, m.W), np.float32)
    assert lib.sc_encoder_embed_tokens(h, _p(long_q), _p(np.array([0, 129], np.int64)), 1, lr.MASK_ID, _p(out), _p(counts)) == -1
    assert "more than 128" in last_error()
    assert same_bits(m.score_all(), before)
    # independent of the pooling mode and the pair head: an embedding call in between changes nothing, and is itself unchanged
    emb = m.enc.embed_packed(m.p_ids, m.p_off)
    m.enc.pooling = "cls"
    assert same_bits(m.score_all(), before)
    m.enc.pooling = "mean"
    assert np.array_equal(m.enc.embed_packed(m.p_ids, m.p_off), emb)
    # arch 2 has no token head
    q2 = _native.Encoder(rt, dict(vocab=400, max_pos=2048, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True, rope_theta=1000000.0, hidden=128, heads=2,
                                  kv_heads=1, ffn=256, layers=1), synth_seed=2)
    assert lib.sc_encoder_set_token_head(q2.handle, _p(m.proj), m.W) == -4 and "arch 2" in last_error()
    q2.close()
    # a pre-norm model with local layers refuses a question whose last expansion row would see no key
    mb = models("mb256")
    short = np.array([lr.CLS_ID, lr.Q_ID, lr.SEP_ID], np.int32)
    assert lib.sc_encoder_embed_tokens(mb.enc.handle, _p(short), _p(np.array([0, 3], np.int64)), 1, lr.MASK_ID, _p(out), _p(counts)) == -1
    assert "local_window" in last_error()


# ---------------------------------------------------------------- the reranker class and Retriever
def test_reranker_on_a_written_directory_reproduces_the_golden_order(models, rt, tmp_path):
    from semcode_amd.embeddings.late import MI355XLateReranker

    m = models("bert128")
    rr = MI355XLateReranker(lr.write_pylate_dir(tmp_path / "m", m.case, m.blob, m.proj), runtime=rt)
    texts_q = [lr.text_of(q, m.cfg) for q in m.questions]
    texts_p = [lr.text_of(p, m.cfg) for p in m.passages]
    assert all(rr.query_ids(t) == q.tolist() for t, q in zip(texts_q, m.questions))
    # (passage 0 is the two tokens [CLS] [D] without a [SEP]: no text tokenises to it; the others round-trip through the tokenizer)
    assert all(rr.document_ids(t) == p.tolist() for t, p in zip(texts_p[1:], m.passages[1:]))
    sel = m.pp != 0
    got = rr.score_pairs([texts_q[i] for i in m.pq[sel]], [texts_p[j] for j in m.pp[sel]])
    assert same_bits(got, m.score_all()[sel])
    T = m.meta["T_score"]
    for q in range(lr.N_QUESTIONS):
        order, scores = rr.rerank(texts_q[q], texts_p[1:])
        assert same_bits(scores, got.reshape(lr.N_QUESTIONS, -1)[q][order])
        rank = {int(p) + 1: r for r, p in enumerate(order)}
        assert all(rank[i] < rank[j] for i, j in lr.ordered_pairs(m.scores[q], 2 * T) if i and j)
    qv, dv = rr.embed_query_tokens(texts_q[:2]), rr.embed_document_tokens(texts_p[1:4])
    assert [v.shape for v in qv] == [(32, m.W)] * 2 and [len(v) for v in dv] == [len(p) for p in m.passages[1:4]]
    # a budget that cuts the passages into several batches: the same bits
    small = MI355XLateReranker(lr.write_stanford_dir(tmp_path / "s", m.case, m.blob, m.proj), runtime=rt, rows_budget=512)
    assert same_bits(small.score_pairs([texts_q[i] for i in m.pq[sel]], [texts_p[j] for j in m.pp[sel]]), got)
    small.close()
    rr.close()


def test_retriever_reranks_with_the_late_reranker(models, rt, tmp_path, monkeypatch):
    from pathlib import Path

    from semcode_amd.embeddings.late import MI355XLateReranker
    from semcode_amd.embeddings.providers import MI355XEmbeddings
    from semcode_amd.services import Retriever, build_payloads
    from semcode_amd.settings import settings
    from semcode_amd.storage import MilvusVectorStore
    from test_seams_gpu import Chunk

    m = models("bert128")
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    vocab = {w: i for i, w in enumerate(lr.vocab_lines(m.cfg))}
    emb = MI355XEmbeddings(cfg=dict(m.cfg), vocab=vocab, runtime=rt, synth_seed=3, allow_synthetic=True)
    reranker = MI355XLateReranker(lr.write_pylate_dir(tmp_path / "m", m.case, m.blob, m.proj), runtime=rt)
    rng = np.random.default_rng(11)
    root = Path("/w/demo")
    texts = [f"w{20 + i} . " + " ".join(f"w{int(j)}" for j in rng.integers(40, 400, int(rng.integers(10, 60)))) for i in range(12)]
    chunks = [Chunk(t, root / "pkg" / f"k{i}.py", "python", 1, 3) for i, t in enumerate(texts)]
    store = MilvusVectorStore(collection_name="test_late", dim=m.cfg["hidden"], metric="COSINE", index_type="FLAT", runtime=rt)
    store.connect()
    store.upsert_embeddings(build_payloads("demo", root, chunks, emb))
    r = Retriever(emb, store, reranker=reranker)
    q = "w25 w26"
    docs = r.retrieve(q, rerank=True, fetch_k=12)
    assert len(docs) == 3 and r.last_error is None
    by_path = dict(zip((f"pkg/k{i}.py" for i in range(12)), reranker.score_pairs([q] * 12, texts)))
    assert all(np.float32(d["score"]) == by_path[d["path"]] for d in docs)
    assert [d["score"] for d in docs] == sorted((float(s) for s in by_path.values()), reverse=True)[:3]
    store.close()
    reranker.close()
    emb.close()
