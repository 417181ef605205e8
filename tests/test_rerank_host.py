"""CPU: the host half of the reranker -- pair stitching and truncation against transformers' BertTokenizer, the safetensors name
mapping against BertForSequenceClassification.state_dict(), the score rules, and Retriever(rerank=...) with a dummy reranker."""
import numpy as np
import pytest

from semcode_amd.embeddings import reranker as rk
from semcode_amd.embeddings.tokenizer import WordPieceTokenizer
from semcode_amd.services import Retriever
from semcode_amd.settings import settings
from tests.test_retrieval import WordEmbedder, filled_store

WORDS = ["def", "class", "return", "parse", "##r", "##s", "config", "load", "token", "##izer", "index", "search", "where", "is", "the", "defined",
         "(", ")", ":", "_", ".", "self", "path", "file", "open", "read", "a", "b", "c", "x", "y"]


@pytest.fixture(scope="module")
def vocab_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("rerank_vocab") / "vocab.txt"
    p.write_text("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS) + "\n", encoding="utf-8")
    return p


def hf_pair(hf, q, p, max_len, max_query_tokens):
    """BertTokenizer(q, p, truncation="only_second") with the question first cut to its own budget."""
    q_tokens = hf.convert_ids_to_tokens(hf(q, truncation=True, max_length=max_query_tokens)["input_ids"][1:-1])
    q_cut = hf.convert_tokens_to_string(q_tokens)  # (the pieces of this text are q_tokens again: every cut word is in the vocabulary)
    assert hf.tokenize(q_cut) == q_tokens
    enc = hf(q_cut, p, truncation="only_second", max_length=max_len, return_token_type_ids=True)
    return enc["input_ids"], enc["token_type_ids"]


def test_pairs_match_bert_tokenizer(vocab_file):
    from transformers import BertTokenizer

    hf = BertTokenizer(str(vocab_file), do_lower_case=True)
    tok = WordPieceTokenizer(str(vocab_file))
    long_q = " ".join(["where is the parser config defined"] * 6)  # 36+ pieces: cut to the question budget
    long_p = " ".join(["def load ( self , path ) : return open ( path ) . read ( )"] * 8)
    cases = [("where is parser defined", "class parser : def parse ( self ) : return self . tokens", 64, 16),
             (long_q, "def parse ( x )", 64, 16),
             ("where is parser defined", long_p, 64, 16),       # passage cut to what is left
             (long_q, long_p, 20, 18),                           # question takes 18 of 20: the passage is cut to ONE token
             ("index search", "", 64, 16),                       # empty passage: the question alone
             ("Tokenizer.load_config", "Where IS it", 512, 64)]  # upper case, punctuation, word pieces
    for q, p, max_len, mq in cases:
        flat, offsets, first = rk.build_pairs(tok, [q], [p], max_len=max_len, max_query_tokens=mq)
        want_ids, want_types = hf_pair(hf, q, p, max_len, mq)
        assert flat.tolist() == want_ids, (q, p)
        assert offsets.tolist() == [0, len(want_ids)] and len(want_ids) <= max_len
        types = (np.arange(len(flat)) >= first[0]).astype(int).tolist()
        assert types == want_types, (q, p)
    flat, offsets, first = rk.build_pairs(tok, [long_q], [long_p], max_len=20, max_query_tokens=18)
    assert first[0] == 18 and offsets[1] == 20  # one passage token + the closing [SEP]
    # several pairs, one question: the layout of the packed call
    flat, offsets, first = rk.build_pairs(tok, ["index search"] * 3, ["a b", "c", "x y a b"], max_len=64, max_query_tokens=16)
    assert offsets.tolist() == [0, 7, 13, 22] and first.tolist() == [4, 4, 4] and flat.dtype == np.int32
    assert rk.pair_limits(512) == (512, 64) and rk.pair_limits(2048) == (512, 64) and rk.pair_limits(40, 64) == (40, 38)


@pytest.mark.parametrize("num_labels,pooler", [(1, True), (2, True), (1, False)])
def test_safetensors_names_of_sequence_classification(tmp_path, num_labels, pooler):
    import torch
    from safetensors.numpy import save_file
    from transformers import BertConfig, BertForSequenceClassification

    from oracle import bert_oracle as bo

    cfg = dict(vocab=50, hidden=64, layers=2, heads=1, ffn=128, max_pos=40, type_vocab=2, ln_eps=1e-12)
    hc = BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, max_position_embeddings=40,
                    type_vocab_size=2, num_labels=num_labels)
    torch.manual_seed(5)
    model = BertForSequenceClassification(hc)
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items() if pooler or not k.startswith("bert.pooler.")}
    save_file(sd, str(tmp_path / "m.safetensors"))
    got_cfg, blob, head = rk.load_reranker(tmp_path / "m.safetensors")
    assert {k: got_cfg[k] for k in cfg} == cfg
    W = bo.unpack(cfg, blob)
    assert np.array_equal(W["type_emb"], sd["bert.embeddings.token_type_embeddings.weight"])
    assert np.array_equal(W["l1.wv"], sd["bert.encoder.layer.1.attention.self.value.weight"])
    assert np.array_equal(W["l1.ln2_b"], sd["bert.encoder.layer.1.output.LayerNorm.bias"])
    assert np.array_equal(head["cls_w"], sd["classifier.weight"]) and head["cls_w"].shape == (num_labels, 64)
    assert np.array_equal(head["cls_b"], sd["classifier.bias"])
    if pooler:
        assert np.array_equal(head["pooler_w"], sd["bert.pooler.dense.weight"]) and np.array_equal(head["pooler_b"], sd["bert.pooler.dense.bias"])
    else:
        assert head["pooler_w"] is None and head["pooler_b"] is None
    del sd["classifier.weight"]
    save_file(sd, str(tmp_path / "bare.safetensors"))
    with pytest.raises(KeyError, match="classifier"):
        rk.load_reranker(tmp_path / "bare.safetensors")


def test_score_rules():
    assert rk.scores_from_logits(np.array([[0.5], [-2.0]], np.float32)).tolist() == [0.5, -2.0]
    assert rk.scores_from_logits(np.array([[1.0, 3.0], [2.0, -1.0]], np.float32)).tolist() == [2.0, -3.0]  # label 1 = relevant
    with pytest.raises(ValueError):
        rk.scores_from_logits(np.zeros((2, 3), np.float32))


class DummyReranker:
    """Scores a snippet by a table; counts its calls."""

    def __init__(self, table, fail=False):
        self.table, self.fail, self.calls = table, fail, []

    def score_pairs(self, questions, passages):
        self.calls.append((list(questions), list(passages)))
        if self.fail:
            raise RuntimeError("reranker down")
        return np.asarray([self.table.get(p, 0.0) for p in passages], np.float32)


class SpyStore:
    """A store with the reference's surface only; records how it is called."""

    def __init__(self):
        self.inner, self.calls = filled_store(), []

    def connect(self):
        pass

    def search(self, vector, top_k=10, **kw):
        self.calls.append(("search", top_k, kw))
        return self.inner.search(vector, top_k=top_k)


def test_retriever_reranks(monkeypatch):
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    monkeypatch.setattr(settings, "mi355x_rerank_fetch_k", 5, raising=False)
    emb, store = WordEmbedder(), filled_store()
    plain = Retriever(emb, store).retrieve("alpha")
    assert [d["path"] for d in plain] == ["src/f0.py", "src/f1.py", "src/f6.py"]
    five = Retriever(emb, store)
    monkeypatch.setattr(settings, "rag_max_context_sources", 5)
    fetched = five.retrieve("alpha")  # what the store returns for fetch_k = 5, in retrieval order
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    # the hit at retrieval rank 3 gets the best score; ranks 0 and 2 tie: the tie keeps retrieval order
    table = {fetched[3]["snippet"]: 9.0, fetched[0]["snippet"]: 1.0, fetched[2]["snippet"]: 1.0, fetched[1]["snippet"]: -4.0, fetched[4]["snippet"]: 0.5}
    rr_ = DummyReranker(table)
    r = Retriever(emb, store, reranker=rr_)
    docs = r.retrieve("alpha", rerank=True)
    assert [d["path"] for d in docs] == [fetched[3]["path"], fetched[0]["path"], fetched[2]["path"]] and r.last_error is None
    assert [d["score"] for d in docs] == [9.0, 1.0, 1.0]
    assert [d["retrieval_score"] for d in docs] == [fetched[3]["score"], fetched[0]["score"], fetched[2]["score"]]
    assert rr_.calls == [(["alpha"] * 5, [d["snippet"] for d in fetched])]
    # rerank None / False: today's documents, no reranker call
    assert r.retrieve("alpha") == plain and r.retrieve("alpha", rerank=False) == plain and len(rr_.calls) == 1
    # the batch form: all questions' pairs in ONE score_pairs call, per question the single-question result
    both = r.retrieve_batch(["alpha", "gamma"], rerank=True)
    assert len(rr_.calls) == 2 and len(rr_.calls[1][0]) == 10 and rr_.calls[1][0][:5] == ["alpha"] * 5 and rr_.calls[1][0][5:] == ["gamma"] * 5
    assert both[0] == docs and both[1] == r.retrieve("gamma", rerank=True)
    assert r.retrieve_batch(["alpha", "gamma"]) == Retriever(emb, store).retrieve_batch(["alpha", "gamma"])


def test_retriever_fetch_k_and_store_arguments(monkeypatch):
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    monkeypatch.setattr(settings, "mi355x_rerank_fetch_k", 40, raising=False)
    store = SpyStore()
    r = Retriever(WordEmbedder(), store, reranker=DummyReranker({}))
    r.retrieve("alpha")
    r.retrieve("alpha", repos=["demo"], fetch_k=6, mmr=0.5)
    assert store.calls == [("search", 3, {}), ("search", 3, {"repos": ["demo"], "mmr": 0.5, "fetch_k": 6})]  # exactly today's arguments
    store.calls.clear()
    assert len(r.retrieve("alpha", rerank=True)) == 3          # the setting: 40 asked, 7 stored, 3 returned
    assert len(r.retrieve("alpha", rerank=True, fetch_k=4, repos=["demo"], group_by="path", hybrid=True)) == 3
    assert len(r.retrieve("alpha", rerank=True, fetch_k=1)) == 3  # at least top_k
    assert store.calls == [("search", 40, {}), ("search", 4, {"repos": ["demo"], "group_by": "path", "hybrid": True, "query_text": "alpha"}),
                           ("search", 3, {})]


def test_retriever_rerank_errors(monkeypatch):
    monkeypatch.setattr(settings, "rag_max_context_sources", 3)
    emb, store = WordEmbedder(), SpyStore()
    with pytest.raises(ValueError, match="reranker"):
        Retriever(emb, store).retrieve("alpha", rerank=True)
    with pytest.raises(ValueError, match="reranker"):
        Retriever(emb, store).retrieve_batch(["alpha"], rerank=True)
    r = Retriever(emb, store, reranker=DummyReranker({}))
    with pytest.raises(ValueError, match="mmr"):
        r.retrieve("alpha", rerank=True, mmr=0.5)
    with pytest.raises(ValueError, match="mmr"):
        r.retrieve_batch(["alpha"], rerank=True, mmr=0.5)
    assert store.calls == [] and emb.calls == []  # raised before anything ran
    bad = Retriever(emb, filled_store(), reranker=DummyReranker({}, fail=True))
    assert bad.retrieve("alpha", rerank=True) == [] and isinstance(bad.last_error, RuntimeError)
    assert bad.retrieve_batch(["alpha", "beta"], rerank=True) == [[], []] and isinstance(bad.last_error, RuntimeError)
    assert len(bad.retrieve("alpha")) == 3 and bad.last_error is None


def test_batches_never_ask_for_more_rows_than_a_call_may_have():
    """cut_pair_batches hands packed_rows at most 1 024 pairs at a time (it refuses more than 524 288 rows), and covers every pair."""
    class Rows:
        def packed_rows(self, offsets):
            lens = np.diff(offsets)
            used = int(((lens + 31) // 32 * 32).sum())
            assert (used + 255) // 256 * 256 <= 524288
            return (used + 255) // 256 * 256

    lens = np.full(5000, 512)
    lens[::7] = 33
    groups = rk.cut_pair_batches(Rows(), lens, 65536)
    assert groups[0][0] == 0 and groups[-1][1] == 5000 and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    assert all(Rows().packed_rows(np.concatenate(([0], np.cumsum(lens[a:b])))) <= 65536 for a, b in groups)


def test_native_tokenizer_path_builds_the_same_pairs(vocab_file, tmp_path):
    """What a reranker with a vocab.txt PATH runs: encode_many through the C++ tokenizer, at both budgets build_pairs asks for (the
    question's, and max_len - 1 with its 512 bucket), gives the ids of the Python tokenizer -- and so the same pairs."""
    from functools import partial

    from semcode_amd import _native

    tok, fast = WordPieceTokenizer(str(vocab_file)), _native.NativeTokenizer(str(vocab_file))
    long_q = " ".join(["where is the parser config defined"] * 6)
    long_p = " ".join(["def load ( self , path ) : return open ( path ) . read ( )"] * 40)  # more than 511 pieces
    texts = ["where is parser defined", long_q, long_p, "", "Tokenizer.load_config", "café tokens 中", "x" * 150]
    for max_tokens in (16, 64, 511):
        got = rk.encode_many(tok, fast, texts, max_tokens)
        assert got == [tok.encode(t, max_tokens) for t in texts], max_tokens
        assert all(isinstance(i, int) for ids in got for i in ids) and max(len(ids) for ids in got) == max_tokens
    assert rk.encode_many(tok, fast, [], 64) == [] and rk.encode_many(tok, None, texts, 64) == [tok.encode(t, 64) for t in texts]
    qs, ps = [long_q, "index search", long_q, "where is parser defined"], [long_p, "", "def parse ( x )", long_p]
    for max_len, mq in ((512, 64), (20, 18)):
        slow = rk.build_pairs(tok, qs, ps, max_len=max_len, max_query_tokens=mq)
        quick = rk.build_pairs(tok, qs, ps, max_len=max_len, max_query_tokens=mq, encode_many=partial(rk.encode_many, tok, fast))
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(slow, quick))
        assert int(np.diff(slow[1]).max()) == max_len
    fast.close()
    fast.close()  # idempotent: MI355XReranker.close() closes it too


def test_checkpoint_without_position_table_needs_cfg(tmp_path):
    from safetensors.numpy import save_file
    from transformers import BertConfig, BertForSequenceClassification

    hc = BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128, max_position_embeddings=40, type_vocab_size=2, num_labels=1)
    sd = {k: v.detach().numpy().copy() for k, v in BertForSequenceClassification(hc).state_dict().items() if "position_embeddings" not in k}
    save_file(sd, str(tmp_path / "nopos.safetensors"))
    with pytest.raises(ValueError, match="max_pos"):
        rk.load_reranker(tmp_path / "nopos.safetensors")
