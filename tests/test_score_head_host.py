"""CPU: the host side of the ModernBERT / Qwen2 / Qwen3 rerankers -- the restatement against the golden files, the directory loader, the pair
builders, the score sign and the factory's dispatch.  No GPU."""
import json

import numpy as np
import pytest
from safetensors.numpy import save_file

import rerank_heads_ref as hr
from semcode_amd.embeddings import providers, reranker as rk


@pytest.fixture(scope="module")
def golden_heads(golden):
    return np.load(golden / "rerank_heads_golden.npz"), json.loads((golden / "rerank_heads_golden.json").read_text())


# ------------------------------------------------------------------ the restatement and the fixtures
def test_golden_covers_the_cases(golden_heads):
    data, meta = golden_heads
    assert list(meta) == list(hr.CASES)
    for name, case in hr.CASES.items():
        m = meta[name]
        assert m["cfg"] == case["cfg"] and m["arch"] == case["arch"] and m["num_labels"] == case["num_labels"] and not m["dropped"]
        ids, offsets = hr.make_pairs(case, m["seed"])
        assert np.array_equal(ids, data[f"{name}_ids"]) and np.array_equal(offsets, data[f"{name}_offsets"])  # the recipe rebuilds the stored pairs
        lens = np.diff(offsets).tolist()
        assert lens[:hr.N_SHAPE_PAIRS] == [3 if hr.kind_of(case) == 1 else 1] + list(hr.SHAPE_LENS) and len(lens) == hr.N_SHAPE_PAIRS + hr.N_QUESTIONS * hr.N_PASSAGES
        assert data[f"{name}_logits"].shape == (len(lens), case["num_labels"]) and data[f"{name}_rows"].shape == (len(lens), case["cfg"]["hidden"])
        assert m["T_logit"] > 0 and m["T_row"] > 0 and min(m["gap_pairs_per_question"]) >= 3
        assert all(miss > m["T_logit"] for miss in m["deviation_min_miss"].values())  # every mix-up that applies lies outside the bound
        assert set(m["deviation_min_miss"]) == {d for d in hr.deviations_of(case) if any(hr.applicable(case, d, n) for n in lens if n > 32)}


@pytest.mark.parametrize("name", list(hr.CASES))
def test_restatement_against_transformers(golden_heads, name):
    """rerank_heads_ref.forward within 1e-4 of the stored transformers rows and logits (the wide cases: the pairs up to 129 tokens)."""
    data, meta = golden_heads
    case, m = hr.CASES[name], meta[name]
    blob = hr.make_weights(case, m["seed"])
    head = hr.make_head(case, m["seed"], blob, m["head_scale"])
    ids, offsets = data[f"{name}_ids"], data[f"{name}_offsets"].astype(np.int64)
    only = [i for i in range(len(offsets) - 1) if case["cfg"]["hidden"] <= 256 or offsets[i + 1] - offsets[i] <= 129]
    rows, logits = hr.forward(case, blob, head, ids, offsets, only=only)
    assert np.abs(rows - data[f"{name}_rows"][only]).max() <= 1e-4 and np.abs(logits - data[f"{name}_logits"][only]).max() <= 1e-4
    # one mix-up of the case, on its 65-token pair: outside T_logit, as the generator recorded
    dev = "no_final_norm"
    _, wrong = hr.forward(case, blob, head, ids, offsets, deviate=dev, only=[4])
    assert np.abs(wrong - data[f"{name}_logits"][4]).max() > m["T_logit"]


def test_f32_yardstick_follows_the_head():
    """head_f32 (float32, the stated order) and head_logits (float64) are the same function: four label / bias variants at H = 128."""
    for nl, biases in ((1, False), (2, True)):
        for kind in (1, 2):
            rows, head = hr.kernel_case(33, 128, kind, nl, biases, seed=3)
            ref = hr.head_logits(head, rows)
            miss = np.abs(hr.head_f32(head, rows) - ref).max(1)
            assert miss[10:].max() <= 1e-5 * max(1.0, np.abs(ref).max())  # the ordinary rows
            assert miss[:10].max() <= 1e-2  # the rows of equal values: last-bit noise times 1 / sqrt(norm_eps) = 316
            if kind == 2:
                ref2, bound = hr.head_bound(head, rows)
                assert np.array_equal(ref, ref2) and (np.abs(hr.head_f32(head, rows) - ref) <= bound).all()


# ------------------------------------------------------------------ load_reranker_dir
TINY_MB = dict(cfg=dict(hr.MB_COMMON, hidden=128, heads=2, ffn=128, layers=2), arch="ModernBertForSequenceClassification", pooling="mean", num_labels=2,
               dense_bias=True, norm_bias=True)
TINY_Q2 = dict(cfg=dict(hr.QW_COMMON, hidden=128, heads=2, kv_heads=1, ffn=128, layers=1), arch="Qwen2ForCausalLM", pooling="last", num_labels=2, tied=True)
TINY_Q3 = dict(cfg=dict(hr.QW_COMMON, hidden=128, heads=2, kv_heads=1, ffn=128, layers=1, head_dim=128, qk_norm=True), arch="Qwen3ForCausalLM", pooling="last",
               num_labels=2, tied=False)
TOKENIZER = {"model": {"type": "BPE", "vocab": {"<pad>": 0, "y": 5, "es": 6, "no": hr.FALSE_ID, "yes": hr.TRUE_ID, "maybe": 13}},
             "added_tokens": [{"id": 20, "content": "<|true|>"}]}


def write_dir(path, case, seed=5, drop=(), config=None, tokenizer=TOKENIZER):
    blob = hr.make_weights(case, seed)
    head = hr.make_head(case, seed, blob)
    path.mkdir()
    sd = {k: v for k, v in hr.to_hf_state_dict(case, blob, head, seed).items() if k not in drop}
    save_file(sd, str(path / "model.safetensors"))
    (path / "config.json").write_text(json.dumps(dict(hr.hf_config(case), **(config or {}))))
    if tokenizer is not None:
        (path / "tokenizer.json").write_text(json.dumps(tokenizer))
    return blob, head


def same_head(got, want):
    for key in ("dense_w", "dense_b", "norm_g", "norm_b", "cls_w", "cls_b"):
        a, b = got.get(key), want.get(key)
        assert (a is None) == (b is None), key
        if a is not None:
            assert np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)), key
    assert got["kind"] == want["kind"] and got["pooling"] == want["pooling"]


def test_loader_modernbert(tmp_path):
    blob, head = write_dir(tmp_path / "mb", TINY_MB)
    cfg, got_blob, got_head, arch = rk.load_reranker_dir(tmp_path / "mb")
    assert arch == "ModernBertForSequenceClassification" and cfg == TINY_MB["cfg"]
    same_head(got_head, head)
    assert got_head["norm_eps"] == pytest.approx(1e-5)
    W, G = hr.mb.unpack(cfg, blob), hr.mb.unpack(cfg, got_blob)
    assert all(np.array_equal(W[k], G[k]) for k in W if k != "l0.ln1_g")  # (layer 0 has no attn_norm: its slot holds ones)
    # the head without the optional biases, [CLS] pooling, dispatch by model_type alone, cfg overrides
    plain = dict(TINY_MB, dense_bias=False, norm_bias=False, pooling="cls", num_labels=1)
    _, head1 = write_dir(tmp_path / "mb1", plain, config={"architectures": None})
    cfg1, _, got1, arch1 = rk.load_reranker_dir(tmp_path / "mb1", cfg={"max_pos": 512})
    assert arch1 == "ModernBertForSequenceClassification" and cfg1["max_pos"] == 512 and got1["dense_b"] is None and got1["norm_b"] is None
    same_head(got1, head1)


def test_loader_refusals(tmp_path):
    write_dir(tmp_path / "act", TINY_MB, config={"classifier_activation": "silu"})
    with pytest.raises(ValueError, match="classifier_activation 'silu'"):
        rk.load_reranker_dir(tmp_path / "act")
    write_dir(tmp_path / "pool", TINY_MB, config={"classifier_pooling": "max"})
    with pytest.raises(ValueError, match="classifier_pooling 'max'"):
        rk.load_reranker_dir(tmp_path / "pool")
    for i, name in enumerate(("head.dense.weight", "head.norm.weight", "classifier.weight", "classifier.bias", "model.final_norm.weight")):
        write_dir(tmp_path / f"miss{i}", TINY_MB, drop=(name,))
        with pytest.raises(KeyError, match=name.replace("model.", "").replace(".", r"\.")):
            rk.load_reranker_dir(tmp_path / f"miss{i}")
    write_dir(tmp_path / "arch", TINY_MB, config={"architectures": ["ModernBertForMaskedLM"]})
    with pytest.raises(ValueError, match="ModernBertForMaskedLM"):
        rk.load_reranker_dir(tmp_path / "arch")
    write_dir(tmp_path / "type", TINY_MB, config={"architectures": None, "model_type": "roberta"})
    with pytest.raises(ValueError, match="roberta"):
        rk.load_reranker_dir(tmp_path / "type")
    (tmp_path / "empty").mkdir()
    with pytest.raises(FileNotFoundError, match="config.json"):
        rk.load_reranker_dir(tmp_path / "empty")
    seqcls = dict(TINY_Q3, arch="Qwen3ForSequenceClassification", num_labels=1)
    seqcls.pop("tied")
    write_dir(tmp_path / "noscore", seqcls, drop=("score.weight",))
    with pytest.raises(KeyError, match=r"score\.weight"):
        rk.load_reranker_dir(tmp_path / "noscore")


def test_loader_causal_lm_and_seq_cls(tmp_path):
    # tied embeddings: the file has no lm_head.weight, the two rows come from the embedding table
    blob, head = write_dir(tmp_path / "tied", TINY_Q2)
    cfg, got_blob, got, arch = rk.load_reranker_dir(tmp_path / "tied")
    assert arch == "Qwen2ForCausalLM" and np.array_equal(got_blob, blob) and cfg == TINY_Q2["cfg"]
    emb = hr.q2.unpack(cfg, blob)["word_emb"]
    assert got["kind"] == 2 and got["cls_b"] is None and np.array_equal(got["cls_w"], emb[[hr.FALSE_ID, hr.TRUE_ID]])  # (false, true)
    same_head(got, head)
    # other score tokens: a vocabulary entry, an added token
    _, _, alt, _ = rk.load_reranker_dir(tmp_path / "tied", true_token="<|true|>", false_token="maybe")
    assert np.array_equal(alt["cls_w"], emb[[13, 20]])
    # untied: lm_head.weight, Qwen3 (QK-norm tensors in the blob)
    blob3, head3 = write_dir(tmp_path / "untied", TINY_Q3)
    cfg3, got_blob3, got3, arch3 = rk.load_reranker_dir(tmp_path / "untied")
    assert arch3 == "Qwen3ForCausalLM" and cfg3["qk_norm"] and cfg3["head_dim"] == 128 and np.array_equal(got_blob3, blob3)
    same_head(got3, head3)
    assert not np.array_equal(got3["cls_w"], hr.q3.unpack(cfg3, blob3)["word_emb"][[hr.FALSE_ID, hr.TRUE_ID]])
    # a "yes" that is two pieces of the vocabulary, a missing tokenizer.json
    pieces = {"model": {"vocab": {"y": 5, "es": 6, "no": 7}}, "added_tokens": []}
    write_dir(tmp_path / "pieces", TINY_Q2, tokenizer=pieces)
    with pytest.raises(ValueError, match="'yes'"):
        rk.load_reranker_dir(tmp_path / "pieces")
    write_dir(tmp_path / "notok", TINY_Q2, tokenizer=None)
    with pytest.raises(FileNotFoundError, match="tokenizer.json"):
        rk.load_reranker_dir(tmp_path / "notok")
    write_dir(tmp_path / "far", TINY_Q2, tokenizer={"model": {"vocab": {"no": 7, "yes": 400}}})
    with pytest.raises(ValueError, match="400"):
        rk.load_reranker_dir(tmp_path / "far")
    # the seq-cls conversions: a bias-free score layer, 1 or 2 labels; no tokenizer needed; model_type + score.weight decide without `architectures`
    for i, (base, arch_name) in enumerate(((TINY_Q3, "Qwen3ForSequenceClassification"), (dict(TINY_Q2), "Qwen2ForSequenceClassification"))):
        case = dict(base, arch=arch_name, num_labels=1 + i)
        case.pop("tied")
        _, head_s = write_dir(tmp_path / f"seq{i}", case, tokenizer=None, config={"architectures": None} if i else None)
        _, _, got_s, arch_s = rk.load_reranker_dir(tmp_path / f"seq{i}")
        assert arch_s == arch_name and got_s["cls_w"].shape == (1 + i, 128)
        same_head(got_s, head_s)
    three = dict(TINY_Q3, arch="Qwen3ForSequenceClassification", num_labels=3)
    three.pop("tied")
    write_dir(tmp_path / "three", three)
    with pytest.raises(ValueError, match="3 labels"):
        rk.load_reranker_dir(tmp_path / "three")


def test_vocab_token_id():
    assert rk.vocab_token_id(TOKENIZER, "yes") == hr.TRUE_ID and rk.vocab_token_id(TOKENIZER, "<|true|>") == 20
    assert rk.vocab_token_id({"model": {"vocab": [["<unk>", 0.0], ["yes", -1.0]]}}, "yes") == 1  # a Unigram list
    with pytest.raises(ValueError, match="'Yes'"):
        rk.vocab_token_id(TOKENIZER, "Yes")


# ------------------------------------------------------------------ builders
class WordTok:
    """[CLS] one id per word [SEP]; encode_plain: the words alone."""
    pad_id, cls_id, sep_id = 0, 1, 2

    def encode_plain(self, text):
        return [10 + len(w) for w in text.split()]

    def encode(self, text, max_tokens=512):
        return ([self.cls_id] + self.encode_plain(text))[: max_tokens - 1] + [self.sep_id]


def test_plain_pairs():
    tok = WordTok()
    q, passage = "aa bbb", "c dd eee ffff"
    ids, offsets = rk.build_plain_pairs(tok, [q, q, q], [passage, "", passage], max_len=8, max_query_tokens=4)
    rows = [ids[offsets[i]:offsets[i + 1]].tolist() for i in range(3)]
    assert rows[0] == [1, 12, 13, 2, 11, 12, 13, 2]      # the passage is cut, the closing [SEP] stays
    assert rows[1] == [1, 12, 13, 2]                     # an empty passage: the question alone
    assert rows[2] == rows[0] and ids.dtype == np.int32 and offsets.dtype == np.int64
    flat, off, first = rk.build_pairs(tok, [q], [passage], 8, 4)  # the same stitching as the typed builder, without its segment lengths
    assert np.array_equal(flat, ids[:8]) and first[0] == 4
    with pytest.raises(ValueError):
        rk.build_plain_pairs(tok, [q], [], 8)


def test_prompt_pairs():
    assert rk.stitch_prompt([1, 2], [5, 6, 7, 8], [9], 6) == [1, 2, 5, 6, 7, 9]   # the body is cut, prefix and suffix stay whole
    assert rk.stitch_prompt([1, 2], [5], [9], 6) == [1, 2, 5, 9]
    assert rk.stitch_prompt([1, 2], [], [9], 6) == [1, 2, 9]
    with pytest.raises(ValueError, match="no room"):
        rk.stitch_prompt([1, 2, 3], [5], [9, 9, 9], 6)
    tok = WordTok()
    template = {"prefix": "sys tem", "body": "I: {instruction} Q: {query} D: {document}", "suffix": "as sist ant", "instruction": "judge it"}
    ids, offsets = rk.build_prompt_pairs(tok.encode_plain, ["what"], ["a bb ccc"], max_len=64, template=template)
    want = tok.encode_plain("sys tem") + tok.encode_plain("I: judge it Q: what D: a bb ccc") + tok.encode_plain("as sist ant")
    assert ids.tolist() == want and offsets.tolist() == [0, len(want)]
    # another instruction; an empty passage; a body longer than the room keeps prefix and suffix whole
    ids2, _ = rk.build_prompt_pairs(tok.encode_plain, ["what"], [""], max_len=64, template=template, instruction="x")
    assert ids2.tolist() == tok.encode_plain("sys tem") + tok.encode_plain("I: x Q: what D:") + tok.encode_plain("as sist ant")
    ids3, off3 = rk.build_prompt_pairs(tok.encode_plain, ["what", "what"], ["a " * 100, "b"], max_len=12, template=template)
    first = ids3[:off3[1]].tolist()
    assert len(first) == 12 and first[:2] == tok.encode_plain("sys tem") and first[-3:] == tok.encode_plain("as sist ant")
    assert first[2:9] == tok.encode_plain("I: judge it Q: what D: a a a a")[:7]
    # the default template is the Qwen3-Reranker prompt, as data
    t = rk.QWEN3_RERANKER_TEMPLATE
    assert t["prefix"].startswith("<|im_start|>system\n") and t["suffix"].endswith("<think>\n\n</think>\n\n") and "{document}" in t["body"]
    ids4, _ = rk.build_prompt_pairs(lambda s: list(s.encode()), ["q"], ["d"], max_len=2048)
    text = bytes(ids4.tolist()).decode()
    assert text == t["prefix"] + f"<Instruct>: {t['instruction']}\n<Query>: q\n<Document>: d" + t["suffix"]


def test_scores_sign_for_false_true_rows():
    logits = np.array([[2.0, 5.0], [1.0, -1.0]], np.float32)  # columns: (false token, true token)
    s = rk.scores_from_logits(logits)
    assert s.tolist() == [3.0, -2.0]  # logit_yes - logit_no: P(yes) = sigmoid(s)
    assert np.allclose(1 / (1 + np.exp(-s)), np.exp(logits[:, 1]) / np.exp(logits).sum(1))
    assert rk.scores_from_logits(np.array([[0.5]], np.float32)).tolist() == [0.5]


def test_pair_batches_respect_the_longer_pairs():
    class Enc:
        def packed_rows(self, offsets):
            rows = int(sum((int(n) + 31) // 32 * 32 for n in np.diff(offsets)))
            if rows > 524288:
                raise AssertionError("more rows than one call may have")
            return (rows + 255) // 256 * 256

    groups = rk.cut_pair_batches(Enc(), [2048] * 600, 65536, max_len=2048)
    assert groups[0] == (0, 32) and groups[-1][1] == 600 and all(b - a <= 32 for a, b in groups)
    assert rk.cut_pair_batches(Enc(), [512] * 300, 65536) == [(0, 128), (128, 256), (256, 300)]


# ------------------------------------------------------------------ the factory
def test_create_reranker_dispatch(tmp_path, monkeypatch):
    made = []

    class Fake:
        def __init__(self, model, **kw):
            made.append((str(model), kw))

    monkeypatch.setattr(rk, "MI355XReranker", Fake)
    s = providers._resolve_settings()
    for name, value in (("mi355x_reranker_path", None), ("mi355x_reranker_instruction", "find the definition"), ("mi355x_reranker_true_token", "yes"),
                        ("mi355x_reranker_false_token", "no")):
        monkeypatch.setattr(s, name, value, raising=False)
    assert providers.create_reranker() is None  # opt-in
    d = tmp_path / "model_dir"
    d.mkdir()
    f = tmp_path / "model.safetensors"
    f.write_bytes(b"")
    providers.create_reranker(str(d))
    providers.create_reranker(str(f), rows_budget=4096)
    providers.create_reranker(str(d), instruction="mine")
    monkeypatch.setattr(s, "mi355x_reranker_path", str(d), raising=False)
    monkeypatch.setattr(s, "mi355x_reranker_instruction", "", raising=False)
    providers.create_reranker()
    assert made[0] == (str(d), dict(instruction="find the definition", true_token="yes", false_token="no"))  # a directory: prompt and tokens from the settings
    assert made[1] == (str(f), dict(rows_budget=4096))                                                       # a file: the BERT cross-encoder, as before
    assert made[2][1]["instruction"] == "mine"
    assert made[3] == (str(d), dict(true_token="yes", false_token="no"))


def test_settings_have_the_reranker_keys(monkeypatch):
    from semcode_amd.settings import Settings

    monkeypatch.setenv("SEMCODE_MI355X_RERANKER_INSTRUCTION", "Given a question, retrieve the code that answers it")
    monkeypatch.setenv("SEMCODE_MI355X_RERANKER_TRUE_TOKEN", "true")
    s = Settings()
    assert s.mi355x_reranker_instruction.startswith("Given a question") and s.mi355x_reranker_true_token == "true" and s.mi355x_reranker_false_token == "no"


# ------------------------------------------------------------------ a decoder reranker from a directory, up to the device's door
def test_causal_directory_builds_prompts_with_its_tokenizer_json(tmp_path, monkeypatch):
    """MI355XReranker(directory) of a causal LM: the loader's head, HFTokenizer on the directory's tokenizer.json, prompts through its public
    encode_plain -- no special tokens from the file's post-processor, prefix and suffix whole.  The encoder is a stand-in: no GPU."""
    from tokenizers import Tokenizer, models as tk_models, pre_tokenizers, processors

    from semcode_amd import _native
    from semcode_amd.embeddings.tokenizer import HFTokenizer

    words = ["<pad>", "<bos>", "<eos>", "<unk>", "sys", "judge", "Q:", "D:", "I:", "find", "it", "as", "ant", "where", "foo"] + [f"w{j}" for j in range(40)]
    for word, at in sorted((("no", hr.FALSE_ID), ("yes", hr.TRUE_ID)), key=lambda x: x[1]):
        words.insert(at, word)
    vocab = {w: i for i, w in enumerate(words)}
    assert vocab["no"] == hr.FALSE_ID and vocab["yes"] == hr.TRUE_ID
    blob, head = write_dir(tmp_path / "lm", TINY_Q2, tokenizer=None)
    tok = Tokenizer(tk_models.WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
    tok.post_processor = processors.TemplateProcessing(single="<bos> $A <eos>", special_tokens=[("<bos>", 1), ("<eos>", 2)])
    tok.save(str(tmp_path / "lm" / "tokenizer.json"))
    hf = HFTokenizer(tmp_path / "lm" / "tokenizer.json")
    assert hf.encode("sys judge") == [1, 4, 5, 2] and hf.encode_plain("sys judge") == [4, 5] and hf.encode_plain("") == []
    assert hf.encode_plain(" ".join(["foo"] * 600)) == [vocab["foo"]] * 600  # uncut

    made = {}

    class Enc:
        def __init__(self, runtime, cfg, weights=None):
            made.update(runtime=runtime, cfg=cfg, weights=weights)

        def set_score_head(self, h):
            made["head"] = h
            self.score_labels = h["cls_w"].shape[0]

        def close(self):
            made["closed"] = True

    monkeypatch.setattr(_native, "Encoder", Enc)
    monkeypatch.setattr(_native, "shared_runtime", lambda device: ("runtime", device))
    template = dict(prefix="sys judge", body="I: {instruction} Q: {query} D: {document}", suffix="as ant", instruction="find it")
    r = rk.MI355XReranker(tmp_path / "lm", template=template, max_pair_tokens=16)
    assert r.family == "causal" and r.num_labels == 2 and r.max_len == 16 and isinstance(r.tokenizer, HFTokenizer)
    assert np.array_equal(made["weights"], blob) and made["cfg"] == TINY_Q2["cfg"]
    same_head(made["head"], head)  # rows (no, yes) of the tied embedding
    ids, offsets = r.build_pairs(["where foo"] * 3, ["w1 w2 w3", "", " ".join(f"w{j}" for j in range(40))])
    rows = [ids[offsets[i]:offsets[i + 1]].tolist() for i in range(3)]
    enc = lambda s: [vocab[w] for w in s.split()]  # noqa: E731
    assert rows[0] == enc("sys judge I: find it Q: where foo D: w1 w2 w3 as ant")
    assert rows[1] == enc("sys judge I: find it Q: where foo D: as ant")
    assert rows[2] == enc("sys judge I: find it Q: where foo D: w0 w1 w2 w3 w4 as ant") and len(rows[2]) == 16  # the body is cut, the suffix stays
    assert not {1, 2} & set(ids.tolist())  # none of the post-processor's <bos> / <eos>
    with pytest.raises(TypeError, match="encode_plain"):
        rk.MI355XReranker(tmp_path / "lm", template=template, tokenizer=WordTokNoPlain()).build_pairs(["a"], ["b"])


class WordTokNoPlain:
    pad_id = 0

    def encode(self, text, max_tokens=512):
        return [1, 2]
