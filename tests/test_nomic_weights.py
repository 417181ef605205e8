"""CPU: nomic-bert weights from GGUF and .safetensors, and the provider's task prefixes.

GGUF: no nomic GGUF and no llama.cpp exist offline, so the tensor names (fused blk.N.attn_qkv, ffn_gate / ffn_up, no Linear bias,
nomic-bert.rope.freq_base) are restated from the published converter and exercised on files this test writes ("parity unpinned").
.safetensors: pinned -- a random transformers NomicBertModel is saved, loaded through load_weight_blob and run through
tests/nomic_ref.forward, which must reproduce the model's own output."""
import numpy as np
import pytest

import nomic_ref as nr
from oracle import bert_oracle as bo
from semcode_amd.embeddings import gguf
from semcode_amd.embeddings.providers import MI355XEmbeddings, load_weight_blob
from semcode_amd.embeddings.tokenizer import WordPieceTokenizer

TINY = dict(vocab=300, hidden=128, layers=2, heads=2, ffn=256, max_pos=2048, type_vocab=2, ln_eps=1e-12, rotary=True, swiglu=True)


def nomic_gguf_tensors(cfg, blob, fused=True):
    """the blob as llama.cpp-named nomic-bert tensors, written independently of gguf_to_blob"""
    u = bo.unpack(nr.layout_cfg(cfg), blob)
    F = cfg["ffn"]
    t = {"token_embd.weight": u["word_emb"], "token_types.weight": u["type_emb"], "token_embd_norm.weight": u["emb_ln_g"], "token_embd_norm.bias": u["emb_ln_b"]}
    for l in range(cfg["layers"]):
        p, b = f"l{l}.", f"blk.{l}."
        if fused:
            t[b + "attn_qkv.weight"] = np.concatenate([u[p + "wq"], u[p + "wk"], u[p + "wv"]], axis=0)
        else:
            t[b + "attn_q.weight"], t[b + "attn_k.weight"], t[b + "attn_v.weight"] = u[p + "wq"], u[p + "wk"], u[p + "wv"]
        t[b + "attn_output.weight"] = u[p + "wo"]
        t[b + "attn_output_norm.weight"], t[b + "attn_output_norm.bias"] = u[p + "ln1_g"], u[p + "ln1_b"]
        t[b + "ffn_gate.weight"], t[b + "ffn_up.weight"], t[b + "ffn_down.weight"] = u[p + "w1"][:F], u[p + "w1"][F:], u[p + "w2"]
        t[b + "layer_output_norm.weight"], t[b + "layer_output_norm.bias"] = u[p + "ln2_g"], u[p + "ln2_b"]
    return t


def nomic_gguf_meta(cfg, freq_base=500.0, tokens=None):
    a = "nomic-bert"
    m = {"general.architecture": a, "general.name": "test", f"{a}.block_count": cfg["layers"], f"{a}.embedding_length": cfg["hidden"],
         f"{a}.feed_forward_length": cfg["ffn"], f"{a}.attention.head_count": cfg["heads"], f"{a}.context_length": cfg["max_pos"],
         f"{a}.attention.layer_norm_epsilon": float(cfg["ln_eps"]), f"{a}.attention.causal": False}
    if freq_base is not None:
        m[f"{a}.rope.freq_base"] = float(freq_base)
    if tokens is not None:
        m["tokenizer.ggml.model"] = "bert"
        m["tokenizer.ggml.tokens"] = tokens
        m["tokenizer.ggml.token_type"] = [3 if t.startswith("[") else 1 for t in tokens]
    return m


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_nomic_gguf_gives_the_source_blob_back(tmp_path, dtype):
    cfg = dict(TINY)
    blob = nr.make_weights(cfg, 11)
    path = tmp_path / f"nomic-{dtype}.gguf"
    gguf.write_gguf(path, nomic_gguf_meta(cfg), nomic_gguf_tensors(cfg, blob), dtype=dtype)
    meta, _ = gguf.read_gguf(path)
    fcfg = gguf.gguf_config(meta)
    assert (fcfg["hidden"], fcfg["layers"], fcfg["heads"], fcfg["ffn"], fcfg["max_pos"]) == (128, 2, 2, 256, 2048)
    assert fcfg["rotary"] is True and fcfg["swiglu"] is True and fcfg["rope_theta"] == 500.0 and not fcfg["alibi"] and not fcfg["geglu"]
    got = load_weight_blob(path, cfg["layers"], cfg)
    want = blob if dtype == "f32" else blob.astype(np.float16).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == blob.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # split attn_q / attn_k / attn_v: the same blob
    split = tmp_path / f"nomic-split-{dtype}.gguf"
    gguf.write_gguf(split, nomic_gguf_meta(cfg), nomic_gguf_tensors(cfg, blob, fused=False), dtype=dtype)
    assert np.array_equal(load_weight_blob(split, cfg["layers"], cfg).view(np.uint32), want.view(np.uint32))


def test_nomic_gguf_details(tmp_path):
    cfg = dict(TINY)
    blob = nr.make_weights(cfg, 12)
    t = nomic_gguf_tensors(cfg, blob)
    # rope.freq_base absent: 1000, the family's default
    gguf.write_gguf(tmp_path / "d.gguf", nomic_gguf_meta(cfg, freq_base=None), t)
    assert gguf.gguf_config(gguf.read_gguf(tmp_path / "d.gguf")[0])["rope_theta"] == 1000.0
    # a Linear bias that IS in the file is used
    t2 = dict(t)
    t2["blk.1.ffn_down.bias"] = np.arange(cfg["hidden"], dtype=np.float32)
    gguf.write_gguf(tmp_path / "b.gguf", nomic_gguf_meta(cfg), t2)
    got = bo.unpack(nr.layout_cfg(cfg), load_weight_blob(tmp_path / "b.gguf", 2, cfg))
    assert np.array_equal(got["l1.b2"], np.arange(cfg["hidden"], dtype=np.float32)) and not got["l0.b2"].any()
    # against an encoder configuration of another family: refused
    for other in (dict(cfg, rotary=False, swiglu=False), dict(cfg, rotary=False, swiglu=False, alibi=True, geglu=True), dict(cfg, swiglu=False)):
        with pytest.raises(ValueError, match="nomic-bert"):
            load_weight_blob(tmp_path / "d.gguf", 2, other)
    # and a BERT / jina configuration file is still refused for a nomic configuration
    bcfg = dict(bo.BERT_BASE, vocab=300, hidden=128, layers=2, heads=2, ffn=256, max_pos=64)
    from test_gguf import gguf_meta, gguf_tensors

    gguf.write_gguf(tmp_path / "bert.gguf", gguf_meta(bcfg), gguf_tensors(bcfg, bo.make_blob(bcfg, 3, "test")))
    with pytest.raises(ValueError, match="BERT"):
        load_weight_blob(tmp_path / "bert.gguf", 2, dict(bcfg, rotary=True, swiglu=True))


def test_transformers_nomic_bert_safetensors_round_trip(tmp_path):
    """NomicBertModel (random init) -> state_dict -> .safetensors -> load_weight_blob -> nomic_ref.forward == the model's output."""
    torch = pytest.importorskip("torch")
    try:
        from transformers import NomicBertConfig, NomicBertModel
    except ImportError:
        pytest.skip("this transformers has no nomic_bert")
    from safetensors.numpy import save_file

    cfg = dict(TINY, vocab=200, max_pos=128)
    torch.manual_seed(3)
    hc = NomicBertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                         intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], type_vocab_size=2, layer_norm_eps=cfg["ln_eps"],
                         hidden_act="silu", initializer_range=0.2, rope_parameters={"rope_type": "default", "rope_theta": 1000.0})
    hc._attn_implementation = "eager"
    model = NomicBertModel(hc, add_pooling_layer=False).eval()
    with torch.no_grad():  # non-trivial LayerNorm parameters too
        for n, p in model.named_parameters():
            if "LayerNorm" in n or "layernorm" in n:
                p.add_(0.3 * torch.randn_like(p))
    sd = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(2)
    ids = rng.integers(1, cfg["vocab"], size=(3, 64)).astype(np.int32)
    lens = np.array([64, 31, 3], np.int32)
    mask = (np.arange(64)[None] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        h = model(input_ids=torch.from_numpy(ids.astype(np.int64)), attention_mask=torch.from_numpy(mask)).last_hidden_state.double().numpy()
    want = np.stack([h[b, : lens[b]].mean(0) for b in range(3)]).astype(np.float32)
    for prefix in ("", "nomic_bert."):
        path = tmp_path / f"m{len(prefix)}.safetensors"
        save_file({prefix + k: v for k, v in sd.items()}, str(path))
        blob = load_weight_blob(path, cfg["layers"], cfg)
        assert blob.size == bo.blob_size(nr.layout_cfg(cfg))
        got = nr.forward(cfg, blob, ids, lens, 1000.0)
        assert np.abs(got - want).max() <= 1e-5, np.abs(got - want).max()
    with pytest.raises(ValueError, match="nomic-bert"):
        load_weight_blob(path, cfg["layers"], dict(cfg, rotary=False, swiglu=False))


class _StubEncoder:
    def close(self):
        pass


def _client(tmp_path, **kw):
    """MI355XEmbeddings' tokenising half without a device: the object is built around the Python WordPiece tokenizer only."""
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "search", "_", "query", "document", ":", "x", "y", "##s"]) + "\n")
    emb = MI355XEmbeddings.__new__(MI355XEmbeddings)
    emb.max_tokens, emb.truncated_texts, emb.total_texts = 32, 0, 0
    emb.tokenizer, emb._fast_tokenizer = WordPieceTokenizer(vocab), None
    emb.document_prefix, emb.query_prefix = kw.get("document_prefix", ""), kw.get("query_prefix", "")
    return emb


def test_task_prefixes(tmp_path):
    plain = _client(tmp_path)
    ids0, lens0 = plain.tokenize(["x", "y xs"])
    for kind in ("document", "query"):  # empty prefixes: today's ids
        ids, lens = plain.tokenize(["x", "y xs"], kind=kind)
        assert np.array_equal(ids, ids0) and np.array_equal(lens, lens0)
    emb = _client(tmp_path, query_prefix="search_query: ", document_prefix="search_document: ")
    q, ql = emb.tokenize(["x"], kind="query")
    want, wl = plain.tokenize(["search_query: x"])
    assert np.array_equal(q, want) and np.array_equal(ql, wl) and ql[0] > lens0[0]
    d, dl = emb.tokenize(["x"])  # kind defaults to "document": what services.indexer.ingest_chunks calls
    want, wl = plain.tokenize(["search_document: x"])
    assert np.array_equal(d, want) and np.array_equal(dl, wl)
    assert not np.array_equal(q, d)
    with pytest.raises(ValueError):
        emb.tokenize(["x"], kind="passage")
