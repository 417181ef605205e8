"""CPU: the host half of head dimension 32 -- where the loaders take the head count from, and the numpy reference the GPU tests lean on
at a head width other than 64."""
import json

import numpy as np

import minilm_ref as mr
from oracle import bert_oracle as bo
from semcode_amd.embeddings import gguf
from semcode_amd.embeddings import reranker as rk


def hf_bert(cfg, cls, **kw):
    from transformers import BertConfig

    hc = BertConfig(vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                    intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], type_vocab_size=cfg["type_vocab"], layer_norm_eps=cfg["ln_eps"],
                    hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hc._attn_implementation = "eager"
    return cls(hc, **kw).eval()


def test_load_reranker_takes_the_head_count_from_config_json(tmp_path):
    import torch
    from safetensors.numpy import save_file
    from transformers import BertForSequenceClassification

    cfg = dict(vocab=50, hidden=128, layers=1, heads=4, ffn=128, max_pos=40, type_vocab=2, ln_eps=1e-12)
    torch.manual_seed(3)
    model = hf_bert(cfg, BertForSequenceClassification)
    save_file({k: v.detach().numpy().copy() for k, v in model.state_dict().items()}, str(tmp_path / "model.safetensors"))
    got, _, _ = rk.load_reranker(tmp_path / "model.safetensors")
    assert got["heads"] == 2 and got["hidden"] == 128  # no config.json: hidden // 64, as before
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "bert", "hidden_size": 128, "num_attention_heads": 4}))
    got, blob, head = rk.load_reranker(tmp_path / "model.safetensors")
    assert {k: got[k] for k in cfg} == cfg
    assert blob.size == bo.blob_size(cfg) and head["cls_w"].shape == (2, 128)
    got, _, _ = rk.load_reranker(tmp_path / "model.safetensors", cfg=dict(heads=2))  # the caller's cfg wins over the file
    assert got["heads"] == 2
    (tmp_path / "config.json").write_text(json.dumps({"model_type": "bert"}))  # a config.json that does not say: the fallback
    assert rk.load_reranker(tmp_path / "model.safetensors")[0]["heads"] == 2


def test_gguf_config_passes_the_head_count_through():
    meta = {"general.architecture": "bert", "bert.embedding_length": 384, "bert.block_count": 6, "bert.attention.head_count": 12,
            "bert.feed_forward_length": 1536, "bert.context_length": 512, "bert.attention.layer_norm_epsilon": 1e-12}
    cfg = gguf.gguf_config(meta)
    assert (cfg["hidden"], cfg["heads"], cfg["layers"], cfg["ffn"], cfg["max_pos"]) == (384, 12, 6, 1536, 512)
    assert not cfg["alibi"] and not cfg.get("rotary")


def test_bert_oracle_at_head_dimension_32_equals_transformers():
    """oracle.bert_oracle.forward derives the head width from hidden / heads; the GPU tests of head dimension 32 rely on that."""
    import torch
    from transformers import BertModel

    cfg = dict(mr.COMMON, hidden=128, heads=4, ffn=256)
    blob = mr.make_weights(cfg, 3)
    ids, lens, _ = mr.make_inputs(cfg, 3)
    model = hf_bert(cfg, BertModel, add_pooling_layer=False)
    missing = model.load_state_dict(bo.to_hf_state_dict(cfg, blob), strict=False)
    assert not missing.missing_keys and not missing.unexpected_keys
    want = np.empty((len(lens), 128), np.float32)
    with torch.no_grad():
        for i, n in enumerate(lens):
            want[i] = model(input_ids=torch.from_numpy(ids[i, :n].astype(np.int64))[None]).last_hidden_state[0].mean(0).numpy()
    got = bo.forward(cfg, blob, ids, lens)
    assert np.abs(got - want).max() <= 1e-5, np.abs(got - want).max()
    wrong = bo.forward(dict(cfg, heads=2), blob, ids, lens)  # the same weights as two heads of 64: far away
    assert np.abs(wrong - want).max(1).min() > 0.1
