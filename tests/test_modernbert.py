"""CPU: the ModernBERT family outside the device -- the numpy restatement against the committed transformers vectors, the deviations
the fixtures must tell apart, the .safetensors + config.json loader, the blob size the library expects, and the tokenizer.json wrapper.

Tolerances: tests/golden/modernbert_golden.json carries T (mean) and T_cls ([CLS]) per case, twice what transformers' own bf16 forward
misses its fp32 forward by (scripts/gen_modernbert_fixtures.py); the restatement itself must land within 1e-5 of the fp32 vectors."""
import ctypes as C
import json

import numpy as np
import pytest

import modernbert_ref as mr
from semcode_amd import _native
from semcode_amd.embeddings.providers import load_weight_blob, modernbert_config, modernbert_config_beside
from semcode_amd.embeddings.tokenizer import HFTokenizer, pack


@pytest.fixture(scope="module")
def mb_golden(golden):
    return np.load(golden / "modernbert_golden.npz"), json.loads((golden / "modernbert_golden.json").read_text())


def weights_of(m):
    return mr.make_weights(m["cfg"], m["seed"], m["qk_scale"], m["vo_scale"], m["mlp_scale"], m["global_qk"])


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


SMALL = ["w128_short", "w32_s128", "w16_s64", "w32_l7", "w32_s32"]  # the cases a float64 forward of which takes well under a second


def test_golden_covers_the_cases_the_kernels_need(mb_golden):
    data, meta = mb_golden
    lens = np.concatenate([data[f"{n}_lens"] for n in meta])
    assert {3, 33, 65, 66, 129, 300, 513, 600, 1100} <= set(lens.tolist())
    assert {m["S"] for m in meta.values()} >= {32, 64, 128, 256, 512, 1024, 2048}
    assert {m["cfg"]["local_window"] for m in meta.values()} >= {16, 32, 128}
    assert {(m["cfg"]["hidden"], m["cfg"]["heads"]) for m in meta.values()} >= {(128, 2), (256, 4), (768, 12)}
    assert any(m["cfg"]["layers"] == 7 for m in meta.values()) and any(m["cfg"]["global_every"] == 2 for m in meta.values())
    assert any(m["cfg"]["ffn"] == 1152 for m in meta.values())


@pytest.mark.parametrize("name", SMALL + ["w128"])
def test_restatement_reproduces_transformers(mb_golden, name):
    data, meta = mb_golden
    m = meta[name]
    blob, ids, lens = weights_of(m), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    for pooling in ("mean", "cls"):
        d = np.abs(mr.forward(m["cfg"], blob, ids, lens, pooling) - data[f"{name}_{pooling}"]).max()
        assert d <= 1e-5, (pooling, d)


@pytest.mark.parametrize("name", SMALL)
def test_every_deviation_misses_the_tolerance(mb_golden, name):
    data, meta = mb_golden
    m = meta[name]
    cfg, blob, ids, lens = m["cfg"], weights_of(m), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    long_ = lens > cfg["local_window"]
    for dev in mr.DEVIATIONS:
        d, cos = miss(mr.forward(cfg, blob, ids, lens, deviate=dev), data[f"{name}_mean"])
        outside = (d > m["T"]) | (cos < 0.999)
        assert outside[long_].all(), (dev, d, m["T"])
        if dev in ("no_window", "window_m2"):  # a text the window covers whole cannot tell
            assert (d[lens <= cfg["local_window"] // 2 - 1] <= 1e-5).all(), (dev, d)


def test_stored_deviation_misses_exceed_T_in_every_case(mb_golden):
    """What the generator measured before it wrote the files (it refuses otherwise), for the cases too long to redo here."""
    _, meta = mb_golden
    for name, m in meta.items():
        for dev in mr.DEVIATIONS:
            v = m["deviation_min_miss"][dev]
            assert v is None or v > m["T"], (name, dev, v, m["T"])


def test_safetensors_loader_round_trip(tmp_path):
    from safetensors.numpy import save_file

    cfg = dict(vocab=300, hidden=128, layers=4, heads=2, ffn=256, max_pos=1024, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True,
               local_window=32, global_every=3, rope_theta=160000.0, rope_theta_local=10000.0)
    blob = mr.make_weights(cfg, 5)
    for prefix, sub in (("", "plain"), ("model.", "prefixed")):
        d = tmp_path / sub
        d.mkdir()
        save_file({prefix + k: v for k, v in mr.to_hf_state_dict(cfg, blob).items()}, str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps(mr.hf_config(cfg)))
        got_cfg = modernbert_config_beside(d / "model.safetensors")
        assert got_cfg == cfg
        got = load_weight_blob(d / "model.safetensors", cfg["layers"], got_cfg)
        want = blob.copy()
        mr.unpack(cfg, want)["l0.ln1_g"][:] = 1.0  # the file has no attn_norm for layer 0: the slot nobody reads is filled with ones
        assert got.dtype == np.float32 and np.array_equal(got, want)
    with pytest.raises(ValueError, match="ModernBERT checkpoint"):
        load_weight_blob(tmp_path / "plain" / "model.safetensors", cfg["layers"], dict(cfg, modernbert=False))


def test_config_forms():
    base = mr.hf_config(dict(vocab=300, hidden=128, layers=6, heads=2, ffn=256, max_pos=1024, ln_eps=1e-5, local_window=128, global_every=3,
                             rope_theta=160000.0, rope_theta_local=10000.0))
    want = modernbert_config(base)
    assert (want["global_every"], want["local_window"], want["rope_theta"], want["rope_theta_local"]) == (3, 128, 160000.0, 10000.0)
    new = {k: v for k, v in base.items() if k not in ("global_attn_every_n_layers", "global_rope_theta", "local_rope_theta")}
    new["layer_types"] = ["full_attention" if l % 3 == 0 else "sliding_attention" for l in range(6)]
    new["rope_parameters"] = {"full_attention": {"rope_type": "default", "rope_theta": 160000.0}, "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}}
    assert modernbert_config(new) == want
    with pytest.raises(ValueError, match="layer_types"):
        modernbert_config(dict(new, layer_types=["sliding_attention"] + new["layer_types"][1:]))
    with pytest.raises(ValueError, match="layer_types"):
        modernbert_config(dict(new, layer_types=["full_attention", "full_attention", "sliding_attention"] * 2))


def test_blob_bytes_of_an_arch1_cfg_equal_the_loaders_blob():
    cfg = dict(vocab=300, hidden=128, layers=3, heads=2, ffn=256, max_pos=1024, type_vocab=1, ln_eps=1e-5, rotary=True, geglu=True, modernbert=True,
               local_window=128, global_every=3, rope_theta=160000.0, rope_theta_local=10000.0)
    c = _native.encoder_cfg(cfg)
    assert (c.arch, c.local_window, c.global_every, c.rope_theta_local) == (1, 128, 3, 10000.0)
    need = C.c_int64()
    assert _native.lib().sc_encoder_blob_bytes(C.byref(c), C.byref(need)) == 0
    assert need.value == mr.blob_size(cfg) * 4 == mr.make_weights(cfg, 1).nbytes
    # the same shape as a post-LN rotary + GEGLU model: a type table more, no final_norm
    need0 = C.c_int64()
    assert _native.lib().sc_encoder_blob_bytes(C.byref(_native.encoder_cfg(dict(cfg, modernbert=False, local_window=0, global_every=0))), C.byref(need0)) == 0
    assert need.value - need0.value == (2 * 128 - 1 * 128) * 4


def test_hf_tokenizer(tmp_path):
    tk = pytest.importorskip("tokenizers")
    from tokenizers import decoders, models, pre_tokenizers, processors, trainers

    tok = tk.Tokenizer(models.BPE(unk_token=None))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=400, special_tokens=["[PAD]", "[CLS]", "[SEP]", "[UNK]"], initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    tok.train_from_iterator(["def forward(self, hidden_states):", "return self.norm(hidden_states)", "for i in range(len(xs)): total += xs[i]"] * 4, trainer)
    cls_id, sep_id = tok.token_to_id("[CLS]"), tok.token_to_id("[SEP]")
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", cls_id), ("[SEP]", sep_id)])
    path = tmp_path / "tokenizer.json"
    tok.save(str(path))

    t = HFTokenizer(path)
    assert t.pad_id == tok.token_to_id("[PAD]") == 0 and t.vocab_size == tok.get_vocab_size()
    text = "def forward(self, xs): return self.norm(xs)"
    ids = t.encode(text, 512)
    assert ids == tok.encode(text).ids and ids[0] == cls_id and ids[-1] == sep_id and len(ids) > 8
    assert tok.decode(ids[1:-1]) == text  # byte-level: nothing is lost, no [UNK]
    cut = t.encode(text, 8)
    assert len(cut) == 8 and cut[:7] == ids[:7] and cut[-1] == sep_id  # truncated to max_tokens, still closed
    assert t.encode(text, len(ids)) == ids
    packed, lens = pack([t.encode(text, 32), t.encode("x", 32)], t.pad_id, 32)
    assert packed.shape == (2, 32) and lens.tolist() == [len(t.encode(text, 32)), 3] and (packed[1, 3:] == t.pad_id).all()
    other = tk.Tokenizer(models.BPE())  # a file without [PAD]: <pad> is found, else 0
    other.add_special_tokens(["<s>", "<pad>"])
    other.save(str(tmp_path / "other.json"))
    assert HFTokenizer(tmp_path / "other.json").pad_id == 1
