"""CPU: heads of 128 and QK-norm on the causal decoder pipeline (sc_encoder_cfg.arch 2 with head_dim / qk_norm: Qwen3-Embedding,
Qwen2.5-1.5B) outside the device -- the numpy restatement against the committed transformers vectors, the mix-ups the fixtures must tell
apart, the blob size the library expects, the create rules that need no device, the config.json -> cfg mappings, the .safetensors loader
with the q_norm / k_norm tensors present, missing and unexpected, and the pooling a Qwen3 directory states.

Tolerances: tests/golden/qwen3_golden.json carries T_last and T_mean per case, twice what transformers' own bf16 forward misses its fp32
forward by (scripts/gen_qwen3_fixtures.py); the restatement itself must land within 1e-5 of the fp32 vectors."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import qwen3_ref as q3
from semcode_amd import _native
from semcode_amd.embeddings.providers import load_weight_blob, qwen2_config, qwen2_config_beside, qwen3_config, resolve_pooling


@pytest.fixture(scope="module")
def q3_golden(golden):
    return np.load(golden / "qwen3_golden.npz"), json.loads((golden / "qwen3_golden.json").read_text())


def weights_of(m):
    return q3.make_weights(m["cfg"], m["seed"], *m["scales"])


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


SMALL = ["n_aw2h", "n_g2", "b_mha"]  # the cases a float64 forward of which takes well under a second
BASE = dict(vocab=300, hidden=128, layers=2, heads=2, kv_heads=1, ffn=256, max_pos=1024, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True,
            rope_theta=1000000.0, head_dim=128, qk_norm=True)  # AW = 256 = 2 hidden


def test_golden_covers_the_cases_the_issue_lists(q3_golden):
    data, meta = q3_golden
    shapes = {(m["cfg"]["hidden"], m["cfg"]["heads"], m["cfg"]["kv_heads"], m["cfg"]["ffn"], bool(m["cfg"]["qk_norm"])) for m in meta.values()}
    assert shapes == {(128, 2, 1, 256, True), (256, 4, 2, 512, True), (256, 2, 2, 512, False), (256, 2, 1, 512, True), (1024, 16, 8, 3072, True), (1536, 12, 2, 8960, False)}
    assert all(m["cfg"]["head_dim"] == 128 for m in meta.values())
    lens = set(np.concatenate([data[f"{n}_lens"] for n in meta]).tolist())
    assert {1, 31, 32, 33, 65, 129, 300, 1100} <= lens
    assert meta["n_s2048"]["S"] == 2048 and meta["n_s2048"]["cfg"]["layers"] == 4 and len(data["n_s2048_lens"]) == 3
    assert meta["n_06b"]["cfg"]["layers"] == 2 and meta["b_15b"]["cfg"]["layers"] == 1
    assert all(m["bf16_cos"] >= 0.99975 for m in meta.values())  # the model's own bf16 forward leaves room under the 0.999 floor


@pytest.mark.parametrize("name", SMALL + ["n_06b", "b_15b"])
def test_restatement_reproduces_transformers(q3_golden, name):
    data, meta = q3_golden
    m = meta[name]
    blob, ids, lens = weights_of(m), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    for pooling in ("last", "mean"):
        d = np.abs(q3.forward(m["cfg"], blob, ids, lens, pooling) - data[f"{name}_{pooling}"]).max()
        assert d <= 1e-5, (pooling, d)


@pytest.mark.parametrize("name", SMALL)
def test_every_mix_up_misses_the_tolerance(q3_golden, name):
    data, meta = q3_golden
    m = meta[name]
    cfg, blob, ids, lens = m["cfg"], weights_of(m), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    long_ = lens > 32
    assert long_.any() and not m["dropped"]
    for dev in q3.DEVIATIONS:
        if not q3.applicable(cfg, dev):
            continue
        d, cos = miss(q3.forward(cfg, blob, ids, lens, "last", deviate=dev), data[f"{name}_last"])
        outside = (d > m["T_last"]) | (cos < 0.999)
        assert outside[long_].all(), (dev, d, m["T_last"])
        if dev in ("no_mask", "mask_p1", "kv_interleaved") or (dev == "norm_after_rope"):  # a text of one token (position 0) cannot tell
            assert (d[lens == 1] <= 1e-5).all(), (dev, d)


def test_stored_mix_up_misses_are_within_the_generators_rules(q3_golden):
    """What the generator measured before it wrote the files (it refuses otherwise): every mix-up that applies to a case is recorded, lands
    outside (T_last, cos 0.999) on every text longer than 32 tokens, or is listed as dropped for that case with its reason."""
    _, meta = q3_golden
    for name, m in meta.items():
        want = {d for d in q3.DEVIATIONS if q3.applicable(m["cfg"], d)}
        assert set(m["deviation_min_miss"]) == want == set(m["deviation_max_cos"]), name
        assert set(m["dropped"]) <= want and all(len(r) > 20 for r in m["dropped"].values())
        for dev in want - set(m["dropped"]):
            assert m["deviation_min_miss"][dev] > m["T_last"] or m["deviation_max_cos"][dev] < 0.999, (name, dev, m["deviation_min_miss"][dev], m["T_last"])
    assert {n: sorted(m["dropped"]) for n, m in meta.items() if m["dropped"]} == {"b_15b": ["mask_p1", "no_mask"], "n_s2048": ["mask_p1"]}


@pytest.mark.parametrize("change", [dict(), dict(qk_norm=False, hidden=256, ffn=512, heads=2, kv_heads=2), dict(head_dim=64, hidden=128, heads=2, kv_heads=1),
                                    dict(hidden=1024, heads=16, kv_heads=8, ffn=3072, layers=3, vocab=500)])
def test_blob_bytes_equal_the_documented_formula(change):
    """The three layouts: heads of 128 with q_norm / k_norm slots (AW = 2 hidden, and the 0.6B width), heads of 128 without them, heads of 64
    stated with them."""
    cfg = dict(BASE, **change)
    c = _native.encoder_cfg(cfg)
    assert (c.arch, c.kv_heads, c.head_dim, c.qk_norm) == (2, cfg["kv_heads"], cfg["head_dim"], int(cfg["qk_norm"]))
    need = C.c_int64()
    assert _native.lib().sc_encoder_blob_bytes(C.byref(c), C.byref(need)) == 0
    H, F, L, hd = cfg["hidden"], cfg["ffn"], cfg["layers"], cfg["head_dim"]
    AW, KV = cfg["heads"] * hd, cfg["kv_heads"] * hd
    per_layer = (AW * H + AW) + 2 * (KV * H + KV) + (H * AW + H) + 2 * H + (2 * F * H + 2 * F) + (H * F + H) + 2 * H + (2 * hd if cfg["qk_norm"] else 0)
    assert need.value == 4 * (cfg["vocab"] * H + L * per_layer + 2 * H) == q3.blob_size(cfg) * 4 == q3.make_weights(cfg, 1).nbytes
    if not cfg["qk_norm"] and hd == 64:
        return
    plain = C.c_int64()  # all-zero new fields: the size of the struct without them
    assert _native.lib().sc_encoder_blob_bytes(C.byref(_native.encoder_cfg(dict(cfg, head_dim=0, qk_norm=False, hidden=cfg["heads"] * 64))), C.byref(plain)) == 0
    import qwen2_ref as qr

    assert plain.value == qr.blob_size(dict(cfg, hidden=cfg["heads"] * 64)) * 4


def create_error(cfg: dict, **raw) -> "tuple[int, str]":
    """sc_encoder_create's answer to a configuration it refuses.  The rules are checked before the runtime is touched, so a stand-in
    handle does: no device is needed (a configuration that passes would be an error of this test, and is not tried)."""
    c = _native.encoder_cfg(cfg)
    for k, v in raw.items():
        setattr(c, k, v)
    stand_in = C.create_string_buffer(4096)
    out = C.c_void_p()
    st = _native.lib().sc_encoder_create(C.cast(stand_in, C.c_void_p), C.byref(c), None, 0, C.byref(out))
    assert st != 0 and not out.value
    buf = C.create_string_buffer(512)
    _native.lib().sc_last_error(buf, 512)
    return st, buf.value.decode()


def test_create_rules_name_the_field():
    header = (Path(__file__).resolve().parent.parent / "include" / "semcode_hip.h").read_text()
    INVALID, UNSUPPORTED = (int(re.search(n + r"\s*=\s*(-?\d+)", header).group(1)) for n in ("SC_ERR_INVALID", "SC_ERR_UNSUPPORTED"))
    st, msg = create_error(dict(BASE, heads=17, kv_heads=17))  # heads * 128 > 2048
    assert st == UNSUPPORTED and "head_dim 128" in msg and "2048" in msg and "17" in msg
    st, msg = create_error(dict(BASE, head_dim=96))
    assert st == UNSUPPORTED and "head_dim" in msg and "96" in msg
    st, msg = create_error(BASE, qk_norm=2)
    assert st == INVALID and "qk_norm" in msg
    for other in (dict(qwen2=False, kv_heads=0, hidden=128, heads=2), dict(qwen2=False, modernbert=True, swiglu=False, geglu=True, local_window=32, global_every=3, kv_heads=0)):
        for field in (dict(head_dim=64, qk_norm=False), dict(head_dim=128, qk_norm=False), dict(head_dim=0, qk_norm=True)):  # on arch 0 / 1, by name
            st, msg = create_error(dict(BASE, **other, **field))
            name = "head_dim" if field["head_dim"] else "qk_norm"
            assert st == UNSUPPORTED and name in msg and "arch 2" in msg, (other, field, st, msg)
    # head_dim 0 keeps every refusal of today: 128-wide heads are never derived from hidden / heads, with or without qk_norm
    for change in (dict(hidden=128, heads=1, kv_heads=1), dict(hidden=256, heads=2, kv_heads=1), dict(hidden=128, heads=4)):
        for qkn in (False, True):
            st, msg = create_error(dict(BASE, head_dim=0, qk_norm=qkn, **change))
            assert st == UNSUPPORTED and "head dimension" in msg, (change, msg)
    st, msg = create_error(dict(BASE, head_dim=64, hidden=256, heads=2))  # 64 stated: hidden must be heads * 64
    assert st == UNSUPPORTED and "head dimension" in msg
    # ... and the rules of arch 2 hold at 128 as well
    for change, words in ((dict(kv_heads=3), ("kv_heads", "3")), (dict(rotary=False), ("arch 2", "pos_type")), (dict(swiglu=False), ("arch 2", "ffn_type")),
                          (dict(local_window=64), ("local_window",)), (dict(ffn=200), ("ffn",)), (dict(hidden=2176), ("hidden",))):
        st, msg = create_error(dict(BASE, **change))
        assert st in (INVALID, UNSUPPORTED) and all(w in msg for w in words), (change, msg)


def test_cfg_dict_forms():
    c = _native.encoder_cfg(dict(BASE, head_dim=None, qk_norm=None))
    assert (c.head_dim, c.qk_norm) == (0, 0)
    c = _native.encoder_cfg(dict(_native.BERT_BASE))
    assert (c.head_dim, c.qk_norm, c.kv_heads, c.arch) == (0, 0, 0, 0)
    # the whole struct: EncoderCfg's fields, then the two appended ones; every EncoderCfg that is constructed is one (the library writes all 88 bytes)
    assert [f[0] for f in _native.EncoderCfgFull._fields_] == ["head_dim", "qk_norm"] and issubclass(_native.EncoderCfgFull, _native.EncoderCfg)
    assert C.sizeof(_native.EncoderCfgFull) == 88 and _native.EncoderCfgFull.head_dim.offset == 80 and _native.EncoderCfgFull.qk_norm.offset == 84
    for made in (_native.EncoderCfg(), _native.EncoderCfg(vocab=5, kv_heads=2), _native.encoder_cfg(BASE)):
        assert type(made) is _native.EncoderCfgFull and C.sizeof(made) == 88
    assert (_native.EncoderCfg(vocab=5, kv_heads=2, qk_norm=1).kv_heads, _native.EncoderCfg(head_dim=128).head_dim) == (2, 128)
    lib = _native.lib()
    for name in ("sc_diag_attention_run", "sc_diag_qknorm_rope"):
        assert name in _native.SIGNATURES and getattr(lib, name) is not None


def test_config_json_mappings(tmp_path):
    hf = q3.hf_config(dict(BASE, max_pos=32768))
    assert hf["model_type"] == "qwen3" and hf["head_dim"] == 128
    got = qwen3_config(hf)
    assert got == dict(BASE, max_pos=2048)  # max_position_embeddings is capped at the 2 048 tokens a text may have
    assert qwen3_config(dict(hf, max_position_embeddings=512))["max_pos"] == 512
    assert qwen3_config({k: v for k, v in hf.items() if k != "head_dim"})["head_dim"] == 64  # absent: hidden_size / num_attention_heads
    assert qwen3_config(dict(hf, layer_types=["full_attention"] * 2)) == got
    assert qwen3_config(dict(hf, use_sliding_window=True, sliding_window=4096))["max_pos"] == 2048  # a window no text reaches
    with pytest.raises(ValueError, match="sliding_window"):
        qwen3_config(dict(hf, use_sliding_window=True, sliding_window=1024))
    with pytest.raises(ValueError, match="sliding_attention"):
        qwen3_config(dict(hf, layer_types=["full_attention", "sliding_attention"]))
    with pytest.raises(ValueError, match="Qwen3"):
        qwen3_config(dict(hf, model_type="qwen2"))
    with pytest.raises(ValueError, match="head_dim 96"):
        qwen3_config(dict(hf, head_dim=96))
    # Qwen2.5-1.5B: heads of 128 from hidden_size / num_attention_heads (or a stated head_dim), no qk_norm; the 0.5B reading is unchanged
    hf2 = q3.hf_config(dict(BASE, qk_norm=False, hidden=1536, heads=12, kv_heads=2, ffn=8960))
    assert hf2["model_type"] == "qwen2" and "head_dim" not in hf2
    got2 = qwen2_config(hf2)
    assert got2["head_dim"] == 128 and "qk_norm" not in got2 and (got2["hidden"], got2["heads"], got2["kv_heads"]) == (1536, 12, 2)
    assert qwen2_config(dict(hf2, head_dim=128)) == got2
    assert "head_dim" not in qwen2_config(dict(hf2, hidden_size=768))
    (tmp_path / "config.json").write_text(json.dumps(hf))
    (tmp_path / "model.safetensors").write_bytes(b"")
    assert qwen2_config_beside(tmp_path / "model.safetensors") == got  # a qwen3 directory is a causal directory
    (tmp_path / "config.json").write_text(json.dumps(hf2))
    assert qwen2_config_beside(tmp_path / "model.safetensors") == got2


def test_safetensors_loader_with_and_without_the_norm_tensors(tmp_path):
    from safetensors.numpy import save_file

    cfg = dict(BASE, hidden=256, heads=4, kv_heads=2, ffn=512)
    blob = q3.make_weights(cfg, 5)
    for prefix, sub in (("", "plain"), ("model.", "prefixed")):
        d = tmp_path / sub
        d.mkdir()
        save_file(q3.to_hf_state_dict(cfg, blob, prefix), str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps(q3.hf_config(cfg)))
        got_cfg = qwen2_config_beside(d / "model.safetensors")
        assert got_cfg == cfg
        got = load_weight_blob(d / "model.safetensors", cfg["layers"], got_cfg)
        assert got.dtype == np.float32 and np.array_equal(got, blob)  # bit for bit: the zero slots are zero in make_weights too
    with pytest.raises(ValueError, match=r"unexpected tensor 'layers\.0\.self_attn\.q_norm\.weight'"):  # a Qwen3 file under a configuration without qk_norm
        load_weight_blob(tmp_path / "plain" / "model.safetensors", cfg["layers"], dict(cfg, qk_norm=False))
    sd = q3.to_hf_state_dict(cfg, blob)
    (tmp_path / "missing").mkdir()
    save_file({k: v for k, v in sd.items() if k != "layers.1.self_attn.k_norm.weight"}, str(tmp_path / "missing" / "model.safetensors"))
    with pytest.raises(ValueError, match=r"'layers\.1\.self_attn\.k_norm\.weight'.*not found"):
        load_weight_blob(tmp_path / "missing" / "model.safetensors", cfg["layers"], cfg)
    with pytest.raises(ValueError, match="heads of 128"):
        load_weight_blob(tmp_path / "plain" / "model.safetensors", cfg["layers"], dict(cfg, kv_heads=1))
    with pytest.raises(ValueError, match="projections are"):  # the widths come from the configuration: this file's q_proj is [512, 256]
        load_weight_blob(tmp_path / "plain" / "model.safetensors", cfg["layers"], dict(cfg, head_dim=64))
    # Qwen2.5-1.5B's kind: heads of 128 with biases, no norm tensors
    cfg2 = dict(BASE, qk_norm=False, hidden=256, heads=2, kv_heads=2, ffn=512)
    blob2 = q3.make_weights(cfg2, 6)
    (tmp_path / "q2").mkdir()
    save_file(q3.to_hf_state_dict(cfg2, blob2, "model."), str(tmp_path / "q2" / "model.safetensors"))
    (tmp_path / "q2" / "config.json").write_text(json.dumps(q3.hf_config(cfg2)))
    got_cfg = qwen2_config_beside(tmp_path / "q2" / "model.safetensors")
    assert got_cfg == {k: v for k, v in cfg2.items() if k != "qk_norm"}
    assert np.array_equal(load_weight_blob(tmp_path / "q2" / "model.safetensors", 2, got_cfg), blob2)


def test_pooling_of_a_qwen3_directory(tmp_path):
    w = tmp_path / "model.safetensors"
    w.write_bytes(b"")
    with pytest.raises(ValueError, match="Qwen2"):
        resolve_pooling("last", None, w)
    (tmp_path / "config.json").write_text(json.dumps(q3.hf_config(BASE)))
    assert resolve_pooling("last", None, w) == "last" and resolve_pooling(None, " Last ", w) == "last"
    assert resolve_pooling(weights=w) == "mean"
    (tmp_path / "1_Pooling").mkdir()
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False, "pooling_mode_lasttoken": True}))
    assert resolve_pooling(weights=w) == "last"
