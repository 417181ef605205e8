"""CPU: the Qwen2 family (sc_encoder_cfg.arch 2) outside the device -- the numpy restatement against the committed transformers
vectors, the deviations the fixtures must tell apart, the blob size the library expects, the create rules that need no device, the
config.json -> cfg mapping, the .safetensors loader and the pooling a model directory states.

Tolerances: tests/golden/qwen2_golden.json carries T_last and T_mean per case, twice what transformers' own bf16 forward misses its fp32
forward by (scripts/gen_qwen2_fixtures.py); the restatement itself must land within 1e-5 of the fp32 vectors."""
import ctypes as C
import json

import numpy as np
import pytest

import qwen2_ref as qr
from semcode_amd import _native
from semcode_amd.embeddings.providers import load_weight_blob, qwen2_config, qwen2_config_beside, resolve_pooling


@pytest.fixture(scope="module")
def q2_golden(golden):
    return np.load(golden / "qwen2_golden.npz"), json.loads((golden / "qwen2_golden.json").read_text())


def weights_of(m):
    return qr.make_weights(m["cfg"], m["seed"], m["qk_scale"], m["bias_sigma"], m["vo_scale"], m["mlp_scale"], m["emb_scale"], m["norm_sigma"], m["bias_first"])


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


SMALL = ["g2_s64", "mha_s128", "g2_s256", "mqa_s128"]  # the cases a float64 forward of which takes well under a second
BASE = dict(vocab=300, hidden=128, layers=2, heads=2, kv_heads=1, ffn=256, max_pos=1024, type_vocab=1, ln_eps=1e-6, rotary=True, swiglu=True, qwen2=True,
            rope_theta=1000000.0)


def test_golden_covers_the_cases_the_kernels_need(q2_golden):
    data, meta = q2_golden
    lens = np.concatenate([data[f"{n}_lens"] for n in meta])
    assert {1, 31, 32, 33, 65, 129, 513, 600, 1100} <= set(lens.tolist())
    assert {m["S"] for m in meta.values()} >= {64, 128, 256, 1024, 2048}
    shapes = {(m["cfg"]["hidden"], m["cfg"]["heads"], m["cfg"]["kv_heads"], m["cfg"]["ffn"]) for m in meta.values()}
    assert shapes >= {(128, 2, 1, 256), (128, 2, 2, 256), (256, 4, 2, 512), (256, 4, 1, 512), (896, 14, 2, 4864)}
    assert any(m["cfg"]["layers"] == 3 for m in meta.values())
    assert all(m["bf16_cos"] >= 0.99975 for m in meta.values())  # the model's own bf16 forward leaves room under the 0.999 floor


@pytest.mark.parametrize("name", SMALL + ["half_b"])
def test_restatement_reproduces_transformers(q2_golden, name):
    data, meta = q2_golden
    m = meta[name]
    blob, ids, lens = weights_of(m), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    for pooling in ("last", "mean"):
        d = np.abs(qr.forward(m["cfg"], blob, ids, lens, pooling) - data[f"{name}_{pooling}"]).max()
        assert d <= 1e-5, (pooling, d)


@pytest.mark.parametrize("name", SMALL)
def test_every_deviation_misses_the_tolerance(q2_golden, name):
    data, meta = q2_golden
    m = meta[name]
    cfg, blob, ids, lens = m["cfg"], weights_of(m), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    long_ = lens > 32
    assert long_.any()
    for dev in qr.DEVIATIONS:
        if dev == "kv_interleaved" and cfg["kv_heads"] in (1, cfg["heads"]):
            continue  # the two mappings coincide
        d, cos = miss(qr.forward(cfg, blob, ids, lens, "last", deviate=dev), data[f"{name}_last"])
        outside = (d > m["T_last"]) | (cos < 0.999)
        assert outside[long_].all(), (dev, d, m["T_last"])
        if dev in ("no_mask", "mask_p1", "base_10000", "k_unrotated"):  # a text of one token cannot tell
            assert (d[lens == 1] <= 1e-5).all(), (dev, d)


def test_stored_deviation_misses_exceed_T_in_every_case(q2_golden):
    """What the generator measured before it wrote the files (it refuses otherwise), for the cases too long to redo here."""
    _, meta = q2_golden
    for name, m in meta.items():
        want = set(qr.DEVIATIONS) - ({"kv_interleaved"} if m["cfg"]["kv_heads"] in (1, m["cfg"]["heads"]) else set())
        assert set(m["deviation_min_miss"]) == want, name
        for dev, v in m["deviation_min_miss"].items():
            assert v is not None and v > m["T_last"], (name, dev, v, m["T_last"])


@pytest.mark.parametrize("change", [dict(), dict(kv_heads=2), dict(hidden=896, heads=14, kv_heads=2, ffn=4864, layers=3, vocab=500)])
def test_blob_bytes_equal_the_documented_formula(change):
    cfg = dict(BASE, **change)
    c = _native.encoder_cfg(cfg)
    assert (c.arch, c.kv_heads, c.pos_type, c.ffn_type) == (2, cfg["kv_heads"], 2, 2)
    need = C.c_int64()
    assert _native.lib().sc_encoder_blob_bytes(C.byref(c), C.byref(need)) == 0
    H, F, KV, L = cfg["hidden"], cfg["ffn"], cfg["kv_heads"] * 64, cfg["layers"]
    per_layer = (H * H + H) + 2 * (KV * H + KV) + (H * H + H) + 2 * H + (2 * F * H + 2 * F) + (H * F + H) + 2 * H
    assert need.value == 4 * (cfg["vocab"] * H + L * per_layer + 2 * H) == qr.blob_size(cfg) * 4 == qr.make_weights(cfg, 1).nbytes
    zero = C.c_int64()  # kv_heads 0 means heads
    assert _native.lib().sc_encoder_blob_bytes(C.byref(_native.encoder_cfg(dict(cfg, kv_heads=0))), C.byref(zero)) == 0
    assert zero.value == qr.blob_size(dict(cfg, kv_heads=cfg["heads"])) * 4


def create_error(cfg: dict) -> "tuple[int, str]":
    """sc_encoder_create's answer to a configuration it refuses.  The rules are checked before the runtime is touched, so a stand-in
    handle does: no device is needed (a configuration that passes would be an error of this test, and is not tried)."""
    c = _native.encoder_cfg(cfg)
    stand_in = C.create_string_buffer(4096)
    out = C.c_void_p()
    st = _native.lib().sc_encoder_create(C.cast(stand_in, C.c_void_p), C.byref(c), None, 0, C.byref(out))
    assert st != 0 and not out.value
    buf = C.create_string_buffer(512)
    _native.lib().sc_last_error(buf, 512)
    return st, buf.value.decode()


def test_create_rules_name_the_field():
    status = {"SC_ERR_INVALID": None, "SC_ERR_UNSUPPORTED": None}
    import re
    from pathlib import Path

    header = (Path(__file__).resolve().parent.parent / "include" / "semcode_hip.h").read_text()
    for name in status:
        status[name] = int(re.search(name + r"\s*=\s*(-?\d+)", header).group(1))
    for change, words in ((dict(rotary=False), ("arch 2", "pos_type")), (dict(rotary=False, alibi=True), ("arch 2", "pos_type")),
                          (dict(swiglu=False), ("arch 2", "ffn_type")), (dict(swiglu=False, geglu=True), ("arch 2", "ffn_type")),
                          (dict(heads=4), ("head dimension",)), (dict(heads=1, kv_heads=1), ("head dimension",)), (dict(kv_heads=3), ("kv_heads", "3")),
                          (dict(heads=2, kv_heads=4), ("kv_heads",)), (dict(kv_heads=-1), ("kv_heads",)), (dict(local_window=64), ("local_window",)),
                          (dict(global_every=3), ("global_every",)), (dict(ffn=200), ("ffn",)), (dict(hidden=2176, heads=34, kv_heads=2), ("hidden",))):
        st, msg = create_error(dict(BASE, **change))
        assert st in (status["SC_ERR_INVALID"], status["SC_ERR_UNSUPPORTED"]), (change, st)
        assert all(w in msg for w in words), (change, msg)
    for other in (dict(qwen2=False), dict(qwen2=False, modernbert=True, swiglu=False, geglu=True, local_window=32, global_every=3)):  # kv_heads on arch 0, 1
        st, msg = create_error(dict(BASE, **other))
        assert st == status["SC_ERR_UNSUPPORTED"] and "kv_heads" in msg and "arch 2" in msg, (other, st, msg)
    c = _native.encoder_cfg(BASE)
    c.arch = 3
    out = C.c_void_p()
    assert _native.lib().sc_encoder_create(C.cast(C.create_string_buffer(4096), C.c_void_p), C.byref(c), None, 0, C.byref(out)) == status["SC_ERR_INVALID"]


def test_cfg_dict_forms():
    assert _native.POOLINGS_QWEN2 == {"mean": 0, "last": 2} and "last" not in _native.POOLINGS  # "last" on arch 2 only, "cls" never there
    assert _native.encoder_cfg(dict(BASE, kv_heads=None)).kv_heads == 0
    assert _native.encoder_cfg(dict(_native.BERT_BASE)).kv_heads == 0 and _native.encoder_cfg(dict(_native.BERT_BASE)).arch == 0
    with pytest.raises(ValueError, match="pick one"):
        _native.encoder_cfg(dict(BASE, modernbert=True))


def test_config_json_mapping(tmp_path):
    hf = qr.hf_config(dict(BASE, max_pos=32768))
    got = qwen2_config(hf)
    assert got == dict(BASE, max_pos=2048, vocab=300)  # max_position_embeddings is capped at the 2 048 tokens a text may have
    assert qwen2_config(dict(hf, max_position_embeddings=512))["max_pos"] == 512
    assert qwen2_config({k: v for k, v in hf.items() if k != "num_key_value_heads"})["kv_heads"] == 2  # absent: multi-head
    assert qwen2_config(dict(hf, use_sliding_window=True, sliding_window=4096))["max_pos"] == 2048  # a window no text reaches
    with pytest.raises(ValueError, match="sliding_window"):
        qwen2_config(dict(hf, use_sliding_window=True, sliding_window=1024))
    with pytest.raises(ValueError, match="Qwen2"):
        qwen2_config(dict(hf, model_type="llama"))
    (tmp_path / "config.json").write_text(json.dumps(hf))
    (tmp_path / "model.safetensors").write_bytes(b"")
    assert qwen2_config_beside(tmp_path / "model.safetensors") == got
    (tmp_path / "config.json").write_text(json.dumps(dict(hf, model_type="bert")))
    assert qwen2_config_beside(tmp_path / "model.safetensors") is None


def test_safetensors_loader_round_trip(tmp_path):
    from safetensors.numpy import save_file

    cfg = dict(BASE, hidden=256, heads=4, kv_heads=2, ffn=512)
    blob = qr.make_weights(cfg, 5)
    for prefix, sub in (("", "plain"), ("model.", "prefixed")):
        d = tmp_path / sub
        d.mkdir()
        save_file(qr.to_hf_state_dict(cfg, blob, prefix), str(d / "model.safetensors"))
        (d / "config.json").write_text(json.dumps(qr.hf_config(cfg)))
        got_cfg = qwen2_config_beside(d / "model.safetensors")
        assert got_cfg == cfg
        got = load_weight_blob(d / "model.safetensors", cfg["layers"], got_cfg)
        assert got.dtype == np.float32 and np.array_equal(got, blob)  # bit for bit: the zero slots are zero in make_weights too
    with pytest.raises(ValueError, match="Qwen2 checkpoint"):
        load_weight_blob(tmp_path / "plain" / "model.safetensors", cfg["layers"], dict(cfg, qwen2=False))
    with pytest.raises(ValueError, match="heads of 64"):
        load_weight_blob(tmp_path / "plain" / "model.safetensors", cfg["layers"], dict(cfg, kv_heads=1))


def test_pooling_of_a_model_directory(tmp_path):
    w = tmp_path / "model.safetensors"
    w.write_bytes(b"")
    assert resolve_pooling(weights=w) == "mean"
    (tmp_path / "1_Pooling").mkdir()
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False, "pooling_mode_lasttoken": True}))
    assert resolve_pooling(weights=w) == "last"
    assert resolve_pooling("mean", weights=w) == "mean"
    for given in (("last", None), (None, "last")):  # as an argument or a setting: for a Qwen2 directory only
        with pytest.raises(ValueError, match="Qwen2"):
            resolve_pooling(*given, weights=w)
        with pytest.raises(ValueError, match="Qwen2"):
            resolve_pooling(*given)
    (tmp_path / "config.json").write_text(json.dumps(qr.hf_config(BASE)))
    assert resolve_pooling("last", None, w) == "last" and resolve_pooling(None, " Last ", w) == "last"


def test_new_symbols_are_exported():
    lib = _native.lib()
    for name in ("sc_diag_attention_run", "sc_diag_rmsnorm"):
        assert name in _native.SIGNATURES and getattr(lib, name) is not None
    assert [f[0] for f in _native.EncoderCfg._fields_][-1] == "kv_heads"
