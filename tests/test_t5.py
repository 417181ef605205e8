"""CPU: the T5 encoder (sc_encoder_cfg.arch 3) outside the device -- the library's bucket rule against transformers' own integers, the
numpy restatement against the committed transformers vectors, the mix-ups the fixtures must tell apart, the blob size the library expects,
the create rules that need no device, the struct's appended fields and the config.json -> cfg mapping.

Tolerances: tests/golden/t5_golden.json carries T_first and T_mean per case, twice what transformers' own bf16 forward misses its fp32
forward by (scripts/gen_t5_fixtures.py); the restatement itself must land within 1e-5 of the fp32 vectors."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import t5_ref as tr
from semcode_amd import _native
from semcode_amd.embeddings.providers import t5_config


@pytest.fixture(scope="module")
def t5_golden(golden):
    return np.load(golden / "t5_golden.npz"), json.loads((golden / "t5_golden.json").read_text())


def miss(got, want):
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return np.abs(got - want).max(1), cos


SMALL = ["relu_s64", "b16_s128", "gated_s512", "aw128_s128", "dense_mean"]  # the cases a float64 forward of which takes about a second
BASE = dict(vocab=300, hidden=128, layers=2, heads=2, ffn=256, max_pos=1024, type_vocab=1, ln_eps=1e-6, t5=True, t5_ffn="relu", rel_buckets=32, rel_max_distance=128)


@pytest.mark.parametrize("buckets,max_distance", [(32, 128), (16, 32), (32, 64)])
def test_bucket_rule_gives_transformers_integers(t5_golden, buckets, max_distance):
    """sc_diag_rel_buckets -- the function that builds the device table -- against T5Attention._relative_position_bucket for the distances
    -2047 .. 2047, bin edges included: exactly."""
    want = t5_golden[0][f"buckets_{buckets}_{max_distance}"].astype(np.int32)
    got = _native.diag_rel_buckets(buckets, max_distance, 2048)
    assert got.shape == want.shape == (4095,) and np.array_equal(got, want), np.nonzero(got != want)[0][:8] - 2047
    assert np.array_equal(tr.buckets(np.arange(-2047, 2048), buckets, max_distance), want)  # the restatement's too
    assert got[2047] == 0 and got[2048] == buckets // 2 + 1 and got.max() == buckets - 1  # key behind the query: the upper half
    short = _native.diag_rel_buckets(buckets, max_distance, 5)
    assert np.array_equal(short, want[2047 - 4:2047 + 5])
    for bad in ((31, 128, 8), (32, 8, 8), (2, 128, 8), (32, 128, 0)):
        with pytest.raises(_native.ScError):
            _native.diag_rel_buckets(*bad)


def test_golden_covers_the_cases_the_kernels_need(t5_golden):
    data, meta = t5_golden
    lens = np.concatenate([data[f"{n}_lens"] for n in meta])
    assert {1, 31, 32, 33, 65, 129, 300, 513, 600, 1100} <= set(lens.tolist())
    assert {m["S"] for m in meta.values()} >= {64, 128, 512, 1024, 2048}
    forms = {(m["cfg"]["hidden"], m["cfg"]["heads"], m["cfg"]["t5_ffn"], m["cfg"]["rel_buckets"], m["cfg"].get("head_dim", 0)) for m in meta.values()}
    assert forms >= {(128, 2, "relu", 32, 0), (128, 2, "relu", 16, 0), (256, 4, "gated-gelu", 32, 0), (256, 2, "gated-gelu", 32, 64), (768, 12, "relu", 32, 0)}
    assert all(m["bf16_cos"] >= 0.99975 for m in meta.values())  # the model's own bf16 forward leaves room under the 0.999 floor
    for name, m in meta.items():  # what the generator may never drop, and what it dropped with its measured miss
        assert {"no_bias", "mirrored", "scores/8"} <= set(m["caught"]), name
        assert all(v and set(v) <= {"first", "mean"} for v in m["dropped"].values()), name
    everywhere = {d for m in meta.values() for d in m["caught"]}
    assert everywhere >= set(tr.DEVIATIONS + tr.PROJ_DEVIATIONS) - {"erf_gelu"}
    # the two projection forms: CodeT5+ (768 -> 256 with bias on the first token) and sentence-T5 (Dense without bias on the mean)
    forms = {(m["cfg"]["hidden"], m["proj"]["E"], m["proj"]["bias"], m["proj"]["pooling"]) for m in meta.values() if "proj" in m}
    assert forms == {(768, 256, True, "first"), (256, 256, False, "mean")}


@pytest.mark.parametrize("name", SMALL + ["base_relu"])
def test_restatement_reproduces_transformers(t5_golden, name):
    data, meta = t5_golden
    m = meta[name]
    blob, ids, lens = tr.make_weights(m["cfg"], m["seed"], *m["scales"]), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    for pooling in ("first", "mean"):
        d = np.abs(tr.forward(m["cfg"], blob, ids, lens, pooling) - data[f"{name}_{pooling}"]).max()
        assert d <= 1e-5, (pooling, d)


@pytest.mark.parametrize("name", ["base_relu", "dense_mean"])
def test_projection_restatement_and_its_mixups(t5_golden, name):
    data, meta = t5_golden
    m = meta[name]
    p = m["proj"]
    W, b = tr.make_proj(m["cfg"]["hidden"], p["E"], m["seed"], p["bias"])
    pooled, want, long_ = data[f"{name}_{p['pooling']}"], data[f"{name}_proj"], data[f"{name}_lens"] > 32
    assert want.shape == (len(long_), p["E"]) and np.abs(tr.project(pooled, W, b) - want).max() <= 1e-5
    assert p["bf16_cos"] >= 0.99975
    for dev in tr.PROJ_DEVIATIONS:
        if dev == "proj_skipped" and p["E"] != m["cfg"]["hidden"]:
            assert dev not in m["caught"] and dev not in m["dropped"]  # another width: not comparable
            continue
        d, cos = miss(tr.project(pooled, W, b, deviate=dev), want)
        outside = ((d > p["T_proj"]) | (cos < 0.999))[long_].all()
        assert outside == (dev in m["caught"]) and (dev in m["dropped"]) == (not outside), (dev, d)
    # without a bias, normalising the pooled row first changes nothing (a positive scale commutes with W): recorded as dropped, 0.0
    assert ("normalise_before_proj" in m["dropped"]) == (not p["bias"])


@pytest.mark.parametrize("name", ["relu_s64", "aw128_s128"])
def test_mixups_miss_as_recorded(t5_golden, name):
    data, meta = t5_golden
    m = meta[name]
    cfg, blob, ids, lens = m["cfg"], tr.make_weights(m["cfg"], m["seed"], *m["scales"]), data[f"{name}_ids"].astype(np.int32), data[f"{name}_lens"]
    long_ = lens > 32
    assert long_.any()
    for dev, poolings in m["caught"].items():
        for pooling in poolings:
            d, cos = miss(tr.forward(cfg, blob, ids, lens, pooling, deviate=dev), data[f"{name}_{pooling}"])
            outside = (d > m[f"T_{pooling}"]) | (cos < 0.999)
            assert outside[long_].all(), (dev, pooling, d, m[f"T_{pooling}"])
    for dev, least in m["dropped"].items():  # e.g. erf_gelu: vanishes in whole-model vectors (tests/test_t5_gpu.py pins it on the kernel)
        for pooling in ("first", "mean"):
            d, _ = miss(tr.forward(cfg, blob, ids, lens, pooling, deviate=dev), data[f"{name}_{pooling}"])
            assert abs(float(d[long_].min()) - least[pooling]) <= 1e-5, (dev, pooling)


@pytest.mark.parametrize("change", [dict(), dict(t5_ffn="gated-gelu"), dict(hidden=256, heads=2, head_dim=64, ffn=512, t5_ffn="gated-gelu"),
                                    dict(hidden=768, heads=12, ffn=3072, layers=3, vocab=500, rel_buckets=16, rel_max_distance=32)])
def test_blob_bytes_equal_the_documented_layout(change):
    cfg = dict(BASE, **change)
    c = _native.encoder_cfg(cfg)
    assert (c.arch, c.pos_type, c.ffn_type, c.rel_buckets, c.rel_max_distance) == (3, 3, 4 if tr.gated(cfg) else 3, cfg["rel_buckets"], cfg["rel_max_distance"])
    need = C.c_int64()
    assert _native.lib().sc_encoder_blob_bytes(C.byref(c), C.byref(need)) == 0
    H, F, L, AW = cfg["hidden"], cfg["ffn"], cfg["layers"], tr.attn_width(cfg)
    F1 = 2 * F if tr.gated(cfg) else F
    per_layer = 3 * (AW * H + AW) + (H * AW + H) + 2 * H + (F1 * H + F1) + (H * F + H) + 2 * H
    assert need.value == 4 * (cfg["vocab"] * H + cfg["rel_buckets"] * cfg["heads"] + L * per_layer + 2 * H) == tr.make_weights(cfg, 1).nbytes


def test_cfg_struct_keeps_its_declared_fields_and_owns_the_appended_ones():
    header = (Path(__file__).resolve().parent.parent / "include" / "semcode_hip.h").read_text()
    body = re.search(r"typedef struct sc_encoder_cfg \{(.*?)\} sc_encoder_cfg;", header, flags=re.S).group(1)
    names = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names[-3:] == ["qk_norm", "rel_buckets", "rel_max_distance"]
    c = _native.EncoderCfg(vocab=7, qk_norm=1, rel_buckets=32, rel_max_distance=128)
    assert type(c) is _native.EncoderCfgFull and _native.EncoderCfgFull.CFG_BYTES == 96
    assert _native.EncoderCfgFull.TAIL_FIELDS == tuple(names[-2:]) and C.sizeof(_native.EncoderCfgFull) + 4 * len(names[-2:]) == 96
    raw = C.string_at(C.addressof(c), 96)
    assert np.frombuffer(raw, np.int32)[[0, 21, 22, 23]].tolist() == [7, 1, 32, 128]
    z = _native.EncoderCfg()
    assert (z.rel_buckets, z.rel_max_distance) == (0, 0) and not any(C.string_at(C.addressof(z), 96))


def create_error(cfg) -> "tuple[int, str]":
    """sc_encoder_create's answer to a configuration it refuses: the rules are checked before the runtime is touched, so a stand-in handle does."""
    c = cfg if isinstance(cfg, _native.EncoderCfg) else _native.encoder_cfg(cfg)
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
    for change, code, words in ((dict(rel_buckets=31), INVALID, ("rel_buckets",)), (dict(rel_buckets=0), INVALID, ("rel_buckets",)),
                                (dict(rel_max_distance=8), INVALID, ("rel_max_distance",)), (dict(heads=1), UNSUPPORTED, ("head dimension",)),
                                (dict(head_dim=128), UNSUPPORTED, ("head_dim",)), (dict(head_dim=32), UNSUPPORTED, ("head_dim",)),
                                (dict(hidden=256, heads=3, head_dim=64), UNSUPPORTED, ("attention width",)), (dict(max_pos=4096), UNSUPPORTED, ("max_pos",)),
                                (dict(ffn=200), UNSUPPORTED, ("ffn",)), (dict(hidden=2176, heads=34), UNSUPPORTED, ("hidden",))):
        st, msg = create_error(dict(BASE, **change))
        assert st == code and all(w in msg for w in words), (change, st, msg)
    for field, value, words in (("pos_type", 2, ("arch 3", "pos_type")), ("pos_type", 0, ("arch 3", "pos_type")), ("ffn_type", 2, ("arch 3", "ffn_type")),
                                ("ffn_type", 0, ("arch 3", "ffn_type")), ("kv_heads", 1, ("kv_heads",)), ("qk_norm", 1, ("qk_norm",)), ("local_window", 64, ("local_window",))):
        c = _native.encoder_cfg(BASE)
        setattr(c, field, value)
        st, msg = create_error(c)
        assert st == UNSUPPORTED and all(w in msg for w in words), (field, st, msg)
    # what the T5 encoder appended is refused on the other architectures
    bert = dict(_native.BERT_BASE, vocab=64, layers=1, hidden=128, heads=2, ffn=256)
    for field, value in (("pos_type", 3), ("ffn_type", 3), ("ffn_type", 4), ("rel_buckets", 32), ("rel_max_distance", 128)):
        for other in (bert, dict(bert, rotary=True, geglu=True, modernbert=True, local_window=32, global_every=3),
                      dict(bert, rotary=True, swiglu=True, qwen2=True, type_vocab=1)):
            c = _native.encoder_cfg(other)
            setattr(c, field, value)
            st, msg = create_error(c)
            assert st == UNSUPPORTED and field in msg and "arch 3" in msg, (field, other, st, msg)
    for field, value in (("pos_type", 4), ("ffn_type", 5), ("arch", 4)):
        c = _native.encoder_cfg(BASE)
        setattr(c, field, value)
        assert create_error(c)[0] == INVALID


def test_config_json_mapping(tmp_path):
    cfg = dict(BASE, max_pos=2048)
    hf = tr.hf_config(cfg)
    assert t5_config(hf) == cfg
    (tmp_path / "config.json").write_text(json.dumps(hf))
    assert t5_config(tmp_path / "config.json") == cfg
    small = t5_config(dict(hf, d_model=512, num_heads=6, feed_forward_proj="gated-gelu"))  # t5-v1.1-small: heads of 64 are stated
    assert (small["head_dim"], small["t5_ffn"], small["hidden"], small["heads"]) == (64, "gated-gelu", 512, 6)
    codet5p = t5_config(dict(hf, model_type="codet5p_embedding", embed_dim=256))
    assert codet5p["embed_dim"] == 256 and codet5p["t5"]
    for bad, word in ((dict(d_kv=128), "d_kv"), (dict(feed_forward_proj="gated-silu"), "gated-silu"), (dict(model_type="bert"), "bert")):
        with pytest.raises(ValueError, match=word):
            t5_config(dict(hf, **bad))
    with pytest.raises(ValueError):
        _native.encoder_cfg(dict(cfg, t5_ffn="gelu"))
    with pytest.raises(ValueError):
        _native.encoder_cfg(dict(cfg, qwen2=True))
    assert _native.POOLINGS_T5 == {"mean": 0, "first": 1}


def write_t5_dir(d, cfg, blob, model_type="t5", proj=None, dense=None, dense_act="torch.nn.modules.linear.Identity", pooling_cfg=None, tokenizer="tokenizer.json"):
    """A transformers-named model directory: config.json, model.safetensors (encoder + a decoder tensor the loader must ignore), tokenizer"""
    from safetensors.numpy import save_file

    d.mkdir(parents=True, exist_ok=True)
    hf = dict(tr.hf_config(cfg), model_type=model_type)
    sd = tr.to_hf_state_dict(cfg, blob)
    sd["decoder.block.0.layer.0.SelfAttention.q.weight"] = np.ones((4, 4), np.float32)
    if proj is not None:
        hf["embed_dim"] = int(proj[0].shape[0])
        sd["proj.weight"] = proj[0]
        if proj[1] is not None:
            sd["proj.bias"] = proj[1]
    (d / "config.json").write_text(json.dumps(hf))
    save_file(sd, str(d / "model.safetensors"))
    if dense is not None:
        (d / "2_Dense").mkdir(exist_ok=True)
        (d / "2_Dense" / "config.json").write_text(json.dumps(dict(in_features=int(dense[0].shape[1]), out_features=int(dense[0].shape[0]), bias=dense[1] is not None,
                                                                    activation_function=dense_act)))
        save_file({"linear.weight": dense[0], **({"linear.bias": dense[1]} if dense[1] is not None else {})}, str(d / "2_Dense" / "model.safetensors"))
    if pooling_cfg is not None:
        (d / "1_Pooling").mkdir(exist_ok=True)
        (d / "1_Pooling" / "config.json").write_text(json.dumps(pooling_cfg))
    if tokenizer:
        (d / tokenizer).write_text("{}")
    return d


def test_loader_round_trip(tmp_path):
    from semcode_amd.embeddings.providers import load_t5_directory, t5_model_dir

    for cfg in (dict(BASE, max_pos=2048), dict(BASE, max_pos=2048, hidden=256, heads=2, head_dim=64, ffn=512, t5_ffn="gated-gelu")):
        blob = tr.make_weights(cfg, 5)
        H = cfg["hidden"]
        # CodeT5+: proj.* in the model file, first-token pooling by its model_type
        W, b = tr.make_proj(H, 48, 5, True)
        d = write_t5_dir(tmp_path / f"codet5p_{H}", cfg, blob, model_type="codet5p_embedding", proj=(W, b))
        assert t5_model_dir(d) == d and t5_model_dir(d / "model.safetensors") == d
        got = load_t5_directory(d)
        assert got["cfg"] == cfg and np.array_equal(got["blob"], blob) and got["pooling"] == "first" and got["tokenizer_json"] == d / "tokenizer.json"
        assert np.array_equal(got["proj"][0], W) and np.array_equal(got["proj"][1], b)
        assert load_t5_directory(d, pooling="mean")["pooling"] == "mean"  # pooling= overrides
        # sentence-T5 / GTR: 2_Dense without bias, 1_Pooling states the mean
        Wd, _ = tr.make_proj(H, H, 6, False)
        d = write_t5_dir(tmp_path / f"st5_{H}", cfg, blob, dense=(Wd, None), pooling_cfg=dict(pooling_mode_mean_tokens=True, pooling_mode_cls_token=False))
        got = load_t5_directory(d)
        assert np.array_equal(got["blob"], blob) and got["pooling"] == "mean" and np.array_equal(got["proj"][0], Wd) and got["proj"][1] is None
        assert load_t5_directory(d, pooling="cls")["pooling"] == "first"
        # a bare encoder: no projection; 1_Pooling may state the first token
        d = write_t5_dir(tmp_path / f"bare_{H}", cfg, blob, pooling_cfg=dict(pooling_mode_cls_token=True))
        got = load_t5_directory(d)
        assert got["proj"] == (None, None) and got["pooling"] == "first"
    cfg, blob = dict(BASE, max_pos=2048), tr.make_weights(dict(BASE, max_pos=2048), 5)
    Wd, _ = tr.make_proj(128, 128, 6, False)
    with pytest.raises(ValueError, match="Tanh"):  # a Dense module with an activation is not linear
        load_t5_directory(write_t5_dir(tmp_path / "tanh", cfg, blob, dense=(Wd, None), dense_act="torch.nn.modules.activation.Tanh"))
    with pytest.raises(ValueError, match="spiece.model"):
        load_t5_directory(write_t5_dir(tmp_path / "spiece", cfg, blob, tokenizer="spiece.model"))
    with pytest.raises(ValueError, match="first.*mean"):
        load_t5_directory(write_t5_dir(tmp_path / "pool", cfg, blob), pooling="last")
    # a missing tensor is named
    from safetensors.numpy import load_file, save_file

    d = write_t5_dir(tmp_path / "missing", cfg, blob)
    sd = load_file(str(d / "model.safetensors"))
    del sd["encoder.block.1.layer.1.DenseReluDense.wo.weight"]
    save_file(sd, str(d / "model.safetensors"))
    with pytest.raises(KeyError, match="encoder.block.1.layer.1.DenseReluDense.wo.weight"):
        load_t5_directory(d)
    assert t5_model_dir(tmp_path) is None and t5_model_dir(None) is None
