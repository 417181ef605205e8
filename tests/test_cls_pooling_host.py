"""CPU: the host half of [CLS] pooling -- where the pooling mode comes from (GGUF key, setting, sentence-transformers config), and the
new symbols of the C ABI."""
import json
import re
from pathlib import Path

import pytest

from semcode_amd.embeddings import gguf
from semcode_amd.embeddings.providers import resolve_pooling
from semcode_amd.settings import Settings

ROOT = Path(__file__).resolve().parent.parent
META = {"general.architecture": "bert", "bert.embedding_length": 384, "bert.block_count": 12, "bert.attention.head_count": 12,
        "bert.feed_forward_length": 1536, "bert.context_length": 512, "bert.attention.layer_norm_epsilon": 1e-12}


def write(path, pooling_type=None):
    meta = dict(META)
    if pooling_type is not None:
        meta["bert.pooling_type"] = pooling_type
    gguf.write_gguf(path, meta, {})
    return path


@pytest.mark.parametrize("ptype,want", [(2, "cls"), (1, "mean"), (None, "mean")])
def test_gguf_pooling_type(tmp_path, ptype, want):
    meta, _ = gguf.read_gguf(write(tmp_path / "m.gguf", ptype))
    cfg = gguf.gguf_config(meta)
    assert cfg["pooling"] == want and (cfg["hidden"], cfg["heads"], cfg["layers"]) == (384, 12, 12)
    assert resolve_pooling(None, "", tmp_path / "m.gguf") == want


@pytest.mark.parametrize("ptype", [0, 3, 4])
def test_gguf_pooling_types_this_encoder_does_not_run_are_refused(tmp_path, ptype):
    meta, _ = gguf.read_gguf(write(tmp_path / "m.gguf", ptype))
    with pytest.raises(gguf.GGUFError, match=rf"pooling_type = {ptype}\b"):
        gguf.gguf_config(meta)
    with pytest.raises(gguf.GGUFError):
        resolve_pooling(None, None, tmp_path / "m.gguf")


def test_other_architectures_read_their_own_key(tmp_path):
    meta = {k.replace("bert.", "nomic-bert."): v for k, v in META.items()}
    meta["general.architecture"] = "nomic-bert"
    assert gguf.gguf_config(dict(meta, **{"nomic-bert.pooling_type": 2}))["pooling"] == "cls"
    assert gguf.gguf_config(dict(meta, **{"bert.pooling_type": 2}))["pooling"] == "mean"  # another architecture's key


def test_resolution_order(tmp_path):
    cls_file, mean_file = write(tmp_path / "cls.gguf", 2), write(tmp_path / "mean.gguf", 1)
    # 1. the argument beats everything
    assert resolve_pooling("mean", "cls", cls_file) == "mean"
    assert resolve_pooling("cls", "mean", mean_file) == "cls"
    # 2. the setting beats the file
    assert resolve_pooling(None, "cls", mean_file) == "cls"
    assert resolve_pooling(None, "mean", cls_file) == "mean"
    assert resolve_pooling(None, " CLS ", None) == "cls"
    # 3. the file
    assert resolve_pooling(None, "", cls_file) == "cls" and resolve_pooling(None, None, mean_file) == "mean"
    assert resolve_pooling(None, None, cls_file, file_pooling="mean") == "mean"  # what the caller already read from it
    # 4. a sentence-transformers directory
    st = tmp_path / "st"
    (st / "1_Pooling").mkdir(parents=True)
    weights = st / "model.safetensors"
    assert resolve_pooling(None, None, weights) == "mean"  # no config.json
    (st / "1_Pooling" / "config.json").write_text(json.dumps({"word_embedding_dimension": 384, "pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}))
    assert resolve_pooling(None, None, weights) == "cls"
    assert resolve_pooling(None, "mean", weights) == "mean" and resolve_pooling("mean", "", weights) == "mean"
    (st / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True}))
    assert resolve_pooling(None, None, weights) == "mean"
    assert resolve_pooling(None, None, st / "blob.npy") == "mean"  # only a .safetensors looks at the directory
    # 5. nothing says
    assert resolve_pooling() == "mean" and resolve_pooling(None, None, None) == "mean"
    for bad in ("last", "max"):
        with pytest.raises(ValueError, match="'mean' or 'cls'"):
            resolve_pooling(bad)
        with pytest.raises(ValueError, match="SEMCODE_MI355X_POOLING"):
            resolve_pooling(None, bad)


def test_setting(monkeypatch):
    monkeypatch.delenv("SEMCODE_MI355X_POOLING", raising=False)
    assert Settings().mi355x_pooling == ""
    monkeypatch.setenv("SEMCODE_MI355X_POOLING", "cls")
    assert Settings().mi355x_pooling == "cls"


def test_new_symbols_are_declared_exported_and_bound():
    import ctypes

    from semcode_amd import _native
    from semcode_amd.csrc import build

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "semcode_hip.h").read_text(), flags=re.S)
    handle = ctypes.CDLL(str(build.build(verbose=False)))
    for sym in ("sc_encoder_set_pooling", "sc_encoder_get_pooling", "sc_diag_attention_run"):
        assert re.search(rf"\b{sym}\s*\(", header), sym
        assert hasattr(handle, sym) and sym in _native.SIGNATURES, sym
    assert _native.POOLINGS == {"mean": 0, "cls": 1}
    assert "Out of scope: CLS-pooled" not in (ROOT / "include" / "semcode_hip.h").read_text()
