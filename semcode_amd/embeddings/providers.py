"""Embedding provider factory with the MI355X encoder as a provider.

Reference: src/semcode/embeddings/providers.py:21-104.  `EmbeddingPayload` and
`EmbeddingProviderFactory.create(provider=None, model=None)` keep their names, signature, dispatch on the
lower-cased provider name and error types (NotImplementedError for unknown providers, ValueError when
the llama.cpp model path is unset, RuntimeError when llama-cpp-python is missing), so
IndexerService._embedding_client_instance (src/semcode/services/indexer.py:180-183) and
SemanticSearchPipeline._embedding_client (src/semcode/rag/pipeline.py:298-301) work unchanged.  New
provider names "mi355x" / "hip" select the HIP encoder (settings.embedding_provider = "mi355x").

The returned object has LangChain's Embeddings surface -- embed_documents(list[str]) -> list[list[float]],
embed_query(str) -> list[float] (duck-typed in reference tests/integration/test_indexer_service.py:7-12)
-- plus array fast paths that skip the list-of-float boxing.
"""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Any, Callable, List, Optional, Sequence

import numpy as np

from ..settings import resolve as _resolve_settings
from .payload import EmbeddingPayload
from .tokenizer import HashTokenizer, HFTokenizer, WordPieceTokenizer, pack

log = logging.getLogger(__name__)

__all__ = ["EmbeddingPayload", "EmbeddingProviderFactory", "MI355XEmbeddings", "create_reranker"]

MI355X_PROVIDER_NAMES = {"mi355x", "hip", "rocm"}

# HF BertModel checkpoint names -> blob order of include/semcode_hip.h (sc_encoder_blob_bytes)
_HF_HEAD = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight",
            "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
_HF_LAYER = ["attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight", "attention.self.key.bias",
             "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
             "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
             "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias"]


# jina-bert-v2 (jina-embeddings-v2-*) checkpoint names: no position table (ALiBi), GLU feed-forward `mlp.gated_layers` [2F, H]
# without bias (gate = first F rows), `mlp.wo`, `mlp.layernorm`.  Written from the published module layout; no such checkpoint
# exists offline, so the mapping is only exercised on a file this repo writes with those names (parity unpinned).
_JINA_HEAD = ["embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
_JINA_LAYER = ["attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight", "attention.self.key.bias",
               "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
               "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias", "mlp.gated_layers.weight", None,  # None: zero bias
               "mlp.wo.weight", "mlp.wo.bias", "mlp.layernorm.weight", "mlp.layernorm.bias"]


# transformers NomicBertModel names (nomic-embed-text-v1 / v1.5 as `nomic_bert`): no position table (rotary), no Linear bias,
# gate_proj (SiLU-activated) and up_proj stacked into W1 = [2F, H], gate rows first.  Checked against NomicBertModel itself
# (tests/test_nomic_weights.py).  Second member: the blob's bias slot after that matrix, which the file has no tensor for (H or 2F zeros).
_NOMIC_HEAD = ["embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
_NOMIC_LAYER = [("self_attn.q_proj.weight", "H"), ("self_attn.k_proj.weight", "H"), ("self_attn.v_proj.weight", "H"), ("self_attn.o_proj.weight", "H"),
                ("post_attention_layernorm.weight", None), ("post_attention_layernorm.bias", None),
                ("mlp.gate_proj.weight", None), ("mlp.up_proj.weight", "2F"), ("mlp.down_proj.weight", "H"),
                ("post_mlp_layernorm.weight", None), ("post_mlp_layernorm.bias", None)]


def _nomic_blob(path, tensors: dict, layers: int) -> np.ndarray:
    def get(name: str) -> np.ndarray:
        for key in (name, "nomic_bert." + name):
            if key in tensors:
                return np.asarray(tensors[key], dtype=np.float32)
        raise KeyError(f"{path}: tensor {name!r} not found")

    parts = [get(n).reshape(-1) for n in _NOMIC_HEAD]
    H = get(_NOMIC_HEAD[2]).shape[0]
    for l in range(layers):
        F = get(f"layers.{l}.mlp.gate_proj.weight").shape[0]
        for n, zeros in _NOMIC_LAYER:
            parts.append(get(f"layers.{l}.{n}").reshape(-1))
            if zeros:  # the bias slot that follows this matrix in blob order
                parts.append(np.zeros(H if zeros == "H" else 2 * F, np.float32))
    return np.concatenate(parts)


# transformers ModernBertModel names (answerdotai/ModernBERT-base, gte-modernbert-base, modernbert-embed-base), with or without a
# "model." prefix: pre-norm layers, no position or type table, Wqkv = [Wq; Wk; Wv] row thirds, Wi = [activated half; gate half] -- the
# activated half is what the GEGLU kernel calls the gate rows, so Wi lands in W1 as it is.  Blob order: arch 1 of include/semcode_hip.h.
# Norm, attention and MLP biases are optional tensors (norm_bias / attention_bias / mlp_bias models); absent = zeros.
def _modernbert_blob(path, tensors: dict, layers: int) -> np.ndarray:
    def find(name: str):
        for key in (name, "model." + name):
            if key in tensors:
                return np.asarray(tensors[key], dtype=np.float32)
        return None

    def get(name: str) -> np.ndarray:
        t = find(name)
        if t is None:
            raise KeyError(f"{path}: tensor {name!r} not found")
        return t

    def opt(name: str, n: int) -> np.ndarray:
        t = find(name)
        return np.zeros(n, np.float32) if t is None else t.reshape(-1)

    H = get("embeddings.norm.weight").shape[0]
    parts = [get("embeddings.tok_embeddings.weight").reshape(-1), get("embeddings.norm.weight"), opt("embeddings.norm.bias", H)]
    for l in range(layers):
        q = f"layers.{l}."
        wqkv, bqkv = get(q + "attn.Wqkv.weight"), opt(q + "attn.Wqkv.bias", 3 * H)
        if wqkv.shape != (3 * H, H):
            raise ValueError(f"{path}: {q}attn.Wqkv.weight is {wqkv.shape}, expected {(3 * H, H)}")
        wi = get(q + "mlp.Wi.weight")
        for third in range(3):
            parts += [wqkv[third * H:(third + 1) * H].reshape(-1), bqkv[third * H:(third + 1) * H]]
        attn_norm = find(q + "attn_norm.weight")  # layer 0 has none (identity): the slot is present and never read
        parts += [get(q + "attn.Wo.weight").reshape(-1), opt(q + "attn.Wo.bias", H),
                  np.ones(H, np.float32) if attn_norm is None else attn_norm, opt(q + "attn_norm.bias", H),
                  wi.reshape(-1), opt(q + "mlp.Wi.bias", wi.shape[0]), get(q + "mlp.Wo.weight").reshape(-1), opt(q + "mlp.Wo.bias", H),
                  get(q + "mlp_norm.weight"), opt(q + "mlp_norm.bias", H)]
    parts += [get("final_norm.weight"), opt("final_norm.bias", H)]
    return np.concatenate(parts)


def modernbert_config(config: "str | Path | dict") -> dict:
    """The encoder configuration of a transformers ModernBERT `config.json` (path or parsed dict).  Layer pattern: the integer
    `global_attn_every_n_layers`, or a `layer_types` list that follows such a pattern ("full_attention" exactly at l % n == 0); any
    other list is refused.  Rotary bases: `global_rope_theta` / `local_rope_theta`, or `rope_parameters` per layer type."""
    if not isinstance(config, dict):
        import json

        config = json.loads(Path(config).read_text())
    c = config
    if c.get("model_type") not in (None, "modernbert"):
        raise ValueError(f"not a ModernBERT configuration (model_type {c.get('model_type')!r})")
    layers = int(c["num_hidden_layers"])
    types = c.get("layer_types")
    if types is not None:
        if len(types) != layers or any(t not in ("full_attention", "sliding_attention") for t in types):
            raise ValueError(f"ModernBERT config: layer_types must name full_attention / sliding_attention for each of the {layers} layers")
        every = next((n for n in range(1, layers + 1) if all((t == "full_attention") == (l % n == 0) for l, t in enumerate(types))), None)
        if every is None:
            raise ValueError(f"ModernBERT config: layer_types {types} is not 'global every n-th layer from layer 0'; no other pattern is supported")
    else:
        every = int(c.get("global_attn_every_n_layers", 3))
    rp = c.get("rope_parameters") or {}
    theta_g = (rp.get("full_attention") or {}).get("rope_theta", c.get("global_rope_theta", 160000.0))
    theta_l = (rp.get("sliding_attention") or {}).get("rope_theta", c.get("local_rope_theta", theta_g if c.get("local_rope_theta", 0) is None else 10000.0))
    if c.get("hidden_activation", "gelu") != "gelu":
        raise ValueError(f"ModernBERT config: hidden_activation {c.get('hidden_activation')!r} is not supported (gelu only)")
    return dict(vocab=int(c["vocab_size"]), hidden=int(c["hidden_size"]), layers=layers, heads=int(c["num_attention_heads"]),
                ffn=int(c["intermediate_size"]), max_pos=int(c.get("max_position_embeddings", 8192)), type_vocab=1,
                ln_eps=float(c.get("norm_eps", 1e-5)), rotary=True, geglu=True, modernbert=True, local_window=int(c.get("local_attention", 128)),
                global_every=int(every), rope_theta=float(theta_g), rope_theta_local=float(theta_l))


def modernbert_config_beside(weights: "str | Path | None") -> Optional[dict]:
    """modernbert_config of the config.json next to a .safetensors file, None when there is none or it is another model's."""
    if not isinstance(weights, (str, Path)) or not str(weights).lower().endswith(".safetensors"):
        return None
    conf = Path(weights).parent / "config.json"
    if not conf.is_file():
        return None
    import json

    c = json.loads(conf.read_text())
    return modernbert_config(c) if c.get("model_type") == "modernbert" else None


# transformers Qwen2Model names (Qwen2 / Qwen2.5 backbones of jina-code-embeddings-0.5b, gte-Qwen2, KaLM-mini), with or without a "model."
# prefix: a pre-norm causal decoder, no position or type table, no embedding norm, biases on q / k / v only, gate_proj (SiLU-activated) and
# up_proj stacked into W1 = [2F, H], gate rows first.  Blob order: arch 2 of include/semcode_hip.h (beta slots and the bo / b1 / b2 slots are
# zeros).  Written from the published module layout and checked against transformers' Qwen2Model on seeded weights
# (scripts/gen_qwen2_fixtures.py); no released checkpoint exists offline, so parity for real files is unpinned.
# The widths come from the configuration: heads of cfg["head_dim"] (64 without it), q_proj [heads * head_dim, H], o_proj [H, heads * head_dim].
# Qwen3 (cfg["qk_norm"]): self_attn.q_norm.weight / k_norm.weight [head_dim] go behind each layer's ln2 beta slot; a file that has them under a
# configuration without qk_norm, or lacks them under one with it, is an error (scripts/gen_qwen3_fixtures.py checks the layout against Qwen3Model).
def _qwen2_blob(path, tensors: dict, layers: int, cfg: Optional[dict] = None) -> np.ndarray:
    def find(name: str):
        for key in (name, "model." + name):
            if key in tensors:
                return np.asarray(tensors[key], dtype=np.float32)
        return None

    def get(name: str) -> np.ndarray:
        t = find(name)
        if t is None:
            raise KeyError(f"{path}: tensor {name!r} not found")
        return t

    def opt(name: str, n: int) -> np.ndarray:
        t = find(name)
        return np.zeros(n, np.float32) if t is None else t.reshape(-1)

    emb = get("embed_tokens.weight")
    H = emb.shape[1]
    hd = int((cfg or {}).get("head_dim") or 64)
    qk_norm = bool((cfg or {}).get("qk_norm"))
    AW = hd * int(cfg["heads"]) if cfg is not None else H  # the attention width: heads * head_dim, which need not be H at 128
    zeros = np.zeros(H, np.float32)
    parts = [emb.reshape(-1)]
    for l in range(layers):
        q = f"layers.{l}."
        wq, wk, wv = get(q + "self_attn.q_proj.weight"), get(q + "self_attn.k_proj.weight"), get(q + "self_attn.v_proj.weight")
        wo = get(q + "self_attn.o_proj.weight")
        KV = wk.shape[0]
        if wq.shape != (AW, H) or wk.shape != (KV, H) or wv.shape != (KV, H) or KV % hd or wo.shape != (H, AW):
            raise ValueError(f"{path}: {q}self_attn q / k / v / o projections are {wq.shape} / {wk.shape} / {wv.shape} / {wo.shape}, expected [{AW}, {H}], "
                             f"two [{hd} * kv_heads, {H}] and [{H}, {AW}]")
        if cfg is not None and KV != hd * int(cfg.get("kv_heads") or cfg["heads"]):
            raise ValueError(f"{path}: {q}self_attn.k_proj has {KV // hd} heads of {hd}, the encoder configuration {int(cfg.get('kv_heads') or cfg['heads'])}")
        norms = []
        for name in ("self_attn.q_norm.weight", "self_attn.k_norm.weight"):
            t = find(q + name)
            if qk_norm and (t is None or t.shape != (hd,)):
                raise ValueError(f"{path}: tensor {q + name!r} [{hd}] not found, the encoder configuration says qk_norm")
            if not qk_norm and t is not None:
                raise ValueError(f"{path}: unexpected tensor {q + name!r}: the encoder configuration has no qk_norm (a Qwen3 file needs its own config.json)")
            if qk_norm:
                norms.append(t.reshape(-1))
        gate, up = get(q + "mlp.gate_proj.weight"), get(q + "mlp.up_proj.weight")
        parts += [wq.reshape(-1), opt(q + "self_attn.q_proj.bias", AW), wk.reshape(-1), opt(q + "self_attn.k_proj.bias", KV), wv.reshape(-1),
                  opt(q + "self_attn.v_proj.bias", KV), wo.reshape(-1), opt(q + "self_attn.o_proj.bias", H),
                  get(q + "input_layernorm.weight"), zeros, gate.reshape(-1), up.reshape(-1), np.zeros(2 * gate.shape[0], np.float32),
                  get(q + "mlp.down_proj.weight").reshape(-1), zeros, get(q + "post_attention_layernorm.weight"), zeros] + norms
    parts += [get("norm.weight"), zeros]
    return np.concatenate(parts)


def qwen2_config(config: "str | Path | dict") -> dict:
    """The encoder configuration of a transformers Qwen2 `config.json` (path or parsed dict): grouped-query heads from
    `num_key_value_heads`, the rotary base `rope_theta`, `rms_norm_eps`, and `max_position_embeddings` capped at the 2 048 tokens a text
    may have here (the cap sizes the rotary table; the released models state 32 768).  A sliding window shorter than that is refused:
    the causal kernel attends to every earlier token."""
    if not isinstance(config, dict):
        import json

        config = json.loads(Path(config).read_text())
    c = config
    if c.get("model_type") not in (None, "qwen2"):
        raise ValueError(f"not a Qwen2 configuration (model_type {c.get('model_type')!r})")
    if c.get("use_sliding_window") and int(c.get("sliding_window") or 0) < 2048:
        raise ValueError(f"Qwen2 config: use_sliding_window with sliding_window {c.get('sliding_window')} < 2048 is not supported (the causal kernel sees every earlier token)")
    if c.get("hidden_act", "silu") != "silu":
        raise ValueError(f"Qwen2 config: hidden_act {c.get('hidden_act')!r} is not supported (silu only)")
    out = _qwen_common(c)
    if int(c.get("head_dim") or out["hidden"] // out["heads"]) == 128:  # Qwen2.5-1.5B: heads of 128 are stated to the library, never derived
        out["head_dim"] = 128
    return out


def _qwen_common(c: dict) -> dict:
    heads = int(c["num_attention_heads"])
    rp = c.get("rope_parameters") or {}
    return dict(vocab=int(c["vocab_size"]), hidden=int(c["hidden_size"]), layers=int(c["num_hidden_layers"]), heads=heads,
                kv_heads=int(c.get("num_key_value_heads") or heads), ffn=int(c["intermediate_size"]),
                max_pos=min(int(c.get("max_position_embeddings", 32768)), 2048), type_vocab=1, ln_eps=float(c.get("rms_norm_eps", 1e-6)), rotary=True,
                swiglu=True, qwen2=True, rope_theta=float(rp.get("rope_theta", c.get("rope_theta", 10000.0))))


def t5_config(config: "str | Path | dict") -> dict:
    """The encoder configuration of a transformers T5 `config.json` (path or parsed dict; model_type `t5`, or `codet5p_embedding`, whose
    `embed_dim` -- the width of the projection behind its first-token pooling -- is reported as "embed_dim"): `d_model`, `num_heads`,
    `num_layers`, `d_ff`, the buckets of the relative position bias, `layer_norm_epsilon`, and `feed_forward_proj` "relu" or "gated-gelu"
    (anything else is refused by name).  `d_kv` must be 64: heads of 64 are stated to the library when d_model / num_heads is not 64
    (t5-v1.1-small).  max_pos is the 2 048 tokens a text may have here: T5 has no position table, the cap sizes the bias table."""
    if not isinstance(config, dict):
        import json

        config = json.loads(Path(config).read_text())
    c = config
    if c.get("model_type") not in (None, "t5", "codet5p_embedding"):
        raise ValueError(f"not a T5 configuration (model_type {c.get('model_type')!r})")
    if int(c.get("d_kv", 64)) != 64:
        raise ValueError(f"T5 config: d_kv {c.get('d_kv')} is not supported (heads of 64 only)")
    ffn = c.get("feed_forward_proj", "relu")
    if ffn not in ("relu", "gated-gelu"):
        raise ValueError(f"T5 config: feed_forward_proj {ffn!r} is not supported ('relu' or 'gated-gelu')")
    hidden, heads = int(c["d_model"]), int(c["num_heads"])
    out = dict(vocab=int(c["vocab_size"]), hidden=hidden, layers=int(c["num_layers"]), heads=heads, ffn=int(c["d_ff"]), max_pos=2048, type_vocab=1,
               ln_eps=float(c.get("layer_norm_epsilon", 1e-6)), t5=True, t5_ffn=ffn, rel_buckets=int(c.get("relative_attention_num_buckets", 32)),
               rel_max_distance=int(c.get("relative_attention_max_distance", 128)))
    if hidden != heads * 64:
        out["head_dim"] = 64
    if c.get("model_type") == "codet5p_embedding":
        out["embed_dim"] = int(c["embed_dim"])
    return out


def t5_model_dir(weights: "str | Path | None") -> Optional[Path]:
    """The directory of a T5 encoder model -- `weights` is that directory or its model.safetensors, and the config.json in it says
    model_type t5 or codet5p_embedding -- else None."""
    if not isinstance(weights, (str, Path)):
        return None
    path = Path(weights)
    d = path if path.is_dir() else path.parent if path.suffix.lower() == ".safetensors" else None
    if d is None or not (d / "config.json").is_file():
        return None
    import json

    try:
        c = json.loads((d / "config.json").read_text())
    except (OSError, ValueError):
        return None
    return d if c.get("model_type") in ("t5", "codet5p_embedding") else None


# transformers' T5EncoderModel / T5Model / CodeT5p_Embedding names -> the arch 3 blob of include/semcode_hip.h; decoder tensors are ignored.
# Checked against T5EncoderModel on seeded weights (tests/test_t5.py); no released checkpoint exists offline, so parity for real files is unpinned.
def _t5_blob(path, tensors: dict, cfg: dict) -> np.ndarray:
    def find(*names: str):
        for name in names:
            if name in tensors:
                return np.asarray(tensors[name], dtype=np.float32)
        return None

    def get(*names: str) -> np.ndarray:
        t = find(*names)
        if t is None:
            raise KeyError(f"{path}: tensor {names[0]!r} not found")
        return t

    H, F, heads, layers = int(cfg["hidden"]), int(cfg["ffn"]), int(cfg["heads"]), int(cfg["layers"])
    AW = heads * 64
    gated = cfg["t5_ffn"] == "gated-gelu"
    emb = get("shared.weight", "encoder.embed_tokens.weight")
    rel = get("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")
    if emb.shape != (int(cfg["vocab"]), H) or rel.shape != (int(cfg["rel_buckets"]), heads):
        raise ValueError(f"{path}: embedding table {emb.shape} / relative_attention_bias {rel.shape}, the configuration says "
                         f"[{cfg['vocab']}, {H}] and [{cfg['rel_buckets']}, {heads}]")
    zH, zA = np.zeros(H, np.float32), np.zeros(AW, np.float32)
    parts = [emb.reshape(-1), rel.reshape(-1)]
    for l in range(layers):
        q = f"encoder.block.{l}.layer."
        wq, wk, wv, wo = (get(q + f"0.SelfAttention.{n}.weight") for n in "qkvo")
        if wq.shape != (AW, H) or wk.shape != (AW, H) or wv.shape != (AW, H) or wo.shape != (H, AW):
            raise ValueError(f"{path}: {q}0.SelfAttention q / k / v / o are {wq.shape} / {wk.shape} / {wv.shape} / {wo.shape}, expected three [{AW}, {H}] and [{H}, {AW}]")
        if gated:
            w1 = np.concatenate([get(q + "1.DenseReluDense.wi_0.weight"), get(q + "1.DenseReluDense.wi_1.weight")])
        else:
            w1 = get(q + "1.DenseReluDense.wi.weight")
        w2 = get(q + "1.DenseReluDense.wo.weight")
        if w1.shape != ((2 * F if gated else F), H) or w2.shape != (H, F):
            raise ValueError(f"{path}: {q}1.DenseReluDense weights are {w1.shape} / {w2.shape}, the configuration says ffn {F} ({cfg['t5_ffn']})")
        parts += [wq.reshape(-1), zA, wk.reshape(-1), zA, wv.reshape(-1), zA, wo.reshape(-1), zH, get(q + "0.layer_norm.weight"), zH,
                  w1.reshape(-1), np.zeros(w1.shape[0], np.float32), w2.reshape(-1), zH, get(q + "1.layer_norm.weight"), zH]
    parts += [get("encoder.final_layer_norm.weight"), zH]
    return np.concatenate(parts)


def t5_projection(model_dir: "str | Path", tensors: Optional[dict] = None) -> "tuple[Optional[np.ndarray], Optional[np.ndarray]]":
    """(W [E, H], b [E] or None) of the projection behind a T5 model's pooling, (None, None) when it has none: `proj.weight` / `proj.bias` of
    the model file (CodeT5+), else the sentence-transformers module `2_Dense/model.safetensors` (`linear.weight`, `linear.bias` if any), whose
    `2_Dense/config.json` must state an Identity activation -- any other is refused: the device applies none."""
    d = Path(model_dir)
    if tensors is None:
        from safetensors.numpy import load_file

        tensors = load_file(str(d / "model.safetensors"))
    if "proj.weight" in tensors:
        b = tensors.get("proj.bias")
        return np.asarray(tensors["proj.weight"], np.float32), None if b is None else np.asarray(b, np.float32)
    dense = d / "2_Dense"
    if not (dense / "model.safetensors").is_file():
        return None, None
    import json

    from safetensors.numpy import load_file

    act = str(json.loads((dense / "config.json").read_text()).get("activation_function", "")) if (dense / "config.json").is_file() else ""
    if not act.endswith("Identity"):
        raise ValueError(f"{dense}: activation_function {act!r} is not supported (the Dense module must be linear: torch.nn.modules.linear.Identity)")
    t = load_file(str(dense / "model.safetensors"))
    if "linear.weight" not in t:
        raise KeyError(f"{dense / 'model.safetensors'}: tensor 'linear.weight' not found")
    b = t.get("linear.bias")
    return np.asarray(t["linear.weight"], np.float32), None if b is None else np.asarray(b, np.float32)


def t5_pooling(model_dir: "str | Path", pooling: Optional[str] = None) -> str:
    """"first" or "mean" for a T5 directory: the argument ("cls" counts as "first"); else first for a codet5p_embedding model; else what
    1_Pooling/config.json states (pooling_mode_cls_token -> first); else mean."""
    if pooling:
        mode = {"cls": "first"}.get(str(pooling).strip().lower(), str(pooling).strip().lower())
        if mode not in ("first", "mean"):
            raise ValueError(f"pooling of a T5 encoder must be 'first' or 'mean', got {pooling!r}")
        return mode
    import json

    d = Path(model_dir)
    if json.loads((d / "config.json").read_text()).get("model_type") == "codet5p_embedding":
        return "first"
    conf = d / "1_Pooling" / "config.json"
    if conf.is_file() and bool(json.loads(conf.read_text()).get("pooling_mode_cls_token")):
        return "first"
    return "mean"


def load_t5_directory(model_dir: "str | Path", pooling: Optional[str] = None) -> dict:
    """Everything MI355XEmbeddings needs of a T5 encoder directory: cfg (t5_config of its config.json), blob (arch 3 order), proj (W, b) or
    (None, None), pooling, and tokenizer_json -- the directory's tokenizer.json (T5's Unigram and CodeT5's byte-level BPE alike go through
    HFTokenizer).  A directory with only the sentencepiece file is refused: convert it to a tokenizer.json first."""
    from safetensors.numpy import load_file

    d = Path(model_dir)
    if not (d / "tokenizer.json").is_file():
        if (d / "spiece.model").is_file():
            raise ValueError(f"{d} has spiece.model but no tokenizer.json: the sentencepiece file is not read here; write the fast tokenizer's "
                             "tokenizer.json (AutoTokenizer.from_pretrained(dir).save_pretrained(dir)) next to it")
        raise ValueError(f"{d} has no tokenizer.json")
    if not (d / "model.safetensors").is_file():
        raise ValueError(f"{d} has no model.safetensors (.bin checkpoints are not read)")
    cfg = t5_config(d / "config.json")
    cfg.pop("embed_dim", None)
    tensors = load_file(str(d / "model.safetensors"))
    return dict(cfg=cfg, blob=_t5_blob(d / "model.safetensors", tensors, cfg), proj=t5_projection(d, tensors), pooling=t5_pooling(d, pooling),
                tokenizer_json=d / "tokenizer.json")


def qwen3_config(config: "str | Path | dict") -> dict:
    """The encoder configuration of a transformers Qwen3 `config.json` (Qwen3-Embedding-0.6B): qwen2_config's fields, `head_dim` from the
    file (hidden_size / num_attention_heads without it; the 0.6B model states 128 at hidden 1 024), qk_norm=True -- the per-head RMSNorm of Q
    and K before the rotation -- and attention_bias honoured (the released models have none; a file with biases loads them).  The same
    max_pos cap and sliding_window refusal; a `layer_types` entry other than "full_attention" is refused by name."""
    if not isinstance(config, dict):
        import json

        config = json.loads(Path(config).read_text())
    c = config
    if c.get("model_type") != "qwen3":
        raise ValueError(f"not a Qwen3 configuration (model_type {c.get('model_type')!r})")
    if c.get("use_sliding_window") and int(c.get("sliding_window") or 0) < 2048:
        raise ValueError(f"Qwen3 config: use_sliding_window with sliding_window {c.get('sliding_window')} < 2048 is not supported (the causal kernel sees every earlier token)")
    for kind in c.get("layer_types") or ():
        if kind != "full_attention":
            raise ValueError(f"Qwen3 config: layer_types entry {kind!r} is not supported (full_attention only)")
    if c.get("hidden_act", "silu") != "silu":
        raise ValueError(f"Qwen3 config: hidden_act {c.get('hidden_act')!r} is not supported (silu only)")
    out = _qwen_common(c)
    hd = int(c.get("head_dim") or out["hidden"] // out["heads"])
    if hd not in (64, 128):
        raise ValueError(f"Qwen3 config: head_dim {hd} is not supported (64 or 128)")
    out.update(head_dim=hd, qk_norm=True)
    return out


def qwen2_config_beside(weights: "str | Path | None") -> Optional[dict]:
    """qwen2_config of the config.json next to a .safetensors file, None when there is none or it is another model's."""
    if not isinstance(weights, (str, Path)) or not str(weights).lower().endswith(".safetensors"):
        return None
    conf = Path(weights).parent / "config.json"
    if not conf.is_file():
        return None
    import json

    c = json.loads(conf.read_text())
    if c.get("model_type") == "qwen3":  # a causal directory too: the same pipeline with QK-norm
        return qwen3_config(c)
    return qwen2_config(c) if c.get("model_type") == "qwen2" else None


def tensors_rows(tensors: dict, name: str) -> int:
    """Number of rows (output features) of a 2-D checkpoint tensor, with or without the "bert." prefix."""
    for key in (name, "bert." + name):
        if key in tensors:
            return int(np.asarray(tensors[key]).shape[0])
    raise KeyError(name)


def load_weight_blob(path: "str | Path", layers: int, cfg: Optional[dict] = None) -> np.ndarray:
    """Flat f32 blob in ABI order from `.npy` (already flat), `.gguf` (llama.cpp's bert / jina-bert-v2 tensor names, F32 / F16 /
    BF16; embeddings/gguf.py) or `.safetensors` (HF BERT names, jina-bert-v2 names when the file holds `mlp.gated_layers`, or
    transformers' NomicBert names when it holds `layers.0.mlp.gate_proj`, or transformers' ModernBert names when it holds
    `layers.0.attn.Wqkv`, or transformers' Qwen2 names when it holds `embed_tokens`; optional "bert." / "nomic_bert." / "model." prefix).
    GGUF files of the ModernBERT and Qwen2 families are not read.  cfg: the
    encoder configuration the blob is for (checked against the checkpoint's architecture: a jina file needs alibi + geglu, a
    nomic file rotary + swiglu, a BERT file none of them)."""
    path = Path(path)
    if path.suffix == ".npy":
        return np.load(path, allow_pickle=False).astype(np.float32).reshape(-1)
    if path.suffix == ".safetensors":
        from safetensors.numpy import load_file

        tensors = load_file(str(path))

        def get(name: str) -> np.ndarray:
            for key in (name, "bert." + name):
                if key in tensors:
                    return np.asarray(tensors[key], dtype=np.float32).reshape(-1)
            raise KeyError(f"{path}: tensor {name!r} not found")

        if any(k in ("embed_tokens.weight", "model.embed_tokens.weight") for k in tensors):
            if cfg is not None and not (cfg.get("qwen2") and cfg.get("rotary") and cfg.get("swiglu")):
                raise ValueError(f"{path} is a Qwen2 checkpoint but the encoder configuration is not qwen2 + rotary + swiglu "
                                 "(qwen2_config reads it from the model's config.json)")
            return _qwen2_blob(path, tensors, layers, cfg)
        if cfg is not None and cfg.get("qwen2"):
            raise ValueError(f"{path} holds no Qwen2 tensors (embed_tokens.weight) but the encoder configuration says qwen2")
        jina = any(k.endswith("encoder.layer.0.mlp.gated_layers.weight") for k in tensors)
        nomic = any(k in ("layers.0.mlp.gate_proj.weight", "nomic_bert.layers.0.mlp.gate_proj.weight") for k in tensors)
        if any(k in ("layers.0.attn.Wqkv.weight", "model.layers.0.attn.Wqkv.weight") for k in tensors):
            if cfg is not None and not (cfg.get("modernbert") and cfg.get("rotary") and cfg.get("geglu")):
                raise ValueError(f"{path} is a ModernBERT checkpoint but the encoder configuration is not modernbert + rotary + geglu "
                                 "(modernbert_config reads it from the model's config.json)")
            return _modernbert_blob(path, tensors, layers)
        if cfg is not None and cfg.get("modernbert"):
            raise ValueError(f"{path} holds no ModernBERT tensors (layers.0.attn.Wqkv.weight) but the encoder configuration says modernbert")
        if cfg is not None and (bool(cfg.get("alibi")) != jina or bool(cfg.get("geglu")) != jina or bool(cfg.get("rotary")) != nomic
                                or bool(cfg.get("swiglu")) != nomic):
            kind = "nomic-bert (rotary + SwiGLU)" if nomic else "jina-bert-v2 (ALiBi + GEGLU)" if jina else "BERT"
            raise ValueError(f"{path} is a {kind} checkpoint but the encoder configuration says alibi={bool(cfg.get('alibi'))}, "
                             f"geglu={bool(cfg.get('geglu'))}, rotary={bool(cfg.get('rotary'))}, swiglu={bool(cfg.get('swiglu'))}")
        if nomic:
            return _nomic_blob(path, tensors, layers)
        head, layer = (_JINA_HEAD, _JINA_LAYER) if jina else (_HF_HEAD, _HF_LAYER)
        parts = [get(n) for n in head]
        for l in range(layers):
            for n in layer:
                if n is None:  # gated_layers has no bias: 2F zeros
                    parts.append(np.zeros(tensors_rows(tensors, f"encoder.layer.{l}.mlp.gated_layers.weight"), np.float32))
                else:
                    parts.append(get(f"encoder.layer.{l}.{n}"))
        return np.concatenate(parts)
    if path.suffix == ".gguf":  # the reference's local model format (settings.embedding_llamacpp_model_path): F32 / F16 / BF16 tensors
        from .gguf import gguf_to_blob

        blob, fcfg, _ = gguf_to_blob(path, cfg)
        if fcfg["layers"] != layers:
            raise ValueError(f"{path} has {fcfg['layers']} layers, the encoder configuration {layers}")
        return blob
    raise ValueError(f"unsupported weight file {path} (use .npy blob, .safetensors or .gguf)")


def cut_packed(lens: Sequence[int], budget: int, rows_of: "Callable[[np.ndarray], int]") -> "list[tuple[int, int]]":
    """Cuts texts of `lens` tokens, in order, into consecutive groups [a, b) for packed encoder calls: a group takes as many texts as
    rows_of(lens[a:b]) -- the token rows the encoder runs for them (Encoder.packed_rows) -- stays within `budget`; a text that alone
    exceeds the budget is a group of its own.  rows_of must not decrease when a text is appended."""
    lens = np.asarray(lens, dtype=np.int64)
    groups, a, n = [], 0, len(lens)
    while a < n:
        lo, hi = a + 1, n  # the largest b in [a + 1, n] whose group fits; a + 1 is taken whatever it costs
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if rows_of(lens[a:mid]) <= budget:
                lo = mid
            else:
                hi = mid - 1
        groups.append((a, lo))
        a = lo
    return groups


def flatten_ids(ids: np.ndarray, lens: np.ndarray) -> "tuple[np.ndarray, np.ndarray]":
    """Padded ids [n, S] + lens [n] -> (the real ids one text after another, offsets [n + 1]): the input of the packed encoder calls."""
    lens = np.asarray(lens, dtype=np.int64)
    offsets = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    keep = np.arange(ids.shape[1])[None, :] < lens[:, None]
    return np.ascontiguousarray(ids[keep], dtype=np.int32), offsets


def resolve_pooling(pooling: Optional[str] = None, setting: Optional[str] = None, weights: "str | Path | None" = None,
                    file_pooling: Optional[str] = None) -> str:
    """"mean", "cls" or "last" for MI355XEmbeddings, the first of: the argument; the setting mi355x_pooling; what a .gguf states
    (file_pooling = gguf_config(meta)["pooling"], or read from `weights` here); for a .safetensors the sentence-transformers
    1_Pooling/config.json in the file's directory (pooling_mode_cls_token true -> cls, pooling_mode_lasttoken true -> last); mean.
    "last" (the last real token's row) exists on Qwen2 encoders only: as an argument or a setting it is taken when `weights` is the
    .safetensors of a Qwen2 directory (config.json with model_type qwen2) and refused like any unknown value otherwise; "cls" on such
    a model is refused by the encoder."""
    for given, where in ((pooling, "pooling"), (setting, "SEMCODE_MI355X_POOLING")):
        if given:
            mode = str(given).strip().lower()
            if mode not in ("mean", "cls") and not (mode == "last" and qwen2_config_beside(weights) is not None):
                raise ValueError(f"{where} must be 'mean' or 'cls' (or 'last' with the weights of a Qwen2 model directory), got {given!r}")
            return mode
    path = Path(weights) if isinstance(weights, (str, Path)) else None
    if path is not None and path.suffix.lower() == ".gguf":
        if file_pooling is None:
            from .gguf import gguf_config, read_gguf

            file_pooling = gguf_config(read_gguf(path)[0])["pooling"]
        return file_pooling
    if path is not None and path.suffix.lower() == ".safetensors":
        conf = path.parent / "1_Pooling" / "config.json"
        if conf.is_file():
            import json

            pc = json.loads(conf.read_text())
            if bool(pc.get("pooling_mode_cls_token")):
                return "cls"
            if bool(pc.get("pooling_mode_lasttoken")):
                return "last"
    return "mean"


class MI355XEmbeddings:
    """LangChain-Embeddings-shaped client whose forward runs in libsemcode_hip on the MI355X.

    The model shape: a `.gguf` states it (head count included); a `.safetensors` or `.npy` blob does not, so `cfg` gives what differs
    from BERT-base.  Heads are 64 wide, or 32 for the 384-hidden family with learned positions -- all-MiniLM-L6-v2 (mean-pooled) is
    `cfg=dict(hidden=384, heads=12, layers=6, ffn=1536)`, all-MiniLM-L12-v2 the same with `layers=12`.

    Pooling: `pooling="mean"` (masked mean over the real tokens) or `"cls"` (the last hidden state of the first token: bge,
    snowflake-arctic-embed, mxbai-embed-large, gte); None resolves it as resolve_pooling does -- the setting mi355x_pooling, then what
    the file states (a GGUF's `bert.pooling_type`, a sentence-transformers `1_Pooling/config.json` next to a .safetensors), then mean.
    bge-small-en-v1.5 is `cfg=dict(hidden=384, heads=12, layers=12, ffn=1536), pooling="cls"`.

    ModernBERT (answerdotai/ModernBERT-base, gte-modernbert-base, modernbert-embed-base): point `weights` at the model.safetensors of
    the model directory -- the `config.json` beside it gives the whole configuration (modernbert_config) and the `tokenizer.json`
    beside it the byte-level BPE tokenizer (HFTokenizer; or `tokenizer_json=` / SEMCODE_MI355X_TOKENIZER_JSON).

    Qwen2 embedding models (the Qwen2 / Qwen2.5 0.5B backbone: jina-code-embeddings-0.5b, gte-Qwen2, KaLM-mini; heads of 64 only): the
    same three files of the model directory (qwen2_config); `pooling="last"` -- the last real token's row -- is what their
    1_Pooling/config.json states (pooling_mode_lasttoken) and what resolve_pooling then returns; their task prefixes go into
    document_prefix / query_prefix.  Texts stay capped at 2 048 tokens."""

    def __init__(self, model: Optional[str] = None, *, cfg: Optional[dict] = None, weights: "np.ndarray | str | Path | None" = None,
                 vocab: "dict | str | Path | None" = None, device: Optional[int] = None, max_tokens: Optional[int] = None,
                 normalize: bool = False, batch_size: int = 256, runtime: Any = None, synth_seed: int = 0,
                 allow_synthetic: Optional[bool] = None, document_prefix: Optional[str] = None, query_prefix: Optional[str] = None,
                 packed: Optional[bool] = None, packed_rows_budget: int = 65536, pooling: Optional[str] = None,
                 tokenizer_json: "str | Path | None" = None) -> None:
        from .. import _native  # raises loudly when libsemcode_hip.so is missing: there is no CPU fallback

        settings = _resolve_settings()
        self.model = model or getattr(settings, "embedding_model", None)
        self.max_tokens = int(max_tokens or getattr(settings, "mi355x_max_tokens", 512))
        self.batch_size = int(batch_size)
        # packed=True: a batch runs on the token rows its texts need (32-row alignment per text) instead of batch x longest text.
        # Off by default: packed and padded vectors agree to bf16 rounding, not bit for bit.
        self.packed = bool(packed if packed is not None else getattr(settings, "mi355x_packed", False))
        self.packed_rows_budget = int(packed_rows_budget)
        # task prefixes (nomic-embed-text expects "search_document: " / "search_query: "); llama.cpp behind LangChain adds none,
        # so none is the default
        self.document_prefix = str(document_prefix if document_prefix is not None else getattr(settings, "mi355x_document_prefix", "") or "")
        self.query_prefix = str(query_prefix if query_prefix is not None else getattr(settings, "mi355x_query_prefix", "") or "")
        # Like the reference's llama.cpp branch, which refuses to start without a model path (providers.py:77-81), a client
        # without weights or without a vocabulary is an error: random-init weights and the hash tokenizer produce vectors that
        # index and search without any error and mean nothing.  Benchmarks and tests opt in explicitly.
        if allow_synthetic is None:
            allow_synthetic = bool(getattr(settings, "mi355x_allow_synthetic", False))
        weights = weights if weights is not None else getattr(settings, "mi355x_weights_path", None)
        vocab = vocab if vocab is not None else getattr(settings, "mi355x_vocab_path", None)
        # the reference's own local-model setting (settings.py:51, providers.py:77-99): a checkout that points it at a GGUF file keeps it
        gguf_path = None
        if weights is None:
            cand = getattr(settings, "embedding_llamacpp_model_path", None)
            if cand and str(cand).lower().endswith(".gguf"):
                weights = cand
        if isinstance(weights, (str, Path)) and str(weights).lower().endswith(".gguf"):
            gguf_path = Path(weights)
        if weights is None and not allow_synthetic:
            raise ValueError("Set SEMCODE_MI355X_WEIGHTS_PATH (.safetensors, .gguf or .npy blob; a .gguf under SEMCODE_EMBEDDING_LLAMACPP_MODEL_PATH is taken too) when using the mi355x embedding provider "
                             "(or SEMCODE_MI355X_ALLOW_SYNTHETIC=1 for random-init benchmark weights).")
        self._native = _native
        self._cfg = dict(_native.BERT_BASE)
        self._vocab_tmp = None
        file_pooling = None
        # a T5 encoder directory (CodeT5+, GTR, sentence-T5; `weights` = the directory or its model.safetensors): config.json, the weights,
        # the projection behind the pooling, the pooling and tokenizer.json all come from it (load_t5_directory)
        t5 = None
        t5_dir = t5_model_dir(weights)
        if t5_dir is not None:
            t5 = load_t5_directory(t5_dir, pooling or getattr(settings, "mi355x_pooling", None))
            self._cfg = dict(t5["cfg"])
            weights = t5["blob"]
            if tokenizer_json is None and getattr(settings, "mi355x_tokenizer_json", None) is None:
                tokenizer_json = t5["tokenizer_json"]
        if gguf_path is not None:  # the file states its own architecture, and carries the WordPiece vocabulary
            from .gguf import gguf_config, gguf_vocab, read_gguf

            meta, tens = read_gguf(gguf_path)
            fcfg = gguf_config(meta)
            file_pooling = fcfg.pop("pooling")
            fcfg["vocab"] = int(tens["token_embd.weight"][1][0])
            fcfg["type_vocab"] = int(tens["token_types.weight"][1][0])
            if fcfg["alibi"]:
                fcfg["max_pos"] = max(int(fcfg["max_pos"]), int(self._cfg["max_pos"]))
            elif fcfg.get("rotary"):
                pass  # the file's context length stands: it bounds the sequence length and sizes the cos / sin table
            elif "position_embd.weight" in tens:
                fcfg["max_pos"] = int(tens["position_embd.weight"][1][0])
            self._cfg.update(fcfg)
            if vocab is None:
                toks = gguf_vocab(meta)
                if toks is not None:
                    import tempfile

                    self._vocab_tmp = tempfile.NamedTemporaryFile("w", suffix=".vocab.txt", encoding="utf-8", delete=False)
                    self._vocab_tmp.write("\n".join(toks) + "\n")
                    self._vocab_tmp.close()
                    vocab = self._vocab_tmp.name
        # a ModernBERT directory: config.json beside the .safetensors states the architecture; its tokenizer is a byte-level BPE
        # tokenizer.json (tokenizer_json=, SEMCODE_MI355X_TOKENIZER_JSON, or the file beside the weights when no vocab.txt is configured)
        mb_cfg = modernbert_config_beside(weights)
        if mb_cfg is not None:
            self._cfg.update(mb_cfg)
        # a Qwen2 directory (jina-code-embeddings-0.5b, gte-Qwen2, KaLM-mini): the same three files; 1_Pooling/config.json states "last"
        q2_cfg = qwen2_config_beside(weights)
        if q2_cfg is not None:
            self._cfg.update(q2_cfg)
        tokenizer_json = tokenizer_json if tokenizer_json is not None else getattr(settings, "mi355x_tokenizer_json", None)
        if tokenizer_json is None and vocab is None and isinstance(weights, (str, Path)) and (Path(weights).parent / "tokenizer.json").is_file():
            tokenizer_json = Path(weights).parent / "tokenizer.json"
        self._cfg.update(cfg or {})
        if vocab is None and tokenizer_json is None and not allow_synthetic:  # (a GGUF file brings its own vocabulary: checked after it was read)
            raise ValueError("Set SEMCODE_MI355X_VOCAB_PATH (vocab.txt of the model) when using the mi355x embedding provider "
                             "(or SEMCODE_MI355X_ALLOW_SYNTHETIC=1 for the hash-tokenizer stand-in).")
        self.max_tokens = min(self.max_tokens, self._cfg["max_pos"])
        self._fast_tokenizer: Any = None
        self._owns_runtime = False  # an explicit runtime is the caller's; the default one is shared with the vector store
        self._runtime = runtime or _native.shared_runtime(int(device if device is not None else getattr(settings, "mi355x_device", 0)))
        self.pooling = t5["pooling"] if t5 else resolve_pooling(pooling, getattr(settings, "mi355x_pooling", None), weights, file_pooling)
        if isinstance(weights, (str, Path)):
            weights = load_weight_blob(weights, self._cfg["layers"], self._cfg)
        if weights is None:
            log.warning("mi355x embeddings: no weights configured (SEMCODE_MI355X_WEIGHTS_PATH); using random-init weights seed=%d", synth_seed)
        self._encoder = _native.Encoder(self._runtime, self._cfg, weights=weights, normalize=normalize, synth_seed=synth_seed, pooling=self.pooling)
        if tokenizer_json is not None:  # the `tokenizers` library on the host; the native WordPiece thread pool is not used
            self.tokenizer = HFTokenizer(tokenizer_json)
        elif vocab is None:
            log.warning("mi355x embeddings: no vocab.txt configured (SEMCODE_MI355X_VOCAB_PATH); using the hash tokenizer stand-in")
            self.tokenizer: Any = HashTokenizer(self._cfg["vocab"])
        else:
            self.tokenizer = WordPieceTokenizer(vocab)
            if isinstance(vocab, (str, Path)):  # the C++ tokenizer (ASCII fast path + full Unicode normalisation, multi-threaded)
                self._fast_tokenizer = _native.NativeTokenizer(vocab)
        if t5 and t5["proj"][0] is not None:
            self._encoder.set_output_proj(*t5["proj"])
        self.dimension = self._encoder.out_dim  # hidden, or the width of the model's output projection: what a store is created with
        # Texts that reached max_tokens lost their tail.  The reference's default chunker emits up to 200 lines / 6 000 characters
        # (tree_sitter_chunker.py:64-65: 1.5-2k word pieces) and only shrinks chunks for llamacpp / lmstudio (ingestion/manager.py:68-79),
        # so with a 512-position BERT most real chunks are cut: counted here and logged (once per power of two), never silent.
        self.truncated_texts = 0
        self.total_texts = 0

    def _note_truncation(self, lens: np.ndarray) -> None:
        cut = int((np.asarray(lens) >= self.max_tokens).sum())
        self.total_texts += int(len(lens))
        if cut:
            before = self.truncated_texts
            self.truncated_texts += cut
            if before == 0 or (self.truncated_texts.bit_length() != before.bit_length()):
                log.warning("mi355x embeddings: %d of %d texts so far reached max_tokens=%d and were truncated (raise SEMCODE_MI355X_MAX_TOKENS up to "
                            "the model's context -- 1024 / 2048 need an encoder without a position table (ALiBi or rotary) or a table that long -- or shrink the chunker's max_lines)",
                            self.truncated_texts, self.total_texts, self.max_tokens)

    # ---- LangChain Embeddings surface (lists of Python floats)
    def embed_documents(self, texts: List[str]) -> List[List[float]]:
        return self.embed_documents_array(texts).tolist()

    def embed_query(self, text: str) -> List[float]:
        return self.embed_documents_array([text], kind="query")[0].tolist()

    # ---- array fast paths
    def embed_documents_array(self, texts: Sequence[str], kind: str = "document") -> np.ndarray:
        """texts -> [n, hidden] f32; tokenise on the host, forward on the device in batches."""
        out = np.empty((len(texts), self.dimension), dtype=np.float32)
        for start in range(0, len(texts), self.batch_size):
            ids, lens = self.tokenize(texts[start:start + self.batch_size], kind=kind)
            if self.packed:
                for a, b in self._packed_groups(lens):
                    out[start + a:start + b] = self._encoder.embed_packed(*flatten_ids(ids[a:b], lens[a:b]))
            else:
                out[start:start + len(lens)] = self._encoder.embed_ids(ids, lens)
        return out

    def _packed_groups(self, lens: np.ndarray) -> "list[tuple[int, int]]":
        """Consecutive groups of one tokenised batch, each within packed_rows_budget token rows."""
        return cut_packed(lens, self.packed_rows_budget, lambda l: self._encoder.packed_rows(np.concatenate(([0], np.cumsum(l)))))

    def tokenize(self, texts: Sequence[str], kind: str = "document") -> "tuple[np.ndarray, np.ndarray]":
        """texts -> (ids [n, S] int32 padded to the smallest sequence bucket that fits, lens [n]).  kind "document" | "query" picks
        the task prefix put in front of every text (both empty by default: the ids are then those of the bare texts)."""
        if kind not in ("document", "query"):
            raise ValueError(f"tokenize: kind must be 'document' or 'query', not {kind!r}")
        prefix = self.query_prefix if kind == "query" else self.document_prefix
        if prefix:
            texts = [prefix + t for t in texts]
        if self._fast_tokenizer is None:
            toks = [self.tokenizer.encode(t, self.max_tokens) for t in texts]
            ids, lens = pack(toks, getattr(self.tokenizer, "pad_id", 0), self.max_tokens)
            self._note_truncation(lens)
            return ids, lens
        from .tokenizer import bucket_for

        smax = bucket_for(10 ** 9, self.max_tokens)
        ids, lens, fallback = self._fast_tokenizer.encode_batch(texts, self.max_tokens, smax)
        for i in np.nonzero(fallback)[0]:  # only input that is not valid UTF-8 (cannot come out of a Python str)
            t = self.tokenizer.encode(texts[i], min(self.max_tokens, smax))
            ids[i, : len(t)] = t
            ids[i, len(t):] = self.tokenizer.pad_id
            lens[i] = len(t)
        S = bucket_for(int(lens.max()) if len(lens) else 1, self.max_tokens)
        self._note_truncation(lens)
        return np.ascontiguousarray(ids[:, :S]), lens

    def embed_ids_array(self, ids: np.ndarray, lens: np.ndarray) -> np.ndarray:
        """Pre-tokenised input: ids [B, S] (S one of 32/64/128/256/512/1024/2048), lens [B] -> [B, hidden] f32."""
        return self._encoder.embed_ids(ids, lens)

    def embed_ids_into(self, store: Any, ids: np.ndarray, lens: np.ndarray, rows: np.ndarray, want_host: bool = False,
                       wait: bool = True) -> "np.ndarray | None":
        """Embed pre-tokenised input and write the vectors into `store`'s device index at `rows` (store.plan_rows),
        device to device.  The store must sit on this client's runtime (the default for both).  wait=False enqueues the
        batch and returns (at most two in flight); call wait() before relying on its completion."""
        index = getattr(store, "_collection", None)
        if index is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        if getattr(store, "_runtime", None) is not self._runtime:
            raise RuntimeError("embed_ids_into: the vector store and the embedding client use different runtimes")
        if not self.packed:
            return self._encoder.embed_ids_into(ids, lens, index, rows, want_host=want_host, wait=wait)
        rows = np.asarray(rows, dtype=np.int64)
        got = [self._encoder.embed_packed_into(*flatten_ids(ids[a:b], lens[a:b]), index, rows[a:b], want_host=want_host, wait=wait)
               for a, b in self._packed_groups(lens)]
        return np.concatenate(got) if want_host else None

    def wait(self) -> None:
        """Block until every batch enqueued with embed_ids_into(..., wait=False) has finished."""
        self._encoder.wait()

    def close(self) -> None:
        self._encoder.close()
        if self._owns_runtime:
            self._runtime.close()


class EmbeddingProviderFactory:
    """Factory that returns embedding clients based on configuration."""

    @staticmethod
    def create(provider: "str | None" = None, model: "str | None" = None) -> Any:
        settings = _resolve_settings()
        provider_name = (provider or settings.embedding_provider).lower()

        if provider_name in MI355X_PROVIDER_NAMES:
            embed_model = model or settings.embedding_model
            log.info("initializing_mi355x_embeddings model=%s", embed_model)
            return MI355XEmbeddings(model=embed_model)

        if provider_name in {"openai", "lmstudio"} or provider_name.startswith("openai"):
            from langchain_openai import OpenAIEmbeddings  # type: ignore

            embed_model = model or settings.embedding_model
            kwargs: dict[str, Any] = {"model": embed_model, "encoding_format": "float"}
            if settings.embedding_api_base:
                kwargs["base_url"] = settings.embedding_api_base
            if settings.embedding_api_key:
                kwargs["api_key"] = settings.embedding_api_key
            if provider_name != "openai" or not settings.embedding_use_tiktoken:
                kwargs["tiktoken_enabled"] = False
            return OpenAIEmbeddings(**kwargs)

        if provider_name == "jina":
            from langchain_community.embeddings import JinaEmbeddings  # type: ignore

            embed_model = model or settings.embedding_model or "jina-embeddings-v2-base-en"
            jina_kwargs: dict[str, Any] = {"model_name": embed_model}
            if settings.embedding_api_key:
                jina_kwargs["jina_api_key"] = settings.embedding_api_key
            return JinaEmbeddings(**jina_kwargs)

        if provider_name in {"llamacpp", "llama.cpp"}:
            try:
                from langchain_community.embeddings import LlamaCppEmbeddings  # type: ignore
            except ImportError as exc:  # pragma: no cover - optional dependency
                raise RuntimeError(
                    "llama-cpp-python is required for llama.cpp embeddings. "
                    "Install it or select a different embedding provider."
                ) from exc
            model_path = settings.embedding_llamacpp_model_path
            if not model_path:
                raise ValueError("Set SEMCODE_EMBEDDING_LLAMACPP_MODEL_PATH when using the llama.cpp embedding provider.")
            # every argument the reference passes (providers.py:85-99): this branch is untouched by the MI355X backend and a
            # checkout that selects it must construct the very same client
            llama_kwargs: dict[str, Any] = {"model_path": str(model_path), "n_ctx": settings.embedding_llamacpp_n_ctx,
                                            "n_threads": settings.embedding_llamacpp_n_threads, "n_parts": -1, "seed": 0, "f16_kv": True,
                                            "logits_all": False, "vocab_only": False, "use_mlock": False,
                                            "n_batch": settings.embedding_llamacpp_batch_size, "n_gpu_layers": 0, "verbose": False,
                                            "device": "cpu"}
            return LlamaCppEmbeddings(**llama_kwargs)

        raise NotImplementedError(f"Embedding provider not yet supported: {provider_name}")


def create_reranker(model: "str | None" = None, **kwargs: Any) -> Any:
    """The cross-encoder for `Retriever(reranker=...)`: an MI355XReranker on settings.mi355x_reranker_path (or `model`) -- a `.safetensors`
    file of a BERT cross-encoder, or a directory of a ModernBERT / Qwen2 / Qwen3 reranker --, None when
    neither is set -- reranking is opt-in, the reference's pipeline has no such stage."""
    settings = _resolve_settings()
    path = model or getattr(settings, "mi355x_reranker_path", None)
    if not path:
        return None
    from . import reranker

    kind = str(kwargs.pop("kind", None) or getattr(settings, "mi355x_reranker_kind", "auto") or "auto").lower()
    if kind not in ("auto", "cross", "late"):
        raise ValueError(f"mi355x_reranker_kind must be auto, cross or late, not {kind!r}")
    from . import late

    if kind == "late" or (kind == "auto" and late.is_late_dir(path)):  # a PyLate or Stanford ColBERT directory: token vectors and MaxSim
        log.info("initializing_mi355x_late_reranker directory=%s", path)
        return late.MI355XLateReranker(path, **kwargs)
    if Path(path).is_dir():  # a transformers directory: a ModernBERT or Qwen2 / Qwen3 reranker, its prompt and score tokens from the settings
        for key, name in (("instruction", "mi355x_reranker_instruction"), ("true_token", "mi355x_reranker_true_token"), ("false_token", "mi355x_reranker_false_token")):
            value = getattr(settings, name, None)
            if value and key not in kwargs:
                kwargs[key] = value
        log.info("initializing_mi355x_reranker directory=%s", path)
    else:
        log.info("initializing_mi355x_reranker model=%s", path)
    return reranker.MI355XReranker(path, **kwargs)
