"""Settings read at the two seams -- same field names and SEMCODE_ env prefix as the reference.

Reference: AppSettings, src/semcode/settings.py:30-82 (pydantic-settings, env prefix SEMCODE_,
extra="allow").  When this package is dropped into a semcode checkout the real
`semcode.settings.settings` object is used instead (see `resolve()`); this stand-alone twin keeps the
seams usable (and testable) without pydantic_settings, which is absent in the build image.

Backend-specific keys ride on the reference's extra="allow" (settings.py:36):
    mi355x_device, mi355x_metric, mi355x_index_type, mi355x_nlist, mi355x_nprobe,
    mi355x_weights_path, mi355x_vocab_path, mi355x_allow_synthetic, mi355x_max_tokens, mi355x_store_path, mi355x_ingest_batch,
    mi355x_document_prefix, mi355x_query_prefix, mi355x_packed, mi355x_pooling, mi355x_lexical,
    mi355x_reranker_path, mi355x_reranker_vocab, mi355x_rerank_fetch_k, mi355x_tokenizer_json,
    mi355x_reranker_instruction, mi355x_reranker_true_token, mi355x_reranker_false_token, mi355x_reranker_kind, mi355x_late_store,
    mi355x_late_handover
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Any

_DEFAULTS: dict[str, Any] = {
    # --- names the reference seams read (settings.py:40-76) ---
    "workspace_root": Path("./workspace"),
    "milvus_uri": "http://localhost:19530",
    "milvus_username": None,
    "milvus_password": None,
    "embedding_provider": "openai",
    "embedding_model": "text-embedding-3-large",
    "embedding_dimension": 3072,
    "embedding_api_base": None,
    "embedding_api_key": None,
    "embedding_use_tiktoken": True,
    "embedding_llamacpp_model_path": None,
    "embedding_llamacpp_n_ctx": 2048,
    "embedding_llamacpp_n_threads": 4,
    "embedding_llamacpp_batch_size": 256,
    "embedding_batch_size": 64,
    "rag_max_context_sources": 5,
    "milvus_upsert_batch_size": 128,
    # --- MI355X backend keys (extra="allow") ---
    "mi355x_device": 0,
    "mi355x_metric": "IP",            # milvus_store.py:78-82
    "mi355x_index_type": "IVF_FLAT",  # milvus_store.py:80
    "mi355x_nlist": 128,              # milvus_store.py:81
    "mi355x_nprobe": 16,              # milvus_store.py:144
    "mi355x_weights_path": None,
    "mi355x_vocab_path": None,
    "mi355x_tokenizer_json": None,    # a `tokenizer.json` (byte-level BPE of ModernBERT models) instead of a WordPiece vocab.txt
    "mi355x_allow_synthetic": False,  # random-init weights / hash tokenizer when the two paths above are unset (benchmarks only)
    "mi355x_max_tokens": 512,
    "mi355x_document_prefix": "",     # put in front of every indexed text ("search_document: " for nomic-embed-text)
    "mi355x_query_prefix": "",        # put in front of every query ("search_query: ")
    "mi355x_store_path": None,
    "mi355x_ingest_batch": 256,       # chunks per embed+upsert batch of services.indexer.ingest_chunks
    "mi355x_packed": False,           # embed variable-length batches packed (no padding to the longest text of a batch)
    "mi355x_pooling": "",             # "mean" | "cls" | "last" (Qwen2 models only); empty: what the weight file states (GGUF pooling_type, 1_Pooling/config.json), else mean
    "mi355x_lexical": False,          # keep a term row per chunk on the device for hybrid (BM25 + dense) search: MilvusVectorStore(lexical=...)
    "mi355x_reranker_path": None,     # .safetensors of a BertForSequenceClassification cross-encoder, or a transformers directory of a ModernBERT / Qwen2 / Qwen3 reranker (embeddings/reranker.py)
    "mi355x_reranker_kind": "auto",   # "auto" | "cross" | "late": late = token vectors + MaxSim (embeddings/late.py); auto = late when the directory holds config_sentence_transformers.json or artifact.metadata
    "mi355x_reranker_vocab": None,    # its vocab.txt (default: mi355x_vocab_path)
    "mi355x_reranker_instruction": "",     # decoder rerankers: the task instruction of the prompt (empty: the template's own)
    "mi355x_reranker_true_token": "yes",   # causal-LM rerankers: the vocabulary entry whose logit says "relevant" ...
    "mi355x_reranker_false_token": "no",   # ... and the one that says "not": score = logit_true - logit_false
    "mi355x_rerank_fetch_k": 40,      # hits the store is asked for when Retriever.retrieve(rerank=True) re-orders them
    "mi355x_late_store": "off",       # "off" | "f32" | "bf16": keep every chunk's token vectors of the late-interaction reranker next to its row (MilvusVectorStore(late=..., late_format=...))
    "mi355x_late_handover": True,     # with a late store: the reranker's token head writes a chunk's vectors straight into the index's token pool; off = download, drop punctuation on the host, upload (the same stored bits)
}


def _coerce(raw: str, like: Any) -> Any:
    if isinstance(like, bool):
        return raw.strip().lower() in {"1", "true", "yes", "on"}
    if isinstance(like, int):
        return int(raw)
    if isinstance(like, float):
        return float(raw)
    if isinstance(like, Path):
        return Path(raw)
    return raw


class Settings:
    """Attribute bag with SEMCODE_<NAME> environment overrides; unknown attributes may be set (extra="allow")."""

    def __init__(self, **overrides: Any) -> None:
        for name, default in _DEFAULTS.items():
            raw = os.environ.get("SEMCODE_" + name.upper())
            setattr(self, name, _coerce(raw, default) if raw is not None else default)
        for name, value in overrides.items():
            setattr(self, name, value)


def resolve() -> Any:
    """semcode's own settings object when running inside a semcode checkout, else the twin above."""
    try:  # pragma: no cover - semcode is not importable in the build image
        from semcode.settings import settings as real

        return real
    except Exception:
        return settings


settings = Settings()
