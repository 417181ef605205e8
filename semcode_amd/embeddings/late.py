"""Late-interaction reranker (ColBERT): one vector per token, scored by MaxSim on the device.

The second kind of reranker next to the cross-encoders of embeddings/reranker.py.  A cross-encoder pays a full forward for every
(question, passage) pair; a late-interaction model encodes every question and every passage once, independently, and a pair costs one
small matrix product (sc_encoder_score_late: both forwards and the MaxSim kernel in one call, the token vectors stay on the device).

  question = [CLS] marker tokens [SEP] cut to 32 rows in all, then [MASK] rows up to 32 added by the library: attended as queries,
             masked as keys -- ColBERT's query augmentation
  passage  = [CLS] marker tokens [SEP] cut to document_length; tokens of the skiplist (punctuation) take no part in a maximum
  score    = sum over the question's rows of the largest dot product with a kept passage token

load_late_dir reads two directory layouts, everything as data:
  PyLate:            config.json + model.safetensors + tokenizer (vocab.txt or tokenizer.json), 1_Dense/model.safetensors with linear.weight
                     [W, H] and no bias, config_sentence_transformers.json (query_prefix, document_prefix, query_length, document_length,
                     attend_to_expansion_tokens, skiplist_words)
  Stanford ColBERT:  artifact.metadata (query_maxlen, doc_maxlen, dim, mask_punctuation, attend_to_mask_tokens), [unused0] / [unused1] as
                     the markers, linear.weight beside the bert.* tensors of model.safetensors
Refused: expansion tokens that are attended (attend_to_expansion_tokens / attend_to_mask_tokens), a query length other than 32, a
projection with a bias.  Backbones: BERT (arch 0, heads of 64 or 32) and ModernBERT (arch 1).
"""
from __future__ import annotations

import json
import logging
import string
from pathlib import Path
from typing import Any, List, Optional, Sequence

import numpy as np

from ..settings import resolve as _resolve_settings
from .providers import cut_packed, load_weight_blob, modernbert_config
from .tokenizer import WordPieceTokenizer

log = logging.getLogger(__name__)

__all__ = ["MI355XLateReranker", "load_late_dir", "is_late_dir", "bert_config", "QUERY_LENGTH", "LATE_CONFIG_FILES"]

QUERY_LENGTH = 32
LATE_CONFIG_FILES = ("config_sentence_transformers.json", "artifact.metadata")


def is_late_dir(path: "str | Path") -> bool:
    """A directory that holds one of the two late-interaction config files."""
    path = Path(path)
    return path.is_dir() and any((path / name).is_file() for name in LATE_CONFIG_FILES)


def bert_config(config: "str | Path | dict") -> dict:
    """The encoder configuration of a transformers BERT `config.json` (path or parsed dict)."""
    c = config if isinstance(config, dict) else json.loads(Path(config).read_text())
    act = c.get("hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_act {act!r} is not supported (gelu only)")
    if c.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError(f"position_embedding_type {c.get('position_embedding_type')!r} is not supported (absolute only)")
    return dict(vocab=int(c["vocab_size"]), hidden=int(c["hidden_size"]), layers=int(c["num_hidden_layers"]), heads=int(c["num_attention_heads"]),
                ffn=int(c["intermediate_size"]), max_pos=int(c["max_position_embeddings"]), type_vocab=int(c.get("type_vocab_size", 2)),
                ln_eps=float(c.get("layer_norm_eps", 1e-12)))


def load_late_dir(path: "str | Path", cfg: Optional[dict] = None) -> "tuple[dict, np.ndarray, np.ndarray, dict]":
    """A late-interaction model directory -> (encoder cfg updated by `cfg`, weight blob in ABI order, projection [W, H] f32, meta).
    meta: layout ("pylate" | "stanford"), query_marker / document_marker (vocabulary entries), query_length, document_length,
    skiplist (list of words)."""
    from safetensors.numpy import load_file

    path = Path(path)
    conf, weights = path / "config.json", path / "model.safetensors"
    if not conf.is_file() or not weights.is_file():
        raise FileNotFoundError(f"{path}: a late-interaction directory needs config.json and model.safetensors")
    st, art = path / LATE_CONFIG_FILES[0], path / LATE_CONFIG_FILES[1]
    c = json.loads(conf.read_text())
    if st.is_file():
        m = json.loads(st.read_text())
        if m.get("attend_to_expansion_tokens"):
            raise ValueError(f"{st}: attend_to_expansion_tokens is true; the expansion rows are never attended as keys here")
        meta = dict(layout="pylate", query_marker=str(m.get("query_prefix", "[Q] ")).strip(), document_marker=str(m.get("document_prefix", "[D] ")).strip(),
                    query_length=int(m.get("query_length", QUERY_LENGTH)), document_length=int(m.get("document_length", 180)),
                    skiplist=list(m.get("skiplist_words") or []))
        dense = path / "1_Dense" / "model.safetensors"
        if not dense.is_file():
            raise FileNotFoundError(f"{path}: 1_Dense/model.safetensors (the per-token projection) not found")
        head = load_file(str(dense))
    elif art.is_file():
        m = json.loads(art.read_text())
        if m.get("attend_to_mask_tokens"):
            raise ValueError(f"{art}: attend_to_mask_tokens is true; the expansion rows are never attended as keys here")
        meta = dict(layout="stanford", query_marker="[unused0]", document_marker="[unused1]", query_length=int(m.get("query_maxlen", QUERY_LENGTH)),
                    document_length=int(m.get("doc_maxlen", 180)), skiplist=list(string.punctuation) if m.get("mask_punctuation", True) else [])
        head = load_file(str(weights))
    else:
        raise FileNotFoundError(f"{path}: neither {LATE_CONFIG_FILES[0]} (PyLate) nor {LATE_CONFIG_FILES[1]} (Stanford ColBERT) found")
    if meta["query_length"] != QUERY_LENGTH:
        raise ValueError(f"{path}: query length {meta['query_length']} is not supported ({QUERY_LENGTH} only: the expansion fills one 32-row span)")
    if "linear.bias" in head:
        raise ValueError(f"{path}: the projection has a bias (linear.bias); the token head is a plain matrix")
    if "linear.weight" not in head:
        raise KeyError(f"{path}: tensor 'linear.weight' (the per-token projection) not found")
    proj = np.ascontiguousarray(head["linear.weight"], dtype=np.float32)
    modern = c.get("model_type") == "modernbert"
    full = modernbert_config(c) if modern else bert_config(c)
    full.update(cfg or {})
    if proj.ndim != 2 or proj.shape[1] != full["hidden"]:
        raise ValueError(f"{path}: linear.weight is {proj.shape}, expected [W, {full['hidden']}]")
    if "dim" in m and int(m["dim"]) != proj.shape[0]:
        raise ValueError(f"{path}: artifact.metadata says dim {m['dim']}, linear.weight has {proj.shape[0]} rows")
    if proj.shape[0] % 16 or not 16 <= proj.shape[0] <= 128:
        raise ValueError(f"{path}: token width {proj.shape[0]} is not supported (a multiple of 16 within 16 .. 128)")
    blob = load_weight_blob(weights, full["layers"], full)
    return full, blob, proj, meta


def _token_id(tokenizer: Any, token: str) -> int:
    vocab = getattr(tokenizer, "vocab", None)
    if isinstance(vocab, dict):
        if token not in vocab:
            raise ValueError(f"token {token!r} is not an entry of the vocabulary")
        return int(vocab[token])
    inner = getattr(tokenizer, "_tok", None)
    i = inner.token_to_id(token) if inner is not None else None
    if i is None:
        raise ValueError(f"token {token!r} is not an entry of the tokenizer's vocabulary")
    return int(i)


def _flatten(rows: "Sequence[Sequence[int]]") -> "tuple[np.ndarray, np.ndarray]":
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return np.fromiter((t for r in rows for t in r), dtype=np.int32, count=int(offsets[-1])), offsets


class MI355XLateReranker:
    """score_pairs(questions, passages) / rerank(question, texts, top_k) with both forwards and MaxSim on the device.

    model: a PyLate or Stanford ColBERT directory (load_late_dir).  Or, for tests and benchmarks: weights (blob) + proj + cfg + tokenizer
    + meta given directly.  `encoder` replaces the device encoder by any object with packed_rows / score_late / embed_tokens."""

    def __init__(self, model: "str | Path | None" = None, *, cfg: Optional[dict] = None, weights: "np.ndarray | None" = None, proj: "np.ndarray | None" = None,
                 meta: Optional[dict] = None, tokenizer: Any = None, device: Optional[int] = None, runtime: Any = None, rows_budget: int = 65536,
                 encoder: Any = None) -> None:
        settings = _resolve_settings()
        model = model if model is not None else getattr(settings, "mi355x_reranker_path", None)
        self.model = str(model) if model else None
        self.rows_budget = int(rows_budget)
        if weights is None and encoder is None:
            if not model:
                raise ValueError("Set SEMCODE_MI355X_RERANKER_PATH to a PyLate or Stanford ColBERT directory to use the late-interaction reranker.")
            full, weights, proj, meta = load_late_dir(model, cfg)
            if tokenizer is None:
                tj, vt = Path(model) / "tokenizer.json", Path(model) / "vocab.txt"
                if vt.is_file():
                    tc = Path(model) / "tokenizer_config.json"
                    tokenizer = WordPieceTokenizer(vt, lowercase=bool(json.loads(tc.read_text()).get("do_lower_case", True)) if tc.is_file() else True)
                elif tj.is_file():
                    from .tokenizer import HFTokenizer

                    tokenizer = HFTokenizer(tj)
                else:
                    raise FileNotFoundError(f"{model}: neither vocab.txt nor tokenizer.json found")
        else:
            if cfg is None or tokenizer is None or meta is None:
                raise ValueError("weights (or an encoder) given directly need cfg, tokenizer and meta")
            full = dict(cfg)
        self._cfg, self.meta, self.tokenizer = full, dict(meta), tokenizer
        self.mask_id = _token_id(tokenizer, "[MASK]")
        self.query_marker_id = _token_id(tokenizer, meta["query_marker"])
        self.document_marker_id = _token_id(tokenizer, meta["document_marker"])
        self.document_length = max(3, min(int(meta["document_length"]), int(full["max_pos"]), 2048))
        skip = set()
        for word in meta.get("skiplist") or ():
            try:
                skip.add(_token_id(tokenizer, word))
            except ValueError:
                pass  # a word the vocabulary does not hold can never appear
        self.skip_ids = np.fromiter(sorted(skip), dtype=np.int32, count=len(skip))
        if encoder is not None:
            self._runtime, self._encoder = None, encoder
            return
        from .. import _native  # raises loudly when libsemcode_hip.so is missing: there is no CPU fallback

        self._runtime = runtime or _native.shared_runtime(int(device if device is not None else getattr(settings, "mi355x_device", 0)))
        self._encoder = _native.Encoder(self._runtime, full, weights=weights)
        self._encoder.set_token_head(proj)

    # ---- texts -> ids
    def _marked(self, text: str, marker: int, max_tokens: int) -> "List[int]":
        ids = self.tokenizer.encode(text, max_tokens - 1)  # [CLS] pieces [SEP]; the marker takes one more row
        return [ids[0], marker] + list(ids[1:])

    def query_ids(self, text: str) -> "List[int]":
        return self._marked(text, self.query_marker_id, QUERY_LENGTH)

    def document_ids(self, text: str) -> "List[int]":
        return self._marked(text, self.document_marker_id, self.document_length)

    def keep_flags(self, d_ids: np.ndarray) -> np.ndarray:
        return (~np.isin(d_ids, self.skip_ids)).astype(np.uint8)

    # ---- token vectors (for callers that keep them; score_pairs never downloads any)
    def embed_query_tokens(self, texts: Sequence[str]) -> "list[np.ndarray]":
        ids, off = _flatten([self.query_ids(t) for t in texts])
        vec, counts = self._encoder.embed_tokens(ids, off, expand_id=self.mask_id)
        return np.split(vec, np.cumsum(counts)[:-1])

    def embed_document_tokens(self, texts: Sequence[str], kept_only: bool = False) -> "list[np.ndarray]":
        """One [n_i, W] array per text.  kept_only: without the tokens whose keep flag is 0 (punctuation) -- what a token store keeps,
        since score_pairs leaves exactly those out of every maximum.  Batches follow rows_budget, as score_pairs' do."""
        rows = [self.document_ids(t) for t in texts]
        out: "list[np.ndarray]" = []
        rows_of = lambda l: self._encoder.packed_rows(np.concatenate(([0], np.cumsum(l))))  # noqa: E731
        window = max(1, 524288 // max(self.document_length, 32) // 2)
        lens = np.asarray([len(r) for r in rows], np.int64)
        for start in range(0, len(rows), window):
            for a, b in cut_packed(lens[start:start + window], self.rows_budget, rows_of):
                ids, off = _flatten(rows[start + a:start + b])
                vec, counts = self._encoder.embed_tokens(ids, off, expand_id=-1)
                parts = np.split(vec, np.cumsum(counts)[:-1])
                if kept_only:
                    keep = self.keep_flags(ids).astype(bool)
                    parts = [p[keep[off[i]:off[i + 1]]] for i, p in enumerate(parts)]
                out += parts
        return out

    def shares_runtime(self, index: Any) -> bool:
        """True when the device encoder and `index` live on one runtime: store_document_tokens can write into that index."""
        rt = getattr(self._encoder, "rt", None)
        return rt is not None and rt is getattr(index, "rt", None) and hasattr(self._encoder, "embed_tokens_into")

    def store_document_tokens(self, texts: Sequence[str], index: Any, rows: Any, fmt: str = "f32") -> np.ndarray:
        """The texts' kept token vectors as the tokens of `rows` of the device index, handed over on the device (Encoder.embed_tokens_into):
        what index.put_tokens(rows, embed_document_tokens(texts, kept_only=True), fmt) stores, bit for bit, without the vectors' trip
        through the host.  Same ids, same keep flags, same batches under rows_budget.  -> the kept counts [n] int32."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if len(rows) != len(texts):
            raise ValueError(f"{len(texts)} texts but {len(rows)} rows")
        docs = [self.document_ids(t) for t in texts]
        counts = np.zeros(len(docs), np.int32)
        rows_of = lambda l: self._encoder.packed_rows(np.concatenate(([0], np.cumsum(l))))  # noqa: E731
        window = max(1, 524288 // max(self.document_length, 32) // 2)
        lens = np.asarray([len(r) for r in docs], np.int64)
        for start in range(0, len(docs), window):
            for a, b in cut_packed(lens[start:start + window], self.rows_budget, rows_of):
                ids, off = _flatten(docs[start + a:start + b])
                counts[start + a:start + b] = self._encoder.embed_tokens_into(ids, off, self.keep_flags(ids), index, rows[start + a:start + b], fmt)
        return counts

    # ---- scores
    def score_pairs(self, questions: Sequence[str], passages: Sequence[str]) -> np.ndarray:
        """(question i, passage i) -> MaxSim scores [n] f32 (higher = more relevant).  Every distinct question and passage is encoded once
        per batch; batches are consecutive groups of distinct passages within rows_budget token rows, sent with the questions they pair with."""
        if len(questions) != len(passages):
            raise ValueError("score_pairs: as many questions as passages")
        n = len(questions)
        if n == 0:
            return np.empty(0, np.float32)
        uq, up = list(dict.fromkeys(questions)), list(dict.fromkeys(passages))
        q_index, p_index = {t: i for i, t in enumerate(uq)}, {t: i for i, t in enumerate(up)}
        q_rows, p_rows = [self.query_ids(t) for t in uq], [self.document_ids(t) for t in up]
        pq = np.fromiter((q_index[t] for t in questions), dtype=np.int64, count=n)
        pp = np.fromiter((p_index[t] for t in passages), dtype=np.int64, count=n)
        rows_of = lambda l: self._encoder.packed_rows(np.concatenate(([0], np.cumsum(l))))  # noqa: E731
        window = max(1, 524288 // max(self.document_length, 32) // 2)  # (a window cut_packed may bisect without a refusal)
        lens = np.asarray([len(r) for r in p_rows], np.int64)
        groups = []
        for start in range(0, len(lens), window):
            groups += [(start + a, start + b) for a, b in cut_packed(lens[start:start + window], self.rows_budget, rows_of)]
        out = np.empty(n, np.float32)
        for a, b in groups:
            sel = np.nonzero((pp >= a) & (pp < b))[0]  # the pairs whose passage lies in this batch
            if len(sel) == 0:
                continue
            qs = np.unique(pq[sel])
            q_local = {int(g): i for i, g in enumerate(qs)}
            q_ids, q_off = _flatten([q_rows[int(g)] for g in qs])
            d_ids, d_off = _flatten(p_rows[a:b])
            out[sel] = self._encoder.score_late(q_ids, q_off, d_ids, d_off, np.fromiter((q_local[int(g)] for g in pq[sel]), np.int32, len(sel)),
                                                (pp[sel] - a).astype(np.int32), expand_id=self.mask_id, d_keep=self.keep_flags(d_ids))
        return out

    def rerank(self, question: str, texts: Sequence[str], top_k: Optional[int] = None) -> "tuple[np.ndarray, np.ndarray]":
        """(order, scores): indices into texts, best first (equal scores keep their order), and their scores; cut to top_k."""
        scores = self.score_pairs([question] * len(texts), list(texts))
        order = np.argsort(-scores, kind="stable")
        if top_k is not None:
            order = order[: max(0, int(top_k))]
        return order, scores[order]

    def close(self) -> None:
        close = getattr(self._encoder, "close", None)
        if close is not None:
            close()
