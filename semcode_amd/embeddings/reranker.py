"""Cross-encoder reranking on the MI355X: the stage after retrieval.

The bi-encoder embeds question and chunk apart; a cross-encoder reads them TOGETHER -- one sequence `[CLS] question [SEP] chunk [SEP]`
with segment ids 0 / 1 -- and scores the pair from its [CLS] row (BertForSequenceClassification: pooler dense + tanh, then a linear
layer to 1 or 2 logits).  The forward is the packed encoder forward of libsemcode_hip (sc_encoder_score_pairs); this module builds the
pairs on the host, cuts them into packed batches and turns logits into scores.  The reference has no such stage (its pipeline hands
the store's hits to the LLM as they come, src/semcode/rag/pipeline.py:93-129); `services.retrieval.Retriever(reranker=...)` adds it.

Weights: a `.safetensors` file with BertForSequenceClassification names (`bert.embeddings...`, `bert.encoder.layer.N...`,
`bert.pooler.dense.{weight,bias}`, `classifier.{weight,bias}`); the encoder shape is read from the tensors, the head count from `num_attention_heads` of a `config.json`
beside the file (MiniLM cross-encoders: 384 hidden = 12 heads of 32), hidden // 64 without one; `cfg` overrides both.  A file without
`bert.pooler.dense` gives a head without pooler.  Models without a position table are accepted when their type_vocab is at least 2
and the caller's cfg names the position scheme and the length bound (alibi=True or rotary=True, max_pos: the file cannot), but no
reference pins what they compute.  Out of scope: SentencePiece vocabularies (XLM-R rerankers),
Electra-style heads, more than two labels.
"""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Any, List, Optional, Sequence

import numpy as np

from ..settings import resolve as _resolve_settings
from .providers import cut_packed, load_weight_blob, tensors_rows
from .tokenizer import WordPieceTokenizer

log = logging.getLogger(__name__)

__all__ = ["MI355XReranker", "build_pairs", "cut_pair_batches", "encode_many", "scores_from_logits", "load_reranker", "pair_limits"]

MAX_PAIR_TOKENS = 512


def pair_limits(max_pos: int, max_query_tokens: int = 64) -> "tuple[int, int]":
    """(tokens a pair may have, tokens its question part may have, specials included): min(max_pos, 512), and the question leaves
    room for at least one passage token and the closing [SEP]."""
    max_len = min(int(max_pos), MAX_PAIR_TOKENS)
    if max_len < 4:
        raise ValueError(f"a pair needs at least 4 positions, the model has {max_pos}")
    return max_len, max(2, min(int(max_query_tokens), max_len - 2))


def stitch_pair(q_ids: Sequence[int], p_ids: Sequence[int], max_len: int) -> "tuple[list[int], int]":
    """q_ids = [CLS] question [SEP] (already cut to the question budget), p_ids = [CLS] passage [SEP] -> ([CLS] question [SEP] passage
    [SEP] within max_len tokens, the passage cut -- BertTokenizer(q, p, truncation="only_second") --, number of segment-0 tokens)."""
    q = list(q_ids)
    room = max_len - len(q)  # passage pieces + the closing [SEP]
    if room < 1:
        raise ValueError(f"question of {len(q)} tokens leaves no room in {max_len}")
    pieces = list(p_ids[1:-1])[: room - 1]
    if not pieces:  # an empty passage: the question alone, as BertTokenizer(q, "") gives it
        return q, len(q)
    return q + pieces + [p_ids[-1]], len(q)


def encode_many(tokenizer: Any, fast_tokenizer: Any, texts: Sequence[str], max_tokens: int) -> "List[List[int]]":
    """texts -> [CLS] pieces [SEP] id lists of at most max_tokens: one batch through the C++ tokenizer (_native.NativeTokenizer) when
    there is one -- a text it leaves alone goes through `tokenizer` --, else tokenizer.encode per text.  The same ids either way."""
    if fast_tokenizer is None or not texts:
        return [tokenizer.encode(t, max_tokens) for t in texts]
    from .tokenizer import bucket_for

    ids, lens, fallback = fast_tokenizer.encode_batch(list(texts), max_tokens, bucket_for(max_tokens, 10 ** 9))
    return [tokenizer.encode(t, max_tokens) if fallback[i] else ids[i, : lens[i]].tolist() for i, t in enumerate(texts)]


def build_pairs(tokenizer: Any, questions: Sequence[str], passages: Sequence[str], max_len: int = MAX_PAIR_TOKENS, max_query_tokens: int = 64,
                encode_many: Any = None) -> "tuple[np.ndarray, np.ndarray, np.ndarray]":
    """(question i, passage i) -> packed input of Encoder.score_pairs: (ids_flat int32, offsets int64 [n + 1], first_lens int32 [n]).
    encode_many(texts, max_tokens) -> id lists may replace tokenizer.encode (the C++ tokenizer)."""
    if len(questions) != len(passages):
        raise ValueError("build_pairs: as many questions as passages")
    enc = encode_many or (lambda texts, mt: [tokenizer.encode(t, mt) for t in texts])
    uniq = list(dict.fromkeys(questions))  # a question comes with many passages: tokenised once
    q_of = dict(zip(uniq, enc(uniq, max_query_tokens)))
    p_all = enc(list(passages), max_len - 1)  # more than any question leaves; cut per pair
    rows, first = [], np.empty(len(questions), np.int32)
    for i, (q, p) in enumerate(zip(questions, p_all)):
        ids, first[i] = stitch_pair(q_of[q], p, max_len)
        rows.append(ids)
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    flat = np.fromiter((t for r in rows for t in r), dtype=np.int32, count=int(offsets[-1]))
    return flat, offsets, first


def cut_pair_batches(encoder: Any, lens: Sequence[int], budget: int) -> "list[tuple[int, int]]":
    """Consecutive groups [a, b) of pairs of `lens` tokens for Encoder.score_pairs, each within `budget` token rows as
    Encoder.packed_rows (sc_encoder_packed_rows) counts them.  cut_packed bisects over the pairs it is given, and packed_rows refuses
    more rows than one call may have, so it is handed windows that cannot exceed that: 1 024 pairs of at most 512 tokens."""
    lens = np.asarray(lens, dtype=np.int64)
    window = 524288 // MAX_PAIR_TOKENS  # SC_ENCODER_PACKED_MAX_ROWS / the longest pair
    rows_of = lambda l: encoder.packed_rows(np.concatenate(([0], np.cumsum(l))))
    groups = []
    for start in range(0, len(lens), window):
        groups += [(start + a, start + b) for a, b in cut_packed(lens[start:start + window], budget, rows_of)]
    return groups


def scores_from_logits(logits: np.ndarray) -> np.ndarray:
    """One label: the logit.  Two labels: logit[1] - logit[0] (label 1 = relevant, the monoBERT convention)."""
    logits = np.asarray(logits, np.float32)
    if logits.ndim != 2 or logits.shape[1] not in (1, 2):
        raise ValueError(f"logits must be [n, 1] or [n, 2], not {logits.shape}")
    return logits[:, 0].copy() if logits.shape[1] == 1 else logits[:, 1] - logits[:, 0]


def load_reranker(path: "str | Path", cfg: Optional[dict] = None) -> "tuple[dict, np.ndarray, dict]":
    """`.safetensors` with BertForSequenceClassification names -> (encoder cfg read from the tensors, heads from the config.json beside
    the file if there is one, all updated by `cfg`; weight blob in ABI order; head = {cls_w, cls_b, pooler_w, pooler_b} with the pooler None when the file has none)."""
    path = Path(path)
    if path.suffix != ".safetensors":
        raise ValueError(f"unsupported reranker file {path} (use .safetensors with BertForSequenceClassification names)")
    from safetensors.numpy import load_file

    tensors = load_file(str(path))

    def get(name: str) -> "np.ndarray | None":
        for key in (name, "bert." + name):
            if key in tensors:
                return np.asarray(tensors[key], dtype=np.float32)
        return None

    if get("classifier.weight") is None or get("classifier.bias") is None:
        raise KeyError(f"{path}: classifier.weight / classifier.bias not found (not a sequence-classification checkpoint)")
    word = get("embeddings.word_embeddings.weight")
    if word is None:
        raise KeyError(f"{path}: tensor 'embeddings.word_embeddings.weight' not found")
    layers = 0
    while get(f"encoder.layer.{layers}.attention.self.query.weight") is not None:
        layers += 1
    hidden = int(word.shape[1])
    # the tensors do not say how wide a head is (MiniLM cross-encoders: 384 = 12 x 32): the config.json beside the file does
    heads = hidden // 64
    cfg_json = path.with_name("config.json")
    if cfg_json.is_file():
        n = json.loads(cfg_json.read_text()).get("num_attention_heads")
        if n is not None:
            heads = int(n)
    out = dict(vocab=int(word.shape[0]), hidden=hidden, layers=layers, heads=heads,
               ffn=tensors_rows(tensors, "encoder.layer.0.intermediate.dense.weight"), type_vocab=tensors_rows(tensors, "embeddings.token_type_embeddings.weight"),
               ln_eps=1e-12)
    pos = get("embeddings.position_embeddings.weight")
    if pos is not None:
        out["max_pos"] = int(pos.shape[0])
    out.update(cfg or {})
    if "max_pos" not in out:  # no position table: the file cannot say how long a sequence may be, nor which scheme replaces the table
        raise ValueError(f"{path} has no position_embeddings: pass cfg with max_pos and the position scheme (alibi=True or rotary=True) for such a model")
    blob = load_weight_blob(path, out["layers"], out)
    cls_w = get("classifier.weight").reshape(-1, hidden)
    head = dict(cls_w=cls_w, cls_b=get("classifier.bias").reshape(-1), pooler_w=get("pooler.dense.weight"), pooler_b=get("pooler.dense.bias"))
    if cls_w.shape[0] not in (1, 2):
        raise ValueError(f"{path}: classifier has {cls_w.shape[0]} labels; 1 or 2 are supported")
    return out, blob, head


class MI355XReranker:
    """score_pairs(questions, passages) / rerank(question, texts, top_k) with the forward and the head on the device."""

    def __init__(self, model: "str | Path | None" = None, *, vocab: "dict | str | Path | None" = None, cfg: Optional[dict] = None,
                 weights: "np.ndarray | None" = None, head: Optional[dict] = None, device: Optional[int] = None, runtime: Any = None,
                 max_query_tokens: int = 64, rows_budget: int = 65536) -> None:
        from .. import _native  # raises loudly when libsemcode_hip.so is missing: there is no CPU fallback

        settings = _resolve_settings()
        model = model if model is not None else getattr(settings, "mi355x_reranker_path", None)
        vocab = vocab if vocab is not None else (getattr(settings, "mi355x_reranker_vocab", None) or getattr(settings, "mi355x_vocab_path", None))
        if weights is None:
            if not model:
                raise ValueError("Set SEMCODE_MI355X_RERANKER_PATH (.safetensors of a BertForSequenceClassification model) to use the mi355x reranker.")
            full, weights, head = load_reranker(model, cfg)
        else:  # a blob and a head given directly (tests, benchmarks)
            if head is None or head.get("cls_w") is None:
                raise ValueError("weights given as an array need head = {cls_w, cls_b[, pooler_w, pooler_b]}")
            full = dict(_native.BERT_BASE)
            full.update(cfg or {})
        if vocab is None:
            raise ValueError("Set SEMCODE_MI355X_RERANKER_VOCAB (vocab.txt of the reranker) to use the mi355x reranker.")
        if full.get("type_vocab", 0) < 2:
            raise ValueError(f"a reranker needs two segment embeddings; this model has type_vocab = {full.get('type_vocab')}")
        self.model = str(model) if model else None
        self._cfg = full
        self.max_len, self.max_query_tokens = pair_limits(full["max_pos"], max_query_tokens)
        self.rows_budget = int(rows_budget)
        self._runtime = runtime or _native.shared_runtime(int(device if device is not None else getattr(settings, "mi355x_device", 0)))
        self._encoder = _native.Encoder(self._runtime, full, weights=weights)
        self._encoder.set_pair_head(head["cls_w"], head["cls_b"], head.get("pooler_w"), head.get("pooler_b"))
        self.num_labels = self._encoder.num_labels
        self.tokenizer = WordPieceTokenizer(vocab)
        self._fast_tokenizer = _native.NativeTokenizer(vocab) if isinstance(vocab, (str, Path)) else None

    def _encode_many(self, texts: Sequence[str], max_tokens: int) -> "List[List[int]]":
        return encode_many(self.tokenizer, self._fast_tokenizer, texts, max_tokens)

    def build_pairs(self, questions: Sequence[str], passages: Sequence[str]) -> "tuple[np.ndarray, np.ndarray, np.ndarray]":
        return build_pairs(self.tokenizer, questions, passages, self.max_len, self.max_query_tokens, encode_many=self._encode_many)

    def score_packed(self, ids_flat: np.ndarray, offsets: np.ndarray, first_lens: np.ndarray) -> np.ndarray:
        """Pairs already built -> scores [n]; consecutive packed batches within rows_budget token rows."""
        offsets = np.asarray(offsets, np.int64)
        lens = np.diff(offsets)
        out = np.empty(len(lens), np.float32)
        for a, b in cut_pair_batches(self._encoder, lens, self.rows_budget):
            logits = self._encoder.score_pairs(ids_flat[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a], first_lens[a:b])
            out[a:b] = scores_from_logits(logits)
        return out

    def score_pairs(self, questions: Sequence[str], passages: Sequence[str]) -> np.ndarray:
        """(question i, passage i) -> relevance scores [n] f32 (higher = more relevant)."""
        if len(questions) == 0:
            return np.empty(0, np.float32)
        return self.score_packed(*self.build_pairs(questions, passages))

    def rerank(self, question: str, texts: Sequence[str], top_k: Optional[int] = None) -> "tuple[np.ndarray, np.ndarray]":
        """(order, scores): indices into texts, best first (equal scores keep their order), and their scores; cut to top_k."""
        scores = self.score_pairs([question] * len(texts), list(texts))
        order = np.argsort(-scores, kind="stable")
        if top_k is not None:
            order = order[: max(0, int(top_k))]
        return order, scores[order]

    def close(self) -> None:
        self._encoder.close()
        if self._fast_tokenizer is not None:
            self._fast_tokenizer.close()
