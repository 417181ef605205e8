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

Rerankers of the other two encoder families come as a `transformers` DIRECTORY (`model.safetensors`, `config.json`, `tokenizer.json`) and
run through sc_encoder_set_score_head / sc_encoder_score_seqs (load_reranker_dir): one packed sequence per pair, no segment ids.
  ModernBertForSequenceClassification (gte-reranker-modernbert-base): `[CLS] question [SEP] passage [SEP]`; classifier = dense -> GELU ->
      LayerNorm -> linear over the [CLS] row or the masked mean (`classifier_pooling`).
  Qwen2ForSequenceClassification / Qwen3ForSequenceClassification (the `-seq-cls` conversions of Qwen3-Reranker): a bias-free `score`
      layer on the last token of the prompt.
  Qwen2ForCausalLM / Qwen3ForCausalLM (Qwen3-Reranker-0.6B, mxbai-rerank-*-v2): the score is the "yes" against the "no" logit of the
      last token -- a 2-label head whose rows are (false token, true token) of `lm_head.weight`, or of the embedding table when the two
      are tied; scores_from_logits gives logit_yes - logit_no, whose sigmoid is the model card's P(yes).
The prompt of the decoder rerankers is DATA (QWEN3_RERANKER_TEMPLATE, overridable by template= and instruction=): it is restated from the
published Qwen3-Reranker model card, because no released checkpoint exists offline -- parity for released checkpoints is unpinned, as for
the embedding models; what is pinned is the arithmetic, against transformers on seeded weights (scripts/gen_rerank_heads_fixtures.py).
Out of scope: sharing a question's prompt prefix across its pairs, XLM-R / SentencePiece rerankers, ModernBERT-large (ffn 2 624),
4B / 8B decoders, sharded checkpoints, GGUF.
"""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Any, List, Optional, Sequence

import numpy as np

from ..settings import resolve as _resolve_settings
from .providers import _modernbert_blob, _qwen2_blob, cut_packed, load_weight_blob, modernbert_config, qwen2_config, qwen3_config, tensors_rows
from .tokenizer import WordPieceTokenizer

log = logging.getLogger(__name__)

__all__ = ["MI355XReranker", "build_pairs", "cut_pair_batches", "encode_many", "scores_from_logits", "load_reranker", "pair_limits",
           "load_reranker_dir", "build_plain_pairs", "build_prompt_pairs", "stitch_prompt", "vocab_token_id", "QWEN3_RERANKER_TEMPLATE"]

MAX_PAIR_TOKENS = 512
MAX_SEQ_TOKENS = 2048  # what a packed text may have (sc_encoder_score_seqs)

# The prompt of Qwen3-Reranker, restated from its published model card: prefix + body + suffix, the body filled with the instruction, the
# query and the document and cut to the room the other two leave.  "instruction" is the card's default.
QWEN3_RERANKER_TEMPLATE = {
    "prefix": "<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct provided. "
              "Note that the answer can only be \"yes\" or \"no\".<|im_end|>\n<|im_start|>user\n",
    "body": "<Instruct>: {instruction}\n<Query>: {query}\n<Document>: {document}",
    "suffix": "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n",
    "instruction": "Given a web search query, retrieve relevant passages that answer the query",
}


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


def cut_pair_batches(encoder: Any, lens: Sequence[int], budget: int, max_len: int = MAX_PAIR_TOKENS) -> "list[tuple[int, int]]":
    """Consecutive groups [a, b) of pairs of `lens` tokens for Encoder.score_pairs / score_seqs, each within `budget` token rows as
    Encoder.packed_rows (sc_encoder_packed_rows) counts them.  cut_packed bisects over the pairs it is given, and packed_rows refuses
    more rows than one call may have, so it is handed windows that cannot exceed that: 1 024 pairs of at most 512 tokens (max_len)."""
    lens = np.asarray(lens, dtype=np.int64)
    window = max(1, 524288 // max(int(max_len), 32))  # SC_ENCODER_PACKED_MAX_ROWS / the longest pair
    rows_of = lambda l: encoder.packed_rows(np.concatenate(([0], np.cumsum(l))))
    groups = []
    for start in range(0, len(lens), window):
        groups += [(start + a, start + b) for a, b in cut_packed(lens[start:start + window], budget, rows_of)]
    return groups


def _flatten(rows: "list[list[int]]") -> "tuple[np.ndarray, np.ndarray]":
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return np.fromiter((t for r in rows for t in r), dtype=np.int32, count=int(offsets[-1])), offsets


def build_plain_pairs(tokenizer: Any, questions: Sequence[str], passages: Sequence[str], max_len: int = MAX_PAIR_TOKENS, max_query_tokens: int = 64,
                      encode_many: Any = None) -> "tuple[np.ndarray, np.ndarray]":
    """(question i, passage i) -> packed input of Encoder.score_seqs for a ModernBERT reranker: (ids_flat int32, offsets int64 [n + 1]).
    `[CLS] question [SEP] passage [SEP]` from the tokenizer's own single-text encodings, stitched and cut as stitch_pair does (the passage
    is cut, the question keeps its budget, an empty passage leaves the question alone); the family has no segment ids."""
    flat, offsets, _ = build_pairs(tokenizer, questions, passages, max_len, max_query_tokens, encode_many)
    return flat, offsets


def stitch_prompt(prefix_ids: Sequence[int], body_ids: Sequence[int], suffix_ids: Sequence[int], max_len: int) -> "list[int]":
    """prefix + body[: max_len - len(prefix) - len(suffix)] + suffix: the model card's own order of operations -- the body (instruction,
    query and document, tokenised as one text) is cut to the room, prefix and suffix stay whole."""
    room = int(max_len) - len(prefix_ids) - len(suffix_ids)
    if room < 1:
        raise ValueError(f"prefix ({len(prefix_ids)} tokens) and suffix ({len(suffix_ids)}) leave no room in {max_len}")
    return list(prefix_ids) + list(body_ids[:room]) + list(suffix_ids)


def build_prompt_pairs(encode: Any, questions: Sequence[str], passages: Sequence[str], max_len: int = MAX_PAIR_TOKENS, template: Optional[dict] = None,
                       instruction: Optional[str] = None) -> "tuple[np.ndarray, np.ndarray]":
    """(question i, passage i) -> packed input of Encoder.score_seqs for a decoder reranker (causal LM or seq-cls): (ids_flat, offsets).
    encode(text) -> ids WITHOUT special tokens added (the template spells its own).  template: {prefix, body, suffix[, instruction]},
    QWEN3_RERANKER_TEMPLATE by default; body is formatted with instruction, query and document."""
    if len(questions) != len(passages):
        raise ValueError("build_prompt_pairs: as many questions as passages")
    t = dict(QWEN3_RERANKER_TEMPLATE, **(template or {}))
    instruction = instruction if instruction else t["instruction"]
    prefix, suffix = list(encode(t["prefix"])), list(encode(t["suffix"]))
    return _flatten([stitch_prompt(prefix, encode(t["body"].format(instruction=instruction, query=q, document=p)), suffix, max_len)
                     for q, p in zip(questions, passages)])


def scores_from_logits(logits: np.ndarray) -> np.ndarray:
    """One label: the logit.  Two labels: logit[1] - logit[0] (label 1 = relevant, the monoBERT convention; the heads of causal LMs
    are built as (false token, true token), so this is logit_yes - logit_no)."""
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


def vocab_token_id(tokenizer_json: "str | Path | dict", token: str) -> int:
    """The id of `token` when it is ONE entry of the vocabulary of a `tokenizer.json` (model.vocab or added_tokens); an error naming it
    otherwise: a score read from the first piece of a multi-piece word would be another word's."""
    if not isinstance(tokenizer_json, dict):
        tokenizer_json = json.loads(Path(tokenizer_json).read_text(encoding="utf-8"))
    vocab = (tokenizer_json.get("model") or {}).get("vocab") or {}
    if isinstance(vocab, list):  # Unigram: [[piece, score], ...]
        vocab = {piece[0]: i for i, piece in enumerate(vocab)}
    if token in vocab:
        return int(vocab[token])
    for added in tokenizer_json.get("added_tokens") or ():
        if added.get("content") == token:
            return int(added["id"])
    raise ValueError(f"token {token!r} is not a single entry of the tokenizer's vocabulary (a score token must be one piece)")


SCORE_ARCHITECTURES = ("ModernBertForSequenceClassification", "Qwen2ForSequenceClassification", "Qwen3ForSequenceClassification", "Qwen2ForCausalLM",
                       "Qwen3ForCausalLM")


def load_reranker_dir(path: "str | Path", cfg: Optional[dict] = None, true_token: Optional[str] = None,
                      false_token: Optional[str] = None) -> "tuple[dict, np.ndarray, dict, str]":
    """A `transformers` directory (model.safetensors, config.json, tokenizer.json) -> (encoder cfg updated by `cfg`, weight blob in ABI
    order, score head as Encoder.set_score_head takes it, architecture name).  Dispatch on config.json's `architectures` (one of
    SCORE_ARCHITECTURES), `model_type` without it (modernbert: sequence classification; qwen2 / qwen3: sequence classification when the
    file has `score.weight`, else causal LM).  true_token / false_token ("yes" / "no"): the vocabulary rows of a causal LM's head."""
    path = Path(path)
    conf, weights = path / "config.json", path / "model.safetensors"
    if not conf.is_file() or not weights.is_file():
        raise FileNotFoundError(f"{path}: a reranker directory needs config.json and model.safetensors")
    from safetensors.numpy import load_file

    c = json.loads(conf.read_text())
    tensors = load_file(str(weights))
    f32 = lambda name: np.asarray(tensors[name], dtype=np.float32) if name in tensors else None  # noqa: E731

    def need(name: str) -> np.ndarray:
        t = f32(name)
        if t is None:
            raise KeyError(f"{weights}: tensor {name!r} not found")
        return t

    archs = c.get("architectures") or []
    arch = next((a for a in archs if a in SCORE_ARCHITECTURES), None)
    if arch is None:
        if archs:
            raise ValueError(f"{conf}: architectures {archs} hold none of {list(SCORE_ARCHITECTURES)}")
        mt = c.get("model_type")
        if mt == "modernbert":
            arch = "ModernBertForSequenceClassification"
        elif mt in ("qwen2", "qwen3"):
            arch = ("Qwen2" if mt == "qwen2" else "Qwen3") + ("ForSequenceClassification" if "score.weight" in tensors else "ForCausalLM")
        else:
            raise ValueError(f"{conf}: model_type {mt!r} is not a supported reranker (modernbert, qwen2, qwen3)")
    if arch.startswith("ModernBert"):
        act = c.get("classifier_activation", "gelu")
        if act != "gelu":
            raise ValueError(f"{conf}: classifier_activation {act!r} is not supported (gelu only)")
        pooling = c.get("classifier_pooling", "cls")
        if pooling not in ("cls", "mean"):
            raise ValueError(f"{conf}: classifier_pooling {pooling!r} is not supported (cls or mean)")
        full = modernbert_config(c)
        full.update(cfg or {})
        blob = _modernbert_blob(weights, tensors, full["layers"])
        H = full["hidden"]
        head = dict(kind=1, pooling=pooling, norm_eps=float(c.get("norm_eps", 1e-5)), dense_w=need("head.dense.weight"), dense_b=f32("head.dense.bias"),
                    norm_g=need("head.norm.weight"), norm_b=f32("head.norm.bias"), cls_w=need("classifier.weight").reshape(-1, H), cls_b=need("classifier.bias"))
    else:
        full = qwen3_config(c) if arch.startswith("Qwen3") else qwen2_config(c)
        full.update(cfg or {})
        blob = _qwen2_blob(weights, tensors, full["layers"], full)
        H = full["hidden"]
        if arch.endswith("ForSequenceClassification"):
            cls_w = need("score.weight").reshape(-1, H)
        else:
            tok = path / "tokenizer.json"
            if not tok.is_file():
                raise FileNotFoundError(f"{path}: a causal-LM reranker needs tokenizer.json to find its score tokens")
            tj = json.loads(tok.read_text(encoding="utf-8"))
            rows = [vocab_token_id(tj, false_token or "no"), vocab_token_id(tj, true_token or "yes")]  # (false, true): score = logit[1] - logit[0]
            table = f32("lm_head.weight")
            if table is None:  # tied embeddings: the file keeps one copy
                table = need("model.embed_tokens.weight") if "model.embed_tokens.weight" in tensors else need("embed_tokens.weight")
            if max(rows) >= table.shape[0]:
                raise ValueError(f"{path}: score token ids {rows} lie outside the {table.shape[0]} rows of the vocabulary projection")
            cls_w = np.ascontiguousarray(table[rows])
        head = dict(kind=2, pooling="last", cls_w=cls_w, cls_b=None)
    if head["cls_w"].shape[0] not in (1, 2):
        raise ValueError(f"{path}: classifier has {head['cls_w'].shape[0]} labels; 1 or 2 are supported")
    return full, blob, head, arch


class MI355XReranker:
    """score_pairs(questions, passages) / rerank(question, texts, top_k) with the forward and the head on the device.

    model: a `.safetensors` file of a BertForSequenceClassification cross-encoder (with vocab=), or a `transformers` directory of a
    ModernBERT or Qwen2 / Qwen3 reranker (load_reranker_dir; its tokenizer.json is used).  max_pair_tokens bounds a pair: 512 by default,
    up to 2 048 for the directory models (BERT cross-encoders stay at min(max_pos, 512)).  instruction / template / true_token /
    false_token: the prompt and the score tokens of a decoder reranker (defaults: settings, then QWEN3_RERANKER_TEMPLATE and "yes" / "no")."""

    def __init__(self, model: "str | Path | None" = None, *, vocab: "dict | str | Path | None" = None, cfg: Optional[dict] = None,
                 weights: "np.ndarray | None" = None, head: Optional[dict] = None, device: Optional[int] = None, runtime: Any = None,
                 max_query_tokens: int = 64, rows_budget: int = 65536, max_pair_tokens: int = MAX_PAIR_TOKENS, tokenizer: Any = None,
                 instruction: Optional[str] = None, template: Optional[dict] = None, true_token: Optional[str] = None,
                 false_token: Optional[str] = None) -> None:
        from .. import _native  # raises loudly when libsemcode_hip.so is missing: there is no CPU fallback

        settings = _resolve_settings()
        model = model if model is not None else getattr(settings, "mi355x_reranker_path", None)
        if not 4 <= int(max_pair_tokens) <= MAX_SEQ_TOKENS:
            raise ValueError(f"max_pair_tokens must lie in 4 .. {MAX_SEQ_TOKENS}, got {max_pair_tokens}")
        self.rows_budget = int(rows_budget)
        self.model = str(model) if model else None
        self._fast_tokenizer = None
        self.family = "bert"
        if (weights is None and model and Path(model).is_dir()) or (head is not None and head.get("kind")):
            # ---- a ModernBERT or Qwen2 / Qwen3 reranker: one packed sequence per pair through the score head
            if weights is None:
                full, weights, head, arch = load_reranker_dir(model, cfg, true_token or getattr(settings, "mi355x_reranker_true_token", None),
                                                              false_token or getattr(settings, "mi355x_reranker_false_token", None))
                if tokenizer is None:
                    from .tokenizer import HFTokenizer

                    tokenizer = HFTokenizer(Path(model) / "tokenizer.json")
            else:  # a blob and a score head given directly (tests, benchmarks)
                if cfg is None or tokenizer is None:
                    raise ValueError("weights given as an array with a score head need cfg and tokenizer")
                full = dict(cfg)
            self.family = "modernbert" if head["kind"] == 1 else "causal"
            self._cfg = full
            self.max_len = min(int(full["max_pos"]), int(max_pair_tokens))
            self.max_query_tokens = max(2, min(int(max_query_tokens), self.max_len - 2))
            self.instruction = instruction or getattr(settings, "mi355x_reranker_instruction", None) or None
            self.template = template
            self.tokenizer = tokenizer
            self._runtime = runtime or _native.shared_runtime(int(device if device is not None else getattr(settings, "mi355x_device", 0)))
            self._encoder = _native.Encoder(self._runtime, full, weights=weights)
            self._encoder.set_score_head(head)
            self.num_labels = self._encoder.score_labels
            return
        vocab = vocab if vocab is not None else (getattr(settings, "mi355x_reranker_vocab", None) or getattr(settings, "mi355x_vocab_path", None))
        if weights is None:
            if not model:
                raise ValueError("Set SEMCODE_MI355X_RERANKER_PATH (.safetensors of a BertForSequenceClassification model, or a transformers "
                                 "directory of a ModernBERT / Qwen2 / Qwen3 reranker) to use the mi355x reranker.")
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
        self._cfg = full
        self.max_len, self.max_query_tokens = pair_limits(full["max_pos"], max_query_tokens)
        self._runtime = runtime or _native.shared_runtime(int(device if device is not None else getattr(settings, "mi355x_device", 0)))
        self._encoder = _native.Encoder(self._runtime, full, weights=weights)
        self._encoder.set_pair_head(head["cls_w"], head["cls_b"], head.get("pooler_w"), head.get("pooler_b"))
        self.num_labels = self._encoder.num_labels
        self.tokenizer = WordPieceTokenizer(vocab)
        self._fast_tokenizer = _native.NativeTokenizer(vocab) if isinstance(vocab, (str, Path)) else None

    def _encode_many(self, texts: Sequence[str], max_tokens: int) -> "List[List[int]]":
        return encode_many(self.tokenizer, self._fast_tokenizer, texts, max_tokens)

    def _encode_plain(self, text: str) -> "List[int]":
        """ids of a prompt piece, no special tokens added: the template spells its own"""
        raw = getattr(self.tokenizer, "encode_plain", None)
        if raw is not None:
            return list(raw(text))
        raise TypeError("the tokenizer of a decoder reranker needs encode_plain(text) -> ids (no special tokens)")

    def build_pairs(self, questions: Sequence[str], passages: Sequence[str]):
        """BERT cross-encoders: (ids_flat, offsets, first_lens); the directory models: (ids_flat, offsets)."""
        if self.family == "modernbert":
            return build_plain_pairs(self.tokenizer, questions, passages, self.max_len, self.max_query_tokens)
        if self.family == "causal":
            return build_prompt_pairs(self._encode_plain, questions, passages, self.max_len, self.template, self.instruction)
        return build_pairs(self.tokenizer, questions, passages, self.max_len, self.max_query_tokens, encode_many=self._encode_many)

    def score_packed(self, ids_flat: np.ndarray, offsets: np.ndarray, first_lens: "np.ndarray | None" = None) -> np.ndarray:
        """Pairs already built -> scores [n]; consecutive packed batches within rows_budget token rows."""
        offsets = np.asarray(offsets, np.int64)
        lens = np.diff(offsets)
        out = np.empty(len(lens), np.float32)
        for a, b in cut_pair_batches(self._encoder, lens, self.rows_budget, self.max_len):
            ids, off = ids_flat[offsets[a]:offsets[b]], offsets[a:b + 1] - offsets[a]
            logits = self._encoder.score_seqs(ids, off) if self.family != "bert" else self._encoder.score_pairs(ids, off, first_lens[a:b])
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
