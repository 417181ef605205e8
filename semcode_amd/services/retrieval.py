"""The retrieval half of SemanticSearchPipeline, restated for the MI355X backend.

Reference: src/semcode/rag/pipeline.py:93-175 (`_retrieve_documents`, `_hit_to_document`, `_embed_query`) -- the one
consumer of `MilvusVectorStore.search`'s result shape.  The reference's pipeline runs unchanged
on the two seams; this module exists so that the same behaviour -- lazy connect, top_k from `rag_max_context_sources`, what
counts as "no results", the document mapping and the score attribute order -- can be used and tested without the LLM half of
that class (answer synthesis, prompts: out of scope), and so that MANY questions can be answered by ONE encoder batch and ONE
batched search (`retrieve_batch`), which is how this backend is meant to be driven.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..settings import resolve as _resolve_settings

log = logging.getLogger(__name__)

_SCORE_ATTRS = ("score", "distance", "similarity")  # pipeline.py:149-155: the first attribute the hit HAS decides


def embed_query(embedding_client: Any, question: str) -> List[float]:
    """pipeline.py:171-175: embed_query when the client has one, else the first row of embed_documents([question])."""
    if hasattr(embedding_client, "embed_query"):
        return embedding_client.embed_query(question)
    return embedding_client.embed_documents([question])[0]


def hit_to_document(hit: Any) -> Optional[Dict[str, Any]]:
    """pipeline.py:131-169: one search hit -> {repo, path, language, snippet, score, metadata}; None for a hit without entity."""
    entity = getattr(hit, "entity", None)
    fetch = getattr(entity, "get", None)
    if entity is None or fetch is None:
        return None
    try:
        repo, path, language = fetch("repo"), fetch("path"), fetch("language")
        snippet = fetch("text")
        metadata = fetch("metadata") or {}
    except Exception:  # an entity with another schema: an empty document, as the reference returns
        repo = path = language = None
        snippet, metadata = "", {}
    score = 0.0
    for attr in _SCORE_ATTRS:
        if hasattr(hit, attr):
            try:
                score = float(getattr(hit, attr))
            except Exception:
                score = 0.0
            break
    return {"repo": repo, "path": path, "language": language, "snippet": snippet or "", "score": score, "metadata": metadata}


def _top_k() -> int:
    return max(1, int(getattr(_resolve_settings(), "rag_max_context_sources", 5)))


def _rerank_fetch_k(fetch_k: Optional[int], top_k: int) -> int:
    """Hits the store is asked for when a reranker re-orders them: fetch_k or settings.mi355x_rerank_fetch_k, at least top_k."""
    k = fetch_k if fetch_k is not None else getattr(_resolve_settings(), "mi355x_rerank_fetch_k", 40)
    return max(int(k), top_k)


def _apply_scores(documents: List[Dict[str, Any]], scores: Any, top_k: int) -> List[Dict[str, Any]]:
    """Documents in retrieval order + one reranker score each -> the top_k by score, ties by retrieval rank; `score` becomes the
    reranker's, `retrieval_score` keeps the store's."""
    order = sorted(range(len(documents)), key=lambda i: (-float(scores[i]), i))[:top_k]
    return [dict(documents[i], retrieval_score=documents[i]["score"], score=float(scores[i])) for i in order]


class Retriever:
    """question -> documents, with the reference's error protocol: every failure yields [] and is kept in `last_error`
    (`_last_retrieval_error` there); a successful retrieval clears it.  reranker (optional): an object with
    score_pairs(questions, passages) -> scores (embeddings.reranker.MI355XReranker), used by calls that pass rerank=True."""

    def __init__(self, embedding_client: Any, vector_store: Any, reranker: Any = None) -> None:
        self.embedding_client = embedding_client
        self.vector_store = vector_store
        self.reranker = reranker
        self.last_error: Optional[BaseException] = None
        self._connected = False

    def _ensure_connected(self) -> bool:
        if self._connected:
            return True
        try:
            self.vector_store.connect()
        except Exception as exc:
            log.error("milvus_connection_failed error=%s", exc)
            self.last_error = exc
            return False
        self._connected = True
        return True

    @staticmethod
    def _filter_kwargs(repos: Any, languages: Any, group_by: Any = None, mmr: Any = None, fetch_k: Any = None, hybrid: Any = None, **text: Any) -> Dict[str, Any]:
        # only what was given: a call without a filter reaches the store exactly as before (any store with the reference's surface);
        # text = query_text / query_texts, the question(s) themselves, handed on only with hybrid
        given = (("repos", repos), ("languages", languages), ("group_by", group_by), ("mmr", mmr), ("fetch_k", fetch_k))
        out = {name: value for name, value in given if value is not None}
        if hybrid is not None and hybrid is not False:
            out.update(hybrid=hybrid, **text)
        return out

    def _check_rerank(self, rerank: Any, mmr: Any) -> bool:
        """Argument errors of rerank=, raised before anything runs."""
        if not rerank:
            return False
        if mmr is not None:
            raise ValueError("rerank together with mmr is not supported: pick one way of re-ordering the candidates")
        if self.reranker is None:
            raise ValueError("rerank=True needs a reranker: Retriever(embedding_client, vector_store, reranker=...)")
        return True

    def _check_late(self, late: Any, rerank: Any, group_by: Any, mmr: Any, hybrid: Any) -> bool:
        """Argument errors of late=, raised before anything runs."""
        if not late:
            return False
        for name, value in (("mmr", mmr), ("group_by", group_by), ("hybrid", hybrid if hybrid is not False else None), ("rerank", rerank or None)):
            if value is not None:
                raise ValueError(f"late together with {name} is not supported: the MaxSim search is the whole retrieval")
        if self.reranker is None or not hasattr(self.reranker, "embed_query_tokens"):
            raise ValueError("late=True needs a late-interaction reranker: Retriever(embedding_client, vector_store, reranker=MI355XLateReranker(...))")
        if not hasattr(self.vector_store, "search_late"):
            raise ValueError(f"late=True needs a store with search_late: {type(self.vector_store).__name__} has none")
        return True

    def _retrieve_late(self, questions: Sequence[str], repos: Any, languages: Any) -> List[List[Dict[str, Any]]]:
        """The MaxSim search as the first stage: the questions' forward, then one exhaustive search over the stored token vectors."""
        if not self._ensure_connected():
            return [[] for _ in questions]
        try:
            dist, rows = self.vector_store.search_late(self.reranker.embed_query_tokens(list(questions)), _top_k(), **self._filter_kwargs(repos, languages))
            results = self.vector_store.hits_for(dist, rows)
        except Exception as exc:
            log.error("late_search_failed error=%s", exc)
            self.last_error = exc
            return [[] for _ in questions]
        self.last_error = None if results else ValueError("no_results")
        return [[doc for doc in (hit_to_document(hit) for hit in hits) if doc] for hits in results]

    def _rerank_from_store(self, questions: Sequence[str], per_question: List[List[Dict[str, Any]]], rows: List[List[Any]],
                           top_k: int) -> Optional[List[List[Dict[str, Any]]]]:
        """The stored token vectors score the candidates when the reranker is a late-interaction one and the store holds tokens for
        EVERY candidate row: the questions' forward only.  None: not possible here, score_pairs does it."""
        store, rr = self.vector_store, self.reranker
        if not (hasattr(rr, "embed_query_tokens") and hasattr(store, "rerank_late") and hasattr(store, "has_late_tokens")):
            return None
        flat = [r for rs in rows for r in rs]
        if not flat or any(r is None for r in flat) or not store.has_late_tokens(flat):
            return None
        width = max(len(rs) for rs in rows)
        cand = np.full((len(rows), width), -1, dtype=np.int64)
        for i, rs in enumerate(rows):
            cand[i, :len(rs)] = rs
        scores = store.rerank_late(rr.embed_query_tokens(list(questions)), cand)
        return [_apply_scores(docs, scores[i, :len(docs)], top_k) for i, docs in enumerate(per_question)]

    def _rerank(self, questions: Sequence[str], per_question: List[List[Dict[str, Any]]], top_k: int,
                rows: Optional[List[List[Any]]] = None) -> List[List[Dict[str, Any]]]:
        """All (question, snippet) pairs of all questions in one score_pairs call (shared packed batches), then _apply_scores each.
        rows (the candidates' row numbers, one per document): tried first against the store's token vectors (_rerank_from_store)."""
        if rows is not None:
            done = self._rerank_from_store(questions, per_question, rows, top_k)
            if done is not None:
                return done
        qs = [q for q, docs in zip(questions, per_question) for _ in docs]
        ps = [doc["snippet"] for docs in per_question for doc in docs]
        scores = self.reranker.score_pairs(qs, ps) if qs else []
        out, at = [], 0
        for docs in per_question:
            out.append(_apply_scores(docs, scores[at:at + len(docs)], top_k))
            at += len(docs)
        return out

    def retrieve(self, question: str, *, repos: Any = None, languages: Any = None, group_by: Optional[str] = None,
                 mmr: Optional[float] = None, fetch_k: Optional[int] = None, hybrid: Any = None, rerank: Any = None, late: Any = None) -> List[Dict[str, Any]]:
        """pipeline.py:93-129, one question.  repos / languages restrict the search itself (MilvusVectorStore.search), where the
        reference front ends drop hits from an unfiltered top-k afterwards.  group_by ("path" | "repo"): at most one document per
        file / per repo, so rag_max_context_sources buys that many different sources.  mmr (in [0, 1]) / fetch_k: maximal marginal
        relevance over the best fetch_k chunks, so near-identical chunks under different paths do not take every slot.  hybrid (True
        or {c, dense_weight, lexical_weight}): the question text goes along and its BM25 hits over the chunks' code terms are fused
        with the dense ones, so a question that names an identifier finds the chunk that defines it.  rerank=True: the store is asked
        for fetch_k hits (default settings.mi355x_rerank_fetch_k, at least top_k; filters, group_by and hybrid apply to that search), the
        reranker scores every (question, snippet) pair, and the top_k by that score come back -- ties by retrieval rank, `score` the
        reranker's, `retrieval_score` the store's.  Not together with mmr (ValueError); a reranker failure yields [] and last_error.
        With a late-interaction reranker and a store that keeps token vectors for every candidate row (MilvusVectorStore(late=...)) the
        scores come from the stored vectors -- the question's forward only, the same bits as score_pairs; otherwise score_pairs runs.
        late=True: the exact MaxSim search over the stored token vectors IS the retrieval (the question's token vectors, no dense
        search); repos / languages apply; with mmr, group_by, hybrid or rerank it raises ValueError before anything runs."""
        if self._check_late(late, rerank, group_by, mmr, hybrid):
            return self._retrieve_late([question], repos, languages)[0]
        reranking = self._check_rerank(rerank, mmr)
        if not self._ensure_connected():
            return []
        vector = embed_query(self.embedding_client, question)
        top_k = _top_k()
        ask_k, store_fetch_k = (_rerank_fetch_k(fetch_k, top_k), None) if reranking else (top_k, fetch_k)
        try:
            results = self.vector_store.search(vector, top_k=ask_k, **self._filter_kwargs(repos, languages, group_by, mmr, store_fetch_k, hybrid, query_text=question))
        except Exception as exc:
            log.error("milvus_search_failed error=%s", exc)
            self.last_error = exc
            return []
        if not results:
            self.last_error = ValueError("no_results")
            return []
        try:
            hits = next(iter(results))
        except StopIteration:
            self.last_error = ValueError("no_results")
            return []
        except TypeError:  # not iterable: taken as the hits themselves, as the reference does
            hits = results
        pairs = [(doc, getattr(hit, "row", None)) for hit, doc in ((hit, hit_to_document(hit)) for hit in hits) if doc]
        documents = [doc for doc, _ in pairs]
        if reranking:
            try:
                documents = self._rerank([question], [documents], top_k, rows=[[row for _, row in pairs]])[0]
            except Exception as exc:
                log.error("rerank_failed error=%s", exc)
                self.last_error = exc
                return []
        self.last_error = None
        return documents

    def retrieve_batch(self, questions: Sequence[str], *, repos: Any = None, languages: Any = None, group_by: Optional[str] = None,
                       mmr: Optional[float] = None, fetch_k: Optional[int] = None, hybrid: Any = None, rerank: Any = None,
                       late: Any = None) -> List[List[Dict[str, Any]]]:
        """Many questions at once: one encoder batch (`embed_documents_array`) and one batched search (`search_batch`) when the
        seams offer them, else `retrieve` per question.  Per question the result is what `retrieve` returns for it (a store
        that returns no hit for a question yields [] for that question).  repos / languages / group_by / mmr / fetch_k / hybrid: one setting
        for the whole batch, as in `retrieve`.  rerank=True: as in `retrieve`, with the pairs of ALL questions scored in shared
        packed batches (or, as in `retrieve`, from the store's token vectors).  late=True: as in `retrieve`, one search for all."""
        questions = list(questions)
        if self._check_late(late, rerank, group_by, mmr, hybrid):
            return self._retrieve_late(questions, repos, languages) if questions else []
        reranking = self._check_rerank(rerank, mmr)
        if not questions:
            return []
        fast = hasattr(self.embedding_client, "embed_documents_array") and hasattr(self.vector_store, "search_batch") and hasattr(self.vector_store, "hits_for")
        if not fast:
            if reranking:
                return [self.retrieve(q, repos=repos, languages=languages, group_by=group_by, fetch_k=fetch_k, hybrid=hybrid, rerank=True) for q in questions]
            return [self.retrieve(q, repos=repos, languages=languages, group_by=group_by, mmr=mmr, fetch_k=fetch_k, hybrid=hybrid) for q in questions]
        if not self._ensure_connected():
            return [[] for _ in questions]
        top_k = _top_k()
        ask_k, store_fetch_k = (_rerank_fetch_k(fetch_k, top_k), None) if reranking else (top_k, fetch_k)
        try:
            vectors = np.asarray(self.embedding_client.embed_documents_array(questions), dtype=np.float32)
            dist, rows = self.vector_store.search_batch(vectors, top_k=ask_k, **self._filter_kwargs(repos, languages, group_by, mmr, store_fetch_k, hybrid, query_texts=questions))
            results = self.vector_store.hits_for(dist, rows)
        except Exception as exc:
            log.error("milvus_search_failed error=%s", exc)
            self.last_error = exc
            return [[] for _ in questions]
        pairs = [[(doc, getattr(hit, "row", None)) for hit, doc in ((hit, hit_to_document(hit)) for hit in hits) if doc] for hits in results]
        out = [[doc for doc, _ in ps] for ps in pairs]
        if reranking:
            try:
                out = self._rerank(questions, out, top_k, rows=[[row for _, row in ps] for ps in pairs])
            except Exception as exc:
                log.error("rerank_failed error=%s", exc)
                self.last_error = exc
                return [[] for _ in questions]
        # as retrieve() (pipeline.py:112-122): "no_results" only when the store's result container itself is falsy; a
        # non-empty container whose hit lists hold nothing usable clears the error
        self.last_error = None if results else ValueError("no_results")
        return out
