"""MilvusVectorStore drop-in backed by the HBM-resident index of libsemcode_hip.

Reference: src/semcode/storage/milvus_store.py:29-148.  Same constructor, attributes, methods,
progress protocol and error behaviour, so IndexerService (src/semcode/services/indexer.py:54-63,
108) and SemanticSearchPipeline (src/semcode/rag/pipeline.py:93-169) run on it unchanged:

    MilvusVectorStore(collection_name="semcode_chunks", dim=None)
    .connect()                                  -> opens the device runtime + index (was: gRPC connect,
                                                   create collection + IVF_FLAT/IP index, load)
    .upsert_embeddings(payloads, progress=None) -> replace-by-primary-key, batches of
                                                   settings.milvus_upsert_batch_size
    .search(vector, top_k=10)                   -> iterable of Hits; hit.entity.get(field), hit.distance,
                                                   hit.score, hit.id  (pymilvus SearchResult shape)
    .search(..., repos=[..], languages=[..])    -> Collection.search(expr=...): only rows of these repos AND languages, exact
    .search(..., group_by="path" | "repo")      -> Collection.search(group_by_field=...): at most one hit per file / per repo, exact
    .search(..., mmr=0.5, fetch_k=40)           -> search_type="mmr" (lambda_mult, fetch_k) of the LangChain stores: diversified top_k, exact, on device
    .search(..., query_text=q, hybrid=True)     -> Collection.hybrid_search(..., RRFRanker()): dense top-fetch_k fused with a BM25 top-fetch_k over
                                                   hashed code terms, on device (needs MilvusVectorStore(lexical=True))
    .delete(ids) / .delete_where(repo=, path=, language=)
                                                -> Collection.delete(expr): rows removed, survivors renumbered densely
    MilvusVectorStore(late=reranker, late_format="f32" | "bf16")
                                                -> a multi-vector collection: every chunk's late-interaction token vectors are kept on the
                                                   device next to its row at upsert (written there by the reranker's own token head when
                                                   both share a runtime; late_handover=False: through the host); .rerank_late(question_vectors, rows) scores candidates
                                                   from them without a passage forward, .search_late(question_vectors, top_k) is the exact
                                                   MaxSim search over them

What lives where: vectors and their norms in HBM (sc_index); the scalar columns of the reference
schema (id, repo, path, language, text, metadata; milvus_store.py:59-74) and the md5 -> row map in
this object.  Additions that do not break the reference surface: search_batch(), metric/index options.
"""
from __future__ import annotations

import json
import logging
import shutil
import threading
from pathlib import Path
from typing import Any, Callable, Iterator, List, Optional, Sequence

import numpy as np

from .._native import pack_allow  # (numpy only: the library itself is loaded on first use, not on import)
from ..embeddings.payload import EmbeddingPayload
from ..settings import resolve as _resolve_settings

log = logging.getLogger(__name__)

OUTPUT_FIELDS = ("repo", "path", "language", "text", "metadata")  # milvus_store.py:146


class _Entity:
    """pymilvus Hit.entity look-alike: .get(name) over the stored scalar columns."""

    __slots__ = ("_fields",)

    def __init__(self, fields: dict) -> None:
        self._fields = fields

    def get(self, name: str, default: Any = None) -> Any:
        return self._fields.get(name, default)

    def to_dict(self) -> dict:
        return dict(self._fields)


class Hit:
    """One search hit: .id (primary key), .distance == .score (metric value), .entity.get(field).

    .row is the row number at the time of the search: a later delete() / delete_where() renumbers the rows behind the deleted
    ones, so the .row of a hit obtained before it is stale afterwards (.id stays valid for as long as the key is stored)."""

    __slots__ = ("id", "distance", "entity", "row")

    def __init__(self, pk: str, distance: float, fields: dict, row: int) -> None:
        self.id = pk
        self.distance = float(distance)
        self.entity = _Entity(fields)
        self.row = row

    @property
    def score(self) -> float:
        return self.distance

    def __repr__(self) -> str:  # pragma: no cover
        return f"Hit(id={self.id!r}, distance={self.distance:.6g})"


class Hits(list):
    """Per-query hit list, best first (pymilvus Hits)."""

    @property
    def ids(self) -> list:
        return [h.id for h in self]

    @property
    def distances(self) -> list:
        return [h.distance for h in self]


class SearchResult(list):
    """List of Hits, one per query; `next(iter(result))` is what pipeline.py:117-118 does."""


class MilvusVectorStore:
    """Thin wrapper with the reference's surface, storing vectors on the MI355X."""

    RETRAIN_GROWTH = 2.0  # re-run k-means when the collection has this many times the rows its centroids were trained on

    def __init__(self, collection_name: str = "semcode_chunks", dim: Optional[int] = None, *, metric: Optional[str] = None,
                 index_type: Optional[str] = None, nlist: Optional[int] = None, nprobe: Optional[int] = None,
                 device: Optional[int] = None, runtime: Any = None, index_factory: Optional[Callable[..., Any]] = None,
                 lexical: Optional[bool] = None, lex_slots: int = 128, late: Any = None, late_format: Optional[str] = None,
                 late_handover: Optional[bool] = None) -> None:
        settings = _resolve_settings()
        self.collection_name = collection_name
        self.dim = dim or settings.embedding_dimension
        self._collection: Any = None  # the device index once connected (name kept from the reference)
        self.metric = (metric or getattr(settings, "mi355x_metric", "IP")).upper()
        self.index_type = (index_type or getattr(settings, "mi355x_index_type", "IVF_FLAT")).upper()
        self.nlist = int(nlist or getattr(settings, "mi355x_nlist", 128))
        self.nprobe = int(nprobe or getattr(settings, "mi355x_nprobe", 16))
        self._device = int(device if device is not None else getattr(settings, "mi355x_device", 0))
        self._runtime = runtime
        self._owns_runtime = runtime is None
        self._index_factory = index_factory
        self._lock = threading.RLock()
        # scalar columns, indexed by row (milvus_store.py:59-74)
        self._ids: List[str] = []
        self._texts: List[str] = []
        self._metadata: List[dict] = []
        self._repos: List[str] = []
        self._paths: List[str] = []
        self._languages: List[str] = []
        self._row_of: dict[str, int] = {}
        # filtered search: an integer code per row for repo and language (the device only sees row numbers: a filter becomes a bitset
        # over rows, built with np.isin over these instead of a Python loop over the strings) and the packed bitsets built so far
        self._repo_code: dict[str, int] = {}
        self._lang_code: dict[str, int] = {}
        self._repo_codes = np.zeros(0, dtype=np.int32)  # capacity >= len(self._ids); entries beyond it are unused
        self._lang_codes = np.zeros(0, dtype=np.int32)
        self._mask_cache: dict = {}  # (frozenset(repos) | None, frozenset(languages) | None) -> (words, every row passes); dropped on every mutation
        # grouped search: an integer code per row for the pair (repo, path) -- group_by="repo" reuses _repo_codes -- handed to the
        # device index as opaque labels before a grouped search; _groups_installed names the column the index holds labels of for
        # the rows as they are (None: none, or a mutation outdated them)
        self._path_code: dict = {}
        self._path_codes = np.zeros(0, dtype=np.int32)
        self._groups_installed: Optional[str] = None
        # IVF_FLAT lists are built lazily before a search (Milvus' background index build).  Once built they are kept across
        # upserts: the device index assigns upserted rows to the existing centroids at the next search (no k-means, like
        # Collection.upsert into an indexed collection, milvus_store.py:128).  k-means runs again only on build_index() or when
        # the collection has grown to RETRAIN_GROWTH x the row count the centroids were trained on.
        self._needs_train = False
        self._trained_rows = 0
        # hybrid search (lexical=True, or SEMCODE_MI355X_LEXICAL): one term row of lex_slots hashed terms per chunk, extracted from its
        # text at commit time into a host matrix (capacity >= len(self._ids)) and uploaded to the device index by row range;
        # _terms_on_device = the rows the index holds valid term rows for (-1: none); the df table is fetched once per mutation
        self.lexical = bool(getattr(settings, "mi355x_lexical", False) if lexical is None else lexical)
        self.lex_slots = int(lex_slots)
        if self.lex_slots not in (32, 64, 128, 256):
            raise ValueError(f"lex_slots must be 32, 64, 128 or 256, got {lex_slots!r}")
        self._terms = np.zeros((0, self.lex_slots), dtype=np.uint16)
        self._terms_on_device = -1
        self._lex_stats: Optional[tuple] = None  # (idf [65536] f32, avgdl f32)
        # late interaction (late=<MI355XLateReranker>, or SEMCODE_MI355X_LATE_STORE=f32|bf16 with the reranker of the settings): every
        # chunk's token vectors, without those of punctuation, go to the device index with its row (Index.put_tokens) and follow it
        # through deletes; late_format None = no token store
        fmt = str(late_format if late_format is not None else getattr(settings, "mi355x_late_store", "off") or "off").lower()
        if late is not None and late_format is None and fmt == "off":
            fmt = "f32"
        if fmt not in ("off", "f32", "bf16"):
            raise ValueError(f"late_format / mi355x_late_store must be off, f32 or bf16, got {fmt!r}")
        self.late = late
        self.late_format: Optional[str] = None if fmt == "off" else fmt
        # the hand-over at ingest (late_handover=, or SEMCODE_MI355X_LATE_HANDOVER): the late reranker's token head writes a chunk's vectors
        # straight into the index's token pool (store_document_tokens) instead of handing them over through the host; the stored bits are the same
        self.late_handover = bool(getattr(settings, "mi355x_late_handover", True) if late_handover is None else late_handover)

    # ------------------------------------------------------------------ lifecycle
    def connect(self) -> None:
        """Open the device and create the (empty) collection.  May raise; callers catch Exception."""
        settings = _resolve_settings()
        log.info("connecting_mi355x device=%s (milvus_uri %s is not used)", self._device, getattr(settings, "milvus_uri", None))
        with self._lock:
            if self._collection is not None:
                return
            self._collection = self._ensure_collection()
            if self.late_format is not None and self.late is None and getattr(settings, "mi355x_reranker_path", None):
                # a format without a reranker object: the late-interaction reranker of the settings (none there: every upsert brings token_vectors=)
                from ..embeddings.late import MI355XLateReranker

                self.late = MI355XLateReranker(runtime=self._runtime)
            store_path = getattr(settings, "mi355x_store_path", None)
            if store_path and (Path(store_path) / "manifest.json").exists() and not self._ids:
                self.load(store_path)  # utility.has_collection(...) -> Collection(name).load() of the reference (milvus_store.py:51-54)

    def _ensure_collection(self) -> Any:
        if self._index_factory is not None:
            return self._index_factory(dim=self.dim, metric=self.metric, kind=self.index_type, nlist=self.nlist)
        from .. import _native  # raises loudly if libsemcode_hip.so is missing

        if self._runtime is None:
            self._runtime = _native.shared_runtime(self._device)  # shared with the embedding client (device-to-device upserts)
            self._owns_runtime = False
        log.info("creating_collection %s dim=%d metric=%s index=%s", self.collection_name, self.dim, self.metric, self.index_type)
        return _native.Index(self._runtime, self.dim, metric=self.metric, kind=self.index_type, nlist=self.nlist)

    def close(self) -> None:
        with self._lock:
            if self._collection is not None and hasattr(self._collection, "close"):
                self._collection.close()
            self._collection = None
            if self._owns_runtime and self._runtime is not None:
                self._runtime.close()
                self._runtime = None

    def __len__(self) -> int:
        return len(self._ids)

    # ------------------------------------------------------------------ upsert
    def upsert_embeddings(self, payloads: Sequence[EmbeddingPayload], progress: Optional[Callable[[int, int], None]] = None,
                          token_vectors: Optional[Sequence[Any]] = None) -> None:
        """Insert or update embeddings (replace by primary key), reference milvus_store.py:87-133.  token_vectors (a store with a
        late format only): one [n_i, W] array per payload instead of the late reranker's own embed_document_tokens."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")

        payload_list: List[EmbeddingPayload] = list(payloads)
        total = len(payload_list)
        log.info("upserting_embeddings count=%d", total)
        if progress:
            progress(0, total)
        if total == 0:
            return

        settings = _resolve_settings()
        batch_size = max(1, getattr(settings, "milvus_upsert_batch_size", 128))
        inserted = 0
        for start in range(0, total, batch_size):
            batch = payload_list[start:start + batch_size]
            with self._lock:
                self._upsert_batch(batch, None if token_vectors is None else token_vectors[start:start + batch_size])
            inserted += len(batch)
            if progress:
                progress(inserted, total)

    def _upsert_batch(self, batch: Sequence[EmbeddingPayload], token_vectors: Optional[Sequence[Any]] = None) -> None:
        vectors = np.asarray([p.vector for p in batch], dtype=np.float32)
        if vectors.ndim != 2 or vectors.shape[1] != self.dim:
            raise ValueError(f"embedding dimension mismatch: collection dim={self.dim}, got array of shape {vectors.shape}")
        # a primary key repeated inside one batch: the last occurrence wins (upsert semantics)
        keep = sorted({p.id: i for i, p in enumerate(batch)}.values())
        ids = [batch[i].id for i in keep]
        rows = self.plan_rows(ids)
        # one native call per batch: it validates that every row is an existing row or the next free one, so a drift between
        # the device index and the host columns fails loudly; the columns are committed only after it has succeeded
        self._put_rows(vectors[keep], rows)
        self.commit_rows(ids, rows, [batch[i].text for i in keep], [batch[i].metadata for i in keep],
                         token_vectors=None if token_vectors is None else [token_vectors[i] for i in keep])

    def _put_rows(self, vectors: np.ndarray, rows: np.ndarray) -> None:
        ix = self._collection
        if hasattr(ix, "put_rows"):
            ix.put_rows(vectors, rows)
        else:  # an index_factory object with only the add / overwrite pair
            new = rows >= len(self._ids)
            if new.any():
                ix.add(vectors[new])
            if (~new).any():
                ix.overwrite(vectors[~new], rows[~new])
        if hasattr(ix, "__len__") and len(ix) != max(len(self._ids), int(rows.max()) + 1):
            raise RuntimeError(f"vector index holds {len(ix)} rows, the collection's columns expect {max(len(self._ids), int(rows.max()) + 1)}")

    # ------------------------------------------------------------------ array fast paths
    def plan_rows(self, ids: Sequence[str]) -> np.ndarray:
        """Row numbers an upsert of these primary keys writes: the existing row of a known key, else the next free rows in
        order of appearance.  Keys must be distinct (deduplicate first: the last occurrence wins in an upsert)."""
        if len(set(ids)) != len(ids):
            raise ValueError("plan_rows: primary keys must be distinct")
        rows = np.empty(len(ids), dtype=np.int64)
        next_row = len(self._ids)
        for i, pk in enumerate(ids):
            row = self._row_of.get(pk)
            if row is None:
                row = next_row
                next_row += 1
            rows[i] = row
        return rows

    def commit_rows(self, ids: Sequence[str], rows: np.ndarray, texts: Sequence[str], metadatas: Sequence[dict],
                    token_vectors: Optional[Sequence[Any]] = None) -> None:
        """Scalar columns + primary-key map for rows whose vectors have just been written (same mapping as _upsert_batch).  A store
        with a late format also stores every row's token vectors (token_vectors, or the late reranker's for `texts`): a replaced
        primary key replaces its row's tokens."""
        if self.late_format is not None and len(rows):
            self._commit_tokens(rows, texts, token_vectors)  # (first: a failure leaves the columns as they were)
        self._mask_cache.clear()
        self._groups_installed = None
        for pk, row, text, meta in zip(ids, rows.tolist(), texts, metadatas):
            cols = (meta.get("repo", ""), meta.get("path", ""), meta.get("language", ""))
            self._set_codes(row, cols[0], cols[2], cols[1])
            if row == len(self._ids):
                self._row_of[pk] = row
                self._ids.append(pk)
                self._repos.append(cols[0])
                self._paths.append(cols[1])
                self._languages.append(cols[2])
                self._texts.append(text)
                self._metadata.append(meta)
            else:
                self._repos[row], self._paths[row], self._languages[row] = cols
                self._texts[row] = text
                self._metadata[row] = meta
        if self.lexical and len(rows):
            self._commit_terms(rows, texts)
        self._note_growth()

    # ------------------------------------------------------------------ token vectors of the late-interaction store
    def _commit_tokens(self, rows: np.ndarray, texts: Sequence[str], token_vectors: Optional[Sequence[Any]]) -> None:
        ix = self._collection
        if not hasattr(ix, "put_tokens"):
            raise NotImplementedError(f"{type(ix).__name__} has no put_tokens(rows, token_vectors, fmt): this vector index cannot keep token vectors")
        if token_vectors is None:
            if self.late is None:
                raise ValueError("a store with a late format needs token vectors: construct it with late=<MI355XLateReranker> or pass token_vectors=")
            if self._hands_over(ix):
                if len(texts) != len(rows):
                    raise ValueError(f"{len(rows)} rows but {len(texts)} texts")
                self.late.store_document_tokens(list(texts), ix, np.asarray(rows, dtype=np.int64), self.late_format)
                return
            token_vectors = self.late.embed_document_tokens(list(texts), kept_only=True)
        if len(token_vectors) != len(rows):
            raise ValueError(f"{len(rows)} rows but {len(token_vectors)} token arrays")
        ix.put_tokens(np.asarray(rows, dtype=np.int64), list(token_vectors), fmt=self.late_format)

    def _hands_over(self, ix: Any) -> bool:
        """The late reranker can write its token vectors into this index on the device: the setting is on, the reranker has
        store_document_tokens, and its encoder lives on the index's runtime.  Anything else takes the path through the host."""
        late = self.late
        if not self.late_handover or not hasattr(late, "store_document_tokens"):
            return False
        shares = getattr(late, "shares_runtime", None)
        return bool(shares is not None and shares(ix))

    def has_late_tokens(self, rows: Any) -> bool:
        """True when the store keeps token vectors and every one of these rows (-1 entries aside) has some."""
        ix = self._collection
        if self.late_format is None or ix is None or not hasattr(ix, "token_counts"):
            return False
        r = np.asarray(rows, dtype=np.int64).reshape(-1)
        r = r[r >= 0]
        with self._lock:
            return bool(r.size == 0 or (ix.token_counts(r) > 0).all())

    def rerank_late(self, question_vectors: Any, rows: Any) -> np.ndarray:
        """MaxSim scores [Bq, C] of every question (one [nq, W] array each, as MI355XLateReranker.embed_query_tokens returns them)
        against the rows [Bq, C] a search returned (-1 = padding: -inf), read from the stored token vectors: no passage forward."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        with self._lock:
            return self._collection.rerank_late(question_vectors, np.asarray(rows, dtype=np.int64))

    def search_late(self, question_vectors: Any, top_k: int = 10, *, repos: Any = None, languages: Any = None) -> "tuple[np.ndarray, np.ndarray]":
        """The exact MaxSim search over the stored token vectors: (score [Bq, k], rows [Bq, k]; -1 = no hit), best first, ties to the
        lower row.  repos / languages as in search_batch.  top_k <= 128."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        if self.late_format is None:
            raise ValueError("search_late needs the token store: construct the store with late=... / late_format=... (or set SEMCODE_MI355X_LATE_STORE)")
        with self._lock:
            flt = self._filter(repos, languages)
            allow = None if flt is None or flt[1] else flt[0]
            return self._collection.search_late(question_vectors, k=int(top_k), allow=allow)

    # ------------------------------------------------------------------ term rows of the hybrid search
    @staticmethod
    def _lex_terms(texts: Sequence[str], slots: int) -> np.ndarray:
        from .. import _native

        return _native.lex_terms(texts, slots)[0]

    def _commit_terms(self, rows: np.ndarray, texts: Sequence[str]) -> None:
        """Term rows of the rows just committed: into the host matrix, then the range [lowest, highest] of them to the device -- an append
        uploads its own rows only.  An index that holds no valid term rows (first use, after a delete) gets the whole matrix."""
        n = len(self._ids)
        if n > self._terms.shape[0]:
            grown = np.full((max(1024, 2 * self._terms.shape[0], n), self.lex_slots), 0xFFFF, dtype=np.uint16)
            grown[: self._terms.shape[0]] = self._terms
            self._terms = grown
        rows = np.asarray(rows, dtype=np.int64)
        self._terms[rows] = self._lex_terms(list(texts), self.lex_slots)
        self._lex_stats = None
        ix = self._collection
        if not hasattr(ix, "set_terms"):
            self._terms_on_device = -1  # (a search with hybrid= names what is missing)
            return
        lo, hi = int(rows.min()), int(rows.max()) + 1
        if self._terms_on_device < 0 or lo > self._terms_on_device:
            self._upload_all_terms()
            return
        ix.set_terms(self._terms[lo:hi], first_row=lo)
        self._terms_on_device = max(hi, self._terms_on_device)

    def _upload_all_terms(self) -> None:
        """The whole host matrix to the device index (after a delete dropped its term rows, after load).  Caller holds the lock."""
        ix = self._collection
        self._lex_stats = None
        self._terms_on_device = -1
        if hasattr(ix, "set_terms"):
            if hasattr(ix, "drop_terms"):
                ix.drop_terms()
            ix.set_terms(self._terms[: len(self._ids)], first_row=0)
            self._terms_on_device = len(self._ids)

    def _set_codes(self, row: int, repo: str, language: str, path: str = "") -> None:
        if row >= self._repo_codes.size:
            cap = max(1024, 2 * self._repo_codes.size, row + 1)
            self._repo_codes = np.concatenate([self._repo_codes, np.zeros(cap - self._repo_codes.size, np.int32)])
            self._lang_codes = np.concatenate([self._lang_codes, np.zeros(cap - self._lang_codes.size, np.int32)])
            self._path_codes = np.concatenate([self._path_codes, np.zeros(cap - self._path_codes.size, np.int32)])
        self._repo_codes[row] = self._repo_code.setdefault(repo, len(self._repo_code))
        self._lang_codes[row] = self._lang_code.setdefault(language, len(self._lang_code))
        self._path_codes[row] = self._path_code.setdefault((repo, path), len(self._path_code))

    def _note_growth(self) -> None:
        n = len(self._ids)
        if self._trained_rows == 0 or n >= self.RETRAIN_GROWTH * self._trained_rows:
            self._needs_train = True

    def upsert_arrays(self, ids: Sequence[str], vectors: Any, texts: Sequence[str], metadatas: Sequence[dict],
                      progress: Optional[Callable[[int, int], None]] = None, token_vectors: Optional[Sequence[Any]] = None) -> None:
        """upsert_embeddings without EmbeddingPayload / list[float] boxing: vectors is one [n, dim] float array.  Same
        progress protocol and batch size (settings.milvus_upsert_batch_size), same replace-by-primary-key result."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        vec = np.asarray(vectors, dtype=np.float32)
        total = len(ids)
        if vec.ndim != 2 or vec.shape != (total, self.dim):
            raise ValueError(f"embedding dimension mismatch: collection dim={self.dim}, expected [{total}, {self.dim}], got {vec.shape}")
        if not (len(texts) == len(metadatas) == total):
            raise ValueError("ids, texts and metadatas must have one entry per vector")
        if progress:
            progress(0, total)
        if total == 0:
            return
        batch_size = max(1, getattr(_resolve_settings(), "milvus_upsert_batch_size", 128))
        done = 0
        for start in range(0, total, batch_size):
            stop = min(total, start + batch_size)
            last = {pk: i for i, pk in enumerate(ids[start:stop], start)}  # repeated key inside a batch: last wins
            keep = sorted(last.values())
            b_ids = [ids[i] for i in keep]
            with self._lock:
                rows = self.plan_rows(b_ids)
                self._put_rows(vec[keep], rows)
                self.commit_rows(b_ids, rows, [texts[i] for i in keep], [metadatas[i] for i in keep],
                                 token_vectors=None if token_vectors is None else [token_vectors[i] for i in keep])
            done = stop
            if progress:
                progress(done, total)

    def upsert_encoded(self, ids: Sequence[str], token_ids: np.ndarray, lens: np.ndarray, texts: Sequence[str], metadatas: Sequence[dict],
                       embedding_client: Any, wait: bool = True, token_vectors: Optional[Sequence[Any]] = None) -> None:
        """One batch, embed + upsert fused: the encoder output goes from its device buffer straight into the index rows.
        wait=False: the device work is only enqueued (embedding_client.wait() completes it); searches issued afterwards are
        ordered behind it on the device stream either way."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        with self._lock:
            rows = self.plan_rows(ids)
            # argument errors surface here, before anything is committed; with wait=False a failure of the enqueued device
            # work is reported by embedding_client.wait() (services.ingest_chunks calls it before it returns) -- the rows of
            # that batch then hold undefined vectors and the caller must upsert them again
            embedding_client.embed_ids_into(self, token_ids, lens, rows, wait=wait)
            self.commit_rows(ids, rows, texts, metadatas, token_vectors=token_vectors)

    # ------------------------------------------------------------------ delete (Collection.delete(expr) of pymilvus)
    def delete(self, ids: Sequence[str]) -> int:
        """Remove the rows of these primary keys; unknown (and repeated) keys are ignored.  Returns the number of rows removed.
        The rows behind a removed row move up (row numbers stay dense): Hit.row values obtained before the call are stale."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        with self._lock:
            return self._delete_rows(sorted({self._row_of[pk] for pk in ids if pk in self._row_of}))

    def _rows_where(self, repo: Optional[str], path: Optional[str], language: Optional[str]) -> "list[int]":
        if repo is None and path is None and language is None:
            raise ValueError("give at least one of repo, path, language")
        return [r for r in range(len(self._ids))
                if (repo is None or self._repos[r] == repo) and (path is None or self._paths[r] == path)
                and (language is None or self._languages[r] == language)]

    def keys_where(self, *, repo: Optional[str] = None, path: Optional[str] = None, language: Optional[str] = None) -> List[str]:
        """Primary keys of the rows whose scalar columns equal ALL the given values (what delete_where would remove), in row order."""
        with self._lock:
            return [self._ids[r] for r in self._rows_where(repo, path, language)]

    def delete_where(self, *, repo: Optional[str] = None, path: Optional[str] = None, language: Optional[str] = None) -> int:
        """Remove every row whose scalar columns equal ALL the given values (`repo == .. and path == ..`, the expr of
        Collection.delete); at least one must be given.  Returns the number of rows removed.  Hit.row values obtained before
        the call are stale afterwards, as with delete()."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        with self._lock:
            return self._delete_rows(self._rows_where(repo, path, language))

    def _delete_rows(self, rows: "list[int]") -> int:
        """rows: ascending, distinct.  One native call, then the columns: committed only after the call has succeeded, so a
        failure leaves the vectors and the columns as they were (caller holds the lock).  With lexical=True the host term matrix is
        compacted with the same renumbering and uploaded again WHOLE (2 * lex_slots bytes per surviving row over the host link): the
        device index drops its term rows on a delete and does not compact them in place."""
        ix = self._collection
        if not hasattr(ix, "delete_rows"):
            raise NotImplementedError(f"{type(ix).__name__} has no delete_rows(rows): this vector index cannot delete")
        if not rows:
            return 0
        ix.delete_rows(np.asarray(rows, dtype=np.int64))
        gone = np.zeros(len(self._ids), dtype=bool)
        gone[rows] = True
        keep = np.flatnonzero(~gone).tolist()
        for name in ("_ids", "_texts", "_metadata", "_repos", "_paths", "_languages"):
            col = getattr(self, name)
            setattr(self, name, [col[r] for r in keep])
        self._row_of = {pk: r for r, pk in enumerate(self._ids)}
        self._repo_codes = self._repo_codes[: gone.size][~gone]
        self._lang_codes = self._lang_codes[: gone.size][~gone]
        self._path_codes = self._path_codes[: gone.size][~gone]
        self._mask_cache.clear()
        self._groups_installed = None
        if self.lexical:
            self._terms = self._terms[: gone.size][~gone]
            self._upload_all_terms()
        if hasattr(ix, "__len__") and len(ix) != len(self._ids):
            raise RuntimeError(f"vector index holds {len(ix)} rows after the delete, the collection's columns expect {len(self._ids)}")
        return len(rows)

    # ------------------------------------------------------------------ search
    def search(self, vector: "list[float]", top_k: int = 10, *, repos: Any = None, languages: Any = None, group_by: Optional[str] = None,
               mmr: Optional[float] = None, fetch_k: Optional[int] = None, query_text: Optional[str] = None, hybrid: Any = None) -> SearchResult:
        """Run a raw vector search (one query), reference milvus_store.py:135-148.  repos / languages / group_by / mmr / fetch_k /
        query_text (query_texts there) / hybrid: see search_batch."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        dist, rows = self.search_batch(np.asarray([vector], dtype=np.float32), top_k, repos=repos, languages=languages, group_by=group_by, mmr=mmr, fetch_k=fetch_k,
                                       query_texts=None if query_text is None else [query_text], hybrid=hybrid)
        return SearchResult([self._hits(dist[0], rows[0])])

    GROUP_BY = ("path", "repo")
    MMR_MAX_FETCH = 128  # the widest candidate list of Index.search_mmr
    HYBRID_MAX_FETCH = 128  # ... and of Index.search_hybrid
    HYBRID_DEFAULTS = {"c": 60, "dense_weight": 1.0, "lexical_weight": 1.0}
    BM25_K1, BM25_B = 1.2, 0.75

    def search_batch(self, queries: Any, top_k: int = 10, *, repos: Any = None, languages: Any = None,
                     group_by: Optional[str] = None, mmr: Optional[float] = None, fetch_k: Optional[int] = None,
                     query_texts: Optional[Sequence[str]] = None, hybrid: Any = None) -> "tuple[np.ndarray, np.ndarray]":
        """Batched search: queries [Q, dim] -> (dist [Q, k] f32, rows [Q, k] i64; -1 = no hit), best first.

        repos / languages (Collection.search(expr=...) for the two filters of the reference front ends): None = no restriction, a
        string or a collection of strings = only rows whose column value is one of them; both given = both must hold.  An empty
        collection or unknown names match nothing: no hits.  A restricted search is always exact -- the exhaustive answer over the
        rows that pass, never an IVF probe (Index.search_masked).  A filter that every row passes is today's unfiltered call.

        group_by (Collection.search(group_by_field=...)): None = every chunk counts; "path" = at most one hit per file, i.e. per
        pair (repo, path); "repo" = at most one hit per repo.  A group is represented by its best row among those the filter
        passes; the hits are the top_k best groups, best first.  Always exact, top_k <= 128 (Index.search_grouped).

        mmr (search_type="mmr" of the LangChain vector stores; the value is their lambda_mult): None = today's behaviour; a number
        in [0, 1] = maximal marginal relevance over the exact top-fetch_k of the rows the filter passes: the best hit first, then
        greedily the candidate with the largest mmr * relevance - (1 - mmr) * (largest similarity to a hit already taken), both in
        the collection's metric.  1 = the plain order, 0 = diversity alone.  The hits come in selection order, not best first.
        fetch_k defaults to min(128, max(20, 4 top_k)); top_k <= fetch_k <= 128.  Always exact (Index.search_mmr); not combined
        with group_by.

        hybrid (Collection.hybrid_search with an RRFRanker; the LangChain ensemble retrievers): None / False = today's behaviour; True
        or a dict with any of c (default 60), dense_weight, lexical_weight (default 1) = the exact dense top-fetch_k and the BM25
        top-fetch_k of query_texts (one text per query) over the chunks' hashed code terms, fused by weighted reciprocal rank:
        score = dense_weight / (c + dense rank) + lexical_weight / (c + lexical rank), ranks from 0, a chunk missing from one list
        getting 0 for it.  The returned distances are these fused scores, best first.  A question that names an identifier finds the
        chunks that contain it even where the embedding does not.  The text goes through the extractor of the chunks and is reduced
        to its at most 32 distinct terms of highest IDF = ln(1 + (N - df + 0.5) / (df + 0.5)) (ties to the lower term); k1 = 1.2,
        b = 0.75, avgdl = sum_dl / N.  fetch_k defaults as for mmr; top_k <= fetch_k <= 128.  Needs lexical=True at construction (or
        SEMCODE_MI355X_LEXICAL); always exact (Index.search_hybrid); not combined with group_by or mmr."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        if group_by is not None and group_by not in self.GROUP_BY:
            raise ValueError(f"group_by must be None or one of {self.GROUP_BY}, got {group_by!r}")
        fuse = self._hybrid_options(hybrid, query_texts, group_by, mmr)
        if mmr is None and fuse is None and fetch_k is not None:
            raise ValueError("fetch_k is the candidate width of an mmr search: give mmr as well")
        if fuse is not None:
            top_k, fetch_k = self._candidate_widths("a hybrid", top_k, fetch_k, self.HYBRID_MAX_FETCH)
        if mmr is not None:
            if group_by is not None:
                raise ValueError("mmr together with group_by is not supported")
            lam = float(mmr)
            if not 0.0 <= lam <= 1.0:  # (NaN fails both comparisons)
                raise ValueError(f"mmr must be within [0, 1], got {mmr!r}")
            top_k, fetch_k = self._candidate_widths("an mmr", top_k, fetch_k, self.MMR_MAX_FETCH)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"query dimension mismatch: collection dim={self.dim}, got shape {q.shape}")
        if fuse is not None and len(query_texts) != q.shape[0]:
            raise ValueError(f"hybrid: {q.shape[0]} query vectors but {len(query_texts)} query texts")
        with self._lock:
            flt = self._filter(repos, languages)
            allow = None if flt is None or flt[1] else flt[0]  # the bitset handed down: none where every row passes
            if fuse is not None:
                return self._search_hybrid(q, top_k, fetch_k, list(query_texts), fuse, allow)
            if group_by is not None:
                return self._search_grouped(q, int(top_k), allow, group_by)
            if mmr is not None:
                ix = self._collection
                if not hasattr(ix, "search_mmr"):
                    raise NotImplementedError(f"{type(ix).__name__} has no search_mmr(queries, k, fetch_k, lam, allow): this vector index cannot diversify")
                return ix.search_mmr(q, k=top_k, fetch_k=fetch_k, lam=lam, allow=allow)
            if allow is None:
                self._maybe_train()
                return self._collection.search(q, k=int(top_k), nprobe=self.nprobe)
            ix = self._collection
            if not hasattr(ix, "search_masked"):
                raise NotImplementedError(f"{type(ix).__name__} has no search_masked(queries, allow, k): this vector index cannot filter")
            return ix.search_masked(q, allow, k=int(top_k))

    @staticmethod
    def _candidate_widths(what: str, top_k: Any, fetch_k: Any, widest: int) -> "tuple[int, int]":
        """(top_k, fetch_k) of `what` ("an mmr" / "a hybrid") search as integers, fetch_k defaulted: top_k <= fetch_k <= widest."""
        top_k = int(top_k)
        if top_k > widest:
            raise ValueError(f"{what} search takes top_k <= {widest}, got {top_k}")
        fetch_k = min(widest, max(20, 4 * top_k)) if fetch_k is None else int(fetch_k)
        if fetch_k > widest:
            raise ValueError(f"{what} search takes fetch_k <= {widest}, got {fetch_k}")
        if fetch_k < top_k:
            raise ValueError(f"fetch_k={fetch_k} is smaller than top_k={top_k}")
        return top_k, fetch_k

    def _search_grouped(self, q: np.ndarray, top_k: int, allow: "Optional[np.ndarray]", group_by: str) -> "tuple[np.ndarray, np.ndarray]":
        """The labels of `group_by` reach the index once per (mutation, column), then every grouped search reuses them.  Caller holds the lock."""
        ix = self._collection
        if not (hasattr(ix, "search_grouped") and hasattr(ix, "set_groups")):
            raise NotImplementedError(f"{type(ix).__name__} has no set_groups(labels) / search_grouped(queries, k, allow): this vector index cannot group")
        if self._groups_installed != group_by:
            codes = self._path_codes if group_by == "path" else self._repo_codes
            ix.set_groups(np.ascontiguousarray(codes[: len(self._ids)], dtype=np.int32))
            self._groups_installed = group_by
        return ix.search_grouped(q, k=top_k, allow=allow)

    def _hybrid_options(self, hybrid: Any, query_texts: Any, group_by: Any, mmr: Any) -> "Optional[dict]":
        """None when no hybrid search is asked for, else {c, dense_weight, lexical_weight}; names every conflict."""
        if hybrid is None or hybrid is False:
            return None
        if hybrid is True:
            opts = dict(self.HYBRID_DEFAULTS)
        elif isinstance(hybrid, dict):
            unknown = sorted(set(hybrid) - set(self.HYBRID_DEFAULTS))
            if unknown:
                raise ValueError(f"hybrid: unknown keys {unknown}; known: {sorted(self.HYBRID_DEFAULTS)}")
            opts = {**self.HYBRID_DEFAULTS, **hybrid}
        else:
            raise ValueError(f"hybrid must be None, a bool or a dict with any of {sorted(self.HYBRID_DEFAULTS)}, got {hybrid!r}")
        if not self.lexical:
            raise ValueError("hybrid search needs the lexical leg: construct the store with lexical=True (or set SEMCODE_MI355X_LEXICAL)")
        if query_texts is None:
            raise ValueError("hybrid search needs the query text: give query_text (search) / query_texts (search_batch)")
        if group_by is not None:
            raise ValueError("hybrid together with group_by is not supported")
        if mmr is not None:
            raise ValueError("hybrid together with mmr is not supported")
        c = opts["c"]
        if isinstance(c, bool) or int(c) != c or int(c) < 1:
            raise ValueError(f"hybrid: c must be an integer >= 1, got {c!r}")
        opts["c"] = int(c)
        for name in ("dense_weight", "lexical_weight"):
            w = float(opts[name])
            if not (0.0 <= w < float("inf")):
                raise ValueError(f"hybrid: {name} must be finite and >= 0, got {opts[name]!r}")
            opts[name] = w
        return opts

    def lex_query(self, text: str, idf: np.ndarray) -> "tuple[np.ndarray, np.ndarray, int]":
        """(qterms [32] uint16 ascending, qweights [32] f32, m) of a query text: its distinct terms through the chunks' extractor, the at
        most 32 of highest idf kept (ties to the lower term), weighted by that idf."""
        ts = np.unique(self._lex_terms([text], self.lex_slots)[0])
        ts = ts[ts != 0xFFFF]
        ts = ts[np.lexsort((ts, -idf[ts].astype(np.float64)))][:32]
        ts.sort()
        qt = np.full(32, 0xFFFF, dtype=np.uint16)
        qw = np.zeros(32, dtype=np.float32)
        qt[: ts.size] = ts
        qw[: ts.size] = idf[ts]
        return qt, qw, int(ts.size)

    def _search_hybrid(self, q: np.ndarray, top_k: int, fetch_k: int, texts: "list[str]", fuse: dict, allow: "Optional[np.ndarray]") -> "tuple[np.ndarray, np.ndarray]":
        """Caller holds the lock.  The df table comes from the device once per mutation."""
        ix = self._collection
        if not (hasattr(ix, "search_hybrid") and hasattr(ix, "set_terms") and hasattr(ix, "lex_stats")):
            raise NotImplementedError(f"{type(ix).__name__} has no set_terms / lex_stats / search_hybrid: this vector index cannot run a hybrid search")
        if self._terms_on_device != len(self._ids):
            self._upload_all_terms()
        if self._lex_stats is None:
            st = ix.lex_stats()
            n = int(st["rows"])
            df = np.asarray(st["df"], dtype=np.float64)
            idf = np.log(1.0 + (n - df + 0.5) / (df + 0.5)).astype(np.float32)
            self._lex_stats = (idf, np.float32(st["sum_dl"] / n) if n > 0 and st["sum_dl"] > 0 else np.float32(1.0))
        idf, avgdl = self._lex_stats
        terms = [self.lex_query(t, idf) for t in texts]
        qt = np.stack([t[0] for t in terms])
        qw = np.stack([t[1] for t in terms])
        nt = np.asarray([t[2] for t in terms], dtype=np.int32)
        return ix.search_hybrid(q, qt, qw, nt, k=top_k, fetch_k=fetch_k, k1=self.BM25_K1, b=self.BM25_B, avgdl=float(avgdl), c=fuse["c"],
                                dense_weight=fuse["dense_weight"], lexical_weight=fuse["lexical_weight"], allow=allow)

    @staticmethod
    def _name_set(names: Any) -> "Optional[frozenset]":
        if names is None:
            return None
        return frozenset([names]) if isinstance(names, str) else frozenset(names)

    def _filter(self, repos: Any, languages: Any) -> "Optional[tuple[np.ndarray, bool]]":
        """(packed bitset over rows, every row passes) of a filter, cached until the next mutation; None without a filter.
        Caller holds the lock."""
        key = (self._name_set(repos), self._name_set(languages))
        if key == (None, None):
            return None
        hit = self._mask_cache.get(key)
        if hit is None:
            n = len(self._ids)
            ok = np.ones(n, dtype=bool)
            for names, table, codes in ((key[0], self._repo_code, self._repo_codes), (key[1], self._lang_code, self._lang_codes)):
                if names is not None:
                    ok &= np.isin(codes[:n], np.asarray([table[x] for x in names if x in table], dtype=np.int32))
            hit = self._mask_cache[key] = (pack_allow(ok, n), bool(ok.all()))
        return hit

    def row_filter(self, *, repos: Any = None, languages: Any = None) -> "Optional[np.ndarray]":
        """The bitset search / search_batch hand to the device for this filter: uint32 words over row numbers (bit r & 31 of word
        r >> 5 = row r passes), or None when neither argument is given.  Valid until the next upsert, delete or load -- row numbers
        move; do not modify it (it is the cached array)."""
        with self._lock:
            flt = self._filter(repos, languages)
            return None if flt is None else flt[0]

    def build_index(self, niter: int = 10) -> None:
        """(Re)build the IVF_FLAT lists now (create_index + load of the reference, milvus_store.py:76-84)."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        with self._lock:
            if self.index_type == "IVF_FLAT" and hasattr(self._collection, "train") and len(self._ids) > 0:
                self._train(niter)
            self._needs_train = False

    def _train(self, niter: int) -> None:
        if hasattr(self._collection, "release_scratch"):
            self._collection.release_scratch()  # training needs a second copy of the corpus: drop what can be rebuilt first
        self._collection.train(niter=niter)
        self._trained_rows = len(self._ids)

    def _maybe_train(self) -> None:
        # faiss' rule of thumb: at least 39 points per centroid, otherwise the exhaustive scan is used (exact results)
        if self._needs_train and self.index_type == "IVF_FLAT" and hasattr(self._collection, "train") and len(self._ids) >= 39 * self.nlist:
            try:
                self._train(10)
            except Exception as exc:  # e.g. no room for the second corpus copy: serve exact exhaustive results instead of failing every search
                log.warning("ivf_train_failed rows=%d nlist=%d: %s -- answering with the exhaustive scan until build_index() succeeds",
                            len(self._ids), self.nlist, exc)
        self._needs_train = False

    def hits_for(self, dist: np.ndarray, rows: np.ndarray) -> SearchResult:
        """Materialise pymilvus-shaped results for a search_batch() output."""
        return SearchResult([self._hits(d, r) for d, r in zip(dist, rows)])

    def _hits(self, dist: np.ndarray, rows: np.ndarray) -> Hits:
        hits = Hits()
        for d, r in zip(dist.tolist(), rows.tolist()):
            if r < 0:
                continue
            fields = {"repo": self._repos[r], "path": self._paths[r], "language": self._languages[r], "text": self._texts[r],
                      "metadata": self._metadata[r]}
            hits.append(Hit(self._ids[r], d, fields, r))
        return hits

    # ------------------------------------------------------------------ persistence (replaces Milvus' volume, docker-compose.yml:13-14)
    def save(self, path: "str | Path") -> None:
        """Write the collection to `path/` : manifest.json, vectors.f32 (row-major [rows, dim]), columns.jsonl
        (id, repo, path, language, text, metadata per row) and, when the IVF_FLAT lists are built, ivf_centroids.f32
        ([nlist, dim]) + ivf_assign.i32 (list of every row).  Written to a temporary directory and renamed."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        path = Path(path)
        tmp = path.with_name(path.name + ".tmp")
        if tmp.exists():
            shutil.rmtree(tmp)
        tmp.mkdir(parents=True)
        with self._lock:
            n = len(self._ids)
            with open(tmp / "vectors.f32", "wb") as f:
                for start in range(0, n, 65536):
                    m = min(65536, n - start)
                    np.ascontiguousarray(self._collection.get_rows(start, m), dtype="<f4").tofile(f)
            with open(tmp / "columns.jsonl", "w", encoding="utf-8") as f:
                for r in range(n):
                    f.write(json.dumps({"id": self._ids[r], "repo": self._repos[r], "path": self._paths[r], "language": self._languages[r],
                                        "text": self._texts[r], "metadata": self._metadata[r]}, ensure_ascii=False) + "\n")
            manifest = {"format": "semcode_amd.collection.v1", "collection_name": self.collection_name, "dim": self.dim, "rows": n,
                        "metric": self.metric, "index_type": self.index_type, "nlist": self.nlist, "nprobe": self.nprobe}
            ivf = self._collection.ivf_info() if (not self._needs_train and hasattr(self._collection, "ivf_info")) else None
            if ivf and ivf.get("nlist", 0) > 0 and hasattr(self._collection, "ivf_assignments"):
                np.ascontiguousarray(ivf["centroids"], dtype="<f4").tofile(tmp / "ivf_centroids.f32")
                np.ascontiguousarray(self._collection.ivf_assignments(), dtype="<i4").tofile(tmp / "ivf_assign.i32")
                manifest["ivf_trained_nlist"] = int(ivf["nlist"])
            st = self._collection.token_stats() if self.late_format is not None and hasattr(self._collection, "token_stats") else None
            if st and st["W"]:  # tokens.f32 | tokens.bf16 ([tokens, W], row after row) + token_counts.i32 ([rows])
                counts_all = []
                with open(tmp / f"tokens.{st['fmt']}", "wb") as f:
                    for start in range(0, n, 16384):
                        counts, vecs = self._collection.get_tokens(np.arange(start, min(n, start + 16384)))
                        counts_all.append(counts)
                        if st["fmt"] == "bf16":  # the stored values have no lower half: the file holds the upper one
                            (np.ascontiguousarray(vecs).view(np.uint32) >> 16).astype("<u2").tofile(f)
                        else:
                            np.ascontiguousarray(vecs, dtype="<f4").tofile(f)
                counts_all = np.concatenate(counts_all) if counts_all else np.zeros(0, np.int32)
                counts_all.astype("<i4").tofile(tmp / "token_counts.i32")
                manifest.update(late_format=st["fmt"], late_width=int(st["W"]), late_tokens=int(counts_all.sum()))
            (tmp / "manifest.json").write_text(json.dumps(manifest, indent=1))
        if path.exists():
            shutil.rmtree(path)
        tmp.rename(path)

    def load(self, path: "str | Path") -> None:
        """Replace the collection's content with a directory written by save() (connect() first)."""
        if self._collection is None:
            raise RuntimeError("Milvus collection is not initialized. Call connect() first.")
        path = Path(path)
        manifest = json.loads((path / "manifest.json").read_text())
        if manifest.get("format") != "semcode_amd.collection.v1":
            raise ValueError(f"{path}: unknown collection format {manifest.get('format')!r}")
        if manifest["dim"] != self.dim:
            raise ValueError(f"{path}: stored dim {manifest['dim']} != collection dim {self.dim}")
        with self._lock:
            if len(self._ids):
                raise RuntimeError("load() needs an empty collection")
            n = manifest["rows"]
            vec = np.memmap(path / "vectors.f32", dtype="<f4", mode="r", shape=(n, self.dim)) if n else np.zeros((0, self.dim), np.float32)
            for start in range(0, n, 65536):
                self._collection.add(np.asarray(vec[start:start + 65536], dtype=np.float32))
            with open(path / "columns.jsonl", encoding="utf-8") as f:
                for line in f:
                    c = json.loads(line)
                    self._row_of[c["id"]] = len(self._ids)
                    self._ids.append(c["id"])
                    self._repos.append(c["repo"])
                    self._paths.append(c["path"])
                    self._languages.append(c["language"])
                    self._texts.append(c["text"])
                    self._metadata.append(c["metadata"])
            if len(self._ids) != n:
                raise ValueError(f"{path}: columns.jsonl holds {len(self._ids)} rows, manifest says {n}")
            self._mask_cache.clear()
            self._groups_installed = None
            for row, (repo, language, col_path) in enumerate(zip(self._repos, self._languages, self._paths)):
                self._set_codes(row, repo, language, col_path)
            if self.lexical:  # (the term rows are not persisted: rebuilt from the saved texts)
                self._terms = self._lex_terms(self._texts, self.lex_slots) if n else np.zeros((0, self.lex_slots), dtype=np.uint16)
                self._upload_all_terms()
            if manifest.get("late_format") in ("f32", "bf16") and n > 0:
                self._load_tokens(path, manifest, n)
            self._needs_train = True
            # the saved lists are reused as they are (no k-means) when they fit this collection's index parameters
            tn = int(manifest.get("ivf_trained_nlist", 0))
            if (tn > 0 and n > 0 and self.index_type == "IVF_FLAT" and manifest.get("metric") == self.metric and hasattr(self._collection, "set_ivf")
                    and (path / "ivf_centroids.f32").exists() and (path / "ivf_assign.i32").exists()):
                cent = np.fromfile(path / "ivf_centroids.f32", dtype="<f4")
                assign = np.fromfile(path / "ivf_assign.i32", dtype="<i4")
                if cent.size == tn * self.dim and assign.size == n:
                    self._collection.set_ivf(cent.reshape(tn, self.dim), assign)
                    self._needs_train = False
                    self._trained_rows = n

    def _load_tokens(self, path: Path, manifest: dict, n: int) -> None:
        """The saved token vectors back into the device index, in the saved format (which becomes the store's).  Caller holds the lock."""
        fmt, W, total = manifest["late_format"], int(manifest["late_width"]), int(manifest["late_tokens"])
        counts = np.fromfile(path / "token_counts.i32", dtype="<i4")
        if counts.size != n or int(counts.sum()) != total:
            raise ValueError(f"{path}: token_counts.i32 holds {counts.size} rows / {int(counts.sum())} tokens, manifest says {n} / {total}")
        data = np.memmap(path / f"tokens.{fmt}", dtype="<u2" if fmt == "bf16" else "<f4", mode="r", shape=(total, W)) if total else None
        self.late_format = fmt
        off = np.concatenate(([0], np.cumsum(counts, dtype=np.int64)))
        for start in range(0, n, 16384):
            stop = min(n, start + 16384)
            if off[stop] == off[start]:
                continue
            block = np.asarray(data[off[start]:off[stop]])
            vecs = (block.astype(np.uint32) << 16).view(np.float32) if fmt == "bf16" else block.astype(np.float32)
            self._collection.put_tokens(np.arange(start, stop), (counts[start:stop].astype(np.int32), vecs), fmt=fmt)

    def __iter__(self) -> Iterator:  # pragma: no cover - convenience
        return iter(self._ids)
