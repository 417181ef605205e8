"""What the token-store tests share (test_late_store_host.py, test_late_store_gpu.py): random ragged token vectors, the search restated in
numpy on top of the pairwise host rule (sc_diag_maxsim_host), and a host model of the store's live / dead bookkeeping."""
import ctypes as C

import numpy as np

from semcode_amd import _native


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def unit_rows(rng, n: int, W: int) -> np.ndarray:
    v = rng.standard_normal((n, W)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def key_of(v) -> np.ndarray:
    """maxsim_key of csrc/maxsim_rule.h: order-preserving, -0 < +0."""
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def pair_scores(questions, docs, W: int) -> np.ndarray:
    """[Bq, n] float32: sc_diag_maxsim_host of every (question, row that has tokens); NaN where the row has none."""
    n = len(docs)
    have = [r for r in range(n) if docs[r] is not None and len(docs[r])]
    out = np.full((len(questions), n), np.nan, np.float32)
    if not have:
        return out
    Q = np.ascontiguousarray(np.concatenate(questions), np.float32)
    q_off = np.concatenate(([0], np.cumsum([len(q) for q in questions]))).astype(np.int32)
    D = np.ascontiguousarray(np.concatenate([docs[r] for r in have]), np.float32)
    d_off = np.concatenate(([0], np.cumsum([len(docs[r]) for r in have]))).astype(np.int32)
    pq, pd = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(len(questions)), np.arange(len(have)), indexing="ij"))
    flat = np.full(len(pq), np.nan, np.float32)
    _native._check(_native.lib().sc_diag_maxsim_host(_p(Q), _p(q_off), len(questions), _p(D), _p(d_off), len(have), None, _p(pq), _p(pd), len(pq), W, _p(flat)))
    out[:, have] = flat.reshape(len(questions), len(have))
    return out


def search_restated(scores: np.ndarray, k: int, allow=None) -> "tuple[np.ndarray, np.ndarray]":
    """The search from a [Bq, n] score matrix (NaN: no tokens): larger key first, ties to the lower row, padded with -inf / -1."""
    Bq, n = scores.shape
    out_s = np.full((Bq, k), -np.inf, np.float32)
    out_r = np.full((Bq, k), -1, np.int64)
    ok = ~np.isnan(scores[0]) if n else np.zeros(0, bool)
    if allow is not None:
        ok &= np.asarray(allow, bool)
    rows = np.nonzero(ok)[0]
    for q in range(Bq):
        keys = key_of(scores[q, rows]).astype(np.int64)
        order = np.lexsort((rows, -keys))[:k]
        out_s[q, :len(order)] = scores[q, rows[order]]
        out_r[q, :len(order)] = rows[order]
    return out_s, out_r


class StoreModel:
    """The store's contents and its live / dead counts as the header states them: a put or a delete kills what the rows pointed to,
    and a compaction -- asked for, or by itself at the end of a put or delete that leaves dead > live -- sets dead to 0."""

    def __init__(self):
        self.docs = []
        self.live = self.dead = 0
        self.auto_compactions = 0

    def _settle(self):
        if self.dead > self.live:
            self.dead = 0
            self.auto_compactions += 1

    def append(self, n: int):
        self.docs += [None] * n

    def put(self, rows, toks):
        for r, t in zip(rows, toks):
            old = 0 if self.docs[r] is None else len(self.docs[r])
            new = 0 if t is None else len(t)
            self.live += new - old
            self.dead += old
            self.docs[r] = t if new else None
        self._settle()

    def delete(self, rows):
        gone = set(int(r) for r in rows)
        for r in gone:
            old = 0 if self.docs[r] is None else len(self.docs[r])
            self.live -= old
            self.dead += old
        self.docs = [d for r, d in enumerate(self.docs) if r not in gone]
        self._settle()

    def compact(self):
        self.dead = 0

    @property
    def rows_with_tokens(self) -> int:
        return sum(d is not None for d in self.docs)
