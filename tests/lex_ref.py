"""numpy / pure-Python restatement of the lexical and hybrid search rules (include/semcode_hip.h, "Hybrid search"), written from
the definition and independent of semcode_amd/csrc/lex_rule.h: the extractor, the BM25 score one rounded f32 operation at a time,
the order of hits, and the weighted reciprocal-rank fusion.  Shared by tests/test_lexical_host.py and tests/test_lexical_gpu.py."""
import re

import numpy as np

PAD = 0xFFFF
MAX_QTERMS = 32
F32 = np.float32

_RUN = re.compile(rb"[A-Za-z0-9_\x80-\xff]+")


def _kind(c: int) -> str:
    if 0x61 <= c <= 0x7A:
        return "l"
    if 0x41 <= c <= 0x5A:
        return "u"
    if 0x30 <= c <= 0x39:
        return "d"
    return "o"  # >= 0x80: a letter without case


def _boundary(a: int, b: int) -> bool:
    ka, kb = _kind(a), _kind(b)
    letter = ("l", "u", "o")
    return (ka == "l" and kb == "u") or (ka in letter and kb == "d") or (ka == "d" and kb in letter)


def tokens(text) -> list:
    """The emitted tokens of a text in text order (lower-cased, cut to 64 bytes, those shorter than 2 bytes dropped)."""
    data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    out = []

    def emit(tok: bytes) -> None:
        if len(tok) >= 2:
            out.append(bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in tok[:64]))

    for m in _RUN.finditer(data):
        run = m.group()
        emit(run)
        parts, cur = [], b""
        split = False
        for i, c in enumerate(run):
            if c == 0x5F:
                split = True
                parts.append(cur)
                cur = b""
                continue
            cur += bytes([c])
            if i + 1 < len(run) and run[i + 1] != 0x5F and _boundary(c, run[i + 1]):
                split = True
                parts.append(cur)
                cur = b""
        parts.append(cur)
        if split:
            for p in parts:
                emit(p)
    return out


def term_hash(tok: bytes) -> int:
    h = 2166136261
    for c in tok:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    f = (h ^ (h >> 16)) & 0xFFFF
    return 0xFFFE if f == PAD else f


def term_rows(texts, T: int):
    """(terms [n, T] uint16, dl [n] int32) of these texts."""
    terms = np.full((len(texts), T), PAD, dtype=np.uint16)
    dl = np.zeros(len(texts), dtype=np.int32)
    for i, t in enumerate(texts):
        hs = sorted(term_hash(tok) for tok in tokens(t)[:T])
        terms[i, : len(hs)] = hs
        dl[i] = len(hs)
    return terms, dl


def score_rows(terms: np.ndarray, qt, qw, k1, b, avgdl):
    """One query against every row: (score [n] f32, hit [n] bool).  Every line below is one rounded f32 operation per element."""
    terms = np.asarray(terms, dtype=np.uint16)
    k1, b, avgdl = F32(k1), F32(b), F32(avgdl)
    dl = (terms != PAD).sum(axis=1).astype(F32)
    x = (b * dl).astype(F32)
    x = (x / avgdl).astype(F32)
    x = ((F32(1.0) - b).astype(F32) + x).astype(F32)
    K = (k1 * x).astype(F32)
    k1p = F32(k1 + F32(1.0))
    score = np.zeros(terms.shape[0], dtype=F32)
    hit = np.zeros(terms.shape[0], dtype=bool)
    for t, w in zip(np.asarray(qt).tolist(), np.asarray(qw, dtype=F32)):
        tf = (terms == t).sum(axis=1)
        on = tf > 0
        tff = tf.astype(F32)
        num = (F32(w) * (tff * k1p).astype(F32)).astype(F32)
        den = (tff + K).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (num / den).astype(F32)
        score = np.where(on, (score + c).astype(F32), score)
        hit |= on
    return score, hit


def topk(score: np.ndarray, hit: np.ndarray, k: int, allow=None):
    """Larger score first, ties to the lower row; rows that are no hits (or not allowed) never appear; padded with -1 / -inf."""
    ok = hit if allow is None else hit & np.asarray(allow, dtype=bool)
    rows = np.flatnonzero(ok)
    order = rows[np.lexsort((rows, -score[rows].astype(np.float64)))][:k]
    out_s = np.full(k, -np.inf, dtype=F32)
    out_r = np.full(k, -1, dtype=np.int64)
    out_s[: order.size] = score[order]
    out_r[: order.size] = order
    return out_s, out_r


def search(terms, qterms, qweights, nterms, k, k1, b, avgdl, allow=None):
    """The batch: qterms / qweights [Q, 32], nterms [Q] -> (score [Q, k], rows [Q, k])."""
    Q = len(nterms)
    S = np.empty((Q, k), dtype=F32)
    R = np.empty((Q, k), dtype=np.int64)
    for q in range(Q):
        m = int(nterms[q])
        s, h = score_rows(terms, qterms[q][:m], qweights[q][:m], k1, b, avgdl)
        S[q], R[q] = topk(s, h, k, allow)
    return S, R


def rrf(dense_rows, lex_rows, k: int, c: int = 60, wd=1.0, wl=1.0):
    """Two best-first row lists (-1 = padding) -> the k best fused (score [k] f32, rows [k]); dense term first, missing rank = 0."""
    wd, wl = F32(wd), F32(wl)
    dense = [int(r) for r in dense_rows]
    lex = [int(r) for r in lex_rows]
    rank_l = {r: i for i, r in enumerate(lex) if r >= 0}
    rank_d = {r: i for i, r in enumerate(dense) if r >= 0}
    cand = {}
    for r in list(rank_d) + list(rank_l):
        fd = F32(wd / F32(c + rank_d[r])) if r in rank_d else F32(0.0)
        fl = F32(wl / F32(c + rank_l[r])) if r in rank_l else F32(0.0)
        cand[r] = F32(fd + fl)
    order = sorted(cand, key=lambda r: (-float(cand[r]), r))[:k]
    out_s = np.full(k, -np.inf, dtype=F32)
    out_r = np.full(k, -1, dtype=np.int64)
    for i, r in enumerate(order):
        out_s[i], out_r[i] = cand[r], r
    return out_s, out_r


def stats(terms: np.ndarray):
    """(rows, sum_dl, df [65536] uint32) of term rows."""
    terms = np.asarray(terms, dtype=np.uint16)
    df = np.zeros(65536, dtype=np.uint32)
    for row in terms:
        u = np.unique(row)
        df[u[u != PAD]] += 1
    return terms.shape[0], int((terms != PAD).sum()), df


def idf(df: np.ndarray, n: int) -> np.ndarray:
    """ln(1 + (N - df + 0.5) / (df + 0.5)) in float64, rounded to f32."""
    d = np.asarray(df, dtype=np.float64)
    return np.log(1.0 + (n - d + 0.5) / (d + 0.5)).astype(F32)


def query_terms(text, df: np.ndarray, n: int, T: int = 128):
    """The store's query-term selection: the distinct terms of the text's first T tokens, the at most 32 with the highest IDF (ties to
    the lower term), ascending -> (qterms [32] uint16 padded with 0xFFFF, qweights [32] f32 padded with 0, m)."""
    ts = sorted({term_hash(t) for t in tokens(text)[:T]})
    w = idf(df, n)
    ts = [t for t in ts if w[t] > 0 and np.isfinite(w[t])]
    keep = sorted(sorted(ts, key=lambda t: (-float(w[t]), t))[:MAX_QTERMS])
    qt = np.full(MAX_QTERMS, PAD, dtype=np.uint16)
    qw = np.zeros(MAX_QTERMS, dtype=F32)
    qt[: len(keep)] = keep
    qw[: len(keep)] = [w[t] for t in keep]
    return qt, qw, len(keep)
