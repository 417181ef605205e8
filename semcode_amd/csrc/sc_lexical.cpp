// sc_lexical.cpp -- the lexical and the hybrid search of the C ABI (sc_index_set_terms, sc_index_drop_terms, sc_index_lex_stats,
// sc_index_search_lexical*, sc_index_search_hybrid*, include/semcode_hip.h).  The term rows are the caller's data parked on the device
// in local row-number order, wherever an IVF layout put the vectors: never persisted, dropped by sc_index_delete_rows, valid while
// their row count equals the index's.  scan_lexical.hip streams them once per pass of 16 queries; the rules are lex_rule.h, which
// the two sc_diag_*_host functions at the end run on the CPU.  The library never computes an IDF: the caller turns df into weights.
#include <algorithm>
#include <cmath>
#include <vector>

#include "lex_rule.h"
#include "sc_internal.h"

static int g_lex_chunk_q = -1;  // sc_diag_set_option("lex_chunk_q", v): queries per chunk (-1: the default below)
void sc_set_lex_chunk_q(int v) { g_lex_chunk_q = v; }

static const int LEX_MAX_K = 128;      // the widest list: 64 KiB of a workgroup's LDS hold its 4 x 16 lists of 128 keys
static const int LEX_CHUNK_Q = 1024;   // queries per chunk: bounds the membership sets (8 KiB per 16 queries) and the candidate lists

static int chunk_q() { return g_lex_chunk_q > 0 ? g_lex_chunk_q : LEX_CHUNK_Q; }

void sc_lex_drop_locked(sc_index* ix) {
    ix->term_rows = -1;
    ix->term_T = 0;
    ix->lex_stat_dirty = true;
}

static sc_status check_terms_state(const sc_index* ix, const char* who) {
    if (ix->term_rows != ix->n)
        return sc_fail(SC_ERR_INVALID, "%s: no valid term rows -- installed for %lld rows (-1: none), the index has %lld; call sc_index_set_terms", who,
                       (long long)ix->term_rows, (long long)ix->n);
    return SC_OK;
}

extern "C" sc_status sc_index_set_terms(sc_index* ix, int64_t first_row, int64_t n, int32_t T, const uint16_t* terms) {
    if (!ix || n < 0 || first_row < 0 || (n > 0 && !terms)) return sc_fail(SC_ERR_INVALID, "sc_index_set_terms: bad argument");
    if (!lex_valid_T(T)) return sc_fail(SC_ERR_INVALID, "sc_index_set_terms: T must be 32, 64, 128 or 256 (got %d)", T);
    std::lock_guard<std::mutex> g(ix->mu);
    const int64_t held = ix->term_rows < 0 ? 0 : ix->term_rows;
    if (ix->term_rows >= 0 && T != ix->term_T) return sc_fail(SC_ERR_INVALID, "sc_index_set_terms: T=%d, the index holds rows of T=%d (sc_index_drop_terms first)", T, ix->term_T);
    if (first_row > held) return sc_fail(SC_ERR_INVALID, "sc_index_set_terms: first_row=%lld exceeds the %lld term rows held", (long long)first_row, (long long)held);
    if (first_row + n > ix->n)
        return sc_fail(SC_ERR_INVALID, "sc_index_set_terms: rows [%lld, %lld) for an index of %lld rows", (long long)first_row, (long long)(first_row + n), (long long)ix->n);
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    const size_t row_bytes = (size_t)T * 2;
    const int64_t rows_after = std::max(held, first_row + n);
    const size_t need = (size_t)rows_after * row_bytes + 1024;  // (a kilobyte of slack: the scan's last wave load is predicated, not padded)
    if (need > ix->terms.cap) {
        // grown with the rows held kept (sc_grow would lose them): to the index's capacity at least, so that appends do not copy every time
        const size_t want = std::max(need, std::max((size_t)ix->capacity * row_bytes + 1024, ix->terms.cap + ix->terms.cap / 2));
        sc_devbuf nb;
        if (nb.alloc(want) != hipSuccess) {
            (void)hipGetLastError();
            return sc_fail(SC_ERR_NOMEM, "sc_index_set_terms: cannot allocate %zu bytes for the term rows", want);
        }
        if (held > 0) SC_HIP(hipMemcpyAsync(nb.p, ix->terms.p, (size_t)held * row_bytes, hipMemcpyDeviceToDevice, s));
        SC_HIP(hipStreamSynchronize(s));
        sc_buf_free(ix->terms);
        ix->terms.p = nb.take<void>();
        ix->terms.cap = want;
    }
    if (n > 0) SC_HIP(hipMemcpyAsync(ix->terms.as<char>() + (size_t)first_row * row_bytes, terms, (size_t)n * row_bytes, hipMemcpyHostToDevice, s));
    SC_HIP(hipStreamSynchronize(s));  // (the caller's array may go once this returns)
    ix->term_rows = rows_after;
    ix->term_T = T;
    ix->lex_stat_dirty = true;
    return SC_OK;
}

extern "C" sc_status sc_index_drop_terms(sc_index* ix) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    SC_HIP(hipStreamSynchronize(ix->rt->stream));
    sc_lex_drop_locked(ix);
    sc_buf_free(ix->terms);
    return SC_OK;
}

extern "C" sc_status sc_index_lex_stats(sc_index* ix, int64_t* rows, int64_t* sum_dl, uint32_t* df) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    sc_status st = check_terms_state(ix, "sc_index_lex_stats");
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    const size_t df_bytes = (size_t)LEX_DF_SIZE * 4;
    if (!ix->lex_stat.p) {
        st = sc_grow(ix, ix->lex_stat, df_bytes + 16);
        if (st) return st;
        ix->lex_stat_dirty = true;
    }
    if (ix->lex_stat_dirty) {
        SC_HIP(hipMemsetAsync(ix->lex_stat.p, 0, df_bytes + 16, s));
        sc_with_prof(ix->rt, SC_PROF_SCAN, [&] {
            sc_launch_lex_stats(ix->terms.as<uint16_t>(), ix->term_rows, ix->term_T, ix->lex_stat.as<uint32_t>(), (unsigned long long*)(ix->lex_stat.as<char>() + df_bytes), s);
        });
        SC_HIP(hipGetLastError());
        ix->lex_stat_dirty = false;
    }
    unsigned long long sum = 0;
    if (df) SC_HIP(hipMemcpyAsync(df, ix->lex_stat.p, df_bytes, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(&sum, ix->lex_stat.as<char>() + df_bytes, 8, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    if (rows) *rows = ix->term_rows;
    if (sum_dl) *sum_dl = (int64_t)sum;
    return SC_OK;
}

struct LexParams {
    float k1, b, avgdl;
};

static sc_status check_lex_args(sc_index* ix, int32_t Q, int32_t k, const void* qt, const void* qw, const void* nt, const LexParams& p, const void* allow,
                                int64_t allow_words, const void* od, const void* orow, const char* who) {
    const sc_status st = sc_check_query_args(who, !ix || !qt || !qw || !nt || !od || !orow, Q, k, LEX_MAX_K);
    if (st) return st;
    if (!std::isfinite(p.k1) || !std::isfinite(p.b) || !std::isfinite(p.avgdl) || !(p.avgdl > 0.0f))
        return sc_fail(SC_ERR_INVALID, "%s: k1=%g, b=%g must be finite and avgdl=%g finite and > 0", who, (double)p.k1, (double)p.b, (double)p.avgdl);
    return sc_check_allow_null(who, allow, allow_words);
}
// (under the lock: the row counts are the index's)
static sc_status check_lex_state(const sc_index* ix, const void* allow, int64_t allow_words, const char* who) {
    const sc_status st = check_terms_state(ix, who);
    return st ? st : sc_check_allow_words(who, ix, allow, allow_words);
}
// the rules of a query's terms, checked on the host where the host holds them (the _dev forms leave it to lex_prep_kernel)
static sc_status check_queries_host(const uint16_t* qt, const float* qw, const int32_t* nt, int32_t Q, const char* who) {
    for (int32_t q = 0; q < Q; ++q) {
        const int32_t m = nt[q];
        if (m < 0 || m > LEX_MAX_QTERMS) return sc_fail(SC_ERR_INVALID, "%s: query %d has %d terms (0..%d)", who, q, m, LEX_MAX_QTERMS);
        for (int32_t j = 0; j < m; ++j) {
            const size_t o = (size_t)q * LEX_MAX_QTERMS + j;
            if (qt[o] == LEX_PAD || (j > 0 && qt[o - 1] >= qt[o]))
                return sc_fail(SC_ERR_INVALID, "%s: terms of query %d must be strictly ascending and below 0xFFFF (term %d = %u)", who, q, j, (unsigned)qt[o]);
            if (!lex_valid_weight(qw[o])) return sc_fail(SC_ERR_INVALID, "%s: weight %d of query %d must be finite and > 0 (got %g)", who, j, q, (double)qw[o]);
        }
    }
    return SC_OK;
}

// The scratch of one chunk of <= QC queries at width k (F: the hybrid search's two candidate lists on top).
struct LexScratch {
    uint32_t* memb;
    int32_t *nt_eff, *bad;
    uint64_t* partial;
    float *cd, *ld;
    int64_t *cr, *lr;
    int nwg;
};
static sc_status lex_scratch(sc_index* ix, int QC, int k, int F, LexScratch* out) {
    const int qp = sc_lex_queries_per_pass();
    out->nwg = sc_lex_scan_workgroups(ix->term_rows, ix->term_T, k, ix->rt->cus);
    const int lists = out->nwg * 4;
    sc_carver carve;
    const size_t o_memb = carve((size_t)((QC + qp - 1) / qp) * 2048 * 4), o_nt = carve((size_t)QC * 4), o_bad = carve(16),
                 o_part = carve((size_t)lists * qp * k * 8 + sc_topk_merge_scratch_bytes(lists, qp, k)), o_cd = carve((size_t)QC * F * 4), o_cr = carve((size_t)QC * F * 8),
                 o_ld = carve((size_t)QC * F * 4), o_lr = carve((size_t)QC * F * 8);
    const sc_status st = sc_grow(ix, ix->lex_scratch, carve.off);
    if (st) return st;
    char* b = ix->lex_scratch.as<char>();
    out->memb = (uint32_t*)(b + o_memb);
    out->nt_eff = (int32_t*)(b + o_nt);
    out->bad = (int32_t*)(b + o_bad);
    out->partial = (uint64_t*)(b + o_part);
    out->cd = (float*)(b + o_cd);
    out->cr = (int64_t*)(b + o_cr);
    out->ld = (float*)(b + o_ld);
    out->lr = (int64_t*)(b + o_lr);
    return SC_OK;
}

// One chunk of nq queries through the lexical scan: every argument device, outputs [nq, k].  The bad-query flag accumulates in *sc.bad.
static sc_status lexical_chunk_locked(sc_index* ix, const LexScratch& sc, int32_t nq, int32_t k, const uint16_t* qt, const float* qw, const int32_t* nt, const LexParams& p,
                                      const uint32_t* allow_dev, float* out_score, int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int qp = sc_lex_queries_per_pass();
    sc_with_prof(rt, SC_PROF_MERGE, [&] { sc_launch_lex_prep(qt, qw, nt, nq, sc.memb, sc.nt_eff, sc.bad, s); });
    for (int32_t q0 = 0; q0 < nq; q0 += qp) {
        const int32_t pq = std::min<int32_t>(qp, nq - q0);
        sc_with_prof(rt, SC_PROF_SCAN, [&] {
            sc_launch_lex_scan(ix->terms.as<uint16_t>(), ix->term_rows, ix->term_T, allow_dev, sc.memb + (size_t)(q0 / qp) * 2048, qt + (size_t)q0 * LEX_MAX_QTERMS,
                               qw + (size_t)q0 * LEX_MAX_QTERMS, sc.nt_eff + q0, pq, k, p.k1, p.b, p.avgdl, sc.nwg, sc.partial, s);
        });
        sc_with_prof(rt, SC_PROF_MERGE, [&] {
            sc_launch_topk_merge(SC_METRIC_IP, sc.partial, 1, sc.nwg * 4, qp, pq, k, ix->row_base, out_score + (size_t)q0 * k, out_rows + (size_t)q0 * k, s);
        });
        ix->last_lex_passes += 1;
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

static void lex_note_call(sc_index* ix) {
    ix->last_lex_rows = ix->term_rows;
    ix->last_lex_bytes = ix->term_rows * (int64_t)ix->term_T * 2;
    ix->last_lex_passes = 0;
}

// reads the bad-query flag back (synchronises): the kernels treated such a query as one without terms
static sc_status lex_check_bad(sc_index* ix, const int32_t* bad_dev, const char* who) {
    int32_t bad = 0;
    SC_HIP(hipMemcpyAsync(&bad, bad_dev, 4, hipMemcpyDeviceToHost, ix->rt->stream));
    SC_HIP(hipStreamSynchronize(ix->rt->stream));
    if (bad)
        return sc_fail(SC_ERR_INVALID, "%s: a query breaks the rules (0..%d terms, strictly ascending, below 0xFFFF, weights finite and > 0); its results are padding", who,
                       LEX_MAX_QTERMS);
    return SC_OK;
}

static sc_status search_lexical_locked(sc_index* ix, int32_t Q, int32_t k, const uint16_t* qt, const float* qw, const int32_t* nt, const LexParams& p,
                                       const uint32_t* allow_dev, float* out_score, int64_t* out_rows, const int32_t** bad_dev) {
    const int QC = std::min<int>(chunk_q(), Q);
    LexScratch sc;
    sc_status st = lex_scratch(ix, QC, k, 0, &sc);
    if (st) return st;
    lex_note_call(ix);
    SC_HIP(hipMemsetAsync(sc.bad, 0, 4, ix->rt->stream));
    for (int32_t q0 = 0; q0 < Q; q0 += QC) {
        st = lexical_chunk_locked(ix, sc, std::min<int32_t>(QC, Q - q0), k, qt + (size_t)q0 * LEX_MAX_QTERMS, qw + (size_t)q0 * LEX_MAX_QTERMS, nt + q0, p, allow_dev,
                                  out_score + (size_t)q0 * k, out_rows + (size_t)q0 * k);
        if (st) return st;
    }
    *bad_dev = sc.bad;
    ix->last_path = 9;
    return SC_OK;
}

static sc_status search_hybrid_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t F, const uint16_t* qt, const float* qw, const int32_t* nt,
                                      const LexParams& p, int32_t c, float wd, float wl, const uint32_t* allow_dev, float* out_score, int64_t* out_rows,
                                      const int32_t** bad_dev) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int64_t n = ix->n;
    const int QC = std::min<int>(chunk_q(), Q);
    LexScratch sc;
    sc_status st = lex_scratch(ix, QC, F, F, &sc);
    if (st) return st;
    lex_note_call(ix);
    SC_HIP(hipMemsetAsync(sc.bad, 0, 4, s));
    for (int32_t q0 = 0; q0 < Q; q0 += QC) {
        const int32_t nq = std::min<int32_t>(QC, Q - q0);
        const float* qc = q_dev + (size_t)q0 * ix->dim;
        // ---- the dense leg (the candidate stage) and the lexical leg at width fetch_k, then the fusion (an empty index: it writes the
        // padding alone)
        if (n > 0) {
            st = sc_candidates_locked(ix, qc, nq, F, allow_dev, sc.cd, sc.cr, nullptr, nullptr);
            if (st) return st;
            st = lexical_chunk_locked(ix, sc, nq, F, qt + (size_t)q0 * LEX_MAX_QTERMS, qw + (size_t)q0 * LEX_MAX_QTERMS, nt + q0, p, allow_dev, sc.ld, sc.lr);
            if (st) return st;
        }
        sc_with_prof(rt, SC_PROF_MERGE, [&] {
            sc_launch_lex_fuse(n > 0 ? sc.cr : nullptr, sc.lr, F, nq, k, c, wd, wl, out_score + (size_t)q0 * k, out_rows + (size_t)q0 * k, s);
        });
        SC_HIP(hipGetLastError());
    }
    *bad_dev = sc.bad;
    ix->last_path = 10;
    return SC_OK;
}

extern "C" sc_status sc_index_search_lexical_dev(sc_index* ix, int32_t Q, int32_t k, const uint16_t* qterms_dev, const float* qweights_dev, const int32_t* nterms_dev,
                                                 float k1, float b, float avgdl, const uint32_t* allow_dev, int64_t allow_words, float* out_score_dev,
                                                 int64_t* out_rows_dev) {
    const char* who = "lexical search";
    const LexParams p{k1, b, avgdl};
    sc_status st = check_lex_args(ix, Q, k, qterms_dev, qweights_dev, nterms_dev, p, allow_dev, allow_words, out_score_dev, out_rows_dev, who);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = check_lex_state(ix, allow_dev, allow_words, who);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    const int32_t* bad = nullptr;
    st = search_lexical_locked(ix, Q, k, qterms_dev, qweights_dev, nterms_dev, p, allow_dev, out_score_dev, out_rows_dev, &bad);
    if (st) return st;
    return lex_check_bad(ix, bad, who);
}

// The staging of the two host-pointer forms (q: the hybrid search's query vectors, or NULL), with the queries' terms uploaded into
// its extra region as [qterms | qweights | nterms].
struct LexQueries {
    uint16_t* qt;
    float* qw;
    int32_t* nt;
};
static sc_status lex_stage_queries(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint16_t* qterms, const float* qweights, const int32_t* nterms,
                                   const uint32_t* allow, sc_host_io* io, LexQueries* lq) {
    hipStream_t s = ix->rt->stream;
    const size_t qt_bytes = (size_t)Q * LEX_MAX_QTERMS * 2, qw_bytes = (size_t)Q * LEX_MAX_QTERMS * 4, nt_bytes = (size_t)Q * 4;
    sc_carver carve;
    const size_t o_qt = carve(qt_bytes), o_qw = carve(qw_bytes), o_nt = carve(nt_bytes);
    const sc_status st = sc_stage_host_locked(ix, q, Q, k, allow, carve.off, io);
    if (st) return st;
    lq->qt = (uint16_t*)(io->extra + o_qt);
    lq->qw = (float*)(io->extra + o_qw);
    lq->nt = (int32_t*)(io->extra + o_nt);
    SC_HIP(hipMemcpyAsync(lq->qt, qterms, qt_bytes, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(lq->qw, qweights, qw_bytes, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(lq->nt, nterms, nt_bytes, hipMemcpyHostToDevice, s));
    return SC_OK;
}

extern "C" sc_status sc_index_search_lexical(sc_index* ix, int32_t Q, int32_t k, const uint16_t* qterms, const float* qweights, const int32_t* nterms, float k1, float b,
                                             float avgdl, const uint32_t* allow, int64_t allow_words, float* out_score, int64_t* out_rows) {
    const char* who = "lexical search";
    const LexParams p{k1, b, avgdl};
    sc_status st = check_lex_args(ix, Q, k, qterms, qweights, nterms, p, allow, allow_words, out_score, out_rows, who);
    if (st) return st;
    st = check_queries_host(qterms, qweights, nterms, Q, who);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = check_lex_state(ix, allow, allow_words, who);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_host_io io;
    LexQueries lq;
    st = lex_stage_queries(ix, nullptr, Q, k, qterms, qweights, nterms, allow, &io, &lq);
    if (st) return st;
    const int32_t* bad = nullptr;
    st = search_lexical_locked(ix, Q, k, lq.qt, lq.qw, lq.nt, p, io.allow, io.dist, io.rows, &bad);
    if (st) return st;
    return sc_fetch_host_locked(ix, io, Q, k, out_score, out_rows);
}

static sc_status check_hybrid_args(const void* q, int32_t k, int32_t fetch_k, int32_t c, float wd, float wl) {
    const char* who = "hybrid search";
    if (!q) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (fetch_k > LEX_MAX_K) return sc_fail(SC_ERR_INVALID, "%s: fetch_k must be <= %d (got %d)", who, LEX_MAX_K, fetch_k);
    if (k > fetch_k) return sc_fail(SC_ERR_INVALID, "%s: top_k=%d exceeds fetch_k=%d", who, k, fetch_k);
    if (c < 1 || c > (1 << 30)) return sc_fail(SC_ERR_INVALID, "%s: c must be >= 1 (got %d)", who, c);
    if (!(wd >= 0.0f && wd < INFINITY) || !(wl >= 0.0f && wl < INFINITY))
        return sc_fail(SC_ERR_INVALID, "%s: the weights must be finite and >= 0 (got %g, %g)", who, (double)wd, (double)wl);
    return SC_OK;
}

extern "C" sc_status sc_index_search_hybrid_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t fetch_k, const uint16_t* qterms_dev,
                                                const float* qweights_dev, const int32_t* nterms_dev, float k1, float b, float avgdl, int32_t c, float wd, float wl,
                                                const uint32_t* allow_dev, int64_t allow_words, float* out_score_dev, int64_t* out_rows_dev) {
    const char* who = "hybrid search";
    const LexParams p{k1, b, avgdl};
    sc_status st = check_lex_args(ix, Q, k, qterms_dev, qweights_dev, nterms_dev, p, allow_dev, allow_words, out_score_dev, out_rows_dev, who);
    if (st) return st;
    st = check_hybrid_args(q_dev, k, fetch_k, c, wd, wl);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = check_lex_state(ix, allow_dev, allow_words, who);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    const int32_t* bad = nullptr;
    st = search_hybrid_locked(ix, q_dev, Q, k, fetch_k, qterms_dev, qweights_dev, nterms_dev, p, c, wd, wl, allow_dev, out_score_dev, out_rows_dev, &bad);
    if (st) return st;
    return lex_check_bad(ix, bad, who);
}

extern "C" sc_status sc_index_search_hybrid(sc_index* ix, const float* q, int32_t Q, int32_t k, int32_t fetch_k, const uint16_t* qterms, const float* qweights,
                                            const int32_t* nterms, float k1, float b, float avgdl, int32_t c, float wd, float wl, const uint32_t* allow,
                                            int64_t allow_words, float* out_score, int64_t* out_rows) {
    const char* who = "hybrid search";
    const LexParams p{k1, b, avgdl};
    sc_status st = check_lex_args(ix, Q, k, qterms, qweights, nterms, p, allow, allow_words, out_score, out_rows, who);
    if (st) return st;
    st = check_hybrid_args(q, k, fetch_k, c, wd, wl);
    if (st) return st;
    st = check_queries_host(qterms, qweights, nterms, Q, who);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = check_lex_state(ix, allow, allow_words, who);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_host_io io;
    LexQueries lq;
    st = lex_stage_queries(ix, q, Q, k, qterms, qweights, nterms, allow, &io, &lq);
    if (st) return st;
    const int32_t* bad = nullptr;
    st = search_hybrid_locked(ix, io.q, Q, k, fetch_k, lq.qt, lq.qw, lq.nt, p, c, wd, wl, io.allow, io.dist, io.rows, &bad);
    if (st) return st;
    return sc_fetch_host_locked(ix, io, Q, k, out_score, out_rows);
}

extern "C" sc_status sc_index_last_lex_stats(sc_index* ix, int64_t* rows_scanned, int64_t* bytes_per_pass, int32_t* passes) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (rows_scanned) *rows_scanned = ix->last_lex_rows;
    if (bytes_per_pass) *bytes_per_pass = ix->last_lex_bytes;
    if (passes) *passes = ix->last_lex_passes;
    return SC_OK;
}

// ---- the two rules on the CPU: the same header the kernels compile (tests on a machine without a GPU)
extern "C" sc_status sc_diag_lex_score_host(const uint16_t* terms, int64_t n, int32_t T, const uint16_t* qterms, const float* qweights, int32_t m, float k1, float b,
                                            float avgdl, float* out_score, uint8_t* out_hit) {
    const char* who = "sc_diag_lex_score_host";
    if (n < 0 || (n > 0 && (!terms || !out_score || !out_hit)) || (m > 0 && (!qterms || !qweights))) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    if (!lex_valid_T(T)) return sc_fail(SC_ERR_INVALID, "%s: T must be 32, 64, 128 or 256 (got %d)", who, T);
    const int32_t one = m;
    const sc_status st = check_queries_host(qterms, qweights, &one, 1, who);
    if (st) return st;
    for (int64_t r = 0; r < n; ++r) {
        float s = 0.0f;
        out_hit[r] = lex_score_row(terms + (size_t)r * T, T, qterms, qweights, m, k1, b, avgdl, &s) ? 1 : 0;
        out_score[r] = s;
    }
    return SC_OK;
}

extern "C" sc_status sc_diag_rrf_host(const int64_t* dense_rows, const int64_t* lex_rows, int32_t F, int32_t k, int32_t c, float wd, float wl, float* out_score,
                                      int64_t* out_rows) {
    const char* who = "sc_diag_rrf_host";
    if (!dense_rows || !lex_rows || !out_score || !out_rows) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (F < 1 || F > LEX_MAX_K || k < 1 || k > F) return sc_fail(SC_ERR_INVALID, "%s: need 1 <= k <= F <= %d (got %d, %d)", who, LEX_MAX_K, k, F);
    const sc_status st = check_hybrid_args(dense_rows, k, F, c, wd, wl);
    if (st) return st;
    std::vector<std::pair<float, int64_t>> cand;
    for (int i = 0; i < F; ++i) {
        if (dense_rows[i] < 0) continue;
        int rl = -1;
        for (int j = 0; j < F; ++j)
            if (lex_rows[j] == dense_rows[i]) rl = j;
        cand.push_back({lex_rrf(wd, wl, c, i, rl), dense_rows[i]});
    }
    for (int j = 0; j < F; ++j) {
        if (lex_rows[j] < 0 || std::find(dense_rows, dense_rows + F, lex_rows[j]) != dense_rows + F) continue;
        cand.push_back({lex_rrf(wd, wl, c, -1, j), lex_rows[j]});
    }
    std::sort(cand.begin(), cand.end(), [](const auto& x, const auto& y) { return lex_before(x.first, x.second, y.first, y.second); });
    for (int i = 0; i < k; ++i) {
        const bool have = i < (int)cand.size();
        out_score[i] = have ? cand[(size_t)i].first : -INFINITY;
        out_rows[i] = have ? cand[(size_t)i].second : -1;
    }
    return SC_OK;
}
