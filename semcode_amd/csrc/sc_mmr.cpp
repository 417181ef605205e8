// sc_mmr.cpp -- the MMR search of the C ABI (sc_index_search_mmr*, include/semcode_hip.h): diversified top-k by maximal marginal
// relevance, exact.  The candidates come from the existing searches -- sc_candidates_locked at width fetch_k -- and scan_mmr.hip
// scores them against each other and runs the greedy selection of mmr_rule.h.  Nothing is kept between calls:
// the row -> position map of a trained index is rebuilt per call into the scratch.
#include <algorithm>
#include <cmath>
#include <vector>

#include "mmr_rule.h"
#include "sc_internal.h"

static int g_mmr_chunk_q = -1;  // sc_diag_set_option("mmr_chunk_q", v): queries per pass (-1: the default below)
void sc_set_mmr_chunk_q(int v) { g_mmr_chunk_q = v; }

static const int MMR_MAX_FETCH = 128;  // the widest candidate list: the planner's fast paths take it, and its score matrix is 64 KiB
static const int MMR_CHUNK_Q = 1024;   // queries per pass: bounds the score matrices (64 KiB per query at fetch_k = 128)

static const char* const WHO = "mmr search";

static int chunk_q() { return g_mmr_chunk_q > 0 ? g_mmr_chunk_q : MMR_CHUNK_Q; }

static sc_status check_mmr_args(sc_index* ix, const void* q, int32_t Q, int32_t k, int32_t fetch_k, float lambda, const void* allow, int64_t allow_words, const void* od,
                                const void* orow) {
    const sc_status st = sc_check_query_args(WHO, !ix || !q || !od || !orow, Q, k, 0);
    if (st) return st;
    if (fetch_k > MMR_MAX_FETCH) return sc_fail(SC_ERR_INVALID, "mmr search: fetch_k must be <= %d (got %d)", MMR_MAX_FETCH, fetch_k);
    if (k > fetch_k) return sc_fail(SC_ERR_INVALID, "mmr search: top_k=%d exceeds fetch_k=%d", k, fetch_k);
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return sc_fail(SC_ERR_INVALID, "mmr search: lambda must be within [0, 1] (got %g)", (double)lambda);
    return sc_check_allow_null(WHO, allow, allow_words);
}

// q_dev tight [Q, dim], allow_dev NULL or >= ceil(n / 32) words, outputs [Q, k]: all device.
static sc_status search_mmr_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t F, float lambda, const uint32_t* allow_dev, float* out_dist,
                                   int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int64_t n = ix->n;
    const int metric = (int)ix->metric;
    const int Fp = (F + 15) & ~15;
    const int QC = std::min<int>(chunk_q(), Q);
    ix->last_mmr_fetch = F;
    ix->last_mmr_scanned = 0;
    ix->mmr_stat_pending = false;

    sc_carver carve;
    const size_t o_cd = carve((size_t)QC * F * 4), o_cr = carve((size_t)QC * F * 8), o_g = carve((size_t)QC * Fp * Fp * 4),
                 o_inv = carve(ix->perm ? (size_t)n * 4 + 16 : 16);
    sc_status st = sc_grow(ix, ix->mmr_scratch, carve.off);
    if (st) return st;
    st = sc_grow(ix, ix->mmr_stat, 16);
    if (st) return st;
    char* b = ix->mmr_scratch.as<char>();
    float *cd = (float*)(b + o_cd), *G = (float*)(b + o_g);
    int64_t* cr = (int64_t*)(b + o_cr);
    uint32_t* inv = (uint32_t*)(b + o_inv);
    int32_t* min_count = ix->mmr_stat.as<int32_t>();
    SC_HIP(hipMemsetAsync(min_count, 0x7f, 4, s));  // (a large count; the selection takes the minimum over the queries)

    bool have_inv = false;
    for (int32_t q0 = 0; q0 < Q; q0 += QC) {
        const int32_t nq = std::min<int32_t>(QC, Q - q0);
        const float* qc = q_dev + (size_t)q0 * ix->dim;
        float* od = out_dist + (size_t)q0 * k;
        int64_t* orow = out_rows + (size_t)q0 * k;
        // ---- candidates: the candidate stage at width fetch_k
        int64_t scanned = 0, allowed = 0;
        if (n > 0) {
            st = sc_candidates_locked(ix, qc, nq, F, allow_dev, cd, cr, &scanned, &allowed);
            if (st) return st;
            ix->last_mmr_scanned += scanned;
        }
        if (allowed > 0) {
            // ---- candidate rows -> stored positions (list-major storage only; once per call, after a search may have extended perm)
            if (ix->perm && !have_inv) {
                sc_with_prof(rt, SC_PROF_MERGE, [&] { sc_launch_mmr_inverse(ix->perm, std::min(n, sc_perm_entries(ix)), n, inv, s); });
                have_inv = true;
            }
            sc_with_prof(rt, SC_PROF_SCAN, [&] { sc_launch_mmr_gram(metric, ix->X, ix->xnorm, ix->ld, n, ix->row_base, ix->perm ? inv : nullptr, cr, F, nq, G, s); });
        }
        // (an empty index: no candidate stage, the selection writes the -1 / +-inf padding alone)
        sc_with_prof(rt, SC_PROF_MERGE, [&] { sc_launch_mmr_select(metric, cd, n > 0 ? cr : nullptr, F, G, nq, k, lambda, od, orow, min_count, s); });
        SC_HIP(hipGetLastError());
    }
    ix->mmr_stat_pending = true;
    ix->last_path = 8;
    return SC_OK;
}

extern "C" sc_status sc_index_search_mmr_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t fetch_k, float lambda, const uint32_t* allow_dev,
                                             int64_t allow_words, float* out_dist_dev, int64_t* out_rows_dev) {
    sc_status st = check_mmr_args(ix, q_dev, Q, k, fetch_k, lambda, allow_dev, allow_words, out_dist_dev, out_rows_dev);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = sc_check_allow_words(WHO, ix, allow_dev, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    return search_mmr_locked(ix, q_dev, Q, k, fetch_k, lambda, allow_dev, out_dist_dev, out_rows_dev);
}

extern "C" sc_status sc_index_search_mmr(sc_index* ix, const float* q, int32_t Q, int32_t k, int32_t fetch_k, float lambda, const uint32_t* allow, int64_t allow_words,
                                         float* out_dist, int64_t* out_rows) {
    sc_status st = check_mmr_args(ix, q, Q, k, fetch_k, lambda, allow, allow_words, out_dist, out_rows);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = sc_check_allow_words(WHO, ix, allow, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_host_io io;
    st = sc_stage_host_locked(ix, q, Q, k, allow, 0, &io);
    if (st) return st;
    st = search_mmr_locked(ix, io.q, Q, k, fetch_k, lambda, io.allow, io.dist, io.rows);
    if (st) return st;
    return sc_fetch_host_locked(ix, io, Q, k, out_dist, out_rows);
}

extern "C" sc_status sc_index_last_mmr_stats(sc_index* ix, int32_t* fetch_k, int32_t* min_candidates, int64_t* rows_scanned) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (fetch_k) *fetch_k = ix->last_mmr_fetch;
    if (rows_scanned) *rows_scanned = ix->last_mmr_scanned;
    if (min_candidates) {
        int32_t c = 0;
        if (ix->mmr_stat_pending && ix->mmr_stat.p) {  // the one host read of the feature, paid by whoever asks
            SC_HIP(hipSetDevice(ix->rt->device));
            SC_HIP(hipMemcpyAsync(&c, ix->mmr_stat.p, 4, hipMemcpyDeviceToHost, ix->rt->stream));
            SC_HIP(hipStreamSynchronize(ix->rt->stream));
        }
        *min_candidates = c;
    }
    return SC_OK;
}

// The selection rule on the CPU: the same header the kernel compiles (tests on a machine without a GPU).
extern "C" sc_status sc_diag_mmr_select_host(const float* rel, const float* G, int32_t C, int32_t ldg, int32_t k, float lambda, int32_t* picked) {
    if (!rel || !G || !picked) return sc_fail(SC_ERR_INVALID, "sc_diag_mmr_select_host: NULL argument");
    if (C < 1 || ldg < C || k < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_mmr_select_host: need C >= 1, ldg >= C, k >= 1 (got %d, %d, %d)", C, ldg, k);
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return sc_fail(SC_ERR_INVALID, "sc_diag_mmr_select_host: lambda must be within [0, 1] (got %g)", (double)lambda);
    std::vector<float> m((size_t)C);
    std::vector<unsigned char> taken((size_t)C);
    mmr_select_seq(rel, G, C, ldg, k, lambda, m.data(), taken.data(), picked);
    return SC_OK;
}
