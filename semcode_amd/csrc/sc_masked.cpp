// sc_masked.cpp -- the masked search of the C ABI (sc_index_search_masked*, include/semcode_hip.h): a per-call bitset over local row
// numbers -> mask_compact -> the gathered exact scan (scan_masked.hip) -> topk_merge.hip.  The index learns nothing about what the
// bits mean, stores nothing per row for them, and no other search path reads anything written here except last_path.
#include <algorithm>

#include "sc_internal.h"

static int g_mask_gather = 0;  // sc_diag_set_option("mask_gather", 1): the gathered kernel answers even when every row is allowed (tests)
void sc_set_mask_gather(int v) { g_mask_gather = v; }

static const char* const WHO = "masked search";
static const int MASK_MAX_K = 1024;  // the widest list of the exact scan

// q_dev tight [Q, dim], allow_dev >= ceil(n / 32) words, outputs [Q, k]: all device.  Synchronises the stream once (the allowed count).
sc_status sc_search_masked_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev, float* out_dist, int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int64_t n = ix->n;
    ix->last_mask_allowed = ix->last_mask_scanned = 0;
    ix->last_mask_gathered = 0;
    // stored position -> row id is valid below `mapped` (the lists of a trained IVF_FLAT index; further where a search extended it over
    // the tail with the identity, which is what positions beyond it mean anyway)
    const int64_t mapped = std::min(n, sc_perm_entries(ix));
    int64_t m = 0;
    if (n > 0) {
        const int64_t nb = sc_mask_blocks(n);
        sc_status st = sc_grow(ix, ix->mask_cnt, (size_t)((n + 63) / 64) * 8 + (size_t)(nb + 1) * 4);
        if (st) return st;
        st = sc_grow(ix, ix->mask_sel, (size_t)((n + 15) / 16 * 16) * 4);
        if (st) return st;
        uint64_t* flags = ix->mask_cnt.as<uint64_t>();
        uint32_t* cnt = (uint32_t*)(flags + (n + 63) / 64);
        sc_launch_mask_count(allow_dev, n, ix->perm, mapped, flags, cnt, s);
        SC_HIP(hipGetLastError());
        uint32_t m32 = 0;
        SC_HIP(hipMemcpyAsync(&m32, cnt + nb, 4, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        m = (int64_t)m32;
    }
    ix->last_mask_allowed = m;
    if (m == n && n > 0 && !g_mask_gather) {
        // every row allowed: the exhaustive planner (same bits; the batched path for large batches)
        ix->last_mask_scanned = n;
        return sc_search_exhaustive_locked(ix, q_dev, Q, k, out_dist, out_rows);
    }
    ScanPlan plan;
    // force_qt = 16: the resident-query variant whatever the row length
    if (!sc_scan_exact_plan(ix->ld, Q, k, rt->cus, &plan, 16, 0, std::max<int64_t>(m, 1)))
        return sc_fail(SC_ERR_UNSUPPORTED, "masked search: k=%d (1..1024) / dim=%d not supported by the exact scan", k, ix->dim);
    sc_status st = sc_grow(ix, ix->partial, std::max<size_t>(plan.partial_bytes, 16));
    if (st) return st;
    uint64_t* partial = ix->partial.as<uint64_t>();
    if (m > 0) {
        st = sc_prep_queries(ix, q_dev, Q);
        if (st) return st;
        const uint64_t* flags = ix->mask_cnt.as<uint64_t>();
        const uint32_t* cnt = (const uint32_t*)(flags + (n + 63) / 64);
        sc_launch_mask_scatter(flags, cnt, n, ix->mask_sel.as<uint32_t>(), s);
        sc_with_prof(rt, SC_PROF_SCAN, [&] {
            sc_launch_scan_gather((int)ix->metric, ix->X, ix->xnorm, ix->ld, ix->qpad.as<float>(), ix->qnorm.as<float>(), Q, k, plan, partial, ix->perm, mapped,
                                  ix->mask_sel.as<uint32_t>(), m, s);
        });
        ix->last_mask_scanned = m;
        ix->last_mask_gathered = 1;
    }
    // (no allowed row, or an empty index: no lists -- the merge writes the -1 / +-inf padding alone)
    sc_with_prof(rt, SC_PROF_MERGE, [&] { sc_launch_topk_merge((int)ix->metric, partial, plan.groups, m > 0 ? plan.lists : 0, plan.qt, Q, k, ix->row_base, out_dist, out_rows, s); });
    SC_HIP(hipGetLastError());
    ix->last_path = 6;
    return SC_OK;
}

extern "C" sc_status sc_index_search_masked_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev, int64_t allow_words,
                                                float* out_dist_dev, int64_t* out_rows_dev) {
    sc_status st = sc_check_query_args(WHO, !ix || !q_dev || !allow_dev || !out_dist_dev || !out_rows_dev, Q, k, MASK_MAX_K);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = sc_check_allow_words(WHO, ix, allow_dev, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    return sc_search_masked_locked(ix, q_dev, Q, k, allow_dev, out_dist_dev, out_rows_dev);
}

extern "C" sc_status sc_index_search_masked(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint32_t* allow, int64_t allow_words, float* out_dist,
                                            int64_t* out_rows) {
    sc_status st = sc_check_query_args(WHO, !ix || !q || !allow || !out_dist || !out_rows, Q, k, MASK_MAX_K);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = sc_check_allow_words(WHO, ix, allow, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_host_io io;
    st = sc_stage_host_locked(ix, q, Q, k, allow, 0, &io);
    if (st) return st;
    st = sc_search_masked_locked(ix, io.q, Q, k, io.allow, io.dist, io.rows);
    if (st) return st;
    return sc_fetch_host_locked(ix, io, Q, k, out_dist, out_rows);
}

extern "C" sc_status sc_index_last_mask_stats(sc_index* ix, int64_t* allowed_rows, int64_t* scanned_rows, int32_t* gathered) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (allowed_rows) *allowed_rows = ix->last_mask_allowed;
    if (scanned_rows) *scanned_rows = ix->last_mask_scanned;
    if (gathered) *gathered = ix->last_mask_gathered;
    return SC_OK;
}
