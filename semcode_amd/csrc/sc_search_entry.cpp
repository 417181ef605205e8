// sc_search_entry.cpp -- what the search entry points of the C ABI share (sc_search.cpp, sc_masked.cpp, sc_grouped.cpp, sc_mmr.cpp,
// sc_lexical.cpp): the argument checks, the staging of a host-pointer call, and the dense candidate stage of the features that pick
// from a best-first list.  Declared in sc_internal.h.
#include <algorithm>

#include "sc_internal.h"

sc_status sc_check_query_args(const char* who, bool any_null, int32_t Q, int32_t k, int32_t k_max) {
    if (any_null) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (Q < 1 || Q > (1 << 20)) return sc_fail(SC_ERR_INVALID, "%s: Q=%d out of range", who, Q);
    if (k_max <= 0 && k < 1) return sc_fail(SC_ERR_INVALID, "%s: top_k must be >= 1 (got %d)", who, k);
    if (k_max > 0 && (k < 1 || k > k_max)) return sc_fail(SC_ERR_INVALID, "%s: top_k must be 1..%d (got %d)", who, k_max, k);
    return SC_OK;
}

sc_status sc_check_allow_null(const char* who, const void* allow, int64_t allow_words) {
    if (!allow && allow_words != 0) return sc_fail(SC_ERR_INVALID, "%s: allow is NULL but allow_words=%lld", who, (long long)allow_words);
    return SC_OK;
}

sc_status sc_check_allow_words(const char* who, const sc_index* ix, const void* allow, int64_t allow_words) {
    const int64_t need = (ix->n + 31) / 32;
    if (allow && allow_words < need)
        return sc_fail(SC_ERR_INVALID, "%s: allow_words=%lld, %lld rows need %lld", who, (long long)allow_words, (long long)ix->n, (long long)need);
    return SC_OK;
}

// ix->io = [queries | dist | rows | extra], ix->mask_words = the allow words; both grown before the first upload into either
sc_status sc_stage_host_locked(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint32_t* allow, size_t extra_bytes, sc_host_io* io) {
    hipStream_t s = ix->rt->stream;
    const size_t q_bytes = q ? (size_t)Q * ix->dim * 4 : 0;
    const size_t words = allow ? (size_t)((ix->n + 31) / 32) : 0;  // bits beyond the rows are never read
    sc_carver carve;
    const size_t o_q = carve(std::max<size_t>(q_bytes, 16)), o_d = carve((size_t)Q * k * 4), o_r = carve((size_t)Q * k * 8), o_x = carve(extra_bytes);
    sc_status st = sc_grow(ix, ix->io, carve.off);
    if (st) return st;
    if (allow) {
        st = sc_grow(ix, ix->mask_words, std::max<size_t>(words * 4, 16));
        if (st) return st;
    }
    char* b = ix->io.as<char>();
    io->q = (float*)(b + o_q);
    io->dist = (float*)(b + o_d);
    io->rows = (int64_t*)(b + o_r);
    io->extra = b + o_x;
    io->allow = allow ? ix->mask_words.as<uint32_t>() : nullptr;
    if (q_bytes) SC_HIP(hipMemcpyAsync(io->q, q, q_bytes, hipMemcpyHostToDevice, s));
    if (words) SC_HIP(hipMemcpyAsync(ix->mask_words.p, allow, words * 4, hipMemcpyHostToDevice, s));
    return SC_OK;
}

sc_status sc_fetch_host_locked(sc_index* ix, const sc_host_io& io, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows) {
    hipStream_t s = ix->rt->stream;
    SC_HIP(hipMemcpyAsync(out_dist, io.dist, (size_t)Q * k * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(out_rows, io.rows, (size_t)Q * k * 8, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

// A trained index is scanned as it lies: its position map is extended over the tail with the identity (the exhaustive paths need
// every position mapped), the tail itself stays a tail.
sc_status sc_search_exhaustive_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows) {
    const sc_status st = sc_ivf_cover_tail_locked(ix);
    if (st) return st;
    return sc_search_flat_locked(ix, q_dev, Q, k, out_dist, out_rows);
}

sc_status sc_candidates_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t W, const uint32_t* allow_dev, float* cand_dist, int64_t* cand_rows, int64_t* scanned,
                               int64_t* allowed) {
    const sc_status st = allow_dev ? sc_search_masked_locked(ix, q_dev, Q, W, allow_dev, cand_dist, cand_rows) : sc_search_exhaustive_locked(ix, q_dev, Q, W, cand_dist, cand_rows);
    if (st) return st;
    if (scanned) *scanned = allow_dev ? ix->last_mask_scanned : ix->n;
    if (allowed) *allowed = allow_dev ? ix->last_mask_allowed : ix->n;
    return SC_OK;
}
