// sc_grouped.cpp -- the grouped search of the C ABI (sc_index_set_groups, sc_index_search_grouped*, include/semcode_hip.h): at most one
// hit per label, exact.  The scores come from the existing searches -- sc_candidates_locked at a candidate width -- and
// scan_grouped.hip picks the first row of every label out of their best-first lists.  Queries whose list ran out before
// k labels go on in rounds: their hit labels are excluded by a bitset and the masked search answers over what is left.
// The labels are the caller's data parked on the device: never interpreted, never persisted, dropped by sc_index_delete_rows.
#include <algorithm>
#include <vector>

#include "sc_internal.h"

static int g_group_width0 = -1, g_group_width1 = -1;  // sc_diag_set_option("group_width0" / "group_width1", v): candidate widths (-1: the defaults below)
void sc_set_group_width0(int v) { g_group_width0 = v; }
void sc_set_group_width1(int v) { g_group_width1 = v; }

static const int GROUP_MAX_K = 128;     // hit labels a workgroup of group_exclude_kernel sorts in LDS
static const int GROUP_MAX_W = 1024;    // the widest list group_select_kernel takes = the widest top_k of the masked search
static const int GROUP_CHUNK_Q = 4096;  // queries per pass: bounds the candidate lists (12 B * width per query)

// Round 0 asks for more than k candidates, but stays within what the planner's fast paths take: 64 for the plain batched form, 128
// for its wide form.  Results do not depend on either width.
static int width0(int k) {
    if (g_group_width0 > 0) return std::min(GROUP_MAX_W, std::max(k, g_group_width0));
    return std::max(k, std::min(std::max(32, 4 * k), k <= 64 ? 64 : 128));
}
// Exclusion rounds: max(64, 4 k) candidates in the first, 256 from then on.  The masked scan they run gets slow with its width -- one
// query over 9.5M x 768 rows: top-10 4.7 ms, top-64 4.9, top-256 6.3, top-1024 45 (profiles/grouped_bench_10Mx768.log) -- so four
// rounds at 256 cost less than one at 1 024 and see as many candidates.
static int width1(int k, int round) {
    if (g_group_width1 > 0) return std::min(GROUP_MAX_W, g_group_width1);
    return round > 1 ? 256 : std::min(256, std::max(64, 4 * k));
}

static const char* const WHO = "grouped search";

static sc_status check_grouped_args(sc_index* ix, const void* q, int32_t Q, int32_t k, const void* allow, int64_t allow_words, const void* od, const void* orow) {
    const sc_status st = sc_check_query_args(WHO, !ix || !q || !od || !orow, Q, k, GROUP_MAX_K);
    return st ? st : sc_check_allow_null(WHO, allow, allow_words);
}
// (under the lock: the row count is the index's)
static sc_status check_grouped_state(const sc_index* ix, const void* allow, int64_t allow_words) {
    if (ix->group_rows != ix->n)
        return sc_fail(SC_ERR_INVALID, "grouped search: no valid labels -- installed for %lld rows (-1: none), the index has %lld; call sc_index_set_groups",
                       (long long)ix->group_rows, (long long)ix->n);
    return sc_check_allow_words(WHO, ix, allow, allow_words);
}

// One pass of <= GROUP_CHUNK_Q queries.  q_dev tight [Q, dim], allow_dev NULL or >= ceil(n / 32) words, outputs [Q, k]: all device.
static sc_status grouped_chunk_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev, float* out_dist, int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int64_t n = ix->n;
    const int metric = (int)ix->metric;
    const int W0 = width0(k), W1max = GROUP_MAX_W;
    const int32_t* labels = ix->groups.as<int32_t>();
    sc_carver carve;
    const size_t o_cd = carve((size_t)Q * W0 * 4), o_cr = carve((size_t)Q * W0 * 8), o_cd1 = carve((size_t)W1max * 4), o_cr1 = carve((size_t)W1max * 8),
                 o_lab = carve((size_t)Q * k * 4), o_cnt = carve((size_t)Q * 4), o_done = carve((size_t)Q * 4), o_excl = carve((size_t)((n + 31) / 32) * 4 + 16);
    sc_status st = sc_grow(ix, ix->group_scratch, carve.off);
    if (st) return st;
    char* b = ix->group_scratch.as<char>();
    float *cd = (float*)(b + o_cd), *cd1 = (float*)(b + o_cd1);
    int64_t *cr = (int64_t*)(b + o_cr), *cr1 = (int64_t*)(b + o_cr1);
    int32_t *found = (int32_t*)(b + o_lab), *cnt = (int32_t*)(b + o_cnt), *done = (int32_t*)(b + o_done);
    uint32_t* excl = (uint32_t*)(b + o_excl);

    // ---- round 0: the candidate stage at width W0 (run on an empty index too: the selection reads the padding it writes)
    int64_t scanned = 0;
    st = sc_candidates_locked(ix, q_dev, Q, W0, allow_dev, cd, cr, &scanned, nullptr);
    if (st) return st;
    ix->last_group_scanned += scanned;
    sc_with_prof(rt, SC_PROF_MERGE, [&] { sc_launch_group_select(metric, cd, cr, W0, Q, labels, n, ix->row_base, k, true, out_dist, out_rows, found, cnt, done, s); });
    SC_HIP(hipGetLastError());
    // the host's one read per round: the done flags
    std::vector<int32_t> hdone((size_t)Q);
    SC_HIP(hipMemcpyAsync(hdone.data(), done, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    std::vector<int> pending;
    for (int i = 0; i < Q; ++i)
        if (!hdone[(size_t)i]) pending.push_back(i);
    ix->last_group_continued += (int)pending.size();

    // ---- rounds >= 1: one query at a time over the rows whose label it has not found yet; every round finds a new label or ends the query
    for (int round = 1; !pending.empty(); ++round) {
        if (round > k + 1) return sc_fail(SC_ERR_STATE, "grouped search: %d queries not finished after %d rounds", (int)pending.size(), round - 1);
        const int W1 = width1(k, round);
        for (const int qi : pending) {
            sc_launch_group_exclude(labels, n, allow_dev, found + (size_t)qi * k, cnt + qi, excl, rt->cus, s);
            st = sc_search_masked_locked(ix, q_dev + (size_t)qi * ix->dim, 1, W1, excl, cd1, cr1);
            if (st) return st;
            sc_with_prof(rt, SC_PROF_MERGE, [&] {
                sc_launch_group_select(metric, cd1, cr1, W1, 1, labels, n, ix->row_base, k, false, out_dist + (size_t)qi * k, out_rows + (size_t)qi * k, found + (size_t)qi * k,
                                       cnt + qi, done + qi, s);
            });
            ix->last_group_rounds += 1;
            ix->last_group_scanned += ix->last_mask_scanned;
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(hdone.data(), done, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        std::vector<int> still;
        for (const int qi : pending)
            if (!hdone[(size_t)qi]) still.push_back(qi);
        pending.swap(still);
    }
    return SC_OK;
}

static sc_status search_grouped_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev, float* out_dist, int64_t* out_rows) {
    ix->last_group_width0 = width0(k);
    ix->last_group_continued = ix->last_group_rounds = 0;
    ix->last_group_scanned = 0;
    for (int32_t q0 = 0; q0 < Q; q0 += GROUP_CHUNK_Q) {
        const sc_status st = grouped_chunk_locked(ix, q_dev + (size_t)q0 * ix->dim, std::min(GROUP_CHUNK_Q, Q - q0), k, allow_dev, out_dist + (size_t)q0 * k,
                                                  out_rows + (size_t)q0 * k);
        if (st) return st;
    }
    ix->last_path = 7;
    return SC_OK;
}

extern "C" sc_status sc_index_set_groups(sc_index* ix, const int32_t* labels, int64_t n) {
    if (!ix || n < 0 || (n > 0 && !labels)) return sc_fail(SC_ERR_INVALID, "sc_index_set_groups: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (n != ix->n) return sc_fail(SC_ERR_INVALID, "sc_index_set_groups: %lld labels for an index of %lld rows", (long long)n, (long long)ix->n);
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    ix->group_rows = -1;
    const sc_status st = sc_grow(ix, ix->groups, std::max<size_t>((size_t)n * 4, 16));
    if (st) return st;
    if (n > 0) SC_HIP(hipMemcpyAsync(ix->groups.p, labels, (size_t)n * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipStreamSynchronize(s));  // (the caller's array may go once this returns)
    ix->group_rows = n;
    return SC_OK;
}

extern "C" sc_status sc_index_search_grouped_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev, int64_t allow_words,
                                                 float* out_dist_dev, int64_t* out_rows_dev) {
    sc_status st = check_grouped_args(ix, q_dev, Q, k, allow_dev, allow_words, out_dist_dev, out_rows_dev);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = check_grouped_state(ix, allow_dev, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    return search_grouped_locked(ix, q_dev, Q, k, allow_dev, out_dist_dev, out_rows_dev);
}

extern "C" sc_status sc_index_search_grouped(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint32_t* allow, int64_t allow_words, float* out_dist,
                                             int64_t* out_rows) {
    sc_status st = check_grouped_args(ix, q, Q, k, allow, allow_words, out_dist, out_rows);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    st = check_grouped_state(ix, allow, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_host_io io;
    st = sc_stage_host_locked(ix, q, Q, k, allow, 0, &io);
    if (st) return st;
    st = search_grouped_locked(ix, io.q, Q, k, io.allow, io.dist, io.rows);
    if (st) return st;
    return sc_fetch_host_locked(ix, io, Q, k, out_dist, out_rows);
}

extern "C" sc_status sc_index_last_group_stats(sc_index* ix, int32_t* first_width, int32_t* queries_continued, int32_t* rounds, int64_t* rows_scanned) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (first_width) *first_width = ix->last_group_width0;
    if (queries_continued) *queries_continued = ix->last_group_continued;
    if (rounds) *rounds = ix->last_group_rounds;
    if (rows_scanned) *rows_scanned = ix->last_group_scanned;
    return SC_OK;
}
