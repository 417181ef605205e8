// sc_ivf_plan.h -- the host planners of IVF probing, free of any device call: plain values in, plain tables out.  No HIP header and no
// sc_index here, so the CPU suite reaches them through sc_diag_ivf_plan (tests/test_ivf_plan_host.py).  The searches
// (sc_ivf_probe.cpp, sc_ivf_coarse.cpp) upload exactly these tables.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// Counting sort of items 0 .. n-1 by key(i) in [0, nkeys) (key < 0: the item is skipped): items[start[c] .. start[c + 1]) are the items
// of key c in ascending order (stable).
template <class Off, class Val, class Key>
static inline void sc_bucket_by_key(size_t n, size_t nkeys, Key&& key, std::vector<Off>& start, std::vector<Val>& items) {
    start.assign(nkeys + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t c = (int64_t)key(i);
        if (c >= 0) ++start[(size_t)c + 1];
    }
    for (size_t c = 0; c < nkeys; ++c) start[c + 1] += start[c];
    items.resize((size_t)start[nkeys]);
    std::vector<Off> cur(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; ++i) {
        const int64_t c = (int64_t)key(i);
        if (c >= 0) items[(size_t)cur[(size_t)c]++] = (Val)i;
    }
}

// What the planners read from the scan plan and the runtime (sc_ivf_plan_params, sc_ivf_probe.cpp, derives them).
struct IvfPlanParams {
    int k = 0;
    int qt = 16;          // queries per narrow group
    int qt_res = 16;      // narrow groups of more queries than this take the streamed-query scan (0: all of them)
    bool qstream = false; // the scan plan streams its queries (long rows)
    bool wide_cap = false;  // scan_listgemm_kernel serves (ld, k) next to a 16-query narrow scan ...
    bool wide_ok = false;   // ... and SC_IVF_WIDE does not switch it off
    int cus = 256;
    int KP = 512;         // candidates per query of the int8 stage (sc_batched_kprime8)
    bool (*merge_ok)(int lists_per_query, int k) = nullptr;  // sc_topk_gather_merge_supported
};

// ---- list-major probe -----------------------------------------------------------------------------------------------------------------
// One class of groups = one launch (the narrow class two: its first G_big groups on the streamed-query variant).
struct IvfGroupClass {
    int width = 0;                // query slots per group: 64, 32, qt
    int groups = 0;
    std::vector<int32_t> qmap;    // [groups][width] query of the slot, -1 beyond the group's queries
    std::vector<int64_t> sr;      // [groups][2] row range of the group
    int64_t streamed_rows() const {
        int64_t n = 0;
        for (size_t g = 0; g < sr.size(); g += 2) n += sr[g + 1] - sr[g];
        return n;
    }
};
struct IvfListMajorPlan {
    int maxparts = 1, L = 0;      // parts a list is cut into at most; k-lists a query merges = nprobe * maxparts
    std::vector<int32_t> src;     // [Q][L] slot of (query, probe j, part), -1: none
    IvfGroupClass cls[3];         // wide 64, wide 32, narrow -- in this order in `partial`
    std::vector<int> sb;          // narrow class: [groups][2] = (0, ceil(rows / 16))
    int G_big = 0;                // narrow groups on the streamed-query variant (they come first)
    int64_t lists_w = 0;          // k-lists of the wide classes
    int64_t target = 0, target_w = 0;  // rows per part, narrow / wide
    int64_t streamed_rows = 0, unique_rows = 0;
    int groups() const { return cls[0].groups + cls[1].groups + cls[2].groups; }
};
// probes [Q][nprobe] (entries outside [0, nlist) are skipped), list_off [nlist + 1]
void sc_ivf_plan_listmajor(const int64_t* probes, int Q, int nprobe, const int64_t* list_off, int nlist, const IvfPlanParams& pp, IvfListMajorPlan* out);

// ---- int8 coarse stage ----------------------------------------------------------------------------------------------------------------
static const int64_t IVFC_PREFIX = 4096;  // rows of one list that phase A takes (all of them are kept: cap > 2 KP + prefix)
struct IvfCoarseItem { long long row0; int rows; int slot_base; };  // one 256-row tile of a list x one group of 64 slots (ivf_coarse.hip)
static_assert(sizeof(IvfCoarseItem) == 16, "the item layout the coarse kernel reads");
struct IvfCoarsePlan {
    std::vector<int> ja;                             // [Q] probes of the query that phase A takes
    std::vector<unsigned> cntA;                      // [Q] rows of every query's phase-A ranges
    std::vector<int32_t> slot_q, slot_l, slot_dst;   // slot_dst (phase A): where the list's rows go in the query's survivor list
    std::vector<IvfCoarseItem> items[3];             // phase A | the rest of long phase-A lists | the other lists -- in this order in memory
    bool two_level = false;
    int64_t streamed_rows = 0, unique_rows = 0;
    size_t nitems() const { return items[0].size() + items[1].size() + items[2].size(); }
};
void sc_ivf_plan_coarse(const int64_t* probes, int Q, int nprobe, const int64_t* list_off, int nlist, const IvfPlanParams& pp, IvfCoarsePlan* out);

// ---- build ----------------------------------------------------------------------------------------------------------------------------
// Re-seeding between Lloyd iterations: (starved centroid, donor) pairs in the order they are applied; cnt [nlist] members per centroid
// of the ns sample rows.
std::vector<int32_t> sc_ivf_reseed_moves(const std::vector<int64_t>& cnt, int64_t ns);

// ---- cost model of the automatic choice -------------------------------------------------------------------------------------------------
// Is list-major probing estimated to be cheaper than the exhaustive paths?  n rows of ld floats, uncert_frac: share of queries the last
// batched exhaustive search re-ran exactly (< 0: never ran).
bool sc_ivf_listmajor_cheaper(const int64_t* list_off, int nlist, int64_t n, int ld, int Q, int nprobe, int qt, bool wide_cap, bool flat_is_batched,
                              double uncert_frac);
