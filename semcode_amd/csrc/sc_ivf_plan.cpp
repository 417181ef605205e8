// sc_ivf_plan.cpp -- the host planners of IVF probing (sc_ivf_plan.h): no device call, no HIP header.
#include "sc_ivf_plan.h"

#include <algorithm>
#include <cmath>
#include <utility>

// ---- list-major probing for query batches ------------------------------------------------------------------------
// The (query, list) pairs are bucketed by list, every list is streamed once per group of queries that probe it (one row range per
// group, the group's queries gathered through qmap), and a query's top-k is merged from the (group, slot) lists it took part in.
namespace {
// The next chunk of a list's queries when `left` of them are in no group yet: wide chunks (scan_listgemm_kernel) of up to 64 while more
// than qt remain -- 17 .. 32 left take the 32-slot form of the kernel: half the time --, each streamed ONCE with 2-4 x the arithmetic
// per row byte (the matrix pipe, not the row stream, bounds it); then narrow ones of up to qt.  width 0: narrow.
struct Chunk { int nq, width; };
inline Chunk next_chunk(int left, int qt, bool wide_ok) {
    if (!wide_ok || left <= qt) return {std::min(qt, left), 0};
    const int nq = std::min(64, left);
    return {nq, nq > 32 ? 64 : 32};
}
}  // namespace

void sc_ivf_plan_listmajor(const int64_t* probes, int Q, int nprobe, const int64_t* list_off, int nlist, const IvfPlanParams& pp, IvfListMajorPlan* out) {
    const int qt = pp.qt;
    const bool wide_ok = pp.wide_ok;
    // the pairs by list (the queries of a list in ascending order: deterministic groups)
    std::vector<int> start;
    std::vector<int32_t> pair_of;
    sc_bucket_by_key((size_t)Q * nprobe, (size_t)nlist, [&](size_t i) { return probes[i] < nlist ? probes[i] : -1; }, start, pair_of);
    // long lists are cut into parts of at most `target` rows (each part its own group) so that no single workgroup streams a
    // 20k-row list while the others idle; a query then merges up to nprobe * maxparts partial lists
    int64_t work_rows = 0, work_rows_w = 0, longest = 0;
    for (int l = 0; l < nlist; ++l) {
        const int m = start[(size_t)l + 1] - start[(size_t)l];
        const int64_t len = list_off[(size_t)l + 1] - list_off[(size_t)l];
        if (m == 0 || len <= 0) continue;
        int mw = 0, mn = 0;  // wide chunks of this list in units of a 32-query chunk's time (a 64-query one takes twice that), narrow chunks
        for (int c = 0; c < m;) {
            const Chunk ch = next_chunk(m - c, qt, wide_ok);
            if (ch.width) mw += ch.width / 32; else ++mn;
            c += ch.nq;
        }
        work_rows_w += len * mw / 2;
        work_rows += len * mn;
        longest = std::max(longest, len);
    }
    // parts: ~8 narrow groups per CU (each streams at the LDS-DMA rate), ~6 wide ones (each 2.5 x longer per row)
    int64_t target = std::min<int64_t>(8192, std::max<int64_t>(512, work_rows / ((int64_t)pp.cus * 8)));
    target = (target + 15) & ~(int64_t)15;
    int64_t target_w = std::min<int64_t>(8192, std::max<int64_t>(512, work_rows_w / ((int64_t)pp.cus * 6)));
    target_w = (target_w + 63) & ~(int64_t)63;
    auto parts_of = [&](int64_t len) { return (int)std::max<int64_t>((len + target - 1) / target, wide_ok ? (len + target_w - 1) / target_w : 0); };
    int maxparts = std::max(1, parts_of(longest));
    while (maxparts > 1 && !pp.merge_ok(nprobe * maxparts, pp.k)) {  // merge capacity: fewer, longer parts
        target *= 2;
        target_w *= 2;
        maxparts = std::max(1, parts_of(longest));
    }
    const int L = nprobe * maxparts;
    out->maxparts = maxparts;
    out->L = L;
    out->target = target;
    out->target_w = target_w;
    out->src.assign((size_t)Q * L, -1);
    out->cls[0].width = 64, out->cls[1].width = 32, out->cls[2].width = qt;
    // With the streamed-query scan (long rows, qt = 16) a group of few queries is still better off on the resident variant,
    // which streams ~30 % faster: groups are numbered in classes -- the wide ones first (64, then 32 query slots), then those
    // with more queries than fit resident (qt_res), then the small ones -- and each class gets its own launch.
    // Within a class the longest parts go first: one workgroup streams one group, and a 100 MB part that starts in the last
    // round would leave the other CUs idle for its whole length (stable sort: the numbering stays deterministic).
    struct GroupDesc { int l, c, nqg, part; int64_t p0, p1; };
    std::vector<GroupDesc> descs;
    for (int ci = 0; ci < 4; ++ci) {  // wide 64, wide 32, narrow / streamed queries, narrow / resident queries (one table: the two narrow classes)
        IvfGroupClass& gc = out->cls[std::min(ci, 2)];
        if (ci == 2) out->lists_w = (int64_t)out->cls[0].groups * 64 + (int64_t)out->cls[1].groups * 32;  // the wide k-lists come first in `partial`
        if (ci == 3) out->G_big = gc.groups;
        const int64_t table_base = ci == 0 ? 0 : ci == 1 ? (int64_t)out->cls[0].groups * 64 : out->lists_w;
        descs.clear();
        for (int l = 0; l < nlist; ++l) {
            const int64_t first = list_off[(size_t)l], end = list_off[(size_t)l + 1];
            const int m = start[(size_t)l + 1] - start[(size_t)l];
            if (m == 0 || end <= first) continue;  // nobody probes it / empty list
            for (int c = 0; c < m;) {
                const Chunk ch = next_chunk(m - c, qt, wide_ok);
                if ((ch.width == 64 ? 0 : ch.width == 32 ? 1 : ch.nq > pp.qt_res ? 2 : 3) == ci) {
                    const int64_t tg = ch.width ? target_w : target;
                    for (int64_t p0 = first, part = 0; p0 < end; p0 += tg, ++part) descs.push_back({l, c, ch.nq, (int)part, p0, std::min(end, p0 + tg)});
                }
                c += ch.nq;
            }
        }
        std::stable_sort(descs.begin(), descs.end(), [](const GroupDesc& x, const GroupDesc& y) { return x.p1 - x.p0 > y.p1 - y.p0; });
        for (const GroupDesc& d : descs) {
            const int64_t base = table_base + (int64_t)gc.groups * gc.width;
            for (int sl = 0; sl < gc.width; ++sl) {
                if (sl < d.nqg) {
                    const int32_t pair = pair_of[(size_t)start[(size_t)d.l] + d.c + sl];
                    const int q = pair / nprobe, j = pair - q * nprobe;
                    gc.qmap.push_back(q);
                    out->src[(size_t)q * L + (size_t)j * maxparts + d.part] = (int32_t)(base + sl);
                } else {
                    gc.qmap.push_back(-1);
                }
            }
            gc.sr.push_back(d.p0);
            gc.sr.push_back(d.p1);
            if (ci >= 2) {
                out->sb.push_back(0);
                out->sb.push_back((int)((d.p1 - d.p0 + 15) >> 4));
            }
            ++gc.groups;
        }
    }
    for (const IvfGroupClass& gc : out->cls) out->streamed_rows += gc.streamed_rows();
    for (int l = 0; l < nlist; ++l)
        if (start[(size_t)l + 1] > start[(size_t)l]) out->unique_rows += list_off[(size_t)l + 1] - list_off[(size_t)l];
}

// ---- list-major probing behind an int8 coarse stage ------------------------------------------------------------------------------------
// Phase A = every query's nearest list(s) -- of a long list only its first IVFC_PREFIX rows: any subset gives a valid
// bound, and phase A keeps every row it sees --, phase B = the other lists and what is left of the phase-A lists; per kind the pairs are
// bucketed by list (queries in ascending order: deterministic), cut into groups of 64 slots, and every group meets every 256-row
// tile of its row range.
void sc_ivf_plan_coarse(const int64_t* probes, int Q, int nprobe, const int64_t* list_off, int nlist, const IvfPlanParams& pp, IvfCoarsePlan* out) {
    typedef IvfCoarseItem Item;
    const int KP = pp.KP;
    const size_t npairs = (size_t)Q * nprobe;
    std::vector<int32_t>&slot_q = out->slot_q, &slot_l = out->slot_l, &slot_dst = out->slot_dst;
    std::vector<unsigned>& cntA = out->cntA;
    cntA.assign((size_t)Q, 0u);
    std::vector<Item>* items = out->items;
    int64_t streamed_rows = 0, unique_rows = 0;
    std::vector<char> touched((size_t)nlist, 0);
    auto list_len = [&](int64_t l) { return list_off[(size_t)l + 1] - list_off[(size_t)l]; };
    // phase A of a query = its nearest lists until they hold 2 KP rows (one list unless the lists are small): enough candidates
    // for a tight bound, which phase B needs -- at +inf every row of the other lists would survive
    std::vector<int>& ja = out->ja;
    ja.assign((size_t)Q, 1);
    // the (query, list) entries: phase A takes the list (of a long one its prefix, and phase B the rest: a tail), or phase B the whole list
    enum : char { NONE, A, A_LONG, B };
    std::vector<char> entry(npairs, NONE);
    std::vector<int32_t> q_of(npairs);
    for (int q = 0; q < Q; ++q) {
        const int64_t* pq = probes + (size_t)q * nprobe;
        int64_t cum = 0;
        int j = 0;
        while (j < nprobe && cum < 2 * (int64_t)KP) {
            const int64_t l = pq[j];
            if (l >= 0 && l < nlist) cum += std::min<int64_t>(list_len(l), IVFC_PREFIX);
            ++j;
        }
        ja[(size_t)q] = j;
        for (int i = 0; i < nprobe; ++i) {
            const int64_t l = pq[i];
            q_of[(size_t)q * nprobe + i] = q;
            if (l >= 0 && l < nlist) entry[(size_t)q * nprobe + i] = i >= j ? B : list_len(l) > IVFC_PREFIX ? A_LONG : A;
        }
    }
    std::vector<int> group_bases;
    // the three kinds of entries -- 0: phase A (prefix of the list); 1: phase B, whole list; 2: phase B, the rest of a phase-A list --
    // by list, the queries of a list in ascending order
    std::vector<int> start3[3];
    std::vector<int32_t> pairs3[3];
    for (int kind = 0; kind < 3; ++kind)
        sc_bucket_by_key(npairs, (size_t)nlist, [&](size_t i) {
            const char e = entry[i];
            return (kind == 0 ? e == A || e == A_LONG : kind == 1 ? e == B : e == A_LONG) ? probes[i] : -1;
        }, start3[kind], pairs3[kind]);
    slot_q.reserve(npairs * 2 + 64);
    slot_l.reserve(npairs * 2 + 64);
    slot_dst.reserve(npairs * 2 + 64);
    int64_t rows_kind[3] = {0, 0, 0};
    for (int kind : {0, 2, 1}) {  // (in this order in memory: the tails form a launch of their own when the bound has two levels)
        const std::vector<int>& start = start3[kind];
        const std::vector<int32_t>& pairs = pairs3[kind];
        if (start[(size_t)nlist] == 0) continue;
        const int ph = kind == 0 ? 0 : kind == 2 ? 1 : 2;
        for (int l = 0; l < nlist; ++l) {
            const int m = start[(size_t)l + 1] - start[(size_t)l];
            const int64_t lfirst = list_off[(size_t)l], lend = list_off[(size_t)l + 1];
            const int64_t first = kind == 2 ? lfirst + IVFC_PREFIX : lfirst, end = kind == 0 ? std::min(lend, lfirst + IVFC_PREFIX) : lend;
            if (m == 0 || end <= first) continue;
            if (!touched[(size_t)l]) { touched[(size_t)l] = 1; unique_rows += lend - lfirst; }
            group_bases.clear();
            for (int c = 0; c < m; c += 64) {
                const int nq = std::min(64, m - c);
                const int slot_base = (int)slot_q.size();
                for (int sl = 0; sl < 64; ++sl) {
                    const int q = sl < nq ? q_of[(size_t)pairs[(size_t)start[(size_t)l] + c + sl]] : -1;
                    slot_q.push_back(q);
                    slot_l.push_back(sl < nq ? l : -1);
                    int32_t dst = 0;
                    if (ph == 0 && q >= 0) {
                        dst = (int32_t)((uint32_t)cntA[(size_t)q] - (uint32_t)first);  // position of stored row r: (uint32)(r + dst)
                        cntA[(size_t)q] = (unsigned)std::min<int64_t>((int64_t)cntA[(size_t)q] + (end - first), (int64_t)1 << 30);
                    }
                    slot_dst.push_back(dst);
                }
                group_bases.push_back(slot_base);
                streamed_rows += end - first;
                rows_kind[kind] += (end - first) * nq;
            }
            // items of one list: blocks of 8 row tiles, every group's copy of a block right behind the previous group's -- the persistent
            // grid hands item i to workgroup i mod grid, workgroups 8 apart share an XCD, so the groups of a popular list stream a
            // tile through the same L2 at the same time instead of one XCD after the other
            for (int64_t b0 = first; b0 < end; b0 += 8 * 256)
                for (const int base : group_bases)
                    for (int64_t r0 = b0; r0 < end && r0 < b0 + 8 * 256; r0 += 256) items[ph].push_back({(long long)r0, (int)std::min<int64_t>(256, end - r0), base});
        }
    }
    // Long lists (the reference's nlist = 128: tens of thousands of rows each): the bound from a 4 096-row prefix of the nearest list is
    // loose, and against it the REST of that list -- where most neighbours are -- overflows the survivor lists (10M x 768, nlist 128:
    // 65 of 1 024 queries).  Then the bound gets a second level: the tails run first, their 128 best lower bounds are re-scored too,
    // and the other lists meet the bound of both samples.
    out->two_level = !items[1].empty() && rows_kind[2] * 4 >= rows_kind[0];
    out->streamed_rows = streamed_rows;
    out->unique_rows = unique_rows;
}

// Re-seeding (every iteration but the last, so that final centroids are plain means).  Strided initialisation leaves
// some true clusters without a centroid and gives others two; Lloyd iterations cannot repair that, and in high
// dimension the orphaned clusters all fall to one "hub" centroid near the global mean (measured on config 5: one list
// of 124k rows at a median of 2.4k, list-major probing reading the corpus 26 times over).  So starved centroids
// (count < 0.75 average, smallest first) are moved onto the largest ones (count > 2 average, largest first, sizes
// halved on every split), as faiss does for empty clusters.  Integer rule + in-order moves: restated exactly by
// oracle/ivf_oracle.py.
std::vector<int32_t> sc_ivf_reseed_moves(const std::vector<int64_t>& cnt, int64_t ns) {
    const int nlist = (int)cnt.size();
    std::vector<int> donors((size_t)nlist);
    for (int c = 0; c < nlist; ++c) donors[(size_t)c] = c;
    std::stable_sort(donors.begin(), donors.end(), [&](int a, int b) { return cnt[(size_t)a] < cnt[(size_t)b]; });
    auto less_big = [](const std::pair<int64_t, int>& a, const std::pair<int64_t, int>& b) {
        return a.first != b.first ? a.first < b.first : a.second > b.second;  // max-heap: larger size, then lower id
    };
    std::vector<std::pair<int64_t, int>> heap;
    for (int c = 0; c < nlist; ++c)
        if (cnt[(size_t)c] * nlist > 2 * ns) heap.emplace_back(cnt[(size_t)c], c);
    std::make_heap(heap.begin(), heap.end(), less_big);
    std::vector<int32_t> moves;
    for (int di = 0; di < nlist && !heap.empty(); ++di) {
        const int e = donors[(size_t)di];
        if (cnt[(size_t)e] * 4 * nlist >= 3 * ns) break;
        std::pop_heap(heap.begin(), heap.end(), less_big);
        const std::pair<int64_t, int> big = heap.back();
        heap.pop_back();
        if (big.first * nlist <= 2 * ns) break;
        moves.push_back(e);
        moves.push_back(big.second);
        const int64_t half = big.first / 2;
        heap.emplace_back(big.first - half, big.second);
        std::push_heap(heap.begin(), heap.end(), less_big);
        heap.emplace_back(half, e);
        std::push_heap(heap.begin(), heap.end(), less_big);
    }
    return moves;
}

// Probe while that is estimated to be cheaper than the exhaustive paths (which return exact results).
// Queries follow the data, so a list is expected to receive (query, list) pairs in proportion to its length:
// work = sum over lists of len * groups(len).  The batched exhaustive path re-runs uncertified queries through the exact
// scan, which on clustered data (what an IVF index is trained on) can be most of them: its share at the last such search
// on this index is fed back (10 % assumed before the first).  Constants measured on MI355X (profiles/r1q_ivf_*.log):
// list-major streams 5.5 TB/s after 1.5 ms of coarse probe + planning; batched exhaustive 1.0 PFLOP/s + 1 ms; exact
// scan 6 TB/s per pass of qt queries.
bool sc_ivf_listmajor_cheaper(const int64_t* list_off_h, int nlist, int64_t rows, int ld, int Q, int nprobe, int qt, bool wide_ok, bool flat_is_batched,
                              double uncert_frac) {
    const double n = (double)rows, row_bytes = (double)ld * 4.0, pairs = (double)Q * nprobe;
    // a list expected to be wanted by m queries: chunks of 64 on the GEMM-shaped kernel (f32 MFMA bound: 2 * 64 * ld FLOP per row at
    // ~100 TFLOP/s, profiles/r2m_kernel_stats.csv), a remainder of <= 16 on the 16-query scan (row stream at 5.5 TB/s)
    const double t_row_narrow = row_bytes / 5.5e12, t_row_wide = 2.0 * 64.0 * (double)ld / 1.0e14;
    double t_scan = 0.0;
    for (int l = 0; l < nlist; ++l) {
        const double len = (double)(list_off_h[(size_t)l + 1] - list_off_h[(size_t)l]);
        if (len <= 0) continue;
        double m = std::max(1.0, std::ceil(pairs * len / n));
        if (wide_ok && m > qt) {
            const double chunks = std::floor(m / 64.0), rest = m - 64.0 * chunks;
            t_scan += len * t_row_wide * (chunks + (rest > qt ? (rest > 32.0 ? 1.0 : 0.5) : 0.0));
            m = rest > qt ? 0.0 : rest;
        }
        t_scan += len * t_row_narrow * std::ceil(m / qt);
    }
    const double t_lm = t_scan + 1.5e-3;
    const double t_pass = n * row_bytes / 6.0e12;
    double t_flat;
    if (flat_is_batched) {
        const double redo = (uncert_frac < 0 ? 0.1 : uncert_frac) * Q;
        t_flat = std::max(2.0 * n * ld * Q / 1.0e15, n * ld * 2.0 / 5.0e12) + 1.0e-3 + std::ceil(redo / qt) * t_pass;
    } else {
        t_flat = std::ceil((double)Q / qt) * t_pass;
    }
    return t_lm < t_flat;
}
