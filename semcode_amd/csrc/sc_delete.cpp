// sc_delete.cpp -- sc_index_delete_rows: in-place compaction of every per-row array of an index (compact.hip has the chunk scheme and
// its hazard argument).
#include <algorithm>
#include <vector>

#include "sc_internal.h"

static int64_t g_delete_chunk_rows = 0;  // sc_diag_set_option("delete_chunk_rows", n): at most n positions per chunk (0: as many as the bounce buffer holds) -- tests of the multi-chunk path
void sc_set_delete_chunk_rows(int v) { g_delete_chunk_rows = v < 0 ? 0 : v; }
static const size_t DELETE_BOUNCE_BYTES = (size_t)192 << 20;  // + 8 B per position of a chunk (<= 8 MiB) + the tile sums: below 256 MiB for any corpus

namespace {
// entries of the sorted list below x
inline int64_t rank_below(const std::vector<int64_t>& sorted, int64_t x) { return (int64_t)(std::lower_bound(sorted.begin(), sorted.end(), x) - sorted.begin()); }
// v (values in [0, n)) ascending; false if a value repeats.  Large lists are sorted by marking: one pass over n flags instead of
// n log n compares (3M random positions of a 10M-row index: 15 ms instead of 250).
bool sort_distinct(std::vector<int64_t>& v, int64_t n) {
    if (std::adjacent_find(v.begin(), v.end(), [](int64_t a, int64_t b) { return a >= b; }) == v.end()) return true;  // strictly ascending already (a filter over the rows)
    if ((int64_t)v.size() * 16 < n) {
        std::sort(v.begin(), v.end());
        return std::adjacent_find(v.begin(), v.end()) == v.end();
    }
    std::vector<uint8_t> mark((size_t)n, 0);
    for (const int64_t r : v) {
        if (mark[(size_t)r]) return false;
        mark[(size_t)r] = 1;
    }
    size_t w = 0;
    for (int64_t r = 0; r < n; ++r)
        if (mark[(size_t)r]) v[w++] = r;
    return true;
}
// a pending-work list after the delete: entries of deleted rows dropped, the rest renumbered
void remap_pending(std::vector<int64_t>& v, const std::vector<int64_t>& del) {
    size_t w = 0;
    for (const int64_t r : v) {
        const int64_t below = rank_below(del, r);
        if (below < (int64_t)del.size() && del[(size_t)below] == r) continue;
        v[w++] = r - below;
    }
    v.resize(w);
}
// --- the delete's view of a shadow
// mirrors rows that are there: its arrays are moved with the corpus.  The centred shadow mirrors the list layout: all of it or nothing
bool shadow_valid(const sc_index* ix, const sc_shadow& sh) {
    for (int i = 0; i < 2; ++i)
        if (sh.row_bytes[i] && !sh.arr[i].p) return false;
    return sh.rows > 0 && (&sh != &ix->sh_c8 || (ix->perm && sh.rows == ix->ivf_rows));
}
// one past the last padding row its build zeroed in an index of n rows, bounded by what is allocated
int64_t shadow_padded_end(const sc_index* ix, const sc_shadow& sh, int64_t n) {
    int64_t end = &sh == &ix->sh_c8 ? (sh.rows + 255) / 256 * 256 + sh.tail_pad : (n + 255) / 256 * 256;
    for (int i = 0; i < 2; ++i)
        if (sh.row_bytes[i]) end = std::min<int64_t>(end, (int64_t)(sh.arr[i].cap / sh.row_bytes[i]));
    return end;
}
}  // namespace

extern "C" sc_status sc_index_delete_rows(sc_index* ix, const int64_t* rows, int64_t n) {
    if (!ix || n < 0 || (n > 0 && !rows)) return sc_fail(SC_ERR_INVALID, "sc_index_delete_rows: bad argument");
    if (n == 0) return SC_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    // ---- validate everything before anything changes
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= ix->n) return sc_fail(SC_ERR_INVALID, "sc_index_delete_rows: rows[%lld] = %lld out of range [0,%lld)", (long long)i, (long long)rows[i], (long long)ix->n);
    std::vector<int64_t> ids(rows, rows + n);
    if (!sort_distinct(ids, ix->n)) return sc_fail(SC_ERR_INVALID, "sc_index_delete_rows: row numbers must be distinct");
    ix->group_rows = -1;  // the rows are renumbered: the caller's group labels (sc_index_set_groups) no longer name them
    sc_lex_drop_locked(ix);  // ... and neither do its term rows (sc_index_set_terms)
    hipStream_t s = ix->rt->stream;
    const int64_t old_n = ix->n, ld = ix->ld;
    const bool listed = ix->perm != nullptr;  // trained layout installed: stored position != row id below ivf_rows
    int valid_before = 0;
    for (const sc_shadow* sh : ix->shadows)
        if (shadow_valid(ix, *sh)) valid_before |= sh->stat_bit;
    if (n == old_n) {  // nothing survives: a fresh index (the lists go, the quantizer's centroids are of no use without rows)
        SC_HIP(hipStreamSynchronize(s));
        sc_ivf_drop_lists_locked(ix);
        ix->n = 0;
        ix->trained = false;
        sc_invalidate_shadows(ix);
        ix->last_del_rows_moved = ix->last_del_bytes_moved = 0;
        ix->last_del_kept = 0;
        ix->last_del_dropped = valid_before;
        if (ix->tok) sc_tok_delete_locked(ix, ids);
        return SC_OK;
    }
    // stored positions of the deleted rows, ascending
    std::vector<int64_t> dpos_own;
    if (listed) {
        dpos_own.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) dpos_own[(size_t)i] = sc_ivf_pos(ix, ids[(size_t)i]);
        (void)sort_distinct(dpos_own, old_n);  // (distinct rows have distinct positions)
    }
    const std::vector<int64_t>& dpos = listed ? dpos_own : ids;
    const int64_t p0 = dpos.front();  // rows below the first deleted position are not touched
    // ---- scratch: the sorted deleted positions (and ids, where they differ) as 32-bit words -- the call's own input, 4 B per deleted row --
    // and the bounded chunk scratch: bounce rows | flags | slot -> source map | tile sums
    int64_t C = std::max<int64_t>(256, std::min<int64_t>((int64_t)1 << 20, (int64_t)(DELETE_BOUNCE_BYTES / ((size_t)ld * 4))));
    if (g_delete_chunk_rows > 0) C = std::min(C, g_delete_chunk_rows);
    C = std::min(C, old_n - p0);
    const size_t o_flags = ((size_t)C * ld * 4 + 255) & ~(size_t)255, o_src = o_flags + (((size_t)C * 4 + 255) & ~(size_t)255),
                 o_sums = o_src + (((size_t)C * 4 + 255) & ~(size_t)255), scratch_bytes = o_sums + ((size_t)(C / 1024 + 2) * 4 + 255);
    sc_status st = sc_grow(ix, ix->ivf_scratch, scratch_bytes);
    if (st) return st;
    sc_devbuf d_del;
    {
        const hipError_t e = hipMalloc(&d_del.p, (size_t)n * 4 * (listed ? 2 : 1));
        if (e != hipSuccess) return sc_fail(SC_ERR_NOMEM, "sc_index_delete_rows: hipMalloc of the delete list (%lld rows) failed: %s", (long long)n, hipGetErrorString(e));
    }
    std::vector<uint32_t> del32((size_t)n * (listed ? 2 : 1));
    for (int64_t i = 0; i < n; ++i) del32[(size_t)i] = (uint32_t)dpos[(size_t)i];
    if (listed)
        for (int64_t i = 0; i < n; ++i) del32[(size_t)(n + i)] = (uint32_t)ids[(size_t)i];
    SC_HIP(hipMemcpyAsync(d_del.p, del32.data(), del32.size() * 4, hipMemcpyHostToDevice, s));
    const uint32_t* d_dpos = (const uint32_t*)d_del.p;
    const uint32_t* d_dids = d_dpos + (listed ? n : 0);
    char* const scratch = ix->ivf_scratch.as<char>();
    uint32_t *flags = (uint32_t*)(scratch + o_flags), *src = (uint32_t*)(scratch + o_src), *sums = (uint32_t*)(scratch + o_sums);

    // the per-row arrays, each valid (and moved) below its own extent of stored positions
    struct Arr { void* base; size_t row_bytes; int64_t extent; };
    const int64_t perm_have = sc_perm_entries(ix);
    std::vector<Arr> arrs;
    arrs.push_back({ix->X, (size_t)ld * 4, old_n});
    arrs.push_back({ix->xnorm, 4, old_n});
    for (const sc_shadow* sh : ix->shadows)
        for (int i = 0; i < 2 && (valid_before & sh->stat_bit) && sh->row_bytes[i]; ++i) arrs.push_back({sh->arr[i].p, sh->row_bytes[i], sh->rows});
    if (listed) arrs.push_back({ix->perm, 4, perm_have});

    int64_t bytes_moved = 0;
    for (const Arr& a : arrs) bytes_moved += std::max<int64_t>(0, (a.extent - p0) - rank_below(dpos, a.extent)) * (int64_t)a.row_bytes;
    int64_t lo = 0;  // deleted positions below the chunk == the distance its rows move down
    // A chunk no longer than the distance its rows move is always disjoint from its destinations.  Once that distance is worth a
    // launch of its own (16 MiB of corpus rows) the chunks are cut to it: one pass over the bytes instead of two through the bounce
    // buffer -- after the first few runs of a delete of contiguous runs, that is the rest of the corpus.
    const int64_t direct_min = std::max<int64_t>(1, ((int64_t)16 << 20) / (ld * 4));
    for (int64_t c0 = p0, len = 0; c0 < old_n; c0 += len) {
        len = lo >= direct_min ? std::min(C, lo) : C;
        const int64_t c1 = std::min(old_n, c0 + len), hi = rank_below(dpos, c1);
        const int64_t cn = c1 - c0, m = cn - (hi - lo), d0 = c0 - lo;
        if (m > 0) {
            const uint32_t* map = nullptr;  // a chunk without deleted rows moves as it is
            if (hi > lo) {
                sc_launch_delete_map(d_dpos, lo, hi, c0, (uint32_t)cn, flags, sums, src, s);
                map = src;
            }
            const bool direct = lo >= m;  // [d0, d0 + m) ends at or below c0: destinations and sources of this launch are disjoint
            for (const Arr& a : arrs) {
                if (a.extent <= c0) continue;
                // kept rows of the chunk below the array's extent: the first of the (ascending) map
                const int64_t ma = a.extent >= c1 ? m : (a.extent - c0) - (rank_below(dpos, a.extent) - lo);
                if (ma <= 0) continue;
                char* dst = (char*)a.base + (size_t)d0 * a.row_bytes;
                if (direct) {
                    sc_launch_move_rows(a.base, c0, map, (uint32_t)ma, a.row_bytes, dst, s);
                } else {
                    sc_launch_move_rows(a.base, c0, map, (uint32_t)ma, a.row_bytes, scratch, s);
                    sc_launch_move_rows(scratch, 0, nullptr, (uint32_t)ma, a.row_bytes, dst, s);
                }
            }
            SC_HIP(hipGetLastError());
        }
        lo = hi;
    }
    // ---- the counts follow.  The running maxima (sc_shadow::maxima) stay as they are: they are upper bounds over the
    // rows that were there, the survivors are a subset, so every bound they enter still holds.
    const int64_t new_n = old_n - n;
    // Rows between the new row count of a shadow and its old padded end go back to what the scan kernels expect of padding rows
    // (sc_ensure_shadow_b16 / _i8 / ivfc_ensure_shadow zero them when they build, and will not build again).
    for (const sc_shadow* sh : ix->shadows) {
        if (!(valid_before & sh->stat_bit)) continue;
        const int64_t new_rows = sh->rows - rank_below(dpos, sh->rows), end = shadow_padded_end(ix, *sh, old_n);
        for (int i = 0; i < 2 && sh->row_bytes[i] && end > new_rows; ++i)
            SC_HIP(hipMemsetAsync(sh->arr[i].as<char>() + (size_t)new_rows * sh->row_bytes[i], 0, (size_t)(end - new_rows) * sh->row_bytes[i], s));
    }
    if (listed) {
        // perm's values are row ids: the second renumbering, by id, on the device
        const int64_t new_have = perm_have - rank_below(dpos, perm_have);
        sc_launch_renumber_ids(ix->perm, new_have, d_dids, n, s);
        SC_HIP(hipGetLastError());
        // host tables, while the device moves rows.  Inside a list the stored order is the order of the row ids (ivf_install_lists_locked)
        // and the compaction keeps it, so the new position of a survivor is the next free slot of its list.
        const int64_t old_ivf = ix->ivf_rows;
        std::vector<int64_t> off((size_t)ix->nlist_trained + 1, 0);
        int64_t w = 0;
        {
            size_t di = 0;
            for (int64_t r = 0; r < old_ivf; ++r) {
                if (di < ids.size() && ids[di] == r) { ++di; continue; }
                const int32_t l = ix->assign_h[(size_t)r];
                ix->assign_h[(size_t)w++] = l;
                off[(size_t)l + 1]++;
            }
        }
        const int64_t new_ivf = w;
        ix->assign_h.resize((size_t)new_ivf);
        for (int c = 0; c < ix->nlist_trained; ++c) off[(size_t)c + 1] += off[(size_t)c];
        ix->inv_h.resize((size_t)new_ivf);
        {
            std::vector<int64_t> cur(off.begin(), off.end() - 1);
            for (int64_t r = 0; r < new_ivf; ++r) ix->inv_h[(size_t)r] = (uint32_t)cur[(size_t)ix->assign_h[(size_t)r]]++;
        }
        ix->list_off_h.swap(off);
        SC_HIP(hipMemcpyAsync(ix->list_off, ix->list_off_h.data(), ix->list_off_h.size() * 8, hipMemcpyHostToDevice, s));
        ix->ivf_rows = new_ivf;
        if (ix->perm_rows > 0) ix->perm_rows = new_have;
        remap_pending(ix->dirty_rows, ids);  // row ids
    }
    // pending shadow repairs are stored positions: dropped with their rows, renumbered otherwise -- nothing is refreshed or rebuilt here
    for (sc_shadow* sh : ix->shadows) {
        remap_pending(sh->dirty, dpos);
        sh->rows -= rank_below(dpos, sh->rows);
    }
    ix->n = new_n;
    ix->last_del_rows_moved = (old_n - p0) - n;
    ix->last_del_bytes_moved = bytes_moved;
    ix->last_del_kept = valid_before;
    ix->last_del_dropped = 0;
    SC_HIP(hipStreamSynchronize(s));  // the delete list and the host tables behind asynchronous copies go out of scope
    if (ix->tok) sc_tok_delete_locked(ix, ids);  // the token store's table is renumbered with the rows (sc_tokens.cpp)
    return SC_OK;
}
