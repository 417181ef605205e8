// sc_index_state.cpp -- the device state an index owns beyond its rows: growable scratch buffers (sc_buf) and the lazily built
// shadows of the corpus (sc_shadow), declared in sc_internal.h.  Caller holds ix->mu everywhere.
#include <algorithm>
#include <vector>

#include "sc_internal.h"

sc_status sc_grow(sc_index* ix, sc_buf& b, size_t need) {
    if (need <= b.cap) return SC_OK;
    SC_HIP(hipStreamSynchronize(ix->rt->stream));
    sc_buf_free(b);
    hipError_t e = hipMalloc(&b.p, need);
    if (e != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
    b.cap = need;
    return SC_OK;
}

void sc_buf_free(sc_buf& b) {
    if (b.p) hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

void sc_shadow_invalidate(sc_shadow& sh) {
    sh.rows = 0;
    sh.dirty.clear();
}

void sc_shadow_free_maxima(sc_shadow& sh) {
    if (sh.maxima) hipFree(sh.maxima);
    sh.maxima = nullptr;
    sc_shadow_invalidate(sh);
}

void sc_shadow_release(sc_shadow& sh) {
    for (sc_buf& a : sh.arr) sc_buf_free(a);
    sc_shadow_free_maxima(sh);
}

void sc_invalidate_shadows(sc_index* ix) {
    for (sc_shadow* sh : ix->shadows) sc_shadow_invalidate(*sh);
}

void sc_shadow_note_overwritten(sc_shadow& sh, const int64_t* rows, const int64_t* pos, int64_t n, int64_t old_n) {
    if (sh.rows == 0) return;
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < old_n && pos[i] < sh.rows) sh.dirty.push_back(pos[i]);
    if ((int64_t)sh.dirty.size() > sc_index::SC_SHADOW_DIRTY_MAX) sc_shadow_invalidate(sh);  // too many single rows: the whole shadow in one pass is cheaper
}

// the rows of a dirty list as runs (first, count) of stored positions, ascending; neighbours up to 32 rows apart share a run (re-building
// a clean row in between changes nothing).  Empties the list.
static std::vector<std::pair<int64_t, int64_t>> dirty_runs(std::vector<int64_t>& dirty, int64_t covered) {
    std::sort(dirty.begin(), dirty.end());
    dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
    std::vector<std::pair<int64_t, int64_t>> runs;
    for (const int64_t r : dirty) {
        if (r >= covered) break;
        if (!runs.empty() && r < runs.back().first + runs.back().second + 32) runs.back().second = r + 1 - runs.back().first;
        else runs.emplace_back(r, 1);
    }
    dirty.clear();
    return runs;
}

// The bf16 and the int8 shadow: arrays for the capacity (rows padded to 256), rows [sh.rows, n) built, the padding rows zeroed, the
// rows overwritten since re-built.  build(first, count) launches the kernel that fills shadow rows [first, first + count) and
// accumulates into sh.maxima + 1.
template <class Build>
static sc_status ensure_shadow(sc_index* ix, sc_shadow& sh, const char* what, Build build) {
    hipStream_t s = ix->rt->stream;
    const int64_t rows_pad = (ix->n + 255) / 256 * 256;
    if ((size_t)rows_pad * sh.row_bytes[0] > sh.arr[0].cap || (size_t)rows_pad * sh.row_bytes[1] > sh.arr[1].cap) {
        SC_HIP(hipStreamSynchronize(s));
        sc_shadow_release(sh);
        const size_t cap_rows = (size_t)((std::max(ix->capacity, ix->n) + 255) / 256 * 256);
        for (int i = 0; i < 2 && sh.row_bytes[i]; ++i) {
            const size_t want = cap_rows * sh.row_bytes[i];
            hipError_t e = hipMalloc(&sh.arr[i].p, want);
            if (e != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc %s shadow (%zu B) failed: %s", what, want, hipGetErrorString(e));
            sh.arr[i].cap = want;
        }
    }
    if (!sh.maxima) {
        hipError_t e = hipMalloc((void**)&sh.maxima, 16);
        if (e != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
        sc_shadow_invalidate(sh);
    }
    if (sh.rows < ix->n) {
        // maxima = float bits of {max |x|^2, max |x - shadow(x)|^2, max |x - shadow(x)|^2 / |x|^2} over the rows
        if (sh.rows == 0) SC_HIP(hipMemsetAsync(sh.maxima, 0, 16, s));
        build(sh.rows, ix->n - sh.rows);
        for (int i = 0; i < 2 && sh.row_bytes[i] && rows_pad > ix->n; ++i)  // the last row tile reads these rows: keep them finite
            SC_HIP(hipMemsetAsync(sh.arr[i].as<char>() + (size_t)ix->n * sh.row_bytes[i], 0, (size_t)(rows_pad - ix->n) * sh.row_bytes[i], s));
        sc_launch_norm_max(ix->xnorm, ix->n, sh.maxima, s);
        sh.rows = ix->n;
        SC_HIP(hipGetLastError());
    }
    if (!sh.dirty.empty()) {  // rows overwritten since: their shadow rows alone (the maxima keep accumulating)
        for (const auto& run : dirty_runs(sh.dirty, sh.rows)) build(run.first, run.second);
        sc_launch_norm_max(ix->xnorm, ix->n, sh.maxima, s);
        SC_HIP(hipGetLastError());
    }
    return SC_OK;
}

sc_status sc_ensure_shadow_b16(sc_index* ix) {
    sc_shadow& sh = ix->sh_b16;
    return ensure_shadow(ix, sh, "bf16", [&](int64_t first, int64_t count) {
        sc_launch_shadow(ix->X, ix->xnorm, first, count, ix->ld, sh.arr[0].p, sh.maxima + 1, ix->rt->stream);
    });
}

sc_status sc_ensure_shadow_i8(sc_index* ix) {
    sc_shadow& sh = ix->sh_i8;
    return ensure_shadow(ix, sh, "int8", [&](int64_t first, int64_t count) {
        sc_launch_shadow8(ix->X, ix->xnorm, first, count, ix->ld, sc_ld8(ix), sh.arr[0].p, sh.arr[1].as<float>(), sh.maxima + 1, ix->rt->stream);
    });
}
