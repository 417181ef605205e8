// sc_ivf_build.cpp -- IVF_FLAT index build: the deterministic k-means, the list-major layout and its incremental refresh, and the
// C ABI around them (train, assign_lists, set_ivf, ivf_info, ivf_assignments).  The probes: sc_ivf_probe.cpp, sc_ivf_coarse.cpp.
//
// Mirrors (reference): Collection.create_index(IVF_FLAT, metric, nlist) + load()
// (src/semcode/storage/milvus_store.py:76-84) and the nprobe parameter of Collection.search
// (src/semcode/storage/milvus_store.py:141-147).  Milvus' own k-means (Knowhere/faiss: random sample,
// random init) is not reproducible offline; this build is deterministic instead and is restated by
// oracle/ivf_oracle.py:
//   sample   : ns = min(n, 256 * nlist) rows, row floor(i * n / ns)
//   init     : centroid c = sample row floor(c * ns / nlist)
//   iterate  : niter x { assign every sample row to its nearest centroid (exact scores, ties -> lower
//              centroid id); centroid = f32 mean of its members summed in sample order; empty cluster
//              keeps its centroid }
//   assign   : L2 for metric L2 and IP (Voronoi cells), cosine for COSINE
//   lists    : every row goes to its nearest centroid; storage is re-ordered list-major (stable by row id)
//   probe    : per query the nprobe best centroids under the INDEX metric (IP: largest inner product),
//              then an exact scan of those lists (scan_exact.hip segment mode)
#include <cstring>
#include <algorithm>
#include <vector>

#include "sc_internal.h"
#include "sc_ivf_plan.h"

static const int ASSIGN_CHUNK = 8192;

static sc_metric assign_metric(sc_metric m) { return m == SC_METRIC_COSINE ? SC_METRIC_COSINE : SC_METRIC_L2; }

// nearest centroid (k = 1) for rows given as a tight [n, dim] device matrix; out: host vector of centroid ids
static sc_status assign_rows(sc_index* ix, const float* q_dev_tight, int64_t n, std::vector<int32_t>& out) {
    sc_index* qz = ix->quant;
    hipStream_t s = ix->rt->stream;
    out.resize((size_t)n);
    sc_status st = sc_grow(ix, ix->ivf_scratch, (size_t)ASSIGN_CHUNK * 12);
    if (st) return st;
    float* dd = ix->ivf_scratch.as<float>();
    int64_t* dr = (int64_t*)(ix->ivf_scratch.as<char>() + (size_t)ASSIGN_CHUNK * 4);
    std::vector<int64_t> host((size_t)ASSIGN_CHUNK);
    for (int64_t r0 = 0; r0 < n; r0 += ASSIGN_CHUNK) {
        const int m = (int)std::min<int64_t>(ASSIGN_CHUNK, n - r0);
        std::lock_guard<std::mutex> g(qz->mu);
        sc_scoped_set<int> mode(qz->search_mode, 2);  // thousands of queries against few centroids: the MFMA path, certified exact
        // ... starting at the bf16 stage: against a few thousand centroids the int8 stage saves nothing in the coarse pass and
        // re-ranks 512 candidates per row instead of 128 (a 10M x 3072 build: 6.4 s vs 16.4 s, profiles/r2i_kernel_stats.csv)
        sc_scoped_set<int> coarse(qz->coarse_mode, qz->coarse_mode == 0 ? 16 : qz->coarse_mode);
        st = sc_search_flat_locked(qz, q_dev_tight + r0 * ix->dim, m, 1, dd, dr);
        if (st) return st;
        SC_HIP(hipMemcpyAsync(host.data(), dr, (size_t)m * 8, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < m; ++i) out[(size_t)(r0 + i)] = (int32_t)host[(size_t)i];
    }
    return SC_OK;
}

void sc_ivf_drop_lists_locked(sc_index* ix) {
    if (ix->perm) hipStreamSynchronize(ix->rt->stream);
    hipFree(ix->perm);
    hipFree(ix->list_off);
    ix->perm = nullptr;
    ix->perm_rows = 0;
    ix->list_off = nullptr;
    ix->inv_h.clear();
    ix->list_off_h.clear();
    ix->assign_h.clear();
    ix->dirty_rows.clear();
    ix->ivf_rows = 0;
    ix->trained = false;
    sc_invalidate_shadows(ix);  // (the centred shadow of the coarse stage mirrors the lists)
    sc_shadow_free_maxima(ix->sh_c8);  // ... and its per-list statistics are sized by their number
    ix->ivfc_off = false;
}

// Xo[pos] = X[g[pos]] for the n stored rows, into fresh corpus-sized buffers that replace X / xnorm on success.
// Needs a second copy of the corpus for the duration of the move: the bf16 and int8 shadows are freed first.
static sc_status ivf_move_rows_locked(sc_index* ix, const std::vector<uint32_t>& g, sc_devbuf& d_g) {
    hipStream_t s = ix->rt->stream;
    const int64_t n = ix->n;
    SC_HIP(hipStreamSynchronize(s));
    sc_shadow_release(ix->sh_b16);  // the layout changes: the shadows are rebuilt anyway
    sc_shadow_release(ix->sh_i8);
    sc_devbuf nx, nn;
    if (nx.alloc((size_t)ix->capacity * ix->ld * sizeof(float)) != hipSuccess || nn.alloc((size_t)ix->capacity * sizeof(float)) != hipSuccess ||
        d_g.alloc((size_t)n * 4) != hipSuccess)
        return sc_fail(SC_ERR_NOMEM, "ivf: hipMalloc of the re-ordered corpus (%lld rows x %d) failed", (long long)ix->capacity, ix->ld);
    SC_HIP(hipMemcpyAsync(d_g.p, g.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    sc_launch_permute_rows(ix->X, ix->xnorm, (const uint32_t*)d_g.p, n, ix->ld, (float*)nx.p, (float*)nn.p, s);
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(s));
    hipFree(ix->X);
    hipFree(ix->xnorm);
    ix->X = nx.take<float>();
    ix->xnorm = nn.take<float>();
    return SC_OK;
}

sc_status sc_ivf_untrain_locked(sc_index* ix) {
    if (!ix->perm) {
        ix->trained = false;
        return SC_OK;
    }
    if (ix->n > 0) {  // Xo[row] = X[position of row]
        std::vector<uint32_t> g((size_t)ix->n);
        for (int64_t r = 0; r < ix->n; ++r) g[(size_t)r] = (uint32_t)sc_ivf_pos(ix, r);
        sc_devbuf d_g;
        sc_status st = ivf_move_rows_locked(ix, g, d_g);
        if (st) return st;  // nothing was changed: the lists stay valid
    }
    sc_ivf_drop_lists_locked(ix);
    return SC_OK;
}

// Given a quantizer already installed in ix->quant and the list of every stored row (by row id), re-order the corpus list-major
// (stable by row id inside a list).  Works from whatever layout is current: insertion order (fresh build) or an older list-major
// layout with appended rows behind it (incremental refresh).  Nothing of the index is modified unless every step succeeded.
static sc_status ivf_install_lists_locked(sc_index* ix, int nlist, std::vector<int32_t>&& assign) {
    hipStream_t s = ix->rt->stream;
    const int64_t n = ix->n;
    std::vector<int64_t> off;
    std::vector<uint32_t> perm, inv((size_t)n), g((size_t)n);
    sc_bucket_by_key((size_t)n, (size_t)nlist, [&](size_t i) { return assign[i]; }, off, perm);
    for (int64_t pos = 0; pos < n; ++pos) {
        const int64_t i = perm[(size_t)pos];
        inv[(size_t)i] = (uint32_t)pos;
        g[(size_t)pos] = ix->perm ? (uint32_t)sc_ivf_pos(ix, i) : (uint32_t)i;  // where row i sits now
    }
    sc_devbuf d_perm, d_off, d_g;
    if (d_perm.alloc((size_t)n * 4) != hipSuccess || d_off.alloc((size_t)(nlist + 1) * 8) != hipSuccess)
        return sc_fail(SC_ERR_NOMEM, "ivf: hipMalloc of the list tables failed");
    SC_HIP(hipMemcpyAsync(d_perm.p, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(d_off.p, off.data(), (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice, s));
    sc_status st = ivf_move_rows_locked(ix, g, d_g);  // synchronises: the uploads above are complete as well
    if (st) return st;
    hipFree(ix->perm);
    hipFree(ix->list_off);
    ix->perm = d_perm.take<uint32_t>();
    ix->perm_rows = 0;
    ix->list_off = d_off.take<int64_t>();
    ix->inv_h.swap(inv);
    ix->list_off_h.swap(off);
    ix->assign_h = std::move(assign);
    ix->ivf_rows = n;
    ix->dirty_rows.clear();
    ix->nlist_trained = nlist;
    sc_invalidate_shadows(ix);  // new lists (a re-train over the same rows included): the centred shadow too is rebuilt, on the next coarse probe
    sc_shadow_free_maxima(ix->sh_c8);  // (its per-list statistics are sized by nlist_trained, which may have grown past what they hold)
    ix->ivfc_off = false;
    ix->uncert_frac = -1.0;
    ix->trained = true;
    return SC_OK;
}

// Incremental upsert: rows appended or overwritten since the lists were built are assigned to the EXISTING centroids and the
// corpus is re-ordered once (one pass over the corpus, no k-means).  The result is exactly what sc_index_assign_lists would
// build from scratch for these centroids.  Called at the start of every search; caller holds ix->mu.
static int g_ivf_refresh_nomem = 0;  // sc_diag_set_option("ivf_refresh_nomem", 1): tests of the fallback below
void sc_ivf_set_refresh_nomem(int v) { g_ivf_refresh_nomem = v; }

sc_status sc_ivf_cover_tail_locked(sc_index* ix) {
    const int64_t have = sc_perm_entries(ix);
    if (!ix->perm || have >= ix->n) return SC_OK;  // (no trained layout, or every position mapped already)
    hipStream_t s = ix->rt->stream;
    sc_devbuf d_new;
    if (d_new.alloc((size_t)ix->n * 4) != hipSuccess) return sc_fail(SC_ERR_NOMEM, "ivf: hipMalloc of the extended row map failed");
    SC_HIP(hipMemcpyAsync(d_new.p, ix->perm, (size_t)have * 4, hipMemcpyDeviceToDevice, s));
    std::vector<uint32_t> tail((size_t)(ix->n - have));
    for (int64_t r = have; r < ix->n; ++r) tail[(size_t)(r - have)] = (uint32_t)r;
    SC_HIP(hipMemcpyAsync((uint32_t*)d_new.p + have, tail.data(), tail.size() * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipStreamSynchronize(s));
    hipFree(ix->perm);
    ix->perm = d_new.take<uint32_t>();
    ix->perm_rows = ix->n;
    return SC_OK;
}

sc_status sc_ivf_refresh_locked(sc_index* ix, bool keep_tail) {
    if (!ix->perm || !ix->quant || (ix->ivf_rows == ix->n && ix->dirty_rows.empty())) return SC_OK;
    if (keep_tail && ix->dirty_rows.empty()) return SC_OK;
    if (g_ivf_refresh_nomem) return sc_fail(SC_ERR_NOMEM, "ivf refresh: out of device memory (forced by sc_diag_set_option)");
    hipStream_t s = ix->rt->stream;
    std::vector<int64_t> rows(ix->dirty_rows);
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    if (!keep_tail)
        for (int64_t r = ix->ivf_rows; r < ix->n; ++r) rows.push_back(r);
    // (the new lists of the rows are collected first: the copy of the whole assignment -- 40 MB at 10M rows, most of what a refresh that
    // moves nothing used to cost -- is made only when something does move)
    std::vector<int32_t> new_list(rows.size());
    bool changed = !keep_tail && ix->n > ix->ivf_rows;
    const int64_t CH = 65536;
    sc_devbuf d_pos, d_tight;
    const int64_t chmax = std::min<int64_t>(CH, (int64_t)rows.size());
    if (d_pos.alloc((size_t)chmax * 8) != hipSuccess || d_tight.alloc((size_t)chmax * ix->dim * 4) != hipSuccess)
        return sc_fail(SC_ERR_NOMEM, "ivf refresh: hipMalloc failed");
    std::vector<int64_t> pos((size_t)chmax);
    std::vector<int32_t> out;
    for (int64_t c0 = 0; c0 < (int64_t)rows.size(); c0 += CH) {
        const int64_t m = std::min<int64_t>(CH, (int64_t)rows.size() - c0);
        for (int64_t i = 0; i < m; ++i) pos[(size_t)i] = sc_ivf_pos(ix, rows[(size_t)(c0 + i)]);
        SC_HIP(hipMemcpyAsync(d_pos.p, pos.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
        sc_launch_rows_to_sample(ix->X, ix->ld, ix->dim, (const int64_t*)d_pos.p, m, (float*)d_tight.p, s);
        SC_HIP(hipGetLastError());
        sc_status st = assign_rows(ix, (const float*)d_tight.p, m, out);  // synchronises
        if (st) return st;
        for (int64_t i = 0; i < m; ++i) {
            const int64_t r = rows[(size_t)(c0 + i)];
            if (r >= (int64_t)ix->assign_h.size() || ix->assign_h[(size_t)r] != out[(size_t)i]) changed = true;
            new_list[(size_t)(c0 + i)] = out[(size_t)i];
        }
    }
    if (!changed) {  // overwritten rows all stayed in their lists: nothing moves
        ix->dirty_rows.clear();
        return SC_OK;
    }
    if (keep_tail) return sc_ivf_refresh_locked(ix, false);  // a row left its list: the layout is rebuilt, the tail joins it
    std::vector<int32_t> assign(ix->assign_h);
    assign.resize((size_t)ix->n, -1);
    for (size_t i = 0; i < rows.size(); ++i) assign[(size_t)rows[i]] = new_list[i];
    return ivf_install_lists_locked(ix, ix->nlist_trained, std::move(assign));
}

// ix->quant = a fresh flat index under the assignment metric: over the given host centroids [nlist, dim], or empty with room for nlist rows
static sc_status ivf_install_quantizer_locked(sc_index* ix, const float* centroids, int nlist) {
    if (ix->quant) {
        sc_index_destroy(ix->quant);
        ix->quant = nullptr;
    }
    sc_status st = sc_index_create(ix->rt, ix->dim, assign_metric(ix->metric), SC_INDEX_FLAT, 0, 0, &ix->quant);
    if (st) return st;
    return centroids ? sc_index_add(ix->quant, centroids, nlist) : sc_index_reserve(ix->quant, nlist);
}

// Quantizer installed in ix->quant: assign every stored row to its nearest centroid and re-order the corpus list-major.
static sc_status ivf_assign_all_and_install_locked(sc_index* ix, int nlist) {
    hipStream_t s = ix->rt->stream;
    const int64_t n = ix->n;
    sc_devbuf d_tight;
    const float* all_tight = ix->X;
    if (ix->ld != ix->dim) {
        if (d_tight.alloc((size_t)n * ix->dim * 4) != hipSuccess)
            return sc_fail(SC_ERR_NOMEM, "ivf: hipMalloc of the tight copy of the corpus (%lld rows x %d) failed", (long long)n, ix->dim);
        sc_launch_gather_rows(ix->X, ix->ld, 0, n, ix->dim, (float*)d_tight.p, s);
        all_tight = (const float*)d_tight.p;
    }
    std::vector<int32_t> assign;
    sc_status st = assign_rows(ix, all_tight, n, assign);
    if (st) return st;
    return ivf_install_lists_locked(ix, nlist, std::move(assign));
}

extern "C" sc_status sc_index_train(sc_index* ix, int32_t niter, uint64_t seed) {
    (void)seed;  // the build is deterministic; kept for ABI stability
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    if (niter < 0 || niter > 1000) return sc_fail(SC_ERR_INVALID, "sc_index_train: niter out of range");
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->kind != SC_INDEX_IVF_FLAT) return sc_fail(SC_ERR_STATE, "sc_index_train: index kind is not IVF_FLAT");
    if (ix->n < 1) return sc_fail(SC_ERR_STATE, "sc_index_train: the index is empty");
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    sc_status st = sc_ivf_untrain_locked(ix);
    if (st) return st;
    const int64_t n = ix->n;
    const int dim = ix->dim, ld = ix->ld;
    const int nlist = (int)std::min<int64_t>(ix->nlist, n);
    const int64_t ns = std::min<int64_t>(n, 256ll * nlist);

    // ---- sample (tight [ns, dim]) and initial centroids
    std::vector<int64_t> srows((size_t)ns);
    for (int64_t i = 0; i < ns; ++i) srows[(size_t)i] = (int64_t)(((__int128)i * n) / ns);
    sc_devbuf d_srows, d_sample, d_cinit, d_members, d_moff, d_cnew, d_moves;
    if (d_srows.alloc((size_t)ns * 8) != hipSuccess || d_sample.alloc((size_t)ns * dim * 4) != hipSuccess || d_cinit.alloc((size_t)nlist * 8) != hipSuccess ||
        d_cnew.alloc((size_t)nlist * dim * 4) != hipSuccess || d_members.alloc((size_t)ns * 8) != hipSuccess || d_moff.alloc((size_t)(nlist + 1) * 8) != hipSuccess ||
        d_moves.alloc((size_t)nlist * 2 * 4) != hipSuccess)
        return sc_fail(SC_ERR_NOMEM, "ivf: hipMalloc of the k-means sample (%lld rows x %d) failed", (long long)ns, dim);
    SC_HIP(hipMemcpyAsync(d_srows.p, srows.data(), (size_t)ns * 8, hipMemcpyHostToDevice, s));
    sc_launch_rows_to_sample(ix->X, ld, dim, (const int64_t*)d_srows.p, ns, (float*)d_sample.p, s);
    std::vector<int64_t> crow((size_t)nlist);
    for (int c = 0; c < nlist; ++c) crow[(size_t)c] = (int64_t)(((__int128)c * ns) / nlist);
    SC_HIP(hipMemcpyAsync(d_cinit.p, crow.data(), (size_t)nlist * 8, hipMemcpyHostToDevice, s));
    sc_launch_rows_to_sample((const float*)d_sample.p, dim, dim, (const int64_t*)d_cinit.p, nlist, (float*)d_cnew.p, s);
    SC_HIP(hipStreamSynchronize(s));

    // ---- quantizer = flat index over the centroids
    st = ivf_install_quantizer_locked(ix, nullptr, nlist);
    if (st) return st;
    sc_index* qz = ix->quant;
    auto set_centroids = [&](const float* c_tight) {
        std::lock_guard<std::mutex> gq(qz->mu);
        sc_launch_ingest_rows(c_tight, nullptr, 0, nlist, dim, qz->X, qz->ld, qz->xnorm, s);
        qz->n = nlist;
        sc_invalidate_shadows(qz);  // the centroids changed: both coarse shadows are stale
    };
    set_centroids((const float*)d_cnew.p);

    // ---- Lloyd iterations on the sample
    std::vector<int32_t> assign;
    std::vector<int64_t> members, moff;
    for (int it = 0; it < niter; ++it) {
        st = assign_rows(ix, (const float*)d_sample.p, ns, assign);
        if (st) return st;
        sc_bucket_by_key((size_t)ns, (size_t)nlist, [&](size_t i) { return assign[i]; }, moff, members);  // sample order inside a cluster
        SC_HIP(hipMemcpyAsync(d_members.p, members.data(), (size_t)ns * 8, hipMemcpyHostToDevice, s));
        SC_HIP(hipMemcpyAsync(d_moff.p, moff.data(), (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice, s));
        sc_launch_centroid_mean((const float*)d_sample.p, dim, dim, (const int64_t*)d_members.p, (const int64_t*)d_moff.p, nlist,
                                (float*)d_cnew.p, qz->X, qz->ld, s);
        SC_HIP(hipGetLastError());
        // re-seeding (every iteration but the last, so that final centroids are plain means): sc_ivf_plan.cpp has the rule
        if (it + 1 < niter) {
            std::vector<int64_t> cnt((size_t)nlist);
            for (int c = 0; c < nlist; ++c) cnt[(size_t)c] = moff[(size_t)c + 1] - moff[(size_t)c];
            const std::vector<int32_t> moves = sc_ivf_reseed_moves(cnt, ns);
            if (!moves.empty()) {  // (at most nlist moves: every one takes a different starved centroid)
                SC_HIP(hipMemcpyAsync(d_moves.p, moves.data(), moves.size() * 4, hipMemcpyHostToDevice, s));
                sc_launch_reseed_centroids((float*)d_cnew.p, dim, (const int32_t*)d_moves.p, (int)(moves.size() / 2), s);
                SC_HIP(hipGetLastError());
                SC_HIP(hipStreamSynchronize(s));
            }
        }
        SC_HIP(hipStreamSynchronize(s));
        set_centroids((const float*)d_cnew.p);
    }

    return ivf_assign_all_and_install_locked(ix, nlist);
}

// List of every row, in insertion order (persistence: together with the centroids this restores the lists without k-means).
extern "C" sc_status sc_index_ivf_assignments(sc_index* ix, int32_t* out) {
    if (!ix || !out) return sc_fail(SC_ERR_INVALID, "sc_index_ivf_assignments: NULL argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->trained) return sc_fail(SC_ERR_STATE, "sc_index_ivf_assignments: the index is not trained");
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_status st = sc_ivf_refresh_locked(ix);  // rows upserted since the build get their list first
    if (st) return st;
    memcpy(out, ix->assign_h.data(), (size_t)ix->n * sizeof(int32_t));
    return SC_OK;
}

// Build the lists for GIVEN centroids (no k-means): every row goes to its nearest centroid under the assignment metric.  Multi-GPU
// IVF: one rank trains, broadcasts its centroids, every rank calls this on its shard -- probing then means the same lists on every
// shard, and the merged result equals that of one index over the whole corpus with these centroids.
extern "C" sc_status sc_index_assign_lists(sc_index* ix, const float* centroids, int32_t nlist) {
    if (!ix || !centroids || nlist < 1) return sc_fail(SC_ERR_INVALID, "sc_index_assign_lists: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->kind != SC_INDEX_IVF_FLAT) return sc_fail(SC_ERR_STATE, "sc_index_assign_lists: index kind is not IVF_FLAT");
    if (ix->n < 1) return sc_fail(SC_ERR_STATE, "sc_index_assign_lists: the index is empty");
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_status st = sc_ivf_untrain_locked(ix);
    if (st) return st;
    st = ivf_install_quantizer_locked(ix, centroids, nlist);
    if (st) return st;
    return ivf_assign_all_and_install_locked(ix, nlist);
}

// Install a previously trained IVF structure: centroids [nlist, dim] (tight f32) and the list of every row.
extern "C" sc_status sc_index_set_ivf(sc_index* ix, const float* centroids, const int32_t* assign, int32_t nlist) {
    if (!ix || !centroids || !assign || nlist < 1) return sc_fail(SC_ERR_INVALID, "sc_index_set_ivf: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->kind != SC_INDEX_IVF_FLAT) return sc_fail(SC_ERR_STATE, "sc_index_set_ivf: index kind is not IVF_FLAT");
    if (ix->n < 1) return sc_fail(SC_ERR_STATE, "sc_index_set_ivf: the index is empty");
    for (int64_t i = 0; i < ix->n; ++i)
        if (assign[i] < 0 || assign[i] >= nlist) return sc_fail(SC_ERR_INVALID, "sc_index_set_ivf: assign[%lld] = %d outside [0,%d)", (long long)i, assign[i], nlist);
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_status st = sc_ivf_untrain_locked(ix);
    if (st) return st;
    st = ivf_install_quantizer_locked(ix, centroids, nlist);
    if (st) return st;
    return ivf_install_lists_locked(ix, nlist, std::vector<int32_t>(assign, assign + ix->n));
}

// Centroids (tight [nlist, dim]) and list sizes back to the host (tests, persistence).
extern "C" sc_status sc_index_ivf_info(sc_index* ix, int32_t* nlist, float* centroids, int64_t* list_sizes) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->trained || !ix->quant) {
        if (nlist) *nlist = 0;
        return SC_OK;
    }
    SC_HIP(hipSetDevice(ix->rt->device));
    {
        sc_status st = sc_ivf_refresh_locked(ix);
        if (st) return st;
    }
    if (nlist) *nlist = ix->nlist_trained;
    if (centroids) {
        sc_status st = sc_index_get_rows(ix->quant, 0, ix->nlist_trained, centroids);
        if (st) return st;
    }
    if (list_sizes)
        for (int c = 0; c < ix->nlist_trained; ++c) list_sizes[c] = ix->list_off_h[(size_t)c + 1] - ix->list_off_h[(size_t)c];
    return SC_OK;
}
