// sc_api.cpp -- host side of the C ABI declared in include/semcode_hip.h: runtime + profiling, sc_diag_set_option, index create / destroy, rows in
// and out, the getters of the last call's statistics.  Search: sc_search.cpp; IVF build and probes: sc_ivf_*.cpp; delete: sc_delete.cpp; buffers and shadows: sc_index_state.cpp.
//
// Mirrors (reference): MilvusVectorStore's use of pymilvus -- connect / create collection + index /
// upsert / search -- src/semcode/storage/milvus_store.py:39-148.  Error behaviour: every failure is
// a negative sc_status plus a thread-local message, so the Python seam can raise ordinary
// exceptions that IndexerService / SemanticSearchPipeline already catch (indexer.py:57-63,
// pipeline.py:95-110).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "encoder_ops.h"  // sc_gemm_set_*
#include "sc_internal.h"

static thread_local std::string g_err;

sc_status sc_fail(sc_status code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char* sc_version(void) { return "semcode_hip 0.1 (gfx950)"; }

extern "C" sc_status sc_last_error(char* buf, size_t n) {
    if (!buf || n == 0) return SC_ERR_INVALID;
    snprintf(buf, n, "%s", g_err.c_str());
    return SC_OK;
}

// ------------------------------------------------------------------ runtime

extern "C" sc_status sc_runtime_create(const sc_runtime_cfg* cfg, sc_runtime** out) {
    if (!out) return sc_fail(SC_ERR_INVALID, "sc_runtime_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return sc_fail(SC_ERR_HIP, "sc_runtime_create: no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    const int dev = cfg ? cfg->device : 0;
    if (dev < 0 || dev >= ndev) return sc_fail(SC_ERR_INVALID, "sc_runtime_create: device %d out of range [0,%d)", dev, ndev);
    SC_HIP(hipSetDevice(dev));
    sc_runtime* rt = new (std::nothrow) sc_runtime();
    if (!rt) return sc_fail(SC_ERR_NOMEM, "sc_runtime_create: out of host memory");
    rt->device = dev;
    if (cfg && cfg->stream) {
        rt->stream = (hipStream_t)cfg->stream;
        rt->own_stream = false;
    } else {
        e = hipStreamCreateWithFlags(&rt->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete rt;
            return sc_fail(SC_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        rt->own_stream = true;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
        snprintf(rt->name, sizeof rt->name, "%s (%s)", prop.name, prop.gcnArchName);
        rt->cus = prop.multiProcessorCount;
        rt->hbm = (int64_t)prop.totalGlobalMem;
    }
    *out = rt;
    return SC_OK;
}

static void prof_clear(sc_runtime* rt) {
    for (int c = 0; c < SC_PROF_CLASSES; ++c) {
        for (auto& p : rt->prof[c]) {
            hipEventDestroy(p.first);
            hipEventDestroy(p.second);
        }
        rt->prof[c].clear();
    }
}

void sc_runtime_retain(sc_runtime* rt) { rt->refs.fetch_add(1, std::memory_order_relaxed); }

void sc_runtime_release(sc_runtime* rt) {
    if (rt->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    hipSetDevice(rt->device);
    hipStreamSynchronize(rt->stream);
    prof_clear(rt);
    if (rt->own_stream) hipStreamDestroy(rt->stream);
    delete rt;
}

// Drops the creator's reference.  Indexes / encoders still alive keep the runtime (device binding + stream) alive until
// they are destroyed themselves: their destroy paths synchronise on rt->stream, which must not be a freed handle.
extern "C" sc_status sc_runtime_destroy(sc_runtime* rt) {
    if (!rt) return SC_OK;
    sc_runtime_release(rt);
    return SC_OK;
}

extern "C" sc_status sc_runtime_set_stream(sc_runtime* rt, void* stream) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "runtime is NULL");
    std::lock_guard<std::mutex> g(rt->mu);
    if (rt->own_stream) {
        hipStreamSynchronize(rt->stream);
        hipStreamDestroy(rt->stream);
        rt->own_stream = false;
    }
    rt->stream = (hipStream_t)stream;
    return SC_OK;
}

extern "C" sc_status sc_runtime_synchronize(sc_runtime* rt) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "runtime is NULL");
    SC_HIP(hipSetDevice(rt->device));
    SC_HIP(hipStreamSynchronize(rt->stream));
    return SC_OK;
}

extern "C" sc_status sc_runtime_device_info(sc_runtime* rt, char* name, size_t n, int32_t* cus, int64_t* hbm_bytes) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "runtime is NULL");
    if (name && n) snprintf(name, n, "%s", rt->name);
    if (cus) *cus = rt->cus;
    if (hbm_bytes) *hbm_bytes = rt->hbm;
    return SC_OK;
}

extern "C" sc_status sc_runtime_set_profiling(sc_runtime* rt, int32_t enabled) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "runtime is NULL");
    rt->profiling = enabled < 0 ? 0 : enabled;
    return SC_OK;
}

void sc_prof_begin(sc_runtime* rt, int which, hipEvent_t* a, hipEvent_t* b) {
    *a = *b = nullptr;
    if (!rt->profiling || rt->prof[which].size() >= 8192) return;
    // the encoder launches ~60 kernels of these classes per step: an event pair around each costs 1.6 % of the step, so they
    // are sampled (bench.py passes a stride co-prime with the 4 GEMM shapes per layer, so every shape is sampled equally)
    if (which >= SC_PROF_GEMM && rt->profiling > 1 && (rt->prof_seen[which]++ % (unsigned)rt->profiling) != 0) return;
    if (hipEventCreate(a) != hipSuccess) { *a = nullptr; return; }
    if (hipEventCreate(b) != hipSuccess) { hipEventDestroy(*a); *a = *b = nullptr; return; }
    hipEventRecord(*a, rt->stream);
}
void sc_prof_end(sc_runtime* rt, int which, hipEvent_t a, hipEvent_t b) {
    if (!a) return;
    hipEventRecord(b, rt->stream);
    std::lock_guard<std::mutex> g(rt->mu);
    rt->prof[which].push_back({a, b});
}

extern "C" sc_status sc_runtime_profile_read(sc_runtime* rt, int32_t which, double* total_ms, int64_t* launches) {
    if (!rt || which < 0 || which >= SC_PROF_CLASSES) return sc_fail(SC_ERR_INVALID, "bad profile class");
    SC_HIP(hipSetDevice(rt->device));
    SC_HIP(hipStreamSynchronize(rt->stream));
    double t = 0;
    std::lock_guard<std::mutex> g(rt->mu);
    for (auto& p : rt->prof[which]) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = (int64_t)rt->prof[which].size();
    return SC_OK;
}

extern "C" sc_status sc_runtime_profile_reset(sc_runtime* rt) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "runtime is NULL");
    SC_HIP(hipSetDevice(rt->device));
    SC_HIP(hipStreamSynchronize(rt->stream));
    std::lock_guard<std::mutex> g(rt->mu);
    prof_clear(rt);
    for (unsigned& c : rt->prof_seen) c = 0;
    return SC_OK;
}

extern "C" sc_status sc_synth_fill_dev(sc_runtime* rt, float* out, int64_t rows, int32_t dim, int32_t ld, uint64_t seed,
                                       int64_t first_row) {
    if (!rt || !out) return sc_fail(SC_ERR_INVALID, "sc_synth_fill_dev: NULL argument");
    if (rows < 0 || dim <= 0 || ld < dim || (ld & 3)) return sc_fail(SC_ERR_INVALID, "sc_synth_fill_dev: need rows>=0, 0<dim<=ld, ld%%4==0");
    SC_HIP(hipSetDevice(rt->device));
    sc_launch_synth_fill(out, rows, dim, ld, seed, first_row, nullptr, rt->stream);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// The process-wide switchboard of the tests and A/B scripts: every option forwards to a setter next to the code it steers.
extern "C" sc_status sc_diag_set_option(const char* name, int32_t value) {
    if (!name) return sc_fail(SC_ERR_INVALID, "sc_diag_set_option: NULL name");
    static const struct { const char* name; void (*set)(int); } options[] = {
        {"coarse_workgroups", sc_scan_set_coarse_workgroups}, {"coarse_persistent", sc_scan_set_coarse_persistent},
        {"gemm_pp", sc_gemm_set_pp},                          {"gemm_nt", sc_gemm_set_nt},
        {"ivf_refresh_nomem", sc_ivf_set_refresh_nomem},      {"ivf_refine_cap", sc_ivf_set_refine_cap},
        {"ivf_coarse_nomem", sc_ivf_set_coarse_nomem},        {"collect_pass", sc_set_collect_pass},
        {"tighten", sc_set_tighten},                          {"wide_candidates", sc_set_wide_force},
        {"ivf_tail_rows", sc_set_ivf_tail_rows},              {"delete_chunk_rows", sc_set_delete_chunk_rows},
        {"rope_fused", sc_encoder_set_rope_fused},            {"mask_gather", sc_set_mask_gather},
        {"group_width0", sc_set_group_width0},                {"group_width1", sc_set_group_width1},
        {"mmr_chunk_q", sc_set_mmr_chunk_q},                  {"lex_chunk_q", sc_set_lex_chunk_q},
        {"gemm_strip", sc_gemm_set_strip},                    {"gemm_strip_n", sc_gemm_set_strip_n},
        {"cls_prune", sc_encoder_set_cls_prune},              {"gemm_order", sc_gemm_set_order},
    };
    for (const auto& o : options)
        if (!strcmp(name, o.name)) {
            o.set(value);
            return SC_OK;
        }
    return sc_fail(SC_ERR_INVALID, "sc_diag_set_option: unknown option '%s'", name);
}

// ------------------------------------------------------------------ index

static inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

extern "C" sc_status sc_index_create(sc_runtime* rt, int32_t dim, sc_metric metric, sc_index_kind kind, int32_t nlist,
                                     int64_t row_base, sc_index** out) {
    if (!rt || !out) return sc_fail(SC_ERR_INVALID, "sc_index_create: NULL argument");
    *out = nullptr;
    if (dim <= 0 || dim > 65536) return sc_fail(SC_ERR_INVALID, "sc_index_create: dim %d out of range", dim);
    if (metric != SC_METRIC_IP && metric != SC_METRIC_L2 && metric != SC_METRIC_COSINE)
        return sc_fail(SC_ERR_INVALID, "sc_index_create: unknown metric %d", (int)metric);
    if (kind != SC_INDEX_FLAT && kind != SC_INDEX_IVF_FLAT) return sc_fail(SC_ERR_INVALID, "sc_index_create: unknown kind %d", (int)kind);
    if (kind == SC_INDEX_IVF_FLAT && nlist < 1) return sc_fail(SC_ERR_INVALID, "sc_index_create: IVF_FLAT needs nlist >= 1");
    sc_index* ix = new (std::nothrow) sc_index();
    if (!ix) return sc_fail(SC_ERR_NOMEM, "out of host memory");
    ix->rt = rt;
    sc_runtime_retain(rt);
    ix->dim = dim;
    ix->ld = round_up(dim, SC_LD_ALIGN);
    ix->metric = metric;
    ix->kind = kind;
    ix->nlist = nlist;
    ix->row_base = row_base;
    const size_t ld8 = (size_t)sc_ld8(ix);
    ix->sh_b16.row_bytes[0] = (size_t)ix->ld * 2;
    ix->sh_b16.stat_bit = 1;
    ix->sh_i8.row_bytes[0] = ix->sh_c8.row_bytes[0] = ld8;
    ix->sh_i8.row_bytes[1] = 4;
    ix->sh_i8.stat_bit = 2;
    ix->sh_c8.row_bytes[1] = 16;
    ix->sh_c8.tail_pad = 256;
    ix->sh_c8.stat_bit = 4;
    *out = ix;
    return SC_OK;
}

extern "C" sc_status sc_index_destroy(sc_index* ix) {
    if (!ix) return SC_OK;
    hipSetDevice(ix->rt->device);
    hipStreamSynchronize(ix->rt->stream);
    hipFree(ix->X);
    hipFree(ix->xnorm);
    hipFree(ix->perm);
    hipFree(ix->list_off);
    for (const sc_index_buf& b : SC_INDEX_BUFS) sc_buf_free(ix->*b.buf);
    for (sc_shadow* sh : ix->shadows) sc_shadow_release(*sh);
    sc_tok_free_locked(ix);
    if (ix->quant) sc_index_destroy(ix->quant);
    sc_runtime* rt = ix->rt;
    delete ix;
    sc_runtime_release(rt);
    return SC_OK;
}

extern "C" sc_status sc_index_info(sc_index* ix, int64_t* rows, int32_t* dim, int32_t* ld) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (rows) *rows = ix->n;
    if (dim) *dim = ix->dim;
    if (ld) *ld = ix->ld;
    return SC_OK;
}

// make room for `rows` rows, preserving the first ix->n
static sc_status ensure_rows(sc_index* ix, int64_t rows, bool exact) {
    if (rows <= ix->capacity) return SC_OK;
    int64_t cap = rows;
    if (!exact) cap = std::max<int64_t>(rows, std::max<int64_t>(ix->capacity * 2, 4096));
    float *nx = nullptr, *nn = nullptr;
    hipError_t e = hipMalloc((void**)&nx, (size_t)cap * ix->ld * sizeof(float));
    if (e != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc corpus (%lld rows x %d) failed: %s", (long long)cap, ix->ld, hipGetErrorString(e));
    e = hipMalloc((void**)&nn, (size_t)cap * sizeof(float));
    if (e != hipSuccess) {
        hipFree(nx);
        return sc_fail(SC_ERR_NOMEM, "hipMalloc norms failed: %s", hipGetErrorString(e));
    }
    hipStream_t s = ix->rt->stream;
    if (ix->n > 0) {
        SC_HIP(hipMemcpyAsync(nx, ix->X, (size_t)ix->n * ix->ld * sizeof(float), hipMemcpyDeviceToDevice, s));
        SC_HIP(hipMemcpyAsync(nn, ix->xnorm, (size_t)ix->n * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    SC_HIP(hipStreamSynchronize(s));
    hipFree(ix->X);
    hipFree(ix->xnorm);
    ix->X = nx;
    ix->xnorm = nn;
    ix->capacity = cap;
    return SC_OK;
}

extern "C" sc_status sc_index_reserve(sc_index* ix, int64_t rows) {
    if (!ix || rows < 0) return sc_fail(SC_ERR_INVALID, "sc_index_reserve: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    return ensure_rows(ix, rows, true);
}

static const int64_t STAGE_ROWS_BYTES = 64ll << 20;

extern "C" sc_status sc_index_add(sc_index* ix, const float* vecs, int64_t n) {
    if (!ix || n < 0 || (n > 0 && !vecs)) return sc_fail(SC_ERR_INVALID, "sc_index_add: bad argument");
    if (n == 0) return SC_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    if (ix->n + n > 0xFFFFFFF0ll) return sc_fail(SC_ERR_UNSUPPORTED, "sc_index_add: more than 2^32 rows per shard");
    // a trained index keeps its lists: the new rows wait behind them (position == row id) for sc_ivf_refresh_locked
    sc_status st = ensure_rows(ix, ix->n + n, false);
    if (st) return st;
    const int64_t chunk = std::max<int64_t>(1, STAGE_ROWS_BYTES / ((int64_t)ix->dim * 4));
    hipStream_t s = ix->rt->stream;
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = std::min(chunk, n - off);
        st = sc_grow(ix, ix->stage, (size_t)m * ix->dim * 4);
        if (st) return st;
        SC_HIP(hipMemcpyAsync(ix->stage.p, vecs + off * ix->dim, (size_t)m * ix->dim * 4, hipMemcpyHostToDevice, s));
        sc_launch_ingest_rows(ix->stage.as<float>(), nullptr, ix->n + off, m, ix->dim, ix->X, ix->ld, ix->xnorm, s);
        SC_HIP(hipGetLastError());
        SC_HIP(hipStreamSynchronize(s));  // staging buffer is reused by the next chunk
    }
    ix->n += n;
    if (!ix->perm) ix->trained = false;
    return SC_OK;  // rows [sh_b16.rows, n) get their bf16 shadow lazily
}

extern "C" sc_status sc_index_overwrite(sc_index* ix, const float* vecs, const int64_t* rows, int64_t n) {
    if (!ix || n < 0 || (n > 0 && (!vecs || !rows))) return sc_fail(SC_ERR_INVALID, "sc_index_overwrite: bad argument");
    if (n == 0) return SC_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= ix->n) return sc_fail(SC_ERR_INVALID, "sc_index_overwrite: row %lld out of range [0,%lld)", (long long)rows[i], (long long)ix->n);
    return sc_index_put_rows_locked(ix, vecs, false, rows, n, "sc_index_overwrite");
}

// rows[i] <- vecs[i], appends allowed (see include/semcode_hip.h sc_index_put_rows).  vecs: host or device [n, dim].
sc_status sc_index_put_rows_locked(sc_index* ix, const float* vecs, bool vecs_on_device, const int64_t* rows, int64_t n, const char* who) {
    int64_t next = ix->n, min_old = INT64_MAX;
    const int64_t old_n = ix->n;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = rows[i];
        if (r == next) ++next;
        else if (r >= 0 && r < ix->n) min_old = std::min(min_old, r);
        else return sc_fail(SC_ERR_INVALID, "%s: rows[%lld] = %lld is neither an existing row [0,%lld) nor the next free row %lld", who, (long long)i,
                            (long long)r, (long long)ix->n, (long long)next);
    }
    if (next > 0xFFFFFFF0ll) return sc_fail(SC_ERR_UNSUPPORTED, "%s: more than 2^32 rows per shard", who);
    {
        std::vector<int64_t> sorted(rows, rows + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return sc_fail(SC_ERR_INVALID, "%s: row numbers must be distinct", who);
    }
    sc_status st = ensure_rows(ix, next, false);
    if (st) return st;
    hipStream_t s = ix->rt->stream;
    // Trained layout: a row of the lists lives at inv_h[row] (replaced in place, re-assigned to its list at the next search);
    // appended rows go behind the lists at position == row id.  The translated positions are a temporary: synchronise
    // before it goes out of scope (upserts into a trained index are not asynchronous).
    std::vector<int64_t> pos;
    const int64_t* row_ids = rows;  // the caller's row numbers (rows is redirected to stored positions below)
    if (ix->perm) {
        pos.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            pos[(size_t)i] = sc_ivf_pos(ix, rows[i]);
        }
        min_old = INT64_MAX;  // the shadow is indexed by stored position
        for (int64_t i = 0; i < n; ++i)
            if (rows[i] < ix->n) min_old = std::min(min_old, pos[(size_t)i]);
        rows = pos.data();
    }
    if (vecs_on_device) {
        st = sc_grow(ix, ix->stage, (size_t)n * 8);
        if (st) return st;
        SC_HIP(hipMemcpyAsync(ix->stage.p, rows, (size_t)n * 8, hipMemcpyHostToDevice, s));
        sc_launch_ingest_rows(vecs, ix->stage.as<int64_t>(), 0, n, ix->dim, ix->X, ix->ld, ix->xnorm, s);
        SC_HIP(hipGetLastError());
        if (ix->perm) SC_HIP(hipStreamSynchronize(s));
    } else {
        const int64_t chunk = std::max<int64_t>(1, STAGE_ROWS_BYTES / ((int64_t)ix->dim * 4 + 8));
        for (int64_t off = 0; off < n; off += chunk) {
            const int64_t m = std::min(chunk, n - off);
            const size_t vbytes = ((size_t)m * ix->dim * 4 + 15) & ~(size_t)15;
            st = sc_grow(ix, ix->stage, vbytes + (size_t)m * 8);
            if (st) return st;
            int64_t* drows = (int64_t*)(ix->stage.as<char>() + vbytes);
            SC_HIP(hipMemcpyAsync(ix->stage.p, vecs + off * ix->dim, (size_t)m * ix->dim * 4, hipMemcpyHostToDevice, s));
            SC_HIP(hipMemcpyAsync(drows, rows + off, (size_t)m * 8, hipMemcpyHostToDevice, s));
            sc_launch_ingest_rows(ix->stage.as<float>(), drows, 0, m, ix->dim, ix->X, ix->ld, ix->xnorm, s);
            SC_HIP(hipGetLastError());
            SC_HIP(hipStreamSynchronize(s));  // staging buffer is reused by the next chunk
        }
    }
    if (ix->perm && row_ids) {  // rows of the lists whose vectors changed: re-assigned at the next refresh (recorded once, after the write)
        const size_t before = ix->dirty_rows.size();
        for (int64_t i = 0; i < n; ++i)
            if (row_ids[i] < ix->ivf_rows) ix->dirty_rows.push_back(row_ids[i]);
        if (ix->dirty_rows.size() > before && ix->dirty_rows.size() > 1024) {
            std::sort(ix->dirty_rows.begin(), ix->dirty_rows.end());
            ix->dirty_rows.erase(std::unique(ix->dirty_rows.begin(), ix->dirty_rows.end()), ix->dirty_rows.end());
        }
    }
    ix->n = next;
    if (!ix->perm) ix->trained = false;
    // replaced rows: their shadow rows are stale.  Remembered by stored position and re-built alone before the next search that reads
    // the shadow (sc_ensure_shadow_b16 / _i8 / ivfc_ensure_shadow); appended rows get theirs lazily as before.  `rows` holds
    // stored positions here, old_n the row count before this call.
    if (min_old != INT64_MAX)
        for (sc_shadow* sh : ix->shadows) sc_shadow_note_overwritten(*sh, row_ids, rows, n, old_n);
    return SC_OK;
}

extern "C" sc_status sc_index_put_rows(sc_index* ix, const float* vecs, const int64_t* rows, int64_t n) {
    if (!ix || n < 0 || (n > 0 && (!vecs || !rows))) return sc_fail(SC_ERR_INVALID, "sc_index_put_rows: bad argument");
    if (n == 0) return SC_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    return sc_index_put_rows_locked(ix, vecs, false, rows, n, "sc_index_put_rows");
}

extern "C" sc_status sc_index_put_rows_dev(sc_index* ix, const float* vecs_dev, const int64_t* rows, int64_t n) {
    if (!ix || n < 0 || (n > 0 && (!vecs_dev || !rows))) return sc_fail(SC_ERR_INVALID, "sc_index_put_rows_dev: bad argument");
    if (n == 0) return SC_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_status st = sc_index_put_rows_locked(ix, vecs_dev, true, rows, n, "sc_index_put_rows_dev");
    if (st) return st;
    SC_HIP(hipStreamSynchronize(ix->rt->stream));  // `rows` is the caller's (pageable) memory: do not return while its copy may be pending
    return SC_OK;
}

extern "C" sc_status sc_index_get_rows(sc_index* ix, int64_t first, int64_t n, float* out) {
    if (!ix || n < 0 || first < 0 || (n > 0 && !out)) return sc_fail(SC_ERR_INVALID, "sc_index_get_rows: bad argument");
    std::lock_guard<std::mutex> g(ix->mu);
    if (first + n > ix->n) return sc_fail(SC_ERR_INVALID, "sc_index_get_rows: [%lld,%lld) exceeds %lld rows", (long long)first, (long long)(first + n), (long long)ix->n);
    if (n == 0) return SC_OK;
    SC_HIP(hipSetDevice(ix->rt->device));
    const int64_t chunk = std::max<int64_t>(1, STAGE_ROWS_BYTES / ((int64_t)ix->dim * 4));
    hipStream_t s = ix->rt->stream;
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = std::min(chunk, n - off);
        sc_status st = sc_grow(ix, ix->stage, (size_t)m * ix->dim * 4);
        if (st) return st;
        if (ix->perm) {  // list-major storage: fetch row ids first+off .. through the inverse permutation
            std::vector<int64_t> pos((size_t)m);
            for (int64_t i = 0; i < m; ++i) pos[(size_t)i] = sc_ivf_pos(ix, first + off + i);
            st = sc_grow(ix, ix->ivf_scratch, (size_t)m * 8);
            if (st) return st;
            SC_HIP(hipMemcpyAsync(ix->ivf_scratch.p, pos.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
            sc_launch_rows_to_sample(ix->X, ix->ld, ix->dim, ix->ivf_scratch.as<int64_t>(), m, ix->stage.as<float>(), s);
            SC_HIP(hipStreamSynchronize(s));  // pos goes out of scope
        } else {
            sc_launch_gather_rows(ix->X, ix->ld, first + off, m, ix->dim, ix->stage.as<float>(), s);
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(out + off * ix->dim, ix->stage.p, (size_t)m * ix->dim * 4, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
    }
    return SC_OK;
}

// Replace the rows by n generated ones: fill(X, xnorm, stream) launches the generator.  Everything learnt about the old rows goes.
template <class Fill>
static sc_status fill_rows(sc_index* ix, int64_t n, Fill fill) {
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    if (n > 0xFFFFFFF0ll) return sc_fail(SC_ERR_UNSUPPORTED, "more than 2^32 rows per shard");
    sc_ivf_drop_lists_locked(ix);  // (invalidates the shadows)
    ix->n = 0;  // nothing to preserve
    sc_status st = ensure_rows(ix, n, true);
    if (st) return st;
    fill(ix->X, ix->xnorm, ix->rt->stream);
    SC_HIP(hipGetLastError());
    ix->n = n;
    ix->trained = false;
    ix->i8_off = false;
    ix->wide_i8 = false;
    ix->i8_sticky = false;
    ix->cost_i8_first = 0.0;
    ix->collect_off8 = ix->collect_off16 = false;
    return SC_OK;
}

extern "C" sc_status sc_index_fill_synthetic(sc_index* ix, int64_t n, uint64_t seed, int64_t first_row) {
    if (!ix || n < 0) return sc_fail(SC_ERR_INVALID, "sc_index_fill_synthetic: bad argument");
    return fill_rows(ix, n, [&](float* X, float* xnorm, hipStream_t s) { sc_launch_synth_fill(X, n, ix->dim, ix->ld, seed, first_row, xnorm, s); });
}

extern "C" sc_status sc_index_fill_synthetic_clustered(sc_index* ix, int64_t n, uint64_t seed, int64_t first_row, int32_t nclusters,
                                                       float spread) {
    if (!ix || n < 0 || nclusters < 1) return sc_fail(SC_ERR_INVALID, "sc_index_fill_synthetic_clustered: bad argument");
    return fill_rows(ix, n, [&](float* X, float* xnorm, hipStream_t s) { sc_launch_synth_clustered(X, n, ix->dim, ix->ld, seed, first_row, nclusters, spread, xnorm, s); });
}

// Free everything that can be rebuilt (the three shadows, search scratch): for corpora close to the HBM capacity.
extern "C" sc_status sc_index_release_scratch(sc_index* ix) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    SC_HIP(hipStreamSynchronize(ix->rt->stream));
    for (sc_shadow* sh : ix->shadows) sc_shadow_release(*sh);
    for (const sc_index_buf& b : SC_INDEX_BUFS)
        if (b.released) sc_buf_free(ix->*b.buf);
    return SC_OK;
}

extern "C" sc_status sc_index_last_delete_stats(sc_index* ix, int64_t* rows_moved, int64_t* bytes_moved, int32_t* shadows_kept, int32_t* shadows_dropped) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (rows_moved) *rows_moved = ix->last_del_rows_moved;
    if (bytes_moved) *bytes_moved = ix->last_del_bytes_moved;
    if (shadows_kept) *shadows_kept = ix->last_del_kept;
    if (shadows_dropped) *shadows_dropped = ix->last_del_dropped;
    return SC_OK;
}

extern "C" sc_status sc_index_set_search_mode(sc_index* ix, int32_t mode) {
    if (!ix || mode < 0 || mode > 5)
        return sc_fail(SC_ERR_INVALID, "sc_index_set_search_mode: mode must be 0 (auto), 1 (exact), 2 (batched), 3 (ivf probe per query), 4 (ivf probe list-major, exact f32) "
                                       "or 5 (ivf probe list-major behind the int8 coarse stage)");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->search_mode = mode;
    return SC_OK;
}

extern "C" sc_status sc_index_last_search_stats(sc_index* ix, int32_t* path, int32_t* uncertified) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (path) *path = ix->last_path;
    if (uncertified) *uncertified = ix->last_uncertified;
    return SC_OK;
}

extern "C" sc_status sc_index_set_coarse_stage(sc_index* ix, int32_t bits) {
    if (!ix || (bits != 0 && bits != 8 && bits != 16)) return sc_fail(SC_ERR_INVALID, "sc_index_set_coarse_stage: bits must be 0 (auto), 8 or 16");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->coarse_mode = bits;
    if (bits == 0) { ix->i8_off = false; ix->wide_i8 = false; ix->i8_sticky = false; ix->cost_i8_first = 0.0; }
    ix->collect_off8 = ix->collect_off16 = false;
    return SC_OK;
}

extern "C" sc_status sc_index_last_coarse_stats(sc_index* ix, int32_t* first_stage_bits, int32_t* handed_to_bf16) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (first_stage_bits) *first_stage_bits = ix->last_coarse_bits;
    if (handed_to_bf16) *handed_to_bf16 = ix->last_uncert_i8;
    return SC_OK;
}

extern "C" sc_status sc_index_last_collect_stats(sc_index* ix, int32_t* tried, int32_t* resolved) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (tried) *tried = ix->last_collect_tried;
    if (resolved) *resolved = ix->last_collect_resolved;
    return SC_OK;
}

extern "C" sc_status sc_index_last_tail_rows(sc_index* ix, int64_t* rows) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (rows) *rows = ix->last_tail_rows;
    return SC_OK;
}

extern "C" sc_status sc_index_last_wide(sc_index* ix, int32_t* wide) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (wide) *wide = ix->last_wide;
    return SC_OK;
}

extern "C" sc_status sc_index_last_probe_stats(sc_index* ix, int64_t* unique_rows, int64_t* streamed_rows, int32_t* groups) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (unique_rows) *unique_rows = ix->last_unique_rows;
    if (streamed_rows) *streamed_rows = ix->last_streamed_rows;
    if (groups) *groups = ix->last_groups;
    return SC_OK;
}

// ------------------------------------------------------------------ host merge of per-shard results

extern "C" sc_status sc_topk_merge_host(sc_metric metric, int32_t lists, int32_t Q, int32_t k, const float* dist, const int64_t* rows,
                                        float* out_dist, int64_t* out_rows) {
    if (lists < 1 || Q < 1 || k < 1 || !dist || !rows || !out_dist || !out_rows) return sc_fail(SC_ERR_INVALID, "sc_topk_merge_host: bad argument");
    struct Ent { uint32_t u; int64_t row; float d; };
    std::vector<Ent> v;
    v.reserve((size_t)lists * k);
    for (int q = 0; q < Q; ++q) {
        v.clear();
        for (int l = 0; l < lists; ++l)
            for (int j = 0; j < k; ++j) {
                const size_t o = ((size_t)l * Q + q) * k + j;
                if (rows[o] < 0) continue;
                float x = (metric == SC_METRIC_L2) ? dist[o] : -dist[o];
                x = x + 0.0f;
                uint32_t u;
                memcpy(&u, &x, 4);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                v.push_back({u, rows[o], dist[o]});
            }
        std::sort(v.begin(), v.end(), [](const Ent& a, const Ent& b) { return a.u != b.u ? a.u < b.u : a.row < b.row; });
        for (int j = 0; j < k; ++j) {
            const size_t o = (size_t)q * k + j;
            if (j < (int)v.size()) {
                out_dist[o] = v[j].d;
                out_rows[o] = v[j].row;
            } else {
                out_dist[o] = (metric == SC_METRIC_L2) ? INFINITY : -INFINITY;
                out_rows[o] = -1;
            }
        }
    }
    return SC_OK;
}
