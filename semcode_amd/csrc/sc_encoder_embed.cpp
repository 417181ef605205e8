// sc_encoder_embed.cpp -- the entry points that embed texts: token ids in, one pooled vector per text out, to the host or into an index.
// Mirrors (reference): embed_documents / embed_query of the provider (src/semcode/embeddings/providers.py:34-104).
// Rectangles [B, S] go to the workspace as they are.  A packed batch (sc_encoder_embed_packed*) is planned on the host into a pinned slot
// (sc_encoder_plan.h), uploaded in one copy and run with a PackedLayout (embed_packed_locked); the heads' calls take the same road.
// Also here: the pinned slots, sc_encoder_wait, and the knobs of a handle (set_path, set_pooling / get_pooling, sc_diag_encoder_read).
#include <cstring>

#include "sc_encoder_state.h"

static sc_status check_embed_args(sc_encoder* e, const void* ids, const void* lens, int32_t B, int32_t S, const void* out) {
    if (!e || !ids || !lens || !out) return sc_fail(SC_ERR_INVALID, "embed: NULL argument");
    if (B < 1 || B > 65536) return sc_fail(SC_ERR_INVALID, "embed: batch %d out of range", B);
    // (arch 2, 3: the head width is the configuration's, hidden need not be heads * head_dim -- only the rule for S is asked for)
    if (e->cfg.arch >= 2 ? !sc_attention_supported(S, 64, 1, 64) : !sc_attention_supported(S, e->cfg.hidden, e->cfg.heads, e->cfg.hidden / e->cfg.heads))
        return sc_fail(SC_ERR_UNSUPPORTED, "embed: sequence length %d not in {32,64,128,256,512,1024,2048} (pad on the host)", S);
    if (S > e->cfg.max_pos && e->cfg.pos_type != 1) return sc_fail(SC_ERR_INVALID, "embed: sequence length %d exceeds max_pos %d", S, e->cfg.max_pos);
    return SC_OK;
}

// the index of an _into call (`who`) takes this encoder's rows
static sc_status check_index(sc_encoder* e, sc_index* ix, const char* who) {
    if (ix->rt != e->rt) return sc_fail(SC_ERR_INVALID, "%s: encoder and index belong to different runtimes", who);
    if (ix->dim != out_width(e))
        return sc_fail(SC_ERR_INVALID, "%s: index dim %d != encoder %s %d", who, ix->dim, e->proj.mem ? "output projection width" : "hidden", out_width(e));
    return SC_OK;
}

// ... of sc_encoder_embed_ids_into and its _async form (`who`)
static sc_status check_into_args(sc_encoder* e, const void* ids, const void* lens, int32_t B, int32_t S, sc_index* ix, const int64_t* rows, const char* who) {
    if (!ix || !rows) return sc_fail(SC_ERR_INVALID, "%s: NULL index / rows", who);
    sc_status st = check_embed_args(e, ids, lens, B, S, rows);
    return st ? st : check_index(e, ix, who);
}

// Host ids [B,S] and lens [B] (pageable, or a pinned slot) into the workspace, forward into e->pooled.  Caller holds e->mu and has
// set the device; nothing is synchronised.
static sc_status embed_host_locked(sc_encoder* e, const void* ids, const void* lens, int32_t B, int32_t S) {
    sc_status st = ensure_ws(e, (int64_t)B * S, B);
    if (st) return st;
    hipStream_t s = e->rt->stream;
    SC_HIP(hipMemcpyAsync(e->ids, ids, (size_t)B * S * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(e->lens, lens, (size_t)B * 4, hipMemcpyHostToDevice, s));
    return forward_locked(e, e->ids, e->lens, B, S, e->pooled);
}

// What an embedding call returns for the B rows in e->pooled: the rows themselves, or -- an output projection is installed, the forward left
// them un-normalised (out_normalize) -- their projection [B, E], normalised by the kernel, in `dst` (NULL: e->projected).  Enqueued, not synchronised.
static const float* finished_rows(sc_encoder* e, int32_t B, float* dst = nullptr) {
    if (!e->proj.mem) return e->pooled;
    if (!dst) dst = e->projected;
    sc_launch_output_proj(e->pooled, B, e->cfg.hidden, e->proj.w, e->proj.b, e->proj.E, e->cfg.normalize, dst, e->rt->stream);
    return dst;
}
// the finished rows into the index rows `rows`; lock order: encoder, then index (nothing takes them the other way round)
static sc_status store_pooled_locked(sc_encoder* e, sc_index* ix, const int64_t* rows, int32_t B, const char* who, const float** done = nullptr) {
    const float* v = finished_rows(e, B);
    if (done) *done = v;
    std::lock_guard<std::mutex> gi(ix->mu);
    return sc_index_put_rows_locked(ix, v, true, rows, B, who);
}
// ... and to the host (asynchronously); `v`: rows that are finished already
static sc_status pooled_to_host(sc_encoder* e, float* out, int32_t B, const float* v = nullptr) {
    if (!v) v = finished_rows(e, B);
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(out, v, (size_t)B * out_width(e) * 4, hipMemcpyDeviceToHost, e->rt->stream));
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_ids_dev(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S,
                                              float* out_dev) {
    sc_status st = check_embed_args(e, ids_dev, lens_dev, B, S, out_dev);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    st = ensure_ws(e, (int64_t)B * S, B);
    if (st) return st;
    if (!e->proj.mem) return forward_locked(e, ids_dev, lens_dev, B, S, out_dev);
    st = forward_locked(e, ids_dev, lens_dev, B, S, e->pooled);
    if (st) return st;
    finished_rows(e, B, out_dev);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_ids(sc_encoder* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, float* out) {
    sc_status st = check_embed_args(e, ids, lens, B, S, out);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    st = embed_host_locked(e, ids, lens, B, S);
    if (st) return st;
    hipStream_t s = e->rt->stream;
    st = pooled_to_host(e, out, B);
    if (st) return st;
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_ids_into(sc_encoder* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, sc_index* ix,
                                               const int64_t* rows, float* out) {
    sc_status st = check_into_args(e, ids, lens, B, S, ix, rows, "sc_encoder_embed_ids_into");
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    st = embed_host_locked(e, ids, lens, B, S);
    if (st) return st;
    hipStream_t s = e->rt->stream;
    const float* done = nullptr;
    st = store_pooled_locked(e, ix, rows, B, "sc_encoder_embed_ids_into", &done);
    if (st) {
        hipStreamSynchronize(s);  // drain the stream before the upsert error is reported
        return st;
    }
    if (out) SC_HIP(hipMemcpyAsync(out, done, (size_t)B * out_width(e) * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

// wait for the batch that last used `slot` (its inputs may be overwritten afterwards); reports a failure of that batch's device work
sc_status pin_slot_wait(sc_encoder::PinSlot& slot) {
    if (!slot.busy) return SC_OK;
    slot.busy = false;
    hipError_t he = hipEventSynchronize(slot.done);
    if (he != hipSuccess) return sc_fail(SC_ERR_HIP, "asynchronous embed batch failed: %s", hipGetErrorString(he));
    return SC_OK;
}

// an idle slot with at least `need` bytes of pinned memory and its event
static sc_status pin_slot_reserve(sc_encoder::PinSlot& slot, size_t need) {
    if (need > slot.cap) {
        if (slot.host) hipHostFree(slot.host);
        slot.host = nullptr;
        slot.cap = 0;
        SC_HIP(hipHostMalloc((void**)&slot.host, need, hipHostMallocDefault));
        slot.cap = need;
    }
    if (!slot.done) SC_HIP(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_ids_into_async(sc_encoder* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, sc_index* ix,
                                                     const int64_t* rows) {
    sc_status st = check_into_args(e, ids, lens, B, S, ix, rows, "sc_encoder_embed_ids_into_async");
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);  // two batches may be in flight; the third waits for the first
    if (st) return st;
    const size_t ids_b = (size_t)B * S * 4, lens_b = sc_align256((size_t)B * 4), rows_b = (size_t)B * 8, need = sc_align256(ids_b) + lens_b + rows_b;
    st = pin_slot_reserve(slot, need);
    if (st) return st;
    char* h_ids = slot.host;
    char* h_lens = slot.host + sc_align256(ids_b);
    int64_t* h_rows = (int64_t*)(h_lens + lens_b);
    memcpy(h_ids, ids, ids_b);
    memcpy(h_lens, lens, (size_t)B * 4);
    memcpy(h_rows, rows, rows_b);
    st = embed_host_locked(e, h_ids, h_lens, B, S);  // (the workspace is grown only now: that synchronises, the wait above came first)
    if (st) return st;
    st = store_pooled_locked(e, ix, h_rows, B, "sc_encoder_embed_ids_into_async");
    if (st) return st;
    SC_HIP(hipEventRecord(slot.done, e->rt->stream));
    slot.busy = true;
    e->pin_next ^= 1;
    return SC_OK;
}

// ------------------------------------------------------------------ packed variable-length batches
sc_status check_packed_offsets(sc_encoder* e, const int64_t* offsets, int32_t B, const char* who, int64_t* rows) {
    if (!e) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    return sc_plan_check_offsets(offsets, B, plan_bounds(e), who, rows);
}

extern "C" sc_status sc_encoder_packed_rows(sc_encoder* e, const int64_t* offsets, int32_t B, int64_t* rows) {
    if (!rows) return sc_fail(SC_ERR_INVALID, "sc_encoder_packed_rows: NULL argument");
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, "sc_encoder_packed_rows", &used);
    if (st) return st;
    *rows = ceil256(used);
    return SC_OK;
}

// Plans the layout of host ids / offsets into `slot` (idle, the caller waited for it), uploads it and runs the forward: e->pooled receives one
// row per sequence, or (a token call) call.tok_out the token vectors.  index_rows (NULL or [B]) are copied behind the plan: *rows_out points at
// the copy.  Caller holds e->mu and has validated the offsets by the rules of `call`'s kind (`used` = the row count); nothing is synchronised.
sc_status embed_packed_locked(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, int64_t used, sc_encoder::PinSlot& slot, const PackedCall& call,
                              const int64_t* index_rows, const int64_t** rows_out) {
    const int64_t M = ceil256(used);
    const PlanOffsets po((size_t)M, (size_t)B, call.kind);
    sc_status st = pin_slot_reserve(slot, po.total + (size_t)B * 8);
    if (st) return st;
    PackedLayout pk{};
    pk.rows = (int)sc_plan_fill(ids, offsets, B, call, po, M, slot.host, pk.nitems);
    if (index_rows) {
        int64_t* h_rows = (int64_t*)(slot.host + po.total);
        memcpy(h_rows, index_rows, (size_t)B * 8);
        *rows_out = h_rows;
    }
    st = ensure_ws(e, M, B);
    if (st) return st;
    SC_HIP(hipMemcpyAsync(e->plan, slot.host, po.total, hipMemcpyHostToDevice, e->rt->stream));
    auto dev = [&](size_t at) { return (const int32_t*)(e->plan + at); };
    pk.pos = dev(po.pos);
    pk.starts = dev(po.starts);
    pk.items = dev(po.items);
    pk.call = call;
    pk.per_row = call.kind == PackedCall::PAIRS ? dev(po.types) : call.kind == PackedCall::TOKENS ? dev(po.dst) : nullptr;
    return forward_locked(e, dev(po.ids), dev(call.kind == PackedCall::PAIRS ? po.ones : po.lens), B, 0, e->pooled, &pk);
}

static sc_status check_packed_into_args(sc_encoder* e, const void* ids, const int64_t* offsets, int32_t B, sc_index* ix, const int64_t* rows, const char* who,
                                        int64_t* used) {
    if (!ix || !rows || !ids) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    sc_status st = check_packed_offsets(e, offsets, B, who, used);
    return st ? st : check_index(e, ix, who);
}

// The synchronous forms stage through the next pinned slot as well (after waiting for the batch that used it) and leave it idle.
extern "C" sc_status sc_encoder_embed_packed(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, float* out) {
    if (!ids || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_embed_packed: NULL argument");
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, "sc_encoder_embed_packed", &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    return packed_call_locked(e, ids, offsets, B, used, PackedCall{}, nullptr, false, [&](const int64_t*) { return pooled_to_host(e, out, B); });
}

extern "C" sc_status sc_encoder_embed_packed_into(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, sc_index* ix, const int64_t* rows,
                                                  float* out) {
    const char* who = "sc_encoder_embed_packed_into";
    int64_t used = 0;
    sc_status st = check_packed_into_args(e, ids, offsets, B, ix, rows, who, &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    return packed_call_locked(e, ids, offsets, B, used, PackedCall{}, rows, false, [&](const int64_t* h_rows) {
        const float* done = nullptr;
        sc_status r = store_pooled_locked(e, ix, h_rows, B, who, &done);
        return r || !out ? r : pooled_to_host(e, out, B, done);
    });
}

extern "C" sc_status sc_encoder_embed_packed_into_async(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, sc_index* ix,
                                                        const int64_t* rows) {
    const char* who = "sc_encoder_embed_packed_into_async";
    int64_t used = 0;
    sc_status st = check_packed_into_args(e, ids, offsets, B, ix, rows, who, &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    return packed_call_locked(e, ids, offsets, B, used, PackedCall{}, rows, true, [&](const int64_t* h_rows) { return store_pooled_locked(e, ix, h_rows, B, who); });
}

extern "C" sc_status sc_encoder_wait(sc_encoder* e) {
    if (!e) return sc_fail(SC_ERR_INVALID, "sc_encoder_wait: NULL encoder");
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_status first = SC_OK;
    for (auto& slot : e->pin) {
        sc_status st = pin_slot_wait(slot);
        if (st && !first) first = st;
    }
    return first;
}

extern "C" sc_status sc_encoder_set_path(sc_encoder* e, int32_t path) {
    if (!e || path < 0 || path > 2) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_path: path must be 0 (auto), 1 (batch pipeline) or 2 (small-batch pipeline)");
    std::lock_guard<std::mutex> g(e->mu);
    e->path = path;
    return SC_OK;
}

extern "C" sc_status sc_encoder_set_pooling(sc_encoder* e, int32_t pooling) {
    if (!e || pooling < 0 || pooling > (e->cfg.arch == 2 ? 2 : 1))
        return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pooling: pooling must be 0 (masked mean) or 1 ([CLS] row); 2 (the last token's row) needs an arch 2 encoder");
    if (e->cfg.arch == 2 && pooling == 1)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pooling: pooling 1 ([CLS] row) is refused on arch 2: a causal first token sees only itself; use 0 (mean) or 2 (last token)");
    std::lock_guard<std::mutex> g(e->mu);
    e->pooling = pooling;
    return SC_OK;
}

extern "C" sc_status sc_encoder_get_pooling(sc_encoder* e, int32_t* out) {
    if (!e || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_get_pooling: NULL argument");
    std::lock_guard<std::mutex> g(e->mu);
    *out = e->pooling;
    return SC_OK;
}

// Diagnostic: copy one workspace buffer of the last forward to the host (0 x, 1 y, 2 qkv, 3 ctx, 4 hm, 5 stat_a, 6 stat_b, 7 fin_a, 8 fin_b).
extern "C" sc_status sc_diag_encoder_read(sc_encoder* e, int32_t which, void* out, size_t nbytes) {
    if (!e || !out) return sc_fail(SC_ERR_INVALID, "sc_diag_encoder_read: NULL argument");
    std::lock_guard<std::mutex> g(e->mu);
    const void* src[9] = {e->x, e->y, e->qkv, e->ctx, e->hm, e->stat_a, e->stat_b, e->fin_a, e->fin_b};
    if (which < 0 || which > 8 || !src[which]) return sc_fail(SC_ERR_INVALID, "sc_diag_encoder_read: no such buffer");
    SC_HIP(hipSetDevice(e->rt->device));
    SC_HIP(hipStreamSynchronize(e->rt->stream));
    SC_HIP(hipMemcpy(out, src[which], nbytes, hipMemcpyDeviceToHost));
    return SC_OK;
}
