// sc_internal.h -- handle structs shared by the host-side translation units.
#pragma once
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <utility>
#include <vector>

#include "sc_common.h"

#define SC_PROF_SCAN 0
#define SC_PROF_MERGE 1
#define SC_PROF_GEMM 2
#define SC_PROF_ATTN 3
#define SC_PROF_CLASSES 4

sc_status sc_fail(sc_status code, const char* fmt, ...);

#define SC_HIP(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return sc_fail(SC_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct sc_runtime {
    // Lifetime: the creator holds one reference, every index / encoder / communicator created on the runtime holds one more.
    // sc_runtime_destroy drops the creator's; the stream and the struct go when the LAST reference does, so handles may be
    // destroyed in any order (a garbage-collected Index after Runtime.close(): DESIGN.md section 9).
    std::atomic<int> refs{1};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int profiling = 0;                            // 0 off; n >= 1: bracket every n-th launch of the encoder classes (all launches of the scan classes)
    unsigned prof_seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // launches seen per class since the last reset
    char name[256] = {0};
    int cus = 256;
    int64_t hbm = 0;
    std::mutex mu;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof[SC_PROF_CLASSES];
};

void sc_runtime_retain(sc_runtime* rt);
void sc_runtime_release(sc_runtime* rt);  // frees the runtime when the last reference is dropped
void sc_prof_begin(sc_runtime* rt, int which, hipEvent_t* a, hipEvent_t* b);
void sc_prof_end(sc_runtime* rt, int which, hipEvent_t a, hipEvent_t b);
// the pair around the launches that `launch` issues
template <class F>
static inline void sc_with_prof(sc_runtime* rt, int which, F&& launch) {
    hipEvent_t a, b;
    sc_prof_begin(rt, which, &a, &b);
    launch();
    sc_prof_end(rt, which, a, b);
}

// A growable device allocation: sc_grow makes room (contents lost), sc_buf_free returns it.
struct sc_buf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    template <class T> T* as() const { return (T*)p; }
};

// device allocation released on scope exit unless handed over with take()
struct sc_devbuf {
    void* p = nullptr;
    ~sc_devbuf() { hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
    template <class T> T* take() { T* q = (T*)p; p = nullptr; return q; }
};

// A lazily built per-row mirror of the corpus, indexed by stored position.  One life cycle for all three (sc_index_state.cpp):
// allocate for the capacity -> build rows [rows, n) -> zero the padding rows -> re-build the rows overwritten since ->
// move / zero / renumber on delete (sc_delete.cpp) -> invalidate when the layout changes.
struct sc_shadow {
    sc_buf arr[2];                 // bf16: {Xb}; int8: {Xq, xscale}; centred: {Xc8, xcs}
    size_t row_bytes[2] = {0, 0};  // ld * 2 | ld8, 4 | ld8, 16  (0: array not used)
    int64_t rows = 0;              // stored positions [0, rows) are valid
    int64_t tail_pad = 0;          // rows of zero padding kept beyond `rows` rounded up to 256 (centred: 256 -- a list's last tile reads up to 255 rows beyond its end)
    unsigned* maxima = nullptr;    // device: running maxima over the rows (xnorm_max | xnorm_max8 | list_stats, below)
    // Rows overwritten in place since the shadow was built (stored positions below `rows`): the next search re-builds the shadow rows of
    // exactly these instead of the whole shadow (8 ms int8 / 54 ms centred at 10M x 768 for one upsert batch of 128:
    // scripts/upsert_search_interleave.py).  The running maxima only grow in between, which keeps every bound valid; a full rebuild
    // (layout change, more than SC_SHADOW_DIRTY_MAX rows) clears the list.
    std::vector<int64_t> dirty;
    int stat_bit = 0;              // 1 | 2 | 4 in sc_index_last_delete_stats
};

struct sc_token_store;

struct sc_index {
    sc_runtime* rt = nullptr;
    int dim = 0, ld = 0;
    sc_metric metric = SC_METRIC_IP;
    sc_index_kind kind = SC_INDEX_FLAT;
    int nlist = 0;
    int64_t row_base = 0;
    int64_t n = 0, capacity = 0;
    float* X = nullptr;      // [capacity, ld]
    float* xnorm = nullptr;  // [capacity]
    bool trained = false;
    // scratch (grown on demand); every sc_buf of the index is listed in SC_INDEX_BUFS below
    sc_buf stage, qpad, qnorm, partial, io;
    // batched path: bf16 shadow of X (rows padded to 128), per-batch scratch.  arr[0] = Xb; maxima = xnorm_max: bits of max |x|^2
    sc_shadow sh_b16;
    // int8 coarse stage: int8 shadow (rows of ld8 = ld rounded up to 128 bytes, rows padded to 256) + per-row scale.
    // arr = {Xq, xscale}; maxima = xnorm_max8: bits of {max |x|^2, max |x - s q|^2, max relative}
    sc_shadow sh_i8;
    int coarse_mode = 0;                          // sc_index_set_coarse_stage: 0 auto (int8 first), 8 int8 only, 16 bf16 only
    bool i8_off = false;                          // the int8 certificate failed for most of a batch on this corpus: use the bf16 stage
    int last_coarse_bits = 0;                     // 8 / 16: coarse stage of the last batched search
    int last_uncert_i8 = 0;                       // queries the int8 stage handed on to the bf16 stage
    bool wide_i8 = false;                         // ... or rather: the int8 stage keeps EVERY key within its exact-score cut (up to 4 096 per query) -- tried before i8_off
    int last_wide = 0;                            // the last batched search ran the wide form
    bool i8_sticky = false;                       // ... but the bf16-first batch that followed cost more: int8 first from now on (search_batched_locked)
    double cost_i8_first = 0.0;                   // seconds per query of the batch that switched the int8 stage off (0 = none pending)
    bool collect_off8 = false, collect_off16 = false;  // the collect pass of that stage resolved less than half of a sub-batch: skip it on this corpus
    int last_collect_tried = 0, last_collect_resolved = 0;  // queries of the last batched search that went through a collect pass / that it answered
    sc_buf bscratch;
    sc_buf fb, fb2;                               // fallback staging (queries + results) of the first stage's uncertified queries; the same for the second stage (int8 -> bf16 -> exact)
    sc_buf tailbuf;                               // two [Q][k] result sets of a search that answers from the lists and from the tail (sc_search.cpp)
    int64_t last_tail_rows = 0;                   // rows the last search scanned behind the lists (0: none)
    // the uploaded allow words of a host-pointer search (sc_stage_host_locked); masked search (sc_masked.cpp): the bitset over stored
    // positions + per-block counts and their scan; sel, the ascending allowed stored positions
    sc_buf mask_words, mask_cnt, mask_sel;
    int64_t last_mask_allowed = 0, last_mask_scanned = 0;  // sc_index_last_mask_stats
    int last_mask_gathered = 0;
    // grouped search (sc_grouped.cpp): the caller's label per row, valid while n == group_rows (-1: none installed) -- not scratch;
    // the candidate lists, hit labels, counts, done flags and the exclusion bitset of a call
    sc_buf groups, group_scratch;
    int64_t group_rows = -1;
    int last_group_width0 = 0, last_group_continued = 0, last_group_rounds = 0;  // sc_index_last_group_stats
    int64_t last_group_scanned = 0;
    // MMR search (sc_mmr.cpp): the candidate lists, the candidate x candidate score matrices and the row -> position map of a call;
    // the smallest candidate count of the last call, a device word that sc_index_last_mmr_stats reads when asked (not scratch)
    sc_buf mmr_scratch, mmr_stat;
    int last_mmr_fetch = 0;
    bool mmr_stat_pending = false;                // the device word holds the last call's count
    int64_t last_mmr_scanned = 0;
    // lexical / hybrid search (sc_lexical.cpp): the caller's term rows [term_cap][term_T] uint16 in local row-number order, valid while
    // n == term_rows (-1: none installed) -- not scratch, grown with its contents kept; df [65536] + sum_dl behind it, recomputed when
    // lex_stat_dirty; the membership sets, partial lists, candidate lists and the bad-query flag of a call
    sc_buf terms, lex_stat, lex_scratch;
    int64_t term_rows = -1, term_cap = 0;
    int term_T = 0;
    bool lex_stat_dirty = true;
    int64_t last_lex_rows = 0, last_lex_bytes = 0;  // sc_index_last_lex_stats
    int last_lex_passes = 0;
    // late interaction (sc_tokens.cpp): the caller's token vectors per row -- a ragged pool and a (start, len) table in local
    // row-number order, NULL until the first sc_index_put_tokens / sc_index_reserve_tokens; not scratch, kept across deletes.
    // late_scratch: the partial lists of a search
    sc_token_store* tok = nullptr;
    sc_buf late_scratch;
    // IVF_FLAT (after sc_index_train): X / xnorm are stored list-major
    sc_index* quant = nullptr;                    // flat index over the nlist centroids (coarse quantizer)
    uint32_t* perm = nullptr;                     // device [ivf_rows]: stored position -> row id (insertion order)
    int64_t* list_off = nullptr;                  // device [nlist + 1]
    std::vector<uint32_t> inv_h;                  // host [ivf_rows]: row id -> stored position (get_rows / overwrite / re-layout)
    std::vector<int64_t> list_off_h;
    std::vector<int32_t> assign_h;                // host [ivf_rows]: list of every row in the lists (persistence, incremental upserts)
    int nlist_trained = 0;
    // Upserts into a trained index do not drop the lists (Milvus: upsert into an indexed collection, milvus_store.py:128).
    // Rows [0, ivf_rows) sit list-major at inv_h[row]; rows appended since sit behind them at position == row id; rows
    // overwritten in place since are listed in dirty_rows (their list may have changed).  The next search first assigns the
    // pending + dirty rows to the EXISTING centroids and re-orders the corpus once (sc_ivf_refresh_locked): no k-means.
    int64_t ivf_rows = 0;
    int64_t perm_rows = 0;                        // entries of `perm` (== ivf_rows unless sc_ivf_cover_tail_locked extended it)
    std::vector<int64_t> dirty_rows;
    sc_buf ivf_scratch;
    // int8 coarse stage of list-major probing (L2; ivf_coarse.hip): every list quantised relative to its centroid.
    // arr[0] = Xc8: [ivf_rows padded to 256][ld8] int8 of x - c_list; arr[1] = xcs: [rows][4] f32 per row: {|x - c_list|^2, int8 scale,
    // 2 |dx|, 2 (|x'| + |dx|)}; rows == ivf_rows when valid; maxima = list_stats: [nlist_trained][2] bits of {max |x' - xq|^2, max |x'|^2}
    // + [4] bits of max |x|^2 behind them (sc_ivfc_stats_words / sc_ivfc_xmax_slot below).  The TRAINED list count sizes it -- set_ivf and
    // assign_lists install any number of lists, whatever `nlist` the handle was created with --, so it is allocated by the full build
    // in ivfc_ensure_shadow and freed whenever lists are installed or dropped (sc_shadow_free_maxima).
    sc_shadow sh_c8;
    sc_shadow* const shadows[3] = {&sh_b16, &sh_i8, &sh_c8};
    static constexpr int64_t SC_SHADOW_DIRTY_MAX = 8192;
    sc_buf ivfc_scratch;
    bool ivfc_off = false;                        // the coarse stage left most of a batch uncertified on this index: probe exactly
    int last_ivfc_uncertified = 0;
    int last_probed_lists = 0;
    int64_t last_unique_rows = 0, last_streamed_rows = 0;  // sc_index_last_probe_stats
    int last_groups = 0;
    int search_mode = 0;                          // 0 auto, 1 exact only, 2 batched whenever supported, 3 / 4 IVF probe per query / list-major whenever trained
    int last_path = 0;                            // 1 exact, 2 batched, 3 ivf probe per query, 4 ivf probe list-major, 5 behind the int8 coarse stage, 6 masked, 7 grouped, 8 mmr, 9 lexical, 10 hybrid
    int last_uncertified = 0;
    // sc_index_last_delete_stats: what the last sc_index_delete_rows moved; bit sets (sc_shadow::stat_bit) of the shadows kept / dropped
    int64_t last_del_rows_moved = 0, last_del_bytes_moved = 0;
    int last_del_kept = 0, last_del_dropped = 0;
    double uncert_frac = -1.0;                    // share of queries the last batched exhaustive search had to re-run exactly (-1 = never ran)
    std::mutex mu;
};

// The scratch buffers of an index (the shadows' arrays are reached through sc_index::shadows).  released: sc_index_release_scratch frees
// it; the others are the small per-call query / result buffers and the caller's group labels, which stay.  sc_index_destroy frees all of them.
struct sc_index_buf { sc_buf sc_index::*buf; bool released; };
inline constexpr sc_index_buf SC_INDEX_BUFS[] = {
    {&sc_index::stage, true},   {&sc_index::partial, true},     {&sc_index::bscratch, true},     {&sc_index::fb, true},
    {&sc_index::fb2, true},     {&sc_index::tailbuf, true},     {&sc_index::ivf_scratch, true},  {&sc_index::ivfc_scratch, true},
    {&sc_index::mask_words, true}, {&sc_index::mask_cnt, true}, {&sc_index::mask_sel, true}, {&sc_index::group_scratch, true},
    {&sc_index::mmr_scratch, true}, {&sc_index::lex_scratch, true}, {&sc_index::late_scratch, true},
    {&sc_index::qpad, false},   {&sc_index::qnorm, false},      {&sc_index::io, false},          {&sc_index::groups, false},
    {&sc_index::mmr_stat, false},   {&sc_index::terms, false},      {&sc_index::lex_stat, false},
};

static inline int sc_ld8(const sc_index* ix) { return (ix->ld + 127) / 128 * 128; }  // int8 row stride: whole 128-byte K-tiles
// list_stats of the centred shadow (sc_index::sh_c8.maxima): two words per TRAINED list, then the bits of max |x|^2 (padded to 4 words)
static inline size_t sc_ivfc_stats_words(int nlist_trained) { return (size_t)nlist_trained * 2 + 4; }
static inline unsigned* sc_ivfc_xmax_slot(const sc_index* ix) { return ix->sh_c8.maxima + (size_t)ix->nlist_trained * 2; }
// Offsets of the pieces of one scratch allocation, each 256-byte aligned: o = carve(bytes) ...; carve.off is the total to sc_grow.
static inline size_t sc_align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct sc_carver {
    size_t off = 0;
    size_t operator()(size_t bytes) { const size_t o = off; off += sc_align256(bytes); return o; }
};
// A field set for the length of a scope (search_mode, coarse_mode, metric of an index under its lock): the old value returns on every way out.
template <class T>
struct sc_scoped_set {
    T& ref;
    const T saved;
    sc_scoped_set(T& r, T v) : ref(r), saved(r) { r = v; }
    ~sc_scoped_set() { ref = saved; }
    sc_scoped_set(const sc_scoped_set&) = delete;
};
// A/B knobs of the environment; every call site keeps the value in a function-local static (read once per process).
// sc_env_flag: a knob that is on by default goes off by a leading '0', one that is off by default goes on by a leading '1'.
static inline int64_t sc_env_i64(const char* name, int64_t dflt) { const char* e = getenv(name); return e ? (int64_t)atoll(e) : dflt; }
static inline bool sc_env_flag(const char* name, bool dflt) { const char* e = getenv(name); return !e ? dflt : dflt ? e[0] != '0' : e[0] == '1'; }

// sc_index_state.cpp (caller holds ix->mu)
sc_status sc_grow(sc_index* ix, sc_buf& b, size_t need);  // grow a device scratch buffer: synchronises, contents not preserved
void sc_buf_free(sc_buf& b);
void sc_shadow_invalidate(sc_shadow& sh);  // stale: the next ensure builds it whole (which covers the pending rows)
void sc_shadow_release(sc_shadow& sh);     // ... and its arrays and maxima are freed
void sc_shadow_free_maxima(sc_shadow& sh); // the maxima alone (the centred shadow's are sized by the trained list count); invalidates
void sc_invalidate_shadows(sc_index* ix);  // all three: the rows or their layout changed wholesale
// rows[i] (ids, rows below old_n existed before) were written at stored position pos[i]: remember those the shadow covers
void sc_shadow_note_overwritten(sc_shadow& sh, const int64_t* rows, const int64_t* pos, int64_t n, int64_t old_n);
sc_status sc_ensure_shadow_b16(sc_index* ix);  // bring the bf16 / int8 shadow up to date with rows [0, n)
sc_status sc_ensure_shadow_i8(sc_index* ix);
// sc_search.cpp
sc_status sc_prep_queries(sc_index* ix, const float* q_dev, int32_t Q);  // tight [Q, dim] queries padded into ix->qpad, their norms into ix->qnorm
// Staging of the R queries `which` of a batch that go through another pass: buf = [queries | dist | rows | index], queries gathered
struct sc_subbatch { float* q; float* d; int64_t* r; int32_t* idx; int R; };
sc_status sc_subbatch_stage(sc_index* ix, sc_buf& buf, const float* q_dev, const std::vector<int>& which, int k, sc_subbatch* sb);
sc_status sc_subbatch_scatter(sc_index* ix, const sc_subbatch& sb, int k, float* out_dist, int64_t* out_rows);  // results back to the batch's rows; synchronises

// sc_search_entry.cpp: what the search entry points share.
// The checks every one of them starts with, `who` being the prefix of the message ("masked search").  any_null: one of the call's
// pointers is NULL; k_max: the widest top_k (0: no upper bound).  Then the two checks of an optional bitset: before the lock that a
// word count comes with words, under it (the row count is the index's) that the words cover the rows.
sc_status sc_check_query_args(const char* who, bool any_null, int32_t Q, int32_t k, int32_t k_max);
sc_status sc_check_allow_null(const char* who, const void* allow, int64_t allow_words);
sc_status sc_check_allow_words(const char* who, const sc_index* ix, const void* allow, int64_t allow_words);
// Staging of a host-pointer search (caller holds ix->mu and has set the device): the device copies of the queries [Q, dim] (q may be
// NULL: none) and of the ceil(n / 32) allow words (allow may be NULL: io->allow is too), room for the [Q, k] results and `extra_bytes`
// more at a 256-byte boundary for the caller's own uploads.  Valid until the next staging on the index.  sc_fetch_host_locked copies
// the results to the caller and synchronises.
struct sc_host_io { float* q; float* dist; int64_t* rows; const uint32_t* allow; char* extra; };
sc_status sc_stage_host_locked(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint32_t* allow, size_t extra_bytes, sc_host_io* io);
sc_status sc_fetch_host_locked(sc_index* ix, const sc_host_io& io, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows);
// The exact top-k over every row through the exhaustive planner, whatever the layout: rows behind the lists of a trained index are
// scanned where they lie (nothing is folded in).
sc_status sc_search_exhaustive_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows);
// The candidate stage of the grouped, MMR and hybrid searches: the exact best-first top-W of every query over the allowed rows
// (allow_dev >= ceil(n / 32) device words: the masked search) or over all rows (NULL: the exhaustive search), lists [Q, W] on the
// device.  scanned / allowed (optional): rows the answering scan read per pass / rows that were eligible.
sc_status sc_candidates_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t W, const uint32_t* allow_dev, float* cand_dist, int64_t* cand_rows, int64_t* scanned,
                               int64_t* allowed);

// search and IVF internals shared between sc_search.cpp and sc_ivf_{build,probe,coarse}.cpp (caller holds ix->mu)
sc_status sc_search_dev_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows);
sc_status sc_search_flat_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows);
sc_status sc_ivf_search_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows);
bool sc_ivf_listmajor_applicable(const sc_index* ix, int Q, int k, int nprobe, bool flat_is_batched);
sc_status sc_ivf_search_listmajor_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows);
bool sc_ivf_coarse_applicable(const sc_index* ix, int Q, int k, int nprobe);
// chunk: which 4 096-query chunk of its batch this call answers (the forced failure "ivf_coarse_nomem" = 2 reads it)
sc_status sc_ivf_search_coarse_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows, int chunk = 0);
// Which exact probe answers a sub-batch of R queries -- the queries the coarse stage could not certify, a batch whose coarse stage
// could not run --: 4 list-major (two queries or more, and the gather merge holds nprobe k-lists), 3 per-query probing, 0 neither
// has a plan for (ld, k, nprobe).  Plain arithmetic (sc_diag_ivf_exact_path, tests/test_ivf_plan_host.py).
int sc_ivf_exact_probe_path(int ld, int R, int k, int nprobe, int cus);
sc_status sc_ivf_untrain_locked(sc_index* ix);  // restore insertion order, drop lists
void sc_ivf_drop_lists_locked(sc_index* ix);    // drop lists without restoring the order (the rows are about to be discarded)
sc_status sc_ivf_cover_tail_locked(sc_index* ix);  // extend perm over rows appended since the build (identity): exhaustive search only
sc_status sc_ivf_refresh_locked(sc_index* ix, bool keep_tail = false);  // fold rows upserted since the lists were built into them (no k-means);
                                                                        // keep_tail: only settle the overwritten rows -- if none left its list, appended rows stay a tail
// entries of ix->perm (0: no trained layout): a stored position below it reports perm[position], one at or beyond it is its own row id
static inline int64_t sc_perm_entries(const sc_index* ix) { return ix->perm ? (ix->perm_rows > 0 ? ix->perm_rows : ix->ivf_rows) : 0; }
// stored position of row `r` (trained layout installed: ix->perm != nullptr)
static inline int64_t sc_ivf_pos(const sc_index* ix, int64_t r) { return r < ix->ivf_rows ? (int64_t)ix->inv_h[(size_t)r] : r; }
// upsert body shared by sc_index_put_rows{,_dev} and sc_encoder_embed_ids_into; caller holds ix->mu and has set the device
sc_status sc_index_put_rows_locked(sc_index* ix, const float* vecs, bool vecs_on_device, const int64_t* rows, int64_t n, const char* who);
bool sc_ivf_applicable(const sc_index* ix, int Q, int nprobe);
// sc_masked.cpp: the masked search under the lock.  q_dev tight [Q, dim], allow_dev >= ceil(n / 32) words, outputs [Q, k] (k <= 1024):
// all device.  Synchronises the stream once (the allowed count).
sc_status sc_search_masked_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev, float* out_dist, int64_t* out_rows);
// sc_lexical.cpp: forget the term rows (sc_index_delete_rows renumbers the rows; sc_index_drop_terms)
void sc_lex_drop_locked(sc_index* ix);
// sc_tokens.cpp: the token store follows a delete -- the table is renumbered with the rows (del: the deleted row numbers, ascending),
// survivors keep their tokens, the deleted rows' tokens become dead (and are compacted away once dead > live); the store is freed
void sc_tok_delete_locked(sc_index* ix, const std::vector<int64_t>& del);
void sc_tok_free_locked(sc_index* ix);
// ... and the steps of a put (the comment at their definitions has the order): the checks that need no lock, then, under ix->mu with the
// device set, rows / format against the store, room (*tail = where `total` tokens of the store's format go), abandon (the store as it was
// before room; the stream is idle), commit (table repointed and uploaded, not synchronised), done (the automatic compaction)
struct sc_tok_put {
    std::vector<int64_t> sorted;  // the rows, ascending
    bool fresh = false;           // room created the store
    int W_before = 0, fmt_before = 0;
};
sc_status sc_tok_check_format(int32_t W, int32_t fmt, const char* who);
sc_status sc_tok_check_counts(const int32_t* counts, int64_t n, const char* who, int64_t* total);
sc_status sc_tok_put_check_locked(sc_index* ix, const int64_t* rows, int64_t n, int32_t W, int32_t fmt, const char* who, sc_tok_put* put);
sc_status sc_tok_put_room_locked(sc_index* ix, int32_t W, int32_t fmt, int64_t total, const char* who, sc_tok_put* put, void** tail);
void sc_tok_put_abandon_locked(sc_index* ix, const sc_tok_put& put);
sc_status sc_tok_put_commit_locked(sc_index* ix, const int64_t* rows, int64_t n, const int32_t* counts, const sc_tok_put& put);
void sc_tok_put_done_locked(sc_index* ix);
// sc_ivf_probe.cpp.  The nprobe nearest centroids of every query under the INDEX metric (the quantizer's own search; takes qz->mu):
// distances and list ids at the head of ix->ivf_scratch, grown to hold `extra_bytes` more behind them; `host`: the ids there too
// (synchronises).
struct sc_ivf_probes { float* dist; int64_t* lists; char* extra; };
sc_status sc_ivf_probe_quantizer_locked(sc_index* ix, const float* q_dev, int Q, int nprobe, size_t extra_bytes, sc_ivf_probes* out,
                                        std::vector<int64_t>* host = nullptr);
// What the host planners (sc_ivf_plan.h) read from the scan plans and the environment for (ld, k, nprobe) on `cus` compute units: the
// one derivation shared by the searches and sc_diag_ivf_plan.  plan / plan_res (optional): the narrow scan's streamed / resident form.
// false: the list-major probe cannot serve (ld, k, nprobe); pp->KP is valid either way.
struct IvfPlanParams;
bool sc_ivf_plan_params(int ld, int k, int nprobe, int cus, IvfPlanParams* pp, ScanPlan* plan = nullptr, ScanPlan* plan_res = nullptr);

// process-wide test / A-B knobs behind sc_diag_set_option (sc_api.cpp), each defined next to the code it steers
void sc_ivf_set_refresh_nomem(int v);  // sc_ivf_build.cpp
void sc_ivf_set_refine_cap(int v);     // sc_ivf_coarse.cpp
void sc_ivf_set_coarse_nomem(int v);
void sc_set_collect_pass(int v);       // sc_search.cpp
void sc_set_tighten(int v);
void sc_set_wide_force(int v);
void sc_set_ivf_tail_rows(int v);
void sc_set_delete_chunk_rows(int v);  // sc_delete.cpp
void sc_set_mask_gather(int v);        // sc_masked.cpp
void sc_set_group_width0(int v);       // sc_grouped.cpp
void sc_set_group_width1(int v);
void sc_set_mmr_chunk_q(int v);        // sc_mmr.cpp
void sc_set_lex_chunk_q(int v);        // sc_lexical.cpp
void sc_encoder_set_rope_fused(int v); // sc_encoder_forward.cpp
void sc_encoder_set_cls_prune(int v);  // sc_encoder_forward.cpp
