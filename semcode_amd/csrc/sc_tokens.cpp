// sc_tokens.cpp -- the multi-vector collection of the C ABI: the token store of an index (sc_index_put_tokens, _reserve_tokens,
// _put_tokens_dev, _compact_tokens, _get_tokens, _token_stats, _drop_tokens) and the two calls that score from it (sc_index_rerank_late,
// sc_index_search_late; kernels: scan_late.hip, rules: maxsim_rule.h, late_rule.h).  The token vectors are the caller's data parked on
// the device next to the rows, as the group labels and the term rows are, but keyed by local row number through a table, so that a
// delete renumbers them instead of dropping them (sc_tok_delete_locked, called by sc_index_delete_rows).  A put has three forms -- vectors
// from the host, vectors on the device (sc_index_put_tokens_dev, late_install_kernel) and vectors the encoder's token head writes straight
// into the pool (sc_encoder_embed_tokens_into) -- over one set of steps (sc_tok_put_*).
//
// Layout: pool = token vectors of W elements (f32 or bf16), appended to; table[row] = (start, len) in tokens, on the device with a
// host mirror that is the truth.  A put appends the new vectors and repoints the rows; what a row pointed to before is dead until a
// compaction gathers the live tokens in row order into a fresh pool.  The table follows the index's row count lazily: rows appended
// since the last token call get empty entries the next time the store is used.
#include <algorithm>
#include <vector>

#include "sc_internal.h"  // (first: the HIP runtime header, whose bit casts maxsim_rule.h uses in a device pass)
#include "late_rule.h"

struct sc_token_store {
    int W = 0, fmt = 0;              // W 0: nothing installed yet (sc_index_reserve_tokens came first)
    sc_buf pool;
    int64_t reserve = 0;             // tokens asked for by sc_index_reserve_tokens before the format was known
    int64_t used = 0, live = 0;      // tokens appended since the last compaction (live + dead); tokens some row points to
    int64_t rows_with = 0;
    sc_buf table;                    // device copy of tab[0, synced rows)
    std::vector<sc_tok_entry> tab;   // one entry per row of the index (after tok_follow_rows)
    int64_t dirty_from = INT64_MAX;  // entries at or beyond it differ from the device copy
};

static size_t tok_bytes(const sc_token_store* ts) { return (size_t)ts->W * (ts->fmt ? 2 : 4); }

void sc_tok_free_locked(sc_index* ix) {
    if (!ix->tok) return;
    sc_buf_free(ix->tok->pool);
    sc_buf_free(ix->tok->table);
    delete ix->tok;
    ix->tok = nullptr;
}

static sc_status alloc_dev(sc_devbuf& b, size_t bytes, const char* who, const char* what) {
    if (b.alloc(bytes) != hipSuccess) {
        (void)hipGetLastError();
        return sc_fail(SC_ERR_NOMEM, "%s: cannot allocate %zu bytes for %s", who, bytes, what);
    }
    return SC_OK;
}

// The host table gets an (empty) entry for every row appended since; the device copy is brought up to date.  May allocate: SC_ERR_NOMEM
// leaves both as they were, apart from the empty entries.
static sc_status tok_follow_rows(sc_index* ix, const char* who) {
    sc_token_store* ts = ix->tok;
    hipStream_t s = ix->rt->stream;
    const int64_t n = ix->n;
    if ((int64_t)ts->tab.size() < n) {
        ts->dirty_from = std::min<int64_t>(ts->dirty_from, (int64_t)ts->tab.size());
        ts->tab.resize((size_t)n, sc_tok_entry{0, 0, 0});
    }
    const size_t need = (size_t)n * sizeof(sc_tok_entry);
    if (need > ts->table.cap) {
        const size_t want = std::max(need, std::max((size_t)ix->capacity * sizeof(sc_tok_entry), ts->table.cap + ts->table.cap / 2));
        sc_devbuf nb;
        const sc_status st = alloc_dev(nb, want, who, "the token table");
        if (st) return st;
        SC_HIP(hipStreamSynchronize(s));
        sc_buf_free(ts->table);
        ts->table.p = nb.take<void>();
        ts->table.cap = want;
        ts->dirty_from = 0;
    }
    if (ts->dirty_from < n) {
        SC_HIP(hipMemcpyAsync(ts->table.as<sc_tok_entry>() + ts->dirty_from, ts->tab.data() + ts->dirty_from, (size_t)(n - ts->dirty_from) * sizeof(sc_tok_entry),
                              hipMemcpyHostToDevice, s));
        SC_HIP(hipStreamSynchronize(s));  // (the mirror may change once this returns)
    }
    ts->dirty_from = INT64_MAX;
    return SC_OK;
}

// The pool holds `tokens` tokens, contents kept.  SC_ERR_NOMEM: nothing changed.
static sc_status tok_grow_pool(sc_index* ix, int64_t tokens, bool geometric, const char* who) {
    sc_token_store* ts = ix->tok;
    const size_t need = (size_t)tokens * tok_bytes(ts);
    if (need <= ts->pool.cap) return SC_OK;
    const size_t want = geometric ? std::max(need, ts->pool.cap + ts->pool.cap / 2) : need;
    sc_devbuf nb;
    const sc_status st = alloc_dev(nb, want, who, "the token pool");
    if (st) return st;
    hipStream_t s = ix->rt->stream;
    if (ts->used > 0) SC_HIP(hipMemcpyAsync(nb.p, ts->pool.p, (size_t)ts->used * tok_bytes(ts), hipMemcpyDeviceToDevice, s));
    SC_HIP(hipStreamSynchronize(s));
    sc_buf_free(ts->pool);
    ts->pool.p = nb.take<void>();
    ts->pool.cap = want;
    return SC_OK;
}

// Live tokens in row order into a fresh pool; dead = 0 afterwards.  SC_ERR_NOMEM: nothing changed.
static sc_status tok_compact_locked(sc_index* ix, const char* who) {
    sc_token_store* ts = ix->tok;
    if (ts->W == 0 || ts->used == ts->live) return SC_OK;  // nothing is dead
    sc_status st = tok_follow_rows(ix, who);
    if (st) return st;
    hipStream_t s = ix->rt->stream;
    const int64_t n = (int64_t)ts->tab.size();
    std::vector<sc_tok_entry> nt((size_t)n);
    int64_t at = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int32_t len = ts->tab[(size_t)r].len;
        nt[(size_t)r] = sc_tok_entry{len ? at : 0, len, 0};
        at += len;
    }
    const size_t pool_want = (size_t)std::max<int64_t>(at + at / 4 + 1024, ts->reserve) * tok_bytes(ts);
    sc_devbuf np, ntab;
    st = alloc_dev(np, pool_want, who, "the compacted token pool");
    if (st) return st;
    st = alloc_dev(ntab, ts->table.cap, who, "the token table");
    if (st) return st;
    if (n > 0) {
        SC_HIP(hipMemcpyAsync(ntab.p, nt.data(), (size_t)n * sizeof(sc_tok_entry), hipMemcpyHostToDevice, s));
        sc_with_prof(ix->rt, SC_PROF_SCAN, [&] {
            sc_launch_late_gather(ts->table.as<sc_tok_entry>(), (const sc_tok_entry*)ntab.p, n, ts->pool.p, np.p, (int)tok_bytes(ts), ix->rt->cus, s);
        });
        SC_HIP(hipGetLastError());
    }
    SC_HIP(hipStreamSynchronize(s));
    sc_buf_free(ts->pool);
    ts->pool.p = np.take<void>();
    ts->pool.cap = pool_want;
    const size_t tcap = ts->table.cap;
    sc_buf_free(ts->table);
    ts->table.p = ntab.take<void>();
    ts->table.cap = tcap;
    ts->tab.swap(nt);
    ts->used = ts->live = at;
    return SC_OK;
}

// after a put or a delete: more dead than live tokens -> compact.  A compaction that cannot allocate is skipped: the store is valid as it is.
static void tok_auto_compact(sc_index* ix) {
    sc_token_store* ts = ix->tok;
    if (ts->used - ts->live > ts->live) (void)tok_compact_locked(ix, "token store");
}

void sc_tok_delete_locked(sc_index* ix, const std::vector<int64_t>& del) {
    sc_token_store* ts = ix->tok;
    if (!ts || del.empty()) return;
    const int64_t have = (int64_t)ts->tab.size();  // rows beyond it never had an entry: they are empty before and after
    size_t di = 0;
    int64_t w = 0;
    for (int64_t r = 0; r < have; ++r) {
        while (di < del.size() && del[di] < r) ++di;
        if (di < del.size() && del[di] == r) {
            if (ts->tab[(size_t)r].len) {
                ts->live -= ts->tab[(size_t)r].len;
                ts->rows_with -= 1;
            }
            continue;
        }
        ts->tab[(size_t)w++] = ts->tab[(size_t)r];
    }
    ts->tab.resize((size_t)w);
    ts->dirty_from = std::min<int64_t>(ts->dirty_from, std::min<int64_t>(del.front(), w));
    if (hipSetDevice(ix->rt->device) == hipSuccess) tok_auto_compact(ix);
}

static sc_status no_store(const char* who) { return sc_fail(SC_ERR_INVALID, "%s: the index holds no token vectors (sc_index_put_tokens)", who); }

// ---- a put, in the steps its three forms share (sc_index_put_tokens: vectors from the host; sc_index_put_tokens_dev: vectors on the device;
// sc_encoder_embed_tokens_into, sc_encoder_heads.cpp: vectors the token head writes).  One copy of every rule:
//   1. sc_tok_check_format / sc_tok_check_counts (no lock), sc_tok_put_check_locked: everything is validated before anything changes
//   2. sc_tok_put_room_locked: the table follows the rows, the pool holds used + total tokens -- the only step that may fail once work has
//      begun (SC_ERR_NOMEM), and it leaves the store as it was.  *tail = pool[used ...), where the caller's device work puts the vectors
//   3. the caller's copies or kernels into the tail: nothing points at it yet, so a failure there (sc_tok_put_abandon_locked) changes nothing
//   4. sc_tok_put_commit_locked: the rows' entries repointed, their runs uploaded, used advanced; the caller synchronises (the uploads read
//      the host table) and ends with sc_tok_put_done_locked, the automatic compaction
sc_status sc_tok_check_format(int32_t W, int32_t fmt, const char* who) {
    if (!maxsim_width_ok(W)) return sc_fail(SC_ERR_INVALID, "%s: W = %d must be a multiple of 16 within 16 .. %d", who, W, MAXSIM_MAX_W);
    if (fmt != 0 && fmt != 1) return sc_fail(SC_ERR_INVALID, "%s: fmt must be 0 (f32) or 1 (bf16), got %d", who, fmt);
    return SC_OK;
}

sc_status sc_tok_check_counts(const int32_t* counts, int64_t n, const char* who, int64_t* total) {
    *total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (counts[i] < 0 || counts[i] > LATE_MAX_TOKENS) return sc_fail(SC_ERR_INVALID, "%s: counts[%lld] = %d outside 0 .. %d", who, (long long)i, counts[i], LATE_MAX_TOKENS);
        *total += counts[i];
    }
    return SC_OK;
}

sc_status sc_tok_put_check_locked(sc_index* ix, const int64_t* rows, int64_t n, int32_t W, int32_t fmt, const char* who, sc_tok_put* put) {
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= ix->n) return sc_fail(SC_ERR_INVALID, "%s: rows[%lld] = %lld out of range [0,%lld)", who, (long long)i, (long long)rows[i], (long long)ix->n);
    put->sorted.assign(rows, rows + n);
    std::sort(put->sorted.begin(), put->sorted.end());
    if (std::adjacent_find(put->sorted.begin(), put->sorted.end()) != put->sorted.end()) return sc_fail(SC_ERR_INVALID, "%s: row numbers must be distinct", who);
    if (ix->tok && ix->tok->W != 0 && (ix->tok->W != W || ix->tok->fmt != fmt))
        return sc_fail(SC_ERR_INVALID, "%s: W=%d fmt=%d, the index holds tokens of W=%d fmt=%d (sc_index_drop_tokens first)", who, W, fmt, ix->tok->W, ix->tok->fmt);
    return SC_OK;
}

// (the caller has set the device)
sc_status sc_tok_put_room_locked(sc_index* ix, int32_t W, int32_t fmt, int64_t total, const char* who, sc_tok_put* put, void** tail) {
    put->fresh = !ix->tok;
    if (put->fresh) ix->tok = new sc_token_store();
    sc_token_store* ts = ix->tok;
    put->W_before = ts->W;
    put->fmt_before = ts->fmt;
    ts->W = W;
    ts->fmt = fmt;
    sc_status st = tok_follow_rows(ix, who);
    if (!st) st = tok_grow_pool(ix, std::max(ts->used + total, put->W_before == 0 ? ts->reserve : 0), true, who);
    if (st) {
        sc_tok_put_abandon_locked(ix, *put);
        return st;
    }
    *tail = ts->pool.as<char>() + (size_t)ts->used * tok_bytes(ts);
    return SC_OK;
}

// the store as it was before sc_tok_put_room_locked (the pool may have grown: its contents are the same).  The stream is idle.
void sc_tok_put_abandon_locked(sc_index* ix, const sc_tok_put& put) {
    if (put.fresh) {
        sc_tok_free_locked(ix);
        return;
    }
    ix->tok->W = put.W_before;
    ix->tok->fmt = put.fmt_before;
}

// the table: the rows' entries repointed at the tail, what they pointed to is dead
sc_status sc_tok_put_commit_locked(sc_index* ix, const int64_t* rows, int64_t n, const int32_t* counts, const sc_tok_put& put) {
    sc_token_store* ts = ix->tok;
    hipStream_t s = ix->rt->stream;
    int64_t at = ts->used;
    for (int64_t i = 0; i < n; ++i) {
        sc_tok_entry& e = ts->tab[(size_t)rows[i]];
        ts->live += counts[i] - e.len;
        ts->rows_with += (counts[i] > 0) - (e.len > 0);
        e = sc_tok_entry{counts[i] ? at : 0, counts[i], 0};
        at += counts[i];
    }
    ts->used = at;
    const std::vector<int64_t>& sorted = put.sorted;
    for (size_t i = 0; i < sorted.size();) {  // one copy per run of consecutive rows
        size_t j = i + 1;
        while (j < sorted.size() && sorted[j] == sorted[j - 1] + 1) ++j;
        SC_HIP(hipMemcpyAsync(ts->table.as<sc_tok_entry>() + sorted[i], ts->tab.data() + sorted[i], (j - i) * sizeof(sc_tok_entry), hipMemcpyHostToDevice, s));
        i = j;
    }
    return SC_OK;
}

void sc_tok_put_done_locked(sc_index* ix) { tok_auto_compact(ix); }

extern "C" sc_status sc_index_put_tokens(sc_index* ix, const int64_t* rows, int64_t n, const int32_t* counts, const float* vecs, int32_t W, int32_t fmt) {
    const char* who = "sc_index_put_tokens";
    if (!ix || n < 0 || (n > 0 && (!rows || !counts))) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    sc_status st = sc_tok_check_format(W, fmt, who);
    int64_t total = 0;
    if (!st) st = sc_tok_check_counts(counts, n, who, &total);
    if (st) return st;
    if (total > 0 && !vecs) return sc_fail(SC_ERR_INVALID, "%s: vecs is NULL", who);
    std::lock_guard<std::mutex> g(ix->mu);
    sc_tok_put put;
    st = sc_tok_put_check_locked(ix, rows, n, W, fmt, who, &put);
    if (st) return st;
    if (n == 0) return SC_OK;
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    // ---- room first: from here to the uploads nothing can fail but the allocations, which leave the store as it was
    void* tail = nullptr;
    st = sc_tok_put_room_locked(ix, W, fmt, total, who, &put, &tail);
    if (st) return st;
    // ---- the vectors behind the pool's contents
    std::vector<uint16_t> half;
    if (total > 0) {
        const void* src = vecs;
        if (fmt == 1) {
            half.resize((size_t)total * W);
            for (size_t i = 0; i < half.size(); ++i) half[i] = late_round_bf16(vecs[i]);
            src = half.data();
        }
        SC_HIP(hipMemcpyAsync(tail, src, (size_t)total * tok_bytes(ix->tok), hipMemcpyHostToDevice, s));
    }
    st = sc_tok_put_commit_locked(ix, rows, n, counts, put);
    if (st) return st;
    SC_HIP(hipStreamSynchronize(s));  // (the caller's arrays may go once this returns)
    sc_tok_put_done_locked(ix);
    return SC_OK;
}

extern "C" sc_status sc_index_put_tokens_dev(sc_index* ix, const int64_t* rows, int64_t n, const int32_t* counts, const float* vecs_dev, const int32_t* src, int32_t W,
                                             int32_t fmt) {
    const char* who = "sc_index_put_tokens_dev";
    if (!ix || n < 0 || (n > 0 && (!rows || !counts))) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    sc_status st = sc_tok_check_format(W, fmt, who);
    int64_t total = 0;
    if (!st) st = sc_tok_check_counts(counts, n, who, &total);
    if (st) return st;
    if (total > 0 && !vecs_dev) return sc_fail(SC_ERR_INVALID, "%s: vecs_dev is NULL", who);
    if (src)
        for (int64_t j = 0; j < total; ++j)
            if (src[j] < 0) return sc_fail(SC_ERR_INVALID, "%s: src[%lld] = %d is not a token of vecs_dev", who, (long long)j, src[j]);
    std::lock_guard<std::mutex> g(ix->mu);
    sc_tok_put put;
    st = sc_tok_put_check_locked(ix, rows, n, W, fmt, who, &put);
    if (st) return st;
    if (n == 0) return SC_OK;
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    void* tail = nullptr;
    st = sc_tok_put_room_locked(ix, W, fmt, total, who, &put, &tail);
    if (st) return st;
    auto run = [&]() -> sc_status {  // the gather list behind the searches' scratch, the vectors into the tail, the table
        if (total > 0) {
            const int32_t* src_dev = nullptr;
            if (src) {
                const sc_status r = sc_grow(ix, ix->late_scratch, (size_t)total * 4);
                if (r) return r;
                SC_HIP(hipMemcpyAsync(ix->late_scratch.p, src, (size_t)total * 4, hipMemcpyHostToDevice, s));
                src_dev = ix->late_scratch.as<int32_t>();
            }
            sc_with_prof(ix->rt, SC_PROF_SCAN, [&] { sc_launch_late_install(vecs_dev, src_dev, total, W, fmt, tail, ix->rt->cus, s); });
            SC_HIP(hipGetLastError());
        }
        return SC_OK;
    };
    st = run();
    if (st) {
        hipStreamSynchronize(s);
        sc_tok_put_abandon_locked(ix, put);
        return st;
    }
    st = sc_tok_put_commit_locked(ix, rows, n, counts, put);
    if (st) return st;
    SC_HIP(hipStreamSynchronize(s));  // (the caller's arrays may go once this returns)
    sc_tok_put_done_locked(ix);
    return SC_OK;
}

extern "C" sc_status sc_index_reserve_tokens(sc_index* ix, int64_t tokens) {
    const char* who = "sc_index_reserve_tokens";
    if (!ix || tokens < 0) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    if (!ix->tok) ix->tok = new sc_token_store();
    sc_token_store* ts = ix->tok;
    ts->reserve = std::max(ts->reserve, tokens);
    if (ts->W == 0) return SC_OK;  // sized by the first install, which fixes the format
    return tok_grow_pool(ix, tokens, false, who);
}

extern "C" sc_status sc_index_compact_tokens(sc_index* ix) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->tok) return SC_OK;
    SC_HIP(hipSetDevice(ix->rt->device));
    return tok_compact_locked(ix, "sc_index_compact_tokens");
}

extern "C" sc_status sc_index_drop_tokens(sc_index* ix) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->tok) return SC_OK;
    SC_HIP(hipSetDevice(ix->rt->device));
    SC_HIP(hipStreamSynchronize(ix->rt->stream));
    sc_tok_free_locked(ix);
    return SC_OK;
}

extern "C" sc_status sc_index_token_stats(sc_index* ix, int64_t* rows_with_tokens, int64_t* live, int64_t* dead, int32_t* W, int32_t* fmt, int64_t* pool_bytes) {
    if (!ix) return sc_fail(SC_ERR_INVALID, "index is NULL");
    std::lock_guard<std::mutex> g(ix->mu);
    const sc_token_store* ts = ix->tok;
    if (rows_with_tokens) *rows_with_tokens = ts ? ts->rows_with : 0;
    if (live) *live = ts ? ts->live : 0;
    if (dead) *dead = ts ? ts->used - ts->live : 0;
    if (W) *W = ts ? ts->W : 0;
    if (fmt) *fmt = ts ? ts->fmt : 0;
    if (pool_bytes) *pool_bytes = ts ? (int64_t)ts->pool.cap : 0;
    return SC_OK;
}

extern "C" sc_status sc_index_get_tokens(sc_index* ix, const int64_t* rows, int64_t n, int32_t* out_counts, float* out_vecs, int64_t cap_tokens) {
    const char* who = "sc_index_get_tokens";
    if (!ix || n < 0 || cap_tokens < 0 || (n > 0 && (!rows || !out_counts))) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    std::lock_guard<std::mutex> g(ix->mu);
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= ix->n) return sc_fail(SC_ERR_INVALID, "%s: rows[%lld] = %lld out of range [0,%lld)", who, (long long)i, (long long)rows[i], (long long)ix->n);
    const sc_token_store* ts = ix->tok;
    const int64_t have = ts ? (int64_t)ts->tab.size() : 0;
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) total += rows[i] < have ? ts->tab[(size_t)rows[i]].len : 0;
    if (out_vecs && total > cap_tokens) return sc_fail(SC_ERR_INVALID, "%s: the rows hold %lld tokens, out_vecs has room for %lld", who, (long long)total, (long long)cap_tokens);
    for (int64_t i = 0; i < n; ++i) out_counts[i] = rows[i] < have ? ts->tab[(size_t)rows[i]].len : 0;
    if (!out_vecs || total == 0) return SC_OK;  // (out_vecs NULL: the counts alone)
    SC_HIP(hipSetDevice(ix->rt->device));
    hipStream_t s = ix->rt->stream;
    const size_t tb = tok_bytes(ts);
    std::vector<uint16_t> half;
    if (ts->fmt == 1) half.resize((size_t)total * ts->W);
    char* dst = ts->fmt == 1 ? (char*)half.data() : (char*)out_vecs;
    int64_t at = 0;
    for (int64_t i = 0; i < n;) {  // one copy per run of rows whose tokens follow each other in the pool
        if (!out_counts[i]) { ++i; continue; }
        const int64_t start = ts->tab[(size_t)rows[i]].start;
        int64_t len = out_counts[i], j = i + 1;
        while (j < n && (!out_counts[j] || ts->tab[(size_t)rows[j]].start == start + len)) len += out_counts[j++];
        SC_HIP(hipMemcpyAsync(dst + (size_t)at * tb, ts->pool.as<char>() + (size_t)start * tb, (size_t)len * tb, hipMemcpyDeviceToHost, s));
        at += len;
        i = j;
    }
    SC_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < half.size(); ++i) out_vecs[i] = late_widen_bf16(half[i]);
    return SC_OK;
}

// ---- the two calls that score from the store
static sc_status check_questions(const char* who, const float* Q, const int32_t* q_off, int32_t Bq) {
    if (!Q || !q_off) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (Bq < 1 || Bq > 65536) return sc_fail(SC_ERR_INVALID, "%s: Bq=%d out of range 1 .. 65536", who, Bq);
    if (q_off[0] != 0) return sc_fail(SC_ERR_INVALID, "%s: q_off[0] must be 0", who);
    for (int32_t q = 0; q < Bq; ++q) {
        const int64_t nq = (int64_t)q_off[q + 1] - q_off[q];
        if (nq < 1 || nq > MAXSIM_MAX_NQ) return sc_fail(SC_ERR_INVALID, "%s: question %d has %lld token vectors (1 .. %d)", who, q, (long long)nq, MAXSIM_MAX_NQ);
    }
    return SC_OK;
}

// Q [q_off[Bq], W] and q_off [Bq + 1] uploaded behind the staging's own regions, `more` further bytes behind them
struct LateQuestions { float* Q; int32_t* q_off; char* more; };
static sc_status stage_questions(sc_index* ix, const float* Q, const int32_t* q_off, int32_t Bq, int32_t k, const uint32_t* allow, size_t more, sc_host_io* io,
                                 LateQuestions* lq) {
    hipStream_t s = ix->rt->stream;
    const size_t q_bytes = (size_t)q_off[Bq] * ix->tok->W * 4, o_bytes = (size_t)(Bq + 1) * 4;
    sc_carver carve;
    const size_t o_q = carve(q_bytes), o_o = carve(o_bytes), o_m = carve(more);
    const sc_status st = sc_stage_host_locked(ix, nullptr, Bq, k, allow, carve.off, io);
    if (st) return st;
    lq->Q = (float*)(io->extra + o_q);
    lq->q_off = (int32_t*)(io->extra + o_o);
    lq->more = io->extra + o_m;
    SC_HIP(hipMemcpyAsync(lq->Q, Q, q_bytes, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(lq->q_off, q_off, o_bytes, hipMemcpyHostToDevice, s));
    return SC_OK;
}

extern "C" sc_status sc_index_rerank_late(sc_index* ix, const float* Q, const int32_t* q_off, int32_t Bq, const int64_t* cand, int32_t C, float* out_scores) {
    const char* who = "sc_index_rerank_late";
    if (!ix || !cand || !out_scores) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    sc_status st = check_questions(who, Q, q_off, Bq);
    if (st) return st;
    if (C < 1 || C > LATE_MAX_C) return sc_fail(SC_ERR_INVALID, "%s: C must be 1..%d (got %d)", who, LATE_MAX_C, C);
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->tok || ix->tok->W == 0) return no_store(who);
    const size_t P = (size_t)Bq * C;
    std::vector<int64_t> local(P);
    for (size_t p = 0; p < P; ++p) {
        if (cand[p] != -1 && (cand[p] < ix->row_base || cand[p] >= ix->row_base + ix->n))
            return sc_fail(SC_ERR_INVALID, "%s: cand[%zu] = %lld is neither -1 nor a row of [%lld,%lld)", who, p, (long long)cand[p], (long long)ix->row_base,
                           (long long)(ix->row_base + ix->n));
        local[p] = cand[p] < 0 ? -1 : cand[p] - ix->row_base;
    }
    SC_HIP(hipSetDevice(ix->rt->device));
    st = tok_follow_rows(ix, who);
    if (st) return st;
    sc_token_store* ts = ix->tok;
    hipStream_t s = ix->rt->stream;
    sc_host_io io;
    LateQuestions lq;
    st = stage_questions(ix, Q, q_off, Bq, C, nullptr, P * 8, &io, &lq);  // (io.dist [Bq][C] takes the scores)
    if (st) return st;
    SC_HIP(hipMemcpyAsync(lq.more, local.data(), P * 8, hipMemcpyHostToDevice, s));
    sc_with_prof(ix->rt, SC_PROF_SCAN, [&] {
        sc_launch_late_rerank(lq.Q, lq.q_off, Bq, ts->pool.p, ts->fmt, ts->table.as<sc_tok_entry>(), (const int64_t*)lq.more, C, ts->W, io.dist, s);
    });
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(out_scores, io.dist, P * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" sc_status sc_index_search_late(sc_index* ix, const float* Q, const int32_t* q_off, int32_t Bq, int32_t k, const uint32_t* allow, int64_t allow_words,
                                          float* out_score, int64_t* out_rows) {
    const char* who = "sc_index_search_late";
    if (!ix || !out_score || !out_rows) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    sc_status st = check_questions(who, Q, q_off, Bq);
    if (st) return st;
    if (k < 1 || k > LATE_MAX_K) return sc_fail(SC_ERR_INVALID, "%s: top_k must be 1..%d (got %d)", who, LATE_MAX_K, k);
    st = sc_check_allow_null(who, allow, allow_words);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    if (!ix->tok || ix->tok->W == 0) return no_store(who);
    st = sc_check_allow_words(who, ix, allow, allow_words);
    if (st) return st;
    SC_HIP(hipSetDevice(ix->rt->device));
    st = tok_follow_rows(ix, who);
    if (st) return st;
    sc_token_store* ts = ix->tok;
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    int nq_max = 1;
    for (int32_t q = 0; q < Bq; ++q) nq_max = std::max(nq_max, q_off[q + 1] - q_off[q]);
    // the partial lists of one question (the widest grid any of them takes) and the levels of their merge
    const int nwg_max = sc_late_scan_workgroups(ix->n, 1, ts->W, k, rt->cus);
    st = sc_grow(ix, ix->late_scratch, 256 + (size_t)nwg_max * 4 * k * 8 + sc_topk_merge_scratch_bytes(nwg_max * 4, 1, k) + 256);
    if (st) return st;
    sc_host_io io;
    LateQuestions lq;
    st = stage_questions(ix, Q, q_off, Bq, k, allow, 0, &io, &lq);
    if (st) return st;
    unsigned* next_block = ix->late_scratch.as<unsigned>();  // the scan's work counter, then the partial lists
    uint64_t* partial = (uint64_t*)(ix->late_scratch.as<char>() + 256);
    for (int32_t q = 0; q < Bq; ++q) {
        const int nq = q_off[q + 1] - q_off[q];
        const int nwg = sc_late_scan_workgroups(ix->n, nq, ts->W, k, rt->cus);
        SC_HIP(hipMemsetAsync(next_block, 0, 4, s));
        sc_with_prof(rt, SC_PROF_SCAN, [&] {
            sc_launch_late_scan(lq.Q + (size_t)q_off[q] * ts->W, nq, ts->pool.p, ts->fmt, ts->table.as<sc_tok_entry>(), ix->n, io.allow, ts->W, k, nwg, partial, next_block,
                                s);
        });
        sc_with_prof(rt, SC_PROF_MERGE, [&] {
            sc_launch_topk_merge(SC_METRIC_IP, partial, 1, nwg * 4, 1, 1, k, ix->row_base, io.dist + (size_t)q * k, io.rows + (size_t)q * k, s);
        });
    }
    SC_HIP(hipGetLastError());
    return sc_fetch_host_locked(ix, io, Bq, k, out_score, out_rows);
}
