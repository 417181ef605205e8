// sc_encoder_heads.cpp -- what runs behind the packed forward instead of plain pooling: the three heads of a handle and their calls.
// Pairs of a cross-encoder (set_pair_head / score_pairs, arch 0; encoder_pairs.hip), sequences of the other two families' rerankers
// (set_score_head / score_seqs: [CLS] or masked mean of final_norm on arch 1, RMS_final of the last token on arch 2; encoder_heads.hip) and
// late interaction (set_token_head / embed_tokens / embed_tokens_into / score_late: the token head on every row asked for -- to the host, or
// straight into the token pool of an index --, MaxSim over those vectors; encoder_tokens.hip).  What each call's batch is travels to the forward as a PackedCall (sc_encoder_plan.h).
#include <vector>

#include "sc_encoder_state.h"

// One array of a head: the pointer of the fresh head that receives it, its host values (NULL: the array is absent, the pointer stays NULL), their
// count, and whether the device holds them as f32 or rounded to bf16
struct HeadPart {
    void** slot;
    const float* src;
    size_t n;
    bool bf16;
    template <class T>
    HeadPart(T** slot, const float* src, size_t n, bool bf16 = false) : slot((void**)slot), src(src), n(n), bf16(bf16) {}
};

// Installs the head `fresh` with the arrays `parts` (their slots lie in *fresh) in place of *installed; `what` names it in the messages.
// Measures over an Arena, allocates, places, uploads while keeping the first error -- a bf16 array through an f32 staging copy, rounded once on
// device as every encoder weight -- and synchronises: the caller's arrays are free on return and nothing still reads the head that goes.
// On failure the fresh allocation is freed and *installed stays; on success the old one is freed.  No parts: the head is removed.
// Takes e->mu; `swapped`, if given, runs behind the exchange under the same hold (the stream is drained by then).
template <class Head>
static sc_status install_head(sc_encoder* e, Head* installed, Head* fresh, const std::vector<HeadPart>& parts, const char* what,
                              void (*swapped)(sc_encoder*) = nullptr) {
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    hipStream_t s = e->rt->stream;
    if (parts.empty()) {
        SC_HIP(hipStreamSynchronize(s));
    } else {
        Arena head, stage;
        std::vector<void*> dst(parts.size());
        std::vector<float*> stg(parts.size());
        auto lay = [&] {
            for (size_t i = 0; i < parts.size(); ++i) {
                const HeadPart& p = parts[i];
                dst[i] = !p.src ? nullptr : p.bf16 ? head.bf16(p.n) : head.f32(p.n);
                stg[i] = p.src && p.bf16 ? stage.f32(p.n) : nullptr;
            }
        };
        lay();  // measure
        sc_devbuf staging;
        if (stage.used && staging.alloc(stage.used) != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc %s staging (%zu B) failed", what, stage.used);
        hipError_t he = hipMalloc((void**)&fresh->mem, head.used);
        if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc %s (%zu B) failed: %s", what, head.used, hipGetErrorString(he));
        head = Arena{fresh->mem};
        stage = Arena{(char*)staging.p};
        lay();  // place
        hipError_t up = hipSuccess;
        for (size_t i = 0; i < parts.size(); ++i) {
            const HeadPart& p = parts[i];
            *p.slot = dst[i];
            if (!p.src || up != hipSuccess) continue;
            up = hipMemcpyAsync(p.bf16 ? (void*)stg[i] : dst[i], p.src, p.n * 4, hipMemcpyHostToDevice, s);
            if (p.bf16 && up == hipSuccess) {
                sc_launch_f32_to_bf16(stg[i], dst[i], (int64_t)p.n, s);
                up = hipGetLastError();
            }
        }
        const hipError_t sy = hipStreamSynchronize(s);
        if (up == hipSuccess) up = sy;
        if (up != hipSuccess) {
            hipFree(fresh->mem);
            return sc_fail(SC_ERR_HIP, "%s upload failed: %s", what, hipGetErrorString(up));
        }
    }
    hipFree(installed->mem);
    *installed = *fresh;
    if (swapped) swapped(e);
    return SC_OK;
}

// the logits [B, labels] of the head that was just launched and, if asked for, the rows it read, to the host (asynchronously)
static sc_status logits_to_host(sc_encoder* e, int32_t B, int labels, float* out_logits, float* out_rows) {
    hipStream_t s = e->rt->stream;
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(out_logits, e->logits, (size_t)B * labels * 4, hipMemcpyDeviceToHost, s));
    if (out_rows) SC_HIP(hipMemcpyAsync(out_rows, e->pooled, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, s));
    return SC_OK;
}

// ------------------------------------------------------------------ pairs (cross-encoder / reranker)
extern "C" sc_status sc_encoder_set_pair_head(sc_encoder* e, const float* pooler_w, const float* pooler_b, const float* cls_w, const float* cls_b,
                                              int32_t num_labels) {
    if (!e) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: NULL encoder");
    const size_t H = (size_t)e->cfg.hidden;
    PairHead fresh;
    std::vector<HeadPart> parts;
    if (cls_w) {
        if (num_labels < 1 || num_labels > 2) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: num_labels %d outside 1 .. 2", num_labels);
        if (!cls_b) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: cls_b is NULL");
        if (pooler_w && !pooler_b) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: pooler_b is NULL");
        if (!sc_pair_head_supported((int)H, num_labels)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_set_pair_head: hidden %d must be a multiple of 16, at most 2048", (int)H);
        fresh.labels = num_labels;
        parts = {{&fresh.wp, pooler_w, H * H}, {&fresh.bp, pooler_w ? pooler_b : nullptr, H}, {&fresh.wc, cls_w, (size_t)num_labels * H},
                 {&fresh.bc, cls_b, (size_t)num_labels}};
    }
    return install_head(e, &e->pair, &fresh, parts, "pair head");
}

extern "C" sc_status sc_encoder_score_pairs(sc_encoder* e, const int32_t* ids, const int64_t* offsets, const int32_t* first_lens, int32_t B,
                                            float* out_logits, float* out_cls) {
    const char* who = "sc_encoder_score_pairs";
    if (!e || !ids || !offsets || !first_lens || !out_logits) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 1)  // ModernBERT's classifier is dense -> GELU -> LayerNorm -> linear; pair_head_kernel is pooler + tanh
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 1 (pre-LN) models have no pair head: their classifier is not pooler + linear", who);
    if (e->cfg.arch == 2)  // no segment ids, no [CLS] row, no pooler: rerankers of this family are out of scope
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models do not score pairs: the family has no [CLS] row and no pair head", who);
    if (e->cfg.arch == 3) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 3 (T5 encoder) models are embedding models only here: no pair, score or token head (seq2seq rerankers are out of scope)", who);
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, who, &used);
    if (!st) st = sc_plan_check_pairs(offsets, first_lens, B, plan_bounds(e), who);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->pair.mem) return sc_fail(SC_ERR_INVALID, "%s: no pair head installed (sc_encoder_set_pair_head)", who);
    return packed_call_locked(e, ids, offsets, B, used, PackedCall::pairs(first_lens), nullptr, false, [&](const int64_t*) {
        const PairHead& h = e->pair;
        sc_launch_pair_head(e->pooled, B, e->cfg.hidden, h.wp, h.bp, h.wc, h.bc, h.labels, e->logits, e->rt->stream);
        return logits_to_host(e, B, h.labels, out_logits, out_cls);
    });
}

// ------------------------------------------------------------------ the output projection behind the pooling (every arch; embedding calls only)
extern "C" sc_status sc_encoder_set_output_proj(sc_encoder* e, const float* W, const float* b, int32_t E) {
    const char* who = "sc_encoder_set_output_proj";
    if (!e) return sc_fail(SC_ERR_INVALID, "%s: NULL encoder", who);
    const size_t H = (size_t)e->cfg.hidden;
    OutProj fresh;
    std::vector<HeadPart> parts;
    if (W) {
        if (E < 16 || E > 2048 || (E % 16)) return sc_fail(SC_ERR_INVALID, "%s: E = %d must be a multiple of 16 within 16 .. 2048", who, E);
        if (!sc_output_proj_supported((int)H, E)) return sc_fail(SC_ERR_UNSUPPORTED, "%s: hidden %d must be a multiple of 16, at most 2048", who, (int)H);
        fresh.E = E;
        parts = {{&fresh.w, W, (size_t)E * H}, {&fresh.b, b, (size_t)E}};
    }
    // the workspace holds the projected rows of a batch: dropped in the lock hold that exchanges the projection, so that no call sees one laid
    // out for the other; the next call lays it out again, with or without them
    return install_head(e, &e->proj, &fresh, parts, "output projection", [](sc_encoder* enc) {
        hipFree(enc->ws);
        enc->ws = nullptr;
        enc->projected = nullptr;
        enc->ws_tokens = 0;
        enc->ws_batch = 0;
    });
}
extern "C" sc_status sc_encoder_out_dim(sc_encoder* e, int32_t* out) {
    if (!e || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_out_dim: NULL argument");
    std::lock_guard<std::mutex> g(e->mu);
    *out = out_width(e);
    return SC_OK;
}

// ------------------------------------------------------------------ score heads of the arch 1 / arch 2 rerankers
// arch: the encoder's, or -1 (sc_diag_score_head: the kernels alone, any kind, pooling not read)
sc_status sc_score_head_check(const sc_score_head* h, int arch, int H, const char* who) {
    if (arch == 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 0 (post-LN BERT family) models take the pooler + linear head of sc_encoder_set_pair_head / sc_encoder_score_pairs", who);
    if (arch == 3) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 3 (T5 encoder) models are embedding models only here: no pair, score or token head (seq2seq rerankers are out of scope)", who);
    if (h->kind != 1 && h->kind != 2)
        return sc_fail(SC_ERR_INVALID, "%s: unknown kind %d (1 = prediction head of the pre-norm family, 2 = linear head on the last token)", who, h->kind);
    if (arch > 0 && h->kind != arch)
        return sc_fail(SC_ERR_INVALID, "%s: kind %d needs an arch %d encoder, this one is arch %d (kind 1: arch 1, kind 2: arch 2)", who, h->kind, h->kind, arch);
    if (arch > 0 && h->kind == 1 && h->pooling != 0 && h->pooling != 1)
        return sc_fail(SC_ERR_INVALID, "%s: pooling %d is not valid for kind 1 (0 = masked mean, 1 = the first row)", who, h->pooling);
    if (arch > 0 && h->kind == 2 && h->pooling != 2) return sc_fail(SC_ERR_INVALID, "%s: pooling %d is not valid for kind 2 (must be 2, the last real token)", who, h->pooling);
    if (h->num_labels < 1 || h->num_labels > 2) return sc_fail(SC_ERR_INVALID, "%s: num_labels %d outside 1 .. 2", who, h->num_labels);
    if (!h->cls_w) return sc_fail(SC_ERR_INVALID, "%s: cls_w is NULL", who);
    if (h->kind == 1) {
        if (!h->dense_w) return sc_fail(SC_ERR_INVALID, "%s: dense_w is NULL (kind 1)", who);
        if (!h->norm_g) return sc_fail(SC_ERR_INVALID, "%s: norm_g is NULL (kind 1)", who);
        if (!(h->norm_eps > 0.f)) return sc_fail(SC_ERR_INVALID, "%s: norm_eps must be > 0 (kind 1), got %g", who, (double)h->norm_eps);
    } else if (h->dense_w || h->dense_b || h->norm_g || h->norm_b) {
        return sc_fail(SC_ERR_INVALID, "%s: dense_w / dense_b / norm_g / norm_b must be NULL on kind 2 (a linear head)", who);
    }
    if (!sc_score_head_supported(H, h->num_labels)) return sc_fail(SC_ERR_UNSUPPORTED, "%s: hidden %d must be a multiple of 16, at most 2048", who, H);
    return SC_OK;
}

extern "C" sc_status sc_encoder_set_score_head(sc_encoder* e, const sc_score_head* h) {
    const char* who = "sc_encoder_set_score_head";
    if (!e) return sc_fail(SC_ERR_INVALID, "%s: NULL encoder", who);
    const size_t H = (size_t)e->cfg.hidden;
    ScoreHead fresh;
    std::vector<HeadPart> parts;
    if (h) {
        sc_status st = sc_score_head_check(h, e->cfg.arch, (int)H, who);
        if (st) return st;
        fresh.kind = h->kind, fresh.pooling = h->pooling, fresh.labels = h->num_labels, fresh.eps = h->norm_eps;
        parts = {{&fresh.wd, h->dense_w, H * H}, {&fresh.bd, h->dense_b, H}, {&fresh.g, h->norm_g, H}, {&fresh.b, h->norm_b, H},
                 {&fresh.wc, h->cls_w, (size_t)h->num_labels * H}, {&fresh.bc, h->cls_b, (size_t)h->num_labels}};
    }
    return install_head(e, &e->score, &fresh, parts, "score head");
}

extern "C" sc_status sc_encoder_score_seqs(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, float* out_logits, float* out_rows) {
    const char* who = "sc_encoder_score_seqs";
    if (!e || !ids || !offsets || !out_logits) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 0 (post-LN BERT family) models score pairs through sc_encoder_set_pair_head / sc_encoder_score_pairs", who);
    if (e->cfg.arch == 3) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 3 (T5 encoder) models are embedding models only here: no pair, score or token head (seq2seq rerankers are out of scope)", who);
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, who, &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->score.mem) return sc_fail(SC_ERR_INVALID, "%s: no score head installed (sc_encoder_set_score_head)", who);
    return packed_call_locked(e, ids, offsets, B, used, PackedCall::scored(e->score.pooling), nullptr, false, [&](const int64_t*) {
        const ScoreHead& h = e->score;
        sc_launch_score_head(e->pooled, B, e->cfg.hidden, h.wd, h.bd, h.g, h.b, h.eps, h.wc, h.bc, h.labels, e->logits, e->rt->stream);
        return logits_to_host(e, B, h.labels, out_logits, out_rows);
    });
}

// ------------------------------------------------------------------ late interaction (ColBERT): token vectors and MaxSim
extern "C" sc_status sc_encoder_set_token_head(sc_encoder* e, const float* w, int32_t W) {
    const char* who = "sc_encoder_set_token_head";
    if (!e) return sc_fail(SC_ERR_INVALID, "%s: NULL encoder", who);
    if (e->cfg.arch == 2) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models have no token head: late interaction needs bidirectional token rows", who);
    if (e->cfg.arch == 3) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 3 (T5 encoder) models are embedding models only here: no pair, score or token head (seq2seq rerankers are out of scope)", who);
    const size_t H = (size_t)e->cfg.hidden;
    if (w && !sc_token_head_supported((int)H, W)) return sc_fail(SC_ERR_INVALID, "%s: W = %d must be a multiple of 16 within 16 .. 128", who, W);
    TokenHead fresh;
    std::vector<HeadPart> parts;
    if (w) {
        fresh.W = W;
        parts = {{&fresh.w, w, (size_t)W * H, true}};
    }
    return install_head(e, &e->token, &fresh, parts, "token head");
}


static sc_status grow_locked(sc_encoder* e, sc_encoder::Grown& g, size_t bytes) {
    if (bytes <= g.cap) return SC_OK;
    SC_HIP(hipStreamSynchronize(e->rt->stream));
    hipFree(g.p);
    g.p = nullptr;
    g.cap = 0;
    const size_t cap = (bytes + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    hipError_t he = hipMalloc((void**)&g.p, cap);
    if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc token buffer (%zu B) failed: %s", cap, hipGetErrorString(he));
    g.cap = cap;
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_tokens(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, int32_t expand_id, float* out,
                                             int32_t* out_counts) {
    const char* who = "sc_encoder_embed_tokens";
    if (!e || !ids || !offsets || !out || !out_counts) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 2) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models have no token head", who);
    int64_t used = 0, nrows = 0;
    sc_status st = sc_plan_check_tokens(offsets, B, expand_id, expand_id >= 0, plan_bounds(e), who, &used, &nrows);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->token.mem) return sc_fail(SC_ERR_INVALID, "%s: no token head installed (sc_encoder_set_token_head)", who);
    SC_HIP(hipSetDevice(e->rt->device));
    const size_t bytes = (size_t)nrows * e->token.W * 4;
    st = grow_locked(e, e->tok[1], bytes);
    if (st) return st;
    st = packed_call_locked(e, ids, offsets, B, used, PackedCall::tokens(expand_id, (float*)e->tok[1].p), nullptr, false, [&](const int64_t*) -> sc_status {
        SC_HIP(hipMemcpyAsync(out, e->tok[1].p, bytes, hipMemcpyDeviceToHost, e->rt->stream));
        return SC_OK;
    });
    if (st) return st;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        out_counts[i] = (int32_t)(expand_id >= 0 ? ceil32(len) : len);
    }
    return SC_OK;
}

// The documents' token call with the token head aimed at the tail of the index's token pool: the put of sc_tokens.cpp (sc_tok_put_*) whose
// step 3 is the forward.  The keep flags enter the plan (a dropped token's row maps to -1, the kept ones count up text after text), so the
// head writes exactly the vectors the host path would upload, in the pool's format, where the table is about to point.  Lock order:
// encoder, then index, as store_pooled_locked (sc_encoder_embed.cpp) takes them; both are held to the end -- the pool may not move
// under the forward.
extern "C" sc_status sc_encoder_embed_tokens_into(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, const uint8_t* keep, sc_index* ix,
                                                  const int64_t* rows, int32_t fmt, int32_t* out_counts) {
    const char* who = "sc_encoder_embed_tokens_into";
    if (!e || !ids || !offsets || !ix || !rows) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 2) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models have no token head", who);
    int64_t used = 0, nrows = 0;
    sc_status st = sc_plan_check_tokens(offsets, B, -1, false, plan_bounds(e), who, &used, &nrows);
    if (st) return st;
    if (ix->rt != e->rt) return sc_fail(SC_ERR_INVALID, "%s: encoder and index belong to different runtimes", who);
    std::vector<int32_t> counts((size_t)B);
    const int64_t total = sc_plan_kept_counts(offsets, B, keep, counts.data());  // (a text has at most 2 048 tokens: so has a row)
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->token.mem) return sc_fail(SC_ERR_INVALID, "%s: no token head installed (sc_encoder_set_token_head)", who);
    const int W = e->token.W;
    st = sc_tok_check_format(W, fmt, who);
    if (st) return st;
    std::lock_guard<std::mutex> gi(ix->mu);
    sc_tok_put put;
    st = sc_tok_put_check_locked(ix, rows, B, W, fmt, who, &put);
    if (st) return st;
    SC_HIP(hipSetDevice(e->rt->device));
    void* tail = nullptr;
    st = sc_tok_put_room_locked(ix, W, fmt, total, who, &put, &tail);
    if (st) return st;
    bool committed = false;
    auto commit = [&](const int64_t*) {
        committed = true;
        return sc_tok_put_commit_locked(ix, rows, B, counts.data(), put);
    };
    if (total > 0) {
        st = packed_call_locked(e, ids, offsets, B, used, PackedCall::kept_tokens(keep, tail, fmt), nullptr, false, commit);  // the one synchronisation is its last step
    } else {  // nothing is kept: the rows lose their tokens, no forward runs
        st = commit(nullptr);
        hipStream_t s = e->rt->stream;
        if (!st) SC_HIP(hipStreamSynchronize(s));
    }
    if (st) {
        if (!committed) sc_tok_put_abandon_locked(ix, put);  // (the stream is drained: nothing points at what the forward wrote)
        return st;
    }
    sc_tok_put_done_locked(ix);
    if (out_counts)
        for (int32_t i = 0; i < B; ++i) out_counts[i] = counts[(size_t)i];
    return SC_OK;
}

extern "C" sc_status sc_encoder_score_late(sc_encoder* e, const int32_t* q_ids, const int64_t* q_offsets, int32_t Bq, int32_t expand_id, const int32_t* d_ids,
                                           const int64_t* d_offsets, int32_t Bd, const uint8_t* d_keep, const int32_t* pair_q, const int32_t* pair_d, int32_t P,
                                           float* out_scores) {
    const char* who = "sc_encoder_score_late";
    if (!e || !q_ids || !q_offsets || !d_ids || !d_offsets || !pair_q || !pair_d || !out_scores) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 2) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models have no token head", who);
    if (P < 1) return sc_fail(SC_ERR_INVALID, "%s: P = %d pairs (needs at least 1)", who, P);
    int64_t q_used = 0, q_rows = 0, d_used = 0, d_rows = 0;
    sc_status st = sc_plan_check_tokens(q_offsets, Bq, expand_id, true, plan_bounds(e), who, &q_used, &q_rows);  // (queries, expanded or not)
    if (!st) st = sc_plan_check_tokens(d_offsets, Bd, -1, false, plan_bounds(e), who, &d_used, &d_rows);
    if (st) return st;
    for (int32_t p = 0; p < P; ++p)
        if (pair_q[p] < 0 || pair_q[p] >= Bq || pair_d[p] < 0 || pair_d[p] >= Bd)
            return sc_fail(SC_ERR_INVALID, "%s: pair %d = (%d, %d) outside the %d queries / %d documents", who, p, pair_q[p], pair_d[p], Bq, Bd);
    if (d_keep)
        for (int32_t i = 0; i < Bd; ++i) {
            bool any = false;
            for (int64_t j = d_offsets[i]; j < d_offsets[i + 1] && !any; ++j) any = d_keep[j] != 0;
            if (!any) return sc_fail(SC_ERR_INVALID, "%s: document %d has no kept token", who, i);
        }
    // token offsets of both sides, as the kernel reads them
    std::vector<int32_t> q_off((size_t)Bq + 1, 0), d_off((size_t)Bd + 1, 0);
    for (int32_t i = 0; i < Bq; ++i) {
        const int64_t len = q_offsets[i + 1] - q_offsets[i];
        q_off[(size_t)i + 1] = q_off[(size_t)i] + (int32_t)(expand_id >= 0 ? ceil32(len) : len);
    }
    for (int32_t i = 0; i <= Bd; ++i) d_off[(size_t)i] = (int32_t)d_offsets[i];

    std::lock_guard<std::mutex> g(e->mu);
    if (!e->token.mem) return sc_fail(SC_ERR_INVALID, "%s: no token head installed (sc_encoder_set_token_head)", who);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot &slot_q = e->pin[e->pin_next], &slot_d = e->pin[e->pin_next ^ 1];  // one plan slot per side
    st = pin_slot_wait(slot_q);
    if (st) return st;
    st = pin_slot_wait(slot_d);
    if (st) return st;
    const int W = e->token.W;
    Arena aux;
    int32_t *a_qoff = nullptr, *a_doff = nullptr, *a_pq = nullptr, *a_pd = nullptr;
    float* a_out = nullptr;
    uint8_t* a_keep = nullptr;
    auto lay = [&] {
        a_qoff = (int32_t*)aux.take(((size_t)Bq + 1) * 4);
        a_doff = (int32_t*)aux.take(((size_t)Bd + 1) * 4);
        a_pq = (int32_t*)aux.take((size_t)P * 4);
        a_pd = (int32_t*)aux.take((size_t)P * 4);
        a_out = aux.f32((size_t)P);
        a_keep = d_keep ? (uint8_t*)aux.take((size_t)d_rows) : nullptr;
    };
    lay();  // measure
    st = grow_locked(e, e->late_aux, aux.used);
    if (!st) st = grow_locked(e, e->tok[0], (size_t)q_rows * W * 4);
    if (!st) st = grow_locked(e, e->tok[1], (size_t)d_rows * W * 4);
    if (!st) st = ensure_ws(e, q_used > d_used ? q_used : d_used, Bq > Bd ? Bq : Bd);  // (both forwards in one workspace: no growth between them)
    if (st) return st;
    aux = Arena{e->late_aux.p};
    lay();  // place
    hipStream_t s = e->rt->stream;
    auto run = [&]() -> sc_status {
        SC_HIP(hipMemcpyAsync(a_qoff, q_off.data(), q_off.size() * 4, hipMemcpyHostToDevice, s));
        SC_HIP(hipMemcpyAsync(a_doff, d_off.data(), d_off.size() * 4, hipMemcpyHostToDevice, s));
        SC_HIP(hipMemcpyAsync(a_pq, pair_q, (size_t)P * 4, hipMemcpyHostToDevice, s));
        SC_HIP(hipMemcpyAsync(a_pd, pair_d, (size_t)P * 4, hipMemcpyHostToDevice, s));
        if (a_keep) SC_HIP(hipMemcpyAsync(a_keep, d_keep, (size_t)d_rows, hipMemcpyHostToDevice, s));
        sc_status r = embed_packed_locked(e, q_ids, q_offsets, Bq, q_used, slot_q, PackedCall::tokens(expand_id, (float*)e->tok[0].p));
        if (!r) r = embed_packed_locked(e, d_ids, d_offsets, Bd, d_used, slot_d, PackedCall::tokens(-1, (float*)e->tok[1].p));
        if (r) return r;
        sc_launch_maxsim((const float*)e->tok[0].p, a_qoff, (const float*)e->tok[1].p, a_doff, a_keep, a_pq, a_pd, P, W, a_out, s);
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(out_scores, a_out, (size_t)P * 4, hipMemcpyDeviceToHost, s));
        return SC_OK;
    };
    st = run();
    if (st) {
        hipStreamSynchronize(s);  // uploads from the caller's arrays and the slots may be in flight
        return st;
    }
    SC_HIP(hipStreamSynchronize(s));  // the one synchronisation of the call: the token vectors never left the device
    return SC_OK;
}
