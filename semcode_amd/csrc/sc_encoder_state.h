// sc_encoder_state.h -- what the host files of the encoder share and nobody else sees: the handle, its weights and workspace, the layout
// of a packed batch on the device, the width helpers and the prototypes across sc_encoder_{model,forward,embed,heads}.cpp (DESIGN.md has
// the map).  The single-kernel harnesses (sc_diag_*) are in sc_encoder_diag.cpp, the device entry points in encoder_ops.h.
// Activations bf16 in HBM ([tokens, H] row-major, tokens padded to 256), weights bf16 [out, in], biases / norm parameters / tables f32.
#pragma once
#include <vector>

#include "encoder_ops.h"
#include "maxsim_rule.h"
#include "sc_encoder_plan.h"
#include "sc_internal.h"

struct LayerW {
    void* wqkv;  // bf16 [3H, H]; arch 2: [AW + 2 KV, H], AW = heads * head_dim, KV = kv_heads * head_dim
    float* bqkv; // [3H]; arch 2: [AW + 2 KV]
    void* wo;    // bf16 [H, H]; arch 2: [H, AW]
    float* bo;
    float *qng = nullptr, *kng = nullptr;  // arch 2 with qk_norm: the per-head RMSNorm gammas of Q and K, [head_dim] each
    float *ln1g, *ln1b;
    void* w1;    // bf16 [F, H]
    float* b1;
    void* w2;    // bf16 [H, F]
    float* b2;
    float *ln2g, *ln2b;
    // LayerNorm-folded copies for the batch pipeline (forward_folded): the LayerNorm in FRONT of a GEMM lives in its weights --
    // Wqkv' = Wqkv diag(gamma of the previous LayerNorm), W1' = W1 diag(ln1 gamma) -- and in two vectors per GEMM (gemm_bf16.hip)
    void *wqkv_f = nullptr, *w1_f = nullptr;
    float *c1q = nullptr, *c2q = nullptr, *c1f = nullptr, *c2f = nullptr;
    const float* g_prev = nullptr;  // gamma of the LayerNorm that produces this layer's input (embedding LN or the previous layer's ln2)
    float *bb_o = nullptr, *bb_2 = nullptr;  // bo + beta_prev, b2 + ln1 beta: the residual epilogues add the normalised residual's beta with the bias
};

// The three heads, a slot each: one device allocation (mem; NULL = no head installed), the arrays inside it (an absent array NULL) and the
// scalars.  install_head (sc_encoder_heads.cpp) is the only writer.
struct PairHead {  // cross-encoder (sc_encoder_set_pair_head): Wp [H,H] | bp [H] | Wc [labels,H] | bc [labels], f32; wp NULL = no pooler
    char* mem = nullptr;
    float *wp = nullptr, *bp = nullptr, *wc = nullptr, *bc = nullptr;
    int labels = 0;
};
struct ScoreHead {  // arch 1 / arch 2 reranker (sc_encoder_set_score_head): dense_w [H,H] | dense_b [H] | norm_g [H] | norm_b [H] | cls_w [labels,H] | cls_b [labels], f32
    char* mem = nullptr;
    float *wd = nullptr, *bd = nullptr, *g = nullptr, *b = nullptr, *wc = nullptr, *bc = nullptr;
    int kind = 0, pooling = 0, labels = 0;
    float eps = 0.f;
};
struct TokenHead {  // late interaction (sc_encoder_set_token_head): the projection [W, H] as bf16
    char* mem = nullptr;
    void* w = nullptr;
    int W = 0;
};

struct OutProj {  // the output projection behind the pooling (sc_encoder_set_output_proj): W [E,H] | b [E], f32; b NULL = none
    char* mem = nullptr;
    float *w = nullptr, *b = nullptr;
    int E = 0;
};

struct sc_encoder {
    sc_runtime* rt = nullptr;
    sc_encoder_cfg cfg{};
    char* params = nullptr;  // one device allocation holding every parameter
    float *wemb = nullptr, *pemb = nullptr, *temb = nullptr, *embg = nullptr, *embb = nullptr;
    float* slopes = nullptr;  // ALiBi head slopes (device) or NULL
    float *rope_cos = nullptr, *rope_sin = nullptr;  // rotary positions: [max_pos][32] f32 each (device) or NULL; arch 2 at head_dim 128: [max_pos][64]
    float *rope_cos_l = nullptr, *rope_sin_l = nullptr;  // arch 1: the table of the local layers (base rope_theta_local); the one above is the global layers'
    float *fing = nullptr, *finb = nullptr;              // arch 1: final_norm gamma / beta
    float* rel_tbl = nullptr;  // pos_type 3 (T5): the distance table of the bias attention, [heads][2 max_pos - 1] f32 (sc_rel_bias_table), one for all layers
    std::vector<LayerW> layers;
    // workspace for `ws_tokens` (multiple of 256) tokens
    int64_t ws_tokens = 0;
    char* ws = nullptr;
    void *x = nullptr, *x1 = nullptr, *y = nullptr, *qkv = nullptr, *ctx = nullptr, *hm = nullptr, *hg = nullptr;
    int32_t* ids = nullptr;
    int32_t* lens = nullptr;
    int32_t* ones = nullptr;  // arch 3: [ws_batch] lengths of 1, under which the last-token pooling kernel takes every text's FIRST row
    // packed batches: padded ids | positions | starts | lens | attention items (PlanOffsets), one upload per call.  Part of every
    // workspace, rectangle callers' too: 8 bytes per token row + 24 per sequence next to the 17-29 KiB a row's activations take
    char* plan = nullptr;
    float* pooled = nullptr;
    float* logits = nullptr;  // [ws_batch][2]
    int64_t ws_batch = 0;
    float *stat_a = nullptr, *stat_b = nullptr;  // [slots][ws_tokens][2] partial row sums of the two pre-LayerNorm tensors (folded pipeline)
    float *fin_a = nullptr, *fin_b = nullptr;    // [ws_tokens][2] their finalised (mu, rs)
    bool foldable = false;                       // shapes allow the folded pipeline (256-tile GEMMs, K % 256 == 0)
    int path = 0;                                // sc_encoder_set_path: 0 auto, 1 batch pipeline always, 2 small-batch pipeline always
    int pooling = 0;                             // sc_encoder_set_pooling: 0 masked mean, 1 the [CLS] / first row, 2 the last real token's row (arch 2)
    void* splitk = nullptr;  // f32 partial products of the split-K GEMMs, allocated on first use (splitk_scratch)
    static constexpr size_t SPLITK_BYTES = 64u << 20;
    // pinned host staging: the plan of one packed batch, or ids | lens | rows of one asynchronous rectangle batch, per slot
    struct PinSlot {
        char* host = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    } pin[2];
    int pin_next = 0;
    PairHead pair;
    OutProj proj;
    float* projected = nullptr;  // [ws_batch][proj.E] in the workspace: what the embedding entry points return when a projection is installed
    ScoreHead score;
    TokenHead token;
    // token vectors of sc_encoder_embed_tokens / sc_encoder_score_late: the queries' (0) and the documents' (1) [rows][W] f32, and the
    // pair call's offsets | keep flags | pair list | scores; each grows on demand and is kept
    struct Grown {
        char* p = nullptr;
        size_t cap = 0;
    } tok[2], late_aux;
    std::mutex mu;
};

// Where the sequences of a packed batch lie, for the position-aware steps of the forward (device pointers into e->plan), and what the batch
// is.  The forward takes it as a parameter: NULL = a [B, S] rectangle of texts.
struct PackedLayout {
    const int32_t *pos, *starts, *items;
    int nitems[3];
    int rows;  // token rows in use = the sum of ceil32(len_i); rows .. M are the tail
    PackedCall call;
    const int32_t* per_row;  // PAIRS: the segment id of every row; TOKENS: its compact output row, -1 for a row not asked for; else NULL
};
static inline bool pair_call(const PackedLayout* pk) { return pk && pk->call.kind == PackedCall::PAIRS; }
static inline bool scored_call(const PackedLayout* pk) { return pk && pk->call.kind == PackedCall::SCORED; }
static inline bool token_call(const PackedLayout* pk) { return pk && pk->call.kind == PackedCall::TOKENS; }
// [CLS] pooling applies to texts only: pairs take their [CLS] row whatever the mode, a scored call pools as its head says, a token call pools nothing
static inline bool cls_pooling(const sc_encoder* e, const PackedLayout* pk) { return e->pooling == 1 && (!pk || pk->call.kind == PackedCall::TEXTS); }
// the rows of a pair call and of a scored call are never L2-normalised
// ... and neither is the pooled row of a text when an output projection follows it: the projection kernel normalises its own output
static inline int out_normalize(const sc_encoder* e, const PackedLayout* pk) {
    return pair_call(pk) || scored_call(pk) || (e->proj.mem && (!pk || pk->call.kind == PackedCall::TEXTS)) ? 0 : e->cfg.normalize;
}
// the width of what an embedding entry point returns
static inline int out_width(const sc_encoder* e) { return e->proj.mem ? e->proj.E : e->cfg.hidden; }

// Lays the buffers of one device allocation out, each 256-byte aligned.  The layout code runs twice: over an arena without a base
// it only measures (every buffer comes back NULL, `used` is the size to allocate), over the allocation it hands out the pointers.
struct Arena {
    char* base = nullptr;
    size_t used = 0;
    void* take(size_t bytes) { const size_t o = used; used += sc_align256(bytes); return base ? base + o : nullptr; }
    float* f32(size_t n) { return (float*)take(n * 4); }
    void* bf16(size_t n) { return take(n * 2); }
};

// ffn_type 1 (GEGLU), 2 (SwiGLU) and 4 (tanh-GELU gate, T5 v1.1): W1 holds gate and up rows, an element-wise kernel sits between the two FFN GEMMs
static inline bool ffn_gated(const sc_encoder_cfg& c) { return c.ffn_type == 1 || c.ffn_type == 2 || c.ffn_type == 4; }
// arch 3 (T5) with head_dim 64 stated: heads of 64 whatever hidden / heads is (t5-v1.1-small: 512 hidden, 6 heads)
static inline bool t5_stated_heads(const sc_encoder_cfg& c) { return c.arch == 3 && c.head_dim == 64; }
// arch 2: heads of 64, or of 128 when cfg.head_dim says so; K and V have kv_heads of them (0 = heads), Q has heads of them -- the attention
// width AW, which need not be hidden at 128.  Every other model projects Q, K and V to hidden columns
static inline int head_width(const sc_encoder_cfg& c) { return c.arch == 2 && c.head_dim == 128 ? 128 : 64; }
static inline int64_t attn_width(const sc_encoder_cfg& c) { return c.arch == 2 || t5_stated_heads(c) ? (int64_t)c.heads * head_width(c) : (int64_t)c.hidden; }
static inline int64_t kv_width(const sc_encoder_cfg& c) { return c.arch == 2 ? (int64_t)(c.kv_heads > 0 ? c.kv_heads : c.heads) * head_width(c) : attn_width(c); }
// arch 1: layer l attends globally iff l % global_every == 0 (global_every 0 counts as 1: every layer global)
static inline bool layer_is_local(const sc_encoder_cfg& c, int l) { return c.arch == 1 && c.global_every > 1 && (l % c.global_every) != 0; }
static inline PlanBounds plan_bounds(const sc_encoder* e) {
    const sc_encoder_cfg& c = e->cfg;
    return PlanBounds{c.max_pos, c.pos_type, c.vocab, c.type_vocab, c.arch, c.global_every, c.local_window, MAXSIM_MAX_NQ};
}

// sc_encoder_model.cpp: the workspace for `rows` token rows (a rectangle's B * S, a packed batch's row count) of B sequences
sc_status ensure_ws(sc_encoder* e, int64_t rows, int64_t B);
// sc_encoder_forward.cpp: ids_dev [B,S], lens_dev [B] device pointers; out_dev [B,H] f32 device.  pk != NULL: a packed batch -- ids_dev holds
// one id per token row of the layout (M of them), S is unused.  Caller holds e->mu.
sc_status forward_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev, const PackedLayout* pk = nullptr);
// sc_encoder_embed.cpp: the packed rules on a handle; a pinned slot; one packed forward through a slot
sc_status check_packed_offsets(sc_encoder* e, const int64_t* offsets, int32_t B, const char* who, int64_t* rows);
sc_status pin_slot_wait(sc_encoder::PinSlot& slot);
sc_status embed_packed_locked(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, int64_t used, sc_encoder::PinSlot& slot, const PackedCall& call,
                              const int64_t* index_rows = nullptr, const int64_t** rows_out = nullptr);

// A packed forward through the next pinned slot, for a caller that holds e->mu: sets the device, waits for the batch that last used the
// slot, runs embed_packed_locked and then `tail(staged index rows)` -- what the call launches behind the forward and copies back, nothing
// synchronised -- and drains the stream before an error of either is reported (the slot's upload may be in flight).  Afterwards the call is
// complete and the slot idle, or (in_flight) the slot's event is recorded and the next call takes the other slot.
template <class Tail>
static sc_status packed_call_locked(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, int64_t used, const PackedCall& call,
                                    const int64_t* index_rows, bool in_flight, Tail&& tail) {
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    sc_status st = pin_slot_wait(slot);  // two batches may be in flight; the third waits for the first
    if (st) return st;
    hipStream_t s = e->rt->stream;
    const int64_t* h_rows = nullptr;
    st = embed_packed_locked(e, ids, offsets, B, used, slot, call, index_rows, &h_rows);
    if (!st) st = tail(h_rows);
    if (st) {
        hipStreamSynchronize(s);
        return st;
    }
    if (!in_flight) {
        SC_HIP(hipStreamSynchronize(s));
        return SC_OK;
    }
    SC_HIP(hipEventRecord(slot.done, s));
    slot.busy = true;
    e->pin_next ^= 1;
    return SC_OK;
}
