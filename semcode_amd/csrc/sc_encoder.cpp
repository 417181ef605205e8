// sc_encoder.cpp -- host side of the transformer-encoder entry points (include/semcode_hip.h).
//
// Mirrors (reference): the object EmbeddingProviderFactory.create() returns and its
// embed_documents / embed_query (src/semcode/embeddings/providers.py:34-104; third-party forward in
// llama.cpp): token ids in, one pooled vector per chunk out.  Tokenisation stays on the host side of
// the boundary (semcode_amd/embeddings/tokenizer.py).
//
// Forward per layer (BERT, post-LN):  QKV = X Wqkv^T + b  ->  attention  ->  Y = ctx Wo^T + bo + X
//   -> X1 = LN(Y) -> Hm = gelu(X1 W1^T + b1) -> Y2 = Hm W2^T + b2 + X1 -> X = LN(Y2); pooled = masked mean, or (sc_encoder_set_pooling 1)
//   the [CLS] row -- the last layer then runs on the [CLS] rows only from its attention on (cls_last_layer, encoder_cls.hip).
// Activations bf16 in HBM ([tokens, H] row-major, tokens padded to 128), weights bf16 [out, in],
// biases / LayerNorm parameters / embedding tables f32.
// Pairs of a cross-encoder (sc_encoder_set_pair_head / sc_encoder_score_pairs) run the packed forward with a segment id per row and
// take each pair's [CLS] row instead of a mean; the head on those rows is encoder_pairs.hip's.
// Rerankers of the other two families (sc_encoder_set_score_head / sc_encoder_score_seqs) run the packed forward as it is and pool the row
// their head reads -- [CLS] or masked mean of final_norm (arch 1), RMS_final of the last token (arch 2), never L2-normalised
// (PackedLayout::head_pool); the heads on those rows are encoder_heads.hip's.
// Late-interaction models (sc_encoder_set_token_head / sc_encoder_embed_tokens / sc_encoder_score_late) run the packed forward without any pooling:
// the token head projects every row that is asked for (PackedLayout::tok_dst) and MaxSim scores pairs over those vectors (encoder_tokens.hip).
// Pre-norm models (cfg.arch 1, ModernBERT): forward_prenorm_locked -- h += Attn(LN(h)), h += MLP(LN(h)) on a raw residual stream, local
// (sliding-window) attention in the layers with l % global_every != 0 (encoder_window.hip), a rotary table per kind of layer, final_norm.
// Causal decoders (cfg.arch 2, the Qwen2 family): forward_causal_locked -- the same raw residual stream with RMSNorm, grouped-query causal
// attention (encoder_causal.hip), SwiGLU, no embedding norm; pooled from RMS_final(h): the last real token's row, or the masked mean.
// The single-kernel harnesses (sc_diag_*) are in sc_encoder_diag.cpp, the device entry points in encoder_ops.h.
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "encoder_ops.h"
#include "maxsim_rule.h"
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

struct sc_encoder {
    sc_runtime* rt = nullptr;
    sc_encoder_cfg cfg{};
    char* params = nullptr;  // one device allocation holding every parameter
    float *wemb = nullptr, *pemb = nullptr, *temb = nullptr, *embg = nullptr, *embb = nullptr;
    float* slopes = nullptr;  // ALiBi head slopes (device) or NULL
    float *rope_cos = nullptr, *rope_sin = nullptr;  // rotary positions: [max_pos][32] f32 each (device) or NULL; arch 2 at head_dim 128: [max_pos][64]
    float *rope_cos_l = nullptr, *rope_sin_l = nullptr;  // arch 1: the table of the local layers (base rope_theta_local); the one above is the global layers'
    float *fing = nullptr, *finb = nullptr;              // arch 1: final_norm gamma / beta
    std::vector<LayerW> layers;
    // workspace for `ws_tokens` (multiple of 256) tokens
    int64_t ws_tokens = 0;
    char* ws = nullptr;
    void *x = nullptr, *x1 = nullptr, *y = nullptr, *qkv = nullptr, *ctx = nullptr, *hm = nullptr, *hg = nullptr;
    int32_t* ids = nullptr;
    int32_t* lens = nullptr;
    // packed batches: padded ids | positions | starts | lens | attention items (PlanOffsets), one upload per call.  Part of every
    // workspace, rectangle callers' too: 8 bytes per token row + 24 per sequence next to the 17-29 KiB a row's activations take
    char* plan = nullptr;
    float* pooled = nullptr;
    int64_t ws_batch = 0;
    float *stat_a = nullptr, *stat_b = nullptr;  // [slots][ws_tokens][2] partial row sums of the two pre-LayerNorm tensors (folded pipeline)
    float *fin_a = nullptr, *fin_b = nullptr;    // [ws_tokens][2] their finalised (mu, rs)
    bool foldable = false;                       // shapes allow the folded pipeline (256-tile GEMMs, K % 256 == 0)
    int path = 0;                                // sc_encoder_set_path: 0 auto, 1 batch pipeline always, 2 small-batch pipeline always
    int pooling = 0;                             // sc_encoder_set_pooling: 0 masked mean, 1 the [CLS] row, 2 the last real token's row (arch 2)
    void* splitk = nullptr;  // f32 partial products of the split-K GEMMs (batches of <= 1024 tokens), allocated on first use
    static constexpr size_t SPLITK_BYTES = 64u << 20;
    // pinned host staging for the asynchronous embed -> index path: ids | lens | rows of one batch per slot
    struct PinSlot {
        char* host = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    } pin[2];
    int pin_next = 0;
    // the pair head of a cross-encoder (sc_encoder_set_pair_head): one device allocation Wp [H,H] | bp [H] | Wc [labels,H] | bc [labels],
    // all f32; head_wp NULL = no pooler, head_wc NULL = no head installed
    char* head = nullptr;
    float *head_wp = nullptr, *head_bp = nullptr, *head_wc = nullptr, *head_bc = nullptr;
    int head_labels = 0;
    float* logits = nullptr;  // [ws_batch][2] (workspace)
    // the score head of an arch 1 / arch 2 reranker (sc_encoder_set_score_head), a slot of its own next to the pair head's: one device allocation
    // dense_w [H,H] | dense_b [H] | norm_g [H] | norm_b [H] | cls_w [labels,H] | cls_b [labels], all f32, an absent array NULL; sh_wc NULL = none
    char* shead = nullptr;
    float *sh_wd = nullptr, *sh_bd = nullptr, *sh_g = nullptr, *sh_b = nullptr, *sh_wc = nullptr, *sh_bc = nullptr;
    int sh_kind = 0, sh_pooling = 0, sh_labels = 0;
    float sh_eps = 0.f;
    // the token head of a late-interaction model (sc_encoder_set_token_head), a third slot: the projection [W, H] as bf16; NULL = none
    void* thead = nullptr;
    int th_w = 0;
    // token vectors of sc_encoder_embed_tokens / sc_encoder_score_late: the queries' (0) and the documents' (1) [rows][W] f32, and the
    // pair call's offsets | keep flags | pair list | scores; each grows on demand and is kept
    struct Grown {
        char* p = nullptr;
        size_t cap = 0;
    } tok[2], late_aux;
    std::mutex mu;
};

// ---- packed variable-length batches (sc_encoder_embed_packed*): sequence i owns the token rows [starts[i], starts[i] + ceil32(len_i)),
// one sequence after another; the GEMMs run on the total rounded up to 256 rows.
static int64_t ceil32(int64_t v) { return (v + 31) & ~(int64_t)31; }
// Where the sequences of a packed batch lie, for the four position-aware steps of the forward (device pointers into e->plan).
// The forward takes it as a parameter: NULL = a [B, S] rectangle.
struct PackedLayout {
    const int32_t *pos, *starts, *items;
    int nitems[3];
    int rows;  // token rows in use = the sum of ceil32(len_i); rows .. M are the tail
    // pairs of a cross-encoder (sc_encoder_score_pairs): the segment id of every row.  Such a batch is embedded with its types, the
    // lens the forward gets are ones (pooling then returns the [CLS] row; attention reads the real lengths from its items) and
    // the output is never L2-normalised.  NULL: texts to embed.
    const int32_t* types = nullptr;
    // sequences of sc_encoder_score_seqs: the pooling of the installed score head (0 mean, 1 first row, 2 last token) instead of the encoder's
    // mode, and no L2 normalisation.  -1: texts to embed.
    int head_pool = -1;
    // token calls (sc_encoder_embed_tokens, sc_encoder_score_late): the compact output row of every packed row, -1 for a row that is not
    // asked for.  Nothing is pooled and the last layer is never pruned: the token head runs on the rows after the model's last norm and writes
    // tok_out [.., W] f32 (device); the forward's out_dev is not written.  NULL: one row per text.
    const int32_t* tok_dst = nullptr;
    float* tok_out = nullptr;
};
// The plan of one packed call, laid out alike in pinned host staging and in e->plan (M token rows, B sequences): monotone in both, so
// a call's plan fits the buffer of any larger workspace
// (pairs: the segment id of every row and a length of one per pair come behind the rest, so that a plan without them lies as before).
struct PlanOffsets {
    size_t ids, pos, starts, lens, items, types = 0, ones = 0, dst = 0, total;
    PlanOffsets(size_t M, size_t B, bool pairs = false, bool tokens = false) {
        size_t u = 0;
        auto take = [&](size_t bytes) { const size_t at = u; u += sc_align256(bytes); return at; };
        ids = take(M * 4);
        pos = take(M * 4);
        starts = take(B * 4);
        lens = take(B * 4);
        items = take((size_t)sc_packed_items_cap((int64_t)M, (int64_t)B) * 16);
        if (pairs) {
            types = take(M * 4);
            ones = take(B * 4);
        }
        if (tokens) dst = take(M * 4);  // (never together with pairs, and no larger than what pairs add: the workspace's plan holds either)
        total = u;
    }
};
void sc_packed_items(const int32_t* starts, const int32_t* lens, int64_t B, int32_t* items, int nitems[3]) {
    int32_t* w = items;
    for (int cls = 0; cls < 3; ++cls) {
        const int32_t* w0 = w;
        for (int64_t i = 0; i < B; ++i) {
            if (sc_packed_attention_class(lens[i]) != cls) continue;
            const int nqb = (int)(ceil32(lens[i]) / 32);
            for (int qb = 0; qb < (cls == 0 ? nqb : 1); qb += 8, w += 4) { w[0] = starts[i]; w[1] = lens[i]; w[2] = qb; w[3] = 0; }
        }
        nitems[cls] = (int)((w - w0) / 4);
    }
}

// Lays the buffers of one device allocation out, each 256-byte aligned.  The layout code runs twice: over an arena without a base
// it only measures (every buffer comes back NULL, `used` is the size to allocate), over the allocation it hands out the pointers.
struct Arena {
    char* base = nullptr;
    size_t used = 0;
    void* take(size_t bytes) { const size_t o = used; used += sc_align256(bytes); return base ? base + o : nullptr; }
    float* f32(size_t n) { return (float*)take(n * 4); }
    void* bf16(size_t n) { return take(n * 2); }
};

// ffn_type 1 (GEGLU) and 2 (SwiGLU): W1 holds gate and up rows, an element-wise kernel sits between the two FFN GEMMs
static bool ffn_gated(const sc_encoder_cfg& c) { return c.ffn_type == 1 || c.ffn_type == 2; }
// arch 2: heads of 64, or of 128 when cfg.head_dim says so; K and V have kv_heads of them (0 = heads), Q has heads of them -- the attention
// width AW, which need not be hidden at 128.  Every other model projects Q, K and V to hidden columns
static int head_width(const sc_encoder_cfg& c) { return c.arch == 2 && c.head_dim == 128 ? 128 : 64; }
static int64_t kv_width(const sc_encoder_cfg& c) { return c.arch == 2 ? (int64_t)(c.kv_heads > 0 ? c.kv_heads : c.heads) * head_width(c) : (int64_t)c.hidden; }
static int64_t attn_width(const sc_encoder_cfg& c) { return c.arch == 2 ? (int64_t)c.heads * head_width(c) : (int64_t)c.hidden; }
static void launch_gate(const sc_encoder_cfg& c, const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    if (c.ffn_type == 2) sc_launch_swiglu(h, tokens, F, out, s);
    else sc_launch_geglu(h, tokens, F, out, s);
}
// batch pipeline of rotary models ("rope_fused" of sc_diag_set_option): -1 = default, 0 = rope_qk_kernel after the QKV GEMM,
// 1 = rotation in that GEMM's epilogue (EPI_LNA_BIAS_ROPE)
// Default: fused -- 14.9k against 14.5k chunks/s at 256 x 256 tokens, 12 layers (+2.7 %, run-to-run spread 0.25 %: profiles/nomic_bench.log).
static int g_rope_fused = -1;
static const int ROPE_FUSED_DEFAULT = 1;
void sc_encoder_set_rope_fused(int v) { g_rope_fused = v < 0 ? -1 : (v ? 1 : 0); }
// [CLS] pooling: the last layer on the [CLS] rows only ("cls_prune" of sc_diag_set_option): -1 = default, 0 = the full last layer, 1 = pruned
static int g_cls_prune = -1;
static const int CLS_PRUNE_DEFAULT = 1;
void sc_encoder_set_cls_prune(int v) { g_cls_prune = v < 0 ? -1 : (v ? 1 : 0); }
static bool cls_prune_enabled() { return (g_cls_prune < 0 ? CLS_PRUNE_DEFAULT : g_cls_prune) != 0; }
// SC_FFN_BLOCKED=0: row-major FFN hidden activations (same-box A/B against the 64-column blocks)
static bool ffn_blocked_enabled() { static const bool on = sc_env_flag("SC_FFN_BLOCKED", true); return on; }

// number of f32 values in the weight blob, in blob order (see include/semcode_hip.h)
static int64_t blob_floats(const sc_encoder_cfg& c) {
    const int64_t H = c.hidden, F = c.ffn, F1 = ffn_gated(c) ? 2 * F : F;
    const int64_t KV = kv_width(c), AW = attn_width(c);
    int64_t n = (int64_t)c.vocab * H + (c.pos_type != 0 ? 0 : (int64_t)c.max_pos * H) + (c.arch != 0 ? 0 : (int64_t)c.type_vocab * H) + (c.arch == 2 ? 0 : 2 * H);
    n += (int64_t)c.layers * ((AW * H + AW) + (H * AW + H) + 2 * (KV * H + KV) + 2 * H + (F1 * H + F1) + (H * F + H) + 2 * H);
    if (c.arch == 2 && c.qk_norm) n += (int64_t)c.layers * 2 * head_width(c);  // q_norm, k_norm gammas behind each layer's ln2_beta
    if (c.arch != 0) n += 2 * H;  // final_norm
    return n;
}
// arch 1: layer l attends globally iff l % global_every == 0 (global_every 0 counts as 1: every layer global)
static bool layer_is_local(const sc_encoder_cfg& c, int l) { return c.arch == 1 && c.global_every > 1 && (l % c.global_every) != 0; }

extern "C" sc_status sc_encoder_blob_bytes(const sc_encoder_cfg* cfg, int64_t* out) {
    if (!cfg || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_blob_bytes: NULL argument");
    *out = blob_floats(*cfg) * 4;
    return SC_OK;
}

static sc_status check_cfg(const sc_encoder_cfg& c) {
    if (c.vocab < 1 || c.hidden < 1 || c.layers < 1 || c.heads < 1 || c.ffn < 1 || c.max_pos < 1 || c.type_vocab < 1)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: non-positive model dimension");
    const bool wide = c.arch == 2 && c.head_dim == 128;  // heads of 128 are stated, never derived: hidden need not be heads * 128
    if (!wide && c.hidden != c.heads * 64 && c.hidden != c.heads * 32)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head dimension must be 64 or 32 (hidden=%d heads=%d)", c.hidden, c.heads);
    if (c.hidden % 128 || c.ffn % 128 || c.hidden > 2048)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: hidden (<=2048) and ffn must be multiples of 128 (got %d, %d)", c.hidden, c.ffn);
    if (!(c.ln_eps > 0.f)) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: ln_eps must be > 0");
    if (c.pos_type < 0 || c.pos_type > 2 || c.ffn_type < 0 || c.ffn_type > 2) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: unknown pos_type / ffn_type");
    if (c.hidden == c.heads * 32 && c.pos_type != 0)  // the rotary kernels pair columns (j, j + 32) of a 64-wide head; no 32-wide ALiBi kernel
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head dimension 32 runs with learned positions only (pos_type 0), not pos_type %d (%s)", c.pos_type,
                       c.pos_type == 1 ? "ALiBi" : "rotary");
    if (c.pos_type == 2 && !(c.rope_theta >= 0.f)) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: rope_theta must be >= 0 (0 = 10000)");
    if (c.arch < 0 || c.arch > 2)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: unknown arch %d (0 = post-LN BERT family, 1 = pre-LN ModernBERT, 2 = causal Qwen2 decoder)", c.arch);
    if (c.arch != 2 && c.kv_heads != 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: kv_heads %d needs arch 2 (grouped-query attention exists in the causal pipeline only)", c.kv_heads);
    if (c.arch != 2 && c.head_dim != 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim %d needs arch 2 (a stated head dimension exists in the causal pipeline only; 0 elsewhere)", c.head_dim);
    if (c.arch != 2 && c.qk_norm != 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: qk_norm %d needs arch 2 (the per-head RMSNorm of Q and K exists in the causal pipeline only)", c.qk_norm);
    if (c.arch == 2) {
        // the causal pipeline: heads of 64 (rope_qk_kernel, attention_causal_kernel) or, stated, of 128 (qknorm_rope_kernel, attention_causal_kernel<2, ..>); SwiGLU
        if (c.head_dim != 0 && c.head_dim != 64 && c.head_dim != 128)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim must be 0 (hidden / heads, which must be 64), 64 or 128 on arch 2, got %d", c.head_dim);
        if (c.qk_norm != 0 && c.qk_norm != 1) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: qk_norm must be 0 or 1, got %d", c.qk_norm);
        if (wide && c.heads * 128 > 2048)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim 128 needs heads * 128 <= 2048 (the attention width), got heads %d", c.heads);
        if (!wide && c.hidden != c.heads * 64)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 2 needs head dimension 64 (hidden=%d heads=%d)", c.hidden, c.heads);
        if (c.pos_type != 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 2 runs with rotary positions only (pos_type 2), not pos_type %d", c.pos_type);
        if (c.ffn_type != 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 2 runs with the SwiGLU feed-forward only (ffn_type 2), not ffn_type %d", c.ffn_type);
        if (c.kv_heads < 0 || c.kv_heads > c.heads || (c.kv_heads > 0 && c.heads % c.kv_heads != 0))
            return sc_fail(SC_ERR_INVALID, "sc_encoder_create: kv_heads must divide heads (1 <= kv_heads <= heads, 0 = heads), got kv_heads %d with heads %d", c.kv_heads,
                           c.heads);
        if (c.local_window != 0 || c.global_every > 1)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window %d / global_every %d need arch 1 (arch 2 attends causally in every layer)", c.local_window,
                           c.global_every);
        return SC_OK;
    }
    if (c.arch == 0) {
        if (c.local_window != 0 || c.global_every > 1)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window %d / global_every %d need arch 1 (local attention exists in the pre-LN pipeline only)",
                           c.local_window, c.global_every);
        return SC_OK;
    }
    // the pre-LN pipeline: rotate-half rotation and the windowed kernel are written for 64-wide heads, its gate is GEGLU
    if (c.hidden != c.heads * 64)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 1 needs head dimension 64 (hidden=%d heads=%d)", c.hidden, c.heads);
    if (c.pos_type != 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 1 runs with rotary positions only (pos_type 2), not pos_type %d", c.pos_type);
    if (c.ffn_type != 1) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 1 runs with the GEGLU feed-forward only (ffn_type 1), not ffn_type %d", c.ffn_type);
    if (c.global_every < 1) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: global_every must be >= 1 with arch 1 (1 = every layer global), got %d", c.global_every);
    if (!sc_attention_window_supported(c.local_window))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window must be even and within 2 .. 128, got %d", c.local_window);
    if (!(c.rope_theta_local >= 0.f)) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: rope_theta_local must be >= 0 (0 = 10000)");
    return SC_OK;
}

std::vector<float> sc_rope_table(int64_t positions, float theta_arg, int head_dim) {
    const double theta = theta_arg > 0.f ? (double)theta_arg : 10000.0;
    const int half = head_dim / 2;
    const size_t n = (size_t)positions * half;
    std::vector<float> tab(2 * n);
    for (int i = 0; i < half; ++i) {
        const double f = std::pow(theta, -2.0 * i / (double)head_dim);
        for (int64_t p = 0; p < positions; ++p) {
            tab[(size_t)p * half + i] = (float)std::cos((double)p * f);
            tab[n + (size_t)p * half + i] = (float)std::sin((double)p * f);
        }
    }
    return tab;
}

// ALiBi head slopes (Press et al.; the non-power-of-two rule of the jina-bert implementation)
static std::vector<float> alibi_slopes(int heads) {
    std::vector<float> sl;
    auto pow2_slopes = [&](int n, int take, int stride) {
        const double start = std::pow(2.0, -std::pow(2.0, -(std::log2((double)n) - 3.0)));
        double v = start;
        for (int i = 0, got = 0; i < n && got < take; ++i, v *= start)
            if (i % stride == 0) { sl.push_back((float)v); ++got; }
    };
    int p2 = 1;
    while (p2 * 2 <= heads) p2 *= 2;
    pow2_slopes(p2, p2, 1);
    if (p2 < heads) pow2_slopes(2 * p2, heads - p2, 2);
    return sl;
}

// the parameter arena: f32 tables + per-layer {bf16 matrices, f32 vectors}; e->layers is sized, e->foldable set
static void layout_params(sc_encoder* e, Arena& a) {
    const sc_encoder_cfg& c = e->cfg;
    const size_t H = c.hidden, F = c.ffn, F1 = ffn_gated(c) ? 2 * F : F, rope_n = (size_t)c.max_pos * (head_width(c) / 2), AW = (size_t)attn_width(c),
                 QN = AW + 2 * (size_t)kv_width(c);
    e->wemb = a.f32((size_t)c.vocab * H);
    e->pemb = c.pos_type == 0 ? a.f32((size_t)c.max_pos * H) : nullptr;
    e->slopes = c.pos_type == 1 ? a.f32((size_t)c.heads) : nullptr;
    e->rope_cos = c.pos_type == 2 ? a.f32(2 * rope_n) : nullptr;  // sc_rope_table: cos, then sin
    e->rope_sin = e->rope_cos ? e->rope_cos + rope_n : nullptr;
    e->rope_cos_l = c.arch == 1 ? a.f32(2 * rope_n) : nullptr;
    e->rope_sin_l = e->rope_cos_l ? e->rope_cos_l + rope_n : nullptr;
    e->temb = a.f32(c.arch != 0 ? H : (size_t)c.type_vocab * H);  // arch 1, 2 have no type table: one row of zeros for the embedding kernels
    e->fing = c.arch != 0 ? a.f32(H) : nullptr;
    e->finb = c.arch != 0 ? a.f32(H) : nullptr;
    e->embg = a.f32(H);
    e->embb = a.f32(H);
    for (LayerW& w : e->layers) {
        w.wqkv = a.bf16(QN * H);    w.bqkv = a.f32(QN);
        w.wo = a.bf16(H * AW);      w.bo = a.f32(H);
        w.qng = c.arch == 2 && c.qk_norm ? a.f32((size_t)head_width(c)) : nullptr;
        w.kng = c.arch == 2 && c.qk_norm ? a.f32((size_t)head_width(c)) : nullptr;  // (by the configuration: a measuring arena hands out NULL)
        w.ln1g = a.f32(H);          w.ln1b = a.f32(H);
        w.w1 = a.bf16(F1 * H);      w.b1 = a.f32(F1);
        w.w2 = a.bf16(H * F);       w.b2 = a.f32(H);
        w.ln2g = a.f32(H);          w.ln2b = a.f32(H);
        if (!e->foldable) continue;
        w.wqkv_f = a.bf16(3 * H * H); w.c1q = a.f32(3 * H); w.c2q = a.f32(3 * H);
        w.w1_f = a.bf16(F1 * H);      w.c1f = a.f32(F1);    w.c2f = a.f32(F1);
        w.bb_o = a.f32(H);            w.bb_2 = a.f32(H);
    }
}

extern "C" sc_status sc_encoder_create(sc_runtime* rt, const sc_encoder_cfg* cfg, const void* weights_blob, size_t nbytes, sc_encoder** out) {
    if (!rt || !cfg || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: NULL argument");
    *out = nullptr;
    sc_status st = check_cfg(*cfg);
    if (st) return st;
    const int64_t nfl = blob_floats(*cfg);
    if (weights_blob && (int64_t)nbytes != nfl * 4)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: weight blob is %zu bytes, config needs %lld", nbytes, (long long)(nfl * 4));
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_encoder* e = new (std::nothrow) sc_encoder();
    if (!e) return sc_fail(SC_ERR_NOMEM, "out of host memory");
    e->rt = rt;
    sc_runtime_retain(rt);
    e->cfg = *cfg;
    if (e->cfg.arch == 2 && e->cfg.kv_heads == 0) e->cfg.kv_heads = e->cfg.heads;  // (sc_encoder_info reports the count in use)
    if (e->cfg.arch == 2) e->cfg.head_dim = head_width(*cfg);                       // (... and the head dimension in use: 64 or 128)
    const int64_t H = cfg->hidden, F = cfg->ffn, L = cfg->layers, F1 = ffn_gated(*cfg) ? 2 * F : F, KV = kv_width(*cfg), AW = attn_width(*cfg), HD = head_width(*cfg);

    // staging copy of the f32 blob on device (freed after conversion)
    float* blob = nullptr;
    hipError_t he = hipMalloc((void**)&blob, (size_t)nfl * 4);
    if (he != hipSuccess) {
        delete e;
        sc_runtime_release(rt);
        return sc_fail(SC_ERR_NOMEM, "hipMalloc weight staging (%lld B) failed: %s", (long long)nfl * 4, hipGetErrorString(he));
    }
    auto fail = [&](sc_status code) {
        hipFree(blob);
        hipFree(e->params);
        delete e;
        sc_runtime_release(rt);
        return code;
    };
    // the LayerNorm-folded batch pipeline needs every GEMM on the 256 x 256 tile and the statistics in whole 256-column slots
    // (arch 1: the LayerNorm-folded pipeline has no pre-norm form yet)
    e->foldable = cfg->arch == 0 && (H % 256) == 0 && (F % 256) == 0 && (F1 % 256) == 0 && ((3 * H) % 256) == 0;
    e->layers.resize(L);
    Arena arena;
    layout_params(e, arena);  // measure
    he = hipMalloc((void**)&e->params, arena.used);
    if (he != hipSuccess) return fail(sc_fail(SC_ERR_NOMEM, "hipMalloc parameters (%zu B) failed: %s", arena.used, hipGetErrorString(he)));
    arena = Arena{e->params};
    layout_params(e, arena);  // place

    if (weights_blob) {
        he = hipMemcpyAsync(blob, weights_blob, (size_t)nfl * 4, hipMemcpyHostToDevice, s);
        if (he != hipSuccess) return fail(sc_fail(SC_ERR_HIP, "weight upload failed: %s", hipGetErrorString(he)));
    } else {
        // synthetic weights: every tensor ~ 0.02 * N(0,1) over the blob index, then LayerNorm gamma = 1,
        // beta = 0 and biases = 0 are overwritten below (same rule in oracle/bert_oracle.py synth_weights)
        sc_launch_synth_scaled(blob, nfl, cfg->synth_seed, 0.02f, 0.0f, s);
    }
    // walk the blob in its documented order
    int64_t off = 0;
    auto take = [&](int64_t n) { float* p = blob + off; off += n; return p; };
    enum { COPY, ONES, ZEROS };  // what a synthetic model holds instead of the blob's values
    auto put_f32 = [&](float* d, const float* src, int64_t n, int synth) {
        if (!weights_blob && synth == ONES) sc_launch_synth_scaled(d, n, 0, 0.0f, 1.0f, s);
        else if (!weights_blob && synth == ZEROS) hipMemsetAsync(d, 0, (size_t)n * 4, s);
        else hipMemcpyAsync(d, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
    };
    auto put_bf16 = [&](void* d, const float* src, int64_t n) { sc_launch_f32_to_bf16(src, d, n, s); };
    auto put_host = [&](float* d, const std::vector<float>& v) {
        hipMemcpyAsync(d, v.data(), v.size() * 4, hipMemcpyHostToDevice, s);
        hipStreamSynchronize(s);  // v goes out of scope
    };
    put_f32(e->wemb, take((int64_t)cfg->vocab * H), (int64_t)cfg->vocab * H, COPY);
    if (e->pemb) put_f32(e->pemb, take((int64_t)cfg->max_pos * H), (int64_t)cfg->max_pos * H, COPY);
    if (e->slopes) put_host(e->slopes, alibi_slopes(cfg->heads));
    if (e->rope_cos) put_host(e->rope_cos, sc_rope_table(cfg->max_pos, cfg->rope_theta, (int)HD));
    if (e->rope_cos_l) put_host(e->rope_cos_l, sc_rope_table(cfg->max_pos, cfg->rope_theta_local));
    if (cfg->arch != 0) hipMemsetAsync(e->temb, 0, (size_t)H * 4, s);
    else put_f32(e->temb, take((int64_t)cfg->type_vocab * H), (int64_t)cfg->type_vocab * H, COPY);
    if (cfg->arch != 2) {  // arch 2 has no embedding norm
        put_f32(e->embg, take(H), H, ONES);
        put_f32(e->embb, take(H), H, ZEROS);
    }
    for (int64_t l = 0; l < L; ++l) {
        LayerW& w = e->layers[l];
        // blob order: Wq bq Wk bk Wv bv Wo bo ln1g ln1b W1 b1 W2 b2 ln2g ln2b ; device: Wqkv = [Wq; Wk; Wv] (Wk, Wv: KV rows each)
        const float* wqkv_f32[3];
        for (int p = 0; p < 3; ++p) {
            const int64_t rows = p == 0 ? AW : KV, row0 = p == 0 ? 0 : AW + (p - 1) * KV;
            wqkv_f32[p] = take(rows * H);
            put_bf16((char*)w.wqkv + (size_t)row0 * H * 2, wqkv_f32[p], rows * H);
            put_f32(w.bqkv + row0, take(rows), rows, ZEROS);
        }
        put_bf16(w.wo, take(H * AW), H * AW);
        put_f32(w.bo, take(H), H, ZEROS);
        put_f32(w.ln1g, take(H), H, ONES);
        put_f32(w.ln1b, take(H), H, ZEROS);
        const float* w1_f32 = take(F1 * H);
        put_bf16(w.w1, w1_f32, F1 * H);
        put_f32(w.b1, take(F1), F1, ZEROS);
        put_bf16(w.w2, take(H * F), H * F);
        put_f32(w.b2, take(H), H, ZEROS);
        put_f32(w.ln2g, take(H), H, ONES);
        put_f32(w.ln2b, take(H), H, ZEROS);
        if (w.qng) {
            put_f32(w.qng, take(HD), HD, ONES);
            put_f32(w.kng, take(HD), HD, ONES);
        }
        if (e->foldable) {
            // the LayerNorm in front of this layer: the embeddings' for layer 0, else the previous layer's second one
            const float* gp = l == 0 ? e->embg : e->layers[l - 1].ln2g;
            const float* bp = l == 0 ? e->embb : e->layers[l - 1].ln2b;
            w.g_prev = gp;
            for (int p = 0; p < 3; ++p)  // Wq, Wk, Wv are separate tensors of the blob
                sc_launch_fold_ln_weights(wqkv_f32[p], gp, bp, w.bqkv + p * H, (int)H, (int)H, (char*)w.wqkv_f + (size_t)p * H * H * 2, w.c1q + p * H, w.c2q + p * H, s);
            sc_launch_fold_ln_weights(w1_f32, w.ln1g, w.ln1b, w.b1, (int)F1, (int)H, w.w1_f, w.c1f, w.c2f, s);
            sc_launch_add_vectors(w.bo, bp, w.bb_o, (int)H, s);
            sc_launch_add_vectors(w.b2, w.ln1b, w.bb_2, (int)H, s);
        }
    }
    if (e->fing) {
        put_f32(e->fing, take(H), H, ONES);
        put_f32(e->finb, take(H), H, ZEROS);
    }
    he = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) return fail(sc_fail(SC_ERR_HIP, "encoder parameter setup failed: %s", hipGetErrorString(he)));
    hipFree(blob);
    *out = e;
    return SC_OK;
}

extern "C" sc_status sc_encoder_destroy(sc_encoder* e) {
    if (!e) return SC_OK;
    hipSetDevice(e->rt->device);
    hipStreamSynchronize(e->rt->stream);
    hipFree(e->params);
    hipFree(e->ws);
    hipFree(e->splitk);
    hipFree(e->head);
    hipFree(e->shead);
    hipFree(e->thead);
    hipFree(e->tok[0].p);
    hipFree(e->tok[1].p);
    hipFree(e->late_aux.p);
    for (auto& slot : e->pin) {
        if (slot.host) hipHostFree(slot.host);
        if (slot.done) hipEventDestroy(slot.done);
    }
    sc_runtime* rt = e->rt;
    delete e;
    sc_runtime_release(rt);
    return SC_OK;
}

// the workspace for `tokens` token rows and `nb` chunks
static void layout_ws(sc_encoder* e, Arena& a, size_t tokens, size_t nb) {
    const size_t H = e->cfg.hidden, F = e->cfg.ffn, F1 = ffn_gated(e->cfg) ? 2 * F : F, slots = H / 256;
    const size_t AW = (size_t)attn_width(e->cfg), QN = AW + 2 * (size_t)kv_width(e->cfg);  // arch 2 at head dimension 128: AW may exceed H, QN 3 H
    e->x = a.bf16(tokens * H);
    e->x1 = a.bf16(tokens * H);
    e->y = a.bf16(tokens * H);
    e->qkv = a.bf16(tokens * (QN > 3 * H ? QN : 3 * H));
    e->ctx = a.bf16(tokens * (AW > H ? AW : H));
    e->hm = a.bf16(tokens * F1);
    e->hg = ffn_gated(e->cfg) ? a.bf16(tokens * F) : nullptr;
    e->ids = (int32_t*)a.take(tokens * 4);
    e->lens = (int32_t*)a.take(nb * 4);
    e->plan = (char*)a.take(PlanOffsets(tokens, nb, true).total);
    e->pooled = a.f32(nb * H);
    e->logits = a.f32(nb * 2);
    e->stat_a = e->foldable ? a.f32(slots * tokens * 2) : nullptr;
    e->stat_b = e->foldable ? a.f32(slots * tokens * 2) : nullptr;
    e->fin_a = e->foldable ? a.f32(tokens * 2) : nullptr;
    e->fin_b = e->foldable ? a.f32(tokens * 2) : nullptr;
}

// ... for `rows` token rows (a rectangle's B * S, a packed batch's row count) of B sequences
static sc_status ensure_ws(sc_encoder* e, int64_t rows, int64_t B) {
    const int64_t tokens = (rows + 255) / 256 * 256;  // GEMM tiles are 256 rows
    if (tokens <= e->ws_tokens && B <= e->ws_batch) return SC_OK;
    SC_HIP(hipStreamSynchronize(e->rt->stream));
    hipFree(e->ws);
    e->ws = nullptr;
    e->ws_tokens = 0;
    e->ws_batch = 0;
    Arena arena;
    layout_ws(e, arena, (size_t)tokens, (size_t)B);  // measure (no buffer is left pointing into the freed workspace)
    hipError_t he = hipMalloc((void**)&e->ws, arena.used);
    if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc encoder workspace (%zu B) failed: %s", arena.used, hipGetErrorString(he));
    SC_HIP(hipMemsetAsync(e->ws, 0, arena.used, e->rt->stream));  // padded rows must hold finite values
    arena = Arena{e->ws};
    layout_ws(e, arena, (size_t)tokens, (size_t)B);  // place
    e->ws_tokens = tokens;
    e->ws_batch = B;
    return SC_OK;
}

// The steps both pipelines launch in a rectangle form and a packed form (pk != NULL).  Packed rotary models always rotate with the
// stand-alone kernel: the rotation fused into the QKV epilogue (EPI_LNA_BIAS_ROPE) takes its position from row & (S - 1).
// local: the table of an arch 1 model's local layers instead of the model's (global) one
static void launch_rope(sc_encoder* e, int M, int S, const PackedLayout* pk, hipStream_t s, bool local = false) {
    const float *cos_t = local ? e->rope_cos_l : e->rope_cos, *sin_t = local ? e->rope_sin_l : e->rope_sin;
    const int nblocks = e->cfg.arch == 2 ? e->cfg.heads + e->cfg.kv_heads : 2 * e->cfg.heads;  // the Q and K heads
    if (pk) sc_launch_rope_qk_packed(e->qkv, M, nblocks, pk->pos, e->cfg.max_pos, cos_t, sin_t, s);
    else sc_launch_rope_qk(e->qkv, M, nblocks, S, cos_t, sin_t, s);
}
static void launch_attention_window(sc_encoder* e, const int32_t* lens_dev, int B, int S, int M, const PackedLayout* pk, hipStream_t s) {
    if (pk) sc_launch_attention_window_packed(e->qkv, pk->items, pk->nitems, e->cfg.hidden, e->cfg.local_window, e->ctx, s, M);
    else sc_launch_attention_window(e->qkv, lens_dev, B, S, e->cfg.hidden, e->cfg.local_window, e->ctx, s, M);
}
static void launch_attention(sc_encoder* e, const int32_t* lens_dev, int B, int S, int M, const PackedLayout* pk, hipStream_t s) {
    const int hd = e->cfg.hidden / e->cfg.heads;  // 64, or 32: a pair of heads per 64-column block (Head32, attention_core.h)
    if (pk) sc_launch_attention_packed(e->qkv, pk->items, pk->nitems, e->cfg.hidden, e->slopes, e->ctx, s, M, hd);
    else sc_launch_attention(e->qkv, lens_dev, B, S, e->cfg.hidden, e->slopes, e->ctx, s, M, hd);
}
static void launch_attention_causal(sc_encoder* e, const int32_t* lens_dev, int B, int S, int M, const PackedLayout* pk, hipStream_t s) {
    const sc_encoder_cfg& c = e->cfg;
    if (pk) sc_launch_attention_causal_packed(e->qkv, pk->items, pk->nitems, c.heads, c.kv_heads, head_width(c), e->ctx, s, M);
    else sc_launch_attention_causal(e->qkv, lens_dev, B, S, c.heads, c.kv_heads, head_width(c), e->ctx, s, M);
}
// [CLS] pooling applies to texts only: the pairs of a cross-encoder take their [CLS] row whatever the mode (PackedLayout::types)
// (a token call pools nothing)
static bool token_call(const PackedLayout* pk) { return pk && pk->tok_dst; }
static bool cls_pooling(const sc_encoder* e, const PackedLayout* pk) { return e->pooling == 1 && !(pk && pk->types) && !token_call(pk); }
// the token head on the rows `x` after the model's last norm, in place of a pooling kernel
static sc_status launch_token_head(sc_encoder* e, const void* x, const PackedLayout* pk, hipStream_t s) {
    sc_launch_token_head(x, pk->rows, e->cfg.hidden, e->thead, e->th_w, pk->tok_dst, pk->tok_out, s);
    SC_HIP(hipGetLastError());
    return SC_OK;
}
// The last layer of a [CLS]-pooled forward from its QKV projection (e->qkv, rotated) on: attention of each text's first row, that row of the
// layer's input as the residual, then the rest of the layer on Mc = ceil256(B) compact rows with the small-batch pipeline's launches, and the
// last LayerNorm inside the pooling kernel.  e->x: the layer's input, normalised, or (res_g != NULL) raw with the LayerNorm (res_g, res_b) pending.
// Buffers: ctx, x1, y, hm, hg are free at this point; every one holds at least M >= Mc rows.
static sc_status cls_last_layer(sc_encoder* e, const LayerW& w, const int32_t* lens_dev, int B, int S, int M, const PackedLayout* pk, const float* res_g,
                                const float* res_b, float* out_dev) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const int H = c.hidden, F = c.ffn, Mc = (B + 255) / 256 * 256;
    const int32_t* starts = pk ? pk->starts : nullptr;
    void* sk = nullptr;
    if (Mc <= 1024 && e->path != 1) {
        if (!e->splitk) SC_HIP(hipMalloc(&e->splitk, sc_encoder::SPLITK_BYTES));
        sk = e->splitk;
    }
    const size_t skb = sk ? sc_encoder::SPLITK_BYTES : 0;
    sc_with_prof(rt, SC_PROF_ATTN, [&] { sc_launch_attention_cls(e->qkv, starts, lens_dev, B, S, M, H, H / c.heads, e->slopes, e->ctx, Mc, s); });
    sc_launch_cls_gather(e->x, starts, B, S, H, res_g, res_b, c.ln_eps, e->x1, Mc, s);
    sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->ctx, H, w.wo, H, w.bo, e->x1, H, e->y, H, Mc, H, H, s, sk, skb); });
    sc_launch_layernorm(e->y, Mc, H, w.ln1g, w.ln1b, c.ln_eps, e->x1, s);
    const void* ffn_in = e->hm;
    sc_with_prof(rt, SC_PROF_GEMM, [&] {
        if (ffn_gated(c)) sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, 2 * F, Mc, 2 * F, H, s, sk, skb);
        else sc_launch_gemm_bf16(EPI_BIAS_GELU, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, F, Mc, F, H, s, sk, skb);
    });
    if (ffn_gated(c)) {
        launch_gate(c, e->hm, Mc, F, e->hg, s);
        ffn_in = e->hg;
    }
    sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, ffn_in, F, w.w2, F, w.b2, e->x1, H, e->y, H, Mc, H, F, s, sk, skb); });
    sc_launch_cls_pool(e->y, nullptr, B, 1, H, w.ln2g, w.ln2b, c.ln_eps, c.normalize, out_dev, s);  // compact rows: text i's row is i
    SC_HIP(hipGetLastError());
    return SC_OK;
}
static void launch_mean_pool(sc_encoder* e, const void* x, const int32_t* lens_dev, int B, int S, const PackedLayout* pk, float* out_dev, hipStream_t s) {
    if (pk) sc_launch_mean_pool_packed(x, pk->starts, lens_dev, B, e->cfg.hidden, pk->types || pk->head_pool >= 0 ? 0 : e->cfg.normalize, out_dev, s);
    else sc_launch_mean_pool(x, lens_dev, B, S, e->cfg.hidden, e->cfg.normalize, out_dev, s);
}

// The batch pipeline with every LayerNorm folded into its neighbours (no layernorm_kernel launch, no LayerNorm round trip
// through HBM: 24 x 33 us and 24 x 200 MB per step at 256 x 256 tokens).  Activations between layers are the PRE-LayerNorm
// tensors (raw bf16 rows) together with their row statistics:
//   embed_raw                     -> x  (raw) + stat_b            x = word + position + type embeddings
//   per layer, LN_p = the LayerNorm that belongs in front of it (embeddings' / previous layer's second):
//     QKV   = LN_p(x) Wqkv^T + b   as  rs (x Wqkv'^T - mu c1) + c2            EPI_LNA_BIAS   (stat_b -> fin_b)
//     y     = ctx Wo^T + bo + LN_p(x)    residual normalised on the fly, row sums of y out   EPI_RESLN_STATS (fin_b -> stat_a)
//     hm    = gelu(LN_1(y) W1^T + b1)    folded the same way                                 EPI_LNA_GELU   (stat_a -> fin_a)
//     x     = hm W2^T + b2 + LN_1(y)                                                         EPI_RESLN_STATS (fin_a -> stat_b)
//   pooled = masked mean of LN_2(x) of the last layer, normalised on the fly (mean_pool_ln)
// Statistics are taken of the bf16-ROUNDED rows, i.e. of exactly what the consumer reads; all reductions run in a fixed order.
static sc_status forward_folded_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev,
                                       const PackedLayout* pk) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const int H = c.hidden, F = c.ffn;
    const int tokens = pk ? pk->rows : B * S;
    const int M = (tokens + 255) / 256 * 256;
    const int slots = H / 256;
    // statistics buffers are laid out for ws_tokens rows; this call uses the first M rows of every slot: slot stride must be M, so
    // they are addressed as [slots][M][2] inside the (larger or equal) allocation
    const bool gated = ffn_gated(c);
    const bool ffn_blocked = !gated && ffn_blocked_enabled();
    const bool rope = c.pos_type == 2, rope_fused = rope && !pk && (g_rope_fused < 0 ? ROPE_FUSED_DEFAULT : g_rope_fused) != 0;
    const bool cls = cls_pooling(e, pk), prune = cls && cls_prune_enabled();
    if (pk && pk->types)
        sc_launch_embed_raw_pairs(ids_dev, pk->pos, pk->types, tokens, M, H, c.vocab, c.max_pos, c.type_vocab, e->wemb, e->pemb, e->temb, e->x, e->stat_b, slots, s);
    else if (pk) sc_launch_embed_raw_packed(ids_dev, pk->pos, tokens, M, H, c.vocab, c.max_pos, e->wemb, e->pemb, e->temb, e->x, e->stat_b, slots, s);
    else sc_launch_embed_raw(ids_dev, tokens, M, S, H, c.vocab, c.max_pos, e->wemb, e->pemb, e->temb, e->x, e->stat_b, slots, s);
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& w = e->layers[l];
        sc_with_prof(rt, SC_PROF_GEMM, [&] {
            if (rope_fused)
                sc_launch_gemm_bf16_ln(EPI_LNA_BIAS_ROPE, e->x, H, w.wqkv_f, H, w.c2q, nullptr, 0, e->qkv, SC_LDC_BLOCKED64, M, 3 * H, H, s, w.c1q, e->stat_b, e->fin_b,
                                       nullptr, nullptr, c.ln_eps, e->rope_cos, e->rope_sin, S, 2 * H);
            else
                sc_launch_gemm_bf16_ln(EPI_LNA_BIAS, e->x, H, w.wqkv_f, H, w.c2q, nullptr, 0, e->qkv, SC_LDC_BLOCKED64, M, 3 * H, H, s, w.c1q, e->stat_b, e->fin_b, nullptr,
                                       nullptr, c.ln_eps);
        });
        if (rope && !rope_fused) launch_rope(e, M, S, pk, s);
        if (prune && l == c.layers - 1)  // the residual rows: LayerNorm of the raw rows by the LayerNorm in front of this layer
            return cls_last_layer(e, w, lens_dev, B, S, M, pk, w.g_prev, l == 0 ? e->embb : e->layers[l - 1].ln2b, out_dev);
        sc_with_prof(rt, SC_PROF_ATTN, [&] { launch_attention(e, lens_dev, B, S, M, pk, s); });
        sc_with_prof(rt, SC_PROF_GEMM, [&] {
            sc_launch_gemm_bf16_ln(EPI_RESLN_STATS, e->ctx, H, w.wo, H, w.bb_o, e->x, H, e->y, H, M, H, H, s, nullptr, nullptr, e->fin_b, w.g_prev, e->stat_a, c.ln_eps);
        });
        const void* ffn_in = e->hm;
        sc_with_prof(rt, SC_PROF_GEMM, [&] {
            if (gated)
                sc_launch_gemm_bf16_ln(EPI_LNA_BIAS, e->y, H, w.w1_f, H, w.c2f, nullptr, 0, e->hm, 2 * F, M, 2 * F, H, s, w.c1f, e->stat_a, e->fin_a, nullptr, nullptr, c.ln_eps);
            else
                sc_launch_gemm_bf16_ln(EPI_LNA_GELU, e->y, H, w.w1_f, H, w.c2f, nullptr, 0, e->hm, ffn_blocked ? SC_LDC_BLOCKED64 : F, M, F, H, s, w.c1f, e->stat_a,
                                       e->fin_a, nullptr, nullptr, c.ln_eps);
        });
        if (gated) {
            launch_gate(c, e->hm, M, F, e->hg, s);
            ffn_in = e->hg;
        }
        sc_with_prof(rt, SC_PROF_GEMM, [&] {
            sc_launch_gemm_bf16_ln(EPI_RESLN_STATS, ffn_in, ffn_blocked ? SC_LDC_BLOCKED64 : F, w.w2, F, w.bb_2, e->y, H, e->x, H, M, H, F, s, nullptr,
                                   nullptr, e->fin_a, w.ln1g, e->stat_b, c.ln_eps);
        });
    }
    const LayerW& last = e->layers[c.layers - 1];
    if (token_call(pk)) {  // the token head reads normalised rows, as the plain pooling kernel below
        sc_launch_layernorm(e->x, tokens, H, last.ln2g, last.ln2b, c.ln_eps, e->x1, s);
        return launch_token_head(e, e->x1, pk, s);
    }
    if (cls) {  // the last LayerNorm on B rows, inside the pooling kernel
        sc_launch_cls_pool(e->x, pk ? pk->starts : nullptr, B, S, H, last.ln2g, last.ln2b, c.ln_eps, c.normalize, out_dev, s);
    } else if (c.normalize && !(pk && pk->types)) {  // L2-normalised output: the plain pooling kernel does it; give it the normalised rows
        sc_launch_layernorm(e->x, tokens, H, last.ln2g, last.ln2b, c.ln_eps, e->x1, s);
        launch_mean_pool(e, e->x1, lens_dev, B, S, pk, out_dev, s);
    } else if (pk) {
        sc_launch_mean_pool_ln_packed(e->x, e->stat_b, slots, M, last.ln2g, last.ln2b, c.ln_eps, pk->starts, lens_dev, B, H, out_dev, s);
    } else {
        sc_launch_mean_pool_ln(e->x, e->stat_b, slots, M, last.ln2g, last.ln2b, c.ln_eps, lens_dev, B, S, H, out_dev, s);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// The pre-norm forward (cfg.arch 1, ModernBERT), on the stand-alone-LayerNorm launches for every batch size (split-K GEMMs up to 1 024
// rows, the 256-tile GEMMs beyond).  The residual stream h stays RAW between the sub-layers:
//   h = LN_emb(word embedding)                                            -> x
//   per layer:  a = l == 0 ? h : LN_attn(h)                               -> x1 (layer 0 reads x itself: its attn_norm is the identity)
//               QKV = a Wqkv^T + b (64-column blocks), rotated with the table of the layer's kind (global / local base)
//               ctx = attention, windowed in the local layers (encoder_window.hip), the model's global kernels otherwise
//               h = ctx Wo^T + bo + h                                     x -> y   (EPI_BIAS_RES, the raw stream as residual)
//               m = LN_mlp(h)                                             -> x1
//               h = (gelu(gate) * up)(m Wi^T + bi) Wo^T + bo + h          y -> x
//   pooled = masked mean of final_norm(h), or final_norm of the [CLS] row (in f32, inside the pooling kernel; never pruned: cls_last_layer
//   is the post-LN layer)
static sc_status forward_prenorm_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev,
                                        const PackedLayout* pk) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const int H = c.hidden, F = c.ffn;
    const int tokens = pk ? pk->rows : B * S;
    const int M = (tokens + 255) / 256 * 256;
    void* sk = nullptr;
    const bool scored = pk && pk->head_pool >= 0;  // the row a score head reads: its own pooling, never L2-normalised
    // A scored call (sc_encoder_score_seqs) never splits K: the split and its factor follow the call's row count, and a pair's logits must be
    // the same bits whichever batch-mates it has.  Every GEMM is then the 256-tile kernel, whose sums for a row do not depend on M.
    // (a token call neither: a text's vectors are the same bits whichever batch-mates it has)
    if (M <= 1024 && e->path != 1 && !scored && !token_call(pk)) {
        if (!e->splitk) SC_HIP(hipMalloc(&e->splitk, sc_encoder::SPLITK_BYTES));
        sk = e->splitk;
    }
    const size_t skb = sk ? sc_encoder::SPLITK_BYTES : 0;
    if (pk) sc_launch_embed_ln_packed(ids_dev, pk->pos, tokens, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    else sc_launch_embed_ln(ids_dev, tokens, S, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& w = e->layers[l];
        const bool local = layer_is_local(c, l);
        const void* a = e->x;
        if (l > 0) {
            sc_launch_layernorm(e->x, tokens, H, w.ln1g, w.ln1b, c.ln_eps, e->x1, s);
            a = e->x1;
        }
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, a, H, w.wqkv, H, w.bqkv, nullptr, 0, e->qkv, SC_LDC_BLOCKED64, M, 3 * H, H, s, sk, skb); });
        launch_rope(e, M, S, pk, s, local);
        sc_with_prof(rt, SC_PROF_ATTN, [&] {
            if (local) launch_attention_window(e, lens_dev, B, S, M, pk, s);
            else launch_attention(e, lens_dev, B, S, M, pk, s);
        });
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->ctx, H, w.wo, H, w.bo, e->x, H, e->y, H, M, H, H, s, sk, skb); });
        sc_launch_layernorm(e->y, tokens, H, w.ln2g, w.ln2b, c.ln_eps, e->x1, s);
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, 2 * F, M, 2 * F, H, s, sk, skb); });
        launch_gate(c, e->hm, M, F, e->hg, s);
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->hg, F, w.w2, F, w.b2, e->y, H, e->x, H, M, H, F, s, sk, skb); });
    }
    if (token_call(pk)) {
        sc_launch_layernorm(e->x, tokens, H, e->fing, e->finb, c.ln_eps, e->x1, s);
        return launch_token_head(e, e->x1, pk, s);
    }
    if (scored ? pk->head_pool == 1 : cls_pooling(e, pk)) {
        sc_launch_cls_pool(e->x, pk ? pk->starts : nullptr, B, S, H, e->fing, e->finb, c.ln_eps, scored ? 0 : c.normalize, out_dev, s);
    } else {
        sc_launch_layernorm(e->x, tokens, H, e->fing, e->finb, c.ln_eps, e->x1, s);
        launch_mean_pool(e, e->x1, lens_dev, B, S, pk, out_dev, s);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// The causal decoder forward (cfg.arch 2, the Qwen2 family), on the stand-alone-norm launches for every batch size as the pre-norm forward:
//   h = bf16(tok_emb[id])                                                 -> x   (the raw embedding kernels, no position table, zero type row)
//   per layer:  a = RMS_in(h)                                             -> x1
//               QKV = a [Wq; Wk; Wv]^T + b, N = AW + 2 KV in 64-column blocks (AW = heads * head_dim: H at heads of 64); the Q and K heads
//               rotated -- at head_dim 128 or with qk_norm by qknorm_rope_kernel, which first RMS-normalises every Q and K head (qk_norm)
//               ctx = causal grouped-query attention (encoder_causal.hip)
//               h = ctx Wo^T + bo + h   (Wo [H, AW])                      x -> y
//               m = RMS_post(h)                                           -> x1
//               h = (silu(gate) * up)(m W1^T + b1) W2^T + b2 + h          y -> x
//   pooled = RMS_final of the last real token's row (in f32, inside the pooling kernel), or the masked mean of RMS_final(h)
static sc_status forward_causal_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev,
                                       const PackedLayout* pk) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const int H = c.hidden, F = c.ffn, AW = (int)attn_width(c), QN = AW + 2 * (int)kv_width(c), HD = head_width(c);
    const int tokens = pk ? pk->rows : B * S;
    const int M = (tokens + 255) / 256 * 256;
    void* sk = nullptr;
    const bool scored = pk && pk->head_pool >= 0;  // the row a score head reads: the last token's, never L2-normalised
    // no split-K for a scored call, as in the pre-norm forward
    if (M <= 1024 && e->path != 1 && !scored) {
        if (!e->splitk) SC_HIP(hipMalloc(&e->splitk, sc_encoder::SPLITK_BYTES));
        sk = e->splitk;
    }
    const size_t skb = sk ? sc_encoder::SPLITK_BYTES : 0;
    if (pk) sc_launch_embed_raw_packed(ids_dev, pk->pos, tokens, M, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->x, nullptr, 0, s);
    else sc_launch_embed_raw(ids_dev, tokens, M, S, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->x, nullptr, 0, s);
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& w = e->layers[l];
        sc_launch_rmsnorm(e->x, tokens, H, w.ln1g, c.ln_eps, e->x1, s);
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.wqkv, H, w.bqkv, nullptr, 0, e->qkv, SC_LDC_BLOCKED64, M, QN, H, s, sk, skb); });
        if (HD == 128 || c.qk_norm)  // per-head RMSNorm of Q and K (qk_norm) and the rotation in one pass; the 64-wide model without it keeps rope_qk_kernel
            sc_launch_qknorm_rope(e->qkv, M, c.heads, c.kv_heads, HD, S, pk ? pk->pos : nullptr, c.max_pos, e->rope_cos, e->rope_sin, w.qng, w.kng, c.ln_eps, s);
        else launch_rope(e, M, S, pk, s);
        sc_with_prof(rt, SC_PROF_ATTN, [&] { launch_attention_causal(e, lens_dev, B, S, M, pk, s); });
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->ctx, AW, w.wo, AW, w.bo, e->x, H, e->y, H, M, H, AW, s, sk, skb); });
        sc_launch_rmsnorm(e->y, tokens, H, w.ln2g, c.ln_eps, e->x1, s);
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, 2 * F, M, 2 * F, H, s, sk, skb); });
        launch_gate(c, e->hm, M, F, e->hg, s);
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->hg, F, w.w2, F, w.b2, e->y, H, e->x, H, M, H, F, s, sk, skb); });
    }
    if (scored || e->pooling == 2) {
        sc_launch_last_pool(e->x, pk ? pk->starts : nullptr, lens_dev, B, S, H, e->fing, c.ln_eps, scored ? 0 : c.normalize, out_dev, s);
    } else {
        sc_launch_rmsnorm(e->x, tokens, H, e->fing, c.ln_eps, e->x1, s);
        launch_mean_pool(e, e->x1, lens_dev, B, S, pk, out_dev, s);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// ids_dev [B,S], lens_dev [B] device pointers; out_dev [B,H] f32 device.  pk != NULL: a packed batch -- ids_dev holds one id per token
// row of the layout (M of them), S is unused.  Caller holds e->mu.
static sc_status forward_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev,
                                const PackedLayout* pk = nullptr) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const int H = c.hidden, F = c.ffn;
    const int tokens = pk ? pk->rows : B * S;
    const int M = (tokens + 255) / 256 * 256;
    if (c.arch == 1) return forward_prenorm_locked(e, ids_dev, lens_dev, B, S, out_dev, pk);
    if (c.arch == 2) return forward_causal_locked(e, ids_dev, lens_dev, B, S, out_dev, pk);
    // batches beyond 1024 token rows (or sc_encoder_set_path 1) take the LayerNorm-folded pipeline where the model's shapes allow it
    static const bool env_fold = sc_env_flag("SC_ENC_FOLD", true);  // SC_ENC_FOLD=0: same-box A/B against the stand-alone LayerNorm kernels
    // A token call's pipeline does not follow its row count (a text's vectors are the same bits whichever batch-mates it has): the folded one
    // where the model allows it, the stand-alone one without split-K otherwise or under sc_encoder_set_path 2
    const bool tok = token_call(pk);
    if (e->foldable && e->path != 2 && (M > 1024 || e->path == 1 || tok) && env_fold) return forward_folded_locked(e, ids_dev, lens_dev, B, S, out_dev, pk);
    void* sk = nullptr;
    if (M <= 1024 && e->path != 1 && !tok) {  // a query or a few chunks: too few tiles for the chip, split K (gemm_bf16.hip)
        if (!e->splitk) SC_HIP(hipMalloc(&e->splitk, sc_encoder::SPLITK_BYTES));
        sk = e->splitk;
    }
    const size_t skb = sk ? sc_encoder::SPLITK_BYTES : 0;
    // batch steps: the FFN hidden activations travel in 64-column blocks ([F / 64][M][64]) between FFN1's epilogue and FFN2's
    // K loop, so that a wave's 16 x 64 output block and a K-tile of an A row panel are contiguous (row-major: 128-byte pieces 6 KB
    // apart).  Only the 256-tile kernel reads that layout: not with split-K (small M), not on the GEGLU path (element-wise kernel
    // in between), and only when F divides into 256-column tiles.
    const bool gated = ffn_gated(c);
    const bool ffn_blocked = !sk && !gated && (F % 256) == 0 && (H % 256) == 0 && ffn_blocked_enabled();
    const bool cls = cls_pooling(e, pk), prune = cls && cls_prune_enabled();
    if (pk && pk->types)
        sc_launch_embed_ln_pairs(ids_dev, pk->pos, pk->types, tokens, H, c.vocab, c.max_pos, c.type_vocab, e->wemb, e->pemb, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    else if (pk) sc_launch_embed_ln_packed(ids_dev, pk->pos, tokens, H, c.vocab, c.max_pos, e->wemb, e->pemb, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    else sc_launch_embed_ln(ids_dev, tokens, S, H, c.vocab, c.max_pos, e->wemb, e->pemb, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& w = e->layers[l];
        sc_with_prof(rt, SC_PROF_GEMM, [&] {
            // QKV in 64-column blocks, i.e. [3 heads][tokens][64]: attention reads each (chunk, head) operand as one contiguous block
            sc_launch_gemm_bf16(EPI_BIAS, e->x, H, w.wqkv, H, w.bqkv, nullptr, 0, e->qkv, SC_LDC_BLOCKED64, M, 3 * H, H, s, sk, skb);
        });
        if (c.pos_type == 2) launch_rope(e, M, S, pk, s);
        if (prune && l == c.layers - 1) return cls_last_layer(e, w, lens_dev, B, S, M, pk, nullptr, nullptr, out_dev);
        sc_with_prof(rt, SC_PROF_ATTN, [&] { launch_attention(e, lens_dev, B, S, M, pk, s); });
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->ctx, H, w.wo, H, w.bo, e->x, H, e->y, H, M, H, H, s, sk, skb); });
        sc_launch_layernorm(e->y, tokens, H, w.ln1g, w.ln1b, c.ln_eps, e->x1, s);
        const void* ffn_in = e->hm;
        sc_with_prof(rt, SC_PROF_GEMM, [&] {
            if (gated) sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, 2 * F, M, 2 * F, H, s, sk, skb);
            else sc_launch_gemm_bf16(EPI_BIAS_GELU, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, ffn_blocked ? SC_LDC_BLOCKED64 : F, M, F, H, s, sk, skb);
        });
        if (gated) {  // GEGLU: gelu(gate) * up; SwiGLU: silu(gate) * up
            launch_gate(c, e->hm, M, F, e->hg, s);
            ffn_in = e->hg;
        }
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, ffn_in, ffn_blocked ? SC_LDC_BLOCKED64 : F, w.w2, F, w.b2, e->x1, H, e->y, H, M, H, F, s, sk, skb); });
        sc_launch_layernorm(e->y, tokens, H, w.ln2g, w.ln2b, c.ln_eps, e->x, s);
    }
    if (tok) return launch_token_head(e, e->x, pk, s);
    if (cls) sc_launch_cls_pool(e->x, pk ? pk->starts : nullptr, B, S, H, nullptr, nullptr, c.ln_eps, c.normalize, out_dev, s);
    else launch_mean_pool(e, e->x, lens_dev, B, S, pk, out_dev, s);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

static sc_status check_embed_args(sc_encoder* e, const void* ids, const void* lens, int32_t B, int32_t S, const void* out) {
    if (!e || !ids || !lens || !out) return sc_fail(SC_ERR_INVALID, "embed: NULL argument");
    if (B < 1 || B > 65536) return sc_fail(SC_ERR_INVALID, "embed: batch %d out of range", B);
    // (arch 2: the head width is the configuration's, hidden need not be heads * head_dim -- only the rule for S is asked for)
    if (e->cfg.arch == 2 ? !sc_attention_supported(S, 64, 1, 64) : !sc_attention_supported(S, e->cfg.hidden, e->cfg.heads, e->cfg.hidden / e->cfg.heads))
        return sc_fail(SC_ERR_UNSUPPORTED, "embed: sequence length %d not in {32,64,128,256,512,1024,2048} (pad on the host)", S);
    if (S > e->cfg.max_pos && e->cfg.pos_type != 1) return sc_fail(SC_ERR_INVALID, "embed: sequence length %d exceeds max_pos %d", S, e->cfg.max_pos);
    return SC_OK;
}

// ... of sc_encoder_embed_ids_into and its _async form (`who`)
static sc_status check_into_args(sc_encoder* e, const void* ids, const void* lens, int32_t B, int32_t S, sc_index* ix, const int64_t* rows, const char* who) {
    if (!ix || !rows) return sc_fail(SC_ERR_INVALID, "%s: NULL index / rows", who);
    sc_status st = check_embed_args(e, ids, lens, B, S, rows);
    if (st) return st;
    if (ix->rt != e->rt) return sc_fail(SC_ERR_INVALID, "%s: encoder and index belong to different runtimes", who);
    if (ix->dim != e->cfg.hidden) return sc_fail(SC_ERR_INVALID, "%s: index dim %d != encoder hidden %d", who, ix->dim, e->cfg.hidden);
    return SC_OK;
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

// e->pooled into the index rows `rows`; lock order: encoder, then index (nothing takes them the other way round)
static sc_status store_pooled_locked(sc_encoder* e, sc_index* ix, const int64_t* rows, int32_t B, const char* who) {
    std::lock_guard<std::mutex> gi(ix->mu);
    return sc_index_put_rows_locked(ix, e->pooled, true, rows, B, who);
}

extern "C" sc_status sc_encoder_embed_ids_dev(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S,
                                              float* out_dev) {
    sc_status st = check_embed_args(e, ids_dev, lens_dev, B, S, out_dev);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    st = ensure_ws(e, (int64_t)B * S, B);
    if (st) return st;
    return forward_locked(e, ids_dev, lens_dev, B, S, out_dev);
}

extern "C" sc_status sc_encoder_embed_ids(sc_encoder* e, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, float* out) {
    sc_status st = check_embed_args(e, ids, lens, B, S, out);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    st = embed_host_locked(e, ids, lens, B, S);
    if (st) return st;
    hipStream_t s = e->rt->stream;
    SC_HIP(hipMemcpyAsync(out, e->pooled, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, s));
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
    st = store_pooled_locked(e, ix, rows, B, "sc_encoder_embed_ids_into");
    if (st) {
        hipStreamSynchronize(s);  // drain the stream before the upsert error is reported
        return st;
    }
    if (out) SC_HIP(hipMemcpyAsync(out, e->pooled, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

// wait for the batch that last used `slot` (its inputs may be overwritten afterwards); reports a failure of that batch's device work
static sc_status pin_slot_wait(sc_encoder::PinSlot& slot) {
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
// offsets [B + 1] of sc_encoder_embed_packed*: every rule of the header; *rows = the token rows in use (the sum of ceil32(len_i))
static sc_status check_packed_offsets(sc_encoder* e, const int64_t* offsets, int32_t B, const char* who, int64_t* rows) {
    if (!e || !offsets) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (B < 1 || B > 65536) return sc_fail(SC_ERR_INVALID, "%s: batch %d out of range", who, B);
    if (offsets[0] != 0) return sc_fail(SC_ERR_INVALID, "%s: offsets[0] must be 0 (got %lld)", who, (long long)offsets[0]);
    const int64_t max_len = e->cfg.pos_type != 1 && e->cfg.max_pos < 2048 ? e->cfg.max_pos : 2048;
    int64_t used = 0;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 1) return sc_fail(SC_ERR_INVALID, "%s: text %d has length %lld (every text needs at least one token)", who, i, (long long)len);
        if (len > max_len)
            return sc_fail(SC_ERR_INVALID, "%s: text %d has %lld tokens, more than %lld (the smaller of 2048 and the model's max_pos)", who, i, (long long)len, (long long)max_len);
        used += ceil32(len);
    }
    if ((used + 255) / 256 * 256 > SC_ENCODER_PACKED_MAX_ROWS)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: %lld token rows, more than SC_ENCODER_PACKED_MAX_ROWS = %d (split the batch)", who, (long long)used, SC_ENCODER_PACKED_MAX_ROWS);
    *rows = used;
    return SC_OK;
}

extern "C" sc_status sc_encoder_packed_rows(sc_encoder* e, const int64_t* offsets, int32_t B, int64_t* rows) {
    if (!rows) return sc_fail(SC_ERR_INVALID, "sc_encoder_packed_rows: NULL argument");
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, "sc_encoder_packed_rows", &used);
    if (st) return st;
    *rows = (used + 255) / 256 * 256;
    return SC_OK;
}

// Plans the layout of host ids / offsets into `slot` (idle, the caller waited for it), uploads it and runs the forward into e->pooled.
// index_rows (NULL or [B]) are copied behind the plan: *rows_out points at the copy.  Caller holds e->mu and has validated the
// offsets (`used` = check_packed_offsets' row count); nothing is synchronised.
// first_lens (NULL or [B], validated): the batch holds the pairs of a cross-encoder -- the first first_lens[i] rows of pair i take segment
// id 0, the rest of the pair 1, and e->pooled receives the last hidden state of every pair's first row.
// head_pool >= 0 (sc_encoder_score_seqs): e->pooled receives the rows the score head reads (PackedLayout::head_pool).
// tk != NULL (sc_encoder_embed_tokens, sc_encoder_score_late): a token call -- tk->out (device) receives the token vectors of the rows asked for,
// compactly and in text order; e->pooled is not written.  tk->expand_id >= 0: queries -- every row of a text's 32-row span is asked for and its
// alignment rows carry that token instead of token 0; < 0: documents -- the len_i real rows.
struct TokenCall {
    int32_t expand_id;
    float* out;
};
static sc_status embed_packed_locked(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, int64_t used, sc_encoder::PinSlot& slot,
                                     const int64_t* index_rows, const int64_t** rows_out, const int32_t* first_lens = nullptr, int head_pool = -1,
                                     const TokenCall* tk = nullptr) {
    const int64_t M = (used + 255) / 256 * 256;
    const PlanOffsets po((size_t)M, (size_t)B, first_lens != nullptr, tk != nullptr);
    sc_status st = pin_slot_reserve(slot, po.total + (size_t)B * 8);
    if (st) return st;
    int32_t* h_ids = (int32_t*)(slot.host + po.ids);
    int32_t* h_pos = (int32_t*)(slot.host + po.pos);
    int32_t* h_starts = (int32_t*)(slot.host + po.starts);
    int32_t* h_lens = (int32_t*)(slot.host + po.lens);
    int32_t* h_items = (int32_t*)(slot.host + po.items);
    memset(h_ids, 0, (size_t)M * 4);  // alignment rows and the tail take token 0 ...
    memset(h_pos, 0, (size_t)M * 4);  // ... the tail position 0
    int64_t row = 0;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i], span = ceil32(len);
        h_starts[i] = (int32_t)row;
        h_lens[i] = (int32_t)len;
        memcpy(h_ids + row, ids + offsets[i], (size_t)len * 4);
        for (int64_t j = 0; j < span; ++j) h_pos[row + j] = (int32_t)j;  // (the kernels clamp an alignment row's position into the table)
        row += span;
    }
    if (first_lens) {
        int32_t* h_types = (int32_t*)(slot.host + po.types);
        int32_t* h_ones = (int32_t*)(slot.host + po.ones);
        memset(h_types, 0, (size_t)M * 4);  // alignment rows and the tail take type 0
        for (int32_t i = 0; i < B; ++i) {
            for (int32_t j = first_lens[i]; j < h_lens[i]; ++j) h_types[h_starts[i] + j] = 1;
            h_ones[i] = 1;
        }
    }
    if (tk) {
        int32_t* h_dst = (int32_t*)(slot.host + po.dst);
        memset(h_dst, 0xFF, (size_t)M * 4);  // -1: alignment rows of documents and the tail are not asked for
        int32_t at = 0;
        for (int32_t i = 0; i < B; ++i) {
            const int32_t n = tk->expand_id >= 0 ? (int32_t)ceil32(h_lens[i]) : h_lens[i];
            for (int32_t j = h_lens[i]; j < n; ++j) h_ids[h_starts[i] + j] = tk->expand_id;
            for (int32_t j = 0; j < n; ++j) h_dst[h_starts[i] + j] = at++;
        }
    }
    PackedLayout pk{};
    sc_packed_items(h_starts, h_lens, B, h_items, pk.nitems);
    if (index_rows) {
        int64_t* h_rows = (int64_t*)(slot.host + po.total);
        memcpy(h_rows, index_rows, (size_t)B * 8);
        *rows_out = h_rows;
    }
    st = ensure_ws(e, M, B);
    if (st) return st;
    SC_HIP(hipMemcpyAsync(e->plan, slot.host, po.total, hipMemcpyHostToDevice, e->rt->stream));
    pk.pos = (const int32_t*)(e->plan + po.pos);
    pk.starts = (const int32_t*)(e->plan + po.starts);
    pk.items = (const int32_t*)(e->plan + po.items);
    pk.rows = (int)used;
    if (first_lens) pk.types = (const int32_t*)(e->plan + po.types);
    pk.head_pool = head_pool;
    if (tk) {
        pk.tok_dst = (const int32_t*)(e->plan + po.dst);
        pk.tok_out = tk->out;
    }
    return forward_locked(e, (const int32_t*)(e->plan + po.ids), (const int32_t*)(e->plan + (first_lens ? po.ones : po.lens)), B, 0, e->pooled, &pk);
}

static sc_status check_packed_into_args(sc_encoder* e, const void* ids, const int64_t* offsets, int32_t B, sc_index* ix, const int64_t* rows, const char* who,
                                        int64_t* used) {
    if (!ix || !rows || !ids) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    sc_status st = check_packed_offsets(e, offsets, B, who, used);
    if (st) return st;
    if (ix->rt != e->rt) return sc_fail(SC_ERR_INVALID, "%s: encoder and index belong to different runtimes", who);
    if (ix->dim != e->cfg.hidden) return sc_fail(SC_ERR_INVALID, "%s: index dim %d != encoder hidden %d", who, ix->dim, e->cfg.hidden);
    return SC_OK;
}

// The synchronous forms stage through the next pinned slot as well (after waiting for the batch that used it) and leave it idle.
extern "C" sc_status sc_encoder_embed_packed(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, float* out) {
    if (!ids || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_embed_packed: NULL argument");
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, "sc_encoder_embed_packed", &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);
    if (st) return st;
    st = embed_packed_locked(e, ids, offsets, B, used, slot, nullptr, nullptr);
    hipStream_t s = e->rt->stream;
    if (st) {
        hipStreamSynchronize(s);  // the slot's upload may be in flight
        return st;
    }
    SC_HIP(hipMemcpyAsync(out, e->pooled, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_packed_into(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, sc_index* ix, const int64_t* rows,
                                                  float* out) {
    int64_t used = 0;
    sc_status st = check_packed_into_args(e, ids, offsets, B, ix, rows, "sc_encoder_embed_packed_into", &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);
    if (st) return st;
    const int64_t* h_rows = nullptr;
    st = embed_packed_locked(e, ids, offsets, B, used, slot, rows, &h_rows);
    hipStream_t s = e->rt->stream;
    if (!st) st = store_pooled_locked(e, ix, h_rows, B, "sc_encoder_embed_packed_into");
    if (st) {
        hipStreamSynchronize(s);  // drain the stream before the error is reported
        return st;
    }
    if (out) SC_HIP(hipMemcpyAsync(out, e->pooled, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" sc_status sc_encoder_embed_packed_into_async(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, sc_index* ix,
                                                        const int64_t* rows) {
    int64_t used = 0;
    sc_status st = check_packed_into_args(e, ids, offsets, B, ix, rows, "sc_encoder_embed_packed_into_async", &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);  // two batches may be in flight; the third waits for the first
    if (st) return st;
    const int64_t* h_rows = nullptr;
    st = embed_packed_locked(e, ids, offsets, B, used, slot, rows, &h_rows);
    if (!st) st = store_pooled_locked(e, ix, h_rows, B, "sc_encoder_embed_packed_into_async");
    if (st) {
        hipStreamSynchronize(e->rt->stream);  // the slot stays idle: nothing may still read it
        return st;
    }
    SC_HIP(hipEventRecord(slot.done, e->rt->stream));
    slot.busy = true;
    e->pin_next ^= 1;
    return SC_OK;
}

// ------------------------------------------------------------------ pairs (cross-encoder / reranker)
extern "C" sc_status sc_encoder_set_pair_head(sc_encoder* e, const float* pooler_w, const float* pooler_b, const float* cls_w, const float* cls_b,
                                              int32_t num_labels) {
    if (!e) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: NULL encoder");
    const size_t H = (size_t)e->cfg.hidden;
    if (cls_w) {
        if (num_labels < 1 || num_labels > 2) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: num_labels %d outside 1 .. 2", num_labels);
        if (!cls_b) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: cls_b is NULL");
        if (pooler_w && !pooler_b) return sc_fail(SC_ERR_INVALID, "sc_encoder_set_pair_head: pooler_b is NULL");
        if (!sc_pair_head_supported((int)H, num_labels)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_set_pair_head: hidden %d must be a multiple of 16, at most 2048", (int)H);
    }
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    hipStream_t s = e->rt->stream;
    char* fresh = nullptr;
    Arena a;
    float *wp = nullptr, *bp = nullptr, *wc = nullptr, *bc = nullptr;
    auto lay = [&] {
        wp = pooler_w ? a.f32(H * H) : nullptr;
        bp = pooler_w ? a.f32(H) : nullptr;
        wc = a.f32((size_t)num_labels * H);
        bc = a.f32((size_t)num_labels);
    };
    if (cls_w) {
        lay();  // measure
        hipError_t he = hipMalloc((void**)&fresh, a.used);
        if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc pair head (%zu B) failed: %s", a.used, hipGetErrorString(he));
        a = Arena{fresh};
        lay();  // place
        hipError_t up = hipSuccess;
        auto put = [&](float* d, const float* src, size_t n) {
            if (up == hipSuccess) up = hipMemcpyAsync(d, src, n * 4, hipMemcpyHostToDevice, s);
        };
        if (pooler_w) {
            put(wp, pooler_w, H * H);
            put(bp, pooler_b, H);
        }
        put(wc, cls_w, (size_t)num_labels * H);
        put(bc, cls_b, (size_t)num_labels);
        if (up == hipSuccess) up = hipStreamSynchronize(s);  // the caller's arrays are free on return
        if (up != hipSuccess) {
            hipFree(fresh);
            return sc_fail(SC_ERR_HIP, "pair head upload failed: %s", hipGetErrorString(up));
        }
    } else {
        SC_HIP(hipStreamSynchronize(s));  // nothing may still read the head that goes
    }
    hipFree(e->head);
    e->head = fresh;
    e->head_wp = wp;
    e->head_bp = bp;
    e->head_wc = cls_w ? wc : nullptr;
    e->head_bc = cls_w ? bc : nullptr;
    e->head_labels = cls_w ? num_labels : 0;
    return SC_OK;
}

extern "C" sc_status sc_encoder_score_pairs(sc_encoder* e, const int32_t* ids, const int64_t* offsets, const int32_t* first_lens, int32_t B,
                                            float* out_logits, float* out_cls) {
    const char* who = "sc_encoder_score_pairs";
    if (!e || !ids || !offsets || !first_lens || !out_logits) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 1)  // ModernBERT's classifier is dense -> GELU -> LayerNorm -> linear; pair_head_kernel is pooler + tanh
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 1 (pre-LN) models have no pair head: their classifier is not pooler + linear", who);
    if (e->cfg.arch == 2)  // no segment ids, no [CLS] row, no pooler: rerankers of this family are out of scope
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models do not score pairs: the family has no [CLS] row and no pair head", who);
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, who, &used);
    if (st) return st;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 2) return sc_fail(SC_ERR_INVALID, "%s: pair %d has %lld token(s) (a pair needs at least 2)", who, i, (long long)len);
        if (first_lens[i] < 1 || first_lens[i] > len)
            return sc_fail(SC_ERR_INVALID, "%s: first_lens[%d] = %d outside 1 .. %lld (the pair's length)", who, i, first_lens[i], (long long)len);
        if (first_lens[i] < len && e->cfg.type_vocab < 2)
            return sc_fail(SC_ERR_INVALID, "%s: pair %d has a second segment, the model's type_vocab is %d (needs 2)", who, i, e->cfg.type_vocab);
    }
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->head_wc) return sc_fail(SC_ERR_INVALID, "%s: no pair head installed (sc_encoder_set_pair_head)", who);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);
    if (st) return st;
    st = embed_packed_locked(e, ids, offsets, B, used, slot, nullptr, nullptr, first_lens);
    hipStream_t s = e->rt->stream;
    if (st) {
        hipStreamSynchronize(s);  // the slot's upload may be in flight
        return st;
    }
    const int H = e->cfg.hidden, nl = e->head_labels;
    sc_launch_pair_head(e->pooled, B, H, e->head_wp, e->head_bp, e->head_wc, e->head_bc, nl, e->logits, s);
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(out_logits, e->logits, (size_t)B * nl * 4, hipMemcpyDeviceToHost, s));
    if (out_cls) SC_HIP(hipMemcpyAsync(out_cls, e->pooled, (size_t)B * H * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

// ------------------------------------------------------------------ score heads of the arch 1 / arch 2 rerankers
// arch: the encoder's, or -1 (sc_diag_score_head: the kernels alone, any kind, pooling not read)
sc_status sc_score_head_check(const sc_score_head* h, int arch, int H, const char* who) {
    if (arch == 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 0 (post-LN BERT family) models take the pooler + linear head of sc_encoder_set_pair_head / sc_encoder_score_pairs", who);
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
    if (h) {
        sc_status st = sc_score_head_check(h, e->cfg.arch, (int)H, who);
        if (st) return st;
    }
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    hipStream_t s = e->rt->stream;
    char* fresh = nullptr;
    Arena a;
    float *wd = nullptr, *bd = nullptr, *ng = nullptr, *nb = nullptr, *wc = nullptr, *bc = nullptr;
    auto lay = [&] {
        wd = h->dense_w ? a.f32(H * H) : nullptr;
        bd = h->dense_b ? a.f32(H) : nullptr;
        ng = h->norm_g ? a.f32(H) : nullptr;
        nb = h->norm_b ? a.f32(H) : nullptr;
        wc = a.f32((size_t)h->num_labels * H);
        bc = h->cls_b ? a.f32((size_t)h->num_labels) : nullptr;
    };
    if (h) {
        lay();  // measure
        hipError_t he = hipMalloc((void**)&fresh, a.used);
        if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc score head (%zu B) failed: %s", a.used, hipGetErrorString(he));
        a = Arena{fresh};
        lay();  // place
        hipError_t up = hipSuccess;
        auto put = [&](float* d, const float* src, size_t n) {
            if (d && up == hipSuccess) up = hipMemcpyAsync(d, src, n * 4, hipMemcpyHostToDevice, s);
        };
        put(wd, h->dense_w, H * H);
        put(bd, h->dense_b, H);
        put(ng, h->norm_g, H);
        put(nb, h->norm_b, H);
        put(wc, h->cls_w, (size_t)h->num_labels * H);
        put(bc, h->cls_b, (size_t)h->num_labels);
        if (up == hipSuccess) up = hipStreamSynchronize(s);  // the caller's arrays are free on return, and nothing still reads the head that goes
        if (up != hipSuccess) {
            hipFree(fresh);
            return sc_fail(SC_ERR_HIP, "score head upload failed: %s", hipGetErrorString(up));
        }
    } else {
        SC_HIP(hipStreamSynchronize(s));  // nothing may still read the head that goes
    }
    hipFree(e->shead);
    e->shead = fresh;
    e->sh_wd = wd;
    e->sh_bd = bd;
    e->sh_g = ng;
    e->sh_b = nb;
    e->sh_wc = h ? wc : nullptr;
    e->sh_bc = bc;
    e->sh_kind = h ? h->kind : 0;
    e->sh_pooling = h ? h->pooling : 0;
    e->sh_labels = h ? h->num_labels : 0;
    e->sh_eps = h ? h->norm_eps : 0.f;
    return SC_OK;
}

extern "C" sc_status sc_encoder_score_seqs(sc_encoder* e, const int32_t* ids, const int64_t* offsets, int32_t B, float* out_logits, float* out_rows) {
    const char* who = "sc_encoder_score_seqs";
    if (!e || !ids || !offsets || !out_logits) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (e->cfg.arch == 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 0 (post-LN BERT family) models score pairs through sc_encoder_set_pair_head / sc_encoder_score_pairs", who);
    int64_t used = 0;
    sc_status st = check_packed_offsets(e, offsets, B, who, &used);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->sh_wc) return sc_fail(SC_ERR_INVALID, "%s: no score head installed (sc_encoder_set_score_head)", who);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);
    if (st) return st;
    st = embed_packed_locked(e, ids, offsets, B, used, slot, nullptr, nullptr, nullptr, e->sh_pooling);
    hipStream_t s = e->rt->stream;
    if (st) {
        hipStreamSynchronize(s);  // the slot's upload may be in flight
        return st;
    }
    const int H = e->cfg.hidden, nl = e->sh_labels;
    sc_launch_score_head(e->pooled, B, H, e->sh_wd, e->sh_bd, e->sh_g, e->sh_b, e->sh_eps, e->sh_wc, e->sh_bc, nl, e->logits, s);
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(out_logits, e->logits, (size_t)B * nl * 4, hipMemcpyDeviceToHost, s));
    if (out_rows) SC_HIP(hipMemcpyAsync(out_rows, e->pooled, (size_t)B * H * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

// ------------------------------------------------------------------ late interaction (ColBERT): token vectors and MaxSim
extern "C" sc_status sc_encoder_set_token_head(sc_encoder* e, const float* w, int32_t W) {
    const char* who = "sc_encoder_set_token_head";
    if (!e) return sc_fail(SC_ERR_INVALID, "%s: NULL encoder", who);
    if (e->cfg.arch == 2) return sc_fail(SC_ERR_UNSUPPORTED, "%s: arch 2 (causal decoder) models have no token head: late interaction needs bidirectional token rows", who);
    const size_t H = (size_t)e->cfg.hidden;
    if (w && !sc_token_head_supported((int)H, W)) return sc_fail(SC_ERR_INVALID, "%s: W = %d must be a multiple of 16 within 16 .. 128", who, W);
    std::lock_guard<std::mutex> g(e->mu);
    SC_HIP(hipSetDevice(e->rt->device));
    hipStream_t s = e->rt->stream;
    void* fresh = nullptr;
    if (w) {
        const size_t n = (size_t)W * H;
        sc_devbuf stage;
        if (stage.alloc(n * 4) != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc token head staging (%zu B) failed", n * 4);
        hipError_t he = hipMalloc(&fresh, n * 2);
        if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc token head (%zu B) failed: %s", n * 2, hipGetErrorString(he));
        hipError_t up = hipMemcpyAsync(stage.p, w, n * 4, hipMemcpyHostToDevice, s);
        if (up == hipSuccess) {
            sc_launch_f32_to_bf16((const float*)stage.p, fresh, (int64_t)n, s);  // rounded once, as every encoder weight
            up = hipGetLastError();
        }
        const hipError_t sy = hipStreamSynchronize(s);  // the caller's array and the staging copy are free on return; nothing still reads the head that goes
        if (up == hipSuccess) up = sy;
        if (up != hipSuccess) {
            hipFree(fresh);
            return sc_fail(SC_ERR_HIP, "token head upload failed: %s", hipGetErrorString(up));
        }
    } else {
        SC_HIP(hipStreamSynchronize(s));  // nothing may still read the head that goes
    }
    hipFree(e->thead);
    e->thead = fresh;
    e->th_w = w ? W : 0;
    return SC_OK;
}

// offsets of a token call: the packed rules, a query (expand_id >= 0) of at most 128 tokens, expand_id inside the vocabulary.
// *used = packed rows, *nrows = token vectors asked for
static sc_status check_token_offsets(sc_encoder* e, const int64_t* offsets, int32_t B, int32_t expand_id, const char* who, int64_t* used, int64_t* nrows) {
    sc_status st = check_packed_offsets(e, offsets, B, who, used);
    if (st) return st;
    if (expand_id >= e->cfg.vocab) return sc_fail(SC_ERR_INVALID, "%s: expand_id %d outside the vocabulary (%d tokens)", who, expand_id, e->cfg.vocab);
    if (expand_id < 0) {
        *nrows = offsets[B];
        return SC_OK;
    }
    const bool local_layers = e->cfg.arch == 1 && e->cfg.global_every > 1;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len > MAXSIM_MAX_NQ) return sc_fail(SC_ERR_INVALID, "%s: query %d has %lld tokens, more than %d", who, i, (long long)len, MAXSIM_MAX_NQ);
        // an expansion row attends the real keys only: in a local layer its last one must still reach the text's last token
        if (local_layers && ceil32(len) - len > e->cfg.local_window / 2)
            return sc_fail(SC_ERR_INVALID, "%s: query %d has %lld tokens: its last expansion row would see no key within local_window %d", who, i, (long long)len,
                           e->cfg.local_window);
    }
    *nrows = *used;
    return SC_OK;
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
    sc_status st = check_token_offsets(e, offsets, B, expand_id, who, &used, &nrows);
    if (st) return st;
    std::lock_guard<std::mutex> g(e->mu);
    if (!e->thead) return sc_fail(SC_ERR_INVALID, "%s: no token head installed (sc_encoder_set_token_head)", who);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot& slot = e->pin[e->pin_next];
    st = pin_slot_wait(slot);
    if (st) return st;
    const size_t bytes = (size_t)nrows * e->th_w * 4;
    st = grow_locked(e, e->tok[1], bytes);
    if (st) return st;
    const TokenCall tk{expand_id, (float*)e->tok[1].p};
    st = embed_packed_locked(e, ids, offsets, B, used, slot, nullptr, nullptr, nullptr, -1, &tk);
    hipStream_t s = e->rt->stream;
    if (st) {
        hipStreamSynchronize(s);  // the slot's upload may be in flight
        return st;
    }
    SC_HIP(hipMemcpyAsync(out, e->tok[1].p, bytes, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        out_counts[i] = (int32_t)(expand_id >= 0 ? ceil32(len) : len);
    }
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
    sc_status st = check_token_offsets(e, q_offsets, Bq, expand_id, who, &q_used, &q_rows);
    if (st) return st;
    st = check_token_offsets(e, d_offsets, Bd, -1, who, &d_used, &d_rows);
    if (st) return st;
    if (expand_id < 0)  // (queries without expansion rows still have to fit the kernel)
        for (int32_t i = 0; i < Bq; ++i)
            if (q_offsets[i + 1] - q_offsets[i] > MAXSIM_MAX_NQ)
                return sc_fail(SC_ERR_INVALID, "%s: query %d has %lld tokens, more than %d", who, i, (long long)(q_offsets[i + 1] - q_offsets[i]), MAXSIM_MAX_NQ);
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
    if (!e->thead) return sc_fail(SC_ERR_INVALID, "%s: no token head installed (sc_encoder_set_token_head)", who);
    SC_HIP(hipSetDevice(e->rt->device));
    sc_encoder::PinSlot &slot_q = e->pin[e->pin_next], &slot_d = e->pin[e->pin_next ^ 1];  // one plan slot per side
    st = pin_slot_wait(slot_q);
    if (st) return st;
    st = pin_slot_wait(slot_d);
    if (st) return st;
    const int W = e->th_w;
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
    const int64_t Mq = (q_used + 255) / 256 * 256, Md = (d_used + 255) / 256 * 256;
    if (!st) st = ensure_ws(e, Mq > Md ? Mq : Md, Bq > Bd ? Bq : Bd);  // (both forwards in one workspace: no growth between them)
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
        const TokenCall tq{expand_id, (float*)e->tok[0].p}, td{-1, (float*)e->tok[1].p};
        sc_status r = embed_packed_locked(e, q_ids, q_offsets, Bq, q_used, slot_q, nullptr, nullptr, nullptr, -1, &tq);
        if (r) return r;
        r = embed_packed_locked(e, d_ids, d_offsets, Bd, d_used, slot_d, nullptr, nullptr, nullptr, -1, &td);
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

extern "C" sc_status sc_encoder_info(sc_encoder* e, sc_encoder_cfg* cfg_out) {
    if (!e || !cfg_out) return sc_fail(SC_ERR_INVALID, "sc_encoder_info: NULL argument");
    *cfg_out = e->cfg;
    return SC_OK;
}
