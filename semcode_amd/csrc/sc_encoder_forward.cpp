// sc_encoder_forward.cpp -- the forwards of the three families, as sequences of kernel launches on the workspace of a handle.
//
// Forward per layer (cfg.arch 0: BERT, post-LN):  QKV = X Wqkv^T + b  ->  attention  ->  Y = ctx Wo^T + bo + X
//   -> X1 = LN(Y) -> Hm = gelu(X1 W1^T + b1) -> Y2 = Hm W2^T + b2 + X1 -> X = LN(Y2); pooled = masked mean, or (sc_encoder_set_pooling 1)
//   the [CLS] row -- the last layer then runs on the [CLS] rows only from its attention on (cls_last_layer, encoder_cls.hip).
//   forward_locked is its small-batch form, forward_folded_locked the batch form with every LayerNorm folded into its neighbours.
// Pre-norm models (cfg.arch 1, ModernBERT), causal decoders (cfg.arch 2, the Qwen2 family) and T5 encoders (cfg.arch 3) share forward_raw_locked: h += Attn(N(h)),
//   h += MLP(N(h)) on a raw residual stream.  What a packed batch is (PackedCall, sc_encoder_plan.h) decides the two ends of each.
#include "sc_encoder_state.h"

static void launch_gate(const sc_encoder_cfg& c, const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    if (c.ffn_type == 2) sc_launch_swiglu(h, tokens, F, out, s);
    else if (c.ffn_type == 4) sc_launch_geglu_tanh(h, tokens, F, out, s);
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

// The steps both pipelines launch in a rectangle form and a packed form (pk != NULL).  Packed rotary models always rotate with the
// stand-alone kernel: the rotation fused into the QKV epilogue (EPI_LNA_BIAS_ROPE) takes its position from row & (S - 1).
// local: the table of an arch 1 model's local layers instead of the model's (global) one
static void launch_rope(sc_encoder* e, int M, int S, const PackedLayout* pk, hipStream_t s, bool local = false) {
    const float *cos_t = local ? e->rope_cos_l : e->rope_cos, *sin_t = local ? e->rope_sin_l : e->rope_sin;
    const int nblocks = e->cfg.arch == 2 ? e->cfg.heads + e->cfg.kv_heads : 2 * e->cfg.heads;  // the Q and K heads
    if (pk) sc_launch_rope_qk_packed(e->qkv, M, nblocks, pk->pos, e->cfg.max_pos, cos_t, sin_t, s);
    else sc_launch_rope_qk(e->qkv, M, nblocks, S, cos_t, sin_t, s);
}
static void launch_attention(sc_encoder* e, const int32_t* lens_dev, int B, int S, int M, const PackedLayout* pk, hipStream_t s) {
    const int hd = e->cfg.hidden / e->cfg.heads;  // 64, or 32: a pair of heads per 64-column block (Head32, attention_core.h)
    if (pk) sc_launch_attention_packed(e->qkv, pk->items, pk->nitems, e->cfg.hidden, e->slopes, e->ctx, s, M, hd);
    else sc_launch_attention(e->qkv, lens_dev, B, S, e->cfg.hidden, e->slopes, e->ctx, s, M, hd);
}
// The three steps in which the layers of the raw-stream forward (arch 1, arch 2) differ.
// norm: LayerNorm with beta (arch 1) or RMSNorm (arch 2 and 3, b unused)
static void launch_norm(const sc_encoder_cfg& c, const void* in, int tokens, const float* g, const float* b, void* out, hipStream_t s) {
    if (c.arch >= 2) sc_launch_rmsnorm(in, tokens, c.hidden, g, c.ln_eps, out, s);
    else sc_launch_layernorm(in, tokens, c.hidden, g, b, c.ln_eps, out, s);
}
// rotation of layer l: arch 1 with the table of the layer's kind; arch 2 at head_dim 128 or with qk_norm by qknorm_rope_kernel -- the per-head
// RMSNorm of Q and K and the rotation in one pass -- while the 64-wide model without it keeps rope_qk_kernel
static void launch_layer_rotation(sc_encoder* e, const LayerW& w, int l, int M, int S, const PackedLayout* pk, hipStream_t s) {
    const sc_encoder_cfg& c = e->cfg;
    if (c.arch == 3) return;  // T5 has no rotation: positions enter through the attention's bias table
    if (c.arch == 2 && (head_width(c) == 128 || c.qk_norm))
        sc_launch_qknorm_rope(e->qkv, M, c.heads, c.kv_heads, head_width(c), S, pk ? pk->pos : nullptr, c.max_pos, e->rope_cos, e->rope_sin, w.qng, w.kng, c.ln_eps, s);
    else launch_rope(e, M, S, pk, s, layer_is_local(c, l));
}
// attention of layer l: causal grouped-query (arch 2), windowed in the local layers of arch 1, the model's global kernels otherwise
static void launch_layer_attention(sc_encoder* e, int l, const int32_t* lens_dev, int B, int S, int M, const PackedLayout* pk, hipStream_t s) {
    const sc_encoder_cfg& c = e->cfg;
    if (c.arch == 2) {
        if (pk) sc_launch_attention_causal_packed(e->qkv, pk->items, pk->nitems, c.heads, c.kv_heads, head_width(c), e->ctx, s, M);
        else sc_launch_attention_causal(e->qkv, lens_dev, B, S, c.heads, c.kv_heads, head_width(c), e->ctx, s, M);
    } else if (c.arch == 3) {  // the one table serves every layer
        if (pk) sc_launch_attention_rel_packed(e->qkv, pk->items, pk->nitems, (int)attn_width(c), e->rel_tbl, c.max_pos, e->ctx, s, M);
        else sc_launch_attention_rel(e->qkv, lens_dev, B, S, (int)attn_width(c), e->rel_tbl, c.max_pos, e->ctx, s, M);
    } else if (layer_is_local(c, l)) {
        if (pk) sc_launch_attention_window_packed(e->qkv, pk->items, pk->nitems, c.hidden, c.local_window, e->ctx, s, M);
        else sc_launch_attention_window(e->qkv, lens_dev, B, S, c.hidden, c.local_window, e->ctx, s, M);
    } else {
        launch_attention(e, lens_dev, B, S, M, pk, s);
    }
}
// the token head on the rows `x` after the model's last norm, in place of a pooling kernel
static sc_status launch_token_head(sc_encoder* e, const void* x, const PackedLayout* pk, hipStream_t s) {
    sc_launch_token_head(x, pk->rows, e->cfg.hidden, e->token.w, e->token.W, pk->per_row, pk->call.tok_out, pk->call.tok_fmt, s);
    SC_HIP(hipGetLastError());
    return SC_OK;
}
// The split-K scratch of a forward on M rows, or nothing: a query or a few chunks (M <= 1024) give the chip too few 256-row tiles, so their GEMMs
// split K (gemm_bf16.hip) -- unless the batch pipeline is forced (sc_encoder_set_path 1), and never for a batch-invariant call.  A scored call
// (sc_encoder_score_seqs) and a token call are batch-invariant: the split and its factor follow the call's row count, and a pair's logits and a
// text's token vectors must be the same bits whichever batch-mates they have.  Every GEMM is then the 256-tile kernel, whose sums for a row do
// not depend on M.  The scratch is allocated on first use.
static sc_status splitk_scratch(sc_encoder* e, int M, bool batch_invariant, void** sk, size_t* bytes) {
    *sk = nullptr;
    *bytes = 0;
    if (M > 1024 || e->path == 1 || batch_invariant) return SC_OK;
    if (!e->splitk) SC_HIP(hipMalloc(&e->splitk, sc_encoder::SPLITK_BYTES));
    *sk = e->splitk;
    *bytes = sc_encoder::SPLITK_BYTES;
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
    const int H = c.hidden, F = c.ffn, Mc = (int)ceil256(B);
    const int32_t* starts = pk ? pk->starts : nullptr;
    void* sk;
    size_t skb;
    if (sc_status st = splitk_scratch(e, Mc, false, &sk, &skb)) return st;  // (decided on Mc, not M: the compact rows are what the GEMMs see)
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
    sc_launch_cls_pool(e->y, nullptr, B, 1, H, w.ln2g, w.ln2b, c.ln_eps, out_normalize(e, pk), out_dev, s);  // compact rows: text i's row is i
    SC_HIP(hipGetLastError());
    return SC_OK;
}
static void launch_mean_pool(sc_encoder* e, const void* x, const int32_t* lens_dev, int B, int S, const PackedLayout* pk, float* out_dev, hipStream_t s) {
    if (pk) sc_launch_mean_pool_packed(x, pk->starts, lens_dev, B, e->cfg.hidden, out_normalize(e, pk), out_dev, s);
    else sc_launch_mean_pool(x, lens_dev, B, S, e->cfg.hidden, out_normalize(e, pk), out_dev, s);
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
    const int M = (int)ceil256(tokens);
    const int slots = H / 256;
    // statistics buffers are laid out for ws_tokens rows; this call uses the first M rows of every slot: slot stride must be M, so
    // they are addressed as [slots][M][2] inside the (larger or equal) allocation
    const bool gated = ffn_gated(c);
    const bool ffn_blocked = !gated && ffn_blocked_enabled();
    const bool rope = c.pos_type == 2, rope_fused = rope && !pk && (g_rope_fused < 0 ? ROPE_FUSED_DEFAULT : g_rope_fused) != 0;
    const bool cls = cls_pooling(e, pk), prune = cls && cls_prune_enabled();
    if (pair_call(pk))
        sc_launch_embed_raw_pairs(ids_dev, pk->pos, pk->per_row, tokens, M, H, c.vocab, c.max_pos, c.type_vocab, e->wemb, e->pemb, e->temb, e->x, e->stat_b, slots, s);
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
        sc_launch_cls_pool(e->x, pk ? pk->starts : nullptr, B, S, H, last.ln2g, last.ln2b, c.ln_eps, out_normalize(e, pk), out_dev, s);
    } else if (out_normalize(e, pk)) {  // L2-normalised output: the plain pooling kernel does it; give it the normalised rows
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

// The forward of the two families whose residual stream h stays RAW between the sub-layers -- pre-norm encoders (cfg.arch 1, ModernBERT) and
// causal decoders (cfg.arch 2, the Qwen2 family) -- on the stand-alone-norm launches for every batch size (split-K GEMMs up to 1 024 rows, the
// 256-tile GEMMs beyond):
//   per layer:  a = N_in(h)                                               -> x1
//               QKV = a Wqkv^T + b, N = AW + 2 KV in 64-column blocks, the Q and K heads rotated
//               ctx = attention
//               h = ctx Wo^T + bo + h   (Wo [H, AW])                      x -> y   (EPI_BIAS_RES, the raw stream as residual)
//               m = N_post(h)                                             -> x1
//               h = (act(gate) * up)(m W1^T + b1) W2^T + b2 + h           y -> x
//                 arch 1                                                     | arch 2
//   h at first    LN_emb(word embedding) -> x                                | bf16(tok_emb[id]) -> x (raw embedding kernels, no position table)
//   N             LayerNorm; layer 0 reads x itself (attn_norm = identity)   | RMSNorm, in every layer
//   widths        AW = KV = H                                                | AW = heads * head_dim (H at heads of 64), KV = kv_heads * head_dim
//   rotation      the table of the layer's kind (global / local base)        | at head_dim 128 or with qk_norm by qknorm_rope_kernel, which first
//                                                                            | RMS-normalises every Q and K head (qk_norm)
//   attention     windowed in the local layers (encoder_window.hip), the     | causal grouped-query (encoder_causal.hip)
//                 model's global kernels otherwise; act = gelu               | act = silu
//   pooled        masked mean of final_norm(h), or final_norm of the [CLS]   | RMS_final of the last real token's row (in f32, inside the
//                 row (in f32, inside the pooling kernel; never pruned:      | pooling kernel), or the masked mean of RMS_final(h)
//                 cls_last_layer is the post-LN layer); a token call: the    | (never a token call: the heads refuse arch 2)
//                 token head on final_norm(h)                                |
// T5 encoders (cfg.arch 3) are the third column: h at first and N as arch 2 (raw embedding kernels, RMSNorm in every layer); widths AW = KV =
// heads * 64 (H unless head_dim 64 is stated); NO rotation; attention = the global kernels on Head64Rel (scores q.k + the bias table of the
// distance, one table for all layers, no 1/8); feed-forward act = ReLU as a pass of its own over FFN1's [M, F] output (ffn_type 3) or the
// tanh-GELU gate (ffn_type 4); pooled = the masked mean of RMS_final(h), or RMS_final of the FIRST token's row in f32 (the last-token kernel
// under lengths of 1); never a scored or a token call (the heads refuse arch 3).
static sc_status forward_raw_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev,
                                    const PackedLayout* pk) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const bool causal = c.arch == 2, raw_emb = c.arch >= 2;  // arch 2 and 3: h starts as the token embedding itself, RMSNorm in every layer
    const int H = c.hidden, F = c.ffn, AW = (int)attn_width(c), QN = AW + 2 * (int)kv_width(c);
    const int tokens = pk ? pk->rows : B * S;
    const int M = (int)ceil256(tokens);
    const bool scored = scored_call(pk);  // the row a score head reads: its own pooling, never L2-normalised
    void* sk;
    size_t skb;
    if (sc_status st = splitk_scratch(e, M, scored || token_call(pk), &sk, &skb)) return st;
    if (raw_emb && pk) sc_launch_embed_raw_packed(ids_dev, pk->pos, tokens, M, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->x, nullptr, 0, s);
    else if (raw_emb) sc_launch_embed_raw(ids_dev, tokens, M, S, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->x, nullptr, 0, s);
    else if (pk) sc_launch_embed_ln_packed(ids_dev, pk->pos, tokens, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    else sc_launch_embed_ln(ids_dev, tokens, S, H, c.vocab, c.max_pos, e->wemb, nullptr, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
    for (int l = 0; l < c.layers; ++l) {
        const LayerW& w = e->layers[l];
        const void* a = e->x;
        if (raw_emb || l > 0) {
            launch_norm(c, e->x, tokens, w.ln1g, w.ln1b, e->x1, s);
            a = e->x1;
        }
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, a, H, w.wqkv, H, w.bqkv, nullptr, 0, e->qkv, SC_LDC_BLOCKED64, M, QN, H, s, sk, skb); });
        launch_layer_rotation(e, w, l, M, S, pk, s);
        sc_with_prof(rt, SC_PROF_ATTN, [&] { launch_layer_attention(e, l, lens_dev, B, S, M, pk, s); });
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, e->ctx, AW, w.wo, AW, w.bo, e->x, H, e->y, H, M, H, AW, s, sk, skb); });
        launch_norm(c, e->y, tokens, w.ln2g, w.ln2b, e->x1, s);
        const void* ffn_in = e->hg;
        if (c.ffn_type == 3) {  // Linear-ReLU-Linear (T5 v1.0): the ReLU as a pass of its own over FFN1's output, no gate
            sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, F, M, F, H, s, sk, skb); });
            sc_launch_relu(e->hm, (int64_t)M * F, s);
            ffn_in = e->hm;
        } else {
            sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS, e->x1, H, w.w1, H, w.b1, nullptr, 0, e->hm, 2 * F, M, 2 * F, H, s, sk, skb); });
            launch_gate(c, e->hm, M, F, e->hg, s);
        }
        sc_with_prof(rt, SC_PROF_GEMM, [&] { sc_launch_gemm_bf16(EPI_BIAS_RES, ffn_in, F, w.w2, F, w.b2, e->y, H, e->x, H, M, H, F, s, sk, skb); });
    }
    const int32_t* starts = pk ? pk->starts : nullptr;
    if (causal && (scored || e->pooling == 2)) {
        sc_launch_last_pool(e->x, starts, lens_dev, B, S, H, e->fing, c.ln_eps, out_normalize(e, pk), out_dev, s);
    } else if (c.arch == 3 && cls_pooling(e, pk)) {  // T5, first token: the last-token kernel under lengths of 1 -- RMS_final in f32 on B rows
        sc_launch_last_pool(e->x, starts, e->ones, B, S, H, e->fing, c.ln_eps, out_normalize(e, pk), out_dev, s);
    } else if (!causal && (scored ? pk->call.head_pool == 1 : cls_pooling(e, pk))) {
        sc_launch_cls_pool(e->x, starts, B, S, H, e->fing, e->finb, c.ln_eps, out_normalize(e, pk), out_dev, s);
    } else {
        launch_norm(c, e->x, tokens, e->fing, e->finb, e->x1, s);
        if (token_call(pk)) return launch_token_head(e, e->x1, pk, s);
        launch_mean_pool(e, e->x1, lens_dev, B, S, pk, out_dev, s);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// ids_dev [B,S], lens_dev [B] device pointers; out_dev [B,H] f32 device.  pk != NULL: a packed batch -- ids_dev holds one id per token
// row of the layout (M of them), S is unused.  Caller holds e->mu.
sc_status forward_locked(sc_encoder* e, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S, float* out_dev, const PackedLayout* pk) {
    const sc_encoder_cfg& c = e->cfg;
    sc_runtime* rt = e->rt;
    hipStream_t s = rt->stream;
    const int H = c.hidden, F = c.ffn;
    const int tokens = pk ? pk->rows : B * S;
    const int M = (int)ceil256(tokens);
    if (c.arch != 0) return forward_raw_locked(e, ids_dev, lens_dev, B, S, out_dev, pk);
    // batches beyond 1024 token rows (or sc_encoder_set_path 1) take the LayerNorm-folded pipeline where the model's shapes allow it
    static const bool env_fold = sc_env_flag("SC_ENC_FOLD", true);  // SC_ENC_FOLD=0: same-box A/B against the stand-alone LayerNorm kernels
    // A token call's pipeline does not follow its row count (a text's vectors are the same bits whichever batch-mates it has): the folded one
    // where the model allows it, the stand-alone one without split-K otherwise or under sc_encoder_set_path 2
    const bool tok = token_call(pk);
    if (e->foldable && e->path != 2 && (M > 1024 || e->path == 1 || tok) && env_fold) return forward_folded_locked(e, ids_dev, lens_dev, B, S, out_dev, pk);
    void* sk;
    size_t skb;
    if (sc_status st = splitk_scratch(e, M, tok, &sk, &skb)) return st;
    // batch steps: the FFN hidden activations travel in 64-column blocks ([F / 64][M][64]) between FFN1's epilogue and FFN2's
    // K loop, so that a wave's 16 x 64 output block and a K-tile of an A row panel are contiguous (row-major: 128-byte pieces 6 KB
    // apart).  Only the 256-tile kernel reads that layout: not with split-K (small M), not on the GEGLU path (element-wise kernel
    // in between), and only when F divides into 256-column tiles.
    const bool gated = ffn_gated(c);
    const bool ffn_blocked = !sk && !gated && (F % 256) == 0 && (H % 256) == 0 && ffn_blocked_enabled();
    const bool cls = cls_pooling(e, pk), prune = cls && cls_prune_enabled();
    if (pair_call(pk))
        sc_launch_embed_ln_pairs(ids_dev, pk->pos, pk->per_row, tokens, H, c.vocab, c.max_pos, c.type_vocab, e->wemb, e->pemb, e->temb, e->embg, e->embb, c.ln_eps, e->x, s);
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
    if (cls) sc_launch_cls_pool(e->x, pk ? pk->starts : nullptr, B, S, H, nullptr, nullptr, c.ln_eps, out_normalize(e, pk), out_dev, s);
    else launch_mean_pool(e, e->x, lens_dev, B, S, pk, out_dev, s);
    SC_HIP(hipGetLastError());
    return SC_OK;
}
