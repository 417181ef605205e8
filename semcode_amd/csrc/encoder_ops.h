// encoder_ops.h -- the encoder's device entry points: what gemm_bf16.hip and encoder_ops.hip define and the encoder host files
// (sc_encoder_*.cpp) call.  Defaults of optional arguments live here only; the .hip files include this header,
// so a definition that drifts from its prototype does not compile.  All launchers enqueue on `s` and never synchronise.
#pragma once
#include <vector>

#include "sc_common.h"

// GEMM epilogues (gemm_bf16.hip describes the LayerNorm-folded ones)
enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RES = 2, EPI_LNA_BIAS = 3, EPI_LNA_GELU = 4, EPI_RESLN_STATS = 5, EPI_LNA_BIAS_ROPE = 6 };

// ---- gemm_bf16.hip
bool sc_gemm_bf16_supported(int M, int N, int K);
// splitk_scratch (optional, f32): lets small-M GEMMs run as tile x K-slice workgroups + a reduce/epilogue kernel
void sc_launch_gemm_bf16(int epi, const void* A, int lda, const void* W, int ldw, const float* bias, const void* R, int ldr, void* C,
                         int ldc, int M, int N, int K, hipStream_t s, void* splitk_scratch = nullptr, size_t splitk_scratch_bytes = 0);
int sc_gemm_splitk_factor(int M, int N, int K, int cus);
// The kernel a plain launch takes: tile 128 or 256 (0: nothing was launched -- blocked A handed to a launch the per-tile 256-tile kernel
// does not serve), K slices (1 = no split-K), the walk order word, the ring depth (0 = one barrier per K-tile) and non-temporal C stores.
struct ScGemmPath { int tile, splitk, order, pp, nt; };
ScGemmPath sc_gemm_plain_path(int M, int N, int K, int cus, size_t scratch_bytes);  // under the current options; host arithmetic
ScGemmPath sc_gemm_last_path(void);                                                 // of the last sc_launch_gemm_bf16 of this process
// LayerNorm-folded batch pipeline (EPI_LNA_* / EPI_RESLN_STATS)
bool sc_gemm_ln_supported(int M, int N, int K);
void sc_launch_gemm_bf16_ln(int epi, const void* A, int lda, const void* W, int ldw, const float* bias, const void* R, int ldr, void* C, int ldc, int M,
                            int N, int K, hipStream_t s, const float* c1, const float* stats_in, float* fin, const float* gam, float* stats_out, float eps,
                            const float* rope_cos = nullptr, const float* rope_sin = nullptr, int rope_S = 0, int rope_ncols = 0);
void sc_launch_gemm_i8_diag(const void* A, const void* W, void* C, int M, int N, int K, hipStream_t s);
// process-wide knobs of the launchers (sc_diag_set_option "gemm_pp" / "gemm_nt" / "gemm_order" / "gemm_strip" / "gemm_strip_n", sc_diag_gemm_trace,
// sc_diag_gemm_bench)
void sc_gemm_set_debug(int v);
void sc_gemm_set_order(int v);
void sc_gemm_set_pp(int v);
void sc_gemm_set_nt(int v);
void sc_gemm_set_strip(int v);
void sc_gemm_set_strip_n(int v);
int sc_gemm_strip_rule(int M, int N, int K, int cus);                       // the shape rule alone (host arithmetic)
int sc_gemm_strip_tiles(int M, int N, int K, int cus, bool a_blocked = false);  // ... under the current options: tiles per strip, 0 = per-tile
int sc_gemm_last_strip(void);                                                // tiles per strip of the last EPI_LNA_* launch (0 = per-tile kernel)
void sc_gemm_set_trace(unsigned long long* dev);
void sc_gemm_force_tile128(bool on);

// ---- encoder_ops.hip
void sc_launch_embed_ln(const int32_t* ids, int tokens, int S, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                        const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s);
void sc_launch_layernorm(const void* in, int tokens, int H, const float* g, const float* b, float eps, void* out, hipStream_t s);
// head_dim 64, or 32 (plain attention only: slopes must be NULL): a 64-column block of qkv / ctx then holds a pair of heads
bool sc_attention_supported(int S, int H, int heads, int head_dim = 64);
void sc_launch_attention(const void* qkv, const int32_t* lens, int B, int S, int H, const float* slopes, void* ctx, hipStream_t s, int blocked = 0,
                         int head_dim = 64);
void sc_launch_geglu(const void* h, int64_t tokens, int F, void* out, hipStream_t s);
void sc_launch_swiglu(const void* h, int64_t tokens, int F, void* out, hipStream_t s);
// T5 (cfg.arch 3).  geglu_tanh: the gate with the tanh-GELU ("gelu_new"), layout of the two above.  relu: in place on h [n] bf16, n a multiple of 8.
// attention_rel / _rel_packed: sc_launch_attention / _packed for heads of 64 with scores q.k + tbl[head][key - query + span - 1] and NO 1/sqrt(d):
// tbl [H / 64][2 span - 1] f32 on the device (sc_rel_bias_table); H = the attention width, heads * 64.
void sc_launch_geglu_tanh(const void* h, int64_t tokens, int F, void* out, hipStream_t s);
void sc_launch_relu(void* h, int64_t n, hipStream_t s);
void sc_launch_attention_rel(const void* qkv, const int32_t* lens, int B, int S, int H, const float* tbl, int span, void* ctx, hipStream_t s, int blocked = 0);
void sc_launch_attention_rel_packed(const void* qkv, const int32_t* items, const int* nitems, int H, const float* tbl, int span, void* ctx, hipStream_t s,
                                    int blocked = 0);
// rotary positions: in-place rotation of the first `nblocks` 64-column blocks (Q and K heads) of a blocked buffer [blocks][M][64];
// cos / sin [>= S][32] f32, row r is position r % S
void sc_launch_rope_qk(void* qkv, int64_t M, int nblocks, int S, const float* cos_t, const float* sin_t, hipStream_t s);
void sc_launch_embed_raw(const int32_t* ids, int tokens, int tokens_pad, int S, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                         const float* temb, void* out, float* stats, int slots, hipStream_t s);
void sc_launch_fold_ln_weights(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, void* Wf, float* c1, float* c2,
                               hipStream_t s);
void sc_launch_add_vectors(const float* a, const float* b, float* out, int n, hipStream_t s);
void sc_launch_mean_pool_ln(const void* y, const float* stats, int slots, int tokens_pad, const float* gamma, const float* beta, float eps,
                            const int32_t* lens, int B, int S, int H, float* out, hipStream_t s);
void sc_launch_mean_pool(const void* x, const int32_t* lens, int B, int S, int H, int normalize, float* out, hipStream_t s);
void sc_launch_f32_to_bf16(const float* in, void* out, int64_t n, hipStream_t s);
void sc_launch_synth_scaled(float* out, int64_t n, uint64_t seed, float scale, float offset, hipStream_t s);
void sc_launch_bf16_to_f32(const void* in, float* out, int64_t n, hipStream_t s);

// ---- encoder_packed.hip: the position-aware steps on packed variable-length rows.  pos [rows] = position of every token row inside
// its sequence, starts / lens [B] = first row and real length of every sequence, items = the attention work-item table
// sc_packed_items builds (4 int32 per item, sorted by launch class, nitems[3] per class).  All device pointers.
void sc_launch_embed_ln_packed(const int32_t* ids, const int32_t* pos, int tokens, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                               const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s);
void sc_launch_embed_raw_packed(const int32_t* ids, const int32_t* pos, int tokens, int tokens_pad, int H, int vocab, int max_pos, const float* wemb,
                                const float* pemb, const float* temb, void* out, float* stats, int slots, hipStream_t s);
void sc_launch_rope_qk_packed(void* qkv, int64_t M, int nblocks, const int32_t* pos, int max_pos, const float* cos_t, const float* sin_t, hipStream_t s);
int sc_packed_attention_class(int len);  // 0: longer than 256 tokens, 1: up to 256, 2: up to 128
void sc_launch_attention_packed(const void* qkv, const int32_t* items, const int* nitems, int H, const float* slopes, void* ctx, hipStream_t s, int blocked = 0,
                                int head_dim = 64);
void sc_launch_mean_pool_packed(const void* x, const int32_t* starts, const int32_t* lens, int B, int H, int normalize, float* out, hipStream_t s);
void sc_launch_mean_pool_ln_packed(const void* y, const float* stats, int slots, int tokens_pad, const float* gamma, const float* beta, float eps,
                                   const int32_t* starts, const int32_t* lens, int B, int H, float* out, hipStream_t s);

// ---- encoder_window.hip: local (sliding-window) attention, head dimension 64, plain scores: a query sees the real keys with
// |query - key| <= local_window / 2.  local_window even, 2 .. 128; the other arguments as the two attention launchers above.
bool sc_attention_window_supported(int local_window);
void sc_launch_attention_window(const void* qkv, const int32_t* lens, int B, int S, int H, int local_window, void* ctx, hipStream_t s, int blocked = 0);
void sc_launch_attention_window_packed(const void* qkv, const int32_t* items, const int* nitems, int H, int local_window, void* ctx, hipStream_t s,
                                       int blocked = 0);

// ---- encoder_causal.hip: the causal decoder family (cfg.arch 2).  Causal grouped-query attention, head dimension 64 (128 below), plain scores: a query
// sees the real keys at or before its own position; query head h reads K / V head h / (heads / kv_heads).  qkv rows are
// [Q (heads) | K (kv_heads) | V (kv_heads)] x 64 columns, row-major (blocked 0) or in 64-column blocks of `blocked` rows; ctx [rows, heads * 64];
// lens / items as the two attention launchers above.  rmsnorm: x * rsqrt(mean(x^2) + eps) * gamma, bf16 rows, H a multiple of 8, <= 2048.
// last_pool: the row start + len - 1 of every text (starts NULL: a [B, S] rectangle, lens clamped to 1 .. S) of x [rows, H] bf16, RMSNorm in
// f32, optional L2 normalisation by the rule of the mean kernels -> out [B, H] f32.
// head_dim 128: a head is two consecutive 64-column blocks, qkv rows are [Q | K | V] x 128 columns, ctx [rows, heads * 128].
// qknorm_rope: in place on the 64-column blocks [(heads + kv_heads) * head_dim / 64 ...][M][64] of the Q and K heads: RMSNorm over each head's
// head_dim values when gq / gk [head_dim] are non-NULL (both or neither), then the rotate-half rotation from the tables [max_pos][head_dim / 2].
// pos NULL: position = row & (S - 1), S a power of two; else pos [M], clamped to max_pos - 1.
bool sc_attention_causal_supported(int heads, int kv_heads, int head_dim = 64);
void sc_launch_attention_causal(const void* qkv, const int32_t* lens, int B, int S, int heads, int kv_heads, int head_dim, void* ctx, hipStream_t s, int blocked = 0);
void sc_launch_attention_causal_packed(const void* qkv, const int32_t* items, const int* nitems, int heads, int kv_heads, int head_dim, void* ctx, hipStream_t s,
                                       int blocked = 0);
void sc_launch_qknorm_rope(void* qkv, int64_t M, int heads, int kv_heads, int head_dim, int S, const int32_t* pos, int max_pos, const float* cos_t, const float* sin_t,
                           const float* gq, const float* gk, float eps, hipStream_t s);
void sc_launch_rmsnorm(const void* in, int tokens, int H, const float* g, float eps, void* out, hipStream_t s);
void sc_launch_last_pool(const void* x, const int32_t* starts, const int32_t* lens, int B, int S, int H, const float* gamma, float eps, int normalize, float* out,
                         hipStream_t s);

// ---- encoder_pairs.hip: the packed embedding with a per-row segment id (types [rows], clamped into type_emb's type_vocab rows), and
// the classification head of a cross-encoder: cls [B,H] f32 -> logits [B,num_labels] = Wc p + bc, p = tanh(Wp cls + bp), or p = cls when
// Wp is NULL.  Wp [H,H], bp [H], Wc [num_labels,H], bc [num_labels] f32 on the device; H a multiple of 16, <= 2048; num_labels 1 or 2.
void sc_launch_embed_ln_pairs(const int32_t* ids, const int32_t* pos, const int32_t* types, int tokens, int H, int vocab, int max_pos, int type_vocab,
                              const float* wemb, const float* pemb, const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s);
void sc_launch_embed_raw_pairs(const int32_t* ids, const int32_t* pos, const int32_t* types, int tokens, int tokens_pad, int H, int vocab, int max_pos,
                               int type_vocab, const float* wemb, const float* pemb, const float* temb, void* out, float* stats, int slots, hipStream_t s);
bool sc_pair_head_supported(int H, int num_labels);
void sc_launch_pair_head(const float* cls, int B, int H, const float* Wp, const float* bp, const float* Wc, const float* bc, int num_labels, float* logits,
                         hipStream_t s);

// ---- encoder_heads.hip: the score heads of the arch 1 / arch 2 rerankers on r [B,H] f32 (device) -> logits [B,num_labels].  Wd non-NULL (kind 1):
// g = gelu_erf(Wd r + bd), p = LayerNorm(g; gam, bet, eps) with two-pass statistics, logits = Wc p + bc.  Wd NULL (kind 2): logits = Wc r + bc.
// Wd [H,H], bd / gam / bet [H], Wc [num_labels,H], bc [num_labels] f32 on the device, 16-byte aligned; bd, bet, bc may be NULL (zeros);
// H a multiple of 16, <= 2048; num_labels 1 or 2; eps > 0.
bool sc_score_head_supported(int H, int num_labels);
void sc_launch_score_head(const float* r, int B, int H, const float* Wd, const float* bd, const float* gam, const float* bet, float eps, const float* Wc,
                          const float* bc, int num_labels, float* logits, hipStream_t s);

// ---- encoder_tokens.hip: late interaction.  token_head: x [rows, H] bf16 (rows a multiple of 32), w [W, H] bf16, dst [rows] = the compact output
// row of every packed row or -1 -> out[dst][W] f32 = the L2-normalised projection (the pooling kernels' 1e-12 rule).  W % 16 == 0, 16 .. 128;
// H % 32 == 0.  fmt 1: out[dst][W] bf16 instead, every component of that f32 vector rounded once by late_round_bf16 (the token pool of an
// index at fmt 1).  maxsim: the rule of maxsim_rule.h over P pairs: Q [.., W] / D [.., W] f32 token vectors, text i's at rows [off[i], off[i + 1]),
// keep NULL or one byte per document token, pair_q / pair_d [P] -> out [P].  A query has at most 128 tokens.  All device pointers.
bool sc_token_head_supported(int H, int W);
void sc_launch_token_head(const void* x, int rows, int H, const void* w, int W, const int32_t* dst, void* out, int fmt, hipStream_t s);
void sc_launch_maxsim(const float* Q, const int32_t* q_off, const float* D, const int32_t* d_off, const uint8_t* keep, const int32_t* pair_q, const int32_t* pair_d,
                      int P, int W, float* out, hipStream_t s);

// ---- encoder_cls.hip: [CLS] pooling.  starts NULL: text i's first row is i * S (a rectangle), else starts[i] (packed rows).
// cls_pool: that row of x [rows, H] bf16 -> out [B, H] f32; gamma / beta non-NULL: the rows are raw and are LayerNorm'ed (f32) first; normalize:
// L2 normalisation by the rule of the mean kernels.  cls_gather: the same rows (optionally LayerNorm'ed) as bf16 [rows_pad, H], rows B .. rows_pad zero.
// attention_cls: one query row per text (its first) over the text's lens[i] keys (rectangles: clamped to 1 .. S; at most 2048), qkv in 64-column
// blocks of M rows, head_dim 64 or 32, slopes NULL or [heads] -> ctx [rows_pad, H] bf16 row-major, rows B .. rows_pad zero.
void sc_launch_cls_pool(const void* x, const int32_t* starts, int B, int S, int H, const float* gamma, const float* beta, float eps, int normalize, float* out,
                        hipStream_t s);
void sc_launch_cls_gather(const void* x, const int32_t* starts, int B, int S, int H, const float* gamma, const float* beta, float eps, void* out, int rows_pad,
                          hipStream_t s);
void sc_launch_attention_cls(const void* qkv, const int32_t* starts, const int32_t* lens, int B, int S, int M, int H, int head_dim, const float* slopes, void* ctx,
                             int rows_pad, hipStream_t s);

// ---- encoder_proj.hip: the output projection behind the pooling.  x [B,H] f32 (un-normalised pooled rows), W [E,H], bias [E] or NULL, f32 on
// the device, 16-byte aligned -> out [B,E] = W x + bias, L2-normalised (x / max(|x|, 1e-12)) when normalize.  H, E multiples of 16, 16 .. 2048.
bool sc_output_proj_supported(int H, int E);
void sc_launch_output_proj(const float* x, int B, int H, const float* W, const float* bias, int E, int normalize, float* out, hipStream_t s);

// ---- sc_encoder_heads.cpp: the rules of a score head, with sc_fail's message under `who`.  arch: the encoder's (0 is refused), or -1 for the kernels
// alone (sc_diag_score_head: any kind, pooling not read)
sc_status sc_score_head_check(const sc_score_head* h, int arch, int H, const char* who);

// ---- sc_encoder_model.cpp: the rotary tables those kernels read.  [positions][32] cos, then [positions][32] sin: rotate-half (GPT-NeoX)
// angles p * theta^(-2 i / 64), i < 32, computed in double; theta <= 0 means 10000.  head_dim 128: [positions][64] each, p * theta^(-2 i / 128)
std::vector<float> sc_rope_table(int64_t positions, float theta, int head_dim = 64);
