// encoder_ops.hip -- the non-GEMM kernels of the transformer-encoder forward (gfx950).
//
// Replaces (reference): what llama.cpp's BERT graph does around the matmuls behind
// LlamaCppEmbeddings.embed_documents / embed_query (src/semcode/embeddings/providers.py:69-100;
// call sites src/semcode/services/indexer.py:150, src/semcode/rag/pipeline.py:171-175):
// token/position/type embedding + LayerNorm, post-attention / post-FFN LayerNorm, masked softmax
// attention, masked mean pooling.  Arithmetic follows BertModel (post-LN, eps inside sqrt, biased
// variance, erf-GELU, additive key mask), restated on CPU in oracle/bert_oracle.py.
//
//   embed_ln_kernel   HBM-bound  : 1 wave / token, f32 tables -> bf16 activations
//   layernorm_kernel  HBM-bound  : 1 wave / token, bf16 -> bf16 (the residual add is fused into the
//                                  producing GEMM's epilogue)
//   attention_kernel  MFMA + LDS : 1 workgroup / (chunk, head of 64 or pair of heads of 32); K and V stay in LDS,
//                                  S^T = K Q^T on v_mfma_f32_32x32x16_bf16 so a lane owns one query
//                                  column, softmax in registers, P feeds P V straight from the
//                                  accumulator registers, V fragments by ds_read_b64_tr_b16.  The math and the head
//                                  widths are attention_core.h's; attention_long_kernel (1 024 / 2 048 tokens) folds
//                                  the keys in segments of 512
//   mean_pool_kernel  HBM-bound  : 1 workgroup / chunk, masked mean (+ optional L2 normalise) -> f32
//   glu_kernel<ACT>   HBM-bound  : gated feed-forward act(gate) * up between the FFN GEMMs (GEGLU: jina-bert-v2, SwiGLU: nomic-bert)
//   rope_qk_kernel    HBM-bound  : rotary position embedding of Q and K, in place on the blocked QKV buffer (nomic-bert)
#include "attention_core.h"  // Head64 / Head32, attn_lds_bytes, attn_launch
#include "encoder_ops.h"
#include "encoder_rows.h"   // the bodies of the embedding, rotary and pooling kernels, wave_sum
#include "gemm_tile.h"  // bf16 helpers, LDS-DMA pointer types

// ------------------------------------------------------------------ embeddings + LayerNorm
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ ids, int tokens, int S, int H, int vocab, int max_pos,
                                                        const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                        const float* __restrict__ temb, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    embed_ln_rows(ids, tokens, PosInRect{S}, H, vocab, max_pos, wemb, pemb, temb, gamma, beta, eps, out);
}

// ------------------------------------------------------------------ LayerNorm-folded batch pipeline (sc_encoder.cpp, gemm_bf16.hip EPI_LNA_* / EPI_RESLN_STATS)
// Embeddings WITHOUT their LayerNorm: the raw sum (bf16) plus the row statistics the consuming GEMM folds in -- slot 0 of
// stats [slots][tokens_pad][2] gets (sum, sum of squares) of the bf16-ROUNDED row, the other slots zero (a GEMM-produced tensor
// fills one slot per 256 columns).
__global__ __launch_bounds__(256) void embed_raw_kernel(const int32_t* __restrict__ ids, int tokens, int tokens_pad, int S, int H, int vocab, int max_pos,
                                                         const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                         const float* __restrict__ temb, bf16_t* __restrict__ out, float* __restrict__ stats, int slots) {
    embed_raw_rows(ids, tokens, tokens_pad, PosInRect{S}, H, vocab, max_pos, wemb, pemb, temb, out, stats, slots);
}

// W' = bf16(W diag(gamma)), c1[n] = sum_k W'[n,k] (of the ROUNDED values: it cancels what the MFMA accumulates),
// c2[n] = bias[n] + sum_k beta[k] W[n,k].  One wave per output row n.
__global__ __launch_bounds__(256) void fold_ln_weights_kernel(const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ bias, int N, int K, bf16_t* __restrict__ Wf,
                                                               float* __restrict__ c1, float* __restrict__ c2) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float s1 = 0.f, s2 = 0.f;
    for (int k0 = 4 * lane; k0 < K; k0 += 256) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k0);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + k0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(beta + k0);
        u16x4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            r[c] = f32_to_bf16(w[c] * g[c]);
            s1 += bf16_to_f32(r[c]);
            s2 = fmaf(b[c], w[c], s2);
        }
        *reinterpret_cast<u16x4*>(Wf + (size_t)n * K + k0) = r;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        c1[n] = s1;
        c2[n] = (bias ? bias[n] : 0.f) + s2;
    }
}
__global__ __launch_bounds__(256) void add_vectors_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// masked mean pooling of LayerNorm(y) computed on the fly from the raw rows and their partial statistics:
// mean_t LN(y_t) = gamma * (sum_t rs_t y_t - sum_t rs_t mu_t) / len + beta.  One workgroup per (chunk, 256 columns).
__global__ __launch_bounds__(256) void mean_pool_ln_kernel(const bf16_t* __restrict__ y, const float* __restrict__ stats, int slots, int tokens_pad,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            const int32_t* __restrict__ lens, int S, int H, float* __restrict__ out) {
    mean_pool_ln_rows(y, stats, slots, tokens_pad, gamma, beta, eps, RectRows{lens, S}, blockIdx.y, blockIdx.x, H, out);
}

// ------------------------------------------------------------------ LayerNorm (input already holds x + sublayer(x))
// HBM-bound (2 x tokens x H x 2 B).  Half a wave per token: lane l of the half owns the 16-byte chunks l, l + 32, ... of
// the row (8 bf16 each; H = 768 -> 3 per lane), so one load instruction moves 2 x 512 B.  Workgroups walk the rows with
// a grid stride and keep the NEXT row's loads in flight while the current one is reduced (two dependent half-wave
// reductions: mean, then the centred sum of squares, as BertModel computes it), gamma / beta stay in registers.
// The first version (one wave per row, 8-byte loads, one row per wave) ran at 3.65 TB/s.
template <int NC>
__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* __restrict__ in, int tokens, int H, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int l32 = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    f32x4 g[NC][2], b[NC][2];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int k0 = (l32 + 32 * j) * 8;
        if (k0 < H) {
            g[j][0] = *reinterpret_cast<const f32x4*>(gamma + k0);
            g[j][1] = *reinterpret_cast<const f32x4*>(gamma + k0 + 4);
            b[j][0] = *reinterpret_cast<const f32x4*>(beta + k0);
            b[j][1] = *reinterpret_cast<const f32x4*>(beta + k0 + 4);
        }
    }
    const float inv_h = 1.0f / (float)H;
    u32x4 nxt[NC];
    int tok = wave * 2 + half;
    if (tok < tokens) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int k0 = (l32 + 32 * j) * 8;
            if (k0 < H) nxt[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + (size_t)tok * H + k0));
        }
    }
    for (int base = wave * 2; base < tokens; base += nwaves * 2) {
        tok = base + half;
        const bool live = tok < tokens;
        u32x4 raw[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) raw[j] = nxt[j];
        const int ntok = tok + nwaves * 2;
        if (ntok < tokens) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int k0 = (l32 + 32 * j) * 8;
                if (k0 < H) nxt[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + (size_t)ntok * H + k0));
            }
        }
        float v[NC][8];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const bool on = live && (l32 + 32 * j) * 8 < H;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[j][2 * c] = on ? __builtin_bit_cast(float, raw[j][c] << 16) : 0.f;
                v[j][2 * c + 1] = on ? __builtin_bit_cast(float, raw[j][c] & 0xFFFF0000u) : 0.f;
            }
            sum += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float mean = sum * inv_h;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const bool on = (l32 + 32 * j) * 8 < H;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float d = on ? v[j][c] - mean : 0.f;
                sq = fmaf(d, d, sq);
            }
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
        const float rstd = 1.0f / sqrtf(sq * inv_h + eps);
        if (live) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int k0 = (l32 + 32 * j) * 8;
                if (k0 < H) {
                    u32x4 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float lo = (v[j][2 * c] - mean) * rstd * g[j][c >> 1][(2 * c) & 3] + b[j][c >> 1][(2 * c) & 3];
                        const float hi = (v[j][2 * c + 1] - mean) * rstd * g[j][c >> 1][(2 * c + 1) & 3] + b[j][c >> 1][(2 * c + 1) & 3];
                        r[c] = pack_bf16x2(lo, hi);
                    }
                    *reinterpret_cast<u32x4*>(out + (size_t)tok * H + k0) = r;
                }
            }
        }
    }
}

#include "attention_rect.h"  // attention_kernel, attention_long_kernel and their launch templates

// ------------------------------------------------------------------ masked mean pooling
__global__ __launch_bounds__(256) void mean_pool_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ lens, int S, int H,
                                                         int normalize, float* __restrict__ out) {
    mean_pool_rows(x, RectRows{lens, S}, blockIdx.x, H, normalize, out);
}

// ------------------------------------------------------------------ f32 -> bf16 weight conversion, fills
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = f32_to_bf16(in[i]);
}
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = bf16_to_f32(in[i]);
}
__global__ __launch_bounds__(256) void synth_scaled_kernel(float* __restrict__ out, int64_t n, uint64_t key, float scale, float offset) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = offset + scale * sc_synth_value(key, (uint64_t)i, 0u, 1u);
}

// ------------------------------------------------------------------ launchers
void sc_launch_embed_ln(const int32_t* ids, int tokens, int S, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                        const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    hipLaunchKernelGGL(embed_ln_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, s, ids, tokens, S, H, vocab, max_pos, wemb, pemb, temb,
                       g, b, eps, (bf16_t*)out);
}
void sc_launch_layernorm(const void* in, int tokens, int H, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    int blocks = (tokens + 7) / 8;  // 8 rows per workgroup per sweep
    if (blocks > 256 * 8) blocks = 256 * 8;
    const dim3 grid((unsigned)blocks), block(256);
    if (H <= 768) hipLaunchKernelGGL(layernorm_kernel<3>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, b, eps, (bf16_t*)out);
    else if (H <= 1024) hipLaunchKernelGGL(layernorm_kernel<4>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, b, eps, (bf16_t*)out);
    else hipLaunchKernelGGL(layernorm_kernel<8>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, b, eps, (bf16_t*)out);
}
bool sc_attention_supported(int S, int H, int heads, int head_dim) {
    return heads > 0 && (head_dim == 64 || head_dim == 32) && H == heads * head_dim && H % 64 == 0 && (S == 32 || S == 64 || S == 128 || S == 256 || S == 512 || S == 1024 || S == 2048);
}
// slopes: NULL = plain attention; else [heads] ALiBi slopes (device).  head_dim 32: plain only, create refuses 32-wide ALiBi models
void sc_launch_attention(const void* qkv, const int32_t* lens, int B, int S, int H, const float* slopes, void* ctx, hipStream_t s, int blocked, int head_dim) {
    if (head_dim == 32) launch_attention<Head32>(qkv, lens, B, S, H, Head32::Extra(), ctx, blocked, s);
    else if (slopes) launch_attention<Head64<true>>(qkv, lens, B, S, H, slopes, ctx, blocked, s);
    else launch_attention<Head64<false>>(qkv, lens, B, S, H, nullptr, ctx, blocked, s);
}
#include "encoder_glu.h"  // glu_kernel<ACT> and the activations
void sc_launch_geglu(const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    int64_t blocks = (tokens * (F / 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(glu_kernel<ActGelu>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)h, tokens, F, (bf16_t*)out);
}
void sc_launch_swiglu(const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    int64_t blocks = (tokens * (F / 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(glu_kernel<ActSilu>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)h, tokens, F, (bf16_t*)out);
}

// Rotary position embedding ("rotate-half", GPT-NeoX) of Q and K in place on the blocked QKV buffer [blocks][M][64] bf16 the QKV
// projections write: a (head, token) vector is 128 contiguous bytes.  HBM-bound (read + write of 2/3 of QKV).  A lane owns columns
// c .. c + 7 and c + 32 .. c + 39 of one row (two 16-byte loads), so both members of every rotated pair (j, j + 32) sit in its
// registers; 4 lanes per row, 16 rows per wave.  cos / sin [>= S][32] f32 (sc_encoder_create); position = row & (S - 1), S a power
// of two, so that padding rows (>= the real tokens, content irrelevant) stay inside the table.  f32 math, one rounding back to bf16.
__global__ __launch_bounds__(256) void rope_qk_kernel(bf16_t* __restrict__ qkv, int64_t M, int nblocks, int smask, const float* __restrict__ cos_t,
                                                       const float* __restrict__ sin_t) {
    rope_qk_rows(qkv, M, nblocks, PosMasked{smask}, cos_t, sin_t);
}
void sc_launch_rope_qk(void* qkv, int64_t M, int nblocks, int S, const float* cos_t, const float* sin_t, hipStream_t s) {
    int64_t blocks = ((int64_t)nblocks * M * 4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(rope_qk_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)qkv, M, nblocks, S - 1, cos_t, sin_t);
}
// Unnormalised pooling with more parallelism than one workgroup per chunk (which ran at 1.3 TB/s): a workgroup owns 256
// columns of one chunk, thread (cc, rg) sums the rows rg, rg + 8, ... of 8 columns with 16-byte loads, LDS combines the 8 row groups
// in a fixed order.
__global__ __launch_bounds__(256) void mean_pool_sliced_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ lens, int S, int H,
                                                                float* __restrict__ out) {
    mean_pool_sliced_rows(x, RectRows{lens, S}, blockIdx.y, blockIdx.x, H, out);
}

void sc_launch_mean_pool(const void* x, const int32_t* lens, int B, int S, int H, int normalize, float* out, hipStream_t s) {
    if (!normalize && (H % 8) == 0)
        hipLaunchKernelGGL(mean_pool_sliced_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)B), dim3(256), 0, s, (const bf16_t*)x, lens, S, H, out);
    else
        hipLaunchKernelGGL(mean_pool_kernel, dim3((unsigned)B), dim3(256), 0, s, (const bf16_t*)x, lens, S, H, normalize, out);
}
void sc_launch_embed_raw(const int32_t* ids, int tokens, int tokens_pad, int S, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                         const float* temb, void* out, float* stats, int slots, hipStream_t s) {
    hipLaunchKernelGGL(embed_raw_kernel, dim3((unsigned)((tokens_pad + 3) / 4)), dim3(256), 0, s, ids, tokens, tokens_pad, S, H, vocab, max_pos, wemb, pemb, temb,
                       (bf16_t*)out, stats, slots);
}
void sc_launch_fold_ln_weights(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, void* Wf, float* c1, float* c2,
                               hipStream_t s) {
    hipLaunchKernelGGL(fold_ln_weights_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, W, gamma, beta, bias, N, K, (bf16_t*)Wf, c1, c2);
}
void sc_launch_add_vectors(const float* a, const float* b, float* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(add_vectors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, out, n);
}
void sc_launch_mean_pool_ln(const void* y, const float* stats, int slots, int tokens_pad, const float* gamma, const float* beta, float eps,
                            const int32_t* lens, int B, int S, int H, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mean_pool_ln_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)B), dim3(256), 0, s, (const bf16_t*)y, stats, slots, tokens_pad, gamma,
                       beta, eps, lens, S, H, out);
}
void sc_launch_f32_to_bf16(const float* in, void* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, (bf16_t*)out, n);
}
void sc_launch_bf16_to_f32(const void* in, float* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)in, out, n);
}
void sc_launch_synth_scaled(float* out, int64_t n, uint64_t seed, float scale, float offset, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(synth_scaled_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, n, sc_synth_key(seed), scale, offset);
}
