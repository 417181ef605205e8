// encoder_cls.hip -- [CLS] pooling (sc_encoder_set_pooling 1: bge, arctic-embed, mxbai, gte) and the last layer on the [CLS] rows only.
//
// Replaces (reference): llama.cpp's LLAMA_POOLING_TYPE_CLS behind LlamaCppEmbeddings (src/semcode/embeddings/providers.py:69-100): the
// embedding of a text is the last hidden state of its first token, not the masked mean.
//
//   cls_rows_kernel       1 wave / text : the text's first row (i * S, or starts[i]), optionally LayerNorm'ed in f32 (the folded pipeline
//                                         keeps raw rows) and L2-normalised by the rule of mean_pool_rows -> f32 [B, H] (cls_pool) or
//                                         bf16 [Mc, H] (cls_gather: the residual rows of the pruned last layer)
//   attention_cls_kernel  HBM-bound     : 1 workgroup / (text, 64-column block).  One query row -- the text's first -- against the text's
//                                         `len` keys: softmax(q K^T / sqrt(hd) - slope_h * j) V.  K and V of the block are streamed once in
//                                         16-byte loads (8 lanes a row, 32 rows a pass), scores and probabilities stay f32 in the LDS, every
//                                         reduction runs in a fixed order inside the workgroup: a text's result does not depend on its
//                                         batch-mates.  A block holds one head of 64 or a pair of heads of 32.
#include "encoder_ops.h"
#include "encoder_rows.h"  // wave_sum, RectRows / PackedRows, LN_MAXJ

// ------------------------------------------------------------------ the [CLS] row of every text
// gamma != NULL: the row is raw, LayerNorm (two-pass, biased variance, eps inside the root: BertModel's) comes first.
template <class ROWS, bool OUT_BF16>
static __device__ __forceinline__ void cls_rows(const bf16_t* __restrict__ x, ROWS rows, int B, int H, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float eps, int normalize, void* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bf16_t* p = x + rows.first(b) * H;
    float v[LN_MAXJ][4];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[j][c] = 0.f;
        if (k0 < H) {
            const u16x4 raw = *reinterpret_cast<const u16x4*>(p + k0);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[j][c] = bf16_to_f32(raw[c]);
            sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    if (gamma) {
        const float mean = wave_sum(sum) / (float)H;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) {
            if (4 * lane + 256 * j < H) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = v[j][c] - mean;
                    sq = fmaf(d, d, sq);
                }
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)H + eps);
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) {
            const int k0 = 4 * lane + 256 * j;
            if (k0 < H) {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[j][c] = (v[j][c] - mean) * rstd * gamma[k0 + c] + beta[k0 + c];
            }
        }
    }
    if (normalize) {
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) ss += (v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3]);
        const float scale = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[j][c] = v[j][c] * scale;
        }
    }
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (k0 < H) {
            if (OUT_BF16) {
                u16x4 r;
#pragma unroll
                for (int c = 0; c < 4; ++c) r[c] = f32_to_bf16(v[j][c]);
                *reinterpret_cast<u16x4*>((bf16_t*)out + (size_t)b * H + k0) = r;
            } else {
                *reinterpret_cast<f32x4*>((float*)out + (size_t)b * H + k0) = f32x4{v[j][0], v[j][1], v[j][2], v[j][3]};
            }
        }
    }
}
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void cls_rows_kernel(const bf16_t* __restrict__ x, int S, int B, int H, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, int normalize, void* __restrict__ out) {
    cls_rows<RectRows, OUT_BF16>(x, RectRows{nullptr, S}, B, H, gamma, beta, eps, normalize, out);
}
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void cls_rows_packed_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ starts, int B, int H,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int normalize,
                                                               void* __restrict__ out) {
    cls_rows<PackedRows, OUT_BF16>(x, PackedRows{starts, nullptr}, B, H, gamma, beta, eps, normalize, out);
}

void sc_launch_cls_pool(const void* x, const int32_t* starts, int B, int S, int H, const float* gamma, const float* beta, float eps, int normalize, float* out,
                        hipStream_t s) {
    const dim3 grid((unsigned)((B + 3) / 4));
    if (starts) hipLaunchKernelGGL(cls_rows_packed_kernel<false>, grid, dim3(256), 0, s, (const bf16_t*)x, starts, B, H, gamma, beta, eps, normalize, (void*)out);
    else hipLaunchKernelGGL(cls_rows_kernel<false>, grid, dim3(256), 0, s, (const bf16_t*)x, S, B, H, gamma, beta, eps, normalize, (void*)out);
}

void sc_launch_cls_gather(const void* x, const int32_t* starts, int B, int S, int H, const float* gamma, const float* beta, float eps, void* out, int rows_pad,
                          hipStream_t s) {
    if (rows_pad > B) hipMemsetAsync((char*)out + (size_t)B * H * 2, 0, (size_t)(rows_pad - B) * H * 2, s);  // rows B .. rows_pad: zeros
    const dim3 grid((unsigned)((B + 3) / 4));
    if (starts) hipLaunchKernelGGL(cls_rows_packed_kernel<true>, grid, dim3(256), 0, s, (const bf16_t*)x, starts, B, H, gamma, beta, eps, 0, out);
    else hipLaunchKernelGGL(cls_rows_kernel<true>, grid, dim3(256), 0, s, (const bf16_t*)x, S, B, H, gamma, beta, eps, 0, out);
}

// ------------------------------------------------------------------ attention of the [CLS] query
// qkv in 64-column blocks [3 * H / 64][M][64] (SC_LDC_BLOCKED64): blockIdx.y = the Q block, its K block lies H / 64 blocks further,
// its V block 2 * H / 64.  Thread t of a pass owns the 16-byte chunk t & 7 of key row t >> 3 (+ 32 per pass).
#define CLS_MAX_KEYS 2048
template <int HD, class ROWS>
static __device__ __forceinline__ void attention_cls(const bf16_t* __restrict__ qkv, ROWS rows, int M, int H, const float* __restrict__ slopes,
                                                     bf16_t* __restrict__ ctx) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int NH = 64 / HD;  // heads in the block
    __shared__ float sc[NH][CLS_MAX_KEYS];
    __shared__ float red[4][NH];
    __shared__ float part[32][64];
    const int tid = threadIdx.x, cc = tid & 7, rg = tid >> 3, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, blk = blockIdx.y, nblk = H / 64;
    int len = rows.len(b);
    len = len > CLS_MAX_KEYS ? CLS_MAX_KEYS : len;
    const size_t row0 = rows.first(b);
    const int hh = cc / (HD / 8);  // the head (of the block) this thread's chunk belongs to
    float q[8];
    {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(qkv + ((size_t)blk * M + row0) * 64 + cc * 8);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            q[2 * c] = __builtin_bit_cast(float, raw[c] << 16);
            q[2 * c + 1] = __builtin_bit_cast(float, raw[c] & 0xFFFF0000u);
        }
    }
    const float scale = HD == 64 ? 0.125f : 0.17677669529663687f;  // 1 / sqrt(HD)
    const float slope = slopes ? slopes[blk * NH + hh] : 0.f;
    const bf16_t* kp = qkv + ((size_t)(nblk + blk) * M + row0) * 64 + cc * 8;
    const bf16_t* vp = qkv + ((size_t)(2 * nblk + blk) * M + row0) * 64 + cc * 8;
    // scores: the 8 (heads of 64) or 4 (heads of 32) lanes of a key row add their partial dot products in a butterfly
    float mx = -3.0e38f;
    for (int j0 = 0; j0 < len; j0 += 32) {
        const int j = j0 + rg;
        float d = 0.f;
        if (j < len) {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(kp + (size_t)j * 64);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d = fmaf(q[2 * c], __builtin_bit_cast(float, raw[c] << 16), d);
                d = fmaf(q[2 * c + 1], __builtin_bit_cast(float, raw[c] & 0xFFFF0000u), d);
            }
        }
#pragma unroll
        for (int off = 1; off < HD / 8; off <<= 1) d += __shfl_xor(d, off, 64);
        if (j < len) {
            const float v = fmaf(d, scale, -slope * (float)j);
            if ((cc & (HD / 8 - 1)) == 0) sc[hh][j] = v;
            mx = fmaxf(mx, v);
        }
    }
    // the maximum of each head: over the wave's 8 row groups (the lanes of a row and head hold the same value), then over the four waves
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane < 8 && (lane & (HD / 8 - 1)) == 0) red[wave][lane / (HD / 8)] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][hh], red[1][hh]), fmaxf(red[2][hh], red[3][hh]));
    // P V, unnormalised: p_j = exp(s_j - max); the row group's sum of p and its 8 columns of sum p_j V_j
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float psum = 0.f;
    for (int j = rg; j < len; j += 32) {
        const float pj = __expf(sc[hh][j] - mx);
        const u32x4 raw = *reinterpret_cast<const u32x4*>(vp + (size_t)j * 64);
        psum += pj;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc[2 * c] = fmaf(pj, __builtin_bit_cast(float, raw[c] << 16), acc[2 * c]);
            acc[2 * c + 1] = fmaf(pj, __builtin_bit_cast(float, raw[c] & 0xFFFF0000u), acc[2 * c + 1]);
        }
    }
    __syncthreads();  // the scores are spent: their memory takes the row groups' sums of p, [32][NH]
    float* psums = &sc[0][0];
#pragma unroll
    for (int c = 0; c < 8; ++c) part[rg][cc * 8 + c] = acc[c];
    if ((cc & (HD / 8 - 1)) == 0) psums[rg * NH + hh] = psum;
    __syncthreads();
    if (tid < 64) {
        const int h = tid / HD;
        float den = 0.f, num = 0.f;
        for (int g = 0; g < 32; ++g) {
            den += psums[g * NH + h];
            num += part[g][tid];
        }
        ctx[(size_t)b * H + blk * 64 + tid] = f32_to_bf16(num / den);
    }
}
template <int HD>
__global__ __launch_bounds__(256) void attention_cls_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int S, int M, int H,
                                                             const float* __restrict__ slopes, bf16_t* __restrict__ ctx) {
    attention_cls<HD>(qkv, RectRows{lens, S}, M, H, slopes, ctx);
}
template <int HD>
__global__ __launch_bounds__(256) void attention_cls_packed_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ starts,
                                                                    const int32_t* __restrict__ lens, int M, int H, const float* __restrict__ slopes,
                                                                    bf16_t* __restrict__ ctx) {
    attention_cls<HD>(qkv, PackedRows{starts, lens}, M, H, slopes, ctx);
}

// starts NULL: a [B, S] rectangle (lens clamped to 1 .. S), else packed rows.  M: the rows of a qkv block.  ctx [rows_pad, H] bf16 row-major, rows
// B .. rows_pad zeroed.
void sc_launch_attention_cls(const void* qkv, const int32_t* starts, const int32_t* lens, int B, int S, int M, int H, int head_dim, const float* slopes, void* ctx,
                             int rows_pad, hipStream_t s) {
    if (rows_pad > B) hipMemsetAsync((char*)ctx + (size_t)B * H * 2, 0, (size_t)(rows_pad - B) * H * 2, s);
    const dim3 grid((unsigned)B, (unsigned)(H / 64));
    const bf16_t* q = (const bf16_t*)qkv;
    bf16_t* o = (bf16_t*)ctx;
    if (starts && head_dim == 32) hipLaunchKernelGGL(attention_cls_packed_kernel<32>, grid, dim3(256), 0, s, q, starts, lens, M, H, slopes, o);
    else if (starts) hipLaunchKernelGGL(attention_cls_packed_kernel<64>, grid, dim3(256), 0, s, q, starts, lens, M, H, slopes, o);
    else if (head_dim == 32) hipLaunchKernelGGL(attention_cls_kernel<32>, grid, dim3(256), 0, s, q, lens, S, M, H, slopes, o);
    else hipLaunchKernelGGL(attention_cls_kernel<64>, grid, dim3(256), 0, s, q, lens, S, M, H, slopes, o);
}
