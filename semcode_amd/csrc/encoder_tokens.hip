// encoder_tokens.hip -- late interaction (ColBERT) on device (gfx950): one vector per token instead of one pooled row per text, and the
// MaxSim score of (query, document) pairs over those vectors (sc_encoder_set_token_head / sc_encoder_embed_tokens / sc_encoder_score_late).
//
// Replaces (reference): nothing -- the reference reranks with nothing and embeds one vector per chunk; late-interaction libraries run
// the projection as a torch Linear and MaxSim as a padded einsum + max + sum on whatever device torch has.
//
// Roofline: token_head is a [rows, H] x [H, W] bf16 GEMM with W <= 128: 2 rows H W FLOP against rows (2 H + 4 W) bytes -- at H = 768,
// W = 128 that is 96 FLOP per byte, memory-bound on the activations it reads once; the weight (<= 512 KiB) stays in L2.  maxsim is f32
// MFMA: 2 nq nd W FLOP per pair against nd W 4 bytes of document vectors, which the nq / 16 query tiles re-read from L2.
//
// token_head_kernel<NT>  one wave per 16 packed token rows, four waves per workgroup, NT = W / 16 column tiles.  dst [rows] maps a packed
//                        row to its compact output row (-1: an alignment row of a document, the tail -- computed if it shares a wave
//                        with a wanted row, never stored; a wave without a wanted row leaves).  Lane (r16, g) loads the 16-byte piece
//                        k = 32 s + 8 g .. + 7 of token row r16 (B operand) and of weight row 16 n + r16 (A operand) straight from
//                        global memory; v_mfma_f32_16x16x32_bf16 accumulates s ascending, one chain per column tile, f32.  The lane then
//                        holds out[row r16][16 n + 4 g + c], c < 4.  |v|^2: per lane over (n, c) as (v0^2 + v1^2) + (v2^2 + v3^2) added in
//                        ascending n, then the four k groups of a row by the xor butterfly 16, 32 (both lanes of a step add the same two
//                        values: every lane of a row ends with the same bits).  scale = 1 / max(sqrt(|v|^2), 1e-12), the pooling
//                        kernels' rule; one 16-byte store per tile.  A column of the MFMA depends on no other column: a row's vector
//                        is the same bits whatever rows stand next to it.  No LDS, no atomics.
// token_head_bf16_kernel<NT>  the same up to the scale; writes the vectors as bf16 (late_round_bf16 of each f32 component, 8-byte stores) so
//                        that sc_encoder_embed_tokens_into can aim it at the tail of an index's bf16 token pool.
// maxsim_kernel          one workgroup (4 waves) per pair.  Wave w takes the document tiles w, w + 4, ... of 16 tokens; the query tiles of
//                        16 are the outer loop.  Per tile pair one v_mfma_f32_16x16x4_f32 chain over W / 4 steps fed as mmr_gram_kernel
//                        feeds it -- lane (r16, g) supplies floats 16 t + 4 g + c of document token 16 dt + r16 (A) and of query token
//                        16 qt + r16 (B), c outer, g inner -- the canonical chain of maxsim_rule.h.  The lane holds
//                        dot(Q[16 qt + r16], D[16 dt + 4 g + c]); tokens at or beyond nd (their loads are clamped to the last token) and
//                        tokens with keep = 0 are left out; the others raise the lane's running maximum, an order-preserving key.  After
//                        the wave's tiles the four k groups are combined by the xor butterfly 16, 32 (integer max), the four waves through
//                        the LDS, and lane 0 adds m_t in ascending t with __fadd_rn.  Integer maxima: no order matters.  No atomics.
// Registers and scratch: at the launchers.
#include "encoder_ops.h"
#include "late_rule.h"

template <int NT>
__global__ __launch_bounds__(256) void token_head_kernel(const bf16_t* __restrict__ x, int rows, int H, const bf16_t* __restrict__ w, const int32_t* __restrict__ dst,
                                                          float* __restrict__ out) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int r0 = 16 * (blockIdx.x * 4 + (threadIdx.x >> 6));
    if (r0 >= rows) return;  // (wave-uniform; rows is a multiple of 32)
    const int row = r0 + r16;
    const int d = dst[row];
    if (!__any(d >= 0)) return;
    const bf16_t* xr = x + (size_t)row * H + 8 * g;
    const bf16_t* wr = w + (size_t)r16 * H + 8 * g;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = H >> 5;
    for (int s = 0; s < steps; ++s) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(xr + 32 * s);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(wr + (size_t)(16 * n) * H + 32 * s);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[n], 0, 0, 0);
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) ss += (acc[n][0] * acc[n][0] + acc[n][1] * acc[n][1]) + (acc[n][2] * acc[n][2] + acc[n][3] * acc[n][3]);
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    const float scale = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    if (d < 0) return;
    float* o = out + (size_t)d * (16 * NT) + 4 * g;
#pragma unroll
    for (int n = 0; n < NT; ++n) *reinterpret_cast<f32x4*>(o + 16 * n) = f32x4{acc[n][0] * scale, acc[n][1] * scale, acc[n][2] * scale, acc[n][3] * scale};
}

// The sibling of token_head_kernel that writes into a bf16 token pool (sc_encoder_embed_tokens_into at fmt 1; that kernel is untouched, as
// late_rerank_kernel leaves maxsim_kernel): the same loads, the same MFMA chains, the same |v|^2 and scale in f32; then each of the lane's
// four consecutive columns rounded once by late_round_bf16 -- what sc_index_put_tokens does to the f32 vector on the host, so the stored
// bits are the same -- and one 8-byte store per column tile where the f32 form stores 16.
template <int NT>
__global__ __launch_bounds__(256) void token_head_bf16_kernel(const bf16_t* __restrict__ x, int rows, int H, const bf16_t* __restrict__ w, const int32_t* __restrict__ dst,
                                                               uint16_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
    const int r0 = 16 * (blockIdx.x * 4 + (threadIdx.x >> 6));
    if (r0 >= rows) return;  // (wave-uniform; rows is a multiple of 32)
    const int row = r0 + r16;
    const int d = dst[row];
    if (!__any(d >= 0)) return;
    const bf16_t* xr = x + (size_t)row * H + 8 * g;
    const bf16_t* wr = w + (size_t)r16 * H + 8 * g;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps = H >> 5;
    for (int s = 0; s < steps; ++s) {
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(xr + 32 * s);
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(wr + (size_t)(16 * n) * H + 32 * s);
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[n], 0, 0, 0);
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) ss += (acc[n][0] * acc[n][0] + acc[n][1] * acc[n][1]) + (acc[n][2] * acc[n][2] + acc[n][3] * acc[n][3]);
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    const float scale = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    if (d < 0) return;
    uint16_t* o = out + (size_t)d * (16 * NT) + 4 * g;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const uint32_t h0 = late_round_bf16(acc[n][0] * scale), h1 = late_round_bf16(acc[n][1] * scale);
        const uint32_t h2 = late_round_bf16(acc[n][2] * scale), h3 = late_round_bf16(acc[n][3] * scale);
        *reinterpret_cast<uint2*>(o + 16 * n) = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
    }
}

__global__ __launch_bounds__(256) void maxsim_kernel(const float* __restrict__ Q, const int32_t* __restrict__ q_off, const float* __restrict__ D,
                                                      const int32_t* __restrict__ d_off, const uint8_t* __restrict__ keep, const int32_t* __restrict__ pair_q,
                                                      const int32_t* __restrict__ pair_d, int W, float* __restrict__ out) {
    __shared__ uint32_t s_key[4][MAXSIM_MAX_NQ];
    __shared__ float s_m[MAXSIM_MAX_NQ];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int p = blockIdx.x;
    const int qi = pair_q[p], di = pair_d[p];
    const int q0 = q_off[qi], d0 = d_off[di];
    int nq = q_off[qi + 1] - q0;
    const int nd = d_off[di + 1] - d0;
    if (nq > MAXSIM_MAX_NQ) nq = MAXSIM_MAX_NQ;  // (the host refuses longer queries)
    const float* Qp = Q + (size_t)q0 * W;
    const float* Dp = D + (size_t)d0 * W;
    const uint8_t* kp = keep ? keep + d0 : nullptr;
    const int nqt = (nq + 15) >> 4, ndt = (nd + 15) >> 4, steps = W >> 4;

    for (int qt = 0; qt < nqt; ++qt) {
        const int tq = min(16 * qt + r16, nq - 1);  // (columns at or beyond nq repeat the last token and are never read)
        const f32x4* __restrict__ xb = reinterpret_cast<const f32x4*>(Qp + (size_t)tq * W) + g;
        uint32_t best = MAXSIM_KEY_NONE;
        for (int dt = wv; dt < ndt; dt += 4) {
            const int td = min(16 * dt + r16, nd - 1);
            const f32x4* __restrict__ xa = reinterpret_cast<const f32x4*>(Dp + (size_t)td * W) + g;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < steps; ++t) {
                const f32x4 a = xa[4 * t], b = xb[4 * t];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc, 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = 16 * dt + 4 * g + c;
                const bool ok = j < nd && (!kp || kp[min(j, nd - 1)] != 0);
                if (ok) best = maxsim_key_max(best, maxsim_key(acc[c]));
            }
        }
        best = maxsim_key_max(best, (uint32_t)__shfl_xor((int)best, 16));
        best = maxsim_key_max(best, (uint32_t)__shfl_xor((int)best, 32));
        if (g == 0) s_key[wv][16 * qt + r16] = best;
    }
    __syncthreads();
    if (tid < nq) s_m[tid] = maxsim_unkey(maxsim_key_max(maxsim_key_max(s_key[0][tid], s_key[1][tid]), maxsim_key_max(s_key[2][tid], s_key[3][tid])));
    __syncthreads();
    if (tid == 0) {
        float acc = 0.0f;
        for (int t = 0; t < nq; ++t) acc = maxsim_add(acc, s_m[t]);
        out[p] = acc;
    }
}

bool sc_token_head_supported(int H, int W) { return maxsim_width_ok(W) && H >= 32 && (H % 32) == 0; }

// Registers / scratch (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): profiles/late_kernels.log; the bf16 sibling and the
// comparison of the f32 instantiations with their earlier text: profiles/late_ingest_kernels.log
void sc_launch_token_head(const void* x, int rows, int H, const void* w, int W, const int32_t* dst, void* out, int fmt, hipStream_t s) {
    if (rows < 1 || !sc_token_head_supported(H, W) || (fmt != 0 && fmt != 1)) return;  // (the host checks these before it plans a call)
    const dim3 grid((unsigned)((rows + 63) / 64)), block(256);
    const bf16_t* xp = (const bf16_t*)x;
    const bf16_t* wp = (const bf16_t*)w;
    switch (W / 16) {
#define TOKEN_HEAD_CASE(NT)                                                                                                       \
    case NT:                                                                                                                      \
        if (fmt == 0) hipLaunchKernelGGL((token_head_kernel<NT>), grid, block, 0, s, xp, rows, H, wp, dst, (float*)out);          \
        else hipLaunchKernelGGL((token_head_bf16_kernel<NT>), grid, block, 0, s, xp, rows, H, wp, dst, (uint16_t*)out);           \
        break;
        TOKEN_HEAD_CASE(1) TOKEN_HEAD_CASE(2) TOKEN_HEAD_CASE(3) TOKEN_HEAD_CASE(4) TOKEN_HEAD_CASE(5) TOKEN_HEAD_CASE(6) TOKEN_HEAD_CASE(7) TOKEN_HEAD_CASE(8)
#undef TOKEN_HEAD_CASE
    }
}

void sc_launch_maxsim(const float* Q, const int32_t* q_off, const float* D, const int32_t* d_off, const uint8_t* keep, const int32_t* pair_q, const int32_t* pair_d,
                      int P, int W, float* out, hipStream_t s) {
    if (P < 1 || !maxsim_width_ok(W)) return;
    hipLaunchKernelGGL(maxsim_kernel, dim3((unsigned)P), dim3(256), 0, s, Q, q_off, D, d_off, keep, pair_q, pair_d, W, out);
}
