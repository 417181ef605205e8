// encoder_packed.hip -- the position-aware kernels of the encoder forward on PACKED variable-length rows (gfx950).
//
// A packed batch holds its sequences one after another: sequence i owns the token rows [starts[i], starts[i] + ceil32(lens[i])),
// the total is rounded up to the 256 rows of a GEMM tile (sc_encoder.cpp plans the layout on the host).  The GEMMs, the LayerNorm
// kernel and the gate kernels treat every row alike and run unchanged; only four steps know where a sequence begins:
//
//   embed_*_packed_kernel       position from a per-row array instead of token % S
//   rope_qk_packed_kernel       likewise
//   attention_packed_kernel     one workgroup per (sequence, group of query blocks) x 64-column block (a head of 64, a pair of heads
//                               of 32), read from a table of work items
//   mean_pool_*_packed_kernel   rows starts[b] .. starts[b] + lens[b] instead of b * S ..
//
// Each shares its device body with the rectangle kernel of encoder_ops.hip (encoder_rows.h, attention_core.h): same arithmetic,
// same reduction orders (relative to the start of the sequence), same statistics conventions.  Alignment rows (lens[i] .. ceil32(lens[i]) of a sequence) carry token 0:
// they are embedded, attended as queries (their keys are masked) and never pooled; the tail rows up to the 256-row multiple are
// zero rows with zero statistics, as the padding rows of a rectangle are.
#include "attention_core.h"
#include "encoder_ops.h"
#include "encoder_rows.h"
#include "gemm_tile.h"

// ------------------------------------------------------------------ embeddings, rotary positions
// The bodies are encoder_rows.h's, shared with the rectangle kernels; here a row's position comes from pos[row] (clamped into the
// model's table) instead of row % S.  Statistics conventions of embed_raw_kernel: slot 0 holds the sums of the rounded row, the tail
// rows tokens .. tokens_pad are zero rows with statistics (0, 0).
__global__ __launch_bounds__(256) void embed_ln_packed_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos, int tokens, int H, int vocab,
                                                               int max_pos, const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                               const float* __restrict__ temb, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    embed_ln_rows(ids, tokens, PosArray{pos, max_pos}, H, vocab, max_pos, wemb, pemb, temb, gamma, beta, eps, out);
}
__global__ __launch_bounds__(256) void embed_raw_packed_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos, int tokens, int tokens_pad,
                                                                int H, int vocab, int max_pos, const float* __restrict__ wemb,
                                                                const float* __restrict__ pemb, const float* __restrict__ temb,
                                                                bf16_t* __restrict__ out, float* __restrict__ stats, int slots) {
    embed_raw_rows(ids, tokens, tokens_pad, PosArray{pos, max_pos}, H, vocab, max_pos, wemb, pemb, temb, out, stats, slots);
}
__global__ __launch_bounds__(256) void rope_qk_packed_kernel(bf16_t* __restrict__ qkv, int64_t M, int nblocks, const int32_t* __restrict__ pos, int max_pos,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t) {
    rope_qk_rows(qkv, M, nblocks, PosArray{pos, max_pos}, cos_t, sin_t);
}

#include "attention_packed.h"  // attention_packed_kernel and its launch template

// ------------------------------------------------------------------ masked mean pooling
// encoder_rows.h's bodies over the rows starts[b] .. starts[b] + lens[b]; blockIdx.x = sequence (up to 65 536 of them), blockIdx.y =
// the 256-column block of the two sliced forms
__global__ __launch_bounds__(256) void mean_pool_packed_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ starts, const int32_t* __restrict__ lens,
                                                                int H, int normalize, float* __restrict__ out) {
    mean_pool_rows(x, PackedRows{starts, lens}, blockIdx.x, H, normalize, out);
}
__global__ __launch_bounds__(256) void mean_pool_sliced_packed_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ starts,
                                                                       const int32_t* __restrict__ lens, int H, float* __restrict__ out) {
    mean_pool_sliced_rows(x, PackedRows{starts, lens}, blockIdx.x, blockIdx.y, H, out);
}
__global__ __launch_bounds__(256) void mean_pool_ln_packed_kernel(const bf16_t* __restrict__ y, const float* __restrict__ stats, int slots, int tokens_pad,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                   const int32_t* __restrict__ starts, const int32_t* __restrict__ lens, int H,
                                                                   float* __restrict__ out) {
    mean_pool_ln_rows(y, stats, slots, tokens_pad, gamma, beta, eps, PackedRows{starts, lens}, blockIdx.x, blockIdx.y, H, out);
}

// ------------------------------------------------------------------ launchers
void sc_launch_embed_ln_packed(const int32_t* ids, const int32_t* pos, int tokens, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                               const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    hipLaunchKernelGGL(embed_ln_packed_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, s, ids, pos, tokens, H, vocab, max_pos, wemb, pemb, temb, g, b,
                       eps, (bf16_t*)out);
}
void sc_launch_embed_raw_packed(const int32_t* ids, const int32_t* pos, int tokens, int tokens_pad, int H, int vocab, int max_pos, const float* wemb,
                                const float* pemb, const float* temb, void* out, float* stats, int slots, hipStream_t s) {
    hipLaunchKernelGGL(embed_raw_packed_kernel, dim3((unsigned)((tokens_pad + 3) / 4)), dim3(256), 0, s, ids, pos, tokens, tokens_pad, H, vocab, max_pos, wemb,
                       pemb, temb, (bf16_t*)out, stats, slots);
}
void sc_launch_rope_qk_packed(void* qkv, int64_t M, int nblocks, const int32_t* pos, int max_pos, const float* cos_t, const float* sin_t, hipStream_t s) {
    int64_t blocks = ((int64_t)nblocks * M * 4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(rope_qk_packed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)qkv, M, nblocks, pos, max_pos, cos_t, sin_t);
}
int sc_packed_attention_class(int len) { return len > 256 ? 0 : (len > 128 ? 1 : 2); }
void sc_launch_attention_packed(const void* qkv, const int32_t* items, const int* nitems, int H, const float* slopes, void* ctx, hipStream_t s, int blocked,
                                int head_dim) {
    if (head_dim == 32) launch_attention_packed<Head32>(qkv, items, nitems, H, Head32::Extra(), ctx, blocked, s);
    else if (slopes) launch_attention_packed<Head64<true>>(qkv, items, nitems, H, slopes, ctx, blocked, s);
    else launch_attention_packed<Head64<false>>(qkv, items, nitems, H, nullptr, ctx, blocked, s);
}
void sc_launch_mean_pool_packed(const void* x, const int32_t* starts, const int32_t* lens, int B, int H, int normalize, float* out, hipStream_t s) {
    if (!normalize && (H % 8) == 0)
        hipLaunchKernelGGL(mean_pool_sliced_packed_kernel, dim3((unsigned)B, (unsigned)((H + 255) / 256)), dim3(256), 0, s, (const bf16_t*)x, starts, lens, H, out);
    else
        hipLaunchKernelGGL(mean_pool_packed_kernel, dim3((unsigned)B), dim3(256), 0, s, (const bf16_t*)x, starts, lens, H, normalize, out);
}
void sc_launch_mean_pool_ln_packed(const void* y, const float* stats, int slots, int tokens_pad, const float* gamma, const float* beta, float eps,
                                   const int32_t* starts, const int32_t* lens, int B, int H, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mean_pool_ln_packed_kernel, dim3((unsigned)B, (unsigned)((H + 255) / 256)), dim3(256), 0, s, (const bf16_t*)y, stats, slots, tokens_pad,
                       gamma, beta, eps, starts, lens, H, out);
}
