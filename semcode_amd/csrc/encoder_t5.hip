// encoder_t5.hip -- what the T5 encoder (cfg.arch 3) adds to the device code, in a translation unit of its own (gfx950): the rectangle and
// packed attention kernels instantiated on Head64Rel (the bucketed relative position bias as a table of the distance, attention_core.h),
// the tanh-GELU gate and the ReLU pass of its two feed-forwards.  Nothing here is launched by another model, and the code objects of
// encoder_ops.hip and encoder_packed.hip hold what they held before this family.
#include "attention_packed.h"
#include "attention_rect.h"
#include "encoder_glu.h"
#include "encoder_ops.h"

// the bucketed relative bias of T5 (cfg.pos_type 3): tbl [H / 64][2 span - 1] f32 (device), the distance table sc_rel_bias_table builds
void sc_launch_attention_rel(const void* qkv, const int32_t* lens, int B, int S, int H, const float* tbl, int span, void* ctx, hipStream_t s, int blocked) {
    launch_attention<Head64Rel>(qkv, lens, B, S, H, RelBias{tbl, span}, ctx, blocked, s);
}
void sc_launch_attention_rel_packed(const void* qkv, const int32_t* items, const int* nitems, int H, const float* tbl, int span, void* ctx, hipStream_t s, int blocked) {
    launch_attention_packed<Head64Rel>(qkv, items, nitems, H, RelBias{tbl, span}, ctx, blocked, s);
}
void sc_launch_geglu_tanh(const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    int64_t blocks = (tokens * (F / 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(glu_kernel<ActGeluTanh>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)h, tokens, F, (bf16_t*)out);
}
// ReLU of the Linear-ReLU-Linear feed-forward (cfg.ffn_type 3, T5 v1.0), in place on the FFN1 output h [n] bf16, n a multiple of 8: the sign
// bit of each half word decides, no arithmetic (-0 and negative NaN become +0).  A stand-alone pass, not an FFN1 epilogue: the GEMM
// instantiations stay as they are; it reads and writes tokens * F * 2 bytes once per layer.
__global__ __launch_bounds__(256) void relu_kernel(bf16_t* __restrict__ h, int64_t n8) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        u32x4 v = *reinterpret_cast<const u32x4*>(h + i * 8);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (v[c] & 0x8000u ? 0u : v[c] & 0xFFFFu) | (v[c] & 0x80000000u ? 0u : v[c] & 0xFFFF0000u);
        *reinterpret_cast<u32x4*>(h + i * 8) = v;
    }
}
void sc_launch_relu(void* h, int64_t n, hipStream_t s) {
    int64_t blocks = (n / 8 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)h, n / 8);
}
