// encoder_glu.h -- the gate kernel between the two FFN GEMMs as a template on the activation.  Included by encoder_ops.hip (GEGLU, SwiGLU)
// and by encoder_t5.hip (the tanh-GELU gate of T5 v1.1).
#pragma once
#include "gemm_tile.h"

// Gated feed-forward: out[m][j] = act(h[m][j]) * h[m][F + j], h = [tokens, 2F] bf16 -> out [tokens, F] bf16.
// GEGLU (jina-bert-v2 GLUMLP): act = erf-GELU.  SwiGLU (nomic-bert): act = silu(g) = g / (1 + exp(-g)) on the hardware exp2 / rcp
// (v_exp_f32, v_rcp_f32: 1 ulp each, in front of a bf16 rounding); exp(-g) overflows to +inf for g < -88.7 and g * rcp(inf) is a
// signed zero -- the limit of silu there -- never NaN.
struct ActGelu {
    static __device__ __forceinline__ f32x2 apply(f32x2 g) { return gelu_erf_fast2(g); }
};
struct ActSilu {
    static __device__ __forceinline__ float one(float g) {
        return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.44269504088896340736f));
    }
    static __device__ __forceinline__ f32x2 apply(f32x2 g) { return f32x2{one(g[0]), one(g[1])}; }
};
// tanh-GELU ("gelu_new", T5 v1.1): 0.5 g (1 + tanh(u)), u = sqrt(2/pi) (g + 0.044715 g^3), computed as g / (1 + exp(-2u)) on the hardware
// exp2 / rcp as ActSilu is; exp(-2u) overflows to +inf for very negative g and g * rcp(inf) is a signed zero -- the limit there -- never NaN.
struct ActGeluTanh {
    static __device__ __forceinline__ float one(float g) {
        const float u = 0.7978845608028654f * (g + 0.044715f * g * g * g);
        return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * (-2.0f * 1.44269504088896340736f)));
    }
    static __device__ __forceinline__ f32x2 apply(f32x2 g) { return f32x2{one(g[0]), one(g[1])}; }
};
template <class ACT>
__global__ __launch_bounds__(256) void glu_kernel(const bf16_t* __restrict__ h, int64_t tokens, int F, bf16_t* __restrict__ out) {
    const int64_t total = tokens * (int64_t)(F / 8);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / (F / 8);
        const int j = (int)(i - m * (F / 8)) * 8;
        const bf16x8 g = *reinterpret_cast<const bf16x8*>(h + m * 2 * F + j);
        const bf16x8 u = *reinterpret_cast<const bf16x8*>(h + m * 2 * F + F + j);
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x2 gg = ACT::apply(f32x2{bf16_to_f32((bf16_t)g[2 * c]), bf16_to_f32((bf16_t)g[2 * c + 1])});
            o[c] = pack_bf16x2(gg[0] * bf16_to_f32((bf16_t)u[2 * c]), gg[1] * bf16_to_f32((bf16_t)u[2 * c + 1]));
        }
        *reinterpret_cast<u32x4*>(out + m * F + j) = o;
    }
}
