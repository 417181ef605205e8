// encoder_proj.hip -- the output projection behind the pooling of an embedding model (gfx950): CodeT5+'s proj (768 -> 256, with bias), the
// Dense module of sentence-T5 / GTR (768 -> 768, no bias).  sc_encoder_set_output_proj installs it; every embedding entry point then
// returns out = W pooled + b, L2-normalised when cfg.normalize says so, instead of the pooled row.
//
//   output_proj_kernel  f32 MFMA : x [B,H] f32 (the UN-normalised pooled rows) -> out [B,E] f32.  One workgroup per 16 rows, as
//                                  pair_head_kernel: the rows wait in LDS, wave w computes the 16-column blocks w, w + 4, ... of the output
//                                  on v_mfma_f32_16x16x4_f32 with W streamed from memory, two accumulators over alternating 16-wide stages of
//                                  K added at the end, + bias, stored.  With normalize, behind a barrier (the workgroup sees its own
//                                  stores), wave w takes rows 4w .. 4w + 3 of the block again: sum of squares lane-strided, then the fixed
//                                  shuffle tree, scale in place by 1 / max(|x|, 1e-12) -- the rule of the pooling kernels.
// The order of every sum depends on (H, E) only, never on B or on the row's place in its block of 16: a text's vector is the same bits
// whichever batch-mates it has.
#include "encoder_ops.h"
#include "encoder_rows.h"  // wave_sum
#include "gemm_tile.h"

#define OUT_PROJ_PAD 4  // floats between two rows in the LDS
__global__ __launch_bounds__(256) void output_proj_kernel(const float* __restrict__ x, int B, int H, const float* __restrict__ W, const float* __restrict__ bias, int E,
                                                           int normalize, float* out) {  // (out is read back: no __restrict__)
    extern __shared__ __attribute__((aligned(16))) float rows[];  // [16][H + OUT_PROJ_PAD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int ld = H + OUT_PROJ_PAD, h4 = H >> 2;
    for (int i = tid; i < 16 * h4; i += 256) {
        const int r = i / h4, c4 = i - r * h4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};  // rows beyond B: zero rows, computed and never stored
        if (b0 + r < B) v = *reinterpret_cast<const f32x4*>(x + (size_t)(b0 + r) * H + 4 * c4);
        *reinterpret_cast<f32x4*>(rows + r * ld + 4 * c4) = v;
    }
    __syncthreads();
    const float* xrow = rows + r16 * ld + 4 * g;
    const int stages = H >> 4;
    for (int n0 = 16 * w; n0 < E; n0 += 64) {  // wave-uniform
        const float* wrow = W + (size_t)(n0 + r16) * H + 4 * g;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        auto stage = [&](int st, f32x4& acc) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(wrow + 16 * st);
            const f32x4 v = *reinterpret_cast<const f32x4*>(xrow + 16 * st);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], v[c], acc, 0, 0, 0);
        };
        for (int st = 0; st + 1 < stages; st += 2) {
            stage(st, acc0);
            stage(st + 1, acc1);
        }
        if (stages & 1) stage(stages - 1, acc0);
        f32x4 d = acc0 + acc1;  // lane holds output n = n0 + 4 g + c of row r16
        if (bias) d += *reinterpret_cast<const f32x4*>(bias + n0 + 4 * g);
        if (b0 + r16 < B) *reinterpret_cast<f32x4*>(out + (size_t)(b0 + r16) * E + n0 + 4 * g) = d;
    }
    if (!normalize) return;  // (uniform over the grid)
    __syncthreads();  // the workgroup's own stores are visible to it: its 16 rows are complete
    for (int r = 4 * w; r < 4 * w + 4; ++r) {  // wave-uniform
        if (b0 + r >= B) break;
        float* o = out + (size_t)(b0 + r) * E;
        float ss = 0.f;
        for (int n = lane; n < E; n += 64) ss = fmaf(o[n], o[n], ss);
        const float scale = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
        for (int n = lane; n < E; n += 64) o[n] *= scale;
    }
}

bool sc_output_proj_supported(int H, int E) { return H >= 16 && (H % 16) == 0 && H <= 2048 && E >= 16 && (E % 16) == 0 && E <= 2048; }
void sc_launch_output_proj(const float* x, int B, int H, const float* W, const float* bias, int E, int normalize, float* out, hipStream_t s) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(output_proj_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (2048 + OUT_PROJ_PAD) * 4);
    });
    const int ld = H + OUT_PROJ_PAD;
    hipLaunchKernelGGL(output_proj_kernel, dim3((unsigned)((B + 15) / 16)), dim3(256), (size_t)16 * ld * 4, s, x, B, H, W, bias, E, normalize, out);
}
