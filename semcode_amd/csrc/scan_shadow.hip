// scan_shadow.hip -- the bf16 / int8 shadow copies of corpus rows and query batches that the coarse stages of the batched
// scan multiply (scan_batched.h), with the rounding residuals the certificate's error bound is made of (gfx950).
//
// Roofline: HBM (one pass over the f32 rows).
#include <algorithm>

#include "sc_common.h"

// ------------------------------------------------------------------ bf16 shadow + max norm + max rounding residual
// One wave per row: Xb = bf16(X); res_bits = max over rows of |x - bf16(x)|^2 (the certificate's error bound uses the
// actual rounding residual, by Cauchy-Schwarz |<x,q> - <xb,qb>| <= |x - xb| |q| + |xb| |q - qb|).
__global__ __launch_bounds__(256) void shadow_kernel(const float* __restrict__ X, const float* __restrict__ xnorm, int64_t first, int64_t n, int ld,
                                                      bf16_t* __restrict__ Xb, unsigned* __restrict__ res_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    float worst = 0.f, worst_rel = 0.f;
    for (int64_t r = wave0; r < n; r += nwaves) {
        const float* x = X + (first + r) * (int64_t)ld;
        bf16_t* o = Xb + (first + r) * (int64_t)ld;
        float res = 0.f;
        for (int k0 = 4 * lane; k0 < ld; k0 += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + k0);
            u16x4 b;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                b[c] = f32_to_bf16(v[c]);
                const float d = v[c] - bf16_to_f32(b[c]);
                res = fmaf(d, d, res);
            }
            *reinterpret_cast<u16x4*>(o + k0) = b;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) res += __shfl_xor(res, off, 64);
        worst = fmaxf(worst, res);
        const float xn = xnorm[first + r];
        if (xn > 0.f) worst_rel = fmaxf(worst_rel, res / xn);
    }
    if (lane == 0 && worst > 0.f) {
        atomicMax(res_bits, __builtin_bit_cast(unsigned, worst * 1.0001f));          // max |x - xb|^2
        atomicMax(res_bits + 1, __builtin_bit_cast(unsigned, worst_rel * 1.0001f));  // max |x - xb|^2 / |x|^2
    }
}
__global__ __launch_bounds__(256) void norm_max_kernel(const float* __restrict__ xnorm, int64_t n, unsigned* __restrict__ out_bits) {
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, xnorm[i]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out_bits, __builtin_bit_cast(unsigned, m));  // non-negative floats order like their bits
}
// f32 padded queries [Q, ld] -> bf16 [Qpad, ld] (rows >= Q zero) and qres[q] = |q - bf16(q)|^2 ; one wave per query row
__global__ __launch_bounds__(256) void query_bf16_kernel(const float* __restrict__ Qp, int Q, int Qpad, int ld, bf16_t* __restrict__ Qb,
                                                          float* __restrict__ qres) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Qpad) return;
    float res = 0.f;
    for (int k0 = 4 * lane; k0 < ld; k0 += 256) {
        u16x4 b = {0, 0, 0, 0};
        if (q < Q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(Qp + (size_t)q * ld + k0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                b[c] = f32_to_bf16(v[c]);
                const float d = v[c] - bf16_to_f32(b[c]);
                res = fmaf(d, d, res);
            }
        }
        *reinterpret_cast<u16x4*>(Qb + (size_t)q * ld + k0) = b;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) res += __shfl_xor(res, off, 64);
    if (lane == 0 && q < Q) qres[q] = res * 1.0001f;
}

// int8 shadow: one wave per row.  Xq [rows][ld8] int8 (ld8 = ld rounded up to 128, zero padded), xscale[row] = s_r,
// res_bits[1] / [2] = max |x - s q|^2 and max |x - s q|^2 / |x|^2 over the rows (the certificate's bound).
template <bool QUERY>
__global__ __launch_bounds__(256) void shadow8_kernel(const float* __restrict__ X, const float* __restrict__ xnorm, int64_t first, int64_t n, int64_t nout,
                                                       int ld, int ld8, int8_t* __restrict__ Xq, float* __restrict__ xscale,
                                                       unsigned* __restrict__ res_bits, float* __restrict__ qres,
                                                       const unsigned* __restrict__ common_absmax_bits) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    float worst = 0.f, worst_rel = 0.f;
    for (int64_t r = wave0; r < nout; r += nwaves) {  // QUERY: rows n .. nout are padding (zeros, scale 1)
        const bool real = r < n;
        const float* x = X + (first + r) * (int64_t)ld;
        float m = 0.f;
        if (real)
            for (int k0 = 4 * lane; k0 < ld; k0 += 256) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + k0);
                m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
            }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (QUERY) m = __builtin_bit_cast(float, *common_absmax_bits);  // queries: ONE scale for the batch (the epilogue's prefilter relies on it)
        const float sc = m > 0.f ? m * (1.0f / 127.0f) : 1.0f;
        const float inv = 1.0f / sc;
        float res = 0.f;
        int8_t* o = Xq + (first + r) * (int64_t)ld8;
        for (int k0 = 16 * lane; k0 < ld8; k0 += 1024) {
            u32x4 packed = {0u, 0u, 0u, 0u};
            if (real && k0 < ld) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(x + k0 + 4 * j);
                    uint32_t word = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float qf = fminf(fmaxf(rintf(v[c] * inv), -127.0f), 127.0f);
                        const float d = fmaf(-sc, qf, v[c]);
                        res = fmaf(d, d, res);
                        word |= ((uint32_t)(int)qf & 0xFFu) << (8 * c);
                    }
                    packed[j] = word;
                }
            }
            *reinterpret_cast<u32x4*>(o + k0) = packed;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) res += __shfl_xor(res, off, 64);
        if (lane == 0) xscale[first + r] = sc;
        if (QUERY) {
            if (lane == 0 && real) qres[r] = res * 1.0001f;
        } else {
            worst = fmaxf(worst, res);
            const float xn = xnorm[first + r];
            if (xn > 0.f) worst_rel = fmaxf(worst_rel, res / xn);
        }
    }
    if (!QUERY && lane == 0 && worst > 0.f) {
        atomicMax(res_bits, __builtin_bit_cast(unsigned, worst * 1.0001f));
        atomicMax(res_bits + 1, __builtin_bit_cast(unsigned, worst_rel * 1.0001f));
    }
}

// max |q_i| over the whole query batch (non-negative floats order like their bits)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ Qp, int64_t n, unsigned* __restrict__ out_bits) {
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(Qp[i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out_bits, __builtin_bit_cast(unsigned, m));
}

// ------------------------------------------------------------------ launchers
void sc_launch_shadow(const float* X, const float* xnorm, int64_t first, int64_t n, int ld, void* Xb, unsigned* res_bits, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(shadow_kernel, dim3((unsigned)blocks), dim3(256), 0, s, X, xnorm, first, n, ld, (bf16_t*)Xb, res_bits);
}
void sc_launch_shadow8(const float* X, const float* xnorm, int64_t first, int64_t n, int ld, int ld8, void* Xq, float* xscale, unsigned* res_bits,
                       hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(shadow8_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, X, xnorm, first, n, n, ld, ld8, (int8_t*)Xq, xscale, res_bits, (float*)nullptr,
                       (const unsigned*)nullptr);
}
void sc_launch_norm_max(const float* xnorm, int64_t n, unsigned* out_bits, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(norm_max_kernel, dim3((unsigned)blocks), dim3(256), 0, s, xnorm, n, out_bits);
}
void sc_launch_query_bf16(const float* Qp, int Q, int Qpad, int ld, void* Qb, float* qres, hipStream_t s) {
    hipLaunchKernelGGL(query_bf16_kernel, dim3((unsigned)((Qpad + 3) / 4)), dim3(256), 0, s, Qp, Q, Qpad, ld, (bf16_t*)Qb, qres);
}
// f32 padded queries [Q, ld] -> int8 [Qpad, ld8] (rows >= Q zero) with ONE scale s = max |q_i| / 127 for the whole batch
// (qscale [Qpad] all equal), qres[q] = |q - s q_q|^2; absmax_bits: 4 bytes of device scratch
void sc_launch_query_i8(const float* Qp, int Q, int Qpad, int ld, int ld8, void* Qq, float* qscale, float* qres, unsigned* absmax_bits, hipStream_t s) {
    hipMemsetAsync(absmax_bits, 0, 4, s);
    const int64_t n = (int64_t)Q * ld;
    hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, s, Qp, n, absmax_bits);
    hipLaunchKernelGGL(shadow8_kernel<true>, dim3((unsigned)((Qpad + 3) / 4)), dim3(256), 0, s, Qp, (const float*)nullptr, (int64_t)0, (int64_t)Q, (int64_t)Qpad, ld,
                       ld8, (int8_t*)Qq, qscale, (unsigned*)nullptr, qres, (const unsigned*)absmax_bits);
}
