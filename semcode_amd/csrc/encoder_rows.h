// encoder_rows.h -- the device bodies of the encoder kernels that know where a sequence's rows lie: embedding (both forms), rotary
// rotation, mean pooling (three forms).  One copy each; a kernel passes in HOW a row finds its position (POS) or a sequence its rows
// (ROWS): encoder_ops.hip for [B, S] rectangles, encoder_packed.hip for packed variable-length rows.  The kernels' own comments
// (encoder_ops.hip) describe the arithmetic.
#pragma once
#include "gemm_tile.h"  // bf16 helpers, vector types

static __device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

#define LN_MAXJ 8  // hidden <= 2048

// position of token row r: rectangles -- r % S (embedding) or r & (S - 1) (rotary, S a power of two); packed rows -- a per-row array,
// clamped into the model's table
struct PosInRect {
    int S;
    __device__ __forceinline__ int operator()(int r) const { return r % S; }
};
struct PosMasked {
    int smask;
    __device__ __forceinline__ int operator()(int64_t r) const { return (int)(r & smask); }
};
struct PosArray {
    const int32_t* pos;
    int max_pos;
    __device__ __forceinline__ int operator()(int64_t r) const {
        const int p = pos[r];
        return p >= max_pos ? max_pos - 1 : p;
    }
};
// type_emb row of token row r: TypeZero -- row 0 (every embedding model); TypeArray -- a per-row segment id, clamped into the table
// (encoder_pairs.hip: the two halves of a cross-encoder's pair)
struct TypeZero {
    __device__ __forceinline__ int operator()(int64_t) const { return 0; }
};
struct TypeArray {
    const int32_t* types;
    int type_vocab;
    __device__ __forceinline__ int operator()(int64_t r) const {
        const int t = types[r];
        return t < 0 ? 0 : (t >= type_vocab ? type_vocab - 1 : t);
    }
};
// the rows of sequence b: rectangles -- b * S .., lens clamped to 1 .. S; packed -- starts[b] ..
struct RectRows {
    const int32_t* lens;
    int S;
    __device__ __forceinline__ int len(int b) const {
        const int l = lens[b];
        return l < 1 ? 1 : (l > S ? S : l);
    }
    __device__ __forceinline__ size_t first(int b) const { return (size_t)b * S; }
};
struct PackedRows {
    const int32_t *starts, *lens;
    __device__ __forceinline__ int len(int b) const {
        const int l = lens[b];
        return l < 1 ? 1 : l;
    }
    __device__ __forceinline__ size_t first(int b) const { return (size_t)starts[b]; }
};

template <class POS, class TYPE = TypeZero>
static __device__ __forceinline__ void embed_ln_rows(const int32_t* __restrict__ ids, int tokens, POS pos_of, int H, int vocab, int max_pos,
                                                     const float* __restrict__ wemb, const float* __restrict__ pemb, const float* __restrict__ temb,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps, bf16_t* __restrict__ out,
                                                     TYPE type_of = TYPE()) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= tokens) return;
    int id = ids[tok];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int pos = pos_of(tok);
    pos = pos >= max_pos ? max_pos - 1 : pos;
    const float* we = wemb + (size_t)id * H;
    const float* pe = pemb ? pemb + (size_t)pos * H : nullptr;  // NULL: no position table (ALiBi models)
    const float* te = temb + (size_t)type_of(tok) * H;
    f32x4 v[LN_MAXJ];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (k0 < H) {
            v[j] = *reinterpret_cast<const f32x4*>(we + k0);
            if (pe) v[j] += *reinterpret_cast<const f32x4*>(pe + k0);
            v[j] += *reinterpret_cast<const f32x4*>(te + k0);
            sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    const float mean = wave_sum(sum) / (float)H;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (k0 < H) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float d = v[j][c] - mean;
                sq = fmaf(d, d, sq);
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)H + eps);
    bf16_t* o = out + (size_t)tok * H;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (k0 < H) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + k0);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + k0);
            u16x4 r;
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = f32_to_bf16((v[j][c] - mean) * rstd * g[c] + b[c]);
            *reinterpret_cast<u16x4*>(o + k0) = r;
        }
    }
}

template <class POS, class TYPE = TypeZero>
static __device__ __forceinline__ void embed_raw_rows(const int32_t* __restrict__ ids, int tokens, int tokens_pad, POS pos_of, int H, int vocab, int max_pos,
                                                      const float* __restrict__ wemb, const float* __restrict__ pemb, const float* __restrict__ temb,
                                                      bf16_t* __restrict__ out, float* __restrict__ stats, int slots, TYPE type_of = TYPE()) {
    const int lane = threadIdx.x & 63;
    const int tok = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= tokens_pad) return;
    float s1 = 0.f, s2 = 0.f;
    if (tok < tokens) {
        int id = ids[tok];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        int pos = pos_of(tok);
        pos = pos >= max_pos ? max_pos - 1 : pos;
        const float* we = wemb + (size_t)id * H;
        const float* pe = pemb ? pemb + (size_t)pos * H : nullptr;
        const float* te = temb + (size_t)type_of(tok) * H;
        bf16_t* o = out + (size_t)tok * H;
#pragma unroll
        for (int j = 0; j < LN_MAXJ; ++j) {
            const int k0 = 4 * lane + 256 * j;
            if (k0 < H) {
                f32x4 v = *reinterpret_cast<const f32x4*>(we + k0);
                if (pe) v += *reinterpret_cast<const f32x4*>(pe + k0);
                v += *reinterpret_cast<const f32x4*>(te + k0);
                u16x4 r;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    r[c] = f32_to_bf16(v[c]);
                    const float y = bf16_to_f32(r[c]);
                    s1 += y;
                    s2 = fmaf(y, y, s2);
                }
                *reinterpret_cast<u16x4*>(o + k0) = r;
            }
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
    } else {
        // padding rows (tokens .. tokens_pad, never read by attention or pooling): zeros with statistics (0, 0), so that whatever the
        // row-independent GEMMs compute for them stays finite (mu 0, rs 1/sqrt(eps), times zero)
        for (int k0 = 4 * lane; k0 < H; k0 += 256) *reinterpret_cast<u16x4*>(out + (size_t)tok * H + k0) = u16x4{0, 0, 0, 0};
    }
    if (lane < slots) {
        float* p = stats + ((size_t)lane * tokens_pad + tok) * 2;
        p[0] = lane == 0 ? s1 : 0.f;
        p[1] = lane == 0 ? s2 : 0.f;
    }
}

template <class POS>
static __device__ __forceinline__ void rope_qk_rows(bf16_t* __restrict__ qkv, int64_t M, int nblocks, POS pos_of, const float* __restrict__ cos_t,
                                                    const float* __restrict__ sin_t) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int64_t total = (int64_t)nblocks * M * 4;  // (block, row, quarter)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t vec = i >> 2;            // block * M + row
        const int c = (int)(i & 3) * 8;
        const int p = pos_of(vec % M);
        bf16_t* v = qkv + vec * 64 + c;
        const u32x4 lo = *reinterpret_cast<const u32x4*>(v), hi = *reinterpret_cast<const u32x4*>(v + 32);
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cos_t + p * 32 + c), c1 = *reinterpret_cast<const f32x4*>(cos_t + p * 32 + c + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sin_t + p * 32 + c), s1 = *reinterpret_cast<const f32x4*>(sin_t + p * 32 + c + 4);
        u32x4 olo, ohi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a0 = __builtin_bit_cast(float, lo[k] << 16), a1 = __builtin_bit_cast(float, lo[k] & 0xFFFF0000u);
            const float b0 = __builtin_bit_cast(float, hi[k] << 16), b1 = __builtin_bit_cast(float, hi[k] & 0xFFFF0000u);
            const float cc0 = k < 2 ? c0[2 * k] : c1[2 * k - 4], cc1 = k < 2 ? c0[2 * k + 1] : c1[2 * k - 3];
            const float ss0 = k < 2 ? s0[2 * k] : s1[2 * k - 4], ss1 = k < 2 ? s0[2 * k + 1] : s1[2 * k - 3];
            olo[k] = pack_bf16x2(fmaf(a0, cc0, -b0 * ss0), fmaf(a1, cc1, -b1 * ss1));
            ohi[k] = pack_bf16x2(fmaf(b0, cc0, a0 * ss0), fmaf(b1, cc1, a1 * ss1));
        }
        *reinterpret_cast<u32x4*>(v) = olo;
        *reinterpret_cast<u32x4*>(v + 32) = ohi;
    }
}

template <class ROWS>
static __device__ __forceinline__ void mean_pool_ln_rows(const bf16_t* __restrict__ y, const float* __restrict__ stats, int slots, int tokens_pad,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps, ROWS rows, int b,
                                                         int colblock, int H, float* __restrict__ out) {
    __shared__ float part[8][32][9];
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int cc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int k0 = colblock * 256 + cc * 8;
    const int len = rows.len(b);
    const size_t row0 = rows.first(b);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float accmu = 0.f;
    const float inv_h = 1.0f / (float)H;
    if (k0 < H) {
        const bf16_t* p = y + row0 * H + k0;
#pragma unroll 2
        for (int s0 = rg; s0 < len; s0 += 8) {
            const size_t tok = row0 + s0;
            float s1 = 0.f, s2 = 0.f;
            for (int t = 0; t < slots; ++t) {
                s1 += stats[((size_t)t * tokens_pad + tok) * 2];
                s2 += stats[((size_t)t * tokens_pad + tok) * 2 + 1];
            }
            const float mu = s1 * inv_h;
            const float rs = 1.0f / sqrtf(fmaxf(s2 * inv_h - mu * mu, 0.f) + eps);
            const u32x4 raw = *reinterpret_cast<const u32x4*>(p + (size_t)s0 * H);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[2 * c] = fmaf(rs, __builtin_bit_cast(float, raw[c] << 16), acc[2 * c]);
                acc[2 * c + 1] = fmaf(rs, __builtin_bit_cast(float, raw[c] & 0xFFFF0000u), acc[2 * c + 1]);
            }
            accmu = fmaf(rs, mu, accmu);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) part[rg][cc][c] = acc[c];
    part[rg][cc][8] = accmu;
    __syncthreads();
    if (rg == 0 && k0 < H) {
        const float inv = 1.0f / (float)len;
        float m = part[0][cc][8];
#pragma unroll
        for (int g = 1; g < 8; ++g) m += part[g][cc][8];
        float o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float t = part[0][cc][c];
#pragma unroll
            for (int g = 1; g < 8; ++g) t += part[g][cc][c];
            o[c] = fmaf((t - m) * inv, gamma[k0 + c], beta[k0 + c]);
        }
        *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0) = f32x4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0 + 4) = f32x4{o[4], o[5], o[6], o[7]};
    }
}

template <class ROWS>
static __device__ __forceinline__ void mean_pool_rows(const bf16_t* __restrict__ x, ROWS rows, int b, int H, int normalize, float* __restrict__ out) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int len = rows.len(b);
    const float inv = 1.0f / (float)len;
    float ss = 0.f;
    for (int k0 = 4 * tid; k0 < H; k0 += 1024) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const bf16_t* p = x + rows.first(b) * H + k0;
        for (int s = 0; s < len; ++s) {
            const u16x4 raw = *reinterpret_cast<const u16x4*>(p + (size_t)s * H);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] += bf16_to_f32(raw[c]);
        }
        acc *= inv;
        *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0) = acc;
        ss += (acc[0] * acc[0] + acc[1] * acc[1]) + (acc[2] * acc[2] + acc[3] * acc[3]);
    }
    if (normalize) {
        red[tid] = ss;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        const float scale = 1.0f / fmaxf(sqrtf(red[0]), 1e-12f);
        for (int k0 = 4 * tid; k0 < H; k0 += 1024) {
            f32x4 v = *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0);
            v *= scale;
            *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0) = v;
        }
    }
}

template <class ROWS>
static __device__ __forceinline__ void mean_pool_sliced_rows(const bf16_t* __restrict__ x, ROWS rows, int b, int colblock, int H, float* __restrict__ out) {
    __shared__ float part[8][32][8];
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int cc = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int k0 = colblock * 256 + cc * 8;
    const int len = rows.len(b);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k0 < H) {
        const bf16_t* p = x + rows.first(b) * H + k0;
#pragma unroll 4
        for (int s0 = rg; s0 < len; s0 += 8) {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(p + (size_t)s0 * H);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[2 * c] += __builtin_bit_cast(float, raw[c] << 16);
                acc[2 * c + 1] += __builtin_bit_cast(float, raw[c] & 0xFFFF0000u);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) part[rg][cc][c] = acc[c];
    __syncthreads();
    if (rg == 0 && k0 < H) {
        const float inv = 1.0f / (float)len;
        f32x4 lo, hi;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float t = part[0][cc][c];
#pragma unroll
            for (int g = 1; g < 8; ++g) t += part[g][cc][c];
            if (c < 4) lo[c] = t * inv;
            else hi[c - 4] = t * inv;
        }
        *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0) = lo;
        *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0 + 4) = hi;
    }
}
