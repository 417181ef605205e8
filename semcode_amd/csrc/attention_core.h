// attention_core.h -- the device code the attention kernels share (encoder_ops.hip: rectangles, encoder_packed.hip: packed
// variable-length rows): the online-softmax state of one 32-row query block, the fold of one segment of keys into it, the store.
// LDS images: K [keys][64] with chunk ^= (row>>1)&7, V [keys][64] with chunk ^= ((row>>1)&1)<<2 (encoder_ops.hip describes them).
#pragma once
#include "gemm_tile.h"  // bf16 helpers, vector types

typedef short s16x4 __attribute__((ext_vector_type(4)));

// The online-softmax state of one 32-row query block: running maximum, running denominator, unnormalised output.  A sequence
// longer than the 512 keys whose K and V fit the LDS is attended segment by segment (attention_long_kernel): the state is
// carried from one segment of keys to the next.
struct AttnState {
    float m_run, l_run;
    f32x16 o0, o1;
};
static __device__ __forceinline__ void attn_state_init(AttnState& a) {
    a.m_run = -3.0e38f;
    a.l_run = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a.o0[r] = 0.f; a.o1[r] = 0.f; }
}
// One segment of keys (the KT tiles in Kl / Vl = keys key0 .. key0 + 32 KT of the sequence; len / nkt count inside the segment)
// folded into the state.  first: the state is fresh (no rescale of O before the first group).
template <int KT, bool FULL, bool ALIBI, int GKMAX = 4>
static __device__ __forceinline__ void attention_qblock_core(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, int len, int nkt, int lane,
                                                             int qbase, float slope2, AttnState& S_, bool first, int key0) {
    constexpr int GK = KT < GKMAX ? KT : GKMAX;   // key tiles per group
    constexpr int NG = (KT + GK - 1) / GK;
    const int l31 = lane & 31, hh = lane >> 5;
    const float sl2 = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) * log2(e)
    const int tail = len & 31;                           // != 0: the last real key tile is partially masked
    float m_run = S_.m_run, l_run = S_.l_run;
    f32x16 o0 = S_.o0, o1 = S_.o1;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (!FULL && g * GK >= nkt) continue;  // wave-uniform: nothing real in this group
        // S^T tiles of the group: st[i][r] = score(key = 32 t + (r&3) + 8 (r>>2) + 4 hh, query = l31), t = g*GK + i
        f32x16 st[GK];
#pragma unroll
        for (int i = 0; i < GK; ++i) {
            const int t = g * GK + i;
            if (FULL || t < nkt) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                const int krow = 32 * t + l31;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int c = 2 * ks + hh;
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kl + krow * 128 + ((c ^ ((krow >> 1) & 7)) << 4));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
                }
                if (ALIBI) {  // work in the exp2 domain from here on: v = s * sl2 - slope2 * |q - key|
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float dist = (float)(key0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh - (qbase + l31));
                        acc[r] = fmaf(acc[r], sl2, -slope2 * fabsf(dist));
                    }
                }
                st[i] = acc;
            }
        }
        const float sc2 = ALIBI ? 1.0f : sl2;  // scores already scaled when ALIBI
        float mx = m_run;
#pragma unroll
        for (int i = 0; i < GK; ++i) {
            const int t = g * GK + i;
            if (FULL || t < nkt) {
                if (!FULL && t == nkt - 1 && tail) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh < len) mx = fmaxf(mx, st[i][r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[i][r]);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mb = mx * sc2;
        const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, sc2, -mb));  // first group: exp2(-huge) = 0, and O, l are 0 anyway
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < GK; ++i) {
            const int t = g * GK + i;
            if (FULL || t < nkt) {
                const bool masked = !FULL && (t == nkt - 1) && tail;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float p = __builtin_amdgcn_exp2f(fmaf(st[i][r], sc2, -mb));
                    if (masked && !(32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh < len)) p = 0.f;
                    st[i][r] = p;
                    sum += p;
                }
            }
        }
        sum += __shfl_xor(sum, 32, 64);
        l_run = fmaf(l_run, alpha, sum);
        m_run = mx;
        if (g > 0 || !first) {  // rescale O: its rows are queries (r&3) + 8 (r>>2) + 4 hh, alpha lives on lane q -> exchange through LDS
            xch[l31] = alpha;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 al = *reinterpret_cast<const f32x4*>(xch + 8 * g4 + 4 * hh);
#pragma unroll
                for (int c = 0; c < 4; ++c) { o0[4 * g4 + c] *= al[c]; o1[4 * g4 + c] *= al[c]; }
            }
        }
        // O += P V: A operand = P straight from the score registers (k order of step s:
        // key = 32 t + 16 s + 8 (j>>2) + 4 hh + (j&3)), B operand = V by transposed LDS reads
#pragma unroll
        for (int i = 0; i < GK; ++i) {
            const int t = g * GK + i;
            if (FULL || t < nkt) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                    u32x4 pp;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pp[j] = pack_bf16x2(st[i][8 * s + 2 * j], st[i][8 * s + 2 * j + 1]);
                    const bf16x8 pf = __builtin_bit_cast(bf16x8, pp);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        bf16x8 vf;
#pragma unroll
                        for (int piece = 0; piece < 2; ++piece) {
                            const int row = 32 * t + 16 * s + 8 * piece + 4 * hh + ((lane & 15) >> 2);
                            const int d0 = 32 * dt + 16 * ((lane >> 4) & 1);
                            const int chunk = (d0 >> 3) + ((lane & 3) >> 1);
                            const int sw = chunk ^ (((row >> 1) & 1) << 2);
                            typedef __attribute__((address_space(3))) s16x4* lds_s16x4p;
                            const s16x4 got = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(Vl + row * 128 + sw * 16 + 8 * (lane & 1)));
                            vf[4 * piece + 0] = got[0];
                            vf[4 * piece + 1] = got[1];
                            vf[4 * piece + 2] = got[2];
                            vf[4 * piece + 3] = got[3];
                        }
                        if (dt == 0) o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, o0, 0, 0, 0);
                        else o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, o1, 0, 0, 0);
                    }
                }
            }
        }
    }
    S_.m_run = m_run;
    S_.l_run = l_run;
    S_.o0 = o0;
    S_.o1 = o1;
}
// o[r] = O[q = (r&3) + 8 (r>>2) + 4 hh][d = 32 dt + l31]: normalise by 1/l[q], stage as bf16 [q][d] in LDS 8 query rows
// at a time (1 KiB, wave-private; LDS runs a wave's instructions in order), then leave as whole 128-byte rows.
static __device__ __forceinline__ void attn_state_store(const AttnState& S_, float* xch, char* ostg, bf16_t* obase, int H, int lane) {
    const int l31 = lane & 31, hh = lane >> 5;
    const float l_run = S_.l_run;
    const f32x16 o0 = S_.o0, o1 = S_.o1;
    xch[l31] = 1.0f / l_run;
    bf16_t* og = reinterpret_cast<bf16_t*>(ostg);
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 il = *reinterpret_cast<const f32x4*>(xch + 8 * g4 + 4 * hh);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ql = 4 * hh + c;  // row inside this block of 8
            og[ql * 64 + l31] = (bf16_t)(pack_bf16x2(o0[4 * g4 + c] * il[c], 0.f) & 0xFFFFu);
            og[ql * 64 + 32 + l31] = (bf16_t)(pack_bf16x2(o1[4 * g4 + c] * il[c], 0.f) & 0xFFFFu);
        }
        const int ql = lane >> 3, c8 = lane & 7;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(ostg + ql * 128 + c8 * 16);
        *reinterpret_cast<bf16x8*>(obase + (size_t)(8 * g4 + ql) * H + c8 * 8) = v;
    }
}
