// attention_core.h -- what the attention kernels share (encoder_ops.hip: rectangles, encoder_packed.hip: packed variable-length
// rows, encoder_window.hip: local attention, encoder_causal.hip: causal grouped-query attention).
//   the math   : the online-softmax state of one 32-row query block, the fold of one segment of keys into it, the store
//                (AttnState / attention_qblock_core / attn_state_store), the band fold of local attention (attention_qblock_window),
//                the causal fold for heads of 64 and of 128 (AttnStateCausal<NB> / attention_qblock_causal<NB, KT>, NB blocks of 64
//                columns a head; at 128 K and V are two 64-wide images each)
//   head width : Head64<ALIBI>, Head64Rel (a table of the distance: T5) and Head32 name state, init, fold and store of a width and its
//                additive bias; the kernels are templates on one of them.
//                Head dimension 32: the LDS images hold a PAIR of heads, AttnState32 / attention_qblock_core32 / attn_state32_store
//                run the softmax once per head of the pair
//   the shell  : what a kernel does around the math (LDS carve-up, operand addressing, the two staging loops, the Q load, wait +
//                barrier) stays written out in each kernel: moved into shared functions, each of those steps changed the compiled
//                text of the kernels that used it, and the 8-tile packed class measured slower (encoder_ops.hip).  What is
//                shared is the LDS size of a launch, attn_lds_bytes
//   launching  : attn_launch (dynamic-LDS limit once per instantiation and device), attn_packed_classes (the three launch classes)
// LDS images: K [keys][64] with chunk ^= (row>>1)&7, V [keys][64] with chunk ^= ((row>>1)&1)<<2 (encoder_ops.hip describes them).
#pragma once
#include <type_traits>  // std::integral_constant (attn_packed_classes)

#include "gemm_tile.h"   // bf16 helpers, vector types, LDS-DMA pointer types
#include "sc_common.h"   // ScDeviceOnce (attn_launch)

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
// BIAS: 0 plain scores q.k / 8; 1 ALiBi, q.k / 8 - slope |query - key|; 2 a table of the distance (Head64Rel below): q.k + tbw[key - query],
// NO 1/sqrt(d), tbw = the LDS image of the head's distance table, placed so that the score of the segment's key kr and this block's query
// l31 reads tbw[kr - l31].  The bias is what the score accumulator STARTS from -- the MFMAs add q.k on top in f32 -- so it costs one LDS read
// per score and no arithmetic; the scale of the exp2 domain is then the policy's own constant log2(e) where the plain arm has log2(e) / 8
template <int KT, bool FULL, int BIAS, int GKMAX = 4>
static __device__ __forceinline__ void attention_qblock_core(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, int len, int nkt, int lane,
                                                             int qbase, float slope2, AttnState& S_, bool first, int key0, const float* tbw = nullptr) {
    constexpr int GK = KT < GKMAX ? KT : GKMAX;   // key tiles per group
    constexpr int NG = (KT + GK - 1) / GK;
    const int l31 = lane & 31, hh = lane >> 5;
    const float sl2 = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) * log2(e)
    const int tail = len & 31;                           // != 0: the last real key tile is partially masked
    const float* tl = BIAS == 2 ? tbw + (4 * hh - l31) : nullptr;  // the lane's part of a bias address in ONE register; tile and r are immediates
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
                for (int r = 0; r < 16; ++r) acc[r] = BIAS == 2 ? tl[32 * t + (r & 3) + 8 * (r >> 2)] : 0.f;
                const int krow = 32 * t + l31;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    const int c = 2 * ks + hh;
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kl + krow * 128 + ((c ^ ((krow >> 1) & 7)) << 4));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
                }
                if (BIAS == 1) {  // work in the exp2 domain from here on: v = s * sl2 - slope2 * |q - key|
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float dist = (float)(key0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh - (qbase + l31));
                        acc[r] = fmaf(acc[r], sl2, -slope2 * fabsf(dist));
                    }
                }
                st[i] = acc;
            }
        }
        const float sc2 = BIAS == 2 ? 1.44269504088896340736f : BIAS == 1 ? 1.0f : sl2;  // ALiBi scores are scaled already; the table's are q.k + bias, scale 1
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

// ------------------------------------------------------------------ head dimension 32: a pair of heads per 64-column block
// The 64 columns of a staged K / V row, of a wave's four Q fragments and of an output row hold heads 2j (columns 0..31) and 2j + 1
// (columns 32..63) of block j.  The state is one (m, l, O tile) per head of the pair: 36 registers against AttnState's 34.
struct AttnState32 {
    float m_run[2], l_run[2];
    f32x16 o[2];
};
static __device__ __forceinline__ void attn_state32_init(AttnState32& a) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        a.m_run[e] = -3.0e38f;
        a.l_run[e] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) a.o[e][r] = 0.f;
    }
}
// attention_qblock_core for a pair of 32-wide heads, plain attention only.  Per group of key tiles and per head e of the pair: the
// score tile is the two MFMA steps ks = 2e, 2e + 1 (K chunks 4e + hh and 4e + 2 + hh of the row, Q fragments 2e and 2e + 1), scaled
// by 1/sqrt(32); P V accumulates into the one tile o[e] from the dt = e half of the V reads.  Nothing head e computes reads a column
// of the other head.  Same LDS addresses per read as the 64-wide core, so its bank analysis holds; masking, the FULL path and the
// fold of later segments are its too.  The two heads of a group run as a real two-trip loop over ONE copy of the code, the current
// head's (m, l, O, Q fragments) swapped with the other's after each trip: unrolled, the scheduler interleaves the two independent
// heads, keeps both score tiles live and spills (2.4 KB of scratch per lane at 16 key tiles).
template <int KT, bool FULL, int GKMAX = 4>
static __device__ __forceinline__ void attention_qblock_core32(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, int len, int nkt, int lane,
                                                               AttnState32& S_, bool first) {
    constexpr int GK = KT < GKMAX ? KT : GKMAX;   // key tiles per group
    constexpr int NG = (KT + GK - 1) / GK;
    const int l31 = lane & 31, hh = lane >> 5;
    const float sl2 = 0.17677669529663688110f * 1.44269504088896340736f;  // 1/sqrt(32) * log2(e)
    const int tail = len & 31;                                            // != 0: the last real key tile is partially masked
    float m_run = S_.m_run[0], l_run = S_.l_run[0], m_oth = S_.m_run[1], l_oth = S_.l_run[1];
    f32x16 o = S_.o[0], o_oth = S_.o[1];
    bf16x8 q0 = qf[0], q1 = qf[1], q0_oth = qf[2], q1_oth = qf[3];
    // LDS byte offsets of this lane's reads for head 0 at key tile 0; head 1 is 64 bytes (4 chunks) away in the same row, and both
    // swizzles only XOR chunk bits, so the head is one XOR with e << 6 and the key tile an immediate
    const int kb0 = l31 * 128 + ((hh ^ ((l31 >> 1) & 7)) << 4), kb1 = l31 * 128 + (((2 + hh) ^ ((l31 >> 1) & 7)) << 4);
    const int vrow = 4 * hh + ((lane & 15) >> 2);
    const int vb = vrow * 128 + (((2 * ((lane >> 4) & 1) + ((lane & 3) >> 1)) ^ (((vrow >> 1) & 1) << 2)) << 4) + 8 * (lane & 1);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (!FULL && g * GK >= nkt) continue;  // wave-uniform: nothing real in this group
#pragma unroll 1
        for (int e = 0; e < 2; ++e) {
            const int ka0 = kb0 ^ (e << 6), ka1 = kb1 ^ (e << 6), va = vb ^ (e << 6);
            // S^T tiles of the group: st[i][r] = score(key = 32 t + (r&3) + 8 (r>>2) + 4 hh, query = l31), t = g*GK + i
            f32x16 st[GK];
#pragma unroll
            for (int i = 0; i < GK; ++i) {
                const int t = g * GK + i;
                if (FULL || t < nkt) {
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {  // row 32 t + l31, chunk (4 e + 2 ks + hh) ^ ((row >> 1) & 7)
                        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kl + 32 * t * 128 + (ks ? ka1 : ka0));
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, ks ? q1 : q0, acc, 0, 0, 0);
                    }
                    st[i] = acc;
                }
            }
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
            const float mb = mx * sl2;
            const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, sl2, -mb));  // first group: exp2(-huge) = 0, and O, l are 0 anyway
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < GK; ++i) {
                const int t = g * GK + i;
                if (FULL || t < nkt) {
                    const bool masked = !FULL && (t == nkt - 1) && tail;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float p = __builtin_amdgcn_exp2f(fmaf(st[i][r], sl2, -mb));
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
                    for (int c = 0; c < 4; ++c) o[4 * g4 + c] *= al[c];
                }
            }
            // O += P V: A operand = P straight from the score registers (k order of step s:
            // key = 32 t + 16 s + 8 (j>>2) + 4 hh + (j&3)), B operand = columns 32 e .. 32 e + 31 of V by transposed LDS reads
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
                        bf16x8 vf;
#pragma unroll
                        for (int piece = 0; piece < 2; ++piece) {
                            // row 32 t + 16 s + 8 piece + vrow, chunk (4 e + 2 ((lane >> 4) & 1) + ((lane & 3) >> 1)) ^ (((row >> 1) & 1) << 2)
                            typedef __attribute__((address_space(3))) s16x4* lds_s16x4p;
                            const s16x4 got = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(Vl + (32 * t + 16 * s + 8 * piece) * 128 + va));
                            vf[4 * piece + 0] = got[0];
                            vf[4 * piece + 1] = got[1];
                            vf[4 * piece + 2] = got[2];
                            vf[4 * piece + 3] = got[3];
                        }
                        o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, o, 0, 0, 0);
                    }
                }
            }
            // the other head's turn (after two trips everything is back in place)
            { const float t = m_run; m_run = m_oth; m_oth = t; }
            { const float t = l_run; l_run = l_oth; l_oth = t; }
            { const f32x16 t = o; o = o_oth; o_oth = t; }
            { const bf16x8 t = q0; q0 = q0_oth; q0_oth = t; }
            { const bf16x8 t = q1; q1 = q1_oth; q1_oth = t; }
        }
    }
    S_.m_run[0] = m_run;
    S_.l_run[0] = l_run;
    S_.m_run[1] = m_oth;
    S_.l_run[1] = l_oth;
    S_.o[0] = o;
    S_.o[1] = o_oth;
}
// o[e][r] = O_e[q = (r&3) + 8 (r>>2) + 4 hh][d = l31]: the left half of an output row is head 2j normalised by 1/l_0[q], the right half
// head 2j + 1 by 1/l_1[q]; staged and stored as attn_state_store does (whole 128-byte rows [q][64]).
static __device__ __forceinline__ void attn_state32_store(const AttnState32& S_, float* xch, char* ostg, bf16_t* obase, int H, int lane) {
    const int l31 = lane & 31, hh = lane >> 5;
    f32x4 il[2][4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {  // LDS runs a wave's instructions in order: the second write follows the first head's reads
        xch[l31] = 1.0f / S_.l_run[e];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) il[e][g4] = *reinterpret_cast<const f32x4*>(xch + 8 * g4 + 4 * hh);
    }
    bf16_t* og = reinterpret_cast<bf16_t*>(ostg);
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ql = 4 * hh + c;  // row inside this block of 8
            og[ql * 64 + l31] = (bf16_t)(pack_bf16x2(S_.o[0][4 * g4 + c] * il[0][g4][c], 0.f) & 0xFFFFu);
            og[ql * 64 + 32 + l31] = (bf16_t)(pack_bf16x2(S_.o[1][4 * g4 + c] * il[1][g4][c], 0.f) & 0xFFFFu);
        }
        const int ql = lane >> 3, c8 = lane & 7;
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(ostg + ql * 128 + c8 * 16);
        *reinterpret_cast<bf16x8*>(obase + (size_t)(8 * g4 + ql) * H + c8 * 8) = v;
    }
}

// ------------------------------------------------------------------ windowed (band) attention, head dimension 64 (encoder_window.hip)
// A query attends to the real keys within `hw` positions of its own: |query - key| <= hw, key < len.  With hw <= 64 the band of a
// 32-row query block touches at most five 32-key tiles (blocks qb - 2 .. qb + 2), so all of them are ONE group: a single softmax pass
// with attention_qblock_core's arithmetic per (query, key) -- S^T = K Q^T on the 32x32x16 MFMA, exp2 of the scaled score against
// the row maximum, P rounded to bf16 straight from the score registers into P V -- and no rescale of O, because there is no
// second group.  ntiles (1 .. WT, wave-uniform) tiles are live; tile i holds the keys 32 (kt_first + i) .. of the sequence and
// lies in the LDS images (those of attention_qblock_core) at tile lt_first + i.  A tile the band covers completely and whose
// keys are all real skips the per-element mask (wave-uniform test).  A query without any visible key -- an alignment row beyond
// len + hw -- ends with l = 1 and O = 0: its output row is zero, never NaN.
template <int WT>
static __device__ __forceinline__ void attention_qblock_window(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, int len, int hw, int lane, int qbase,
                                                               int kt_first, int lt_first, int ntiles, AttnState& S_) {
    const int l31 = lane & 31, hh = lane >> 5;
    const float sl2 = 0.125f * 1.44269504088896340736f;  // 1/sqrt(64) * log2(e)
    const int q = qbase + l31;
    f32x16 o0 = S_.o0, o1 = S_.o1;
    f32x16 st[WT];
#pragma unroll
    for (int i = 0; i < WT; ++i) {
        if (i < ntiles) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const int krow = 32 * (lt_first + i) + l31;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int c = 2 * ks + hh;
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kl + krow * 128 + ((c ^ ((krow >> 1) & 7)) << 4));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
            st[i] = acc;
        }
    }
    // st[i][r] = score(key = 32 (kt_first + i) + (r&3) + 8 (r>>2) + 4 hh, query = q)
    float mx = -3.0e38f;
#pragma unroll
    for (int i = 0; i < WT; ++i) {
        if (i < ntiles) {
            const int k0 = 32 * (kt_first + i);
            // whole tile visible to every query of the block: |q - key| <= 32 |tile - block| + 31, and every key real
            const int dt = k0 - qbase;
            const bool whole = (dt < 0 ? -dt : dt) + 31 <= hw && k0 + 32 <= len;
            if (whole) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[i][r]);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh, d = key - q;
                    if (key < len && d <= hw && -d <= hw) mx = fmaxf(mx, st[i][r]);
                }
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mb = mx * sl2;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < WT; ++i) {
        if (i < ntiles) {
            const int k0 = 32 * (kt_first + i);
            const int dt = k0 - qbase;
            const bool whole = (dt < 0 ? -dt : dt) + 31 <= hw && k0 + 32 <= len;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = __builtin_amdgcn_exp2f(fmaf(st[i][r], sl2, -mb));
                if (!whole) {
                    const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh, d = key - q;
                    p = (key < len && d <= hw && -d <= hw) ? p : 0.f;  // a select: a masked score may have overflowed exp2
                }
                st[i][r] = p;
                sum += p;
            }
        }
    }
    sum += __shfl_xor(sum, 32, 64);
    // O += P V: operands as in attention_qblock_core
#pragma unroll
    for (int i = 0; i < WT; ++i) {
        if (i < ntiles) {
            const int t = lt_first + i;
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
    S_.m_run = mx;
    S_.l_run = sum > 0.f ? sum : 1.0f;
    S_.o0 = o0;
    S_.o1 = o1;
}

// ------------------------------------------------------------------ causal attention, head dimension 64 NB (encoder_causal.hip)
// A query attends to the real keys at or before its own position: key <= query, key < len.  One segment of keys (the KT tiles in Kl / Vl
// = keys key0 .. key0 + 32 KT of the sequence, key0 a multiple of 128) folded into the state with attention_qblock_core's arithmetic per
// (query, key); `ntiles` (0 .. KT, wave-uniform) of them are live for this query block: the tiles up to its diagonal or up to the last
// real key, whichever comes first.  Keys are folded in groups of FOUR tiles counted from key 0 whatever KT is (KT a multiple of 4), so
// the sequence of maxima, rescales and sums of a query block -- its bits -- does not depend on the segment size of the launch.  A tile
// strictly below the block's diagonal whose keys are all real skips the per-element mask (wave-uniform test); the diagonal tile masks
// key > query, the tile that holds len masks key >= len.  A group of four such whole tiles -- most groups of a long text -- runs
// as straight-line code without bounds (attention_causal_group<.., true, ..>).  Every query sees key 0, so group 0 always leaves a finite
// maximum and l > 0: nothing is ever NaN, alignment and padding rows included.
// NB: the head is NB blocks of 64 columns wide (1 or 2).  At NB 2 K and V of a segment lie in LDS as TWO of the 64-wide images each: the
// low half of the head (columns 0 .. 63) in the first IMG = KT * 4096 bytes, the high half (64 .. 127) in the next IMG -- every read
// keeps the 64-wide core's address inside its image (swizzles, ds_read_tr16_b64 addressing and bank analysis are unchanged), the half is
// one added constant.  The score tile of a (query block, key tile) is then 8 MFMA steps (Q fragments 0 .. 3 against the low image, 4 .. 7
// against the high one), the scale 1/sqrt(128), the output four 32 x 32 f32 tiles o[dt], d = 32 dt + l31 (dt 0, 1 from the low V image,
// 2, 3 from the high one), and there is no straight-line arm: it pays for itself in the 16-tile segments, which do not exist at NB 2.
template <int NB>
struct AttnStateCausal {
    float m_run, l_run;
    f32x16 o[2 * NB];
};
template <int NB>
static __device__ __forceinline__ void attn_state_init(AttnStateCausal<NB>& a) {
    a.m_run = -3.0e38f;
    a.l_run = 0.f;
#pragma unroll
    for (int dt = 0; dt < 2 * NB; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) a.o[dt][r] = 0.f;
}
// One group of four key tiles (tiles TB .. TB + 3 of the segment).  WHOLE: all four are live, lie strictly below the block's diagonal and
// hold real keys only -- no bounds, no masks, straight-line code as the FULL arm of attention_qblock_core; else the guarded form.  Both
// run the same operations on the same values in the same order for every visible key: which arm ran does not show in the bits.
template <int NB, int KT, bool WHOLE, int TB>
static __device__ __forceinline__ void attention_causal_group(const bf16x8 (&qf)[4 * NB], const char* Kl, const char* Vl, float* xch, int len, int ntiles, int lane,
                                                              int qbase, int key0, float& m_run, float& l_run, f32x16 (&o)[2 * NB]) {
    constexpr int GK = 4, IMG = KT * 32 * 128;
    const int l31 = lane & 31, hh = lane >> 5;
    const float sl2 = (NB == 1 ? 0.125f : 0.08838834764831844055f) * 1.44269504088896340736f;  // 1/sqrt(64 NB) * log2(e)
    const int q = qbase + l31;
    // S^T tiles of the group: st[i][r] = score(key = key0 + 32 t + (r&3) + 8 (r>>2) + 4 hh, query = q), t = TB + i
    f32x16 st[GK];
#pragma unroll
    for (int i = 0; i < GK; ++i) {
        const int t = TB + i;
        if (WHOLE || t < ntiles) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const int krow = 32 * t + l31;
#pragma unroll
            for (int ks = 0; ks < 4 * NB; ++ks) {
                const int c = 2 * (ks & 3) + hh;
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kl + (ks >> 2) * IMG + krow * 128 + ((c ^ ((krow >> 1) & 7)) << 4));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
            }
            st[i] = acc;
        }
    }
    float mx = m_run;
#pragma unroll
    for (int i = 0; i < GK; ++i) {
        const int t = TB + i;
        if (WHOLE || t < ntiles) {
            const int k0 = key0 + 32 * t;
            const bool whole = WHOLE || (k0 + 31 <= qbase && k0 + 32 <= len);  // below the diagonal of every query of the block, every key real
            if (whole) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[i][r]);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    if (key <= q && key < len) mx = fmaxf(mx, st[i][r]);
                }
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mb = mx * sl2;
    const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, sl2, -mb));  // group 0 of the sequence: exp2(-huge) = 0, and O, l are 0 anyway
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < GK; ++i) {
        const int t = TB + i;
        if (WHOLE || t < ntiles) {
            const int k0 = key0 + 32 * t;
            const bool whole = WHOLE || (k0 + 31 <= qbase && k0 + 32 <= len);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = __builtin_amdgcn_exp2f(fmaf(st[i][r], sl2, -mb));
                if (!whole) {
                    const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                    p = (key <= q && key < len) ? p : 0.f;  // a select: a masked score may have overflowed exp2
                }
                st[i][r] = p;
                sum += p;
            }
        }
    }
    sum += __shfl_xor(sum, 32, 64);
    l_run = fmaf(l_run, alpha, sum);
    m_run = mx;
    if (TB > 0 || key0 > 0) {  // rescale O (attention_qblock_core): alpha lives on lane q -> exchange through LDS
        xch[l31] = alpha;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 al = *reinterpret_cast<const f32x4*>(xch + 8 * g4 + 4 * hh);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int dt = 0; dt < 2 * NB; ++dt) o[dt][4 * g4 + c] *= al[c];
        }
    }
    // O += P V: operands as in attention_qblock_core, the V image of the output tile's half
#pragma unroll
    for (int i = 0; i < GK; ++i) {
        const int t = TB + i;
        if (WHOLE || t < ntiles) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                u32x4 pp;
#pragma unroll
                for (int j = 0; j < 4; ++j) pp[j] = pack_bf16x2(st[i][8 * s + 2 * j], st[i][8 * s + 2 * j + 1]);
                const bf16x8 pf = __builtin_bit_cast(bf16x8, pp);
#pragma unroll
                for (int dt = 0; dt < 2 * NB; ++dt) {
                    bf16x8 vf;
#pragma unroll
                    for (int piece = 0; piece < 2; ++piece) {
                        const int row = 32 * t + 16 * s + 8 * piece + 4 * hh + ((lane & 15) >> 2);
                        const int d0 = 32 * (dt & 1) + 16 * ((lane >> 4) & 1);
                        const int chunk = (d0 >> 3) + ((lane & 3) >> 1);
                        const int sw = chunk ^ (((row >> 1) & 1) << 2);
                        typedef __attribute__((address_space(3))) s16x4* lds_s16x4p;
                        const s16x4 got = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4p)(Vl + (dt >> 1) * IMG + row * 128 + sw * 16 + 8 * (lane & 1)));
                        vf[4 * piece + 0] = got[0];
                        vf[4 * piece + 1] = got[1];
                        vf[4 * piece + 2] = got[2];
                        vf[4 * piece + 3] = got[3];
                    }
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, vf, o[dt], 0, 0, 0);
                }
            }
        }
    }
}
template <int NB, int KT, int G = 0>
static __device__ __forceinline__ void attention_causal_groups(const bf16x8 (&qf)[4 * NB], const char* Kl, const char* Vl, float* xch, int len, int ntiles, int lane,
                                                               int qbase, int key0, float& m_run, float& l_run, f32x16 (&o)[2 * NB]) {
    if constexpr (4 * G < KT) {
        if (4 * G >= ntiles) return;  // wave-uniform: nothing for this query block in this group or a later one
        const int klast = key0 + 32 * (4 * G + 3);  // first key of the group's last tile
        // (segments of 4 tiles: no group lies below a diagonal; of 8: one group of half the blocks does, and the second arm cost the
        // 256-token class more in registers than it saved -- 82 against 70 us a launch)
        if (KT > 8 && 4 * G + 4 <= ntiles && klast + 31 <= qbase && klast + 32 <= len)
            attention_causal_group<NB, KT, true, 4 * G>(qf, Kl, Vl, xch, len, ntiles, lane, qbase, key0, m_run, l_run, o);
        else
            attention_causal_group<NB, KT, false, 4 * G>(qf, Kl, Vl, xch, len, ntiles, lane, qbase, key0, m_run, l_run, o);
        attention_causal_groups<NB, KT, G + 1>(qf, Kl, Vl, xch, len, ntiles, lane, qbase, key0, m_run, l_run, o);
    }
}
template <int NB, int KT>
static __device__ __forceinline__ void attention_qblock_causal(const bf16x8 (&qf)[4 * NB], const char* Kl, const char* Vl, float* xch, int len, int ntiles, int lane,
                                                               int qbase, int key0, AttnStateCausal<NB>& S_) {
    static_assert(KT % 4 == 0, "segments are whole groups of four key tiles");
    static_assert(NB == 1 || KT <= 8, "two images a key tile for K and for V: a 128-wide segment is at most 8 tiles of the 160 KiB");
    attention_causal_groups<NB, KT>(qf, Kl, Vl, xch, len, ntiles, lane, qbase, key0, S_.m_run, S_.l_run, S_.o);
}
// The store of a causal state, by its width.  64: attn_state_store above, the one of the non-causal kernels.
static __device__ __forceinline__ void attn_state_store(const AttnStateCausal<1>& S_, float* xch, char* ostg, bf16_t* obase, int H, int lane) {
    attn_state_store(AttnState{S_.m_run, S_.l_run, S_.o[0], S_.o[1]}, xch, ostg, obase, H, lane);
}
// 128: o[dt][r] = O[q = (r&3) + 8 (r>>2) + 4 hh][d = 32 dt + l31]: normalise by 1/l[q], stage as bf16 [q][128 d] in LDS 8 query rows at a
// time (2 KiB, wave-private), then leave as whole 256-byte rows, two 16-byte stores per lane.
static __device__ __forceinline__ void attn_state_store(const AttnStateCausal<2>& S_, float* xch, char* ostg, bf16_t* obase, int AW, int lane) {
    const int l31 = lane & 31, hh = lane >> 5;
    xch[l31] = 1.0f / S_.l_run;
    bf16_t* og = reinterpret_cast<bf16_t*>(ostg);
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 il = *reinterpret_cast<const f32x4*>(xch + 8 * g4 + 4 * hh);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ql = 4 * hh + c;  // row inside this block of 8
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) og[ql * 128 + 32 * dt + l31] = (bf16_t)(pack_bf16x2(S_.o[dt][4 * g4 + c] * il[c], 0.f) & 0xFFFFu);
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int idx = half * 64 + lane, ql = idx >> 4, c16 = idx & 15;
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(ostg + ql * 256 + c16 * 16);
            *reinterpret_cast<bf16x8*>(obase + (size_t)(8 * g4 + ql) * AW + c16 * 8) = v;
        }
    }
}

// ------------------------------------------------------------------ LDS of a launch
// Dynamic LDS of a workgroup of `nw` waves that stages `kts` key tiles of heads nb blocks of 64 columns wide: nb K images, nb V images
// (32 rows x 128 B per tile each), then per wave 32 floats of alpha / 1/l exchange and one [8 q][64 nb d] bf16 block of output staging.
// Every launcher sizes its launch with it.
static constexpr int attn_lds_bytes(int kts, int nw, int nb = 1) { return 2 * nb * kts * 32 * 128 + nw * 128 + nw * nb * 1024; }

// ------------------------------------------------------------------ head width as a policy
// What a kernel shell needs to know about the head width: the state of a query block, its init, the fold of the staged keys, the store,
// and Extra, the kernel argument the width brings along (ALiBi slopes; the 32-wide kernels have none: no 32-wide ALiBi model exists).
template <bool ALIBI>
struct Head64 {
    typedef AttnState State;
    typedef const float* __restrict__ Extra;  // [heads] ALiBi slopes (device), NULL without ALIBI
    typedef float Bias;                       // what the fold gets per head: the slope in the exp2 domain
    static constexpr bool TABLE = false;      // no LDS table behind the staging areas
    static constexpr int table_bytes(int, int) { return 0; }
    static __device__ __forceinline__ void init(State& st) { attn_state_init(st); }
    static __device__ __forceinline__ float slope2(Extra slopes, int head) { return ALIBI ? slopes[head] * 1.44269504088896340736f : 0.f; }
    template <int KT, bool FULL, int GKMAX>
    static __device__ __forceinline__ void fold(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, int len, int nkt, int lane, int qbase, float slope2, State& st, bool first,
                                                int key0) {
        attention_qblock_core<KT, FULL, ALIBI, GKMAX>(qf, Kl, Vl, xch, len, nkt, lane, qbase, slope2, st, first, key0);
    }
    static __device__ __forceinline__ void store(const State& st, float* xch, char* ostg, bf16_t* obase, int H, int lane) {
        attn_state_store(st, xch, ostg, obase, H, lane);
    }
};
struct Head32 {
    typedef AttnState32 State;
    struct Extra {};
    typedef float Bias;
    static constexpr bool TABLE = false;
    static constexpr int table_bytes(int, int) { return 0; }
    static __device__ __forceinline__ void init(State& st) { attn_state32_init(st); }
    static __device__ __forceinline__ float slope2(Extra, int) { return 0.f; }
    template <int KT, bool FULL, int GKMAX>
    static __device__ __forceinline__ void fold(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, int len, int nkt, int lane, int, float, State& st, bool first, int) {
        attention_qblock_core32<KT, FULL, GKMAX>(qf, Kl, Vl, xch, len, nkt, lane, st, first);
    }
    static __device__ __forceinline__ void store(const State& st, float* xch, char* ostg, bf16_t* obase, int H, int lane) {
        attn_state32_store(st, xch, ostg, obase, H, lane);
    }
};

// Heads of 64 with a bucketed relative position bias (T5, cfg.pos_type 3): score = q.k + bias[head][bucket(key - query)], no 1/sqrt(d).
// The host expands the model's [buckets][heads] table through the bucket rule (rel_bucket_rule.h) into a DISTANCE table per head,
// tbl[head][d + span - 1] for d = key - query in -(span - 1) .. span - 1.  A workgroup stages the slice its queries
// (QW of them from qlo) and the staged keys (SEG of them from key0) can reach behind the staging areas of the shell -- entry j holds the
// distance key0 - qlo - (QW - 1) + j, SEG + QW - 1 entries -- and the fold starts each score accumulator from tbw[kr - l31]: one LDS read per
// score, no transcendental, no global load, no arithmetic beside the MFMAs.  key0 and qbase enter through the staging exactly as ALiBi uses
// them: segments of the long kernel, positions relative to the text's start in packed rows.
struct RelBias {
    const float* tbl;  // [heads][2 span - 1] f32 (device)
    int span;          // cfg.max_pos
};
struct Head64Rel {
    typedef AttnState State;
    typedef RelBias Extra;
    typedef const float* Bias;  // tbw of attention_qblock_core
    static constexpr bool TABLE = true;
    static constexpr int table_bytes(int seg, int qw) { return (seg + qw) * 4; }
    static __device__ __forceinline__ void init(State& st) { attn_state_init(st); }
    // entries d0 .. d0 + n - 1 of the head's table -> tb[0 .. n); a distance no (query, key) of a text can have is clamped into the table
    static __device__ __forceinline__ void stage(Extra ex, int head, float* tb, int d0, int n, int tid, int nthreads) {
        const int last = 2 * ex.span - 2;
        const float* src = ex.tbl + (size_t)head * (last + 1);
        for (int j = tid; j < n; j += nthreads) {
            int g = d0 + j + ex.span - 1;
            g = g < 0 ? 0 : (g > last ? last : g);
            tb[j] = src[g];
        }
    }
    // the wave's view of the staged slice: its query block starts `qoff` = (QW - 1) - (qbase - qlo) entries in
    static __device__ __forceinline__ Bias bias(const float* tb, int qoff) { return tb + qoff; }
    template <int KT, bool FULL, int GKMAX>
    static __device__ __forceinline__ void fold(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, int len, int nkt, int lane, int qbase, Bias tbw, State& st, bool first,
                                                int key0) {
        // segments of 16 tiles fold in groups of TWO: with four, the bias reads in flight on top of 64 live scores put attention_kernel<.., 16, 8>
        // (one workgroup per CU by its LDS, 256 registers a lane) 7 registers into scratch; with two it has none
        attention_qblock_core<KT, FULL, 2, (KT >= 16 && GKMAX > 2 ? 2 : GKMAX)>(qf, Kl, Vl, xch, len, nkt, lane, qbase, 0.f, st, first, key0, tbw);
    }
    static __device__ __forceinline__ void store(const State& st, float* xch, char* ostg, bf16_t* obase, int H, int lane) {
        attn_state_store(st, xch, ostg, obase, H, lane);
    }
};
// What a shell hands the fold per head: the slope (Head64, Head32) or the wave's view of the staged table (Head64Rel)
template <class HEAD>
static __device__ __forceinline__ typename HEAD::Bias attn_bias_arg(typename HEAD::Extra extra, int head, const float* tb, int qoff) {
    if constexpr (HEAD::TABLE) return HEAD::bias(tb, qoff);
    else return HEAD::slope2(extra, head);
}

// The lane id for the store behind a segment loop.  The table policy's loop kernels sit at the 256 registers of their launch bounds, and the
// compiler kept lane & 7 -- needed by the store only -- alive across the loop in scratch (4 bytes, 8 allocated) instead of recomputing it;
// read afresh from the hardware behind the loop, nothing of it lives across.  The other policies keep their `lane`.
template <class HEAD>
static __device__ __forceinline__ int attn_store_lane(int lane) {
    if constexpr (HEAD::TABLE) return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    else return lane;
}

// ------------------------------------------------------------------ launching
// Raises KERNEL's dynamic-LDS limit to LDS bytes once per instantiation and device, then launches it with that much.
template <auto KERNEL, int LDS, class... ARGS>
static void attn_launch(dim3 grid, int threads, hipStream_t s, ARGS... args) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS); });
    hipLaunchKernelGGL(KERNEL, grid, dim3((unsigned)threads), (size_t)LDS, s, args...);
}
// The three launch classes of a packed work-item table (sc_packed_items: items sorted by class, nitems[3] per class):
// launch(class as std::integral_constant, first item of the class, their number) for every class that has items.
template <class F>
static void attn_packed_classes(const int32_t* items, const int* nitems, F launch) {
    if (nitems[0] > 0) launch(std::integral_constant<int, 0>(), items, nitems[0]);
    if (nitems[1] > 0) launch(std::integral_constant<int, 1>(), items + 4 * (size_t)nitems[0], nitems[1]);
    if (nitems[2] > 0) launch(std::integral_constant<int, 2>(), items + 4 * ((size_t)nitems[0] + nitems[1]), nitems[2]);
}
