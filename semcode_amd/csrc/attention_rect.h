// attention_rect.h -- the rectangle attention kernels as templates on the head policy (attention_core.h) and their launch templates.
// Included by encoder_ops.hip (Head64<false / true>, Head32) and by encoder_t5.hip (Head64Rel): the T5 instantiations are a translation
// unit, and so a code object, of their own, and the code objects of the models that existed before them stay what they were.
#pragma once
#include "attention_core.h"

// ------------------------------------------------------------------ attention
// qkv: [tokens, 3H] bf16 rows = [Q | K | V], head h at columns h*64 of each third.  ctx: [tokens, H].
// KT = S / 32 key tiles.  LDS: K image [S][64] with chunk ^= (row>>1)&7, V image [S][64] with
// chunk ^= ((row>>1)&1)<<2 (conflict-free for ds_read_b128 rows / ds_read_b64_tr_b16 blocks).
// One 32-row query block of one wave, keys processed in groups of 4 tiles (128 keys) with an online softmax, so
// that only 64 score registers are live (S = 256 runs 2 workgroups per CU, S = 512 no longer spills).
// FULL = every key of the padded sequence is real (len == S): no per-tile guards or masks.
// HEAD (attention_core.h): Head64<ALIBI> -- one head of 64 per 64-column block; ALIBI: scores get the symmetric linear bias
// -slope_head * |query - key| (jina-bert-v2 style encoders, no position table) -- or Head32, a pair of heads of 32 per block.
// State, fold and store stay inside each FULL arm: declared around the branch, the compiler merges the two store tails and the
// kernels come out with other register counts.
// The shell around the math (LDS carve-up, operand addressing, staging loops, Q load) is written out in every attention kernel
// (here, encoder_packed.hip, encoder_window.hip).  As shared functions -- tried: carve-up, operand, staging, Q load, one segmented
// body under attention_long_kernel and attention_packed_kernel -- each alone changes the compiler's text of these kernels (registers
// at 1 - 4 key tiles, scratch at S = 512, block order), and the 8-tile packed class measured 1.6 - 1.9 % slower per launch through
// them.  Written out, every Head64 instantiation is the instruction text it was before the head width became a policy
// (profiles/attention_shell_kernels.log).
template <class HEAD, int KT, bool FULL, int GKMAX>
static __device__ __forceinline__ void attention_qblock(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, char* ostg,
                                                        bf16_t* obase, int H, int len, int nkt, int lane, int qbase, typename HEAD::Bias slope2) {
    typename HEAD::State st;
    HEAD::init(st);
    HEAD::template fold<KT, FULL, GKMAX>(qf, Kl, Vl, xch, len, nkt, lane, qbase, slope2, st, true, 0);
    HEAD::store(st, xch, ostg, obase, H, lane);
}

// One workgroup per (chunk, 64-column block), NW waves (4, or 8 from S = 256 on; at S = 256 one query block per wave and two key-tile
// groups of 2 -> half the registers, so that 4 waves instead of 2 share a SIMD and cover each other's MFMA -> softmax -> MFMA
// dependency stalls)
template <class HEAD, int KT, int NW>
__global__ __launch_bounds__(NW * 64, (KT <= 8 ? 2 : 1)) void attention_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int H,
                                                            typename HEAD::Extra extra, bf16_t* __restrict__ ctx, int blocked) {
    constexpr int S = KT * 32;
    constexpr int NQB = (KT + NW - 1) / NW;  // query blocks per wave
    constexpr int GKMAX = (NW == 8 && KT <= 8) ? 2 : 4;  // S = 512 runs one workgroup per CU anyway (LDS): registers are not its limit
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + S * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * S * 128) + w * 32;  // [NW waves][32] alpha / 1/l exchange
    char* ostg = smem + 2 * S * 128 + NW * 128 + w * 1024;               // per-wave [8 q][64 d] bf16 output staging
    float* tb = nullptr;  // HEAD::TABLE: the head's distance table for the queries and keys 0 .. S - 1, behind the staging areas
    if constexpr (HEAD::TABLE) tb = reinterpret_cast<float*>(smem + attn_lds_bytes(KT, NW));
    const int head = blockIdx.x, b = blockIdx.y;
    // row-major QKV [tokens][3H] (Q | K | V, block j at column 64 j), or -- blocked -- [3H/64][tokens][64] as the QKV projection writes it
    // (gemm_bf16.hip c_index; `blocked` = tokens padded to that GEMM's M, 0 = row-major): every operand of this (chunk, block) is then one contiguous [S][64] block
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nh = (size_t)(H >> 6);  // blocked = the row count (M) of the projection that wrote the blocks
    const bf16_t* base = blocked ? qkv + ((size_t)head * T + (size_t)b * S) * 64 : qkv + (size_t)b * S * ld + head * 64;
    const size_t koff = blocked ? nh * T * 64 : (size_t)H, voff = 2 * koff;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    const int nkt = (len + 31) >> 5;  // key tiles holding at least one real key; later tiles are skipped entirely

    // ---- stage K then V rows [0, 32 nkt) of this (chunk, block): pieces of 8 rows x 128 B = 1 KiB
    for (int piece = w; piece < nkt * 4; piece += NW) {
        const int p = piece * 64 + lane;
        const int r = p >> 3, ck = (p & 7) ^ ((r >> 1) & 7);
        __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)r * ld + koff + ck * 8), (lds_vptr)(Kl + piece * 1024), 16, 0, 0);
    }
    for (int piece = w; piece < nkt * 4; piece += NW) {
        const int p = piece * 64 + lane;
        const int r = p >> 3, cv = (p & 7) ^ (((r >> 1) & 1) << 2);
        __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)r * ld + voff + cv * 8), (lds_vptr)(Vl + piece * 1024), 16, 0, 0);
    }
    // Q fragments of all of this wave's query blocks (B operand: lane (q = lane&31, hh) holds Q[q][16 ks + 8 hh .. +7]),
    // requested now so that their latency hides behind the K/V staging
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[NQB][4];
#pragma unroll
    for (int i = 0; i < NQB; ++i) {
        const int qb = w + NW * i;
        if (qb < KT) {
            const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[i][ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
        }
    }
    if constexpr (HEAD::TABLE) HEAD::stage(extra, head, tb, -(S - 1), 2 * S - 1, tid, NW * 64);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

#pragma unroll
    for (int i = 0; i < NQB; ++i) {
        const int qb = w + NW * i;
        if (qb < KT) {
            bf16_t* obase = ctx + (size_t)(b * S + qb * 32) * H + head * 64;
            const typename HEAD::Bias slope2 = attn_bias_arg<HEAD>(extra, head, tb, (S - 1) - qb * 32);
            if (nkt == KT && (len & 31) == 0) attention_qblock<HEAD, KT, true, GKMAX>(qf[i], Kl, Vl, xch, ostg, obase, H, len, nkt, lane, qb * 32, slope2);
            else attention_qblock<HEAD, KT, false, GKMAX>(qf[i], Kl, Vl, xch, ostg, obase, H, len, nkt, lane, qb * 32, slope2);
        }
    }
}

// ---- sequences of 1 024 and 2 048 tokens (the reference's default chunker emits up to 200 lines / 6 000 characters per chunk --
// src/semcode/chunking/tree_sitter_chunker.py:64-65 -- i.e. 1.5-2k word pieces; jina-embeddings-v2 is an 8k-context ALiBi
// model).  K and V of 512 keys fill the LDS (128 KiB), so the keys are attended in SEGMENTS of 512: stage a segment, every wave
// folds it into the online-softmax state of its ONE 32-row query block (AttnState, 34 registers), next segment.  A workgroup takes 8 query blocks (256 queries) of one (chunk, block); the S / 256 workgroups of a
// (chunk, block) each stage all its keys (from L2 after the first).  Same arithmetic per (query, key) as attention_kernel: a
// sequence of <= 512 real tokens padded to 1 024 gives the bits the S = 512 kernel gives.
template <class HEAD>
__global__ __launch_bounds__(512, 1) void attention_long_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int S, int H,
                                                                typename HEAD::Extra extra, bf16_t* __restrict__ ctx, int blocked) {
    constexpr int KT = 16, NW = 8, SEG = 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + SEG * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * SEG * 128) + w * 32;
    char* ostg = smem + 2 * SEG * 128 + NW * 128 + w * 1024;
    float* tb = nullptr;  // HEAD::TABLE: the slice of the head's distance table this workgroup's 256 queries and ALL the text's keys reach, staged once
    if constexpr (HEAD::TABLE) tb = reinterpret_cast<float*>(smem + attn_lds_bytes(KT, NW));
    const int head = blockIdx.x, b = blockIdx.y, qb = (int)blockIdx.z * NW + w;  // this wave's 32-row query block
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nh = (size_t)(H >> 6);
    const bf16_t* base = blocked ? qkv + ((size_t)head * T + (size_t)b * S) * 64 : qkv + (size_t)b * S * ld + head * 64;
    const size_t koff = blocked ? nh * T * 64 : (size_t)H, voff = 2 * koff;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[4];
    {
        const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
    }
    typename HEAD::State st;
    HEAD::init(st);
    typename HEAD::Bias slope2 = attn_bias_arg<HEAD>(extra, head, tb, (32 * NW - 1) - 32 * w);
    const int nseg = (len + SEG - 1) / SEG;
    // (entry j = distance -qlo - (QW - 1) + j; the barrier behind the first segment's K / V covers it, and a segment's view is key0 entries on)
    if constexpr (HEAD::TABLE) HEAD::stage(extra, head, tb, -(int)blockIdx.z * 32 * NW - (32 * NW - 1), nseg * SEG + 32 * NW - 1, tid, NW * 64);
#pragma unroll 1
    for (int seg = 0; seg < nseg; ++seg) {
        const int key0 = seg * SEG;
        const int slen = len - key0 < SEG ? len - key0 : SEG;  // real keys in this segment
        const int nkt = (slen + 31) >> 5;
        if (seg) __syncthreads();  // every wave is done with the previous segment's K / V
        for (int piece = w; piece < nkt * 4; piece += NW) {
            const int p = piece * 64 + lane;
            const int r = p >> 3, ck = (p & 7) ^ ((r >> 1) & 7);
            __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)(key0 + r) * ld + koff + ck * 8), (lds_vptr)(Kl + piece * 1024), 16, 0, 0);
        }
        for (int piece = w; piece < nkt * 4; piece += NW) {
            const int p = piece * 64 + lane;
            const int r = p >> 3, cv = (p & 7) ^ (((r >> 1) & 1) << 2);
            __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)(key0 + r) * ld + voff + cv * 8), (lds_vptr)(Vl + piece * 1024), 16, 0, 0);
        }
        if constexpr (HEAD::TABLE) slope2 = HEAD::bias(tb, (32 * NW - 1) - 32 * w + key0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nkt == KT && (slen & 31) == 0) HEAD::template fold<KT, true, 4>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
        else HEAD::template fold<KT, false, 4>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
    }
    HEAD::store(st, xch, ostg, ctx + (size_t)(b * S + qb * 32) * H + head * 64, H, attn_store_lane<HEAD>(lane));
}

// ------------------------------------------------------------------ launch templates
template <class HEAD, int KT>
static void launch_attn(const void* qkv, const int32_t* lens, int B, int H, typename HEAD::Extra extra, void* ctx, int blocked, hipStream_t s) {
    constexpr int NW = KT >= 8 ? 8 : 4;
    attn_launch<attention_kernel<HEAD, KT, NW>, attn_lds_bytes(KT, NW) + HEAD::table_bytes(32 * KT, 32 * KT)>(dim3((unsigned)(H / 64), (unsigned)B), NW * 64, s,
                                                                                                               (const bf16_t*)qkv, lens, H, extra, (bf16_t*)ctx, blocked);
}
template <class HEAD>
static void launch_attention(const void* qkv, const int32_t* lens, int B, int S, int H, typename HEAD::Extra extra, void* ctx, int blocked, hipStream_t s) {
    if (S > 512) {  // K / V streamed through the LDS in segments of 512 keys
        attn_launch<attention_long_kernel<HEAD>, attn_lds_bytes(16, 8) + HEAD::table_bytes(2048, 256)>(dim3((unsigned)(H / 64), (unsigned)B, (unsigned)(S / 256)), 512, s,
                                                                                                       (const bf16_t*)qkv, lens, S, H, extra, (bf16_t*)ctx, blocked);
        return;
    }
    switch (S) {
        case 32: launch_attn<HEAD, 1>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 64: launch_attn<HEAD, 2>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 128: launch_attn<HEAD, 4>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 256: launch_attn<HEAD, 8>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 512: launch_attn<HEAD, 16>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        default: break;
    }
}
