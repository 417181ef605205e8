// encoder_attn32.hip -- attention for head dimension 32 (gfx950): the 384-hidden BERT family (MiniLM, e5-small, the ms-marco MiniLM
// cross-encoders), 12 heads of 32.
//
// The QKV projections write 64-column blocks [3H/64][M][64] whatever the head width, so with 32-wide heads block j of each third holds
// the PAIR of heads 2j (columns 0..31) and 2j + 1 (columns 32..63); hidden % 128 == 0 makes the head count even.  A workgroup takes
// one (pair, sequence) -- or (pair, work item) on packed rows -- where the 64-wide kernels take one (head, ...): the grids, the
// K / V images in the LDS (128-byte rows, both swizzles, the global_load_lds pieces), the Q fragments, the LDS budgets and the launch
// classes are those of attention_kernel, attention_long_kernel (encoder_ops.hip) and attention_packed_kernel (encoder_packed.hip),
// restated here so that not one instruction of those kernels changes.  What differs is the per-wave math, attention_core.h:
// attention_qblock_core32 runs the online softmax once per head of the pair over half of the columns, attn_state32_store normalises
// the two halves of an output row by their own denominators.  Plain attention only: no 32-wide ALiBi or rotary model exists.
//
// Registers / LDS as the compiler reports them (-Rpass-analysis=kernel-resource-usage: VGPRs, no AGPRs; dynamic LDS of the launch):
//   attention32_kernel         KT 1 / 2 / 4 (4 waves)  102 / 130 / 165 registers, 12.5 / 20.5 / 36.5 KiB -> KT 4: 3 workgroups per CU, as at 64
//                              KT 8 (8 waves)          157 registers, 73 KiB  -> 1 workgroup per CU (the 64-wide kernel's 124 let 2 in)
//                              KT 16 (8 waves)         248 registers, 137 KiB -> 1 workgroup per CU, as at 64
//   attention32_long_kernel    8 waves                 256 registers + 8 bytes of scratch per lane (two dwords spilled), 137 KiB
//   attention32_packed_kernel  KT 4 / 8 / 16           165 / 159 / 256 registers, 36.5 / 73 / 137 KiB, no scratch
// The state itself is 36 registers against AttnState's 34; the rest of the difference to the 64-wide kernels (131 / 124 / 256) is what
// the compiler holds across the two-trip head loop of attention_qblock_core32.  Unrolling that loop instead costs 244 registers at
// KT 4 and 0.4 - 2.4 KB of scratch per lane from KT 8 on.
// Measured (scripts/bench_minilm.py, 384 hidden, 256-token texts): attention takes 1.56 x the time of 6 heads of 64.
#include "attention_core.h"  // AttnState32, attention_qblock_core32, attn_state32_store
#include "encoder_ops.h"
#include "gemm_tile.h"  // bf16 helpers, LDS-DMA pointer types

// ------------------------------------------------------------------ rectangles, S <= 512 (attention_kernel's twin)
template <int KT, int NW = 4>
__global__ __launch_bounds__(NW * 64, (KT <= 8 ? 2 : 1)) void attention32_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int H,
                                                                                  bf16_t* __restrict__ ctx, int blocked) {
    constexpr int S = KT * 32;
    constexpr int NQB = (KT + NW - 1) / NW;  // query blocks per wave
    constexpr int GKMAX = (NW == 8 && KT <= 8) ? 2 : 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + S * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * S * 128) + w * 32;  // [NW waves][32] alpha / 1/l exchange
    char* ostg = smem + 2 * S * 128 + NW * 128 + w * 1024;               // per-wave [8 q][64 d] bf16 output staging
    const int pair = blockIdx.x, b = blockIdx.y;                         // heads 2 pair, 2 pair + 1
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nb = (size_t)(H >> 6);  // blocked = the row count (M) of the projection that wrote the blocks
    const bf16_t* base = blocked ? qkv + ((size_t)pair * T + (size_t)b * S) * 64 : qkv + (size_t)b * S * ld + pair * 64;
    const size_t koff = blocked ? nb * T * 64 : (size_t)H, voff = 2 * koff;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    const int nkt = (len + 31) >> 5;  // key tiles holding at least one real key; later tiles are skipped entirely

    // ---- stage K then V rows [0, 32 nkt) of this (chunk, pair): pieces of 8 rows x 128 B = 1 KiB
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
    // Q fragments (B operand: lane (q = lane&31, hh) holds Q[q][16 ks + 8 hh .. +7]; ks 0, 1 = head 2 pair, ks 2, 3 = head 2 pair + 1)
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
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

#pragma unroll
    for (int i = 0; i < NQB; ++i) {
        const int qb = w + NW * i;
        if (qb < KT) {
            AttnState32 st;
            attn_state32_init(st);
            if (nkt == KT && (len & 31) == 0) attention_qblock_core32<KT, true, GKMAX>(qf[i], Kl, Vl, xch, len, nkt, lane, st, true);
            else attention_qblock_core32<KT, false, GKMAX>(qf[i], Kl, Vl, xch, len, nkt, lane, st, true);
            attn_state32_store(st, xch, ostg, ctx + (size_t)(b * S + qb * 32) * H + pair * 64, H, lane);
        }
    }
}

// ------------------------------------------------------------------ rectangles of 1 024 and 2 048 tokens (attention_long_kernel's twin)
// Keys in segments of 512, every wave folds each segment into the AttnState32 of its one query block.  Same arithmetic per (query, key)
// as attention32_kernel at S = 512: a sequence of <= 512 real tokens padded to 1 024 gives the same bits.
__global__ __launch_bounds__(512, 1) void attention32_long_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int S, int H,
                                                                  bf16_t* __restrict__ ctx, int blocked) {
    constexpr int KT = 16, NW = 8, SEG = 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + SEG * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * SEG * 128) + w * 32;
    char* ostg = smem + 2 * SEG * 128 + NW * 128 + w * 1024;
    const int pair = blockIdx.x, b = blockIdx.y, qb = (int)blockIdx.z * NW + w;  // this wave's 32-row query block
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nb = (size_t)(H >> 6);
    const bf16_t* base = blocked ? qkv + ((size_t)pair * T + (size_t)b * S) * 64 : qkv + (size_t)b * S * ld + pair * 64;
    const size_t koff = blocked ? nb * T * 64 : (size_t)H, voff = 2 * koff;
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
    AttnState32 st;
    attn_state32_init(st);
    const int nseg = (len + SEG - 1) / SEG;
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
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nkt == KT && (slen & 31) == 0) attention_qblock_core32<KT, true, 4>(qf, Kl, Vl, xch, slen, nkt, lane, st, seg == 0);
        else attention_qblock_core32<KT, false, 4>(qf, Kl, Vl, xch, slen, nkt, lane, st, seg == 0);
    }
    attn_state32_store(st, xch, ostg, ctx + (size_t)(b * S + qb * 32) * H + pair * 64, H, lane);
}

// ------------------------------------------------------------------ packed rows (attention_packed_kernel's twin)
// Work items and launch classes of encoder_packed.hip; blockIdx.y is the pair.  A wave whose block lies at or beyond ceil32(len) stages
// its share of K and V and reaches every barrier, but does no math and stores nothing.
template <int KT, int NW>
__global__ __launch_bounds__(NW * 64, (KT <= 8 ? 2 : 1)) void attention32_packed_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ items, int H,
                                                                                         bf16_t* __restrict__ ctx, int blocked) {
    constexpr int SEG = KT * 32;
    constexpr int GKMAX = (NW == 8 && KT <= 8) ? 2 : 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + SEG * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * SEG * 128) + w * 32;
    char* ostg = smem + 2 * SEG * 128 + NW * 128 + w * 1024;
    const int pair = blockIdx.y;
    const int32_t* it = items + 4 * (size_t)blockIdx.x;
    const int start = __builtin_amdgcn_readfirstlane(it[0]);
    int len = it[1];
    len = len < 1 ? 1 : len;
    len = __builtin_amdgcn_readfirstlane(len);
    const int qb = __builtin_amdgcn_readfirstlane(it[2]) + w;  // this wave's 32-row query block of the sequence
    const bool live = qb * 32 < len;                            // wave-uniform
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nb = (size_t)(H >> 6);
    const bf16_t* base = blocked ? qkv + ((size_t)pair * T + (size_t)start) * 64 : qkv + (size_t)start * ld + pair * 64;
    const size_t koff = blocked ? nb * T * 64 : (size_t)H, voff = 2 * koff;
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[4];
    if (live) {
        const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
    }
    AttnState32 st;
    attn_state32_init(st);
    const int nseg = KT == 16 ? (len + SEG - 1) / SEG : 1;  // the shorter classes hold the whole sequence: no loop, no carried state
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
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (!live) continue;
        if (nkt == KT && (slen & 31) == 0) attention_qblock_core32<KT, true, GKMAX>(qf, Kl, Vl, xch, slen, nkt, lane, st, seg == 0);
        else attention_qblock_core32<KT, false, GKMAX>(qf, Kl, Vl, xch, slen, nkt, lane, st, seg == 0);
    }
    if (live) attn_state32_store(st, xch, ostg, ctx + ((size_t)start + (size_t)qb * 32) * H + pair * 64, H, lane);
}

// ------------------------------------------------------------------ launchers (sc_launch_attention / sc_launch_attention_packed dispatch here)
template <int KT>
static void launch_attn32(const void* qkv, const int32_t* lens, int B, int H, void* ctx, int blocked, hipStream_t s) {
    constexpr int NW = KT >= 8 ? 8 : 4;
    constexpr int lds = KT * 32 * 256 + NW * 1152;
    static ScDeviceOnce once;  // per instantiation and device
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(attention32_kernel<KT, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    hipLaunchKernelGGL((attention32_kernel<KT, NW>), dim3((unsigned)(H / 64), (unsigned)B), dim3(NW * 64), (size_t)lds, s, (const bf16_t*)qkv, lens, H, (bf16_t*)ctx,
                       blocked);
}
void sc_launch_attention32(const void* qkv, const int32_t* lens, int B, int S, int H, void* ctx, hipStream_t s, int blocked) {
    if (S > 512) {  // K / V streamed through the LDS in segments of 512 keys
        static ScDeviceOnce once;
        const int lds = 2 * 512 * 128 + 8 * 128 + 8 * 1024;
        sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(attention32_long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
        hipLaunchKernelGGL(attention32_long_kernel, dim3((unsigned)(H / 64), (unsigned)B, (unsigned)(S / 256)), dim3(512), (size_t)lds, s, (const bf16_t*)qkv, lens, S, H,
                           (bf16_t*)ctx, blocked);
        return;
    }
    switch (S) {
        case 32: launch_attn32<1>(qkv, lens, B, H, ctx, blocked, s); break;
        case 64: launch_attn32<2>(qkv, lens, B, H, ctx, blocked, s); break;
        case 128: launch_attn32<4>(qkv, lens, B, H, ctx, blocked, s); break;
        case 256: launch_attn32<8>(qkv, lens, B, H, ctx, blocked, s); break;
        case 512: launch_attn32<16>(qkv, lens, B, H, ctx, blocked, s); break;
        default: break;
    }
}
template <int KT, int NW>
static void launch_attn32_packed(const void* qkv, const int32_t* items, int nitems, int H, void* ctx, int blocked, hipStream_t s) {
    if (nitems < 1) return;
    constexpr int lds = 2 * KT * 32 * 128 + NW * 128 + NW * 1024;
    static ScDeviceOnce once;  // per instantiation and device
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(attention32_packed_kernel<KT, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    hipLaunchKernelGGL((attention32_packed_kernel<KT, NW>), dim3((unsigned)nitems, (unsigned)(H / 64)), dim3(NW * 64), (size_t)lds, s, (const bf16_t*)qkv, items, H,
                       (bf16_t*)ctx, blocked);
}
void sc_launch_attention32_packed(const void* qkv, const int32_t* items, const int* nitems, int H, void* ctx, hipStream_t s, int blocked) {
    launch_attn32_packed<16, 8>(qkv, items, nitems[0], H, ctx, blocked, s);
    launch_attn32_packed<8, 8>(qkv, items + 4 * (size_t)nitems[0], nitems[1], H, ctx, blocked, s);
    launch_attn32_packed<4, 4>(qkv, items + 4 * ((size_t)nitems[0] + nitems[1]), nitems[2], H, ctx, blocked, s);
}
