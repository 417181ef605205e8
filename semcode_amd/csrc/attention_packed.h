// attention_packed.h -- the packed attention kernel as a template on the head policy (attention_core.h) and its launch template.
// Included by encoder_packed.hip (Head64<false / true>, Head32) and by encoder_t5.hip (Head64Rel), as attention_rect.h is.
#pragma once
#include "attention_core.h"

// ------------------------------------------------------------------ attention
// A work item is four int32 {start row of the sequence, its length, first 32-row query block of the item, 0}; a workgroup of NW
// waves takes one item and one 64-column block (a head of 64, a pair of heads of 32: HEAD, attention_core.h), wave w the query block
// `first + w`.  The keys of the sequence are staged into the LDS in segments of 32 KT keys from row `start`, as
// attention_long_kernel stages them from b * S, and every wave folds each segment into the state of its query block.  A wave whose
// block lies at or beyond ceil32(len) stages its share of K and V and reaches every barrier, but does no math and stores nothing.
// ALiBi distances count from the start of the sequence.
//
// The shell is written out here as in attention_kernel (encoder_ops.hip says why): through shared shell functions,
// as a wrapper of one segmented body shared with attention_long_kernel, the 8-tile class ran 1.6 - 1.9 % slower per launch on 256
// texts of 256 tokens at 384 hidden (heads of 64; 0.7 - 1.0 % with heads of 32) in two measurements, with no register or occupancy
// change to show for it.  Written out, all nine instantiations are the instruction text of the kernels they replace.
//
// Three launch classes keep short sequences from holding a 512-thread workgroup and 128 KiB of LDS (sc_packed_items sorts the
// items by class; a class depends on the sequence's own length only, so a text's result does not depend on its neighbours):
//   len <= 128 : KT 4,  4 waves,  37 KiB LDS, 131 registers (ALiBi 195, head_dim 32 165) -> 3 (2, 3) workgroups per CU
//   len <= 256 : KT 8,  8 waves,  73 KiB LDS, 124 registers (ALiBi 256, head_dim 32 159) -> 2 (1, 1) workgroups per CU, key tiles in groups of 2 (attention_kernel at S = 256)
//   longer     : KT 16, 8 waves, 137 KiB LDS, 256 registers -> 1 workgroup per CU, one item per 8 query blocks, segments of 512 keys
// (registers as the compiler reports them; they, not the LDS, bound the two short classes)
template <class HEAD, int KT, int NW>
__global__ __launch_bounds__(NW * 64, (KT <= 8 ? 2 : 1)) void attention_packed_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ items, int H,
                                                                                         typename HEAD::Extra extra, bf16_t* __restrict__ ctx, int blocked) {
    constexpr int SEG = KT * 32;
    constexpr int GKMAX = (NW == 8 && KT <= 8) ? 2 : 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + SEG * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * SEG * 128) + w * 32;
    char* ostg = smem + 2 * SEG * 128 + NW * 128 + w * 1024;
    float* tb = nullptr;  // HEAD::TABLE: the slice of the head's distance table this item's 32 NW queries and ALL the text's keys reach, staged once
    if constexpr (HEAD::TABLE) tb = reinterpret_cast<float*>(smem + attn_lds_bytes(KT, NW));
    const int head = blockIdx.y;
    const int32_t* it = items + 4 * (size_t)blockIdx.x;
    const int start = __builtin_amdgcn_readfirstlane(it[0]);
    int len = it[1];
    len = len < 1 ? 1 : len;
    len = __builtin_amdgcn_readfirstlane(len);
    const int qb = __builtin_amdgcn_readfirstlane(it[2]) + w;  // this wave's 32-row query block of the sequence
    const bool live = qb * 32 < len;                            // wave-uniform
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nh = (size_t)(H >> 6);  // blocked = the row count (M) of the projection that wrote the blocks
    const bf16_t* base = blocked ? qkv + ((size_t)head * T + (size_t)start) * 64 : qkv + (size_t)start * ld + head * 64;
    const size_t koff = blocked ? nh * T * 64 : (size_t)H, voff = 2 * koff;
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[4];
    if (live) {
        const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
    }
    typename HEAD::State st;
    HEAD::init(st);
    typename HEAD::Bias slope2 = attn_bias_arg<HEAD>(extra, head, tb, (32 * NW - 1) - 32 * w);
    const int nseg = KT == 16 ? (len + SEG - 1) / SEG : 1;  // the shorter classes hold the whole sequence: no loop, no carried state
    // (entry j = distance -qlo - (QW - 1) + j; the barrier behind the first segment's K / V covers it, and a segment's view is key0 entries on)
    if constexpr (HEAD::TABLE) HEAD::stage(extra, head, tb, -32 * (qb - w) - (32 * NW - 1), nseg * SEG + 32 * NW - 1, tid, NW * 64);
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
        if (!live) continue;
        if (nkt == KT && (slen & 31) == 0) HEAD::template fold<KT, true, GKMAX>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
        else HEAD::template fold<KT, false, GKMAX>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
    }
    if (live) HEAD::store(st, xch, ostg, ctx + ((size_t)start + (size_t)qb * 32) * H + head * 64, H, attn_store_lane<HEAD>(lane));
}

// ------------------------------------------------------------------ launch template
template <class HEAD>
static void launch_attention_packed(const void* qkv, const int32_t* items, const int* nitems, int H, typename HEAD::Extra extra, void* ctx, int blocked, hipStream_t s) {
    attn_packed_classes(items, nitems, [&](auto cls, const int32_t* first, int n) {
        constexpr int KT = 16 >> decltype(cls)::value, NW = KT >= 8 ? 8 : 4;  // 16 / 8 / 4 key tiles
        attn_launch<attention_packed_kernel<HEAD, KT, NW>, attn_lds_bytes(KT, NW) + HEAD::table_bytes(KT == 16 ? 2048 : 32 * KT, 32 * NW)>(dim3((unsigned)n, (unsigned)(H / 64)), NW * 64, s,
                                                                                                                         (const bf16_t*)qkv, first, H, extra, (bf16_t*)ctx, blocked);
    });
}
