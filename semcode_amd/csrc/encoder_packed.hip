// encoder_packed.hip -- the position-aware kernels of the encoder forward on PACKED variable-length rows (gfx950).
//
// A packed batch holds its sequences one after another: sequence i owns the token rows [starts[i], starts[i] + ceil32(lens[i])),
// the total is rounded up to the 256 rows of a GEMM tile (sc_encoder.cpp plans the layout on the host).  The GEMMs, the LayerNorm
// kernel and the gate kernels treat every row alike and run unchanged; only four steps know where a sequence begins:
//
//   embed_*_packed_kernel       position from a per-row array instead of token % S
//   rope_qk_packed_kernel       likewise
//   attention_packed_kernel     one workgroup per (sequence, group of query blocks) x 64-column block (a head of 64, a pair of heads
//                               of 32), read from a table of work items
//   mean_pool_*_packed_kernel   rows starts[b] .. starts[b] + lens[b] instead of b * S ..
//
// Each shares its device body with the rectangle kernel of encoder_ops.hip (encoder_rows.h, attention_core.h): same arithmetic,
// same reduction orders (relative to the start of the sequence), same statistics conventions.  Alignment rows (lens[i] .. ceil32(lens[i]) of a sequence) carry token 0:
// they are embedded, attended as queries (their keys are masked) and never pooled; the tail rows up to the 256-row multiple are
// zero rows with zero statistics, as the padding rows of a rectangle are.
#include "attention_core.h"
#include "encoder_ops.h"
#include "encoder_rows.h"
#include "gemm_tile.h"

// ------------------------------------------------------------------ embeddings, rotary positions
// The bodies are encoder_rows.h's, shared with the rectangle kernels; here a row's position comes from pos[row] (clamped into the
// model's table) instead of row % S.  Statistics conventions of embed_raw_kernel: slot 0 holds the sums of the rounded row, the tail
// rows tokens .. tokens_pad are zero rows with statistics (0, 0).
__global__ __launch_bounds__(256) void embed_ln_packed_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos, int tokens, int H, int vocab,
                                                               int max_pos, const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                               const float* __restrict__ temb, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    embed_ln_rows(ids, tokens, PosArray{pos, max_pos}, H, vocab, max_pos, wemb, pemb, temb, gamma, beta, eps, out);
}
__global__ __launch_bounds__(256) void embed_raw_packed_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos, int tokens, int tokens_pad,
                                                                int H, int vocab, int max_pos, const float* __restrict__ wemb,
                                                                const float* __restrict__ pemb, const float* __restrict__ temb,
                                                                bf16_t* __restrict__ out, float* __restrict__ stats, int slots) {
    embed_raw_rows(ids, tokens, tokens_pad, PosArray{pos, max_pos}, H, vocab, max_pos, wemb, pemb, temb, out, stats, slots);
}
__global__ __launch_bounds__(256) void rope_qk_packed_kernel(bf16_t* __restrict__ qkv, int64_t M, int nblocks, const int32_t* __restrict__ pos, int max_pos,
                                                              const float* __restrict__ cos_t, const float* __restrict__ sin_t) {
    rope_qk_rows(qkv, M, nblocks, PosArray{pos, max_pos}, cos_t, sin_t);
}

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
    const float slope2 = HEAD::slope2(extra, head);
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
        if (nkt == KT && (slen & 31) == 0) HEAD::template fold<KT, true, GKMAX>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
        else HEAD::template fold<KT, false, GKMAX>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
    }
    if (live) HEAD::store(st, xch, ostg, ctx + ((size_t)start + (size_t)qb * 32) * H + head * 64, H, lane);
}

// ------------------------------------------------------------------ masked mean pooling
// encoder_rows.h's bodies over the rows starts[b] .. starts[b] + lens[b]; blockIdx.x = sequence (up to 65 536 of them), blockIdx.y =
// the 256-column block of the two sliced forms
__global__ __launch_bounds__(256) void mean_pool_packed_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ starts, const int32_t* __restrict__ lens,
                                                                int H, int normalize, float* __restrict__ out) {
    mean_pool_rows(x, PackedRows{starts, lens}, blockIdx.x, H, normalize, out);
}
__global__ __launch_bounds__(256) void mean_pool_sliced_packed_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ starts,
                                                                       const int32_t* __restrict__ lens, int H, float* __restrict__ out) {
    mean_pool_sliced_rows(x, PackedRows{starts, lens}, blockIdx.x, blockIdx.y, H, out);
}
__global__ __launch_bounds__(256) void mean_pool_ln_packed_kernel(const bf16_t* __restrict__ y, const float* __restrict__ stats, int slots, int tokens_pad,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                   const int32_t* __restrict__ starts, const int32_t* __restrict__ lens, int H,
                                                                   float* __restrict__ out) {
    mean_pool_ln_rows(y, stats, slots, tokens_pad, gamma, beta, eps, PackedRows{starts, lens}, blockIdx.x, blockIdx.y, H, out);
}

// ------------------------------------------------------------------ launchers
void sc_launch_embed_ln_packed(const int32_t* ids, const int32_t* pos, int tokens, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                               const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    hipLaunchKernelGGL(embed_ln_packed_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, s, ids, pos, tokens, H, vocab, max_pos, wemb, pemb, temb, g, b,
                       eps, (bf16_t*)out);
}
void sc_launch_embed_raw_packed(const int32_t* ids, const int32_t* pos, int tokens, int tokens_pad, int H, int vocab, int max_pos, const float* wemb,
                                const float* pemb, const float* temb, void* out, float* stats, int slots, hipStream_t s) {
    hipLaunchKernelGGL(embed_raw_packed_kernel, dim3((unsigned)((tokens_pad + 3) / 4)), dim3(256), 0, s, ids, pos, tokens, tokens_pad, H, vocab, max_pos, wemb,
                       pemb, temb, (bf16_t*)out, stats, slots);
}
void sc_launch_rope_qk_packed(void* qkv, int64_t M, int nblocks, const int32_t* pos, int max_pos, const float* cos_t, const float* sin_t, hipStream_t s) {
    int64_t blocks = ((int64_t)nblocks * M * 4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(rope_qk_packed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)qkv, M, nblocks, pos, max_pos, cos_t, sin_t);
}
int sc_packed_attention_class(int len) { return len > 256 ? 0 : (len > 128 ? 1 : 2); }
template <class HEAD>
static void launch_attention_packed(const void* qkv, const int32_t* items, const int* nitems, int H, typename HEAD::Extra extra, void* ctx, int blocked, hipStream_t s) {
    attn_packed_classes(items, nitems, [&](auto cls, const int32_t* first, int n) {
        constexpr int KT = 16 >> decltype(cls)::value, NW = KT >= 8 ? 8 : 4;  // 16 / 8 / 4 key tiles
        attn_launch<attention_packed_kernel<HEAD, KT, NW>, attn_lds_bytes(KT, NW)>(dim3((unsigned)n, (unsigned)(H / 64)), NW * 64, s, (const bf16_t*)qkv, first, H, extra,
                                                                                    (bf16_t*)ctx, blocked);
    });
}
void sc_launch_attention_packed(const void* qkv, const int32_t* items, const int* nitems, int H, const float* slopes, void* ctx, hipStream_t s, int blocked,
                                int head_dim) {
    if (head_dim == 32) launch_attention_packed<Head32>(qkv, items, nitems, H, Head32::Extra(), ctx, blocked, s);
    else if (slopes) launch_attention_packed<Head64<true>>(qkv, items, nitems, H, slopes, ctx, blocked, s);
    else launch_attention_packed<Head64<false>>(qkv, items, nitems, H, nullptr, ctx, blocked, s);
}
void sc_launch_mean_pool_packed(const void* x, const int32_t* starts, const int32_t* lens, int B, int H, int normalize, float* out, hipStream_t s) {
    if (!normalize && (H % 8) == 0)
        hipLaunchKernelGGL(mean_pool_sliced_packed_kernel, dim3((unsigned)B, (unsigned)((H + 255) / 256)), dim3(256), 0, s, (const bf16_t*)x, starts, lens, H, out);
    else
        hipLaunchKernelGGL(mean_pool_packed_kernel, dim3((unsigned)B), dim3(256), 0, s, (const bf16_t*)x, starts, lens, H, normalize, out);
}
void sc_launch_mean_pool_ln_packed(const void* y, const float* stats, int slots, int tokens_pad, const float* gamma, const float* beta, float eps,
                                   const int32_t* starts, const int32_t* lens, int B, int H, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mean_pool_ln_packed_kernel, dim3((unsigned)B, (unsigned)((H + 255) / 256)), dim3(256), 0, s, (const bf16_t*)y, stats, slots, tokens_pad,
                       gamma, beta, eps, starts, lens, H, out);
}
