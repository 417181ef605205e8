// encoder_window.hip -- local (sliding-window) attention of the pre-norm encoder family (ModernBERT), head dimension 64 (gfx950).
//
// In a local layer a token attends to the real keys within hw = local_window / 2 positions of its own (|i - j| <= hw, j < len),
// hw <= 64.  The band of a 32-row query block then touches at most five 32-key tiles, whatever the length of the text: a
// 2 048-token text costs a query block 160 keys instead of 2 048.  The global kernels (encoder_ops.hip, encoder_packed.hip)
// stage every key of the sequence and multiply all of them; here
//
//   * a workgroup of NW waves takes NW consecutive query blocks of one (sequence, head), one block per wave, and stages ONLY
//     the K / V rows those blocks can see: tiles max(0, 32 qb0 - hw) / 32 .. (min(len, 32 (qb0 + NW) + hw) - 1) / 32, at most
//     NW + 4 of them (384 keys for 8 blocks).  That is one LDS segment: no segment loop, no carried softmax state, one barrier;
//   * a wave folds the (at most five) tiles of its own band in a single softmax pass (attention_qblock_window, attention_core.h:
//     the arithmetic of attention_qblock_core per (query, key) plus the band mask) and skips every other staged tile with
//     wave-uniform bounds;
//   * LDS images, swizzles, Q fragments, the output staging and store are those of attention_kernel.
//
// Two forms share the body: rectangles [B, S] (grid = heads x B x groups of NW query blocks) and packed variable-length rows (the
// work-item table of encoder_packed.hip: one item per 8 query blocks for texts longer than 256 tokens, one item otherwise).  Three
// instantiations, chosen by the rectangle's S or the item's class -- i.e. by the text's own length only, so a text's result does
// not depend on its batch-mates:
//   up to 128 keys : 4 tiles staged,  4 waves,  37 KiB LDS
//   up to 256 keys : 8 tiles staged,  8 waves,  73 KiB LDS
//   longer         : 12 tiles staged, 8 waves, 105 KiB LDS, one workgroup per 8 query blocks
// Rows of a rectangle at or beyond len are queries too (alignment and padding rows): their keys are masked like everybody's, a
// row that sees no key at all is written as zeros.  Nothing is ever NaN, so a later layer's P V over such a row stays finite.
#include "attention_core.h"
#include "encoder_ops.h"
#include "gemm_tile.h"

// start: first token row of the sequence, len its real length (>= 1), qb0 the workgroup's first 32-row query block, nqb the query
// blocks of the sequence that exist as rows (S / 32, or ceil32(len) / 32 of packed rows)
template <int KTS, int NW>
static __device__ __forceinline__ void attention_window_body(const bf16_t* __restrict__ qkv, int start, int len, int qb0, int nqb, int head, int H, int hw,
                                                             bf16_t* __restrict__ ctx, int blocked, char* smem) {
    char* Kl = smem;
    char* Vl = smem + KTS * 32 * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * KTS * 32 * 128) + w * 32;
    char* ostg = smem + 2 * KTS * 32 * 128 + NW * 128 + w * 1024;
    const int qb = qb0 + w;       // this wave's query block
    const bool live = qb < nqb;   // wave-uniform
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nh = (size_t)(H >> 6);  // blocked = the row count (M) of the projection that wrote the blocks
    const bf16_t* base = blocked ? qkv + ((size_t)head * T + (size_t)start) * 64 : qkv + (size_t)start * ld + head * 64;
    const size_t koff = blocked ? nh * T * 64 : (size_t)H, voff = 2 * koff;

    // ---- the key tiles this workgroup's query blocks can see: [kt0, kt0 + n)
    const int qlast = (qb0 + NW < nqb ? qb0 + NW : nqb) * 32;  // one past the last query row of the workgroup
    const int klo = qb0 * 32 - hw > 0 ? qb0 * 32 - hw : 0;
    const int khi = qlast + hw < len ? qlast + hw : len;        // one past the last visible real key
    const int kt0 = klo >> 5;
    int n = ((khi + 31) >> 5) - kt0;
    n = n < 0 ? 0 : (n > KTS ? KTS : n);
    n = __builtin_amdgcn_readfirstlane(n);
    const bf16_t* kbase = base + (size_t)kt0 * 32 * ld;
    for (int piece = w; piece < n * 4; piece += NW) {  // pieces of 8 rows x 128 B = 1 KiB
        const int p = piece * 64 + lane;
        const int r = p >> 3, ck = (p & 7) ^ ((r >> 1) & 7);
        __builtin_amdgcn_global_load_lds((gbl_vptr)(kbase + (size_t)r * ld + koff + ck * 8), (lds_vptr)(Kl + piece * 1024), 16, 0, 0);
    }
    for (int piece = w; piece < n * 4; piece += NW) {
        const int p = piece * 64 + lane;
        const int r = p >> 3, cv = (p & 7) ^ (((r >> 1) & 1) << 2);
        __builtin_amdgcn_global_load_lds((gbl_vptr)(kbase + (size_t)r * ld + voff + cv * 8), (lds_vptr)(Vl + piece * 1024), 16, 0, 0);
    }
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[4];
    if (live) {
        const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!live) return;

    // ---- this wave's band: tiles [lo, lo + nt), nt <= 5 because hw <= 64
    const int lo = (qb * 32 - hw > 0 ? qb * 32 - hw : 0) >> 5;
    const int last = qb * 32 + 31 + hw < len - 1 ? qb * 32 + 31 + hw : len - 1;  // last visible real key
    int nt = (last >> 5) - lo + 1;
    if (lo - kt0 + nt > n) nt = n - (lo - kt0);  // never beyond what was staged
    nt = nt < 0 ? 0 : (nt > 5 ? 5 : nt);
    nt = __builtin_amdgcn_readfirstlane(nt);
    AttnState st;
    attn_state_init(st);
    attention_qblock_window<5>(qf, Kl, Vl, len, hw, lane, qb * 32, lo, lo - kt0, nt, st);
    attn_state_store(st, xch, ostg, ctx + ((size_t)start + (size_t)qb * 32) * H + head * 64, H, lane);
}

template <int KTS, int NW>
__global__ __launch_bounds__(NW * 64, (KTS <= 8 ? 2 : 1)) void attention_window_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int S, int H,
                                                                                         int hw, bf16_t* __restrict__ ctx, int blocked) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int head = blockIdx.x, b = blockIdx.y;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    attention_window_body<KTS, NW>(qkv, b * S, len, (int)blockIdx.z * NW, S >> 5, head, H, hw, ctx, blocked, smem);
}

template <int KTS, int NW>
__global__ __launch_bounds__(NW * 64, (KTS <= 8 ? 2 : 1)) void attention_window_packed_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ items,
                                                                                                int H, int hw, bf16_t* __restrict__ ctx, int blocked) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int head = blockIdx.y;
    const int32_t* it = items + 4 * (size_t)blockIdx.x;
    const int start = __builtin_amdgcn_readfirstlane(it[0]);
    int len = it[1];
    len = len < 1 ? 1 : (len > KTS * 32 && KTS < 12 ? KTS * 32 : len);  // (an item of a short class never holds a longer text)
    len = __builtin_amdgcn_readfirstlane(len);
    const int qb0 = __builtin_amdgcn_readfirstlane(it[2]);
    attention_window_body<KTS, NW>(qkv, start, len, qb0, (len + 31) >> 5, head, H, hw, ctx, blocked, smem);
}

// ------------------------------------------------------------------ launchers
bool sc_attention_window_supported(int local_window) { return local_window >= 2 && local_window <= 128 && (local_window & 1) == 0; }

template <int KTS, int NW>
static void launch_window(const void* qkv, const int32_t* lens, int B, int S, int H, int hw, void* ctx, int blocked, hipStream_t s) {
    const dim3 grid((unsigned)(H / 64), (unsigned)B, (unsigned)((S / 32 + NW - 1) / NW));
    attn_launch<attention_window_kernel<KTS, NW>, attn_lds_bytes(KTS, NW)>(grid, NW * 64, s, (const bf16_t*)qkv, lens, S, H, hw, (bf16_t*)ctx, blocked);
}
void sc_launch_attention_window(const void* qkv, const int32_t* lens, int B, int S, int H, int local_window, void* ctx, hipStream_t s, int blocked) {
    const int hw = local_window / 2;
    if (S <= 128) launch_window<4, 4>(qkv, lens, B, S, H, hw, ctx, blocked, s);
    else if (S <= 256) launch_window<8, 8>(qkv, lens, B, S, H, hw, ctx, blocked, s);
    else launch_window<12, 8>(qkv, lens, B, S, H, hw, ctx, blocked, s);
}
void sc_launch_attention_window_packed(const void* qkv, const int32_t* items, const int* nitems, int H, int local_window, void* ctx, hipStream_t s, int blocked) {
    const int hw = local_window / 2;
    attn_packed_classes(items, nitems, [&](auto cls, const int32_t* first, int n) {
        constexpr int KTS = decltype(cls)::value == 0 ? 12 : (decltype(cls)::value == 1 ? 8 : 4), NW = KTS >= 8 ? 8 : 4;  // 12 / 8 / 4 tiles staged
        attn_launch<attention_window_packed_kernel<KTS, NW>, attn_lds_bytes(KTS, NW)>(dim3((unsigned)n, (unsigned)(H / 64)), NW * 64, s, (const bf16_t*)qkv, first, H, hw,
                                                                                       (bf16_t*)ctx, blocked);
    });
}
