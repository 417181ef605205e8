// encoder_causal.hip -- the kernels of the pre-norm causal decoder family (cfg.arch 2: Qwen2 / Qwen2.5 embedding models), gfx950:
// causal grouped-query attention, RMSNorm, last-token pooling.
//
//   attention_causal_kernel         MFMA + LDS : a query attends to the real keys at or before its own position (key <= query, key < len).
//   attention_causal_packed_kernel               A workgroup of NW waves takes NW consecutive 32-row query blocks of one (sequence, query
//                                                head), one block per wave, and stages ONLY the key tiles at or below its last block's
//                                                diagonal (and below len): tiles 0 .. min(qb0 + NW, ceil(len / 32)) - 1, in LDS segments of
//                                                KTS tiles with the softmax state carried from segment to segment as attention_long_kernel
//                                                does.  A wave folds the tiles up to its OWN diagonal (attention_qblock_causal,
//                                                attention_core.h) and skips the rest of a segment with wave-uniform bounds: a 2 048-token
//                                                text costs about half the MFMAs of the global kernel.  LDS images, swizzles, Q fragments,
//                                                output staging and store are those of attention_kernel.
//                                                Grouped-query layout: query head h reads K / V head h / (heads / kv_heads); the heads of
//                                                a group re-read their K / V head from L2.  qkv rows are [Q (heads) | K (kv_heads) |
//                                                V (kv_heads)] x 64 columns, row-major or in 64-column blocks [(heads + 2 kv_heads)][M][64].
//   rmsnorm_kernel                  HBM-bound  : x * rsqrt(mean(x^2) + eps) * gamma, bf16 rows in and out, f32 statistics, 16-byte loads and
//                                                stores, half a wave per row with the next row's loads in flight (layernorm_kernel's walk)
//   last_rows_kernel                1 wave/text: the row of the text's last real token (start + len - 1), RMSNorm in f32, optional L2
//                                                normalisation by the rule of the mean kernels -> f32 [B, H]
//
// Keys are folded in groups of four tiles counted from key 0 whatever the segment size, and a query block's tiles depend on its own
// position and the text's length only: the bits of a text's rows do not depend on the rectangle's S, on the packed launch class or on
// its batch-mates.  Rows of a rectangle at or beyond len, and alignment rows of packed texts, are queries too: they see key 0 at least.
//
// Both kernels are templates on NB, the 64-column blocks of a head: 1 (head dimension 64) or 2 (cfg.head_dim 128: Qwen3-Embedding,
// Qwen2.5-1.5B) -- one shell, one set of rules for tiles, groups of four, masks, grids and bits.  At NB 2 a head is two consecutive
// 64-column blocks; a key tile is 8 KiB of K and 8 KiB of V, each staged as two of the 64-wide images (low half, high half of the head);
// a wave holds 8 Q fragments, the score tile of a (query block, key tile) is 8 MFMA steps, the output four 32 x 32 tiles.  With 160 KiB
// of LDS a 128-wide segment is at most 8 tiles.  The instantiations <NB, KTS, NW>, by the rectangle's S or the packed item's class
// (sc_packed_items):
//   head dimension 64
//     up to 128 keys : <1, 4, 4>   segments of 4 tiles,  4 waves,  37 KiB LDS
//     up to 256 keys : <1, 8, 8>   segments of 8 tiles,  8 waves,  73 KiB LDS
//     longer         : <1, 16, 8>  segments of 16 tiles, 8 waves, 137 KiB LDS, one workgroup per 8 query blocks
//   head dimension 128
//     up to 128 keys : <2, 4, 4>   segments of 4 tiles, 4 waves,  72.5 KiB LDS (64 KiB of K / V + 4 x 128 B exchange + 4 x 2 KiB output
//                                  block), 204 VGPRs, two workgroups a CU
//     longer         : <2, 8, 8>   segments of 8 tiles, 8 waves, 145 KiB LDS (128 KiB + 1 KiB + 16 KiB), 249 VGPRs, one workgroup a CU; a
//                                  text beyond 256 keys walks its segments with the state carried along (packed: one item per 8 query
//                                  blocks, LONG)
// No scratch in any (the compiler's summaries are in profiles/qwen3_kernels.log and profiles/causal_width_kernels.log).
//   qknorm_rope_kernel              HBM-bound  : the per-head RMSNorm of Q and K (cfg.qk_norm) and the rotate-half rotation in one pass over the
//   qknorm_rope_packed_kernel                    blocked QKV buffer, head dimension 64 or 128, 16-byte accesses, one rounding to bf16.  The forward
//                                                calls it when head_dim == 128 or qk_norm; the 64-wide model without QK-norm keeps rope_qk_kernel
#include "attention_core.h"
#include "encoder_ops.h"
#include "encoder_rows.h"  // wave_sum, RectRows / PackedRows, LN_MAXJ
#include "gemm_tile.h"

// start: first token row of the sequence, len its real length (>= 1), qb0 the workgroup's first 32-row query block, nqb the query
// blocks of the sequence that exist as rows (S / 32, or ceil32(len) / 32 of packed rows).  heads / kvh: query heads, K / V heads.
// NB: a head is NB consecutive 64-column blocks of the fused projection, row-major or blocked: block j of a row lies at j * bs, bs = 64
// elements (row-major) or blocked * 64 (64-column blocks).  K and V of a segment are staged as NB 64-wide images each (attention_core.h).
template <int NB, int KTS, int NW>
static __device__ __forceinline__ void attention_causal_body(const bf16_t* __restrict__ qkv, int start, int len, int qb0, int nqb, int head, int heads, int kvh,
                                                             bf16_t* __restrict__ ctx, int blocked, char* smem) {
    constexpr int IMG = KTS * 32 * 128;
    char* Kl = smem;
    char* Vl = smem + NB * IMG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * NB * IMG) + w * 32;
    char* ostg = smem + 2 * NB * IMG + NW * 128 + w * (NB * 1024);
    const int qb = qb0 + w;      // this wave's query block
    const bool live = qb < nqb;  // wave-uniform
    const int kvhead = head / (heads / kvh);  // grouped mapping: consecutive query heads share a K / V head
    const int H = heads * (NB * 64);
    const int ld = blocked ? 64 : (heads + 2 * kvh) * (NB * 64);
    const size_t bs = blocked ? (size_t)blocked * 64 : 64;  // blocked = the row count (M) of the projection that wrote the blocks
    // The same three addresses in two spellings.  At 64 the one the kernels had before they took NB: with row0 + NB * head * bs the packed
    // 8-tile kernel takes one register more (157 against 156, profiles/causal_width_kernels.log); at 128 this one is its text to the letter.
    const bf16_t *qbase, *kbase, *vbase;
    if constexpr (NB == 1) {
        const size_t T = (size_t)blocked;  // the row count (M) of the blocks
        qbase = blocked ? qkv + ((size_t)head * T + (size_t)start) * 64 : qkv + (size_t)start * ld + head * 64;
        kbase = blocked ? qkv + ((size_t)(heads + kvhead) * T + (size_t)start) * 64 : qkv + (size_t)start * ld + (heads + kvhead) * 64;
        vbase = blocked ? qkv + ((size_t)(heads + kvh + kvhead) * T + (size_t)start) * 64 : qkv + (size_t)start * ld + (heads + kvh + kvhead) * 64;
    } else {
        const bf16_t* row0 = qkv + (size_t)start * ld;
        qbase = row0 + (size_t)(NB * head) * bs;
        kbase = row0 + (size_t)(NB * (heads + kvhead)) * bs;
        vbase = row0 + (size_t)(NB * (heads + kvh + kvhead)) * bs;
    }
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[4 * NB];
    if (live) {
        const bf16_t* qrow = qbase + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
        for (int ks = 0; ks < 4 * NB; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + (size_t)(ks >> 2) * bs + 16 * (ks & 3) + 8 * hh);
    }
    const int nrt = (len + 31) >> 5;                          // key tiles holding at least one real key
    const int ntw = qb0 + NW < nrt ? qb0 + NW : nrt;          // tiles this workgroup stages: up to its last block's diagonal
    const int ntq = live ? (qb + 1 < nrt ? qb + 1 : nrt) : 0; // tiles this wave folds: up to its own diagonal
    const int nseg = (ntw + KTS - 1) / KTS;
    AttnStateCausal<NB> st;
    attn_state_init(st);
#pragma unroll 1
    for (int seg = 0; seg < nseg; ++seg) {
        const int t0 = seg * KTS;
        const int nst = ntw - t0 < KTS ? ntw - t0 : KTS;  // tiles staged in this segment
        if (seg) __syncthreads();  // every wave is done with the previous segment's K / V
#pragma unroll
        for (int e = 0; e < NB; ++e) {  // the 64-column blocks of the head: one image each
            for (int piece = w; piece < nst * 4; piece += NW) {  // pieces of 8 rows x 128 B = 1 KiB
                const int p = piece * 64 + lane;
                const int r = p >> 3, ck = (p & 7) ^ ((r >> 1) & 7);
                __builtin_amdgcn_global_load_lds((gbl_vptr)(kbase + e * bs + (size_t)(t0 * 32 + r) * ld + ck * 8), (lds_vptr)(Kl + e * IMG + piece * 1024), 16, 0, 0);
            }
            for (int piece = w; piece < nst * 4; piece += NW) {
                const int p = piece * 64 + lane;
                const int r = p >> 3, cv = (p & 7) ^ (((r >> 1) & 1) << 2);
                __builtin_amdgcn_global_load_lds((gbl_vptr)(vbase + e * bs + (size_t)(t0 * 32 + r) * ld + cv * 8), (lds_vptr)(Vl + e * IMG + piece * 1024), 16, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int nt = ntq - t0;
        nt = nt < 0 ? 0 : (nt > nst ? nst : nt);  // never beyond what was staged
        nt = __builtin_amdgcn_readfirstlane(nt);
        if (nt > 0) attention_qblock_causal<NB, KTS>(qf, Kl, Vl, xch, len, nt, lane, qb * 32, t0 * 32, st);
    }
    if (live) attn_state_store(st, xch, ostg, ctx + ((size_t)start + (size_t)qb * 32) * H + head * (NB * 64), H, lane);
}

template <int NB, int KTS, int NW>
__global__ __launch_bounds__(NW * 64, (KTS <= 4 ? 2 : 1)) void attention_causal_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int S, int heads, int kvh,
                                                                      bf16_t* __restrict__ ctx, int blocked) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int head = blockIdx.x, b = blockIdx.y;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    // the groups of query blocks of a sequence from the last -- the most key tiles -- to the first: the long workgroups start first
    attention_causal_body<NB, KTS, NW>(qkv, b * S, len, (int)(gridDim.z - 1 - blockIdx.z) * NW, S >> 5, head, heads, kvh, ctx, blocked, smem);
}

// LONG: the items are groups of 8 query blocks of texts of any length (the first class of sc_packed_items: 16-tile segments at head
// dimension 64, 8-tile ones at 128).  Else one item per text of at most KTS * 32 tokens.
template <int NB, int KTS, int NW, bool LONG>
__global__ __launch_bounds__(NW * 64, (KTS <= 4 ? 2 : 1)) void attention_causal_packed_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ items, int nitems, int heads,
                                                                             int kvh, bf16_t* __restrict__ ctx, int blocked) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // One grid dimension, the head fastest, the items from the last to the first.  The items of a long text are its groups of 8 query
    // blocks in ascending order, 8 per 2 048 tokens: with the item as the fastest index, workgroup id mod 8 -- the XCD a workgroup lands
    // on -- would be the group's position in its text, i.e. one XCD would get all the groups with the most key tiles.  Heads fastest
    // spreads every item over the XCDs and puts the query heads that share a K / V head next to each other in time.
    // The two short classes have one item per text, nothing to balance: the item is the fastest index there, so that the heads of a
    // text -- 7 of them read the same K / V head -- land on one XCD and find it in that L2 (60 us a launch at 128 x 256 tokens, against 69
    // for the same work as a rectangle, whose grid runs the heads fastest).
    const int head = LONG ? (int)(blockIdx.x % (unsigned)heads) : (int)(blockIdx.x / (unsigned)nitems);
    const int32_t* it = items + 4 * (size_t)(LONG ? nitems - 1 - (int)(blockIdx.x / (unsigned)heads) : (int)(blockIdx.x % (unsigned)nitems));
    const int start = __builtin_amdgcn_readfirstlane(it[0]);
    int len = it[1];
    len = len < 1 ? 1 : (len > KTS * 32 && !LONG ? KTS * 32 : len);  // (an item of a short class never holds a longer text)
    len = __builtin_amdgcn_readfirstlane(len);
    const int qb0 = __builtin_amdgcn_readfirstlane(it[2]);
    attention_causal_body<NB, KTS, NW>(qkv, start, len, qb0, (len + 31) >> 5, head, heads, kvh, ctx, blocked, smem);
}

// ------------------------------------------------------------------ QK-norm + rotation
// Per (row, Q or K head) of the blocked QKV buffer [64-column blocks][M][64], in place: optionally RMSNorm over the head's HD values
// (f32 sum of squares, x * rsqrt(mean + eps) * gamma in f32; Q heads gamma_q, K heads gamma_k), then the rotate-half rotation with the
// pairs (j, j + HD / 2) and the angle p * theta^(-2j / HD) from the table [max_pos][HD / 2], then ONE rounding to bf16.  HBM-bound: a
// lane owns 8 columns of the head's low half and the same 8 of its high half (two 16-byte loads, two 16-byte stores), so both members
// of every pair sit in its registers; HD / 16 lanes per (row, head), their sum of squares combined by 2 or 3 shuffles inside the group.
// At HD 64 the halves are the two halves of one 128-byte block (rope_qk_rows' ownership), at 128 the same columns of the head's two
// blocks, M * 64 elements apart.  nq of the nheads heads are Q heads.  Positions as rope_qk_rows gets them.
template <int HD, bool NORM, class POS>
static __device__ __forceinline__ void qknorm_rope_rows(bf16_t* __restrict__ qkv, int64_t M, int nheads, int nq, POS pos_of, const float* __restrict__ cos_t,
                                                        const float* __restrict__ sin_t, const float* __restrict__ gq, const float* __restrict__ gk, float eps) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int L = HD / 16, HALF = HD / 2;  // lanes per (row, head); columns per half
    const int64_t total = (int64_t)nheads * M * L;  // a multiple of L: the lanes of a group run, or stop, together
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t vec = i / L;  // head * M + row
        const int c = (int)(i % L) * 8;
        const int64_t row = vec % M, head = vec / M;
        const int p = pos_of(row);
        bf16_t* vlo = HD == 64 ? qkv + vec * 64 + c : qkv + (2 * head * M + row) * 64 + c;
        bf16_t* vhi = HD == 64 ? vlo + 32 : vlo + M * 64;
        const u32x4 lo = *reinterpret_cast<const u32x4*>(vlo), hi = *reinterpret_cast<const u32x4*>(vhi);
        float a[8], b[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a[2 * k] = __builtin_bit_cast(float, lo[k] << 16);
            a[2 * k + 1] = __builtin_bit_cast(float, lo[k] & 0xFFFF0000u);
            b[2 * k] = __builtin_bit_cast(float, hi[k] << 16);
            b[2 * k + 1] = __builtin_bit_cast(float, hi[k] & 0xFFFF0000u);
        }
        if (NORM) {
            float sq = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) sq = fmaf(a[k], a[k], sq);
#pragma unroll
            for (int k = 0; k < 8; ++k) sq = fmaf(b[k], b[k], sq);
#pragma unroll
            for (int off = L / 2; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
            const float rstd = 1.0f / sqrtf(sq * (1.0f / (float)HD) + eps);
            const float* g = head < nq ? gq : gk;
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(g + c), g1 = *reinterpret_cast<const f32x4*>(g + c + 4);
            const f32x4 h0 = *reinterpret_cast<const f32x4*>(g + HALF + c), h1 = *reinterpret_cast<const f32x4*>(g + HALF + c + 4);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a[k] = a[k] * rstd * (k < 4 ? g0[k & 3] : g1[k & 3]);
                b[k] = b[k] * rstd * (k < 4 ? h0[k & 3] : h1[k & 3]);
            }
        }
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cos_t + (size_t)p * HALF + c), c1 = *reinterpret_cast<const f32x4*>(cos_t + (size_t)p * HALF + c + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sin_t + (size_t)p * HALF + c), s1 = *reinterpret_cast<const f32x4*>(sin_t + (size_t)p * HALF + c + 4);
        u32x4 olo, ohi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float cc0 = k < 2 ? c0[2 * k] : c1[2 * k - 4], cc1 = k < 2 ? c0[2 * k + 1] : c1[2 * k - 3];
            const float ss0 = k < 2 ? s0[2 * k] : s1[2 * k - 4], ss1 = k < 2 ? s0[2 * k + 1] : s1[2 * k - 3];
            olo[k] = pack_bf16x2(fmaf(a[2 * k], cc0, -b[2 * k] * ss0), fmaf(a[2 * k + 1], cc1, -b[2 * k + 1] * ss1));
            ohi[k] = pack_bf16x2(fmaf(b[2 * k], cc0, a[2 * k] * ss0), fmaf(b[2 * k + 1], cc1, a[2 * k + 1] * ss1));
        }
        *reinterpret_cast<u32x4*>(vlo) = olo;
        *reinterpret_cast<u32x4*>(vhi) = ohi;
    }
}
template <int HD, bool NORM>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(bf16_t* __restrict__ qkv, int64_t M, int nheads, int nq, int smask, const float* __restrict__ cos_t,
                                                           const float* __restrict__ sin_t, const float* __restrict__ gq, const float* __restrict__ gk, float eps) {
    qknorm_rope_rows<HD, NORM>(qkv, M, nheads, nq, PosMasked{smask}, cos_t, sin_t, gq, gk, eps);
}
template <int HD, bool NORM>
__global__ __launch_bounds__(256) void qknorm_rope_packed_kernel(bf16_t* __restrict__ qkv, int64_t M, int nheads, int nq, const int32_t* __restrict__ pos, int max_pos,
                                                                  const float* __restrict__ cos_t, const float* __restrict__ sin_t, const float* __restrict__ gq,
                                                                  const float* __restrict__ gk, float eps) {
    qknorm_rope_rows<HD, NORM>(qkv, M, nheads, nq, PosArray{pos, max_pos}, cos_t, sin_t, gq, gk, eps);
}

// ------------------------------------------------------------------ RMSNorm
// layernorm_kernel's walk (encoder_ops.hip): half a wave per row, lane l of the half owns the 16-byte chunks l, l + 32, ... of the row,
// workgroups stride over the rows with the next row's loads in flight.  One half-wave reduction: the sum of squares.
template <int NC>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const bf16_t* __restrict__ in, int tokens, int H, const float* __restrict__ gamma, float eps,
                                                       bf16_t* __restrict__ out) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int l32 = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    f32x4 g[NC][2];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int k0 = (l32 + 32 * j) * 8;
        if (k0 < H) {
            g[j][0] = *reinterpret_cast<const f32x4*>(gamma + k0);
            g[j][1] = *reinterpret_cast<const f32x4*>(gamma + k0 + 4);
        }
    }
    const float inv_h = 1.0f / (float)H;
    u32x4 nxt[NC];
    int tok = wave * 2 + half;
    if (tok < tokens) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int k0 = (l32 + 32 * j) * 8;
            if (k0 < H) nxt[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + (size_t)tok * H + k0));
        }
    }
    for (int base = wave * 2; base < tokens; base += nwaves * 2) {
        tok = base + half;
        const bool live = tok < tokens;
        u32x4 raw[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) raw[j] = nxt[j];
        const int ntok = tok + nwaves * 2;
        if (ntok < tokens) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int k0 = (l32 + 32 * j) * 8;
                if (k0 < H) nxt[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + (size_t)ntok * H + k0));
            }
        }
        float v[NC][8];
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const bool on = live && (l32 + 32 * j) * 8 < H;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[j][2 * c] = on ? __builtin_bit_cast(float, raw[j][c] << 16) : 0.f;
                v[j][2 * c + 1] = on ? __builtin_bit_cast(float, raw[j][c] & 0xFFFF0000u) : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) sq = fmaf(v[j][c], v[j][c], sq);
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
        const float rstd = 1.0f / sqrtf(sq * inv_h + eps);
        if (live) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int k0 = (l32 + 32 * j) * 8;
                if (k0 < H) {
                    u32x4 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float lo = v[j][2 * c] * rstd * g[j][c >> 1][(2 * c) & 3];
                        const float hi = v[j][2 * c + 1] * rstd * g[j][c >> 1][(2 * c + 1) & 3];
                        r[c] = pack_bf16x2(lo, hi);
                    }
                    *reinterpret_cast<u32x4*>(out + (size_t)tok * H + k0) = r;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ last-token pooling
// The row of every text's last real token: RMSNorm (gamma, f32), then L2 normalisation by the rule of mean_pool_rows.
template <class ROWS>
static __device__ __forceinline__ void last_rows(const bf16_t* __restrict__ x, ROWS rows, int B, int H, const float* __restrict__ gamma, float eps, int normalize,
                                                 float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bf16_t* p = x + (rows.first(b) + (size_t)(rows.len(b) - 1)) * H;
    float v[LN_MAXJ][4];
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[j][c] = 0.f;
        if (k0 < H) {
            const u16x4 raw = *reinterpret_cast<const u16x4*>(p + k0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[j][c] = bf16_to_f32(raw[c]);
                sq = fmaf(v[j][c], v[j][c], sq);
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)H + eps);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (k0 < H) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[j][c] = v[j][c] * rstd * gamma[k0 + c];
            ss += (v[j][0] * v[j][0] + v[j][1] * v[j][1]) + (v[j][2] * v[j][2] + v[j][3] * v[j][3]);
        }
    }
    const float scale = normalize ? 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f) : 1.0f;
#pragma unroll
    for (int j = 0; j < LN_MAXJ; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (k0 < H) *reinterpret_cast<f32x4*>(out + (size_t)b * H + k0) = f32x4{v[j][0] * scale, v[j][1] * scale, v[j][2] * scale, v[j][3] * scale};
    }
}
__global__ __launch_bounds__(256) void last_rows_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ lens, int S, int B, int H,
                                                         const float* __restrict__ gamma, float eps, int normalize, float* __restrict__ out) {
    last_rows(x, RectRows{lens, S}, B, H, gamma, eps, normalize, out);
}
__global__ __launch_bounds__(256) void last_rows_packed_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ starts, const int32_t* __restrict__ lens,
                                                                int B, int H, const float* __restrict__ gamma, float eps, int normalize, float* __restrict__ out) {
    last_rows(x, PackedRows{starts, lens}, B, H, gamma, eps, normalize, out);
}

// ------------------------------------------------------------------ launchers
bool sc_attention_causal_supported(int heads, int kv_heads, int head_dim) {
    return (head_dim == 64 || head_dim == 128) && heads >= 1 && heads * head_dim <= 2048 && kv_heads >= 1 && kv_heads <= heads && heads % kv_heads == 0;
}

template <int HD, bool NORM>
static void launch_qknorm_rope(void* qkv, int64_t M, int nheads, int nq, int S, const int32_t* pos, int max_pos, const float* cos_t, const float* sin_t, const float* gq,
                               const float* gk, float eps, hipStream_t s) {
    int64_t blocks = ((int64_t)nheads * M * (HD / 16) + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    const dim3 grid((unsigned)blocks), block(256);
    if (pos) hipLaunchKernelGGL((qknorm_rope_packed_kernel<HD, NORM>), grid, block, 0, s, (bf16_t*)qkv, M, nheads, nq, pos, max_pos, cos_t, sin_t, gq, gk, eps);
    else hipLaunchKernelGGL((qknorm_rope_kernel<HD, NORM>), grid, block, 0, s, (bf16_t*)qkv, M, nheads, nq, S - 1, cos_t, sin_t, gq, gk, eps);
}
void sc_launch_qknorm_rope(void* qkv, int64_t M, int heads, int kv_heads, int head_dim, int S, const int32_t* pos, int max_pos, const float* cos_t, const float* sin_t,
                           const float* gq, const float* gk, float eps, hipStream_t s) {
    const int nh = heads + kv_heads;
    const bool norm = gq != nullptr;
    if (head_dim == 128) {
        if (norm) launch_qknorm_rope<128, true>(qkv, M, nh, heads, S, pos, max_pos, cos_t, sin_t, gq, gk, eps, s);
        else launch_qknorm_rope<128, false>(qkv, M, nh, heads, S, pos, max_pos, cos_t, sin_t, gq, gk, eps, s);
    } else {
        if (norm) launch_qknorm_rope<64, true>(qkv, M, nh, heads, S, pos, max_pos, cos_t, sin_t, gq, gk, eps, s);
        else launch_qknorm_rope<64, false>(qkv, M, nh, heads, S, pos, max_pos, cos_t, sin_t, gq, gk, eps, s);
    }
}

template <int NB, int KTS, int NW>
static void launch_causal(const void* qkv, const int32_t* lens, int B, int S, int heads, int kvh, void* ctx, int blocked, hipStream_t s) {
    const dim3 grid((unsigned)heads, (unsigned)B, (unsigned)((S / 32 + NW - 1) / NW));
    attn_launch<attention_causal_kernel<NB, KTS, NW>, attn_lds_bytes(KTS, NW, NB)>(grid, NW * 64, s, (const bf16_t*)qkv, lens, S, heads, kvh, (bf16_t*)ctx, blocked);
}
void sc_launch_attention_causal(const void* qkv, const int32_t* lens, int B, int S, int heads, int kv_heads, int head_dim, void* ctx, hipStream_t s, int blocked) {
    if (head_dim == 128) {
        if (S <= 128) launch_causal<2, 4, 4>(qkv, lens, B, S, heads, kv_heads, ctx, blocked, s);
        else launch_causal<2, 8, 8>(qkv, lens, B, S, heads, kv_heads, ctx, blocked, s);
    } else {
        if (S <= 128) launch_causal<1, 4, 4>(qkv, lens, B, S, heads, kv_heads, ctx, blocked, s);
        else if (S <= 256) launch_causal<1, 8, 8>(qkv, lens, B, S, heads, kv_heads, ctx, blocked, s);
        else launch_causal<1, 16, 8>(qkv, lens, B, S, heads, kv_heads, ctx, blocked, s);
    }
}
template <int NB>
static void launch_causal_packed(const void* qkv, const int32_t* items, const int* nitems, int heads, int kvh, void* ctx, int blocked, hipStream_t s) {
    attn_packed_classes(items, nitems, [&](auto cls, const int32_t* first, int n) {
        // texts beyond 256 tokens (items of 8 query blocks), up to 256, up to 128: segments of 16 / 8 / 4 tiles at 64, 8 / 8 / 4 at 128
        constexpr int C = decltype(cls)::value, KTS = C == 2 ? 4 : (C == 0 && NB == 1 ? 16 : 8), NW = KTS >= 8 ? 8 : 4;
        attn_launch<attention_causal_packed_kernel<NB, KTS, NW, C == 0>, attn_lds_bytes(KTS, NW, NB)>(dim3((unsigned)n * (unsigned)heads), NW * 64, s, (const bf16_t*)qkv, first, n,
                                                                                                     heads, kvh, (bf16_t*)ctx, blocked);
    });
}
void sc_launch_attention_causal_packed(const void* qkv, const int32_t* items, const int* nitems, int heads, int kv_heads, int head_dim, void* ctx, hipStream_t s, int blocked) {
    if (head_dim == 128) launch_causal_packed<2>(qkv, items, nitems, heads, kv_heads, ctx, blocked, s);
    else launch_causal_packed<1>(qkv, items, nitems, heads, kv_heads, ctx, blocked, s);
}
void sc_launch_rmsnorm(const void* in, int tokens, int H, const float* g, float eps, void* out, hipStream_t s) {
    int blocks = (tokens + 7) / 8;  // 8 rows per workgroup per sweep
    if (blocks > 256 * 8) blocks = 256 * 8;
    const dim3 grid((unsigned)blocks), block(256);
    if (H <= 768) hipLaunchKernelGGL(rmsnorm_kernel<3>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, eps, (bf16_t*)out);
    else if (H <= 1024) hipLaunchKernelGGL(rmsnorm_kernel<4>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, eps, (bf16_t*)out);
    else hipLaunchKernelGGL(rmsnorm_kernel<8>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, eps, (bf16_t*)out);
}
void sc_launch_last_pool(const void* x, const int32_t* starts, const int32_t* lens, int B, int S, int H, const float* gamma, float eps, int normalize, float* out,
                         hipStream_t s) {
    const dim3 grid((unsigned)((B + 3) / 4));
    if (starts) hipLaunchKernelGGL(last_rows_packed_kernel, grid, dim3(256), 0, s, (const bf16_t*)x, starts, lens, B, H, gamma, eps, normalize, out);
    else hipLaunchKernelGGL(last_rows_kernel, grid, dim3(256), 0, s, (const bf16_t*)x, lens, S, B, H, gamma, eps, normalize, out);
}
