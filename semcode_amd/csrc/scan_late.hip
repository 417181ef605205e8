// scan_late.hip -- late interaction over the token store of an index (gfx950): the rerank that reads stored token vectors instead of
// running the passages' forward (sc_index_rerank_late), the exhaustive MaxSim search (sc_index_search_late) and the gather of a
// compaction (sc_index_compact_tokens).  Store: sc_tokens.cpp; rules: maxsim_rule.h, late_rule.h.
//
// Replaces (reference): nothing -- the reference embeds one vector per chunk and reranks with nothing; late-interaction libraries keep the
// token vectors in a torch tensor and score with a padded einsum + max + sum.
//
// Roofline of the scan: a document token costs 2 nq W FLOP on the f32 MFMA (155 TF measured on MI355X) against 4 W (fmt 0) or 2 W (fmt 1)
// bytes of HBM (6.3 TB/s achievable): the two cross at nq = 49 (f32) / 25 (bf16) -- f32 storage is memory-bound up to there, bf16
// storage compute-bound from nq = 32 on.  Measured fractions: profiles/late_store_bench.log.
//
// late_rerank_kernel<FMT>   the sibling of maxsim_kernel (encoder_tokens.hip; that kernel is untouched): one workgroup per (question,
//                           candidate), the same tiles, the same v_mfma_f32_16x16x4_f32 chain, maxima under maxsim_key, the ordered sum
//                           by one lane.  The document's tokens come through the table (64-bit pool offsets) and are widened from bf16
//                           in registers at FMT 1.  A padding candidate (-1) or a row without tokens scores -inf.
// late_scan_kernel<NT, FMT> one question per launch, NT = W / 16.  The question's tokens sit in LDS in fragment order: the 16-byte piece
//                           lane (r16, g) feeds to the MFMA for (query tile qt, step t) is s_q[(qt NT + t) 64 + lane], so a wave's
//                           ds_read_b128 is 1 KiB contiguous and conflict-free.  Query tiles come in pairs (an odd count repeats the
//                           last token: never read back), so that two independent accumulator chains keep the MFMA issuing (32-cycle
//                           issue against 40-cycle dependent latency).
//                           Work: blocks of LATE_BLOCK_ROWS rows, handed out in row order by one integer atomic per block (a counter
//                           the host zeroes before the launch): documents have 1 .. 2 048 tokens, and blocks of 16 dealt by static
//                           striding left the grid waiting for its slowest wave (15.5 ms where this takes 11.1, nq = 128:
//                           profiles/late_store_bench.log).  The counter decides which wave scores a row, never a result.  A wave's
//                           lanes fetch the block's table entries at once -- a row's allow bit is tested before its entry, its entry
//                           before its tokens -- and the wave then walks the rows that have tokens, one document at a time, in tiles of 16
//                           tokens: lane (r16, g) loads floats 16 t + 4 g + c of token 16 dt + r16 straight from global memory (the
//                           next tile, of this document or the next, is in flight while this one multiplies), one running maximum
//                           key per query tile in registers, tokens at or beyond len (loads clamped to the last token) left out.  A
//                           document ends with the xor butterfly 16, 32 over g and the ordered sum, wave-uniform, then its key
//                           (late_hit_key) enters the wave's sorted list of k keys in LDS: every lane moves its one or two slots.
//                           Keys are distinct (the row is part of them) and sc_launch_topk_merge is exact, so the result does not
//                           depend on the partition of rows over waves.  No atomic touches a score or a list.
// late_gather_kernel        one wave per row: the row's len W elements from the old pool to its place in the new one, 16 bytes per lane.
// late_install_kernel<FMT>  the put whose vectors are on the device already (sc_index_put_tokens_dev): f32 token vectors, in order or through
//                           a gather list, to the pool's tail -- copied at FMT 0, rounded by late_round_bf16 at FMT 1.  16-byte loads,
//                           16- or 8-byte stores, a grid-stride loop over a grid capped by the CU count.  HBM-bound: 4 W bytes read and
//                           4 W or 2 W written per token.  No atomics, no LDS.
// Registers and scratch: profiles/late_store_kernels.log, profiles/late_ingest_kernels.log.
#include "sc_common.h"  // (first: the HIP runtime header, whose bit casts maxsim_rule.h uses)
#include "late_rule.h"

#define LATE_BLOCK_ROWS 4

template <int FMT> struct LateRaw { typedef f32x4 T; };
template <> struct LateRaw<1> { typedef uint2 T; };

// four consecutive elements of the pool at element offset e (a multiple of 4)
template <int FMT>
static __device__ __forceinline__ typename LateRaw<FMT>::T late_load_raw(const void* __restrict__ pool, int64_t e) {
    if constexpr (FMT == 0) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(pool) + e);
    else return *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(pool) + e);
}
static __device__ __forceinline__ f32x4 late_widen(const f32x4& r) { return r; }
static __device__ __forceinline__ f32x4 late_widen(const uint2& r) {
    return f32x4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xFFFF0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xFFFF0000u)};
}

template <int FMT>
__global__ __launch_bounds__(256) void late_rerank_kernel(const float* __restrict__ Q, const int32_t* __restrict__ q_off, const void* __restrict__ pool,
                                                           const sc_tok_entry* __restrict__ table, const int64_t* __restrict__ cand, int C, int W,
                                                           float* __restrict__ out) {
    __shared__ uint32_t s_key[4][MAXSIM_MAX_NQ];
    __shared__ float s_m[MAXSIM_MAX_NQ];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int p = blockIdx.x;
    const int qi = p / C;
    const int64_t row = cand[p];
    int nd = 0;
    int64_t d0 = 0;
    if (row >= 0) {
        const sc_tok_entry e = table[row];
        nd = e.len;
        d0 = e.start;
    }
    if (nd < 1) {  // (the whole workgroup: padding, or a row without tokens)
        if (tid == 0) out[p] = -__builtin_inff();
        return;
    }
    const int q0 = q_off[qi];
    int nq = q_off[qi + 1] - q0;
    if (nq > MAXSIM_MAX_NQ) nq = MAXSIM_MAX_NQ;  // (the host refuses longer questions)
    const float* Qp = Q + (size_t)q0 * W;
    const int nqt = (nq + 15) >> 4, ndt = (nd + 15) >> 4, steps = W >> 4;

    for (int qt = 0; qt < nqt; ++qt) {
        const int tq = min(16 * qt + r16, nq - 1);  // (columns at or beyond nq repeat the last token and are never read)
        const f32x4* __restrict__ xb = reinterpret_cast<const f32x4*>(Qp + (size_t)tq * W) + g;
        uint32_t best = MAXSIM_KEY_NONE;
        for (int dt = wv; dt < ndt; dt += 4) {
            const int td = min(16 * dt + r16, nd - 1);
            const int64_t ea = (d0 + td) * (int64_t)W + 4 * g;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < steps; ++t) {
                const f32x4 a = late_widen(late_load_raw<FMT>(pool, ea + 16 * t)), b = xb[4 * t];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], acc, 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (16 * dt + 4 * g + c < nd) best = maxsim_key_max(best, maxsim_key(acc[c]));
        }
        best = maxsim_key_max(best, (uint32_t)__shfl_xor((int)best, 16));
        best = maxsim_key_max(best, (uint32_t)__shfl_xor((int)best, 32));
        if (g == 0) s_key[wv][16 * qt + r16] = best;
    }
    __syncthreads();
    if (tid < nq) s_m[tid] = maxsim_unkey(maxsim_key_max(maxsim_key_max(s_key[0][tid], s_key[1][tid]), maxsim_key_max(s_key[2][tid], s_key[3][tid])));
    __syncthreads();
    if (tid == 0) {
        float acc = 0.0f;
        for (int t = 0; t < nq; ++t) acc = maxsim_add(acc, s_m[t]);
        out[p] = acc;
    }
}

struct LateScanArgs {
    const float* Q;             // [nq][W] of this question
    int nq;
    const void* pool;
    const sc_tok_entry* table;  // [n]
    int64_t n;
    const uint32_t* allow;      // bitset over rows, or NULL
    int k;
    uint64_t* partial;          // [gridDim.x * 4][k]
    unsigned* next_block;       // the next block of rows to hand out (0 at launch)
};

static __device__ __forceinline__ int64_t late_readlane64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <int NT, int FMT>
__global__ __launch_bounds__(256) void late_scan_kernel(LateScanArgs a) {
    typedef typename LateRaw<FMT>::T Raw;
    extern __shared__ __attribute__((aligned(16))) unsigned char late_lds[];
    constexpr int W = 16 * NT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int nq = a.nq, k = a.k;
    const int nqt = (nq + 15) >> 4, nqt2 = (nqt + 1) & ~1;
    f32x4* s_q = reinterpret_cast<f32x4*>(late_lds);                                       // [nqt2][NT][64]
    uint64_t* s_list = reinterpret_cast<uint64_t*>(late_lds + (size_t)nqt2 * NT * 1024);  // [4][k]

    for (int i = tid; i < nqt2 * NT * 64; i += 256) {
        const int l = i & 63, t = (i >> 6) % NT, qt = i / (64 * NT);
        const int tok = min(16 * qt + (l & 15), nq - 1);
        s_q[i] = *reinterpret_cast<const f32x4*>(a.Q + (size_t)tok * W + 16 * t + 4 * (l >> 4));
    }
    for (int i = tid; i < 4 * k; i += 256) s_list[i] = SC_KEY_MAX;
    __syncthreads();

    volatile uint64_t* L = s_list + (size_t)w * k;
    const f32x4* __restrict__ qfrag = s_q + lane;
    const int64_t blocks = (a.n + LATE_BLOCK_ROWS - 1) / LATE_BLOCK_ROWS;
    uint32_t best[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i] = MAXSIM_KEY_NONE;

    for (;;) {
        unsigned claimed = 0;
        if (lane == 0) claimed = atomicAdd(a.next_block, 1u);
        const int64_t b = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)claimed);
        if (b >= blocks) break;
        // ---- the block's rows: allow bit, then table entry
        const int64_t row = b * LATE_BLOCK_ROWS + lane;
        bool ok = lane < LATE_BLOCK_ROWS && row < a.n;
        if (ok && a.allow) ok = (a.allow[row >> 5] >> (row & 31)) & 1u;
        int64_t start = 0;
        int len = 0;
        if (ok) {
            const sc_tok_entry e = a.table[row];
            start = e.start;
            len = e.len;
        }
        uint64_t todo = __ballot(ok && len > 0);
        // ---- (document, tile) pairs in order; the tile after the current one is loaded before the current one multiplies
        int j_n = 0, len_n = 0, dt_n = 0;
        int64_t start_n = 0;
        bool have = todo != 0;
        Raw nxt[NT];
        if (have) {
            j_n = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            start_n = late_readlane64(start, j_n);
            len_n = __builtin_amdgcn_readlane(len, j_n);
            const int64_t e = (start_n + min(r16, len_n - 1)) * (int64_t)W + 4 * g;
#pragma unroll
            for (int t = 0; t < NT; ++t) nxt[t] = late_load_raw<FMT>(a.pool, e + 16 * t);
        }
        while (have) {
            f32x4 av[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) av[t] = late_widen(nxt[t]);
            const int cj = j_n, clen = len_n, cdt = dt_n;
            const bool last = 16 * (cdt + 1) >= clen;
            if (!last) {
                dt_n = cdt + 1;
            } else if (todo) {
                j_n = (int)__builtin_ctzll(todo);
                todo &= todo - 1;
                start_n = late_readlane64(start, j_n);
                len_n = __builtin_amdgcn_readlane(len, j_n);
                dt_n = 0;
            } else {
                have = false;
            }
            if (have) {
                const int64_t e = (start_n + min(16 * dt_n + r16, len_n - 1)) * (int64_t)W + 4 * g;
#pragma unroll
                for (int t = 0; t < NT; ++t) nxt[t] = late_load_raw<FMT>(a.pool, e + 16 * t);
            }
            // ---- this tile against every query tile, two chains at a time
#pragma unroll
            for (int qp = 0; qp < 4; ++qp) {
                if (2 * qp < nqt) {
                    const f32x4* __restrict__ b0p = qfrag + (size_t)(2 * qp) * NT * 64;
                    const f32x4* __restrict__ b1p = b0p + NT * 64;
                    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const f32x4 b0 = b0p[t * 64], b1 = b1p[t * 64];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][c], b0[c], acc0, 0, 0, 0);
                            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][c], b1[c], acc1, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (16 * cdt + 4 * g + c < clen) {
                            best[2 * qp] = maxsim_key_max(best[2 * qp], maxsim_key(acc0[c]));
                            best[2 * qp + 1] = maxsim_key_max(best[2 * qp + 1], maxsim_key(acc1[c]));
                        }
                }
            }
            if (!last) continue;
            // ---- the document is complete: m_t over the four k groups, the ordered sum (wave-uniform), the wave's list
            float acc = 0.0f;
#pragma unroll
            for (int qt = 0; qt < 8; ++qt) {
                if (qt < nqt) {
                    uint32_t m = best[qt];
                    m = maxsim_key_max(m, (uint32_t)__shfl_xor((int)m, 16));
                    m = maxsim_key_max(m, (uint32_t)__shfl_xor((int)m, 32));
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (16 * qt + r < nq) acc = maxsim_add(acc, maxsim_unkey((uint32_t)__builtin_amdgcn_readlane((int)m, r)));
                }
                best[qt] = MAXSIM_KEY_NONE;
            }
            const uint64_t key = late_hit_key(acc, (uint32_t)(b * LATE_BLOCK_ROWS + cj));
            if (key < L[k - 1]) {  // (wave-uniform) slot p becomes: itself if it is before the key, the key if its left neighbour is, else that neighbour
                const int p0 = lane, p1 = lane + 64;
                const uint64_t c0 = p0 < k ? L[p0] : SC_KEY_MAX, l0 = p0 > 0 && p0 < k ? L[p0 - 1] : 0ull;
                const uint64_t c1 = p1 < k ? L[p1] : SC_KEY_MAX, l1 = p1 < k ? L[p1 - 1] : 0ull;
                if (p0 < k && c0 > key) L[p0] = l0 < key ? key : l0;
                if (p1 < k && c1 > key) L[p1] = l1 < key ? key : l1;
            }
        }
    }
    __syncthreads();
    uint64_t* out = a.partial + (size_t)blockIdx.x * 4 * k;
    for (int i = tid; i < 4 * k; i += 256) out[i] = s_list[i];
}

static size_t late_scan_lds_bytes(int nq, int W, int k) {
    const int nqt2 = (((nq + 15) >> 4) + 1) & ~1;
    return (size_t)nqt2 * (W / 16) * 1024 + (size_t)4 * k * sizeof(uint64_t);
}

// workgroups of one question's pass over n rows on `cus` compute units: up to three per CU (the registers' limit at W = 128) while the LDS
// allows it, never more than the blocks need
int sc_late_scan_workgroups(int64_t n, int nq, int W, int k, int cus) {
    const int64_t blocks = (n + LATE_BLOCK_ROWS - 1) / LATE_BLOCK_ROWS, want = (blocks + 3) / 4;
    int per_cu = (int)(((size_t)160 * 1024) / late_scan_lds_bytes(nq, W, k));
    per_cu = per_cu < 1 ? 1 : per_cu > 3 ? 3 : per_cu;
    const int64_t cap = (int64_t)cus * per_cu;
    return (int)(want < 1 ? 1 : want > cap ? cap : want);
}

static ScDeviceOnce g_late_attr_once;

template <int FMT>
static const void* late_scan_fn(int nt) {
    switch (nt) {
#define LATE_SCAN_CASE(NT) \
    case NT: return reinterpret_cast<const void*>(late_scan_kernel<NT, FMT>);
        LATE_SCAN_CASE(1) LATE_SCAN_CASE(2) LATE_SCAN_CASE(3) LATE_SCAN_CASE(4) LATE_SCAN_CASE(5) LATE_SCAN_CASE(6) LATE_SCAN_CASE(7) LATE_SCAN_CASE(8)
#undef LATE_SCAN_CASE
    }
    return nullptr;
}

void sc_launch_late_scan(const float* Q, int nq, const void* pool, int fmt, const sc_tok_entry* table, int64_t n, const uint32_t* allow, int W, int k, int nwg,
                         uint64_t* partial, unsigned* next_block, hipStream_t s) {
    if (nq < 1 || nq > MAXSIM_MAX_NQ || k < 1 || k > LATE_MAX_K || nwg < 1 || !maxsim_width_ok(W) || (fmt != 0 && fmt != 1)) return;  // (the host checks these first)
    sc_device_once(g_late_attr_once, [&] {
        for (int nt = 1; nt <= 8; ++nt) {
            hipFuncSetAttribute(late_scan_fn<0>(nt), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
            hipFuncSetAttribute(late_scan_fn<1>(nt), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024);
        }
    });
    LateScanArgs a;
    a.Q = Q; a.nq = nq; a.pool = pool; a.table = table; a.n = n; a.allow = allow; a.k = k; a.partial = partial; a.next_block = next_block;
    const size_t lds = late_scan_lds_bytes(nq, W, k);
    const dim3 grid((unsigned)nwg), block(256);
    switch (W / 16) {
#define LATE_SCAN_CASE(NT)                                                                          \
    case NT:                                                                                        \
        if (fmt == 0) hipLaunchKernelGGL((late_scan_kernel<NT, 0>), grid, block, lds, s, a);        \
        else hipLaunchKernelGGL((late_scan_kernel<NT, 1>), grid, block, lds, s, a);                 \
        break;
        LATE_SCAN_CASE(1) LATE_SCAN_CASE(2) LATE_SCAN_CASE(3) LATE_SCAN_CASE(4) LATE_SCAN_CASE(5) LATE_SCAN_CASE(6) LATE_SCAN_CASE(7) LATE_SCAN_CASE(8)
#undef LATE_SCAN_CASE
    }
}

void sc_launch_late_rerank(const float* Q, const int32_t* q_off, int Bq, const void* pool, int fmt, const sc_tok_entry* table, const int64_t* cand, int C, int W,
                           float* out, hipStream_t s) {
    if (Bq < 1 || C < 1 || !maxsim_width_ok(W)) return;
    const dim3 grid((unsigned)((size_t)Bq * C)), block(256);
    if (fmt == 0) hipLaunchKernelGGL(late_rerank_kernel<0>, grid, block, 0, s, Q, q_off, pool, table, cand, C, W, out);
    else hipLaunchKernelGGL(late_rerank_kernel<1>, grid, block, 0, s, Q, q_off, pool, table, cand, C, W, out);
}

// row r: old_pool[old_tab[r].start ...] -> new_pool[new_tab[r].start ...], new_tab[r].len tokens of tok_bytes (a multiple of 32) each
__global__ __launch_bounds__(256) void late_gather_kernel(const sc_tok_entry* __restrict__ old_tab, const sc_tok_entry* __restrict__ new_tab, int64_t n,
                                                           const unsigned char* __restrict__ old_pool, unsigned char* __restrict__ new_pool, int tok_bytes) {
    const int lane = threadIdx.x & 63;
    const int64_t GW = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += GW) {
        const sc_tok_entry ne = new_tab[r];
        if (ne.len < 1) continue;
        const int64_t pieces = (int64_t)ne.len * tok_bytes / 16;
        const u32x4_t* __restrict__ src = reinterpret_cast<const u32x4_t*>(old_pool + old_tab[r].start * (int64_t)tok_bytes);
        u32x4_t* __restrict__ dst = reinterpret_cast<u32x4_t*>(new_pool + ne.start * (int64_t)tok_bytes);
        for (int64_t i = lane; i < pieces; i += 64) dst[i] = src[i];
    }
}

void sc_launch_late_gather(const sc_tok_entry* old_tab, const sc_tok_entry* new_tab, int64_t n, const void* old_pool, void* new_pool, int tok_bytes, int cus, hipStream_t s) {
    if (n < 1) return;
    const int64_t want = (n + 3) / 4, cap = (int64_t)cus * 8;
    hipLaunchKernelGGL(late_gather_kernel, dim3((unsigned)(want > cap ? cap : want)), dim3(256), 0, s, old_tab, new_tab, n, (const unsigned char*)old_pool,
                       (unsigned char*)new_pool, tok_bytes);
}

// token j of the put: the f32 vector vecs[src ? src[j] : j] -> dst + j W elements in the pool's format.  A lane moves one piece of four
// consecutive floats: the pieces of the `total` tokens form one flat range, so a wave's 64 loads (and stores) are contiguous wherever
// src is ascending, whatever W.  FMT 1 rounds each float once by late_round_bf16, the rule sc_index_put_tokens applies on the host.
template <int FMT>
__global__ __launch_bounds__(256) void late_install_kernel(const float* __restrict__ vecs, const int32_t* __restrict__ src, int64_t total, int W, void* __restrict__ dst) {
    const int ppt = W >> 2;  // pieces per token
    const int64_t pieces = total * ppt, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += stride) {
        const int64_t j = i / ppt;
        const int p = (int)(i - j * ppt);
        const int64_t from = src ? (int64_t)src[j] : j;
        const f32x4 v = *reinterpret_cast<const f32x4*>(vecs + from * W + 4 * p);
        if constexpr (FMT == 0) {
            reinterpret_cast<f32x4*>(dst)[i] = v;
        } else {
            const uint32_t h0 = late_round_bf16(v[0]), h1 = late_round_bf16(v[1]), h2 = late_round_bf16(v[2]), h3 = late_round_bf16(v[3]);
            reinterpret_cast<uint2*>(dst)[i] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
        }
    }
}

void sc_launch_late_install(const float* vecs, const int32_t* src, int64_t total, int W, int fmt, void* dst, int cus, hipStream_t s) {
    if (total < 1 || !maxsim_width_ok(W) || (fmt != 0 && fmt != 1)) return;  // (the host checks these first)
    const int64_t want = (total * (W >> 2) + 255) / 256, cap = (int64_t)cus * 8;
    const dim3 grid((unsigned)(want > cap ? cap : want)), block(256);
    if (fmt == 0) hipLaunchKernelGGL(late_install_kernel<0>, grid, block, 0, s, vecs, src, total, W, dst);
    else hipLaunchKernelGGL(late_install_kernel<1>, grid, block, 0, s, vecs, src, total, W, dst);
}
