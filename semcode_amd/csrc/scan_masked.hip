// scan_masked.hip -- the masked search's device side (gfx950 / CDNA4): a per-call bitset over row ids compacted into the list of
// allowed stored positions, and the exact scan of scan_exact.hip fed from that list instead of a row range.
//
// Replaces (reference): nothing on the server side -- the reference filters AFTER retrieval (src/semcode/frontend/app.py:100-116 drops the hits
// of an unfiltered top-k that fail the repo / language filter), so a small repo in a large collection usually shows no source.
//
// Roofline: HBM.  Algorithmic bytes = m * ld * 4 per pass of <= qt queries for m allowed rows: a filter that passes 1 % of the
// corpus reads 1 % of it.  mask_compact adds one pass over the position map (4 B per stored row, trained IVF_FLAT only) and over
// the bitset.
//
// mask_compact (three small kernels, no atomics, the order of sel is decided by position alone):
//   mask_flags_kernel   a workgroup takes 2 048 consecutive stored positions: position p is allowed when bit perm[p] of the bitset
//                       is set (p < perm_rows: list-major IVF storage) or bit p (beyond, and without a position map).  Ballots give
//                       the bitset over POSITIONS (flags) and the workgroup's popcount.
//   mask_scan_kernel    exclusive scan of the popcounts in place (one workgroup), the total m behind them.  The host reads m.
//   mask_scatter_kernel the same 2 048 positions again: allowed position -> sel[offset of the workgroup + rank inside it].
//                       sel is padded with position 0 (always a stored row) to a multiple of 16 entries.
//
// scan_gather_kernel is the resident-query form of scan_exact_kernel -- same XOR swizzle through the source address, same 4-deep
// private LDS ring per wave ordered by counted vmcnt, same MFMA chain per (row, query) in the canonical k order of
// oracle/sc_oracle.c, same threshold / append / rank-sort compaction, same flush into partial[grp][wg][slot][k] for topk_merge.hip
// -- with three differences:
//   * tile ordinal t covers sel[16 t .. 16 t + 15]; a slot at or beyond m (the padding) streams row 0 and its score is dropped;
//   * the row base of every LDS-DMA piece and of the norm load come from those entries; the reported ids come through the norm
//     piece as before (lanes 16-31): perm[position] below perm_rows, else the sel entry itself;
//   * the 16 entries of a tile reach the wave as ONE scalar load (64 B, wave-uniform address, constant address space) issued when
//     the PREVIOUS tile's first stage is requested, a whole tile ahead of their first use.  Scalar loads count on lgkmcnt, so they
//     neither enter the vmcnt queue that orders the ring nor make the compiler drain it; each lane then picks its five entries
//     (four piece rows, one norm row) with selects.  A dependent sel -> address -> row chain per stage would pay the HBM latency
//     once per stage.
// Long rows: the queries are resident, so ld > ~1400 floats holds fewer than 16 of them (3 072-d: 6) and a batch of 16 takes three
// passes over the allowed rows; the streamed-query variant of scan_exact.hip is not carried over.
// wave_compact and the LDS layout are copies of scan_exact.hip's (static there; the tuned kernel's file is left untouched).
#include "sc_common.h"

#define GS_WAVES 4
#define GS_NSTAGE 4
#define GS_NORM_SLOTS 4
#define GS_STAGE_BYTES 4096
#define GS_NORM_BYTES 256
#define GS_QPAD 8  // floats

typedef __attribute__((address_space(3))) void* lds_vptr;
typedef const __attribute__((address_space(1))) void* gbl_vptr;
// volatile accesses must carry the LDS address space explicitly (scan_exact.hip): a FLAT access counts on vmcnt and would drain the ring
typedef __attribute__((address_space(3))) volatile uint64_t* lds_u64p;
typedef __attribute__((address_space(3))) volatile unsigned* lds_u32p;
typedef unsigned u32x16_t __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) u32x16_t* const_u32x16p;  // constant address space: a uniform load becomes s_load_dwordx16

// ------------------------------------------------------------------ mask_compact

// (every load is unconditional -- clamped indices instead of branches -- so that the eight positions of a thread are in flight together)
template <bool HAS_PERM>
__global__ __launch_bounds__(256) void mask_flags_kernel(const uint32_t* __restrict__ allow, int64_t n, const uint32_t* __restrict__ perm, int64_t perm_rows,
                                                          uint64_t* __restrict__ flags, uint32_t* __restrict__ cnt) {
    constexpr int IT = SC_MASK_BLOCK_ROWS / 256;
    __shared__ unsigned wave_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * SC_MASK_BLOCK_ROWS;
    const int64_t nwords = (n + 63) >> 6;
    uint32_t r[IT], aw[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int64_t p = base + it * 256 + tid;
        const int64_t pc = p < n ? p : 0;
        r[it] = (uint32_t)pc;
        if (HAS_PERM) {
            const uint32_t v = perm[pc < perm_rows ? pc : 0];
            r[it] = pc < perm_rows ? v : (uint32_t)pc;
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) aw[it] = allow[((int64_t)r[it] < n ? r[it] : 0u) >> 5];
    unsigned count = 0;
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int64_t p = base + it * 256 + tid;
        const bool on = p < n && (int64_t)r[it] < n && ((aw[it] >> (r[it] & 31)) & 1u);
        const uint64_t word = __ballot(on);
        const int64_t wi = (base + it * 256 + w * 64) >> 6;
        if (lane == 0 && wi < nwords) flags[wi] = word;
        count += (unsigned)__popcll(word);
    }
    if (lane == 0) wave_cnt[w] = count;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// cnt [nb] -> exclusive scan in place, cnt[nb] = total (m <= n < 2^32)
__global__ __launch_bounds__(1024) void mask_scan_kernel(uint32_t* __restrict__ cnt, int64_t nb) {
    __shared__ unsigned wave_sum[16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned carry = 0;
    for (int64_t base = 0; base < nb; base += 1024) {
        const int64_t i = base + tid;
        const unsigned v = i < nb ? cnt[i] : 0u;
        unsigned x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[w] = x;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned sj = wave_sum[j];
            before += j < w ? sj : 0u;
            total += sj;
        }
        if (i < nb) cnt[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) cnt[nb] = carry;
}

__global__ __launch_bounds__(256) void mask_scatter_kernel(const uint64_t* __restrict__ flags, const uint32_t* __restrict__ cnt, int64_t n, int64_t nb,
                                                            uint32_t* __restrict__ sel) {
    constexpr int WORDS = SC_MASK_BLOCK_ROWS / 64;  // 32: lane j < 32 of every wave holds word j of the workgroup and the popcount below it
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t nwords = (n + 63) >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * WORDS;
    const uint64_t mine = (lane < WORDS && w0 + lane < nwords) ? flags[w0 + lane] : 0ull;
    const unsigned pc = (unsigned)__popcll(mine);
    unsigned incl = pc;
#pragma unroll
    for (int d = 1; d < WORDS; d <<= 1) {
        const unsigned y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    const unsigned below = cnt[blockIdx.x] + incl - pc;
#pragma unroll
    for (int it = 0; it < SC_MASK_BLOCK_ROWS / 256; ++it) {
        const int j = it * 4 + w;  // this wave's word of the step
        const uint64_t word = ((uint64_t)(unsigned)__shfl((int)(mine >> 32), j) << 32) | (unsigned)__shfl((int)mine, j);
        const unsigned pre = (unsigned)__shfl((int)below, j);
        if ((word >> lane) & 1ull) sel[(size_t)pre + (unsigned)__popcll(word & ((1ull << lane) - 1ull))] = (uint32_t)((w0 + j) * 64 + lane);
    }
    if (blockIdx.x == 0 && tid < 16) {  // padding: a stored row that is safe to stream; the scan drops slots at or beyond m
        const int64_t m = cnt[nb], i = m + tid;
        if (i < ((m + 15) & ~(int64_t)15)) sel[i] = 0u;
    }
}

void sc_launch_mask_count(const uint32_t* allow, int64_t n, const uint32_t* perm, int64_t perm_rows, uint64_t* flags, uint32_t* cnt, hipStream_t s) {
    const int64_t nb = sc_mask_blocks(n);
    if (nb <= 0) return;
    if (perm && perm_rows > 0) hipLaunchKernelGGL(mask_flags_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, allow, n, perm, perm_rows, flags, cnt);
    else hipLaunchKernelGGL(mask_flags_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, allow, n, perm, (int64_t)0, flags, cnt);
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, nb);
}

void sc_launch_mask_scatter(const uint64_t* flags, const uint32_t* cnt, int64_t n, uint32_t* sel, hipStream_t s) {
    const int64_t nb = sc_mask_blocks(n);
    if (nb <= 0) return;
    hipLaunchKernelGGL(mask_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, s, flags, cnt, n, nb, sel);
}

// ------------------------------------------------------------------ the gathered scan

struct GatherArgs {
    const float* X;
    const float* xnorm;
    int ld;
    const float* Qp;
    const float* qnorm;
    int Q;
    int qt;
    int k;
    int cap;
    int tiles_per_wg;
    uint64_t* partial;
    const uint32_t* perm;  // stored position -> reported row id below perm_rows; NULL / beyond: the position is the id
    int64_t perm_rows;
    const uint32_t* sel;   // [m rounded up to 16] allowed stored positions, ascending
    int64_t m;
};

struct GatherLds {
    unsigned ring, norms, qs, qn, thr, cnt, cand, tmp, total;
};
// scan_exact.hip scan_lds_layout, resident queries, no probe ranges (sc_scan_exact_plan sized qt and cap for it)
__host__ __device__ static inline GatherLds gather_lds_layout(int ld, int qt, int cap) {
    GatherLds L;
    unsigned o = 0;
    L.ring = o; o += GS_WAVES * GS_NSTAGE * GS_STAGE_BYTES;
    L.norms = o; o += GS_WAVES * GS_NORM_SLOTS * GS_NORM_BYTES;
    L.qs = o; o += (unsigned)qt * (unsigned)(ld + GS_QPAD) * 4u;
    L.qn = o; o += 64;
    L.thr = o; o += GS_WAVES * 16 * 8;
    L.cnt = o; o += GS_WAVES * 16 * 4;
    L.cand = o; o += (unsigned)GS_WAVES * (unsigned)qt * (unsigned)cap * 8u;
    L.tmp = o; o += (unsigned)GS_WAVES * (unsigned)cap * 8u;
    L.total = o;
    return L;
}

// Rank-sort the n (<= cap) candidate keys of one query slot, keep the k smallest in order, refresh the pruning threshold
// (scan_exact.hip wave_compact: one whole wave, all traffic through volatile LDS).
static __device__ __forceinline__ void gs_wave_compact(lds_u64p cand, lds_u64p tmp, lds_u32p cnt, lds_u64p thr, int k, int lane) {
    const int n = (int)*cnt;
    if (n <= 64) {
        const uint64_t key = lane < n ? cand[lane] : SC_KEY_MAX;
        const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint64_t kj = ((uint64_t)(unsigned)__builtin_amdgcn_readlane((int)khi, j) << 32) | (unsigned)__builtin_amdgcn_readlane((int)klo, j);
            rank += kj < key ? 1 : 0;
        }
        if (lane < n && rank < k) cand[rank] = key;  // keys are unique (row id in the low word): ranks are a permutation
        if (n >= k && lane < n && rank == k - 1) *thr = key;
        if (lane == 0) *cnt = (unsigned)(n < k ? n : k);
        return;
    }
    for (int e = lane; e < n; e += 64) {
        const uint64_t key = cand[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (cand[j] < key) ? 1 : 0;
        if (rank < k) tmp[rank] = key;
    }
    const int m = n < k ? n : k;
    for (int e = lane; e < m; e += 64) cand[e] = tmp[e];
    if (lane == 0) {
        *cnt = (unsigned)m;
        if (n >= k) *thr = tmp[k - 1];
    }
}

static __device__ __forceinline__ unsigned gs_pick4(unsigned a, unsigned b, unsigned c, unsigned d, int i) {
    const unsigned lo = (i & 1) ? b : a, hi = (i & 1) ? d : c;
    return (i & 2) ? hi : lo;
}

template <int METRIC>
__global__ __launch_bounds__(256) void scan_gather_kernel(GatherArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15;  // A row / B column (query slot)
    const int g = lane >> 4;    // k-group
    const GatherLds L = gather_lds_layout(a.ld, a.qt, a.cap);
    const int ld = a.ld;
    const int spt = ld >> 6;  // stages per tile
    const int grp = blockIdx.y;
    const int q0 = grp * a.qt;
    const int nq = min(a.qt, a.Q - q0);

    // ---- queries -> LDS (once), thresholds / counters
    {
        const int qstride = ld + GS_QPAD;
        float* qs = reinterpret_cast<float*>(smem + L.qs);
        for (int c = 0; c < a.qt; ++c) {
            const bool have = c < nq;
            const float* src = a.Qp + (int64_t)(q0 + (have ? c : 0)) * ld;
            for (int kk = tid * 4; kk < ld; kk += 1024) {
                f32x4 v = have ? *reinterpret_cast<const f32x4*>(src + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(qs + c * qstride + kk) = v;
            }
        }
        if (tid < 16) reinterpret_cast<float*>(smem + L.qn)[tid] = (tid < nq) ? a.qnorm[q0 + tid] : 1.0f;
        if (tid < GS_WAVES * 16) {
            reinterpret_cast<uint64_t*>(smem + L.thr)[tid] = SC_KEY_MAX;
            reinterpret_cast<unsigned*>(smem + L.cnt)[tid] = 0u;
        }
    }
    __syncthreads();

    // ---- this wave's tiles of sel: wg range [t0, t1), wave takes t0 + w, t0 + w + 4, ...
    const int64_t total_tiles = (a.m + 15) >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * a.tiles_per_wg;
    int64_t t1 = t0 + a.tiles_per_wg;
    if (t1 > total_tiles) t1 = total_tiles;
    int ntiles = 0;
    if (t0 + w < t1) ntiles = (int)((t1 - (t0 + w) + GS_WAVES - 1) / GS_WAVES);
    const int total_stages = ntiles * spt;

    char* ring = smem + L.ring + w * (GS_NSTAGE * GS_STAGE_BYTES);
    char* nrm = smem + L.norms + w * (GS_NORM_SLOTS * GS_NORM_BYTES);
    const char* qsb = smem + L.qs + (size_t)(r16 < a.qt ? r16 : a.qt - 1) * (size_t)(ld + GS_QPAD) * 4u + (size_t)g * 16u;
    lds_u64p thr_w = (lds_u64p)(smem + L.thr) + w * 16;
    lds_u32p cnt_w = (lds_u32p)(smem + L.cnt) + w * 16;
    lds_u64p cand_w = (lds_u64p)(smem + L.cand) + w * a.qt * a.cap;
    lds_u64p tmp_w = (lds_u64p)(smem + L.tmp) + w * a.cap;
    const float qn_mine = reinterpret_cast<const float*>(smem + L.qn)[r16];

    // issue side: (tile, k-chunk) of the next stage to request
    int iss = 0, iss_tile = 0, iss_kc = 0, iss_slot = 0;
    // per-lane source geometry of one LDS-DMA piece: row-in-piece = lane>>4, slot = lane&15
    const int prow = lane >> 4, pslot = lane & 15;
    // the 16 sel entries of a tile as one scalar load; `ahead` holds those of the tile whose first stage is requested next
    const_u32x16p selc = (const_u32x16p)(uintptr_t)a.sel;
    u32x16_t ahead = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ntiles > 0) ahead = selc[t0 + w];
    unsigned piece_row[4] = {0, 0, 0, 0};  // this lane's stored position for piece p of the tile being requested: entry 4 p + prow

    auto issue_stage = [&]() {
        const int slot = iss_slot;
        if (++iss_slot == GS_NSTAGE) iss_slot = 0;
        if (iss_kc == 0) {
            const int64_t ord = t0 + w + (int64_t)iss_tile * GS_WAVES;
            const u32x16_t e = ahead;
            if (iss_tile + 1 < ntiles) ahead = selc[ord + GS_WAVES];
#pragma unroll
            for (int p = 0; p < 4; ++p) piece_row[p] = gs_pick4(e[4 * p], e[4 * p + 1], e[4 * p + 2], e[4 * p + 3], prow);
            const unsigned mine = gs_pick4(gs_pick4(e[0], e[1], e[2], e[3], r16), gs_pick4(e[4], e[5], e[6], e[7], r16), gs_pick4(e[8], e[9], e[10], e[11], r16),
                                           gs_pick4(e[12], e[13], e[14], e[15], r16), r16 >> 2);  // entry r16
            // tile norms first (older than the tile's data in the vmcnt queue), one dword per lane: lanes 0-15 the 16 row norms, lanes
            // 16-31 the 16 reported row ids -- the candidate path never touches global memory
            const float* nsrc = a.xnorm + mine;
            if ((lane & 48) == 16)
                nsrc = (int64_t)mine < a.perm_rows ? reinterpret_cast<const float*>(a.perm + mine) : reinterpret_cast<const float*>(a.sel + (ord << 4) + r16);
            __builtin_amdgcn_global_load_lds((gbl_vptr)nsrc, (lds_vptr)(nrm + (iss_tile & (GS_NORM_SLOTS - 1)) * GS_NORM_BYTES), 4, 0, 0);
        }
        char* dst = ring + slot * GS_STAGE_BYTES;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = 4 * p + prow;
            const float* src = a.X + (int64_t)piece_row[p] * (int64_t)ld + (iss_kc << 6) + ((pslot ^ r) << 2);
            __builtin_amdgcn_global_load_lds((gbl_vptr)src, (lds_vptr)(dst + p * 1024), 16, 0, 2);
        }
        ++iss;
        if (++iss_kc == spt) { iss_kc = 0; ++iss_tile; }
    };

#pragma unroll 1
    for (int j = 0; j < GS_NSTAGE - 1; ++j)
        if (iss < total_stages) issue_stage();

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int con_tile = 0, con_kc = 0, con_slot = 0;
#pragma unroll 1
    for (int si = 0; si < total_stages; ++si) {
        if (iss < total_stages) issue_stage();
        // younger stages in flight behind stage si: each is >= 4 LDS-DMA instructions
        const int pend = iss - si - 1;
        if (pend >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else if (pend == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (pend == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const char* st = ring + con_slot * GS_STAGE_BYTES + r16 * 256;
        f32x4 av[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) av[t] = *reinterpret_cast<const f32x4*>(st + (((4 * t + g) ^ r16) << 4));
        const char* qb = qsb + (size_t)con_kc * 256u;
        if (++con_slot == GS_NSTAGE) con_slot = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(qb + t * 64);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][c], bv[c], acc, 0, 0, 0);
        }

        if (++con_kc == spt) {
            // ---- tile done: lane holds query r16, sel slots 16 ord + 4g + {0..3}
            const int64_t slot0 = ((t0 + w + (int64_t)con_tile * GS_WAVES) << 4) + 4 * g;
            const f32x4 xn = *reinterpret_cast<const f32x4*>(nrm + (con_tile & (GS_NORM_SLOTS - 1)) * GS_NORM_BYTES + g * 16);
            const u32x4_t pid = *reinterpret_cast<const u32x4_t*>(nrm + (con_tile & (GS_NORM_SLOTS - 1)) * GS_NORM_BYTES + 64 + g * 16);
            const uint64_t thr = thr_w[r16];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float sc = sc_score<METRIC>(acc[c], xn[c], qn_mine);
                const uint64_t key = sc_make_key<METRIC>(sc, pid[c]);
                const bool cand = r16 < nq && slot0 + c < a.m;
                if (cand && key < thr) {
                    // inline asm: a compiler-visible LDS write here would get an s_waitcnt vmcnt(0) in front of it and drain the ring
                    unsigned pos;
                    const unsigned cnt_addr = (unsigned)(uintptr_t)(cnt_w + r16), one = 1u;
                    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(pos) : "v"(cnt_addr), "v"(one) : "memory");
                    const unsigned slot_addr = (unsigned)(uintptr_t)(cand_w + r16 * a.cap + pos);
                    asm volatile("ds_write_b64 %0, %1" ::"v"(slot_addr), "v"(key) : "memory");
                }
            }
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const bool full = cnt_w[r16] > (unsigned)(a.cap - 16);
            if (__any(full)) {
                for (int c = 0; c < nq; ++c)
                    if (cnt_w[c] > (unsigned)(a.cap - 16))
                        gs_wave_compact(cand_w + c * a.cap, tmp_w, cnt_w + c, thr_w + c, a.k, lane);
            }
            con_kc = 0;
            ++con_tile;
        }
    }

    // ---- flush: every wave sorts its slots; the workgroup then merges its 4 lists per slot (rank among the union,
    // keys are unique) and writes ONE sorted list: partial[grp][wg][slot][k]
    for (int c = 0; c < nq; ++c) gs_wave_compact(cand_w + c * a.cap, tmp_w, cnt_w + c, thr_w + c, a.k, lane);
    __syncthreads();
    uint64_t* out = a.partial + ((size_t)grp * gridDim.x + blockIdx.x) * (size_t)a.qt * a.k;
    lds_u64p cand_all = (lds_u64p)(smem + L.cand);
    lds_u32p cnt_all = (lds_u32p)(smem + L.cnt);
    for (int c = 0; c < a.qt; ++c) {
        int m[GS_WAVES], total = 0;
#pragma unroll
        for (int v = 0; v < GS_WAVES; ++v) {
            m[v] = c < nq ? (int)cnt_all[v * 16 + c] : 0;
            total += m[v];
        }
        for (int e = tid; e < total; e += 256) {
            int v = 0, idx = e;
            while (idx >= m[v]) { idx -= m[v]; ++v; }
            const uint64_t key = cand_all[(v * a.qt + c) * a.cap + idx];
            int rank = 0;
#pragma unroll
            for (int u = 0; u < GS_WAVES; ++u)
                for (int j = 0; j < m[u]; ++j) rank += (cand_all[(u * a.qt + c) * a.cap + j] < key) ? 1 : 0;
            if (rank < a.k) out[(size_t)c * a.k + rank] = key;
        }
        const int have = total < a.k ? total : a.k;
        for (int e = have + tid; e < a.k; e += 256) out[(size_t)c * a.k + e] = SC_KEY_MAX;
    }
}

template <int METRIC>
static void launch_scan_gather(const GatherArgs& a, dim3 grid, size_t lds, hipStream_t s) {
    static ScDeviceOnce once;  // per instantiation and device
    sc_device_once(once, [&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scan_gather_kernel<METRIC>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    hipLaunchKernelGGL((scan_gather_kernel<METRIC>), grid, dim3(256), lds, s, a);
}

void sc_launch_scan_gather(int metric, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, int Q, int k, const ScanPlan& p,
                           uint64_t* partial, const uint32_t* perm, int64_t perm_rows, const uint32_t* sel, int64_t m, hipStream_t s) {
    if (m <= 0) return;
    GatherArgs a;
    a.X = X; a.xnorm = xnorm; a.ld = ld; a.Qp = Qp; a.qnorm = qnorm; a.Q = Q; a.qt = p.qt; a.k = k; a.cap = p.cap;
    const int64_t tiles = (m + 15) / 16;
    a.tiles_per_wg = (int)((tiles + p.nwg - 1) / p.nwg);
    a.partial = partial;
    a.perm = perm; a.perm_rows = perm ? perm_rows : 0; a.sel = sel; a.m = m;
    const dim3 grid((unsigned)p.nwg, (unsigned)p.groups);
    const size_t lds = gather_lds_layout(ld, p.qt, p.cap).total;
    sc_dispatch_metric(metric, [&](auto mc) { launch_scan_gather<mc.value>(a, grid, lds, s); });
}
