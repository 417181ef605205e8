// scan_lexical.hip -- the lexical (BM25) scan over the term rows of an index, their statistics, and the reciprocal-rank fusion of
// the hybrid search (sc_index_search_lexical*, sc_index_lex_stats, sc_index_search_hybrid*: include/semcode_hip.h; gfx950).
//
// The rules -- term rows, the score, the order of hits, the fusion -- are lex_rule.h, which sc_lexical.cpp compiles for the CPU too.
//
// lex_scan_kernel is the hot path.  Roofline: HBM.  Algorithmic bytes = rows * 2 T per pass, and a pass serves LEX_QP = 16 queries.
//   - A lane loads 16 bytes = 8 slots; a row is T / 8 lanes, so one wave load (1 KiB) covers 1024 / 2T rows: 4 at T = 128.  A wave
//     keeps LEX_UNROLL = 4 such loads in flight.  The allow bit of a lane's row is tested before the load is issued: rows that are
//     not allowed are never read.
//   - The terms of the pass's queries are a 65 536-bit membership set in LDS (8 KiB, built once per pass by lex_prep_kernel): every
//     slot costs one LDS read and a bit test.  The padding slot 0xFFFF is never a member.
//   - A wave load with a member slot takes the slow path, every row in its own T / 8 lanes: dl and, for every distinct member value
//     of the row in ascending order, tf are sums over the row's lanes (xor shuffles that stay inside the row) -- integers, so exact
//     in any order; the row's lanes share the 16 queries (16 / (T / 8) each, at least one), look the value up in the query's sorted
//     terms (LDS, binary search) and add lex_term to the score, which is the rule's ascending-j sum.
//   - A wave keeps the k best 64-bit keys (sc_make_key of the score as an IP score: larger first, then the lower row) of every
//     query sorted in LDS; the rows of a wave load insert one after the other, so a list has one writer at a time (LDS operations of
//     one wave complete in order).  The workgroup writes its 4 x 16 lists as partial lists and sc_launch_topk_merge finishes the job.
// LDS: 11 328 B + 512 k B, so 4 workgroups per CU up to k = 56, 3 at k = 64 and 2 at k = 128.
//
// lex_stats_kernel: df[t] += 1 for the first slot of every run of a row, sum_dl += dl: integer atomics only.
// lex_fuse_kernel: one workgroup per query, one thread per entry of the two candidate lists; a thread ranks its row by counting the
// rows before it (lex_before), so no atomic decides an order.
#include "lex_rule.h"
#include "sc_common.h"

#define LEX_QP 16
#define LEX_UNROLL 4
#define LEX_THREADS 256
#define LEX_FIXED_LDS (8192 + LEX_QP * LEX_MAX_QTERMS * 2 + LEX_QP * LEX_MAX_QTERMS * 4 + LEX_QP * 4)

// ---- per pass: validate the queries, build the membership set
// qterms [Q][32], qweights [Q][32], nterms [Q]; pass p = queries [16 p, 16 p + 16).  memb [passes][2048]; nt_eff [Q] = nterms, or 0 for
// a query that breaks the rules (m outside 0..32, terms not strictly ascending or 0xFFFF, a weight not finite or not > 0), which
// also sets *bad.
__global__ __launch_bounds__(LEX_THREADS) void lex_prep_kernel(const uint16_t* __restrict__ qterms, const float* __restrict__ qweights, const int32_t* __restrict__ nterms,
                                                               int Q, uint32_t* __restrict__ memb, int32_t* __restrict__ nt_eff, int32_t* __restrict__ bad) {
    __shared__ uint32_t s_set[2048];
    __shared__ int s_ok[LEX_QP];
    const int tid = threadIdx.x, q0 = blockIdx.x * LEX_QP;
    for (int i = tid; i < 2048; i += LEX_THREADS) s_set[i] = 0u;
    if (tid < LEX_QP) {
        const int q = q0 + tid;
        s_ok[tid] = q < Q && nterms[q] >= 0 && nterms[q] <= LEX_MAX_QTERMS ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < LEX_QP * LEX_MAX_QTERMS; i += LEX_THREADS) {
        const int ql = i / LEX_MAX_QTERMS, j = i - ql * LEX_MAX_QTERMS, q = q0 + ql;
        if (q < Q && s_ok[ql] && j < nterms[q]) {
            const size_t o = (size_t)q * LEX_MAX_QTERMS + j;
            const bool fine = qterms[o] != LEX_PAD && (j == 0 || qterms[o - 1] < qterms[o]) && lex_valid_weight(qweights[o]);
            if (!fine) s_ok[ql] = 0;  // (benign race: every writer stores 0)
        }
    }
    __syncthreads();
    for (int i = tid; i < LEX_QP * LEX_MAX_QTERMS; i += LEX_THREADS) {
        const int ql = i / LEX_MAX_QTERMS, j = i - ql * LEX_MAX_QTERMS, q = q0 + ql;
        if (q < Q && s_ok[ql] && j < nterms[q]) {
            const uint32_t t = qterms[(size_t)q * LEX_MAX_QTERMS + j];
            atomicOr(&s_set[t >> 5], 1u << (t & 31));
        }
    }
    __syncthreads();
    for (int i = tid; i < 2048; i += LEX_THREADS) memb[(size_t)blockIdx.x * 2048 + i] = s_set[i];
    if (tid < LEX_QP && q0 + tid < Q) {
        const int q = q0 + tid;
        const bool given_ok = s_ok[tid] != 0;
        nt_eff[q] = given_ok ? nterms[q] : 0;
        if (!given_ok) atomicOr(bad, 1);
    }
}

struct LexScanArgs {
    const uint4* terms;       // [n][T / 8] 16-byte pieces
    int64_t n;
    const uint32_t* allow;    // bitset over rows, or NULL
    const uint32_t* memb;     // [2048] of this pass
    const uint16_t* qterms;   // [nq][32] of this pass
    const float* qweights;    // [nq][32]
    const int32_t* nt_eff;    // [nq]
    int nq, k;
    float k1, b, avgdl;
    uint64_t* partial;        // [gridDim.x * 4][LEX_QP][k]
};

template <int I>
static __device__ __forceinline__ uint32_t lex_slot(const uint4& v) {
    const uint32_t w = I < 2 ? v.x : I < 4 ? v.y : I < 6 ? v.z : v.w;
    return (I & 1) ? (w >> 16) : (w & 0xFFFFu);
}

// LPR = lanes per row = T / 8
template <int LPR>
__global__ __launch_bounds__(LEX_THREADS) void lex_scan_kernel(LexScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lex_lds[];
    uint32_t* s_memb = (uint32_t*)lex_lds;                                       // [2048]
    uint16_t* s_qt = (uint16_t*)(lex_lds + 8192);                                // [16][32]
    float* s_qw = (float*)(lex_lds + 8192 + LEX_QP * LEX_MAX_QTERMS * 2);         // [16][32]
    int* s_qm = (int*)(lex_lds + 8192 + LEX_QP * LEX_MAX_QTERMS * 6);             // [16]
    uint64_t* s_list = (uint64_t*)(lex_lds + LEX_FIXED_LDS);                      // [4][16][k]
    constexpr int RPW = 64 / LPR;  // rows per wave load
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, k = a.k;

    for (int i = tid; i < 2048; i += LEX_THREADS) s_memb[i] = a.memb[i];
    for (int i = tid; i < LEX_QP * LEX_MAX_QTERMS; i += LEX_THREADS) {
        const bool in = i < a.nq * LEX_MAX_QTERMS;
        s_qt[i] = in ? a.qterms[i] : (uint16_t)LEX_PAD;
        s_qw[i] = in ? a.qweights[i] : 0.0f;
    }
    if (tid < LEX_QP) s_qm[tid] = tid < a.nq ? a.nt_eff[tid] : 0;
    for (int i = tid; i < 4 * LEX_QP * k; i += LEX_THREADS) s_list[i] = SC_KEY_MAX;
    __syncthreads();

    const int64_t ntiles = (a.n + RPW - 1) / RPW;
    const int64_t GW = (int64_t)gridDim.x * 4, gw = (int64_t)blockIdx.x * 4 + w;
    const int sub = lane / LPR;
    const float k1p = lex_add(a.k1, 1.0f);
    // lane l of a row's LPR lanes scores queries [l * QPL, l * QPL + QPL) for that row (lanes beyond the 16 queries: none)
    constexpr int QPL = LPR >= LEX_QP ? 1 : LEX_QP / LPR;
    const int q_first = (lane % LPR) * QPL < LEX_QP ? (lane % LPR) * QPL : 0;
    int qm[QPL];
#pragma unroll
    for (int i = 0; i < QPL; ++i) qm[i] = (lane % LPR) * QPL < LEX_QP ? s_qm[q_first + i] : 0;
    volatile uint64_t* my_list = s_list + (size_t)(w * LEX_QP + q_first) * k;  // the lists of my queries, k keys each
    for (int64_t t0 = gw; t0 < ntiles; t0 += GW * LEX_UNROLL) {
        uint4 v[LEX_UNROLL];
        bool on[LEX_UNROLL];
#pragma unroll
        for (int u = 0; u < LEX_UNROLL; ++u) {
            const int64_t t = t0 + (int64_t)u * GW, row = t * RPW + sub;
            on[u] = t < ntiles && row < a.n;
            if (on[u] && a.allow) on[u] = (a.allow[row >> 5] >> (row & 31)) & 1u;
        }
#pragma unroll
        for (int u = 0; u < LEX_UNROLL; ++u) {
            const int64_t t = t0 + (int64_t)u * GW;
            v[u] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (on[u]) v[u] = a.terms[t * 64 + lane];  // (row * LPR + lane % LPR)
        }
#pragma unroll
        for (int u = 0; u < LEX_UNROLL; ++u) {
            const uint4 x = v[u];
            const uint32_t s0 = lex_slot<0>(x), s1 = lex_slot<1>(x), s2 = lex_slot<2>(x), s3 = lex_slot<3>(x), s4 = lex_slot<4>(x), s5 = lex_slot<5>(x),
                           s6 = lex_slot<6>(x), s7 = lex_slot<7>(x);
            uint32_t hm = (s_memb[s0 >> 5] >> (s0 & 31)) & 1u;
            hm |= ((s_memb[s1 >> 5] >> (s1 & 31)) & 1u) << 1;
            hm |= ((s_memb[s2 >> 5] >> (s2 & 31)) & 1u) << 2;
            hm |= ((s_memb[s3 >> 5] >> (s3 & 31)) & 1u) << 3;
            hm |= ((s_memb[s4 >> 5] >> (s4 & 31)) & 1u) << 4;
            hm |= ((s_memb[s5 >> 5] >> (s5 & 31)) & 1u) << 5;
            hm |= ((s_memb[s6 >> 5] >> (s6 & 31)) & 1u) << 6;
            hm |= ((s_memb[s7 >> 5] >> (s7 & 31)) & 1u) << 7;
            // ---- the slow path: the rows of this wave load that hold a member slot, all of them at once, each in its own lanes
            if (__ballot(hm != 0u)) {
                const int64_t row = (t0 + (int64_t)u * GW) * RPW + sub;
                int dl = (int)(s0 != LEX_PAD) + (int)(s1 != LEX_PAD) + (int)(s2 != LEX_PAD) + (int)(s3 != LEX_PAD) + (int)(s4 != LEX_PAD) + (int)(s5 != LEX_PAD) +
                         (int)(s6 != LEX_PAD) + (int)(s7 != LEX_PAD);
#pragma unroll
                for (int off = LPR / 2; off >= 1; off >>= 1) dl += __shfl_xor(dl, off);
                const float K = lex_K(a.k1, a.b, a.avgdl, dl);
                float score[QPL];
                bool matched[QPL];
#pragma unroll
                for (int i = 0; i < QPL; ++i) {
                    score[i] = 0.0f;
                    matched[i] = false;
                }
                uint32_t lo = 0;  // member values below it are done
                for (;;) {
                    uint32_t mv = 0x10000u;  // the smallest member value >= lo of my row
                    if ((hm & 1u) && s0 >= lo && s0 < mv) mv = s0;
                    if ((hm & 2u) && s1 >= lo && s1 < mv) mv = s1;
                    if ((hm & 4u) && s2 >= lo && s2 < mv) mv = s2;
                    if ((hm & 8u) && s3 >= lo && s3 < mv) mv = s3;
                    if ((hm & 16u) && s4 >= lo && s4 < mv) mv = s4;
                    if ((hm & 32u) && s5 >= lo && s5 < mv) mv = s5;
                    if ((hm & 64u) && s6 >= lo && s6 < mv) mv = s6;
                    if ((hm & 128u) && s7 >= lo && s7 < mv) mv = s7;
#pragma unroll
                    for (int off = LPR / 2; off >= 1; off >>= 1) {
                        const uint32_t o = (uint32_t)__shfl_xor((int)mv, off);
                        mv = o < mv ? o : mv;
                    }
                    if (!__ballot(mv != 0x10000u)) break;  // (every row of the wave load is done)
                    lo = mv + 1u;
                    int tf = (int)(s0 == mv) + (int)(s1 == mv) + (int)(s2 == mv) + (int)(s3 == mv) + (int)(s4 == mv) + (int)(s5 == mv) + (int)(s6 == mv) + (int)(s7 == mv);
#pragma unroll
                    for (int off = LPR / 2; off >= 1; off >>= 1) tf += __shfl_xor(tf, off);
                    if (mv != 0x10000u) {
#pragma unroll
                        for (int i = 0; i < QPL; ++i) {  // is mv one of this query's terms?  (first index with term >= mv)
                            const uint16_t* qt = s_qt + (q_first + i) * LEX_MAX_QTERMS;
                            int lb = 0, hb = qm[i];
                            while (lb < hb) {
                                const int mid = (lb + hb) >> 1;
                                if ((uint32_t)qt[mid] < mv) lb = mid + 1;
                                else hb = mid;
                            }
                            if (lb < qm[i] && (uint32_t)qt[lb] == mv) {
                                score[i] = lex_add(score[i], lex_term(s_qw[(q_first + i) * LEX_MAX_QTERMS + lb], tf, k1p, K));
                                matched[i] = true;
                            }
                        }
                    }
                }
                // a (wave, query) list has one writer at a time: the rows of the wave load insert one after the other
                bool want = false;
#pragma unroll
                for (int i = 0; i < QPL; ++i) want = want || (matched[i] && sc_make_key<SC_METRIC_IP>(score[i], (uint32_t)row) < my_list[(size_t)i * k + k - 1]);
                uint64_t pend = __ballot(want);
                {
                    while (pend) {  // (wave-uniform: the next row with a key to insert)
                        const int g = (int)__builtin_ctzll(pend) / LPR;
                        pend &= ~((((uint64_t)1 << LPR) - 1ull) << (g * LPR));
                        if (sub == g) {
#pragma unroll
                            for (int i = 0; i < QPL; ++i) {
                                volatile uint64_t* L = my_list + (size_t)i * k;
                                const uint64_t key = sc_make_key<SC_METRIC_IP>(score[i], (uint32_t)row);
                                if (matched[i] && key < L[k - 1]) {
                                    int p = k - 1;
                                    while (p > 0 && L[p - 1] > key) {
                                        L[p] = L[p - 1];
                                        --p;
                                    }
                                    L[p] = key;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    uint64_t* out = a.partial + (size_t)blockIdx.x * 4 * LEX_QP * k;
    for (int i = tid; i < 4 * LEX_QP * k; i += LEX_THREADS) out[i] = s_list[i];
}

static size_t sc_lex_scan_lds_bytes(int k) { return (size_t)LEX_FIXED_LDS + (size_t)4 * LEX_QP * k * sizeof(uint64_t); }
int sc_lex_queries_per_pass(void) { return LEX_QP; }

// workgroups of a pass over n rows of T slots at width k on `cus` compute units
int sc_lex_scan_workgroups(int64_t n, int T, int k, int cus) {
    const int rpw = 64 / (T / 8);
    const int64_t tiles = (n + rpw - 1) / rpw, want = (tiles + 4 * LEX_UNROLL - 1) / (4 * LEX_UNROLL);
    int per_cu = (int)((160 * 1024) / sc_lex_scan_lds_bytes(k));
    per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
    const int64_t cap = (int64_t)cus * per_cu;
    return (int)(want < 1 ? 1 : want > cap ? cap : want);
}

void sc_launch_lex_prep(const uint16_t* qterms, const float* qweights, const int32_t* nterms, int Q, uint32_t* memb, int32_t* nt_eff, int32_t* bad, hipStream_t s) {
    if (Q < 1) return;
    hipLaunchKernelGGL(lex_prep_kernel, dim3((unsigned)((Q + LEX_QP - 1) / LEX_QP)), dim3(LEX_THREADS), 0, s, qterms, qweights, nterms, Q, memb, nt_eff, bad);
}

static ScDeviceOnce g_lex_attr_once;

void sc_launch_lex_scan(const uint16_t* terms, int64_t n, int T, const uint32_t* allow, const uint32_t* memb, const uint16_t* qterms, const float* qweights,
                        const int32_t* nt_eff, int nq, int k, float k1, float b, float avgdl, int nwg, uint64_t* partial, hipStream_t s) {
    if (nq < 1 || nq > LEX_QP || k < 1 || k > 128 || nwg < 1 || !lex_valid_T(T)) return;  // (the host checks these before it plans a call)
    sc_device_once(g_lex_attr_once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(lex_scan_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(lex_scan_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(lex_scan_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(lex_scan_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    });
    LexScanArgs a;
    a.terms = reinterpret_cast<const uint4*>(terms); a.n = n; a.allow = allow; a.memb = memb; a.qterms = qterms; a.qweights = qweights; a.nt_eff = nt_eff;
    a.nq = nq; a.k = k; a.k1 = k1; a.b = b; a.avgdl = avgdl; a.partial = partial;
    const size_t lds = sc_lex_scan_lds_bytes(k);
    const dim3 grid((unsigned)nwg), block(LEX_THREADS);
    if (T == 32) hipLaunchKernelGGL(lex_scan_kernel<4>, grid, block, lds, s, a);
    else if (T == 64) hipLaunchKernelGGL(lex_scan_kernel<8>, grid, block, lds, s, a);
    else if (T == 128) hipLaunchKernelGGL(lex_scan_kernel<16>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(lex_scan_kernel<32>, grid, block, lds, s, a);
}

// ---- statistics: one thread per 16-byte piece; a slot opens a run when it differs from the slot before it in its row
__global__ __launch_bounds__(256) void lex_stats_kernel(const uint4* __restrict__ terms, int64_t pieces, int lpr, uint32_t* __restrict__ df,
                                                        unsigned long long* __restrict__ sum_dl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    if (i < pieces) {
        const uint4 x = terms[i];
        uint32_t prev = LEX_PAD;  // (a row's first slot opens a run unless it is padding)
        if (i % lpr != 0) prev = reinterpret_cast<const uint16_t*>(terms)[i * 8 - 1];
        const uint32_t sl[8] = {lex_slot<0>(x), lex_slot<1>(x), lex_slot<2>(x), lex_slot<3>(x), lex_slot<4>(x), lex_slot<5>(x), lex_slot<6>(x), lex_slot<7>(x)};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (sl[j] != LEX_PAD) {
                ++cnt;
                if (sl[j] != prev) atomicAdd(&df[sl[j]], 1u);
            }
            prev = sl[j];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(sum_dl, (unsigned long long)cnt);
}

void sc_launch_lex_stats(const uint16_t* terms, int64_t n, int T, uint32_t* df, unsigned long long* sum_dl, hipStream_t s) {
    if (n < 1) return;
    const int64_t pieces = n * (T / 8);
    hipLaunchKernelGGL(lex_stats_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const uint4*>(terms), pieces, T / 8, df, sum_dl);
}

// ---- fusion: thread t < F is entry t of the dense list, thread F + t entry t of the lexical list (dropped when the dense list holds
// its row).  Lists are best first, rows -1 = padding.  dense_rows NULL: no candidates at all, padding only.
#define LEX_MAX_F 128
__global__ __launch_bounds__(2 * LEX_MAX_F) void lex_fuse_kernel(const int64_t* __restrict__ dense_rows, const int64_t* __restrict__ lex_rows, int F, int k, int32_t c,
                                                                 float wd, float wl, float* __restrict__ out_score, int64_t* __restrict__ out_rows) {
    __shared__ int64_t s_d[LEX_MAX_F], s_l[LEX_MAX_F];
    __shared__ int64_t s_row[2 * LEX_MAX_F];
    __shared__ float s_f[2 * LEX_MAX_F];
    const int q = blockIdx.x, tid = threadIdx.x;
    out_score += (size_t)q * k;
    out_rows += (size_t)q * k;
    if (tid < LEX_MAX_F) {
        s_d[tid] = dense_rows && tid < F ? dense_rows[(size_t)q * F + tid] : (int64_t)-1;
        s_l[tid] = dense_rows && tid < F ? lex_rows[(size_t)q * F + tid] : (int64_t)-1;
    }
    __syncthreads();
    const bool is_lex = tid >= LEX_MAX_F;
    const int e = is_lex ? tid - LEX_MAX_F : tid;
    int64_t row = is_lex ? s_l[e] : s_d[e];
    float f = 0.0f;
    if (row >= 0) {
        int other = -1;  // my row's rank in the other list
        for (int i = 0; i < F; ++i)
            if ((is_lex ? s_d[i] : s_l[i]) == row) other = i;
        if (is_lex && other >= 0) row = -1;  // counted by the dense entry
        else f = is_lex ? lex_rrf(wd, wl, c, -1, e) : lex_rrf(wd, wl, c, e, other);
    }
    s_row[tid] = row;
    s_f[tid] = f;
    __syncthreads();
    int cnt = 0;  // valid candidates in all
    int pos = 0;  // candidates before mine
    for (int i = 0; i < 2 * LEX_MAX_F; ++i) {
        const int64_t r = s_row[i];
        if (r < 0) continue;
        ++cnt;
        if (row >= 0 && i != tid && lex_before(s_f[i], r, f, row)) ++pos;
    }
    if (row >= 0 && pos < k) {
        out_score[pos] = f;
        out_rows[pos] = row;
    }
    for (int p = cnt + tid; p < k; p += 2 * LEX_MAX_F) {
        out_score[p] = -__builtin_inff();
        out_rows[p] = -1;
    }
}

void sc_launch_lex_fuse(const int64_t* dense_rows, const int64_t* lex_rows, int F, int Q, int k, int32_t c, float wd, float wl, float* out_score, int64_t* out_rows,
                        hipStream_t s) {
    if (Q < 1 || F < 1 || F > LEX_MAX_F || k < 1 || k > F) return;
    hipLaunchKernelGGL(lex_fuse_kernel, dim3((unsigned)Q), dim3(2 * LEX_MAX_F), 0, s, dense_rows, lex_rows, F, k, c, wd, wl, out_score, out_rows);
}
