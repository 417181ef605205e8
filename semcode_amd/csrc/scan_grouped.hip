// scan_grouped.hip -- the grouped search's device side (gfx950 / CDNA4): at most one hit per label.  Two small kernels around the
// existing exact scans (sc_grouped.cpp runs the rounds); neither computes a score.
//
// Replaces (reference): nothing -- the reference spends its rag_max_context_sources on whatever the top-k holds, so five chunks of
// one file are five sources (rag/pipeline.py:93-129).  Milvus: Collection.search(..., group_by_field=...).
//
// Roofline: group_select reads one best-first candidate list per query (<= 1 024 entries of 12 B) and one label per candidate (a
// scattered 4 B load each): latency, not bandwidth.  group_exclude streams the labels once per (query, round): 4 B per row, HBM.
//
// group_select_kernel   one workgroup per query.  Candidate i of the list (ids >= 0, best first; -1 = padding, which the scans put
//                       last) carries label L[i] = labels[id - row_base].  It is a FIRST occurrence when no candidate before it has
//                       its label.  In a best-first list the first row of a label is that label's best allowed row, and labels
//                       appear in the order of their best rows, so the first occurrences -- in list order -- are the next hits.
//                       Their ranks are counted, not raced for: rank(i) = first occurrences below i, so the output order depends on
//                       the list alone.  Both counts are loops over LDS (every lane reads the same word: a broadcast); at most
//                       2 * 1 024 words per candidate, four candidates per thread.
//                       The hits are appended at out[count ..] up to k; round 0 also writes the -1 / +-inf padding behind them.
//                       done = k hits, or the list held padding (then every allowed row of the query has been seen).
//                       Rounds >= 1 see only rows whose label is not among the hits so far (group_exclude), so a label never has
//                       to be compared with the hits of earlier rounds.
// group_exclude_kernel  one query: out bit r = (allow bit r, if a mask was given) && labels[r] is none of the query's `count` hit
//                       labels.  Every workgroup rank-sorts the <= 128 hit labels into LDS (they are distinct) and a lane tests
//                       its row's label by binary search; a wave's 64 verdicts are one ballot = two words of the bitset.
#include <algorithm>

#include "sc_common.h"

#define GRP_THREADS 256
#define GRP_MAX_W 1024
#define GRP_MAX_K 128

__global__ __launch_bounds__(GRP_THREADS) void group_select_kernel(const float* __restrict__ cand_dist, const int64_t* __restrict__ cand_rows, int W,
                                                                   const int32_t* __restrict__ labels, int64_t n, int64_t row_base, int k, int first_round,
                                                                   float pad_dist, float* __restrict__ out_dist, int64_t* __restrict__ out_rows,
                                                                   int32_t* __restrict__ found_labels, int32_t* __restrict__ count, int32_t* __restrict__ done) {
    constexpr int PER = GRP_MAX_W / GRP_THREADS;
    __shared__ int32_t s_lab[GRP_MAX_W];
    __shared__ unsigned char s_valid[GRP_MAX_W];
    __shared__ unsigned char s_first[GRP_MAX_W];
    __shared__ int s_total, s_pad;
    const int q = blockIdx.x, tid = threadIdx.x;
    cand_dist += (size_t)q * W;
    cand_rows += (size_t)q * W;
    out_dist += (size_t)q * k;
    out_rows += (size_t)q * k;
    found_labels += (size_t)q * k;
    const int c0 = first_round ? 0 : count[q];
    if (tid == 0) s_total = s_pad = 0;
    __syncthreads();
    int64_t row[PER];
    bool pad = false;
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int i = c * GRP_THREADS + tid;
        row[c] = -1;
        if (i < W) {
            row[c] = cand_rows[i];
            const int64_t local = row[c] - row_base;
            const bool ok = row[c] >= 0 && local >= 0 && local < n;
            pad |= !ok;
            s_valid[i] = ok;
            s_lab[i] = ok ? labels[local] : 0;
        }
    }
    if (pad) s_pad = 1;  // (every writer stores the same value)
    __syncthreads();
    bool first[PER];
    int mine = 0;
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int i = c * GRP_THREADS + tid;
        first[c] = false;
        if (i < W && s_valid[i]) {
            const int32_t l = s_lab[i];
            bool seen = false;
            for (int j = 0; j < i; ++j) seen |= s_valid[j] && s_lab[j] == l;
            first[c] = !seen;
        }
        if (i < W) s_first[i] = first[c];
        mine += first[c] ? 1 : 0;
    }
    if (mine) atomicAdd(&s_total, mine);  // (an integer sum: the order of arrival does not show)
    __syncthreads();
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const int i = c * GRP_THREADS + tid;
        if (!first[c]) continue;
        int rank = 0;
        for (int j = 0; j < i; ++j) rank += s_first[j];
        const int pos = c0 + rank;
        if (pos < k) {
            out_dist[pos] = cand_dist[i];
            out_rows[pos] = row[c];
            found_labels[pos] = s_lab[i];
        }
    }
    const int c1 = min(k, c0 + s_total);
    if (first_round)
        for (int pos = c1 + tid; pos < k; pos += GRP_THREADS) {
            out_dist[pos] = pad_dist;
            out_rows[pos] = -1;
        }
    if (tid == 0) {
        count[q] = c1;
        done[q] = (c1 >= k || s_pad) ? 1 : 0;
    }
}

__global__ __launch_bounds__(GRP_THREADS) void group_exclude_kernel(const int32_t* __restrict__ labels, int64_t n, const uint32_t* __restrict__ allow,
                                                                    const int32_t* __restrict__ found_labels, const int32_t* __restrict__ count,
                                                                    uint32_t* __restrict__ out) {
    __shared__ int32_t s_raw[GRP_MAX_K];
    __shared__ int32_t s_sorted[GRP_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = min(*count, GRP_MAX_K);
    if (tid < c) s_raw[tid] = found_labels[tid];
    __syncthreads();
    if (tid < c) {  // rank sort: the hit labels are distinct
        const int32_t l = s_raw[tid];
        int rank = 0;
        for (int j = 0; j < c; ++j) rank += s_raw[j] < l ? 1 : 0;
        s_sorted[rank] = l;
    }
    __syncthreads();
    const int64_t words = (n + 31) >> 5;
    const int64_t chunks = (n + 63) >> 6;  // 64 rows = one ballot
    const int64_t wave = (int64_t)blockIdx.x * (GRP_THREADS / 64) + (tid >> 6), nwaves = (int64_t)gridDim.x * (GRP_THREADS / 64);
    for (int64_t ch = wave; ch < chunks; ch += nwaves) {
        const int64_t r = ch * 64 + lane;
        bool on = false;
        if (r < n) {
            const int32_t l = labels[r];
            int lo = 0, hi = c;  // first entry >= l
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_sorted[mid] < l) lo = mid + 1;
                else hi = mid;
            }
            on = !(lo < c && s_sorted[lo] == l);
        }
        const uint64_t word = __ballot(on);
        if (lane < 2) {
            const int64_t w = ch * 2 + lane;
            if (w < words) {
                uint32_t v = lane ? (uint32_t)(word >> 32) : (uint32_t)word;
                if (allow) v &= allow[w];
                out[w] = v;
            }
        }
    }
}

void sc_launch_group_select(int metric, const float* cand_dist, const int64_t* cand_rows, int W, int Q, const int32_t* labels, int64_t n, int64_t row_base, int k,
                            bool first_round, float* out_dist, int64_t* out_rows, int32_t* found_labels, int32_t* count, int32_t* done, hipStream_t s) {
    if (Q < 1 || W < 1 || W > GRP_MAX_W || k < 1 || k > GRP_MAX_K) return;  // (the host checks these before it plans a round)
    const float pad = metric == SC_METRIC_L2 ? __builtin_inff() : -__builtin_inff();
    hipLaunchKernelGGL(group_select_kernel, dim3((unsigned)Q), dim3(GRP_THREADS), 0, s, cand_dist, cand_rows, W, labels, n, row_base, k, first_round ? 1 : 0, pad,
                       out_dist, out_rows, found_labels, count, done);
}

void sc_launch_group_exclude(const int32_t* labels, int64_t n, const uint32_t* allow, const int32_t* found_labels, const int32_t* count, uint32_t* out, int cus,
                             hipStream_t s) {
    if (n < 1) return;
    const int64_t chunks = (n + 63) >> 6, per_wg = GRP_THREADS / 64;
    const int64_t grid = std::min<int64_t>((chunks + per_wg - 1) / per_wg, (int64_t)std::max(cus, 1) * 8);
    hipLaunchKernelGGL(group_exclude_kernel, dim3((unsigned)grid), dim3(GRP_THREADS), 0, s, labels, n, allow, found_labels, count, out);
}
