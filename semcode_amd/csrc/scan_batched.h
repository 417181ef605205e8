// scan_batched.h -- large query batches: bf16 MFMA coarse scores fused with threshold filtering, then an
// exact f32 re-rank with a per-query certificate (gfx950).  Internal header of the stages of that path:
// scan_shadow.hip (shadow copies), scan_coarse.hip / scan_coarse64.hip (coarse GEMM + filter), scan_select.hip
// (per-phase selection), scan_rerank.hip (exact re-rank, certificate, collect pass, tightening).
//
// Replaces (reference): the server side of Collection.search for a FLAT scan
// (src/semcode/storage/milvus_store.py:141-147), for batches the reference never sends (it issues one
// query per call); BASELINE.json's configs[2] (batch-1024 over 10M x 768) is this path.
//
// Why two stages: at Q = 1024 the scan is 2*N*d*Q = 1.6e13 FLOP per batch -- 101 ms on the f32 matrix
// pipe but 6.3 ms at the bf16 MFMA peak, against 4.9 ms to stream the f32 corpus.
// So the corpus keeps a bf16 shadow copy in HBM and the batch runs as a bf16 GEMM (gemm_tile.h) whose
// epilogue never stores scores: it compares each of them with a per-query threshold and appends the
// rare survivors (64-bit key = coarse score | row) to a per-query list.  Thresholds tighten between
// "phases" of geometrically growing row ranges (1 Ki, 4 Ki, 16 Ki, ... rows, x4 each): after each phase a
// small kernel keeps the k' best coarse keys per query and publishes the new threshold.
//
// Exactness: the k' (= 128) coarse candidates of a query are re-scored in f32 in the canonical
// summation order of scan_exact.hip / oracle/sc_oracle.c, so every returned distance is bit-identical
// to the exact path.  |coarse - exact| <= eps_q (bf16 input rounding, bound below), therefore a row that
// is NOT a candidate has exact score >= tau_q - eps_q; if the k-th exact candidate score is strictly
// below that, the top-k is proven complete and correctly ordered.  Queries that fail the test (or whose
// survivor list overflowed) are flagged and re-run through the exact scan by the host code.
//
// Roofline: MFMA bf16; algorithmic FLOPs = 2 * rows * ld * Qpad per phase launch.
#pragma once
#include "gemm_tile.h"

#define KPRIME 128         // coarse candidates kept per query (one re-rank thread each)
#define KPRIME8 512        // the same for the int8 coarse stage, whose error bound is ~7x wider (see below); with 256 the certificate
                           // fails for 51 of 1 024 queries at 10M x 768 and the bf16 stage they go to costs more than is saved: 84k -> 63k QPS
#define SEL_THREADS 256
#define SEL_BINS 4096      // radix_select_pivot: bins of one 12-bit pass

// ---- int8 coarse stage -------------------------------------------------------------------------------------------------
// At Q = 1024 the bf16 GEMM is the whole cost (15 ms at 1.0 PF; 6.3 ms even at the nominal peak).  v_mfma_i32_16x16x64_i8 runs
// at twice the bf16 rate, so the coarse scores can also be taken from an int8 shadow: row r is stored as q_r = round(x_r / s_r),
// s_r = max|x_r| / 127 (7.7 GB at 10M x 768), the query likewise, and <x,q> ~ s_r s_q <q_r,q_q> with an EXACT integer dot.
// Nothing else changes: survivors below a per-query threshold, the KPRIME8 best kept between phases, every candidate re-scored in
// f32 in the canonical order (returned distances stay bit-identical to the exact path), and the same certificate
//     kth exact score + eps_q < tau_q      with eps_q from Cauchy-Schwarz on the ACTUAL rounding residuals
//     |<x,q> - s_r s_q <q_r,q_q>| <= max_r|x_r - s_r q_r| |q| + max_r|s_r q_r| |q - s_q q_q| .
// int8 residuals are ~7x those of bf16 (step max|x|/127 vs 2^-9 relative), so tau_q has to sit further out: 512 candidates
// instead of 128 (on N(0,1) data at 768 dimensions eps ~ 24 in squared-L2 units against a gap of ~48 between the 10th and the
// 512th neighbour).  A query that fails the int8 certificate is re-run on the bf16 stage, and only then exactly.

// ------------------------------------------------------------------ coarse GEMM + filter
struct CoarseArgs {
    const bf16_t* Xb;      // [rows padded to 128, ld]
    const float* xnorm;    // [n]
    int64_t row0, row1;    // phase row range [row0, row1), row0 % 128 == 0
    int ld;
    const bf16_t* Qb;      // [Qpad, ld]
    const float* qnorm;    // [Q]
    int Q, qtiles;
    const float* thr;      // [Q] threshold in v-space (v = score for L2, -score otherwise), +inf at start
    const float* thr_fast; // [Q] pre-adjusted threshold of the cheap test (superset of v <= thr)
    uint64_t* surv;        // [Q][cap]
    unsigned* count;       // [Q]
    int cap;
    int ntiles;
    const float* xscale;   // int8 stage: s_r per corpus row (rows padded to 256 hold anything finite)
    const float* qscale;   // int8 stage: s_q per query [Qpad]
    unsigned long long* trace;  // TRACE (SC_COARSE_TRACE): [ntiles][8] = HW_ID | XCC_ID << 32, t_entry, t_mainloop_done, t_end (100 MHz), 3 counters
};
// GROUPED (IVF_FLAT coarse stage, ivf_coarse.hip): a work item is one 256-row tile of a LIST PART against one group of up to 64
// query SLOTS (the (query, list) pairs that probe the list): rows from the centred int8 shadow, slots from the per-pair centred
// queries, thresholds / norms / scales / query ids per slot.  Same stream of stages, same tests; a hit names the slot's query.
struct GroupItem {
    long long row0;  // first stored position of the tile
    int rows;        // valid rows (<= 256)
    int slot_base;   // first of the group's 64 slots
};
struct GroupedArgs {
    const GroupItem* items;
    int nitems;
    const float *slot_tf, *slot_thr, *slot_qn, *slot_qs;
    const int32_t* slot_q;
    const float *slot_qb, *slot_qd;  // |q'|, |q' - qq|: the pair factors of the row-wise error bound
    const f32x4* xrow;               // per row {|x'|^2, scale, 2 |dx|, 2 (|x'| + |dx|)}
    const int32_t* slot_dst;         // DENSE: survivor-list position of the slot's list row r = (uint32)(r + slot_dst) (mod 2^32)
};

// scan_coarse.hip -> scan_coarse64.hip: the narrow streaming kernel for batches of <= 64 queries, and the workgroup count the
// coarse_workgroups option of sc_diag_set_option forces on every persistent coarse kernel (0 = one per CU)
bool sc_scan_coarse64_supported(int Q, int ld8, size_t hit_bytes);
void sc_launch_coarse64s(int metric, const CoarseArgs& a, hipStream_t s, void* hit_scratch, size_t hit_bytes);
int sc_scan_coarse_workgroups(void);

// ---- one score of the coarse GEMM: fast test value, then the precise test ------------------------------------------------------------
// acc is the accumulator of (corpus row, query): the bf16 dot, or (I8) the bits of the exact integer dot, which s_r s_q scales.
// The fast value t (compared with thr_fast[q], a superset of the precise test: fast_threshold below) leaves out everything that
// depends on the query alone: xs = 1 / |x| (cosine), ar = the row's factor -2 s_r (L2), -s_r / |x| (cosine), -s_r (IP), sq = s_q.
template <int METRIC, bool I8>
static __device__ __forceinline__ float coarse_fast_value(float acc, float xn, float xs, float ar, float sq) {
    if (I8) {
        const float av = (float)__float_as_int(acc) * ar;
        return (METRIC == SC_METRIC_L2) ? fmaf(av, sq, xn) : av * sq;
    }
    if (METRIC == SC_METRIC_L2) return fmaf(-2.0f, acc, xn);
    if (METRIC == SC_METRIC_COSINE) return -acc * xs;
    return -acc;
}
// The precise test: the coarse score in the arithmetic of sc_score against thr[q] in v-space (-inf for padded queries).  True: the
// score survives; `key` is its survivor key (set either way).  xn / qn = |x|^2 / |q|^2, sx / sq = the int8 scales of row and query.
template <int METRIC, bool I8>
static __device__ __forceinline__ bool coarse_survivor(float acc, float xn, float sx, float sq, float qn, float thr, uint32_t row, uint64_t& key) {
    const float dot = I8 ? (float)__float_as_int(acc) * (sx * sq) : acc;
    const float sc = sc_score<METRIC>(dot, xn, qn);
    const float v = (METRIC == SC_METRIC_L2) ? sc : -sc;
    key = sc_make_key<METRIC>(sc, row);  // (before the test, not under it: as `if (!(v <= thr)) return false;` the 256-tile kernels came out of
    return v <= thr;                     // hipcc with one more exec-mask level per score and, for COSINE, 31 spilled VGPRs)
}

// The fast-test form of a threshold t (v-space) for a query of squared norm qn: what thr_fast[q] holds next to thr[q] = t.  The
// fast test must pass whatever the precise one passes, hence the slack (cosine: -dot/|x| <= (t + slack) * |q|, |q| > 0).
template <int METRIC>
static __device__ __forceinline__ float fast_threshold(float t, float qn) {
    const float slack = 1e-3f * fabsf(t) + 1e-6f;
    if (METRIC == SC_METRIC_L2) return (t - qn) + slack + 1e-3f * fabsf(qn);
    if (METRIC == SC_METRIC_COSINE) return (t + slack) * sqrtf(qn) + 1e-5f * sqrtf(qn);
    return t + slack;
}

// Radix select over the 64-bit keys cand[0 .. n): the key of rank `want` (0-based, want < n), 12 bits per pass from the top
// (SEL_BINS-bin histogram in LDS, atomics; after the first pass only the keys of one bin are still in play).  Called by all
// SEL_THREADS threads of the workgroup; hist [SEL_BINS], part [SEL_THREADS] (per-wave partial sums of the bin scan), misc[1] /
// misc[2] (chosen bin, rank inside it) are LDS scratch.
static __device__ __forceinline__ uint64_t radix_select_pivot(const uint64_t* cand, int n, unsigned want, unsigned* hist, unsigned* part, unsigned* misc) {
    const int tid = threadIdx.x;
    uint64_t prefix = 0;  // the fixed high bits (width 64 - shift - 12 ... ); `want` is the remaining rank among the keys that share them
    for (int shift = 52; shift >= -8; shift -= 12) {  // 52, 40, 28, 16, 4, then the last 4 bits (shift -8 -> 4-bit digit)
        const int sh = shift < 0 ? 0 : shift;
        const int bits = shift < 0 ? 4 : 12;
        const unsigned mask = (1u << bits) - 1u;
        for (int i = tid; i < SEL_BINS; i += SEL_THREADS) hist[i] = 0;
        __syncthreads();
        const int hi_shift = sh + bits;  // bits above the current digit must equal prefix
        for (int i = tid; i < n; i += SEL_THREADS) {
            const uint64_t key = cand[i];
            if (hi_shift >= 64 || (key >> hi_shift) == prefix) atomicAdd(&hist[(unsigned)(key >> sh) & mask], 1u);
        }
        __syncthreads();
        // bin scan: thread t owns bins [16 t, 16 t + 16); exclusive prefix over the threads by wave shuffles + 4 wave totals
        unsigned local = 0;
        for (int j = 0; j < SEL_BINS / SEL_THREADS; ++j) local += hist[tid * (SEL_BINS / SEL_THREADS) + j];
        unsigned incl = local;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off, 64);
            if ((tid & 63) >= off) incl += o;
        }
        if ((tid & 63) == 63) part[tid >> 6] = incl;
        __syncthreads();
        unsigned pre = incl - local;
        for (int w = 0; w < (tid >> 6); ++w) pre += part[w];
        if (pre <= want && want < pre + local) {  // exactly one thread: the wanted rank falls into its 16 bins
            unsigned acc = pre;
            int bin = tid * (SEL_BINS / SEL_THREADS);
            for (;; ++bin) {
                if (acc + hist[bin] > want) break;
                acc += hist[bin];
            }
            misc[1] = (unsigned)bin;
            misc[2] = want - acc;
        }
        __syncthreads();
        prefix = (prefix << bits) | (uint64_t)misc[1];
        want = misc[2];
        __syncthreads();
    }
    return prefix;
}
