// scan_coarse.hip -- the coarse GEMM + filter stage of the batched scan (scan_batched.h): 128-tile, 256-tile and persistent
// 256-tile kernels, their threshold epilogues and the launcher that chooses between them (gfx950).
//
// Roofline: MFMA bf16 / int8; algorithmic FLOPs = 2 * rows * ld * Qpad per phase launch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "scan_batched.h"

template <int METRIC>
__global__ __launch_bounds__(256) void scan_coarse_kernel(CoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;
    const int tile = xcd_remap(blockIdx.x, a.ntiles);
    const int rt = tile / a.qtiles, qt = tile - rt * a.qtiles;  // consecutive tiles share the corpus row panel
    const int64_t m0 = a.row0 + (int64_t)rt * G_BM;
    const int n0 = qt * G_BN;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm_tile_mainloop(a.Xb + m0 * a.ld, a.ld, 0, a.Qb, a.ld, n0, a.ld, smem, acc, w, lane);

    // acc[ni][mi][r] = <x[m0 + wm*64 + mi*16 + fr], q[n0 + wn*64 + ni*16 + 4*fq + r]>  (bf16 inputs)
    const int fr = lane & 15, fq = lane >> 4;
    float xn[4], xs[4];
    int64_t rows[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        rows[mi] = m0 + wm * 64 + mi * 16 + fr;
        xn[mi] = rows[mi] < a.row1 ? a.xnorm[rows[mi]] : 0.f;
        xs[mi] = (METRIC == SC_METRIC_COSINE) ? sc_inv_norm(xn[mi]) : 0.f;
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int q0 = n0 + wn * 64 + ni * 16 + 4 * fq;
        if (q0 >= a.Q) continue;
        const f32x4 tf = *reinterpret_cast<const f32x4*>(a.thr_fast + q0);  // thr_fast is allocated padded to 128
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            if (rows[mi] >= a.row1) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dot = acc[ni][mi][r];
                if (coarse_fast_value<METRIC, false>(dot, xn[mi], xs[mi], 0.f, 0.f) <= tf[r]) {
                    const int q = q0 + r;
                    uint64_t key;
                    if (q < a.Q && coarse_survivor<METRIC, false>(dot, xn[mi], 0.f, 0.f, a.qnorm[q], a.thr[q], (uint32_t)rows[mi], key)) {
                        const unsigned pos = atomicAdd(a.count + q, 1u);
                        if (pos < (unsigned)a.cap) a.surv[(size_t)q * a.cap + pos] = key;
                    }
                }
            }
        }
    }
}

// 256 x 256 tile variant (gemm_tile.h, second half): 8 waves, each 128 corpus rows x 64 queries.
// Per-query thresholds / norms of the workgroup's 256 queries sit in LDS behind the pipeline buffers, and a
// lane queues its (rare) hits in registers so that the global atomics that allocate list slots are issued
// back to back and their latency is paid once per tile, not once per hit.
#define COARSE_QLDS (4 * T_TILE_BYTES)  // byte offset of {thr_fast[256], thr[256], qnorm[256], xnorm[256], qscale[256], xscale[256], row bounds [256][2]} in LDS
#define COARSE_LDS_BYTES (4 * T_TILE_BYTES + 8 * 256 * 4)
// per-tile staging of the workgroup's 256 query thresholds / norms and the tile's 256 row norms (visible to everyone after
// the main loop's barriers)
// ROWS / QUERIES: which half of the staging a call does (the persistent kernel stages the query side only when its query tile
// changes and feeds the row side from registers it loaded a tile earlier)
// int8 stage: the two per-row constants of the epilogue's prefilter.  The fast test t <= tf_q is  acc >= (base_r - tf_q) R_r  with
// base_r = |x|^2 (L2) or 0, R_r = 1 / (c_r s_r s_q), c_r = 2 (L2), 1 (IP), 1/|x| (cosine) and ONE query scale s_q per batch; with the
// loosest tf of a lane's 16 queries the integer bound of a row is  Ti = (int)(A_r - tfmax' B_r)  -- one FMA per row block in the
// epilogue instead of a reciprocal, the slack arithmetic and the clamps, which every lane of every tile recomputed (8 waves x 8 row
// blocks; the epilogue is issue bound: 2.1-3.4 us per tile, profiles/r3k_coarse_trace.log).  A_r already carries every slack of the
// row side (4e-6 relative, 2 units for the bound's own rounding, 1 for the truncation), B_r > 0 always; rows beyond the phase's end
// (scale 0) get a bound nothing passes.
template <int METRIC>
static __device__ __forceinline__ void coarse_row_bound(float xn, float sx, float sq0, float& A, float& B) {
    if (!(sx > 0.f)) { A = 3.0e38f; B = 1.0e-30f; return; }
    const float c = (METRIC == SC_METRIC_L2) ? 2.0f * sx : (METRIC == SC_METRIC_COSINE) ? sx / sqrtf(xn) : sx;
    float R = __builtin_amdgcn_rcpf(c * sq0);
    if (!(R < 3.0e38f)) R = 3.0e38f;   // (cosine, |x| = 0: c = inf -> R = 0 is fine; c = 0 cannot happen with sx > 0 and finite xn)
    if (!(R > 1.0e-30f)) R = 1.0e-30f;
    float base = (METRIC == SC_METRIC_L2) ? xn * R : 0.f;
    if (!(fabsf(base) < 3.0e38f)) base = -3.0e38f;  // inf / NaN: let everything through to the precise test
    A = base - fabsf(base) * 4e-6f - 3.0f;
    B = R;
}
template <bool I8 = false, bool ROWS = true, bool QUERIES = true, int METRIC = SC_METRIC_L2>
static __device__ __forceinline__ void coarse256_stage(const CoarseArgs& a, int64_t m0, int n0, char* smem, int tid) {
    float* q_tf = reinterpret_cast<float*>(smem + COARSE_QLDS);
    if (ROWS && tid >= 256) {
        const int64_t row = m0 + (tid - 256);
        const float xn = row < a.row1 ? a.xnorm[row] : 1.0f;
        q_tf[768 + tid - 256] = xn;
        if (I8) {
            const float sx = row < a.row1 ? a.xscale[row] : 0.0f;
            q_tf[1280 + tid - 256] = sx;
            float A, B;
            coarse_row_bound<METRIC>(xn, sx, a.qscale[0], A, B);
            *reinterpret_cast<f32x2*>(q_tf + 1536 + 2 * (tid - 256)) = f32x2{A, B};
        }
    }
    if (QUERIES && tid < 256) {
        const int q = n0 + tid;
        q_tf[tid] = q < a.Q ? a.thr_fast[q] : -__builtin_inff();  // padding never passes (and does not loosen the lane's prefilter bound)
        q_tf[256 + tid] = q < a.Q ? a.thr[q] : -__builtin_inff();
        q_tf[512 + tid] = q < a.Q ? a.qnorm[q] : 1.0f;
        if (I8) q_tf[1024 + tid] = a.qscale[q];  // padded to Qpad
    }
}
// tile (rt, qt) of logical tile index `tile`: column-major walk inside groups of 8 row panels (as the encoder GEMMs once did)
static __device__ __forceinline__ void coarse256_coords(const CoarseArgs& a, int tile, int64_t& m0, int& n0) {
    const int G = 8, rtiles = a.ntiles / a.qtiles;
    const int gsz = G * a.qtiles, g = tile / gsz, r = tile - g * gsz;
    const int rows_here = (g * G + G <= rtiles) ? G : rtiles - g * G;
    m0 = a.row0 + (int64_t)(g * G + r % rows_here) * T_BM;
    n0 = (r / rows_here) * T_BN;
}
// Epilogue.  One compare per score against a per-row bound, a wave-uniform branch per group of 4 scores around the precise test.
// A variant without that branch -- every lane that passes the bound runs the precise test under its own exec mask and parks
// its key in a per-wave LDS list flushed once per tile -- was measured on the same box and lost (int8 stage 11.25 -> 12.28 ms,
// bf16 15.05 -> 16.2 ms per step, measurement pass r2f; logs not kept): the divergent bodies cost more than the uniform branch saves.
// So did a two-phase form (branch-free bound tests into a 32-bit group mask, DPP OR over the wave, then a loop over the set bits
// with the precise test present once and the accumulators fetched by a switch): the per-workgroup stamps (SC_COARSE_TRACE,
// profiles/r2j_coarse_trace.log) put this version at 3.4 / 4.4 us of epilogue per tile with 10 / 35 of 256 groups entering the
// precise test (0.46 us of that is wave skew, ~1.9 us the 32 bound tests: a wave64 VALU instruction issues over 4 cycles and two
// waves share a SIMD), the two-phase form at 3.4-3.7 / 5.5-6.2 us -- its loop body costs more per entered group than 32 unrolled
// copies do.  Removing the returning atomics changed nothing (4.3 vs 4.4 us).
// TRACE (SC_COARSE_TRACE): counts per workgroup / tile how many wave-groups entered the precise test, how many scores passed the fast
// test and how many survived (a.trace[.][4..6]); `tslot` is the caller's row of the trace
template <int METRIC, bool I8 = false, bool TRACE = false>
static __device__ __forceinline__ void coarse256_epilogue(const CoarseArgs& a, const f32x4 (&acc)[4][8], int64_t m0, int n0, char* smem, int w,
                                                          int lane, size_t tslot = 0) {
    const int wm = w >> 2, wn = w & 3;
    asm volatile("" : "+v"(lane));
    const float* q_tf = reinterpret_cast<const float*>(smem + COARSE_QLDS);
    const float* q_thr = q_tf + 256;
    const float* q_qn = q_tf + 512;
    const float* x_xn = q_tf + 768;  // |x|^2 of the tile's 256 corpus rows
    // acc[ni][mi][r] = <x[m0 + wm*128 + mi*16 + fr], q[n0 + wn*64 + ni*16 + 4*fq + r]>  (bf16 inputs)
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 tf[4], sq[4];  // sq: int8 stage only, the query scales of this lane's 16 columns
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        tf[ni] = *reinterpret_cast<const f32x4*>(q_tf + wn * 64 + ni * 16 + 4 * fq);
        if (I8) sq[ni] = *reinterpret_cast<const f32x4*>(q_tf + 1024 + wn * 64 + ni * 16 + 4 * fq);
    }
    float tfmax = -__builtin_inff();  // loosest fast threshold among this lane's 16 queries
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) tfmax = fmaxf(fmaxf(tfmax, fmaxf(tf[ni][0], tf[ni][1])), fmaxf(tf[ni][2], tf[ni][3]));
    // int8: the lane's side of the row bound (coarse_row_bound): tfmax with its own relative slack, rounded up
    const float tfm = fabsf(tfmax) < 3.0e38f ? fmaf(fabsf(tfmax), 4e-6f, tfmax) : tfmax;
    const f32x2* rowb = reinterpret_cast<const f32x2*>(q_tf + 1536);
    // hits of this lane: up to 4 queued (local query index, key); a 5th and later ones are flushed directly
    int nh = 0;
    int hq0 = 0, hq1 = 0, hq2 = 0, hq3 = 0;
    uint64_t hk0 = 0, hk1 = 0, hk2 = 0, hk3 = 0;
    // int8: a first, branch-free pass over the 8 row blocks -- bound, maximum of the lane's 16 scores, one ballot each -- collects
    // which row blocks hold anything at all; in the late phases of a batch (most of its tiles) none does and the epilogue ends here.
    // The per-row-block form below is ~2 KB of code per block, nearly all of it cold: its hot path hopped over 17 000 instructions
    // in eight jumps (2.1-2.3 us per tile with NOTHING passing, profiles/r3k_coarse_trace.log); this pass is ~150 contiguous ones.
    unsigned blockmask = 0xFFu;
    int TiA[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (I8) {
        blockmask = 0u;
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const f32x2 ab = rowb[wm * 128 + mi * 16 + fr];
            const float tl = fmaf(-tfm, ab[1], ab[0]);
            TiA[mi] = (int)__builtin_amdgcn_fmed3f(tl, -2.0e9f, 2.0e9f);
            int mx = max(max(__float_as_int(acc[0][mi][0]), __float_as_int(acc[0][mi][1])), max(__float_as_int(acc[0][mi][2]), __float_as_int(acc[0][mi][3])));
#pragma unroll
            for (int ni = 1; ni < 4; ++ni)
                mx = max(max(mx, max(__float_as_int(acc[ni][mi][0]), __float_as_int(acc[ni][mi][1]))), max(__float_as_int(acc[ni][mi][2]), __float_as_int(acc[ni][mi][3])));
            blockmask |= __any(mx >= TiA[mi]) ? (1u << mi) : 0u;
        }
        blockmask = __builtin_amdgcn_readfirstlane(blockmask);
        if (blockmask == 0u) return;
    }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        if (I8 && !(blockmask & (1u << mi))) continue;
        const int rl = wm * 128 + mi * 16 + fr;
        const int Ti = TiA[mi];  // int8 only
        const float xn = x_xn[rl];  // staged at kernel start; rows >= row1 hold +inf (L2) / 0 scale so that they never pass
        const float xs = (METRIC == SC_METRIC_COSINE) ? sc_inv_norm(xn) : 0.f;  // exact: the precise test below uses it too
        const float sx = I8 ? q_tf[1280 + rl] : 0.f;  // int8 stage: the integer dot is scaled by s_r s_q
        const float ar = (METRIC == SC_METRIC_L2) ? -2.0f * sx : (METRIC == SC_METRIC_COSINE) ? -sx * xs : -sx;
        // Prefilter: ONE compare per score.  The fast test t <= tf_q is  dot >= (base_r - tf_q) / c_r  with base_r = |x|^2 (L2) or
        // 0 and c_r = 2 (L2), 1 (IP), 1/|x| (cosine), times s_r s_q in the int8 stage, where every query of the batch shares one
        // scale (sc_launch_query_i8) -- so the right-hand side differs between this lane's 16 queries only through tf_q, and with
        // tfmax = max of those it is bounded below by a per-row constant.  Anything that passes is tested precisely below.
        float Tlb = 0.f;
        if (!I8) {
            Tlb = (METRIC == SC_METRIC_L2) ? 0.5f * (xn - tfmax) : (METRIC == SC_METRIC_COSINE) ? -tfmax / xs : -tfmax;
            Tlb = Tlb - fabsf(Tlb) * 4e-6f;  // rounding of this bound itself (the precise test has its own slack)
            if (!(Tlb == Tlb)) Tlb = -__builtin_inff();  // NaN (0 * inf on an all-zero row): let the precise test decide
        }
        // Round 3: first ONE test per row block -- the maximum of the lane's 16 scores (8 v_max3) against the bound, one wave-uniform
        // branch per 16 x 64 scores instead of four; the per-group tests below run only for the row blocks that pass (15-45 % of
        // them).  The bound tests were 1.9 us of a 3.4-4.4 us epilogue at ~28 vector instructions per row block (a wave64
        // instruction issues over 4 cycles, two waves share a SIMD); the common path is now 9.
        if (!I8) {
            float mx = fmaxf(fmaxf(acc[0][mi][0], acc[0][mi][1]), fmaxf(acc[0][mi][2], acc[0][mi][3]));
#pragma unroll
            for (int ni = 1; ni < 4; ++ni) mx = fmaxf(fmaxf(mx, fmaxf(acc[ni][mi][0], acc[ni][mi][1])), fmaxf(acc[ni][mi][2], acc[ni][mi][3]));
            if (!__any(mx >= Tlb)) continue;
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            // one uniform branch per group of 4 scores; taken by ~1 group in 500 once thresholds are tight
            bool g;
            if (I8) {
                // (__float_as_int, not __builtin_bit_cast(int, acc[ni][mi][r]): hipcc lowers the bit_cast of a vector-ELEMENT lvalue as
                // element 0 -- the first int8 build tested the wrong accumulators for three queries in four)
                // the group's maximum against the bound: 3 instructions instead of 4 compares and 3 ORs (a wave64 instruction issues
                // over 4 cycles, two waves share a SIMD, and a third of all row blocks get here: DESIGN.md section 4)
                const int gm = max(max(__float_as_int(acc[ni][mi][0]), __float_as_int(acc[ni][mi][1])),
                                   max(__float_as_int(acc[ni][mi][2]), __float_as_int(acc[ni][mi][3])));
                g = gm >= Ti;
            } else {
                g = (acc[ni][mi][0] >= Tlb) | (acc[ni][mi][1] >= Tlb) | (acc[ni][mi][2] >= Tlb) | (acc[ni][mi][3] >= Tlb);
            }
            if (!__any(g)) continue;
            if (TRACE && lane == 0) atomicAdd(&a.trace[tslot * 8 + 4], 1ull);
            f32x4 t;
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = coarse_fast_value<METRIC, I8>(acc[ni][mi][r], xn, xs, ar, I8 ? sq[ni][r] : 0.f);
            {
                const int64_t row = m0 + rl;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // (int8: entering the precise test on the integer bound alone -- it is a superset of this float test -- saved these
                    // 12 instructions per entered group but ran the precise test 1.3x as often: 7.94 -> 7.95 ms of kernels per step)
                    if (row < a.row1 && t[r] <= tf[ni][r]) {
                        if (TRACE) atomicAdd(&a.trace[tslot * 8 + 5], 1ull);
                        const int ql = wn * 64 + ni * 16 + 4 * fq + r;
                        uint64_t key;
                        if (coarse_survivor<METRIC, I8>(acc[ni][mi][r], xn, sx, I8 ? sq[ni][r] : 0.f, q_qn[ql], q_thr[ql], (uint32_t)row, key)) {  // q_thr = -inf for padded queries
                            if (TRACE) atomicAdd(&a.trace[tslot * 8 + 6], 1ull);
                            if (nh == 0) { hq0 = ql; hk0 = key; }
                            else if (nh == 1) { hq1 = ql; hk1 = key; }
                            else if (nh == 2) { hq2 = ql; hk2 = key; }
                            else if (nh == 3) { hq3 = ql; hk3 = key; }
                            else {
                                const unsigned pos = atomicAdd(a.count + n0 + ql, 1u);
                                if (pos < (unsigned)a.cap) a.surv[(size_t)(n0 + ql) * a.cap + pos] = key;
                            }
                            ++nh;
                        }
                    }
                }
            }
        }
    }
    if (!__any(nh > 0)) return;
    // allocate the queued hits' list slots with back-to-back atomics, then store
    unsigned p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    if (nh > 0) p0 = atomicAdd(a.count + n0 + hq0, 1u);
    if (nh > 1) p1 = atomicAdd(a.count + n0 + hq1, 1u);
    if (nh > 2) p2 = atomicAdd(a.count + n0 + hq2, 1u);
    if (nh > 3) p3 = atomicAdd(a.count + n0 + hq3, 1u);
    if (nh > 0 && p0 < (unsigned)a.cap) a.surv[(size_t)(n0 + hq0) * a.cap + p0] = hk0;
    if (nh > 1 && p1 < (unsigned)a.cap) a.surv[(size_t)(n0 + hq1) * a.cap + p1] = hk1;
    if (nh > 2 && p2 < (unsigned)a.cap) a.surv[(size_t)(n0 + hq2) * a.cap + p2] = hk2;
    if (nh > 3 && p3 < (unsigned)a.cap) a.surv[(size_t)(n0 + hq3) * a.cap + p3] = hk3;
}

// Epilogue for tiles in which MOST scores survive (the first phases of a batch: thresholds are still +inf or loose, a 256 x 256
// tile yields thousands of survivors).  The epilogue above allocates a list slot per hit with a returning global atomic -- four
// queued per lane, the rest one round trip each: the first six launches of a 10M-row batch (3.5 % of the rows) took 2.5 of its
// 10.9 ms (measurement pass r3l: 500, 644, 411, 243, 286, 407 us; one 256-row tile with 9 400 hits 230 us).  Here a tile makes ONE global
// atomic per query: pass 1 counts the hits per query in LDS (the pipeline buffers are dead), 256 threads reserve [base, base + n)
// of each query's list, pass 2 re-evaluates the same tests and writes each hit at base + an LDS ticket.  Same survivor set as
// the sparse epilogue (the same coarse_fast_value / coarse_survivor); the order inside a list differs, which the selection does not see.
// Those six launches now take 86, 86, 64, 58, 198, 553 us (measurement pass r3n), the step 10.7 -> 9.1 ms.
template <int METRIC, bool I8>
static __device__ __forceinline__ void coarse256_epilogue_dense(const CoarseArgs& a, const f32x4 (&acc)[4][8], int64_t m0, int n0, char* smem, int w,
                                                                int lane, int tid) {
    const int wm = w >> 2, wn = w & 3;
    asm volatile("" : "+v"(lane));
    const float* q_tf = reinterpret_cast<const float*>(smem + COARSE_QLDS);
    const float* q_thr = q_tf + 256;
    const float* q_qn = q_tf + 512;
    const float* x_xn = q_tf + 768;
    unsigned* cnt = reinterpret_cast<unsigned*>(smem);  // [256] hits per local query, then the tickets of pass 2
    unsigned* base = cnt + 256;                         // [256] first list slot of this tile's hits
    const int fr = lane & 15, fq = lane >> 4;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave is out of the main loop: the ring is free
    if (tid < 256) cnt[tid] = 0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    f32x4 tf[4], sq[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        tf[ni] = *reinterpret_cast<const f32x4*>(q_tf + wn * 64 + ni * 16 + 4 * fq);
        if (I8) sq[ni] = *reinterpret_cast<const f32x4*>(q_tf + 1024 + wn * 64 + ni * 16 + 4 * fq);
    }
    // the tests of coarse256_epilogue, score by score: fast test, then the precise one; key valid when it returns true
    auto hit = [&](int mi, int ni, int r, uint64_t& key) -> bool {
        const int rl = wm * 128 + mi * 16 + fr;
        const int64_t row = m0 + rl;
        const float xn = x_xn[rl];
        const float xs = (METRIC == SC_METRIC_COSINE) ? sc_inv_norm(xn) : 0.f;
        const float sx = I8 ? q_tf[1280 + rl] : 0.f;
        const float ar = (METRIC == SC_METRIC_L2) ? -2.0f * sx : (METRIC == SC_METRIC_COSINE) ? -sx * xs : -sx;
        const float accv = acc[ni][mi][r], sqv = I8 ? sq[ni][r] : 0.f;
        if (!(row < a.row1 && coarse_fast_value<METRIC, I8>(accv, xn, xs, ar, sqv) <= tf[ni][r])) return false;
        const int ql = wn * 64 + ni * 16 + 4 * fq + r;
        return coarse_survivor<METRIC, I8>(accv, xn, sx, sqv, q_qn[ql], q_thr[ql], (uint32_t)row, key);
    };
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint64_t key;
                if (hit(mi, ni, r, key)) __hip_atomic_fetch_add(&cnt[wn * 64 + ni * 16 + 4 * fq + r], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (tid < 256) {
        const unsigned c = cnt[tid];
        unsigned b = 0;
        if (c) b = atomicAdd(a.count + n0 + tid, c);  // (padded queries never hit: their threshold is -inf)
        base[tid] = b;
        cnt[tid] = 0;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint64_t key;
                if (hit(mi, ni, r, key)) {
                    const int ql = wn * 64 + ni * 16 + 4 * fq + r;
                    const unsigned pos = base[ql] + __hip_atomic_fetch_add(&cnt[ql], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (pos < (unsigned)a.cap) a.surv[(size_t)(n0 + ql) * a.cap + pos] = key;
                }
            }
}

// PP: 0 = one barrier per K-tile, 2..5 = the ping-pong main loop with that many half-tiles in flight (gemm_tile.h)
// DENSE: the two-pass epilogue above (launches whose tiles are expected to keep hundreds of survivors)
// TRACE (SC_COARSE_TRACE=1): time stamps of the workgroup and the sparse epilogue's counters in a.trace[blockIdx.x]
template <int METRIC, bool I8 = false, int PP = 4, bool DENSE = false, bool TRACE = false>
__global__ __launch_bounds__(512) void scan_coarse256_kernel(CoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t m0;
    int n0;
    if (TRACE && tid == 0) {
        a.trace[(size_t)blockIdx.x * 8 + 0] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
        a.trace[(size_t)blockIdx.x * 8 + 1] = (unsigned long long)wall_clock64();
    }
    coarse256_coords(a, xcd_remap(blockIdx.x, a.ntiles), m0, n0);
    // (requesting the first two K-tiles before this staging -- so that the two memory round trips overlap -- measured no change:
    // entry -> main loop done stayed at 11.2 us per int8 tile)
    coarse256_stage<I8, true, true, METRIC>(a, m0, n0, smem, tid);
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // int8 stage: a.ld counts PAIRS of int8 (the tile machinery addresses 2-byte elements), zero accumulators are zero i32 bits
    if constexpr (PP > 0) gemm_tile256_mainloop_pp<PP, 0, NoTailHook, I8>(a.Xb + m0 * a.ld, a.ld, 0, a.Qb, a.ld, n0, a.ld, smem, acc, w, lane);
    else gemm_tile256_mainloop<0, NoTailHook, I8>(a.Xb + m0 * a.ld, a.ld, 0, a.Qb, a.ld, n0, a.ld, smem, acc, w, lane);
    asm volatile("" ::: "memory");  // keep the epilogue's loads out of the register-tight main loop
    __builtin_amdgcn_sched_barrier(0);
    if (TRACE && tid == 0) a.trace[(size_t)blockIdx.x * 8 + 2] = (unsigned long long)wall_clock64();
    if constexpr (DENSE) coarse256_epilogue_dense<METRIC, I8>(a, acc, m0, n0, smem, w, lane, tid);
    else coarse256_epilogue<METRIC, I8, TRACE>(a, acc, m0, n0, smem, w, lane, blockIdx.x);
    if (TRACE) {
        __syncthreads();
        if (tid == 0) a.trace[(size_t)blockIdx.x * 8 + 3] = (unsigned long long)wall_clock64();
    }
}

// A first persistent variant (one workgroup per CU walking tiles b, b + grid, ..., the tail hook of tile t requesting K-tiles 0 and 1
// of tile t + grid under its last 32 MFMAs, but the row side of every tile -- norms, scales -- still fetched in front of it) lost
// a same-box A/B to this kernel: 64.7k -> 60.4k QPS.  The later form below, which also carries the row side one tile ahead and
// walks the tiles XCD by XCD, wins and is the default (scan_coarse256p_kernel); this kernel serves row strides below three K-tiles,
// the dense first phases and the A/B switches.

// ---- persistent form: one workgroup per CU walks its share of the tiles, and the LDS ring never drains between them: the last
// phases of a tile request the first two K-tiles of the NEXT tile into the slots that fall free (gemm_tile.h, PPNextTileHook), so
// a tile's first bytes (HBM latency: the corpus rows are read once) and a third of its fill travel under the previous tile's
// tail and threshold epilogue.  A tile is 6 (int8) or 12 (bf16) K-tiles at 768 dimensions: with one workgroup per launch slot the
// stamps read entry -> main loop done 11.6 us for 6.1 us of MFMAs, epilogue 4.2, 0.5 to the next workgroup
// (profiles/r3g_coarse_trace.log).  Tiles: XCD x owns a contiguous range of logical tiles (as xcd_remap gives it); its G / 8
// workgroups take consecutive tiles of it per round, i.e. one group of 8 row panels x 4 query tiles runs on one XCD at a time, as
// under hardware dispatch.  The per-tile thresholds / norms in LDS are double buffered (a wave may be a whole epilogue ahead).
static int g_coarse_wgs = 0, g_coarse_persistent = 1;  // sc_diag_set_option
int sc_scan_coarse_workgroups(void) { return g_coarse_wgs; }
void sc_scan_set_coarse_workgroups(int v) { g_coarse_wgs = v; }
void sc_scan_set_coarse_persistent(int v) { g_coarse_persistent = v; }
#define COARSE_QLDS_BYTES (8 * 256 * 4)
#define COARSEP_LDS_BYTES (4 * T_TILE_BYTES + 2 * COARSE_QLDS_BYTES)
template <int METRIC, bool I8, bool TRACE = false>
__global__ __launch_bounds__(512) void scan_coarse256p_kernel(CoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // this workgroup's tiles: lo + idx, lo + idx + per_round, ... below hi
    const int G = (int)gridDim.x, x = (int)blockIdx.x & 7, idx = (int)blockIdx.x >> 3, per_round = G >> 3;
    const int q8 = a.ntiles >> 3, r8 = a.ntiles & 7;
    const int lo = x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8, hi = lo + (x < r8 ? q8 + 1 : q8);
    int tile = lo + idx;
    if (tile >= hi) return;
    const int nk = a.ld / G_BK;
    uint32_t va[2], vw[2];
    pp_piece_offsets(a.ld, a.ld, w, lane, va, vw);
    PPNextTileHook hook;
    hook.a_kbytes = (uint32_t)(G_BK * 2); hook.a1_off = (uint32_t)(64 * a.ld * 2); hook.w1_off = (uint32_t)(32 * a.ld * 2);
    hook.w = w; hook.smem = smem;
    int64_t m0;
    int n0;
    coarse256_coords(a, tile, m0, n0);
    hook.ra = __builtin_amdgcn_make_buffer_rsrc((void*)(a.Xb + m0 * a.ld), 0, -1, 0x00020000);
    hook.rw = __builtin_amdgcn_make_buffer_rsrc((void*)(a.Qb + (size_t)n0 * a.ld), 0, -1, 0x00020000);
#pragma unroll
    for (int h = 0; h < 8; ++h) hook.coop(h, h, va, vw);  // the first tile's first two K-tiles, in ring order from parity 0
    int par = 0, it = 0;
    // Staging without a global round trip in front of every tile: the row side (|x|^2 and the int8 row scale of the tile's 256 rows,
    // threads 256..511) is loaded one tile ahead into two registers and only WRITTEN to LDS here (the compiler guards that write with
    // s_waitcnt vmcnt(0) in waves 4-7, which also waits for the prefetched half-tiles; an LDS-DMA form of this staging without that
    // wait was built and measured: no gain -- 6.98 -> 6.92 ms of kernels with the epilogue switched off, slower with it); the query side (thresholds, norms,
    // scales of the 256 queries) is staged again only when the query tile changes -- a workgroup's tiles are one round (a
    // multiple of the group of 8 row panels x all query tiles, at 1 024 queries and 256 CUs) apart, so it never does there.
    float* q_cur = reinterpret_cast<float*>(smem + COARSE_QLDS);
    float xn_next = 1.0f, xs_next = 0.0f;
    const float sq0_batch = I8 ? a.qscale[0] : 1.0f;  // every query of a batch shares one scale (sc_launch_query_i8)
    if (tid >= 256) {
        const int64_t row = m0 + (tid - 256);
        xn_next = row < a.row1 ? a.xnorm[row] : 1.0f;
        if (I8) xs_next = row < a.row1 ? a.xscale[row] : 0.0f;
    }
    int n0_even = -1, n0_odd = -1;  // query tile staged in either copy
#pragma unroll 1
    for (;; ++it) {
        char* smem_q = smem + (it & 1) * COARSE_QLDS_BYTES;  // this tile's thresholds / norms (the other copy may still be read)
        q_cur = reinterpret_cast<float*>(smem_q + COARSE_QLDS);
        if (tid >= 256) {
            q_cur[768 + tid - 256] = xn_next;
            if (I8) {
                q_cur[1280 + tid - 256] = xs_next;
                float A, B;
                coarse_row_bound<METRIC>(xn_next, xs_next, sq0_batch, A, B);
                *reinterpret_cast<f32x2*>(q_cur + 1536 + 2 * (tid - 256)) = f32x2{A, B};
            }
        }
        if (((it & 1) ? n0_odd : n0_even) != n0) {
            coarse256_stage<I8, false, true>(a, m0, n0, smem_q, tid);
            if (it & 1) n0_odd = n0;
            else n0_even = n0;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int next = tile + per_round;
        const bool more = next < hi;
        int64_t m0n = m0;
        int n0n = n0;
        if (more) coarse256_coords(a, next, m0n, n0n);  // the last tile "prefetches" itself: the request counts of the loop stay what they are
        if (more && tid >= 256) {  // the next tile's row side: in flight under this tile's main loop
            const int64_t row = m0n + (tid - 256);
            xn_next = row < a.row1 ? a.xnorm[row] : 1.0f;
            if (I8) xs_next = row < a.row1 ? a.xscale[row] : 0.0f;
        }
        hook.ra = __builtin_amdgcn_make_buffer_rsrc((void*)(a.Xb + m0n * a.ld), 0, -1, 0x00020000);
        hook.rw = __builtin_amdgcn_make_buffer_rsrc((void*)(a.Qb + (size_t)n0n * a.ld), 0, -1, 0x00020000);
        f32x4 acc[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (TRACE && tid == 0) {
            a.trace[(size_t)tile * 8 + 0] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
            a.trace[(size_t)tile * 8 + 1] = (unsigned long long)wall_clock64();
        }
        gemm_tile256_mainloop_pp<4, 0, PPNextTileHook, I8, true>(a.Xb + m0 * a.ld, a.ld, 0, a.Qb, a.ld, n0, a.ld, smem, acc, w, lane, hook, G_BK, par);
        par ^= nk & 1;
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (TRACE && tid == 0) a.trace[(size_t)tile * 8 + 2] = (unsigned long long)wall_clock64();
        // (a query tile without a real query has no survivors.  Qpad rounds Q up to the tile, so the test is always true today; it also
        // keeps a wave-uniform branch in front of the epilogue, without which hipcc spills 7-12 VGPRs per lane in the int8 kernels
        // instead of 4: profiles/scan_split_kernels.log)
        if (n0 < a.Q) coarse256_epilogue<METRIC, I8, TRACE>(a, acc, m0, n0, smem_q, w, lane, tile);
        if (TRACE && tid == 0) a.trace[(size_t)tile * 8 + 3] = (unsigned long long)wall_clock64();
        if (!more) break;
        tile = next;
        m0 = m0n;
        n0 = n0n;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last tile's self-prefetch must not outlive the workgroup's LDS
}

template <int METRIC, bool I8>
static void launch_coarse256(const CoarseArgs& a, hipStream_t s, bool dense) {
    static const char* envd = getenv("SC_COARSE_DENSE");  // A/B: 0 = the sparse epilogue everywhere
    static const bool dense_ok = envd ? atoi(envd) != 0 : true;
    if (dense && dense_ok && a.ld >= 2 * G_BK) {
        static ScDeviceOnce once_d;
        sc_device_once(once_d, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256_kernel<METRIC, I8, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSE_LDS_BYTES); });
        hipLaunchKernelGGL((scan_coarse256_kernel<METRIC, I8, 4, true>), dim3((unsigned)a.ntiles), dim3(512), COARSE_LDS_BYTES, s, a);
        return;
    }
    static const char* env = getenv("SC_COARSE_PP");  // A/B: 0 = the one-barrier main loop
    static const bool pp = (env ? atoi(env) : 4) != 0;
    static ScDeviceOnce once;  // per instantiation and device
    sc_device_once(once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256_kernel<METRIC, I8, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSE_LDS_BYTES);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256_kernel<METRIC, I8, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSE_LDS_BYTES);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256p_kernel<METRIC, I8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSEP_LDS_BYTES);
    });
    static const char* envp = getenv("SC_COARSE_PERSIST");  // A/B: 0 = one workgroup per tile
    static const bool persist_env = envp ? atoi(envp) != 0 : true;
    if (pp && persist_env && g_coarse_persistent && a.ld >= 3 * G_BK) {
        const int cus = sc_device_cus(), cus8 = cus >= 8 ? (cus & ~7) : 8;
        const int wgs = g_coarse_wgs > 0 ? ((g_coarse_wgs + 7) & ~7) : cus8;  // a multiple of 8: blocks b, b + 8, ... share an XCD
        hipLaunchKernelGGL((scan_coarse256p_kernel<METRIC, I8>), dim3((unsigned)wgs), dim3(512), COARSEP_LDS_BYTES, s, a);
        return;
    }
    if (pp && a.ld >= 2 * G_BK) hipLaunchKernelGGL((scan_coarse256_kernel<METRIC, I8, 4>), dim3((unsigned)a.ntiles), dim3(512), COARSE_LDS_BYTES, s, a);
    else hipLaunchKernelGGL((scan_coarse256_kernel<METRIC, I8, 0>), dim3((unsigned)a.ntiles), dim3(512), COARSE_LDS_BYTES, s, a);
}

// i8: Xb / Qb are the int8 shadows with rows of ld8 bytes (`ld` is then ld8), xscale / qscale their per-row scales; the batch must be
// padded to 256 queries (the int8 stage only exists on the 256 x 256 tile)
// SC_COARSE_TRACE: one traced launch, summarised on stderr (mean us per workgroup: entry -> main loop done -> end, and the idle gap
// between consecutive workgroups of one CU)
static void coarse256_trace(CoarseArgs a, bool i8, hipStream_t s) {
    unsigned long long* dev = nullptr;
    const size_t words = (size_t)a.ntiles * 8;
    if (hipMalloc(&dev, words * 8) != hipSuccess) return;
    (void)hipMemsetAsync(dev, 0, words * 8, s);
    a.trace = dev;
    static const int mode = atoi(getenv("SC_COARSE_TRACE"));  // 5: the persistent kernel (int8 stage), anything else: one workgroup per tile
    if (i8 && mode == 5) {  // stamps of wave 0 per tile (entry = its own loop start)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256p_kernel<SC_METRIC_L2, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSEP_LDS_BYTES);
        hipLaunchKernelGGL((scan_coarse256p_kernel<SC_METRIC_L2, true, true>), dim3(256), dim3(512), COARSEP_LDS_BYTES, s, a);
    } else if (i8) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256_kernel<SC_METRIC_L2, true, 4, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSE_LDS_BYTES);
        hipLaunchKernelGGL((scan_coarse256_kernel<SC_METRIC_L2, true, 4, false, true>), dim3((unsigned)a.ntiles), dim3(512), COARSE_LDS_BYTES, s, a);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse256_kernel<SC_METRIC_L2, false, 4, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COARSE_LDS_BYTES);
        hipLaunchKernelGGL((scan_coarse256_kernel<SC_METRIC_L2, false, 4, false, true>), dim3((unsigned)a.ntiles), dim3(512), COARSE_LDS_BYTES, s, a);
    }
    std::vector<unsigned long long> h(words);
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(h.data(), dev, words * 8, hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    std::map<unsigned long long, std::vector<std::pair<unsigned long long, unsigned long long>>> per_cu;
    double ml = 0, ep = 0, taken = 0, fastpass = 0, hits = 0;
    unsigned long long t_first = ~0ull, t_last = 0;
    for (int t = 0; t < a.ntiles; ++t) {
        const unsigned long long* r = &h[(size_t)t * 8];
        taken += (double)r[4]; fastpass += (double)r[5]; hits += (double)r[6];
        ml += (double)(r[2] - r[1]);
        ep += (double)(r[3] - r[2]);
        // HW_ID: wave 3:0, simd 5:4, pipe 7:6, cu 11:8, sh 12, se 15:13; XCC_ID low bits of the high word
        per_cu[(r[0] >> 32) << 16 | ((r[0] >> 8) & 0xFF)].push_back({r[1], r[3]});
        t_first = r[1] < t_first ? r[1] : t_first;
        t_last = r[3] > t_last ? r[3] : t_last;
    }
    double gap = 0;
    size_t gaps = 0;
    for (auto& kv : per_cu) {
        auto& v = kv.second;
        std::sort(v.begin(), v.end());
        for (size_t i = 1; i < v.size(); ++i) { gap += (double)((long long)v[i].first - (long long)v[i - 1].second); ++gaps; }
    }
    fprintf(stderr, "[coarse trace] %s tiles %d on %zu CUs, launch %.1f us: per tile entry->mainloop done %.2f us, epilogue %.2f us, gap to the next workgroup of the CU %.2f us; per tile: %.1f of 256 wave-groups entered the precise test, %.1f scores passed the fast test, %.1f survivors\n",
            i8 ? "int8" : "bf16", a.ntiles, per_cu.size(), (double)(t_last - t_first) / 100.0, ml / a.ntiles / 100.0, ep / a.ntiles / 100.0, gaps ? gap / gaps / 100.0 : 0.0, taken / a.ntiles, fastpass / a.ntiles, hits / a.ntiles);
}

void sc_launch_scan_coarse(int metric, const void* Xb, const float* xnorm, int64_t row0, int64_t row1, int ld, const void* Qb,
                           const float* qnorm, int Q, int Qpad, const float* thr, const float* thr_fast, uint64_t* surv, unsigned* count,
                           int cap, hipStream_t s, bool i8, const float* xscale, const float* qscale, bool dense, void* hit_scratch, size_t hit_bytes) {
    CoarseArgs a;
    a.Xb = (const bf16_t*)Xb; a.xnorm = xnorm; a.row0 = row0; a.row1 = row1; a.ld = i8 ? ld / 2 : ld; a.Qb = (const bf16_t*)Qb; a.qnorm = qnorm;
    a.Q = Q; a.thr = thr; a.thr_fast = thr_fast; a.surv = surv; a.count = count; a.cap = cap; a.xscale = xscale; a.qscale = qscale;
    static const char* env64 = getenv("SC_COARSE64");  // A/B: 0 = small batches through the 256-query tiles
    if (i8 && !dense && hit_scratch && (row0 % T_BM) == 0 && sc_scan_coarse64_supported(Q, ld, hit_bytes) && !(env64 && env64[0] == '0') && !getenv("SC_COARSE_TRACE")) {
        a.qtiles = 1;
        a.ntiles = (int)((row1 - row0 + T_BM - 1) / T_BM);
        a.trace = nullptr;
        sc_launch_coarse64s(metric, a, s, hit_scratch, hit_bytes);
        return;
    }
    if ((Qpad % T_BN) == 0 && (row0 % T_BM) == 0) {  // large batches: 256 x 256 tiles (corpus rows are padded to 256)
        a.qtiles = Qpad / T_BN;
        a.ntiles = (int)(((row1 - row0 + T_BM - 1) / T_BM) * a.qtiles);
        a.trace = nullptr;
        static const bool trace = getenv("SC_COARSE_TRACE") != nullptr;  // diagnostic: per-workgroup time stamps of the large L2 launches -> stderr
        static const int trace_min = [] { const char* e = getenv("SC_COARSE_TRACE_MIN"); return e ? atoi(e) : 20000; }();
        if (trace && metric == SC_METRIC_L2 && a.ntiles >= trace_min) {
            coarse256_trace(a, i8, s);
            return;
        }
        sc_dispatch_metric(metric, [&](auto m) {
            if (i8) launch_coarse256<m.value, true>(a, s, dense);
            else launch_coarse256<m.value, false>(a, s, dense);
        });
        return;
    }
    a.qtiles = Qpad / G_BN;
    const int64_t rtiles = (row1 - row0 + G_BM - 1) / G_BM;
    a.ntiles = (int)(rtiles * a.qtiles);
    const size_t lds = 4 * G_TILE_BYTES;
    static ScDeviceOnce once128;
    sc_device_once(once128, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse_kernel<SC_METRIC_IP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse_kernel<SC_METRIC_L2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse_kernel<SC_METRIC_COSINE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    dim3 grid((unsigned)a.ntiles), block(256);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_coarse_kernel<m.value>, grid, block, lds, s, a); });
}
