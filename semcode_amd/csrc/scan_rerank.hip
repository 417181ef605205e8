// scan_rerank.hip -- the exact side of the batched scan (scan_batched.h): f32 re-rank of the coarse candidates in the canonical
// summation order, the certificate, and the thresholds derived from exact scores (collect pass, tightening) (gfx950).
//
// Roofline: HBM latency (scattered candidate rows, 128 per query and block).
#include "scan_batched.h"

int sc_batched_kprime(void) { return KPRIME; }
int sc_batched_kprime8(void) { return KPRIME8; }

// ------------------------------------------------------------------ exact re-rank + certificate
// One 128-thread workgroup per query: thread j re-scores candidate j with the canonical f32 fmaf chain.  The 128 candidate rows
// are scattered over the corpus; read row-per-thread, every load instruction touched 64 different cache lines and the kernel
// took 0.34 ms per 1024 queries.  So the rows are fetched cooperatively, 64 floats of all 128 rows at a time (16 lanes x 16 B
// = one 256-byte row segment per load), through an LDS tile [128][64 + 4] (the pad keeps the row-per-thread ds_read_b128 of
// the chain conflict-free), the next tile's loads in flight while this one is multiplied.  The chain itself is unchanged:
// k = 16 t + 4 g + c, c outer, g inner -- bit-identical scores.
#define RR_STRIDE 68  // floats per LDS row

// The certificate: is the k-th exact key provably better than every row that is NOT a candidate?  Such a row has coarse
// v-score >= tau, hence exact v-score >= tau - eps with
//   |coarse dot - exact dot| <= |x - xc| |q| + |xc| |q - qc| + accumulation noise   (Cauchy-Schwarz on the ACTUAL rounding
// residuals of the coarse operands xc, qc -- bf16 or scaled int8; bits = {max |x|^2, max |x - xc|^2, max |x - xc|^2 / |x|^2}
// over the corpus, qres = |q - qc|^2).  The int8 dot itself is exact; its scaling to f32 rounds three times, which the
// ld * 1.2e-7 term (sized for the f32 accumulation of the bf16 stage) covers many times over.
template <int METRIC>
static __device__ __forceinline__ float certificate_eps(const unsigned* __restrict__ bits, float qnorm2, float qres2, int ld) {
    const float xmax = sqrtf(__builtin_bit_cast(float, bits[0]));
    const float xres = sqrtf(__builtin_bit_cast(float, bits[1]));
    const float qn = sqrtf(qnorm2);
    const float ddot = xres * qn + (xmax + xres) * sqrtf(qres2) + (float)ld * 1.2e-7f * (xmax + xres) * qn;
    float eps;
    if (METRIC == SC_METRIC_L2) eps = 2.0f * ddot;
    else if (METRIC == SC_METRIC_COSINE) {  // relative form: |x - xc|/|x| + (1 + .)|q - qc|/|q|
        const float relx = sqrtf(__builtin_bit_cast(float, bits[2]));
        eps = relx + (1.0f + relx) * (sqrtf(qres2) / fmaxf(qn, 1e-30f)) + (float)ld * 1.2e-7f * (1.0f + relx);
    } else eps = ddot;
    return eps * 1.01f + 1e-6f;
}
template <int METRIC>
static __device__ __forceinline__ bool certified(uint64_t kth_key, const unsigned* __restrict__ bits, float qnorm2, float qres2, int ld, float tau) {
    const float sc = sc_key_score(METRIC, kth_key);
    const float vk = (METRIC == SC_METRIC_L2) ? sc : -sc;
    return vk + certificate_eps<METRIC>(bits, qnorm2, qres2, ld) < tau;
}
// SPLIT (int8 stage, KPRIME8 candidates): blockIdx.y selects a block of 128 candidates, the exact keys go to ekeys [Q][kp] and
// scan_finalize_kernel sorts them and evaluates the certificate.
template <int METRIC, bool SPLIT = false>
__global__ __launch_bounds__(KPRIME) void scan_rerank_kernel(const float* __restrict__ X, const float* __restrict__ xnorm, int ld,
                                                          const float* __restrict__ Qp, const float* __restrict__ qnorm,
                                                          const uint64_t* __restrict__ best, const float* __restrict__ thr,
                                                          const unsigned* __restrict__ xnorm_max_bits, const float* __restrict__ qres,
                                                          const int* __restrict__ overflow, int k,
                                                          int64_t row_base, const uint32_t* __restrict__ perm, float* __restrict__ out_dist,
                                                          int64_t* __restrict__ out_rows, int* __restrict__ flags, int kp = KPRIME,
                                                          uint64_t* __restrict__ ekeys = nullptr, const int* __restrict__ ncand = nullptr) {
    static_assert(KPRIME == 128, "the cooperative tile load assumes 128 candidates = 128 threads");
    __shared__ uint64_t keys[KPRIME];
    __shared__ uint32_t rowid[KPRIME];
    __shared__ __attribute__((aligned(16))) float tile[KPRIME * RR_STRIDE];
    __shared__ __attribute__((aligned(16))) float qch[64];
    const int q = blockIdx.x, lane = threadIdx.x;
    // ncand (SPLIT; the widened re-rank of the IVF coarse stage): only the first ncand[q] of the kp slots hold keys
    const int nc = (SPLIT && ncand) ? ncand[q] : kp;
    if (SPLIT && (int)blockIdx.y * KPRIME >= nc) return;
    const uint64_t ck = (SPLIT ? (int)blockIdx.y * KPRIME : 0) + lane < nc ? best[(size_t)q * kp + (SPLIT ? blockIdx.y * KPRIME : 0) + lane] : SC_KEY_MAX;
    rowid[lane] = ck != SC_KEY_MAX ? (uint32_t)ck : 0u;  // padding slots re-score row 0 and are discarded below
    __syncthreads();
    const int seg = lane & 15, r0 = lane >> 4;  // this thread fetches 16-byte piece `seg` of rows r0, r0 + 8, ...
    const float* qv = Qp + (size_t)q * ld;
    f32x4 nxt[16];
    float nq = 0.f;
    auto fetch = [&](int ch) {
#pragma unroll
        for (int i = 0; i < 16; ++i) nxt[i] = *reinterpret_cast<const f32x4*>(X + (size_t)rowid[r0 + 8 * i] * ld + ch * 64 + seg * 4);
        if (lane < 64) nq = qv[ch * 64 + lane];
    };
    fetch(0);
    float acc = 0.f;
    const int nch = ld >> 6;
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();  // everyone is done with the previous tile
#pragma unroll
        for (int i = 0; i < 16; ++i) *reinterpret_cast<f32x4*>(tile + (r0 + 8 * i) * RR_STRIDE + seg * 4) = nxt[i];
        if (lane < 64) qch[lane] = nq;
        __syncthreads();
        if (ch + 1 < nch) fetch(ch + 1);
        const float* xr = tile + lane * RR_STRIDE;
#pragma unroll
        for (int t = 0; t < 64; t += 16) {
            f32x4 xa[4], qa[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                xa[g] = *reinterpret_cast<const f32x4*>(xr + t + 4 * g);
                qa[g] = *reinterpret_cast<const f32x4*>(qch + t + 4 * g);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc = fmaf(xa[g][c], qa[g][c], acc);
        }
    }
    uint64_t ek = SC_KEY_MAX;
    if (ck != SC_KEY_MAX) {
        const uint32_t row = (uint32_t)ck;
        ek = sc_make_key<METRIC>(sc_score<METRIC>(acc, xnorm[row], qnorm[q]), perm ? perm[row] : row);  // ties: reported row id
    }
    if (SPLIT) {
        ekeys[(size_t)q * kp + blockIdx.y * KPRIME + lane] = ek;
        return;
    }
    keys[lane] = ek;
    __syncthreads();
    int rank = 0;
    int have = 0;
    for (int j = 0; j < KPRIME; ++j) {
        const uint64_t o = keys[j];
        rank += (o < ek) ? 1 : 0;
        have += (o != SC_KEY_MAX) ? 1 : 0;
    }
    __syncthreads();
    if (ek != SC_KEY_MAX) keys[rank] = ek;  // unique keys -> a permutation of the first `have` slots
    __syncthreads();
    if (lane < k) {
        const size_t o = (size_t)q * k + lane;
        if (lane < have) {
            out_dist[o] = sc_key_score(METRIC, keys[lane]);
            out_rows[o] = row_base + (int64_t)(uint32_t)keys[lane];
        } else {
            out_dist[o] = (METRIC == SC_METRIC_L2) ? __builtin_inff() : -__builtin_inff();
            out_rows[o] = -1;
        }
    }
    if (lane == 0) {
        int bad = overflow[q];
        if (have == KPRIME) {  // otherwise every row of the corpus is a candidate: nothing can be missing
            const int kk = k < have ? k : have;
            if (!certified<METRIC>(keys[kk - 1], xnorm_max_bits, qnorm[q], qres[q], ld, thr[q])) bad = 1;
        }
        flags[q] = bad;
    }
}

// int8 stage: the KPRIME8 exact keys of one query (scan_rerank_kernel<.., SPLIT>) -> sorted top-k + certificate
template <int METRIC>
__global__ __launch_bounds__(256) void scan_finalize_kernel(const uint64_t* __restrict__ ekeys, int kp, const float* __restrict__ qnorm,
                                                             const float* __restrict__ thr, const unsigned* __restrict__ xnorm_max_bits,
                                                             const float* __restrict__ qres, const int* __restrict__ overflow, int ld, int k,
                                                             int64_t row_base, float* __restrict__ out_dist, int64_t* __restrict__ out_rows,
                                                             int* __restrict__ flags) {
    __shared__ uint64_t keys[KPRIME8], sorted[KPRIME8];
    __shared__ int s_have;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_have = 0;
    for (int i = tid; i < kp; i += 256) {
        keys[i] = ekeys[(size_t)q * kp + i];
        sorted[i] = SC_KEY_MAX;
    }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < kp; i += 256) {
        const uint64_t key = keys[i];
        if (key == SC_KEY_MAX) continue;
        int rank = 0;
        for (int j = 0; j < kp; ++j) rank += (keys[j] < key) ? 1 : 0;  // exact keys are unique (row id in the low word)
        sorted[rank] = key;
        ++mine;
    }
    if (mine) atomicAdd(&s_have, mine);
    __syncthreads();
    const int have = s_have;
    if (tid < k) {
        const size_t o = (size_t)q * k + tid;
        if (tid < have) {
            out_dist[o] = sc_key_score(METRIC, sorted[tid]);
            out_rows[o] = row_base + (int64_t)(uint32_t)sorted[tid];
        } else {
            out_dist[o] = (METRIC == SC_METRIC_L2) ? __builtin_inff() : -__builtin_inff();
            out_rows[o] = -1;
        }
    }
    if (tid == 0) {
        int bad = overflow[q];
        if (have == kp) {
            const int kk = k < have ? k : have;
            if (!certified<METRIC>(sorted[kk - 1], xnorm_max_bits, qnorm[q], qres[q], ld, thr[q])) bad = 1;
        }
        flags[q] = bad;
    }
}

// ---- the collect pass (second chance of a query whose certificate failed) ------------------------------------------------------------
// The certificate compares the k-th exact score with the kp-th best COARSE score; it fails when more than kp rows are within the
// coarse error of the k-th neighbour (clustered corpora: a whole cluster is).  The failed pass still leaves a true upper bound of
// the k-th score: vk, the k-th exact score among its candidates.  A row can only belong to the result if its exact v-score is
// <= vk, i.e. its coarse v-score <= vk + eps =: T.  The collect pass runs the same coarse kernel once more over all rows with the
// FIXED threshold T (no selection, no shrinking), keeps every row that passes (up to BATCH_CAP per query), re-scores them all exactly
// and takes the exact top-k: correct by construction -- no candidate count to exceed.  Only a query with more than BATCH_CAP rows
// within T goes on to the next stage.  10M x 768 in 4096 clusters of spread 0.1: every query used to end in the exact scan
// (347 ms per 1024-query batch, profiles/r3t_clustered_probe.log); see DESIGN.md section 4 for what it takes now.
template <int METRIC>
__global__ __launch_bounds__(256) void scan_collect_bound_kernel(const float* __restrict__ prev_dist, int k, const float* __restrict__ qnorm,
                                                                  const float* __restrict__ qres, const unsigned* __restrict__ bits, int ld,
                                                                  float* __restrict__ thr, float* __restrict__ thr_fast, int* __restrict__ flags, int Q) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const float d = prev_dist[(size_t)q * k + (k - 1)];
    const float vk = (METRIC == SC_METRIC_L2) ? d : -d;
    const bool ok = fabsf(vk) < 3.0e38f;  // fewer than k candidates (+-inf) or NaN: nothing to bound with
    float t = -__builtin_inff(), tf = -__builtin_inff();
    if (ok) {
        t = vk + certificate_eps<METRIC>(bits, qnorm[q], qres[q], ld);
        tf = fast_threshold<METRIC>(t, qnorm[q]);
    }
    thr[q] = t;
    thr_fast[q] = tf;
    flags[q] = ok ? 0 : 1;
}
// ---- thresholds from EXACT scores before the large phases ---------------------------------------------------------------------------
// Between phases the threshold of a query is its kp-th best coarse key; a phase of 3 r0 new rows then yields 3 kp survivors per
// query (kp = 512: 1 536), each of which costs the threshold epilogue a trip through its precise test -- 1.3 of the 7.9 ms of coarse
// kernels per step, most of it in the last two phases (94 % of the rows).  But a row matters only if its coarse score is within
// eps of the k-th EXACT score, and far fewer than kp rows are (~150 on the Gaussian benchmark: what the certificate needs kp = 512
// for is the worst query, not the typical one).  So before a large phase the 128 best of the kp candidates are re-scored exactly
// (0.4 GB of scattered rows) and the threshold becomes  min(kp-th coarse key, k-th exact score + eps (+ a hair))  -- eps is the
// certificate's own bound, so the cut is one the certificate accepts: a row dropped by it has coarse > v_k + eps, i.e. exact > v_k.
// thr_cut keeps the smallest cut ever applied to a query; the certificate compares with min(final kp-th key, thr_cut).
template <int METRIC>
__global__ __launch_bounds__(128) void scan_tighten_kernel(const uint64_t* __restrict__ ekeys, int kp, int k, const float* __restrict__ qnorm,
                                                            const float* __restrict__ qres, const unsigned* __restrict__ bits, int ld,
                                                            float* __restrict__ thr, float* __restrict__ thr_fast, float* __restrict__ thr_cut) {
    __shared__ uint64_t keys[512];  // kp = 128 (k <= 64) or 512 (k <= 256: every candidate of the int8 stage)
    __shared__ float s_v;
    const int q = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < kp; i += 128) keys[i] = ekeys[(size_t)q * kp + i];
    if (tid == 0) s_v = __builtin_inff();
    __syncthreads();
    for (int i = tid; i < kp; i += 128) {
        const uint64_t key = keys[i];
        if (key == SC_KEY_MAX) continue;
        int rank = 0;
        for (int j = 0; j < kp; ++j) rank += keys[j] < key ? 1 : 0;  // exact keys are unique (row id in the low word)
        if (rank == k - 1) {
            const float sc = sc_key_score(METRIC, key);
            s_v = (METRIC == SC_METRIC_L2) ? sc : -sc;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float t = thr[q];
        const float vk = s_v;
        if (vk < 3.0e38f) {
            const float eps = certificate_eps<METRIC>(bits, qnorm[q], qres[q], ld);
            const float cut = (vk + eps) + fabsf(vk + eps) * 2e-6f + 1e-30f;  // strictly above v_k + eps: the certificate's "<" must hold when v_k does not improve
            t = fminf(t, cut);
        }
        t = fminf(t, thr_cut[q]);
        thr_cut[q] = t;
        thr[q] = t;
        float tf = __builtin_inff();
        if (t < __builtin_inff()) tf = fast_threshold<METRIC>(t, qnorm[q]);
        thr_fast[q] = tf;
    }
}
// the certificate of the wide form: the k-th exact score (out_dist, already final) + eps below the threshold, or nothing was ever dropped
template <int METRIC>
__global__ __launch_bounds__(256) void scan_wide_certify_kernel(const float* __restrict__ out_dist, int k, const float* __restrict__ qnorm, const float* __restrict__ qres,
                                                                 const unsigned* __restrict__ bits, int ld, const float* __restrict__ thr,
                                                                 const int* __restrict__ overflow, int* __restrict__ flags, int Q) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    int bad = overflow[q];
    const float tau = thr[q];
    if (tau < __builtin_inff()) {
        const float d = out_dist[(size_t)q * k + (k - 1)];
        const float vk = (METRIC == SC_METRIC_L2) ? d : -d;
        if (!(vk + certificate_eps<METRIC>(bits, qnorm[q], qres[q], ld) < tau)) bad = 1;
    }
    flags[q] = bad;
}

// ------------------------------------------------------------------ launchers
// kp = KPRIME: one fused kernel; kp = KPRIME8 (int8 stage): blocks of 128 candidates re-scored into ekeys [Q][kp], then sorted
void sc_launch_scan_rerank(int metric, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, const uint64_t* best,
                           const float* thr, const unsigned* xnorm_max_bits, const float* qres, const int* overflow, int Q, int k,
                           int64_t row_base, const uint32_t* perm, float* out_dist, int64_t* out_rows, int* flags, hipStream_t s, int kp,
                           uint64_t* ekeys) {
    sc_dispatch_metric(metric, [&](auto m) {
        if (kp == KPRIME) {
            hipLaunchKernelGGL((scan_rerank_kernel<m.value, false>), dim3((unsigned)Q), dim3(KPRIME), 0, s, X, xnorm, ld, Qp, qnorm, best, thr, xnorm_max_bits, qres,
                               overflow, k, row_base, perm, out_dist, out_rows, flags, kp, (uint64_t*)nullptr);
            return;
        }
        hipLaunchKernelGGL((scan_rerank_kernel<m.value, true>), dim3((unsigned)Q, (unsigned)(kp / KPRIME)), dim3(KPRIME), 0, s, X, xnorm, ld, Qp, qnorm, best, thr,
                           xnorm_max_bits, qres, overflow, k, row_base, perm, out_dist, out_rows, flags, kp, ekeys);
        hipLaunchKernelGGL(scan_finalize_kernel<m.value>, dim3((unsigned)Q), dim3(256), 0, s, ekeys, kp, qnorm, thr, xnorm_max_bits, qres, overflow, ld, k, row_base,
                           out_dist, out_rows, flags);
    });
}
// exact keys of cand [Q][kp] (the first ncand[q] slots of query q) -> ekeys [Q][kp]; nothing else (no sort, no certificate)
void sc_launch_scan_rerank_keys(int metric, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, const uint64_t* cand, const int* ncand, int kp,
                                const uint32_t* perm, uint64_t* ekeys, int Q, hipStream_t s) {
    sc_dispatch_metric(metric, [&](auto m) {
        hipLaunchKernelGGL((scan_rerank_kernel<m.value, true>), dim3((unsigned)Q, (unsigned)(kp / KPRIME)), dim3(KPRIME), 0, s, X, xnorm, ld, Qp, qnorm, cand,
                           (const float*)nullptr, (const unsigned*)nullptr, (const float*)nullptr, (const int*)nullptr, 0, (int64_t)0, perm, (float*)nullptr,
                           (int64_t*)nullptr, (int*)nullptr, kp, ekeys, ncand);
    });
}
void sc_launch_scan_collect_bound(int metric, const float* prev_dist, int k, const float* qnorm, const float* qres, const unsigned* bits, int ld, float* thr,
                                  float* thr_fast, int* flags, int Q, hipStream_t s) {
    const dim3 grid((unsigned)((Q + 255) / 256)), block(256);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_collect_bound_kernel<m.value>, grid, block, 0, s, prev_dist, k, qnorm, qres, bits, ld, thr, thr_fast, flags, Q); });
}
void sc_launch_scan_tighten(int metric, const uint64_t* ekeys, int kp, int k, const float* qnorm, const float* qres, const unsigned* bits, int ld, float* thr,
                            float* thr_fast, float* thr_cut, int Q, hipStream_t s) {
    const dim3 grid((unsigned)Q), block(128);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_tighten_kernel<m.value>, grid, block, 0, s, ekeys, kp, k, qnorm, qres, bits, ld, thr, thr_fast, thr_cut); });
}
void sc_launch_scan_wide_certify(int metric, const float* out_dist, int k, const float* qnorm, const float* qres, const unsigned* bits, int ld, const float* thr,
                                 const int* overflow, int* flags, int Q, hipStream_t s) {
    const dim3 grid((unsigned)((Q + 255) / 256)), block(256);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_wide_certify_kernel<m.value>, grid, block, 0, s, out_dist, k, qnorm, qres, bits, ld, thr, overflow, flags, Q); });
}
