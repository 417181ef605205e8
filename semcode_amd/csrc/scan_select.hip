// scan_select.hip -- between the phases of the batched scan (scan_batched.h): keep the best coarse keys of every query, publish
// its new threshold; the wide candidate set; the small kernels that set up and close a batch (gfx950).
//
// Roofline: LDS (one workgroup per query, a few thousand keys each).
#include "scan_batched.h"

// ------------------------------------------------------------------ per-phase selection: keep the kp (KPRIME or KPRIME8) best coarse keys
// best [Q][kp] keys in no particular order (SC_KEY_MAX padded).  One workgroup per query.
//
// The kp-th smallest of the n <= cap + kp keys (survivors of this phase + the previous best) is found by a radix select over
// the 64-bit keys, 12 bits per pass from the top (4096-bin histogram in LDS, atomics; after the first pass only the keys of one
// bin are still in play), then every key <= that pivot is kept -- exactly kp of them, keys being unique (row id in the low
// word).  The rank sort this replaces was quadratic in n: 0.31 ms per step at kp = 128 and 2.6 ms at kp = 512
// (measurement pass r2c, int8 scan; log not kept); the re-rank never needed the list sorted.
template <int METRIC>
__global__ __launch_bounds__(SEL_THREADS) void scan_select_kernel(uint64_t* __restrict__ surv, unsigned* __restrict__ count, int cap,
                                                                   uint64_t* __restrict__ best, const float* __restrict__ qnorm,
                                                                   float* __restrict__ thr, float* __restrict__ thr_fast,
                                                                   int* __restrict__ overflow, int kp) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sel_lds[];  // [cap + kp] candidates | hist[SEL_BINS] | scan[SEL_THREADS] | misc
    uint64_t* cand = sel_lds;
    unsigned* hist = reinterpret_cast<unsigned*>(sel_lds + cap + kp);
    unsigned* part = hist + SEL_BINS;          // per-thread partial sums of the bin scan
    unsigned* misc = part + SEL_THREADS;       // [0] n, [1] chosen bin, [2] rank inside it, [3] output cursor
    const int q = blockIdx.x, tid = threadIdx.x;
    unsigned c = count[q];
    if (c > (unsigned)cap) {
        if (tid == 0) overflow[q] = 1;
        c = cap;
    }
    if (tid == 0) { misc[0] = 0; misc[3] = 0; }
    __syncthreads();
    // gather the real keys (the previous best is padded with SC_KEY_MAX)
    for (int i = tid; i < (int)c + kp; i += SEL_THREADS) {
        const uint64_t key = i < (int)c ? surv[(size_t)q * cap + i] : best[(size_t)q * kp + (i - (int)c)];
        if (key != SC_KEY_MAX) cand[atomicAdd(&misc[0], 1u)] = key;
    }
    __syncthreads();
    const int n = (int)misc[0];
    uint64_t pivot = SC_KEY_MAX;  // keep every key <= pivot
    bool have_kth = false;
    if (n > kp) {
        pivot = radix_select_pivot(cand, n, (unsigned)(kp - 1), hist, part, misc);  // rank kp - 1 (0-based)
        have_kth = true;
    } else if (n == kp) {
        // exactly kp keys: all stay, the threshold is their maximum
        uint64_t m = 0;
        for (int i = tid; i < n; i += SEL_THREADS) m = cand[i] > m ? cand[i] : m;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint64_t o = ((uint64_t)__shfl_xor((unsigned)(m >> 32), off, 64) << 32) | (uint64_t)__shfl_xor((unsigned)m, off, 64);
            m = o > m ? o : m;
        }
        uint64_t* wmax = reinterpret_cast<uint64_t*>(hist);
        if ((tid & 63) == 0) wmax[tid >> 6] = m;
        __syncthreads();
        pivot = wmax[0];
        for (int w = 1; w < SEL_THREADS / 64; ++w) pivot = wmax[w] > pivot ? wmax[w] : pivot;
        have_kth = true;
        __syncthreads();
    }
    for (int i = tid; i < n; i += SEL_THREADS) {
        const uint64_t key = cand[i];
        if (key <= pivot) best[(size_t)q * kp + atomicAdd(&misc[3], 1u)] = key;
    }
    __syncthreads();
    const int kept = (int)misc[3];  // == min(n, kp)
    for (int i = kept + tid; i < kp; i += SEL_THREADS) best[(size_t)q * kp + i] = SC_KEY_MAX;
    if (tid == 0) {
        count[q] = 0;
        float t = __builtin_inff(), tf = __builtin_inff();
        if (have_kth) {
            const float sc = sc_key_score(METRIC, pivot);
            t = (METRIC == SC_METRIC_L2) ? sc : -sc;
            tf = fast_threshold<METRIC>(t, qnorm[q]);
        }
        thr[q] = t;
        thr_fast[q] = tf;
    }
}

// ---- the wide candidate set (corpora whose certificate fails at kp candidates: clusters) ----------------------------------------------
// With thresholds from exact scores the selection between phases need not truncate at kp: it keeps EVERY key within the cut (up to
// kcap = 4 096) and at least the kp best.  Nothing within the coarse error of the k-th exact score is ever dropped then, so the
// certificate holds by construction and the batch is answered in this one pass -- where the kp-candidate form sent a clustered
// batch through a second pass (the collect pass) or to the bf16 stage.  best [Q][kcap] holds nbest[q] keys (no padding).
template <int METRIC>
__global__ __launch_bounds__(SEL_THREADS) void scan_select_wide_kernel(const uint64_t* __restrict__ surv, unsigned* __restrict__ count, int cap,
                                                                        uint64_t* __restrict__ best, unsigned* __restrict__ nbest, int kcap, int kp,
                                                                        const float* __restrict__ qnorm, float* __restrict__ thr, float* __restrict__ thr_fast,
                                                                        const float* __restrict__ thr_cut, int* __restrict__ overflow) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sel_lds[];  // [cap + kcap] candidates | hist[SEL_BINS] | scan[SEL_THREADS] | misc
    uint64_t* cand = sel_lds;
    unsigned* hist = reinterpret_cast<unsigned*>(sel_lds + cap + kcap);
    unsigned* part = hist + SEL_BINS;
    unsigned* misc = part + SEL_THREADS;  // [0] n, [1] chosen bin, [2] rank inside it, [3] output cursor, [4] keys within the cut
    const int q = blockIdx.x, tid = threadIdx.x;
    unsigned c = count[q];
    if (c > (unsigned)cap) {
        if (tid == 0) overflow[q] = 1;
        c = cap;
    }
    const unsigned nb = nbest[q];
    const float cutv = thr_cut[q];
    const bool have_cut = cutv < __builtin_inff();
    if (tid == 0) { misc[0] = 0; misc[3] = 0; misc[4] = 0; }
    __syncthreads();
    for (unsigned i = tid; i < c + nb; i += SEL_THREADS) {
        const uint64_t key = i < c ? surv[(size_t)q * cap + i] : best[(size_t)q * kcap + (i - c)];
        if (key == SC_KEY_MAX) continue;
        cand[atomicAdd(&misc[0], 1u)] = key;
        if (have_cut) {
            const float sc = sc_key_score(METRIC, key);
            if (((METRIC == SC_METRIC_L2) ? sc : -sc) <= cutv) atomicAdd(&misc[4], 1u);
        }
    }
    __syncthreads();
    const int n = (int)misc[0];
    const int cle = (int)misc[4];
    if (cle > kcap && tid == 0) overflow[q] = 1;  // more keys within the cut than the set holds: the query goes on to the next stage
    const int keep = (n < kp ? n : kp) > (cle < kcap ? cle : kcap) ? (n < kp ? n : kp) : (cle < kcap ? cle : kcap);
    uint64_t pivot = SC_KEY_MAX;  // keep every key <= pivot
    if (n > keep) {
        pivot = radix_select_pivot(cand, n, (unsigned)(keep - 1), hist, part, misc);
    }
    for (int i = tid; i < n; i += SEL_THREADS) {
        const uint64_t key = cand[i];
        if (key <= pivot) best[(size_t)q * kcap + atomicAdd(&misc[3], 1u)] = key;
    }
    __syncthreads();
    if (tid == 0) {
        nbest[q] = misc[3];  // == keep
        count[q] = 0;
        // what the rows dropped here (and by the phase's own test) exceed: the cut when every key within it was kept, else the kp-th key
        float t = __builtin_inff();
        if (have_cut && cle >= kp && cle <= kcap) t = cutv;
        else if (n > keep && keep >= kp) {
            const float sc = sc_key_score(METRIC, pivot);
            t = (METRIC == SC_METRIC_L2) ? sc : -sc;
        } else if (n == keep && keep >= kp && n == kp) {  // exactly kp keys: all stay, the threshold is their maximum (as scan_select_kernel has it)
            uint64_t m = 0;
            for (int i = 0; i < n; ++i) m = cand[i] > m ? cand[i] : m;
            const float sc = sc_key_score(METRIC, m);
            t = (METRIC == SC_METRIC_L2) ? sc : -sc;
        }
        float tf = __builtin_inff();
        if (t < __builtin_inff()) tf = fast_threshold<METRIC>(t, qnorm[q]);
        thr[q] = t;
        thr_fast[q] = tf;
    }
}
// the keys of best within the final threshold, compacted: what the exact re-score has to look at
template <int METRIC>
__global__ __launch_bounds__(256) void scan_wide_compact_kernel(const uint64_t* __restrict__ best, const unsigned* __restrict__ nbest, int kcap,
                                                                 const float* __restrict__ thr, uint64_t* __restrict__ cand, int* __restrict__ ncand) {
    __shared__ unsigned s_n;
    const int q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const unsigned nb = nbest[q];
    const float tau = thr[q];
    for (unsigned i = tid; i < nb; i += 256) {
        const uint64_t key = best[(size_t)q * kcap + i];
        if (key == SC_KEY_MAX) continue;  // (the plain form pads its kp slots)
        const float sc = sc_key_score(METRIC, key);
        if (((METRIC == SC_METRIC_L2) ? sc : -sc) <= tau) cand[(size_t)q * kcap + atomicAdd(&s_n, 1u)] = key;
    }
    __syncthreads();
    if (tid == 0) ncand[q] = (int)s_n;
}

// thr[q] = min(thr[q], thr_cut[q]) before the certificate (the last selection may have left +inf: fewer than kp keys)
__global__ __launch_bounds__(256) void scan_thr_min_kernel(float* __restrict__ thr, const float* __restrict__ thr_cut, int Q) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < Q) thr[q] = fminf(thr[q], thr_cut[q]);
}
__global__ __launch_bounds__(256) void scan_fill_u32_kernel(unsigned* __restrict__ p, unsigned v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(256) void scan_collect_counts_kernel(const unsigned* __restrict__ count, int cap, int* __restrict__ ncand, int* __restrict__ flags, int Q) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const unsigned c = count[q];
    const bool fits = c <= (unsigned)cap && !flags[q];
    ncand[q] = fits ? (int)c : 0;
    if (!fits) flags[q] = 1;
}

__global__ __launch_bounds__(256) void scan_batched_init_kernel(float* thr, float* thr_fast, int qpad, uint64_t* best, unsigned* count,
                                                                 int* overflow, int Q, int kp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < qpad) { thr[i] = __builtin_inff(); thr_fast[i] = __builtin_inff(); }
    if (i < Q) { count[i] = 0u; overflow[i] = 0; }
    if (i < Q * kp) best[i] = SC_KEY_MAX;
}

// ------------------------------------------------------------------ launchers
void sc_launch_scan_batched_init(float* thr, float* thr_fast, int qpad, uint64_t* best, unsigned* count, int* overflow, int Q, int kp, hipStream_t s) {
    const int n = Q * kp > qpad ? Q * kp : qpad;
    hipLaunchKernelGGL(scan_batched_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, thr, thr_fast, qpad, best, count, overflow, Q, kp);
}
void sc_launch_scan_select(int metric, uint64_t* surv, unsigned* count, int cap, uint64_t* best, const float* qnorm, float* thr,
                           float* thr_fast, int* overflow, int Q, int kp, hipStream_t s) {
    const size_t lds = (size_t)(cap + kp) * 8 + (SEL_BINS + SEL_THREADS + 8) * 4;
    static ScDeviceOnce once_sel;
    sc_device_once(once_sel, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_select_kernel<SC_METRIC_IP>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_select_kernel<SC_METRIC_L2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_select_kernel<SC_METRIC_COSINE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    dim3 grid((unsigned)Q), block(SEL_THREADS);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_select_kernel<m.value>, grid, block, lds, s, surv, count, cap, best, qnorm, thr, thr_fast, overflow, kp); });
}
void sc_launch_scan_select_wide(int metric, const uint64_t* surv, unsigned* count, int cap, uint64_t* best, unsigned* nbest, int kcap, int kp, const float* qnorm,
                                float* thr, float* thr_fast, const float* thr_cut, int* overflow, int Q, hipStream_t s) {
    const size_t lds = (size_t)(cap + kcap) * 8 + (SEL_BINS + SEL_THREADS + 8) * 4;
    static ScDeviceOnce once;
    sc_device_once(once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_select_wide_kernel<SC_METRIC_IP>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_select_wide_kernel<SC_METRIC_L2>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_select_wide_kernel<SC_METRIC_COSINE>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    const dim3 grid((unsigned)Q), block(SEL_THREADS);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_select_wide_kernel<m.value>, grid, block, lds, s, surv, count, cap, best, nbest, kcap, kp, qnorm, thr, thr_fast, thr_cut, overflow); });
}
void sc_launch_scan_wide_compact(int metric, const uint64_t* best, const unsigned* nbest, int kcap, const float* thr, uint64_t* cand, int* ncand, int Q, hipStream_t s) {
    const dim3 grid((unsigned)Q), block(256);
    sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(scan_wide_compact_kernel<m.value>, grid, block, 0, s, best, nbest, kcap, thr, cand, ncand); });
}
void sc_launch_scan_thr_min(float* thr, const float* thr_cut, int Q, hipStream_t s) {
    hipLaunchKernelGGL(scan_thr_min_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, thr, thr_cut, Q);
}
void sc_launch_fill_u32(unsigned* p, unsigned v, int n, hipStream_t s) {
    hipLaunchKernelGGL(scan_fill_u32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, v, n);
}
void sc_launch_scan_collect_counts(const unsigned* count, int cap, int* ncand, int* flags, int Q, hipStream_t s) {
    hipLaunchKernelGGL(scan_collect_counts_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, count, cap, ncand, flags, Q);
}
