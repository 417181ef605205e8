// mmr_rule.h -- the selection rule of the MMR search (sc_index_search_mmr*, include/semcode_hip.h), one copy for the device
// (scan_mmr.hip mmr_select_kernel) and the host (sc_diag_mmr_select_host, sc_mmr.cpp): mu, the value of a candidate, the comparison
// with its tie rule, and the greedy loop over them in its plain sequential form.
//
// Everything is f32, one correctly rounded operation at a time: v = fsub(fmul(lambda, rel), fmul(mu, m)) with mu = fsub(1, lambda),
// never a fused multiply-add, whatever -ffp-contract says -- the device uses the _rn intrinsics, the host rounds both products into
// volatile floats.  m is an f32 max and so exact.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MMR_HD __host__ __device__
#else
#define MMR_HD
#endif

MMR_HD static inline float mmr_mu(float lambda) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(1.0f, lambda);
#else
    return 1.0f - lambda;
#endif
}

// v_i of a candidate with relevance rel (the oriented score against the query) and m = its largest oriented score against a pick
MMR_HD static inline float mmr_value(float lambda, float mu, float rel, float m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(__fmul_rn(lambda, rel), __fmul_rn(mu, m));
#else
    volatile float a = lambda * rel;
    volatile float b = mu * m;
    return a - b;
#endif
}

MMR_HD static inline float mmr_max(float a, float b) { return fmaxf(a, b); }

// Does candidate (v, i) replace the best so far (bv, bi)?  i, bi < 0: none.  Larger v wins, equal v goes to the smaller index; the
// relation is a total order on distinct indices, so a reduction tree and a sequential walk agree.
MMR_HD static inline bool mmr_takes(float v, int i, float bv, int bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    return v > bv || (v == bv && i < bi);
}

// The whole selection of one query, sequentially: rel [C], G [C rows of ldg] (G[i * ldg + j] = red_ij), picked [min(k, C)] receives
// candidate indices in selection order.  m is caller scratch of C floats.  Returns the number of picks.
MMR_HD static inline int mmr_select_seq(const float* rel, const float* G, int C, int ldg, int k, float lambda, float* m, unsigned char* taken, int32_t* picked) {
    const int steps = k < C ? k : C;
    if (steps < 1) return 0;
    const float mu = mmr_mu(lambda);
    for (int i = 0; i < C; ++i) {
        m[i] = -INFINITY;
        taken[i] = 0;
    }
    int last = 0;
    picked[0] = 0;
    taken[0] = 1;
    for (int t = 1; t < steps; ++t) {
        float bv = 0.0f;
        int bi = -1;
        for (int i = 0; i < C; ++i) {
            if (taken[i]) continue;
            m[i] = mmr_max(m[i], G[(size_t)i * ldg + last]);
            const float v = mmr_value(lambda, mu, rel[i], m[i]);
            if (mmr_takes(v, i, bv, bi)) {
                bv = v;
                bi = i;
            }
        }
        last = bi;
        picked[t] = bi;
        taken[bi] = 1;
    }
    return steps;
}
