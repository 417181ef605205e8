// maxsim_rule.h -- the late-interaction (ColBERT) score of one (query, document) pair, one copy for the device (encoder_tokens.hip
// maxsim_kernel) and the host (sc_diag_maxsim_host, sc_encoder_diag.cpp; scripts/maxsim_rule_check.cpp): the dot product of two token
// vectors, the order under which a query token's maximum is taken, and the whole pair in its plain sequential form.
//
// Everything is f32.  Token vectors have W floats, W % 16 == 0, 16 <= W <= 128.
//   dot(q, d)  one fmaf chain from +0 in the k order in which v_mfma_f32_16x16x4_f32 consumes four 16-byte fragments: inside each block
//              of 16, k = 16 t + 4 g + c with c outer and g inner -- the order of oracle/sc_oracle.c sc_oracle_dot.
//   m_t        the maximum of dot(Q_t, D_j) over the kept j < nd, under the total order of the order-preserving score key
//              (maxsim_key: -0 < +0, no two finite floats equal), so the result is one bit pattern whatever the order of visiting.
//              No kept token: m_t = -inf (the key the maximum starts from); the encoder entry points refuse such a document.
//   score      acc = +0; for t ascending: acc = fadd(acc, m_t) -- one correctly rounded addition at a time, never fused with anything:
//              the device uses __fadd_rn, the host rounds through a volatile float.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MAXSIM_HD __host__ __device__
#else
#define MAXSIM_HD
#endif

#define MAXSIM_MAX_W 128
#define MAXSIM_MAX_NQ 128

MAXSIM_HD static inline bool maxsim_width_ok(int W) { return W >= 16 && W <= MAXSIM_MAX_W && (W % 16) == 0; }

MAXSIM_HD static inline float maxsim_dot(const float* q, const float* d, int W) {
    float acc = 0.0f;
    for (int t = 0; t < W; t += 16)
        for (int c = 0; c < 4; ++c)
            for (int g = 0; g < 4; ++g) {
                const int k = t + 4 * g + c;
                acc = fmaf(d[k], q[k], acc);
            }
    return acc;
}

// order-preserving map of a float onto unsigned integers: a < b as floats (and -0 < +0) iff key(a) < key(b)
MAXSIM_HD static inline uint32_t maxsim_key(float v) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(v);
#else
    memcpy(&u, &v, 4);
#endif
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MAXSIM_HD static inline float maxsim_unkey(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __uint_as_float(u);
#else
    memcpy(&v, &u, 4);
#endif
    return v;
}
#define MAXSIM_KEY_NONE 0x007FFFFFu  // maxsim_key(-inf): what a maximum starts from
MAXSIM_HD static inline uint32_t maxsim_key_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

MAXSIM_HD static inline float maxsim_add(float acc, float m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(acc, m);
#else
    volatile float r = acc + m;
    return r;
#endif
}

// One pair, sequentially: Q [nq][W], D [nd][W], keep [nd] (NULL: every token is kept).
MAXSIM_HD static inline float maxsim_score_seq(const float* Q, int nq, const float* D, int nd, const unsigned char* keep, int W) {
    float acc = 0.0f;
    for (int t = 0; t < nq; ++t) {
        uint32_t best = MAXSIM_KEY_NONE;
        for (int j = 0; j < nd; ++j) {
            if (keep && !keep[j]) continue;
            best = maxsim_key_max(best, maxsim_key(maxsim_dot(Q + (size_t)t * W, D + (size_t)j * W, W)));
        }
        acc = maxsim_add(acc, maxsim_unkey(best));
    }
    return acc;
}
