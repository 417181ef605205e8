// lex_rule.h -- the rules of the lexical and the hybrid search (sc_index_search_lexical*, sc_index_search_hybrid*,
// include/semcode_hip.h), one copy for the device (scan_lexical.hip) and the host (sc_diag_lex_score_host, sc_diag_rrf_host in
// sc_lexical.cpp): the BM25 score of a term row, the comparison of two hits, and the weighted reciprocal-rank fusion.
//
// Term row: T uint16 slots (T = 32, 64, 128 or 256), sorted ascending, repeats kept (tf = the length of a run), padded with
// LEX_PAD; dl = the number of slots that are not LEX_PAD.  Neither dl nor tf depends on the order of the slots as computed here.
//
// Everything is f32, one correctly rounded operation at a time, never a fused multiply-add whatever -ffp-contract says: the device
// uses the _rn intrinsics (__fdiv_rn is the IEEE division), the host rounds every intermediate into a volatile float.
//   K     = k1 * ((1 - b) + (b * (float)dl) / avgdl)
//   c_j   = (w_j * ((float)tf_j * (k1 + 1))) / ((float)tf_j + K)
//   score = ((0 + c_j0) + c_j1) + ...      over the query terms j with tf_j > 0, j ascending
//   f     = wd / (float)(c + rank_dense) + wl / (float)(c + rank_lex)      a missing rank gives 0 for its term; dense first
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEX_HD __host__ __device__
#else
#define LEX_HD
#endif

#define LEX_PAD 0xFFFFu        // the padding slot; never a term
#define LEX_MAX_QTERMS 32      // terms of one query
#define LEX_DF_SIZE 65536      // entries of the df table

LEX_HD static inline bool lex_valid_T(int T) { return T == 32 || T == 64 || T == 128 || T == 256; }

LEX_HD static inline float lex_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    volatile float r = a * b;
    return r;
#endif
}
LEX_HD static inline float lex_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    volatile float r = a + b;
    return r;
#endif
}
LEX_HD static inline float lex_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    volatile float r = a - b;
    return r;
#endif
}
LEX_HD static inline float lex_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    volatile float r = a / b;
    return r;
#endif
}

// the length normalisation of a row of dl terms
LEX_HD static inline float lex_K(float k1, float b, float avgdl, int dl) {
    return lex_mul(k1, lex_add(lex_sub(1.0f, b), lex_div(lex_mul(b, (float)dl), avgdl)));
}
// c_j of a query term of weight w that the row holds tf > 0 times; k1p = lex_add(k1, 1)
LEX_HD static inline float lex_term(float w, int tf, float k1p, float K) {
    return lex_div(lex_mul(w, lex_mul((float)tf, k1p)), lex_add((float)tf, K));
}
// a weight the search accepts: finite and > 0
LEX_HD static inline bool lex_valid_weight(float w) { return w > 0.0f && w < INFINITY; }

// The score of one row for one query, sequentially.  row [T]; qterms [m] strictly ascending, none LEX_PAD; qweights [m].
// Returns false (and *score = 0) when the row holds none of the terms: such a row is never a hit.
LEX_HD static inline bool lex_score_row(const uint16_t* row, int T, const uint16_t* qterms, const float* qweights, int m, float k1, float b, float avgdl,
                                        float* score) {
    int dl = 0;
    for (int i = 0; i < T; ++i) dl += row[i] != LEX_PAD ? 1 : 0;
    const float K = lex_K(k1, b, avgdl, dl), k1p = lex_add(k1, 1.0f);
    float s = 0.0f;
    bool hit = false;
    for (int j = 0; j < m; ++j) {
        int tf = 0;
        for (int i = 0; i < T; ++i) tf += row[i] == qterms[j] ? 1 : 0;
        if (tf > 0) {
            s = lex_add(s, lex_term(qweights[j], tf, k1p, K));
            hit = true;
        }
    }
    *score = s;
    return hit;
}

// The fused score of a row at rank rd of the dense list and rank rl of the lexical list (ranks from 0; < 0: not in that list).
LEX_HD static inline float lex_rrf(float wd, float wl, int32_t c, int rd, int rl) {
    const float fd = rd >= 0 ? lex_div(wd, (float)(c + rd)) : 0.0f;
    const float fl = rl >= 0 ? lex_div(wl, (float)(c + rl)) : 0.0f;
    return lex_add(fd, fl);
}
// Does hit (score a, row ra) come before hit (score b, row rb)?  Larger score first, equal scores by the lower row: a total order
// on distinct rows, for the lexical hits and the fused ones alike.
LEX_HD static inline bool lex_before(float a, int64_t ra, float b, int64_t rb) { return a > b || (a == b && ra < rb); }
