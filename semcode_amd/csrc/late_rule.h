// late_rule.h -- what the token store of an index (sc_tokens.cpp, scan_late.hip) adds to maxsim_rule.h, one copy for the device and the
// host (sc_diag_late_search_host, sc_diag_round_bf16): the table entry of a row, the bf16 storage rule and the order of hits.
//
//   storage    fmt 0: the caller's f32 bits.  fmt 1: every float rounded to nearest-even on its upper 16 bits ONCE, at install
//              (late_round_bf16), and widened back exactly when read (late_widen_bf16): the stored value is one f32 bit pattern, every
//              score is the rule of maxsim_rule.h on those values, and no bf16 arithmetic happens anywhere.
//   hits       larger score first under the total order of maxsim_key (-0 < +0), ties to the lower row: ascending late_hit_key.  The
//              upper word is the order-preserving map of -score -- the map sc_make_key uses, without its +0.0f, which folds the two
//              zeros --, so sc_topk_merge decodes it under SC_METRIC_IP to the score's own bits.
#pragma once
#include "maxsim_rule.h"

#define LATE_MAX_TOKENS 2048  // tokens of one row
#define LATE_MAX_K 128        // widest top-k of the search
#define LATE_MAX_C 1024       // candidates per question of the rerank

// one row of the table: its tokens are pool[start, start + len) (token vectors of W elements); len 0: the row has none
struct sc_tok_entry {
    int64_t start;
    int32_t len;
    int32_t pad;
};

MAXSIM_HD static inline uint16_t late_round_bf16(float v) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(v);
#else
    memcpy(&u, &v, 4);
#endif
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
MAXSIM_HD static inline float late_widen_bf16(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float v;
#if defined(__HIP_DEVICE_COMPILE__)
    v = __uint_as_float(u);
#else
    memcpy(&v, &u, 4);
#endif
    return v;
}

// 64-bit total order of hits, smaller = better
MAXSIM_HD static inline uint64_t late_hit_key(float score, uint32_t row) { return ((uint64_t)maxsim_key(-score) << 32) | row; }
