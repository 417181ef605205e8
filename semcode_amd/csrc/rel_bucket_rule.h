// rel_bucket_rule.h -- the bucket rule of T5's relative position bias (cfg.pos_type 3), host arithmetic only: what builds the device table of
// the bias attention (sc_encoder_model.cpp), what sc_diag_rel_buckets returns, and what a stand-alone program can include without a runtime.
//
// transformers' T5Attention._relative_position_bucket, bidirectional: with nb = buckets / 2, me = nb / 2 and n = |rel|, rel = key - query,
//   b = rel > 0 ? nb : 0;   b += n                                                         if n < me
//                           b += min(nb - 1, me + trunc(log(n / me) / log(max_distance / me) * (nb - me)))   otherwise
// transformers evaluates the logarithmic arm on float32 tensors: n / me and its log in float32, the division by the DOUBLE log(max_distance /
// me) rounded to float32 first (a tensor divided by a Python number), the product with nb - me in float32, then truncation.  The same
// steps in the same precision here, so the integers agree bin edge by bin edge (tests/golden/t5_golden.npz holds transformers' own).
// What this rests on: the host libm's float32 log rounds as torch's float32 log does at the arguments n / me that land on a bin edge (the
// quotient of two such logs then truncates to the same integer).  The fixture pins it where the tests run; a libm that rounds one of those
// logs the other way would move single distances by one bucket, and tests/test_t5.py would name them.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

static inline int sc_rel_bucket(int rel, int buckets, int max_distance) {
    const int nb = buckets / 2, me = nb / 2;
    const int n = rel < 0 ? -rel : rel;
    int b = rel > 0 ? nb : 0;
    if (n < me) return b + n;
    const float ratio = std::log((float)n / (float)me) / (float)std::log((double)max_distance / (double)me);
    int large = me + (int)(ratio * (float)(nb - me));
    if (large > nb - 1) large = nb - 1;
    return b + large;
}
// the rule's own conditions: an even number of buckets with me >= 1, max_distance beyond me (the logarithm's denominator is positive)
static inline bool sc_rel_buckets_valid(int buckets, int max_distance) {
    return buckets >= 4 && buckets <= 256 && (buckets % 2) == 0 && max_distance > buckets / 4 && max_distance <= (1 << 20);
}
// out[d + span - 1] = bucket(d) for d = key - query in -(span - 1) .. span - 1
static inline void sc_rel_buckets(int buckets, int max_distance, int span, int32_t* out) {
    for (int d = -(span - 1); d <= span - 1; ++d) out[d + span - 1] = sc_rel_bucket(d, buckets, max_distance);
}
// The distance table of the bias attention kernels: rel_bias [buckets][heads] (transformers' layout of relative_attention_bias.weight)
// -> [heads][2 span - 1] f32, the values as they are (the kernels start their score accumulators from them).
static inline std::vector<float> sc_rel_bias_table(const float* rel_bias, int buckets, int heads, int max_distance, int span) {
    const int n = 2 * span - 1;
    std::vector<int32_t> bk((size_t)n);
    sc_rel_buckets(buckets, max_distance, span, bk.data());
    std::vector<float> tbl((size_t)heads * n);
    for (int h = 0; h < heads; ++h)
        for (int j = 0; j < n; ++j) tbl[(size_t)h * n + j] = rel_bias[(size_t)bk[j] * heads + h];
    return tbl;
}
