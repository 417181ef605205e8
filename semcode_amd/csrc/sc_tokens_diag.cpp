// sc_tokens_diag.cpp -- the rules of the token store on the CPU, from the headers the kernels compile (tests on a machine without a
// GPU): sc_diag_late_search_host is sc_index_search_late, sc_diag_round_bf16 the install-time rounding of fmt 1.
#include <algorithm>
#include <cmath>
#include <vector>

#include "sc_internal.h"  // (first: the HIP runtime header, whose bit casts maxsim_rule.h uses in a device pass)
#include "late_rule.h"

extern "C" sc_status sc_diag_round_bf16(const float* in, int64_t n, float* out) {
    if (n < 0 || (n > 0 && (!in || !out))) return sc_fail(SC_ERR_INVALID, "sc_diag_round_bf16: bad argument");
    for (int64_t i = 0; i < n; ++i) out[i] = late_widen_bf16(late_round_bf16(in[i]));
    return SC_OK;
}

extern "C" sc_status sc_diag_late_search_host(const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int64_t* d_off, int64_t n, int32_t W, int32_t k,
                                              const uint32_t* allow, int64_t allow_words, float* out_score, int64_t* out_rows) {
    const char* who = "sc_diag_late_search_host";
    if (!Q || !q_off || !d_off || !out_score || !out_rows) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (!maxsim_width_ok(W)) return sc_fail(SC_ERR_INVALID, "%s: W = %d must be a multiple of 16 within 16 .. %d", who, W, MAXSIM_MAX_W);
    if (Bq < 1 || Bq > 65536 || n < 0 || n > (int64_t)0xFFFFFFFFll) return sc_fail(SC_ERR_INVALID, "%s: Bq=%d or n=%lld out of range", who, Bq, (long long)n);
    if (k < 1 || k > LATE_MAX_K) return sc_fail(SC_ERR_INVALID, "%s: top_k must be 1..%d (got %d)", who, LATE_MAX_K, k);
    if (q_off[0] != 0 || d_off[0] != 0) return sc_fail(SC_ERR_INVALID, "%s: offsets must start at 0", who);
    for (int32_t q = 0; q < Bq; ++q) {
        const int64_t nq = (int64_t)q_off[q + 1] - q_off[q];
        if (nq < 1 || nq > MAXSIM_MAX_NQ) return sc_fail(SC_ERR_INVALID, "%s: question %d has %lld token vectors (1 .. %d)", who, q, (long long)nq, MAXSIM_MAX_NQ);
    }
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = d_off[r + 1] - d_off[r];
        if (len < 0 || len > LATE_MAX_TOKENS) return sc_fail(SC_ERR_INVALID, "%s: row %lld has %lld tokens (0 .. %d)", who, (long long)r, (long long)len, LATE_MAX_TOKENS);
    }
    if (d_off[n] > 0 && !D) return sc_fail(SC_ERR_INVALID, "%s: D is NULL", who);
    if ((!allow && allow_words != 0) || (allow && allow_words < (n + 31) / 32))
        return sc_fail(SC_ERR_INVALID, "%s: allow_words=%lld, %lld rows need %lld", who, (long long)allow_words, (long long)n, (long long)((n + 31) / 32));
    std::vector<uint64_t> keys;
    for (int32_t q = 0; q < Bq; ++q) {
        const float* Qq = Q + (size_t)q_off[q] * W;
        const int nq = q_off[q + 1] - q_off[q];
        keys.clear();
        for (int64_t r = 0; r < n; ++r) {
            const int len = (int)(d_off[r + 1] - d_off[r]);
            if (len == 0 || (allow && !((allow[r >> 5] >> (r & 31)) & 1u))) continue;
            keys.push_back(late_hit_key(maxsim_score_seq(Qq, nq, D + (size_t)d_off[r] * W, len, nullptr, W), (uint32_t)r));
        }
        std::sort(keys.begin(), keys.end());
        for (int i = 0; i < k; ++i) {
            const bool have = i < (int)keys.size();
            out_score[(size_t)q * k + i] = have ? -maxsim_unkey((uint32_t)(keys[(size_t)i] >> 32)) : -INFINITY;
            out_rows[(size_t)q * k + i] = have ? (int64_t)(uint32_t)keys[(size_t)i] : -1;
        }
    }
    return SC_OK;
}
