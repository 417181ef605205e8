// late_ingest_plan_check.cpp -- stand-alone run of the keep-flag rule of a packed token call (semcode_amd/csrc/sc_encoder_plan.cpp:
// sc_plan_kept_counts and the TOKENS branch of sc_plan_fill, what sc_encoder_embed_tokens_into plans) on the CPU, meant to be built with
// the sanitizers; no HIP header is involved, so a plain compiler takes it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Isemcode_amd/csrc
//       scripts/late_ingest_plan_check.cpp semcode_amd/csrc/sc_encoder_plan.cpp -o late_ingest_plan_check
// Every array has exactly the size the entry point is promised -- ids and keep of offsets[B] entries, counts of B, a heap buffer of
// PlanOffsets::total bytes -- so that an index one past any of them is an error, and the plan is compared with a restatement: -1 exactly on
// dropped, alignment and tail rows, the kept rows numbered compactly text after text, counts as reported.  Exit status 0 and "ok".
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sc_encoder_plan.h"

static char last_error[512];
sc_status sc_fail(sc_status code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof last_error, fmt, ap);
    va_end(ap);
    return code;
}
int sc_packed_attention_class(int len) { return len > 256 ? 0 : (len > 128 ? 1 : 2); }  // (encoder_packed.hip)

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (ok) return;
    ++failures;
    std::printf("FAIL %s\n", what);
}

static const PlanBounds BERT{2048, 0, 30522, 2, 0, 0, 0, 128};

enum Pattern { NONE_GIVEN, ONES, NOTHING, FIRST, LAST, ALTERNATING, RANDOM70 };

static void run(const std::vector<int64_t>& lens, Pattern pat) {
    const int32_t B = (int32_t)lens.size();
    std::vector<int64_t> off(1, 0);
    for (int64_t n : lens) off.push_back(off.back() + n);
    const size_t total = (size_t)off.back();
    std::vector<int32_t> ids(total, 7);
    std::vector<uint8_t> keep(total, pat == ONES ? 1 : 0);
    uint32_t lcg = 12345u + (uint32_t)pat;
    for (int32_t i = 0; i < B; ++i)
        for (int64_t j = off[i]; j < off[i + 1]; ++j) {
            if (pat == FIRST) keep[(size_t)j] = j == off[i];
            if (pat == LAST) keep[(size_t)j] = j == off[i + 1] - 1 ? 200 : 0;
            if (pat == ALTERNATING) keep[(size_t)j] = (uint8_t)(j & 1);
            if (pat == RANDOM70) keep[(size_t)j] = (lcg = lcg * 1664525u + 1013904223u) >> 8 < (uint32_t)(0.7 * (1u << 24));
        }
    const uint8_t* kp = pat == NONE_GIVEN ? nullptr : keep.data();
    int64_t used = 0, nrows = 0;
    const sc_status st = sc_plan_check_tokens(off.data(), B, -1, false, BERT, "check", &used, &nrows);
    expect(st == SC_OK && nrows == (int64_t)total, "an accepted case was refused");
    if (st) return;
    std::vector<int32_t> counts((size_t)B, -7);
    const int64_t kept = sc_plan_kept_counts(off.data(), B, kp, counts.data());
    const PackedCall call = PackedCall::kept_tokens(kp, nullptr, 1);
    const int64_t M = ceil256(used);
    const PlanOffsets po((size_t)M, (size_t)B, call.kind);
    std::vector<char> buf(po.total);
    int nitems[3];
    const int64_t rows = sc_plan_fill(ids.data(), off.data(), B, call, po, M, buf.data(), nitems);
    expect(rows == used, "row count");
    const int32_t* dst = (const int32_t*)(buf.data() + po.dst);
    int64_t row = 0, at = 0, sum = 0;
    for (int32_t i = 0; i < B; ++i) {
        int32_t n = 0;
        for (int64_t j = 0; j < ceil32(lens[(size_t)i]); ++j, ++row) {
            const bool real = j < lens[(size_t)i], k = real && (!kp || kp[(size_t)(off[i] + j)]);
            expect(dst[row] == (k ? (int32_t)at : -1), "dst of a text's row");
            at += k;
            n += k;
        }
        expect(counts[(size_t)i] == n, "kept count of a text");
        sum += n;
    }
    for (; row < M; ++row) expect(dst[row] == -1, "dst of a tail row");
    expect(kept == sum && kept == at, "kept total");
}

int main() {
    const std::vector<int64_t> lens{1, 2, 15, 16, 17, 31, 32, 33, 180, 1100}, rev(lens.rbegin(), lens.rend());
    for (int p = NONE_GIVEN; p <= RANDOM70; ++p) {
        run(lens, (Pattern)p);
        run(rev, (Pattern)p);
        run({1}, (Pattern)p);
        run({2048}, (Pattern)p);
        run(std::vector<int64_t>(256, 2048), (Pattern)p);  // the largest plan: SC_ENCODER_PACKED_MAX_ROWS rows
    }
    // a query call never reads flags, even where a caller left some in the call
    {
        const std::vector<int64_t> off{0, 5};
        const std::vector<int32_t> ids(5, 7);
        const std::vector<uint8_t> keep(5, 0);
        PackedCall call = PackedCall::tokens(103, nullptr);
        call.keep = keep.data();
        const PlanOffsets po(256, 1, call.kind);
        std::vector<char> buf(po.total);
        int nitems[3];
        sc_plan_fill(ids.data(), off.data(), 1, call, po, 256, buf.data(), nitems);
        const int32_t* dst = (const int32_t*)(buf.data() + po.dst);
        expect(dst[0] == 0 && dst[31] == 31 && dst[32] == -1, "a query's rows are all asked for");
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
