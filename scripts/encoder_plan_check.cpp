// encoder_plan_check.cpp -- stand-alone run of semcode_amd/csrc/sc_encoder_plan.cpp (the plan of a packed encoder call) on the CPU, meant to be
// built with the sanitizers; the file includes no HIP header, so a plain compiler takes it:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Isemcode_amd/csrc
//       scripts/encoder_plan_check.cpp semcode_amd/csrc/sc_encoder_plan.cpp -o encoder_plan_check
// It calls the checks and the filler on the cases of tests/test_encoder_plan_host.py the way embed_packed_locked does -- ids of exactly
// offsets[B] entries and a heap buffer of exactly PlanOffsets::total bytes, so that an index one past either end is an error -- and looks at
// the few facts a wrong index would break.  The two functions the library takes from elsewhere are given here.  Exit status 0 and "ok".
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

// one accepted call: checks by kind, then the filler into a buffer of exactly the plan's size
static void run(const std::vector<int64_t>& lens, PackedCall call, bool query = false, PlanBounds mb = BERT) {
    const int32_t B = (int32_t)lens.size();
    std::vector<int64_t> off(1, 0);
    for (int64_t n : lens) off.push_back(off.back() + n);
    std::vector<int32_t> ids((size_t)off.back(), 7);
    int64_t used = 0, nrows = 0;
    sc_status st = call.kind == PackedCall::TOKENS ? sc_plan_check_tokens(off.data(), B, call.expand_id, query, mb, "check", &used, &nrows)
                                                   : sc_plan_check_offsets(off.data(), B, mb, "check", &used);
    if (!st && call.kind == PackedCall::PAIRS) st = sc_plan_check_pairs(off.data(), call.first_lens, B, mb, "check");
    expect(st == SC_OK, "an accepted case was refused");
    if (st) return;
    const int64_t M = ceil256(used);
    const PlanOffsets po((size_t)M, (size_t)B, call.kind);
    std::vector<char> buf(po.total);
    int nitems[3];
    const int64_t rows = sc_plan_fill(ids.data(), off.data(), B, call, po, M, buf.data(), nitems);
    expect(rows == used, "row count");
    expect(nitems[0] + nitems[1] + nitems[2] <= sc_packed_items_cap(M, B), "items within their capacity");
    const int32_t* h_starts = (const int32_t*)(buf.data() + po.starts);
    expect(h_starts[B - 1] + ceil32(lens.back()) == rows, "last start");
    if (call.kind == PackedCall::TOKENS) {
        const int32_t* dst = (const int32_t*)(buf.data() + po.dst);
        expect(rows == 0 || dst[rows - 1] == (int32_t)nrows - 1 || call.expand_id < 0, "last output row of a query call");
    }
}

static void refuse(const std::vector<int64_t>& off, PackedCall call, bool query, PlanBounds mb, const char* part, const int32_t* first_lens = nullptr) {
    const int32_t B = (int32_t)off.size() - 1;
    int64_t used = 0, nrows = 0;
    last_error[0] = 0;
    sc_status st = call.kind == PackedCall::TOKENS ? sc_plan_check_tokens(off.data(), B, call.expand_id, query, mb, "check", &used, &nrows)
                                                   : sc_plan_check_offsets(off.data(), B, mb, "check", &used);
    if (!st && first_lens) st = sc_plan_check_pairs(off.data(), first_lens, B, mb, "check");
    expect(st != SC_OK && std::strstr(last_error, part), part);
}

int main() {
    run({1, 31, 32, 33, 128, 129, 256, 257, 2048}, PackedCall{});
    run({1}, PackedCall{});
    run(std::vector<int64_t>(256, 2048), PackedCall{});  // the largest plan: SC_ENCODER_PACKED_MAX_ROWS rows
    const std::vector<int32_t> first{1, 33, 10, 128, 1};
    run({2, 33, 64, 129, 300}, PackedCall::pairs(first.data()));
    run({1, 31, 32, 33, 100, 128}, PackedCall::tokens(-1, nullptr));
    run({1, 31, 32, 33, 100, 128}, PackedCall::tokens(103, nullptr), true);
    run({61}, PackedCall::tokens(103, nullptr), true, PlanBounds{8192, 2, 50368, 1, 1, 3, 6, 128});

    PlanBounds small = BERT, alibi = BERT, one_type = BERT;
    small.max_pos = alibi.max_pos = 512;
    alibi.pos_type = 1;
    one_type.type_vocab = 1;
    refuse({3, 8}, PackedCall{}, false, BERT, "offsets[0] must be 0");
    refuse({0, 4, 4, 9}, PackedCall{}, false, BERT, "has length 0");
    refuse({0, 513}, PackedCall{}, false, small, "more than 512");
    refuse({0, 2049}, PackedCall{}, false, alibi, "more than 2048");
    std::vector<int64_t> big;
    for (int64_t i = 0; i <= 257; ++i) big.push_back(i * 2048);
    refuse(big, PackedCall{}, false, BERT, "SC_ENCODER_PACKED_MAX_ROWS");
    refuse({0}, PackedCall{}, false, BERT, "batch 0 out of range");
    refuse(std::vector<int64_t>(65538, 0), PackedCall{}, false, BERT, "batch 65537 out of range");
    const int32_t fl_short[2] = {2, 1}, fl_zero[1] = {0}, fl_over[2] = {5, 7}, fl_seg[1] = {3};
    refuse({0, 5, 6}, PackedCall{}, false, BERT, "a pair needs at least 2", fl_short);
    refuse({0, 5}, PackedCall{}, false, BERT, "outside 1 .. 5", fl_zero);
    refuse({0, 5, 11}, PackedCall{}, false, BERT, "outside 1 .. 6", fl_over);
    refuse({0, 5}, PackedCall{}, false, one_type, "type_vocab is 1", fl_seg);
    refuse({0, 4, 133}, PackedCall::tokens(103, nullptr), true, BERT, "more than 128");
    refuse({0, 4, 133}, PackedCall::tokens(-1, nullptr), true, BERT, "more than 128");
    refuse({0, 4}, PackedCall::tokens(30522, nullptr), true, BERT, "outside the vocabulary");
    refuse({0, 33}, PackedCall::tokens(103, nullptr), true, PlanBounds{8192, 2, 50368, 1, 1, 3, 6, 128}, "within local_window 6");
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
