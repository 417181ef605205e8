// lex_terms_check.cpp -- stand-alone check of sc_lex_terms (semcode_amd/csrc/sc_lex_terms.cpp, the term extractor of the hybrid
// search) on the CPU, meant to be built with the sanitizers; it links that one translation unit and nothing else:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Isemcode_amd/csrc \
//       scripts/lex_terms_check.cpp semcode_amd/csrc/sc_lex_terms.cpp -o lex_terms_check
// Every text sits in a heap buffer of exactly its length and every output row in one of exactly T slots, so that a read or a write
// one past either end is an error.  It runs the fixed list of tests/test_lexical_host.py (with the hashes that test expects for four
// of them) and random bytes through all four T.  Exit status 0 and "ok" when every row is sorted, padded and within its count.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "semcode_hip.h"

static int failures = 0;

static std::vector<uint16_t> row_of(const std::string& text, int T, int32_t* count) {
    std::vector<uint8_t> bytes(text.begin(), text.end());  // exactly text.size() bytes (none when empty)
    const int64_t offsets[2] = {0, (int64_t)bytes.size()};
    std::vector<uint16_t> row((size_t)T, 0x1234);
    const sc_status st = sc_lex_terms(bytes.empty() ? nullptr : bytes.data(), offsets, 1, T, row.data(), count);
    if (st != SC_OK) {
        std::printf("FAIL: status %d\n", (int)st);
        std::exit(1);
    }
    return row;
}

static void check_row(const std::vector<uint16_t>& row, int32_t cnt, int T, const char* what) {
    bool fine = cnt >= 0 && cnt <= T;
    for (int i = 0; fine && i < T; ++i) fine = i < cnt ? (row[(size_t)i] != 0xFFFF && (i == 0 || row[(size_t)i - 1] <= row[(size_t)i])) : row[(size_t)i] == 0xFFFF;
    if (!fine) {
        std::printf("FAIL: %s, T=%d: row not sorted / padded (count %d)\n", what, T, (int)cnt);
        ++failures;
    }
}

static void expect(const std::string& text, std::vector<uint16_t> want) {
    int32_t cnt = -1;
    const std::vector<uint16_t> row = row_of(text, 32, &cnt);
    std::sort(want.begin(), want.end());
    if (cnt != (int32_t)want.size() || !std::equal(want.begin(), want.end(), row.begin())) {
        std::printf("FAIL: '%s' gives %d terms, not the expected ones\n", text.c_str(), (int)cnt);
        ++failures;
    }
}

int main() {
    expect("camelCase", {38225, 29287, 41876});
    expect("HTTPServer2", {32188, 56753});
    expect("snake_case_name", {21038, 19886, 41876, 12511});
    expect("__init__", {52560, 50626});
    std::string many;
    for (int i = 0; i < 90; ++i) many += "tok" + std::to_string(i) + "Word_" + std::to_string(i) + " ";
    const std::vector<std::string> fixed = {
        "camelCase", "HTTPServer2", "snake_case_name", "__init__", "def parse_frobnicate_v2(self, x2y): return SC_ERR_NOMEM  # ivf_listmajor_plan",
        "gr\xc3\xb6\xc3\x9f" "e = na\xc3\xafve\xc3\x9c" "ber_stra\xc3\x9f" "e + \xe6\x95\xb0\xe6\x8d\xae\xe5\xba\x93Name2 \xce\xbbx", std::string(200, 'a'),
        std::string(200, 'Z') + "_" + std::string(140, '9'), "", "a b c _ 1 __ _x_ y_", std::string("\x00\x01 tab\there\nnew.line", 20), many, "_", "__", "a_", "_a", "aB", "a1", "1a",
        std::string(64, 'q'), std::string(65, 'q'), std::string(63, 'q') + "\xc3"};
    for (const int T : {32, 64, 128, 256})
        for (const std::string& t : fixed) {
            int32_t cnt = -1;
            const std::vector<uint16_t> row = row_of(t, T, &cnt);
            check_row(row, cnt, T, "fixed list");
        }
    // random bytes: every byte value, runs of term bytes and separators, lengths 0 .. 600
    uint64_t z = 0x9E3779B97F4A7C15ull;
    auto next = [&z]() {
        z ^= z << 13;
        z ^= z >> 7;
        z ^= z << 17;
        return z;
    };
    for (int it = 0; it < 4000; ++it) {
        const size_t len = (size_t)(next() % 601);
        std::string t(len, '\0');
        const int mode = (int)(next() % 3);
        for (size_t i = 0; i < len; ++i) {
            const uint64_t r = next();
            t[i] = mode == 0 ? (char)(r & 0xFF) : mode == 1 ? "abXY09__ \n\xc3\xa9"[r % 12] : (char)('A' + r % 58);
        }
        const int T = 32 << (int)(next() % 4);
        int32_t cnt = -1;
        const std::vector<uint16_t> row = row_of(t, T, &cnt);
        check_row(row, cnt, T, "random bytes");
    }
    // a batch: several texts behind one another, one of them empty, counts optional
    {
        const std::string a = "alphaBeta", b = "", c = "gamma_delta9";
        std::vector<uint8_t> bytes;
        bytes.insert(bytes.end(), a.begin(), a.end());
        bytes.insert(bytes.end(), c.begin(), c.end());
        const int64_t offsets[4] = {0, (int64_t)a.size(), (int64_t)a.size(), (int64_t)(a.size() + c.size())};
        std::vector<uint16_t> rows(3 * 64);
        if (sc_lex_terms(bytes.data(), offsets, 3, 64, rows.data(), nullptr) != SC_OK) ++failures;
        if (rows[64] != 0xFFFF || rows[0] == 0xFFFF || rows[128] == 0xFFFF) ++failures;
        if (sc_lex_terms(bytes.data(), offsets, 3, 48, rows.data(), nullptr) != SC_ERR_INVALID) ++failures;  // (no library around it: the bare status)
    }
    if (failures) {
        std::printf("FAIL: %d\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
