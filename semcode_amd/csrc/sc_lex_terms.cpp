// sc_lex_terms.cpp -- sc_lex_terms (include/semcode_hip.h): chunk text -> the term rows of the lexical search.  Plain C++, no
// runtime, no device: the translation unit links on its own (scripts/lex_terms_check.cpp).
//
// A term run is a maximal run of bytes in [A-Za-z0-9_] or >= 0x80.  A run has a split point at every '_' (which belongs to no part)
// and between two bytes where a lower-case ASCII letter is followed by an upper-case one or a letter by a digit or a digit by a
// letter (bytes >= 0x80 count as letters without case).  The run emits itself and then, if it has a split point, every part between
// split points, in text order.  Emitted tokens have their ASCII letters lower-cased, are cut to their first 64 bytes, and are
// dropped when shorter than 2 bytes.  A token is hashed by 32-bit FNV-1a over its bytes, folded to (h ^ (h >> 16)) & 0xFFFF, with
// 0xFFFF mapped to 0xFFFE.  The first T tokens of a text are kept, sorted ascending (repeats stay), and padded with 0xFFFF.
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/semcode_hip.h"
#include "lex_rule.h"

// (the error text goes through the library's sc_fail when this file is part of it)
sc_status sc_fail(sc_status code, const char* fmt, ...) __attribute__((weak));

static inline bool is_upper(unsigned char c) { return c >= 'A' && c <= 'Z'; }
static inline bool is_lower(unsigned char c) { return c >= 'a' && c <= 'z'; }
static inline bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
static inline bool is_letter(unsigned char c) { return is_upper(c) || is_lower(c) || c >= 0x80; }
static inline bool is_term_byte(unsigned char c) { return is_letter(c) || is_digit(c) || c == '_'; }

static const size_t MAX_TOKEN = 64;

static inline uint16_t hash_token(const unsigned char* p, size_t len) {
    if (len > MAX_TOKEN) len = MAX_TOKEN;
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < len; ++i) {
        const unsigned char c = is_upper(p[i]) ? (unsigned char)(p[i] + 32) : p[i];
        h = (h ^ c) * 16777619u;
    }
    const uint32_t f = (h ^ (h >> 16)) & 0xFFFFu;
    return (uint16_t)(f == LEX_PAD ? 0xFFFEu : f);
}

// tokens of text [p, p + len) into out[0 .. T): returns how many (<= T)
static int extract(const unsigned char* p, size_t len, int T, uint16_t* out) {
    int cnt = 0;
    size_t i = 0;
    while (i < len && cnt < T) {
        if (!is_term_byte(p[i])) {
            ++i;
            continue;
        }
        size_t e = i;
        while (e < len && is_term_byte(p[e])) ++e;
        // the run [i, e)
        if (e - i >= 2) out[cnt++] = hash_token(p + i, e - i);
        bool split = false;
        for (size_t j = i; j < e && !split; ++j)
            split = p[j] == '_' || (j + 1 < e && p[j + 1] != '_' &&
                                    ((is_lower(p[j]) && is_upper(p[j + 1])) || (is_letter(p[j]) && is_digit(p[j + 1])) || (is_digit(p[j]) && is_letter(p[j + 1]))));
        if (split) {
            size_t s = i;  // start of the current part
            for (size_t j = i; j < e && cnt < T; ++j) {
                bool end_here;  // the part ends with byte j (or before it, when j is '_')
                if (p[j] == '_') {
                    if (j - s >= 2) out[cnt++] = hash_token(p + s, j - s);
                    s = j + 1;
                    continue;
                }
                if (j + 1 == e || p[j + 1] == '_') end_here = true;
                else end_here = (is_lower(p[j]) && is_upper(p[j + 1])) || (is_letter(p[j]) && is_digit(p[j + 1])) || (is_digit(p[j]) && is_letter(p[j + 1]));
                if (end_here) {
                    if (j + 1 - s >= 2) out[cnt++] = hash_token(p + s, j + 1 - s);
                    s = j + 1;
                }
            }
        }
        i = e;
    }
    return cnt;
}

extern "C" sc_status sc_lex_terms(const uint8_t* bytes, const int64_t* offsets, int64_t n, int32_t T, uint16_t* out_terms, int32_t* out_counts) {
    const char* bad = nullptr;
    if (n < 0 || !lex_valid_T(T)) bad = "sc_lex_terms: need n >= 0 and T one of 32, 64, 128, 256";
    else if (n > 0 && (!offsets || !out_terms)) bad = "sc_lex_terms: NULL argument";
    for (int64_t r = 0; !bad && r < n; ++r)
        if (offsets[r] < 0 || offsets[r + 1] < offsets[r] || (offsets[r + 1] > offsets[r] && !bytes)) bad = "sc_lex_terms: offsets must be ascending and >= 0";
    if (bad) return sc_fail ? sc_fail(SC_ERR_INVALID, "%s", bad) : SC_ERR_INVALID;
    for (int64_t r = 0; r < n; ++r) {
        uint16_t* row = out_terms + (size_t)r * T;
        const size_t len = (size_t)(offsets[r + 1] - offsets[r]);
        const int cnt = len ? extract(bytes + offsets[r], len, T, row) : 0;
        std::sort(row, row + cnt);
        for (int i = cnt; i < T; ++i) row[i] = (uint16_t)LEX_PAD;
        if (out_counts) out_counts[r] = cnt;
    }
    return SC_OK;
}
