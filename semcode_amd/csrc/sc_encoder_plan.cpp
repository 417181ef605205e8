// sc_encoder_plan.cpp -- the rules and the filler of a packed call's plan (sc_encoder_plan.h): host arithmetic only.
#include "sc_encoder_plan.h"

#include <cstring>

void sc_packed_items(const int32_t* starts, const int32_t* lens, int64_t B, int32_t* items, int nitems[3]) {
    int32_t* w = items;
    for (int cls = 0; cls < 3; ++cls) {
        const int32_t* w0 = w;
        for (int64_t i = 0; i < B; ++i) {
            if (sc_packed_attention_class(lens[i]) != cls) continue;
            const int nqb = (int)(ceil32(lens[i]) / 32);
            for (int qb = 0; qb < (cls == 0 ? nqb : 1); qb += 8, w += 4) { w[0] = starts[i]; w[1] = lens[i]; w[2] = qb; w[3] = 0; }
        }
        nitems[cls] = (int)((w - w0) / 4);
    }
}

sc_status sc_plan_check_offsets(const int64_t* offsets, int32_t B, const PlanBounds& mb, const char* who, int64_t* rows) {
    if (!offsets) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (B < 1 || B > 65536) return sc_fail(SC_ERR_INVALID, "%s: batch %d out of range", who, B);
    if (offsets[0] != 0) return sc_fail(SC_ERR_INVALID, "%s: offsets[0] must be 0 (got %lld)", who, (long long)offsets[0]);
    const int64_t max_len = mb.pos_type != 1 && mb.max_pos < 2048 ? mb.max_pos : 2048;
    int64_t used = 0;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 1) return sc_fail(SC_ERR_INVALID, "%s: text %d has length %lld (every text needs at least one token)", who, i, (long long)len);
        if (len > max_len)
            return sc_fail(SC_ERR_INVALID, "%s: text %d has %lld tokens, more than %lld (the smaller of 2048 and the model's max_pos)", who, i, (long long)len, (long long)max_len);
        used += ceil32(len);
    }
    if (ceil256(used) > SC_ENCODER_PACKED_MAX_ROWS)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: %lld token rows, more than SC_ENCODER_PACKED_MAX_ROWS = %d (split the batch)", who, (long long)used, SC_ENCODER_PACKED_MAX_ROWS);
    *rows = used;
    return SC_OK;
}

sc_status sc_plan_check_pairs(const int64_t* offsets, const int32_t* first_lens, int32_t B, const PlanBounds& mb, const char* who) {
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 2) return sc_fail(SC_ERR_INVALID, "%s: pair %d has %lld token(s) (a pair needs at least 2)", who, i, (long long)len);
        if (first_lens[i] < 1 || first_lens[i] > len)
            return sc_fail(SC_ERR_INVALID, "%s: first_lens[%d] = %d outside 1 .. %lld (the pair's length)", who, i, first_lens[i], (long long)len);
        if (first_lens[i] < len && mb.type_vocab < 2)
            return sc_fail(SC_ERR_INVALID, "%s: pair %d has a second segment, the model's type_vocab is %d (needs 2)", who, i, mb.type_vocab);
    }
    return SC_OK;
}

sc_status sc_plan_check_tokens(const int64_t* offsets, int32_t B, int32_t expand_id, bool query, const PlanBounds& mb, const char* who, int64_t* used,
                               int64_t* nrows) {
    sc_status st = sc_plan_check_offsets(offsets, B, mb, who, used);
    if (st) return st;
    if (expand_id >= mb.vocab) return sc_fail(SC_ERR_INVALID, "%s: expand_id %d outside the vocabulary (%d tokens)", who, expand_id, mb.vocab);
    *nrows = expand_id >= 0 ? *used : offsets[B];
    if (!query) return SC_OK;
    const bool local_layers = mb.arch == 1 && mb.global_every > 1;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len > mb.max_query) return sc_fail(SC_ERR_INVALID, "%s: query %d has %lld tokens, more than %d", who, i, (long long)len, mb.max_query);
        // an expansion row attends the real keys only: in a local layer its last one must still reach the text's last token
        if (expand_id >= 0 && local_layers && ceil32(len) - len > mb.local_window / 2)
            return sc_fail(SC_ERR_INVALID, "%s: query %d has %lld tokens: its last expansion row would see no key within local_window %d", who, i, (long long)len,
                           mb.local_window);
    }
    return SC_OK;
}

int64_t sc_plan_kept_counts(const int64_t* offsets, int32_t B, const uint8_t* keep, int32_t* counts) {
    int64_t total = 0;
    for (int32_t i = 0; i < B; ++i) {
        int32_t n = 0;
        if (!keep) n = (int32_t)(offsets[i + 1] - offsets[i]);
        else
            for (int64_t j = offsets[i]; j < offsets[i + 1]; ++j) n += keep[j] != 0;
        counts[i] = n;
        total += n;
    }
    return total;
}

int64_t sc_plan_fill(const int32_t* ids, const int64_t* offsets, int32_t B, const PackedCall& call, const PlanOffsets& po, int64_t M, char* buf, int nitems[3]) {
    int32_t* h_ids = (int32_t*)(buf + po.ids);
    int32_t* h_pos = (int32_t*)(buf + po.pos);
    int32_t* h_starts = (int32_t*)(buf + po.starts);
    int32_t* h_lens = (int32_t*)(buf + po.lens);
    memset(h_ids, 0, (size_t)M * 4);  // alignment rows and the tail take token 0 ...
    memset(h_pos, 0, (size_t)M * 4);  // ... the tail position 0
    int64_t row = 0;
    for (int32_t i = 0; i < B; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i], span = ceil32(len);
        h_starts[i] = (int32_t)row;
        h_lens[i] = (int32_t)len;
        memcpy(h_ids + row, ids + offsets[i], (size_t)len * 4);
        for (int64_t j = 0; j < span; ++j) h_pos[row + j] = (int32_t)j;  // (the kernels clamp an alignment row's position into the table)
        row += span;
    }
    if (call.kind == PackedCall::PAIRS) {
        int32_t* h_types = (int32_t*)(buf + po.types);
        int32_t* h_ones = (int32_t*)(buf + po.ones);
        memset(h_types, 0, (size_t)M * 4);  // alignment rows and the tail take type 0
        for (int32_t i = 0; i < B; ++i) {
            for (int32_t j = call.first_lens[i]; j < h_lens[i]; ++j) h_types[h_starts[i] + j] = 1;
            h_ones[i] = 1;
        }
    }
    if (call.kind == PackedCall::TOKENS) {
        int32_t* h_dst = (int32_t*)(buf + po.dst);
        memset(h_dst, 0xFF, (size_t)M * 4);  // -1: alignment rows of documents and the tail are not asked for
        int32_t at = 0;
        for (int32_t i = 0; i < B; ++i) {
            const int32_t n = call.expand_id >= 0 ? (int32_t)ceil32(h_lens[i]) : h_lens[i];
            for (int32_t j = h_lens[i]; j < n; ++j) h_ids[h_starts[i] + j] = call.expand_id;
            const uint8_t* kp = call.expand_id < 0 && call.keep ? call.keep + offsets[i] : nullptr;  // (flags belong to documents)
            for (int32_t j = 0; j < n; ++j)
                if (!kp || kp[j]) h_dst[h_starts[i] + j] = at++;
        }
    }
    sc_packed_items(h_starts, h_lens, B, (int32_t*)(buf + po.items), nitems);
    return row;
}
