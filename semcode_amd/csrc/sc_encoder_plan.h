// sc_encoder_plan.h -- the plan of one packed encoder call as a function of plain values: the rules its offsets must meet, the layout
// of its buffers and the bytes in them.  No HIP header and no sc_encoder here, so the CPU suite reaches all of it through
// sc_diag_encoder_plan (tests/test_encoder_plan_host.py).  embed_packed_locked (sc_encoder_embed.cpp) uploads exactly these bytes.
//
// Sequence i of a packed batch owns the token rows [starts[i], starts[i] + ceil32(len_i)), one sequence after another; the GEMMs run on
// the total rounded up to 256 rows (ceil256).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/semcode_hip.h"

sc_status sc_fail(sc_status code, const char* fmt, ...);  // sc_api.cpp (as sc_internal.h declares it)
int sc_packed_attention_class(int len);                   // encoder_packed.hip: 0 longer than 256 tokens, 1 up to 256, 2 up to 128

static inline int64_t ceil32(int64_t v) { return (v + 31) & ~(int64_t)31; }
static inline int64_t ceil256(int64_t v) { return (v + 255) & ~(int64_t)255; }  // GEMM tiles are 256 rows; buffers are 256-byte aligned

// What the batch of a packed call is.  At most one payload is read, the one of the kind.
struct PackedCall {
    enum Kind {
        TEXTS,   // texts to embed: one pooled row per text
        PAIRS,   // pairs of a cross-encoder (sc_encoder_score_pairs): the first first_lens[i] rows of pair i take segment id 0, the rest of the
                 // pair 1; the lens the forward gets are ones (pooling then returns the [CLS] row whatever the encoder's mode; attention reads
                 // the real lengths from its items); never L2-normalised
        SCORED,  // sequences of sc_encoder_score_seqs: pooled as the installed score head reads them (head_pool: 0 mean, 1 first row, 2 last
                 // token) instead of the encoder's mode; never L2-normalised
        TOKENS   // a token call (sc_encoder_embed_tokens, sc_encoder_score_late): nothing is pooled, the last layer is never pruned; the token
                 // head writes tok_out [.., W] f32 (device) compactly and in text order.  expand_id >= 0: queries -- every row of a text's
                 // 32-row span is asked for and its alignment rows carry that token instead of token 0; < 0: documents -- the len_i real rows,
                 // or (keep given) those of them whose keep flag is not 0: a dropped token's row is attended like any other and its
                 // vector never stored.  tok_fmt 1: tok_out takes the vectors rounded to bf16 (late_rule.h), 2 W bytes each
    } kind = TEXTS;
    const int32_t* first_lens = nullptr;  // PAIRS: host [B], validated
    int head_pool = -1;                   // SCORED
    int32_t expand_id = -1;               // TOKENS
    void* tok_out = nullptr;              // TOKENS
    int tok_fmt = 0;                      // TOKENS
    const uint8_t* keep = nullptr;        // TOKENS, documents: host [offsets[B]] in ids order, validated; NULL = every token is asked for
    static PackedCall pairs(const int32_t* first_lens) { PackedCall c; c.kind = PAIRS; c.first_lens = first_lens; return c; }
    static PackedCall scored(int head_pool) { PackedCall c; c.kind = SCORED; c.head_pool = head_pool; return c; }
    static PackedCall tokens(int32_t expand_id, void* out) { PackedCall c; c.kind = TOKENS; c.expand_id = expand_id; c.tok_out = out; return c; }
    // the documents of sc_encoder_embed_tokens_into: the kept tokens' vectors, numbered compactly text after text, at `out` in format `fmt`
    static PackedCall kept_tokens(const uint8_t* keep, void* out, int fmt) { PackedCall c = tokens(-1, out); c.keep = keep; c.tok_fmt = fmt; return c; }
};

// The attention work items of packed sequences: per sequence one item for every 8 query blocks of 32 rows (class 0) or one item
// (classes 1, 2), written as {start, len, first query block, 0} in class order.  items must hold sc_packed_items_cap(rows, B) items.
inline int64_t sc_packed_items_cap(int64_t rows, int64_t B) { return B + rows / 256; }
void sc_packed_items(const int32_t* starts, const int32_t* lens, int64_t B, int32_t* items, int nitems[3]);

// The plan of one packed call, laid out alike in pinned host staging and in the workspace (M token rows, B sequences): monotone in both, so
// a call's plan fits the buffer of any larger workspace.  A pair call's segment id per row (types) and its length of one per pair (ones)
// come behind the rest, so that a plan without them lies as before; a token call's output row per row (dst) takes no more than those two.
struct PlanOffsets {
    size_t ids, pos, starts, lens, items, types = 0, ones = 0, dst = 0, total;
    PlanOffsets(size_t M, size_t B, PackedCall::Kind kind = PackedCall::TEXTS) {
        size_t u = 0;
        auto take = [&](size_t bytes) { const size_t at = u; u += (size_t)ceil256((int64_t)bytes); return at; };
        ids = take(M * 4);
        pos = take(M * 4);
        starts = take(B * 4);
        lens = take(B * 4);
        items = take((size_t)sc_packed_items_cap((int64_t)M, (int64_t)B) * 16);
        if (kind == PackedCall::PAIRS) {
            types = take(M * 4);
            ones = take(B * 4);
        }
        if (kind == PackedCall::TOKENS) dst = take(M * 4);
        total = u;
    }
};

// What the rules read of the model, as plain values (sc_encoder_cfg's fields of the same names)
struct PlanBounds {
    int max_pos, pos_type, vocab, type_vocab, arch, global_every, local_window;
    int max_query;  // MAXSIM_MAX_NQ (maxsim_rule.h): the tokens of a late-interaction query
};

// The rules, each with sc_fail's message under `who`.
// offsets [B + 1] of any packed call: every rule of the header; *rows = the token rows in use (the sum of ceil32(len_i))
sc_status sc_plan_check_offsets(const int64_t* offsets, int32_t B, const PlanBounds& mb, const char* who, int64_t* rows);
// ... of a pair call, behind those: a pair has two tokens, first_lens[i] lies in 1 .. len_i, a second segment needs a type_vocab of 2
sc_status sc_plan_check_pairs(const int64_t* offsets, const int32_t* first_lens, int32_t B, const PlanBounds& mb, const char* who);
// ... of a token call: the packed rules and expand_id inside the vocabulary.  query: the texts are MaxSim's query side -- at most
// mb.max_query tokens each, with or without expansion, and with it the last expansion row must reach a key in the local layers.
// *used = packed rows, *nrows = token vectors asked for
sc_status sc_plan_check_tokens(const int64_t* offsets, int32_t B, int32_t expand_id, bool query, const PlanBounds& mb, const char* who, int64_t* used,
                               int64_t* nrows);

// The token vectors a document-side token call under keep flags stores for each text: counts[i] = the tokens of text i whose flag is not 0
// (keep NULL: len_i); returns their sum.  sc_plan_fill numbers exactly these rows.
int64_t sc_plan_kept_counts(const int64_t* offsets, int32_t B, const uint8_t* keep, int32_t* counts);

// Fills `buf`, laid out by po = PlanOffsets(M, B, call.kind) with M = ceil256(rows), from host ids / validated offsets: ids (0 on alignment
// rows and the tail, or expand_id on a query's alignment rows), pos (0 .. span - 1 per text, 0 on the tail), starts, lens, items and, by kind,
// types / ones or dst (-1 for a row that is not asked for: alignment rows, the tail, a document token whose keep flag is 0; the others count up
// from 0, text after text).  Returns the token rows in use.
int64_t sc_plan_fill(const int32_t* ids, const int64_t* offsets, int32_t B, const PackedCall& call, const PlanOffsets& po, int64_t M, char* buf, int nitems[3]);
