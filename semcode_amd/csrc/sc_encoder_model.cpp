// sc_encoder_model.cpp -- an encoder handle from its configuration and weight blob: the rules of a configuration (check_cfg), the blob's
// size and order, the rotary and ALiBi tables, the parameter arena with its LayerNorm-folded copies, create / destroy / info, and the
// workspace every forward runs in (layout_ws / ensure_ws).
//
// Mirrors (reference): the object EmbeddingProviderFactory.create() returns (src/semcode/embeddings/providers.py:34-104; third-party
// forward in llama.cpp).  Tokenisation stays on the host side of the boundary (semcode_amd/embeddings/tokenizer.py).
#include <cmath>
#include <new>

#include "rel_bucket_rule.h"
#include "sc_encoder_state.h"

// number of f32 values in the weight blob, in blob order (see include/semcode_hip.h)
static int64_t blob_floats(const sc_encoder_cfg& c) {
    const int64_t H = c.hidden, F = c.ffn, F1 = ffn_gated(c) ? 2 * F : F;
    const int64_t KV = kv_width(c), AW = attn_width(c);
    int64_t n = (int64_t)c.vocab * H + (c.pos_type != 0 ? 0 : (int64_t)c.max_pos * H) + (c.arch != 0 ? 0 : (int64_t)c.type_vocab * H) + (c.arch >= 2 ? 0 : 2 * H);
    if (c.pos_type == 3) n += (int64_t)c.rel_buckets * c.heads;  // rel_bias [rel_buckets, heads] behind word_emb
    n += (int64_t)c.layers * ((AW * H + AW) + (H * AW + H) + 2 * (KV * H + KV) + 2 * H + (F1 * H + F1) + (H * F + H) + 2 * H);
    if (c.arch == 2 && c.qk_norm) n += (int64_t)c.layers * 2 * head_width(c);  // q_norm, k_norm gammas behind each layer's ln2_beta
    if (c.arch != 0) n += 2 * H;  // final_norm
    return n;
}
extern "C" sc_status sc_encoder_blob_bytes(const sc_encoder_cfg* cfg, int64_t* out) {
    if (!cfg || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_blob_bytes: NULL argument");
    *out = blob_floats(*cfg) * 4;
    return SC_OK;
}

static sc_status check_cfg(const sc_encoder_cfg& c) {
    if (c.vocab < 1 || c.hidden < 1 || c.layers < 1 || c.heads < 1 || c.ffn < 1 || c.max_pos < 1 || c.type_vocab < 1)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: non-positive model dimension");
    const bool wide = c.arch == 2 && c.head_dim == 128;  // heads of 128 are stated, never derived: hidden need not be heads * 128
    if (!wide && !t5_stated_heads(c) && c.hidden != c.heads * 64 && c.hidden != c.heads * 32)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head dimension must be 64 or 32 (hidden=%d heads=%d)", c.hidden, c.heads);
    if (c.hidden % 128 || c.ffn % 128 || c.hidden > 2048)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: hidden (<=2048) and ffn must be multiples of 128 (got %d, %d)", c.hidden, c.ffn);
    if (!(c.ln_eps > 0.f)) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: ln_eps must be > 0");
    if (c.pos_type < 0 || c.pos_type > 3 || c.ffn_type < 0 || c.ffn_type > 4) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: unknown pos_type / ffn_type");
    if (c.hidden == c.heads * 32 && c.pos_type != 0)  // the rotary kernels pair columns (j, j + 32) of a 64-wide head; no 32-wide ALiBi kernel
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head dimension 32 runs with learned positions only (pos_type 0), not pos_type %d (%s)", c.pos_type,
                       c.pos_type == 1 ? "ALiBi" : "rotary");
    if (c.pos_type == 2 && !(c.rope_theta >= 0.f)) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: rope_theta must be >= 0 (0 = 10000)");
    if (c.arch < 0 || c.arch > 3)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: unknown arch %d (0 = post-LN BERT family, 1 = pre-LN ModernBERT, 2 = causal Qwen2 decoder, 3 = T5 encoder)", c.arch);
    if (c.arch == 3 && !sc_rel_buckets_valid(c.rel_buckets, c.rel_max_distance))  // (first: an arch 3 configuration without its table is no model at all)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: arch 3 needs rel_buckets even, 4 .. 256, and rel_max_distance beyond rel_buckets / 4, got %d / %d",
                       c.rel_buckets, c.rel_max_distance);
    if (c.arch != 3) {  // what the T5 encoder brought along exists in its pipeline only
        if (c.pos_type == 3) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: pos_type 3 (bucketed relative position bias) needs arch 3, not arch %d", c.arch);
        if (c.ffn_type > 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: ffn_type %d (3 = ReLU, 4 = tanh-GELU gate) needs arch 3, not arch %d", c.ffn_type, c.arch);
        if (c.rel_buckets != 0 || c.rel_max_distance != 0)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: rel_buckets %d / rel_max_distance %d need arch 3 (0 elsewhere)", c.rel_buckets, c.rel_max_distance);
    }
    if (c.arch != 2 && c.kv_heads != 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: kv_heads %d needs arch 2 (grouped-query attention exists in the causal pipeline only)", c.kv_heads);
    if (c.arch != 2 && c.arch != 3 && c.head_dim != 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim %d needs arch 2 (a stated head dimension exists in the causal pipeline only; 0 elsewhere)", c.head_dim);
    if (c.arch != 2 && c.qk_norm != 0)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: qk_norm %d needs arch 2 (the per-head RMSNorm of Q and K exists in the causal pipeline only)", c.qk_norm);
    if (c.arch == 2) {
        // the causal pipeline: heads of 64 (rope_qk_kernel, attention_causal_kernel) or, stated, of 128 (qknorm_rope_kernel, attention_causal_kernel<2, ..>); SwiGLU
        if (c.head_dim != 0 && c.head_dim != 64 && c.head_dim != 128)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim must be 0 (hidden / heads, which must be 64), 64 or 128 on arch 2, got %d", c.head_dim);
        if (c.qk_norm != 0 && c.qk_norm != 1) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: qk_norm must be 0 or 1, got %d", c.qk_norm);
        if (wide && c.heads * 128 > 2048)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim 128 needs heads * 128 <= 2048 (the attention width), got heads %d", c.heads);
        if (!wide && c.hidden != c.heads * 64)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 2 needs head dimension 64 (hidden=%d heads=%d)", c.hidden, c.heads);
        if (c.pos_type != 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 2 runs with rotary positions only (pos_type 2), not pos_type %d", c.pos_type);
        if (c.ffn_type != 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 2 runs with the SwiGLU feed-forward only (ffn_type 2), not ffn_type %d", c.ffn_type);
        if (c.kv_heads < 0 || c.kv_heads > c.heads || (c.kv_heads > 0 && c.heads % c.kv_heads != 0))
            return sc_fail(SC_ERR_INVALID, "sc_encoder_create: kv_heads must divide heads (1 <= kv_heads <= heads, 0 = heads), got kv_heads %d with heads %d", c.kv_heads,
                           c.heads);
        if (c.local_window != 0 || c.global_every > 1)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window %d / global_every %d need arch 1 (arch 2 attends causally in every layer)", c.local_window,
                           c.global_every);
        return SC_OK;
    }
    if (c.arch == 3) {
        // the T5 encoder: heads of 64 (Head64Rel), the bias table instead of positions, ReLU or the tanh-GELU gate
        if (c.head_dim != 0 && c.head_dim != 64)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: head_dim must be 0 (hidden / heads, which must be 64) or 64 on arch 3, got %d", c.head_dim);
        if (c.head_dim == 0 && c.hidden != c.heads * 64)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 3 needs head dimension 64 (hidden=%d heads=%d; head_dim 64 states it when hidden differs)", c.hidden,
                           c.heads);
        if ((c.heads * 64) % 128 || c.heads * 64 > 2048)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 3 needs heads * 64 (the attention width) a multiple of 128, at most 2048, got heads %d", c.heads);
        if (c.pos_type != 3) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 3 runs with the relative position bias only (pos_type 3), not pos_type %d", c.pos_type);
        if (c.ffn_type != 3 && c.ffn_type != 4)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 3 runs with ffn_type 3 (ReLU) or 4 (tanh-GELU gate), not ffn_type %d", c.ffn_type);
        if (c.max_pos > 2048) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 3 needs max_pos <= 2048 (the distance table's span), got %d", c.max_pos);
        if (c.local_window != 0 || c.global_every > 1)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window %d / global_every %d need arch 1 (arch 3 attends globally in every layer)", c.local_window,
                           c.global_every);
        return SC_OK;
    }
    if (c.arch == 0) {
        if (c.local_window != 0 || c.global_every > 1)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window %d / global_every %d need arch 1 (local attention exists in the pre-LN pipeline only)",
                           c.local_window, c.global_every);
        return SC_OK;
    }
    // the pre-LN pipeline: rotate-half rotation and the windowed kernel are written for 64-wide heads, its gate is GEGLU
    if (c.hidden != c.heads * 64)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 1 needs head dimension 64 (hidden=%d heads=%d)", c.hidden, c.heads);
    if (c.pos_type != 2) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 1 runs with rotary positions only (pos_type 2), not pos_type %d", c.pos_type);
    if (c.ffn_type != 1) return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: arch 1 runs with the GEGLU feed-forward only (ffn_type 1), not ffn_type %d", c.ffn_type);
    if (c.global_every < 1) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: global_every must be >= 1 with arch 1 (1 = every layer global), got %d", c.global_every);
    if (!sc_attention_window_supported(c.local_window))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_encoder_create: local_window must be even and within 2 .. 128, got %d", c.local_window);
    if (!(c.rope_theta_local >= 0.f)) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: rope_theta_local must be >= 0 (0 = 10000)");
    return SC_OK;
}

std::vector<float> sc_rope_table(int64_t positions, float theta_arg, int head_dim) {
    const double theta = theta_arg > 0.f ? (double)theta_arg : 10000.0;
    const int half = head_dim / 2;
    const size_t n = (size_t)positions * half;
    std::vector<float> tab(2 * n);
    for (int i = 0; i < half; ++i) {
        const double f = std::pow(theta, -2.0 * i / (double)head_dim);
        for (int64_t p = 0; p < positions; ++p) {
            tab[(size_t)p * half + i] = (float)std::cos((double)p * f);
            tab[n + (size_t)p * half + i] = (float)std::sin((double)p * f);
        }
    }
    return tab;
}

// ALiBi head slopes (Press et al.; the non-power-of-two rule of the jina-bert implementation)
static std::vector<float> alibi_slopes(int heads) {
    std::vector<float> sl;
    auto pow2_slopes = [&](int n, int take, int stride) {
        const double start = std::pow(2.0, -std::pow(2.0, -(std::log2((double)n) - 3.0)));
        double v = start;
        for (int i = 0, got = 0; i < n && got < take; ++i, v *= start)
            if (i % stride == 0) { sl.push_back((float)v); ++got; }
    };
    int p2 = 1;
    while (p2 * 2 <= heads) p2 *= 2;
    pow2_slopes(p2, p2, 1);
    if (p2 < heads) pow2_slopes(2 * p2, heads - p2, 2);
    return sl;
}

// the parameter arena: f32 tables + per-layer {bf16 matrices, f32 vectors}; e->layers is sized, e->foldable set
static void layout_params(sc_encoder* e, Arena& a) {
    const sc_encoder_cfg& c = e->cfg;
    const size_t H = c.hidden, F = c.ffn, F1 = ffn_gated(c) ? 2 * F : F, rope_n = (size_t)c.max_pos * (head_width(c) / 2), AW = (size_t)attn_width(c),
                 QN = AW + 2 * (size_t)kv_width(c);
    e->wemb = a.f32((size_t)c.vocab * H);
    e->pemb = c.pos_type == 0 ? a.f32((size_t)c.max_pos * H) : nullptr;
    e->slopes = c.pos_type == 1 ? a.f32((size_t)c.heads) : nullptr;
    e->rope_cos = c.pos_type == 2 ? a.f32(2 * rope_n) : nullptr;  // sc_rope_table: cos, then sin
    e->rope_sin = e->rope_cos ? e->rope_cos + rope_n : nullptr;
    e->rope_cos_l = c.arch == 1 ? a.f32(2 * rope_n) : nullptr;
    e->rope_sin_l = e->rope_cos_l ? e->rope_cos_l + rope_n : nullptr;
    e->rel_tbl = c.pos_type == 3 ? a.f32((size_t)c.heads * (2 * (size_t)c.max_pos - 1)) : nullptr;
    e->temb = a.f32(c.arch != 0 ? H : (size_t)c.type_vocab * H);  // arch 1, 2 have no type table: one row of zeros for the embedding kernels
    e->fing = c.arch != 0 ? a.f32(H) : nullptr;
    e->finb = c.arch != 0 ? a.f32(H) : nullptr;
    e->embg = a.f32(H);
    e->embb = a.f32(H);
    for (LayerW& w : e->layers) {
        w.wqkv = a.bf16(QN * H);    w.bqkv = a.f32(QN);
        w.wo = a.bf16(H * AW);      w.bo = a.f32(H);
        w.qng = c.arch == 2 && c.qk_norm ? a.f32((size_t)head_width(c)) : nullptr;
        w.kng = c.arch == 2 && c.qk_norm ? a.f32((size_t)head_width(c)) : nullptr;  // (by the configuration: a measuring arena hands out NULL)
        w.ln1g = a.f32(H);          w.ln1b = a.f32(H);
        w.w1 = a.bf16(F1 * H);      w.b1 = a.f32(F1);
        w.w2 = a.bf16(H * F);       w.b2 = a.f32(H);
        w.ln2g = a.f32(H);          w.ln2b = a.f32(H);
        if (!e->foldable) continue;
        w.wqkv_f = a.bf16(3 * H * H); w.c1q = a.f32(3 * H); w.c2q = a.f32(3 * H);
        w.w1_f = a.bf16(F1 * H);      w.c1f = a.f32(F1);    w.c2f = a.f32(F1);
        w.bb_o = a.f32(H);            w.bb_2 = a.f32(H);
    }
}

extern "C" sc_status sc_encoder_create(sc_runtime* rt, const sc_encoder_cfg* cfg, const void* weights_blob, size_t nbytes, sc_encoder** out) {
    if (!rt || !cfg || !out) return sc_fail(SC_ERR_INVALID, "sc_encoder_create: NULL argument");
    *out = nullptr;
    sc_status st = check_cfg(*cfg);
    if (st) return st;
    const int64_t nfl = blob_floats(*cfg);
    if (weights_blob && (int64_t)nbytes != nfl * 4)
        return sc_fail(SC_ERR_INVALID, "sc_encoder_create: weight blob is %zu bytes, config needs %lld", nbytes, (long long)(nfl * 4));
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_encoder* e = new (std::nothrow) sc_encoder();
    if (!e) return sc_fail(SC_ERR_NOMEM, "out of host memory");
    e->rt = rt;
    sc_runtime_retain(rt);
    e->cfg = *cfg;
    if (e->cfg.arch == 2 && e->cfg.kv_heads == 0) e->cfg.kv_heads = e->cfg.heads;  // (sc_encoder_info reports the count in use)
    if (e->cfg.arch == 2) e->cfg.head_dim = head_width(*cfg);                       // (... and the head dimension in use: 64 or 128)
    const int64_t H = cfg->hidden, F = cfg->ffn, L = cfg->layers, F1 = ffn_gated(*cfg) ? 2 * F : F, KV = kv_width(*cfg), AW = attn_width(*cfg), HD = head_width(*cfg);

    // staging copy of the f32 blob on device (freed after conversion)
    float* blob = nullptr;
    hipError_t he = hipMalloc((void**)&blob, (size_t)nfl * 4);
    if (he != hipSuccess) {
        delete e;
        sc_runtime_release(rt);
        return sc_fail(SC_ERR_NOMEM, "hipMalloc weight staging (%lld B) failed: %s", (long long)nfl * 4, hipGetErrorString(he));
    }
    auto fail = [&](sc_status code) {
        hipFree(blob);
        hipFree(e->params);
        delete e;
        sc_runtime_release(rt);
        return code;
    };
    // the LayerNorm-folded batch pipeline needs every GEMM on the 256 x 256 tile and the statistics in whole 256-column slots
    // (arch 1: the LayerNorm-folded pipeline has no pre-norm form yet)
    e->foldable = cfg->arch == 0 && (H % 256) == 0 && (F % 256) == 0 && (F1 % 256) == 0 && ((3 * H) % 256) == 0;
    e->layers.resize(L);
    Arena arena;
    layout_params(e, arena);  // measure
    he = hipMalloc((void**)&e->params, arena.used);
    if (he != hipSuccess) return fail(sc_fail(SC_ERR_NOMEM, "hipMalloc parameters (%zu B) failed: %s", arena.used, hipGetErrorString(he)));
    arena = Arena{e->params};
    layout_params(e, arena);  // place

    if (weights_blob) {
        he = hipMemcpyAsync(blob, weights_blob, (size_t)nfl * 4, hipMemcpyHostToDevice, s);
        if (he != hipSuccess) return fail(sc_fail(SC_ERR_HIP, "weight upload failed: %s", hipGetErrorString(he)));
    } else {
        // synthetic weights: every tensor ~ 0.02 * N(0,1) over the blob index, then LayerNorm gamma = 1,
        // beta = 0 and biases = 0 are overwritten below (same rule in oracle/bert_oracle.py synth_weights)
        sc_launch_synth_scaled(blob, nfl, cfg->synth_seed, 0.02f, 0.0f, s);
    }
    // walk the blob in its documented order
    int64_t off = 0;
    auto take = [&](int64_t n) { float* p = blob + off; off += n; return p; };
    enum { COPY, ONES, ZEROS };  // what a synthetic model holds instead of the blob's values
    auto put_f32 = [&](float* d, const float* src, int64_t n, int synth) {
        if (!weights_blob && synth == ONES) sc_launch_synth_scaled(d, n, 0, 0.0f, 1.0f, s);
        else if (!weights_blob && synth == ZEROS) hipMemsetAsync(d, 0, (size_t)n * 4, s);
        else hipMemcpyAsync(d, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
    };
    auto put_bf16 = [&](void* d, const float* src, int64_t n) { sc_launch_f32_to_bf16(src, d, n, s); };
    auto put_host = [&](float* d, const std::vector<float>& v) {
        hipMemcpyAsync(d, v.data(), v.size() * 4, hipMemcpyHostToDevice, s);
        hipStreamSynchronize(s);  // v goes out of scope
    };
    put_f32(e->wemb, take((int64_t)cfg->vocab * H), (int64_t)cfg->vocab * H, COPY);
    if (e->pemb) put_f32(e->pemb, take((int64_t)cfg->max_pos * H), (int64_t)cfg->max_pos * H, COPY);
    if (e->slopes) put_host(e->slopes, alibi_slopes(cfg->heads));
    if (e->rope_cos) put_host(e->rope_cos, sc_rope_table(cfg->max_pos, cfg->rope_theta, (int)HD));
    if (e->rope_cos_l) put_host(e->rope_cos_l, sc_rope_table(cfg->max_pos, cfg->rope_theta_local));
    if (e->rel_tbl) {  // rel_bias [rel_buckets, heads] of the blob (synthetic: the 0.02 N(0,1) values) -> the distance table, expanded on the host
        const int64_t nb = (int64_t)cfg->rel_buckets * cfg->heads;
        std::vector<float> rb((size_t)nb);
        he = hipMemcpyAsync(rb.data(), take(nb), (size_t)nb * 4, hipMemcpyDeviceToHost, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        if (he != hipSuccess) return fail(sc_fail(SC_ERR_HIP, "relative bias download failed: %s", hipGetErrorString(he)));
        put_host(e->rel_tbl, sc_rel_bias_table(rb.data(), cfg->rel_buckets, cfg->heads, cfg->rel_max_distance, cfg->max_pos));
    }
    if (cfg->arch != 0) hipMemsetAsync(e->temb, 0, (size_t)H * 4, s);
    else put_f32(e->temb, take((int64_t)cfg->type_vocab * H), (int64_t)cfg->type_vocab * H, COPY);
    if (cfg->arch < 2) {  // arch 2 and 3 have no embedding norm
        put_f32(e->embg, take(H), H, ONES);
        put_f32(e->embb, take(H), H, ZEROS);
    }
    for (int64_t l = 0; l < L; ++l) {
        LayerW& w = e->layers[l];
        // blob order: Wq bq Wk bk Wv bv Wo bo ln1g ln1b W1 b1 W2 b2 ln2g ln2b ; device: Wqkv = [Wq; Wk; Wv] (Wk, Wv: KV rows each)
        const float* wqkv_f32[3];
        for (int p = 0; p < 3; ++p) {
            const int64_t rows = p == 0 ? AW : KV, row0 = p == 0 ? 0 : AW + (p - 1) * KV;
            wqkv_f32[p] = take(rows * H);
            put_bf16((char*)w.wqkv + (size_t)row0 * H * 2, wqkv_f32[p], rows * H);
            put_f32(w.bqkv + row0, take(rows), rows, ZEROS);
        }
        put_bf16(w.wo, take(H * AW), H * AW);
        put_f32(w.bo, take(H), H, ZEROS);
        put_f32(w.ln1g, take(H), H, ONES);
        put_f32(w.ln1b, take(H), H, ZEROS);
        const float* w1_f32 = take(F1 * H);
        put_bf16(w.w1, w1_f32, F1 * H);
        put_f32(w.b1, take(F1), F1, ZEROS);
        put_bf16(w.w2, take(H * F), H * F);
        put_f32(w.b2, take(H), H, ZEROS);
        put_f32(w.ln2g, take(H), H, ONES);
        put_f32(w.ln2b, take(H), H, ZEROS);
        if (w.qng) {
            put_f32(w.qng, take(HD), HD, ONES);
            put_f32(w.kng, take(HD), HD, ONES);
        }
        if (e->foldable) {
            // the LayerNorm in front of this layer: the embeddings' for layer 0, else the previous layer's second one
            const float* gp = l == 0 ? e->embg : e->layers[l - 1].ln2g;
            const float* bp = l == 0 ? e->embb : e->layers[l - 1].ln2b;
            w.g_prev = gp;
            for (int p = 0; p < 3; ++p)  // Wq, Wk, Wv are separate tensors of the blob
                sc_launch_fold_ln_weights(wqkv_f32[p], gp, bp, w.bqkv + p * H, (int)H, (int)H, (char*)w.wqkv_f + (size_t)p * H * H * 2, w.c1q + p * H, w.c2q + p * H, s);
            sc_launch_fold_ln_weights(w1_f32, w.ln1g, w.ln1b, w.b1, (int)F1, (int)H, w.w1_f, w.c1f, w.c2f, s);
            sc_launch_add_vectors(w.bo, bp, w.bb_o, (int)H, s);
            sc_launch_add_vectors(w.b2, w.ln1b, w.bb_2, (int)H, s);
        }
    }
    if (e->fing) {
        put_f32(e->fing, take(H), H, ONES);
        put_f32(e->finb, take(H), H, ZEROS);
    }
    he = hipStreamSynchronize(s);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) return fail(sc_fail(SC_ERR_HIP, "encoder parameter setup failed: %s", hipGetErrorString(he)));
    hipFree(blob);
    *out = e;
    return SC_OK;
}

extern "C" sc_status sc_encoder_destroy(sc_encoder* e) {
    if (!e) return SC_OK;
    hipSetDevice(e->rt->device);
    hipStreamSynchronize(e->rt->stream);
    hipFree(e->params);
    hipFree(e->ws);
    hipFree(e->splitk);
    hipFree(e->pair.mem);
    hipFree(e->proj.mem);
    hipFree(e->score.mem);
    hipFree(e->token.mem);
    hipFree(e->tok[0].p);
    hipFree(e->tok[1].p);
    hipFree(e->late_aux.p);
    for (auto& slot : e->pin) {
        if (slot.host) hipHostFree(slot.host);
        if (slot.done) hipEventDestroy(slot.done);
    }
    sc_runtime* rt = e->rt;
    delete e;
    sc_runtime_release(rt);
    return SC_OK;
}

// the workspace for `tokens` token rows and `nb` chunks
static void layout_ws(sc_encoder* e, Arena& a, size_t tokens, size_t nb) {
    const size_t H = e->cfg.hidden, F = e->cfg.ffn, F1 = ffn_gated(e->cfg) ? 2 * F : F, slots = H / 256;
    const size_t AW = (size_t)attn_width(e->cfg), QN = AW + 2 * (size_t)kv_width(e->cfg);  // arch 2 at head dimension 128: AW may exceed H, QN 3 H
    e->x = a.bf16(tokens * H);
    e->x1 = a.bf16(tokens * H);
    e->y = a.bf16(tokens * H);
    e->qkv = a.bf16(tokens * (QN > 3 * H ? QN : 3 * H));
    e->ctx = a.bf16(tokens * (AW > H ? AW : H));
    e->hm = a.bf16(tokens * F1);
    e->hg = ffn_gated(e->cfg) ? a.bf16(tokens * F) : nullptr;
    e->ids = (int32_t*)a.take(tokens * 4);
    e->lens = (int32_t*)a.take(nb * 4);
    e->ones = e->cfg.arch == 3 ? (int32_t*)a.take(nb * 4) : nullptr;
    e->plan = (char*)a.take(PlanOffsets(tokens, nb, PackedCall::PAIRS).total);
    e->pooled = a.f32(nb * H);
    e->projected = e->proj.mem ? a.f32(nb * (size_t)e->proj.E) : nullptr;
    e->logits = a.f32(nb * 2);
    e->stat_a = e->foldable ? a.f32(slots * tokens * 2) : nullptr;
    e->stat_b = e->foldable ? a.f32(slots * tokens * 2) : nullptr;
    e->fin_a = e->foldable ? a.f32(tokens * 2) : nullptr;
    e->fin_b = e->foldable ? a.f32(tokens * 2) : nullptr;
}

sc_status ensure_ws(sc_encoder* e, int64_t rows, int64_t B) {
    const int64_t tokens = ceil256(rows);
    if (tokens <= e->ws_tokens && B <= e->ws_batch) return SC_OK;
    SC_HIP(hipStreamSynchronize(e->rt->stream));
    hipFree(e->ws);
    e->ws = nullptr;
    e->ws_tokens = 0;
    e->ws_batch = 0;
    Arena arena;
    layout_ws(e, arena, (size_t)tokens, (size_t)B);  // measure (no buffer is left pointing into the freed workspace)
    hipError_t he = hipMalloc((void**)&e->ws, arena.used);
    if (he != hipSuccess) return sc_fail(SC_ERR_NOMEM, "hipMalloc encoder workspace (%zu B) failed: %s", arena.used, hipGetErrorString(he));
    SC_HIP(hipMemsetAsync(e->ws, 0, arena.used, e->rt->stream));  // padded rows must hold finite values
    arena = Arena{e->ws};
    layout_ws(e, arena, (size_t)tokens, (size_t)B);  // place
    if (e->ones) SC_HIP(hipMemsetD32Async((hipDeviceptr_t)e->ones, 1, (size_t)B, e->rt->stream));
    e->ws_tokens = tokens;
    e->ws_batch = B;
    return SC_OK;
}

extern "C" sc_status sc_encoder_info(sc_encoder* e, sc_encoder_cfg* cfg_out) {
    if (!e || !cfg_out) return sc_fail(SC_ERR_INVALID, "sc_encoder_info: NULL argument");
    *cfg_out = e->cfg;
    return SC_OK;
}
