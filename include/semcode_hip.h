/*
 * semcode_hip.h -- C ABI of libsemcode_hip.so (MI355X / gfx950 backend for semcode's
 * embed -> store -> top-k path).
 *
 * This is the drop-in boundary: plain C, opaque handles, plain pointers and sizes, no
 * torch / C++ types.  The only callers are the two Python seam classes in
 * semcode_amd/embeddings/providers.py and semcode_amd/storage/milvus_store.py (via ctypes),
 * bench.py and the tests.
 *
 * Reference interfaces each group replaces (paths relative to the reference checkout):
 *   - encoder  : Embeddings.embed_documents / embed_query reached through
 *                EmbeddingProviderFactory.create   src/semcode/embeddings/providers.py:34-104
 *                called at                         src/semcode/services/indexer.py:150
 *                                                  src/semcode/rag/pipeline.py:171-175
 *   - index    : pymilvus Collection.{create_index,upsert,search,load} as used by
 *                MilvusVectorStore                  src/semcode/storage/milvus_store.py:39-148
 *
 * Conventions
 *   - every function returns sc_status (0 = OK, negative = error); the message of the last
 *     error raised on the calling thread is available through sc_last_error();
 *     no exception or abort crosses this boundary;
 *   - host pointers are contiguous, little-endian, row-major; the caller owns every buffer
 *     it passes, the library owns only handle-internal device memory;
 *   - "_dev" variants take DEVICE pointers (e.g. torch tensor data_ptr()) and enqueue on the
 *     runtime's stream; where one of them has to wait for the stream (a flag read back, a host
 *     table that must outlive a kernel) its comment says so; host variants always synchronise;
 *   - row ids are int64 row numbers (shard base + local row); string primary keys and
 *     metadata stay in Python (milvus_store.py:110-130 column lists);
 *   - a handle may be used from several threads (FastAPI threadpool, api/main.py:202):
 *     calls on one handle are serialised by a per-handle mutex.
 */
#ifndef SEMCODE_HIP_H
#define SEMCODE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t sc_status;

enum {
    SC_OK = 0,
    SC_ERR_INVALID = -1,     /* bad argument                                  */
    SC_ERR_HIP = -2,         /* a HIP runtime call failed (no GPU, OOM, ...)   */
    SC_ERR_STATE = -3,       /* call not valid in the handle's current state  */
    SC_ERR_UNSUPPORTED = -4, /* shape / option outside what the kernels cover */
    SC_ERR_NOMEM = -5        /* host or device allocation failed              */
};

/* metric_type of milvus_store.py:78-82,144 ("IP" in the reference; L2 and COSINE are the
 * other two Milvus float-vector metrics and are what BASELINE.json measures). */
typedef enum { SC_METRIC_IP = 0, SC_METRIC_L2 = 1, SC_METRIC_COSINE = 2 } sc_metric;
/* index_type of milvus_store.py:80 ("IVF_FLAT"); FLAT = exhaustive scan. */
typedef enum { SC_INDEX_FLAT = 0, SC_INDEX_IVF_FLAT = 1 } sc_index_kind;

typedef struct sc_runtime sc_runtime;
typedef struct sc_index sc_index;
typedef struct sc_encoder sc_encoder;

/* ------------------------------------------------------------------ runtime ---- */

typedef struct sc_runtime_cfg {
    int32_t device;  /* HIP device ordinal (one process per GPU: LOCAL_RANK)            */
    void* stream;    /* hipStream_t to enqueue on, or NULL = library-owned stream       */
    int32_t flags;   /* reserved, 0                                                     */
} sc_runtime_cfg;

/* Library version string ("semcode_hip x.y"). Never fails. */
const char* sc_version(void);
/* Copies the calling thread's last error message into buf (NUL-terminated, truncated to n). */
sc_status sc_last_error(char* buf, size_t n);

/* Replaces pymilvus connections.connect(...) (milvus_store.py:42-47): binds a device. */
sc_status sc_runtime_create(const sc_runtime_cfg* cfg, sc_runtime** out);
/* Drops the creator's reference.  Indexes, encoders and communicators created on the runtime hold references of their own,
 * so they stay usable and may be destroyed afterwards, in any order; the stream is released with the last of them. */
sc_status sc_runtime_destroy(sc_runtime* rt);
/* Re-point the runtime at another hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). */
sc_status sc_runtime_set_stream(sc_runtime* rt, void* stream);
/* Block until everything enqueued on the runtime's stream has finished. */
sc_status sc_runtime_synchronize(sc_runtime* rt);
/* Device facts for bench.py / DESIGN.md: name (<=255 chars), CU count, total HBM bytes. */
sc_status sc_runtime_device_info(sc_runtime* rt, char* name, size_t n, int32_t* cus, int64_t* hbm_bytes);
/* When enabled (> 0), the dominant kernels of each search / embed call are bracketed by hipEvents on the runtime's
 * stream (bench.py's roofline figure): every launch of the scan classes; every `enabled`-th launch of the encoder
 * classes (GEMM, attention), whose ~60 launches per step would otherwise pay 1.6 % for their event pairs. */
sc_status sc_runtime_set_profiling(sc_runtime* rt, int32_t enabled);
/* Sum (ms) and count of profiled (bracketed) launches of kernel class `which` since the last reset
 * (which: 0 = distance scan, 1 = top-k merge, 2 = encoder GEMM, 3 = attention). Synchronises. */
sc_status sc_runtime_profile_read(sc_runtime* rt, int32_t which, double* total_ms, int64_t* launches);
sc_status sc_runtime_profile_reset(sc_runtime* rt);

/* Deterministic synthetic data (bench / tests): out[r*ld + c] = g(seed, first_row + r, c, dim)
 * for c < dim, 0 for dim <= c < ld, with g an integer-hash Irwin-Hall(12) approximation of
 * N(0,1) that oracle/sc_oracle.c reproduces bit for bit.  `out` is a DEVICE pointer. */
sc_status sc_synth_fill_dev(sc_runtime* rt, float* out, int64_t rows, int32_t dim, int32_t ld,
                            uint64_t seed, int64_t first_row);

/* ------------------------------------------------------------------- encoder ---- */

/* Transformer encoder: the BERT-family post-LN models (arch 0; the "transformer-encoder forward" of BASELINE.json;
 * BERT-base shape = 30522 / 768 / 12 / 12 / 3072 / 512 / 2, eps 1e-12) and the pre-LN ModernBERT family (arch 1, below).  Head
 * dimension hidden / heads must be 64, or 32 with
 * pos_type 0 (MiniLM-L6 shape = 30522 / 384 / 6 / 12 / 1536 / 512 / 2); 32 with ALiBi or rotary positions is SC_ERR_UNSUPPORTED.
 *
 * arch 1 (answerdotai/ModernBERT-base, gte-modernbert-base, modernbert-embed-base; base shape = 50368 / 768 / 22 / 12 / 1152, eps 1e-5):
 *   h = LN_emb(tok_emb[id]);  per layer  h += Attn(attn_norm(h)),  h += MLP(mlp_norm(h))  with attn_norm of layer 0 the identity;
 *   pooled from final_norm(h).  No position and no type table.  MLP = Wo (gelu(gate) * up) (ffn_type 1).  Rotary positions (pos_type 2)
 *   with two bases: rope_theta in the global layers, rope_theta_local in the local ones.  Layer l is global iff l % global_every == 0;
 *   in the other layers a token attends to the real keys with |i - j| <= local_window / 2 only (encoder_window.hip).
 *   arch 1 requires pos_type 2, ffn_type 1 and head dimension 64; anything else is SC_ERR_UNSUPPORTED.  ffn must be a multiple of 128
 *   as for every model (base: 1 152), so ModernBERT-large (ffn 2 624) is refused by that rule.  The forward runs the stand-alone
 *   LayerNorm pipeline for every batch size (sc_encoder_set_path only decides about split-K); a LayerNorm-folded pre-norm pipeline
 *   is a follow-up.  [CLS] pooling runs the whole last layer (the pruned last layer is the post-LN one).  sc_encoder_score_pairs is
 *   SC_ERR_UNSUPPORTED (the family's classifier is dense -> GELU -> LayerNorm -> linear, not pooler + linear: sc_encoder_set_score_head /
 *   sc_encoder_score_seqs run it).  Texts stay capped at 2 048 tokens.
 *
 * arch 2 (the Qwen2 / Qwen2.5 decoder backbone behind code-embedding models such as jina-code-embeddings-0.5b, gte-Qwen2, KaLM-mini;
 *   0.5B shape = 151936 / 896 / 24 layers / 14 heads, 2 K/V heads / 4864, eps 1e-6, rope_theta 1e6): a pre-norm CAUSAL decoder.
 *   h = tok_emb[id] (no embedding norm, no position and no type table);  per layer  h += Attn(RMS_in(h)),  h += MLP(RMS_post(h));  pooled
 *   from RMS_final(h).  RMS(x) = x * rsqrt(mean(x^2) + ln_eps) * gamma, statistics in f32, no beta.  MLP = W2 (silu(gate) * up) (ffn_type 2).
 *   Rotary positions (pos_type 2) with the one base rope_theta.  Scores are q.k / 8 over the keys j <= i, j < len only (encoder_causal.hip).
 *   Grouped-query attention: K and V have kv_heads heads of 64 (0 = heads); query head h reads K/V head h / (heads / kv_heads) (grouped,
 *   not interleaved).  arch 2 requires pos_type 2, ffn_type 2, head dimension 64 (or 128, stated: below), 1 <= kv_heads <= heads with heads % kv_heads == 0,
 *   local_window 0 and global_every <= 1, next to the hidden % 128, ffn % 128 and hidden <= 2048 rules of every model; anything else is
 *   SC_ERR_UNSUPPORTED or SC_ERR_INVALID.  kv_heads != 0 on arch 0 or 1 is SC_ERR_UNSUPPORTED.  The forward runs the stand-alone-norm
 *   pipeline for every batch size (sc_encoder_set_path only decides about split-K).  Pooling: sc_encoder_set_pooling 2 (the last real
 *   token's row) or 0 (masked mean); 1 ([CLS]) is SC_ERR_INVALID.  sc_encoder_score_pairs is SC_ERR_UNSUPPORTED (rerankers of this family:
 *   sc_encoder_set_score_head / sc_encoder_score_seqs).  Texts stay capped at
 *   2 048 tokens.
 *   Heads of 128 (head_dim 128: Qwen3-Embedding-0.6B = 151669 / 1024 / 28 layers / 16 heads, 8 K/V heads of 128 / 3072, qk_norm 1, no q/k/v
 *   bias; Qwen2.5-1.5B behind jina-code-embeddings-1.5b and gte-Qwen2-1.5B-instruct = 1536 / 28 / 12 heads, 2 K/V heads of 128 / 8960, biases,
 *   no QK-norm).  head_dim 0 keeps the rule above (hidden / heads, which must be 64); 64 states it; 128 must be stated -- it is never derived
 *   from hidden / heads -- and then hidden need not equal heads * 128: the attention width AW = heads * head_dim (a multiple of 128, at most
 *   2 048) is the width of Q and of the attention output, the output projection is [H, AW].  Scores are q.k / sqrt(head_dim); the rotation pairs
 *   the columns (j, j + head_dim / 2) of a head with the angle p * rope_theta^(-2j / head_dim).  qk_norm 1: Q and K get an RMSNorm over each
 *   head's head_dim columns BEFORE the rotation (f32 statistics, eps = ln_eps, one gamma [head_dim] for Q and one for K per layer), at either
 *   head width.  Any other head_dim is SC_ERR_UNSUPPORTED, any other qk_norm SC_ERR_INVALID; a non-zero head_dim or qk_norm on arch 0 or 1 is
 *   SC_ERR_UNSUPPORTED.  Out of scope: heads of 128 on arch 0 / 1, hidden above 2 048 (Qwen3-Embedding-4B / 8B, the 7B models), sliding windows.
 *
 * arch 3 (the T5 ENCODER behind Salesforce/codet5p-110m-embedding = 32100 / 768 / 12 layers / 12 heads / 3072 ReLU, sentence-transformers/gtr-t5-*,
 *   sentence-t5-* and the instructor backbones; eps 1e-6): h = tok_emb[id] (no embedding norm, no position and no type table);  per layer
 *   h += Wo Attn(RMS(h)),  h += W2 act(W1 RMS(h));  pooled from RMS_final(h), RMS as on arch 2.  Positions enter through a bucketed relative
 *   bias only (pos_type 3): scores are q.k + rel_bias[bucket(j - i)][head] over the real keys j < len, with NO 1/sqrt(d) scaling, one
 *   learned table [rel_buckets, heads] for all layers.  Bucket rule (transformers' bidirectional one), nb = rel_buckets / 2, me = nb / 2,
 *   n = |j - i|:  b = (j > i) ? nb : 0;  b += n if n < me, else b += min(nb - 1, me + trunc(log(n / me) / log(rel_max_distance / me) * (nb - me))),
 *   evaluated in float32 as transformers does (sc_diag_rel_buckets returns the integers).  ffn_type 3 = Linear-ReLU-Linear (T5 v1.0, CodeT5+);
 *   ffn_type 4 = gated tanh-GELU ("gelu_new": 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))); T5 v1.1, flan, sentence-T5), W1 [2*ffn, H] with
 *   the wi_0 (activated) rows first, then wi_1.  arch 3 requires pos_type 3, ffn_type 3 or 4, rel_buckets even (32 in released models) and
 *   rel_max_distance (128), head dimension 64 -- head_dim 0 = hidden / heads, which must be 64; 64 stated: the attention width AW = heads * 64
 *   may differ from hidden as on arch 2 (t5-v1.1-small: 512 hidden, 6 heads) -- AW a multiple of 128, kv_heads, qk_norm, local_window all 0,
 *   max_pos <= 2048, next to the hidden % 128, ffn % 128 and hidden <= 2048 rules; anything else is SC_ERR_UNSUPPORTED or SC_ERR_INVALID with a
 *   message naming the field.  pos_type 3, ffn_type 3 / 4, rel_buckets and rel_max_distance on arch 0 - 2 are SC_ERR_UNSUPPORTED.  Pooling:
 *   sc_encoder_set_pooling 0 (masked mean of RMS_final(h)) or 1 (the first token's row, RMS_final in f32 inside the pooling kernel; the whole
 *   last layer runs); 2 is SC_ERR_INVALID.  sc_encoder_score_pairs, sc_encoder_set_score_head, sc_encoder_score_seqs and
 *   sc_encoder_set_token_head are SC_ERR_UNSUPPORTED.  The forward is the stand-alone-norm pipeline of arch 1 / 2 for every batch size.
 *   The projection behind the pooling of these models (CodeT5+'s proj, the Dense module of sentence-T5 / GTR) is sc_encoder_set_output_proj.
 *   Out of scope: the T5 decoder and seq2seq rerankers (monoT5), d_kv 128 and hidden above 2 048 (t5-3b / 11b, the xl / xxl sentence
 *   models), Instructor's instruction-masked pooling, .bin checkpoints, GGUF, the LayerNorm-folded pipeline and the pruned first-token layer
 *   for arch 3, texts beyond 2 048 tokens. */
typedef struct sc_encoder_cfg {
    int32_t vocab, hidden, layers, heads, ffn, max_pos, type_vocab;
    float ln_eps;
    int32_t normalize;    /* 1 = L2-normalise the pooled vector                               */
    uint64_t synth_seed;  /* used only when no weight blob is given (benchmarks)              */
    int32_t pos_type;     /* 0 = learned absolute position table (BERT); 1 = ALiBi: no table, scores get
                             -slope_h * |i - j| (jina-embeddings-v2 family named in the reference README);
                             2 = rotary (nomic-bert): no table, Q and K rotated by position ("rotate-half" pairing
                             (j, j + 32) of a head, angle p * rope_theta^(-2j/64)); max_pos bounds the sequence length;
                             3 = the bucketed relative position bias of arch 3 (above): no table, no rotation */
    int32_t ffn_type;     /* 0 = Linear-GELU-Linear (BERT); 1 = GEGLU: W1 is [2*ffn, H] (gate rows first, then up
                             rows), hidden = gelu(gate) * up, b1 is [2*ffn] (zeros for bias-free models);
                             2 = SwiGLU (nomic-bert): the same layout, hidden = silu(gate) * up;
                             3 = Linear-ReLU-Linear, 4 = gated tanh-GELU in the layout of 1 (both arch 3 only, above) */
    float rope_theta;     /* pos_type 2: rotary base (1000 for nomic-embed-text); 0 = 10000                   */
    /* appended; all zero = the behaviour of the struct without them */
    int32_t arch;           /* 0 = post-LN BERT family; 1 = pre-LN ModernBERT; 2 = pre-norm causal decoder, Qwen2 family (above) */
    int32_t local_window;   /* arch 1: total window of the local layers, even, 2 .. 128 (128 for the released models) */
    int32_t global_every;   /* arch 1: layer l is global iff l % global_every == 0; 1 = every layer global; 3 for the released models */
    float rope_theta_local; /* arch 1: rotary base of the local layers (10000); rope_theta is the global layers' (160000); 0 = 10000 */
    int32_t kv_heads;       /* arch 2: K / V heads of the grouped-query attention, a divisor of heads; 0 = heads.  Must be 0 on arch 0, 1 */
    int32_t head_dim;       /* arch 2: 0 = hidden / heads (must be 64), 64, or 128 (stated; hidden need not be heads * 128).  Must be 0 on arch 0, 1 */
    int32_t qk_norm;        /* arch 2: 1 = per-head RMSNorm of Q and K before the rotation (Qwen3); 0 = none.  Must be 0 on arch 0, 1 */
    int32_t rel_buckets;      /* arch 3 (pos_type 3): buckets of the relative position bias, even (32 in released models).  Must be 0 on arch 0 - 2 */
    int32_t rel_max_distance; /* arch 3 (pos_type 3): distance from which on every position shares the last bucket (128).  Must be 0 on arch 0 - 2 */
} sc_encoder_cfg;

/* Size in bytes of the f32 weight blob sc_encoder_create expects for cfg.  Blob order (all f32,
 * torch.nn.Linear layout [out, in]): word_emb [vocab,H], pos_emb [max_pos,H], type_emb [type_vocab,H],
 * emb_ln_gamma [H], emb_ln_beta [H], then per layer: Wq [H,H], bq, Wk, bk, Wv, bv, Wo [H,H], bo,
 * ln1_gamma, ln1_beta, W1 [ffn,H], b1 [ffn], W2 [H,ffn], b2 [H], ln2_gamma, ln2_beta.
 * pos_type 1 and 2 drop pos_emb from the blob; ffn_type 1 and 2 make W1 [2*ffn,H] (gate rows, then up rows) and b1 [2*ffn].
 * Bias-free models (nomic-bert) keep their bias slots, filled with zeros.
 * arch 1: word_emb [vocab,H], emb_ln_gamma, emb_ln_beta, the same per-layer order with ln1 = attn_norm (layer 0's slot is present and
 * ignored) and ln2 = mlp_norm, W1 = Wi (its first ffn rows are the activated half, i.e. the gate rows), W2 = mlp.Wo, then
 * final_norm_gamma [H], final_norm_beta [H].  No pos_emb, no type_emb (type_vocab is not read).  Bias and beta slots stay present:
 * zeros for the released models, the values of a model with norm_bias / attention_bias / mlp_bias.
 * arch 2, KV = kv_heads * 64: word_emb [vocab,H], then per layer Wq [H,H], bq [H], Wk [KV,H], bk [KV], Wv [KV,H], bv [KV], Wo [H,H], bo [H],
 * ln1_gamma [H] (= input_layernorm), ln1_beta [H], W1 [2*ffn,H] (gate_proj rows, then up_proj rows), b1 [2*ffn], W2 [H,ffn] (= down_proj),
 * b2 [H], ln2_gamma [H] (= post_attention_layernorm), ln2_beta [H], then final_norm_gamma [H], final_norm_beta [H].  No embedding norm, no
 * pos_emb, no type_emb.  The beta slots are present and never read (RMSNorm has none); slots of biases a model lacks (Qwen2: bo, b1, b2)
 * hold zeros.  On the device the projection is fused as [Wq; Wk; Wv], N = H + 2 KV (always a multiple of 128), written in 64-column
 * blocks; the rotation covers its first heads + kv_heads blocks.
 * arch 2 with head_dim 128 (or 64 stated), AW = heads * head_dim, KV = kv_heads * head_dim: Wq [AW,H], bq [AW], Wk [KV,H], bk [KV], Wv [KV,H],
 * bv [KV], Wo [H,AW], bo [H], the rest as above; with qk_norm, q_norm_gamma [head_dim] and k_norm_gamma [head_dim] follow each layer's ln2_beta.
 * The fused projection stays in 64-column blocks, N = AW + 2 KV: a 128-wide head is two consecutive blocks.  sc_encoder_info reports the
 * head_dim in use on arch 2 (64 or 128, never 0).
 * arch 3, AW = heads * 64: word_emb [vocab,H], rel_bias [rel_buckets, heads] (transformers' layout of relative_attention_bias.weight), then
 * the arch 2 per-layer order without the QK-norm vectors -- Wq [AW,H], bq, Wk, bk, Wv, bv, Wo [H,AW], bo, ln1_gamma (layer.0.layer_norm),
 * ln1_beta, W1 ([ffn,H] = wi at ffn_type 3; [2*ffn,H] = wi_0 rows, then wi_1 rows at ffn_type 4), b1, W2 [H,ffn] (= wo), b2, ln2_gamma
 * (layer.1.layer_norm), ln2_beta -- then final_norm_gamma [H], final_norm_beta [H].  Bias slots hold zeros for released models and are
 * honoured by the GEMM epilogues; the beta slots are present and never read. */
sc_status sc_encoder_blob_bytes(const sc_encoder_cfg* cfg, int64_t* out);
/* Replaces EmbeddingProviderFactory.create() loading a model (providers.py:69-100): uploads the
 * weights (converted to bf16 on device).  weights_blob == NULL: synthetic weights 0.02*N(0,1) from
 * cfg.synth_seed, LayerNorm gamma 1 / beta 0, biases 0 (random-init benchmark weights). */
sc_status sc_encoder_create(sc_runtime* rt, const sc_encoder_cfg* cfg, const void* weights_blob, size_t nbytes, sc_encoder** out);
sc_status sc_encoder_destroy(sc_encoder* enc);
sc_status sc_encoder_info(sc_encoder* enc, sc_encoder_cfg* cfg_out);
/* The forward has two pipelines with the same arithmetic up to rounding: batches of more than 1 024 token rows run 256 x 256-tile
 * GEMMs with every LayerNorm folded into the neighbouring GEMMs (statistics from the producing epilogue, normalisation in the
 * consuming one: no LayerNorm kernel); smaller batches -- a query -- run split-K GEMMs with stand-alone LayerNorm kernels.
 * path 0 = that rule, 1 = the batch pipeline for every size, 2 = the small-batch pipeline for every size (tests, A/B runs). */
sc_status sc_encoder_set_path(sc_encoder* enc, int32_t path);
/* How a text's vector is taken from the last hidden state: pooling 0 (the default) = the masked mean over its real tokens; 1 = the
 * row of its first token, [CLS] (llama.cpp's pooling type 2: BAAI/bge-*-en-v1.5, snowflake-arctic-embed-*, mxbai-embed-large, gte-*).
 * With pooling 1 every embedding entry point -- sc_encoder_embed_ids, _dev, _into, _into_async, sc_encoder_embed_packed, _into,
 * _into_async, both pipelines -- returns the last hidden state, after its LayerNorm, of row i * S (rectangles) or of the text's first
 * packed row, L2-normalised when cfg.normalize is set by the rule of the mean kernels (x / max(|x|, 1e-12)).  The last LayerNorm then
 * runs on B rows (cls_rows_kernel, f32), and -- unless "cls_prune" of sc_diag_set_option is 0 -- so does the last layer behind its QKV
 * projection: attention of the one query row per text (attention_cls_kernel), output projection and feed-forward on ceil256(B)
 * compact rows.  Pruned and unpruned vectors agree to bf16 rounding, not bit for bit; a text's vector does not depend on its
 * batch-mates either way.  The mode takes effect with the next call; any other value is SC_ERR_INVALID and changes nothing.
 * sc_encoder_score_pairs does not read the mode.
 * pooling 2 = the row of the text's last real token (row start + len - 1 of a rectangle or of packed rows): the vector of causal
 * embedding models.  Accepted on arch 2 only (on arch 0 and 1 it is SC_ERR_INVALID like any unknown value): the row gets RMS_final in
 * f32 and is L2-normalised by the rule above.  On arch 2 pooling 1 is SC_ERR_INVALID (a causal first token sees only itself) and
 * pooling 0 takes RMS_final over all rows, then the mean kernels.  On arch 3 pooling 1 is the first token's row with RMS_final in f32. */
sc_status sc_encoder_set_pooling(sc_encoder* enc, int32_t pooling);
sc_status sc_encoder_get_pooling(sc_encoder* enc, int32_t* out);
/* The output projection behind the pooling of an embedding model: CodeT5+ (first token -> Linear(768, 256) -> L2), sentence-T5 / GTR (mean ->
 * Dense(768, 768, no bias) -> L2).  W [E,H] f32 host, torch.nn.Linear layout; b [E] or NULL; E a multiple of 16, 16 <= E <= 2048 (else
 * SC_ERR_INVALID); W == NULL removes it.  Accepted on every arch, for the pooled embedding calls only: pair, score and token calls do not read
 * it.  With a projection installed the pooled row is taken UN-normalised, out = W pooled + b, then x / max(|x|, 1e-12) when cfg.normalize;
 * every embedding entry point -- sc_encoder_embed_ids, _dev, _into, _into_async, sc_encoder_embed_packed, _into, _into_async -- writes [B, E],
 * and the _into forms require an index of dimension E.  A text's vector is the same bits whichever batch-mates it has (output_proj_kernel:
 * f32 MFMA, 16 rows a workgroup, every sum in an order that depends on (H, E) only).  The call drains the stream and lets go of the workspace.
 * sc_encoder_out_dim: the width of what the embedding entry points return now (E, or hidden). */
sc_status sc_encoder_set_output_proj(sc_encoder* enc, const float* W, const float* b, int32_t E);
sc_status sc_encoder_out_dim(sc_encoder* enc, int32_t* out);
/* Replaces Embeddings.embed_documents / embed_query after tokenisation (indexer.py:150,
 * pipeline.py:171-175): ids [B,S] int32 (S in {32,64,128,256,512}, padded by the caller), lens [B] =
 * number of real tokens per row (keys >= len are masked, pooling = mean over the first len tokens),
 * out [B,hidden] f32.  Host pointers; synchronises. */
sc_status sc_encoder_embed_ids(sc_encoder* enc, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, float* out);
/* Same with DEVICE pointers; asynchronous on the runtime's stream. */
sc_status sc_encoder_embed_ids_dev(sc_encoder* enc, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t S,
                                   float* out_dev);

/* embed_documents + upsert of one batch (indexer.py:150 -> milvus_store.py:128) without leaving the device: the
 * pooled vectors go straight from the encoder's output buffer into index rows `rows` (semantics of
 * sc_index_put_rows).  out may be NULL; if not, the vectors are also copied to the host [B,hidden].  Encoder and
 * index must belong to the same runtime and hidden == dim.  Host pointers; synchronises. */
sc_status sc_encoder_embed_ids_into(sc_encoder* enc, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, sc_index* ix,
                                    const int64_t* rows, float* out);

/* The same, pipelined: returns as soon as the batch is enqueued (ids, lens and rows are first copied into pinned staging
 * owned by the encoder, so the caller's buffers are free immediately).  Up to two batches are in flight; a third call
 * waits for the first.  The host prepares batch i+1 (tokenising, primary-key bookkeeping) while the device embeds batch i.
 * Argument errors are reported at once; a failure of the device work is reported by the call that next waits for that
 * batch (a later _async call or sc_encoder_wait). */
sc_status sc_encoder_embed_ids_into_async(sc_encoder* enc, const int32_t* ids, const int32_t* lens, int32_t B, int32_t S, sc_index* ix,
                                          const int64_t* rows);
/* Block until every batch enqueued by sc_encoder_embed_ids_into_async has finished. */
sc_status sc_encoder_wait(sc_encoder* enc);

/* Packed variable-length batches: the same forward without padding every text to the longest one.  The caller passes the token
 * ids of B texts one after another, unpadded: ids [offsets[B]] int32, offsets [B+1] with offsets[0] == 0, text i = ids[offsets[i] ..
 * offsets[i+1]).  The library lays text i out on ceil32(len_i) token rows, one text after another, rounds the total up to 256 rows
 * (the GEMM tile) and builds -- on the host, in pinned staging -- what the kernels need: the padded id array (alignment rows and the
 * tail take token 0; their keys are masked, their outputs are finite and never pooled), a position per row, the first row and the
 * length of every text, and the table of attention work items.  GEMMs, LayerNorm and the gate kernels run unchanged over those
 * rows; embedding, rotary rotation, attention and pooling have packed forms (encoder_packed.hip).  Rotary models rotate Q and K with
 * the stand-alone kernel in both pipelines: fusing the rotation into the QKV epilogue for packed rows is a follow-up.
 * sc_encoder_set_path applies as for rectangles; the automatic rule (folded above 1 024 rows) looks at the packed row count.
 * Packed and padded vectors of a text agree to bf16 rounding, not bit for bit.
 * SC_ERR_INVALID, with nothing launched and nothing changed: a NULL pointer, B outside 1 .. 65536, offsets[0] != 0, a text shorter
 * than 1 or longer than 2 048 tokens, or longer than max_pos for models with a position or rotary table.  SC_ERR_UNSUPPORTED: more
 * than SC_ENCODER_PACKED_MAX_ROWS token rows -- 256 x 2 048, the largest rectangle sc_encoder_embed_ids is given by this project's
 * callers; the workspace takes 17 KiB (BERT-base) to 29 KiB (nomic-bert) per row, i.e. up to 15 GiB at the bound. */
#define SC_ENCODER_PACKED_MAX_ROWS 524288
/* The token rows the packed forward runs for these offsets (a multiple of 256).  Validates as the embed calls do; no GPU work.
 * Callers size their batches with it. */
sc_status sc_encoder_packed_rows(sc_encoder* enc, const int64_t* offsets, int32_t B, int64_t* rows);
/* sc_encoder_embed_ids on packed input: out [B,hidden] f32.  Host pointers; synchronises. */
sc_status sc_encoder_embed_packed(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, int32_t B, float* out);
/* sc_encoder_embed_ids_into / _into_async on packed input: same semantics, same in-flight rules (the two kinds share the two pinned
 * slots: at most two batches of either kind are in flight, sc_encoder_wait covers both). */
sc_status sc_encoder_embed_packed_into(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, int32_t B, sc_index* ix, const int64_t* rows,
                                       float* out);
sc_status sc_encoder_embed_packed_into_async(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, int32_t B, sc_index* ix,
                                             const int64_t* rows);

/* Pairs (cross-encoder / reranker): the stage after retrieval.  A pair is ONE packed sequence [CLS] question [SEP] passage [SEP]; the
 * first first_lens[i] tokens of pair i take segment id 0 (type_emb row 0), the rest segment id 1.  The forward is the packed one --
 * same plan, same GEMMs, same attention over the pair's real length, both pipelines (sc_encoder_set_path applies as for packed
 * embeds) -- with three differences: the embedding kernels read a per-row segment id that the plan carries next to the positions
 * (alignment rows and the tail take 0), the output is the last hidden state (after its LayerNorm) of each pair's FIRST row instead
 * of a mean (the packed pooling kernels with a length of one), and it is never L2-normalised, whatever cfg.normalize says.  The
 * head then computes, in f32 from f32 weights kept on the device, p = tanh(pooler_w cls + pooler_b) -- or p = cls without a pooler --
 * and logits = cls_w p + cls_b (pair_head_kernel: 16 pairs per workgroup, f32 MFMA, fixed reduction orders; tanh saturates to +-1
 * and is finite for every input).  What the logits mean is the model's business: a caller scores with logit[0] (1 label) or
 * logit[1] - logit[0] (2 labels).
 * sc_encoder_set_pair_head installs, replaces or (cls_w == NULL) removes the head; pooler_w == NULL = no pooler; the arrays are
 * copied before it returns.  Embedding calls on the same encoder are not affected by a head.
 * sc_encoder_score_pairs: ids / offsets as sc_encoder_embed_packed; out_logits [B,num_labels]; out_cls [B,hidden] (the [CLS] rows the
 * head read) or NULL.  Host pointers; synchronises; shares the two pinned slots and the in-flight rules of the packed embed calls.
 * SC_ERR_INVALID, with nothing launched and nothing changed: no head installed, a NULL pointer, B outside 1 .. 65536, offsets[0] != 0,
 * a pair shorter than 2 or longer than 2 048 tokens, or longer than max_pos for models with a position or rotary table,
 * first_lens[i] outside 1 .. len_i, a second segment (first_lens[i] < len_i) on a model with type_vocab < 2, num_labels outside
 * 1 .. 2.  SC_ERR_UNSUPPORTED: more than SC_ENCODER_PACKED_MAX_ROWS token rows (size batches with sc_encoder_packed_rows).
 * [CLS]-pooled embedding models are sc_encoder_set_pooling's business, not the head's: pairs ignore that mode, embeds ignore the head.
 * Out of scope: heads other than pooler + linear (Electra), more than 2 labels, an asynchronous or
 * device-pointer form.  ALiBi and rotary models with type_vocab >= 2 run, but no reference pins their result. */
sc_status sc_encoder_set_pair_head(sc_encoder* enc, const float* pooler_w /*[H,H]*/, const float* pooler_b /*[H]*/,
                                   const float* cls_w /*[num_labels,H]*/, const float* cls_b /*[num_labels]*/, int32_t num_labels);
sc_status sc_encoder_score_pairs(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, const int32_t* first_lens, int32_t B,
                                 float* out_logits, float* out_cls);

/* Score heads of the other two families (rerankers on ModernBERT and on the Qwen2 / Qwen3 decoders).  New surface next to the pair head:
 * sc_encoder_set_pair_head / sc_encoder_score_pairs stay as they are on every arch, their refusals on arch 1 and 2 included.
 * A sequence is ONE packed text the caller built ([CLS] question [SEP] passage [SEP], or a decoder's prompt around query and document);
 * there are no segment ids -- neither family has a type table.  The forward is the packed forward's, with one choice taken away: a scored
 * call never takes the split-K GEMMs, which the embedding calls pick, with their factor, by the call's row count (up to 1 024 rows).  Every
 * GEMM is the 256-tile kernel, whose sums for a row do not depend on the rows around it, so sc_encoder_set_path is accepted and leaves the
 * logits unchanged; a call of few rows pays for it with GEMMs that fill less of the chip (DESIGN.md has the measured cost).  What else
 * differs is the row that is pooled and what happens to it:
 *   the row r [H], f32, NEVER L2-normalised whatever cfg.normalize and sc_encoder_set_pooling say --
 *     kind 1, pooling 1: final_norm of the text's first row;  pooling 0: the mean of the final_norm rows over the text's real tokens
 *       (alignment rows and tail rows are never included);
 *     kind 2 (pooling 2): RMS_final of row start + len - 1, the last real token.
 *   the head, in f32 from f32 weights kept on the device --
 *     kind 1 (score_head_kernel):  a_n = sum_k dense_w[n][k] r[k] + dense_b[n];  g_n = gelu_erf(a_n) (the FFN epilogue's erf GELU, |error| <=
 *       2.5e-7);  mean = (sum_n g_n) / H;  var = (sum_n (g_n - mean)^2) / H -- two passes, the mean first, then centred squares;
 *       rstd = 1 / sqrt(var + norm_eps);  p_n = (g_n - mean) * rstd * norm_g[n] + norm_b[n];  logit_c = sum_n cls_w[c][n] p_n + cls_b[c].
 *       Reduction orders: a_n accumulates k in 16-wide stages, k = 16 st + 4 j + c taken by the f32 MFMA of (j, c), even and odd stages in
 *       two chains added at the end, then the bias.  The three sums over n each run per lane over n = 16 w + 64 t + 4 j + c in (t, c)
 *       order (squares and classifier terms by fmaf) for the 16 (w, j) lanes of a row, whose partials are added in (w, j) order, w < 4,
 *       j < 4; cls_b last.  16 rows per workgroup; the activated values never leave the registers between the three passes.
 *     kind 2 (score_linear_kernel):  logit_c = sum_k cls_w[c][k] r[k] + cls_b[c]; lane j < 64 takes the 4-element pieces j, j + 64, ... in
 *       ascending order into one fmaf chain, the 64 chains are added by the xor butterfly 32, 16, .. 1; cls_b last.
 *   No atomics, every order fixed and independent of the batch, in the forward as in the head: a text's logits are the same bits
 *   whichever batch-mates it has and wherever it stands among them, on every sc_encoder_set_path setting.  What the logits mean is the model's business: logit[0] for one
 *   label, logit[1] - logit[0] for two -- for a causal LM scored through two vocabulary rows the caller passes (false row, true row).
 * sc_encoder_set_score_head installs, replaces or (head == NULL) removes the head; the arrays are copied before it returns, and it waits for
 * the stream before a head goes.  Validation comes first: SC_ERR_UNSUPPORTED on an arch 0 encoder (its head is sc_encoder_set_pair_head's);
 * SC_ERR_INVALID for a kind other than 1 on arch 1 / 2 on arch 2, a pooling the kind does not have, num_labels outside 1 .. 2, norm_eps
 * not > 0 (kind 1), a NULL dense_w / norm_g (kind 1) or cls_w, a non-NULL dense / norm array on kind 2 -- the installed head stays.
 * The head is independent of the pair head's slot and of the embedding calls: those are unaffected by it, and it by them.
 * sc_encoder_score_seqs: ids / offsets as sc_encoder_embed_packed; out_logits [B,num_labels]; out_rows [B,hidden] (the rows r the head
 * read) or NULL.  Host pointers; synchronises; shares the two pinned slots and the in-flight rules of the packed calls.  With nothing
 * launched and nothing changed -- SC_ERR_INVALID: no head installed, a NULL pointer, B outside 1 .. 65536, offsets[0] != 0, a text shorter
 * than 1 token, longer than 2 048 tokens or than max_pos; SC_ERR_UNSUPPORTED: an arch 0 encoder (sc_encoder_score_pairs), more than
 * SC_ENCODER_PACKED_MAX_ROWS token rows.
 * Out of scope: a _dev or asynchronous form, other activations, more than 2 labels, hidden above 2 048, heads on arch 0; sharing the K / V
 * of a prompt prefix across the pairs of one question (the real lever for decoder rerankers: it needs a new attention launch form) and
 * pruning the last layer to the scored rows. */
typedef struct sc_score_head {
    int32_t kind;        /* 1 = prediction head of the pre-norm family (arch 1 only); 2 = linear head on the last token (arch 2 only) */
    int32_t pooling;     /* kind 1: 0 = masked mean over the text's real rows, 1 = its first row; kind 2: must be 2 (last real token) */
    int32_t num_labels;  /* 1 or 2 */
    float   norm_eps;    /* kind 1 */
    const float *dense_w /*[H,H]*/, *dense_b /*[H] or NULL*/, *norm_g /*[H]*/, *norm_b /*[H] or NULL*/;   /* kind 1; all NULL on kind 2 */
    const float *cls_w /*[num_labels,H]*/, *cls_b /*[num_labels] or NULL*/;
} sc_score_head;
sc_status sc_encoder_set_score_head(sc_encoder* enc, const sc_score_head* head /* NULL removes */);
sc_status sc_encoder_score_seqs(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, int32_t B, float* out_logits /*[B,num_labels]*/,
                                float* out_rows /*[B,H] or NULL*/);

/* Late interaction (ColBERT): one vector per token and MaxSim, the second kind of reranker next to the cross-encoders above.  A document is
 * encoded once, independently of the question; a (question, document) pair then costs one small matrix product.  New surface: the pair
 * head, the score head, the pooling mode and every embedding call stay as they are and are unaffected by the token head, and it by them.
 * The forward is the packed forward's up to and including the model's last norm, with no pooling kernel and no pruned [CLS] last layer;
 * the token head then runs on the rows that are asked for.  As a scored call, a token call never takes the split-K GEMMs, and on arch 0 its
 * pipeline does not follow its row count: the LayerNorm-folded pipeline where the model's shapes allow it, the stand-alone one otherwise
 * (sc_encoder_set_path 2 still forces the stand-alone one, and the two differ in their rounding points).  So a text's vectors are the same
 * bits whichever batch-mates it has and wherever it stands among them.
 *   token head (token_head_kernel):  v = Wt x, Wt [W,H] rounded to bf16 once at install, x the bf16 row after the last norm (arch 0: the last
 *     layer's second LayerNorm; arch 1: final_norm), f32 accumulation by v_mfma_f32_16x16x32_bf16 over k ascending in steps of 32; then
 *     v * (1 / max(sqrt(|v|^2), 1e-12)), |v|^2 reduced in a fixed order (per lane over its 4-column pieces in ascending column tile, then the
 *     four lanes of a row by the xor butterfly 16, 32).  No bias.  W a multiple of 16 within 16 .. 128.  No atomics.
 *   rows asked for:  expand_id < 0 (documents): the len_i real rows of text i.  expand_id >= 0 (queries): all ceil32(len_i) rows of the text's
 *     32-row span; the alignment rows len_i .. ceil32(len_i) carry token expand_id (the model's [MASK]) at the positions that continue the
 *     text's, are attended as queries and stay masked as keys -- ColBERT's query augmentation with unattended [MASK] tokens at query_maxlen
 *     32.  A query has at most 128 tokens.  Vectors are written compactly, text after text: out[tok_start[i] + t][W].
 *   MaxSim (maxsim_kernel; the rule lives once, in semcode_amd/csrc/maxsim_rule.h):  dot(Q_t, D_j) = one fmaf chain from +0 in the canonical
 *     k order of the f32 MFMA (inside each block of 16: k = 16 t + 4 g + c, c outer, g inner);  m_t = the maximum over the kept j < nd under
 *     the total order of the order-preserving score key (-0 < +0);  score = ((+0 + m_0) + m_1) + ..., t ascending, one correctly rounded
 *     addition at a time, never fused.  One workgroup per pair, document tokens in tiles of 16 spread over four waves, the waves' maxima
 *     combined through the LDS under the same order, the sum taken by one lane.  Bit-identical to sc_diag_maxsim_host for every finite input.
 * sc_encoder_set_token_head installs, replaces or (w == NULL) removes the head; the array is copied before it returns and it waits for the
 * stream before a head goes.  SC_ERR_UNSUPPORTED on an arch 2 encoder; SC_ERR_INVALID for a W outside the rule -- the installed head stays.
 * sc_encoder_embed_tokens: ids / offsets as sc_encoder_embed_packed; out [sum n_i, W] f32 and out_counts [B] = n_i (host).  Synchronises.
 * sc_encoder_score_late: the queries' forward into one device buffer, the documents' into a second, maxsim_kernel over the P pairs
 * (pair_q[p], pair_d[p]); out_scores [P].  d_keep: one byte per document token in d_ids order, 0 = the token takes no part in a maximum
 * (punctuation), NULL = every token does.  The token vectors never leave the device; the call synchronises once, at its end.  It uses the two
 * pinned plan slots, one per side; the token buffers belong to the encoder and grow on demand.
 * With nothing launched and nothing changed -- SC_ERR_INVALID: no head installed, a NULL pointer, B outside 1 .. 65536, offsets[0] != 0, a
 * text shorter than 1 token, longer than 2 048 tokens or than max_pos, a query longer than 128 tokens, on an arch 1 model with local layers a query whose last expansion row lies more than local_window / 2
 * behind its last token (it would see no key there; never the case at the released window of 128), expand_id outside the vocabulary, P < 1,
 * a pair index out of range, a document without a kept token; SC_ERR_UNSUPPORTED: an arch 2 encoder, either side over
 * SC_ENCODER_PACKED_MAX_ROWS token rows.
 * sc_diag_maxsim runs the kernel alone on uploaded arrays, sc_diag_maxsim_host the rule on the CPU (no GPU involved): Q / D [.., W] f32 token
 * vectors, text i's at rows [off[i], off[i + 1]) (int32 offsets from 0), keep NULL or one byte per document token.  A document without a
 * kept token scores nq * -inf = -inf there.
 * Storing token vectors in the index (a multi-vector collection) and scoring from them without a passage forward: sc_index_put_tokens,
 * sc_index_rerank_late and sc_index_search_late, below.
 * sc_encoder_embed_tokens_into: the hand-over at ingest.  The document-side call of sc_encoder_embed_tokens (expand_id < 0; the same
 * pipeline rules, so the same bits) whose token head writes straight into the token pool of `ix`: text i's KEPT token vectors become the
 * tokens of local row rows[i], with the semantics of sc_index_put_tokens(ix, rows, B, kept counts, .., W, fmt) below -- appended, the rows
 * repointed, their old tokens dead, the automatic compaction at the end.  keep: one byte per input token in ids order, as d_keep above,
 * 0 = the token is not stored (it is still attended), NULL = every token is stored; a text without a kept token gets count 0, which
 * removes the row's tokens.  The flags enter the host plan: a dropped token's packed row maps to no output row, the kept ones are numbered
 * compactly, text after text (sc_diag_encoder_plan_keep shows that plan without a device).  fmt 0 stores the head's f32 bits; fmt 1 rounds
 * them in the kernel's epilogue by the rule of the store (sc_diag_round_bf16), 8-byte stores: the stored bits are those the host path
 * (sc_encoder_embed_tokens, drop, sc_index_put_tokens) stores.  out_counts [B] or NULL receives the kept counts.  No token vector crosses
 * to the host; the call synchronises once, at its end (and where the pool has to grow).  Order: everything validated; room made (the
 * table follows the rows, the pool grows -- SC_ERR_NOMEM leaves the store as it was); the forward into pool[used ...); only then the
 * table repointed and used advanced -- a failed forward leaves the store unchanged, nothing points at the tail it wrote.  Takes the
 * encoder's mutex, then the index's, as sc_encoder_embed_packed_into.  With nothing launched and nothing changed -- SC_ERR_INVALID: a NULL
 * pointer (keep and out_counts aside), no token head installed, fmt outside 0 / 1, the head's W or fmt differing from an installed
 * store's, encoder and index on different runtimes, rows out of range or not distinct, every refusal of sc_encoder_embed_tokens;
 * SC_ERR_UNSUPPORTED: an arch 2 encoder, more than SC_ENCODER_PACKED_MAX_ROWS token rows.
 * Out of scope: arch 2; an asynchronous form of the hand-over (pool growth reallocates and must synchronise; the late model shares the
 * dense encoder's stream); query lengths above 128; XLM-R backbones (jina-colbert-v2); a projection with a bias. */
sc_status sc_encoder_set_token_head(sc_encoder* enc, const float* w /*[W,H] or NULL*/, int32_t W);
sc_status sc_encoder_embed_tokens(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, int32_t B, int32_t expand_id, float* out /*[sum n_i,W]*/,
                                  int32_t* out_counts /*[B]*/);
sc_status sc_encoder_score_late(sc_encoder* enc, const int32_t* q_ids, const int64_t* q_offsets, int32_t Bq, int32_t expand_id, const int32_t* d_ids,
                                const int64_t* d_offsets, int32_t Bd, const uint8_t* d_keep /*or NULL*/, const int32_t* pair_q, const int32_t* pair_d, int32_t P,
                                float* out_scores /*[P]*/);
sc_status sc_encoder_embed_tokens_into(sc_encoder* enc, const int32_t* ids, const int64_t* offsets, int32_t B, const uint8_t* keep /*[offsets[B]] or NULL*/,
                                       sc_index* ix, const int64_t* rows /*[B]*/, int32_t fmt, int32_t* out_counts /*[B] or NULL*/);
sc_status sc_diag_maxsim(sc_runtime* rt, const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int32_t* d_off, int32_t Bd, const uint8_t* keep,
                         const int32_t* pair_q, const int32_t* pair_d, int32_t P, int32_t W, float* out);
sc_status sc_diag_maxsim_host(const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int32_t* d_off, int32_t Bd, const uint8_t* keep,
                              const int32_t* pair_q, const int32_t* pair_d, int32_t P, int32_t W, float* out);

/* ----------------------------------------------------------------- tokenizer ---- */
typedef struct sc_tokenizer sc_tokenizer;
/* Host-side WordPiece tokenizer (BERT scheme), the step the reference leaves to its provider's library (raw strings
 * are handed over at indexer.py:150).  vocab_utf8 = contents of a vocab.txt (one token per line; needs [UNK] [CLS]
 * [SEP]).  No GPU involved. */
sc_status sc_tokenizer_create(const char* vocab_utf8, size_t nbytes, int32_t lowercase, sc_tokenizer** out);
sc_status sc_tokenizer_destroy(sc_tokenizer* tok);
sc_status sc_tokenizer_info(sc_tokenizer* tok, int32_t* vocab_size, int32_t* pad, int32_t* unk, int32_t* cls, int32_t* sep);
/* texts i = bytes[offsets[i] .. offsets[i+1]) (UTF-8).  ids [n,S] ([CLS] pieces [SEP], truncated to min(max_tokens,S),
 * padded with [PAD]), lens [n].  Non-ASCII text is normalised as BERT's tokenizer does (NFD accent stripping and lower-casing for
 * uncased vocabularies, CJK ideographs spaced out, Unicode punctuation and whitespace classes, control / format characters
 * dropped; tables generated from the build image's transformers BertTokenizer, tests/golden/tokenizer_unicode.json).  Only a
 * text that is not valid UTF-8 is left alone: needs_fallback[i] = 1, lens[i] = 0.  threads <= 0: all hardware threads. */
sc_status sc_tokenizer_encode(sc_tokenizer* tok, const char* bytes, const int64_t* offsets, int32_t n, int32_t max_tokens, int32_t S,
                              int32_t* ids, int32_t* lens, uint8_t* needs_fallback, int32_t threads);

/* Diagnostics: run ONE encoder kernel on host f32 data (rounded to bf16 on device, result widened
 * back to f32) so that the parity tests can check the GEMM and the attention kernel in isolation.
 * epi: 0 = bias, 1 = bias + erf-GELU, 2 = bias + residual R [M,N]; + 16: let small shapes take the split-K path the
 * encoder uses for batches of <= 1024 tokens.  out [M,N] = A [M,K] * W [N,K]^T.
 * M, N multiples of 128, K multiple of 64. */
sc_status sc_diag_gemm_bf16(sc_runtime* rt, int32_t epi, const float* A, const float* W, const float* bias, const float* R,
                            int32_t M, int32_t N, int32_t K, float* out);
/* sc_diag_gemm_bf16_ex: the same launch (epi 0, 1 or 2, no "+ 16") in the forms the forward passes use.  flags bit 0: C is written and
 *   returned in 64-column blocks [N/64][M][64]; bit 1: A is given as [K/64][M][64]; bit 2: the split-K scratch is offered (the launcher
 *   splits where sc_diag_gemm_splitk says so); bit 3: the 128-tile kernel runs even where M and N divide by 256.  The arguments are
 *   checked by host arithmetic before rt is looked at.  Blocked A is read by the per-tile 256-tile kernel only: with M or N not a
 *   multiple of 256, with bit 2 or with bit 3 it is SC_ERR_UNSUPPORTED (the launcher itself launches nothing for such a call).
 *   path (or NULL) [5] = what the launcher ran: {tile 128 / 256, K slices (1 = no split-K), walk order word, ring depth of the main loop
 *   (0 = one barrier per K-tile), non-temporal C stores 0 / 1}.  The 128-tile kernel reports order 0, depth 0, nt 0 (it has none of
 *   them), the split-K pair order 1 (row-major, no XCD remap), depth 0, nt 0.
 * sc_diag_gemm_path: M > 0: the path an [M,K] x [N,K] launch would take under the current options ("gemm_order", "gemm_pp", "gemm_nt")
 *   on a device with `cus` compute units (<= 0: the current device's), with the split-K scratch offered or not; host arithmetic only.
 *   M == 0: the path of the most recent plain launch of this process.
 * sc_diag_gemm_splitk: the K slices of the split-K rule alone (1 = no split) for `cus` compute units (<= 0: the current device's).
 * "gemm_order" of sc_diag_set_option: tile walk of the plain 256-tile launches (-1 = default: by shape, 0 below 8 MiB of weights and
 *   16 from there; else the order word: bit 0 = no XCD remap, word >> 1 = G > 1: column-major inside groups of G row panels). */
sc_status sc_diag_gemm_bf16_ex(sc_runtime* rt, int32_t epi, int32_t flags, const float* A, const float* W, const float* bias, const float* R,
                               int32_t M, int32_t N, int32_t K, float* out, int32_t* path);
sc_status sc_diag_gemm_path(int32_t M, int32_t N, int32_t K, int32_t cus, int32_t splitk_scratch, int32_t* path);
int32_t sc_diag_gemm_splitk(int32_t M, int32_t N, int32_t K, int32_t cus);
/* Times `iters` launches of one GEMM shape on device-resident synthetic data (kernel tuning; variant 0 =
 * the product kernel, other values = diagnostic ablations whose outputs are meaningless). */
sc_status sc_diag_gemm_bench(sc_runtime* rt, int32_t epi, int32_t M, int32_t N, int32_t K, int32_t iters, int32_t variant,
                             double* ms_per_launch);
/* cap_words / (8 * tiles) back-to-back traced launches of the 256x256-tile GEMM (M, N multiples of 256): out[launch][tile][8] =
 * {0: HW_ID, 1: XCC_ID, 2: entry, 3: main loop done, 4: epilogue issued, 5: stores drained}, stamps in 10 ns wall-clock
 * ticks.  Kernel tuning aid (scripts/gemm_trace.py). */
sc_status sc_diag_gemm_trace(sc_runtime* rt, int32_t epi, int32_t M, int32_t N, int32_t K, uint64_t* out, int64_t cap_words);
/* The int8 form of the 256 x 256 tile (the batched scan's int8 coarse stage) on its own: out [M,N] i32 = A [M,K] i8 * W [N,K]^T,
 * exact.  M, N multiples of 256, K multiple of 128. */
sc_status sc_diag_gemm_i8(sc_runtime* rt, const int8_t* A, const int8_t* W, int32_t M, int32_t N, int32_t K, int32_t* out);
/* Copies one workspace buffer of the encoder's last forward to the host (kernel debugging: 0 x, 1 y, 2 qkv, 3 ctx, 4 ffn hidden,
 * 5 / 6 partial row statistics, 7 / 8 finalised row statistics of the LayerNorm-folded pipeline). */
sc_status sc_diag_encoder_read(sc_encoder* enc, int32_t which, void* out, size_t nbytes);
/* Process-wide test / tuning switches, by name (results stay identical; unknown names: SC_ERR_INVALID).  "coarse_workgroups": grid
 * of the persistent coarse-scan kernel (0 = one workgroup per CU), so that tests can make a few workgroups walk many tiles;
 * "coarse_persistent": 0 = one workgroup per tile instead; "gemm_pp": main loop of the 256-tile GEMMs (-1 default, 0 = one barrier
 * per K-tile, 2..5 = ping-pong with that many half-tiles in flight); "ivf_refresh_nomem": 1 = the re-layout of a trained IVF index
 * after upserts fails as if the device were full (the search must then answer exhaustively instead of failing); "tighten": 0 = the batched scan's thresholds stay the kp-th best coarse keys
 * (no exact re-score of the 128 best before the large phases); "ivf_tail_rows": how many rows appended to a trained IVF_FLAT index may
 * stay behind its lists as a tail that probes scan exactly (-1 = default 65536; 0 = fold appended rows into the lists before every search);
 * "wide_candidates": 1 = the int8 stage keeps every key within its cut
 * (the form it otherwise switches to on corpora whose certificate fails) wherever it can; "collect_pass": 0 = queries a
 * coarse stage cannot certify go straight to the next stage (no collect pass); "ivf_coarse_nomem": 1 = the IVF coarse stage
 * cannot allocate its centred shadow (the search must then probe exactly instead of failing), 2 = the stage runs out of memory from
 * the second 4 096-query chunk of a batch on (the first chunk keeps its results, the exact probes answer the rest); "ivf_refine_cap":
 * rows per query the IVF coarse stage's refine step takes on (-1 = default 4096; a small value sends queries to the exact re-probe). */
sc_status sc_diag_set_option(const char* name, int32_t value);
/* "rope_fused" of sc_diag_set_option: how the batch pipeline of a rotary encoder rotates Q and K (-1 = default, 0 = the stand-alone
 * kernel after the QKV projection, 1 = inside that projection's epilogue); the two agree to bf16 rounding, not bit for bit.
 * sc_diag_rope: the stand-alone rotation kernel on qk [rows, heads*64] f32, in place (rounded to bf16 on device first; row r is
 * position r % S, S a power of two; theta <= 0 = 10000). */
sc_status sc_diag_rope(sc_runtime* rt, float* qk, int32_t rows, int32_t S, int32_t heads, float theta);
/* sc_diag_rel_buckets: T5's bucket rule of sc_encoder_cfg's comment, the function that builds the device table: out[d + span - 1] =
 *   bucket(d) for d = key - query in -(span - 1) .. span - 1.  Host arithmetic only: no runtime, no device.
 * sc_diag_ffn_act: the kernel between the two FFN GEMMs, kind = the model's ffn_type.  1 GEGLU, 2 SwiGLU, 4 the tanh-GELU gate: h [rows, 2F]
 *   (gate | up) -> out [rows, F] = gelu / silu / gelu_new (gate) * up.  3 = the ReLU pass on h [rows, F] (rounded to bf16) -> out [rows, F].
 *   F a multiple of 8. */
sc_status sc_diag_rel_buckets(int32_t rel_buckets, int32_t max_distance, int32_t span, int32_t* out);
sc_status sc_diag_ffn_act(sc_runtime* rt, int32_t kind, const float* h, int32_t rows, int32_t F, float* out);
/* sc_diag_output_proj: output_proj_kernel on its own.  x [B,H] f32 (taken as it is: pooled rows are f32), W [E,H], bias [E] or NULL ->
 * out [B,E] = W x + bias, L2-normalised by x / max(|x|, 1e-12) when normalize.  H, E multiples of 16 within 16 .. 2048. */
sc_status sc_diag_output_proj(sc_runtime* rt, const float* x, int32_t B, int32_t H, const float* W, const float* bias, int32_t E, int32_t normalize,
                              float* out);
/* sc_diag_attention_run: ONE launch of a product attention launcher, whichever the descriptor names.  The descriptor is validated and its
 * geometry derived by host arithmetic before rt is looked at.  d = head_dim, H = heads * d, kvh = kv_heads under the causal mask (query
 * head h reads K / V head h / (heads / kv_heads)), else heads; kv_heads is then 0 or heads.  qkv rows are [Q (heads) | K (kvh) | V (kvh)] x d.
 * mask: FULL    out = softmax over the keys j < len of QK^T / sqrt(d), times V.  d 64, or 32 (an even number of heads: a 64-column block holds
 *                 heads 2j and 2j+1).  slopes [heads]: the ALiBi bias of the product (d 64).  rel_bias [rel_buckets][heads] f32: T5, the scores
 *                 are q.k + rel_bias[bucket(key - query)][head] with NO 1 / sqrt(d), positions from the start of each sequence (d 64).
 *       WINDOW  the keys j < len with |i - j| <= local_window / 2 (even, 2 .. 128); a row that sees no key is zero.  d 64.
 *       CAUSAL  the keys j <= i, j < len.  d 64 or 128, 1 <= kv_heads <= heads <= 2048 / d, heads % kv_heads == 0.
 *       CLS     FULL for the first row of each text only, slopes with either d: out [B, H].  A row-major rectangle with S 1 .. 2048 (the
 *                 harness lays it out in 64-column blocks of ceil256(B*S) rows, as the QKV projection writes it).
 * Rows, starts == NULL: a rectangle of B texts of S rows (S one of 32, 64, 128, 256, 512, 1024, 2048), lens [B] clamped to 1 .. S, R = B*S
 *   rows in and out.  Every row is finite (rows at or beyond len are queries too).
 * Rows, starts != NULL: packed, S is not read; sequence b owns the rows starts[b] .. starts[b] + ceil32(lens[b]) (starts multiples of 32, lens
 *   1 .. 2048), R = the end of the last sequence rounded up to 256 rows in and out.  Every row of a sequence is finite, rows outside every
 *   sequence stay NaN.
 * blocked_rows == 0: qkv is [R][columns] row-major.  > 0: qkv is in 64-column blocks [columns / 64][blocked_rows][64], the layout the QKV
 *   projections write; a rectangle needs blocked_rows >= B*S (that GEMM's M) and still returns B*S rows, packed rows have R = blocked_rows >=
 *   the last sequence's end.  out [rows, H] is row-major; both forms give the same bits.
 * B 1 .. 65536, H <= 2048.  A head_dim, kv_heads or local_window no kernel has, and a combination no launcher serves (slopes with WINDOW,
 * CAUSAL, rel_bias or -- outside CLS -- d 32; rel_bias or WINDOW with d != 64; rel_bias with another mask than FULL; CLS with starts or
 * blocked_rows) are SC_ERR_UNSUPPORTED with a message naming the fields; anything else out of range is SC_ERR_INVALID. */
enum { SC_DIAG_ATTN_FULL = 0, SC_DIAG_ATTN_WINDOW = 1, SC_DIAG_ATTN_CAUSAL = 2, SC_DIAG_ATTN_CLS = 3 };
typedef struct sc_diag_attn {
    int32_t mask; /* SC_DIAG_ATTN_* */
    int32_t B, S, heads, kv_heads, head_dim, blocked_rows, local_window;
    const int32_t* starts;  /* NULL = the rectangle form, else [B] */
    const int32_t* lens;    /* [B] */
    const float* slopes;    /* NULL or [heads] */
    const float* rel_bias;  /* NULL = no T5 bias, else [rel_buckets][heads] */
    int32_t rel_buckets, rel_max_distance;
} sc_diag_attn;
sc_status sc_diag_attention_run(sc_runtime* rt, const sc_diag_attn* a, const float* qkv, float* out);

/* Single-kernel diagnostics of the LayerNorm-folded batch pipeline and of the stand-alone encoder kernels (tests/test_fold_kernels_gpu.py).
 * Same pattern as above: host f32 in, activations rounded to bf16 on the device, ONE launch through the product's own launcher, the
 * result widened to f32; synchronous; outputs are pre-filled with NaN so that an element the kernel leaves unwritten shows.
 * "gemm_nt" of sc_diag_set_option: C stores of the 256-tile GEMMs (-1 = default: non-temporal from 64 MiB of output, or the SC_GEMM_NT
 * environment variable; 0 = never; 1 = always) -- lets a small shape take the non-temporal store path; results are identical.
 * "gemm_strip": the EPI_LNA_* GEMMs as strips of consecutive column tiles of one row panel per workgroup (-1 = default: by shape, or
 * the SC_GEMM_STRIP environment variable; 0 = one workgroup per tile; L >= 1 = L tiles per strip, clamped to the tiles of a panel);
 * "gemm_strip_n": N > 0 applies a forced "gemm_strip" to the launches with that N only, the others run per tile (scripts/strip_sweep.py).
 * sc_diag_fold_ln: W [N,K], gamma / beta [K], bias [N] or NULL -> Wf [N,K] = bf16(W diag(gamma)) widened, c1 [N] = row sums of Wf,
 *   c2 [N] = bias + W beta (K a multiple of 4).
 * sc_diag_gemm_lna: epi 3 (EPI_LNA_BIAS), 4 (EPI_LNA_GELU) or 6 (EPI_LNA_BIAS_ROPE): C [M,N] = LN(A) W^T + b computed as
 *   rs (A Wf^T - mu c1) + c2 from the raw rows A [M,K], Wf / c1 / c2 as sc_diag_fold_ln returns them and the caller's partial row
 *   statistics stats_in [K/256][M][2] = (sum, sum of squares) per 256-column slot; fin [M][2] = the (mu, rs) the kernel publishes.
 *   flags bit 0: C is written (and returned) in 64-column blocks [N/64][M][64].  Rotary form: row r has position r & (rope_S - 1),
 *   rope_S a power of two, the first rope_ncols columns (multiple of 64) are rotated, theta <= 0 = 10000.  M, N, K multiples of 256.
 * sc_diag_gemm_resln: EPI_RESLN_STATS: C [M,N] = A W^T + bias + (R - mu) rs gam with (mu, rs) = fin [M][2] of the raw residual R [M,N]
 *   (bias already holds + beta); stats_out [N/256][M][2] = (sum, sum of squares) of the bf16 C per 256-column tile.  flags bit 0: A is
 *   given in 64-column blocks [K/64][M][64].
 * sc_diag_layernorm: x [tokens,H] -> LayerNorm rows (H a multiple of 8, <= 2048).
 * sc_diag_mean_pool: x [B*S,H] -> out [B,H] f32, masked mean over the first lens[b] rows (lens clamped to 1..S); normalize 0 = the
 *   sliced kernel, 1 = the one-workgroup kernel with L2 normalisation.  sc_diag_mean_pool_ln: the same of LayerNorm(y) from raw rows
 *   y [tokens_pad,H] and their partial statistics stats [slots][tokens_pad][2].
 * sc_diag_embed: ln 0 = embed_raw_kernel: rows [tokens_pad,H] = bf16((word + position) + type), stats [slots][tokens_pad][2] (slot 0 the
 *   sums of the rounded row, other slots and padding rows zero); ln 1 = embed_ln_kernel: rows [tokens,H] = LayerNorm of that sum.
 *   ids [tokens] are clamped to [0, vocab), position = token % S clamped to max_pos - 1; pemb NULL = no position table. */
sc_status sc_diag_fold_ln(sc_runtime* rt, const float* W, const float* gamma, const float* beta, const float* bias, int32_t N, int32_t K,
                          float* Wf, float* c1, float* c2);
sc_status sc_diag_gemm_lna(sc_runtime* rt, int32_t epi, int32_t flags, const float* A, const float* Wf, const float* c1, const float* c2,
                           const float* stats_in, float eps, int32_t M, int32_t N, int32_t K, int32_t rope_S, float rope_theta,
                           int32_t rope_ncols, float* C, float* fin);
/* Strip selection of the EPI_LNA_* GEMM launcher.  M > 0: tiles per strip an [M,K] x [N,K] launch would get under the current options
 * ("gemm_strip", "gemm_strip_n", "gemm_pp", SC_GEMM_STRIP) on a device with `cus` compute units (cus <= 0: the current device's),
 * 0 = one workgroup per tile; host arithmetic only.  M == 0: what the most recent EPI_LNA_* launch of this process used. */
int32_t sc_diag_gemm_strip(int32_t M, int32_t N, int32_t K, int32_t cus);
sc_status sc_diag_gemm_resln(sc_runtime* rt, int32_t flags, const float* A, const float* W, const float* bias, const float* gam, const float* R,
                             const float* fin, float eps, int32_t M, int32_t N, int32_t K, float* C, float* stats_out);
/* "cls_prune" of sc_diag_set_option: the last layer of a [CLS]-pooled forward (-1 = default: pruned, 0 = the full last layer over every
 * token row, 1 = on the [CLS] rows only). */
/* sc_diag_qknorm_rope: qknorm_rope_kernel (pos NULL: position = row % S, S a power of two <= 65536) or its packed form (pos [rows], clamped to
 * max_pos - 1; S then is the table's length, max_pos) on their own.  x [rows, (heads + 2 kv_heads) * head_dim] f32 as [Q | K | V] is rounded to
 * bf16, laid out in 64-column blocks, processed in place and returned widened in the same row-major form: the first heads + kv_heads heads
 * normalised (gamma_q / gamma_k [head_dim] non-NULL, both or neither; eps) and rotated (theta, 0 = 10000), the V columns as they went in.
 * head_dim 64 or 128. */
sc_status sc_diag_qknorm_rope(sc_runtime* rt, float* x, int32_t rows, int32_t S, const int32_t* pos, int32_t heads, int32_t kv_heads, int32_t head_dim,
                              float theta, const float* gamma_q, const float* gamma_k, float eps);
sc_status sc_diag_layernorm(sc_runtime* rt, const float* x, int32_t tokens, int32_t H, const float* gamma, const float* beta, float eps, float* out);
/* sc_diag_rmsnorm: rmsnorm_kernel, conventions of sc_diag_layernorm: x [tokens,H] -> x * rsqrt(mean(x^2) + eps) * gamma, bf16 rows. */
sc_status sc_diag_rmsnorm(sc_runtime* rt, const float* x, int32_t tokens, int32_t H, const float* gamma, float eps, float* out);
sc_status sc_diag_mean_pool(sc_runtime* rt, const float* x, const int32_t* lens, int32_t B, int32_t S, int32_t H, int32_t normalize, float* out);
sc_status sc_diag_mean_pool_ln(sc_runtime* rt, const float* y, const float* stats, int32_t slots, int32_t tokens_pad, const float* gamma,
                               const float* beta, float eps, const int32_t* lens, int32_t B, int32_t S, int32_t H, float* out);
sc_status sc_diag_embed(sc_runtime* rt, int32_t ln, const int32_t* ids, int32_t tokens, int32_t S, int32_t H, int32_t vocab, int32_t max_pos,
                        const float* wemb, const float* pemb, const float* temb, const float* gamma, const float* beta, float eps,
                        int32_t tokens_pad, int32_t slots, float* rows, float* stats);
/* The kernels of the pair path on their own (tests/test_rerank_gpu.py).  sc_diag_embed_pairs: sc_diag_embed with a position and a
 * segment id per row -- pos / types [tokens] int32, clamped into the tables, temb [type_vocab,H]; rows and stats as there.
 * sc_diag_pair_head: pair_head_kernel on f32 data as they are: cls [B,H], pooler_w [H,H] / pooler_b [H] (both NULL: no pooler),
 * cls_w [num_labels,H], cls_b [num_labels] -> out_logits [B,num_labels].  B 1 .. 65536, H a multiple of 16 up to 2 048, num_labels 1 or 2. */
sc_status sc_diag_embed_pairs(sc_runtime* rt, int32_t ln, const int32_t* ids, const int32_t* pos, const int32_t* types, int32_t tokens, int32_t H,
                              int32_t vocab, int32_t max_pos, int32_t type_vocab, const float* wemb, const float* pemb, const float* temb,
                              const float* gamma, const float* beta, float eps, int32_t tokens_pad, int32_t slots, float* rows, float* stats);
sc_status sc_diag_pair_head(sc_runtime* rt, const float* cls, int32_t B, int32_t H, const float* pooler_w, const float* pooler_b,
                            const float* cls_w, const float* cls_b, int32_t num_labels, float* out_logits);
/* sc_diag_score_head: the kernels of sc_encoder_set_score_head on f32 data as they are (tests/test_score_head_gpu.py): rows [B,H], the
 * head's host arrays -> out_logits [B,num_labels].  head->pooling is not read (the rows are given); the other rules of the head hold,
 * B 1 .. 65536, H a multiple of 16 up to 2 048. */
sc_status sc_diag_score_head(sc_runtime* rt, const float* rows, int32_t B, int32_t H, const sc_score_head* head, float* out_logits);

/* -------------------------------------------------------------- vector index ---- */

/* Replaces Collection(...)+create_index(IVF_FLAT, metric, nlist) (milvus_store.py:59-84).
 * nlist is ignored for SC_INDEX_FLAT.  row_base = global id of local row 0 (shard offset). */
sc_status sc_index_create(sc_runtime* rt, int32_t dim, sc_metric metric, sc_index_kind kind,
                          int32_t nlist, int64_t row_base, sc_index** out);
sc_status sc_index_destroy(sc_index* ix);
/* Number of stored rows / dimension / padded row stride (floats). */
sc_status sc_index_info(sc_index* ix, int64_t* rows, int32_t* dim, int32_t* ld);
/* Pre-size device storage for `rows` rows (avoids regrowth copies). */
sc_status sc_index_reserve(sc_index* ix, int64_t rows);
/* Append n host vectors [n,dim]; they become rows [old_rows, old_rows+n).  Part of
 * Collection.upsert (milvus_store.py:128) for ids not seen before. */
sc_status sc_index_add(sc_index* ix, const float* vecs, int64_t n);
/* Replace existing rows: rows[i] (local row number) <- vecs[i].  The replace-by-primary-key half
 * of Collection.upsert (milvus_store.py:128); the md5 -> row map lives in Python. */
sc_status sc_index_overwrite(sc_index* ix, const float* vecs, const int64_t* rows, int64_t n);
/* Upsert in one call: rows[i] <- vecs[i] where rows[i] is either an existing row (replace) or the next free row
 * (append; new rows must be numbered old_rows, old_rows+1, ... in the order they appear).  Row numbers must be
 * distinct.  One Collection.upsert batch (milvus_store.py:119-130) without the add/overwrite split. */
sc_status sc_index_put_rows(sc_index* ix, const float* vecs, const int64_t* rows, int64_t n);
/* Same with vecs a DEVICE pointer ([n,dim] f32, tight); rows stays a host pointer.  The copy of the vectors is enqueued on
 * the runtime's stream (the embed -> store hand-over without a trip through host memory); the call itself
 * waits for the stream before returning, because `rows` is the caller's pageable memory. */
sc_status sc_index_put_rows_dev(sc_index* ix, const float* vecs_dev, const int64_t* rows, int64_t n);
/* Delete rows: replaces Collection.delete(expr) of pymilvus.  (The reference never calls it -- its re-index only upserts,
 * src/semcode/services/indexer.py:185-188, so chunks whose key changed stay searchable for ever; MilvusVectorStore.delete /
 * delete_where and ingest_chunks(prune=True) close that gap on top of this call.)
 * rows: n distinct local row numbers in [0, rows).  They are removed and the survivors are renumbered densely in their order:
 * new number = old number - (deleted rows below it).  Afterwards the index answers every call as one into which only the
 * surviving vectors had been put in that order -- same results bit for bit on every search path; a trained IVF_FLAT index
 * stays trained with the same centroid bits and every survivor in its list (no k-means, no re-assignment, no re-layout; a
 * list may become empty).  Every per-row array is compacted in place on the device by stored position (corpus, norms, the
 * bf16 / int8 / centred shadows as far as they are valid, the IVF position map and list offsets); shadows that were valid
 * stay valid, pending per-row repairs stay pending.  Scratch is bounded (< 256 MiB) whatever the corpus size, plus 4 - 8 B
 * per deleted row for the delete list itself.
 * Everything is validated before anything changes: a row outside [0, rows), a repeated row or rows == NULL with n > 0 give
 * SC_ERR_INVALID and leave the index bit for bit as it was.  n == 0 is SC_OK and does nothing.  Deleting every row leaves
 * the index as freshly created (IVF lists dropped).  row_base is unchanged: the renumbering is local to this index.
 * Serialised with searches and upserts by the index lock, like sc_index_put_rows; synchronises the stream before returning.
 * Sharded collections (sc_index_*_sharded, storage/sharded.py) have no delete: out of scope here. */
sc_status sc_index_delete_rows(sc_index* ix, const int64_t* rows, int64_t n);
/* After sc_index_delete_rows: survivors above the first deleted stored position (`rows_moved`), bytes moved over all per-row
 * arrays (`bytes_moved`; each is read once and written once, twice where a chunk goes through the bounce buffer), and the
 * shadows that were valid before the call as bit sets (1 bf16, 2 int8, 4 centred IVF): `shadows_kept` were compacted,
 * `shadows_dropped` invalidated -- 0 unless every row was deleted. */
sc_status sc_index_last_delete_stats(sc_index* ix, int64_t* rows_moved, int64_t* bytes_moved, int32_t* shadows_kept, int32_t* shadows_dropped);
/* Copy rows [first, first+n) back to the host as [n,dim] (persistence, tests). */
sc_status sc_index_get_rows(sc_index* ix, int64_t first, int64_t n, float* out);
/* Resize to n rows and fill them on device with sc_synth_fill_dev(seed, first_row). */
sc_status sc_index_fill_synthetic(sc_index* ix, int64_t n, uint64_t seed, int64_t first_row);

/* Clustered synthetic corpus (IVF recall benchmarks): row = centre[hash(row) % nclusters] + spread * noise, all
 * from the same integer-hash generator. */
sc_status sc_index_fill_synthetic_clustered(sc_index* ix, int64_t n, uint64_t seed, int64_t first_row, int32_t nclusters, float spread);
/* Free the rebuildable device buffers of an index (bf16 shadow, search scratch). */
sc_status sc_index_release_scratch(sc_index* ix);

/* Replaces Collection.search(data=[vector], param={metric, nprobe}, limit=top_k)
 * (milvus_store.py:141-147), batched: q [Q,dim] host, out_dist [Q,k] f32, out_rows [Q,k] i64
 * (global ids, best first; ties broken by lower row id; missing hits = -1 / +inf-or--inf).
 * nprobe is ignored by FLAT indexes.  Distances: L2 = squared L2, IP = dot, COSINE = cosine.
 * Value contract (this and every other search entry point; stored rows and queries alike):
 *   - covered: vectors of finite f32 components whose squared norm |v|^2 is representable in f32 (neither overflows nor loses
 *     its terms to underflow; corpora scaled by 2^-40 .. 2^+40 are tested).  upsert accepts whatever the caller sends; what lies
 *     outside the contract is stored and searched, but nothing is promised about where it ranks.
 *   - zero-norm rule: under COSINE a row or a query with |v|^2 == 0 scores exactly +0.0 against anything (never 0 / 0): such
 *     a row ranks between the positive and the negative cosines, and a zero query returns rows 0 .. k-1.  Under IP a zero vector
 *     scores 0, under L2 the other vector's |.|^2.  (Results are read back from the sort key, where a score of +0.0 under IP /
 *     COSINE reads -0.0; compare zero scores by value, not by sign bit.)
 *   - ties: equal scores go to the lower row id, on every path (exact, batched at either coarse stage, masked, every IVF probe)
 *     -- also when thousands of rows tie with the k-th score.
 *   - outside the contract: NaN or Inf components, norms that overflow, subnormal intermediates (scales below 2^-40). */
sc_status sc_index_search(sc_index* ix, const float* q, int32_t Q, int32_t k, int32_t nprobe,
                          float* out_dist, int64_t* out_rows);
/* Same with DEVICE pointers (q row stride = dim): enqueued on the runtime's stream.  The exact scan (<= 16 queries, no IVF
 * probe) returns without waiting.  The batched path (bf16 coarse + f32 re-rank) reads the per-query certificate flags back and
 * so synchronises the stream once per call, and list-major IVF probing synchronises twice (probe ids to the host planner, plan
 * tables alive until the scan has run); the per-index mutex is held meanwhile.  Results are complete once the stream has
 * passed the call in either case. */
sc_status sc_index_search_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe,
                              float* out_dist_dev, int64_t* out_rows_dev);

/* Filtered search: Collection.search(..., expr=...) restricted to a set of rows the caller names.  (The reference has no such
 * call: its front ends drop the hits of an unfiltered top-k that fail the user's repo / language filter, src/semcode/frontend/app.py:100-116,
 * so a small repo in a large collection usually shows nothing.)  The index learns nothing about repos or languages: `allow` is a
 * bitset over LOCAL row numbers, bit (r & 31) of 32-bit word (r >> 5) set = row r may be returned; allow_words >= ceil(rows / 32);
 * bits at or beyond `rows` are ignored.  The result is, bit for bit, the exact exhaustive answer of an index that holds only the
 * allowed rows: ids are the rows' own (row_base + local row), distances the canonical fmaf chain, best first, ties by lower row
 * id, padded with -1 and +inf (L2) / -inf (IP, COSINE) when fewer than k rows are allowed.  All three metrics.  Always exact:
 * there is no nprobe, and a trained IVF_FLAT index is scanned where its rows lie -- listed rows through the position map, rows
 * appended since the layout behind the lists, overwritten rows in place -- without a refresh, a re-layout or k-means; a pending
 * tail and pending overwritten rows stay pending.  Nothing about later unmasked searches changes.
 * How: the bitset is compacted on the device into the ascending list of allowed stored positions (two deterministic passes, no
 * atomics), and a gathered form of the exact scan streams only those rows -- its 16-row tiles are fed by per-lane source addresses
 * from that list (HBM bytes = allowed * ld * 4 per pass of <= 16 queries; a larger batch runs ceil(Q / 16) passes in one launch).
 * The queries of a pass are resident in LDS, so rows too long for 16 of them take more passes: 3 072 dimensions leave room for
 * 6, i.e. 3 passes for 16 queries.  No allowed row, or an empty index: no scan is launched.  Every row allowed: the ordinary
 * exhaustive planner answers (same bits, and the batched path for large batches).
 * k outside 1 .. 1024, Q < 1, a NULL pointer or allow_words < ceil(rows / 32) give SC_ERR_INVALID before anything changes.
 * Host pointers; synchronises.
 * Out of scope: masks on the batched MFMA path and on the IVF probe paths (approximate filtered search), sharded collections
 * (sc_index_search_sharded*), a `paths` filter, Milvus expr strings. */
sc_status sc_index_search_masked(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint32_t* allow, int64_t allow_words,
                                 float* out_dist, int64_t* out_rows);
/* Same with DEVICE pointers (q row stride = dim), enqueued on the runtime's stream.  Synchronises the stream ONCE per call: the
 * number of allowed rows is read back to size the scan's grid and to take the two shortcuts above (plus whatever the exhaustive
 * planner waits for when every row is allowed, see sc_index_search_dev); the per-index mutex is held meanwhile.  Results are
 * complete once the stream has passed the call. */
sc_status sc_index_search_masked_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev,
                                     int64_t allow_words, float* out_dist_dev, int64_t* out_rows_dev);
/* After a masked search: rows its bitset allowed, rows the scan that answered read per pass (0: no scan was launched; allowed_rows:
 * the gathered scan; all rows: the exhaustive planner) and whether the gathered kernel ran.  "mask_gather" of sc_diag_set_option
 * (1) forces the gathered kernel even when every row is allowed (tests; results are identical; default 0). */
sc_status sc_index_last_mask_stats(sc_index* ix, int64_t* allowed_rows, int64_t* scanned_rows, int32_t* gathered);

/* Grouped search: Collection.search(..., group_by_field=...) -- at most ONE hit per group, exact.  (The reference has no such call:
 * its RAG pipeline spends rag_max_context_sources on whatever the top-k holds, src/semcode/rag/pipeline.py:93-129, so the chunks of one
 * large file crowd every other source out.)  The index learns nothing about files or repos: every local row carries an opaque int32
 * LABEL, any value, compared for equality only.
 * sc_index_set_groups installs labels[n] for the current rows (a device copy, 4 B per row; replaces any earlier set); n must equal the
 * row count.  The labels are the caller's data parked on the device: the library does not persist, compact or interpret them, and
 * they are not search scratch (sc_index_release_scratch keeps them).  They are valid while the index's row count equals the count
 * they were installed for: an append outdates them, and sc_index_delete_rows drops them, because it renumbers the rows.  Host
 * pointer; synchronises. */
sc_status sc_index_set_groups(sc_index* ix, const int32_t* labels, int64_t n);
/* The answer for a query: walk the allowed rows best first in the order of the keys (score, row) -- better score first, ties by
 * lower row id -- keep a row if no earlier row had its label, stop after k rows.  out_rows = row_base + row, out_dist = the same bits
 * the exact scan reports for that row, best first, padded with -1 and +inf (L2) / -inf (IP, COSINE) when the allowed rows hold
 * fewer than k distinct labels.  All labels distinct: the plain exact search.  All labels equal: a single hit.
 * allow == NULL (allow_words 0): every row; else the bitset of sc_index_search_masked (allow_words >= ceil(rows / 32)); a group whose
 * best row is not allowed is represented by its best allowed row.  Always exact, all three metrics, no nprobe; a trained IVF_FLAT
 * index is scanned as it lies, tail and overwritten rows included, without a refresh or a re-layout.
 * How: round 0 takes every query through the exhaustive planner (the masked search, with a bitset) at a candidate width W0 >= k, and a
 * selection kernel keeps the first row of every label of each best-first list, in list order.  A query is done with k labels, or when
 * its list held padding (every allowed row was seen).  Each remaining query then goes on in rounds of its own: an exclusion kernel
 * streams the labels (4 B per row) into a bitset of the allowed rows whose label is not among its hits, the masked search answers
 * over that bitset at width W1, the selection kernel appends.  Every round finds a new label or ends the query: at most k rounds.
 * The host reads the done flags once per round.  W0 = max(32, 4 k) within 64 (k <= 64) or 128, at least k; W1 = max(64, 4 k) within
 * 256 in the first exclusion round and 256 in every further one (a masked scan gets slow with its width: 1 024 candidates cost
 * seven times what 256 do); "group_width0" / "group_width1" of sc_diag_set_option set them (group_width1: every exclusion round; -1 =
 * default; tests).  Results do not depend on either.
 * Without valid labels: SC_ERR_INVALID naming both row counts, nothing launched.  k outside 1 .. 128, Q < 1, a NULL pointer or a
 * short allow give SC_ERR_INVALID before anything changes.  Host pointers; synchronises.
 * Out of scope: more than one hit per group, grouping on the IVF probe paths, sharded collections, labels that survive deletes. */
sc_status sc_index_search_grouped(sc_index* ix, const float* q, int32_t Q, int32_t k, const uint32_t* allow, int64_t allow_words,
                                  float* out_dist, int64_t* out_rows);
/* Same with DEVICE pointers (q row stride = dim; allow_dev may be NULL), enqueued on the runtime's stream.  Synchronises the stream
 * once per round (the done flags) plus whatever the searches underneath wait for; the per-index mutex is held meanwhile.  Results
 * are complete once the stream has passed the call. */
sc_status sc_index_search_grouped_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, const uint32_t* allow_dev,
                                      int64_t allow_words, float* out_dist_dev, int64_t* out_rows_dev);
/* After a grouped search: the width of round 0, the queries that needed further rounds, the exclusion rounds run (summed over those
 * queries; each is one masked search of one query) and the rows read by all scans of the call, per pass. */
sc_status sc_index_last_group_stats(sc_index* ix, int32_t* first_width, int32_t* queries_continued, int32_t* rounds, int64_t* rows_scanned);

/* MMR search: diversified top-k by maximal marginal relevance -- search_type="mmr" with fetch_k and lambda_mult of the LangChain vector
 * stores, which download fetch_k embeddings and run numpy on them.  (The reference has no such call: vendored copies, generated code,
 * license headers and forks are near-identical vectors under different paths and take every one of its rag_max_context_sources,
 * src/semcode/rag/pipeline.py:93-129; grouping by file or repo does not touch them.)  Exact, all three metrics, bit for bit:
 * 1. Candidates c_0 .. c_{C-1}: the exact top-fetch_k of the allowed rows in the order of the keys (better score first, ties by lower
 *    row id) -- what sc_index_search / sc_index_search_masked return at k = fetch_k on an exhaustive scan.  C <= fetch_k is the number of
 *    real hits (smaller when fewer rows are allowed).
 * 2. Oriented score s(a, b): the index metric's score (IP: dot, COSINE: cosine, the canonical fmaf chain and the stored row norms),
 *    negated for L2 so that larger is always better (the negation is exact).  rel_i = s(x_ci, q): the bits the search reported, negated
 *    for L2.  red_ij = s(x_ci, x_cj): the dot in the canonical k order, both norms the stored row norms; red_ij and red_ji are the same bits.
 * 3. Greedy selection: p_0 = 0; for t = 1 .. min(k, C) - 1 and every i not yet picked, m_i = max over the picked j of red_ij (an f32
 *    max: exact) and v_i = fsub(fmul(lambda, rel_i), fmul(mu, m_i)) with mu = fsub(1, lambda) computed once -- three correctly rounded
 *    f32 operations, never a fused multiply-add.  p_t is the i with the largest v_i; ties go to the smallest i.
 * 4. Output in selection order: out_rows[t] = row_base + row(c_pt), out_dist[t] = the bits the exact scan reports for that row (the
 *    distance: not v, not negated), padded with -1 and +inf (L2) / -inf (IP, COSINE) beyond min(k, C).
 * So lambda = 1 gives the first k entries of the plain search, fetch_k = k a permutation of the plain top-k, k = 1 the best hit.
 * allow == NULL (allow_words 0): every row; else the bitset of sc_index_search_masked (allow_words >= ceil(rows / 32)).
 * 1 <= k <= fetch_k <= 128: the fast paths under the exhaustive planner take that width, and a 128 x 128 f32 score matrix is 64 KiB.
 * Always exact and exhaustive, like the masked and the grouped search: no nprobe; a trained IVF_FLAT index is searched as it lies, tail
 * and overwritten rows included, without a refresh or a re-layout.  Nothing about later searches changes.
 * How: the candidate stage is the exhaustive planner (the masked search, with a bitset) at width fetch_k.  On a trained IVF_FLAT index a
 * scatter kernel inverts the position map (4 B read + 4 B written per stored row) into the call's scratch: the candidates are row ids,
 * the corpus is addressed by stored position.  mmr_gram_kernel computes the upper triangle of every query's candidate x candidate
 * matrix in 16 x 16 tiles, one f32 MFMA chain per tile over rows gathered by position, and mirrors it; mmr_select_kernel runs the k - 1
 * greedy steps, one workgroup per query, a butterfly arg-max per wave; no atomics decide anything.  Queries go through in chunks of
 * 1 024 so that the matrices stay within 64 MiB; "mmr_chunk_q" of sc_diag_set_option shrinks the chunk (-1 = default; tests; results
 * do not depend on it).  An empty index or no allowed row: no scan and no matrix kernel is launched, the selection kernel writes the
 * padding alone.
 * k < 1, k > fetch_k, fetch_k > 128, Q < 1, lambda outside [0, 1] or NaN, a NULL pointer or a short allow give SC_ERR_INVALID, naming
 * the value, before anything changes.  Host pointers; synchronises.
 * Out of scope: approximate candidates (nprobe, the IVF probe paths), fetch_k > 128, MMR together with grouping, sharded collections
 * (sc_index_search_sharded*), a similarity for the redundancy term other than the index metric, caching the inverse position map
 * (it would need invalidation hooks throughout the IVF code). */
sc_status sc_index_search_mmr(sc_index* ix, const float* q, int32_t Q, int32_t k, int32_t fetch_k, float lambda, const uint32_t* allow,
                              int64_t allow_words, float* out_dist, int64_t* out_rows);
/* Same with DEVICE pointers (q row stride = dim; allow_dev may be NULL), enqueued on the runtime's stream.  Synchronises only where the
 * searches underneath do (sc_index_search_dev, sc_index_search_masked_dev); the kernels added here need no host read.  The per-index
 * mutex is held meanwhile.  Results are complete once the stream has passed the call. */
sc_status sc_index_search_mmr_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t fetch_k, float lambda,
                                  const uint32_t* allow_dev, int64_t allow_words, float* out_dist_dev, int64_t* out_rows_dev);
/* After an MMR search: its fetch_k, the smallest candidate count C over the queries of the call (a device word read back here:
 * synchronises the stream) and the rows read by the candidate scans of the call, per pass. */
sc_status sc_index_last_mmr_stats(sc_index* ix, int32_t* fetch_k, int32_t* min_candidates, int64_t* rows_scanned);
/* The selection rule (step 3) on the CPU, from the header the kernel compiles (tests on a machine without a GPU): rel [C], G [C rows of
 * ldg >= C floats] = red_ij, picked [min(k, C)] receives candidate indices in selection order.  Nothing else of the search runs. */
sc_status sc_diag_mmr_select_host(const float* rel, const float* G, int32_t C, int32_t ldg, int32_t k, float lambda, int32_t* picked);

/* Hybrid search: a lexical BM25 leg over hashed code terms, on device, fused with the dense leg by weighted reciprocal rank
 * (Milvus: hybrid_search + RRFRanker; the LangChain ensemble retrievers).  Off unless asked for: no other call changes.  The rules
 * live once, in semcode_amd/csrc/lex_rule.h, for the kernels and for the two sc_diag_*_host functions below.
 * Term row: T uint16 slots, T one of 32, 64, 128, 256 and fixed per index by the first install; slots sorted ascending, repeats kept
 * (tf of a term = the length of its run), padded with 0xFFFF; dl = the number of slots that are not padding.
 * sc_lex_terms: the extractor, plain C++ (no runtime, no device).  Text i is bytes[offsets[i] .. offsets[i + 1]) (offsets [n + 1],
 * ascending); out_terms [n][T] receives its term row, out_counts [n] (may be NULL) its dl.  A term run is a maximal run of bytes in
 * [A-Za-z0-9_] or >= 0x80.  It has a split point at every '_' (part of no token) and between a lower-case ASCII letter and an upper-
 * case one that follows it, a letter and a digit, a digit and a letter (bytes >= 0x80 are letters without case).  A run emits itself
 * and then, when it has a split point, every part between split points.  Tokens have their ASCII letters lower-cased, are cut to
 * their first 64 bytes and dropped when shorter than 2 bytes; the hash is 32-bit FNV-1a over the bytes, folded as
 * (h ^ (h >> 16)) & 0xFFFF, with 0xFFFF mapped to 0xFFFE.  The first T tokens in text order are kept, then sorted.  No vocabulary, no
 * stemming: collisions are accepted and deterministic. */
sc_status sc_lex_terms(const uint8_t* bytes, const int64_t* offsets, int64_t n, int32_t T, uint16_t* out_terms, int32_t* out_counts);
/* Term rows are caller data parked on the device in LOCAL ROW-NUMBER order, wherever an IVF layout put the vectors; they are handled
 * as the labels of sc_index_set_groups are: not persisted, not search scratch (sc_index_release_scratch keeps them), dropped by
 * sc_index_delete_rows, valid only while their row count equals the index's.  sc_index_set_terms installs or overwrites rows
 * [first_row, first_row + n) from terms [n][T] (host): first_row must not exceed the term rows already held, first_row + n not the
 * index's rows, and T must be the T of the rows held -- an append costs only its own bytes (the device array grows geometrically,
 * contents kept).  Synchronises.  sc_index_drop_terms removes them and frees the array. */
sc_status sc_index_set_terms(sc_index* ix, int64_t first_row, int64_t n, int32_t T, const uint16_t* terms);
sc_status sc_index_drop_terms(sc_index* ix);
/* rows = the term rows held, sum_dl = the sum of their dl, df [65536] (host; may be NULL): df[t] = the number of rows that hold term
 * t.  A statistics kernel recomputes them only when the term rows changed since the last call (integer atomics: the result does not
 * depend on any order); otherwise the call is a 256 KiB copy.  The library never computes an IDF: the caller turns df into the query
 * weights, which keeps log() out of the parity question.  Term rows not valid: SC_ERR_INVALID naming both counts.  Synchronises. */
sc_status sc_index_lex_stats(sc_index* ix, int64_t* rows, int64_t* sum_dl, uint32_t* df);
/* The lexical search.  Query q has m = nterms[q] <= 32 terms qterms[q * 32 ..] = t_0 < ... < t_{m-1}, STRICTLY ascending and none
 * 0xFFFF, with weights qweights[q * 32 ..] finite and > 0 -- anything else is SC_ERR_INVALID (the _dev form cannot see them
 * before it launches: its kernels treat such a query as one without terms and the call returns SC_ERR_INVALID after its one host read).
 * Score of a row, every step one correctly rounded f32 operation, never fused:
 *   K = k1 * ((1 - b) + (b * (float)dl) / avgdl);  c_j = (w_j * ((float)tf_j * (k1 + 1))) / ((float)tf_j + K);
 *   score = ((0 + c_j0) + c_j1) + ... over the j with tf_j > 0, ascending.  A row with no matching term is never a hit.
 * Larger score first, ties to the lower row; out_rows = row_base + row; padded with -1 and -inf.  1 <= k <= 128.  allow == NULL
 * (allow_words 0): every row; else the bitset of sc_index_search_masked over local row numbers: the bit is tested before a row's
 * slots are read.  Exact and exhaustive on FLAT and IVF_FLAT alike: bit-identical to the rule run on the CPU.
 * How: one pass over the rows * 2 T bytes of term rows serves 16 queries: their terms form a 65 536-bit set in LDS, every slot is
 * one LDS bit test, only rows with a member slot compute tf (integer sums over the row's lanes) and the score; per-wave sorted key lists,
 * sc_topk_merge's tree merge finishes.  Q queries take ceil(Q / 16) passes, in chunks of 1 024 queries ("lex_chunk_q" of
 * sc_diag_set_option shrinks the chunk; -1 = default; results do not depend on it).
 * Term rows not valid: SC_ERR_INVALID naming both counts, nothing launched.  k outside 1 .. 128, Q < 1, k1 / b not finite, avgdl not
 * finite or <= 0, a NULL pointer or a short allow: SC_ERR_INVALID before anything changes.  Host pointers; synchronises. */
sc_status sc_index_search_lexical(sc_index* ix, int32_t Q, int32_t k, const uint16_t* qterms, const float* qweights, const int32_t* nterms, float k1, float b,
                                  float avgdl, const uint32_t* allow, int64_t allow_words, float* out_score, int64_t* out_rows);
/* Same with DEVICE pointers, enqueued on the runtime's stream; synchronises it once at the end (the flag of the query check). */
sc_status sc_index_search_lexical_dev(sc_index* ix, int32_t Q, int32_t k, const uint16_t* qterms_dev, const float* qweights_dev, const int32_t* nterms_dev,
                                      float k1, float b, float avgdl, const uint32_t* allow_dev, int64_t allow_words, float* out_score_dev,
                                      int64_t* out_rows_dev);
/* The hybrid search: q [Q, dim] dense queries plus the lexical arguments above; 1 <= k <= fetch_k <= 128.  The dense leg is the
 * exhaustive planner at width fetch_k (the masked search when a bitset is given; exact, a trained IVF_FLAT index is searched as it
 * lies, as sc_index_search_mmr does); the lexical leg runs at width fetch_k.  Fusion, ranks from 0 in the two best-first lists:
 *   f(row) = wd / (float)(c + rank_dense) + wl / (float)(c + rank_lex), a row missing from one list gets 0 for that term, the dense
 * term is added first; c an int32 >= 1 (60 is customary), wd and wl finite and >= 0.  Output best first by f, ties to the lower row,
 * out_score = f, padded with -1 and -inf.  One fusion kernel, one workgroup per query, no atomics deciding an order.  With wl = 0 and
 * fetch_k = k the rows come in the dense order.  Errors as for the lexical search, plus k > fetch_k, fetch_k > 128, c < 1, a weight
 * negative or not finite.  Host pointers; synchronises.  Out of scope: sharded collections, grouping or MMR on top, approximate (IVF
 * probe) candidates. */
sc_status sc_index_search_hybrid(sc_index* ix, const float* q, int32_t Q, int32_t k, int32_t fetch_k, const uint16_t* qterms, const float* qweights,
                                 const int32_t* nterms, float k1, float b, float avgdl, int32_t c, float wd, float wl, const uint32_t* allow,
                                 int64_t allow_words, float* out_score, int64_t* out_rows);
/* Same with DEVICE pointers; synchronises where the dense searches underneath do and once at the end (the flag of the query check). */
sc_status sc_index_search_hybrid_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t fetch_k, const uint16_t* qterms_dev,
                                     const float* qweights_dev, const int32_t* nterms_dev, float k1, float b, float avgdl, int32_t c, float wd, float wl,
                                     const uint32_t* allow_dev, int64_t allow_words, float* out_score_dev, int64_t* out_rows_dev);
/* After a lexical or hybrid search: term rows a pass streams, their bytes (rows * 2 T) and the passes the call ran (16 queries each). */
sc_status sc_index_last_lex_stats(sc_index* ix, int64_t* rows_scanned, int64_t* bytes_per_pass, int32_t* passes);
/* The two rules on the CPU, from the header the kernels compile (tests on a machine without a GPU).  sc_diag_lex_score_host: terms
 * [n][T] rows, one query of m terms -> out_score [n], out_hit [n] (1: the row holds a query term; else score 0).
 * sc_diag_rrf_host: one query's best-first lists dense_rows / lex_rows [F] (-1 = padding) -> the k best fused hits, padded. */
sc_status sc_diag_lex_score_host(const uint16_t* terms, int64_t n, int32_t T, const uint16_t* qterms, const float* qweights, int32_t m, float k1, float b,
                                 float avgdl, float* out_score, uint8_t* out_hit);
sc_status sc_diag_rrf_host(const int64_t* dense_rows, const int64_t* lex_rows, int32_t F, int32_t k, int32_t c, float wd, float wl, float* out_score,
                           int64_t* out_rows);

/* The token store: late interaction (ColBERT, above) with the documents encoded ONCE, at ingest.  Every row of an index may carry
 * 0 .. 2 048 token vectors of W floats (W a multiple of 16 within 16 .. 128, the rule of maxsim_rule.h), parked on the device next to
 * the rows like the group labels and the term rows -- caller data, not scratch (sc_index_release_scratch keeps it), not persisted by
 * the library -- but keyed by LOCAL ROW NUMBER through a table, wherever an IVF layout put the row's vector.
 *   layout   a pool of token vectors, appended to, and a table (int64 start, int32 len) per row, 16 bytes, on the device with a host
 *            mirror.  fmt 0 stores the f32 bits; fmt 1 stores bf16: every float rounded to nearest-even on its upper 16 bits once, at
 *            install, and widened back exactly when read -- the stored value is one f32 bit pattern (sc_diag_round_bf16 of the input),
 *            every score below is the MaxSim rule on those values, and no bf16 arithmetic happens anywhere.  W and fmt are fixed by
 *            the first install; another W or fmt later is SC_ERR_INVALID (sc_index_drop_tokens first).
 *   dead     a put appends the new vectors and repoints the row; what the row pointed to before is dead.  sc_index_compact_tokens
 *            gathers the live tokens in row order into a fresh pool (one kernel), after which dead = 0; it also runs by itself at the
 *            end of a put or a delete that leaves dead > live (skipped when it cannot allocate).  Results of every call are the same
 *            bits before and after.
 *   rows     rows that never got tokens have none; the table follows the index's row count (rows appended later have none).
 *            sc_index_put_rows / _overwrite / _add leave a row's tokens alone -- replacing them is the caller's second call.
 *            sc_index_delete_rows renumbers the table with the rows: survivors keep their tokens, the deleted rows' become dead
 *            (group labels and term rows are still dropped by a delete).
 * sc_index_put_tokens: rows [n] distinct local row numbers in [0, rows), counts [n] in 0 .. 2 048 (0 removes the row's tokens), vecs
 * [sum counts, W] f32 (host) row after row.  Everything is validated before anything changes; SC_ERR_NOMEM leaves the store as it
 * was.  Synchronises.  sc_index_reserve_tokens pre-sizes the pool (before the first install: remembered until the format is known);
 * otherwise it grows geometrically, contents kept.  sc_index_get_tokens: out_counts [n] and, unless out_vecs is NULL, the rows' vectors
 * one after the other as f32 (widened as stored), at most cap_tokens of them (more: SC_ERR_INVALID, nothing written) -- it serves a
 * save.  sc_index_token_stats: rows that have tokens, live and dead tokens, W and fmt (0, 0: nothing installed), the pool's bytes.
 * sc_index_drop_tokens frees the store.
 * sc_index_put_tokens_dev is sc_index_put_tokens with the vectors on the device: vecs_dev [.., W] f32 (DEVICE), src [sum counts] (host)
 * or NULL.  Stored token j (in stored order: row after row of `rows`) is vecs_dev[src[j]], or vecs_dev[j] without a list -- a gather list
 * of 4 bytes a token, so a caller drops or reorders tokens without moving a vector; its entries must be >= 0 (SC_ERR_INVALID) and name
 * tokens the caller's array holds (not checked: the array's length is the caller's).  late_install_kernel copies (fmt 0) or rounds
 * (fmt 1, the rule above) into pool[used ...) before the table is repointed.  The same checks, the same order of work, the same
 * semantics; synchronises once, at its end.  sc_encoder_embed_tokens_into (above) is the third form: the encoder's token head writes
 * the pool's tail itself. */
sc_status sc_index_put_tokens(sc_index* ix, const int64_t* rows, int64_t n, const int32_t* counts, const float* vecs /*[sum counts,W]*/, int32_t W, int32_t fmt);
sc_status sc_index_put_tokens_dev(sc_index* ix, const int64_t* rows, int64_t n, const int32_t* counts, const float* vecs_dev /*[..,W] f32, device*/,
                                  const int32_t* src /*[sum counts] host, or NULL*/, int32_t W, int32_t fmt);
sc_status sc_index_reserve_tokens(sc_index* ix, int64_t tokens);
sc_status sc_index_compact_tokens(sc_index* ix);
sc_status sc_index_get_tokens(sc_index* ix, const int64_t* rows, int64_t n, int32_t* out_counts, float* out_vecs /*or NULL*/, int64_t cap_tokens);
sc_status sc_index_token_stats(sc_index* ix, int64_t* rows_with_tokens, int64_t* live, int64_t* dead, int32_t* W, int32_t* fmt, int64_t* pool_bytes);
sc_status sc_index_drop_tokens(sc_index* ix);
/* Scoring from the store.  Questions: Q [q_off[Bq], W] f32 token vectors (what sc_encoder_embed_tokens returns for the query side),
 * question q's at rows [q_off[q], q_off[q + 1]), 1 .. 128 of them; 1 <= Bq <= 65 536.  Score of (question, row) =
 * maxsim_score_seq(Q_q, nq, D_row, len_row, NULL, W) of maxsim_rule.h on the stored values: bit-identical to sc_diag_maxsim_host, and at
 * fmt 0 to what sc_encoder_score_late gives for the same texts (a text's token vectors do not depend on its batch-mates).
 * sc_index_rerank_late (late_rerank_kernel, one workgroup per pair, the tile code of maxsim_kernel reading through the table): cand
 * [Bq, C] holds what the searches return, row_base + local row, -1 = padding; 1 <= C <= 1 024; out_scores [Bq, C] in candidate order
 * (the caller sorts); a padding entry or a row without tokens scores -inf.  No passage forward runs.
 * sc_index_search_late (late_scan_kernel): the exact, exhaustive MaxSim top-k over every row that has tokens, 1 <= k <= 128.  allow ==
 * NULL (allow_words 0): every row; else the bitset of sc_index_search_masked over local row numbers, tested before any of a row's
 * tokens is read.  Larger score first under the order of the score key (-0 < +0), ties to the lower row; out_rows = row_base + row;
 * padded with -1 and -inf.  The same on FLAT and trained IVF_FLAT: the store is in row-number order.  How: one launch per question, its
 * token vectors resident in LDS in MFMA fragment order; a wave takes one document at a time in tiles of 16 tokens straight from
 * global memory against every question tile (v_mfma_f32_16x16x4_f32, two chains at a time), one running maximum key per question
 * tile, the ordered sum per document, per-wave sorted key lists, sc_topk_merge's tree merge.  Rows are dealt in fixed blocks of 4, in
 * row order, by one integer work counter (documents differ too much in length for a static split); the counter decides which wave
 * scores a row and nothing else: keys are distinct and the merge exact, so the result is bit-identical to sc_diag_late_search_host
 * whatever the partition.
 * SC_ERR_INVALID before anything changes: no tokens installed, a NULL pointer, Bq / C / k out of range, q_off[0] != 0, a question with 0
 * or more than 128 vectors, a candidate that is neither -1 nor a row, a short allow.  Host pointers; both synchronise.
 * Out of scope: sharded collections, _dev / asynchronous forms of the two scoring calls, several questions per pass, a bf16-MFMA coarse
 * pass with exact re-score.
 * sc_diag_late_search_host is the search on the CPU over D [d_off[n], W] f32 (row r's vectors at [d_off[r], d_off[r + 1]), int64), rows
 * reported without a row_base; sc_diag_round_bf16 the install-time rounding of fmt 1 (out = the value stored for in).  No GPU involved. */
sc_status sc_index_rerank_late(sc_index* ix, const float* Q, const int32_t* q_off /*[Bq+1]*/, int32_t Bq, const int64_t* cand /*[Bq,C]*/, int32_t C,
                               float* out_scores /*[Bq,C]*/);
sc_status sc_index_search_late(sc_index* ix, const float* Q, const int32_t* q_off /*[Bq+1]*/, int32_t Bq, int32_t k, const uint32_t* allow, int64_t allow_words,
                               float* out_score /*[Bq,k]*/, int64_t* out_rows /*[Bq,k]*/);
sc_status sc_diag_late_search_host(const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int64_t* d_off /*[n+1]*/, int64_t n, int32_t W, int32_t k,
                                   const uint32_t* allow, int64_t allow_words, float* out_score, int64_t* out_rows);
sc_status sc_diag_round_bf16(const float* in, int64_t n, float* out);

/* Replaces Collection.create_index(IVF_FLAT, nlist) + load() (milvus_store.py:76-84) for an index created with
 * SC_INDEX_IVF_FLAT: deterministic k-means (niter Lloyd iterations on <= 256*nlist sampled rows), assignment of
 * every row to its nearest centroid, list-major re-ordering of the corpus in HBM.  Until it is called an IVF_FLAT index
 * answers with the exhaustive scan.  After it, searches with Q * nprobe < nlist probe only the nprobe nearest lists
 * (approximate, like the reference); larger batches probe list-major or, where that is estimated to be cheaper, keep using the
 * exhaustive paths, whose results are a superset in quality.
 * Upserts into a trained index (sc_index_add / _overwrite / _put_rows*) KEEP the lists -- Collection.upsert into an indexed
 * collection does not retrain either (milvus_store.py:128): the next search first assigns the new and the replaced rows to the
 * existing centroids and re-orders the corpus once (one pass over it, no k-means; the result is exactly what
 * sc_index_assign_lists builds from scratch for these centroids).  k-means runs again only when this function is called. */
sc_status sc_index_train(sc_index* ix, int32_t niter, uint64_t seed);
/* Persistence of a trained index (the `ivf.*` files of the on-disk collection): the list of every row in insertion order
 * (out [rows] int32), and the inverse -- install centroids [nlist, dim] + that list without running k-means. */
sc_status sc_index_ivf_assignments(sc_index* ix, int32_t* out);
sc_status sc_index_set_ivf(sc_index* ix, const float* centroids, const int32_t* assign, int32_t nlist);
/* Build the lists for given centroids [nlist, dim] without k-means (every row to its nearest centroid).  Multi-GPU IVF_FLAT: one
 * rank trains and broadcasts its centroids, every rank calls this on its shard; the merged probe results then equal those of one
 * index over the whole corpus with these centroids. */
sc_status sc_index_assign_lists(sc_index* ix, const float* centroids, int32_t nlist);
/* nlist actually trained (0 = untrained), centroids [nlist, dim] and list sizes [nlist] (either may be NULL). */
sc_status sc_index_ivf_info(sc_index* ix, int32_t* nlist, float* centroids, int64_t* list_sizes);

/* Search path selection.  mode 0 (default): exact f32 scan for <= 16 queries, MFMA coarse scan (int8, then bf16: see
 * sc_index_set_coarse_stage) + exact f32 re-rank + certificate (uncertified queries re-run exactly) for larger batches with
 * k <= 64 -- both return identical results; 1: exact scan only; 2: batched path whenever supported;
 * 3: per-query IVF probing whenever the index is trained (any batch size; used to measure recall);
 * 4: list-major IVF probing (the probed lists are streamed once per group of queries that want them; same results as 3).
 * In mode 0 a trained IVF_FLAT index probes per query while Q * nprobe < nlist, list-major while that is estimated to be
 * cheaper than the exhaustive paths, and otherwise answers exhaustively (exact results). */
sc_status sc_index_set_search_mode(sc_index* ix, int32_t mode);
/* After a search: which path ran (1 exact, 2 batched, 3 ivf probe per query, 4 ivf probe list-major, 5 list-major behind the int8 coarse
 * stage, 6 masked: sc_index_search_masked* answered without the exhaustive planner, 7 grouped: sc_index_search_grouped*, 8 mmr: sc_index_search_mmr*, 9 lexical: sc_index_search_lexical*, 10 hybrid: sc_index_search_hybrid*) and how many queries the batched path had to
 * re-run through the exact scan because their certificate failed. */
sc_status sc_index_last_search_stats(sc_index* ix, int32_t* path, int32_t* uncertified);

/* Coarse stage of the batched path.  0 (default): the int8 stage first (v_mfma_i32_16x16x64_i8 at twice the bf16 rate on an int8
 * shadow with per-row scales, 512 candidates per query); queries whose certificate fails there go to the bf16 stage (128
 * candidates), and only what fails there too to the exact scan -- results are identical whichever stage answers.  8 / 16 pin the
 * first stage (8: no bf16 stage in between).  An index whose int8 stage could not certify most of a batch starts at the bf16
 * stage from then on (tightly clustered corpora); setting 0 again clears that.  Under 0 the int8 stage is only taken from 2^20
 * rows and 129 queries up (below that its four times larger re-rank, and its 256-query tiles, cost more than the coarse pass
 * saves) or under search mode 2. */
sc_status sc_index_set_coarse_stage(sc_index* ix, int32_t bits);
/* After a batched search: the stage it started on (8 / 16) and how many queries the int8 stage handed to the bf16 stage
 * (sc_index_last_search_stats' `uncertified` counts the queries that ended in the exact scan). */
sc_status sc_index_last_coarse_stats(sc_index* ix, int32_t* first_stage_bits, int32_t* handed_to_bf16);
/* Collect passes of the last batched search: queries whose certificate failed at a stage are given a second pass at the same
 * precision with a fixed threshold (k-th exact score found + the coarse error bound) whose survivors are ALL re-scored exactly;
 * `tried` = such queries (summed over the stages), `resolved` = those it answered (the rest went on to the next stage). */
sc_status sc_index_last_collect_stats(sc_index* ix, int32_t* tried, int32_t* resolved);
/* 1 if the last batched search ran the int8 stage in its wide form: every key within the exact-score cut kept between the phases
 * (up to 4 096 per query) instead of the 512 best -- what the stage switches to on corpora whose certificate fails (clusters). */
sc_status sc_index_last_wide(sc_index* ix, int32_t* wide);
/* Rows the last search scanned exactly BEHIND the lists of a trained IVF_FLAT index: rows appended since the lists were laid out stay
 * there (up to 65 536) instead of forcing a re-layout before the next search -- Milvus' brute-force search of its growing segment;
 * 0 = the lists covered every stored row. */
sc_status sc_index_last_tail_rows(sc_index* ix, int64_t* rows);

/* After an IVF probe search: rows of the DISTINCT lists the batch probed (`unique_rows`: the algorithmic bytes of SURVEY.md 8d
 * config 5 = unique_rows * ld * 4), rows the scan kernel streamed (`streamed_rows`: list-major probing streams a list once per
 * group of <= 16 queries that want it; per-query probing once per query) and the number of (list part, query group) work items. */
sc_status sc_index_last_probe_stats(sc_index* ix, int64_t* unique_rows, int64_t* streamed_rows, int32_t* groups);
/* The host plan of a batched IVF probe, computed without a device (tests): path "listmajor" (the exact list-major probe) or "coarse"
 * (the probe behind the int8 stage) for the probe table probes [Q, nprobe] (list ids; entries outside [0, nlist) are skipped), the
 * list offsets list_off [nlist + 1], top-k k, row stride ld (floats) and cus compute units; wide 0 = no wide groups (as SC_IVF_WIDE=0).
 * The scan parameters are derived exactly as the searches derive them.  out receives the plan's tables as records of
 * {char name[16]; int32 kind (0 int32, 1 int64, 2 uint32, 3 {int64 row0; int32 rows; int32 slot_base}); int32 0; int64 count;
 * count elements, padded to 8 bytes}; *need_bytes is their total size, and nothing is written when cap_bytes is smaller. */
sc_status sc_diag_ivf_plan(const char* path, const int64_t* probes, int32_t Q, int32_t nprobe, const int64_t* list_off, int32_t nlist,
                           int32_t k, int32_t ld, int32_t cus, int32_t wide, void* out, int64_t cap_bytes, int64_t* need_bytes);
/* Which exact probe answers a sub-batch of R queries over rows of stride ld at top-k k and nprobe lists on cus compute units, computed
 * without a device (tests): the queries the int8 coarse stage of an IVF probe could not certify, or a batch whose coarse stage could
 * not run.  *path = 4: list-major probing (R >= 2 and the gather merge holds nprobe k-lists: nprobe * k <= 8192); 3: per-query
 * probing; 0: neither has a plan -- the coarse stage is then not applicable either. */
sc_status sc_diag_ivf_exact_path(int32_t ld, int32_t R, int32_t k, int32_t nprobe, int32_t cus, int32_t* path);
/* The host plan of a packed encoder call, computed without a device or an encoder (tests): the rules of sc_encoder_embed_packed and, by
 * kind, of its siblings on ids / offsets [B + 1] -- kind 0 texts, 1 pairs (first_lens [B]: sc_encoder_score_pairs), 2 sequences of
 * sc_encoder_score_seqs, 3 a token call (expand_id as sc_encoder_embed_tokens; query != 0: the texts are the query side of
 * sc_encoder_score_late, at most 128 tokens each with or without expansion) -- under a model stated by the sc_encoder_cfg fields of the same
 * names, with the messages of those entry points; then every array the call would upload.  out as sc_diag_ivf_plan's, all int32: ids / pos
 * [M], starts / lens [B], items [4 per item], nitems [3], types [M] / ones [B] (kind 1), dst [M] (kind 3), common (the bytes every kind lays
 * out alike, uint32); int64 scalars rows, M (rows rounded up to 256), nrows (token vectors asked for), items_cap, plan_bytes, common_bytes. */
sc_status sc_diag_encoder_plan(const int32_t* ids, const int64_t* offsets, int32_t B, int32_t kind, const int32_t* first_lens, int32_t expand_id,
                               int32_t query, int32_t max_pos, int32_t pos_type, int32_t vocab, int32_t type_vocab, int32_t arch, int32_t global_every,
                               int32_t local_window, void* out, int64_t cap_bytes, int64_t* need_bytes);
/* The same for the documents' token call under keep flags (sc_encoder_embed_tokens_into): keep [offsets[B]] one byte per token or NULL.
 * out: ids / pos / dst [M], starts / lens / counts [B] int32 -- dst is -1 on a dropped token's row, on alignment rows and on the tail, the
 * kept rows count up from 0 text after text; counts the kept tokens per text -- and int64 scalars rows, M, nrows (tokens given), kept. */
sc_status sc_diag_encoder_plan_keep(const int32_t* ids, const int64_t* offsets, int32_t B, const uint8_t* keep, int32_t max_pos, int32_t pos_type, int32_t vocab,
                                    void* out, int64_t cap_bytes, int64_t* need_bytes);

/* Multi-GPU final step (one process per GPU): merge `lists` per-shard results
 * dist [lists,Q,k] / rows [lists,Q,k] (as produced by sc_index_search* on each shard and
 * all-gathered over RCCL) into the global best-first [Q,k], same tie rule.  Host buffers. */
sc_status sc_topk_merge_host(sc_metric metric, int32_t lists, int32_t Q, int32_t k,
                             const float* dist, const int64_t* rows, float* out_dist, int64_t* out_rows);

/* -------------------------------------------------------------- communicator ---- */

/* The path's collectives, RCCL over xGMI, one process per GPU.  Not in the reference (a single Milvus
 * server); this is north_star's multi-GPU scheme: the corpus is sharded by row range, every rank searches the same queries on
 * its shard (sc_index created with row_base = shard start), ONE all-gather moves the per-shard [Q,k] results to every rank,
 * sc_topk_merge_host merges them with the (distance, lower row id) rule.  For IVF_FLAT one rank trains, broadcasts its
 * centroids, and every rank builds its lists for them (sc_index_assign_lists).  librccl is bound at run time on first use.
 * All calls enqueue on the communicator's runtime stream; every rank must make the same calls in the same order. */
typedef struct sc_comm sc_comm;
#define SC_COMM_ID_BYTES 128
/* Rank 0 obtains the rendezvous id (ncclGetUniqueId) and hands the 128 bytes to the other ranks out of band (an environment
 * variable, a file, the launcher's store: control plane, not part of this library). */
sc_status sc_comm_unique_id(void* id_out, size_t nbytes);
/* Collective over all `world` ranks (ncclCommInitRank) on rt's device. */
sc_status sc_comm_create(sc_runtime* rt, int32_t rank, int32_t world, const void* unique_id, size_t nbytes, sc_comm** out);
sc_status sc_comm_destroy(sc_comm* comm);
sc_status sc_comm_info(sc_comm* comm, int32_t* rank, int32_t* world);
/* ncclGetVersion of the RCCL copy this process bound (0 when that copy lacks the entry point). */
sc_status sc_comm_rccl_version(int32_t* version);
/* The search path's one exchange step: dist_dev / rows_dev [Q,k] of this rank (as written by sc_index_search_dev) ->
 * all_dist_dev / all_rows_dev [world,Q,k] on every rank (DEVICE pointers; asynchronous on the runtime's stream; both arrays
 * travel in one grouped RCCL launch). */
sc_status sc_comm_allgather_topk(sc_comm* comm, const float* dist_dev, const int64_t* rows_dev, int32_t Q, int32_t k,
                                 float* all_dist_dev, int64_t* all_rows_dev);
/* The IVF build's one collective: nbytes at DEVICE pointer buf_dev from rank `root` to every rank (asynchronous). */
sc_status sc_comm_broadcast(sc_comm* comm, void* buf_dev, size_t nbytes, int32_t root);
/* Row-sharded search in one call per rank (every rank passes the same queries): this rank's shard is searched as by
 * sc_index_search, the per-shard [Q,k] results are all-gathered and merged on the host; out_dist / out_rows [Q,k] (global row
 * ids) are identical on every rank and equal to the result of one index over the whole corpus.  Host pointers; synchronises. */
sc_status sc_index_search_sharded(sc_index* ix, sc_comm* comm, const float* q, int32_t Q, int32_t k, int32_t nprobe,
                                  float* out_dist, int64_t* out_rows);
/* The same up to the exchange, with DEVICE pointers: q_dev [Q,dim]; all_dist_dev / all_rows_dev [world,Q,k] receive every
 * shard's result (this rank's is written in place into its own slot); enqueued on the runtime's stream like
 * sc_index_search_dev.  The caller merges (sc_topk_merge_host) where it needs the result. */
sc_status sc_index_search_sharded_dev(sc_index* ix, sc_comm* comm, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe,
                                      float* all_dist_dev, int64_t* all_rows_dev);
/* IVF_FLAT over a sharded collection: rank `root` runs sc_index_train on ITS shard, the centroids are broadcast, every other
 * rank builds its lists for them (sc_index_assign_lists).  Probing then means the same lists on every shard. */
sc_status sc_index_train_sharded(sc_index* ix, sc_comm* comm, int32_t niter, int32_t root);
/* max over the ranks of a host double (in place); synchronises, so it also serves as the barrier that brackets a timed
 * region (bench.py). */
sc_status sc_comm_allreduce_max(sc_comm* comm, double* value);

#ifdef __cplusplus
}
#endif
#endif /* SEMCODE_HIP_H */
