// encoder_ops.hip -- the non-GEMM kernels of the transformer-encoder forward (gfx950).
//
// Replaces (reference): what llama.cpp's BERT graph does around the matmuls behind
// LlamaCppEmbeddings.embed_documents / embed_query (src/semcode/embeddings/providers.py:69-100;
// call sites src/semcode/services/indexer.py:150, src/semcode/rag/pipeline.py:171-175):
// token/position/type embedding + LayerNorm, post-attention / post-FFN LayerNorm, masked softmax
// attention, masked mean pooling.  Arithmetic follows BertModel (post-LN, eps inside sqrt, biased
// variance, erf-GELU, additive key mask), restated on CPU in oracle/bert_oracle.py.
//
//   embed_ln_kernel   HBM-bound  : 1 wave / token, f32 tables -> bf16 activations
//   layernorm_kernel  HBM-bound  : 1 wave / token, bf16 -> bf16 (the residual add is fused into the
//                                  producing GEMM's epilogue)
//   attention_kernel  MFMA + LDS : 1 workgroup / (chunk, head of 64 or pair of heads of 32); K and V stay in LDS,
//                                  S^T = K Q^T on v_mfma_f32_32x32x16_bf16 so a lane owns one query
//                                  column, softmax in registers, P feeds P V straight from the
//                                  accumulator registers, V fragments by ds_read_b64_tr_b16.  The math and the head
//                                  widths are attention_core.h's; attention_long_kernel (1 024 / 2 048 tokens) folds
//                                  the keys in segments of 512
//   mean_pool_kernel  HBM-bound  : 1 workgroup / chunk, masked mean (+ optional L2 normalise) -> f32
//   glu_kernel<ACT>   HBM-bound  : gated feed-forward act(gate) * up between the FFN GEMMs (GEGLU: jina-bert-v2, SwiGLU: nomic-bert)
//   rope_qk_kernel    HBM-bound  : rotary position embedding of Q and K, in place on the blocked QKV buffer (nomic-bert)
#include "attention_core.h"  // Head64 / Head32, attn_lds_bytes, attn_launch
#include "encoder_ops.h"
#include "encoder_rows.h"   // the bodies of the embedding, rotary and pooling kernels, wave_sum
#include "gemm_tile.h"  // bf16 helpers, LDS-DMA pointer types

// ------------------------------------------------------------------ embeddings + LayerNorm
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ ids, int tokens, int S, int H, int vocab, int max_pos,
                                                        const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                        const float* __restrict__ temb, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    embed_ln_rows(ids, tokens, PosInRect{S}, H, vocab, max_pos, wemb, pemb, temb, gamma, beta, eps, out);
}

// ------------------------------------------------------------------ LayerNorm-folded batch pipeline (sc_encoder.cpp, gemm_bf16.hip EPI_LNA_* / EPI_RESLN_STATS)
// Embeddings WITHOUT their LayerNorm: the raw sum (bf16) plus the row statistics the consuming GEMM folds in -- slot 0 of
// stats [slots][tokens_pad][2] gets (sum, sum of squares) of the bf16-ROUNDED row, the other slots zero (a GEMM-produced tensor
// fills one slot per 256 columns).
__global__ __launch_bounds__(256) void embed_raw_kernel(const int32_t* __restrict__ ids, int tokens, int tokens_pad, int S, int H, int vocab, int max_pos,
                                                         const float* __restrict__ wemb, const float* __restrict__ pemb,
                                                         const float* __restrict__ temb, bf16_t* __restrict__ out, float* __restrict__ stats, int slots) {
    embed_raw_rows(ids, tokens, tokens_pad, PosInRect{S}, H, vocab, max_pos, wemb, pemb, temb, out, stats, slots);
}

// W' = bf16(W diag(gamma)), c1[n] = sum_k W'[n,k] (of the ROUNDED values: it cancels what the MFMA accumulates),
// c2[n] = bias[n] + sum_k beta[k] W[n,k].  One wave per output row n.
__global__ __launch_bounds__(256) void fold_ln_weights_kernel(const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ bias, int N, int K, bf16_t* __restrict__ Wf,
                                                               float* __restrict__ c1, float* __restrict__ c2) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float s1 = 0.f, s2 = 0.f;
    for (int k0 = 4 * lane; k0 < K; k0 += 256) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k0);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + k0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(beta + k0);
        u16x4 r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            r[c] = f32_to_bf16(w[c] * g[c]);
            s1 += bf16_to_f32(r[c]);
            s2 = fmaf(b[c], w[c], s2);
        }
        *reinterpret_cast<u16x4*>(Wf + (size_t)n * K + k0) = r;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        c1[n] = s1;
        c2[n] = (bias ? bias[n] : 0.f) + s2;
    }
}
__global__ __launch_bounds__(256) void add_vectors_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// masked mean pooling of LayerNorm(y) computed on the fly from the raw rows and their partial statistics:
// mean_t LN(y_t) = gamma * (sum_t rs_t y_t - sum_t rs_t mu_t) / len + beta.  One workgroup per (chunk, 256 columns).
__global__ __launch_bounds__(256) void mean_pool_ln_kernel(const bf16_t* __restrict__ y, const float* __restrict__ stats, int slots, int tokens_pad,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            const int32_t* __restrict__ lens, int S, int H, float* __restrict__ out) {
    mean_pool_ln_rows(y, stats, slots, tokens_pad, gamma, beta, eps, RectRows{lens, S}, blockIdx.y, blockIdx.x, H, out);
}

// ------------------------------------------------------------------ LayerNorm (input already holds x + sublayer(x))
// HBM-bound (2 x tokens x H x 2 B).  Half a wave per token: lane l of the half owns the 16-byte chunks l, l + 32, ... of
// the row (8 bf16 each; H = 768 -> 3 per lane), so one load instruction moves 2 x 512 B.  Workgroups walk the rows with
// a grid stride and keep the NEXT row's loads in flight while the current one is reduced (two dependent half-wave
// reductions: mean, then the centred sum of squares, as BertModel computes it), gamma / beta stay in registers.
// The first version (one wave per row, 8-byte loads, one row per wave) ran at 3.65 TB/s.
template <int NC>
__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* __restrict__ in, int tokens, int H, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int l32 = threadIdx.x & 31, half = (threadIdx.x >> 5) & 1;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    f32x4 g[NC][2], b[NC][2];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int k0 = (l32 + 32 * j) * 8;
        if (k0 < H) {
            g[j][0] = *reinterpret_cast<const f32x4*>(gamma + k0);
            g[j][1] = *reinterpret_cast<const f32x4*>(gamma + k0 + 4);
            b[j][0] = *reinterpret_cast<const f32x4*>(beta + k0);
            b[j][1] = *reinterpret_cast<const f32x4*>(beta + k0 + 4);
        }
    }
    const float inv_h = 1.0f / (float)H;
    u32x4 nxt[NC];
    int tok = wave * 2 + half;
    if (tok < tokens) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int k0 = (l32 + 32 * j) * 8;
            if (k0 < H) nxt[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + (size_t)tok * H + k0));
        }
    }
    for (int base = wave * 2; base < tokens; base += nwaves * 2) {
        tok = base + half;
        const bool live = tok < tokens;
        u32x4 raw[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) raw[j] = nxt[j];
        const int ntok = tok + nwaves * 2;
        if (ntok < tokens) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int k0 = (l32 + 32 * j) * 8;
                if (k0 < H) nxt[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + (size_t)ntok * H + k0));
            }
        }
        float v[NC][8];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const bool on = live && (l32 + 32 * j) * 8 < H;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                v[j][2 * c] = on ? __builtin_bit_cast(float, raw[j][c] << 16) : 0.f;
                v[j][2 * c + 1] = on ? __builtin_bit_cast(float, raw[j][c] & 0xFFFF0000u) : 0.f;
            }
            sum += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float mean = sum * inv_h;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const bool on = (l32 + 32 * j) * 8 < H;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float d = on ? v[j][c] - mean : 0.f;
                sq = fmaf(d, d, sq);
            }
        }
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) sq += __shfl_xor(sq, off, 64);
        const float rstd = 1.0f / sqrtf(sq * inv_h + eps);
        if (live) {
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int k0 = (l32 + 32 * j) * 8;
                if (k0 < H) {
                    u32x4 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float lo = (v[j][2 * c] - mean) * rstd * g[j][c >> 1][(2 * c) & 3] + b[j][c >> 1][(2 * c) & 3];
                        const float hi = (v[j][2 * c + 1] - mean) * rstd * g[j][c >> 1][(2 * c + 1) & 3] + b[j][c >> 1][(2 * c + 1) & 3];
                        r[c] = pack_bf16x2(lo, hi);
                    }
                    *reinterpret_cast<u32x4*>(out + (size_t)tok * H + k0) = r;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ attention
// qkv: [tokens, 3H] bf16 rows = [Q | K | V], head h at columns h*64 of each third.  ctx: [tokens, H].
// KT = S / 32 key tiles.  LDS: K image [S][64] with chunk ^= (row>>1)&7, V image [S][64] with
// chunk ^= ((row>>1)&1)<<2 (conflict-free for ds_read_b128 rows / ds_read_b64_tr_b16 blocks).
// One 32-row query block of one wave, keys processed in groups of 4 tiles (128 keys) with an online softmax, so
// that only 64 score registers are live (S = 256 runs 2 workgroups per CU, S = 512 no longer spills).
// FULL = every key of the padded sequence is real (len == S): no per-tile guards or masks.
// HEAD (attention_core.h): Head64<ALIBI> -- one head of 64 per 64-column block; ALIBI: scores get the symmetric linear bias
// -slope_head * |query - key| (jina-bert-v2 style encoders, no position table) -- or Head32, a pair of heads of 32 per block.
// State, fold and store stay inside each FULL arm: declared around the branch, the compiler merges the two store tails and the
// kernels come out with other register counts.
// The shell around the math (LDS carve-up, operand addressing, staging loops, Q load) is written out in every attention kernel
// (here, encoder_packed.hip, encoder_window.hip).  As shared functions -- tried: carve-up, operand, staging, Q load, one segmented
// body under attention_long_kernel and attention_packed_kernel -- each alone changes the compiler's text of these kernels (registers
// at 1 - 4 key tiles, scratch at S = 512, block order), and the 8-tile packed class measured 1.6 - 1.9 % slower per launch through
// them.  Written out, every Head64 instantiation is the instruction text it was before the head width became a policy
// (profiles/attention_shell_kernels.log).
template <class HEAD, int KT, bool FULL, int GKMAX>
static __device__ __forceinline__ void attention_qblock(const bf16x8 (&qf)[4], const char* Kl, const char* Vl, float* xch, char* ostg,
                                                        bf16_t* obase, int H, int len, int nkt, int lane, int qbase, float slope2) {
    typename HEAD::State st;
    HEAD::init(st);
    HEAD::template fold<KT, FULL, GKMAX>(qf, Kl, Vl, xch, len, nkt, lane, qbase, slope2, st, true, 0);
    HEAD::store(st, xch, ostg, obase, H, lane);
}

// One workgroup per (chunk, 64-column block), NW waves (4, or 8 from S = 256 on; at S = 256 one query block per wave and two key-tile
// groups of 2 -> half the registers, so that 4 waves instead of 2 share a SIMD and cover each other's MFMA -> softmax -> MFMA
// dependency stalls)
template <class HEAD, int KT, int NW>
__global__ __launch_bounds__(NW * 64, (KT <= 8 ? 2 : 1)) void attention_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int H,
                                                            typename HEAD::Extra extra, bf16_t* __restrict__ ctx, int blocked) {
    constexpr int S = KT * 32;
    constexpr int NQB = (KT + NW - 1) / NW;  // query blocks per wave
    constexpr int GKMAX = (NW == 8 && KT <= 8) ? 2 : 4;  // S = 512 runs one workgroup per CU anyway (LDS): registers are not its limit
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + S * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * S * 128) + w * 32;  // [NW waves][32] alpha / 1/l exchange
    char* ostg = smem + 2 * S * 128 + NW * 128 + w * 1024;               // per-wave [8 q][64 d] bf16 output staging
    const int head = blockIdx.x, b = blockIdx.y;
    // row-major QKV [tokens][3H] (Q | K | V, block j at column 64 j), or -- blocked -- [3H/64][tokens][64] as the QKV projection writes it
    // (gemm_bf16.hip c_index; `blocked` = tokens padded to that GEMM's M, 0 = row-major): every operand of this (chunk, block) is then one contiguous [S][64] block
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nh = (size_t)(H >> 6);  // blocked = the row count (M) of the projection that wrote the blocks
    const bf16_t* base = blocked ? qkv + ((size_t)head * T + (size_t)b * S) * 64 : qkv + (size_t)b * S * ld + head * 64;
    const size_t koff = blocked ? nh * T * 64 : (size_t)H, voff = 2 * koff;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    const int nkt = (len + 31) >> 5;  // key tiles holding at least one real key; later tiles are skipped entirely

    // ---- stage K then V rows [0, 32 nkt) of this (chunk, block): pieces of 8 rows x 128 B = 1 KiB
    for (int piece = w; piece < nkt * 4; piece += NW) {
        const int p = piece * 64 + lane;
        const int r = p >> 3, ck = (p & 7) ^ ((r >> 1) & 7);
        __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)r * ld + koff + ck * 8), (lds_vptr)(Kl + piece * 1024), 16, 0, 0);
    }
    for (int piece = w; piece < nkt * 4; piece += NW) {
        const int p = piece * 64 + lane;
        const int r = p >> 3, cv = (p & 7) ^ (((r >> 1) & 1) << 2);
        __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)r * ld + voff + cv * 8), (lds_vptr)(Vl + piece * 1024), 16, 0, 0);
    }
    // Q fragments of all of this wave's query blocks (B operand: lane (q = lane&31, hh) holds Q[q][16 ks + 8 hh .. +7]),
    // requested now so that their latency hides behind the K/V staging
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[NQB][4];
#pragma unroll
    for (int i = 0; i < NQB; ++i) {
        const int qb = w + NW * i;
        if (qb < KT) {
            const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qf[i][ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

#pragma unroll
    for (int i = 0; i < NQB; ++i) {
        const int qb = w + NW * i;
        if (qb < KT) {
            bf16_t* obase = ctx + (size_t)(b * S + qb * 32) * H + head * 64;
            const float slope2 = HEAD::slope2(extra, head);
            if (nkt == KT && (len & 31) == 0) attention_qblock<HEAD, KT, true, GKMAX>(qf[i], Kl, Vl, xch, ostg, obase, H, len, nkt, lane, qb * 32, slope2);
            else attention_qblock<HEAD, KT, false, GKMAX>(qf[i], Kl, Vl, xch, ostg, obase, H, len, nkt, lane, qb * 32, slope2);
        }
    }
}

// ---- sequences of 1 024 and 2 048 tokens (the reference's default chunker emits up to 200 lines / 6 000 characters per chunk --
// src/semcode/chunking/tree_sitter_chunker.py:64-65 -- i.e. 1.5-2k word pieces; jina-embeddings-v2 is an 8k-context ALiBi
// model).  K and V of 512 keys fill the LDS (128 KiB), so the keys are attended in SEGMENTS of 512: stage a segment, every wave
// folds it into the online-softmax state of its ONE 32-row query block (AttnState, 34 registers), next segment.  A workgroup takes 8 query blocks (256 queries) of one (chunk, block); the S / 256 workgroups of a
// (chunk, block) each stage all its keys (from L2 after the first).  Same arithmetic per (query, key) as attention_kernel: a
// sequence of <= 512 real tokens padded to 1 024 gives the bits the S = 512 kernel gives.
template <class HEAD>
__global__ __launch_bounds__(512, 1) void attention_long_kernel(const bf16_t* __restrict__ qkv, const int32_t* __restrict__ lens, int S, int H,
                                                                typename HEAD::Extra extra, bf16_t* __restrict__ ctx, int blocked) {
    constexpr int KT = 16, NW = 8, SEG = 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kl = smem;
    char* Vl = smem + SEG * 128;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* xch = reinterpret_cast<float*>(smem + 2 * SEG * 128) + w * 32;
    char* ostg = smem + 2 * SEG * 128 + NW * 128 + w * 1024;
    const int head = blockIdx.x, b = blockIdx.y, qb = (int)blockIdx.z * NW + w;  // this wave's 32-row query block
    const int ld = blocked ? 64 : 3 * H;
    const size_t T = (size_t)blocked, nh = (size_t)(H >> 6);
    const bf16_t* base = blocked ? qkv + ((size_t)head * T + (size_t)b * S) * 64 : qkv + (size_t)b * S * ld + head * 64;
    const size_t koff = blocked ? nh * T * 64 : (size_t)H, voff = 2 * koff;
    int len = lens[b];
    len = len < 1 ? 1 : (len > S ? S : len);
    len = __builtin_amdgcn_readfirstlane(len);
    const int l31 = lane & 31, hh = lane >> 5;
    bf16x8 qf[4];
    {
        const bf16_t* qrow = base + (size_t)(qb * 32 + l31) * ld;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + 16 * ks + 8 * hh);
    }
    typename HEAD::State st;
    HEAD::init(st);
    const float slope2 = HEAD::slope2(extra, head);
    const int nseg = (len + SEG - 1) / SEG;
#pragma unroll 1
    for (int seg = 0; seg < nseg; ++seg) {
        const int key0 = seg * SEG;
        const int slen = len - key0 < SEG ? len - key0 : SEG;  // real keys in this segment
        const int nkt = (slen + 31) >> 5;
        if (seg) __syncthreads();  // every wave is done with the previous segment's K / V
        for (int piece = w; piece < nkt * 4; piece += NW) {
            const int p = piece * 64 + lane;
            const int r = p >> 3, ck = (p & 7) ^ ((r >> 1) & 7);
            __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)(key0 + r) * ld + koff + ck * 8), (lds_vptr)(Kl + piece * 1024), 16, 0, 0);
        }
        for (int piece = w; piece < nkt * 4; piece += NW) {
            const int p = piece * 64 + lane;
            const int r = p >> 3, cv = (p & 7) ^ (((r >> 1) & 1) << 2);
            __builtin_amdgcn_global_load_lds((gbl_vptr)(base + (size_t)(key0 + r) * ld + voff + cv * 8), (lds_vptr)(Vl + piece * 1024), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (nkt == KT && (slen & 31) == 0) HEAD::template fold<KT, true, 4>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
        else HEAD::template fold<KT, false, 4>(qf, Kl, Vl, xch, slen, nkt, lane, qb * 32, slope2, st, seg == 0, key0);
    }
    HEAD::store(st, xch, ostg, ctx + (size_t)(b * S + qb * 32) * H + head * 64, H, lane);
}

// ------------------------------------------------------------------ masked mean pooling
__global__ __launch_bounds__(256) void mean_pool_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ lens, int S, int H,
                                                         int normalize, float* __restrict__ out) {
    mean_pool_rows(x, RectRows{lens, S}, blockIdx.x, H, normalize, out);
}

// ------------------------------------------------------------------ f32 -> bf16 weight conversion, fills
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = f32_to_bf16(in[i]);
}
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const bf16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = bf16_to_f32(in[i]);
}
__global__ __launch_bounds__(256) void synth_scaled_kernel(float* __restrict__ out, int64_t n, uint64_t key, float scale, float offset) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = offset + scale * sc_synth_value(key, (uint64_t)i, 0u, 1u);
}

// ------------------------------------------------------------------ launchers
void sc_launch_embed_ln(const int32_t* ids, int tokens, int S, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                        const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    hipLaunchKernelGGL(embed_ln_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, s, ids, tokens, S, H, vocab, max_pos, wemb, pemb, temb,
                       g, b, eps, (bf16_t*)out);
}
void sc_launch_layernorm(const void* in, int tokens, int H, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    int blocks = (tokens + 7) / 8;  // 8 rows per workgroup per sweep
    if (blocks > 256 * 8) blocks = 256 * 8;
    const dim3 grid((unsigned)blocks), block(256);
    if (H <= 768) hipLaunchKernelGGL(layernorm_kernel<3>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, b, eps, (bf16_t*)out);
    else if (H <= 1024) hipLaunchKernelGGL(layernorm_kernel<4>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, b, eps, (bf16_t*)out);
    else hipLaunchKernelGGL(layernorm_kernel<8>, grid, block, 0, s, (const bf16_t*)in, tokens, H, g, b, eps, (bf16_t*)out);
}
bool sc_attention_supported(int S, int H, int heads, int head_dim) {
    return heads > 0 && (head_dim == 64 || head_dim == 32) && H == heads * head_dim && H % 64 == 0 && (S == 32 || S == 64 || S == 128 || S == 256 || S == 512 || S == 1024 || S == 2048);
}
template <class HEAD, int KT>
static void launch_attn(const void* qkv, const int32_t* lens, int B, int H, typename HEAD::Extra extra, void* ctx, int blocked, hipStream_t s) {
    constexpr int NW = KT >= 8 ? 8 : 4;
    attn_launch<attention_kernel<HEAD, KT, NW>, attn_lds_bytes(KT, NW)>(dim3((unsigned)(H / 64), (unsigned)B), NW * 64, s, (const bf16_t*)qkv, lens, H, extra,
                                                                         (bf16_t*)ctx, blocked);
}
template <class HEAD>
static void launch_attention(const void* qkv, const int32_t* lens, int B, int S, int H, typename HEAD::Extra extra, void* ctx, int blocked, hipStream_t s) {
    if (S > 512) {  // K / V streamed through the LDS in segments of 512 keys
        attn_launch<attention_long_kernel<HEAD>, attn_lds_bytes(16, 8)>(dim3((unsigned)(H / 64), (unsigned)B, (unsigned)(S / 256)), 512, s, (const bf16_t*)qkv, lens, S,
                                                                         H, extra, (bf16_t*)ctx, blocked);
        return;
    }
    switch (S) {
        case 32: launch_attn<HEAD, 1>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 64: launch_attn<HEAD, 2>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 128: launch_attn<HEAD, 4>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 256: launch_attn<HEAD, 8>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        case 512: launch_attn<HEAD, 16>(qkv, lens, B, H, extra, ctx, blocked, s); break;
        default: break;
    }
}
// slopes: NULL = plain attention; else [heads] ALiBi slopes (device).  head_dim 32: plain only, create refuses 32-wide ALiBi models
void sc_launch_attention(const void* qkv, const int32_t* lens, int B, int S, int H, const float* slopes, void* ctx, hipStream_t s, int blocked, int head_dim) {
    if (head_dim == 32) launch_attention<Head32>(qkv, lens, B, S, H, Head32::Extra(), ctx, blocked, s);
    else if (slopes) launch_attention<Head64<true>>(qkv, lens, B, S, H, slopes, ctx, blocked, s);
    else launch_attention<Head64<false>>(qkv, lens, B, S, H, nullptr, ctx, blocked, s);
}
// Gated feed-forward: out[m][j] = act(h[m][j]) * h[m][F + j], h = [tokens, 2F] bf16 -> out [tokens, F] bf16.
// GEGLU (jina-bert-v2 GLUMLP): act = erf-GELU.  SwiGLU (nomic-bert): act = silu(g) = g / (1 + exp(-g)) on the hardware exp2 / rcp
// (v_exp_f32, v_rcp_f32: 1 ulp each, in front of a bf16 rounding); exp(-g) overflows to +inf for g < -88.7 and g * rcp(inf) is a
// signed zero -- the limit of silu there -- never NaN.
struct ActGelu {
    static __device__ __forceinline__ f32x2 apply(f32x2 g) { return gelu_erf_fast2(g); }
};
struct ActSilu {
    static __device__ __forceinline__ float one(float g) {
        return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.44269504088896340736f));
    }
    static __device__ __forceinline__ f32x2 apply(f32x2 g) { return f32x2{one(g[0]), one(g[1])}; }
};
template <class ACT>
__global__ __launch_bounds__(256) void glu_kernel(const bf16_t* __restrict__ h, int64_t tokens, int F, bf16_t* __restrict__ out) {
    const int64_t total = tokens * (int64_t)(F / 8);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / (F / 8);
        const int j = (int)(i - m * (F / 8)) * 8;
        const bf16x8 g = *reinterpret_cast<const bf16x8*>(h + m * 2 * F + j);
        const bf16x8 u = *reinterpret_cast<const bf16x8*>(h + m * 2 * F + F + j);
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x2 gg = ACT::apply(f32x2{bf16_to_f32((bf16_t)g[2 * c]), bf16_to_f32((bf16_t)g[2 * c + 1])});
            o[c] = pack_bf16x2(gg[0] * bf16_to_f32((bf16_t)u[2 * c]), gg[1] * bf16_to_f32((bf16_t)u[2 * c + 1]));
        }
        *reinterpret_cast<u32x4*>(out + m * F + j) = o;
    }
}
void sc_launch_geglu(const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    int64_t blocks = (tokens * (F / 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(glu_kernel<ActGelu>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)h, tokens, F, (bf16_t*)out);
}
void sc_launch_swiglu(const void* h, int64_t tokens, int F, void* out, hipStream_t s) {
    int64_t blocks = (tokens * (F / 8) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(glu_kernel<ActSilu>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)h, tokens, F, (bf16_t*)out);
}

// Rotary position embedding ("rotate-half", GPT-NeoX) of Q and K in place on the blocked QKV buffer [blocks][M][64] bf16 the QKV
// projections write: a (head, token) vector is 128 contiguous bytes.  HBM-bound (read + write of 2/3 of QKV).  A lane owns columns
// c .. c + 7 and c + 32 .. c + 39 of one row (two 16-byte loads), so both members of every rotated pair (j, j + 32) sit in its
// registers; 4 lanes per row, 16 rows per wave.  cos / sin [>= S][32] f32 (sc_encoder_create); position = row & (S - 1), S a power
// of two, so that padding rows (>= the real tokens, content irrelevant) stay inside the table.  f32 math, one rounding back to bf16.
__global__ __launch_bounds__(256) void rope_qk_kernel(bf16_t* __restrict__ qkv, int64_t M, int nblocks, int smask, const float* __restrict__ cos_t,
                                                       const float* __restrict__ sin_t) {
    rope_qk_rows(qkv, M, nblocks, PosMasked{smask}, cos_t, sin_t);
}
void sc_launch_rope_qk(void* qkv, int64_t M, int nblocks, int S, const float* cos_t, const float* sin_t, hipStream_t s) {
    int64_t blocks = ((int64_t)nblocks * M * 4 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(rope_qk_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (bf16_t*)qkv, M, nblocks, S - 1, cos_t, sin_t);
}
// Unnormalised pooling with more parallelism than one workgroup per chunk (which ran at 1.3 TB/s): a workgroup owns 256
// columns of one chunk, thread (cc, rg) sums the rows rg, rg + 8, ... of 8 columns with 16-byte loads, LDS combines the 8 row groups
// in a fixed order.
__global__ __launch_bounds__(256) void mean_pool_sliced_kernel(const bf16_t* __restrict__ x, const int32_t* __restrict__ lens, int S, int H,
                                                                float* __restrict__ out) {
    mean_pool_sliced_rows(x, RectRows{lens, S}, blockIdx.y, blockIdx.x, H, out);
}

void sc_launch_mean_pool(const void* x, const int32_t* lens, int B, int S, int H, int normalize, float* out, hipStream_t s) {
    if (!normalize && (H % 8) == 0)
        hipLaunchKernelGGL(mean_pool_sliced_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)B), dim3(256), 0, s, (const bf16_t*)x, lens, S, H, out);
    else
        hipLaunchKernelGGL(mean_pool_kernel, dim3((unsigned)B), dim3(256), 0, s, (const bf16_t*)x, lens, S, H, normalize, out);
}
void sc_launch_embed_raw(const int32_t* ids, int tokens, int tokens_pad, int S, int H, int vocab, int max_pos, const float* wemb, const float* pemb,
                         const float* temb, void* out, float* stats, int slots, hipStream_t s) {
    hipLaunchKernelGGL(embed_raw_kernel, dim3((unsigned)((tokens_pad + 3) / 4)), dim3(256), 0, s, ids, tokens, tokens_pad, S, H, vocab, max_pos, wemb, pemb, temb,
                       (bf16_t*)out, stats, slots);
}
void sc_launch_fold_ln_weights(const float* W, const float* gamma, const float* beta, const float* bias, int N, int K, void* Wf, float* c1, float* c2,
                               hipStream_t s) {
    hipLaunchKernelGGL(fold_ln_weights_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, W, gamma, beta, bias, N, K, (bf16_t*)Wf, c1, c2);
}
void sc_launch_add_vectors(const float* a, const float* b, float* out, int n, hipStream_t s) {
    hipLaunchKernelGGL(add_vectors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, out, n);
}
void sc_launch_mean_pool_ln(const void* y, const float* stats, int slots, int tokens_pad, const float* gamma, const float* beta, float eps,
                            const int32_t* lens, int B, int S, int H, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mean_pool_ln_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)B), dim3(256), 0, s, (const bf16_t*)y, stats, slots, tokens_pad, gamma,
                       beta, eps, lens, S, H, out);
}
void sc_launch_f32_to_bf16(const float* in, void* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, (bf16_t*)out, n);
}
void sc_launch_bf16_to_f32(const void* in, float* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)in, out, n);
}
void sc_launch_synth_scaled(float* out, int64_t n, uint64_t seed, float scale, float offset, hipStream_t s) {
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(synth_scaled_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, n, sc_synth_key(seed), scale, offset);
}
