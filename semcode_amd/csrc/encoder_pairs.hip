// encoder_pairs.hip -- what a cross-encoder (reranker) needs on top of the packed encoder forward (gfx950).
//
// A reranker reads a question and a passage TOGETHER: one packed sequence [CLS] question [SEP] passage [SEP] whose first part carries
// segment id 0 and whose second part segment id 1, and scores the pair from the last hidden state of its [CLS] row.  The forward
// itself is encoder_packed.hip's; two things are new here:
//
//   embed_*_pairs_kernel   encoder_rows.h's embedding bodies with a per-row type_emb row (TypeArray) next to the per-row position.
//                          Statistics conventions of embed_raw_packed_kernel; alignment rows and the tail carry type 0 (the host
//                          plans them so), the tail rows are zero rows with statistics (0, 0).
//   pair_head_kernel       cls [B, H] f32 -> p = tanh(Wp cls + bp) (or p = cls without a pooler) -> logits = Wc p + bc, num_labels 1 or 2.
//
// Taking the [CLS] row needs no kernel: the packed pooling kernels, given a length of one for every sequence, return row starts[b].
//
// pair_head_kernel: one workgroup (4 waves) per 16 pairs.  Their CLS rows lie in the LDS as [16][H + 4] f32 (the 4 floats of padding
// move consecutive rows one 16-byte slot apart: for H a multiple of 64 -- every encoder shape tested -- two of the 16 lanes
// ds_read_b128 serves per cycle share a slot, against all 16 on unpadded rows; other H give another residue, not worked out).  Wave w computes the pooler outputs n of the 16-row tiles w, w + 4, ... of Wp as
// D[n][pair] = sum_k Wp[n][k] cls[pair][k] with v_mfma_f32_16x16x4_f32 (A = Wp: lane holds A[l & 15][k = l >> 4]; B = cls^T: lane holds
// B[k = l >> 4][l & 15]): a lane loads the four consecutive k of ITS k group as one 16-byte piece of a Wp row (global) and of a CLS row
// (LDS), so the MFMA of step c multiplies k = kk + 4 (l >> 4) + c on both sides -- every k of a 16-wide stage is taken once.  Wp is
// read once per workgroup, straight into registers: nothing of it is reused inside the workgroup.  Even and odd stages accumulate
// into two chains (a dependent f32 MFMA waits 40 cycles, an independent one issues after 32) that are added at the end.  A lane
// then holds D[4 (l >> 4) + c][l & 15]: it adds the bias, takes tanh and multiplies by its rows of Wc; the partial logits of the 16
// lane groups of a workgroup are added in a fixed order through the LDS.  No atomics, every order fixed: two runs give the same bits.
// Cost at H = 768: 2 x 16 x 768 x 768 flop per workgroup on the f32 MFMA pipe and 2.4 MB of Wp from the L2 -- about 0.3 ms per 40 960
// pairs next to the 12 layers in front of it.
#include "encoder_ops.h"
#include "encoder_rows.h"
#include "gemm_tile.h"

__global__ __launch_bounds__(256) void embed_ln_pairs_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos, const int32_t* __restrict__ types,
                                                              int tokens, int H, int vocab, int max_pos, int type_vocab, const float* __restrict__ wemb,
                                                              const float* __restrict__ pemb, const float* __restrict__ temb, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, bf16_t* __restrict__ out) {
    embed_ln_rows(ids, tokens, PosArray{pos, max_pos}, H, vocab, max_pos, wemb, pemb, temb, gamma, beta, eps, out, TypeArray{types, type_vocab});
}
__global__ __launch_bounds__(256) void embed_raw_pairs_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ pos, const int32_t* __restrict__ types,
                                                               int tokens, int tokens_pad, int H, int vocab, int max_pos, int type_vocab,
                                                               const float* __restrict__ wemb, const float* __restrict__ pemb, const float* __restrict__ temb,
                                                               bf16_t* __restrict__ out, float* __restrict__ stats, int slots) {
    embed_raw_rows(ids, tokens, tokens_pad, PosArray{pos, max_pos}, H, vocab, max_pos, wemb, pemb, temb, out, stats, slots, TypeArray{types, type_vocab});
}

// tanh of any finite or infinite x: the argument is clamped to +-20 first (tanh(20) rounds to 1 in f32), so no exponential overflows
// and the result saturates to exactly +-1
static __device__ __forceinline__ float tanh_sat(float x) { return tanhf(fminf(fmaxf(x, -20.f), 20.f)); }

#define PAIR_HEAD_PAD 4  // floats between two CLS rows in the LDS
__global__ __launch_bounds__(256) void pair_head_kernel(const float* __restrict__ cls, int B, int H, const float* __restrict__ Wp, const float* __restrict__ bp,
                                                         const float* __restrict__ Wc, const float* __restrict__ bc, int num_labels,
                                                         float* __restrict__ logits) {
    extern __shared__ __attribute__((aligned(16))) float rows[];  // [16][H + PAIR_HEAD_PAD]
    __shared__ float part[4][4][2][16];                           // [wave][k group][label][pair]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int ld = H + PAIR_HEAD_PAD, h4 = H >> 2;
    for (int i = tid; i < 16 * h4; i += 256) {
        const int r = i / h4, c4 = i - r * h4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};  // pairs beyond B: zero rows, computed and never stored
        if (b0 + r < B) v = *reinterpret_cast<const f32x4*>(cls + (size_t)(b0 + r) * H + 4 * c4);
        *reinterpret_cast<f32x4*>(rows + r * ld + 4 * c4) = v;
    }
    __syncthreads();

    const float* xrow = rows + r16 * ld + 4 * g;
    float lg[2] = {0.f, 0.f};
    const int stages = H >> 4;
    for (int n0 = 16 * w; n0 < H; n0 += 64) {  // wave-uniform
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        if (Wp) {
            const float* wrow = Wp + (size_t)(n0 + r16) * H + 4 * g;
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            auto stage = [&](int st, f32x4& acc) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(wrow + 16 * st);
                const f32x4 x = *reinterpret_cast<const f32x4*>(xrow + 16 * st);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], x[c], acc, 0, 0, 0);
            };
            for (int st = 0; st + 1 < stages; st += 2) {
                stage(st, acc0);
                stage(st + 1, acc1);
            }
            if (stages & 1) stage(stages - 1, acc0);
            d = acc0 + acc1;
        }
        // lane holds pooler output n = n0 + 4 g + c of pair r16
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = n0 + 4 * g + c;
            const float p = Wp ? tanh_sat(d[c] + bp[n]) : rows[r16 * ld + n];
            lg[0] = fmaf(Wc[n], p, lg[0]);
            if (num_labels > 1) lg[1] = fmaf(Wc[H + n], p, lg[1]);
        }
    }
    part[w][g][0][r16] = lg[0];
    part[w][g][1][r16] = lg[1];
    __syncthreads();
    if (tid < 16 * num_labels) {
        const int b = tid & 15, c = tid >> 4;
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) s += part[ww][gg][c][b];
        if (b0 + b < B) logits[(size_t)(b0 + b) * num_labels + c] = s + bc[c];
    }
}

// ------------------------------------------------------------------ launchers
void sc_launch_embed_ln_pairs(const int32_t* ids, const int32_t* pos, const int32_t* types, int tokens, int H, int vocab, int max_pos, int type_vocab,
                              const float* wemb, const float* pemb, const float* temb, const float* g, const float* b, float eps, void* out, hipStream_t s) {
    hipLaunchKernelGGL(embed_ln_pairs_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, s, ids, pos, types, tokens, H, vocab, max_pos, type_vocab, wemb,
                       pemb, temb, g, b, eps, (bf16_t*)out);
}
void sc_launch_embed_raw_pairs(const int32_t* ids, const int32_t* pos, const int32_t* types, int tokens, int tokens_pad, int H, int vocab, int max_pos,
                               int type_vocab, const float* wemb, const float* pemb, const float* temb, void* out, float* stats, int slots, hipStream_t s) {
    hipLaunchKernelGGL(embed_raw_pairs_kernel, dim3((unsigned)((tokens_pad + 3) / 4)), dim3(256), 0, s, ids, pos, types, tokens, tokens_pad, H, vocab, max_pos,
                       type_vocab, wemb, pemb, temb, (bf16_t*)out, stats, slots);
}
bool sc_pair_head_supported(int H, int num_labels) { return H >= 16 && (H % 16) == 0 && H <= 2048 && num_labels >= 1 && num_labels <= 2; }
void sc_launch_pair_head(const float* cls, int B, int H, const float* Wp, const float* bp, const float* Wc, const float* bc, int num_labels, float* logits,
                         hipStream_t s) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(pair_head_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (2048 + PAIR_HEAD_PAD) * 4);
    });
    hipLaunchKernelGGL(pair_head_kernel, dim3((unsigned)((B + 15) / 16)), dim3(256), (size_t)16 * (H + PAIR_HEAD_PAD) * 4, s, cls, B, H, Wp, bp, Wc, bc, num_labels,
                       logits);
}
