// encoder_heads.hip -- the classification heads of the rerankers that sit on the pre-norm family (cfg.arch 1) and on the causal decoders
// (cfg.arch 2), on the f32 row the forward pooled for every sequence (gfx950).  Siblings of encoder_pairs.hip's pair_head_kernel.
//
//   score_head_kernel<NT>   kind 1, the prediction head of the pre-norm family:  r [B, H] f32 ->
//                               g = gelu_erf(Wd r + bd),  p = (g - mean(g)) * rstd * gamma + beta,  rstd = 1 / sqrt(var(g) + eps),
//                               logits = Wc p + bc,  num_labels 1 or 2;  bd, beta, bc may be NULL (zeros).
//   score_linear_kernel     kind 2, the `score` layer of a decoder (or two rows of its vocabulary projection): logits = Wc r + bc.
//
// score_head_kernel: one workgroup (4 waves) per 16 rows, staged in the LDS as [16][H + 4] f32 exactly as pair_head_kernel stages its [CLS]
// rows, and the dense layer runs as there: wave w owns the 16-column tiles n0 = 16 w + 64 t of Wd, D[n][row] = sum_k Wd[n][k] r[row][k] with
// v_mfma_f32_16x16x4_f32, a lane loading four consecutive k of its k group (l >> 4) as one 16-byte piece from either side, even and odd
// 16-wide stages in two accumulator chains that are added at the end.  A lane then holds g[n0 + 4 (l >> 4) + c] of row l & 15, c < 4.
// What is new is the LayerNorm between the dense layer and the classifier: a row's statistics need every one of its H columns, and a second
// f32 copy of the 16 x H tile does not fit the LDS next to the first (2 x 128 KiB at H = 2 048 against 160 KiB).  So the activated values
// STAY in the registers of the lane that computed them -- gv[t][c], t < NT tiles per wave, NT = 8 / 16 / 32 for H <= 512 / 1 024 / 2 048,
// every index a compile-time constant -- and only sums cross lanes, through three [wave][k group][row] tables in the LDS:
//   1. the lane's sum of gv in (t, c) order -> sum1;  every lane of a row adds the 16 partials in (wave, k group) order: mean = s / H
//   2. the lane's sum of (gv - mean)^2, same orders -> sum2: var = q / H, rstd = 1 / sqrtf(var + eps)   (two-pass, centred)
//   3. p = (gv - mean) * rstd * gamma[n] + beta[n];  the lane's fmaf chain over Wc[label][n] p in (t, c) order -> part; one thread per
//      (row, label) adds the 16 partials in (wave, k group) order and then bc.
// Every lane of a row reads the same 16 partials in the same order, so all hold the same mean and rstd bits.  No atomics, every order
// fixed, nothing depends on the other rows of the workgroup: a row's logits are the same bits wherever it stands and whoever stands next
// to it.  Rows beyond B are zero rows: computed (finite: eps > 0), never stored.
// The GELU is gemm_tile.h's gelu_erf_fast2, the one the FFN epilogues use (|error| <= 2.5e-7).
// Registers and scratch: at the launcher.
//
// score_linear_kernel: one wave per row, four rows per workgroup.  Lane j multiplies the 16-byte pieces j, j + 64, ... of the row and of
// Wc's rows in ascending order into one fmaf chain per label (element order inside a piece), then the 64 chains are added by the xor
// butterfly 32, 16, 8, 4, 2, 1 (every lane ends with the same bits), then bc.
#include "encoder_ops.h"
#include "gemm_tile.h"

#define SCORE_HEAD_PAD 4  // floats between two rows in the LDS (pair_head_kernel's reasoning)
// Keeps a value out of the compiler's packed-f32 forms: a v_pk_*_f32 whose low lane takes the high register of an operand (op_sel) is the
// encoding gemm_bf16.hip's SC_OPAQUE_PAIR comment describes and tests/test_isa.py refuses in every kernel of the library.
#define SCORE_OPAQUE(v) asm volatile("" : "+v"(v))

template <int NT>
__global__ __launch_bounds__(256) void score_head_kernel(const float* __restrict__ r, int B, int H, const float* __restrict__ Wd, const float* __restrict__ bd,
                                                          const float* __restrict__ gam, const float* __restrict__ bet, float eps, const float* __restrict__ Wc,
                                                          const float* __restrict__ bc, int num_labels, float* __restrict__ logits) {
    extern __shared__ __attribute__((aligned(16))) float rows[];  // [16][H + SCORE_HEAD_PAD]
    __shared__ float sum1[4][4][16], sum2[4][4][16];              // [wave][k group][row]
    __shared__ float part[4][4][2][16];                           // [wave][k group][label][row]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int ld = H + SCORE_HEAD_PAD, h4 = H >> 2;
    for (int i = tid; i < 16 * h4; i += 256) {
        const int rr = i / h4, c4 = i - rr * h4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};  // rows beyond B: zero rows, computed and never stored
        if (b0 + rr < B) v = *reinterpret_cast<const f32x4*>(r + (size_t)(b0 + rr) * H + 4 * c4);
        *reinterpret_cast<f32x4*>(rows + rr * ld + 4 * c4) = v;
    }
    __syncthreads();

    const float* xrow = rows + r16 * ld + 4 * g;
    const int stages = H >> 4;
    f32x4 gv[NT];  // the activated dense outputs n = 16 w + 64 t + 4 g + c of row r16; tiles at or beyond H stay zero and are never read
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n0 = 16 * w + 64 * t;  // wave-uniform
        gv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (n0 < H) {
            const float* wrow = Wd + (size_t)(n0 + r16) * H + 4 * g;
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
            f32x4 d = acc0 + acc1;
            if (bd) d += *reinterpret_cast<const f32x4*>(bd + n0 + 4 * g);
            const f32x2 lo = gelu_erf_fast2(f32x2{d[0], d[1]}), hi = gelu_erf_fast2(f32x2{d[2], d[3]});
            gv[t] = f32x4{lo[0], lo[1], hi[0], hi[1]};
        }
    }
    const float fh = (float)H;
    // 1. mean
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (16 * w + 64 * t < H) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s += gv[t][c];
        }
    sum1[w][g][r16] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) tot += sum1[ww][gg][r16];
    const float mean = tot / fh;
    // 2. centred squares
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (16 * w + 64 * t < H) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float dv = gv[t][c] - mean;
                q = fmaf(dv, dv, q);
            }
        }
    sum2[w][g][r16] = q;
    __syncthreads();
    float qt = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) qt += sum2[ww][gg][r16];
    const float rstd = 1.0f / sqrtf(qt / fh + eps);
    // 3. normalise, classify
    float lg[2] = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n0 = 16 * w + 64 * t;
        if (n0 < H) {
            const f32x4 ga = *reinterpret_cast<const f32x4*>(gam + n0 + 4 * g);
            f32x4 be = {0.f, 0.f, 0.f, 0.f};
            if (bet) be = *reinterpret_cast<const f32x4*>(bet + n0 + 4 * g);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wc + n0 + 4 * g);
            f32x4 w1 = {0.f, 0.f, 0.f, 0.f};
            if (num_labels > 1) w1 = *reinterpret_cast<const f32x4*>(Wc + H + n0 + 4 * g);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float p = (gv[t][c] - mean) * rstd * ga[c] + be[c];
                lg[0] = fmaf(w0[c], p, lg[0]);
                lg[1] = fmaf(w1[c], p, lg[1]);
            }
        }
    }
    part[w][g][0][r16] = lg[0];
    part[w][g][1][r16] = lg[1];
    __syncthreads();
    if (tid < 16 * num_labels) {
        const int b = tid & 15, c = tid >> 4;
        float sl = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww)
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) sl += part[ww][gg][c][b];
        if (b0 + b < B) logits[(size_t)(b0 + b) * num_labels + c] = bc ? sl + bc[c] : sl;
    }
}

__global__ __launch_bounds__(256) void score_linear_kernel(const float* __restrict__ r, int B, int H, const float* __restrict__ Wc, const float* __restrict__ bc,
                                                            int num_labels, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;  // wave-uniform; no barrier below
    const float* x = r + (size_t)b * H;
    float lg[2] = {0.f, 0.f};
    for (int k4 = lane; k4 < (H >> 2); k4 += 64) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * k4);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(Wc + 4 * k4);
        f32x4 w1 = {0.f, 0.f, 0.f, 0.f};
        if (num_labels > 1) w1 = *reinterpret_cast<const f32x4*>(Wc + H + 4 * k4);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            lg[0] = fmaf(w0[c], xv[c], lg[0]);
            SCORE_OPAQUE(lg[0]);  // two scalar chains: packed into one v_pk_fma_f32 the shared xv[c] becomes an op_sel broadcast (below)
            lg[1] = fmaf(w1[c], xv[c], lg[1]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lg[0] += __shfl_xor(lg[0], off);
        lg[1] += __shfl_xor(lg[1], off);
    }
    if (lane < num_labels) {
        const float v = lane == 0 ? lg[0] : lg[1];
        logits[(size_t)b * num_labels + lane] = bc ? v + bc[lane] : v;
    }
}

// ------------------------------------------------------------------ launchers
bool sc_score_head_supported(int H, int num_labels) { return H >= 16 && (H % 16) == 0 && H <= 2048 && num_labels >= 1 && num_labels <= 2; }

// Resource use (the library's flags, build.py: -O3 -ffp-contract=off --offload-arch=gfx950 -munsafe-fp-atomics, with
// -Rpass-analysis=kernel-resource-usage; without -ffp-contract=off <16> and <32> take one VGPR more; profiles/rerank_heads_kernels.log), VGPRs + AGPRs,
// scratch bytes per lane, waves per SIMD:  score_head_kernel<8> 74 + 8, 0, 5;  <16> 120 + 8, 0, 4;  <32> 233 + 8, 0, 2 (the 128 registers of
// gv and the unrolled tiles' addresses; the LDS allows one workgroup per CU at H = 2 048 anyway);  score_linear_kernel 22 + 0, 0, 8.
template <int NT>
static void launch_score_head(const float* r, int B, int H, const float* Wd, const float* bd, const float* gam, const float* bet, float eps, const float* Wc,
                              const float* bc, int num_labels, float* logits, hipStream_t s) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(score_head_kernel<NT>), hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (64 * NT + SCORE_HEAD_PAD) * 4);
    });
    hipLaunchKernelGGL(score_head_kernel<NT>, dim3((unsigned)((B + 15) / 16)), dim3(256), (size_t)16 * (H + SCORE_HEAD_PAD) * 4, s, r, B, H, Wd, bd, gam, bet, eps, Wc,
                       bc, num_labels, logits);
}

void sc_launch_score_head(const float* r, int B, int H, const float* Wd, const float* bd, const float* gam, const float* bet, float eps, const float* Wc,
                          const float* bc, int num_labels, float* logits, hipStream_t s) {
    if (!Wd) {
        hipLaunchKernelGGL(score_linear_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, r, B, H, Wc, bc, num_labels, logits);
        return;
    }
    if (H <= 512) launch_score_head<8>(r, B, H, Wd, bd, gam, bet, eps, Wc, bc, num_labels, logits, s);
    else if (H <= 1024) launch_score_head<16>(r, B, H, Wd, bd, gam, bet, eps, Wc, bc, num_labels, logits, s);
    else launch_score_head<32>(r, B, H, Wd, bd, gam, bet, eps, Wc, bc, num_labels, logits, s);
}
