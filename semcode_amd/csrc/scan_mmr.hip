// scan_mmr.hip -- the MMR search's device side (gfx950 / CDNA4): diversified top-k by maximal marginal relevance over the exact
// top-fetch_k of the existing searches (sc_mmr.cpp runs the candidate stage).  Three kernels, none of which touches the corpus scan.
//
// Replaces (reference): nothing on the server side -- the LangChain vector stores the reference's users know offer
// search_type="mmr" by downloading fetch_k embeddings and running numpy on them; this backend keeps the vectors in HBM.
//
// Roofline: mmr_gram is f32 MFMA: F^2 * ld * 2 FLOP per query for F = fetch_k candidates when both triangles are computed; the upper
// triangle alone (what runs here, T (T + 1) / 2 of T^2 tiles, T = ceil(F / 16)) is 14.2 GFLOP at Q = 1 024, F = 128, ld = 768.  It
// gathers F * ld * 4 B of rows per query from HBM once (0.4 GB for that batch); the T re-reads of a row come from L2.  mmr_select
// is latency: k - 1 dependent steps of one L2 line per lane and two barriers.
//
// mmr_inverse_kernel  trained IVF_FLAT only: inv[perm[p]] = p for the stored positions p below `mapped`, inv[p] = p beyond -- the
//                     candidates are row ids, the corpus is addressed by stored position, and the device holds position -> row only.
//                     perm is a permutation of [0, mapped) there, so every entry of inv has exactly one writer.
// mmr_gram_kernel     one wave per 16 x 16 tile (ti <= tj) of a query's candidate x candidate matrix.  Lane (r16, g) streams row
//                     16 ti + r16 (A operand) and row 16 tj + r16 (B operand) straight into registers, 16 B per load, at the float
//                     offsets 64 kc + 16 t + 4 g: the four fragments of a 64-float stage.  One v_mfma_f32_16x16x4_f32 chain per
//                     tile in the canonical k order of oracle/sc_oracle.c (inside each block of 16: k = 16 t + 4 g + c, c outer, g
//                     inner), i.e. the order of scan_exact.hip; no LDS -- a tile's rows have no second reader inside the wave.
//                     Epilogue: sc_score with both norms from xnorm, negated for L2 ("oriented": larger is better), stored at
//                     G[q][i][j] and, off the diagonal, mirrored to G[q][j][i] -- a * b = b * a in every fmaf of the chain and the
//                     norms enter sc_score symmetrically, so the mirrored entry is the bit pattern the other tile would compute.
//                     Slots at or beyond the query's candidate count stream stored position 0; a tile whose rows or columns are
//                     all such slots is skipped, and the selection never reads those entries.
// mmr_select_kernel   one workgroup (two waves, lane i = candidate i) per query: k - 1 greedy steps of mmr_rule.h -- the running
//                     max m_i against the last pick (row `last` of G: one contiguous read), v_i, a butterfly arg-max per wave and
//                     the two wave results combined through LDS.  mmr_takes is a total order, so the tree and a sequential walk
//                     pick the same index; no atomics decide anything (one atomicMin reports the smallest candidate count).
#include "mmr_rule.h"
#include "sc_common.h"

#define MMR_MAX_F 128
#define MMR_SEL_THREADS 128

__global__ __launch_bounds__(256) void mmr_inverse_kernel(const uint32_t* __restrict__ perm, int64_t mapped, int64_t n, uint32_t* __restrict__ inv) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    if (p < mapped) {
        const uint32_t r = perm[p];
        if ((int64_t)r < n) inv[r] = (uint32_t)p;
    } else {
        inv[p] = (uint32_t)p;
    }
}

struct MmrGramArgs {
    const float* X;
    const float* xnorm;
    int ld;
    const int64_t* cand_rows;  // [Q][F] row_base + row, -1 = padding (last)
    int F, Fp, T;              // fetch_k, rounded up to 16, tiles per side
    int64_t row_base, n;
    const uint32_t* inv;       // row -> stored position, NULL: the row is the position
    float* G;                  // [Q][Fp][Fp]
};

// stored position of candidate slot idx (0 and !valid for padding)
static __device__ __forceinline__ int64_t mmr_slot_pos(const MmrGramArgs& a, const int64_t* cand, int idx, bool* valid) {
    const int64_t row = idx < a.F ? cand[idx] : (int64_t)-1;
    const int64_t local = row - a.row_base;
    const bool ok = row >= 0 && local >= 0 && local < a.n;
    int64_t pos = 0;
    if (ok) {
        pos = a.inv ? (int64_t)a.inv[local] : local;
        if (pos >= a.n) pos = 0;
    }
    *valid = ok;
    return pos;
}

template <int METRIC>
__global__ __launch_bounds__(64) void mmr_gram_kernel(MmrGramArgs a) {
    const int lane = threadIdx.x;
    const int r16 = lane & 15, g = lane >> 4;
    const int q = blockIdx.y;
    // tile (ti, tj), ti <= tj, from the linear index over the upper triangle
    int t = blockIdx.x, ti = 0;
    while (t >= a.T - ti) {
        t -= a.T - ti;
        ++ti;
    }
    const int tj = ti + t;
    const int64_t* cand = a.cand_rows + (size_t)q * a.F;
    bool va, vb;
    const int64_t pa = mmr_slot_pos(a, cand, 16 * ti + r16, &va);
    const int64_t pb = mmr_slot_pos(a, cand, 16 * tj + r16, &vb);
    if (!__any(va) || !__any(vb)) return;  // (wave-uniform) nothing of this tile is ever read
    const f32x4* __restrict__ xa = reinterpret_cast<const f32x4*>(a.X + pa * (int64_t)a.ld) + g;
    const f32x4* __restrict__ xb = reinterpret_cast<const f32x4*>(a.X + pb * (int64_t)a.ld) + g;
    const float na = a.xnorm[pa], nb = a.xnorm[pb];
    const int stages = a.ld >> 6;

    f32x4 av[4], bv[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        av[f] = xa[4 * f];
        bv[f] = xb[4 * f];
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int kc = 0; kc < stages; ++kc) {
        f32x4 an[4], bn[4];
        const int nx = kc + 1 < stages ? kc + 1 : kc;  // (the last stage re-reads itself: no branch around the loads)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            an[f] = xa[16 * nx + 4 * f];
            bn[f] = xb[16 * nx + 4 * f];
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[f][c], bv[f][c], acc, 0, 0, 0);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            av[f] = an[f];
            bv[f] = bn[f];
        }
    }

    // lane holds D[row 4 g + c][column r16]: candidate i = 16 ti + 4 g + c against candidate j = 16 tj + r16
    float* Gq = a.G + (size_t)q * a.Fp * a.Fp;
    const int j = 16 * tj + r16;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float ni = __shfl(na, 4 * g + c);
        float s = sc_score<METRIC>(acc[c], ni, nb);
        if (METRIC == SC_METRIC_L2) s = -s;
        const int i = 16 * ti + 4 * g + c;
        Gq[(size_t)i * a.Fp + j] = s;
        if (ti != tj) Gq[(size_t)j * a.Fp + i] = s;
    }
}

__global__ __launch_bounds__(MMR_SEL_THREADS) void mmr_select_kernel(const float* __restrict__ cand_dist, const int64_t* __restrict__ cand_rows, int F, int Fp,
                                                                     const float* __restrict__ G, int k, float lambda, int l2, float pad_dist,
                                                                     float* __restrict__ out_dist, int64_t* __restrict__ out_rows, int32_t* __restrict__ min_count) {
    __shared__ float s_v[2];
    __shared__ int s_i[2];
    __shared__ int s_cnt[2];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    out_dist += (size_t)q * k;
    out_rows += (size_t)q * k;
    // cand_rows == NULL: no candidate stage ran (an empty index) -- padding only
    const int64_t row = (cand_rows && tid < F) ? cand_rows[(size_t)q * F + tid] : (int64_t)-1;
    const bool valid = row >= 0;
    const float d = valid ? cand_dist[(size_t)q * F + tid] : pad_dist;
    const int wave_cnt = (int)__popcll(__ballot(valid));  // (padding is last: the count is the prefix length)
    if (lane == 0) s_cnt[w] = wave_cnt;
    __syncthreads();
    const int C = s_cnt[0] + s_cnt[1];
    if (tid == 0) atomicMin(min_count, C);
    const int steps = k < C ? k : C;
    const float* Gq = G + (size_t)q * Fp * Fp;
    const float rel = l2 ? -d : d;
    const float mu = mmr_mu(lambda);
    bool taken = !valid || tid >= C;
    float m = -__builtin_inff();
    int last = 0;
    if (tid == 0 && steps > 0) {
        out_dist[0] = d;
        out_rows[0] = row;
        taken = true;
    }
    for (int t = 1; t < steps; ++t) {
        float v = 0.0f;
        int idx = -1;
        if (!taken) {
            m = mmr_max(m, Gq[(size_t)last * Fp + tid]);
            v = mmr_value(lambda, mu, rel, m);
            idx = tid;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(v, off);
            const int oi = __shfl_xor(idx, off);
            if (mmr_takes(ov, oi, v, idx)) {
                v = ov;
                idx = oi;
            }
        }
        if (lane == 0) {
            s_v[w] = v;
            s_i[w] = idx;
        }
        __syncthreads();
        float bv = s_v[0];
        int bi = s_i[0];
        if (mmr_takes(s_v[1], s_i[1], bv, bi)) {
            bv = s_v[1];
            bi = s_i[1];
        }
        __syncthreads();  // (s_v / s_i are written again in the next step)
        last = bi;        // (>= 0: t < steps <= C leaves a candidate that is not taken)
        if (tid == last) {
            out_dist[t] = d;
            out_rows[t] = row;
            taken = true;
        }
    }
    for (int pos = steps + tid; pos < k; pos += MMR_SEL_THREADS) {
        out_dist[pos] = pad_dist;
        out_rows[pos] = -1;
    }
}

void sc_launch_mmr_inverse(const uint32_t* perm, int64_t mapped, int64_t n, uint32_t* inv, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(mmr_inverse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, perm, perm ? mapped : (int64_t)0, n, inv);
}

void sc_launch_mmr_gram(int metric, const float* X, const float* xnorm, int ld, int64_t n, int64_t row_base, const uint32_t* inv, const int64_t* cand_rows, int F, int Q,
                        float* G, hipStream_t s) {
    if (Q < 1 || F < 1 || F > MMR_MAX_F || n < 1) return;  // (the host checks these before it plans a call)
    MmrGramArgs a;
    a.X = X; a.xnorm = xnorm; a.ld = ld; a.cand_rows = cand_rows; a.F = F; a.Fp = (F + 15) & ~15; a.T = a.Fp / 16;
    a.row_base = row_base; a.n = n; a.inv = inv; a.G = G;
    const dim3 grid((unsigned)(a.T * (a.T + 1) / 2), (unsigned)Q);
    sc_dispatch_metric(metric, [&](auto mc) { hipLaunchKernelGGL((mmr_gram_kernel<mc.value>), grid, dim3(64), 0, s, a); });
}

void sc_launch_mmr_select(int metric, const float* cand_dist, const int64_t* cand_rows, int F, const float* G, int Q, int k, float lambda, float* out_dist,
                          int64_t* out_rows, int32_t* min_count, hipStream_t s) {
    if (Q < 1 || F < 1 || F > MMR_MAX_F || k < 1 || k > F) return;
    const float pad = metric == SC_METRIC_L2 ? __builtin_inff() : -__builtin_inff();
    hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)Q), dim3(MMR_SEL_THREADS), 0, s, cand_dist, cand_rows, F, (F + 15) & ~15, G, k, lambda,
                       metric == SC_METRIC_L2 ? 1 : 0, pad, out_dist, out_rows, min_count);
}
