// gemm_bf16.hip -- C[M,N] = A[M,K] * W[N,K]^T (+ bias, + GELU | + residual), bf16 in, f32 accumulate,
// bf16 out, on the CDNA4 matrix cores (v_mfma_f32_16x16x32_bf16).  gfx950 only.
//
// Replaces (reference): the per-layer matmuls llama.cpp runs on CPU threads behind
// LlamaCppEmbeddings.embed_documents (src/semcode/embeddings/providers.py:69-100, called at
// src/semcode/services/indexer.py:150).  Both operands are "K-contiguous" (activations [M,K] and
// torch-Linear weights [N,K]), so A and W tiles are staged and read identically.
//
// Roofline: MFMA bf16 (2.5 PFLOP/s dense).  Algorithmic FLOPs = 2*M*N*K.
//
// Structure (128x128x64 tile, 4 waves as 2x2, each wave 64x64 = 4x4 MFMA tiles):
//   * both tiles are staged global -> LDS by LDS-DMA (global_load_lds_dwordx4, 16 B/lane), two LDS
//     buffers, the load of K-step t+1 is issued before the MFMAs of K-step t, one barrier per K-step;
//   * LDS rows are 128 B (64 bf16); the 16-byte chunk c of row r is stored at chunk c ^ ((r>>1)&7)
//     (applied on the per-lane SOURCE address, because LDS-DMA writes linearly) which makes every
//     ds_read_b128 fragment read bank-conflict free;
//   * operands are swapped (MFMA A = weight rows, B = activation rows) so that each lane ends up with
//     4 consecutive output columns of one output row -> 8-byte bf16 stores, bias as one float4;
//   * workgroup ids are remapped so that the tiles of one 128-row panel run on the same XCD (shared A
//     panel stays in that XCD's L2).
#include <algorithm>
#include <cstdlib>

#include "encoder_ops.h"
#include "gemm_tile.h"

#ifndef SC_GEMM_PP_DEFAULT
#define SC_GEMM_PP_DEFAULT 4
#endif

// EPI_LNA_*: the A operand is a PRE-LayerNorm tensor y (raw bf16 rows) and the weights carry the LayerNorm's gamma
// (W' = W diag(gamma)): with the row statistics mu, rs of y,  LN(y) W^T + b = rs (y W'^T - mu c1) + c2,  c1[n] = sum_k W'[n,k],
// c2[n] = b[n] + sum_k beta[k] W[n,k] -- the normalisation becomes two FMAs in the epilogue and the LayerNorm kernel disappears.
// EPI_RESLN_STATS: bias + LayerNorm(residual) applied on the fly ((r - mu) rs g + beta, beta folded into the bias), and the
// row sums / sums of squares of THIS output (after its bf16 rounding) written per 256-column tile for the consumer's statistics.
// EPI_LNA_BIAS_ROPE: EPI_LNA_BIAS of a QKV projection with the rotary position embedding (rotate-half) applied to the Q and K
// columns in the accumulator registers, before the one rounding to bf16.
// (the EPI_* codes: encoder_ops.h)

struct GemmArgs {
    const bf16_t* A;   // [M, lda]
    const bf16_t* W;   // [N, ldw]
    const float* bias; // [N]
    const bf16_t* R;   // [M, ldr] residual (EPI_BIAS_RES)
    bf16_t* C;         // [M, ldc]
    int M, N, K, lda, ldw, ldr, ldc;
    int tiles_n;       // N / 128
    int ntiles;        // (M/128) * tiles_n
    int order;         // 256-tile kernels: tile walk (see gemm256_tile)
    int splitk;        // split-K kernels: number of K slices (grid = ntiles * splitk)
    int strip;         // strip kernel: column tiles per workgroup (grid = (M / 256) * ceil(tiles_n / strip))
    float* partial;    // split-K kernels: [splitk][M][N] f32 partial products
    unsigned long long* trace;  // diagnostic: per-workgroup time stamps [ntiles][8] (sc_diag_gemm_trace), else nullptr
    int nt;            // 256-tile kernel: write C with non-temporal stores (outputs far larger than L2)
    int cblock;        // 1: C is stored as [N / 64][M][64] (64-column blocks, each contiguous over the rows) instead of [M][ldc]
    int ablock;        // 1: A is stored that way, [K / 64][M][64] (256-tile kernel only)
    // LayerNorm fold (EPI_LNA_*, EPI_RESLN_STATS; 256-tile kernel only)
    const float* c1;         // EPI_LNA_*: [N] column sums of the bf16 W' (bias = c2)
    const float* stats_in;   // EPI_LNA_*: [slots][M][2] partial (sum, sum of squares) of the A tensor's rows, one slot per 256 columns of it
    int stat_slots;          //            K / 256
    float* fin;              // EPI_LNA_*: out, EPI_RESLN_STATS: in -- [M][2] finalised (mu, rs) of those rows
    const float* gam;        // EPI_RESLN_STATS: [N] gamma of the residual's LayerNorm (its beta is folded into bias)
    float* stats_out;        // EPI_RESLN_STATS: [N / 256][M][2] partial sums of this output's rows
    float ln_eps;
    // rotary positions (EPI_LNA_BIAS_ROPE): cos / sin tables [>= rope_smask + 1][32] f32, position of row m = m & rope_smask
    // (sequence length a power of two), column tiles below rope_ncols (= 2 H: Q and K) are rotated
    const float* rope_cos;
    const float* rope_sin;
    int rope_smask, rope_ncols;
};

// address of C[m][n] (n % 4 == 0 where vectors are stored): row-major, or 64-column blocks that are contiguous over the rows --
// the QKV projection writes that, so that attention reads each head's Q / K / V as one contiguous [tokens][64] block and a wave's
// 16 x 64 output block is 2 KiB of consecutive bytes instead of 16 segments 4.6 KB apart
static __device__ __forceinline__ size_t c_index(const GemmArgs& a, int64_t m, int n) {
    return a.cblock ? ((size_t)(n >> 6) * (size_t)a.M + (size_t)m) * 64 + (size_t)(n & 63) : (size_t)m * a.ldc + n;
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][A tile | W tile]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;

    const int tile = xcd_remap(blockIdx.x, a.ntiles);
    const int mt = tile / a.tiles_n, nt = tile - mt * a.tiles_n;
    const int m0 = mt * G_BM, n0 = nt * G_BN;

    f32x4 acc[4][4];  // [ni][mi]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm_tile_mainloop(a.A, a.lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, lane);
    const int fr = lane & 15, fq = lane >> 4;

    // epilogue: acc[ni][mi][r] = C[m0 + wm*64 + mi*16 + fr][n0 + wn*64 + ni*16 + 4*fq + r]
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wn * 64 + ni * 16 + 4 * fq;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = m0 + wm * 64 + mi * 16 + fr;
            f32x4 v = acc[ni][mi] + bv;
            if (EPI == EPI_BIAS_GELU) {
                // the form of the 256-tile and split-K epilogues: 0.5 x (1 + erff(x / sqrt 2)) cancels in f32 for x < -3.4 and is off by
                // more than a bf16 ulp of the result at |gelu| ~ 1e-5 .. 1e-4 (tests/test_gemm_plain_gpu.py)
                const f32x2 g0 = gelu_erf_fast2(f32x2{v[0], v[1]}), g1 = gelu_erf_fast2(f32x2{v[2], v[3]});
                v = f32x4{g0[0], g0[1], g1[0], g1[1]};
            }
            if (EPI == EPI_BIAS_RES) {
                const u16x4 rv = *reinterpret_cast<const u16x4*>(a.R + (size_t)m * a.ldr + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(rv[r]);
            }
            u16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = f32_to_bf16(v[r]);
            *reinterpret_cast<u16x4*>(a.C + c_index(a, m, n)) = o;
        }
    }
}


// ---- 256 x 256 x 64 tile variant (gemm_tile.h, second half); used when M % 256 == 0 and N % 256 == 0.
// tile walk: bit 0 of order = skip the XCD remap; order >> 1 = G: walk column-major inside groups of G row panels
static __device__ __forceinline__ void tile_coords256(const GemmArgs& a, int vt, int& m0, int& n0) {
    const int tile = (a.order & 1) ? vt : xcd_remap(vt, a.ntiles);
    int mt = tile / a.tiles_n, nt = tile - mt * a.tiles_n;
    const int G = a.order >> 1;
    if (G > 1) {
        const int tiles_m = a.ntiles / a.tiles_n;
        const int gsz = G * a.tiles_n, g = tile / gsz, r = tile - g * gsz;
        const int rows_here = (g * G + G <= tiles_m) ? G : tiles_m - g * G;  // last group may be short
        mt = g * G + r % rows_here;
        nt = r / rows_here;
    }
    m0 = __builtin_amdgcn_readfirstlane(mt * T_BM);
    n0 = __builtin_amdgcn_readfirstlane(nt * T_BN);
}

// Residual tile -> LDS.  After the last barrier of the main loop the 128 KiB of pipeline buffers are dead, exactly the size of
// the 256 x 256 bf16 residual tile: every wave LDS-DMAs its own 128 x 64 part (16 pieces of 1 KiB = 8 rows x 128 B each)
// into its own 16 KiB, under the final 32 MFMAs and at no register cost.  Rows are 128 B; the 16-byte chunk c of row r
// sits at chunk c ^ ((r >> 1) & 7) (applied on the source address, LDS-DMA writes linearly), which makes the epilogue's
// 8-byte reads in the MFMA layout bank-conflict free.  Fetched from registers block by block next to the stores, the
// residual cost a full load + store round trip per block: 12 us per tile against a 20 us main loop
// (profiles/r1o_gemm_trace.log).
struct ResidualTailHook {
    static constexpr bool kCoop = false;
    const bf16_t* R;  // tile origin: R + m0 * ldr + n0
    int ldr, w, lane;
    char* smem;
    __device__ __forceinline__ void coop(int, int, const uint32_t (&)[2], const uint32_t (&)[2]) const {}
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void operator()() const {
        int ln = lane;
        asm volatile("" : "+v"(ln));  // keep the address arithmetic out of the register-tight K loop
        const int wm = w >> 2, wn = w & 3;
        const int prow = ln >> 3, pos = ln & 7;
        char* dst = smem + w * 16384;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            const int row = d * 8 + prow;
            const int cs = pos ^ ((row >> 1) & 7);
            const bf16_t* g = R + (size_t)(wm * 128 + row) * ldr + wn * 64 + cs * 8;
            __builtin_amdgcn_global_load_lds((gbl_vptr)g, (lds_vptr)(dst + d * 1024), 16, 0, 2);
        }
    }
};

// EPI_LNA_*: the partial row sums of this wave's 128 rows, stat_slots pieces of 1 KiB (128 rows x {sum, sumsq} f32), into the wave's
// own slice of the dead pipeline buffers, under the last 32 MFMAs.
struct LnaTailHook {
    static constexpr bool kCoop = false;
    const float* stats;  // stats_in + (m0 + wm * 128) * 2, slot stride = M * 2 floats
    size_t slot_stride;
    int slots, w, lane;
    char* smem;
    __device__ __forceinline__ void coop(int, int, const uint32_t (&)[2], const uint32_t (&)[2]) const {}
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void operator()() const {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        char* dst = smem + w * 16384;
        for (int sl = 0; sl < slots; ++sl)
            __builtin_amdgcn_global_load_lds((gbl_vptr)(stats + sl * slot_stride + ln * 4), (lds_vptr)(dst + sl * 1024), 16, 0, 0);
    }
};
// EPI_RESLN_STATS: the residual tile as in ResidualTailHook, plus the finalised (mu, rs) of this wave's 128 rows (1 KiB) into its
// epilogue staging slice (read into registers before the first staging write).
struct ResLnTailHook {
    static constexpr bool kCoop = false;
    ResidualTailHook res;
    const float* fin;  // fin + (m0 + wm * 128) * 2
    __device__ __forceinline__ void coop(int, int, const uint32_t (&)[2], const uint32_t (&)[2]) const {}
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ void operator()() const {
        res();
        int ln = res.lane;
        asm volatile("" : "+v"(ln));
        __builtin_amdgcn_global_load_lds((gbl_vptr)(fin + ln * 4), (lds_vptr)(res.smem + 4 * T_TILE_BYTES + res.w * (16 * T_EPI_ROW)), 16, 0, 0);
    }
};

// Ping-pong main loop: the residual tile continues the ring (gemm_tile.h, "tail hooks").  Slot s receives the 128 x 64 part of
// wave s -- the image the epilogues read from smem + w * 16384, same swizzle -- but every wave requests two of its 16 pieces
// (pieces 2 w, 2 w + 1: rows 16 w .. 16 w + 15 of the part), one slot per phase as the slots fall free: the requests are spread
// over the last 1.5 K-tiles like the loop's own instead of bursting 16 per wave into the last phase (out-projection:
// gpurun_out/r3b_gemm_pp_epi.log, 88 us per launch of which ~6 per tile were this epilogue's fetch).  The epilogue then needs
// vmcnt(0) + one barrier of all 8 waves before its first read.
struct ResidualCoopHook {
    static constexpr bool kCoop = true;
    const bf16_t* R;  // tile origin: R + m0 * ldr + n0
    int ldr, w, lane;
    char* smem;
    __amdgpu_buffer_rsrc_t rr;
    uint32_t v0, v1;
    __device__ __forceinline__ void prepare() {  // called once, in front of the last two K-tiles
        int ln = lane;
        asm volatile("" : "+v"(ln));  // keep the address arithmetic out of the register-tight K loop
        rr = __builtin_amdgcn_make_buffer_rsrc((void*)R, 0, -1, 0x00020000);
        const int prow = ln >> 3, pos = ln & 7;
        const int r0 = 16 * w + prow, r1 = r0 + 8;
        v0 = (uint32_t)((r0 * ldr + (pos ^ ((r0 >> 1) & 7)) * 8) * 2);
        v1 = (uint32_t)((r1 * ldr + (pos ^ ((r1 >> 1) & 7)) * 8) * 2);
    }
    __device__ __forceinline__ void coop(int slot, int, const uint32_t (&)[2], const uint32_t (&)[2]) const {
        const uint32_t so = (uint32_t)(((slot >> 2) * 128 * ldr + (slot & 3) * 64) * 2);
        char* dst = smem + slot * 16384 + 2 * w * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_vptr)dst, 16, v0, so, 0, 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_vptr)(dst + 1024), 16, v1, so, 0, 2);
    }
    __device__ __forceinline__ void operator()() const {}
};
struct ResLnCoopHook {
    static constexpr bool kCoop = true;
    ResidualCoopHook res;
    const float* fin;  // fin + (m0 + wm * 128) * 2
    __device__ __forceinline__ void prepare() { res.prepare(); }
    __device__ __forceinline__ void coop(int slot, int h, const uint32_t (&va)[2], const uint32_t (&vw)[2]) const { res.coop(slot, h, va, vw); }
    __device__ __forceinline__ void operator()() const {  // the wave's own (mu, rs) rows into its own staging slice
        int ln = res.lane;
        asm volatile("" : "+v"(ln));
        __builtin_amdgcn_global_load_lds((gbl_vptr)(fin + ln * 4), (lds_vptr)(res.smem + 4 * T_TILE_BYTES + res.w * (16 * T_EPI_ROW)), 16, 0, 0);
    }
};

// A scalar broadcast to both halves of a packed-f32 operand, as a real 64-bit register pair.  Left to itself hipcc encodes such a
// broadcast with the VOP3P selects (op_sel / op_sel_hi) on whatever register holds the scalar, and one of those forms --
// "v_pk_mul_f32 D, S0, S1 op_sel:[0,1]", the LOW result lane taking the HIGH register of src1 -- intermittently returned 0 in
// lanes 48..63 of the low result on MI355X while other waves of the CU were still in their MFMA loop (first waves into the
// epilogue, row blocks 0..2; operands verified correct in registers, ~2e-4 of the instances; gpurun_out/dbg_fold4..6: the same
// multiply with an explicit pair, with the operands swapped (op_sel:[1,0]) or as two v_mul_f32 never failed, s_nop in front did
// not help).  The 256-tile epilogues therefore carry no op_sel on a packed-f32 operand: tests/test_isa.py greps the ISA for it.
#define SC_OPAQUE_PAIR(p) asm volatile("" : "+v"(p))

// Epilogue: the MFMA layout gives each lane 4 columns of 16 different rows (32-byte row segments per store).  Each
// wave stages one 16-row x 64-column block at a time as bf16 in its private LDS slice BEHIND the pipeline buffers and
// stores whole 128-byte row segments, 16 B per lane.  bias, GELU and the residual (read from LDS, see above) are applied
// in f32 before the single bf16 rounding.  DS operations of one wave execute in order, so the slice is reused without
// waits beyond the data dependencies.  Everything per lane is derived from an opaque copy of the lane id so that hipcc
// cannot hoist it above the register-tight K loop.
template <int EPI, bool COOP = false>
static __device__ __forceinline__ void gemm256_epilogue(const GemmArgs& a, int m0, int n0, char* smem, int w, int lane, f32x4 (&acc)[4][8]) {
    const int wm = w >> 2, wn = w & 3;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    __builtin_amdgcn_sched_barrier(0);
    const int fr = ln & 15, fq = ln >> 4;
    const int prow = ln >> 3, c8 = (ln & 7) * 8;
    char* stg = smem + 4 * T_TILE_BYTES + w * (16 * T_EPI_ROW);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    f32x4 bias4[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bias4[ni] = *reinterpret_cast<const f32x4*>(a.bias + n0 + wn * 64 + ni * 16 + 4 * fq);
    const char* rlds = smem + w * 16384 + fr * 128 + (fq & 1) * 8;  // + mi * 2048 + ((chunk ^ swz) << 4)
    const int swz = (fr >> 1) & 7;                                  // ((mi * 16 + fr) >> 1) & 7
    u32x2 rr[8][4];  // residual in the MFMA layout, read up front (the fragment registers are dead): the compiler cannot
                     // move LDS reads across the staging writes below, and one read -> add -> write chain per block is slow
    if (EPI == EPI_BIAS_RES) {
        if (COOP) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");  // every wave's pieces of every part have landed
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's residual DMA has landed
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                rr[mi][ni] = *reinterpret_cast<const u32x2*>(rlds + mi * 2048 + (((ni * 2 + (fq >> 1)) ^ swz) << 4));
    }
    const size_t crs = a.cblock ? 64 : (size_t)a.ldc;  // row stride of this wave's 64-column block
    bf16_t* cp = a.C + c_index(a, m0 + wm * 128 + prow, n0 + wn * 64) + c8;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            f32x4 v = acc[ni][mi] + bias4[ni];
            if (EPI == EPI_BIAS_GELU) {
                const f32x2 g0 = gelu_erf_fast2(f32x2{v[0], v[1]}), g1 = gelu_erf_fast2(f32x2{v[2], v[3]});
                v = f32x4{g0[0], g0[1], g1[0], g1[1]};
            }
            if (EPI == EPI_BIAS_RES) {
                const u32x2 r2 = rr[mi][ni];
                v += f32x4{__builtin_bit_cast(float, r2[0] << 16), __builtin_bit_cast(float, r2[0] & 0xFFFF0000u),
                           __builtin_bit_cast(float, r2[1] << 16), __builtin_bit_cast(float, r2[1] & 0xFFFF0000u)};
            }
            *reinterpret_cast<u32x2*>(stg + fr * T_EPI_ROW + (ni * 16 + 4 * fq) * 2) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const u32x4 o = *reinterpret_cast<const u32x4*>(stg + (j * 8 + prow) * T_EPI_ROW + c8 * 2);
            bf16_t* dst = cp + (size_t)(mi * 16 + j * 8) * crs;
            // Large outputs are written non-temporally: a launch of the batch step writes 100-400 MB of C through 32 MB of L2
            // and, written back normally, evicts the A row panels the next column tiles of the same panel are about to re-read
            // (same-box A/B: QKV +3 %, out-proj +7 %, FFN1 +8 %, FFN2 +3 %, encoder 18.9k -> 19.7k chunks/s).  Inline asm because
            // the two stores of an if/else get merged by the compiler, which drops the non-temporal hint.
            if (a.nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(o) : "memory");
            else *reinterpret_cast<u32x4*>(dst) = o;
        }
    }
}

// ---- LayerNorm-folded epilogues --------------------------------------------------------------------------------------
// EPI_LNA_BIAS_ROPE: a wave owns 64 output columns = one head of Q, K or V, and lane (fr, fq) holds columns ni 16 + 4 fq + {0..3},
// ni = 0..3, of row fr of each mi block: columns j and j + 32 of the head are acc[ni][mi][c] and acc[ni + 2][mi][c] of the SAME lane,
// so the rotation t'[j] = t[j] cos - t[j + 32] sin, t'[j + 32] = t[j + 32] cos + t[j] sin needs no exchange: 8 cos + 8 sin values per
// (lane, mi) from the table row of that output row's position.  Scalar FMAs (packed f32 with a broadcast operand: tests/test_isa.py).
// EPI_LNA_BIAS / EPI_LNA_GELU: out = rs_m (acc - mu_m c1[n]) + c2[n] (+ GELU).  (mu, rs) of a row come from the partial sums the
// producing GEMM left per 256-column tile of the A tensor (LnaTailHook put this wave's 128 rows x slots into its pipeline slice);
// the column tile n0 == 0 also publishes them finalised ([M][2]) for the residual epilogue of the next GEMM.
// (mu, rs) of two rows from their summed {sum, sumsq | sum, sumsq}: v_rsq_f32 (1 ulp) is ample in front of a bf16 rounding
static __device__ __forceinline__ f32x4 lna_finalise(const GemmArgs& a, const f32x4& sacc) {
    const float inv_k = 1.0f / (float)a.K;
    const float mu0 = sacc[0] * inv_k, mu1 = sacc[2] * inv_k;
    const float rs0 = __builtin_amdgcn_rsqf(fmaxf(fmaf(-mu0, mu0, sacc[1] * inv_k), 0.f) + a.ln_eps);
    const float rs1 = __builtin_amdgcn_rsqf(fmaxf(fmaf(-mu1, mu1, sacc[3] * inv_k), 0.f) + a.ln_eps);
    return f32x4{mu0, rs0, mu1, rs1};
}

// mrs: where the finalised (mu, rs) of this wave's 128 rows live in LDS (1 KiB).  Per-tile kernel: the wave's pipeline slice -- the
// statistics slots arrive there and are finalised in place.  STRIP (gemm256_strip_kernel): behind the staging area, finalised once
// by the caller -- the pipeline ring already holds the next tile and is not touched here.
template <int EPI, bool STRIP = false>
static __device__ __forceinline__ void gemm256_epilogue_lna(const GemmArgs& a, int m0, int n0, char* smem, int w, int lane, f32x4 (&acc)[4][8], char* mrs) {
    const int wm = w >> 2, wn = w & 3;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    __builtin_amdgcn_sched_barrier(0);
    const int fr = ln & 15, fq = ln >> 4;
    const int prow = ln >> 3, c8 = (ln & 7) * 8;
    char* stg = smem + 4 * T_TILE_BYTES + w * (16 * T_EPI_ROW);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    f32x4 c1v[4], c2v[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        c1v[ni] = *reinterpret_cast<const f32x4*>(a.c1 + n0 + wn * 64 + ni * 16 + 4 * fq);
        c2v[ni] = *reinterpret_cast<const f32x4*>(a.bias + n0 + wn * 64 + ni * 16 + 4 * fq);
    }
    if constexpr (!STRIP) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's statistics DMA has landed
        // (mu, rs) of the wave's 128 rows: lane ln finalises rows 2 ln and 2 ln + 1 ONCE (every lane doing its own 8 rows cost 8 divide
        // + square-root sequences per lane: +29 / +52 us per QKV / FFN1 launch, gpurun_out/prof_fold1) and parks them in place of
        // slot 0.
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f};  // {sum, sumsq} of row 2 ln | of row 2 ln + 1
        for (int t = 0; t < a.stat_slots; ++t) sacc += *reinterpret_cast<const f32x4*>(mrs + t * 1024 + ln * 16);
        const f32x4 fin4 = lna_finalise(a, sacc);
        *reinterpret_cast<f32x4*>(mrs + ln * 16) = fin4;
        if (n0 == 0 && wn == 0) *reinterpret_cast<f32x4*>(a.fin + (size_t)(m0 + wm * 128) * 2 + ln * 4) = fin4;  // for the residual epilogue of the next GEMM
    }
    const char* sl = mrs + fr * 8;
    const size_t crs = a.cblock ? 64 : (size_t)a.ldc;
    bf16_t* cp = a.C + c_index(a, m0 + wm * 128 + prow, n0 + wn * 64) + c8;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        const f32x2_t st = *reinterpret_cast<const f32x2_t*>(sl + mi * 128);
        const float mu = st[0], rs = st[1];
        f32x2 nrm = {-rs * mu, -rs * mu}, rs2 = {rs, rs};
        SC_OPAQUE_PAIR(nrm);  // broadcasts as real register pairs, see SC_OPAQUE_PAIR
        SC_OPAQUE_PAIR(rs2);
#pragma unroll
        for (int ni = 0; ni < (EPI == EPI_LNA_BIAS_ROPE ? 0 : 4); ++ni) {  // (the rotary form keeps all four ni in registers: below)
            // rs (acc - mu c1) + c2  as  rs acc + (c2 - rs mu c1): two packed FMAs per pair of values (the epilogue is VALU bound: every
            // op per value costs ~0.55 us per tile)
            const f32x2 d01 = __builtin_elementwise_fma(nrm, f32x2{c1v[ni][0], c1v[ni][1]}, f32x2{c2v[ni][0], c2v[ni][1]});
            const f32x2 d23 = __builtin_elementwise_fma(nrm, f32x2{c1v[ni][2], c1v[ni][3]}, f32x2{c2v[ni][2], c2v[ni][3]});
            const f32x2 v01 = __builtin_elementwise_fma(rs2, f32x2{acc[ni][mi][0], acc[ni][mi][1]}, d01);
            const f32x2 v23 = __builtin_elementwise_fma(rs2, f32x2{acc[ni][mi][2], acc[ni][mi][3]}, d23);
            f32x4 v = {v01[0], v01[1], v23[0], v23[1]};
            if (EPI == EPI_LNA_GELU) {
                const f32x2 g0 = gelu_erf_fast2(f32x2{v[0], v[1]}), g1 = gelu_erf_fast2(f32x2{v[2], v[3]});
                v = f32x4{g0[0], g0[1], g1[0], g1[1]};
            }
            *reinterpret_cast<u32x2*>(stg + fr * T_EPI_ROW + (ni * 16 + 4 * fq) * 2) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        }
        if constexpr (EPI == EPI_LNA_BIAS_ROPE) {
            f32x4 v[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const f32x2 d01 = __builtin_elementwise_fma(nrm, f32x2{c1v[ni][0], c1v[ni][1]}, f32x2{c2v[ni][0], c2v[ni][1]});
                const f32x2 d23 = __builtin_elementwise_fma(nrm, f32x2{c1v[ni][2], c1v[ni][3]}, f32x2{c2v[ni][2], c2v[ni][3]});
                const f32x2 v01 = __builtin_elementwise_fma(rs2, f32x2{acc[ni][mi][0], acc[ni][mi][1]}, d01);
                const f32x2 v23 = __builtin_elementwise_fma(rs2, f32x2{acc[ni][mi][2], acc[ni][mi][3]}, d23);
                v[ni] = f32x4{v01[0], v01[1], v23[0], v23[1]};
            }
            if (n0 + wn * 64 < a.rope_ncols) {  // wave-uniform: this wave's head belongs to Q or K
                const size_t p = (size_t)((m0 + wm * 128 + mi * 16 + fr) & a.rope_smask) * 32 + 4 * fq;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x4 cs = *reinterpret_cast<const f32x4*>(a.rope_cos + p + 16 * h);
                    const f32x4 sn = *reinterpret_cast<const f32x4*>(a.rope_sin + p + 16 * h);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float x = v[h][c], y = v[h + 2][c];
                        v[h][c] = fmaf(x, cs[c], -(y * sn[c]));
                        v[h + 2][c] = fmaf(y, cs[c], x * sn[c]);
                    }
                }
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                *reinterpret_cast<u32x2*>(stg + fr * T_EPI_ROW + (ni * 16 + 4 * fq) * 2) = u32x2{pack_bf16x2(v[ni][0], v[ni][1]), pack_bf16x2(v[ni][2], v[ni][3])};
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const u32x4 o = *reinterpret_cast<const u32x4*>(stg + (j * 8 + prow) * T_EPI_ROW + c8 * 2);
            bf16_t* dst = cp + (size_t)(mi * 16 + j * 8) * crs;
            if (a.nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(o) : "memory");
            else *reinterpret_cast<u32x4*>(dst) = o;
        }
    }
}

// EPI_RESLN_STATS: out = acc + bias[n] + (r - mu_m) rs_m gam[n]   (r = the raw pre-LayerNorm residual, bias already holds + beta),
// and the partial sums (sum, sum of squares) of this tile's 256 columns of the bf16-ROUNDED output, per row, into stats_out.
template <bool COOP = false>
static __device__ __forceinline__ void gemm256_epilogue_resln(const GemmArgs& a, int m0, int n0, char* smem, int w, int lane, f32x4 (&acc)[4][8]) {
    const int wm = w >> 2, wn = w & 3;
    int ln = lane;
    asm volatile("" : "+v"(ln));
    __builtin_amdgcn_sched_barrier(0);
    const int fr = ln & 15, fq = ln >> 4;
    const int prow = ln >> 3, c8 = (ln & 7) * 8;
    char* stg = smem + 4 * T_TILE_BYTES + w * (16 * T_EPI_ROW);
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    f32x4 bias4[4], gam4[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        bias4[ni] = *reinterpret_cast<const f32x4*>(a.bias + n0 + wn * 64 + ni * 16 + 4 * fq);
        gam4[ni] = *reinterpret_cast<const f32x4*>(a.gam + n0 + wn * 64 + ni * 16 + 4 * fq);
    }
    if (COOP) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");  // every wave's pieces of the residual tile + this wave's row statistics
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // residual tile + row statistics have landed
    f32x2_t st[8];  // (mu, rs) of this lane's 8 rows: out of the staging slice before it is written
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) st[mi] = *reinterpret_cast<const f32x2_t*>(stg + (mi * 16 + fr) * 8);
    const char* rlds = smem + w * 16384 + fr * 128 + (fq & 1) * 8;
    const int swz = (fr >> 1) & 7;
    auto read_res = [&](int mi, u32x2 (&dst)[4]) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) dst[ni] = *reinterpret_cast<const u32x2*>(rlds + mi * 2048 + (((ni * 2 + (fq >> 1)) ^ swz) << 4));
    };
    u32x2 rr[2][4];  // residual of row block mi (one ahead: LDS reads cannot be moved across the staging writes by the compiler)
    read_res(0, rr[0]);
    float sum1[8], sum2[8];
    const size_t crs = a.cblock ? 64 : (size_t)a.ldc;
    bf16_t* cp = a.C + c_index(a, m0 + wm * 128 + prow, n0 + wn * 64) + c8;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        if (mi + 1 < 8) read_res(mi + 1, rr[(mi + 1) & 1]);
        f32x2 nmu2 = {-st[mi][0], -st[mi][0]}, rs2 = {st[mi][1], st[mi][1]};
        SC_OPAQUE_PAIR(nmu2);  // broadcasts as real register pairs, see SC_OPAQUE_PAIR
        SC_OPAQUE_PAIR(rs2);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const u32x2 r2 = rr[mi & 1][ni];
            const f32x2 rv01 = {__builtin_bit_cast(float, r2[0] << 16), __builtin_bit_cast(float, r2[0] & 0xFFFF0000u)};
            const f32x2 rv23 = {__builtin_bit_cast(float, r2[1] << 16), __builtin_bit_cast(float, r2[1] & 0xFFFF0000u)};
            const f32x2 v01 = __builtin_elementwise_fma(rv01 + nmu2, rs2 * f32x2{gam4[ni][0], gam4[ni][1]},
                                                        f32x2{acc[ni][mi][0], acc[ni][mi][1]} + f32x2{bias4[ni][0], bias4[ni][1]});
            const f32x2 v23 = __builtin_elementwise_fma(rv23 + nmu2, rs2 * f32x2{gam4[ni][2], gam4[ni][3]},
                                                        f32x2{acc[ni][mi][2], acc[ni][mi][3]} + f32x2{bias4[ni][2], bias4[ni][3]});
            const f32x4 v = {v01[0], v01[1], v23[0], v23[1]};
            const uint32_t p0 = pack_bf16x2(v[0], v[1]), p1 = pack_bf16x2(v[2], v[3]);
            *reinterpret_cast<u32x2*>(stg + fr * T_EPI_ROW + (ni * 16 + 4 * fq) * 2) = u32x2{p0, p1};
            // statistics of what the consumer will read: the rounded values
            const float y0 = __builtin_bit_cast(float, p0 << 16), y1 = __builtin_bit_cast(float, p0 & 0xFFFF0000u);
            const float y2 = __builtin_bit_cast(float, p1 << 16), y3 = __builtin_bit_cast(float, p1 & 0xFFFF0000u);
            s1 += (y0 + y1) + (y2 + y3);
            s2 = fmaf(y0, y0, fmaf(y1, y1, fmaf(y2, y2, fmaf(y3, y3, s2))));
        }
        sum1[mi] = s1;
        sum2[mi] = s2;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const u32x4 o = *reinterpret_cast<const u32x4*>(stg + (j * 8 + prow) * T_EPI_ROW + c8 * 2);
            bf16_t* dst = cp + (size_t)(mi * 16 + j * 8) * crs;
            if (a.nt) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(dst), "v"(o) : "memory");
            else *reinterpret_cast<u32x4*>(dst) = o;
        }
    }
    // row sums: over this lane's 16 columns (above), the 4 k-groups of the wave (lanes fr + 16 fq), then the 4 waves of the row
    // half through LDS -- a fixed order, so the statistics (and everything downstream) are reproducible bit for bit
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
        sum1[mi] += __shfl_xor(sum1[mi], 16, 64);
        sum2[mi] += __shfl_xor(sum2[mi], 16, 64);
        sum1[mi] += __shfl_xor(sum1[mi], 32, 64);
        sum2[mi] += __shfl_xor(sum2[mi], 32, 64);
    }
    float* part = reinterpret_cast<float*>(smem + w * 16384);  // this wave's residual slice is dead: [128 rows][2]
    if (fq == 0) {
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) *reinterpret_cast<f32x2_t*>(part + (mi * 16 + fr) * 2) = f32x2_t{sum1[mi], sum2[mi]};
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // raw barrier: __syncthreads() would also wait for the C stores
    if (wn == 0) {  // waves 0 and 4: rows 2 ln, 2 ln + 1 of their half, summed over the four column blocks in wave order
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 4; ++v) t += *reinterpret_cast<const f32x4*>(smem + (wm * 4 + v) * 16384 + ln * 16);
        float* out = a.stats_out + ((size_t)(n0 / T_BN) * a.M + m0 + wm * 128) * 2 + ln * 4;
        *reinterpret_cast<f32x4*>(out) = t;
    }
}

// diagnostic time stamps (100 MHz wall clock): slot 0 = HW_ID, 1 = XCC_ID, 2.. = stamps
static __device__ __forceinline__ void gemm256_stamp(const GemmArgs& a, int tile, int slot) {
    if (a.trace && threadIdx.x == 0) {
        a.trace[(size_t)tile * 8 + slot] = (unsigned long long)wall_clock64();
        // slots 6 / 7: the shader clock (s_memtime) next to stamps 2 / 3 -- cycles of the main loop, and with the 100 MHz stamps the clock it ran at
        if (slot == 2 || slot == 3) a.trace[(size_t)tile * 8 + slot + 4] = (unsigned long long)__builtin_readcyclecounter();
    }
}

// PP = 0: the one-barrier main loop; 2..5: the ping-pong main loop with that many half-tiles in flight (gemm_tile.h)
template <int PP, int ML, class Hook>
static __device__ __forceinline__ void gemm256_mainloop_sel(const GemmArgs& a, int lda, int m0, int n0, char* smem, f32x4 (&acc)[4][8], int w, int lane, Hook hook,
                                                            size_t a_kstep) {
    if constexpr (PP > 0) gemm_tile256_mainloop_pp<PP, ML, Hook>(a.A, lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, lane, hook, a_kstep);
    else gemm_tile256_mainloop<ML, Hook>(a.A, lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, lane, hook, a_kstep);
}

template <int EPI, int DBG = 0, int PP = 0>
__global__ __launch_bounds__(512) void gemm256_bf16_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 128 KiB pipeline buffers + epilogue staging
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (a.trace && threadIdx.x == 0) {
        a.trace[(size_t)blockIdx.x * 8 + 0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID
        a.trace[(size_t)blockIdx.x * 8 + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
    }
    gemm256_stamp(a, blockIdx.x, 2);
    int m0, n0;
    tile_coords256(a, blockIdx.x, m0, n0);
    f32x4 acc[4][8];  // [ni][mi]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // DBG bits: 1 no in-loop DMA, 2 no MFMA, 4 no epilogue, 16 no fragment reads (ablations, outputs meaningless);
    constexpr int ML = (DBG & 3) | ((DBG & 16) ? 4 : 0);
    const int lda = a.ablock ? 64 : a.lda;
    const size_t a_kstep = a.ablock ? (size_t)a.M * 64 : (size_t)G_BK;
    constexpr bool COOP = PP > 0;  // ping-pong loop: the residual tile comes through the ring
    if (EPI == EPI_BIAS_RES && !(DBG & 31)) {
        if constexpr (COOP)
            gemm256_mainloop_sel<PP, ML>(a, lda, m0, n0, smem, acc, w, lane, ResidualCoopHook{a.R + (size_t)m0 * a.ldr + n0, a.ldr, w, lane, smem}, a_kstep);
        else
            gemm256_mainloop_sel<PP, ML>(a, lda, m0, n0, smem, acc, w, lane, ResidualTailHook{a.R + (size_t)m0 * a.ldr + n0, a.ldr, w, lane, smem}, a_kstep);
    } else if (EPI == EPI_RESLN_STATS) {
        if constexpr (COOP)
            gemm256_mainloop_sel<PP, ML>(a, lda, m0, n0, smem, acc, w, lane,
                                         ResLnCoopHook{ResidualCoopHook{a.R + (size_t)m0 * a.ldr + n0, a.ldr, w, lane, smem},
                                                       a.fin + (size_t)(m0 + (w >> 2) * 128) * 2}, a_kstep);
        else
            gemm256_mainloop_sel<PP, ML>(a, lda, m0, n0, smem, acc, w, lane,
                                         ResLnTailHook{ResidualTailHook{a.R + (size_t)m0 * a.ldr + n0, a.ldr, w, lane, smem},
                                                       a.fin + (size_t)(m0 + (w >> 2) * 128) * 2}, a_kstep);
    }
    else if (EPI == EPI_LNA_BIAS || EPI == EPI_LNA_GELU || EPI == EPI_LNA_BIAS_ROPE)
        gemm256_mainloop_sel<PP, ML>(a, lda, m0, n0, smem, acc, w, lane,
                                     LnaTailHook{a.stats_in + (size_t)(m0 + (w >> 2) * 128) * 2, (size_t)a.M * 2, a.stat_slots, w, lane, smem}, a_kstep);
    else
        gemm256_mainloop_sel<PP, ML>(a, lda, m0, n0, smem, acc, w, lane, NoTailHook{}, a_kstep);
    gemm256_stamp(a, blockIdx.x, 3);
    if (DBG & 4) {  // diagnostic: no epilogue, keep the accumulators alive
        float sink = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) sink += acc[i][j][0] + acc[i][j][3];
        if (sink == 12345.678f) a.C[0] = 1;
        return;
    }
    if (EPI == EPI_RESLN_STATS) gemm256_epilogue_resln<COOP>(a, m0, n0, smem, w, lane, acc);
    else if (EPI == EPI_LNA_BIAS || EPI == EPI_LNA_GELU || EPI == EPI_LNA_BIAS_ROPE) gemm256_epilogue_lna<EPI>(a, m0, n0, smem, w, lane, acc, smem + w * 16384);
    else gemm256_epilogue<EPI, COOP && !(DBG & 31)>(a, m0, n0, smem, w, lane, acc);
    if (a.trace) {
        gemm256_stamp(a, blockIdx.x, 4);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        gemm256_stamp(a, blockIdx.x, 5);
    }
}

// ---- strip walk of the EPI_LNA_* GEMMs: one workgroup takes `strip` consecutive column tiles of ONE row panel, in order, and the
// LDS ring never drains between them (scan_coarse.hip's persistent form, gemm_tile.h "persistent use"): every tile but the last hands
// PPNextTileHook to the loop, which requests the first two K-tiles of the next tile (same A rows, W rows n0 + 256 ...) into the
// slots that fall free, and every tile but the first starts behind that prefetch (PREF).  K is a multiple of 256, so a tile is a
// multiple of 4 K-tiles and the ring parity stays 0.
// All tiles of a strip have the same rows: the row statistics are loaded and finalised ONCE, before the first tile, and parked in
// 1 KiB per wave behind the epilogue staging area.  The epilogue then neither fetches (no LnaTailHook: the tail phases belong to the
// prefetch) nor waits nor finalises, and it never touches the ring, which holds the next tile by then.  Its C stores are younger
// than the prefetched pieces, which only makes the next tile's first wait conservative (gemm_tile.h).
// A is row-major [M][lda] (no caller hands blocked A to an EPI_LNA_* GEMM; the launcher keeps such a launch on the per-tile kernel).
// No per-lane value lives across tiles (the hook is all scalars; everything else is re-derived per tile from the lane id).
#define T_STRIP_LDS_BYTES (T_LDS_BYTES + 8 * 1024)
template <int EPI, int PP>
__global__ __launch_bounds__(512) void gemm256_strip_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 128 KiB ring + epilogue staging + 8 x 1 KiB (mu, rs)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // strips of one row panel are consecutive logical ids: they share the A panel in one XCD's L2 (xcd_remap)
    const int spp = (a.tiles_n + a.strip - 1) / a.strip;
    const int sid = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = sid / spp;
    const int m0 = __builtin_amdgcn_readfirstlane(mt * T_BM);
    const int t0 = __builtin_amdgcn_readfirstlane((sid - mt * spp) * a.strip);
    const int t1 = t0 + a.strip < a.tiles_n ? t0 + a.strip : a.tiles_n;
    char* mrs = smem + T_LDS_BYTES + w * 1024;
    {   // lane ln: rows 2 ln, 2 ln + 1 of the wave's 128; slots summed in order t = 0, 1, ... as the per-tile epilogue does
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const float* st = a.stats_in + (size_t)(m0 + (w >> 2) * 128) * 2 + ln * 4;
        f32x4 sacc = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < a.stat_slots; ++t) sacc += *reinterpret_cast<const f32x4*>(st + (size_t)t * a.M * 2);
        const f32x4 fin4 = lna_finalise(a, sacc);
        *reinterpret_cast<f32x4*>(mrs + ln * 16) = fin4;
        if (t0 == 0 && (w & 3) == 0) *reinterpret_cast<f32x4*>(a.fin + (size_t)(m0 + (w >> 2) * 128) * 2 + ln * 4) = fin4;
    }
    const int lda = a.lda;  // A is row-major here (the launcher keeps blocked A on the per-tile kernel)
    const size_t a_kstep = G_BK;
    PPNextTileHook hook;
    hook.a_kbytes = (uint32_t)(G_BK * 2); hook.a1_off = (uint32_t)(64 * lda * 2); hook.w1_off = (uint32_t)(32 * a.ldw * 2);
    hook.w = w; hook.smem = smem;
    hook.ra = __builtin_amdgcn_make_buffer_rsrc((void*)(a.A + (size_t)m0 * lda), 0, -1, 0x00020000);
#pragma unroll 1
    for (int t = t0; t < t1; ++t) {
        const int n0 = __builtin_amdgcn_readfirstlane(t * T_BN);
        const bool first = t == t0, last = t + 1 == t1;
        int ln = lane;
        asm volatile("" : "+v"(ln));  // the loop's per-lane addresses are derived again for every tile instead of living across the epilogue
        hook.rw = __builtin_amdgcn_make_buffer_rsrc((void*)(a.W + (size_t)(last ? n0 : n0 + T_BN) * a.ldw), 0, -1, 0x00020000);
        f32x4 acc[4][8];  // [ni][mi]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (first) {
            if (last) gemm_tile256_mainloop_pp<PP, 0, NoTailHook, false, false>(a.A, lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, ln, NoTailHook{}, a_kstep);
            else gemm_tile256_mainloop_pp<PP, 0, PPNextTileHook, false, false>(a.A, lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, ln, hook, a_kstep);
        } else {
            if (last) gemm_tile256_mainloop_pp<PP, 0, NoTailHook, false, true>(a.A, lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, ln, NoTailHook{}, a_kstep);
            else gemm_tile256_mainloop_pp<PP, 0, PPNextTileHook, false, true>(a.A, lda, m0, a.W, a.ldw, n0, a.K, smem, acc, w, ln, hook, a_kstep);
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        gemm256_epilogue_lna<EPI, true>(a, m0, n0, smem, w, lane, acc, mrs);
    }
}

// ---- diagnostic: the int8 variant of the 256 tile main loop (scan_coarse.hip's coarse stage) on its own, raw i32 accumulators out.
// The A/B lane maps of v_mfma_i32_16x16x64_i8 are not documented in the guide ("check the map with exact integer data"): this
// kernel is that check -- C[m][n] = sum_k A[m][k] * W[n][k] must hold exactly.
__global__ __launch_bounds__(512) void gemm256_i8_diag_kernel(const int8_t* __restrict__ A, const int8_t* __restrict__ W, int32_t* __restrict__ C, int M, int N,
                                                               int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles_n = N / T_BN;
    const int m0 = ((int)blockIdx.x / tiles_n) * T_BM, n0 = ((int)blockIdx.x % tiles_n) * T_BN;
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm_tile256_mainloop<0, NoTailHook, true>(reinterpret_cast<const bf16_t*>(A), K / 2, m0, reinterpret_cast<const bf16_t*>(W), K / 2, n0, K / 2, smem, acc, w, lane);
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int wm = w >> 2, wn = w & 3, fr = ln & 15, fq = ln >> 4;
    int32_t* out = C + (size_t)(m0 + wm * 128 + fr) * N + n0 + wn * 64 + 4 * fq;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) *reinterpret_cast<f32x4*>(out + (size_t)(mi * 16) * N + ni * 16) = acc[ni][mi];
}
void sc_launch_gemm_i8_diag(const void* A, const void* W, void* C, int M, int N, int K, hipStream_t s) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(gemm256_i8_diag_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T_LDS_BYTES); });
    hipLaunchKernelGGL(gemm256_i8_diag_kernel, dim3((unsigned)((M / T_BM) * (N / T_BN))), dim3(512), T_LDS_BYTES, s, (const int8_t*)A, (const int8_t*)W, (int32_t*)C, M, N, K);
}

// M, N multiples of 128; K multiple of 64; all leading dimensions multiples of 8 elements.
bool sc_gemm_bf16_supported(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && (M % G_BM) == 0 && (N % G_BN) == 0 && (K % G_BK) == 0; }

// -1 = by shape: weights that fit the L2s (the encoder's, <= 4.7 MB) walk row panel by row panel (with non-temporal C stores the
// A panel then stays cached for all of its column tiles: encoder 19.50k -> 19.66k chunks/s in a same-box A/B); larger W walks
// column-major inside groups of 8 row panels, which bounds the W re-reads (profiles/r1n_gemm_tile_order.log).  Both XCD-remapped.
static int g_gemm_order = -1;
void sc_gemm_set_order(int v) { g_gemm_order = v < 0 ? -1 : v; }
static unsigned long long* g_gemm_trace = nullptr;
void sc_gemm_set_trace(unsigned long long* dev) { g_gemm_trace = dev; }
static int g_gemm_dbg = 0;
void sc_gemm_set_debug(int v) { g_gemm_dbg = v; }
static bool g_force_tile128 = false;
void sc_gemm_force_tile128(bool on) { g_force_tile128 = on; }

// ---- split-K for small M (a single query or a handful of chunks): with M = 256 a GEMM has 3..12 tiles for 256 CUs and each
// walks its whole K loop alone (1.7 us per K-tile: 20 us at K = 768, 80 us at K = 3072 -> 1.7 ms per embed_query).  Here
// tile x K-slice pairs fill the chip, each workgroup writes its raw f32 accumulators, and a second, element-wise kernel
// sums the slices and applies the epilogue (same formulas as gemm256_epilogue, one bf16 rounding).
__global__ __launch_bounds__(512) void gemm256_splitk_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = (int)blockIdx.x / a.splitk, slice = (int)blockIdx.x - tile * a.splitk;
    const int mt = tile / a.tiles_n, nt = tile - mt * a.tiles_n;
    const int m0 = __builtin_amdgcn_readfirstlane(mt * T_BM), n0 = __builtin_amdgcn_readfirstlane(nt * T_BN);
    const int kslice = a.K / a.splitk, k0 = slice * kslice;
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm_tile256_mainloop<0>(a.A + k0, a.lda, m0, a.W + k0, a.ldw, n0, kslice, smem, acc, w, lane);
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int wm = w >> 2, wn = w & 3, fr = ln & 15, fq = ln >> 4;
    float* out = a.partial + ((size_t)slice * a.M + m0 + wm * 128 + fr) * a.N + n0 + wn * 64 + 4 * fq;
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) *reinterpret_cast<f32x4*>(out + (size_t)(mi * 16) * a.N + ni * 16) = acc[ni][mi];
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(GemmArgs a) {
    const int64_t quads = (int64_t)a.M * (a.N / 4);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        const int64_t m = i / (a.N / 4);
        const int n = (int)(i - m * (a.N / 4)) * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(a.bias + n);
        for (int sidx = 0; sidx < a.splitk; ++sidx) v += *reinterpret_cast<const f32x4*>(a.partial + ((size_t)sidx * a.M + m) * a.N + n);
        if (EPI == EPI_BIAS_GELU) {
            const f32x2 g0 = gelu_erf_fast2(f32x2{v[0], v[1]}), g1 = gelu_erf_fast2(f32x2{v[2], v[3]});
            v = f32x4{g0[0], g0[1], g1[0], g1[1]};
        }
        if (EPI == EPI_BIAS_RES) {
            const u16x4 rv = *reinterpret_cast<const u16x4*>(a.R + (size_t)m * a.ldr + n);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(rv[r]);
        }
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<u32x2*>(a.C + c_index(a, m, n)) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
    }
}

// K slices for a GEMM whose tiles alone would leave most CUs idle: the largest divisor of the K-tile count that keeps at least
// 3 K-tiles per slice and tiles * slices within the CU count (1 = do not split)
int sc_gemm_splitk_factor(int M, int N, int K, int cus) {
    if ((M % T_BM) || (N % T_BN) || M > 1024) return 1;
    const int tiles = (M / T_BM) * (N / T_BN), nk = K / G_BK;
    int best = 1;
    for (int d = 2; d <= nk; ++d)
        if (nk % d == 0 && nk / d >= 3 && tiles * d <= cus) best = d;
    return tiles * 2 <= cus ? best : 1;
}

// main loop of the 256-tile kernels: 0 = one barrier per K-tile, 2..5 = ping-pong with that many half-tiles in flight (SC_GEMM_PP)
static int g_gemm_pp = -1;
void sc_gemm_set_pp(int v) { g_gemm_pp = v; }
static int gemm_pp() {
    static const char* env = getenv("SC_GEMM_PP");
    return g_gemm_pp >= 0 ? g_gemm_pp : env ? atoi(env) : SC_GEMM_PP_DEFAULT;
}
// non-temporal C stores of the 256-tile kernels ("gemm_nt" of sc_diag_set_option): -1 = outputs of 64 MiB and more (or SC_GEMM_NT),
// 0 = never, 1 = always -- so that a small test shape can take the store path of the batch step
static int g_gemm_nt = -1;
void sc_gemm_set_nt(int v) { g_gemm_nt = v < 0 ? -1 : (v ? 1 : 0); }
static int gemm_nt(int M, int N) {
    static const char* env_nt = getenv("SC_GEMM_NT");
    return g_gemm_nt >= 0 ? g_gemm_nt : env_nt ? atoi(env_nt) : ((size_t)M * (size_t)N * 2 >= ((size_t)64 << 20));
}
// main loop a 256-tile launch of depth K gets: a single K-tile has no ring to ping-pong through
static int gemm_pp_for(int K) { return K >= 2 * G_BK ? gemm_pp() : 0; }

// Which kernel sc_launch_gemm_bf16 runs for a shape under the current options, as host arithmetic: the launcher dispatches on this and
// keeps the last one (sc_diag_gemm_path; tests assert the path they name).  scratch_bytes = the split-K scratch on offer (0 = none).
// The 128-tile kernel has no walk order, ring or non-temporal stores (order 0, pp 0, nt 0); the split-K pair walks row-major without
// the XCD remap (order 1) on the one-barrier loop and stores plainly.
static ScGemmPath g_gemm_last = {0, 1, 0, 0, 0};
ScGemmPath sc_gemm_last_path(void) { return g_gemm_last; }
ScGemmPath sc_gemm_plain_path(int M, int N, int K, int cus, size_t scratch_bytes) {
    if ((M % T_BM) || (N % T_BN) || g_force_tile128) return ScGemmPath{G_BM, 1, 0, 0, 0};
    if (scratch_bytes && !g_gemm_dbg && !g_gemm_trace) {
        const int d = sc_gemm_splitk_factor(M, N, K, cus);
        if (d > 1 && (size_t)d * M * N * sizeof(float) <= scratch_bytes) return ScGemmPath{T_BM, d, 1, 0, 0};
    }
    static const char* env_order = getenv("SC_GEMM_ORDER");  // A/B experiments
    const int order = env_order ? atoi(env_order) : g_gemm_order >= 0 ? g_gemm_order : ((size_t)N * (size_t)K * 2 <= ((size_t)8 << 20) ? 0 : 16);
    return ScGemmPath{T_BM, 1, order, gemm_pp_for(K) ? 4 : 0, gemm_nt(M, N) ? 1 : 0};
}

// Strip walk of the EPI_LNA_* GEMMs ("gemm_strip" of sc_diag_set_option, SC_GEMM_STRIP): -1 = by shape, 0 = one workgroup per tile,
// L >= 1 = L column tiles per workgroup (clamped to the tiles of a row panel).  "gemm_strip_n" (scripts/strip_sweep.py) restricts a
// forced value to the launches with that N; the others then run one workgroup per tile, so that a sweep measures one shape alone.  A strip needs the ping-pong loop, a row-major A and
// no trace / ablation mode (the strip kernel has neither stamps nor DBG forms).
static int g_gemm_strip = -1, g_gemm_strip_n = 0, g_gemm_strip_last = 0;
void sc_gemm_set_strip(int v) { g_gemm_strip = v < 0 ? -1 : v; }
void sc_gemm_set_strip_n(int v) { g_gemm_strip_n = v > 0 ? v : 0; }
int sc_gemm_last_strip(void) { return g_gemm_strip_last; }
// The shape rule (host arithmetic only: tests/test_gemm_strip_host.py).  Lengths that won a same-box A/B of the encoder step
// (profiles/strip_ab.log): QKV (9 tiles, K = 768) 3, FFN1 (12 tiles, K = 768) 6; no other shape has been measured.  A strip makes
// the scheduling quantum L tiles instead of one, so the rule also counts rounds: with `cus` workgroups side by side the strips
// take ceil(strips / cus) * L tile-times and the per-tile kernel ceil(tiles / cus); a strip is chosen only where it needs no more
// (M = 32768: QKV would need 6 tile-times against 5 and measured 1 % slower -> per-tile; FFN1 needs 6 against 6 and measured
// 1.7 % faster), and only with at least one strip per CU.
int sc_gemm_strip_rule(int M, int N, int K, int cus) {
    if (M <= 0 || (M % T_BM) || N <= 0 || (N % T_BN) || K != 768 || cus <= 0) return 0;
    const int tiles_n = N / T_BN, L = tiles_n == 9 ? 3 : tiles_n == 12 ? 6 : 0;
    if (!L) return 0;
    const int64_t panels = M / T_BM, strips = panels * (tiles_n / L), tiles = panels * tiles_n;
    if (strips < (int64_t)cus) return 0;
    return ((strips + cus - 1) / cus) * L <= (tiles + cus - 1) / cus ? L : 0;
}
// what sc_launch_gemm_bf16_ln does with an EPI_LNA_* launch of this shape under the current options: tiles per strip, 0 = per-tile
int sc_gemm_strip_tiles(int M, int N, int K, int cus, bool a_blocked) {
    static const char* env = getenv("SC_GEMM_STRIP");
    if (K < 256 || gemm_pp() == 0 || a_blocked || g_gemm_trace || g_gemm_dbg) return 0;
    int v = g_gemm_strip >= 0 ? g_gemm_strip : env ? atoi(env) : -1;
    if (v >= 0 && g_gemm_strip_n && N != g_gemm_strip_n) v = 0;
    if (v < 0) v = sc_gemm_strip_rule(M, N, K, cus);
    return std::min(v, N / T_BN);
}
template <int EPI>
static void launch256_strip(GemmArgs a, int strip, hipStream_t s) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(gemm256_strip_kernel<EPI, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T_STRIP_LDS_BYTES); });
    a.strip = strip;
    const unsigned grid = (unsigned)((a.M / T_BM) * ((a.tiles_n + strip - 1) / strip));
    hipLaunchKernelGGL((gemm256_strip_kernel<EPI, 4>), dim3(grid), dim3(512), T_STRIP_LDS_BYTES, s, a);
}
template <int EPI, int DBG, int PP>
static void launch256_pp(const GemmArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    static ScDeviceOnce once;  // one per instantiation (and device)
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(gemm256_bf16_kernel<EPI, DBG, PP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T_LDS_BYTES); });
    hipLaunchKernelGGL((gemm256_bf16_kernel<EPI, DBG, PP>), grid, block, T_LDS_BYTES, s, a);  // 128 KiB pipeline + 18 KiB epilogue staging
}
template <int EPI, int DBG>
static void launch256(const GemmArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    const int pp = gemm_pp_for(a.K);
    if (pp == 0) return launch256_pp<EPI, DBG, 0>(a, grid, block, s);
    if constexpr (DBG == 4) {  // other depths: only as the no-epilogue diagnostic
        if (pp == 3) return launch256_pp<EPI, DBG, 3>(a, grid, block, s);
        if (pp == 5) return launch256_pp<EPI, DBG, 5>(a, grid, block, s);
    }
    launch256_pp<EPI, DBG, 4>(a, grid, block, s);
}
template <int DBG>
static void launch256_epi(int epi, const GemmArgs& a, dim3 grid, dim3 block, hipStream_t s) {
    if (epi == EPI_BIAS_GELU) launch256<EPI_BIAS_GELU, DBG>(a, grid, block, s);
    else if (epi == EPI_BIAS_RES) launch256<EPI_BIAS_RES, DBG>(a, grid, block, s);
    else launch256<EPI_BIAS, DBG>(a, grid, block, s);
}

// LayerNorm-folded GEMMs of the batch pipeline (sc_encoder.cpp): M, N multiples of 256, K a multiple of 256 for EPI_LNA_* (the
// statistics come in one slot per 256 columns of A).  epi = EPI_LNA_BIAS / EPI_LNA_GELU: bias = c2; EPI_RESLN_STATS: bias = b + beta.
bool sc_gemm_ln_supported(int M, int N, int K) { return M > 0 && (M % T_BM) == 0 && (N % T_BN) == 0 && (K % 256) == 0; }
void sc_launch_gemm_bf16_ln(int epi, const void* A, int lda, const void* W, int ldw, const float* bias, const void* R, int ldr, void* C, int ldc, int M,
                            int N, int K, hipStream_t s, const float* c1, const float* stats_in, float* fin, const float* gam, float* stats_out, float eps,
                            const float* rope_cos, const float* rope_sin, int rope_S, int rope_ncols) {
    GemmArgs a;
    a.rope_cos = rope_cos; a.rope_sin = rope_sin; a.rope_smask = rope_S - 1; a.rope_ncols = rope_ncols;
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.bias = bias; a.R = (const bf16_t*)R; a.C = (bf16_t*)C;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldr = ldr; a.ldc = ldc;
    a.cblock = ldc == SC_LDC_BLOCKED64 ? 1 : 0;
    a.ablock = lda == SC_LDC_BLOCKED64 ? 1 : 0;
    static const char* env_order = getenv("SC_GEMM_ORDER");
    a.order = env_order ? atoi(env_order) : ((size_t)N * (size_t)K * 2 <= ((size_t)8 << 20) ? 0 : 16);
    a.trace = nullptr;
    a.nt = gemm_nt(M, N);
    a.tiles_n = N / T_BN;
    a.ntiles = (M / T_BM) * a.tiles_n;
    a.splitk = 1;
    a.partial = nullptr;
    a.c1 = c1; a.stats_in = stats_in; a.stat_slots = K / 256; a.fin = fin; a.gam = gam; a.stats_out = stats_out; a.ln_eps = eps;
    dim3 grid((unsigned)a.ntiles), block(512);
    a.strip = 0;
    if (epi != EPI_RESLN_STATS) {
        g_gemm_strip_last = sc_gemm_strip_tiles(M, N, K, sc_device_cus(), a.ablock != 0);
        if (const int strip = g_gemm_strip_last) {
            if (epi == EPI_LNA_BIAS) launch256_strip<EPI_LNA_BIAS>(a, strip, s);
            else if (epi == EPI_LNA_BIAS_ROPE) launch256_strip<EPI_LNA_BIAS_ROPE>(a, strip, s);
            else launch256_strip<EPI_LNA_GELU>(a, strip, s);
            return;
        }
    }
    if (epi == EPI_LNA_BIAS) launch256<EPI_LNA_BIAS, 0>(a, grid, block, s);
    else if (epi == EPI_LNA_BIAS_ROPE) launch256<EPI_LNA_BIAS_ROPE, 0>(a, grid, block, s);
    else if (epi == EPI_LNA_GELU) launch256<EPI_LNA_GELU, 0>(a, grid, block, s);
    else launch256<EPI_RESLN_STATS, 0>(a, grid, block, s);
}

void sc_launch_gemm_bf16(int epi, const void* A, int lda, const void* W, int ldw, const float* bias, const void* R, int ldr, void* C,
                         int ldc, int M, int N, int K, hipStream_t s, void* splitk_scratch, size_t splitk_scratch_bytes) {
    GemmArgs a;
    a.c1 = nullptr; a.stats_in = nullptr; a.stat_slots = 0; a.fin = nullptr; a.gam = nullptr; a.stats_out = nullptr; a.ln_eps = 0.f;
    a.rope_cos = nullptr; a.rope_sin = nullptr; a.rope_smask = 0; a.rope_ncols = 0;
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.bias = bias; a.R = (const bf16_t*)R; a.C = (bf16_t*)C;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldr = ldr; a.ldc = ldc;
    a.cblock = ldc == SC_LDC_BLOCKED64 ? 1 : 0;
    a.ablock = lda == SC_LDC_BLOCKED64 ? 1 : 0;
    const ScGemmPath p = sc_gemm_plain_path(M, N, K, splitk_scratch ? sc_device_cus() : 0, splitk_scratch ? splitk_scratch_bytes : 0);
    // A in 64-column blocks is read by the per-tile 256-tile kernel alone (M % 256 == 0, N % 256 == 0, no split-K scratch): the other
    // kernels would take the sentinel for a leading dimension.  Nothing is launched then, and the record says so (tile 0).
    if (a.ablock && (p.tile != T_BM || p.splitk != 1)) {
        g_gemm_last = ScGemmPath{0, 1, 0, 0, 0};
        return;
    }
    g_gemm_last = p;
    a.order = p.order;
    a.trace = g_gemm_trace;
    a.nt = gemm_nt(M, N);
    if (p.tile == T_BM) {
        a.tiles_n = N / T_BN;
        a.ntiles = (M / T_BM) * a.tiles_n;
        dim3 grid((unsigned)a.ntiles), block(512);
        a.splitk = 1;
        a.strip = 0;
        a.partial = nullptr;
        if (p.splitk > 1) {
            const int d = p.splitk;
            a.splitk = d;
            a.partial = (float*)splitk_scratch;
            static ScDeviceOnce once_sk;
            sc_device_once(once_sk, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(gemm256_splitk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T_LDS_BYTES); });
            hipLaunchKernelGGL(gemm256_splitk_kernel, dim3((unsigned)(a.ntiles * d)), block, T_LDS_BYTES, s, a);
            const int rb = (int)std::min<int64_t>(((int64_t)M * (N / 4) + 255) / 256, 1024);
            if (epi == EPI_BIAS_GELU) hipLaunchKernelGGL(gemm_splitk_reduce_kernel<EPI_BIAS_GELU>, dim3((unsigned)rb), dim3(256), 0, s, a);
            else if (epi == EPI_BIAS_RES) hipLaunchKernelGGL(gemm_splitk_reduce_kernel<EPI_BIAS_RES>, dim3((unsigned)rb), dim3(256), 0, s, a);
            else hipLaunchKernelGGL(gemm_splitk_reduce_kernel<EPI_BIAS>, dim3((unsigned)rb), dim3(256), 0, s, a);
            return;
        }
        switch (g_gemm_dbg) {  // ablations (sc_diag_gemm_bench): results are meaningless
            case 1: launch256<EPI_BIAS, 1>(a, grid, block, s); return;
            case 2: launch256<EPI_BIAS, 2>(a, grid, block, s); return;
            case 4: launch256<EPI_BIAS, 4>(a, grid, block, s); return;
            case 5: launch256<EPI_BIAS, 5>(a, grid, block, s); return;
            case 20: launch256<EPI_BIAS, 20>(a, grid, block, s); return;
            case 21: launch256<EPI_BIAS, 21>(a, grid, block, s); return;
            default: break;
        }
        launch256_epi<0>(epi, a, grid, block, s);
        return;
    }
    a.tiles_n = N / G_BN;
    a.ntiles = (M / G_BM) * a.tiles_n;
    const size_t lds = 4 * G_TILE_BYTES;  // 64 KiB
    static ScDeviceOnce once128;
    sc_device_once(once128, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_kernel<EPI_BIAS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_kernel<EPI_BIAS_GELU>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16_kernel<EPI_BIAS_RES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    dim3 grid((unsigned)a.ntiles), block(256);
    if (epi == EPI_BIAS_GELU) hipLaunchKernelGGL(gemm_bf16_kernel<EPI_BIAS_GELU>, grid, block, lds, s, a);
    else if (epi == EPI_BIAS_RES) hipLaunchKernelGGL(gemm_bf16_kernel<EPI_BIAS_RES>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(gemm_bf16_kernel<EPI_BIAS>, grid, block, lds, s, a);
}
