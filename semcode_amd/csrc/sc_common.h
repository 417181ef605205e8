// sc_common.h -- shared host/device definitions for libsemcode_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/semcode_hip.h"

#include <mutex>
#include <type_traits>

#define SC_WAVE 64
#define SC_LD_ALIGN 64            // corpus row stride is a multiple of 64 floats (256 B)
#define SC_KEY_MAX 0xFFFFFFFFFFFFFFFFull

// sc_launch_gemm_bf16: ldc value that selects the 64-column-blocked output layout C[N / 64][M][64] (gemm_bf16.hip c_index);
// sc_launch_attention reads a QKV buffer of that layout when `blocked` (= that GEMM's M) is non-zero
#define SC_LDC_BLOCKED64 (-64)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short bf16_t;
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }
static __device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    // round to nearest even; NaN stays NaN
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (bf16_t)((u >> 16) | 0x40);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}

__host__ __device__ static inline uint64_t sc_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Irwin-Hall(12) integer-hash N(0,1) approximation; bit-exact twin: oracle/sc_oracle.c sc_oracle_synth.
__host__ __device__ static inline float sc_synth_value(uint64_t key, uint64_t row, uint32_t col, uint32_t dim) {
    const uint64_t ctr = (row * (uint64_t)dim + col) * 3ull;
    int32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        uint64_t h = sc_mix64(key ^ ((ctr + (uint64_t)j) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull));
        sum += (int32_t)(h & 0xFFFF) + (int32_t)((h >> 16) & 0xFFFF) + (int32_t)((h >> 32) & 0xFFFF) + (int32_t)(h >> 48);
    }
    return (float)(sum - 393210) * (1.0f / 65536.0f);
}
__host__ __device__ static inline uint64_t sc_synth_key(uint64_t seed) { return sc_mix64(seed + 0x9E3779B97F4A7C15ull); }

// score from the exact dot product and the two squared norms (metric: sc_metric)
// COSINE, the zero-norm rule (include/semcode_hip.h, "value contract"): a row or a query with |v|^2 == 0 scores exactly +0.0 against
// anything.  dot is +0.0 there (an fmaf chain from +0.0 over products of +-0), so only the 0 / 0 changes: the denominator |x| |q|
// is 0 exactly when one of the norms is, and a floor at the smallest normal float (below every denominator the contract covers)
// turns it into +0.0 / FLT_MIN = +0.0 -- one v_max_f32, no compare, no select, nothing for hipcc to branch around.  The forms
// `(xn == 0 || qn == 0) ? 0 : dot / den` and `dot / (den > 0 ? den : 1)` cost the 10M x 768 COSINE batch 9.4 -> 10.0 and 9.7 ms
// (scan_coarse256_kernel, dense epilogue: 28.5k -> 37.2k / 35.1k instructions).  Bit-exact twin: oracle/sc_oracle.c sc_oracle_score.
#define SC_NORM_FLOOR 1.17549435e-38f
template <int METRIC>
__host__ __device__ static inline float sc_score(float dot, float xn, float qn) {
    if (METRIC == SC_METRIC_L2) return fmaf(-2.0f, dot, xn + qn);
    if (METRIC == SC_METRIC_COSINE) return dot / fmaxf(sqrtf(xn) * sqrtf(qn), SC_NORM_FLOOR);
    return dot;
}
// 1 / |x| of a corpus row for the cosine form of the coarse tests (scan_coarse.hip, scan_coarse64.hip; ivf_coarse.hip guards its
// centred form itself): finite for a zero row, whose coarse dot is exactly 0, so that its coarse score is 0 like its exact one and
// never 0 * inf.  The floor sits on sqrtf(xn) itself -- the very expression of sc_score, which the precise test evaluates next to this
// one: floored inside the root, the dense epilogue computed two roots per score (+16 % instructions, the COSINE batch 9.16 -> 9.36 ms)
__host__ __device__ static inline float sc_inv_norm(float xn) { return 1.0f / fmaxf(sqrtf(xn), 1.0e-19f); }

// 64-bit total order, smaller = better: (order-preserving float map of +-score) << 32 | row
template <int METRIC>
__host__ __device__ static inline uint64_t sc_make_key(float score, uint32_t row) {
    float v = (METRIC == SC_METRIC_L2) ? score : -score;
    v = v + 0.0f;
    uint32_t u = __builtin_bit_cast(uint32_t, v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | row;
}
__host__ __device__ static inline float sc_key_score(int metric, uint64_t key) {
    uint32_t u = (uint32_t)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float v = __builtin_bit_cast(float, u);
    return (metric == SC_METRIC_L2) ? v : -v;
}

// Calls f with the metric as a compile-time constant (std::integral_constant<int, SC_METRIC_...>): the one place where a launcher
// turns its run-time `metric` into the METRIC template argument of a kernel.  Anything that is not L2 or COSINE is IP.
//   sc_dispatch_metric(metric, [&](auto m) { hipLaunchKernelGGL(some_kernel<m.value>, grid, block, 0, s, ...); });
template <class F>
static inline void sc_dispatch_metric(int metric, F&& f) {
    if (metric == SC_METRIC_L2) f(std::integral_constant<int, SC_METRIC_L2>{});
    else if (metric == SC_METRIC_COSINE) f(std::integral_constant<int, SC_METRIC_COSINE>{});
    else f(std::integral_constant<int, SC_METRIC_IP>{});
}

// One-time, PER-DEVICE setup at a launch site.  hipFuncSetAttribute (the dynamic-LDS limit of a kernel) applies to the calling
// thread's current device only, so a process-wide "done" flag leaves every other device at the 64 KiB default: one process could
// not drive two devices (a service that owns a sharded collection).  Usage: static ScDeviceOnce once; sc_device_once(once, [&] { ... });
struct ScDeviceOnce {
    std::mutex mu;
    uint64_t done[4] = {0, 0, 0, 0};
};
template <class F>
static inline void sc_device_once(ScDeviceOnce& o, F&& f) {
    int d = 0;
    (void)hipGetDevice(&d);
    d &= 255;
    std::lock_guard<std::mutex> lk(o.mu);
    if (!((o.done[d >> 6] >> (d & 63)) & 1)) {
        f();
        o.done[d >> 6] |= 1ull << (d & 63);
    }
}
// compute units of the calling thread's current device (cached per device)
static inline int sc_device_cus() {
    static std::mutex mu;
    static int cus[256] = {0};
    int d = 0;
    (void)hipGetDevice(&d);
    d &= 255;
    std::lock_guard<std::mutex> lk(mu);
    if (!cus[d]) {
        hipDeviceProp_t prop;
        cus[d] = hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return cus[d];
}

// ---- launchers implemented in the .hip files (all enqueue on `s`, never synchronise) ----

// rows.hip: out [rows, ld] synthetic (+ optional |x|^2); tight [n, dim] -> padded rows (+ |x|^2); rows -> tight
void sc_launch_synth_fill(float* out, int64_t rows, int dim, int ld, uint64_t seed, int64_t first_row, float* xnorm, hipStream_t s);
void sc_launch_synth_clustered(float* out, int64_t rows, int dim, int ld, uint64_t seed, int64_t first_row, int nclusters, float spread,
                               float* xnorm, hipStream_t s);
void sc_launch_ingest_rows(const float* src, const int64_t* rows, int64_t first, int64_t n, int dim, float* dst, int ld,
                           float* xnorm, hipStream_t s);
void sc_launch_gather_rows(const float* src, int ld, int64_t first, int64_t n, int dim, float* dst, hipStream_t s);
// rows of row_bytes (a multiple of 4) by index: gather dst[i] = src[idx[i]], or scatter dst[idx[i]] = src[i]
void sc_launch_copy_rows_indexed(const void* src, void* dst, const int32_t* idx_dev, int n, size_t row_bytes, bool scatter, hipStream_t s);

struct ScanPlan {
    int qt;          // queries per group (<=16)
    int qstream;     // 0: queries resident in LDS; else streamed per k-chunk through a shared LDS ring that many stages deep
    int groups;      // ceil(Q / qt)
    int gstride;     // slots per group in qmap / partial when that differs from qt (0 = qt)
    int nwg;         // workgroups per group (grid.x)
    int cap;         // per-(wave,query) candidate capacity
    int lists;       // partial lists per query = nwg * 4
    size_t lds;      // dynamic LDS bytes
    size_t partial_bytes;
};
// returns false when (ld, k) cannot be served by the exact kernel
// n_rows > 0: size the grid for that many rows (small corpora), else one workgroup per CU
bool sc_scan_exact_plan(int ld, int Q, int k, int cus, ScanPlan* p, int force_qt = 0, int nprobe = 0, int64_t n_rows = 0);
// X [n, ld], xnorm [n]; Qp [Q, ld] zero padded, qnorm [Q]; partial: plan.partial_bytes
// perm: stored position -> reported row (NULL = identity); seg_*: IVF probe ranges per group (NULL = all rows);
// qmap: query slot -> row of Qp / qnorm (NULL = identity), see scan_exact.hip ScanArgs
void sc_launch_scan_exact(int metric, const float* X, const float* xnorm, int64_t n, int ld, const float* Qp,
                          const float* qnorm, int Q, int k, const ScanPlan& p, uint64_t* partial, const uint32_t* perm,
                          const int* seg_base, const int64_t* seg_rows, int nprobe, hipStream_t s, const int32_t* qmap = nullptr);
// scan_exact.hip, wide groups of list-major IVF probing: one workgroup = one list part [seg_rows[2g], seg_rows[2g+1]) x up to
// `width` (32 or 64) queries (qmap [groups][width], valid slots a prefix, -1 beyond); partial [groups][width][k] sorted keys
bool sc_scan_listgemm_supported(int ld, int k);
void sc_launch_scan_listgemm(int metric, int width, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, int k, int groups,
                             uint64_t* partial, const uint32_t* perm, const int64_t* seg_rows, const int32_t* qmap, hipStream_t s);
// scan_masked.hip: the masked search (sc_index_search_masked*).
// mask_compact: allow (bitset over row ids) -> sel[m], the ascending list of allowed stored positions among [0, n), padded to a
// multiple of 16 entries; perm [perm_rows]: stored position -> row id (positions at or beyond perm_rows are row ids; NULL: all are).
// Two launchers with the host's read of cnt[blocks] (= m) between them: ..._count fills flags [(n + 63) / 64] (bitset over
// positions) and cnt [blocks + 1] (exclusive scan of the per-block popcounts, total last); ..._scatter writes sel.
#define SC_MASK_BLOCK_ROWS 2048
static inline int64_t sc_mask_blocks(int64_t n) { return (n + SC_MASK_BLOCK_ROWS - 1) / SC_MASK_BLOCK_ROWS; }
void sc_launch_mask_count(const uint32_t* allow, int64_t n, const uint32_t* perm, int64_t perm_rows, uint64_t* flags, uint32_t* cnt, hipStream_t s);
void sc_launch_mask_scatter(const uint64_t* flags, const uint32_t* cnt, int64_t n, uint32_t* sel, hipStream_t s);
// the gathered exact scan: sc_launch_scan_exact (resident queries; plan from sc_scan_exact_plan with force_qt = 16 and n_rows = m) over
// the m stored positions sel[] instead of a row range; reported ids = perm[position] below perm_rows, the position itself beyond
void sc_launch_scan_gather(int metric, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, int Q, int k, const ScanPlan& p,
                           uint64_t* partial, const uint32_t* perm, int64_t perm_rows, const uint32_t* sel, int64_t m, hipStream_t s);
// scan_grouped.hip: the grouped search (sc_index_search_grouped*).
// group_select: per query, the first occurrence of every label in its best-first candidate list cand_* [Q][W <= 1024] (ids; -1 =
// padding) is appended, in list order, to out_* [Q][k <= 128] / found_labels [Q][k] at count[q]; count and done [Q] are updated (done:
// k hits, or the list held padding).  first_round: count starts at 0 and the outputs are padded behind the hits.
void sc_launch_group_select(int metric, const float* cand_dist, const int64_t* cand_rows, int W, int Q, const int32_t* labels, int64_t n, int64_t row_base, int k,
                            bool first_round, float* out_dist, int64_t* out_rows, int32_t* found_labels, int32_t* count, int32_t* done, hipStream_t s);
// group_exclude: out [ceil(n / 32)] = allow (NULL: every row) minus the rows whose label is one of ONE query's *count hit labels
void sc_launch_group_exclude(const int32_t* labels, int64_t n, const uint32_t* allow, const int32_t* found_labels, const int32_t* count, uint32_t* out, int cus,
                             hipStream_t s);
// scan_mmr.hip: the MMR search (sc_index_search_mmr*).
// mmr_inverse: inv [n] = row -> stored position from perm [mapped] (stored position -> row; positions at or beyond mapped are rows).
// mmr_gram: G [Q][Fp][Fp] (Fp = F rounded up to 16), G[q][i][j] = the oriented score (sc_score, negated for L2) of candidates i and j of
// query q's best-first list cand_rows [Q][F <= 128] (ids; -1 = padding, last); inv NULL: the row is the position.  Entries of padding
// slots are unspecified.  mmr_select: the greedy selection of mmr_rule.h over cand_* and G -> out_* [Q][k <= F] in selection order,
// padded; cand_rows NULL: padding only.  *min_count = min(*min_count, candidates of every query).
void sc_launch_mmr_inverse(const uint32_t* perm, int64_t mapped, int64_t n, uint32_t* inv, hipStream_t s);
void sc_launch_mmr_gram(int metric, const float* X, const float* xnorm, int ld, int64_t n, int64_t row_base, const uint32_t* inv, const int64_t* cand_rows, int F, int Q,
                        float* G, hipStream_t s);
void sc_launch_mmr_select(int metric, const float* cand_dist, const int64_t* cand_rows, int F, const float* G, int Q, int k, float lambda, float* out_dist,
                          int64_t* out_rows, int32_t* min_count, hipStream_t s);
// scan_lexical.hip: the lexical and the hybrid search (sc_index_search_lexical*, sc_index_search_hybrid*; rules: lex_rule.h).
// lex_prep: qterms / qweights [Q][32], nterms [Q] -> memb [ceil(Q / qp)][2048] (the membership set of every pass of qp =
// sc_lex_queries_per_pass() queries), nt_eff [Q] (nterms; 0 for a query that breaks the rules, which also sets *bad).
// lex_scan: one pass -- nq <= qp queries (the pass's slice of qterms / qweights / nt_eff and its memb) over terms [n][T], allow NULL or a
// bitset over rows -> partial [nwg * 4][qp][k] sorted IP keys for sc_launch_topk_merge (groups 1, lists nwg * 4, qt qp); nwg from
// sc_lex_scan_workgroups.  lex_stats: df [65536] += rows holding each term, *sum_dl += slots that are not padding (both zeroed by
// the caller).  lex_fuse: dense_rows / lex_rows [Q][F <= 128] best first (-1 = padding) -> out_* [Q][k <= F] by lex_rrf, padded;
// dense_rows NULL: padding only.
int sc_lex_queries_per_pass(void);
int sc_lex_scan_workgroups(int64_t n, int T, int k, int cus);
void sc_launch_lex_prep(const uint16_t* qterms, const float* qweights, const int32_t* nterms, int Q, uint32_t* memb, int32_t* nt_eff, int32_t* bad, hipStream_t s);
void sc_launch_lex_scan(const uint16_t* terms, int64_t n, int T, const uint32_t* allow, const uint32_t* memb, const uint16_t* qterms, const float* qweights,
                        const int32_t* nt_eff, int nq, int k, float k1, float b, float avgdl, int nwg, uint64_t* partial, hipStream_t s);
void sc_launch_lex_stats(const uint16_t* terms, int64_t n, int T, uint32_t* df, unsigned long long* sum_dl, hipStream_t s);
void sc_launch_lex_fuse(const int64_t* dense_rows, const int64_t* lex_rows, int F, int Q, int k, int32_t c, float wd, float wl, float* out_score, int64_t* out_rows,
                        hipStream_t s);
// scan_late.hip: late interaction over the token store of an index (sc_tokens.cpp; rules: maxsim_rule.h, late_rule.h).  pool: token
// vectors of W elements, f32 (fmt 0) or bf16 (fmt 1); table [n]: a row's tokens are pool[start, start + len).
// late_rerank: out [Bq][C] = the MaxSim score of question q (rows [q_off[q], q_off[q + 1]) of Q [.., W]) against row cand[q][c] (local
// row number; -1 or a row without tokens: -inf).  late_scan: ONE question Q [nq <= 128][W] over every row that has tokens (allow NULL or
// a bitset over rows) -> partial [nwg * 4][k] sorted late_hit_key lists for sc_launch_topk_merge (SC_METRIC_IP, groups 1, lists nwg * 4,
// qt 1); nwg from sc_late_scan_workgroups; next_block: one device word the caller zeroes before the launch (the work counter).  late_gather: the live tokens of every row from old_pool (old_tab) to new_pool (new_tab).
struct sc_tok_entry;
int sc_late_scan_workgroups(int64_t n, int nq, int W, int k, int cus);
void sc_launch_late_rerank(const float* Q, const int32_t* q_off, int Bq, const void* pool, int fmt, const sc_tok_entry* table, const int64_t* cand, int C, int W,
                           float* out, hipStream_t s);
void sc_launch_late_scan(const float* Q, int nq, const void* pool, int fmt, const sc_tok_entry* table, int64_t n, const uint32_t* allow, int W, int k, int nwg,
                         uint64_t* partial, unsigned* next_block, hipStream_t s);
void sc_launch_late_gather(const sc_tok_entry* old_tab, const sc_tok_entry* new_tab, int64_t n, const void* old_pool, void* new_pool, int tok_bytes, int cus, hipStream_t s);
// late_install: vecs [.., W] f32 (device), src [total] source token of each stored token (device) or NULL (0 .. total - 1) -> dst, `total`
// tokens of W elements in the pool's format (fmt 1: rounded by late_round_bf16)
void sc_launch_late_install(const float* vecs, const int32_t* src, int64_t total, int W, int fmt, void* dst, int cus, hipStream_t s);
// partial [groups][lists][qt][k] sorted keys -> out_dist [Q,k], out_rows [Q,k]
// more lists than one LDS tree merge holds (2 * lists * k keys > 128 KiB) are merged in levels whose intermediate k-lists live right
// behind the partial lists: that many extra bytes (included in ScanPlan::partial_bytes)
size_t sc_topk_merge_scratch_bytes(int lists, int Q, int k);
void sc_launch_topk_merge(int metric, const uint64_t* partial, int groups, int lists, int qt, int Q, int k,
                          int64_t row_base, float* out_dist, int64_t* out_rows, hipStream_t s);
// lists_per_query sorted k-lists per query, list j of query q = partial[src[q * lists_per_query + j] * k ...] (src < 0: none);
// needs 2 * lists_per_query * k * 8 <= 128 KiB (sc_topk_gather_merge_supported)
bool sc_topk_gather_merge_supported(int lists_per_query, int k);
void sc_launch_topk_merge2(int metric, const float* d1, const int64_t* r1, const float* d2, const int64_t* r2, int k, float* out_dist, int64_t* out_rows, int Q,
                           hipStream_t s);
void sc_launch_topk_gather_merge(int metric, const uint64_t* partial, const int32_t* src, int lists_per_query, int Q, int k,
                                 int64_t row_base, float* out_dist, int64_t* out_rows, hipStream_t s);

// scan_shadow.hip, scan_coarse.hip, scan_coarse64.hip, scan_select.hip, scan_rerank.hip (the batched scan, scan_batched.h): bf16 / int8
// shadows, coarse GEMM + filter phases, selection, exact re-rank
int sc_batched_kprime(void);   // candidates kept per query: bf16 stage
int sc_batched_kprime8(void);  // int8 stage
void sc_launch_shadow(const float* X, const float* xnorm, int64_t first, int64_t n, int ld, void* Xb, unsigned* res_bits, hipStream_t s);
void sc_launch_shadow8(const float* X, const float* xnorm, int64_t first, int64_t n, int ld, int ld8, void* Xq, float* xscale, unsigned* res_bits,
                       hipStream_t s);
void sc_launch_norm_max(const float* xnorm, int64_t n, unsigned* out_bits, hipStream_t s);
void sc_launch_query_bf16(const float* Qp, int Q, int Qpad, int ld, void* Qb, float* qres, hipStream_t s);
void sc_launch_query_i8(const float* Qp, int Q, int Qpad, int ld, int ld8, void* Qq, float* qscale, float* qres, unsigned* absmax_bits, hipStream_t s);
void sc_launch_scan_batched_init(float* thr, float* thr_fast, int qpad, uint64_t* best, unsigned* count, int* overflow, int Q, int kp, hipStream_t s);
void sc_launch_scan_coarse(int metric, const void* Xb, const float* xnorm, int64_t row0, int64_t row1, int ld, const void* Qb,
                           const float* qnorm, int Q, int Qpad, const float* thr, const float* thr_fast, uint64_t* surv, unsigned* count,
                           int cap, hipStream_t s, bool i8 = false, const float* xscale = nullptr, const float* qscale = nullptr,
                           bool dense = false,  // dense: most scores of this row range are expected to survive (loose thresholds)
                           void* hit_scratch = nullptr, size_t hit_bytes = 0);  // per-wave hit lists of the narrow kernel (batches of <= 64 queries)
// scan_coarse.hip, the coarse_workgroups / coarse_persistent options of sc_diag_set_option: workgroups of the persistent coarse kernels
// (0 = one per CU); 0 = one workgroup per tile instead of the persistent 256-tile kernel
void sc_scan_set_coarse_workgroups(int v);
void sc_scan_set_coarse_persistent(int v);
void sc_launch_scan_select(int metric, uint64_t* surv, unsigned* count, int cap, uint64_t* best, const float* qnorm, float* thr,
                           float* thr_fast, int* overflow, int Q, int kp, hipStream_t s);
void sc_launch_scan_rerank(int metric, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, const uint64_t* best,
                           const float* thr, const unsigned* xnorm_max_bits, const float* qres, const int* overflow, int Q, int k,
                           int64_t row_base, const uint32_t* perm, float* out_dist, int64_t* out_rows, int* flags, hipStream_t s,
                           int kp, uint64_t* ekeys);

// ivf_coarse.hip + scan_coarse64.hip: the int8 coarse stage of list-major IVF probing (L2)
void sc_launch_ivf_center_shadow(const float* X, int64_t rows, int ld, int ld8, const float* C, int ldc, const int64_t* list_off, int nlist, void* Xc8,
                                 float* xrow, unsigned* list_stats, hipStream_t s, const float* xnorm = nullptr, const float* cnorm = nullptr, const int64_t* only = nullptr);  // norms: COSINE
void sc_launch_ivf_pair_query(const float* Qp, int ld, int ld8, const float* C, int ldc, const int32_t* slot_q, const int32_t* slot_l, int nslots,
                              const unsigned* list_stats, void* Qc8, float* slot_qs, float* slot_qnlb, float* slot_qb, float* slot_qd, float* slot_eps, hipStream_t s,
                              int metric = SC_METRIC_L2, const float* qnorm = nullptr, const float* cnorm = nullptr);
void sc_launch_ivf_slot_thr(const int32_t* slot_q, const float* slot_qnlb, const float* slot_eps, const float* thr, int nslots, float* slot_thr, float* slot_tf,
                            hipStream_t s);
void sc_launch_ivf_coarse(const void* Xc8, const float* xrow, int ld8, const void* Qc8, const void* items, int nitems, const float* slot_tf,
                          const float* slot_thr, const float* slot_qn, const float* slot_qs, const int32_t* slot_q, const float* slot_qb, const float* slot_qd,
                          uint64_t* surv, unsigned* count, int cap, void* hit_scratch, size_t hit_bytes, hipStream_t s,
                          const int32_t* slot_dst = nullptr, int metric = SC_METRIC_L2);  // non-null: dense phase (every row survives; count[] preset by the caller)
// scan_rerank.hip
void sc_launch_scan_rerank_keys(int metric, const float* X, const float* xnorm, int ld, const float* Qp, const float* qnorm, const uint64_t* cand, const int* ncand, int kp,
                                const uint32_t* perm, uint64_t* ekeys, int Q, hipStream_t s);
// the collect pass of the exhaustive batched path (scan_rerank.hip, scan_select.hip): thresholds from the k-th exact score of the failed pass; survivor counts -> candidate counts
void sc_launch_scan_collect_bound(int metric, const float* prev_dist, int k, const float* qnorm, const float* qres, const unsigned* bits, int ld, float* thr,
                                  float* thr_fast, int* flags, int Q, hipStream_t s);
void sc_launch_scan_collect_counts(const unsigned* count, int cap, int* ncand, int* flags, int Q, hipStream_t s);
// thresholds from exact scores before the large phases (scan_rerank.hip): ekeys [Q][kp <= 128] exact keys of the best coarse candidates
void sc_launch_scan_tighten(int metric, const uint64_t* ekeys, int kp, int k, const float* qnorm, const float* qres, const unsigned* bits, int ld, float* thr,
                            float* thr_fast, float* thr_cut, int Q, hipStream_t s);
void sc_launch_scan_thr_min(float* thr, const float* thr_cut, int Q, hipStream_t s);
// the wide candidate set (scan_select.hip, scan_rerank.hip): best [Q][kcap] with nbest[q] keys, every key within thr_cut kept
void sc_launch_scan_select_wide(int metric, const uint64_t* surv, unsigned* count, int cap, uint64_t* best, unsigned* nbest, int kcap, int kp, const float* qnorm,
                                float* thr, float* thr_fast, const float* thr_cut, int* overflow, int Q, hipStream_t s);
void sc_launch_scan_wide_compact(int metric, const uint64_t* best, const unsigned* nbest, int kcap, const float* thr, uint64_t* cand, int* ncand, int Q, hipStream_t s);
void sc_launch_scan_wide_certify(int metric, const float* out_dist, int k, const float* qnorm, const float* qres, const unsigned* bits, int ld, const float* thr,
                                 const int* overflow, int* flags, int Q, hipStream_t s);
void sc_launch_fill_u32(unsigned* p, unsigned v, int n, hipStream_t s);
void sc_launch_refine_finalize(int metric, const uint64_t* ekeys, const int* ncand, const int* flags, int k, int64_t row_base, float* out_dist, int64_t* out_rows,
                               int Q, hipStream_t s, int stride = 0);
int sc_ivf_widen_cap(void);
void sc_launch_ivf_bound(int metric, const uint64_t* ekeysA, int kpa, int k, const float* qnorm, const unsigned* xmax_bits, int ld, float* thr, int Q, hipStream_t s,
                         const uint64_t* ekeysT = nullptr, bool keep_min = false);
void sc_launch_ivf_candidates(int metric, const uint64_t* survA, const unsigned* cntA, const uint64_t* bestA, int kpa, const uint64_t* survB, const unsigned* cntB, int cap,
                              const float* thr, uint64_t* cand, int* ncand, int* flags, int Q, int wcap, hipStream_t s, int capB = 0);
void sc_launch_ivf_refine_finalize(int metric, const uint64_t* ekeysA, int kpa, const uint64_t* ekeys, const int* ncand, const int* flags, int k, int64_t row_base,
                                   float* out_dist, int64_t* out_rows, int Q, hipStream_t s);

// ivf.hip
void sc_launch_ivf_plan(const int64_t* probe_rows, int Q, int nprobe, const int64_t* list_off, int nlist, int* seg_base, int64_t* seg_rows,
                        hipStream_t s);
void sc_launch_centroid_mean(const float* X, int ld, int dim, const int64_t* members, const int64_t* member_off, int nlist, float* C_tight,
                             const float* C_old, int ldc_old, hipStream_t s);
void sc_launch_permute_rows(const float* X, const float* xnorm, const uint32_t* perm, int64_t n, int ld, float* Xo, float* xnorm_o, hipStream_t s);
void sc_launch_rows_to_sample(const float* X, int ld, int dim, const int64_t* rows, int64_t n, float* out_tight, hipStream_t s);
// compact.hip: in-place compaction after sc_index_delete_rows
void sc_launch_delete_map(const uint32_t* del_dev, int64_t lo, int64_t hi, int64_t c0, uint32_t cn, uint32_t* flags, uint32_t* tile_sum, uint32_t* src, hipStream_t s);
void sc_launch_move_rows(const void* in, int64_t row0, const uint32_t* src, uint32_t m, size_t row_bytes, void* dst, hipStream_t s);
void sc_launch_renumber_ids(uint32_t* ids, int64_t n, const uint32_t* del_dev, int64_t ndel, hipStream_t s);
void sc_launch_reseed_centroids(float* C_tight, int dim, const int32_t* moves_dev, int m, hipStream_t s);
