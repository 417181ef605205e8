// sc_encoder_diag.cpp -- sc_diag_*: one encoder kernel per call, for the single-kernel parity tests and the GEMM timing scripts.
//
// The pattern of every harness: host f32 in (activations rounded to bf16 by f32_to_bf16_kernel), THE PRODUCT LAUNCHER, result widened
// to f32 and copied back, synchronous.  Output buffers are pre-filled with 0xFF bytes (NaN as bf16 and as f32), so that an element a
// kernel does not write shows in the result.  (sc_diag_encoder_read, which needs the encoder handle, is in sc_encoder_embed.cpp.)
// sc_diag_encoder_plan and sc_diag_encoder_plan_keep, at the end, touch no device: the host plan of a packed call (sc_encoder_plan.h).
#include <cstring>
#include <vector>

#include "encoder_ops.h"
#include "maxsim_rule.h"
#include "rel_bucket_rule.h"
#include "sc_diag_blob.h"
#include "sc_encoder_plan.h"
#include "sc_internal.h"

namespace {
#define SC_TRY(expr)              \
    do {                          \
        sc_status st_ = (expr);   \
        if (st_) return st_;      \
    } while (0)

sc_status dev_alloc(sc_devbuf& out, size_t bytes) {
    if (out.alloc(bytes) != hipSuccess) return sc_fail(SC_ERR_NOMEM, "diag: hipMalloc failed");
    return SC_OK;
}
// host bytes -> device, as they are (f32 vectors, int32 ids / lens, int8 operands)
sc_status upload(const void* host, size_t bytes, sc_devbuf& out, hipStream_t s) {
    SC_TRY(dev_alloc(out, bytes));
    if (host && bytes) SC_HIP(hipMemcpyAsync(out.p, host, bytes, hipMemcpyHostToDevice, s));
    return SC_OK;
}
// host f32 [n] -> device bf16 (through a device f32 staging buffer)
sc_status upload_bf16(const float* host, int64_t n, sc_devbuf& f32buf, sc_devbuf& out, hipStream_t s) {
    SC_TRY(upload(host, (size_t)n * 4, f32buf, s));
    SC_TRY(dev_alloc(out, (size_t)n * 2));
    sc_launch_f32_to_bf16((const float*)f32buf.p, out.p, n, s);
    return SC_OK;
}
sc_status alloc_nan(sc_devbuf& out, size_t bytes, hipStream_t s) {
    SC_TRY(dev_alloc(out, bytes));
    SC_HIP(hipMemsetAsync(out.p, 0xFF, bytes ? bytes : 16, s));
    return SC_OK;
}
// device bytes -> host; synchronises
sc_status download(const void* dev, size_t bytes, void* host, hipStream_t s) {
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}
// T5's bias for the attention harness: rel_bias [buckets][heads] (valid buckets / max_distance) -> the distance table of a 2 048-token span on the device
const int DIAG_REL_SPAN = 2048;
sc_status upload_rel_table(const float* rel_bias, int buckets, int heads, int max_distance, sc_devbuf& out, hipStream_t s) {
    const std::vector<float> tbl = sc_rel_bias_table(rel_bias, buckets, heads, max_distance, DIAG_REL_SPAN);
    SC_TRY(upload(tbl.data(), tbl.size() * 4, out, s));
    SC_HIP(hipStreamSynchronize(s));  // tbl goes out of scope
    return SC_OK;
}
// device bf16 [n] -> host f32 [n]; synchronises
sc_status download_bf16(const void* dev, int64_t n, float* host, hipStream_t s) {
    sc_devbuf fo;
    SC_TRY(dev_alloc(fo, (size_t)n * 4));
    sc_launch_bf16_to_f32(dev, (float*)fo.p, n, s);
    return download(fo.p, (size_t)n * 4, host, s);
}
}  // namespace

// ------------------------------------------------------------------ the GEMMs

// sc_diag_gemm_bf16_ex in three steps: the rules (host arithmetic, before the runtime is looked at), stage / launch / download, the path
// the launcher took.  sc_diag_gemm_bf16 is the same with the flags its "+ 16" stands for and its own name in the messages.
namespace {
enum { GEMM_EX_CBLOCK = 1, GEMM_EX_ABLOCK = 2, GEMM_EX_SPLITK = 4, GEMM_EX_TILE128 = 8 };

sc_status gemm_ex_validate(const char* who, int epi, int flags, const float* A, const float* W, const float* bias, const float* R, int M, int N, int K,
                           const float* out) {
    if (!A || !W || !bias || !out) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (epi < 0 || epi > 2 || (epi == EPI_BIAS_RES && !R)) return sc_fail(SC_ERR_INVALID, "%s: bad epilogue / missing residual", who);
    if (flags & ~15) return sc_fail(SC_ERR_INVALID, "%s: flags %d has bits beyond 0 (C blocked), 1 (A blocked), 2 (split-K scratch), 3 (128-tile kernel)", who, flags);
    if (!sc_gemm_bf16_supported(M, N, K)) return sc_fail(SC_ERR_UNSUPPORTED, "%s: need M%%128==0, N%%128==0, K%%64==0", who);
    // the launcher's contract for A in 64-column blocks: only the per-tile 256-tile kernel reads that layout
    if ((flags & GEMM_EX_ABLOCK) && ((M % 256) || (N % 256) || (flags & (GEMM_EX_SPLITK | GEMM_EX_TILE128))))
        return sc_fail(SC_ERR_UNSUPPORTED,
                       "%s: blocked A (flags bit 1) is read by the per-tile 256-tile kernel only: needs M%%256==0, N%%256==0, no split-K scratch (bit 2) and "
                       "no forced 128-tile kernel (bit 3); got M %d, N %d, flags %d", who, M, N, flags);
    return SC_OK;
}

sc_status gemm_ex_run(const char* who, sc_runtime* rt, int epi, int flags, const float* A, const float* W, const float* bias, const float* R, int M, int N,
                      int K, float* out, int32_t* path) {
    SC_TRY(gemm_ex_validate(who, epi, flags, A, W, bias, R, M, N, K, out));
    if (!rt) return sc_fail(SC_ERR_INVALID, "%s: the runtime is NULL", who);
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fa, fw, fr, da, dw, dr, db, dc, sk;
    size_t sk_bytes = 0;
    if (flags & GEMM_EX_SPLITK) {
        sk_bytes = (size_t)sc_gemm_splitk_factor(M, N, K, rt->cus) * M * N * 4;
        SC_TRY(dev_alloc(sk, sk_bytes));
    }
    SC_TRY(upload_bf16(A, (int64_t)M * K, fa, da, s));  // blocked A is the same M K values in another order
    SC_TRY(upload_bf16(W, (int64_t)N * K, fw, dw, s));
    if (R) SC_TRY(upload_bf16(R, (int64_t)M * N, fr, dr, s));
    SC_TRY(upload(bias, (size_t)N * 4, db, s));
    SC_TRY(alloc_nan(dc, (size_t)M * N * 2, s));
    sc_gemm_force_tile128((flags & GEMM_EX_TILE128) != 0);
    sc_launch_gemm_bf16(epi, da.p, (flags & GEMM_EX_ABLOCK) ? SC_LDC_BLOCKED64 : K, dw.p, K, (const float*)db.p, dr.p, N, dc.p,
                        (flags & GEMM_EX_CBLOCK) ? SC_LDC_BLOCKED64 : N, M, N, K, s, sk.p, sk_bytes);
    sc_gemm_force_tile128(false);
    const ScGemmPath p = sc_gemm_last_path();
    if (path) path[0] = p.tile, path[1] = p.splitk, path[2] = p.order, path[3] = p.pp, path[4] = p.nt;
    if (!p.tile) return sc_fail(SC_ERR_UNSUPPORTED, "%s: the launcher refused blocked A for this launch", who);
    return download_bf16(dc.p, (int64_t)M * N, out, s);
}
}  // namespace

extern "C" sc_status sc_diag_gemm_bf16(sc_runtime* rt, int32_t epi, const float* A, const float* W, const float* bias, const float* R,
                                       int32_t M, int32_t N, int32_t K, float* out) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_bf16: NULL argument");
    const bool allow_splitk = epi >= 0 && (epi & 16);
    if (epi >= 0) epi &= 15;
    return gemm_ex_run("sc_diag_gemm_bf16", rt, epi, allow_splitk ? GEMM_EX_SPLITK : 0, A, W, bias, R, M, N, K, out, nullptr);
}

extern "C" sc_status sc_diag_gemm_bf16_ex(sc_runtime* rt, int32_t epi, int32_t flags, const float* A, const float* W, const float* bias, const float* R,
                                          int32_t M, int32_t N, int32_t K, float* out, int32_t* path) {
    return gemm_ex_run("sc_diag_gemm_bf16_ex", rt, epi, flags, A, W, bias, R, M, N, K, out, path);
}

// The plain launcher's choice without a launch, and without a device when cus > 0 (include/semcode_hip.h)
extern "C" sc_status sc_diag_gemm_path(int32_t M, int32_t N, int32_t K, int32_t cus, int32_t splitk_scratch, int32_t* path) {
    if (!path) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_path: NULL argument");
    ScGemmPath p = sc_gemm_last_path();
    if (M != 0) {
        if (!sc_gemm_bf16_supported(M, N, K)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_gemm_path: need M%%128==0, N%%128==0, K%%64==0");
        if (cus <= 0) cus = sc_device_cus();
        p = sc_gemm_plain_path(M, N, K, cus, splitk_scratch ? (size_t)sc_gemm_splitk_factor(M, N, K, cus) * M * N * 4 : 0);
    }
    path[0] = p.tile, path[1] = p.splitk, path[2] = p.order, path[3] = p.pp, path[4] = p.nt;
    return SC_OK;
}
extern "C" int32_t sc_diag_gemm_splitk(int32_t M, int32_t N, int32_t K, int32_t cus) { return sc_gemm_splitk_factor(M, N, K, cus > 0 ? cus : sc_device_cus()); }

extern "C" sc_status sc_diag_gemm_i8(sc_runtime* rt, const int8_t* A, const int8_t* W, int32_t M, int32_t N, int32_t K, int32_t* out) {
    if (!rt || !A || !W || !out) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_i8: NULL argument");
    if (M <= 0 || N <= 0 || K <= 0 || (M % 256) || (N % 256) || (K % 128)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_gemm_i8: need M%%256==0, N%%256==0, K%%128==0");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf da, dw, dc;
    SC_TRY(upload(A, (size_t)M * K, da, s));
    SC_TRY(upload(W, (size_t)N * K, dw, s));
    SC_TRY(alloc_nan(dc, (size_t)M * N * 4, s));
    sc_launch_gemm_i8_diag(da.p, dw.p, dc.p, M, N, K, s);
    return download(dc.p, (size_t)M * N * 4, out, s);
}

namespace {
// device-resident synthetic operands of one GEMM shape (sc_diag_gemm_trace, sc_diag_gemm_bench): A ~ N(0,1), W ~ 0.05 N(0,1), both
// bf16; bias and residual zero
struct SynthGemm {
    int epi, M, N, K;
    sc_devbuf fa, da, fw, dw, db, dr, dc;
    sc_status init(hipStream_t s) {
        const int64_t na = (int64_t)M * K, nw = (int64_t)N * K, nc = (int64_t)M * N;
        SC_TRY(dev_alloc(fa, na * 4));
        SC_TRY(dev_alloc(da, na * 2));
        SC_TRY(dev_alloc(fw, nw * 4));
        SC_TRY(dev_alloc(dw, nw * 2));
        SC_TRY(dev_alloc(db, (size_t)N * 4));
        SC_TRY(dev_alloc(dr, nc * 2));
        SC_TRY(dev_alloc(dc, nc * 2));
        sc_launch_synth_scaled((float*)fa.p, na, 1, 1.0f, 0.0f, s);
        sc_launch_synth_scaled((float*)fw.p, nw, 2, 0.05f, 0.0f, s);
        sc_launch_f32_to_bf16((const float*)fa.p, da.p, na, s);
        sc_launch_f32_to_bf16((const float*)fw.p, dw.p, nw, s);
        SC_HIP(hipMemsetAsync(db.p, 0, (size_t)N * 4, s));
        SC_HIP(hipMemsetAsync(dr.p, 0, (size_t)nc * 2, s));
        return SC_OK;
    }
    void launch(hipStream_t s) const { sc_launch_gemm_bf16(epi, da.p, K, dw.p, K, (const float*)db.p, dr.p, N, dc.p, N, M, N, K, s); }
};
}  // namespace

// Per-workgroup time stamps of the 256-tile kernel: out [launch][tile][8] words of back-to-back traced launches (as many as fit into
// cap_words) on synthetic operands
extern "C" sc_status sc_diag_gemm_trace(sc_runtime* rt, int32_t epi, int32_t M, int32_t N, int32_t K, uint64_t* out, int64_t cap_words) {
    if (!rt || !out) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_trace: bad argument");
    if (M <= 0 || N <= 0 || K <= 0 || (M % 256) || (N % 256) || (K % 64)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_gemm_trace: need M%%256==0, N%%256==0, K%%64==0");
    const int64_t ntiles = (int64_t)(M / 256) * (N / 256);
    const int64_t launches = cap_words / (ntiles * 8);
    if (launches < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_trace: out too small (need 8 words per tile)");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    SynthGemm g{epi, M, N, K};
    sc_devbuf tr;
    const size_t trace_bytes = (size_t)launches * ntiles * 64;
    SC_TRY(dev_alloc(tr, trace_bytes));
    SC_TRY(g.init(s));
    SC_HIP(hipMemsetAsync(tr.p, 0, trace_bytes, s));
    static const int dbg = (int)sc_env_i64("SC_GEMM_TRACE_DBG", 0);  // stamps around an ablated main loop (scripts/gemm_clock.py)
    sc_gemm_set_debug(dbg);
    for (int i = 0; i < 2; ++i) g.launch(s);
    for (int64_t l = 0; l < launches; ++l) {
        sc_gemm_set_trace((unsigned long long*)tr.p + l * ntiles * 8);
        g.launch(s);
    }
    sc_gemm_set_trace(nullptr);
    sc_gemm_set_debug(0);
    hipError_t he = hipStreamSynchronize(s);
    if (he != hipSuccess) return sc_fail(SC_ERR_HIP, "diag gemm trace failed: %s", hipGetErrorString(he));
    SC_HIP(hipMemcpy(out, tr.p, trace_bytes, hipMemcpyDeviceToHost));
    return SC_OK;
}

// Time `iters` launches of one GEMM shape on device-resident synthetic bf16 data (hipEvents on the
// runtime's stream).  variant: 0 = product kernel; 1/2/4/5 = diagnostic ablations of the 256-tile kernel
// (no in-loop LDS-DMA / no MFMA / no epilogue / no DMA + no epilogue); 128 = force the 128x128 tile.
extern "C" sc_status sc_diag_gemm_bench(sc_runtime* rt, int32_t epi, int32_t M, int32_t N, int32_t K, int32_t iters, int32_t variant,
                                        double* ms_per_launch) {
    if (!rt || !ms_per_launch || iters < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_bench: bad argument");
    if (!sc_gemm_bf16_supported(M, N, K)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_gemm_bench: need M%%128==0, N%%128==0, K%%64==0");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    SynthGemm g{epi, M, N, K};
    SC_TRY(g.init(s));
    // variant = 100000 * pp + v: pp = main loop of the 256-tile kernel (0 = as configured, 1 = one barrier per K-tile, 2..5 = ping-pong depth)
    const int pp = variant / 100000;
    variant %= 100000;
    sc_gemm_set_pp(pp == 0 ? -1 : pp == 1 ? 0 : pp);
    sc_gemm_force_tile128(variant == 128);
    sc_gemm_set_debug((variant == 128 || variant >= 1000) ? 0 : variant);
    sc_gemm_set_order(variant >= 1000 ? variant - 1000 : 16);  // variants 1000+o: tile order o with the real epilogue
    hipEvent_t e0, e1;
    SC_HIP(hipEventCreate(&e0));
    SC_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) g.launch(s);
    hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) g.launch(s);
    hipEventRecord(e1, s);
    hipError_t he = hipStreamSynchronize(s);
    sc_gemm_force_tile128(false);
    sc_gemm_set_debug(0);
    sc_gemm_set_order(-1);  // back to "by shape", the resting value
    sc_gemm_set_pp(-1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (he != hipSuccess) return sc_fail(SC_ERR_HIP, "diag gemm bench failed: %s", hipGetErrorString(he));
    *ms_per_launch = ms / iters;
    return SC_OK;
}

// ------------------------------------------------------------------ the LayerNorm-folded pipeline and the stand-alone kernels, one launch each

// fold_ln_weights_kernel: W [N,K], gamma / beta [K], bias [N] or NULL (all f32) -> Wf [N,K] (the bf16 W', widened), c1 [N], c2 [N]
extern "C" sc_status sc_diag_fold_ln(sc_runtime* rt, const float* W, const float* gamma, const float* beta, const float* bias, int32_t N, int32_t K,
                                     float* Wf, float* c1, float* c2) {
    if (!rt || !W || !gamma || !beta || !Wf || !c1 || !c2) return sc_fail(SC_ERR_INVALID, "sc_diag_fold_ln: NULL argument");
    if (N < 1 || K < 4 || (K % 4)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_fold_ln: need N >= 1 and K a multiple of 4");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf dw, dg, db, dbias, dwf, dc1, dc2;
    SC_TRY(upload(W, (size_t)N * K * 4, dw, s));
    SC_TRY(upload(gamma, (size_t)K * 4, dg, s));
    SC_TRY(upload(beta, (size_t)K * 4, db, s));
    if (bias) SC_TRY(upload(bias, (size_t)N * 4, dbias, s));
    SC_TRY(alloc_nan(dwf, (size_t)N * K * 2, s));
    SC_TRY(alloc_nan(dc1, (size_t)N * 4, s));
    SC_TRY(alloc_nan(dc2, (size_t)N * 4, s));
    sc_launch_fold_ln_weights((const float*)dw.p, (const float*)dg.p, (const float*)db.p, bias ? (const float*)dbias.p : nullptr, N, K, dwf.p, (float*)dc1.p,
                              (float*)dc2.p, s);
    SC_TRY(download(dc1.p, (size_t)N * 4, c1, s));
    SC_TRY(download(dc2.p, (size_t)N * 4, c2, s));
    return download_bf16(dwf.p, (int64_t)N * K, Wf, s);
}

// EPI_LNA_BIAS / EPI_LNA_GELU / EPI_LNA_BIAS_ROPE through sc_launch_gemm_bf16_ln.  A [M,K] raw rows, Wf [N,K] / c1 / c2 [N] as
// sc_diag_fold_ln returned them, stats_in [K/256][M][2] the caller's partial (sum, sum of squares).  flags bit 0: C in 64-column blocks
// ([N/64][M][64], returned that way).  Rotary form: positions = row & (rope_S - 1), tables of sc_rope_table.
extern "C" sc_status sc_diag_gemm_lna(sc_runtime* rt, int32_t epi, int32_t flags, const float* A, const float* Wf, const float* c1, const float* c2,
                                      const float* stats_in, float eps, int32_t M, int32_t N, int32_t K, int32_t rope_S, float rope_theta,
                                      int32_t rope_ncols, float* C, float* fin) {
    if (!rt || !A || !Wf || !c1 || !c2 || !stats_in || !C || !fin) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_lna: NULL argument");
    if (epi != EPI_LNA_BIAS && epi != EPI_LNA_GELU && epi != EPI_LNA_BIAS_ROPE) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_lna: epilogue must be 3, 4 or 6");
    if ((flags & ~1) || !(eps > 0.f)) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_lna: bad flags / eps");
    if (!sc_gemm_ln_supported(M, N, K) || K > 4096) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_gemm_lna: need M%%256==0, N%%256==0, K%%256==0, K<=4096");
    const bool rope = epi == EPI_LNA_BIAS_ROPE;
    if (rope && (rope_S < 1 || rope_S > 65536 || (rope_S & (rope_S - 1)) || rope_ncols < 0 || rope_ncols > N || (rope_ncols % 64)))
        return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_lna: rope_S must be a power of two, rope_ncols a multiple of 64 within N");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fa, da, fw, dw, dc1, dc2, dst, dfin, dc, dt;
    SC_TRY(upload_bf16(A, (int64_t)M * K, fa, da, s));
    SC_TRY(upload_bf16(Wf, (int64_t)N * K, fw, dw, s));
    SC_TRY(upload(c1, (size_t)N * 4, dc1, s));
    SC_TRY(upload(c2, (size_t)N * 4, dc2, s));
    SC_TRY(upload(stats_in, (size_t)(K / 256) * M * 8, dst, s));
    SC_TRY(alloc_nan(dfin, (size_t)M * 8, s));
    SC_TRY(alloc_nan(dc, (size_t)M * N * 2, s));
    const float *cos_t = nullptr, *sin_t = nullptr;
    std::vector<float> tab;
    if (rope) {
        tab = sc_rope_table(rope_S, rope_theta);
        SC_TRY(upload(tab.data(), tab.size() * 4, dt, s));
        cos_t = (const float*)dt.p;
        sin_t = cos_t + tab.size() / 2;
    }
    sc_launch_gemm_bf16_ln(epi, da.p, K, dw.p, K, (const float*)dc2.p, nullptr, 0, dc.p, (flags & 1) ? SC_LDC_BLOCKED64 : N, M, N, K, s, (const float*)dc1.p,
                           (const float*)dst.p, (float*)dfin.p, nullptr, nullptr, eps, cos_t, sin_t, rope ? rope_S : 0, rope ? rope_ncols : 0);
    SC_TRY(download(dfin.p, (size_t)M * 8, fin, s));  // synchronises: tab may go
    return download_bf16(dc.p, (int64_t)M * N, C, s);
}

// Strip selection of the EPI_LNA_* launcher, without a launch and without a device when cus > 0 (include/semcode_hip.h)
extern "C" int32_t sc_diag_gemm_strip(int32_t M, int32_t N, int32_t K, int32_t cus) {
    if (M == 0) return sc_gemm_last_strip();
    return sc_gemm_strip_tiles(M, N, K, cus > 0 ? cus : sc_device_cus());
}

// EPI_RESLN_STATS through sc_launch_gemm_bf16_ln.  A [M,K] (flags bit 0: given as [K/64][M][64]), W [N,K], bias [N] (= b + beta), gam [N],
// R [M,N] the raw residual, fin [M][2] its (mu, rs) -> C [M,N], stats_out [N/256][M][2].
extern "C" sc_status sc_diag_gemm_resln(sc_runtime* rt, int32_t flags, const float* A, const float* W, const float* bias, const float* gam, const float* R,
                                        const float* fin, float eps, int32_t M, int32_t N, int32_t K, float* C, float* stats_out) {
    if (!rt || !A || !W || !bias || !gam || !R || !fin || !C || !stats_out) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_resln: NULL argument");
    if ((flags & ~1) || !(eps > 0.f)) return sc_fail(SC_ERR_INVALID, "sc_diag_gemm_resln: bad flags / eps");
    if (!sc_gemm_ln_supported(M, N, K)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_gemm_resln: need M%%256==0, N%%256==0, K%%256==0");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fa, da, fw, dw, fr, dr, db, dg, dfin, dc, dso;
    SC_TRY(upload_bf16(A, (int64_t)M * K, fa, da, s));
    SC_TRY(upload_bf16(W, (int64_t)N * K, fw, dw, s));
    SC_TRY(upload_bf16(R, (int64_t)M * N, fr, dr, s));
    SC_TRY(upload(bias, (size_t)N * 4, db, s));
    SC_TRY(upload(gam, (size_t)N * 4, dg, s));
    SC_TRY(upload(fin, (size_t)M * 8, dfin, s));
    SC_TRY(alloc_nan(dc, (size_t)M * N * 2, s));
    SC_TRY(alloc_nan(dso, (size_t)(N / 256) * M * 8, s));
    sc_launch_gemm_bf16_ln(EPI_RESLN_STATS, da.p, (flags & 1) ? SC_LDC_BLOCKED64 : K, dw.p, K, (const float*)db.p, dr.p, N, dc.p, N, M, N, K, s, nullptr, nullptr,
                           (float*)dfin.p, (const float*)dg.p, (float*)dso.p, eps);
    SC_TRY(download(dso.p, (size_t)(N / 256) * M * 8, stats_out, s));
    return download_bf16(dc.p, (int64_t)M * N, C, s);
}

// ------------------------------------------------------------------ attention: one harness over every product launcher
// sc_diag_attention_run in three steps, each written once: the descriptor's rules, the geometry (both host arithmetic, before the runtime
// is looked at), then stage / launch / download.  The layouts and the NaN contract are in include/semcode_hip.h.
namespace {
const char* const ATTN = "sc_diag_attention_run";

sc_status attn_validate(const sc_diag_attn* a) {
    const int heads = a->heads, hd = a->head_dim;
    const bool window = a->mask == SC_DIAG_ATTN_WINDOW, causal = a->mask == SC_DIAG_ATTN_CAUSAL, cls = a->mask == SC_DIAG_ATTN_CLS;
    if (a->mask < SC_DIAG_ATTN_FULL || a->mask > SC_DIAG_ATTN_CLS) return sc_fail(SC_ERR_INVALID, "%s: mask %d is none of 0 (full), 1 (window), 2 (causal), 3 (CLS rows)", ATTN, a->mask);
    if (!a->lens || a->B < 1 || a->B > 65536 || a->blocked_rows < 0) return sc_fail(SC_ERR_INVALID, "%s: bad argument (lens, B 1 .. 65536, blocked_rows >= 0)", ATTN);
    if (causal) {
        if (!sc_attention_causal_supported(heads, a->kv_heads, hd))
            return sc_fail(SC_ERR_UNSUPPORTED, "%s: mask causal needs head_dim 64 or 128 and 1 <= kv_heads <= heads <= 2048 / head_dim with heads %% kv_heads == 0, got heads %d, kv_heads %d, head_dim %d",
                           ATTN, heads, a->kv_heads, hd);
    } else {
        if (heads < 1) return sc_fail(SC_ERR_INVALID, "%s: bad argument (heads %d)", ATTN, heads);
        if (hd != 64 && !(hd == 32 && heads % 2 == 0))
            return sc_fail(SC_ERR_UNSUPPORTED, "%s: head_dim must be 64, or 32 with an even number of heads (got %d, %d heads)", ATTN, hd, heads);
        if (heads > 2048 / hd) return sc_fail(SC_ERR_INVALID, "%s: bad argument (%d heads of %d: heads * head_dim beyond 2048)", ATTN, heads, hd);
        if (a->kv_heads && a->kv_heads != heads) return sc_fail(SC_ERR_UNSUPPORTED, "%s: kv_heads %d of %d heads needs mask causal, got mask %d", ATTN, a->kv_heads, heads, a->mask);
    }
    if (a->slopes && (window || causal)) return sc_fail(SC_ERR_UNSUPPORTED, "%s: mask %d has no ALiBi kernel (slopes must be NULL)", ATTN, a->mask);
    if (a->slopes && hd == 32 && !cls) return sc_fail(SC_ERR_UNSUPPORTED, "%s: head_dim 32 has no ALiBi kernel outside the CLS form (slopes must be NULL)", ATTN);
    if (window) {
        if (!sc_attention_window_supported(a->local_window)) return sc_fail(SC_ERR_UNSUPPORTED, "%s: local_window must be even and within 2 .. 128, got %d", ATTN, a->local_window);
        if (hd != 64) return sc_fail(SC_ERR_UNSUPPORTED, "%s: mask window (local_window) needs head_dim 64, got %d", ATTN, hd);
    }
    if (a->rel_bias) {
        if (a->mask != SC_DIAG_ATTN_FULL) return sc_fail(SC_ERR_UNSUPPORTED, "%s: rel_bias needs mask full, got mask %d", ATTN, a->mask);
        if (hd != 64) return sc_fail(SC_ERR_UNSUPPORTED, "%s: rel_bias needs head_dim 64, got %d", ATTN, hd);
        if (a->slopes) return sc_fail(SC_ERR_UNSUPPORTED, "%s: rel_bias and slopes exclude each other", ATTN);
        if (!sc_rel_buckets_valid(a->rel_buckets, a->rel_max_distance))
            return sc_fail(SC_ERR_INVALID, "%s: rel_buckets must be even, 4 .. 256, and rel_max_distance beyond rel_buckets / 4, got %d / %d", ATTN, a->rel_buckets, a->rel_max_distance);
    }
    if (cls) {
        if (a->starts || a->blocked_rows) return sc_fail(SC_ERR_UNSUPPORTED, "%s: mask CLS is a row-major rectangle: starts must be NULL and blocked_rows 0", ATTN);
        if (a->S < 1 || a->S > 2048) return sc_fail(SC_ERR_INVALID, "%s: mask CLS: S must be within 1 .. 2048, got %d", ATTN, a->S);
    }
    return SC_OK;
}

// rows_in x qkv_cols is what the launcher reads, rows_out x out_cols what comes back; a packed call's work items as the packed forward builds them
struct AttnGeom {
    int64_t rows_in = 0, rows_out = 0;
    int qkv_cols = 0, out_cols = 0;
    std::vector<int32_t> items;
    int nitems[3] = {0, 0, 0};
};
sc_status attn_geometry(const sc_diag_attn* a, AttnGeom& g) {
    g.out_cols = a->heads * a->head_dim;
    g.qkv_cols = (a->heads + 2 * (a->mask == SC_DIAG_ATTN_CAUSAL ? a->kv_heads : a->heads)) * a->head_dim;
    const int64_t tokens = (int64_t)a->B * a->S;
    if (a->mask == SC_DIAG_ATTN_CLS) {  // the harness blocks the rows itself, as the QKV projection writes them
        g.rows_in = ceil256(tokens), g.rows_out = a->B;
        return SC_OK;
    }
    if (!a->starts) {
        if (!sc_attention_supported(a->S, 64, 1, 64)) return sc_fail(SC_ERR_UNSUPPORTED, "%s: S must be one of 32,64,128,256,512,1024,2048, got %d", ATTN, a->S);
        if (a->blocked_rows && a->blocked_rows < tokens) return sc_fail(SC_ERR_INVALID, "%s: blocked_rows < B*S", ATTN);
        g.rows_in = a->blocked_rows ? (int64_t)a->blocked_rows : tokens, g.rows_out = tokens;
        return SC_OK;
    }
    int64_t end = 0, used = 0;
    for (int32_t b = 0; b < a->B; ++b) {
        const int32_t start = a->starts[b], len = a->lens[b];
        if (len < 1 || len > 2048 || start < 0 || (start % 32) || start > (1 << 24))
            return sc_fail(SC_ERR_INVALID, "%s: sequence %d: start %d (multiple of 32) / length %d (1..2048) out of range", ATTN, b, start, len);
        used += ceil32(len);
        if (start + ceil32(len) > end) end = start + ceil32(len);
    }
    const int64_t R = a->blocked_rows ? (int64_t)a->blocked_rows : ceil256(end);
    if (R < end) return sc_fail(SC_ERR_INVALID, "%s: blocked_rows %d < the last sequence's end %lld", ATTN, a->blocked_rows, (long long)end);
    g.rows_in = g.rows_out = R;
    g.items.resize((size_t)sc_packed_items_cap(used, a->B) * 4);  // by the rows the sequences own: they may overlap here
    sc_packed_items(a->starts, a->lens, a->B, g.items.data(), g.nitems);
    return SC_OK;
}
}  // namespace

extern "C" sc_status sc_diag_attention_run(sc_runtime* rt, const sc_diag_attn* a, const float* qkv, float* out) {
    if (!a || !qkv || !out) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", ATTN);
    SC_TRY(attn_validate(a));
    AttnGeom g;
    SC_TRY(attn_geometry(a, g));
    if (!rt) return sc_fail(SC_ERR_INVALID, "%s: the runtime is NULL", ATTN);
    const bool packed = a->starts != nullptr;
    const int B = a->B, S = a->S, heads = a->heads, hd = a->head_dim, H = g.out_cols, blocked = a->blocked_rows;
    std::vector<float> cls_rows;  // mask CLS: qkv [B*S][3H] laid out in 64-column blocks of rows_in rows, the padding rows zero
    if (a->mask == SC_DIAG_ATTN_CLS) {
        const int64_t nblk = g.qkv_cols / 64;
        cls_rows.assign((size_t)(nblk * g.rows_in * 64), 0.f);
        for (int64_t r = 0; r < (int64_t)B * S; ++r)
            for (int64_t cb = 0; cb < nblk; ++cb) memcpy(&cls_rows[(size_t)(cb * g.rows_in + r) * 64], qkv + r * g.qkv_cols + cb * 64, 64 * sizeof(float));
        qkv = cls_rows.data();
    }
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fq, dq, dseq, dex, dc;
    SC_TRY(upload_bf16(qkv, g.rows_in * g.qkv_cols, fq, dq, s));
    if (packed) SC_TRY(upload(g.items.data(), g.items.size() * 4, dseq, s));
    else SC_TRY(upload(a->lens, (size_t)B * 4, dseq, s));
    if (a->slopes) SC_TRY(upload(a->slopes, (size_t)heads * 4, dex, s));
    SC_TRY(alloc_nan(dc, (size_t)g.rows_out * H * 2, s));
    if (a->rel_bias) SC_TRY(upload_rel_table(a->rel_bias, a->rel_buckets, heads, a->rel_max_distance, dex, s));
    const int32_t* seq = (const int32_t*)dseq.p;  // lens [B], or the packed items
    const float* ex = (const float*)dex.p;        // slopes, the distance table, or NULL
    switch (a->mask) {
    case SC_DIAG_ATTN_CLS: sc_launch_attention_cls(dq.p, nullptr, seq, B, S, (int)g.rows_in, H, hd, ex, dc.p, B, s); break;
    case SC_DIAG_ATTN_WINDOW:
        if (packed) sc_launch_attention_window_packed(dq.p, seq, g.nitems, H, a->local_window, dc.p, s, blocked);
        else sc_launch_attention_window(dq.p, seq, B, S, H, a->local_window, dc.p, s, blocked);
        break;
    case SC_DIAG_ATTN_CAUSAL:
        if (packed) sc_launch_attention_causal_packed(dq.p, seq, g.nitems, heads, a->kv_heads, hd, dc.p, s, blocked);
        else sc_launch_attention_causal(dq.p, seq, B, S, heads, a->kv_heads, hd, dc.p, s, blocked);
        break;
    default:
        if (a->rel_bias && packed) sc_launch_attention_rel_packed(dq.p, seq, g.nitems, H, ex, DIAG_REL_SPAN, dc.p, s, blocked);
        else if (a->rel_bias) sc_launch_attention_rel(dq.p, seq, B, S, H, ex, DIAG_REL_SPAN, dc.p, s, blocked);
        else if (packed) sc_launch_attention_packed(dq.p, seq, g.nitems, H, ex, dc.p, s, blocked, hd);
        else sc_launch_attention(dq.p, seq, B, S, H, ex, dc.p, s, blocked, hd);
    }
    return download_bf16(dc.p, g.rows_out * H, out, s);  // synchronises: cls_rows and the items may go
}

// The bucket rule alone: host arithmetic, no runtime (rel_bucket_rule.h, what builds the device table)
extern "C" sc_status sc_diag_rel_buckets(int32_t rel_buckets, int32_t max_distance, int32_t span, int32_t* out) {
    if (!out || span < 1 || span > (1 << 20)) return sc_fail(SC_ERR_INVALID, "sc_diag_rel_buckets: bad argument (span 1 .. 2^20)");
    if (!sc_rel_buckets_valid(rel_buckets, max_distance))
        return sc_fail(SC_ERR_INVALID, "sc_diag_rel_buckets: rel_buckets must be even, 4 .. 256, and max_distance beyond rel_buckets / 4, got %d / %d", rel_buckets,
                       max_distance);
    sc_rel_buckets(rel_buckets, max_distance, span, out);
    return SC_OK;
}

// qknorm_rope_kernel / qknorm_rope_packed_kernel on their own: x [rows, (heads + 2 kv_heads) * head_dim] f32 as [Q | K | V] -> bf16 in 64-column
// blocks [N / 64][rows][64], the Q and K heads normalised (gamma_q non-NULL) and rotated in place, everything widened and laid out row-major again
extern "C" sc_status sc_diag_qknorm_rope(sc_runtime* rt, float* x, int32_t rows, int32_t S, const int32_t* pos, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                         float theta, const float* gamma_q, const float* gamma_k, float eps) {
    const char* who = "sc_diag_qknorm_rope";
    if (!rt || !x || rows < 1 || rows > (1 << 24) || (gamma_q == nullptr) != (gamma_k == nullptr)) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    if (!sc_attention_causal_supported(heads, kv_heads, head_dim))
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: need head_dim 64 or 128 and 1 <= kv_heads <= heads <= 2048 / head_dim with heads %% kv_heads == 0, got heads %d, kv_heads %d, head_dim %d",
                       who, heads, kv_heads, head_dim);
    if (S < 1 || S > 65536 || (!pos && (S & (S - 1)))) return sc_fail(SC_ERR_INVALID, "%s: S must be a power of two (the table's length, 1 .. 65536, with pos)", who);
    if (gamma_q && !(eps > 0.f)) return sc_fail(SC_ERR_INVALID, "%s: eps must be > 0", who);
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    const int nb = (heads + 2 * kv_heads) * head_dim / 64;
    const int64_t n = (int64_t)rows * nb * 64;
    std::vector<float> blk((size_t)n);
    const std::vector<float> tab = sc_rope_table(S, theta, head_dim);
    for (int64_t r = 0; r < rows; ++r)
        for (int b = 0; b < nb; ++b) memcpy(&blk[((size_t)b * rows + r) * 64], x + ((size_t)r * nb + b) * 64, 256);
    sc_devbuf fb, db, dt, dp, dgq, dgk;
    SC_TRY(upload_bf16(blk.data(), n, fb, db, s));
    SC_TRY(upload(tab.data(), tab.size() * 4, dt, s));
    if (pos) SC_TRY(upload(pos, (size_t)rows * 4, dp, s));
    if (gamma_q) {
        SC_TRY(upload(gamma_q, (size_t)head_dim * 4, dgq, s));
        SC_TRY(upload(gamma_k, (size_t)head_dim * 4, dgk, s));
    }
    sc_launch_qknorm_rope(db.p, rows, heads, kv_heads, head_dim, S, pos ? (const int32_t*)dp.p : nullptr, S, (const float*)dt.p, (const float*)dt.p + tab.size() / 2,
                          gamma_q ? (const float*)dgq.p : nullptr, gamma_q ? (const float*)dgk.p : nullptr, eps, s);
    SC_TRY(download_bf16(db.p, n, blk.data(), s));
    for (int64_t r = 0; r < rows; ++r)
        for (int b = 0; b < nb; ++b) memcpy(x + ((size_t)r * nb + b) * 64, &blk[((size_t)b * rows + r) * 64], 256);
    return SC_OK;
}

// rmsnorm_kernel<3|4|8>: x [tokens,H] -> out [tokens,H] = x * rsqrt(mean(x^2) + eps) * gamma
extern "C" sc_status sc_diag_rmsnorm(sc_runtime* rt, const float* x, int32_t tokens, int32_t H, const float* gamma, float eps, float* out) {
    if (!rt || !x || !gamma || !out || tokens < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_rmsnorm: bad argument");
    if (H < 8 || (H % 8) || H > 2048 || !(eps > 0.f)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_rmsnorm: H must be a multiple of 8, <= 2048");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fx, dx, dg, dc;
    SC_TRY(upload_bf16(x, (int64_t)tokens * H, fx, dx, s));
    SC_TRY(upload(gamma, (size_t)H * 4, dg, s));
    SC_TRY(alloc_nan(dc, (size_t)tokens * H * 2, s));
    sc_launch_rmsnorm(dx.p, tokens, H, (const float*)dg.p, eps, dc.p, s);
    return download_bf16(dc.p, (int64_t)tokens * H, out, s);
}

// rope_qk_kernel on its own: qk [rows, heads * 64] f32 (row r = position r % S) -> bf16 in the blocked layout [heads][rows][64],
// rotated in place, widened and laid out row-major again.
extern "C" sc_status sc_diag_rope(sc_runtime* rt, float* qk, int32_t rows, int32_t S, int32_t heads, float theta) {
    if (!rt || !qk || rows < 1 || heads < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_rope: bad argument");
    if (S < 1 || S > 65536 || (S & (S - 1))) return sc_fail(SC_ERR_INVALID, "sc_diag_rope: S must be a power of two");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    const int64_t n = (int64_t)rows * heads * 64;
    std::vector<float> blk((size_t)n);
    const std::vector<float> tab = sc_rope_table(S, theta);
    for (int64_t r = 0; r < rows; ++r)
        for (int h = 0; h < heads; ++h) memcpy(&blk[((size_t)h * rows + r) * 64], qk + ((size_t)r * heads + h) * 64, 256);
    sc_devbuf fb, db, dt;
    SC_TRY(upload_bf16(blk.data(), n, fb, db, s));
    SC_TRY(upload(tab.data(), tab.size() * 4, dt, s));
    sc_launch_rope_qk(db.p, rows, heads, S, (const float*)dt.p, (const float*)dt.p + tab.size() / 2, s);
    SC_TRY(download_bf16(db.p, n, blk.data(), s));
    for (int64_t r = 0; r < rows; ++r)
        for (int h = 0; h < heads; ++h) memcpy(qk + ((size_t)r * heads + h) * 64, &blk[((size_t)h * rows + r) * 64], 256);
    return SC_OK;
}

// layernorm_kernel<3|4|8>: x [tokens,H] -> out [tokens,H]
extern "C" sc_status sc_diag_layernorm(sc_runtime* rt, const float* x, int32_t tokens, int32_t H, const float* gamma, const float* beta, float eps, float* out) {
    if (!rt || !x || !gamma || !beta || !out || tokens < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_layernorm: bad argument");
    if (H < 8 || (H % 8) || H > 2048 || !(eps > 0.f)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_layernorm: H must be a multiple of 8, <= 2048");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fx, dx, dg, db, dc;
    SC_TRY(upload_bf16(x, (int64_t)tokens * H, fx, dx, s));
    SC_TRY(upload(gamma, (size_t)H * 4, dg, s));
    SC_TRY(upload(beta, (size_t)H * 4, db, s));
    SC_TRY(alloc_nan(dc, (size_t)tokens * H * 2, s));
    sc_launch_layernorm(dx.p, tokens, H, (const float*)dg.p, (const float*)db.p, eps, dc.p, s);
    return download_bf16(dc.p, (int64_t)tokens * H, out, s);
}

// sc_launch_mean_pool: normalize 0 = mean_pool_sliced_kernel, 1 = mean_pool_kernel with the L2 normalisation.  x [B*S,H] -> out [B,H] f32
extern "C" sc_status sc_diag_mean_pool(sc_runtime* rt, const float* x, const int32_t* lens, int32_t B, int32_t S, int32_t H, int32_t normalize, float* out) {
    if (!rt || !x || !lens || !out || B < 1 || S < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_mean_pool: bad argument");
    if (H < 8 || (H % 8)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_mean_pool: H must be a multiple of 8");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fx, dx, dl, dout;
    SC_TRY(upload_bf16(x, (int64_t)B * S * H, fx, dx, s));
    SC_TRY(upload(lens, (size_t)B * 4, dl, s));
    SC_TRY(alloc_nan(dout, (size_t)B * H * 4, s));
    sc_launch_mean_pool(dx.p, (const int32_t*)dl.p, B, S, H, normalize ? 1 : 0, (float*)dout.p, s);
    return download(dout.p, (size_t)B * H * 4, out, s);
}

// mean_pool_ln_kernel: y [tokens_pad,H] raw rows (the first B*S are read), stats [slots][tokens_pad][2] -> out [B,H] f32
extern "C" sc_status sc_diag_mean_pool_ln(sc_runtime* rt, const float* y, const float* stats, int32_t slots, int32_t tokens_pad, const float* gamma,
                                          const float* beta, float eps, const int32_t* lens, int32_t B, int32_t S, int32_t H, float* out) {
    if (!rt || !y || !stats || !gamma || !beta || !lens || !out || B < 1 || S < 1 || slots < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_mean_pool_ln: bad argument");
    if (H < 8 || (H % 8) || !(eps > 0.f)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_mean_pool_ln: H must be a multiple of 8");
    if ((int64_t)tokens_pad < (int64_t)B * S) return sc_fail(SC_ERR_INVALID, "sc_diag_mean_pool_ln: tokens_pad < B*S");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fy, dy, dst, dg, db, dl, dout;
    SC_TRY(upload_bf16(y, (int64_t)tokens_pad * H, fy, dy, s));
    SC_TRY(upload(stats, (size_t)slots * tokens_pad * 8, dst, s));
    SC_TRY(upload(gamma, (size_t)H * 4, dg, s));
    SC_TRY(upload(beta, (size_t)H * 4, db, s));
    SC_TRY(upload(lens, (size_t)B * 4, dl, s));
    SC_TRY(alloc_nan(dout, (size_t)B * H * 4, s));
    sc_launch_mean_pool_ln(dy.p, (const float*)dst.p, slots, tokens_pad, (const float*)dg.p, (const float*)db.p, eps, (const int32_t*)dl.p, B, S, H, (float*)dout.p, s);
    return download(dout.p, (size_t)B * H * 4, out, s);
}

// The kernels between the two FFN GEMMs, kind = the model's ffn_type.  The gates (1 glu_kernel<ActGelu>, 2 swiglu_kernel, 4
// glu_kernel<ActGeluTanh>): h [rows, 2F] (gate | up) -> out [rows, F] = act(gate) * up; 3: relu_kernel, in place on the bf16-rounded h [rows, F]
extern "C" sc_status sc_diag_ffn_act(sc_runtime* rt, int32_t kind, const float* h, int32_t rows, int32_t F, float* out) {
    const char* who = "sc_diag_ffn_act";
    if (kind < 1 || kind > 4) return sc_fail(SC_ERR_INVALID, "%s: kind must be 1 (GEGLU), 2 (SwiGLU), 3 (ReLU) or 4 (tanh-GELU gate), got %d", who, kind);
    if (!rt || !h || !out || rows < 1 || F < 8 || (F % 8)) return sc_fail(SC_ERR_INVALID, "%s: bad argument (F must be a multiple of 8)", who);
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf fh, dh, dc;
    SC_TRY(upload_bf16(h, (int64_t)rows * (kind == 3 ? 1 : 2) * F, fh, dh, s));
    if (kind == 3) {
        sc_launch_relu(dh.p, (int64_t)rows * F, s);
        return download_bf16(dh.p, (int64_t)rows * F, out, s);
    }
    SC_TRY(alloc_nan(dc, (size_t)rows * F * 2, s));
    if (kind == 1) sc_launch_geglu(dh.p, rows, F, dc.p, s);
    else if (kind == 2) sc_launch_swiglu(dh.p, rows, F, dc.p, s);
    else sc_launch_geglu_tanh(dh.p, rows, F, dc.p, s);
    return download_bf16(dc.p, (int64_t)rows * F, out, s);
}

// output_proj_kernel on its own: x [B,H] f32 as it is (the pooled rows are f32), W [E,H], bias [E] or NULL -> out [B,E]
extern "C" sc_status sc_diag_output_proj(sc_runtime* rt, const float* x, int32_t B, int32_t H, const float* W, const float* bias, int32_t E, int32_t normalize,
                                         float* out) {
    const char* who = "sc_diag_output_proj";
    if (!rt || !x || !W || !out || B < 1 || B > 65536 * 16) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    if (!sc_output_proj_supported(H, E)) return sc_fail(SC_ERR_INVALID, "%s: H and E must be multiples of 16 within 16 .. 2048, got %d, %d", who, H, E);
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf dx, dw, db, dout;
    SC_TRY(upload(x, (size_t)B * H * 4, dx, s));
    SC_TRY(upload(W, (size_t)E * H * 4, dw, s));
    if (bias) SC_TRY(upload(bias, (size_t)E * 4, db, s));
    SC_TRY(alloc_nan(dout, (size_t)B * E * 4, s));
    sc_launch_output_proj((const float*)dx.p, B, H, (const float*)dw.p, bias ? (const float*)db.p : nullptr, E, normalize, (float*)dout.p, s);
    return download(dout.p, (size_t)B * E * 4, out, s);
}

// The embedding kernels.  ln == 0: embed_raw_kernel -> rows [tokens_pad,H] + stats [slots][tokens_pad][2]; ln != 0: embed_ln_kernel ->
// rows [tokens,H] (tokens_pad, slots, stats unused).  ids [tokens] (tokens = B*S, position = token % S), wemb [vocab,H], pemb [max_pos,H] or
// NULL, temb [>= 1, H] (row 0 is used), all f32.
extern "C" sc_status sc_diag_embed(sc_runtime* rt, int32_t ln, const int32_t* ids, int32_t tokens, int32_t S, int32_t H, int32_t vocab, int32_t max_pos,
                                   const float* wemb, const float* pemb, const float* temb, const float* gamma, const float* beta, float eps,
                                   int32_t tokens_pad, int32_t slots, float* rows, float* stats) {
    if (!rt || !ids || !wemb || !temb || !rows || tokens < 1 || S < 1 || vocab < 1 || max_pos < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_embed: bad argument");
    if (H < 4 || (H % 4) || H > 2048) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_embed: H must be a multiple of 4, <= 2048");
    if (ln && (!gamma || !beta || !(eps > 0.f))) return sc_fail(SC_ERR_INVALID, "sc_diag_embed: the LayerNorm form needs gamma, beta, eps");
    if (!ln && (!stats || tokens_pad < tokens || slots < 1 || slots > 64)) return sc_fail(SC_ERR_INVALID, "sc_diag_embed: the raw form needs stats, tokens_pad >= tokens, 1 <= slots <= 64");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf di, dw, dp, dt, dg, db, dout, dst;
    SC_TRY(upload(ids, (size_t)tokens * 4, di, s));
    SC_TRY(upload(wemb, (size_t)vocab * H * 4, dw, s));
    if (pemb) SC_TRY(upload(pemb, (size_t)max_pos * H * 4, dp, s));
    SC_TRY(upload(temb, (size_t)H * 4, dt, s));
    const int64_t nrows = ln ? tokens : tokens_pad;
    SC_TRY(alloc_nan(dout, (size_t)nrows * H * 2, s));
    if (ln) {
        SC_TRY(upload(gamma, (size_t)H * 4, dg, s));
        SC_TRY(upload(beta, (size_t)H * 4, db, s));
        sc_launch_embed_ln((const int32_t*)di.p, tokens, S, H, vocab, max_pos, (const float*)dw.p, pemb ? (const float*)dp.p : nullptr, (const float*)dt.p,
                           (const float*)dg.p, (const float*)db.p, eps, dout.p, s);
    } else {
        SC_TRY(alloc_nan(dst, (size_t)slots * tokens_pad * 8, s));
        sc_launch_embed_raw((const int32_t*)di.p, tokens, tokens_pad, S, H, vocab, max_pos, (const float*)dw.p, pemb ? (const float*)dp.p : nullptr,
                            (const float*)dt.p, dout.p, (float*)dst.p, slots, s);
        SC_TRY(download(dst.p, (size_t)slots * tokens_pad * 8, stats, s));
    }
    return download_bf16(dout.p, nrows * H, rows, s);
}

// The typed embedding kernels of encoder_pairs.hip: sc_diag_embed with a position and a segment id per row (pos / types [tokens]) instead
// of token % S and type 0; temb [type_vocab, H].
extern "C" sc_status sc_diag_embed_pairs(sc_runtime* rt, int32_t ln, const int32_t* ids, const int32_t* pos, const int32_t* types, int32_t tokens, int32_t H,
                                         int32_t vocab, int32_t max_pos, int32_t type_vocab, const float* wemb, const float* pemb, const float* temb,
                                         const float* gamma, const float* beta, float eps, int32_t tokens_pad, int32_t slots, float* rows, float* stats) {
    if (!rt || !ids || !pos || !types || !wemb || !temb || !rows || tokens < 1 || vocab < 1 || max_pos < 1 || type_vocab < 1)
        return sc_fail(SC_ERR_INVALID, "sc_diag_embed_pairs: bad argument");
    if (H < 4 || (H % 4) || H > 2048) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_embed_pairs: H must be a multiple of 4, <= 2048");
    if (ln && (!gamma || !beta || !(eps > 0.f))) return sc_fail(SC_ERR_INVALID, "sc_diag_embed_pairs: the LayerNorm form needs gamma, beta, eps");
    if (!ln && (!stats || tokens_pad < tokens || slots < 1 || slots > 64))
        return sc_fail(SC_ERR_INVALID, "sc_diag_embed_pairs: the raw form needs stats, tokens_pad >= tokens, 1 <= slots <= 64");
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf di, dpo, dty, dw, dp, dt, dg, db, dout, dst;
    SC_TRY(upload(ids, (size_t)tokens * 4, di, s));
    SC_TRY(upload(pos, (size_t)tokens * 4, dpo, s));
    SC_TRY(upload(types, (size_t)tokens * 4, dty, s));
    SC_TRY(upload(wemb, (size_t)vocab * H * 4, dw, s));
    if (pemb) SC_TRY(upload(pemb, (size_t)max_pos * H * 4, dp, s));
    SC_TRY(upload(temb, (size_t)type_vocab * H * 4, dt, s));
    const int64_t nrows = ln ? tokens : tokens_pad;
    SC_TRY(alloc_nan(dout, (size_t)nrows * H * 2, s));
    if (ln) {
        SC_TRY(upload(gamma, (size_t)H * 4, dg, s));
        SC_TRY(upload(beta, (size_t)H * 4, db, s));
        sc_launch_embed_ln_pairs((const int32_t*)di.p, (const int32_t*)dpo.p, (const int32_t*)dty.p, tokens, H, vocab, max_pos, type_vocab, (const float*)dw.p,
                                 pemb ? (const float*)dp.p : nullptr, (const float*)dt.p, (const float*)dg.p, (const float*)db.p, eps, dout.p, s);
    } else {
        SC_TRY(alloc_nan(dst, (size_t)slots * tokens_pad * 8, s));
        sc_launch_embed_raw_pairs((const int32_t*)di.p, (const int32_t*)dpo.p, (const int32_t*)dty.p, tokens, tokens_pad, H, vocab, max_pos, type_vocab,
                                  (const float*)dw.p, pemb ? (const float*)dp.p : nullptr, (const float*)dt.p, dout.p, (float*)dst.p, slots, s);
        SC_TRY(download(dst.p, (size_t)slots * tokens_pad * 8, stats, s));
    }
    return download_bf16(dout.p, nrows * H, rows, s);
}

// pair_head_kernel on host f32 data, as they are (nothing is rounded): cls [B,H], pooler_w [H,H] / pooler_b [H] or both NULL,
// cls_w [num_labels,H], cls_b [num_labels] -> out_logits [B,num_labels].
extern "C" sc_status sc_diag_pair_head(sc_runtime* rt, const float* cls, int32_t B, int32_t H, const float* pooler_w, const float* pooler_b, const float* cls_w,
                                       const float* cls_b, int32_t num_labels, float* out_logits) {
    if (!rt || !cls || !cls_w || !cls_b || !out_logits || (pooler_w && !pooler_b)) return sc_fail(SC_ERR_INVALID, "sc_diag_pair_head: NULL argument");
    if (B < 1 || B > 65536) return sc_fail(SC_ERR_INVALID, "sc_diag_pair_head: batch %d out of range", B);
    if (num_labels < 1 || num_labels > 2) return sc_fail(SC_ERR_INVALID, "sc_diag_pair_head: num_labels %d outside 1 .. 2", num_labels);
    if (!sc_pair_head_supported(H, num_labels)) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_pair_head: H must be a multiple of 16, <= 2048 (got %d)", H);
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf dx, dwp, dbp, dwc, dbc, dout;
    SC_TRY(upload(cls, (size_t)B * H * 4, dx, s));
    if (pooler_w) {
        SC_TRY(upload(pooler_w, (size_t)H * H * 4, dwp, s));
        SC_TRY(upload(pooler_b, (size_t)H * 4, dbp, s));
    }
    SC_TRY(upload(cls_w, (size_t)num_labels * H * 4, dwc, s));
    SC_TRY(upload(cls_b, (size_t)num_labels * 4, dbc, s));
    SC_TRY(alloc_nan(dout, (size_t)B * num_labels * 4, s));
    sc_launch_pair_head((const float*)dx.p, B, H, pooler_w ? (const float*)dwp.p : nullptr, pooler_w ? (const float*)dbp.p : nullptr, (const float*)dwc.p,
                        (const float*)dbc.p, num_labels, (float*)dout.p, s);
    return download(dout.p, (size_t)B * num_labels * 4, out_logits, s);
}

// score_head_kernel / score_linear_kernel on host f32 data, as they are: rows [B,H] and the head's arrays -> out_logits [B,num_labels].
extern "C" sc_status sc_diag_score_head(sc_runtime* rt, const float* rows, int32_t B, int32_t H, const sc_score_head* h, float* out_logits) {
    if (!rt || !rows || !h || !out_logits) return sc_fail(SC_ERR_INVALID, "sc_diag_score_head: NULL argument");
    if (B < 1 || B > 65536) return sc_fail(SC_ERR_INVALID, "sc_diag_score_head: batch %d out of range", B);
    SC_TRY(sc_score_head_check(h, -1, H, "sc_diag_score_head"));
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    const int nl = h->num_labels;
    sc_devbuf dx, dwd, dbd, dg, db, dwc, dbc, dout;
    SC_TRY(upload(rows, (size_t)B * H * 4, dx, s));
    if (h->dense_w) SC_TRY(upload(h->dense_w, (size_t)H * H * 4, dwd, s));
    if (h->dense_b) SC_TRY(upload(h->dense_b, (size_t)H * 4, dbd, s));
    if (h->norm_g) SC_TRY(upload(h->norm_g, (size_t)H * 4, dg, s));
    if (h->norm_b) SC_TRY(upload(h->norm_b, (size_t)H * 4, db, s));
    SC_TRY(upload(h->cls_w, (size_t)nl * H * 4, dwc, s));
    if (h->cls_b) SC_TRY(upload(h->cls_b, (size_t)nl * 4, dbc, s));
    SC_TRY(alloc_nan(dout, (size_t)B * nl * 4, s));
    sc_launch_score_head((const float*)dx.p, B, H, (const float*)dwd.p, (const float*)dbd.p, (const float*)dg.p, (const float*)db.p, h->norm_eps, (const float*)dwc.p,
                         (const float*)dbc.p, nl, (float*)dout.p, s);
    return download(dout.p, (size_t)B * nl * 4, out_logits, s);
}

// ------------------------------------------------------------------ late interaction: MaxSim alone
// the arguments both forms take: offsets start at 0 and ascend, every query has 1 .. 128 tokens, every pair index is in range
static sc_status maxsim_check(const char* who, const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int32_t* d_off, int32_t Bd, const int32_t* pair_q,
                              const int32_t* pair_d, int32_t P, int32_t W, const float* out) {
    if (!Q || !q_off || !D || !d_off || !pair_q || !pair_d || !out) return sc_fail(SC_ERR_INVALID, "%s: NULL argument", who);
    if (Bq < 1 || Bd < 1 || P < 1) return sc_fail(SC_ERR_INVALID, "%s: need Bq, Bd, P >= 1 (got %d, %d, %d)", who, Bq, Bd, P);
    if (!maxsim_width_ok(W)) return sc_fail(SC_ERR_INVALID, "%s: W = %d must be a multiple of 16 within 16 .. 128", who, W);
    if (q_off[0] != 0 || d_off[0] != 0) return sc_fail(SC_ERR_INVALID, "%s: offsets must start at 0", who);
    for (int32_t i = 0; i < Bq; ++i)
        if (q_off[i + 1] - q_off[i] < 1 || q_off[i + 1] - q_off[i] > MAXSIM_MAX_NQ)
            return sc_fail(SC_ERR_INVALID, "%s: query %d has %d tokens (1 .. %d)", who, i, q_off[i + 1] - q_off[i], MAXSIM_MAX_NQ);
    for (int32_t i = 0; i < Bd; ++i)
        if (d_off[i + 1] - d_off[i] < 1) return sc_fail(SC_ERR_INVALID, "%s: document %d has %d tokens", who, i, d_off[i + 1] - d_off[i]);
    for (int32_t p = 0; p < P; ++p)
        if (pair_q[p] < 0 || pair_q[p] >= Bq || pair_d[p] < 0 || pair_d[p] >= Bd)
            return sc_fail(SC_ERR_INVALID, "%s: pair %d = (%d, %d) outside the %d queries / %d documents", who, p, pair_q[p], pair_d[p], Bq, Bd);
    return SC_OK;
}

// The rule on the CPU: the same header the kernel compiles (tests on a machine without a GPU).
extern "C" sc_status sc_diag_maxsim_host(const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int32_t* d_off, int32_t Bd, const uint8_t* keep,
                                         const int32_t* pair_q, const int32_t* pair_d, int32_t P, int32_t W, float* out) {
    SC_TRY(maxsim_check("sc_diag_maxsim_host", Q, q_off, Bq, D, d_off, Bd, pair_q, pair_d, P, W, out));
    for (int32_t p = 0; p < P; ++p) {
        const int32_t q0 = q_off[pair_q[p]], d0 = d_off[pair_d[p]];
        out[p] = maxsim_score_seq(Q + (size_t)q0 * W, q_off[pair_q[p] + 1] - q0, D + (size_t)d0 * W, d_off[pair_d[p] + 1] - d0, keep ? keep + d0 : nullptr, W);
    }
    return SC_OK;
}

extern "C" sc_status sc_diag_maxsim(sc_runtime* rt, const float* Q, const int32_t* q_off, int32_t Bq, const float* D, const int32_t* d_off, int32_t Bd,
                                    const uint8_t* keep, const int32_t* pair_q, const int32_t* pair_d, int32_t P, int32_t W, float* out) {
    if (!rt) return sc_fail(SC_ERR_INVALID, "sc_diag_maxsim: NULL argument");
    SC_TRY(maxsim_check("sc_diag_maxsim", Q, q_off, Bq, D, d_off, Bd, pair_q, pair_d, P, W, out));
    SC_HIP(hipSetDevice(rt->device));
    hipStream_t s = rt->stream;
    sc_devbuf dq, dqo, dd, ddo, dk, dpq, dpd, dout;
    SC_TRY(upload(Q, (size_t)q_off[Bq] * W * 4, dq, s));
    SC_TRY(upload(q_off, ((size_t)Bq + 1) * 4, dqo, s));
    SC_TRY(upload(D, (size_t)d_off[Bd] * W * 4, dd, s));
    SC_TRY(upload(d_off, ((size_t)Bd + 1) * 4, ddo, s));
    if (keep) SC_TRY(upload(keep, (size_t)d_off[Bd], dk, s));
    SC_TRY(upload(pair_q, (size_t)P * 4, dpq, s));
    SC_TRY(upload(pair_d, (size_t)P * 4, dpd, s));
    SC_TRY(alloc_nan(dout, (size_t)P * 4, s));
    sc_launch_maxsim((const float*)dq.p, (const int32_t*)dqo.p, (const float*)dd.p, (const int32_t*)ddo.p, (const uint8_t*)dk.p, (const int32_t*)dpq.p,
                     (const int32_t*)dpd.p, P, W, (float*)dout.p, s);
    return download(dout.p, (size_t)P * 4, out, s);
}

// The plan of a packed call without a device or a handle: the rules of its kind (kind = PackedCall::Kind: 0 texts, 1 pairs, 2 scored,
// 3 tokens) under the model bounds given as plain values, then the filler into a buffer sized by PlanOffsets; out as sc_diag_ivf_plan's.
extern "C" sc_status sc_diag_encoder_plan(const int32_t* ids, const int64_t* offsets, int32_t B, int32_t kind, const int32_t* first_lens, int32_t expand_id,
                                          int32_t query, int32_t max_pos, int32_t pos_type, int32_t vocab, int32_t type_vocab, int32_t arch, int32_t global_every,
                                          int32_t local_window, void* out, int64_t cap_bytes, int64_t* need_bytes) {
    const char* who = "sc_diag_encoder_plan";
    if (!ids || !need_bytes || kind < 0 || kind > 3 || (kind == 1 && !first_lens)) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    const PlanBounds mb{max_pos, pos_type, vocab, type_vocab, arch, global_every, local_window, MAXSIM_MAX_NQ};
    int64_t used = 0, nrows = B;
    if (kind == PackedCall::TOKENS) SC_TRY(sc_plan_check_tokens(offsets, B, expand_id, query != 0, mb, who, &used, &nrows));
    else SC_TRY(sc_plan_check_offsets(offsets, B, mb, who, &used));
    if (kind == PackedCall::PAIRS) SC_TRY(sc_plan_check_pairs(offsets, first_lens, B, mb, who));
    PackedCall call = kind == PackedCall::PAIRS ? PackedCall::pairs(first_lens) : kind == PackedCall::TOKENS ? PackedCall::tokens(expand_id, nullptr) : PackedCall{};
    call.kind = (PackedCall::Kind)kind;
    const int64_t M = ceil256(used);
    const PlanOffsets po((size_t)M, (size_t)B, call.kind);
    std::vector<char> buf(po.total, (char)0xCD);
    int nitems[3];
    const int64_t rows = sc_plan_fill(ids, offsets, B, call, po, M, buf.data(), nitems);
    DiagBlob bl;
    bl.put("ids", 0, buf.data() + po.ids, (size_t)M, 4), bl.put("pos", 0, buf.data() + po.pos, (size_t)M, 4);
    bl.put("starts", 0, buf.data() + po.starts, (size_t)B, 4), bl.put("lens", 0, buf.data() + po.lens, (size_t)B, 4);
    bl.put("items", 0, buf.data() + po.items, (size_t)(nitems[0] + nitems[1] + nitems[2]) * 4, 4), bl.put("nitems", 0, nitems, 3, 4);
    if (kind == PackedCall::PAIRS) bl.put("types", 0, buf.data() + po.types, (size_t)M, 4), bl.put("ones", 0, buf.data() + po.ones, (size_t)B, 4);
    if (kind == PackedCall::TOKENS) bl.put("dst", 0, buf.data() + po.dst, (size_t)M, 4);
    bl.num("rows", rows), bl.num("M", M), bl.num("nrows", nrows), bl.num("items_cap", sc_packed_items_cap(M, B)), bl.num("plan_bytes", (int64_t)po.total);
    bl.num("common_bytes", (int64_t)PlanOffsets((size_t)M, (size_t)B).total);
    bl.put("common", 2, buf.data(), PlanOffsets((size_t)M, (size_t)B).total / 4, 4);
    bl.give(out, cap_bytes, need_bytes);
    return SC_OK;
}

// The plan of the documents' token call under keep flags (sc_encoder_embed_tokens_into), without a device or a handle: the rules of a
// document-side token call, the kept counts, then the filler.  keep NULL: every token is kept.  out as sc_diag_encoder_plan's.
extern "C" sc_status sc_diag_encoder_plan_keep(const int32_t* ids, const int64_t* offsets, int32_t B, const uint8_t* keep, int32_t max_pos, int32_t pos_type,
                                               int32_t vocab, void* out, int64_t cap_bytes, int64_t* need_bytes) {
    const char* who = "sc_diag_encoder_plan_keep";
    if (!ids || !need_bytes) return sc_fail(SC_ERR_INVALID, "%s: bad argument", who);
    const PlanBounds mb{max_pos, pos_type, vocab, 2, 0, 0, 0, MAXSIM_MAX_NQ};
    int64_t used = 0, nrows = 0;
    SC_TRY(sc_plan_check_tokens(offsets, B, -1, false, mb, who, &used, &nrows));
    std::vector<int32_t> counts((size_t)B);
    const int64_t kept = sc_plan_kept_counts(offsets, B, keep, counts.data());
    const PackedCall call = PackedCall::kept_tokens(keep, nullptr, 0);
    const int64_t M = ceil256(used);
    const PlanOffsets po((size_t)M, (size_t)B, call.kind);
    std::vector<char> buf(po.total, (char)0xCD);
    int nitems[3];
    const int64_t rows = sc_plan_fill(ids, offsets, B, call, po, M, buf.data(), nitems);
    DiagBlob bl;
    bl.put("ids", 0, buf.data() + po.ids, (size_t)M, 4), bl.put("pos", 0, buf.data() + po.pos, (size_t)M, 4);
    bl.put("starts", 0, buf.data() + po.starts, (size_t)B, 4), bl.put("lens", 0, buf.data() + po.lens, (size_t)B, 4);
    bl.put("dst", 0, buf.data() + po.dst, (size_t)M, 4), bl.i32("counts", counts);
    bl.num("rows", rows), bl.num("M", M), bl.num("nrows", nrows), bl.num("kept", kept);
    bl.give(out, cap_bytes, need_bytes);
    return SC_OK;
}
