// sc_search.cpp -- the flat-search planner and its stages (exact scan, batched coarse stages with their collect pass), the dispatch
// between them and the IVF probes of sc_ivf_probe.cpp / sc_ivf_coarse.cpp, and the search entry points of the C ABI.  Caller holds ix->mu in every *_locked.
#include <algorithm>
#include <chrono>
#include <vector>

#include "sc_internal.h"

// ---- shared openings of the search functions

sc_status sc_prep_queries(sc_index* ix, const float* q_dev, int32_t Q) {
    sc_status st = sc_grow(ix, ix->qpad, (size_t)Q * ix->ld * 4);
    if (st) return st;
    st = sc_grow(ix, ix->qnorm, (size_t)Q * 4);
    if (st) return st;
    sc_launch_ingest_rows(q_dev, nullptr, 0, Q, ix->dim, ix->qpad.as<float>(), ix->ld, ix->qnorm.as<float>(), ix->rt->stream);
    return SC_OK;
}

sc_status sc_subbatch_stage(sc_index* ix, sc_buf& buf, const float* q_dev, const std::vector<int>& which, int k, sc_subbatch* sb) {
    const int R = (int)which.size();
    const size_t qb = ((size_t)R * ix->dim * 4 + 255) & ~(size_t)255, db = ((size_t)R * k * 4 + 255) & ~(size_t)255, rb = ((size_t)R * k * 8 + 255) & ~(size_t)255;
    sc_status st = sc_grow(ix, buf, qb + db + rb + (size_t)R * 4);
    if (st) return st;
    char* b = buf.as<char>();
    *sb = {(float*)b, (float*)(b + qb), (int64_t*)(b + qb + db), (int32_t*)(b + qb + db + rb), R};
    // one gather and two scatters by query index (one hipMemcpyAsync per query cost ~9 us each); `which` must outlive the copy:
    // sc_subbatch_scatter synchronises
    SC_HIP(hipMemcpyAsync(sb->idx, which.data(), (size_t)R * 4, hipMemcpyHostToDevice, ix->rt->stream));
    sc_launch_copy_rows_indexed(q_dev, sb->q, sb->idx, R, (size_t)ix->dim * 4, false, ix->rt->stream);
    return SC_OK;
}

sc_status sc_subbatch_scatter(sc_index* ix, const sc_subbatch& sb, int k, float* out_dist, int64_t* out_rows) {
    sc_launch_copy_rows_indexed(sb.d, out_dist, sb.idx, sb.R, (size_t)k * 4, true, ix->rt->stream);
    sc_launch_copy_rows_indexed(sb.r, out_rows, sb.idx, sb.R, (size_t)k * 8, true, ix->rt->stream);
    SC_HIP(hipStreamSynchronize(ix->rt->stream));
    return SC_OK;
}

// The exact scan over stored rows [first, first + nrows).  q_dev: tight [Q, dim] device; outputs device.  perm: stored position -> row
// id, or null where positions equal row ids (an untrained index; the tail behind the lists of a trained IVF index).
static sc_status search_exact_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int64_t first, int64_t nrows, const uint32_t* perm, float* out_dist,
                                     int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    ScanPlan plan;
    if (!sc_scan_exact_plan(ix->ld, Q, k, rt->cus, &plan, 0, 0, nrows))
        return sc_fail(SC_ERR_UNSUPPORTED, "search: k=%d (1..1024) / dim=%d not supported by the exact scan", k, ix->dim);
    sc_status st = sc_prep_queries(ix, q_dev, Q);
    if (st) return st;
    st = sc_grow(ix, ix->partial, std::max<size_t>(plan.partial_bytes, 16));
    if (st) return st;
    uint64_t* partial = ix->partial.as<uint64_t>();
    hipEvent_t e0, e1;
    if (nrows > 0) {
        sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
        sc_launch_scan_exact((int)ix->metric, ix->X + (size_t)first * ix->ld, ix->xnorm + first, nrows, ix->ld, ix->qpad.as<float>(), ix->qnorm.as<float>(), Q, k, plan, partial,
                             perm, nullptr, nullptr, 0, s);
        sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
    }
    sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
    sc_launch_topk_merge((int)ix->metric, partial, plan.groups, nrows > 0 ? plan.lists : 0, plan.qt, Q, k, ix->row_base + first, out_dist, out_rows, s);
    sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// ---- batched path (scan_batched.h): bf16 / int8 shadow + coarse GEMM phases + exact re-rank + certified fallback

static const int BATCH_CAP = 4096;        // survivors kept per query and phase
// first phase: every row of it survives (thresholds start at +inf), so it must stay well below BATCH_CAP; each next phase covers 4x
// more rows.  256 rows when the selection was a quadratic rank sort; with the radix select and the two-pass epilogue of the dense
// phases 2 048 saves two launches + selections per batch (10M rows: 9 -> 7 phases).  SC_PHASE0 overrides (A/B).
static int64_t phase0_rows() {
    static const int64_t x = sc_env_i64("SC_PHASE0", 2048), v = x >= 256 && x <= 2048 ? (x / 256) * 256 : 2048;
    return v;
}

static int coarse_pin(const sc_index* ix);
static int64_t i8_min_rows() {  // corpora below this never build an int8 shadow (SC_I8_MINROWS: A/B)
    static const int64_t v = sc_env_i64("SC_I8_MINROWS", (int64_t)1 << 20);
    return v;
}
static int i8_min_queries() {
    static const int v = (int)sc_env_i64("SC_I8_MINQ", 1);
    return v;
}
static bool batched_applicable(const sc_index* ix, int Q, int k) {
    if (ix->search_mode == 1) return false;
    if (ix->n < 1) return false;
    // top_k beyond 64: only the int8 stage has the candidates for it (512: k <= 256); without it the exact scan answers -- one pass
    // per 16 queries, the cliff this removes where the int8 stage may run (10M x 768, 256 queries, top-100: see profiles/r3z_k100.log)
    if (k > sc_batched_kprime() / 2) {
        // (up to 128: beyond, the keys within the cut outgrow the wide set's 4 096 -- 256 queries, top-256 overflowed for most of them)
        const bool i8_ok = k <= sc_batched_kprime8() / 4 && !ix->i8_off && coarse_pin(ix) != 16 && (ix->n >= i8_min_rows() || ix->search_mode == 2);
        if (!i8_ok) return false;
        return ix->search_mode == 2 || Q >= i8_min_queries();
    }
    if (ix->search_mode == 2) return true;
    static const int64_t min_rows = sc_env_i64("SC_BATCHED_MINROWS", 4096);  // A/B
    if (Q > 16) return ix->n >= min_rows;
    // 16 queries and fewer: the exact scan reads the f32 rows once (10M x 768: 4.8 ms); where the int8 stage may run, its narrow
    // streaming kernel reads a quarter of the bytes and the certificate still makes the result exact: 1.7 ms for one query, 1.9 for
    // 16 (scripts/q_sweep.py, profiles/r3z_q_small.log).  SC_I8_MINQ > 1 restores the exact scan below that many queries (A/B).
    return ix->n >= i8_min_rows() && !ix->i8_off && coarse_pin(ix) != 16 && Q >= i8_min_queries();
}

// The int8 stage is tried first (twice the MFMA rate, half the shadow bytes); what it cannot certify goes to the bf16 stage, and
// only what that cannot certify either to the exact scan.  SC_COARSE=bf16 | i8 pins the stage (A/B runs, tests).
static int coarse_env();
static int coarse_pin(const sc_index* ix) { return ix->coarse_mode ? ix->coarse_mode : coarse_env(); }
static int coarse_env() {
    static const int v = [] {
        const char* e = getenv("SC_COARSE");
        if (!e) return 0;
        return (e[0] == 'b' || e[0] == 'B') ? 16 : (e[0] == 'i' || e[0] == 'I') ? 8 : 0;
    }();
    return v;
}

static int g_wide_force = 0;  // sc_diag_set_option("wide_candidates", 1): the int8 stage runs its wide form wherever it can (tests)
void sc_set_wide_force(int v) { g_wide_force = v; }
static int g_tighten = 1;  // sc_diag_set_option("tighten", 0): thresholds stay the kp-th coarse keys (tests, A/B)
void sc_set_tighten(int v) { g_tighten = v; }
static int g_collect_pass = 1;  // sc_diag_set_option("collect_pass", 0): uncertified queries go straight to the next stage (tests, A/B)
void sc_set_collect_pass(int v) { g_collect_pass = v; }

// The collect pass (scan_rerank.hip, "the collect pass"): the sub-batch `fq` [R][dim] of queries a stage could not certify, with
// that stage's results in fd / fr [R][k] (fd's k-th column bounds the k-th score).  Resolved queries get their final results
// written into fd / fr; `left` receives the sub-batch positions of those that still need the next stage (more than BATCH_CAP rows
// within the bound, or no bound).  Uses the same scratch as the stage that called it (which is done with it).
static sc_status search_collect_locked(sc_index* ix, const float* fq, int R, int k, float* fd, int64_t* fr, bool i8, std::vector<int>& left) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int metric = (int)ix->metric, ld = ix->ld, ld8 = sc_ld8(ix);
    const sc_shadow& sh = i8 ? ix->sh_i8 : ix->sh_b16;
    const int Qpad = (i8 || R > 64) ? (R + 255) / 256 * 256 : 128;
    static_assert(BATCH_CAP == 4096, "the refine kernels' candidate stride (sc_ivf_widen_cap) is the survivor cap");
    if (sc_ivf_widen_cap() != BATCH_CAP) return sc_fail(SC_ERR_STATE, "collect pass: candidate stride mismatch");
    sc_carver carve;
    const size_t o_qres = carve((size_t)R * 4), o_amax = carve(16);
    const size_t o_qb = carve(i8 ? (size_t)Qpad * ld8 : (size_t)Qpad * ld * 2), o_qs = carve((size_t)Qpad * 4), o_thr = carve((size_t)Qpad * 4),
                 o_tf = carve((size_t)Qpad * 4), o_cnt = carve((size_t)R * 4), o_ovf = carve((size_t)R * 4), o_flag = carve((size_t)R * 4), o_nc = carve((size_t)R * 4),
                 o_surv = carve((size_t)R * BATCH_CAP * 8), o_ek = carve((size_t)R * BATCH_CAP * 8);
    const size_t hit_bytes = (i8 && R <= 64) ? (size_t)2048 * (4 + 1024 * 16) + 256 : 0;
    const size_t o_hits = carve(hit_bytes ? hit_bytes : 16);
    sc_status st = sc_grow(ix, ix->bscratch, carve.off);
    if (st) return st;
    char* b = ix->bscratch.as<char>();
    void* Qb = b + o_qb;
    float *qres = (float*)(b + o_qres), *qscale = (float*)(b + o_qs), *thr = (float*)(b + o_thr), *tf = (float*)(b + o_tf);
    unsigned* cnt = (unsigned*)(b + o_cnt);
    int *ovf = (int*)(b + o_ovf), *flags = (int*)(b + o_flag), *ncand = (int*)(b + o_nc);
    uint64_t *surv = (uint64_t*)(b + o_surv), *ekeys = (uint64_t*)(b + o_ek);
    st = sc_prep_queries(ix, fq, R);
    if (st) return st;
    float *const qpad = ix->qpad.as<float>(), *const qnorm = ix->qnorm.as<float>();
    if (i8) sc_launch_query_i8(qpad, R, Qpad, ld, ld8, Qb, qscale, qres, (unsigned*)(b + o_amax), s);
    else sc_launch_query_bf16(qpad, R, Qpad, ld, Qb, qres, s);
    sc_launch_scan_batched_init(thr, tf, Qpad, nullptr, cnt, ovf, R, 0, s);
    sc_launch_scan_collect_bound(metric, fd, k, qnorm, qres, sh.maxima, ld, thr, tf, flags, R, s);
    hipEvent_t e0, e1;
    sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
    if (i8) sc_launch_scan_coarse(metric, sh.arr[0].p, ix->xnorm, 0, ix->n, ld8, Qb, qnorm, R, Qpad, thr, tf, surv, cnt, BATCH_CAP, s, true, sh.arr[1].as<float>(), qscale, false, hit_bytes ? (void*)(b + o_hits) : nullptr, hit_bytes);
    else sc_launch_scan_coarse(metric, sh.arr[0].p, ix->xnorm, 0, ix->n, ld, Qb, qnorm, R, Qpad, thr, tf, surv, cnt, BATCH_CAP, s, false, nullptr, nullptr, false);
    sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
    sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
    sc_launch_scan_collect_counts(cnt, BATCH_CAP, ncand, flags, R, s);
    sc_launch_scan_rerank_keys(metric, ix->X, ix->xnorm, ld, qpad, qnorm, surv, ncand, BATCH_CAP, ix->perm, ekeys, R, s);
    sc_launch_refine_finalize(metric, ekeys, ncand, flags, k, ix->row_base, fd, fr, R, s);
    sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
    SC_HIP(hipGetLastError());
    std::vector<int> hflags(R);
    SC_HIP(hipMemcpyAsync(hflags.data(), flags, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    left.clear();
    for (int j = 0; j < R; ++j)
        if (hflags[j]) left.push_back(j);
    return SC_OK;
}

static sc_status search_batched_stage_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows, bool i8, int depth,
                                             int Q_top) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    const int metric = (int)ix->metric, ld = ix->ld, KP = i8 ? sc_batched_kprime8() : sc_batched_kprime();
    const int ld8 = sc_ld8(ix);
    const sc_shadow& sh = i8 ? ix->sh_i8 : ix->sh_b16;
    // 256-wide query tiles for batches above 64 queries (always for the int8 stage); 65 .. 128 queries used to take the 128-query tiles:
    // 1M x 768, 65 queries 2.02 ms there against 0.86 ms for 256 queries on the 256-wide tiles (profiles/r3z_q_rows.log)
    const int Qpad = (i8 || Q > 64) ? (Q + 255) / 256 * 256 : 128;
    // the wide candidate set (scan_select.hip): on corpora whose certificate fails at kp candidates the int8 stage keeps every key
    // within its exact-score cut -- needs the cuts (tightening: 2 k <= 128, a corpus beyond 2^17 rows) and 64 KiB of keys per query
    static const bool tighten_env = sc_env_flag("SC_TIGHTEN", true);  // A/B
    // (the cut needs the k-th exact score among re-scored candidates: the 128 best for k <= 64, all 512 of the int8 stage beyond)
    const bool tighten = tighten_env && g_tighten && (2 * k <= 128 || (i8 && 2 * k <= KP));
    const int TK = 2 * k <= 128 ? 128 : KP;
    const int WB = BATCH_CAP;  // capacity of the wide set
    // (top_k beyond 64 goes straight to the wide form: the 512-candidate certificate is hopeless there -- 256 queries, top-100 over 10M x 768:
    // 5.9 ms, against 211 ms through the exact scan, profiles/r3z_k100.log)
    const bool big_k = k > sc_batched_kprime() / 2;
    const bool wide = i8 && tighten && (ix->wide_i8 || g_wide_force || big_k) && depth == 0 && Q <= 16384 && ix->n > ((int64_t)1 << 18);
    const int KB = wide ? WB : KP;  // row stride of `best`
    sc_status st = i8 ? sc_ensure_shadow_i8(ix) : sc_ensure_shadow_b16(ix);
    if (st) return st;
    // scratch layout
    sc_carver carve;
    const size_t o_qres = carve((size_t)Q * 4), o_amax = carve(16);
    const size_t o_qb = carve(i8 ? (size_t)Qpad * ld8 : (size_t)Qpad * ld * 2), o_qs = carve((size_t)Qpad * 4), o_thr = carve((size_t)Qpad * 4),
                 o_tf = carve((size_t)Qpad * 4), o_cnt = carve((size_t)Q * 4), o_ovf = carve((size_t)Q * 4), o_flag = carve((size_t)Q * 4),
                 o_best = carve((size_t)Q * KB * 8), o_ek = carve(i8 ? (size_t)Q * KB * 8 : 16), o_surv = carve((size_t)Q * BATCH_CAP * 8),
                 o_nbest = carve((size_t)Q * 4), o_wcand = carve((size_t)Q * KB * 8), o_wnc = carve((size_t)Q * 4),
                 o_b128 = carve((size_t)Q * 512 * 8), o_e128 = carve((size_t)Q * 512 * 8), o_cut = carve((size_t)Qpad * 4), o_cnt2 = carve((size_t)Q * 4),
                 o_thrT = carve((size_t)Qpad * 4), o_tfT = carve((size_t)Qpad * 4);
    // per-wave hit lists of the narrow int8 kernel (batches of <= 64 queries): 2048 lists x 1024 entries of 16 B
    const size_t hit_bytes = (i8 && Q <= 64) ? (size_t)2048 * (4 + 1024 * 16) + 256 : 0;
    const size_t o_hits = carve(hit_bytes ? hit_bytes : 16);
    // the fallback sub-batch (depth 1) runs while the caller's scratch is no longer needed: one buffer serves both
    st = sc_grow(ix, ix->bscratch, carve.off);
    if (st) return st;
    char* b = ix->bscratch.as<char>();
    void* Qb = b + o_qb;
    float* qres = (float*)(b + o_qres);
    float *qscale = (float*)(b + o_qs), *thr = (float*)(b + o_thr), *tf = (float*)(b + o_tf);
    unsigned* cnt = (unsigned*)(b + o_cnt);
    int *ovf = (int*)(b + o_ovf), *flags = (int*)(b + o_flag);
    uint64_t *best = (uint64_t*)(b + o_best), *ekeys = (uint64_t*)(b + o_ek), *surv = (uint64_t*)(b + o_surv);

    st = sc_prep_queries(ix, q_dev, Q);
    if (st) return st;
    float *const qpad = ix->qpad.as<float>(), *const qnorm = ix->qnorm.as<float>();
    if (i8) sc_launch_query_i8(qpad, Q, Qpad, ld, ld8, Qb, qscale, qres, (unsigned*)(b + o_amax), s);
    else sc_launch_query_bf16(qpad, Q, Qpad, ld, Qb, qres, s);
    sc_launch_scan_batched_init(thr, tf, Qpad, best, cnt, ovf, Q, wide ? 0 : KP, s);  // (wide: `best` carries its own counts, no padding)
    unsigned* nbest = (unsigned*)(b + o_nbest);
    if (wide) SC_HIP(hipMemsetAsync(nbest, 0, (size_t)Q * 4, s));
    ix->last_wide = wide ? 1 : 0;
    // thresholds from exact scores before the large phases (scan_rerank.hip, scan_tighten_kernel): from 2^17 rows seen on
    // (10M x 768 x 1024, same box: from 2^19 8.45 ms per step, 2^17 8.38, 2^15 8.36; without 8.80)
    float* thr_cut = (float*)(b + o_cut);
    bool cut_used = false;
    if (tighten) sc_launch_fill_u32((unsigned*)thr_cut, 0x7F800000u, Qpad, s);  // +inf
    int64_t r0 = 0, span = phase0_rows();
    while (r0 < ix->n) {
        const int64_t r1 = std::min(ix->n, r0 + span);
        hipEvent_t e0, e1;
        static const int64_t tighten_from = sc_env_i64("SC_TIGHTEN_FROM", (int64_t)1 << 17);  // A/B
        // (wide form: a cut before every phase but the first -- nothing may be truncated at kp while keys within reach of the k-th exact
        // score can still arrive; the first selection keeps all of its 2 048 rows)
        if (tighten && r0 >= (wide ? (int64_t)1 : tighten_from)) {
            uint64_t *b128 = (uint64_t*)(b + o_b128), *e128 = (uint64_t*)(b + o_e128);
            unsigned* cnt2 = (unsigned*)(b + o_cnt2);
            sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
            const uint64_t* from = best;
            if (wide || KP > TK) {  // the TK best of the candidates (a selection over `best` as if it were a survivor list)
                if (wide) SC_HIP(hipMemcpyAsync(cnt2, nbest, (size_t)Q * 4, hipMemcpyDeviceToDevice, s));
                else sc_launch_fill_u32(cnt2, (unsigned)KP, Q, s);
                SC_HIP(hipMemsetAsync(b128, 0xFF, (size_t)Q * TK * 8, s));
                sc_launch_scan_select(metric, best, cnt2, KB, b128, qnorm, (float*)(b + o_thrT), (float*)(b + o_tfT), (int*)(b + o_wnc), Q, TK, s);
                from = b128;
            }
            sc_launch_scan_rerank_keys(metric, ix->X, ix->xnorm, ld, qpad, qnorm, from, nullptr, TK, ix->perm, e128, Q, s);
            sc_launch_scan_tighten(metric, e128, TK, k, qnorm, qres, sh.maxima, ld, thr, tf, thr_cut, Q, s);
            sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
            cut_used = true;
        }
        sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
        // a query keeps about KP of the r0 rows seen so far: a 256 x 256 tile of this phase about 65536 KP / r0 survivors -- above a few
        // hundred the two-pass epilogue (one list-slot atomic per query and tile instead of one per survivor)
        const bool dense = r0 < (int64_t)256 * KP;
        if (i8) sc_launch_scan_coarse(metric, sh.arr[0].p, ix->xnorm, r0, r1, ld8, Qb, qnorm, Q, Qpad, thr, tf, surv, cnt, BATCH_CAP, s, true, sh.arr[1].as<float>(), qscale, dense, hit_bytes ? (void*)(b + o_hits) : nullptr, hit_bytes);
        else sc_launch_scan_coarse(metric, sh.arr[0].p, ix->xnorm, r0, r1, ld, Qb, qnorm, Q, Qpad, thr, tf, surv, cnt, BATCH_CAP, s, false, nullptr, nullptr, dense);
        sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
        sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
        if (wide) sc_launch_scan_select_wide(metric, surv, cnt, BATCH_CAP, best, nbest, WB, cut_used ? KP : WB, qnorm, thr, tf, thr_cut, ovf, Q, s);
        else sc_launch_scan_select(metric, surv, cnt, BATCH_CAP, best, qnorm, thr, tf, ovf, Q, KP, s);
        sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
        r0 = r1;
        span *= 4;
    }
    if (cut_used) sc_launch_scan_thr_min(thr, thr_cut, Q, s);  // the certificate's threshold: no looser than any cut that was applied
    // (the plain form can take the same final step over its kp slots -- SC_FINAL_COMPACT=1 -- but gains nothing from it: on the Gaussian
    // benchmark ~200 of the 512 lie within the final threshold, and the step measures 8.47 ms either way)
    static const bool compact_env = sc_env_flag("SC_FINAL_COMPACT", false);
    const bool compact_final = !wide && i8 && cut_used && compact_env;
    if (wide || compact_final) {  // the keys within the final threshold, re-scored exactly; exact top-k; the certificate as a kernel of its own
        uint64_t* wcand = (uint64_t*)(b + o_wcand);
        int* wnc = (int*)(b + o_wnc);
        hipEvent_t e0, e1;
        sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
        if (!wide) sc_launch_fill_u32(nbest, (unsigned)KP, Q, s);
        sc_launch_scan_wide_compact(metric, best, nbest, KB, thr, wcand, wnc, Q, s);
        sc_launch_scan_rerank_keys(metric, ix->X, ix->xnorm, ld, qpad, qnorm, wcand, wnc, KB, ix->perm, ekeys, Q, s);
        SC_HIP(hipMemsetAsync(flags, 0, (size_t)Q * 4, s));
        sc_launch_refine_finalize(metric, ekeys, wnc, flags, k, ix->row_base, out_dist, out_rows, Q, s, KB);
        sc_launch_scan_wide_certify(metric, out_dist, k, qnorm, qres, sh.maxima, ld, thr, ovf, flags, Q, s);
        sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
    } else {
        sc_launch_scan_rerank(metric, ix->X, ix->xnorm, ld, qpad, qnorm, best, thr, sh.maxima, qres, ovf, Q, k, ix->row_base,
                              ix->perm, out_dist, out_rows, flags, s, KP, ekeys);
    }
    SC_HIP(hipGetLastError());
    // uncertified queries: hand them to the next stage (int8 -> bf16 -> exact scan)
    std::vector<int> hflags(Q);
    SC_HIP(hipMemcpyAsync(hflags.data(), flags, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    std::vector<int> redo;
    for (int i = 0; i < Q; ++i)
        if (hflags[i]) redo.push_back(i);
    int R = (int)redo.size();
    if (i8) {
        // most of a real batch uncertified: this corpus does not quantise well enough (tight clusters, outlier dimensions) --
        // later searches start at the bf16 stage until the rows are replaced wholesale
        // (first resort: the wide candidate set -- the next batch keeps every key within the exact-score cut; if that fails too, bf16)
        if (depth == 0 && coarse_pin(ix) != 8 && !ix->i8_sticky && !big_k) {  // (a large top_k says nothing about the corpus)
            const bool wide_possible = tighten && Q <= 16384 && ix->n > ((int64_t)1 << 18);
            // the wide form is never wrong and costs a few percent where it is not needed: a small batch that fails is evidence enough for it
            // (one clustered query: 3.1 ms through plain form + collect pass, 2.0 ms wide); giving up on int8 takes a real batch
            if (!wide && wide_possible && !ix->wide_i8) {
                if (R * 2 > Q) ix->wide_i8 = true;
            } else if (Q >= 32 && R * 4 > Q) {
                ix->i8_off = true;
            }
        }
    }
    // second chance at this stage's precision: the collect pass (every row within the coarse error of the k-th exact score found)
    bool& collect_off = i8 ? ix->collect_off8 : ix->collect_off16;
    if (R > 0 && g_collect_pass && !collect_off) {
        sc_subbatch sb;
        st = sc_subbatch_stage(ix, depth == 0 ? ix->fb : ix->fb2, q_dev, redo, k, &sb);
        if (st) return st;
        sc_launch_copy_rows_indexed(out_dist, sb.d, sb.idx, R, (size_t)k * 4, false, s);  // the failed pass's results: their k-th score is the bound
        sc_launch_copy_rows_indexed(out_rows, sb.r, sb.idx, R, (size_t)k * 8, false, s);
        std::vector<int> left;
        st = search_collect_locked(ix, sb.q, R, k, sb.d, sb.r, i8, left);
        if (st) return st;
        st = sc_subbatch_scatter(ix, sb, k, out_dist, out_rows);
        if (st) return st;
        ix->last_collect_tried += R;
        ix->last_collect_resolved += R - (int)left.size();
        if (R >= 32 && (int)left.size() * 2 > R) collect_off = true;
        std::vector<int> still;
        for (int j : left) still.push_back(redo[(size_t)j]);
        redo.swap(still);
        R = (int)redo.size();
    }
    if (i8) ix->last_uncert_i8 = R;
    // (a handful of queries is one pass of the exact scan: not worth a bf16 shadow; top_k beyond 64 is beyond the bf16 stage's 128 candidates)
    const bool to_bf16 = i8 && coarse_pin(ix) != 8 && R > 16 && k <= sc_batched_kprime() / 2;
    if (!to_bf16) {  // what is left goes to the exact scan
        ix->last_uncertified = R;
        ix->uncert_frac = (double)R / (double)Q_top;
    }
    if (R > 0) {
        // the sub-batch gets its own staging (queries + results); nested stages each need one: fb for the first, fb2 for the second
        sc_subbatch sb;
        st = sc_subbatch_stage(ix, depth == 0 ? ix->fb : ix->fb2, q_dev, redo, k, &sb);
        if (st) return st;
        if (to_bf16) st = search_batched_stage_locked(ix, sb.q, R, k, sb.d, sb.r, false, depth + 1, Q_top);
        else st = search_exact_locked(ix, sb.q, R, k, 0, ix->n, ix->perm, sb.d, sb.r);
        if (st) return st;
        st = sc_subbatch_scatter(ix, sb, k, out_dist, out_rows);  // (synchronises: `redo` is on this stack frame)
        if (st) return st;
    }
    ix->last_path = 2;
    return SC_OK;
}

static sc_status search_batched_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows) {
    const int env = coarse_pin(ix);
    // The int8 stage halves the coarse GEMM but re-ranks 512 candidates per query instead of 128 (512 * ld * 4 B of scattered rows
    // each): it pays from about a million rows up (10M x 768: coarse 12.9 -> 7.0 ms against +0.3 ms of re-rank).  Small corpora --
    // above all the IVF quantizer, whose nearest-centroid searches of a build went 6.4 -> 16.4 s through it at 4096 x 3072
    // (profiles/r2i_kernel_stats.csv: scan_rerank_kernel 7.4 s) -- start at the bf16 stage.
    // (search mode 2, "batched whenever supported", is the tests' switch: it keeps the int8 stage eligible at any size.)
    // ... and from 129 queries up: the int8 stage always runs 256-query tiles, and a batch of 32 spends 4.05 ms in them against the
    // 3.8 ms of the bf16 stage's 128-query tiles (profiles/r2p_bench.json.log sweep vs r1v)
    // (round 3: the persistent int8 kernel answers a 32-query batch in 3.1 ms where the bf16 stage's 128-query tiles take 3.9: the
    // int8 stage now starts at 17 queries; SC_I8_MINQ restores any other limit for A/B runs)
    const int i8_minq = i8_min_queries();  // (round 3, later: from one query on -- batched_applicable)
    const bool i8 = env == 8 || (env == 0 && !ix->i8_off && ((ix->n >= i8_min_rows() && Q >= i8_minq) || (Q > 16 && Q <= 64 && ix->n >= 65536) || ix->search_mode == 2));
    // (17 .. 64 queries from 65 536 rows on: that batch size is the narrow streaming kernel's -- 1M x 768, 64 queries: 0.71 ms against
    // 2.01 through the bf16 stage's 128-query tiles; 300k rows: 0.51 against 1.74 -- profiles/r3z_q_rows.log)
    ix->last_coarse_bits = i8 ? 8 : 16;
    ix->last_uncert_i8 = 0;
    ix->last_uncertified = 0;
    ix->last_collect_tried = ix->last_collect_resolved = 0;
    // Which stage to START at on a corpus the int8 certificate fails on is settled by the clock: the int8 stage switches itself off
    // when it fails for a quarter of a batch (above); the cost per query of that batch (int8 pass + its collect pass + whatever went
    // on) is remembered, and if the bf16-first batch that follows costs more (tight clusters: bf16 needs its collect pass too, at
    // twice the bytes and half the MFMA rate), the int8 stage is switched back on for good.  10M x 768, 4096 clusters of spread
    // 0.1: 26.2 ms bf16-first, 16.9 ms int8-first (profiles/r3z_clustered_probe.log).
    const bool was_off = ix->i8_off;
    const auto t0 = std::chrono::steady_clock::now();
    const sc_status st = search_batched_stage_locked(ix, q_dev, Q, k, out_dist, out_rows, i8, 0, Q);
    if (st == SC_OK && env == 0 && Q >= 64 && !ix->i8_sticky) {
        const double per_q = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / Q;
        if (i8 && !was_off && ix->i8_off) ix->cost_i8_first = per_q;  // the batch that switched the int8 stage off
        else if (!i8 && was_off && ix->cost_i8_first > 0.0 && ix->last_collect_tried * 4 > Q) {
            if (ix->cost_i8_first < 0.85 * per_q) {
                ix->i8_off = false;
                ix->i8_sticky = true;
            }
            ix->cost_i8_first = 0.0;  // decided either way
        }
    }
    return st;
}

sc_status sc_search_flat_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, float* out_dist, int64_t* out_rows) {
    ix->last_uncertified = 0;
    if (batched_applicable(ix, Q, k)) return search_batched_locked(ix, q_dev, Q, k, out_dist, out_rows);
    const sc_status st = search_exact_locked(ix, q_dev, Q, k, 0, ix->n, ix->perm, out_dist, out_rows);
    if (st == SC_OK) ix->last_path = 1;
    return st;
}

static int64_t g_ivf_tail_rows = 65536;  // sc_diag_set_option("ivf_tail_rows", n): appended rows a trained index leaves behind its lists (0: fold them in at once)
void sc_set_ivf_tail_rows(int v) { g_ivf_tail_rows = v < 0 ? 65536 : v; }

static sc_status probe_dispatch_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows, bool tail_merged);

sc_status sc_search_dev_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows) {
    ix->last_probed_lists = 0;
    ix->last_unique_rows = ix->last_streamed_rows = 0;
    ix->last_groups = 0;
    ix->last_tail_rows = 0;
    // Rows APPENDED to a trained index since its lists were laid out.  Folding them in means re-ordering the corpus (a second copy
    // of it, the shadows that mirror the layout): 1.9 - 4.1 s per search at 10M x 768 when searches and upserts alternate
    // (scripts/upsert_search_interleave.py).  Milvus answers from its growing segment by brute force; the same here: up to 65 536
    // appended rows stay behind the lists as a tail, a probe answers from the lists AND from an exact scan of the tail (positions
    // there are row ids), merged; beyond that, or when listed rows were overwritten (their list may have changed), or for an
    // exhaustive search, the lists are refreshed as before.  A tail row is always seen -- the probed lists plus the whole tail --
    // so recall can only be higher than after the refresh.
    {
        int64_t tail = (ix->kind == SC_INDEX_IVF_FLAT && ix->trained && ix->perm) ? ix->n - ix->ivf_rows : 0;
        if (tail > 0 && tail <= g_ivf_tail_rows && !ix->dirty_rows.empty() && ix->search_mode != 1 && ix->search_mode != 2) {
            // listed rows were overwritten as well (a re-index: known chunks again, new ones appended): settle those first -- rows that
            // stayed in their lists (unchanged or lightly edited chunks) leave the layout alone and the tail a tail
            const sc_status rst = sc_ivf_refresh_locked(ix, true);
            if (rst && rst != SC_ERR_NOMEM) return rst;
            if (rst) (void)hipGetLastError();
            tail = ix->n - ix->ivf_rows;
        }
        if (tail > 0 && tail <= g_ivf_tail_rows && ix->dirty_rows.empty() && ix->search_mode != 1 && ix->search_mode != 2 && nprobe >= 1 && nprobe < ix->nlist_trained &&
            (sc_ivf_coarse_applicable(ix, Q, k, nprobe) || sc_ivf_applicable(ix, Q, nprobe) ||
             sc_ivf_listmajor_applicable(ix, Q, k, nprobe, batched_applicable(ix, Q, k)))) {
            const size_t db = ((size_t)Q * k * 4 + 255) & ~(size_t)255, rb = ((size_t)Q * k * 8 + 255) & ~(size_t)255;
            sc_status st = sc_grow(ix, ix->tailbuf, 2 * (db + rb));
            if (st) return st;
            char* tb = ix->tailbuf.as<char>();
            float *d1 = (float*)tb, *d2 = (float*)(tb + db);
            int64_t *r1 = (int64_t*)(tb + 2 * db), *r2 = (int64_t*)(tb + 2 * db + rb);
            st = probe_dispatch_locked(ix, q_dev, Q, k, nprobe, d1, r1, true);  // (the lists alone: topk_merge2 joins disjoint rows)
            if (st) return st;
            const int path = ix->last_path, unc = ix->last_uncertified;
            st = search_exact_locked(ix, q_dev, Q, k, ix->ivf_rows, tail, nullptr, d2, r2);  // (positions there are row ids)
            if (st) return st;
            sc_launch_topk_merge2((int)ix->metric, d1, r1, d2, r2, k, out_dist, out_rows, Q, ix->rt->stream);
            SC_HIP(hipGetLastError());
            ix->last_path = path;
            ix->last_uncertified = unc;
            ix->last_tail_rows = tail;
            return SC_OK;
        }
    }
    {   // rows upserted since the IVF lists were built join their lists first (no k-means): the reported ids of a
        // list-major corpus go through ix->perm, which must cover every stored row
        sc_status rst = sc_ivf_refresh_locked(ix);
        if (rst == SC_ERR_NOMEM && ix->perm) {
            // The re-layout needs a second copy of the corpus (246 GB at 10M x 3072).  Without it the rows upserted since the build
            // cannot join their lists -- but they can still be FOUND: extend the position -> row id map over the tail (positions
            // == row ids there, 4 B per row) and answer exhaustively (exact results) until a refresh or a rebuild succeeds.
            return sc_search_exhaustive_locked(ix, q_dev, Q, k, out_dist, out_rows);
        }
        if (rst) return rst;
    }
    return probe_dispatch_locked(ix, q_dev, Q, k, nprobe, out_dist, out_rows, false);
}

// which path answers.  tail_merged: rows lie behind the lists and the caller merges an exact scan of them into what this returns, so
// the answer must come from the lists alone -- never from a scan that covers the tail as well, whose rows would enter the merge twice.
static sc_status probe_dispatch_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows, bool tail_merged) {
    bool lists_only = tail_merged;  // ... or the first chunks of the batch were probed: the rest is probed too, not scanned exhaustively
    if (!sc_ivf_coarse_applicable(ix, Q, k, nprobe) && sc_ivf_applicable(ix, Q, nprobe)) return sc_ivf_search_locked(ix, q_dev, Q, k, nprobe, out_dist, out_rows);
    if (sc_ivf_coarse_applicable(ix, Q, k, nprobe)) {
        // per-query scratch of the coarse stage is ~200 KB (two survivor lists of 8 192 keys, the refine sets): very large batches go
        // through it in chunks of 4 096 queries (0.8 GB), each a full batch of its own
        const int chunk = 4096;
        int uncert = 0;
        int64_t uniq = 0, streamed = 0;
        int groups = 0;
        for (int q0 = 0; q0 < Q; q0 += chunk) {
            const int nq = std::min(chunk, Q - q0);
            const sc_status st = sc_ivf_search_coarse_locked(ix, q_dev + (size_t)q0 * ix->dim, nq, k, nprobe, out_dist + (size_t)q0 * k, out_rows + (size_t)q0 * k, q0 / chunk);
            if (st == SC_ERR_NOMEM) {
                // no room for the centred shadow (a quarter of the corpus again) or the stage's scratch: the exact probes need neither, and
                // they answer this chunk and the ones behind it (the chunks before it are answered already: same results either way).
                // The stage stays off until the lists are rebuilt (a failed hipMalloc of tens of GB per search is not free either).
                (void)hipGetLastError();
                ix->ivfc_off = true;
                sc_shadow_release(ix->sh_c8);
                sc_buf_free(ix->ivfc_scratch);
                q_dev += (size_t)q0 * ix->dim, out_dist += (size_t)q0 * k, out_rows += (size_t)q0 * k, Q -= q0;
                if (q0 > 0) lists_only = true;
                goto exact_probe;
            }
            if (st) return st;
            uncert += ix->last_uncertified;
            uniq = std::max(uniq, ix->last_unique_rows);
            streamed += ix->last_streamed_rows;
            groups += ix->last_groups;
        }
        ix->last_uncertified = ix->last_ivfc_uncertified = uncert;
        ix->last_unique_rows = uniq;
        ix->last_streamed_rows = streamed;
        ix->last_groups = groups;
        return SC_OK;
    }
exact_probe:
    if (sc_ivf_listmajor_applicable(ix, Q, k, nprobe, batched_applicable(ix, Q, k)))
        return sc_ivf_search_listmajor_locked(ix, q_dev, Q, k, nprobe, out_dist, out_rows);
    if (lists_only) {  // list-major has no plan here or was not the cheaper choice: the lists are probed all the same
        const int path = sc_ivf_exact_probe_path(ix->ld, Q, k, nprobe, ix->rt->cus);
        if (path == 4) return sc_ivf_search_listmajor_locked(ix, q_dev, Q, k, nprobe, out_dist, out_rows);
        if (path == 3) return sc_ivf_search_locked(ix, q_dev, Q, k, nprobe, out_dist, out_rows);
        return sc_fail(SC_ERR_UNSUPPORTED, "ivf search: k=%d / dim=%d / nprobe=%d not supported by an exact probe", k, ix->dim, nprobe);
    }
    return sc_search_exhaustive_locked(ix, q_dev, Q, k, out_dist, out_rows);  // (no tail is merged behind this: every stored row is scanned once)
}

extern "C" sc_status sc_index_search_dev(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist_dev,
                                         int64_t* out_rows_dev) {
    const sc_status st = sc_check_query_args("search", !ix || !q_dev || !out_dist_dev || !out_rows_dev, Q, k, 0);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    return sc_search_dev_locked(ix, q_dev, Q, k, nprobe, out_dist_dev, out_rows_dev);
}

extern "C" sc_status sc_index_search(sc_index* ix, const float* q, int32_t Q, int32_t k, int32_t nprobe, float* out_dist,
                                     int64_t* out_rows) {
    sc_status st = sc_check_query_args("search", !ix || !q || !out_dist || !out_rows, Q, k, 0);
    if (st) return st;
    std::lock_guard<std::mutex> g(ix->mu);
    SC_HIP(hipSetDevice(ix->rt->device));
    sc_host_io io;
    st = sc_stage_host_locked(ix, q, Q, k, nullptr, 0, &io);
    if (st) return st;
    st = sc_search_dev_locked(ix, io.q, Q, k, nprobe, io.dist, io.rows);
    if (st) return st;
    return sc_fetch_host_locked(ix, io, Q, k, out_dist, out_rows);
}
