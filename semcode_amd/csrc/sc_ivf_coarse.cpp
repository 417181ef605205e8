// sc_ivf_coarse.cpp -- list-major IVF probing behind the int8 coarse stage: the centred shadow, and the search as the sequence probe ->
// plan (sc_ivf_plan.cpp) -> grow scratch -> upload -> launch -> stats -> trace -> exact re-probe of the uncertified queries.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

#include "sc_internal.h"
#include "sc_ivf_plan.h"

// ---- list-major probing behind an int8 coarse stage (L2) ---------------------------------------------------------------------------
// ivf_coarse.hip has the idea: every list quantised relative to its centroid, one centred int8 query per (query, probed list)
// pair, coarse scores turned into lower bounds of the exact distance, then bound and refine.  Here: the plan (pairs bucketed by
// list, groups of up to 64 query slots, one work item per 256-row tile of a list x group) and the sequence
//   phase A  every query's NEAREST list(s) through the grouped streaming kernel (scan_coarse64s_kernel<GROUPED, DENSE>): all lower-bound
//            keys kept; the 128 best re-scored exactly (canonical fmaf chain from the original rows) -> T = k-th exact distance + allowance;
//   phase B  the other nprobe - 1 lists: rows with lower bound <= T survive;
//   refine   all survivors of both phases within T re-scored exactly, exact top-k.
// No probed row outside the re-scored set can be closer than the k-th result, so the results are those of the exact list-major path,
// bit for bit.  Queries whose survivor lists overflow or whose refine set exceeds 4096 rows are probed again exactly
// (scan_listgemm / scan_exact kernels).
static const int IVFC_CAP = 8192;  // survivors per query, phase A (everything it sees: 2 KP + one prefix at most)
static const int IVFC_CAPB = 16384; // ... and phase B (the rest of a long nearest list against the prefix's bound can be thousands)
static int g_ivf_refine_cap = 1 << 30;  // sc_diag_set_option("ivf_refine_cap", n): the coarse stage's refine step takes on at most n rows per query (tests of the exact re-probe)
void sc_ivf_set_refine_cap(int v) { g_ivf_refine_cap = v < 0 ? (1 << 30) : v; }

bool sc_ivf_coarse_applicable(const sc_index* ix, int Q, int k, int nprobe) {
    static const bool env_off = !sc_env_flag("SC_IVF_COARSE", true);
    if (ix->kind != SC_INDEX_IVF_FLAT || !ix->trained || !ix->quant || !ix->perm || (ix->metric != SC_METRIC_L2 && ix->metric != SC_METRIC_IP && ix->metric != SC_METRIC_COSINE)) return false;
    if (nprobe < 2 || nprobe > 512 || nprobe >= ix->nlist_trained || k < 1 || k > sc_batched_kprime8() / 2) return false;
    // what the stage cannot certify is probed again exactly, one query or many: without a plan for either the whole batch would be refused
    if (!sc_ivf_exact_probe_path(ix->ld, 1, k, nprobe, ix->rt->cus) || !sc_ivf_exact_probe_path(ix->ld, 2, k, nprobe, ix->rt->cus)) return false;
    if (ix->search_mode == 5) return Q >= 1;
    if (ix->search_mode != 0 || env_off || ix->ivfc_off) return false;
    // auto: any batch over a corpus worth a shadow.  The first rule here (Q >= 64 and Q nprobe >= nlist: "every list wanted by several
    // queries") was list-major thinking -- the stage's gain is the int8 bytes, not the sharing: at config 5 a batch of 32 queries
    // takes 22.9 ms through the per-query probe, 4.9 ms list-major exact and 1.9 ms here; of 2 queries 1.5 / 1.4 / 0.7 ms
    // (scripts/ivf_small_batch.py, profiles/r3z_ivf_small_batch*.log).  Fewer than 8 queries take it when ONE probe would stream a
    // gigabyte of f32 rows or more (config 5, one query: 0.50 ms against 0.83 through the per-query probe; 10M x 768 at the
    // reference's nlist 128 / nprobe 16: 0.51 against 0.67); below that the plan's round trip to the host costs more than the
    // bytes saved (1M x 768, 2 queries: 0.32 ms against 0.14).
    if (ix->n < 100000) return false;
    if (Q >= 8) return true;
    const double probed_bytes = (double)nprobe * ((double)ix->n / (double)ix->nlist_trained) * (double)ix->ld * 4.0;
    return probed_bytes >= 1.0e9;
}

// sc_diag_set_option("ivf_coarse_nomem", 1): the centred shadow cannot be allocated; 2: the stage runs out of memory from the second
// 4 096-query chunk of a batch on (tests of the fallbacks to the exact probes)
static int g_ivfc_nomem = 0;
void sc_ivf_set_coarse_nomem(int v) { g_ivfc_nomem = v; }
static sc_status ivfc_ensure_shadow(sc_index* ix) {
    sc_shadow& sh = ix->sh_c8;  // arr = {Xc8, xcs}, maxima = list_stats
    hipStream_t s = ix->rt->stream;
    const int ld8 = sc_ld8(ix), nlist = ix->nlist_trained;
    const bool unit = ix->metric == SC_METRIC_COSINE;  // the IP form on normalised rows and centroids
    if (sh.rows == ix->ivf_rows && sh.arr[0].p) {
        if (sh.dirty.empty()) return SC_OK;
        // rows of the lists overwritten in place and still in their lists (sc_ivf_refresh_locked found nothing to move, or the layout
        // would have been rebuilt and this shadow with it): their shadow rows alone; the per-list maxima keep accumulating
        std::vector<int64_t>& d = sh.dirty;
        std::sort(d.begin(), d.end());
        d.erase(std::unique(d.begin(), d.end()), d.end());
        while (!d.empty() && d.back() >= sh.rows) d.pop_back();
        if (!d.empty()) {
            sc_status st = sc_grow(ix, ix->stage, d.size() * 8);
            if (st) return st;
            SC_HIP(hipMemcpyAsync(ix->stage.p, d.data(), d.size() * 8, hipMemcpyHostToDevice, s));
            sc_launch_ivf_center_shadow(ix->X, (int64_t)d.size(), ix->ld, ld8, ix->quant->X, ix->quant->ld, ix->list_off, nlist, sh.arr[0].p, sh.arr[1].as<float>(),
                                        sh.maxima, s, unit ? ix->xnorm : nullptr, unit ? ix->quant->xnorm : nullptr, ix->stage.as<int64_t>());
            sc_launch_norm_max(ix->xnorm, sh.rows, sc_ivfc_xmax_slot(ix), s);
            SC_HIP(hipGetLastError());
            SC_HIP(hipStreamSynchronize(s));  // (the position list is a host temporary behind an asynchronous copy)
        }
        d.clear();
        return SC_OK;
    }
    sh.dirty.clear();  // a full build covers them
    if (g_ivfc_nomem == 1) return sc_fail(SC_ERR_NOMEM, "ivf coarse stage: out of device memory (forced by sc_diag_set_option)");
    const int64_t rows = ix->ivf_rows, rows_pad = (rows + 255) / 256 * 256 + sh.tail_pad;
    for (int i = 0; i < 2; ++i) {
        const sc_status st = sc_grow(ix, sh.arr[i], (size_t)rows_pad * sh.row_bytes[i]);
        if (st) return st;
    }
    // (the statistics were freed with the lists they described -- ivf_install_lists_locked --, so a buffer found here has nlist words)
    if (!sh.maxima && hipMalloc((void**)&sh.maxima, sc_ivfc_stats_words(nlist) * 4) != hipSuccess) {
        sh.maxima = nullptr;
        return sc_fail(SC_ERR_NOMEM, "ivf coarse stage: hipMalloc of the per-list statistics (%d lists) failed", nlist);
    }
    SC_HIP(hipMemsetAsync(sh.maxima, 0, sc_ivfc_stats_words(nlist) * 4, s));
    for (int i = 0; i < 2; ++i)
        SC_HIP(hipMemsetAsync(sh.arr[i].as<char>() + (size_t)rows * sh.row_bytes[i], 0, (size_t)(rows_pad - rows) * sh.row_bytes[i], s));
    sc_launch_ivf_center_shadow(ix->X, rows, ix->ld, ld8, ix->quant->X, ix->quant->ld, ix->list_off, nlist, sh.arr[0].p, sh.arr[1].as<float>(), sh.maxima, s,
                                unit ? ix->xnorm : nullptr, unit ? ix->quant->xnorm : nullptr);
    sc_launch_norm_max(ix->xnorm, rows, sc_ivfc_xmax_slot(ix), s);  // bits of max |x|^2: the re-rank's rounding allowance
    SC_HIP(hipGetLastError());
    sh.rows = rows;
    return SC_OK;
}

sc_status sc_ivf_search_coarse_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows, int chunk) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    sc_index* qz = ix->quant;
    const int ld = ix->ld, ld8 = sc_ld8(ix);
    if (g_ivfc_nomem == 2 && chunk >= 1) return sc_fail(SC_ERR_NOMEM, "ivf coarse stage: out of device memory at chunk %d (forced by sc_diag_set_option)", chunk);
    sc_status st = ivfc_ensure_shadow(ix);
    if (st) return st;
    // 1. coarse probe (the quantizer's own search) -> host; the probes stay in ivf_scratch, which the exact re-probe below reuses
    sc_ivf_probes pr;
    std::vector<int64_t> probes;
    st = sc_ivf_probe_quantizer_locked(ix, q_dev, Q, nprobe, 0, &pr, &probes);
    if (st) return st;
    // 2. plan (lives until the stream synchronisation below: its vectors are the sources of the uploads)
    IvfPlanParams pp;
    sc_ivf_plan_params(ld, k, nprobe, rt->cus, &pp);  // (only KP is read here; whether the exact list-major probe could serve does not matter)
    IvfCoarsePlan cp;
    sc_ivf_plan_coarse(probes.data(), Q, nprobe, ix->list_off_h.data(), ix->nlist_trained, pp, &cp);
    typedef IvfCoarseItem Item;
    const std::vector<Item>* const items = cp.items;
    const std::vector<unsigned>& cntA = cp.cntA;
    const int nslots = (int)cp.slot_q.size(), KP = pp.KP;
    const size_t nitems = cp.nitems();
    const bool two_level = cp.two_level;
    // 3. scratch: slot tables, per-pair queries, per-query state, survivor lists of both phases, hit lists, the refine stage's sets
    sc_carver carve;
    const int Qpad = (Q + 255) / 256 * 256;
    const int kpa = k <= sc_batched_kprime() / 2 ? sc_batched_kprime() : KP;  // phase-A candidates re-scored for the bound (128; 512 for k > 64)
    const int WCAP = sc_ivf_widen_cap();
    const size_t o_sq = carve((size_t)nslots * 4), o_sl = carve((size_t)nslots * 4), o_qs = carve((size_t)nslots * 4), o_qn = carve((size_t)nslots * 4),
                 o_st = carve((size_t)nslots * 4), o_stf = carve((size_t)nslots * 4), o_qb = carve((size_t)nslots * 4), o_qd = carve((size_t)nslots * 4),
                 o_se = carve((size_t)nslots * 4), o_sd = carve((size_t)nslots * 4), o_items = carve(nitems * sizeof(Item)), o_qc = carve((size_t)nslots * ld8),
                 o_thr = carve((size_t)Qpad * 4), o_tf = carve((size_t)Qpad * 4), o_cnt = carve((size_t)Q * 4), o_cntA = carve((size_t)Q * 4), o_ovf = carve((size_t)Q * 4),
                 o_flag = carve((size_t)Q * 4), o_nc = carve((size_t)Q * 4), o_best = carve((size_t)Q * kpa * 8), o_ekA = carve((size_t)Q * kpa * 8),
                 o_bestT = carve((size_t)Q * kpa * 8), o_ekT = carve((size_t)Q * kpa * 8), o_cntT = carve((size_t)Q * 4), o_thrT = carve((size_t)Qpad * 4), o_tfT = carve((size_t)Qpad * 4),
                 o_survA = carve((size_t)Q * IVFC_CAP * 8), o_survB = carve((size_t)Q * IVFC_CAPB * 8), o_cand = carve((size_t)Q * WCAP * 8),
                 o_ek2 = carve((size_t)Q * WCAP * 8);
    const size_t hit_bytes = (size_t)2048 * (4 + 8192 * 16) + 256;
    const size_t o_hits = carve(hit_bytes);
    st = sc_grow(ix, ix->ivfc_scratch, carve.off);
    if (st) return st;
    char* b = ix->ivfc_scratch.as<char>();
    int32_t *d_sq = (int32_t*)(b + o_sq), *d_sl = (int32_t*)(b + o_sl), *d_sd = (int32_t*)(b + o_sd);
    float *d_qs = (float*)(b + o_qs), *d_qn = (float*)(b + o_qn), *d_st = (float*)(b + o_st), *d_stf = (float*)(b + o_stf), *d_qb = (float*)(b + o_qb),
          *d_qd = (float*)(b + o_qd), *d_se = (float*)(b + o_se);
    float *thr = (float*)(b + o_thr), *tf = (float*)(b + o_tf);
    unsigned *cnt = (unsigned*)(b + o_cnt), *cntA_d = (unsigned*)(b + o_cntA);
    int *ovf = (int*)(b + o_ovf), *flags = (int*)(b + o_flag), *ncand = (int*)(b + o_nc);
    uint64_t *best = (uint64_t*)(b + o_best), *ekeysA = (uint64_t*)(b + o_ekA), *survA = (uint64_t*)(b + o_survA), *survB = (uint64_t*)(b + o_survB),
             *cand2 = (uint64_t*)(b + o_cand), *ekeys2 = (uint64_t*)(b + o_ek2);
    SC_HIP(hipMemcpyAsync(d_sq, cp.slot_q.data(), (size_t)nslots * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(d_sl, cp.slot_l.data(), (size_t)nslots * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(d_sd, cp.slot_dst.data(), (size_t)nslots * 4, hipMemcpyHostToDevice, s));
    for (size_t ph = 0, at = 0; ph < 3; at += items[ph++].size())  // the three arrays back to back
        if (!items[ph].empty()) SC_HIP(hipMemcpyAsync(b + o_items + at * sizeof(Item), items[ph].data(), items[ph].size() * sizeof(Item), hipMemcpyHostToDevice, s));
    st = sc_prep_queries(ix, q_dev, Q);
    if (st) return st;
    float *const qpad = ix->qpad.as<float>(), *const qnorm = ix->qnorm.as<float>();
    const void* const Xc8 = ix->sh_c8.arr[0].p;
    const float* const xcs = ix->sh_c8.arr[1].as<float>();
    const unsigned* const list_stats = ix->sh_c8.maxima;
    const int metric = (int)ix->metric;  // L2; IP (rows centred only); COSINE (the IP form on unit vectors) -- ivf_coarse.hip
    const int kmetric = metric == SC_METRIC_COSINE ? (int)SC_METRIC_IP : metric;  // what the streaming kernel computes
    sc_launch_ivf_pair_query(qpad, ld, ld8, qz->X, qz->ld, d_sq, d_sl, nslots, list_stats, b + o_qc, d_qs, d_qn, d_qb, d_qd, d_se, s, metric, qnorm, qz->xnorm);
    sc_launch_scan_batched_init(thr, tf, Qpad, best, cnt, ovf, Q, kpa, s);
    // phase A is dense: every row of its lists survives, at a known place of survA; the counts are known here
    SC_HIP(hipMemcpyAsync(cnt, cntA.data(), (size_t)Q * 4, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(cntA_d, cntA.data(), (size_t)Q * 4, hipMemcpyHostToDevice, s));
    const unsigned* xmax_bits = sc_ivfc_xmax_slot(ix);  // bits of max |x|^2: the rounding allowance of the exact scores
    hipEvent_t e0, e1;
    // 4. phase A: lower bounds of the nearest list(s) -> the kpa best re-scored exactly -> T = their k-th exact distance + allowance
    if (!items[0].empty()) {
        sc_launch_ivf_slot_thr(d_sq, d_qn, d_se, thr, nslots, d_st, d_stf, s);  // (+inf everywhere; the dense form tests nothing)
        sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
        sc_launch_ivf_coarse(Xc8, xcs, ld8, b + o_qc, b + o_items, (int)items[0].size(), d_stf, d_st, d_qn, d_qs, d_sq, d_qb, d_qd, survA, cnt, IVFC_CAP,
                             b + o_hits, hit_bytes, s, d_sd, kmetric);
        sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
    }
    sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
    sc_launch_scan_select(metric, survA, cnt, IVFC_CAP, best, qnorm, thr, tf, ovf, Q, kpa, s);  // (resets cnt: phase B counts from 0)
    sc_launch_scan_rerank_keys(metric, ix->X, ix->xnorm, ld, qpad, qnorm, best, nullptr, kpa, ix->perm, ekeysA, Q, s);
    sc_launch_ivf_bound(metric, ekeysA, kpa, k, qnorm, xmax_bits, ld, thr, Q, s);
    sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
    // 5. phase B: the other lists (and the rest of long phase-A lists) against T
    size_t b_first = items[0].size(), b_count = items[1].size() + items[2].size();
    // (two-level bounds) the 128 best lower bounds among phase B's survivors so far, re-scored: T = min(T, k-th of that sample + phase A's)
    auto tighten = [&]() -> sc_status {
        uint64_t *bestT = (uint64_t*)(b + o_bestT), *ekeysT = (uint64_t*)(b + o_ekT);
        unsigned* cntT = (unsigned*)(b + o_cntT);
        sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
        SC_HIP(hipMemcpyAsync(cntT, cnt, (size_t)Q * 4, hipMemcpyDeviceToDevice, s));  // (the selection resets the counts; the survivors stay where they are)
        SC_HIP(hipMemsetAsync(bestT, 0xFF, (size_t)Q * kpa * 8, s));
        sc_launch_scan_select(metric, survB, cnt, IVFC_CAPB, bestT, qnorm, (float*)(b + o_thrT), (float*)(b + o_tfT), ovf, Q, kpa, s);
        SC_HIP(hipMemcpyAsync(cnt, cntT, (size_t)Q * 4, hipMemcpyDeviceToDevice, s));
        sc_launch_scan_rerank_keys(metric, ix->X, ix->xnorm, ld, qpad, qnorm, bestT, nullptr, kpa, ix->perm, ekeysT, Q, s);
        sc_launch_ivf_bound(metric, ekeysA, kpa, k, qnorm, xmax_bits, ld, thr, Q, s, ekeysT, true);
        sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
        return SC_OK;
    };
    if (two_level) {  // the tails first: most neighbours live there, and what they yield tightens T for the other lists
        sc_launch_ivf_slot_thr(d_sq, d_qn, d_se, thr, nslots, d_st, d_stf, s);
        sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
        sc_launch_ivf_coarse(Xc8, xcs, ld8, b + o_qc, b + o_items + b_first * sizeof(Item), (int)items[1].size(), d_stf, d_st, d_qn, d_qs, d_sq, d_qb, d_qd, survB,
                             cnt, IVFC_CAPB, b + o_hits, hit_bytes, s, nullptr, kmetric);
        sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
        st = tighten();
        if (st) return st;
        b_first += items[1].size();
        b_count = items[2].size();
    }
    if (b_count > 0) {
        sc_launch_ivf_slot_thr(d_sq, d_qn, d_se, thr, nslots, d_st, d_stf, s);
        sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
        sc_launch_ivf_coarse(Xc8, xcs, ld8, b + o_qc, b + o_items + b_first * sizeof(Item), (int)b_count, d_stf, d_st, d_qn, d_qs, d_sq, d_qb, d_qd, survB, cnt,
                             IVFC_CAPB, b + o_hits, hit_bytes, s, nullptr, kmetric);
        sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
    }
    if (two_level && b_count > 0) {  // ... and once more over everything phase B kept: a query between two clusters finds its neighbours in the other lists
        st = tighten();
        if (st) return st;
    }
    // 6. refine: every row whose lower bound is within T, re-scored exactly; exact top-k
    sc_prof_begin(rt, SC_PROF_MERGE, &e0, &e1);
    sc_launch_ivf_candidates(metric, survA, cntA_d, best, kpa, survB, cnt, IVFC_CAP, thr, cand2, ncand, flags, Q, g_ivf_refine_cap < WCAP ? g_ivf_refine_cap : WCAP, s, IVFC_CAPB);
    sc_launch_scan_rerank_keys(metric, ix->X, ix->xnorm, ld, qpad, qnorm, cand2, ncand, WCAP, ix->perm, ekeys2, Q, s);
    sc_launch_ivf_refine_finalize(metric, ekeysA, kpa, ekeys2, ncand, flags, k, ix->row_base, out_dist, out_rows, Q, s);
    sc_prof_end(rt, SC_PROF_MERGE, e0, e1);
    SC_HIP(hipGetLastError());
    static const bool trace_c = getenv("SC_IVF_TRACE") != nullptr;  // tuning aid
    std::vector<int> hflags(Q);
    SC_HIP(hipMemcpyAsync(hflags.data(), flags, (size_t)Q * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    std::vector<int> redo;
    for (int i = 0; i < Q; ++i)
        if (hflags[i]) redo.push_back(i);
    const int R = (int)redo.size();
    ix->last_ivfc_uncertified = R;
    ix->last_uncertified = R;
    if (trace_c) {
        std::vector<int> hnc(Q);
        std::vector<unsigned> hcb(Q);
        std::vector<float> hthr(Q);
        SC_HIP(hipMemcpy(hnc.data(), ncand, (size_t)Q * 4, hipMemcpyDeviceToHost));
        SC_HIP(hipMemcpy(hcb.data(), cnt, (size_t)Q * 4, hipMemcpyDeviceToHost));
        SC_HIP(hipMemcpy(hthr.data(), thr, (size_t)Q * 4, hipMemcpyDeviceToHost));
        int novf = 0, ninf = 0, nc_max = 0, ja_max = 0;
        double nc_sum = 0, cb_sum = 0, ca_sum = 0, ja_sum = 0;
        for (int i = 0; i < Q; ++i) {
            novf += hcb[i] > (unsigned)IVFC_CAPB || cntA[(size_t)i] > (unsigned)IVFC_CAP;
            ninf += !(hthr[i] < 1e30f);
            nc_max = std::max(nc_max, hnc[i]);
            nc_sum += hnc[i];
            cb_sum += hcb[i];
            ca_sum += cntA[(size_t)i];
            ja_max = std::max(ja_max, cp.ja[(size_t)i]);
            ja_sum += cp.ja[(size_t)i];
        }
        fprintf(stderr, "[ivf coarse] Q %d: to the exact probe %d (survivor overflow %d, bound +inf %d); re-scored per query %d + avg %.1f max %d; phase A rows avg %.0f, "
                        "phase B survivors avg %.1f; phase A lists per query avg %.2f max %d; items %zu + %zu%s + %zu, slots %d; streamed %.1f GB int8\n",
                Q, R, novf, ninf, kpa, nc_sum / Q, nc_max, ca_sum / Q, cb_sum / Q, ja_sum / Q, ja_max, items[0].size(), items[1].size(), two_level ? " (own level)" : "",
                items[2].size(), nslots,
                (double)cp.streamed_rows * ld8 / 1e9);
    }
    if (ix->search_mode == 0 && Q >= 32 && R * 4 > Q) ix->ivfc_off = true;  // this index does not quantise well enough: later batches probe exactly
    ix->last_probed_lists = nprobe;
    ix->last_unique_rows = cp.unique_rows;
    ix->last_streamed_rows = cp.streamed_rows;
    ix->last_groups = (int)(nslots / 64);
    if (R > 0) {  // probed again exactly: the sub-batch gets its own staging (queries + results)
        sc_subbatch sb;
        st = sc_subbatch_stage(ix, ix->fb, q_dev, redo, k, &sb);
        if (st) return st;
        {
            sc_scoped_set<int> mode(ix->search_mode, 4);
            // list-major where it has a plan, per-query probing where not (nprobe * k beyond the gather merge; one query): the same
            // lists either way, so every query of the batch is answered under probe semantics (sc_ivf_coarse_applicable: one of them serves)
            if (sc_ivf_exact_probe_path(ld, R, k, nprobe, rt->cus) == 4) st = sc_ivf_search_listmajor_locked(ix, sb.q, R, k, nprobe, sb.d, sb.r);
            else st = sc_ivf_search_locked(ix, sb.q, R, k, nprobe, sb.d, sb.r);
        }
        if (st) return st;
        st = sc_subbatch_scatter(ix, sb, k, out_dist, out_rows);
        if (st) return st;
        ix->last_ivfc_uncertified = R;
        ix->last_uncertified = R;
    }
    ix->last_path = 5;
    return SC_OK;
}
