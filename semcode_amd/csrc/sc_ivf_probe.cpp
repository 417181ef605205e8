// sc_ivf_probe.cpp -- the exact IVF probes: per query (one scan over the nprobe lists of every query) and list-major (every probed
// list streamed once per group of queries that want it).  Each search is the sequence probe -> plan -> grow scratch -> upload ->
// launch -> stats -> trace; the list-major plan itself is host arithmetic in sc_ivf_plan.cpp.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

#include "sc_internal.h"
#include "sc_ivf_plan.h"

bool sc_ivf_applicable(const sc_index* ix, int Q, int nprobe) {
    if (ix->kind != SC_INDEX_IVF_FLAT || !ix->trained || !ix->quant) return false;
    if (nprobe < 1 || nprobe > 512 || ix->search_mode == 1 || ix->search_mode == 2 || ix->search_mode == 4 || ix->search_mode == 5) return false;
    if (nprobe >= ix->nlist_trained) return false;  // probing every list = the exhaustive scan
    if (ix->search_mode == 3) return true;
    // one pass per query over nprobe/nlist of the corpus vs one exhaustive pass per 16 queries (or the
    // batched path): probe only while it reads less than a single full pass
    return (int64_t)Q * nprobe < (int64_t)ix->nlist_trained;
}

sc_status sc_ivf_probe_quantizer_locked(sc_index* ix, const float* q_dev, int Q, int nprobe, size_t extra_bytes, sc_ivf_probes* out,
                                        std::vector<int64_t>* host) {
    sc_index* qz = ix->quant;
    hipStream_t s = ix->rt->stream;
    const size_t npairs = (size_t)Q * nprobe;
    sc_carver carve;
    const size_t o_pd = carve(npairs * 4), o_pr = carve(npairs * 8), o_extra = carve(extra_bytes);
    sc_status st = sc_grow(ix, ix->ivf_scratch, carve.off);
    if (st) return st;
    char* b = ix->ivf_scratch.as<char>();
    *out = {(float*)(b + o_pd), (int64_t*)(b + o_pr), b + o_extra};
    {
        std::lock_guard<std::mutex> gq(qz->mu);
        sc_scoped_set<sc_metric> metric(qz->metric, ix->metric);
        st = sc_search_flat_locked(qz, q_dev, Q, nprobe, out->dist, out->lists);
        if (st) return st;
    }
    if (host) {
        host->resize(npairs);
        SC_HIP(hipMemcpyAsync(host->data(), out->lists, npairs * 8, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
    }
    return SC_OK;
}

sc_status sc_ivf_search_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist, int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    ScanPlan plan;
    if (!sc_scan_exact_plan(ix->ld, Q, k, rt->cus, &plan, 1, nprobe))
        return sc_fail(SC_ERR_UNSUPPORTED, "ivf search: k=%d / dim=%d / nprobe=%d not supported", k, ix->dim, nprobe);
    // scratch: probe results + plan tables
    const size_t sb_bytes = sc_align256((size_t)Q * (nprobe + 1) * 4);
    sc_ivf_probes pr;
    sc_status st = sc_ivf_probe_quantizer_locked(ix, q_dev, Q, nprobe, sb_bytes + (size_t)Q * nprobe * 16, &pr);
    if (st) return st;
    int* sb = (int*)pr.extra;
    int64_t* sr = (int64_t*)(pr.extra + sb_bytes);
    sc_launch_ivf_plan(pr.lists, Q, nprobe, ix->list_off, ix->nlist_trained, sb, sr, s);
    st = sc_prep_queries(ix, q_dev, Q);
    if (st) return st;
    st = sc_grow(ix, ix->partial, std::max<size_t>(plan.partial_bytes, 16));
    if (st) return st;
    uint64_t* partial = ix->partial.as<uint64_t>();
    hipEvent_t e0, e1;
    sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
    sc_launch_scan_exact((int)ix->metric, ix->X, ix->xnorm, ix->n, ix->ld, ix->qpad.as<float>(), ix->qnorm.as<float>(), Q, k, plan, partial, ix->perm, sb, sr, nprobe, s);
    sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
    sc_launch_topk_merge((int)ix->metric, partial, plan.groups, plan.lists, plan.qt, Q, k, ix->row_base, out_dist, out_rows, s);
    SC_HIP(hipGetLastError());
    ix->last_path = 3;
    ix->last_probed_lists = nprobe;
    return SC_OK;
}

// ---- list-major probing for query batches ------------------------------------------------------------------------
// Per-query probing streams nprobe lists once PER QUERY; with Q * nprobe >= nlist probes every list is wanted by several
// queries, so the batch is turned round: the (query, list) pairs are bucketed by list, every list is streamed once per
// group of up to qt queries that probe it (scan_exact_kernel, one row range per group, the group's queries gathered
// through qmap), and a query's top-k is merged from the nprobe (group, slot) lists it took part in.  Same lists, same exact
// f32 scores and tie rule as per-query probing, so the results are identical to it.
//
// The planners' parameters.  Wide groups (scan_listgemm_kernel) need the 16-query narrow scan next to them; SC_IVF_WIDE=0 switches
// the class off (A/B, tests of the narrow classes).  With the streamed-query scan (long rows, qt = 16) a group of few queries is
// still better off on the resident variant, which streams ~30 % faster: qt_res is the most that fit resident.  Both variables are
// read on every call: the tests flip them inside one process.
bool sc_ivf_plan_params(int ld, int k, int nprobe, int cus, IvfPlanParams* pp, ScanPlan* plan_out, ScanPlan* plan_res_out) {
    pp->k = k;
    pp->cus = cus;
    pp->KP = sc_batched_kprime8();
    pp->merge_ok = sc_topk_gather_merge_supported;
    ScanPlan plan;
    if (!sc_scan_exact_plan(ld, 16, k, cus, &plan, 0, 1) || !sc_topk_gather_merge_supported(nprobe, k)) return false;
    pp->qt = plan.qt;
    pp->qstream = plan.qstream != 0;
    pp->wide_cap = pp->wide_ok = sc_scan_listgemm_supported(ld, k) && plan.qt == 16;
    if (const char* e = getenv("SC_IVF_WIDE"))
        if (e[0] == '0') pp->wide_ok = false;
    ScanPlan plan_res = plan;
    if (plan.qstream && !sc_scan_exact_plan(ld, 16, k, cus, &plan_res, 16, 1)) plan_res = plan;
    pp->qt_res = plan_res.qstream ? plan.qt : std::min(plan.qt, plan_res.qt);
    if (const char* e = getenv("SC_SCAN_QSTREAM"))
        if (plan.qstream && e[0] != '0') pp->qt_res = 0;  // forced: every group on the streamed variant (tests, A/B)
    if (plan_out) *plan_out = plan;
    if (plan_res_out) *plan_res_out = plan_res;
    return true;
}

int sc_ivf_exact_probe_path(int ld, int R, int k, int nprobe, int cus) {
    if (R < 1 || nprobe < 1 || nprobe > 512) return 0;
    IvfPlanParams pp;
    if (R >= 2 && sc_ivf_plan_params(ld, k, nprobe, cus, &pp)) return 4;
    ScanPlan plan;
    return sc_scan_exact_plan(ld, R, k, cus, &plan, 1, nprobe) ? 3 : 0;  // (as sc_ivf_search_locked plans it)
}

bool sc_ivf_listmajor_applicable(const sc_index* ix, int Q, int k, int nprobe, bool flat_is_batched) {
    if (ix->kind != SC_INDEX_IVF_FLAT || !ix->trained || !ix->quant || Q < 2) return false;
    if (nprobe < 1 || nprobe > 512 || nprobe >= ix->nlist_trained || (ix->search_mode >= 1 && ix->search_mode <= 3)) return false;
    IvfPlanParams pp;
    if (!sc_ivf_plan_params(ix->ld, k, nprobe, ix->rt->cus, &pp)) return false;
    if (ix->search_mode == 4 || ix->search_mode == 5) return true;  // (5: the coarse stage was asked for and could not run)
    // auto: probe while that is estimated to be cheaper than the exhaustive paths (which return exact results)
    return sc_ivf_listmajor_cheaper(ix->list_off_h.data(), ix->nlist_trained, ix->n, ix->ld, Q, nprobe, pp.qt, pp.wide_cap, flat_is_batched, ix->uncert_frac);
}

sc_status sc_ivf_search_listmajor_locked(sc_index* ix, const float* q_dev, int32_t Q, int32_t k, int32_t nprobe, float* out_dist,
                                         int64_t* out_rows) {
    sc_runtime* rt = ix->rt;
    hipStream_t s = rt->stream;
    IvfPlanParams pp;
    ScanPlan plan, plan_res;
    if (!sc_ivf_plan_params(ix->ld, k, nprobe, rt->cus, &pp, &plan, &plan_res))
        return sc_fail(SC_ERR_UNSUPPORTED, "ivf list-major search: k=%d / dim=%d / nprobe=%d not supported", k, ix->dim, nprobe);
    const int qt = pp.qt;
    static const bool trace = getenv("SC_IVF_TRACE") != nullptr;  // tuning aid: host-side phase times on stderr
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    // 1. coarse probe under the index metric -> host
    sc_ivf_probes pr;
    std::vector<int64_t> probes;
    sc_status st = sc_ivf_probe_quantizer_locked(ix, q_dev, Q, nprobe, 0, &pr, &probes);
    if (st) return st;
    const double t_probe = since();
    // 2. plan (lives until the stream synchronisation below: its vectors are the sources of the uploads)
    IvfListMajorPlan lm;
    sc_ivf_plan_listmajor(probes.data(), Q, nprobe, ix->list_off_h.data(), ix->nlist_trained, pp, &lm);
    const double t_plan = since();
    // 3. plan tables -> device (they replace the probe results in the scratch buffer), queries padded + normed
    sc_carver carve;
    const size_t o_src = carve(lm.src.size() * 4), o_sb = carve(lm.sb.size() * 4 + 16);
    size_t o_qmap[3], o_sr[3];
    for (int c = 0; c < 3; ++c) o_qmap[c] = carve(lm.cls[c].qmap.size() * 4 + 16), o_sr[c] = carve(lm.cls[c].sr.size() * 8 + 16);
    st = sc_grow(ix, ix->ivf_scratch, carve.off);
    if (st) return st;
    char* b = ix->ivf_scratch.as<char>();
    SC_HIP(hipMemcpyAsync(b + o_src, lm.src.data(), lm.src.size() * 4, hipMemcpyHostToDevice, s));
    if (!lm.sb.empty()) SC_HIP(hipMemcpyAsync(b + o_sb, lm.sb.data(), lm.sb.size() * 4, hipMemcpyHostToDevice, s));
    for (int c = 0; c < 3; ++c) {
        const IvfGroupClass& gc = lm.cls[c];
        if (gc.groups == 0) continue;
        SC_HIP(hipMemcpyAsync(b + o_qmap[c], gc.qmap.data(), gc.qmap.size() * 4, hipMemcpyHostToDevice, s));
        SC_HIP(hipMemcpyAsync(b + o_sr[c], gc.sr.data(), gc.sr.size() * 8, hipMemcpyHostToDevice, s));
    }
    st = sc_prep_queries(ix, q_dev, Q);
    if (st) return st;
    const int G = lm.cls[2].groups;
    st = sc_grow(ix, ix->partial, std::max<size_t>(((size_t)lm.lists_w + (size_t)G * qt) * k * 8, 16));
    if (st) return st;
    float *const qpad = ix->qpad.as<float>(), *const qnorm = ix->qnorm.as<float>();
    uint64_t* const partial = ix->partial.as<uint64_t>();
    // 4. one workgroup per group (grid.y is limited to 65535 groups per launch); the wide classes go first: their workgroups are
    // the long ones
    hipEvent_t e0, e1;
    sc_prof_begin(rt, SC_PROF_SCAN, &e0, &e1);
    size_t lists_before = 0;  // k-lists of the classes before this one in `partial`
    for (int c = 0; c < 2; ++c) {
        const IvfGroupClass& gc = lm.cls[c];
        sc_launch_scan_listgemm((int)ix->metric, gc.width, ix->X, ix->xnorm, ix->ld, qpad, qnorm, k, gc.groups, partial + lists_before * k, ix->perm,
                                (const int64_t*)(b + o_sr[c]), (const int32_t*)(b + o_qmap[c]), s);
        lists_before += (size_t)gc.groups * gc.width;
    }
    for (int res = 0; res < 2; ++res)  // the narrow class: streamed queries, then resident ones
      for (int g0 = res ? lm.G_big : 0, hi = res ? G : lm.G_big; g0 < hi; g0 += 65535) {
        const int gn = std::min(65535, hi - g0);
        ScanPlan p = res ? plan_res : plan;
        p.groups = gn;
        p.nwg = 1;
        p.lists = 1;
        p.gstride = qt;
        sc_launch_scan_exact((int)ix->metric, ix->X, ix->xnorm, ix->n, ix->ld, qpad, qnorm, gn * qt, k, p,
                             partial + ((size_t)lm.lists_w + (size_t)g0 * qt) * k, ix->perm, (const int*)(b + o_sb) + (size_t)g0 * 2,
                             (const int64_t*)(b + o_sr[2]) + (size_t)g0 * 2, 1, s, (const int32_t*)(b + o_qmap[2]) + (size_t)g0 * qt);
    }
    sc_prof_end(rt, SC_PROF_SCAN, e0, e1);
    // 5. a query's result = merge of the nprobe (group, slot) lists it took part in
    sc_launch_topk_gather_merge((int)ix->metric, partial, (const int32_t*)(b + o_src), lm.L, Q, k, ix->row_base, out_dist, out_rows, s);
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(s));  // the host plan vectors go out of scope
    if (trace) {
        const double row_gb = (double)ix->ld * 4.0 / 1e9;
        double streamed_big = 0.0;
        for (int g = 0; g < lm.G_big; ++g) streamed_big += (double)(lm.cls[2].sr[(size_t)g * 2 + 1] - lm.cls[2].sr[(size_t)g * 2]);
        fprintf(stderr, "[ivf list-major] wide groups: %d of <= 64 queries = %.1f GB, %d of <= 32 = %.1f GB\n", lm.cls[0].groups, (double)lm.cls[0].streamed_rows() * row_gb,
                lm.cls[1].groups, (double)lm.cls[1].streamed_rows() * row_gb);
        const double t_scan = since() - t_plan, streamed_gb = (double)lm.streamed_rows * row_gb;
        fprintf(stderr, "[ivf list-major] Q=%d nprobe=%d qt=%d groups=%d (%d = %.1f GB on streamed queries) parts<=%d target=%lld / %lld rows | probe + D2H %.3f ms, host plan %.3f ms, H2D + scan + merge %.3f ms = %.1f GB at %.2f TB/s\n",
                Q, nprobe, qt, G, plan.qstream ? lm.G_big : 0, plan.qstream ? streamed_big * row_gb : 0.0, lm.maxparts, (long long)lm.target, (long long)lm.target_w, t_probe, t_plan - t_probe, t_scan, streamed_gb, streamed_gb / t_scan);
    }
    ix->last_path = 4;
    ix->last_probed_lists = nprobe;
    ix->last_groups = lm.groups();
    ix->last_streamed_rows += lm.streamed_rows;  // (accumulated: sums over the chunks of a batch, and on top of a coarse stage that re-probes here)
    ix->last_unique_rows += lm.unique_rows;
    return SC_OK;
}
