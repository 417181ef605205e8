// sc_ivf_diag.cpp -- sc_diag_ivf_plan: the host planners of IVF probing (sc_ivf_plan.cpp) on caller-given probe tables and list offsets,
// fed through sc_ivf_plan_params like the searches; no device is touched (tests/test_ivf_plan_host.py).
#include <string>
#include <vector>

#include "sc_diag_blob.h"
#include "sc_internal.h"
#include "sc_ivf_plan.h"

extern "C" sc_status sc_diag_ivf_exact_path(int32_t ld, int32_t R, int32_t k, int32_t nprobe, int32_t cus, int32_t* path) {
    if (!path || cus < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_ivf_exact_path: bad argument");
    *path = sc_ivf_exact_probe_path(ld, R, k, nprobe, cus);
    return SC_OK;
}

extern "C" sc_status sc_diag_ivf_plan(const char* path, const int64_t* probes, int32_t Q, int32_t nprobe, const int64_t* list_off, int32_t nlist, int32_t k,
                                      int32_t ld, int32_t cus, int32_t wide, void* out, int64_t cap_bytes, int64_t* need_bytes) {
    if (!path || !probes || !list_off || !need_bytes || Q < 1 || nprobe < 1 || nlist < 1 || cus < 1) return sc_fail(SC_ERR_INVALID, "sc_diag_ivf_plan: bad argument");
    for (int l = 0; l < nlist; ++l)
        if (list_off[l] < 0 || list_off[l + 1] < list_off[l]) return sc_fail(SC_ERR_INVALID, "sc_diag_ivf_plan: list_off must start at >= 0 and not decrease");
    const std::string which(path);
    IvfPlanParams pp;
    const bool lm_ok = sc_ivf_plan_params(ld, k, nprobe, cus, &pp);
    if (!wide) pp.wide_ok = false;
    DiagBlob bl;
    if (which == "listmajor") {
        if (!lm_ok) return sc_fail(SC_ERR_UNSUPPORTED, "sc_diag_ivf_plan: k=%d / ld=%d / nprobe=%d not supported by the list-major probe", k, ld, nprobe);
        IvfListMajorPlan lm;
        sc_ivf_plan_listmajor(probes, Q, nprobe, list_off, nlist, pp, &lm);
        static const char* const qmap_names[3] = {"qmap_w", "qmap_w2", "qmap"};
        static const char* const sr_names[3] = {"sr_w", "sr_w2", "sr"};
        static const char* const g_names[3] = {"Gw", "Gw2", "G"};
        bl.i32("src", lm.src);
        for (int c = 0; c < 3; ++c) {
            bl.i32(qmap_names[c], lm.cls[c].qmap);
            bl.i64(sr_names[c], lm.cls[c].sr);
            bl.num(g_names[c], lm.cls[c].groups);
        }
        bl.put("sb", 0, lm.sb.data(), lm.sb.size(), 4);
        bl.num("L", lm.L), bl.num("maxparts", lm.maxparts), bl.num("G_big", lm.G_big), bl.num("lists_w", lm.lists_w);
        bl.num("target", lm.target), bl.num("target_w", lm.target_w), bl.num("groups", lm.groups());
        bl.num("streamed_rows", lm.streamed_rows), bl.num("unique_rows", lm.unique_rows);
        bl.num("qt", pp.qt), bl.num("qt_res", pp.qt_res), bl.num("qstream", pp.qstream), bl.num("wide_ok", pp.wide_ok);
    } else if (which == "coarse") {
        IvfCoarsePlan cp;
        sc_ivf_plan_coarse(probes, Q, nprobe, list_off, nlist, pp, &cp);
        static const char* const item_names[3] = {"items_a", "items_tail", "items_b"};
        bl.put("ja", 0, cp.ja.data(), cp.ja.size(), 4);
        bl.put("cntA", 2, cp.cntA.data(), cp.cntA.size(), 4);
        bl.i32("slot_q", cp.slot_q), bl.i32("slot_l", cp.slot_l), bl.i32("slot_dst", cp.slot_dst);
        for (int ph = 0; ph < 3; ++ph) bl.put(item_names[ph], 3, cp.items[ph].data(), cp.items[ph].size(), sizeof(IvfCoarseItem));
        bl.num("two_level", cp.two_level), bl.num("groups", (int64_t)cp.slot_q.size() / 64);
        bl.num("streamed_rows", cp.streamed_rows), bl.num("unique_rows", cp.unique_rows), bl.num("KP", pp.KP);
    } else {
        return sc_fail(SC_ERR_INVALID, "sc_diag_ivf_plan: path must be \"listmajor\" or \"coarse\"");
    }
    bl.give(out, cap_bytes, need_bytes);
    return SC_OK;
}
