// scan_coarse64.hip -- the narrow streaming form of the coarse stage (scan_batched.h): batches of up to 64 queries over the int8
// shadow, and the list-major int8 coarse stage of IVF_FLAT, which runs through the same kernel (gfx950).
//
// Roofline: HBM (the int8 shadow streams once per batch).
#include <algorithm>

#include "scan_batched.h"

// ---- narrow streaming form for small batches (17 .. 64 queries, int8 shadow) -----------------------------------------------
// A 256 x 256 tile spends 6.1 us of MFMAs per 256 corpus rows whatever the batch holds; below ~100 queries the bound is not the
// matrix pipe but the memory system: the 7.7 GB int8 shadow streams in 1.2 ms.  This kernel is shaped for that: a persistent
// workgroup (8 waves) walks row tiles of 256 rows x 64 query slots and sees the corpus as ONE stream of stages (tile, K-tile) --
// 32 KiB of rows + 8 KiB of queries each -- through a three-deep LDS ring: two stages are always in flight, across tile
// boundaries too, so neither the first bytes of a tile nor the threshold epilogue interrupts the stream.  Wave w multiplies rows
// 32 w .. 32 w + 31 by all 64 slots (16 MFMAs per stage: the pipe idles, by design).  One barrier per stage.  Survivors (rare
// in the phases this kernel serves) are appended to a per-wave list in global memory -- no atomics, nothing to wait for -- and a
// small kernel scatters the lists into the per-query survivor lists afterwards.
// 10M x 768, 32 queries: 2.6 ms through the 256-query tiles -> see profiles/r3*_q_sweep.log.
#define C64_STAGE_A (256 * 128)
#define C64_STAGE_W (64 * 128)
#define C64_STAGE (C64_STAGE_A + C64_STAGE_W)
#define C64_RING (3 * C64_STAGE)
#define C64_LDS_BYTES (C64_RING + 3 * 1024 * 4 + 1024 * 4 + 3 * 512 * 4 + 4 * 64 * 4)
// GROUPED (IVF_FLAT coarse stage): work items and per-slot arrays instead of one row range and one query batch; GroupItem /
// GroupedArgs in scan_batched.h
// DENSE (GROUPED; phase A of the IVF coarse stage): the thresholds are still +inf, EVERY row of the list survives -- so a row's place in
// the query's survivor list is known in advance (its offset in the list + what the query's earlier lists hold) and the key goes
// straight there: no test, no hit list, no atomics (the hit lists + their scatter cost 1.3 ms of a config-5 batch, all of it phase A).
template <int METRIC, bool GROUPED = false, bool DENSE = false>
__global__ __launch_bounds__(512) void scan_coarse64s_kernel(CoarseArgs a, u32x4_t* __restrict__ hitlist, unsigned* __restrict__ hitcount, int hitcap, GroupedArgs ga) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ld8 = a.ld * 2;  // bytes per int8 row (a.ld counts 2-byte elements)
    const int nk = ld8 >> 7;   // stages per tile
    const int64_t ntiles = GROUPED ? (int64_t)ga.nitems : (a.row1 - a.row0 + 255) >> 8;
    const int64_t first = blockIdx.x;
    if (first >= ntiles) {
        if (tid < 8) hitcount[(size_t)blockIdx.x * 8 + tid] = 0;
        return;
    }
    const int64_t mine = (ntiles - first + gridDim.x - 1) / gridDim.x, S = mine * nk;
    // [3][xnorm 256 | xscale 256]: a tile's row side is requested two stages ahead, i.e. (one stage per tile, ld8 = 128) while the
    // epilogue of the tile two before it is still reading its copy -- three copies; the slot side (GROUPED) likewise
    // GROUPED: the row side is one 16-byte record per row ([3][256] f32x4 + 4 KiB that take the second copy waves 4-7 request so that
    // every wave issues the same number of pieces)
    float* rowlds = reinterpret_cast<float*>(smem + C64_RING);
    float* slotlds = rowlds + 3 * 1024 + 1024;  // GROUPED: [3][8][64]: tf | thr | qn | qs | query id | |q'| | |dq| | (unused)
    float* qlds = slotlds + 3 * 512;            // flat: thr_fast[64] | thr[64] | qnorm[64] | qscale[64]
    if (!GROUPED && tid < 64) {
        const bool real = tid < a.Q;
        qlds[tid] = real ? a.thr_fast[tid] : -__builtin_inff();
        qlds[64 + tid] = real ? a.thr[tid] : -__builtin_inff();
        qlds[128 + tid] = real ? a.qnorm[tid] : 1.0f;
        qlds[192 + tid] = a.qscale[tid];  // padded to Qpad
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // per-lane source offsets: a piece = 8 rows x 128 B; the 16-byte chunk of row r at position pos comes from chunk pos ^ ((r >> 1) & 7)
    uint32_t va[4], vw;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (4 * w + i) * 8 + (lane >> 3), c = (lane & 7) ^ ((r >> 1) & 7);
        va[i] = (uint32_t)(r * ld8 + c * 16);
    }
    {
        const int r = w * 8 + (lane >> 3), c = (lane & 7) ^ ((r >> 1) & 7);
        vw = (uint32_t)(r * ld8 + c * 16);
    }
    // row side: |x|^2 (waves 0-3) and the int8 row scale (waves 4-7), 64 rows per wave and tile; rows beyond the tile's end read as 0
    // (the descriptor ends there)
    const float* rowsrc = w < 4 ? a.xnorm : a.xscale;
    const uint32_t vrow = (uint32_t)(((w & 3) * 64 + lane) * 4);
    const float* slotsrc = nullptr;  // GROUPED: wave w requests slot array w % 5 of the item (256 B)
    if (GROUPED)
        slotsrc = w == 0 ? ga.slot_tf : w == 1 ? ga.slot_thr : w == 2 ? ga.slot_qn : w == 3 ? ga.slot_qs : w == 4 ? reinterpret_cast<const float*>(ga.slot_q)
                  : w == 5 ? ga.slot_qb : w == 6 ? ga.slot_qd : reinterpret_cast<const float*>(ga.slot_dst);

    int64_t t_i = first;  // issue side: tile and K-tile of the next stage to request
    int kt_i = 0, j_i = 0;
    int64_t m0_i = 0;
    int rows_i = 256, sb_i = 0;
    auto issue = [&](int slot) {
        char* dst = smem + slot * C64_STAGE;
        if (kt_i == 0) {
            if (GROUPED) {
                const GroupItem it = ga.items[t_i];
                m0_i = it.row0;
                rows_i = it.rows;
                sb_i = it.slot_base;
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(slotsrc + sb_i), 0, 256, 0x00020000);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_vptr)(reinterpret_cast<char*>(slotlds) + ((j_i % 3) * 512 + w * 64) * 4), 4, (uint32_t)(lane * 4), 0, 0, 0);
            } else {
                m0_i = a.row0 + (t_i << 8);
                const int64_t left = a.row1 - m0_i;
                rows_i = (int)(left >= 256 ? 256 : left > 0 ? left : 0);
            }
            if (GROUPED) {  // 64 row records of 16 B per wave (waves 4-7: the same rows again, into the spare 4 KiB)
                const __amdgpu_buffer_rsrc_t rrow = __builtin_amdgcn_make_buffer_rsrc((void*)(ga.xrow + m0_i), 0, rows_i * 16, 0x00020000);
                char* rdst = reinterpret_cast<char*>(rowlds) + (w < 4 ? (j_i % 3) * 4096 : 3 * 4096) + (w & 3) * 1024;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rrow, (lds_vptr)rdst, 16, (uint32_t)(((w & 3) * 64 + lane) * 16), 0, 0, 0);
            } else {
                const __amdgpu_buffer_rsrc_t rrow = __builtin_amdgcn_make_buffer_rsrc((void*)(rowsrc + m0_i), 0, rows_i * 4, 0x00020000);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rrow, (lds_vptr)(reinterpret_cast<char*>(rowlds) + ((j_i % 3) * 512 + (w >> 2) * 256 + (w & 3) * 64) * 4), 4, vrow, 0, 0, 0);
            }
        }
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const char*>(a.Xb) + m0_i * (int64_t)ld8), 0, -1, 0x00020000);
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const char*>(a.Qb) + (int64_t)sb_i * ld8), 0, -1, 0x00020000);
        const uint32_t so = (uint32_t)kt_i * 128u;
#pragma unroll
        for (int i = 0; i < 4; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_vptr)(dst + (4 * w + i) * 1024), 16, va[i], so, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, (lds_vptr)(dst + C64_STAGE_A + w * 1024), 16, vw, so, 0, 0);
        if (++kt_i == nk) {
            kt_i = 0;
            t_i += gridDim.x;
            ++j_i;
        }
    };
    issue(0);
    if (S > 1) issue(1);

    const int fr = lane & 15, fq = lane >> 4;
    const int sw = (fr >> 1) & 7;
    // fragment addresses inside a stage (k-step 0; k-step 1 = ^ 64): rows 32 w + 16 mi + fr of A, 16 ni + fr of W
    const uint32_t a_rd = (uint32_t)((32 * w + fr) * 128 + ((fq ^ sw) << 4));
    const uint32_t w_rd = (uint32_t)(C64_STAGE_A + fr * 128 + ((fq ^ sw) << 4));
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    u32x4_t* hlist = hitlist + ((size_t)blockIdx.x * 8 + w) * (size_t)hitcap;
    int hn = 0;
    int64_t t_c = first;
    int kt_c = 0, j_c = 0;
    constexpr int P0 = GROUPED ? 7 : 6;  // pieces of a stage that opens a tile: 5 + the row side (+ the slot side)
#pragma unroll 1
    for (int64_t s = 0; s < S; ++s) {
        // stage s has landed (this wave's pieces); the stage behind it may fly (5 pieces, P0 when it opens a tile)
        if (s + 1 >= S) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (kt_c + 1 == nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P0) : "memory");
        else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");  // ... and everyone's; every wave is done with stage s - 1, whose slot stage s + 2 takes
        if (s + 2 < S) issue((int)((s + 2) % 3));
        const char* st = smem + (int)(s % 3) * C64_STAGE;
        bf16x8 af[2][2], wf[4][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) af[mi][ks] = *reinterpret_cast<const bf16x8*>(st + ((a_rd ^ (uint32_t)(ks << 6)) + mi * 2048));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) wf[ni][ks] = *reinterpret_cast<const bf16x8*>(st + ((w_rd ^ (uint32_t)(ks << 6)) + ni * 2048));
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) acc[ni][mi] = pp_mma<true>(wf[ni][ks], af[mi][ks], acc[ni][mi]);
        if (kt_c + 1 < nk) {
            ++kt_c;
            continue;
        }
        // ---- the tile is complete: thresholds (the tests of coarse256_epilogue), survivors appended to this wave's list
        int64_t m0;
        int rows_c;
        if (GROUPED) {
            const GroupItem it = ga.items[t_c];
            m0 = it.row0;
            rows_c = it.rows;
        } else {
            m0 = a.row0 + (t_c << 8);
            const int64_t left = a.row1 - m0;
            rows_c = (int)(left >= 256 ? 256 : left);
        }
        const float* rs = rowlds + (j_c % 3) * (GROUPED ? 1024 : 512);
        const float* sl = GROUPED ? slotlds + (j_c % 3) * 512 : qlds;  // tf | thr | qn | qs (| query id | |q'| | |dq|)
        f32x4 tf[4], sq[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            tf[ni] = *reinterpret_cast<const f32x4*>(sl + ni * 16 + 4 * fq);
            sq[ni] = *reinterpret_cast<const f32x4*>(sl + 192 + ni * 16 + 4 * fq);
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const int rl = 32 * w + 16 * mi + fr;
            const int64_t row = m0 + rl;
            const bool rowok = rl < rows_c;
            float xn, sx, ea = 0.f, ec = 0.f;  // GROUPED: ea = 2 |dx_r|, ec = 2 (|x'_r| + |dx_r|)
            if (GROUPED) {
                const f32x4 rec = *reinterpret_cast<const f32x4*>(rs + 4 * rl);
                xn = rec[0]; sx = rec[1]; ea = rec[2]; ec = rec[3];
            } else {
                xn = rs[rl];
                sx = rs[256 + rl];
            }
            const float xs = (METRIC == SC_METRIC_COSINE) ? sc_inv_norm(xn) : 0.f;
            const float ar = (METRIC == SC_METRIC_L2) ? -2.0f * sx : (METRIC == SC_METRIC_COSINE) ? -sx * xs : -sx;
            if (GROUPED && DENSE) {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int ql = 16 * ni + 4 * fq + r;
                        const int qid = __float_as_int(sl[256 + ql]);
                        if (rowok && qid >= 0) {
                            const float dotv = (float)__float_as_int(acc[ni][mi][r]) * (sx * sq[ni][r]);
                            float sc;  // L2: lower bound of the distance; IP: upper bound of the inner product (slot constant = -(<c, q> + allowance))
                            if (METRIC == SC_METRIC_L2) sc = fmaf(-ec, sl[384 + ql], fmaf(-ea, sl[320 + ql], sc_score<METRIC>(dotv, xn, sl[128 + ql])));
                            else sc = fmaf(ec, sl[384 + ql], fmaf(ea, sl[320 + ql], dotv - sl[128 + ql]));
                            const uint32_t pos = (uint32_t)row + (uint32_t)__float_as_int(sl[448 + ql]);
                            if (pos < (uint32_t)a.cap) a.surv[(size_t)qid * a.cap + pos] = sc_make_key<METRIC>(sc, (uint32_t)row);
                        }
                    }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
                continue;
            }
            // (the row factor as a real register pair: -s_r taken straight from the odd half of the row record came out of hipcc as
            // v_pk_mul_f32 ... op_sel:[1,0], the encoding tests/test_isa.py keeps out of every kernel)
            f32x2 ar2 = {ar, ar};
            asm volatile("" : "+v"(ar2));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                f32x4 t;
                bool g = false;
                const f32x2 av01 = f32x2{(float)__float_as_int(acc[ni][mi][0]), (float)__float_as_int(acc[ni][mi][1])} * ar2;
                const f32x2 av23 = f32x2{(float)__float_as_int(acc[ni][mi][2]), (float)__float_as_int(acc[ni][mi][3])} * ar2;
                const f32x4 av4 = {av01[0], av01[1], av23[0], av23[1]};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float av = av4[r];
                    t[r] = (METRIC == SC_METRIC_L2) ? fmaf(av, sq[ni][r], xn) : av * sq[ni][r];
                    g |= t[r] <= tf[ni][r];
                }
                if (!__any(g && rowok)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    bool h = false;
                    uint64_t key = 0;
                    const int ql = 16 * ni + 4 * fq + r;
                    if (rowok && t[r] <= tf[ni][r]) {
                        const float dotv = (float)__float_as_int(acc[ni][mi][r]) * (sx * sq[ni][r]);
                        float sc = sc_score<METRIC>(dotv, xn, sl[128 + ql]);
                        if (GROUPED) {  // the row's own error bound: a lower bound of the exact distance (L2) / an upper bound of the inner product (IP)
                            if (METRIC == SC_METRIC_L2) sc = fmaf(-ec, sl[384 + ql], fmaf(-ea, sl[320 + ql], sc));
                            else sc = fmaf(ec, sl[384 + ql], fmaf(ea, sl[320 + ql], dotv - sl[128 + ql]));
                        }
                        const float v = (METRIC == SC_METRIC_L2) ? sc : -sc;
                        if (v <= sl[64 + ql]) {  // -inf for padded slots
                            h = true;
                            key = sc_make_key<METRIC>(sc, (uint32_t)row);
                        }
                    }
                    const uint64_t m = __ballot(h);
                    if (m) {
                        const int off = hn + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        if (h) {
                            const uint32_t qid = GROUPED ? (uint32_t)__float_as_int(sl[256 + ql]) : (uint32_t)ql;
                            if (off < hitcap) {
                                hlist[off] = u32x4_t{(uint32_t)key, (uint32_t)(key >> 32), qid, 0u};
                            } else {  // list full: allocate the slot here
                                const unsigned pos = atomicAdd(a.count + qid, 1u);
                                if (pos < (unsigned)a.cap) a.surv[(size_t)qid * a.cap + pos] = key;
                            }
                        }
                        hn += (int)__popcll(m);
                    }
                }
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        hn = __builtin_amdgcn_readfirstlane(hn);
        kt_c = 0;
        t_c += gridDim.x;
        ++j_c;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) hitcount[(size_t)blockIdx.x * 8 + w] = (unsigned)(hn < hitcap ? hn : hitcap);
}

// the per-wave hit lists of scan_coarse64s_kernel -> the per-query survivor lists (one wave per list)
__global__ __launch_bounds__(64) void scan_hits_scatter_kernel(const u32x4_t* __restrict__ hitlist, const unsigned* __restrict__ hitcount, int hitcap,
                                                               unsigned* __restrict__ count, uint64_t* __restrict__ surv, int cap) {
    const unsigned n = hitcount[blockIdx.x];
    const u32x4_t* l = hitlist + (size_t)blockIdx.x * (size_t)hitcap;
    for (unsigned i = threadIdx.x; i < n; i += 64) {
        const u32x4_t e = l[i];
        const unsigned pos = atomicAdd(count + e[2], 1u);
        if (pos < (unsigned)cap) surv[(size_t)e[2] * cap + pos] = ((uint64_t)e[1] << 32) | e[0];
    }
}

template <int METRIC>
static void launch_coarse64s(const CoarseArgs& a, hipStream_t s, void* hit_scratch, size_t hit_bytes) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse64s_kernel<METRIC, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C64_LDS_BYTES); });
    const int64_t ntiles = (a.row1 - a.row0 + 255) >> 8;
    const int cus = sc_device_cus(), forced = sc_scan_coarse_workgroups();
    const int wgs = (int)std::min<int64_t>(ntiles, forced > 0 ? forced : cus);
    const size_t lists = (size_t)wgs * 8, off = (lists * 4 + 255) & ~(size_t)255;
    unsigned* hitcount = (unsigned*)hit_scratch;
    u32x4_t* hitlist = (u32x4_t*)((char*)hit_scratch + off);
    const int hitcap = (int)std::min<size_t>((hit_bytes - off) / (lists * 16), (size_t)1 << 20);
    hipLaunchKernelGGL((scan_coarse64s_kernel<METRIC, false>), dim3((unsigned)wgs), dim3(512), C64_LDS_BYTES, s, a, hitlist, hitcount, hitcap, GroupedArgs{});
    hipLaunchKernelGGL(scan_hits_scatter_kernel, dim3((unsigned)lists), dim3(64), 0, s, (const u32x4_t*)hitlist, (const unsigned*)hitcount, hitcap, a.count, a.surv, a.cap);
}
void sc_launch_coarse64s(int metric, const CoarseArgs& a, hipStream_t s, void* hit_scratch, size_t hit_bytes) {
    sc_dispatch_metric(metric, [&](auto m) { launch_coarse64s<m.value>(a, s, hit_scratch, hit_bytes); });
}
template <int METRIC>
static void launch_ivf_coarse_m(const CoarseArgs& a, const GroupedArgs& ga, int wgs, u32x4_t* hitlist, unsigned* hitcount, int hitcap, size_t lists, bool dense,
                                unsigned* count, uint64_t* surv, int cap, hipStream_t s) {
    static ScDeviceOnce once;
    sc_device_once(once, [&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse64s_kernel<METRIC, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C64_LDS_BYTES);
        hipFuncSetAttribute(reinterpret_cast<const void*>(scan_coarse64s_kernel<METRIC, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C64_LDS_BYTES);
    });
    if (dense) {  // keys go straight to their places
        hipLaunchKernelGGL((scan_coarse64s_kernel<METRIC, true, true>), dim3((unsigned)wgs), dim3(512), C64_LDS_BYTES, s, a, hitlist, hitcount, hitcap, ga);
        return;
    }
    hipLaunchKernelGGL((scan_coarse64s_kernel<METRIC, true>), dim3((unsigned)wgs), dim3(512), C64_LDS_BYTES, s, a, hitlist, hitcount, hitcap, ga);
    hipLaunchKernelGGL(scan_hits_scatter_kernel, dim3((unsigned)lists), dim3(64), 0, s, (const u32x4_t*)hitlist, (const unsigned*)hitcount, hitcap, count, surv, cap);
}
// IVF_FLAT coarse stage (L2 / IP): `nitems` work items {row0, rows, slot_base} over the centred int8 shadow Xc8 / per-pair queries Qc8; per-slot
// thresholds etc.; hits go to the survivor lists of the slots' queries.  hit_scratch as for the flat form.
void sc_launch_ivf_coarse(const void* Xc8, const float* xrow, int ld8, const void* Qc8, const void* items, int nitems, const float* slot_tf,
                          const float* slot_thr, const float* slot_qn, const float* slot_qs, const int32_t* slot_q, const float* slot_qb, const float* slot_qd,
                          uint64_t* surv, unsigned* count, int cap, void* hit_scratch, size_t hit_bytes, hipStream_t s, const int32_t* slot_dst, int metric) {
    if (nitems <= 0) return;
    CoarseArgs a;
    a.Xb = (const bf16_t*)Xc8; a.xnorm = nullptr; a.xscale = nullptr; a.row0 = 0; a.row1 = 0; a.ld = ld8 / 2; a.Qb = (const bf16_t*)Qc8; a.qnorm = nullptr; a.Q = 0; a.qtiles = 1;
    a.thr = nullptr; a.thr_fast = nullptr; a.surv = surv; a.count = count; a.cap = cap; a.ntiles = nitems; a.qscale = nullptr; a.trace = nullptr;
    GroupedArgs ga;
    ga.items = (const GroupItem*)items; ga.nitems = nitems; ga.slot_tf = slot_tf; ga.slot_thr = slot_thr; ga.slot_qn = slot_qn; ga.slot_qs = slot_qs; ga.slot_q = slot_q; ga.slot_qb = slot_qb; ga.slot_qd = slot_qd; ga.xrow = (const f32x4*)xrow;
    ga.slot_dst = slot_dst ? slot_dst : slot_q;  // (wave 7 requests it either way)
    const int cus = sc_device_cus(), forced = sc_scan_coarse_workgroups();
    const int wgs = std::min(nitems, forced > 0 ? forced : cus);
    const size_t lists = (size_t)wgs * 8, off = (lists * 4 + 255) & ~(size_t)255;
    unsigned* hitcount = (unsigned*)hit_scratch;
    u32x4_t* hitlist = (u32x4_t*)((char*)hit_scratch + off);
    const int hitcap = (int)std::min<size_t>((hit_bytes - off) / (lists * 16), (size_t)1 << 20);
    // (two metrics, not sc_dispatch_metric's three: the caller scores COSINE lists as IP, and the grouped kernel is not built for it)
    if (metric == SC_METRIC_L2) launch_ivf_coarse_m<SC_METRIC_L2>(a, ga, wgs, hitlist, hitcount, hitcap, lists, slot_dst != nullptr, count, surv, cap, s);
    else launch_ivf_coarse_m<SC_METRIC_IP>(a, ga, wgs, hitlist, hitcount, hitcap, lists, slot_dst != nullptr, count, surv, cap, s);
}
bool sc_scan_coarse64_supported(int Q, int ld8, size_t hit_bytes) { return Q >= 1 && Q <= 64 && ld8 >= 128 && (ld8 % 128) == 0 && hit_bytes >= (size_t)2048 * (4 + 64 * 16) + 256; }
