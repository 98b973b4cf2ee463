// The offline analyses' host code: PR / RR evaluation (one estimate, many, by class), the overlap report, the frame check, the scans'
// labels, the clustering, the k nearest neighbours and density filters, the normals, the point-to-plane refinement, the see-through check, the carving of free space, the ground, label_map and static_complement, the bird's-eye renderer, their test hooks and the parameter sweep.  Included by erasor_hip.hip
// at its end -- one translation unit, like the kernel headers -- so it sees the handle, ensure / LAUNCH / HIPC, scan_u32, radix_sort,
// map_to_device and voxelize_device from there; nothing of the step path depends on this file.  Kernels: evaluate.hip.h, nearest.hip.h,
// align.hip.h, label_scans.hip.h, cluster.hip.h, knn.hip.h, normals.hip.h, refine_plane.hip.h, visibility.hip.h, carve.hip.h, ground.hip.h, render.hip.h,
// and objects.hip.h (the decision per object), which this file includes itself.
#pragma once

#include "objects.hip.h"

extern "C" {

// ---- what the offline analyses share: the checks of their arguments, the caller's clouds and the handle's map on the device ----

// The analyses run on the main stream (every launch names h->stream), behind whatever a collected step launched ahead there, in the
// evaluator's scratch (h->ev).  Where one sorts (a tree's Morton keys, the instances' records) its radix sort runs in histogram bank 2, so
// that the query chains of nodes announced ahead (bank 0) keep theirs.

static int invalid(erasor_hip_handle *h, const std::string &who, const std::string &why) {
    h->err = who + ": " + why;
    return ERASOR_E_INVALID;
}

// a caller cloud has at most 2^30 points (two clouds together index in 31 bits) and a pointer when it has any: refused before anything is read
static constexpr size_t MAX_POINTS = 0x3FFFFFFFull;
static const char *const BAD_CLOUD = "NULL cloud or more than 2^30 points";
static int check_cloud(erasor_hip_handle *h, const std::string &who, const char *what, const void *xyzi, size_t n) {
    return ((!xyzi && n) || n > MAX_POINTS) ? invalid(h, who, what) : ERASOR_OK;
}

// res, voxelsize and voxel_leaf of the calls that take them; per_point: the call has a per-point output, which voxel_leaf > 0 rules out
static int check_voxel_args(erasor_hip_handle *h, const char *prefix, double voxel_leaf, double voxelsize, bool per_point, const char *per_point_msg,
                            const void *res) {
    if (!res) return invalid(h, prefix, "res is NULL");
    if (!(voxelsize > 0) || !std::isfinite(voxelsize)) return invalid(h, prefix, "voxelsize must be a finite number > 0");
    if (!(voxel_leaf >= 0) || !std::isfinite(voxel_leaf)) return invalid(h, prefix, "voxel_leaf must be 0 or a finite number > 0");
    if (per_point && voxel_leaf > 0) return invalid(h, prefix, per_point_msg);
    return ERASOR_OK;
}

// the frames of one scans array (align_frames, the sweep): offsets[0 .. n] from 0, never decreasing, up to the scans' point count
static int check_scan_offsets(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n) {
    if (n_scan_points > MAX_POINTS) return invalid(h, who, "more than 2^30 scan points");
    if (!scans_xyzi && n_scan_points) return invalid(h, who, "NULL scans");
    if (offsets[0] != 0) return invalid(h, who, "offsets[0] must be 0");
    for (size_t f = 0; f < n; ++f)
        if (offsets[f + 1] < offsets[f]) return invalid(h, who, "offsets decrease");
    if (offsets[n] != n_scan_points) return invalid(h, who, "the last offset is not the scans' point count");
    return ERASOR_OK;
}
static bool all_finite(const float *v, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// the handle's map as one dense device array in buf (the evaluator's h->ev.map, the renderer's h->ev.rd_map)
static int map_on_device(erasor_hip_handle *h, const char *who, DBuf<float4> &buf, const float4 **pts, uint32_t *n) {
    if (!h->have_map) {
        h->err = std::string(who) + ": the handle has no map (erasor_hip_set_map first)";
        return ERASOR_E_STATE;
    }
    size_t n_map = 0;
    const int rc = map_to_device(h, buf, &n_map);
    if (rc) return rc;
    if (n_map > MAX_POINTS) return invalid(h, who, "map larger than 2^30 points");
    *pts = buf.p;
    *n = (uint32_t)n_map;
    return ERASOR_OK;
}

// ---- PR / RR of a cleaned map against a labelled ground-truth map (scripts/analysis_runner.py:74-105; kernels: evaluate.hip.h) ----
// Everything runs on the main stream, behind whatever a collected step launched ahead there, in the handle's own scratch (h->ev).
// n_rec (the breakdown by class): the kernels also fill the per-key table E.bc_tab and the dynamic points' records; *n_rec = their count.
static void ev_fill(const unsigned long long c[EV_NCTR], erasor_eval_result *res);
static int ev_run(erasor_hip_handle *h, const float4 *gt, uint32_t n_gt, const float4 *est, uint32_t n_est, double voxelsize, uint8_t *per_gt,
                  erasor_eval_result *res, uint32_t *n_rec = nullptr, bool codes_on_device = false) {
    auto &E = h->ev;
    const bool want_codes = per_gt || codes_on_device;  // (codes_on_device: E.code keeps them for the renderer, no host copy)
    uint32_t nb = 1024;  // buckets: a power of two >= the estimate's size (<= 1 point per bucket on average)
    while (nb < n_est) nb <<= 1;
#ifdef ERASOR_HIP_TEST_HOOKS
    E.dbg_nb = nb;
#endif
    if (ensure(h, E.ctr, EV_NCTR) || ensure(h, E.cnt, (size_t)nb + 1) || ensure(h, E.pl, (size_t)nb + 1) || ensure(h, E.tops, nb / 1024 + 4) ||
        ensure(h, E.bkt, (size_t)n_est + 1) || ensure(h, E.pts, (size_t)n_est + 1) || ensure(h, E.idx, (size_t)n_est + 1) ||
        (want_codes && ensure(h, E.code, (size_t)n_gt + 1)))
        return ERASOR_E_NO_DEVICE;
    const size_t n_all = (size_t)n_gt + n_est;  // (< 2^31: each cloud has at most 2^30 points)
    if (n_rec && (ensure(h, E.bc_tab, (size_t)EV_NKEYS * EV_KC) || ensure(h, E.bc_cur, 4) || ensure(h, E.bc_ikey, n_all + 1) ||
                  ensure(h, E.bc_ival, n_all + 1)))
        return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemsetAsync(E.ctr.p, 0, EV_NCTR * sizeof(unsigned long long), h->stream));
    if (n_rec) {
        HIPC(h, hipMemsetAsync(E.bc_tab.p, 0, (size_t)EV_NKEYS * EV_KC * sizeof(uint32_t), h->stream));
        HIPC(h, hipMemsetAsync(E.bc_cur.p, 0, sizeof(uint32_t), h->stream));
    }
    const double thr = (voxelsize * sqrt(3.0)) / 2.0;  // evalmap / analysis_runner.py: voxelsize * np.sqrt(3) / 2
    if (n_est) {
        HIPC(h, hipMemsetAsync(E.cnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), h->stream));
        if (n_rec)
            LAUNCH(h, h->stream, "ev_index", k_ev_hist_keys, cdiv(n_est, 256), 256, est, n_est, voxelsize, nb - 1, E.bkt.p, E.cnt.p, E.ctr.p, E.bc_tab.p, E.bc_cur.p,
                   E.bc_ikey.p, E.bc_ival.p);
        else
            LAUNCH(h, h->stream, "ev_index", k_ev_hist, cdiv(n_est, 256), 256, est, n_est, voxelsize, nb - 1, E.bkt.p, E.cnt.p, E.ctr.p);
        scan_u32(h, h->stream, E.cnt.p, E.pl.p, E.tops.p, nb + 1, nb + 1, nullptr, nullptr, "ev_index");
        LAUNCH(h, h->stream, "ev_index", k_ev_offsets, cdiv(nb + 1, 256), 256, (const uint32_t *)E.pl.p, (const uint32_t *)E.tops.p, nb + 1, E.cnt.p, E.pl.p);
        LAUNCH(h, h->stream, "ev_index", k_ev_scatter, cdiv(n_est, 256), 256, est, n_est, (const uint32_t *)E.bkt.p, E.pl.p, E.pts.p, E.idx.p);
    }
    if (n_gt && n_rec)
        LAUNCH(h, h->stream, "ev_query", k_ev_query_keys, cdiv(n_gt, 256), 256, gt, n_gt, (const float4 *)E.pts.p, (const uint32_t *)E.idx.p,
               (const uint32_t *)E.cnt.p, nb - 1, n_est, voxelsize, thr, E.ctr.p, E.bc_tab.p, E.bc_cur.p, E.bc_ikey.p, E.bc_ival.p);
    else if (n_gt)
        LAUNCH(h, h->stream, "ev_query", k_ev_query, cdiv(n_gt, 256), 256, gt, n_gt, (const float4 *)E.pts.p, (const uint32_t *)E.idx.p, (const uint32_t *)E.cnt.p,
               nb - 1, n_est, voxelsize, thr, want_codes ? E.code.p : (uint8_t *)nullptr, E.ctr.p);
    unsigned long long c[EV_NCTR];
    HIPC(h, hipMemcpyAsync(c, E.ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    if (n_rec) HIPC(h, hipMemcpyAsync(n_rec, E.bc_cur.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (c[EV_NON_FINITE]) {
        h->err = "erasor_hip_evaluate: non-finite coordinate (NaN / Inf) in " + std::to_string(c[EV_NON_FINITE]) + " point(s)";
        return ERASOR_E_INVALID;
    }
    if (per_gt && n_gt) HIPC(h, hipMemcpy(per_gt, E.code.p, n_gt, hipMemcpyDeviceToHost));
    ev_fill(c, res);
    return ERASOR_OK;
}

// erasor_eval_result from one evaluation's counters
static void ev_fill(const unsigned long long c[EV_NCTR], erasor_eval_result *res) {
    erasor_eval_result r;
    memset(&r, 0, sizeof(r));
    r.gt_static = c[EV_GT_STATIC];
    r.gt_dynamic = c[EV_GT_DYNAMIC];
    r.est_static = c[EV_EST_STATIC];
    r.est_dynamic = c[EV_EST_DYNAMIC];
    r.preserved_static = c[EV_KEPT_STATIC];
    r.preserved_dynamic = c[EV_KEPT_DYNAMIC];
    r.n_tied = c[EV_TIED];
    r.n_label_out_of_range = c[EV_LABEL_OOR];
    // evalmap.evaluate's formulas, operation by operation (Python int / int is the correctly rounded quotient: the same as in double here)
    const double ns = (double)r.gt_static, nd = (double)r.gt_dynamic;
    r.PR = r.gt_static ? (double)r.preserved_static / ns * 100.0 : 0.0;
    r.RR = r.gt_dynamic ? (double)(r.gt_dynamic - r.preserved_dynamic) / nd * 100.0 : 0.0;
    r.F1 = (r.PR + r.RR) > 0 ? 2 * (r.PR / 100) * (r.RR / 100) / ((r.PR / 100) + (r.RR / 100)) : 0.0;
    *res = r;
}

// voxelize_preserving_labels of a device cloud at `leaf` (the save_static_map protocol, OMU.cpp:174-196) into dst[off ..) (borrows a query
// side).  passthrough (optional): set when VoxelGrid's indices overflowed and the cloud came back unchanged.
static int ev_voxelize(erasor_hip_handle *h, const float4 *src, uint32_t n, double leaf, DBuf<float4> &dst, uint32_t *n_out,
                       bool *passthrough = nullptr, size_t off = 0) {
    *n_out = 0;
    if (passthrough) *passthrough = false;
    if (!n) return ERASOR_OK;
    uint32_t nq = 0;
    const int rc = voxelize_device(h, src, n, leaf, &nq, passthrough);
    if (rc) return rc;
    if (ensure(h, dst, off + nq + 1)) return ERASOR_E_NO_DEVICE;  // (nq <= n: no reallocation when src is dst itself)
    if (nq) HIPC(h, hipMemcpyAsync(dst.p + off, h->q[h->qi].query.p, (size_t)nq * sizeof(float4), hipMemcpyDeviceToDevice, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    *n_out = nq;
    return ERASOR_OK;
}

static int ev_check_args(erasor_hip_handle *h, double voxel_leaf, double voxelsize, bool per_gt, const void *res) {
    return check_voxel_args(h, "erasor_hip_evaluate", voxel_leaf, voxelsize, per_gt,
                            "per_gt needs voxel_leaf == 0 (the codes would describe the voxelised ground truth)", res);
}

// a caller cloud on the device: its own pointer, or a copy of the host cloud in `buf`
static int ev_input(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, DBuf<float4> &buf, const float4 **out) {
    *out = nullptr;
    if (!n) return ERASOR_OK;
    if (is_device) {
        *out = (const float4 *)xyzi;
        return ERASOR_OK;
    }
    if (ensure(h, buf, n + 1)) return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemcpyAsync(buf.p, xyzi, n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    *out = buf.p;
    return ERASOR_OK;
}

// The ground truth and the estimate of one call on the device, as the *_run functions take them: the caller's clouds checked and brought
// in through h->ev.gt / h->ev.est (ev_pair_clouds), or the handle's map in h->ev.map as the estimate (ev_pair_map); voxel_leaf > 0: both
// voxelised at that leaf, into h->ev.gt / h->ev.est.
struct EvPair {
    const float4 *g = nullptr, *e = nullptr;
    uint32_t ng = 0, ne = 0;
};
static int ev_pair_voxelize(erasor_hip_handle *h, double voxel_leaf, EvPair *p) {
    if (!(voxel_leaf > 0)) return ERASOR_OK;
    int rc;
    if ((rc = ev_voxelize(h, p->g, p->ng, voxel_leaf, h->ev.gt, &p->ng)) || (rc = ev_voxelize(h, p->e, p->ne, voxel_leaf, h->ev.est, &p->ne))) return rc;
    p->g = h->ev.gt.p;
    p->e = h->ev.est.p;
    return ERASOR_OK;
}
static int ev_pair_clouds(erasor_hip_handle *h, const char *who, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *est_xyzi, size_t n_est,
                          int est_is_device, double voxel_leaf, EvPair *p) {
    int rc;
    if ((rc = check_cloud(h, who, BAD_CLOUD, gt_xyzi, n_gt)) || (rc = check_cloud(h, who, BAD_CLOUD, est_xyzi, n_est))) return rc;
    HIPC(h, hipSetDevice(h->device));
    if ((rc = ev_input(h, gt_xyzi, n_gt, gt_is_device, h->ev.gt, &p->g)) || (rc = ev_input(h, est_xyzi, n_est, est_is_device, h->ev.est, &p->e))) return rc;
    p->ng = (uint32_t)n_gt;
    p->ne = (uint32_t)n_est;
    return ev_pair_voxelize(h, voxel_leaf, p);
}
static int ev_pair_map(erasor_hip_handle *h, const char *who, const void *gt_xyzi, size_t n_gt, int gt_is_device, double voxel_leaf, EvPair *p) {
    int rc = check_cloud(h, who, BAD_CLOUD, gt_xyzi, n_gt);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    if ((rc = map_on_device(h, who, h->ev.map, &p->e, &p->ne)) || (rc = ev_input(h, gt_xyzi, n_gt, gt_is_device, h->ev.gt, &p->g))) return rc;
    p->ng = (uint32_t)n_gt;
    return ev_pair_voxelize(h, voxel_leaf, p);
}

int erasor_hip_evaluate_clouds(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *est_xyzi, size_t n_est,
                               int est_is_device, double voxel_leaf, double voxelsize, uint8_t *per_gt, erasor_eval_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    EvPair p;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, per_gt != nullptr, res);
    if (rc || (rc = ev_pair_clouds(h, "erasor_hip_evaluate_clouds", gt_xyzi, n_gt, gt_is_device, est_xyzi, n_est, est_is_device, voxel_leaf, &p))) return rc;
    return ev_run(h, p.g, p.ng, p.e, p.ne, voxelsize, per_gt, res);
}

int erasor_hip_evaluate_map(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, double voxel_leaf, double voxelsize,
                            erasor_eval_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    EvPair p;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, false, res);
    if (rc || (rc = ev_pair_map(h, "erasor_hip_evaluate_map", gt_xyzi, n_gt, gt_is_device, voxel_leaf, &p))) return rc;
    return ev_run(h, p.g, p.ng, p.e, p.ne, voxelsize, nullptr, res);
}

// ---- K estimates against one ground truth (erasor_hip_evaluate_many; kernels: k_evm_* in evaluate.hip.h) ----
// The callers copy the estimates back to back into E.em_cat.  Estimate j gets ev_run's bucket count for its size (a power of two >= n_j,
// at least 1024) as its own range of one combined table: one histogram launch, one scan, one offsets launch, one scatter, one query.
// Device memory, besides a host GT's copy (16 B a point): per estimated point the combined copy, its bucketed copy, its bucket and its
// index (40 B); per bucket the counts and their scan (8 B, fewer than 2 buckets a point + 1024 per estimate): below 56 B per estimated
// point + 8 KiB per estimate.  Like ev_run: the main stream, the evaluator's scratch.
static int evm_run(erasor_hip_handle *h, const char *who, const float4 *gt, uint32_t n_gt, const uint32_t *n_est, size_t k, double voxelsize,
                   erasor_eval_result *rows) {
    auto &E = h->ev;
    std::vector<EvmEst> tab(k + 1);
    memset(tab.data(), 0, tab.size() * sizeof(EvmEst));
    uint64_t n_all = 0, nb_all = 0, blk = 0;
    for (size_t j = 0; j <= k; ++j) {
        tab[j].off = (uint32_t)n_all;
        tab[j].base = (uint32_t)nb_all;
        tab[j].blk0 = (uint32_t)blk;
        if (j == k) break;
        uint32_t nb = 1024;
        while (nb < n_est[j]) nb <<= 1;
        tab[j].n = n_est[j];
        tab[j].mask = nb - 1;
        n_all += n_est[j];
        nb_all += nb;
        blk += cdiv(n_est[j], 256);
    }
    if (n_all > 0x7FFFFFFFull || nb_all > 0x7FFFFFFFull) {
        h->err = std::string(who) + ": more than 2^31 estimated points or buckets in all";
        return ERASOR_E_INVALID;
    }
    const uint32_t nb = (uint32_t)nb_all, n = (uint32_t)n_all;
#ifdef ERASOR_HIP_TEST_HOOKS
    E.dbg_nb = nb;
    E.dbg_tab = tab;
#endif
    if (ensure(h, E.em_tab, k + 1) || ensure(h, E.em_ctr, (k + 1) * EV_NCTR) || ensure(h, E.cnt, (size_t)nb + 1) || ensure(h, E.pl, (size_t)nb + 1) ||
        ensure(h, E.tops, nb / 1024 + 4) || ensure(h, E.bkt, (size_t)n + 1) || ensure(h, E.pts, (size_t)n + 1) || ensure(h, E.idx, (size_t)n + 1))
        return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemcpyAsync(E.em_tab.p, tab.data(), (k + 1) * sizeof(EvmEst), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.em_ctr.p, 0, (k + 1) * EV_NCTR * sizeof(unsigned long long), h->stream));
    const double thr = (voxelsize * sqrt(3.0)) / 2.0;  // (ev_run's)
    if (n) {
        HIPC(h, hipMemsetAsync(E.cnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), h->stream));
        LAUNCH(h, h->stream, "evm_index", k_evm_hist, (uint32_t)blk, 256, (const float4 *)E.em_cat.p, (const EvmEst *)E.em_tab.p, (uint32_t)k, voxelsize, E.bkt.p,
               E.cnt.p, E.em_ctr.p);
        scan_u32(h, h->stream, E.cnt.p, E.pl.p, E.tops.p, nb + 1, nb + 1, nullptr, nullptr, "evm_index");
        LAUNCH(h, h->stream, "evm_index", k_ev_offsets, cdiv(nb + 1, 256), 256, (const uint32_t *)E.pl.p, (const uint32_t *)E.tops.p, nb + 1, E.cnt.p, E.pl.p);
        LAUNCH(h, h->stream, "evm_index", k_ev_scatter, cdiv(n, 256), 256, (const float4 *)E.em_cat.p, n, (const uint32_t *)E.bkt.p, E.pl.p, E.pts.p, E.idx.p);
    }
    if (n_gt) {
        // one estimate per blockIdx.y: workgroups are dispatched x fastest, so the estimates are searched one after the other, each
        // against its own bucket table while that is cache-resident.  (All K in one lane's loop reads the GT once but walks K tables at
        // a time: for 8 estimates of 9.8 M points against a 9.8 M-point GT that took 147 ms against 137 ms for 8 evaluate_clouds calls.)
        const uint32_t gx = cdiv(n_gt, 256), per_y = 1, gy = (uint32_t)std::max<size_t>(k, 1);
        LAUNCH(h, h->stream, "evm_query", k_evm_query, dim3(gx, gy), 256, gt, n_gt, (const float4 *)E.pts.p, (const uint32_t *)E.idx.p, (const uint32_t *)E.cnt.p,
               (const EvmEst *)E.em_tab.p, (uint32_t)k, per_y, voxelsize, thr, E.em_ctr.p);
    }
    std::vector<unsigned long long> c((k + 1) * EV_NCTR);
    HIPC(h, hipMemcpyAsync(c.data(), E.em_ctr.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    const unsigned long long *cg = &c[k * EV_NCTR];
    if (cg[EV_NON_FINITE]) {
        h->err = std::string(who) + ": non-finite coordinate (NaN / Inf) in " + std::to_string(cg[EV_NON_FINITE]) + " point(s) of the ground truth";
        return ERASOR_E_INVALID;
    }
    for (size_t j = 0; j < k; ++j)
        if (c[j * EV_NCTR + EV_NON_FINITE]) {
            h->err = std::string(who) + ": non-finite coordinate (NaN / Inf) in " + std::to_string(c[j * EV_NCTR + EV_NON_FINITE]) +
                     " point(s) of estimate " + std::to_string(j);
            return ERASOR_E_INVALID;
        }
    for (size_t j = 0; j < k; ++j) {
        unsigned long long *cj = &c[j * EV_NCTR];
        cj[EV_GT_STATIC] = cg[EV_GT_STATIC];
        cj[EV_GT_DYNAMIC] = cg[EV_GT_DYNAMIC];
        cj[EV_LABEL_OOR] += cg[EV_LABEL_OOR];
        ev_fill(cj, &rows[j]);
    }
    return ERASOR_OK;
}

int erasor_hip_evaluate_many(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *const *est_xyzi, const size_t *n_est,
                             const int *est_is_device, size_t k, double voxel_leaf, double voxelsize, erasor_eval_result *rows) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const std::string who = "erasor_hip_evaluate_many";
    erasor_eval_result unused;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, false, k ? rows : &unused);
    if (rc) return rc;
    if (k && (!est_xyzi || !n_est)) return invalid(h, who, "est_xyzi or n_est is NULL");
    if ((rc = check_cloud(h, who, "NULL ground truth or more than 2^30 points", gt_xyzi, n_gt))) return rc;
    uint64_t total = 0;
    for (size_t j = 0; j < k; ++j) {
        if ((rc = check_cloud(h, who + ": estimate " + std::to_string(j), BAD_CLOUD, est_xyzi[j], n_est[j]))) return rc;
        total += n_est[j];
    }
    if (total > 0x7FFFFFFFull) return invalid(h, who, "more than 2^31 estimated points in all");
    if (!k) return ERASOR_OK;
    HIPC(h, hipSetDevice(h->device));
    auto &E = h->ev;
    const float4 *g = nullptr;
    if ((rc = ev_input(h, gt_xyzi, n_gt, gt_is_device, E.gt, &g))) return rc;
    uint32_t ng = (uint32_t)n_gt;
    if (voxel_leaf > 0) {
        if ((rc = ev_voxelize(h, g, ng, voxel_leaf, E.gt, &ng))) return rc;
        g = E.gt.p;
    }
    // every estimate into the combined array (voxelised first with voxel_leaf > 0: never more points than given)
    if (ensure(h, E.em_cat, total + 1)) return ERASOR_E_NO_DEVICE;
    std::vector<uint32_t> ne(k, 0);
    uint64_t off = 0;
    for (size_t j = 0; j < k; ++j) {
        const uint32_t n = (uint32_t)n_est[j];
        const bool dev = est_is_device && est_is_device[j];
        if (!n) continue;
        if (voxel_leaf > 0) {
            const float4 *e = nullptr;
            if ((rc = ev_input(h, est_xyzi[j], n, dev, E.est, &e)) || (rc = ev_voxelize(h, e, n, voxel_leaf, E.em_cat, &ne[j], nullptr, off))) {
                h->err = who + ": estimate " + std::to_string(j) + ": " + h->err;
                return rc;
            }
        } else {
            HIPC(h, hipMemcpyAsync(E.em_cat.p + off, est_xyzi[j], (size_t)n * sizeof(float4), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                   h->stream));
            ne[j] = n;
        }
        off += ne[j];
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    return evm_run(h, who.c_str(), g, ng, ne.data(), k, voxelsize, rows);
}

// ---- the estimate-to-GT overlap report (scripts/analysis_runner.py:53-71, overlap_report; kernels: nearest.hip.h) ----
// Like ev_run: the main stream, the evaluator's scratch (h->ev), and the tree's radix sort in a histogram bank of its own (bank 2), so
// that the query chains of nodes announced ahead (bank 0) keep theirs.

// np.percentile(d, p) (method "linear") from the sorted values v(rank), operation by operation: q = p / 100, virtual index (n-1)*q,
// previous / next index (both n-1 at or above it), gamma = index - previous, and _lerp with its t >= 0.5 branch
static void ov_percentile_ranks(uint64_t n, double p, uint64_t *prev, uint64_t *next, double *gamma) {
    const double q = p / 100.0;
    const double vi = (double)(n - 1) * q;
    double pi = floor(vi);
    *prev = (uint64_t)pi;
    *next = (uint64_t)pi + 1;
    if (vi >= (double)(n - 1)) {
        pi = -1.0;  // (numpy indexes with -1: the last value)
        *prev = *next = n - 1;
    }
    *gamma = vi - pi;
}
static double ov_lerp(double a, double b, double t) {
    const double diff = b - a;
    double r = a + diff * t;
    if (t >= 0.5) r = b - diff * (1 - t);
    return r;
}

// The bounding-volume tree over pts[0 .. n) (nearest.hip.h) in E.nn_pts / nn_idx / nn_lo / nn_hi, and *T its view for the query kernels.
// The leaf count is padded to a power of two (T->n_pad); a cloud whose tree would not fit the traversal stack is refused ("<who>: <cloud>
// too large ..."), before anything else is done.  E.nn_ctr (OV_NCTR entries) is zeroed here; a non-finite point refuses the call
// ("<who>: ... in <k> <noun>").  n == 0: T->n = 0, T->n_pad = 1, nothing is built and no search may start.
static int nn_build(erasor_hip_handle *h, const float4 *pts, uint32_t n, const char *who, const char *cloud, const char *noun, NnTree *T) {
    auto &E = h->ev;
    const uint32_t n_leaves = std::max(1u, cdiv(n, NN_LEAF));
    uint32_t P = 1, levels = 0;  // leaves padded to a power of two, levels below the root
    while (P < n_leaves) {
        P <<= 1;
        ++levels;
    }
    if (levels >= NN_STACK) {
        h->err = std::string(who) + ": " + cloud + " too large for the traversal stack";
        return ERASOR_E_INVALID;
    }
    const size_t n1 = (size_t)n + 1;
    if (ensure(h, E.nn_ctr, OV_NCTR) ||
        (n && (ensure(h, E.nn_bb, 8) || ensure(h, E.nn_key, n1) || ensure(h, E.nn_ka, n1) || ensure(h, E.nn_kb, n1) || ensure(h, E.nn_va, n1) ||
               ensure(h, E.nn_vb, n1) || ensure(h, E.nn_idx, n1) || ensure(h, E.nn_pts, n1) || ensure(h, E.nn_lo, 2 * (size_t)P) ||
               ensure(h, E.nn_hi, 2 * (size_t)P))))
        return ERASOR_E_NO_DEVICE;
    *T = NnTree{E.nn_pts.p, E.nn_idx.p, E.nn_lo.p, E.nn_hi.p, n, P};
    HIPC(h, hipMemsetAsync(E.nn_ctr.p, 0, OV_NCTR * sizeof(unsigned long long), h->stream));
    if (!n) return ERASOR_OK;
    // the box: k_bbox's fkey_ord min (3 x ~0u) / max (3 x 0)
    HIPC(h, hipMemsetAsync(E.nn_bb.p, 0xFF, 3 * sizeof(uint32_t), h->stream));
    HIPC(h, hipMemsetAsync(E.nn_bb.p + 3, 0, 3 * sizeof(uint32_t), h->stream));
    LAUNCH(h, h->stream, "ov_tree", k_bbox, bbox_grid(n), 256, pts, n, E.nn_bb.p);
    LAUNCH(h, h->stream, "ov_tree", k_nn_keys, cdiv(n, 256), 256, pts, n, (const uint32_t *)E.nn_bb.p, E.nn_key.p, E.nn_ctr.p);
    const uint32_t *skeys = nullptr, *sperm = nullptr;
    if (radix_sort(h, h->stream, 2, E.nn_key.p, n, nullptr, 30, E.nn_ka.p, E.nn_kb.p, E.nn_va.p, E.nn_vb.p, &skeys, &sperm, "ov_tree"))
        return ERASOR_E_NO_DEVICE;
#ifdef ERASOR_HIP_TEST_HOOKS
    E.dbg_skeys = skeys;
#endif
    LAUNCH(h, h->stream, "ov_tree", k_nn_gather, cdiv(n, 256), 256, pts, n, sperm, E.nn_pts.p, E.nn_idx.p);
    LAUNCH(h, h->stream, "ov_tree", k_nn_leaves, cdiv(P * NN_LEAF, 256), 256, (const float4 *)E.nn_pts.p, n, P, E.nn_lo.p, E.nn_hi.p);
    for (uint32_t first = P / 2; first >= 1; first /= 2) LAUNCH(h, h->stream, "ov_tree", k_nn_level, cdiv(first, 256), 256, E.nn_lo.p, E.nn_hi.p, first);
    unsigned long long c[OV_NCTR];
    HIPC(h, hipMemcpyAsync(c, E.nn_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (c[OV_NON_FINITE]) {
        h->err = std::string(who) + ": non-finite coordinate (NaN / Inf) in " + std::to_string(c[OV_NON_FINITE]) + " " + noun;
        return ERASOR_E_INVALID;
    }
    return ERASOR_OK;
}

// the target ranks of n > 0 sorted distances: the median's one or two, the two of each percentile (and the percentiles' gammas)
static void ov_ranks(uint64_t n, uint64_t rk[OV_SEL_MAX], double *g90, double *g99) {
    rk[0] = (n - 1) / 2;
    rk[1] = n / 2;
    ov_percentile_ranks(n, 90, &rk[2], &rk[3], g90);
    ov_percentile_ranks(n, 99, &rk[4], &rk[5], g99);
}

// the exact radix select over the bit patterns v[0 .. count), driven from the host (k_ov_select_hist): the values at the ranks rk, from the
// top digit down; every target keeps its prefix and its rank inside that prefix.  Values above every rank (align's sentinel) never matter.
static int ov_select(erasor_hip_handle *h, const unsigned long long *v, uint32_t count, const uint64_t rk[OV_SEL_MAX], double out[OV_SEL_MAX],
                     int top_shift = 56) {  // (top_shift: the highest digit that can differ -- 24 for values below 2^32)
    auto &E = h->ev;
    unsigned long long pref[OV_SEL_MAX] = {};
    uint64_t left[OV_SEL_MAX];
    for (uint32_t t = 0; t < OV_SEL_MAX; ++t) left[t] = rk[t];
    std::vector<uint32_t> hist(OV_SEL_MAX * 256);
    const uint32_t grid = std::min(cdiv(count, 256 * 8), 1024u);
    for (int shift = top_shift; shift >= 0; shift -= 8) {
        OvSelect s;
        memset(&s, 0, sizeof(s));
        s.shift = shift;
        uint32_t slot[OV_SEL_MAX];
        for (uint32_t t = 0; t < OV_SEL_MAX; ++t) {
            uint32_t k = 0;
            while (k < s.n && s.pref[k] != pref[t]) ++k;
            if (k == s.n) s.pref[s.n++] = pref[t];
            slot[t] = k;
        }
        HIPC(h, hipMemsetAsync(E.nn_hist.p, 0, (size_t)s.n * 256 * sizeof(uint32_t), h->stream));
        LAUNCH(h, h->stream, "ov_select", k_ov_select_hist, grid, 256, v, count, s, E.nn_hist.p);
        HIPC(h, hipMemcpyAsync(hist.data(), E.nn_hist.p, (size_t)s.n * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        for (uint32_t t = 0; t < OV_SEL_MAX; ++t) {
            const uint32_t *hh = hist.data() + (size_t)slot[t] * 256;
            uint64_t cum = 0;
            uint32_t d = 0;
            while (d < 255 && left[t] >= cum + hh[d]) cum += hh[d++];
            left[t] -= cum;
            pref[t] = (pref[t] << 8) | d;
        }
    }
    memcpy(out, pref, sizeof(pref));
    return ERASOR_OK;
}

// one report from n distances: the counts below the thresholds, the largest distance's bits, and (n > 0) the values at ov_ranks' ranks
static void ov_fill(uint64_t n, uint64_t below_half, uint64_t below_one, uint64_t below_two, unsigned long long max_bits, const double v[OV_SEL_MAX],
                    double g90, double g99, erasor_overlap_result *res) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    erasor_overlap_result r;
    memset(&r, 0, sizeof(r));
    r.n_est = n;
    r.n_below_half = below_half;
    r.n_below_one = below_one;
    r.n_below_two = below_two;
    r.median = r.p90 = r.p99 = r.max = r.frac_half = r.frac_one = r.frac_two = nan;
    if (n) {
        // np.median: the middle value, or the mean of the two middle ones, (a + b) / 2
        r.median = (n % 2) ? v[0] : (v[0] + v[1]) / 2.0;
        r.p90 = ov_lerp(v[2], v[3], g90);
        r.p99 = ov_lerp(v[4], v[5], g99);
        double mx;
        memcpy(&mx, &max_bits, sizeof(mx));
        r.max = mx;
        // np.mean(d < x) * 100
        r.frac_half = (double)r.n_below_half / (double)n * 100.0;
        r.frac_one = (double)r.n_below_one / (double)n * 100.0;
        r.frac_two = (double)r.n_below_two / (double)n * 100.0;
    }
    *res = r;
}

static int ov_run(erasor_hip_handle *h, const float4 *gt, uint32_t n_gt, const float4 *est, uint32_t n_est, double voxelsize, double *per_dist,
                  uint32_t *per_nearest, erasor_overlap_result *res) {
    auto &E = h->ev;
    if (ensure(h, E.nn_hist, OV_SEL_MAX * 256) ||
        (n_est && (ensure(h, E.nn_dbits, (size_t)n_est + 1) || (per_nearest && ensure(h, E.nn_near, (size_t)n_est + 1)))))
        return ERASOR_E_NO_DEVICE;
    unsigned long long c[OV_NCTR];
    NnTree T;
    int rc = nn_build(h, gt, n_gt, "erasor_hip_overlap", "ground truth", "ground-truth point(s)", &T);
    if (rc) return rc;
    // the thresholds as overlap_report forms them: half = 0.5 * voxelsize, one = voxelsize, 2 * one
    const double half = 0.5 * voxelsize, one = voxelsize, two = 2 * one;
    if (n_est)
        LAUNCH(h, h->stream, "ov_query", k_nn_query, cdiv(n_est, NN_QBLOCK), NN_QBLOCK, est, n_est, T, half, one, two, E.nn_dbits.p,
               per_nearest ? E.nn_near.p : (uint32_t *)nullptr, E.nn_ctr.p);
    HIPC(h, hipMemcpyAsync(c, E.nn_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (c[OV_NON_FINITE]) {
        h->err = "erasor_hip_overlap: non-finite coordinate (NaN / Inf) in " + std::to_string(c[OV_NON_FINITE]) + " estimated point(s)";
        return ERASOR_E_INVALID;
    }
    erasor_overlap_result r;
    const uint64_t n = n_est;
    double v[OV_SEL_MAX] = {}, g90 = 0, g99 = 0;
    if (n_est) {
        uint64_t rk[OV_SEL_MAX];
        ov_ranks(n, rk, &g90, &g99);
        if ((rc = ov_select(h, E.nn_dbits.p, n_est, rk, v))) return rc;
    }
    ov_fill(n, c[OV_BELOW_HALF], c[OV_BELOW_ONE], c[OV_BELOW_TWO], c[OV_MAX_BITS], v, g90, g99, &r);
    if (n_est) {
        if (per_dist) HIPC(h, hipMemcpy(per_dist, E.nn_dbits.p, (size_t)n_est * sizeof(double), hipMemcpyDeviceToHost));
        if (per_nearest) HIPC(h, hipMemcpy(per_nearest, E.nn_near.p, (size_t)n_est * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    *res = r;
    return ERASOR_OK;
}

static int ov_check_args(erasor_hip_handle *h, double voxel_leaf, double voxelsize, bool per_point, const void *res) {
    return check_voxel_args(h, "erasor_hip_overlap", voxel_leaf, voxelsize, per_point,
                            "per-point outputs need voxel_leaf == 0 (they would describe the voxelised estimate)", res);
}
static int ov_check_gt(erasor_hip_handle *h, const char *who, const EvPair &p) {
    return (!p.ng && p.ne) ? invalid(h, who, "empty ground truth (no nearest point to measure against)") : ERASOR_OK;
}

int erasor_hip_overlap_clouds(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *est_xyzi, size_t n_est,
                              int est_is_device, double voxel_leaf, double voxelsize, double *per_est_dist, uint32_t *per_est_nearest,
                              erasor_overlap_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_overlap_clouds";
    EvPair p;
    int rc = ov_check_args(h, voxel_leaf, voxelsize, per_est_dist || per_est_nearest, res);
    if (rc || (rc = ev_pair_clouds(h, who, gt_xyzi, n_gt, gt_is_device, est_xyzi, n_est, est_is_device, voxel_leaf, &p)) || (rc = ov_check_gt(h, who, p)))
        return rc;
    return ov_run(h, p.g, p.ng, p.e, p.ne, voxelsize, per_est_dist, per_est_nearest, res);
}

int erasor_hip_overlap_map(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, double voxel_leaf, double voxelsize,
                           erasor_overlap_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_overlap_map";
    EvPair p;
    int rc = ov_check_args(h, voxel_leaf, voxelsize, false, res);
    if (rc || (rc = ev_pair_map(h, who, gt_xyzi, n_gt, gt_is_device, voxel_leaf, &p)) || (rc = ov_check_gt(h, who, p))) return rc;
    return ov_run(h, p.g, p.ng, p.e, p.ne, voxelsize, nullptr, nullptr, res);
}

// ---- every frame's pose against the map, before a run (the reference README's pitfalls 1, 3 and 5; kernels: align.hip.h) ----
// Like ov_run: the main stream, the evaluator's scratch, the map's tree sorted in bank 2.  Round trips: the per-frame counters once, the
// per-frame values once, and the summary's host-driven select (8 passes).

// the arguments both entry points check: ERASOR_E_INVALID with h->err set, else ERASOR_OK and the scans' point count in *n_scan
static int al_check_args(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets,
                         size_t n_frames, const float *T_lidar2body, const float *T_body2origin, double voxelsize, const void *rows) {
    if (!(voxelsize > 0) || !std::isfinite(voxelsize)) return invalid(h, who, "voxelsize must be a finite number > 0");
    if (n_frames > 65536) return invalid(h, who, "more than 65536 frames");
    if (!offsets) return invalid(h, who, "offsets is NULL (n_frames + 1 entries)");
    if (n_frames && (!rows || !T_body2origin)) return invalid(h, who, "rows or T_body2origin is NULL");
    const int rc = check_scan_offsets(h, who, scans_xyzi, n_scan_points, offsets, n_frames);
    if (rc) return rc;
    if (T_lidar2body && !all_finite(T_lidar2body, 16)) return invalid(h, who, "non-finite entry in T_lidar2body");
    if (!all_finite(T_body2origin, n_frames * 16)) return invalid(h, who, "non-finite entry in T_body2origin");
    return ERASOR_OK;
}

// the frames of one call on the device (align_frames, label_scans), for k_al_query's frame lookup: the offsets (< 2^30) in E.al_off, the
// frame of every query workgroup's first point (the last frame after the last) in E.al_wg, the poses in E.al_xf.  The host copies live in
// the caller's AlFrames until its next synchronisation.
struct AlFrames {
    std::vector<uint32_t> off, wg;
    std::vector<Xf> xf;
};
static int al_put_frames(erasor_hip_handle *h, uint32_t n, const uint64_t *offsets, uint32_t n_frames, const float *T_body2origin, AlFrames &F) {
    auto &E = h->ev;
    const uint32_t grid = cdiv(n, NN_QBLOCK), nf = std::max(n_frames, 1u);
    if (ensure(h, E.al_off, (size_t)nf + 1) || ensure(h, E.al_wg, (size_t)grid + 1) || ensure(h, E.al_xf, nf)) return ERASOR_E_NO_DEVICE;
    F.off.resize(n_frames + 1);
    F.wg.resize(grid + 1);
    F.xf.resize(nf);
    for (uint32_t f = 0; f <= n_frames; ++f) F.off[f] = (uint32_t)offsets[f];
    for (uint32_t b = 0, f = 0; b < grid; ++b) {  // the largest f < n_frames with off[f] <= b * NN_QBLOCK
        while (f + 1 < n_frames && F.off[f + 1] <= b * NN_QBLOCK) ++f;
        F.wg[b] = f;
    }
    F.wg[grid] = n_frames ? n_frames - 1 : 0;
    for (uint32_t f = 0; f < n_frames; ++f) F.xf[f] = to_xf(T_body2origin + 16 * (size_t)f);
    HIPC(h, hipMemcpyAsync(E.al_off.p, F.off.data(), F.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.al_wg.p, F.wg.data(), F.wg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.al_xf.p, F.xf.data(), nf * sizeof(Xf), hipMemcpyHostToDevice, h->stream));
    return ERASOR_OK;
}
static const float AL_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static int al_run(erasor_hip_handle *h, const char *who, const float4 *map, uint32_t n_map, const float4 *scans, uint32_t n, const uint64_t *offsets,
                  uint32_t n_frames, const float *T_lidar2body, const float *T_body2origin, double voxelsize, erasor_align_row *rows,
                  erasor_overlap_result *summary) {
    auto &E = h->ev;
    if (!n_map && n) {
        h->err = std::string(who) + ": empty map with a non-empty frame (no nearest point to measure against)";
        return ERASOR_E_INVALID;
    }
    const uint32_t grid = cdiv(n, NN_QBLOCK), nf = std::max(n_frames, 1u);
    if (ensure(h, E.nn_hist, OV_SEL_MAX * 256) || ensure(h, E.nn_dbits, (size_t)n + 1) || ensure(h, E.al_ctr, (size_t)nf * AL_NCTR) ||
        ensure(h, E.al_rank, nf) || ensure(h, E.al_val, (size_t)nf * OV_SEL_MAX))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    int rc = nn_build(h, map, n_map, who, "map", "map point(s)", &T);
    if (rc) return rc;
    AlFrames F;
    if ((rc = al_put_frames(h, n, offsets, n_frames, T_body2origin, F))) return rc;
    const std::vector<uint32_t> &off = F.off;
    HIPC(h, hipMemsetAsync(E.al_ctr.p, 0, (size_t)nf * AL_NCTR * sizeof(unsigned long long), h->stream));
    // the thresholds as overlap_report forms them: half = 0.5 * voxelsize, one = voxelsize, 2 * one
    const double half = 0.5 * voxelsize, one = voxelsize, two = 2 * one;
    if (n)
        LAUNCH(h, h->stream, "al_query", k_al_query, grid, NN_QBLOCK, scans, n, (const uint32_t *)E.al_off.p, (const uint32_t *)E.al_wg.p,
               to_xf(T_lidar2body ? T_lidar2body : AL_IDENTITY), (const Xf *)E.al_xf.p, T, half, one, two, E.nn_dbits.p, E.al_ctr.p);
    std::vector<unsigned long long> c((size_t)nf * AL_NCTR);
    HIPC(h, hipMemcpyAsync(c.data(), E.al_ctr.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    // every frame's ranks over its kept points, one select launch for all frames, and numpy's formulas on the six values of each
    std::vector<AlRanks> rk(nf);
    std::vector<double> g(2 * (size_t)nf), v((size_t)nf * OV_SEL_MAX);
    uint64_t n_kept = 0, below[3] = {0, 0, 0};
    unsigned long long max_bits = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const unsigned long long *cf = &c[(size_t)f * AL_NCTR];
        memset(&rk[f], 0, sizeof(AlRanks));
        rk[f].n = (off[f + 1] - off[f]) - cf[AL_NON_FINITE];
        if (rk[f].n) {
            uint64_t r6[OV_SEL_MAX];
            ov_ranks(rk[f].n, r6, &g[2 * f], &g[2 * f + 1]);
            for (uint32_t k = 0; k < OV_SEL_MAX; ++k) rk[f].rk[k] = r6[k];
        }
        n_kept += rk[f].n;
        below[0] += cf[AL_BELOW_HALF];
        below[1] += cf[AL_BELOW_ONE];
        below[2] += cf[AL_BELOW_TWO];
        max_bits = std::max(max_bits, cf[AL_MAX_BITS]);
    }
    if (n_kept) {
        HIPC(h, hipMemcpyAsync(E.al_rank.p, rk.data(), n_frames * sizeof(AlRanks), hipMemcpyHostToDevice, h->stream));
        LAUNCH(h, h->stream, "al_select", k_al_select, n_frames, 256, (const unsigned long long *)E.nn_dbits.p, (const uint32_t *)E.al_off.p,
               (const AlRanks *)E.al_rank.p, E.al_val.p);
        HIPC(h, hipMemcpyAsync(v.data(), E.al_val.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
    }
    for (uint32_t f = 0; f < n_frames; ++f) {
        const unsigned long long *cf = &c[(size_t)f * AL_NCTR];
        rows[f].n_points = off[f + 1] - off[f];
        rows[f].n_non_finite = cf[AL_NON_FINITE];
        ov_fill(rk[f].n, cf[AL_BELOW_HALF], cf[AL_BELOW_ONE], cf[AL_BELOW_TWO], cf[AL_MAX_BITS], &v[(size_t)f * OV_SEL_MAX], g[2 * f], g[2 * f + 1],
                &rows[f].r);
    }
    if (summary) {  // the kept points of all frames: the whole distance array, the dropped points' sentinels above every rank
        double sv[OV_SEL_MAX] = {}, g90 = 0, g99 = 0;
        if (n_kept) {
            uint64_t srk[OV_SEL_MAX];
            ov_ranks(n_kept, srk, &g90, &g99);
            if ((rc = ov_select(h, E.nn_dbits.p, n, srk, sv))) return rc;
        }
        ov_fill(n_kept, below[0], below[1], below[2], max_bits, sv, g90, g99, summary);
    }
    return ERASOR_OK;
}

int erasor_hip_align_frames_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi,
                                   size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device,
                                   const float T_lidar2body[16], const float *T_body2origin, double voxelsize, erasor_align_row *rows,
                                   erasor_overlap_result *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_align_frames_clouds";
    int rc = al_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, voxelsize, rows);
    if (rc || (rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    if ((rc = ev_input(h, map_xyzi, n_map, map_is_device, h->ev.gt, &m)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q)))
        return rc;
    return al_run(h, who, m, (uint32_t)n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, voxelsize, rows,
                  summary);
}

int erasor_hip_align_frames_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, double voxelsize,
                                erasor_align_row *rows, erasor_overlap_result *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_align_frames_map";
    int rc = al_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, voxelsize, rows);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return al_run(h, who, m, n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, voxelsize, rows, summary);
}

// ---- every frame's pose refined against the map: point-to-point ICP, all frames side by side (kernels: refine.hip.h) ----
// Like al_run: the main stream, the evaluator's scratch, the map's tree built once and sorted in bank 2.  Per iteration, for the live
// frames together: the poses and live flags up, k_rf_query and k_rf_partials, the frames' sums and counters back, and the solve below
// on the host -- a few dozen flops per frame, in + - * / and sqrt on doubles only (this file is compiled with -ffp-contract=off), so that
// evalmap.refine_poses, in plain Python floats, restates it bit for bit.

// cyclic Jacobi on the symmetric 4x4 A: pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), until every element above the diagonal is exactly
// zero before a sweep, or 32 sweeps.  A's diagonal: the eigenvalues; V's columns: the eigenvectors.
static void rf_jacobi4(double A[4][4], double V[4][4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[0][3] == 0.0 && A[1][2] == 0.0 && A[1][3] == 0.0 && A[2][3] == 0.0) break;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double at = theta < 0.0 ? -theta : theta;
                double t = 1.0 / (at + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {  // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {  // A <- Jt A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0;
                for (int i = 0; i < 4; ++i)
                    for (int j = i + 1; j < 4; ++j) A[j][i] = A[i][j];
                for (int k = 0; k < 4; ++k) {  // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// one frame's update from its sums S (RF_NSUM) over n >= 1 pairs: Horn's quaternion from the centred cross-covariance, R <- dR R,
// t <- t + delta.  *step_t: |delta|; *step_r: 2 |q_xyz| of the unit quaternion (w >= 0).
static void rf_solve(const double *S, uint64_t n, RfPose &P, double *step_t, double *step_r) {
    const double nn = (double)n;
    double mq[3], mm[3], H[3][3];
    for (int a = 0; a < 3; ++a) {
        mq[a] = S[a] / nn;
        mm[a] = S[3 + a] / nn;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) H[a][b] = S[6 + 3 * a + b] - (S[a] * S[3 + b]) / nn;
    double N[4][4], V[4][4];
    N[0][0] = (H[0][0] + H[1][1]) + H[2][2];
    N[0][1] = H[1][2] - H[2][1];
    N[0][2] = H[2][0] - H[0][2];
    N[0][3] = H[0][1] - H[1][0];
    N[1][1] = (H[0][0] - H[1][1]) - H[2][2];
    N[1][2] = H[0][1] + H[1][0];
    N[1][3] = H[2][0] + H[0][2];
    N[2][2] = (H[1][1] - H[0][0]) - H[2][2];
    N[2][3] = H[1][2] + H[2][1];
    N[3][3] = (H[2][2] - H[0][0]) - H[1][1];
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j) N[j][i] = N[i][j];
    rf_jacobi4(N, V);
    int k = 0;  // the largest eigenvalue, the first of equal ones
    for (int i = 1; i < 4; ++i)
        if (N[i][i] > N[k][k]) k = i;
    double w = V[0][k], x = V[1][k], y = V[2][k], z = V[3][k];
    if (w < 0.0) {
        w = -w;
        x = -x;
        y = -y;
        z = -z;
    }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / nrm;
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    const double D[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                            {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                            {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
    double d[3], R[9];
    for (int a = 0; a < 3; ++a) d[a] = mm[a] - ((D[a][0] * mq[0] + D[a][1] * mq[1]) + D[a][2] * mq[2]);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = (D[a][0] * P.R[b] + D[a][1] * P.R[3 + b]) + D[a][2] * P.R[6 + b];
    for (int e = 0; e < 9; ++e) P.R[e] = R[e];
    for (int a = 0; a < 3; ++a) P.t[a] = P.t[a] + d[a];
    *step_t = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    *step_r = 2.0 * sqrt((xx + yy) + zz);
}

static int rf_check_args(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets,
                         size_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_refine_params *p) {
    if (!p) return invalid(h, who, "params is NULL");
    if (p->max_iters < 1 || p->max_iters > 64) return invalid(h, who, "max_iters must be 1 .. 64");
    if (!(p->max_dist > 0) || !std::isfinite(p->max_dist)) return invalid(h, who, "max_dist must be a finite number > 0");
    if (!(p->eps_t > 0) || !std::isfinite(p->eps_t)) return invalid(h, who, "eps_t must be a finite number > 0");
    if (!(p->eps_r > 0) || !std::isfinite(p->eps_r)) return invalid(h, who, "eps_r must be a finite number > 0");
    if (n_frames > 65536) return invalid(h, who, "more than 65536 frames");
    if (!offsets) return invalid(h, who, "offsets is NULL (n_frames + 1 entries)");
    if (n_frames && !T_body2origin) return invalid(h, who, "T_body2origin is NULL");
    const int rc = check_scan_offsets(h, who, scans_xyzi, n_scan_points, offsets, n_frames);
    if (rc) return rc;
    if (T_lidar2body && !all_finite(T_lidar2body, 16)) return invalid(h, who, "non-finite entry in T_lidar2body");
    return ERASOR_OK;
}

static int rf_run(erasor_hip_handle *h, const char *who, const float4 *map, uint32_t n_map, const float4 *scans, uint32_t n, const uint64_t *offsets,
                  uint32_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_refine_params &prm, erasor_refine_row *rows,
                  erasor_refine_summary *summary) {
    auto &E = h->ev;
    if (!n_map && n) {
        h->err = std::string(who) + ": empty map with a non-empty frame (no nearest point to match)";
        return ERASOR_E_INVALID;
    }
    const uint32_t nf = std::max(n_frames, 1u);
    // the frames' chunks of RF_CHUNK points, counted from each frame's own first point
    std::vector<uint32_t> off(n_frames + 1), cb(n_frames + 1, 0u);
    for (uint32_t f = 0; f <= n_frames; ++f) off[f] = (uint32_t)offsets[f];
    for (uint32_t f = 0; f < n_frames; ++f) cb[f + 1] = cb[f] + cdiv(off[f + 1] - off[f], RF_CHUNK);
    const uint32_t grid = cb[n_frames];  // (<= n / 256 + n_frames)
    std::vector<RfChunk> chunks(grid);
    for (uint32_t f = 0; f < n_frames; ++f)
        for (uint32_t b = cb[f]; b < cb[f + 1]; ++b) chunks[b] = RfChunk{f, b - cb[f]};
    if (ensure(h, E.al_off, (size_t)nf + 1) || ensure(h, E.rf_cb, (size_t)nf + 1) || ensure(h, E.rf_chunk, (size_t)grid + 1) || ensure(h, E.rf_pose, nf) ||
        ensure(h, E.rf_live, nf) || ensure(h, E.rf_part, ((size_t)grid + 1) * RF_NSUM) || ensure(h, E.rf_sums, (size_t)nf * RF_NSUM) ||
        ensure(h, E.rf_ctr, (size_t)nf * RF_NCTR))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    int rc = nn_build(h, map, n_map, who, "map", "map point(s)", &T);
    if (rc) return rc;
    HIPC(h, hipMemcpyAsync(E.al_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.rf_cb.p, cb.data(), cb.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (grid) HIPC(h, hipMemcpyAsync(E.rf_chunk.p, chunks.data(), (size_t)grid * sizeof(RfChunk), hipMemcpyHostToDevice, h->stream));
    const Xf Tl = to_xf(T_lidar2body ? T_lidar2body : AL_IDENTITY);
    const double gate2 = prm.max_dist * prm.max_dist;
    const uint64_t min_pairs = std::max(prm.min_pairs, 1u);

    std::vector<RfPose> P(nf), P0(nf);
    for (uint32_t f = 0; f < n_frames; ++f) {  // the float32 pose, widened
        const float *Tf = T_body2origin + 16 * (size_t)f;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) P[f].R[3 * a + b] = (double)Tf[4 * a + b];
            P[f].t[a] = (double)Tf[4 * a + 3];
        }
        P0[f] = P[f];
    }
    std::vector<uint32_t> live(nf, 1u), status(nf, ERASOR_REFINE_MAX_ITERS), iters(nf, 0u);
    std::vector<double> S((size_t)nf * RF_NSUM, 0.0), d2_first(nf, 0.0);
    std::vector<unsigned long long> c((size_t)nf * RF_NCTR, 0ull), pairs_first(nf, 0ull), non_finite(nf, 0ull);
    // the live frames' sums and counters under the poses P (into S and c; a frame that is not live keeps what it had)
    auto evaluate = [&]() -> int {
        if (!n_frames) return ERASOR_OK;
        HIPC(h, hipMemcpyAsync(E.rf_pose.p, P.data(), (size_t)n_frames * sizeof(RfPose), hipMemcpyHostToDevice, h->stream));
        HIPC(h, hipMemcpyAsync(E.rf_live.p, live.data(), (size_t)n_frames * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPC(h, hipMemsetAsync(E.rf_ctr.p, 0, (size_t)n_frames * RF_NCTR * sizeof(unsigned long long), h->stream));
        if (grid)
            LAUNCH(h, h->stream, "rf_query", k_rf_query, grid, NN_QBLOCK, scans, (const uint32_t *)E.al_off.p, (const RfChunk *)E.rf_chunk.p, Tl,
                   (const RfPose *)E.rf_pose.p, (const uint32_t *)E.rf_live.p, map, T, gate2, E.rf_part.p, E.rf_ctr.p);
        LAUNCH(h, h->stream, "rf_partials", k_rf_partials<RF_NSUM>, cdiv(n_frames * RF_NSUM, 256), 256, (const double *)E.rf_part.p, (const uint32_t *)E.rf_cb.p,
               (const uint32_t *)E.rf_live.p, n_frames, E.rf_sums.p);
        HIPC(h, hipMemcpyAsync(S.data(), E.rf_sums.p, (size_t)n_frames * RF_NSUM * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipMemcpyAsync(c.data(), E.rf_ctr.p, (size_t)n_frames * RF_NCTR * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        return ERASOR_OK;
    };
    uint32_t n_live = n_frames;
    for (uint32_t it = 1; it <= prm.max_iters && n_live; ++it) {
        if ((rc = evaluate())) return rc;
        for (uint32_t f = 0; f < n_frames; ++f) {
            if (!live[f]) continue;
            const uint64_t np = c[(size_t)f * RF_NCTR + RF_PAIRS];
            if (it == 1) {
                pairs_first[f] = np;
                d2_first[f] = S[(size_t)f * RF_NSUM + 15];
                non_finite[f] = c[(size_t)f * RF_NCTR + RF_NON_FINITE];
            }
            if (np < min_pairs) {  // the frame keeps the pose it has
                status[f] = (uint64_t)(off[f + 1] - off[f]) == non_finite[f] ? ERASOR_REFINE_NO_POINTS : ERASOR_REFINE_FEW_PAIRS;
                live[f] = 0;
                --n_live;
                continue;
            }
            double st, sr;
            rf_solve(&S[(size_t)f * RF_NSUM], np, P[f], &st, &sr);
            iters[f] = it;
            if (st <= prm.eps_t && sr <= prm.eps_r) {
                status[f] = ERASOR_REFINE_CONVERGED;
                live[f] = 0;
                --n_live;
            }
        }
    }
    // the returned poses' pairs and distances: one more evaluation of every frame, nothing updated
    std::fill(live.begin(), live.end(), 1u);
    if ((rc = evaluate())) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    erasor_refine_summary sm;
    memset(&sm, 0, sizeof(sm));
    sm.n_frames = n_frames;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const uint64_t np = c[(size_t)f * RF_NCTR + RF_PAIRS];
        const double d2 = S[(size_t)f * RF_NSUM + 15];
        sm.n_status[status[f]] += 1;
        sm.n_pairs_first += pairs_first[f];
        sm.n_pairs_last += np;
        sm.sum_d2_first = sm.sum_d2_first + d2_first[f];
        sm.sum_d2_last = sm.sum_d2_last + d2;
        if (!rows) continue;
        erasor_refine_row r;
        memset(&r, 0, sizeof(r));
        const RfPose &A = P[f], &B = P0[f];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) r.T[4 * a + b] = A.R[3 * a + b];
            r.T[4 * a + 3] = A.t[a];
        }
        r.T[15] = 1.0;
        r.status = status[f];
        r.iters = iters[f];
        r.n_points = off[f + 1] - off[f];
        r.n_non_finite = non_finite[f];
        r.n_pairs_first = pairs_first[f];
        r.n_pairs_last = np;
        r.rms_first = pairs_first[f] ? sqrt(d2_first[f] / (double)pairs_first[f]) : nan;
        r.rms_last = np ? sqrt(d2 / (double)np) : nan;
        const double dx = A.t[0] - B.t[0], dy = A.t[1] - B.t[1], dz = A.t[2] - B.t[2];
        r.moved_t = sqrt((dx * dx + dy * dy) + dz * dz);
        double tr = 0.0;  // trace of R R0t: the rows' dot products, one after another
        for (int a = 0; a < 3; ++a) tr = tr + ((A.R[3 * a] * B.R[3 * a] + A.R[3 * a + 1] * B.R[3 * a + 1]) + A.R[3 * a + 2] * B.R[3 * a + 2]);
        double cs = (tr - 1.0) / 2.0;
        if (cs > 1.0) cs = 1.0;
        if (cs < -1.0) cs = -1.0;
        r.moved_r = acos(cs);
        rows[f] = r;
    }
    if (summary) *summary = sm;
    return ERASOR_OK;
}

int erasor_hip_refine_poses_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi,
                                   size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device,
                                   const float T_lidar2body[16], const float *T_body2origin, const erasor_refine_params *params,
                                   erasor_refine_row *rows, erasor_refine_summary *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_refine_poses_clouds";
    int rc = rf_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc || (rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    if ((rc = ev_input(h, map_xyzi, n_map, map_is_device, h->ev.gt, &m)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q)))
        return rc;
    return rf_run(h, who, m, (uint32_t)n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, rows,
                  summary);
}

int erasor_hip_refine_poses_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, const erasor_refine_params *params,
                                erasor_refine_row *rows, erasor_refine_summary *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_refine_poses_map";
    int rc = rf_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return rf_run(h, who, m, n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, rows, summary);
}

// ---- every scan's points labelled static / dynamic / unknown from a cleaned map (kernels: label_scans.hip.h) ----
// Like al_run: the main stream, the evaluator's scratch, the trees' sorts in bank 2.  One tree is resident at a time: the static map's,
// then -- for the points the static pass left -- the raw map's in the same scratch; a host raw map is brought in only then, into the
// buffer the static map's copy no longer needs (the tree holds its own sorted copy).  Round trips: the counters after each pass.

// T2: the largest double whose correctly rounded sqrt is < tau (tau finite, > 0), by steps of one ulp from tau * tau
static double ls_bound(double tau) {
    const double inf = std::numeric_limits<double>::infinity();
    double x = tau * tau;
    while (x > 0 && !(sqrt(x) < tau)) x = std::nextafter(x, 0.0);
    for (;;) {
        const double y = std::nextafter(x, inf);
        if (!(y < inf) || !(sqrt(y) < tau)) break;
        x = y;
    }
    return x;
}

// what a call's split arguments ask for
struct LsSplit {
    int code = 0;
    float *xyzi = nullptr;
    size_t cap = 0;
    uint64_t *offsets = nullptr;
    bool wanted() const { return xyzi || offsets; }
};

static int ls_check_args(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                         const float *T_lidar2body, const float *T_body2origin, double tau, const void *raw_xyzi, size_t n_raw, int have_raw,
                         const LsSplit &sp, const erasor_scan_label_row *rows) {
    if (!(tau > 0) || !std::isfinite(tau)) return invalid(h, who, "tau must be a finite number > 0");
    if (sp.wanted() && (sp.code < 0 || sp.code > 2)) return invalid(h, who, "split_code must be 0 (static), 1 (dynamic) or 2 (unknown)");
    if (sp.wanted() && sp.code == 2 && !have_raw) return invalid(h, who, "split_code 2 (unknown) needs a raw map");
    int rc = al_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, 1.0, rows);
    if (rc) return rc;
    return have_raw ? check_cloud(h, who, "NULL raw map or more than 2^30 raw map points", raw_xyzi, n_raw) : ERASOR_OK;
}

// the launch of one pass (list == nullptr: all n points; else the n_list left points)
static int ls_pass(erasor_hip_handle *h, const float4 *scans, uint32_t n, const uint32_t *list, uint32_t n_list, uint32_t n_frames, const Xf &Tl,
                   const NnTree &T, double T2, uint32_t code_hit, uint32_t code_miss, uint32_t count_miss, uint32_t *left) {
    auto &E = h->ev;
    const uint32_t m = list ? n_list : n;
    if (!m) return ERASOR_OK;
    LAUNCH(h, h->stream, "ls_query", k_ls_query, cdiv(m, NN_QBLOCK), NN_QBLOCK, scans, n, list, n_list, (const uint32_t *)E.al_off.p, n_frames,
           (const uint32_t *)E.al_wg.p, Tl, (const Xf *)E.al_xf.p, T, T2, code_hit, code_miss, count_miss, E.code.p, left, E.al_ctr.p);
    return ERASOR_OK;
}

static int ls_run(erasor_hip_handle *h, const char *who, const float4 *smap, uint32_t n_smap, const void *raw_xyzi, uint32_t n_raw, int raw_is_device,
                  int have_raw, const float4 *scans, uint32_t n, const uint64_t *offsets, uint32_t n_frames, const float *T_lidar2body,
                  const float *T_body2origin, double tau, uint8_t *codes, const LsSplit &sp, erasor_scan_label_row *rows,
                  erasor_scan_label_row *summary) {
    auto &E = h->ev;
    const double T2 = ls_bound(tau);
    const uint32_t nf = std::max(n_frames, 1u);
    const bool scan = have_raw || sp.wanted();
    if (ensure(h, E.al_ctr, (size_t)nf * LS_NCTR) || ensure(h, E.code, (size_t)n + 1) ||
        (scan && (ensure(h, E.fm_flag, (size_t)n + 1) || ensure(h, E.fm_pl, (size_t)n + 1) || ensure(h, E.fm_tops, n / 1024 + 4))) ||
        (have_raw && ensure(h, E.nn_near, (size_t)n + 1)) || (sp.xyzi && ensure(h, E.fm_out, (size_t)n + 1)))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    int rc = nn_build(h, smap, n_smap, who, "static map", "static map point(s)", &T);
    if (rc) return rc;
    AlFrames F;
    if ((rc = al_put_frames(h, n, offsets, n_frames, T_body2origin, F))) return rc;
    const std::vector<uint32_t> &off = F.off;
    const Xf Tl = to_xf(T_lidar2body ? T_lidar2body : AL_IDENTITY);
    HIPC(h, hipMemsetAsync(E.al_ctr.p, 0, (size_t)nf * LS_NCTR * sizeof(unsigned long long), h->stream));
    // the static pass: code 0, or 1 for now
    if ((rc = ls_pass(h, scans, n, nullptr, 0, n_frames, Tl, T, T2, LS_STATIC, LS_DYNAMIC, have_raw ? 0u : 1u,
                      have_raw ? E.fm_flag.p : (uint32_t *)nullptr)))
        return rc;
    std::vector<unsigned long long> c((size_t)nf * LS_NCTR, 0ull);
    if (have_raw) {
        // the points it left (kept and not static: nothing counted them yet), as an ascending list of their indices; then the raw map's
        // tree where the static map's was (built even when nothing is left: a bad raw map is refused whatever the scans hold), and the
        // raw pass over the list: code 1 stays, or 2
        HIPC(h, hipMemcpyAsync(c.data(), E.al_ctr.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        uint64_t decided = 0;
        for (uint32_t f = 0; f < n_frames; ++f)
            decided += c[(size_t)f * LS_NCTR + LS_STATIC] + c[(size_t)f * LS_NCTR + 3 + LS_STATIC] + c[(size_t)f * LS_NCTR + LS_NON_FINITE];
        const uint32_t n_left = n - (uint32_t)decided;
        if (n_left) {
            scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n, n, nullptr, nullptr, "ls_left");
            LAUNCH(h, h->stream, "ls_left", k_ls_list, cdiv(n, 256), 256, n, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p,
                   (const uint32_t *)E.fm_tops.p, E.nn_near.p);
        }
        const float4 *rmap = nullptr;
        if ((rc = ev_input(h, raw_xyzi, n_raw, raw_is_device, E.gt, &rmap)) ||
            (rc = nn_build(h, rmap, n_raw, who, "raw map", "raw map point(s)", &T)))
            return rc;
        if ((rc = ls_pass(h, scans, n, E.nn_near.p, n_left, n_frames, Tl, T, T2, LS_DYNAMIC, LS_UNKNOWN, 1u, nullptr))) return rc;
    }
    HIPC(h, hipMemcpyAsync(c.data(), E.al_ctr.p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    erasor_scan_label_row sum;
    memset(&sum, 0, sizeof(sum));
    uint64_t out_n = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const unsigned long long *cf = &c[(size_t)f * LS_NCTR];
        erasor_scan_label_row r;
        memset(&r, 0, sizeof(r));
        r.n_points = off[f + 1] - off[f];
        r.n_non_finite = cf[LS_NON_FINITE];
        r.n_label_out_of_range = cf[LS_LABEL_OOR];
        for (int g = 0; g < 2; ++g)
            for (int k = 0; k < 3; ++k) {
                r.n[g][k] = cf[g * 3 + k];
                sum.n[g][k] += r.n[g][k];
            }
        sum.n_points += r.n_points;
        sum.n_non_finite += r.n_non_finite;
        sum.n_label_out_of_range += r.n_label_out_of_range;
        rows[f] = r;
        if (sp.wanted()) {
            if (sp.offsets) sp.offsets[f] = out_n;
            out_n += r.n[0][sp.code] + r.n[1][sp.code];
        }
    }
    if (sp.offsets) sp.offsets[n_frames] = out_n;
    if (summary) *summary = sum;
    if (codes && n) HIPC(h, hipMemcpy(codes, E.code.p, n, hipMemcpyDeviceToHost));
    if (!sp.xyzi) return ERASOR_OK;
    if (out_n > sp.cap) return ERASOR_E_CAPACITY;
    if (!out_n) return ERASOR_OK;
    // the rows of the chosen code, as given: a stable compaction over the concatenated scans (frames are consecutive ranges)
    LAUNCH(h, h->stream, "ls_split", k_ls_flag, cdiv(n, 256), 256, (const uint8_t *)E.code.p, n, (uint32_t)sp.code, E.fm_flag.p);
    scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n, n, nullptr, nullptr, "ls_split");
    LAUNCH(h, h->stream, "ls_split", k_f_compact, cdiv(n, 256), 256, scans, n, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p,
           (const uint32_t *)E.fm_tops.p, E.fm_out.p);
    return d2h(h, sp.xyzi, E.fm_out.p, (size_t)out_n * sizeof(float4));
}

int erasor_hip_label_scans_clouds(erasor_hip_handle *h, const void *static_xyzi, size_t n_static, int static_is_device, const void *raw_xyzi, size_t n_raw,
                                  int raw_is_device, int have_raw, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                  int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, double tau, uint8_t *codes,
                                  int split_code, float *split_xyzi, size_t split_cap, uint64_t *split_offsets, erasor_scan_label_row *rows,
                                  erasor_scan_label_row *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_label_scans_clouds";
    LsSplit sp;
    sp.code = split_code, sp.xyzi = split_xyzi, sp.cap = split_cap, sp.offsets = split_offsets;
    int rc = ls_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, tau, raw_xyzi, n_raw, have_raw, sp, rows);
    if (rc || (rc = check_cloud(h, who, "NULL static map or more than 2^30 static map points", static_xyzi, n_static))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    if ((rc = ev_input(h, static_xyzi, n_static, static_is_device, h->ev.gt, &m)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q)))
        return rc;
    return ls_run(h, who, m, (uint32_t)n_static, raw_xyzi, (uint32_t)n_raw, raw_is_device, have_raw, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames,
                  T_lidar2body, T_body2origin, tau, codes, sp, rows, summary);
}

int erasor_hip_label_scans_map(erasor_hip_handle *h, const void *raw_xyzi, size_t n_raw, int raw_is_device, int have_raw, const void *scans_xyzi,
                               size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device, const float T_lidar2body[16],
                               const float *T_body2origin, double tau, uint8_t *codes, int split_code, float *split_xyzi, size_t split_cap,
                               uint64_t *split_offsets, erasor_scan_label_row *rows, erasor_scan_label_row *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_label_scans_map";
    LsSplit sp;
    sp.code = split_code, sp.xyzi = split_xyzi, sp.cap = split_cap, sp.offsets = split_offsets;
    int rc = ls_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, tau, raw_xyzi, n_raw, have_raw, sp, rows);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return ls_run(h, who, m, n_map, raw_xyzi, (uint32_t)n_raw, raw_is_device, have_raw, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body,
                  T_body2origin, tau, codes, sp, rows, summary);
}

// ---- a cloud as connected objects: Euclidean clustering, listed and filtered by size (kernels: cluster.hip.h) ----
// Like ev_run: the main stream, the evaluator's scratch; the grid is the evaluator's, at a cell edge a little above tol.  One round trip
// for the counters (they size the rows), then the rows, the ids and the kept cloud.
static int cl_check_args(erasor_hip_handle *h, const char *who, double tol, const void *res) {
    if (!res) return invalid(h, who, "res is NULL");
    if (!(tol > 0) || !std::isfinite(tol)) return invalid(h, who, "tol must be a finite number > 0");
    return ERASOR_OK;
}

static int cl_run(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, double tol, size_t min_size, size_t max_size, uint32_t *ids,
                  erasor_cluster_row *rows, size_t cap_rows, float *kept_xyzi, size_t cap_points, erasor_cluster_result *res) {
    static_assert(sizeof(erasor_cluster_row) == CL_ROW * sizeof(uint32_t), "the device writes erasor_cluster_row word by word");
    auto &E = h->ev;
    erasor_cluster_result r;
    memset(&r, 0, sizeof(r));
    r.n_points = n;
    if (!n) {
        *res = r;
        return ERASOR_OK;
    }
    const uint32_t mn = (uint32_t)std::min<size_t>(std::max<size_t>(min_size, 1), 0xFFFFFFFFull);
    const uint32_t mx = (uint32_t)std::min<size_t>(max_size, 0xFFFFFFFFull);  // (0: no upper limit)
    uint32_t nb = 1024;  // buckets: ev_run's (a power of two >= the cloud's size)
    while (nb < n) nb <<= 1;
    const size_t n1 = (size_t)n + 1;
    if (ensure(h, E.ctr, EV_NCTR) || ensure(h, E.cl_ctr, CL_NCTR) || ensure(h, E.cnt, (size_t)nb + 1) || ensure(h, E.pl, (size_t)nb + 1) ||
        ensure(h, E.tops, nb / 1024 + 4) || ensure(h, E.bkt, n1) || ensure(h, E.pts, n1) || ensure(h, E.idx, n1) || ensure(h, E.cl_parent, n1) ||
        ensure(h, E.cl_root, n1) || ensure(h, E.cl_tab, n1 * CL_TROW) || ensure(h, E.cl_rank, n1) || ensure(h, E.cl_ids, n1) || ensure(h, E.fm_flag, n1) ||
        ensure(h, E.fm_pl, n1) || ensure(h, E.fm_tops, n / 1024 + 4))
        return ERASOR_E_NO_DEVICE;
    const double cell = tol * CL_CELL_MARGIN, tol2 = tol * tol;
    const uint32_t g = cdiv(n, 256);
    HIPC(h, hipMemsetAsync(E.ctr.p, 0, EV_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.cl_ctr.p, 0, CL_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.cnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), h->stream));
    LAUNCH(h, h->stream, "cl_index", k_ev_hist, g, 256, pts, n, cell, nb - 1, E.bkt.p, E.cnt.p, E.ctr.p);
    scan_u32(h, h->stream, E.cnt.p, E.pl.p, E.tops.p, nb + 1, nb + 1, nullptr, nullptr, "cl_index");
    LAUNCH(h, h->stream, "cl_index", k_ev_offsets, cdiv(nb + 1, 256), 256, (const uint32_t *)E.pl.p, (const uint32_t *)E.tops.p, nb + 1, E.cnt.p, E.pl.p);
    LAUNCH(h, h->stream, "cl_index", k_ev_scatter, g, 256, pts, n, (const uint32_t *)E.bkt.p, E.pl.p, E.pts.p, E.idx.p);
    LAUNCH(h, h->stream, "cl_index", k_cl_init, g, 256, n, E.cl_parent.p, E.cl_tab.p);
    LAUNCH(h, h->stream, "cl_unite", k_cl_unite, g, 256, pts, n, (const float4 *)E.pts.p, (const uint32_t *)E.idx.p, (const uint32_t *)E.cnt.p, nb - 1, cell, tol2,
           E.cl_parent.p);
    LAUNCH(h, h->stream, "cl_table", k_cl_table, g, 256, pts, n, (const uint32_t *)E.cl_parent.p, E.cl_root.p, E.cl_tab.p);
    LAUNCH(h, h->stream, "cl_list", k_cl_flags, g, 256, n, (const uint32_t *)E.cl_root.p, (const uint32_t *)E.cl_tab.p, mn, mx, E.fm_flag.p, E.cl_ctr.p);
    unsigned long long c[EV_NCTR], cc[CL_NCTR];
    HIPC(h, hipMemcpyAsync(c, E.ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(cc, E.cl_ctr.p, sizeof(cc), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (c[EV_NON_FINITE])
        return invalid(h, who, "non-finite coordinate (NaN / Inf) in " + std::to_string(c[EV_NON_FINITE]) + " point(s)");
    r.n_clusters = cc[CL_C_CLUSTERS];
    r.n_listed = cc[CL_C_LISTED];
    r.n_points_listed = cc[CL_C_POINTS_LISTED];
    r.n_singletons = cc[CL_C_SINGLETONS];
    r.largest = cc[CL_C_LARGEST];
    *res = r;
    if (!ids && !rows && !kept_xyzi) return ERASOR_OK;
    // the listed roots ranked in index order (= `first` order), their rows, every point's row
    if (ensure(h, E.cl_rows, (size_t)r.n_listed * CL_ROW + 1)) return ERASOR_E_NO_DEVICE;
    scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n, n, nullptr, nullptr, "cl_list");
    LAUNCH(h, h->stream, "cl_list", k_cl_rows, g, 256, n, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p, (const uint32_t *)E.fm_tops.p,
           (const uint32_t *)E.cl_tab.p, E.cl_rows.p, E.cl_rank.p);
    if (ids || kept_xyzi)
        LAUNCH(h, h->stream, "cl_list", k_cl_ids, g, 256, n, (const uint32_t *)E.cl_root.p, (const uint32_t *)E.cl_rank.p, E.cl_ids.p, E.fm_flag.p);
    int rc;
    if (ids && (rc = d2h(h, ids, E.cl_ids.p, (size_t)n * sizeof(uint32_t)))) return rc;
    if ((rows && r.n_listed > cap_rows) || (kept_xyzi && r.n_points_listed > cap_points)) {
        HIPC(h, hipStreamSynchronize(h->stream));
        return ERASOR_E_CAPACITY;
    }
    if (rows && (rc = d2h(h, rows, E.cl_rows.p, (size_t)r.n_listed * sizeof(erasor_cluster_row)))) return rc;
    if (kept_xyzi && r.n_points_listed) {
        // the rows of the listed clusters' points, as given: the stable compaction over the keep flags
        if (ensure(h, E.fm_out, n1)) return ERASOR_E_NO_DEVICE;
        scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n, n, nullptr, nullptr, "cl_keep");
        LAUNCH(h, h->stream, "cl_keep", k_f_compact, g, 256, pts, n, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p, (const uint32_t *)E.fm_tops.p,
               E.fm_out.p);
        return d2h(h, kept_xyzi, E.fm_out.p, (size_t)r.n_points_listed * sizeof(float4));
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    return ERASOR_OK;
}

int erasor_hip_cluster_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, double tol, size_t min_size, size_t max_size, uint32_t *ids,
                              erasor_cluster_row *rows, size_t cap_rows, float *kept_xyzi, size_t cap_points, erasor_cluster_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_cluster_clouds";
    int rc = cl_check_args(h, who, tol, res);
    if (rc || (rc = check_cloud(h, who, BAD_CLOUD, xyzi, n))) return rc;
    const float4 *p = nullptr;
    if (n) {
        HIPC(h, hipSetDevice(h->device));
        if ((rc = ev_input(h, xyzi, n, is_device, h->ev.gt, &p))) return rc;
    }
    return cl_run(h, who, p, (uint32_t)n, tol, min_size, max_size, ids, rows, cap_rows, kept_xyzi, cap_points, res);
}

int erasor_hip_cluster_map(erasor_hip_handle *h, double tol, size_t min_size, size_t max_size, uint32_t *ids, erasor_cluster_row *rows, size_t cap_rows,
                           float *kept_xyzi, size_t cap_points, erasor_cluster_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_cluster_map";
    int rc = cl_check_args(h, who, tol, res);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &p, &n))) return rc;
    return cl_run(h, who, p, n, tol, min_size, max_size, ids, rows, cap_rows, kept_xyzi, cap_points, res);
}

// ---- the decision per object: per-point votes spread over the clusters they fall on, fragments reverted (kernels: objects.hip.h) ----
// Like cl_run: the main stream, the evaluator's scratch, the evaluator's grid at a cell edge a little above tol -- over the non-ground
// rows, compacted stably so that a cluster's lowest compacted index is its lowest given index.  The host counts the ground bytes it was
// given (they size the compacted cloud's launches); one round trip for the counters (they size the rows), then the copies.
static int obj_check_args(erasor_hip_handle *h, const char *who, const uint8_t *votes, const erasor_object_vote_params *p, const void *res) {
    if (!res) return invalid(h, who, "res is NULL");
    if (!p) return invalid(h, who, "params is NULL");
    if (!votes) return invalid(h, who, "votes is NULL");
    if (!(p->tol > 0) || !std::isfinite(p->tol)) return invalid(h, who, "tol must be a finite number > 0");
    if (p->vote_thr < 1 || p->vote_thr > 255) return invalid(h, who, "vote_thr must be within 1 .. 255");
    if (!(p->max_extent >= 0) || !std::isfinite(p->max_extent)) return invalid(h, who, "max_extent must be 0 or a finite number > 0");
    if (!(p->remove_ratio > 0 && p->remove_ratio <= 1)) return invalid(h, who, "remove_ratio must be within (0, 1]");
    if (!(p->revert_ratio >= 0 && p->revert_ratio < 1) || !(p->revert_ratio < p->remove_ratio))
        return invalid(h, who, "revert_ratio must be within [0, 1) and below remove_ratio");
    return ERASOR_OK;
}

static int obj_run(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, const uint8_t *votes, const uint8_t *ground,
                   const erasor_object_vote_params &P, uint8_t *mask, uint32_t *ids, erasor_object_row *rows, size_t cap_rows, float *kept_xyzi,
                   size_t cap_points, erasor_object_vote_result *res) {
    static_assert(sizeof(erasor_object_row) == OB_ROW * sizeof(uint32_t), "the device writes erasor_object_row word by word");
    auto &E = h->ev;
    erasor_object_vote_result r;
    memset(&r, 0, sizeof(r));
    r.n_points = n;
    if (!n) {
        *res = r;
        return ERASOR_OK;
    }
    ObDecide D;
    D.min_size = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(P.min_size, 1), 0xFFFFFFFFull);
    D.max_size = (uint32_t)std::min<uint64_t>(P.max_size, 0xFFFFFFFFull);  // (0: no upper limit)
    D.min_voted = (uint32_t)std::min<uint64_t>(P.min_voted, 0xFFFFFFFFull);
    D.max_extent = P.max_extent, D.remove_ratio = P.remove_ratio, D.revert_ratio = P.revert_ratio;
    uint32_t m = n;  // the points in the graph
    if (ground)
        for (uint32_t i = 0; i < n; ++i) m -= ground[i] != 0 ? 1u : 0u;
    uint32_t nb = 1024;  // buckets: ev_run's (a power of two >= the compacted cloud's size)
    while (nb < m) nb <<= 1;
    const size_t n1 = (size_t)n + 1;
    if (ensure(h, E.ctr, EV_NCTR) || ensure(h, E.ob_ctr, OB_NCTR) || ensure(h, E.cnt, (size_t)nb + 1) || ensure(h, E.pl, (size_t)nb + 1) ||
        ensure(h, E.tops, nb / 1024 + 4) || ensure(h, E.bkt, n1) || ensure(h, E.pts, n1) || ensure(h, E.idx, n1) || ensure(h, E.cl_parent, n1) ||
        ensure(h, E.cl_root, n1) || ensure(h, E.ob_tab, n1 * OB_TROW) || ensure(h, E.ob_code, n1) || ensure(h, E.ob_touched, n1) ||
        ensure(h, E.ob_keep, n1) || ensure(h, E.ob_ids, n1) || ensure(h, E.ob_mask, n1) || ensure(h, E.ob_cls, n1) || ensure(h, E.ob_votes, n1) ||
        ensure(h, E.fm_pl, n1) || ensure(h, E.fm_tops, n / 1024 + 4))
        return ERASOR_E_NO_DEVICE;
    if (ground && (ensure(h, E.ob_ground, n1) || ensure(h, E.ob_ng, n1) || ensure(h, E.ob_gpl, n1) || ensure(h, E.ob_gtops, n / 1024 + 4) ||
                   ensure(h, E.ob_pts, n1) || ensure(h, E.ob_src, n1)))
        return ERASOR_E_NO_DEVICE;
    const double cell = P.tol * CL_CELL_MARGIN, tol2 = P.tol * P.tol;
    const uint32_t g = cdiv(n, 256), gm = cdiv(m, 256);
    HIPC(h, hipMemcpyAsync(E.ob_votes.p, votes, n, hipMemcpyHostToDevice, h->stream));
    if (ground) HIPC(h, hipMemcpyAsync(E.ob_ground.p, ground, n, hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.ctr.p, 0, EV_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.ob_ctr.p, 0, OB_NCTR * sizeof(unsigned long long), h->stream));
    LAUNCH(h, h->stream, "obj_flags", k_obj_flags, g, 256, pts, n, (const uint8_t *)E.ob_votes.p, ground ? (const uint8_t *)E.ob_ground.p : nullptr, P.vote_thr,
           E.ob_cls.p, ground ? E.ob_ng.p : nullptr, E.ob_ctr.p);
    // the graph's points: the rows given, or the non-ground ones of them in the order given with their source indices
    const float4 *cp = pts;
    const uint32_t *src = nullptr, *gpl = nullptr, *gtops = nullptr;
    if (ground) {
        scan_u32(h, h->stream, E.ob_ng.p, E.ob_gpl.p, E.ob_gtops.p, n, n, nullptr, nullptr, "obj_flags");
        LAUNCH(h, h->stream, "obj_flags", k_obj_compact, g, 256, pts, n, (const uint32_t *)E.ob_ng.p, (const uint32_t *)E.ob_gpl.p, (const uint32_t *)E.ob_gtops.p,
               E.ob_pts.p, E.ob_src.p);
        cp = E.ob_pts.p, src = E.ob_src.p, gpl = E.ob_gpl.p, gtops = E.ob_gtops.p;
    }
    if (m) {
        HIPC(h, hipMemsetAsync(E.cnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), h->stream));
        LAUNCH(h, h->stream, "obj_index", k_ev_hist, gm, 256, cp, m, cell, nb - 1, E.bkt.p, E.cnt.p, E.ctr.p);
        scan_u32(h, h->stream, E.cnt.p, E.pl.p, E.tops.p, nb + 1, nb + 1, nullptr, nullptr, "obj_index");
        LAUNCH(h, h->stream, "obj_index", k_ev_offsets, cdiv(nb + 1, 256), 256, (const uint32_t *)E.pl.p, (const uint32_t *)E.tops.p, nb + 1, E.cnt.p, E.pl.p);
        LAUNCH(h, h->stream, "obj_index", k_ev_scatter, gm, 256, cp, m, (const uint32_t *)E.bkt.p, E.pl.p, E.pts.p, E.idx.p);
        LAUNCH(h, h->stream, "obj_index", k_obj_init, gm, 256, m, E.cl_parent.p, E.ob_tab.p);
        LAUNCH(h, h->stream, "obj_unite", k_cl_unite, gm, 256, cp, m, (const float4 *)E.pts.p, (const uint32_t *)E.idx.p, (const uint32_t *)E.cnt.p, nb - 1, cell,
               tol2, E.cl_parent.p);
        LAUNCH(h, h->stream, "obj_table", k_obj_table, gm, 256, cp, m, (const uint32_t *)E.cl_parent.p, (const uint8_t *)E.ob_cls.p, src, E.cl_root.p, E.ob_tab.p);
        LAUNCH(h, h->stream, "obj_decide", k_obj_decide, gm, 256, m, (const uint32_t *)E.cl_root.p, (const uint32_t *)E.ob_tab.p, D, E.ob_code.p, E.ob_touched.p,
               E.ob_ctr.p);
        // the touched roots ranked in compacted-index order (= `first` order)
        scan_u32(h, h->stream, E.ob_touched.p, E.fm_pl.p, E.fm_tops.p, m, m, nullptr, nullptr, "obj_decide");
    }
    LAUNCH(h, h->stream, "obj_apply", k_obj_apply, g, 256, pts, n, (const uint8_t *)E.ob_cls.p, gpl, gtops, (const uint32_t *)E.cl_root.p,
           (const uint32_t *)E.ob_code.p, (const uint32_t *)E.ob_touched.p, (const uint32_t *)E.fm_pl.p, (const uint32_t *)E.fm_tops.p, P.ground_keep,
           E.ob_mask.p, E.ob_ids.p, E.ob_keep.p, E.ob_ctr.p);
    // (k_ev_hist's own counters in E.ctr cover the compacted rows only and stay on the device: a ground point's coordinates count too)
    unsigned long long oc[OB_NCTR];
    HIPC(h, hipMemcpyAsync(oc, E.ob_ctr.p, sizeof(oc), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (oc[OB_C_NON_FINITE])
        return invalid(h, who, "non-finite coordinate (NaN / Inf) in " + std::to_string(oc[OB_C_NON_FINITE]) + " point(s)");
    r.n_ground = oc[OB_C_GROUND];
    r.n_clusters = oc[OB_C_CLUSTERS];
    r.n_touched = oc[OB_C_TOUCHED];
    r.n_removed_clusters = oc[OB_C_REMOVED_CL];
    r.n_reverted_clusters = oc[OB_C_REVERTED_CL];
    r.n_not_object = oc[OB_C_NOT_OBJECT];
    r.n_voted = oc[OB_C_VOTED];
    r.n_removed = oc[OB_C_REMOVED];
    r.n_grown = oc[OB_C_GROWN];
    r.n_grown_dynamic = oc[OB_C_GROWN_DYN];
    r.n_reverted = oc[OB_C_REVERTED];
    r.n_reverted_dynamic = oc[OB_C_REVERTED_DYN];
    r.n_ground_reverted = oc[OB_C_GROUND_REV];
    r.n_ground_reverted_dynamic = oc[OB_C_GROUND_REV_DYN];
    r.largest = oc[OB_C_LARGEST];
    *res = r;
    int rc;
    if (mask && (rc = d2h(h, mask, E.ob_mask.p, n))) return rc;
    if (ids && (rc = d2h(h, ids, E.ob_ids.p, (size_t)n * sizeof(uint32_t)))) return rc;
    const uint64_t n_kept = r.n_points - r.n_removed;
    if ((rows && r.n_touched > cap_rows) || (kept_xyzi && n_kept > cap_points)) return ERASOR_E_CAPACITY;
    if (rows && r.n_touched) {
        if (ensure(h, E.ob_rows, (size_t)r.n_touched * OB_ROW + 1)) return ERASOR_E_NO_DEVICE;
        LAUNCH(h, h->stream, "obj_rows", k_obj_rows, gm, 256, m, (const uint32_t *)E.ob_touched.p, (const uint32_t *)E.fm_pl.p, (const uint32_t *)E.fm_tops.p,
               (const uint32_t *)E.ob_tab.p, (const uint32_t *)E.ob_code.p, src, E.ob_rows.p);
        if ((rc = d2h(h, rows, E.ob_rows.p, (size_t)r.n_touched * sizeof(erasor_object_row)))) return rc;
    }
    if (kept_xyzi && n_kept) {
        // the rows with mask 1, as given: the stable compaction over the keep flags (the touched flags' scan is spent by now)
        if (ensure(h, E.fm_out, n1)) return ERASOR_E_NO_DEVICE;
        scan_u32(h, h->stream, E.ob_keep.p, E.fm_pl.p, E.fm_tops.p, n, n, nullptr, nullptr, "obj_keep");
        LAUNCH(h, h->stream, "obj_keep", k_f_compact, g, 256, pts, n, (const uint32_t *)E.ob_keep.p, (const uint32_t *)E.fm_pl.p, (const uint32_t *)E.fm_tops.p,
               E.fm_out.p);
        return d2h(h, kept_xyzi, E.fm_out.p, (size_t)n_kept * sizeof(float4));
    }
    return ERASOR_OK;
}

int erasor_hip_object_vote_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, const uint8_t *votes, const uint8_t *ground,
                                  const erasor_object_vote_params *params, uint8_t *mask, uint32_t *ids, erasor_object_row *rows, size_t cap_rows,
                                  float *kept_xyzi, size_t cap_points, erasor_object_vote_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_object_vote_clouds";
    int rc = obj_check_args(h, who, votes, params, res);
    if (rc || (rc = check_cloud(h, who, BAD_CLOUD, xyzi, n))) return rc;
    const float4 *p = nullptr;
    if (n) {
        HIPC(h, hipSetDevice(h->device));
        if ((rc = ev_input(h, xyzi, n, is_device, h->ev.gt, &p))) return rc;
    }
    return obj_run(h, who, p, (uint32_t)n, votes, ground, *params, mask, ids, rows, cap_rows, kept_xyzi, cap_points, res);
}

int erasor_hip_object_vote_map(erasor_hip_handle *h, const uint8_t *votes, const uint8_t *ground, size_t n, const erasor_object_vote_params *params,
                               uint8_t *mask, uint32_t *ids, erasor_object_row *rows, size_t cap_rows, float *kept_xyzi, size_t cap_points,
                               erasor_object_vote_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_object_vote_map";
    int rc = obj_check_args(h, who, votes, params, res);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &p, &n_map))) return rc;
    if (n != (size_t)n_map) return invalid(h, who, "n is not the map's size (erasor_hip_map_size)");
    return obj_run(h, who, p, n_map, votes, ground, *params, mask, ids, rows, cap_rows, kept_xyzi, cap_points, res);
}

// ---- k nearest neighbours, radius counts and the density filters on them (kernels: knn.hip.h) ----
// Like ov_run and cl_run: the main stream, the evaluator's scratch, the tree's sort in bank 2, the grid the evaluator's at a cell edge a
// little above the radius.  Round trips: the counters once per pass, and the host-driven select (8 passes) per score and for the MAD.
static const double KN_NAN = std::numeric_limits<double>::quiet_NaN();

static int kn_check_k(erasor_hip_handle *h, const char *who, uint32_t k) {
    return (k < 1 || k > KN_MAX_K) ? invalid(h, who, "k must be within 1 .. 32") : ERASOR_OK;
}
static int kn_check_radius(erasor_hip_handle *h, const char *who, double radius) {
    return (!(radius > 0) || !std::isfinite(radius)) ? invalid(h, who, "radius must be a finite number > 0") : ERASOR_OK;
}
static int kn_check_lists(erasor_hip_handle *h, const char *who, size_t n, uint32_t k, bool lists) {
    return (lists && (uint64_t)n * k > (1ull << 30)) ? invalid(h, who, "neighbour lists need n * k <= 2^30") : ERASOR_OK;
}
static int kn_check_filter(erasor_hip_handle *h, const char *who, const erasor_density_filter *f, const void *res) {
    if (!res) return invalid(h, who, "res is NULL");
    if (!f) return invalid(h, who, "filter is NULL");
    if (f->score != ERASOR_DENSITY_KTH && f->score != ERASOR_DENSITY_MEAN && f->score != ERASOR_DENSITY_COUNT)
        return invalid(h, who, "unknown score (ERASOR_DENSITY_KTH, _MEAN or _COUNT)");
    if (f->rule != ERASOR_DENSITY_ABS && f->rule != ERASOR_DENSITY_MAD) return invalid(h, who, "unknown rule (ERASOR_DENSITY_ABS or _MAD)");
    if (f->score == ERASOR_DENSITY_COUNT) return kn_check_radius(h, who, f->radius);
    int rc = kn_check_k(h, who, f->k);
    if (rc) return rc;
    if (f->rule == ERASOR_DENSITY_ABS && (!(f->thr >= 0) || !std::isfinite(f->thr))) return invalid(h, who, "thr must be a finite number >= 0");
    if (f->rule == ERASOR_DENSITY_MAD && (!(f->mul >= 0) || !std::isfinite(f->mul))) return invalid(h, who, "mul must be a finite number >= 0");
    return ERASOR_OK;
}

// the counters at their identities
static int kn_reset(erasor_hip_handle *h) {
    auto &E = h->ev;
    if (ensure(h, E.kn_ctr, KN_NCTR) || ensure(h, E.nn_hist, OV_SEL_MAX * 256)) return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemsetAsync(E.kn_ctr.p, 0, KN_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.kn_ctr.p + KN_C_KTH_MIN, 0xFF, sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.kn_ctr.p + KN_C_MEAN_MIN, 0xFF, sizeof(unsigned long long), h->stream));
    return ERASOR_OK;
}
static int kn_counters(erasor_hip_handle *h, unsigned long long c[KN_NCTR]) {
    return d2h(h, c, h->ev.kn_ctr.p, KN_NCTR * sizeof(unsigned long long));
}

// both knn scores of pts[0 .. n) (n > 0) into E.kn_kth / E.kn_mean, with `lists` the neighbour lists into E.kn_ni / E.kn_nd; the counters in c
static int kn_search(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, uint32_t k, bool lists, unsigned long long c[KN_NCTR]) {
    auto &E = h->ev;
    int rc = kn_reset(h);
    if (rc) return rc;
    const size_t n1 = (size_t)n + 1;
    if (ensure(h, E.kn_kth, n1) || ensure(h, E.kn_mean, n1) ||
        (lists && (ensure(h, E.kn_ni, (size_t)n * k + 1) || ensure(h, E.kn_nd, (size_t)n * k + 1))))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    if ((rc = nn_build(h, pts, n, who, "cloud", "point(s)", &T))) return rc;
    uint32_t *ni = lists ? E.kn_ni.p : nullptr;
    double *nd = lists ? E.kn_nd.p : nullptr;
    const uint32_t g = cdiv(n, KN_QBLOCK);
#define KN_QUERY(KC) LAUNCH(h, h->stream, "kn_query", k_kn_query<KC>, g, KN_QBLOCK, T, k, E.kn_kth.p, E.kn_mean.p, ni, nd, E.kn_ctr.p)
    if (k <= 8) KN_QUERY(8);
    else if (k <= 16) KN_QUERY(16);
    else KN_QUERY(32);
#undef KN_QUERY
    return kn_counters(h, c);
}

// the radius counts of pts[0 .. n) (n > 0) into E.kn_cnt, and as float64 bit patterns into E.kn_kth; the counters in c
static int kn_count(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, double radius, unsigned long long c[KN_NCTR]) {
    auto &E = h->ev;
    uint32_t nb = 1024;  // buckets: ev_run's (a power of two >= the cloud's size)
    while (nb < n) nb <<= 1;
    const size_t n1 = (size_t)n + 1;
    int rc = kn_reset(h);
    if (rc) return rc;
    if (ensure(h, E.ctr, EV_NCTR) || ensure(h, E.cnt, (size_t)nb + 1) || ensure(h, E.pl, (size_t)nb + 1) || ensure(h, E.tops, nb / 1024 + 4) ||
        ensure(h, E.bkt, n1) || ensure(h, E.pts, n1) || ensure(h, E.idx, n1) || ensure(h, E.kn_cnt, n1) || ensure(h, E.kn_kth, n1))
        return ERASOR_E_NO_DEVICE;
    const double cell = radius * CL_CELL_MARGIN, r2 = radius * radius;
    const uint32_t g = cdiv(n, 256);
    HIPC(h, hipMemsetAsync(E.ctr.p, 0, EV_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.cnt.p, 0, ((size_t)nb + 1) * sizeof(uint32_t), h->stream));
    LAUNCH(h, h->stream, "kn_index", k_ev_hist, g, 256, pts, n, cell, nb - 1, E.bkt.p, E.cnt.p, E.ctr.p);
    scan_u32(h, h->stream, E.cnt.p, E.pl.p, E.tops.p, nb + 1, nb + 1, nullptr, nullptr, "kn_index");
    LAUNCH(h, h->stream, "kn_index", k_ev_offsets, cdiv(nb + 1, 256), 256, (const uint32_t *)E.pl.p, (const uint32_t *)E.tops.p, nb + 1, E.cnt.p, E.pl.p);
    LAUNCH(h, h->stream, "kn_index", k_ev_scatter, g, 256, pts, n, (const uint32_t *)E.bkt.p, E.pl.p, E.pts.p, E.idx.p);
    unsigned long long ec[EV_NCTR];
    if ((rc = d2h(h, ec, E.ctr.p, sizeof(ec)))) return rc;
    if (ec[EV_NON_FINITE]) return invalid(h, who, "non-finite coordinate (NaN / Inf) in " + std::to_string(ec[EV_NON_FINITE]) + " point(s)");
    LAUNCH(h, h->stream, "kn_count", k_kn_count, g, 256, pts, n, (const float4 *)E.pts.p, (const uint32_t *)E.idx.p, (const uint32_t *)E.cnt.p, nb - 1, cell, r2,
           E.kn_cnt.p, E.kn_kth.p, E.kn_ctr.p);
    return kn_counters(h, c);
}

static void kn_no_stats(erasor_score_stats *s) {
    s->n_scored = 0;
    s->min = s->median = s->p90 = s->p99 = s->max = KN_NAN;
}
// the statistics of the n_scored finite scores among bits[0 .. n): infinite scores lie above every rank
static int kn_stats(erasor_hip_handle *h, const unsigned long long *bits, uint32_t n, uint64_t n_scored, unsigned long long min_bits,
                    unsigned long long max_bits, erasor_score_stats *s) {
    kn_no_stats(s);
    if (!n_scored) return ERASOR_OK;
    uint64_t rk[OV_SEL_MAX];
    double v[OV_SEL_MAX] = {}, g90 = 0, g99 = 0;
    ov_ranks(n_scored, rk, &g90, &g99);
    const int rc = ov_select(h, bits, n, rk, v);
    if (rc) return rc;
    s->n_scored = n_scored;
    memcpy(&s->min, &min_bits, sizeof(double));
    memcpy(&s->max, &max_bits, sizeof(double));
    s->median = (n_scored % 2) ? v[0] : (v[0] + v[1]) / 2.0;
    s->p90 = ov_lerp(v[2], v[3], g90);
    s->p99 = ov_lerp(v[4], v[5], g99);
    return ERASOR_OK;
}

static int kn_run(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, uint32_t k, uint32_t *nbr_idx, double *nbr_dist, double *kth,
                  double *mean, erasor_knn_result *res) {
    auto &E = h->ev;
    erasor_knn_result r;
    memset(&r, 0, sizeof(r));
    r.n_points = n;
    kn_no_stats(&r.kth);
    kn_no_stats(&r.mean);
    if (!n) {
        *res = r;
        return ERASOR_OK;
    }
    unsigned long long c[KN_NCTR];
    int rc = kn_search(h, who, pts, n, k, nbr_idx || nbr_dist, c);
    if (rc) return rc;
    r.n_short = c[KN_C_SHORT];
    const uint64_t n_scored = n - r.n_short;
    if ((rc = kn_stats(h, E.kn_kth.p, n, n_scored, c[KN_C_KTH_MIN], c[KN_C_KTH_MAX], &r.kth)) ||
        (rc = kn_stats(h, E.kn_mean.p, n, n_scored, c[KN_C_MEAN_MIN], c[KN_C_MEAN_MAX], &r.mean)))
        return rc;
    *res = r;
    if (nbr_idx && (rc = d2h(h, nbr_idx, E.kn_ni.p, (size_t)n * k * sizeof(uint32_t)))) return rc;
    if (nbr_dist && (rc = d2h(h, nbr_dist, E.kn_nd.p, (size_t)n * k * sizeof(double)))) return rc;
    if (kth && (rc = d2h(h, kth, E.kn_kth.p, (size_t)n * sizeof(double)))) return rc;
    if (mean && (rc = d2h(h, mean, E.kn_mean.p, (size_t)n * sizeof(double)))) return rc;
    return ERASOR_OK;
}

static int rc_run(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, double radius, uint32_t *count, erasor_score_stats *res) {
    kn_no_stats(res);
    if (!n) return ERASOR_OK;
    unsigned long long c[KN_NCTR];
    int rc = kn_count(h, who, pts, n, radius, c);
    if (rc || (rc = kn_stats(h, h->ev.kn_kth.p, n, n, c[KN_C_KTH_MIN], c[KN_C_KTH_MAX], res))) return rc;
    return count ? d2h(h, count, h->ev.kn_cnt.p, (size_t)n * sizeof(uint32_t)) : ERASOR_OK;
}

static int df_run(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, const erasor_density_filter &f, uint8_t *keep_mask,
                  float *kept_xyzi, size_t cap_points, erasor_density_result *res) {
    auto &E = h->ev;
    erasor_density_result r;
    memset(&r, 0, sizeof(r));
    r.n_points = n;
    r.m = r.mad = r.thr = r.min = r.median = r.p90 = r.p99 = r.max = KN_NAN;
    const bool by_count = f.score == ERASOR_DENSITY_COUNT, mad = !by_count && f.rule == ERASOR_DENSITY_MAD;
    if (by_count) r.thr = (double)f.min_neighbors;
    else if (!mad) r.thr = f.thr;
    if (!n) {
        *res = r;
        return ERASOR_OK;
    }
    unsigned long long c[KN_NCTR];
    int rc = by_count ? kn_count(h, who, pts, n, f.radius, c) : kn_search(h, who, pts, n, f.k, false, c);
    if (rc) return rc;
    const bool use_mean = f.score == ERASOR_DENSITY_MEAN;
    const unsigned long long *score = use_mean ? E.kn_mean.p : E.kn_kth.p;
    r.n_short = by_count ? 0 : c[KN_C_SHORT];
    erasor_score_stats st;
    if ((rc = kn_stats(h, score, n, n - r.n_short, c[use_mean ? KN_C_MEAN_MIN : KN_C_KTH_MIN], c[use_mean ? KN_C_MEAN_MAX : KN_C_KTH_MAX], &st))) return rc;
    r.n_scored = st.n_scored;
    r.min = st.min, r.median = st.median, r.p90 = st.p90, r.p99 = st.p99, r.max = st.max;
    const size_t n1 = (size_t)n + 1;
    const uint32_t g = cdiv(n, 256);
    if (mad && st.n_scored) {
        // the median absolute deviation: |s - m| over the scored points, and a second select for its median
        if (ensure(h, E.kn_dev, n1)) return ERASOR_E_NO_DEVICE;
        r.m = st.median;
        LAUNCH(h, h->stream, "kn_mad", k_kn_absdev, g, 256, score, n, r.m, E.kn_dev.p);
        const uint64_t lo = (st.n_scored - 1) / 2, hi = st.n_scored / 2;
        const uint64_t rk[OV_SEL_MAX] = {lo, hi, lo, hi, lo, hi};
        double v[OV_SEL_MAX] = {};
        if ((rc = ov_select(h, E.kn_dev.p, n, rk, v))) return rc;
        r.mad = (st.n_scored % 2) ? v[0] : (v[0] + v[1]) / 2.0;
        const double scaled = 1.4826 * r.mad;
        r.thr = r.m + f.mul * scaled;
    }
    if (ensure(h, E.fm_flag, n1) || ensure(h, E.fm_pl, n1) || ensure(h, E.fm_tops, n / 1024 + 4) || ensure(h, E.kn_mask, n1)) return ERASOR_E_NO_DEVICE;
    LAUNCH(h, h->stream, "kn_keep", k_kn_keep, g, 256, pts, n, score, (const uint32_t *)E.kn_cnt.p, by_count ? 1u : 0u, r.thr, f.min_neighbors, E.fm_flag.p,
           E.kn_mask.p, E.kn_ctr.p);
    if ((rc = kn_counters(h, c))) return rc;
    r.n_kept = c[KN_C_KEPT];
    r.n_removed = n - r.n_kept;
    r.n_removed_dynamic = c[KN_C_REMOVED_DYNAMIC];
    r.n_removed_static = c[KN_C_REMOVED_STATIC];
    *res = r;
    if (keep_mask && (rc = d2h(h, keep_mask, E.kn_mask.p, n))) return rc;
    if (kept_xyzi && r.n_kept > cap_points) return ERASOR_E_CAPACITY;
    if (kept_xyzi && r.n_kept) {
        // the kept rows, as given: the stable compaction over the keep flags
        if (ensure(h, E.fm_out, n1)) return ERASOR_E_NO_DEVICE;
        scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n, n, nullptr, nullptr, "kn_keep");
        LAUNCH(h, h->stream, "kn_keep", k_f_compact, g, 256, pts, n, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p, (const uint32_t *)E.fm_tops.p,
               E.fm_out.p);
        return d2h(h, kept_xyzi, E.fm_out.p, (size_t)r.n_kept * sizeof(float4));
    }
    return ERASOR_OK;
}

// the caller's cloud (checked, brought in through h->ev.gt) or the handle's map (h->ev.map) on the device
static int kn_cloud(erasor_hip_handle *h, const char *who, const void *xyzi, size_t n, int is_device, const float4 **p) {
    int rc = check_cloud(h, who, BAD_CLOUD, xyzi, n);
    if (rc || !n) return rc;
    HIPC(h, hipSetDevice(h->device));
    return ev_input(h, xyzi, n, is_device, h->ev.gt, p);
}

int erasor_hip_knn_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, uint32_t k, uint32_t *nbr_idx, double *nbr_dist, double *kth,
                          double *mean, erasor_knn_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_knn_clouds";
    if (!res) return invalid(h, who, "res is NULL");
    const float4 *p = nullptr;
    int rc = kn_check_k(h, who, k);
    if (rc || (rc = check_cloud(h, who, BAD_CLOUD, xyzi, n)) || (rc = kn_check_lists(h, who, n, k, nbr_idx || nbr_dist)) ||
        (rc = kn_cloud(h, who, xyzi, n, is_device, &p)))
        return rc;
    return kn_run(h, who, p, (uint32_t)n, k, nbr_idx, nbr_dist, kth, mean, res);
}

int erasor_hip_knn_map(erasor_hip_handle *h, uint32_t k, uint32_t *nbr_idx, double *nbr_dist, double *kth, double *mean, erasor_knn_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_knn_map";
    if (!res) return invalid(h, who, "res is NULL");
    int rc = kn_check_k(h, who, k);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &p, &n)) || (rc = kn_check_lists(h, who, n, k, nbr_idx || nbr_dist))) return rc;
    return kn_run(h, who, p, n, k, nbr_idx, nbr_dist, kth, mean, res);
}

int erasor_hip_radius_count_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, double radius, uint32_t *count,
                                   erasor_score_stats *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_radius_count_clouds";
    if (!res) return invalid(h, who, "res is NULL");
    const float4 *p = nullptr;
    int rc = kn_check_radius(h, who, radius);
    if (rc || (rc = kn_cloud(h, who, xyzi, n, is_device, &p))) return rc;
    return rc_run(h, who, p, (uint32_t)n, radius, count, res);
}

int erasor_hip_radius_count_map(erasor_hip_handle *h, double radius, uint32_t *count, erasor_score_stats *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_radius_count_map";
    if (!res) return invalid(h, who, "res is NULL");
    int rc = kn_check_radius(h, who, radius);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &p, &n))) return rc;
    return rc_run(h, who, p, n, radius, count, res);
}

int erasor_hip_density_filter_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, const erasor_density_filter *filter,
                                     uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_density_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_density_filter_clouds";
    const float4 *p = nullptr;
    int rc = kn_check_filter(h, who, filter, res);
    if (rc || (rc = kn_cloud(h, who, xyzi, n, is_device, &p))) return rc;
    return df_run(h, who, p, (uint32_t)n, *filter, keep_mask, kept_xyzi, cap_points, res);
}

int erasor_hip_density_filter_map(erasor_hip_handle *h, const erasor_density_filter *filter, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points,
                                  erasor_density_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_density_filter_map";
    int rc = kn_check_filter(h, who, filter, res);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &p, &n))) return rc;
    return df_run(h, who, p, n, *filter, keep_mask, kept_xyzi, cap_points, res);
}

// ---- every point's surface normal, curvature and eigenvalues from its k nearest neighbours (kernel: normals.hip.h) ----
// Like kn_run: the main stream, the evaluator's scratch, the tree's sort in bank 2.  Round trips: the counters once, and the host-driven
// select (8 passes) for the curvature's statistics.
static int nm_check_args(erasor_hip_handle *h, const char *who, uint32_t k, const double *viewpoint, const void *res) {
    if (!res) return invalid(h, who, "res is NULL");
    if (k < NM_MIN_K || k > KN_MAX_K) return invalid(h, who, "k must be within 2 .. 32");
    if (viewpoint && !(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2])))
        return invalid(h, who, "viewpoint must be three finite numbers");
    return ERASOR_OK;
}

// the device part: the normals and curvature of pts[0 .. n) (n > 0, T their tree) into E.nm_nrm (if want_nrm), E.nm_curv and E.nm_eig (if
// want_eig), the counters into E.nm_ctr.  Nothing is copied out; erasor_hip_refine_poses_plane_* reads the two arrays where they lie.
static int nm_device(erasor_hip_handle *h, const float4 *pts, uint32_t n, const NnTree &T, uint32_t k, const double *viewpoint, bool want_nrm,
                     bool want_eig) {
    auto &E = h->ev;
    const size_t n1 = (size_t)n + 1;
    if (ensure(h, E.nm_ctr, NM_NCTR) || ensure(h, E.nm_curv, n1) || (want_nrm && ensure(h, E.nm_nrm, 3 * n1)) || (want_eig && ensure(h, E.nm_eig, 3 * n1)))
        return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemsetAsync(E.nm_ctr.p, 0, NM_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.nm_ctr.p + NM_C_CURV_MIN, 0xFF, sizeof(unsigned long long), h->stream));
    float *nrm = want_nrm ? E.nm_nrm.p : nullptr;
    double *eig = want_eig ? E.nm_eig.p : nullptr;
    const uint32_t view = viewpoint ? 1u : 0u;
    const double vx = viewpoint ? viewpoint[0] : 0.0, vy = viewpoint ? viewpoint[1] : 0.0, vz = viewpoint ? viewpoint[2] : 0.0;
    const uint32_t g = cdiv(n, KN_QBLOCK);
#define NM_QUERY(KC) LAUNCH(h, h->stream, "nm_query", k_nm_query<KC>, g, KN_QBLOCK, T, pts, k, view, vx, vy, vz, nrm, E.nm_curv.p, eig, E.nm_ctr.p)
    if (k <= 8) NM_QUERY(8);
    else if (k <= 16) NM_QUERY(16);
    else NM_QUERY(32);
#undef NM_QUERY
    return ERASOR_OK;
}

static int nm_run(erasor_hip_handle *h, const char *who, const float4 *pts, uint32_t n, uint32_t k, const double *viewpoint, float *normals,
                  double *curvature, double *eigenvalues, erasor_normals_result *res) {
    auto &E = h->ev;
    erasor_normals_result r;
    memset(&r, 0, sizeof(r));
    r.n_points = n;
    kn_no_stats(&r.curvature);
    if (!n) {
        *res = r;
        return ERASOR_OK;
    }
    if (ensure(h, E.nn_hist, OV_SEL_MAX * 256)) return ERASOR_E_NO_DEVICE;
    NnTree T;
    int rc = nn_build(h, pts, n, who, "cloud", "point(s)", &T);
    if (rc || (rc = nm_device(h, pts, n, T, k, viewpoint, normals != nullptr, eigenvalues != nullptr))) return rc;
    unsigned long long c[NM_NCTR];
    if ((rc = d2h(h, c, E.nm_ctr.p, NM_NCTR * sizeof(unsigned long long)))) return rc;
    r.n_short = c[NM_C_SHORT];
    r.n_degenerate = c[NM_C_DEGENERATE];
    r.n_ambiguous = c[NM_C_AMBIGUOUS];
    r.n_flipped = c[NM_C_FLIPPED];
    if ((rc = kn_stats(h, E.nm_curv.p, n, n - r.n_short - r.n_degenerate, c[NM_C_CURV_MIN], c[NM_C_CURV_MAX], &r.curvature))) return rc;
    *res = r;
    if (normals && (rc = d2h(h, normals, E.nm_nrm.p, (size_t)n * 3 * sizeof(float)))) return rc;
    if (curvature && (rc = d2h(h, curvature, E.nm_curv.p, (size_t)n * sizeof(double)))) return rc;
    if (eigenvalues && (rc = d2h(h, eigenvalues, E.nm_eig.p, (size_t)n * 3 * sizeof(double)))) return rc;
    return ERASOR_OK;
}

int erasor_hip_normals_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, uint32_t k, const double *viewpoint, float *normals,
                              double *curvature, double *eigenvalues, erasor_normals_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_normals_clouds";
    const float4 *p = nullptr;
    int rc = nm_check_args(h, who, k, viewpoint, res);
    if (rc || (rc = kn_cloud(h, who, xyzi, n, is_device, &p))) return rc;
    return nm_run(h, who, p, (uint32_t)n, k, viewpoint, normals, curvature, eigenvalues, res);
}

int erasor_hip_normals_map(erasor_hip_handle *h, uint32_t k, const double *viewpoint, float *normals, double *curvature, double *eigenvalues,
                           erasor_normals_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_normals_map";
    int rc = nm_check_args(h, who, k, viewpoint, res);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &p, &n))) return rc;
    return nm_run(h, who, p, n, k, viewpoint, normals, curvature, eigenvalues, res);
}

// ---- every frame's pose refined point-to-plane against the map's normals, all frames side by side (kernel: refine_plane.hip.h) ----
// rf_run's shape, with the map's normals computed first by nm_device over the same tree and left on the device; per iteration the poses
// and live flags up, k_rfp_query and k_rf_partials, the frames' 29 sums and three counters back, and the 6x6 solve below on the host,
// restated in plain Python floats by evalmap._jacobi6 / refine_plane_solve.

// rf_jacobi4 on a symmetric 6x6: pivots (p, q), p < q, row-major
static void rfp_jacobi6(double A[6][6], double V[6][6]) {
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        bool diagonal = true;
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 6; ++j) diagonal = diagonal && A[i][j] == 0.0;
        if (diagonal) break;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double at = theta < 0.0 ? -theta : theta;
                double t = 1.0 / (at + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) {  // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; ++k) {  // A <- Jt A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0;
                for (int i = 0; i < 6; ++i)
                    for (int j = i + 1; j < 6; ++j) A[j][i] = A[i][j];
                for (int k = 0; k < 6; ++k) {  // V <- V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
}

// one frame's update from its sums S (RFP_NSUM): the pseudo-inverse of the normal equations over the eigen-directions above rank_tol,
// in index order; the rotation from the half vector, R <- D R, t <- t + x[3..5].  Returns the rank; 0: P is untouched.  *ratio:
// lambda_min / lambda_max, NaN when lambda_max is not > 0.
static uint32_t rfp_solve(const double *S, double rank_tol, RfPose &P, double *step_t, double *step_r, double *ratio) {
    double A[6][6], V[6][6], b[6], x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c, ++k) A[a][c] = A[c][a] = S[k];
    for (int a = 0; a < 6; ++a) b[a] = -S[21 + a];
    rfp_jacobi6(A, V);
    double lmax = A[0][0], lmin = A[0][0];
    for (int i = 1; i < 6; ++i) {
        if (A[i][i] > lmax) lmax = A[i][i];
        if (A[i][i] < lmin) lmin = A[i][i];
    }
    *ratio = lmax > 0 ? lmin / lmax : std::numeric_limits<double>::quiet_NaN();
    uint32_t rank = 0;
    for (int i = 0; i < 6; ++i) {
        if (!(lmax > 0 && A[i][i] > rank_tol * lmax)) continue;
        ++rank;
        const double g = (((((V[0][i] * b[0] + V[1][i] * b[1]) + V[2][i] * b[2]) + V[3][i] * b[3]) + V[4][i] * b[4]) + V[5][i] * b[5]) / A[i][i];
        for (int a = 0; a < 6; ++a) x[a] = x[a] + V[a][i] * g;
    }
    *step_t = 0.0;
    *step_r = 0.0;
    if (!rank) return 0;
    const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
    const double w = 1.0 / sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz));
    const double qx = hx * w, qy = hy * w, qz = hz * w;
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = w * qx, wy = w * qy, wz = w * qz;
    const double D[3][3] = {{1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)},
                            {2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)},
                            {2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)}};
    double R[9];
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) R[3 * a + c] = (D[a][0] * P.R[c] + D[a][1] * P.R[3 + c]) + D[a][2] * P.R[6 + c];
    for (int e = 0; e < 9; ++e) P.R[e] = R[e];
    for (int a = 0; a < 3; ++a) P.t[a] = P.t[a] + x[3 + a];
    *step_t = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    *step_r = 2.0 * sqrt((xx + yy) + zz);
    return rank;
}

static int rfp_check_args(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets,
                          size_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_refine_plane_params *p) {
    if (!p) return invalid(h, who, "params is NULL");
    if (p->normals_k < NM_MIN_K || p->normals_k > KN_MAX_K) return invalid(h, who, "normals_k must be within 2 .. 32");
    if (!(p->max_curvature > 0) || !std::isfinite(p->max_curvature)) return invalid(h, who, "max_curvature must be a finite number > 0");
    if (!(p->rank_tol >= 0 && p->rank_tol < 1)) return invalid(h, who, "rank_tol must be a finite number within [0, 1)");
    const erasor_refine_params base = {p->max_dist, p->eps_t, p->eps_r, p->max_iters, p->min_pairs};
    return rf_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, &base);
}

static int rfp_run(erasor_hip_handle *h, const char *who, const float4 *map, uint32_t n_map, const float4 *scans, uint32_t n, const uint64_t *offsets,
                   uint32_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_refine_plane_params &prm,
                   erasor_refine_plane_row *rows, erasor_refine_plane_summary *summary) {
    auto &E = h->ev;
    if (!n_map && n) {
        h->err = std::string(who) + ": empty map with a non-empty frame (no nearest point to match)";
        return ERASOR_E_INVALID;
    }
    const uint32_t nf = std::max(n_frames, 1u);
    // the frames' chunks of RF_CHUNK points, counted from each frame's own first point (as rf_run)
    std::vector<uint32_t> off(n_frames + 1), cb(n_frames + 1, 0u);
    for (uint32_t f = 0; f <= n_frames; ++f) off[f] = (uint32_t)offsets[f];
    for (uint32_t f = 0; f < n_frames; ++f) cb[f + 1] = cb[f] + cdiv(off[f + 1] - off[f], RF_CHUNK);
    const uint32_t grid = cb[n_frames];
    std::vector<RfChunk> chunks(grid);
    for (uint32_t f = 0; f < n_frames; ++f)
        for (uint32_t b = cb[f]; b < cb[f + 1]; ++b) chunks[b] = RfChunk{f, b - cb[f]};
    if (ensure(h, E.al_off, (size_t)nf + 1) || ensure(h, E.rf_cb, (size_t)nf + 1) || ensure(h, E.rf_chunk, (size_t)grid + 1) || ensure(h, E.rf_pose, nf) ||
        ensure(h, E.rf_live, nf) || ensure(h, E.rf_part, ((size_t)grid + 1) * RFP_NSUM) || ensure(h, E.rf_sums, (size_t)nf * RFP_NSUM) ||
        ensure(h, E.rf_ctr, (size_t)nf * RFP_NCTR))
        return ERASOR_E_NO_DEVICE;
    // one tree for the map's normals and for every iteration; the normals and the curvature stay in E.nm_nrm / E.nm_curv
    NnTree T;
    int rc = nn_build(h, map, n_map, who, "map", "map point(s)", &T);
    if (rc) return rc;
    uint64_t n_no_normal = 0;
    if (n_map) {
        if ((rc = nm_device(h, map, n_map, T, prm.normals_k, nullptr, true, false))) return rc;
        unsigned long long nc[NM_NCTR];
        if ((rc = d2h(h, nc, E.nm_ctr.p, NM_NCTR * sizeof(unsigned long long)))) return rc;
        n_no_normal = nc[NM_C_SHORT] + nc[NM_C_DEGENERATE];
    }
    HIPC(h, hipMemcpyAsync(E.al_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.rf_cb.p, cb.data(), cb.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (grid) HIPC(h, hipMemcpyAsync(E.rf_chunk.p, chunks.data(), (size_t)grid * sizeof(RfChunk), hipMemcpyHostToDevice, h->stream));
    const Xf Tl = to_xf(T_lidar2body ? T_lidar2body : AL_IDENTITY);
    const double gate2 = prm.max_dist * prm.max_dist;
    const uint64_t min_pairs = std::max(prm.min_pairs, 1u);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    std::vector<RfPose> P(nf), P0(nf);
    for (uint32_t f = 0; f < n_frames; ++f) {  // the float32 pose, widened
        const float *Tf = T_body2origin + 16 * (size_t)f;
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) P[f].R[3 * a + b] = (double)Tf[4 * a + b];
            P[f].t[a] = (double)Tf[4 * a + 3];
        }
        P0[f] = P[f];
    }
    std::vector<uint32_t> live(nf, 1u), status(nf, ERASOR_REFINE_MAX_ITERS), iters(nf, 0u), rank(nf, 0u);
    std::vector<double> S((size_t)nf * RFP_NSUM, 0.0), d2_first(nf, 0.0), r2_first(nf, 0.0), ratio(nf, nan);
    std::vector<unsigned long long> c((size_t)nf * RFP_NCTR, 0ull), pairs_first(nf, 0ull), non_finite(nf, 0ull), unusable_first(nf, 0ull);
    // the live frames' sums and counters under the poses P (into S and c; a frame that is not live keeps what it had)
    auto evaluate = [&]() -> int {
        if (!n_frames) return ERASOR_OK;
        HIPC(h, hipMemcpyAsync(E.rf_pose.p, P.data(), (size_t)n_frames * sizeof(RfPose), hipMemcpyHostToDevice, h->stream));
        HIPC(h, hipMemcpyAsync(E.rf_live.p, live.data(), (size_t)n_frames * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPC(h, hipMemsetAsync(E.rf_ctr.p, 0, (size_t)n_frames * RFP_NCTR * sizeof(unsigned long long), h->stream));
        if (grid)
            LAUNCH(h, h->stream, "rfp_query", k_rfp_query, grid, NN_QBLOCK, scans, (const uint32_t *)E.al_off.p, (const RfChunk *)E.rf_chunk.p, Tl,
                   (const RfPose *)E.rf_pose.p, (const uint32_t *)E.rf_live.p, map, (const float *)E.nm_nrm.p,
                   (const unsigned long long *)E.nm_curv.p, T, gate2, prm.max_curvature, E.rf_part.p, E.rf_ctr.p);
        LAUNCH(h, h->stream, "rfp_partials", k_rf_partials<RFP_NSUM>, cdiv(n_frames * RFP_NSUM, 256), 256, (const double *)E.rf_part.p,
               (const uint32_t *)E.rf_cb.p, (const uint32_t *)E.rf_live.p, n_frames, E.rf_sums.p);
        HIPC(h, hipMemcpyAsync(S.data(), E.rf_sums.p, (size_t)n_frames * RFP_NSUM * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipMemcpyAsync(c.data(), E.rf_ctr.p, (size_t)n_frames * RFP_NCTR * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        return ERASOR_OK;
    };
    uint32_t n_live = n_frames;
    for (uint32_t it = 1; it <= prm.max_iters && n_live; ++it) {
        if ((rc = evaluate())) return rc;
        for (uint32_t f = 0; f < n_frames; ++f) {
            if (!live[f]) continue;
            const double *Sf = &S[(size_t)f * RFP_NSUM];
            const uint64_t np = c[(size_t)f * RFP_NCTR + RFP_PAIRS];
            if (it == 1) {
                pairs_first[f] = np;
                d2_first[f] = Sf[28];
                r2_first[f] = Sf[27];
                non_finite[f] = c[(size_t)f * RFP_NCTR + RFP_NON_FINITE];
                unusable_first[f] = c[(size_t)f * RFP_NCTR + RFP_UNUSABLE];
            }
            bool ended = false;
            if (np < min_pairs) {  // the frame keeps the pose it has
                status[f] = (uint64_t)(off[f + 1] - off[f]) == non_finite[f] ? ERASOR_REFINE_NO_POINTS : ERASOR_REFINE_FEW_PAIRS;
                ended = true;
            } else {
                double st, sr;
                rank[f] = rfp_solve(Sf, prm.rank_tol, P[f], &st, &sr, &ratio[f]);
                if (!rank[f]) {  // nothing to solve for: the pose is kept
                    status[f] = ERASOR_REFINE_DEGENERATE;
                    ended = true;
                } else {
                    iters[f] = it;
                    if (st <= prm.eps_t && sr <= prm.eps_r) {
                        status[f] = ERASOR_REFINE_CONVERGED;
                        ended = true;
                    }
                }
            }
            if (ended) {
                live[f] = 0;
                --n_live;
            }
        }
    }
    // the returned poses' pairs, distances and residuals: one more evaluation of every frame, nothing updated
    std::fill(live.begin(), live.end(), 1u);
    if ((rc = evaluate())) return rc;
    erasor_refine_plane_summary sm;
    memset(&sm, 0, sizeof(sm));
    sm.n_frames = n_frames;
    sm.n_map_no_normal = n_no_normal;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const uint64_t np = c[(size_t)f * RFP_NCTR + RFP_PAIRS];
        const double d2 = S[(size_t)f * RFP_NSUM + 28], r2 = S[(size_t)f * RFP_NSUM + 27];
        sm.n_status[status[f]] += 1;
        sm.n_pairs_first += pairs_first[f];
        sm.n_pairs_last += np;
        sm.sum_d2_first = sm.sum_d2_first + d2_first[f];
        sm.sum_d2_last = sm.sum_d2_last + d2;
        sm.sum_r2_first = sm.sum_r2_first + r2_first[f];
        sm.sum_r2_last = sm.sum_r2_last + r2;
        if (!rows) continue;
        erasor_refine_plane_row r;
        memset(&r, 0, sizeof(r));
        const RfPose &A = P[f], &B = P0[f];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) r.T[4 * a + b] = A.R[3 * a + b];
            r.T[4 * a + 3] = A.t[a];
        }
        r.T[15] = 1.0;
        r.status = status[f];
        r.iters = iters[f];
        r.n_points = off[f + 1] - off[f];
        r.n_non_finite = non_finite[f];
        r.n_pairs_first = pairs_first[f];
        r.n_pairs_last = np;
        r.rms_first = pairs_first[f] ? sqrt(d2_first[f] / (double)pairs_first[f]) : nan;
        r.rms_last = np ? sqrt(d2 / (double)np) : nan;
        const double dx = A.t[0] - B.t[0], dy = A.t[1] - B.t[1], dz = A.t[2] - B.t[2];
        r.moved_t = sqrt((dx * dx + dy * dy) + dz * dz);
        double tr = 0.0;  // trace of R R0t: the rows' dot products, one after another
        for (int a = 0; a < 3; ++a) tr = tr + ((A.R[3 * a] * B.R[3 * a] + A.R[3 * a + 1] * B.R[3 * a + 1]) + A.R[3 * a + 2] * B.R[3 * a + 2]);
        double cs = (tr - 1.0) / 2.0;
        if (cs > 1.0) cs = 1.0;
        if (cs < -1.0) cs = -1.0;
        r.moved_r = acos(cs);
        r.rank = rank[f];
        r.lambda_ratio = ratio[f];
        r.n_unusable_first = unusable_first[f];
        r.n_unusable_last = c[(size_t)f * RFP_NCTR + RFP_UNUSABLE];
        r.rms_plane_first = pairs_first[f] ? sqrt(r2_first[f] / (double)pairs_first[f]) : nan;
        r.rms_plane_last = np ? sqrt(r2 / (double)np) : nan;
        rows[f] = r;
    }
    if (summary) *summary = sm;
    return ERASOR_OK;
}

int erasor_hip_refine_poses_plane_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi,
                                         size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device,
                                         const float T_lidar2body[16], const float *T_body2origin, const erasor_refine_plane_params *params,
                                         erasor_refine_plane_row *rows, erasor_refine_plane_summary *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_refine_poses_plane_clouds";
    int rc = rfp_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc || (rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    if ((rc = ev_input(h, map_xyzi, n_map, map_is_device, h->ev.gt, &m)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q)))
        return rc;
    return rfp_run(h, who, m, (uint32_t)n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, rows,
                   summary);
}

int erasor_hip_refine_poses_plane_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                      int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                                      const erasor_refine_plane_params *params, erasor_refine_plane_row *rows,
                                      erasor_refine_plane_summary *summary) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_refine_poses_plane_map";
    int rc = rfp_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return rfp_run(h, who, m, n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, rows, summary);
}

// ---- the see-through check: every scan's range image votes on every map point (kernels: visibility.hip.h) ----
// Like al_run: the main stream, the evaluator's scratch; with k > 0 the map's tree (bank 2) and normals as rfp_run takes them, once a
// call.  The frames are cut into batches whose images fit the budget; per batch one memset, one k_vis_image over the batch's scan points
// and one k_vis_vote over the map.  Round trips: the normals' counters (k > 0), and at the end the per-frame counters, the decision's
// counters and the outputs asked for.

static int vs_check_args(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets,
                         size_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_visibility *p) {
    if (!p) return invalid(h, who, "params is NULL");
    if (p->width % 8 || p->width < 8 || p->width > VIS_MAX_W) return invalid(h, who, "width must be a multiple of 8 within 8 .. 4096");
    if (p->height < 1 || p->height > VIS_MAX_H) return invalid(h, who, "height must be within 1 .. 256");
    const uint32_t nc = p->width / 8 - 1, nr = p->height + 1;
    if ((nc && !p->col_tan) || !p->row_tan) return invalid(h, who, "col_tan or row_tan is NULL");
    for (uint32_t j = 0; j < nc; ++j)
        if (!(p->col_tan[j] > 0 && p->col_tan[j] < 1) || (j && !(p->col_tan[j] > p->col_tan[j - 1])))
            return invalid(h, who, "col_tan must be strictly increasing within (0, 1)");
    for (uint32_t j = 0; j < nr; ++j)
        if (!std::isfinite(p->row_tan[j]) || (j && !(p->row_tan[j] > p->row_tan[j - 1])))
            return invalid(h, who, "row_tan must be finite and strictly increasing");
    if (!std::isfinite(p->min_range) || !std::isfinite(p->max_range) || !(p->min_range >= 0) || !(p->min_range < p->max_range))
        return invalid(h, who, "0 <= min_range < max_range, both finite");
    if (!std::isfinite(p->margin_abs) || !std::isfinite(p->margin_rel) || !(p->margin_abs >= 0) || !(p->margin_rel >= 0))
        return invalid(h, who, "the margins must be finite numbers >= 0");
    if (p->window > 2) return invalid(h, who, "window must be 0, 1 or 2");
    if (p->k && (p->k < NM_MIN_K || p->k > KN_MAX_K)) return invalid(h, who, "k must be 0 or within 2 .. 32");
    if (!std::isfinite(p->min_cos) || !std::isfinite(p->hit_weight) || !(p->hit_weight >= 0))
        return invalid(h, who, "min_cos must be finite and hit_weight a finite number >= 0");
    if (n_frames > ERASOR_VISIBILITY_MAX_FRAMES) return invalid(h, who, "more than 65535 frames");
    if (!offsets) return invalid(h, who, "offsets is NULL (n_frames + 1 entries)");
    if (n_frames && !T_body2origin) return invalid(h, who, "T_body2origin is NULL");
    const int rc = check_scan_offsets(h, who, scans_xyzi, n_scan_points, offsets, n_frames);
    if (rc) return rc;
    if (T_lidar2body && !all_finite(T_lidar2body, 16)) return invalid(h, who, "non-finite entry in T_lidar2body");
    if (!all_finite(T_body2origin, n_frames * 16)) return invalid(h, who, "non-finite entry in T_body2origin");
    return ERASOR_OK;
}

// a frame's map-to-lidar transform and origin: evalmap.visibility_transforms, the same function in the same order; false: not finite
static bool vs_frame(const float *A, const float *B, VisFrame *F) {
    double M[3][4];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            const double v = ((double)A[4 * i + 0] * (double)B[0 + j] + (double)A[4 * i + 1] * (double)B[4 + j]) + (double)A[4 * i + 2] * (double)B[8 + j];
            M[i][j] = j == 3 ? v + (double)A[4 * i + 3] : v;
        }
    bool ok = true;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) F->m[4 * i + j] = M[j][i];
        F->m[4 * i + 3] = -((M[0][i] * M[0][3] + M[1][i] * M[1][3]) + M[2][i] * M[2][3]);
        F->o[i] = M[i][3];
    }
    F->pad = 0.0;
    for (int k = 0; k < 12; ++k) ok = ok && std::isfinite(F->m[k]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) ok = ok && std::isfinite(M[i][j]);
    return ok;
}

static int vs_run(erasor_hip_handle *h, const char *who, const float4 *map, uint32_t n_map, const float4 *scans, uint32_t n, const uint64_t *offsets,
                  uint32_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_visibility &prm, uint16_t *votes,
                  uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_visibility_row *rows, erasor_visibility_result *res) {
    auto &E = h->ev;
    const uint32_t W = prm.width, H = prm.height, M = W / 8, nf = std::max(n_frames, 1u);
    const VisParams P{W, H, M, prm.window, prm.min_range, prm.max_range, prm.margin_abs, prm.margin_rel, prm.min_cos};
    // the frames: transforms (refused before anything runs), offsets, every image workgroup's first frame
    std::vector<VisFrame> fr(nf);
    const float *Tl = T_lidar2body ? T_lidar2body : AL_IDENTITY;
    for (uint32_t f = 0; f < n_frames; ++f)
        if (!vs_frame(T_body2origin + 16 * (size_t)f, Tl, &fr[f])) return invalid(h, who, "non-finite transform of frame " + std::to_string(f));
    const uint32_t grid_all = cdiv(n, 256);
    std::vector<uint32_t> off(n_frames + 1), wg(grid_all + 1);
    for (uint32_t f = 0; f <= n_frames; ++f) off[f] = (uint32_t)offsets[f];
    for (uint32_t b = 0, f = 0; b < grid_all; ++b) {  // the largest f < n_frames with off[f] <= b * 256 (as al_put_frames)
        while (f + 1 < n_frames && off[f + 1] <= b * 256u) ++f;
        wg[b] = f;
    }
    wg[grid_all] = n_frames ? n_frames - 1 : 0;
    // the batches: as many whole images as fit the budget, at least one
    const uint64_t image_bytes = (uint64_t)H * W * sizeof(uint32_t);
    const uint64_t budget = prm.image_budget_bytes ? prm.image_budget_bytes : ERASOR_VISIBILITY_IMAGE_BUDGET;
    const uint32_t batch = (uint32_t)std::min<uint64_t>(nf, std::max<uint64_t>(1, budget / image_bytes));
    const size_t n1 = (size_t)n_map + 1, ntab = (size_t)(M - 1) + (H + 1);
    if (ensure(h, E.al_off, (size_t)nf + 1) || ensure(h, E.al_wg, (size_t)grid_all + 1) || ensure(h, E.vs_frames, nf) || ensure(h, E.vs_tab, ntab) ||
        ensure(h, E.vs_img, (size_t)batch * H * W) || ensure(h, E.vs_votes, n1) || ensure(h, E.vs_ctr, (size_t)nf * VIS_NCTR + VD_NCTR) ||
        ensure(h, E.fm_flag, n1) || ensure(h, E.fm_pl, n1) || ensure(h, E.fm_tops, n_map / 1024 + 4) || ensure(h, E.kn_mask, n1))
        return ERASOR_E_NO_DEVICE;
    // the map's normals, once a call (rfp_run's): they stay in E.nm_nrm
    uint64_t n_no_normal = 0;
    int rc;
    if (prm.k && n_map) {
        NnTree T;
        if ((rc = nn_build(h, map, n_map, who, "map", "map point(s)", &T)) || (rc = nm_device(h, map, n_map, T, prm.k, nullptr, true, false))) return rc;
        unsigned long long nc[NM_NCTR];
        if ((rc = d2h(h, nc, E.nm_ctr.p, NM_NCTR * sizeof(unsigned long long)))) return rc;
        n_no_normal = nc[NM_C_SHORT] + nc[NM_C_DEGENERATE];
    }
    std::vector<double> tabs(ntab);
    for (uint32_t j = 0; j + 1 < M; ++j) tabs[j] = prm.col_tan[j];
    for (uint32_t j = 0; j <= H; ++j) tabs[(M - 1) + j] = prm.row_tan[j];
    unsigned long long *const dctr = E.vs_ctr.p + (size_t)nf * VIS_NCTR;  // the decision's counters, behind the frames'
    HIPC(h, hipMemcpyAsync(E.al_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.al_wg.p, wg.data(), wg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.vs_frames.p, fr.data(), (size_t)nf * sizeof(VisFrame), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.vs_tab.p, tabs.data(), ntab * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.vs_ctr.p, 0, ((size_t)nf * VIS_NCTR + VD_NCTR) * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.vs_votes.p, 0, n1 * sizeof(VisVote), h->stream));
    const uint32_t gm = cdiv(n_map, 256);
    for (uint32_t f0 = 0; f0 < n_frames; f0 += batch) {
        const uint32_t f1 = std::min(n_frames, f0 + batch), lo = off[f0], hi = off[f1];
        HIPC(h, hipMemsetAsync(E.vs_img.p, 0xFF, (size_t)(f1 - f0) * image_bytes, h->stream));
        if (hi > lo) {
            const uint32_t b0 = lo / 256u, b1 = cdiv(hi, 256);
            LAUNCH(h, h->stream, "vis_image", k_vis_image, b1 - b0, 256, scans, lo, hi, b0, (const uint32_t *)E.al_off.p, (const uint32_t *)E.al_wg.p, f0, f1, P,
                   (const double *)E.vs_tab.p, E.vs_img.p, E.vs_ctr.p);
        }
        if (n_map)
            LAUNCH(h, h->stream, "vis_vote", k_vis_vote, gm, 256, map, n_map, prm.k ? (const float *)E.nm_nrm.p : (const float *)nullptr,
                   (const VisFrame *)E.vs_frames.p, f0, f1, P, (const double *)E.vs_tab.p, (const uint32_t *)E.vs_img.p, E.vs_votes.p, E.vs_ctr.p);
    }
    if (n_map)
        LAUNCH(h, h->stream, "vis_decide", k_vis_decide, gm, 256, map, n_map, (const VisVote *)E.vs_votes.p, prm.min_through, prm.hit_weight, E.fm_flag.p,
               E.kn_mask.p, dctr);
    std::vector<unsigned long long> c((size_t)nf * VIS_NCTR + VD_NCTR);
    if ((rc = d2h(h, c.data(), E.vs_ctr.p, c.size() * sizeof(unsigned long long)))) return rc;
    erasor_visibility_result r;
    memset(&r, 0, sizeof(r));
    for (uint32_t f = 0; f < n_frames; ++f) {
        const unsigned long long *cf = &c[(size_t)f * VIS_NCTR];
        erasor_visibility_row row;
        row.n_points = off[f + 1] - off[f];
        row.n_non_finite = cf[VIS_C_NON_FINITE];
        row.n_on_axis = cf[VIS_C_AXIS];
        row.n_out_of_range = cf[VIS_C_RANGE];
        row.n_out_of_view = cf[VIS_C_VIEW];
        row.n_pixels = cf[VIS_C_PIXELS];
        row.n_map_in_view = cf[VIS_C_IN_VIEW];
        row.n_hit = cf[VIS_C_VERDICT + VIS_HIT];
        row.n_occluded = cf[VIS_C_VERDICT + VIS_OCCLUDED];
        row.n_no_return = cf[VIS_C_VERDICT + VIS_NO_RETURN];
        row.n_through = cf[VIS_C_VERDICT + VIS_THROUGH];
        row.n_grazing = cf[VIS_C_VERDICT + VIS_GRAZING];
        if (rows) rows[f] = row;
        r.n_in_view += row.n_map_in_view;
        r.n_hit += row.n_hit;
        r.n_occluded += row.n_occluded;
        r.n_no_return += row.n_no_return;
        r.n_through += row.n_through;
        r.n_grazing += row.n_grazing;
    }
    const unsigned long long *cd = &c[(size_t)nf * VIS_NCTR];
    r.n_points = n_map;
    r.n_never_in_view = n_map - cd[VD_C_SEEN];
    r.n_removed_dynamic = cd[VD_C_REMOVED_DYNAMIC];
    r.n_removed_static = cd[VD_C_REMOVED_STATIC];
    r.n_removed = r.n_removed_dynamic + r.n_removed_static;
    r.n_kept = n_map - r.n_removed;
    r.n_map_no_normal = n_no_normal;
    if (res) *res = r;
    if (votes && (rc = d2h(h, votes, E.vs_votes.p, (size_t)n_map * sizeof(VisVote)))) return rc;
    if (keep_mask && (rc = d2h(h, keep_mask, E.kn_mask.p, n_map))) return rc;
    if (kept_xyzi && r.n_kept > cap_points) return ERASOR_E_CAPACITY;
    if (kept_xyzi && r.n_kept) {
        // the kept rows, as given: the stable compaction over the keep flags (df_run's)
        if (ensure(h, E.fm_out, n1)) return ERASOR_E_NO_DEVICE;
        scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n_map, n_map, nullptr, nullptr, "vis_keep");
        LAUNCH(h, h->stream, "vis_keep", k_f_compact, gm, 256, map, n_map, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p,
               (const uint32_t *)E.fm_tops.p, E.fm_out.p);
        return d2h(h, kept_xyzi, E.fm_out.p, (size_t)r.n_kept * sizeof(float4));
    }
    return ERASOR_OK;
}

int erasor_hip_visibility_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi,
                                 size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device, const float T_lidar2body[16],
                                 const float *T_body2origin, const erasor_visibility *params, uint16_t *votes, uint8_t *keep_mask, float *kept_xyzi,
                                 size_t cap_points, erasor_visibility_row *rows, erasor_visibility_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_visibility_clouds";
    int rc = vs_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc || (rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    if ((rc = ev_input(h, map_xyzi, n_map, map_is_device, h->ev.gt, &m)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q)))
        return rc;
    return vs_run(h, who, m, (uint32_t)n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, votes, keep_mask,
                  kept_xyzi, cap_points, rows, res);
}

int erasor_hip_visibility_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                              int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, const erasor_visibility *params,
                              uint16_t *votes, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_visibility_row *rows,
                              erasor_visibility_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_visibility_map";
    int rc = vs_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return vs_run(h, who, m, n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, votes, keep_mask, kept_xyzi,
                  cap_points, rows, res);
}

// ---- carving free space: every scan's rays walked through the map's voxels (kernels: carve.hip.h) ----
// Like vs_run: the main stream, the evaluator's scratch.  The block table is built once a call (claim, slots, scan, base) and its
// counters read (the refusal of a map point out of the cell range comes before any ray is walked); then the frames go in batches of at
// most CV_BATCH in index order, one k_cv_walk over the batch's scan points and one k_cv_integrate over the voxels each; at the end
// k_cv_gather, one round trip for the counters, and the outputs asked for.

static int cv_check_args(erasor_hip_handle *h, const char *who, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                         const float *T_lidar2body, const float *T_body2origin, const erasor_carve *p) {
    if (!p) return invalid(h, who, "params is NULL");
    if (!std::isfinite(p->voxel) || !(p->voxel > 0)) return invalid(h, who, "voxel must be a finite number > 0");
    if (!std::isfinite(p->min_range) || !std::isfinite(p->max_range) || !(p->min_range >= 0) || !(p->min_range < p->max_range))
        return invalid(h, who, "0 <= min_range < max_range, both finite");
    if (p->max_range / p->voxel > (double)ERASOR_CARVE_MAX_CELLS) return invalid(h, who, "max_range / voxel must not exceed 4096");
    const float lg[6] = {p->l_init, p->l_hit, p->l_miss, p->l_min, p->l_max, p->l_thr};
    if (!all_finite(lg, 6) || !(p->l_hit >= 0) || !(p->l_miss <= 0) || !(p->l_min <= p->l_init) || !(p->l_init <= p->l_max))
        return invalid(h, who, "the log-odds must be finite, l_hit >= 0, l_miss <= 0 and l_min <= l_init <= l_max");
    if (p->stop_short > ERASOR_CARVE_MAX_STOP_SHORT) return invalid(h, who, "stop_short must be within 0 .. 64");
    if (n_frames > ERASOR_CARVE_MAX_FRAMES) return invalid(h, who, "more than 65535 frames");
    if (!offsets) return invalid(h, who, "offsets is NULL (n_frames + 1 entries)");
    if (n_frames && !T_body2origin) return invalid(h, who, "T_body2origin is NULL");
    const int rc = check_scan_offsets(h, who, scans_xyzi, n_scan_points, offsets, n_frames);
    if (rc) return rc;
    if (T_lidar2body && !all_finite(T_lidar2body, 16)) return invalid(h, who, "non-finite entry in T_lidar2body");
    if (!all_finite(T_body2origin, n_frames * 16)) return invalid(h, who, "non-finite entry in T_body2origin");
    return ERASOR_OK;
}

// a frame's forward matrix and the cell of its origin: evalmap._carve_frames, the same operations in the same order.  0: fine; 1: not
// finite; 2: the origin's cell reaches 2^28
static int cv_frame(const float *A, const float *B, double voxel, CvFrame *F) {
    VisFrame V;
    if (!vs_frame(A, B, &V)) return 1;  // (M and its inverse, as evalmap.visibility_transforms refuses them)
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) {
            const double v = ((double)A[4 * i + 0] * (double)B[0 + j] + (double)A[4 * i + 1] * (double)B[4 + j]) + (double)A[4 * i + 2] * (double)B[8 + j];
            F->m[4 * i + j] = j == 3 ? v + (double)A[4 * i + 3] : v;
        }
        const double c = floor(F->m[4 * i + 3] / voxel);
        if (!(fabs(c) < CV_CELL_LIMIT)) return 2;
        F->c0[i] = (int32_t)c;
    }
    F->pad = 0;
    return 0;
}

static int cv_run(erasor_hip_handle *h, const char *who, const float4 *map, uint32_t n_map, const float4 *scans, uint32_t n, const uint64_t *offsets,
                  uint32_t n_frames, const float *T_lidar2body, const float *T_body2origin, const erasor_carve &prm, uint16_t *votes, float *logodds,
                  uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_carve_row *rows, erasor_carve_result *res) {
    auto &E = h->ev;
    const uint32_t nf = std::max(n_frames, 1u);
    const CvParams P{prm.voxel, prm.min_range, prm.max_range, prm.l_init, prm.l_hit, prm.l_miss, prm.l_min, prm.l_max, prm.l_thr, prm.stop_short, 0u};
    // the frames: matrices and origin cells (refused before anything runs), offsets, every walk workgroup's first frame
    std::vector<CvFrame> fr(nf);
    const float *Tl = T_lidar2body ? T_lidar2body : AL_IDENTITY;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const int bad = cv_frame(T_body2origin + 16 * (size_t)f, Tl, prm.voxel, &fr[f]);
        if (bad == 1) return invalid(h, who, "non-finite transform of frame " + std::to_string(f));
        if (bad) return invalid(h, who, "the origin of frame " + std::to_string(f) + " lies in a cell whose coordinate reaches 2^28");
    }
    const uint32_t grid_all = cdiv(n, 256);
    std::vector<uint32_t> off(n_frames + 1), wg(grid_all + 1);
    for (uint32_t f = 0; f <= n_frames; ++f) off[f] = (uint32_t)offsets[f];
    for (uint32_t b = 0, f = 0; b < grid_all; ++b) {  // the largest f < n_frames with off[f] <= b * 256 (as vs_run)
        while (f + 1 < n_frames && off[f + 1] <= b * 256u) ++f;
        wg[b] = f;
    }
    wg[grid_all] = n_frames ? n_frames - 1 : 0;
    // the table: a power of two of at least twice the point count
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)n_map) cap <<= 1;
    const uint32_t capmask = (uint32_t)(cap - 1);
    const size_t n1 = (size_t)n_map + 1, nctr = (size_t)nf * CV_NCTR + CG_NCTR;
    if (ensure(h, E.al_off, (size_t)nf + 1) || ensure(h, E.al_wg, (size_t)grid_all + 1) || ensure(h, E.cv_frames, nf) || ensure(h, E.cv_tab, cap) ||
        ensure(h, E.cv_cnt, cap + 1) || ensure(h, E.cv_pl, cap + 1) || ensure(h, E.cv_tops, cap / 1024 + 4) || ensure(h, E.cv_slot, n1) ||
        ensure(h, E.cv_hm, n1) || ensure(h, E.cv_wfree, n1) || ensure(h, E.cv_whit, n1) || ensure(h, E.cv_votes, n1) || ensure(h, E.cv_L, n1) ||
        ensure(h, E.cv_lo, n1) || ensure(h, E.cv_ctr, nctr + 1) || ensure(h, E.fm_flag, n1) || ensure(h, E.fm_pl, n1) ||
        ensure(h, E.fm_tops, n_map / 1024 + 4) || ensure(h, E.kn_mask, n1))
        return ERASOR_E_NO_DEVICE;
    unsigned long long *const gctr = E.cv_ctr.p + (size_t)nf * CV_NCTR;  // the call's counters, behind the frames'
    uint32_t *const d_nvox = (uint32_t *)(E.cv_ctr.p + nctr);           // the number of map voxels (the scan's total)
    HIPC(h, hipMemcpyAsync(E.al_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.al_wg.p, wg.data(), wg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemcpyAsync(E.cv_frames.p, fr.data(), (size_t)nf * sizeof(CvFrame), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.cv_ctr.p, 0, (nctr + 1) * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.cv_tab.p, 0, cap * sizeof(CvBlock), h->stream));
    HIPC(h, hipMemsetAsync(E.cv_hm.p, 0, n1 * sizeof(uint32_t), h->stream));
    HIPC(h, hipMemsetAsync(E.cv_wfree.p, 0, n1 * sizeof(uint32_t), h->stream));
    HIPC(h, hipMemsetAsync(E.cv_whit.p, 0, n1 * sizeof(uint32_t), h->stream));
    const uint32_t gm = cdiv(n_map, 256), gc = cdiv(cap, 256);
    if (n_map) {
        LAUNCH(h, h->stream, "cv_claim", k_cv_claim, gm, 256, map, n_map, prm.voxel, E.cv_tab.p, capmask, E.cv_slot.p, gctr);
        LAUNCH(h, h->stream, "cv_slots", k_cv_slots, std::min(gc, CV_SLOTS_GRID), 256, map, prm.voxel, E.cv_tab.p, capmask, E.cv_cnt.p, gctr);
        scan_u32(h, h->stream, E.cv_cnt.p, E.cv_pl.p, E.cv_tops.p, (uint32_t)cap, (uint32_t)cap, nullptr, d_nvox, "cv_scan");
        LAUNCH(h, h->stream, "cv_base", k_cv_base, gc, 256, E.cv_tab.p, capmask, (const uint32_t *)E.cv_pl.p, (const uint32_t *)E.cv_tops.p);
        LAUNCH(h, h->stream, "cv_fill", k_cv_fill, gm, 256, E.cv_L.p, n_map, prm.l_init);
    }
    int rc;
    unsigned long long g0[CG_NCTR + 1];
    if ((rc = d2h(h, g0, gctr, sizeof(g0)))) return rc;
    if (g0[CG_C_BAD_CELL]) return invalid(h, who, std::to_string(g0[CG_C_BAD_CELL]) + " map point(s) lie in a cell whose coordinate reaches 2^28");
    const uint32_t n_voxels = (uint32_t)(g0[CG_NCTR] & 0xFFFFFFFFull);  // (the low word of the last counter: d_nvox)
    const uint32_t gv = cdiv(n_voxels, 256);
    for (uint32_t f0 = 0; f0 < n_frames; f0 += CV_BATCH) {
        const uint32_t f1 = std::min(n_frames, f0 + CV_BATCH), lo = off[f0], hi = off[f1];
        if (hi > lo) {
            const uint32_t b0 = lo / 256u, b1 = cdiv(hi, 256);
            LAUNCH(h, h->stream, "cv_walk", k_cv_walk, b1 - b0, 256, scans, lo, hi, b0, (const uint32_t *)E.al_off.p, (const uint32_t *)E.al_wg.p, f0, f1, P,
                   (const CvFrame *)E.cv_frames.p, (const CvBlock *)E.cv_tab.p, capmask, E.cv_wfree.p, E.cv_whit.p, E.cv_ctr.p);
            if (n_voxels)
                LAUNCH(h, h->stream, "cv_integrate", k_cv_integrate, gv, 256, n_voxels, f0, f1 - f0, P, E.cv_L.p, E.cv_hm.p, E.cv_wfree.p, E.cv_whit.p, E.cv_ctr.p,
                       gctr);
        }
    }
    if (n_map)
        LAUNCH(h, h->stream, "cv_gather", k_cv_gather, gm, 256, map, n_map, (const uint32_t *)E.cv_slot.p, (const CvBlock *)E.cv_tab.p, P, (const float *)E.cv_L.p,
               (const uint32_t *)E.cv_hm.p, E.cv_votes.p, E.cv_lo.p, E.fm_flag.p, E.kn_mask.p, gctr);
    std::vector<unsigned long long> c(nctr);
    if ((rc = d2h(h, c.data(), E.cv_ctr.p, c.size() * sizeof(unsigned long long)))) return rc;
    erasor_carve_result r;
    memset(&r, 0, sizeof(r));
    for (uint32_t f = 0; f < n_frames; ++f) {
        const unsigned long long *cf = &c[(size_t)f * CV_NCTR];
        erasor_carve_row row;
        row.n_points = off[f + 1] - off[f];
        row.n_non_finite = cf[CV_C_NON_FINITE];
        row.n_out_of_range = cf[CV_C_RANGE];
        row.n_rays = cf[CV_C_RAYS];
        row.n_steps = cf[CV_C_STEPS];
        row.n_end_in_map = cf[CV_C_END];
        row.n_voxels_hit = cf[CV_C_VHIT];
        row.n_voxels_free = cf[CV_C_VFREE];
        if (rows) rows[f] = row;
        r.n_scan_points += row.n_points;
        r.n_non_finite += row.n_non_finite;
        r.n_out_of_range += row.n_out_of_range;
        r.n_rays += row.n_rays;
        r.n_steps += row.n_steps;
        r.n_end_in_map += row.n_end_in_map;
        r.n_voxels_hit += row.n_voxels_hit;
        r.n_voxels_free += row.n_voxels_free;
    }
    const unsigned long long *cg = &c[(size_t)nf * CV_NCTR];
    r.n_points = n_map;
    r.n_map_non_finite = cg[CG_C_NON_FINITE];
    r.n_voxels = n_voxels;
    r.n_blocks = cg[CG_C_BLOCKS];
    r.n_voxels_touched = cg[CG_C_TOUCHED];
    r.n_removed_dynamic = cg[CG_C_REMOVED_DYNAMIC];
    r.n_removed_static = cg[CG_C_REMOVED_STATIC];
    r.n_removed = r.n_removed_dynamic + r.n_removed_static;
    r.n_kept = n_map - r.n_removed;
    if (res) *res = r;
    if (votes && (rc = d2h(h, votes, E.cv_votes.p, (size_t)n_map * sizeof(uint32_t)))) return rc;
    if (logodds && (rc = d2h(h, logodds, E.cv_lo.p, (size_t)n_map * sizeof(float)))) return rc;
    if (keep_mask && (rc = d2h(h, keep_mask, E.kn_mask.p, n_map))) return rc;
    if (kept_xyzi && r.n_kept > cap_points) return ERASOR_E_CAPACITY;
    if (kept_xyzi && r.n_kept) {
        // the kept rows, as given: the stable compaction over the keep flags (vs_run's)
        if (ensure(h, E.fm_out, n1)) return ERASOR_E_NO_DEVICE;
        scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n_map, n_map, nullptr, nullptr, "cv_keep");
        LAUNCH(h, h->stream, "cv_keep", k_f_compact, gm, 256, map, n_map, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p,
               (const uint32_t *)E.fm_tops.p, E.fm_out.p);
        return d2h(h, kept_xyzi, E.fm_out.p, (size_t)r.n_kept * sizeof(float4));
    }
    return ERASOR_OK;
}

int erasor_hip_carve_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi, size_t n_scan_points,
                            const uint64_t *offsets, size_t n_frames, int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                            const erasor_carve *params, uint16_t *votes, float *logodds, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points,
                            erasor_carve_row *rows, erasor_carve_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_carve_clouds";
    int rc = cv_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc || (rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    if ((rc = ev_input(h, map_xyzi, n_map, map_is_device, h->ev.gt, &m)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q)))
        return rc;
    return cv_run(h, who, m, (uint32_t)n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, votes, logodds,
                  keep_mask, kept_xyzi, cap_points, rows, res);
}

int erasor_hip_carve_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device,
                         const float T_lidar2body[16], const float *T_body2origin, const erasor_carve *params, uint16_t *votes, float *logodds,
                         uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_carve_row *rows, erasor_carve_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_carve_map";
    int rc = cv_check_args(h, who, scans_xyzi, n_scan_points, offsets, n_frames, T_lidar2body, T_body2origin, params);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr, *q = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map)) || (rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return cv_run(h, who, m, n_map, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, T_lidar2body, T_body2origin, *params, votes, logodds, keep_mask,
                  kept_xyzi, cap_points, rows, res);
}

// ---- the ground: R-GPF on every polar patch of every scan, and the map's ground points by vote (kernels: ground.hip.h) ----
// Like cv_run: the main stream, the evaluator's scratch, the sort in histogram bank 2.  The frames go in batches in index order (the
// scans: as many as keep a batch's patch table within GR_MAX_PATCHES; the map form: also within the work budget); per batch one
// k_gr_key, the counts' scan, the keys' stable radix sort and the three k_gr_fit launches; the map form gathers in front and votes
// behind.  Round trips: a batch's patch rows where they are asked for, and at the end the counters and the outputs asked for.

static int gr_check_params(erasor_hip_handle *h, const char *who, const erasor_ground *p, size_t n_frames) {
    if (!p) return invalid(h, who, "params is NULL");
    if (p->n_rings < 1 || p->n_rings > ERASOR_GROUND_MAX_RINGS) return invalid(h, who, "n_rings must be within 1 .. 64");
    if (p->n_sectors % 8 || p->n_sectors < 8 || p->n_sectors > ERASOR_GROUND_MAX_SECTORS)
        return invalid(h, who, "n_sectors must be a multiple of 8 within 8 .. 512");
    const uint32_t nc = p->n_sectors / 8 - 1;
    if (!p->ring_edge || (nc && !p->col_tan)) return invalid(h, who, "ring_edge or col_tan is NULL");
    for (uint32_t j = 0; j <= p->n_rings; ++j)
        if (!std::isfinite(p->ring_edge[j]) || (j ? !(p->ring_edge[j] > p->ring_edge[j - 1]) : !(p->ring_edge[0] >= 0)))
            return invalid(h, who, "ring_edge must be finite, strictly increasing and start at >= 0");
    for (uint32_t j = 0; j < nc; ++j)
        if (!(p->col_tan[j] > 0 && p->col_tan[j] < 1) || (j && !(p->col_tan[j] > p->col_tan[j - 1])))
            return invalid(h, who, "col_tan must be strictly increasing within (0, 1)");
    for (uint32_t j = 0; j < p->n_rings; ++j)
        if ((p->elevation && std::isnan(p->elevation[j])) || (p->flatness && std::isnan(p->flatness[j])))
            return invalid(h, who, "elevation and flatness must not hold a NaN");
    if (p->num_lpr < 1 || p->num_lpr > ERASOR_GROUND_MAX_LPR) return invalid(h, who, "num_lpr must be within 1 .. 64");
    if (p->iters < 1 || p->iters > ERASOR_GROUND_MAX_ITERS) return invalid(h, who, "iters must be within 1 .. 16");
    if (p->min_points < 3) return invalid(h, who, "min_points must be at least 3");
    if (!std::isfinite(p->th_seeds) || !std::isfinite(p->th_dist) || !std::isfinite(p->min_z) || !std::isfinite(p->uprightness))
        return invalid(h, who, "th_seeds, th_dist, min_z and uprightness must be finite");
    if (!std::isfinite(p->ratio)) return invalid(h, who, "ratio must be finite");
    if (n_frames > ERASOR_GROUND_MAX_FRAMES) return invalid(h, who, "more than 65535 frames");
    return ERASOR_OK;
}

// the tables on the device (ring_edge, col_tan, elevation, flatness) and the kernels' parameters
static int gr_put_tables(erasor_hip_handle *h, const erasor_ground &prm, GrParams *P) {
    auto &E = h->ev;
    const uint32_t R = prm.n_rings, S = prm.n_sectors, M = S / 8;
    *P = GrParams{R, S, M, prm.num_lpr, prm.iters, prm.min_points, prm.th_seeds, prm.th_dist, prm.min_z, prm.uprightness};
    std::vector<double> tabs;
    tabs.insert(tabs.end(), prm.ring_edge, prm.ring_edge + R + 1);
    if (M > 1) tabs.insert(tabs.end(), prm.col_tan, prm.col_tan + (M - 1));
    for (uint32_t j = 0; j < R; ++j) tabs.push_back(prm.elevation ? prm.elevation[j] : (double)INFINITY);
    for (uint32_t j = 0; j < R; ++j) tabs.push_back(prm.flatness ? prm.flatness[j] : 0.0);
    if (ensure(h, E.gr_tab, tabs.size())) return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemcpyAsync(E.gr_tab.p, tabs.data(), tabs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));  // (tabs leaves scope)
    return ERASOR_OK;
}

// One batch: nb frames with the device offsets d_off[0 .. nb] (absolute indices into pts), their points lo + k, k < n (n = *n_dev when
// given, n_ub its bound).  codes: by absolute index; patches: the batch's nb R S rows, zeroed, or NULL; ctr: the batch's first frame's.
static int gr_segment(erasor_hip_handle *h, const float4 *pts, uint32_t lo, uint32_t n_ub, const uint32_t *n_dev, const uint32_t *d_off, uint32_t nb,
                      const GrParams &P, uint8_t *codes, erasor_ground_patch *patches, unsigned long long *ctr) {
    auto &E = h->ev;
    if (!n_ub || !nb) return ERASOR_OK;
    const uint32_t np = nb * P.R * P.S;  // (<= GR_MAX_PATCHES)
    const size_t n1 = (size_t)n_ub + 1;
    if (ensure(h, E.gr_key, n1) || ensure(h, E.gr_ka, n1) || ensure(h, E.gr_kb, n1) || ensure(h, E.gr_va, n1) || ensure(h, E.gr_vb, n1) ||
        ensure(h, E.gr_cnt, (size_t)np + 2) || ensure(h, E.gr_pl, (size_t)np + 2) || ensure(h, E.gr_tops, np / 1024 + 4))
        return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemsetAsync(E.gr_cnt.p, 0, ((size_t)np + 1) * sizeof(uint32_t), h->stream));
    LAUNCH(h, h->stream, "gr_key", k_gr_key, cdiv(n_ub, 256), 256, pts, lo, n_ub, n_dev, d_off, nb, P, (const double *)E.gr_tab.p, E.gr_key.p, E.gr_cnt.p, codes,
           ctr);
    scan_u32(h, h->stream, E.gr_cnt.p, E.gr_pl.p, E.gr_tops.p, np + 1, np + 1, nullptr, nullptr, "gr_scan");
    const uint32_t *skeys = nullptr, *sperm = nullptr;
    const int rc = radix_sort(h, h->stream, 2, E.gr_key.p, n_ub, n_dev, key_bits(np + 1), E.gr_ka.p, E.gr_kb.p, E.gr_va.p, E.gr_vb.p, &skeys, &sperm, "gr_sort");
    if (rc) return rc;
    // The three size classes, each over the whole table.  One launch per class, not one launch that dispatches by class: a launch has one
    // workgroup size, one static LDS allotment and one register budget, and the classes differ in all three (64 lanes, 768 B and 146
    // VGPRs for the wavefront class; 256 lanes with 21 KiB or 57 KiB and about 100 VGPRs for the other two), so a single kernel would
    // give every patch of 20 points the large class's 57 KiB and two workgroups per CU.  What a single launch would cost or save was
    // not measured (EXPERIMENTS "Ground").
    LAUNCH(h, h->stream, "gr_fit_wave", (k_gr_fit<64, GR_WAVE_POINTS, 0>), std::min(np, 16384u), 64, pts, lo, sperm, (const uint32_t *)E.gr_cnt.p,
           (const uint32_t *)E.gr_pl.p, (const uint32_t *)E.gr_tops.p, np, P, (const double *)E.gr_tab.p, codes, patches, ctr);
    LAUNCH(h, h->stream, "gr_fit_small", (k_gr_fit<256, GR_SMALL_POINTS, 1>), std::min(np, 4096u), 256, pts, lo, sperm, (const uint32_t *)E.gr_cnt.p,
           (const uint32_t *)E.gr_pl.p, (const uint32_t *)E.gr_tops.p, np, P, (const double *)E.gr_tab.p, codes, patches, ctr);
    LAUNCH(h, h->stream, "gr_fit_large", (k_gr_fit<256, GR_LDS_POINTS, 2>), std::min(np, 1024u), 256, pts, lo, sperm, (const uint32_t *)E.gr_cnt.p,
           (const uint32_t *)E.gr_pl.p, (const uint32_t *)E.gr_tops.p, np, P, (const double *)E.gr_tab.p, codes, patches, ctr);
    return ERASOR_OK;
}

// a frame's row from its counters (n_points: the scan's, or the gathered count in the map form), added into the result
static erasor_ground_row gr_row(const unsigned long long *cf, uint64_t n_points, uint64_t n_gathered, erasor_ground_result *r) {
    erasor_ground_row row;
    row.n_points = n_points;
    row.n_non_finite = cf[GR_C_NON_FINITE];
    row.n_out_of_range = cf[GR_C_RANGE];
    row.n_judged = cf[GR_C_JUDGED];
    row.n_ground = cf[GR_C_GROUND];
    row.n_ground_dynamic = cf[GR_C_GROUND_DYNAMIC];
    row.n_patches = cf[GR_C_PATCHES];
    row.n_sparse = cf[GR_C_STATUS + (uint32_t)ERASOR_GROUND_SPARSE];
    row.n_degenerate = cf[GR_C_STATUS + (uint32_t)ERASOR_GROUND_DEGENERATE];
    row.n_rejected_upright = cf[GR_C_STATUS + (uint32_t)ERASOR_GROUND_REJECTED_UPRIGHT];
    row.n_rejected_elevation = cf[GR_C_STATUS + (uint32_t)ERASOR_GROUND_REJECTED_ELEVATION];
    row.n_gathered = n_gathered;
    r->n_points += row.n_points;
    r->n_non_finite += row.n_non_finite;
    r->n_out_of_range += row.n_out_of_range;
    r->n_judged += row.n_judged;
    r->n_ground += row.n_ground;
    r->n_ground_dynamic += row.n_ground_dynamic;
    r->n_patches += row.n_patches;
    r->n_sparse += row.n_sparse;
    r->n_degenerate += row.n_degenerate;
    r->n_rejected_upright += row.n_rejected_upright;
    r->n_rejected_elevation += row.n_rejected_elevation;
    return row;
}

static int gr_run_scans(erasor_hip_handle *h, const float4 *scans, uint32_t n, const uint64_t *offsets, uint32_t n_frames, const erasor_ground &prm,
                        uint8_t *codes, erasor_ground_row *rows, erasor_ground_patch *patches, erasor_ground_result *res) {
    auto &E = h->ev;
    GrParams P;
    int rc;
    if ((rc = gr_put_tables(h, prm, &P))) return rc;
    const uint32_t nf = std::max(n_frames, 1u), RS = P.R * P.S, nbmax = std::max(1u, GR_MAX_PATCHES / RS);
    std::vector<uint32_t> off(n_frames + 1);
    for (uint32_t f = 0; f <= n_frames; ++f) off[f] = (uint32_t)offsets[f];
    if (ensure(h, E.al_off, (size_t)nf + 1) || ensure(h, E.gr_codes, (size_t)n + 1) || ensure(h, E.gr_ctr, (size_t)nf * GR_NCTR) ||
        (patches && ensure(h, E.gr_patch, (size_t)std::min(nbmax, nf) * RS)))
        return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemcpyAsync(E.al_off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.gr_ctr.p, 0, (size_t)nf * GR_NCTR * sizeof(unsigned long long), h->stream));
    for (uint32_t f0 = 0; f0 < n_frames; f0 += nbmax) {
        const uint32_t f1 = std::min(n_frames, f0 + nbmax), nb = f1 - f0, lo = off[f0], hi = off[f1];
        erasor_ground_patch *const hp = patches ? patches + (size_t)f0 * RS : nullptr;
        if (hi == lo) {
            if (hp) memset(hp, 0, (size_t)nb * RS * sizeof(erasor_ground_patch));
            continue;
        }
        if (hp) HIPC(h, hipMemsetAsync(E.gr_patch.p, 0, (size_t)nb * RS * sizeof(erasor_ground_patch), h->stream));
        if ((rc = gr_segment(h, scans, lo, hi - lo, nullptr, (const uint32_t *)E.al_off.p + f0, nb, P, E.gr_codes.p, hp ? E.gr_patch.p : nullptr,
                             E.gr_ctr.p + (size_t)f0 * GR_NCTR)))
            return rc;
        if (hp && (rc = d2h(h, hp, E.gr_patch.p, (size_t)nb * RS * sizeof(erasor_ground_patch)))) return rc;
    }
    std::vector<unsigned long long> c((size_t)nf * GR_NCTR);
    if ((rc = d2h(h, c.data(), E.gr_ctr.p, c.size() * sizeof(unsigned long long)))) return rc;
    erasor_ground_result r;
    memset(&r, 0, sizeof(r));
    r.n_frames = n_frames;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const erasor_ground_row row = gr_row(&c[(size_t)f * GR_NCTR], off[f + 1] - off[f], 0, &r);
        if (rows) rows[f] = row;
    }
    if (res) *res = r;
    if (codes && n) return d2h(h, codes, E.gr_codes.p, n);
    return ERASOR_OK;
}

static int gr_run_votes(erasor_hip_handle *h, const char *who, const float4 *map, uint32_t n_map, const float *T_lidar2body, const float *T_body2origin,
                        uint32_t n_frames, const erasor_ground &prm, uint16_t *votes, uint8_t *ground_mask, float *kept_xyzi, size_t cap_points,
                        erasor_ground_row *rows, erasor_ground_result *res) {
    auto &E = h->ev;
    const uint32_t nf = std::max(n_frames, 1u);
    std::vector<VisFrame> fr(nf);
    const float *Tl = T_lidar2body ? T_lidar2body : AL_IDENTITY;
    for (uint32_t f = 0; f < n_frames; ++f)
        if (!vs_frame(T_body2origin + 16 * (size_t)f, Tl, &fr[f])) return invalid(h, who, "non-finite transform of frame " + std::to_string(f));
    GrParams P;
    int rc;
    if ((rc = gr_put_tables(h, prm, &P))) return rc;
    // the batches: whole frames of n_map * 16 bytes each within the budget, at least one; the patch table and the pairs' index bound them too
    const uint32_t RS = P.R * P.S;
    const uint64_t budget = prm.work_budget_bytes ? prm.work_budget_bytes : ERASOR_GROUND_WORK_BUDGET;
    uint64_t nbmax = n_map ? budget / ((uint64_t)n_map * sizeof(float4)) : nf;
    nbmax = std::min<uint64_t>(nbmax, GR_MAX_PATCHES / RS);
    if (n_map) nbmax = std::min<uint64_t>(nbmax, (1ull << 30) / n_map);
    nbmax = std::max<uint64_t>(1, std::min<uint64_t>(nbmax, nf));
    const size_t n1 = (size_t)n_map + 1, npair = (size_t)nbmax * n_map, nctr = (size_t)nf * GR_NCTR + GD_NCTR;
    if (ensure(h, E.gr_frames, nf) || ensure(h, E.gr_flag, npair + 1) || ensure(h, E.gr_fpl, npair + 1) || ensure(h, E.gr_ftops, npair / 1024 + 4) ||
        ensure(h, E.gr_cloud, npair + 1) || ensure(h, E.gr_midx, npair + 1) || ensure(h, E.gr_off, (size_t)nbmax + 2) || ensure(h, E.gr_votes, n1) ||
        ensure(h, E.gr_codes, npair + 1) || ensure(h, E.gr_ctr, nctr) || ensure(h, E.fm_flag, n1) || ensure(h, E.fm_pl, n1) ||
        ensure(h, E.fm_tops, n_map / 1024 + 4) || ensure(h, E.kn_mask, n1))
        return ERASOR_E_NO_DEVICE;
    unsigned long long *const dctr = E.gr_ctr.p + (size_t)nf * GR_NCTR;  // the decision's counters, behind the frames'
    HIPC(h, hipMemcpyAsync(E.gr_frames.p, fr.data(), (size_t)nf * sizeof(VisFrame), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.gr_ctr.p, 0, nctr * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.gr_votes.p, 0, n1 * sizeof(uint32_t), h->stream));
    const uint32_t gm = cdiv(n_map, 256);
    for (uint32_t f0 = 0; n_map && f0 < n_frames; f0 += (uint32_t)nbmax) {
        const uint32_t f1 = (uint32_t)std::min<uint64_t>(n_frames, f0 + nbmax), nb = f1 - f0, tot = nb * n_map;
        unsigned long long *const cf = E.gr_ctr.p + (size_t)f0 * GR_NCTR;
        uint32_t *const d_n = E.gr_off.p + nb;  // the batch's gathered total: the last offset
        LAUNCH(h, h->stream, "gr_gather", k_gr_gather_flag, dim3(gm, nb), 256, map, n_map, (const VisFrame *)E.gr_frames.p + f0, P, (const double *)E.gr_tab.p,
               E.gr_flag.p);
        scan_u32(h, h->stream, E.gr_flag.p, E.gr_fpl.p, E.gr_ftops.p, tot, tot, nullptr, d_n, "gr_gather");
        LAUNCH(h, h->stream, "gr_gather", k_gr_gather_put, dim3(gm, nb), 256, map, n_map, (const VisFrame *)E.gr_frames.p + f0, (const uint32_t *)E.gr_flag.p, (const uint32_t *)E.gr_fpl.p, (const uint32_t *)E.gr_ftops.p, E.gr_cloud.p, E.gr_midx.p, E.gr_off.p);
        LAUNCH(h, h->stream, "gr_gather", k_gr_count_frames, cdiv(nb, 256), 256, (const uint32_t *)E.gr_off.p, nb, cf);
        if ((rc = gr_segment(h, E.gr_cloud.p, 0, tot, d_n, (const uint32_t *)E.gr_off.p, nb, P, E.gr_codes.p, nullptr, cf))) return rc;
        LAUNCH(h, h->stream, "gr_vote", k_gr_vote, cdiv(tot, 256), 256, (const uint8_t *)E.gr_codes.p, (const uint32_t *)E.gr_midx.p, (const uint32_t *)d_n,
               E.gr_votes.p);
    }
    if (n_map)
        LAUNCH(h, h->stream, "gr_decide", k_gr_decide, gm, 256, map, n_map, (const uint32_t *)E.gr_votes.p, prm.min_votes, prm.ratio, prm.keep, E.fm_flag.p,
               E.kn_mask.p, dctr);
    std::vector<unsigned long long> c(nctr);
    if ((rc = d2h(h, c.data(), E.gr_ctr.p, c.size() * sizeof(unsigned long long)))) return rc;
    erasor_ground_result r;
    memset(&r, 0, sizeof(r));
    r.n_frames = n_frames;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const unsigned long long *cf = &c[(size_t)f * GR_NCTR];
        const erasor_ground_row row = gr_row(cf, cf[GR_C_POINTS], cf[GR_C_POINTS], &r);
        if (rows) rows[f] = row;
    }
    const unsigned long long *cd = &c[(size_t)nf * GR_NCTR];
    r.n_map_points = n_map;
    r.n_map_ground_dynamic = cd[GD_C_GROUND_DYNAMIC];
    r.n_map_ground_static = cd[GD_C_GROUND_STATIC];
    r.n_map_ground = r.n_map_ground_dynamic + r.n_map_ground_static;
    r.n_map_unseen = cd[GD_C_UNSEEN];
    r.n_kept = prm.keep ? r.n_map_ground : n_map - r.n_map_ground;
    if (res) *res = r;
    if (votes && n_map && (rc = d2h(h, votes, E.gr_votes.p, (size_t)n_map * sizeof(uint32_t)))) return rc;
    if (ground_mask && n_map && (rc = d2h(h, ground_mask, E.kn_mask.p, n_map))) return rc;
    if (kept_xyzi && r.n_kept > cap_points) return ERASOR_E_CAPACITY;
    if (kept_xyzi && r.n_kept) {
        // the rows asked for, as given: the stable compaction over the flags (cv_run's)
        if (ensure(h, E.fm_out, n1)) return ERASOR_E_NO_DEVICE;
        scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, n_map, n_map, nullptr, nullptr, "gr_keep");
        LAUNCH(h, h->stream, "gr_keep", k_f_compact, gm, 256, map, n_map, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p,
               (const uint32_t *)E.fm_tops.p, E.fm_out.p);
        return d2h(h, kept_xyzi, E.fm_out.p, (size_t)r.n_kept * sizeof(float4));
    }
    return ERASOR_OK;
}

int erasor_hip_ground_scans(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                            int scans_are_device, const erasor_ground *params, uint8_t *codes, erasor_ground_row *rows, erasor_ground_patch *patches,
                            erasor_ground_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_ground_scans";
    int rc = gr_check_params(h, who, params, n_frames);
    if (rc) return rc;
    if (!offsets) return invalid(h, who, "offsets is NULL (n_frames + 1 entries)");
    if ((rc = check_scan_offsets(h, who, scans_xyzi, n_scan_points, offsets, n_frames))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *q = nullptr;
    if ((rc = ev_input(h, scans_xyzi, n_scan_points, scans_are_device, h->ev.est, &q))) return rc;
    return gr_run_scans(h, q, (uint32_t)n_scan_points, offsets, (uint32_t)n_frames, *params, codes, rows, patches, res);
}

static int gr_check_votes_args(erasor_hip_handle *h, const char *who, const float *T_lidar2body, const float *T_body2origin, size_t n_frames,
                               const erasor_ground *params) {
    const int rc = gr_check_params(h, who, params, n_frames);
    if (rc) return rc;
    if (n_frames && !T_body2origin) return invalid(h, who, "T_body2origin is NULL");
    if (T_lidar2body && !all_finite(T_lidar2body, 16)) return invalid(h, who, "non-finite entry in T_lidar2body");
    if (!all_finite(T_body2origin, n_frames * 16)) return invalid(h, who, "non-finite entry in T_body2origin");
    return ERASOR_OK;
}

int erasor_hip_ground_votes_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const float T_lidar2body[16],
                                   const float *T_body2origin, size_t n_frames, const erasor_ground *params, uint16_t *votes, uint8_t *ground_mask,
                                   float *kept_xyzi, size_t cap_points, erasor_ground_row *rows, erasor_ground_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_ground_votes_clouds";
    int rc = gr_check_votes_args(h, who, T_lidar2body, T_body2origin, n_frames, params);
    if (rc || (rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr;
    if ((rc = ev_input(h, map_xyzi, n_map, map_is_device, h->ev.gt, &m))) return rc;
    return gr_run_votes(h, who, m, (uint32_t)n_map, T_lidar2body, T_body2origin, (uint32_t)n_frames, *params, votes, ground_mask, kept_xyzi, cap_points, rows,
                        res);
}

int erasor_hip_ground_votes_map(erasor_hip_handle *h, const float T_lidar2body[16], const float *T_body2origin, size_t n_frames,
                                const erasor_ground *params, uint16_t *votes, uint8_t *ground_mask, float *kept_xyzi, size_t cap_points,
                                erasor_ground_row *rows, erasor_ground_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_ground_votes_map";
    int rc = gr_check_votes_args(h, who, T_lidar2body, T_body2origin, n_frames, params);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *m = nullptr;
    uint32_t n_map = 0;
    if ((rc = map_on_device(h, who, h->ev.map, &m, &n_map))) return rc;
    return gr_run_votes(h, who, m, n_map, T_lidar2body, T_body2origin, (uint32_t)n_frames, *params, votes, ground_mask, kept_xyzi, cap_points, rows, res);
}

// ---- label_map (fill_removert_intensity.cpp:24-59, compare_map.cpp:77-110) and calc_complement (compare_complement.cpp:43-75): the
// overlap report's tree searched in FLANN's float32 metric (kernels: nearest.hip.h).  Like ov_run: the main stream, the evaluator's
// scratch, the tree's sort in bank 2.

int erasor_hip_label_map(erasor_hip_handle *h, const void *src_xyzi, size_t n_src, int src_is_device, const void *medium_xyzi, size_t n_medium,
                         int medium_is_device, double leaf, float *dst_xyzi, size_t cap_points, erasor_label_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    if (!res) {
        h->err = "erasor_hip_label_map: res is NULL";
        return ERASOR_E_INVALID;
    }
    if (!(leaf > 0) || !std::isfinite(leaf)) {
        h->err = "erasor_hip_label_map: leaf must be a finite number > 0";
        return ERASOR_E_INVALID;
    }
    int rc = check_cloud(h, "erasor_hip_label_map", BAD_CLOUD, src_xyzi, n_src);
    if (rc || (rc = check_cloud(h, "erasor_hip_label_map", BAD_CLOUD, medium_xyzi, n_medium))) return rc;
    if (n_src && !n_medium) {
        h->err = "erasor_hip_label_map: empty medium (no labelled point to take a label from)";
        return ERASOR_E_INVALID;
    }
    erasor_label_result r;
    memset(&r, 0, sizeof(r));
    r.n_src = n_src;
    if (!n_src) {
        *res = r;
        return ERASOR_OK;
    }
    HIPC(h, hipSetDevice(h->device));
    auto &E = h->ev;
    const float4 *s = nullptr, *m = nullptr;
    if ((rc = ev_input(h, src_xyzi, n_src, src_is_device, E.est, &s)) || (rc = ev_input(h, medium_xyzi, n_medium, medium_is_device, E.gt, &m)))
        return rc;
    // 1. pcl::VoxelGrid at leaf (the centroids; their w is not read).  Index overflow: the input itself, as PCL returns it
    uint32_t nq = 0;
    bool passthrough = false;
    if ((rc = ev_voxelize(h, s, (uint32_t)n_src, leaf, E.est, &nq, &passthrough))) return rc;
    // 2. every centroid takes the intensity of its nearest medium point (KdTreeFLANN, K = 1)
    const uint32_t nm = (uint32_t)n_medium;
    if (ensure(h, E.fm_ctr, FM_NCTR) || ensure(h, E.fm_out, (size_t)nq + 1)) return ERASOR_E_NO_DEVICE;
    NnTree T;
    if ((rc = nn_build(h, m, nm, "erasor_hip_label_map", "medium", "medium point(s)", &T))) return rc;
    HIPC(h, hipMemsetAsync(E.fm_ctr.p, 0, FM_NCTR * sizeof(unsigned long long), h->stream));
    if (nq)
        LAUNCH(h, h->stream, "lm_query", k_lm_query, cdiv(nq, NN_QBLOCK), NN_QBLOCK, (const float4 *)E.est.p, nq, T, E.fm_out.p, E.fm_ctr.p);
    unsigned long long c[FM_NCTR];
    HIPC(h, hipMemcpyAsync(c, E.fm_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (c[FM_NON_FINITE]) {
        h->err = "erasor_hip_label_map: non-finite coordinate (NaN / Inf) in " + std::to_string(c[FM_NON_FINITE]) + " centroid(s)";
        return ERASOR_E_INVALID;
    }
    r.n_out = nq;
    r.n_tied = c[FM_TIED];
    r.passthrough = passthrough ? 1u : 0u;
    *res = r;
    if (!dst_xyzi) return ERASOR_OK;
    if (nq > cap_points) return ERASOR_E_CAPACITY;
    return d2h(h, dst_xyzi, E.fm_out.p, (size_t)nq * sizeof(float4));
}

int erasor_hip_static_complement(erasor_hip_handle *h, const void *est_xyzi, size_t n_est, int est_is_device, const void *gt_xyzi, size_t n_gt,
                                 int gt_is_device, float *dst_xyzi, size_t cap_points, erasor_complement_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    if (!res) {
        h->err = "erasor_hip_static_complement: res is NULL";
        return ERASOR_E_INVALID;
    }
    int rc = check_cloud(h, "erasor_hip_static_complement", BAD_CLOUD, est_xyzi, n_est);
    if (rc || (rc = check_cloud(h, "erasor_hip_static_complement", BAD_CLOUD, gt_xyzi, n_gt))) return rc;
    erasor_complement_result r;
    memset(&r, 0, sizeof(r));
    r.n_gt = n_gt;
    if (!n_gt) {
        *res = r;
        return ERASOR_OK;
    }
    HIPC(h, hipSetDevice(h->device));
    auto &E = h->ev;
    const float4 *e = nullptr, *g = nullptr;
    if ((rc = ev_input(h, est_xyzi, n_est, est_is_device, E.est, &e)) || (rc = ev_input(h, gt_xyzi, n_gt, gt_is_device, E.gt, &g))) return rc;
    const uint32_t ne = (uint32_t)n_est, ng = (uint32_t)n_gt;
    if (ensure(h, E.fm_ctr, FM_NCTR) || ensure(h, E.fm_flag, (size_t)ng + 1) || ensure(h, E.fm_pl, (size_t)ng + 1) ||
        ensure(h, E.fm_tops, ng / 1024 + 4) || ensure(h, E.fm_out, (size_t)ng + 1))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    if ((rc = nn_build(h, e, ne, "erasor_hip_static_complement", "estimate", "estimated point(s)", &T))) return rc;
    HIPC(h, hipMemsetAsync(E.fm_ctr.p, 0, FM_NCTR * sizeof(unsigned long long), h->stream));
    // the lost flags, then the lost points in ground-truth order: an exclusive scan of the flags and a scatter (no atomic decides a slot)
    LAUNCH(h, h->stream, "cp_query", k_cp_query, cdiv(ng, NN_QBLOCK), NN_QBLOCK, g, ng, T, 0.03, E.fm_flag.p, E.fm_ctr.p);
    if (dst_xyzi) {
        scan_u32(h, h->stream, E.fm_flag.p, E.fm_pl.p, E.fm_tops.p, ng, ng, nullptr, nullptr, "cp_compact");
        LAUNCH(h, h->stream, "cp_compact", k_f_compact, cdiv(ng, 256), 256, g, ng, (const uint32_t *)E.fm_flag.p, (const uint32_t *)E.fm_pl.p,
               (const uint32_t *)E.fm_tops.p, E.fm_out.p);
    }
    unsigned long long c[FM_NCTR];
    HIPC(h, hipMemcpyAsync(c, E.fm_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (c[FM_NON_FINITE]) {
        h->err = "erasor_hip_static_complement: non-finite coordinate (NaN / Inf) in " + std::to_string(c[FM_NON_FINITE]) + " ground-truth point(s)";
        return ERASOR_E_INVALID;
    }
    r.n_gt_static = c[FM_GT_STATIC];
    r.n_lost = c[FM_LOST];
    r.n_label_out_of_range = c[FM_LABEL_OOR];
    *res = r;
    if (!dst_xyzi) return ERASOR_OK;
    if (r.n_lost > cap_points) return ERASOR_E_CAPACITY;
    return d2h(h, dst_xyzi, E.fm_out.p, (size_t)r.n_lost * sizeof(float4));
}

// ---- PR / RR by class and by dynamic instance (kernels: evaluate.hip.h, k_ev_*_keys onwards) ----
// ev_run in its by-key mode, then the rows on the main stream in the evaluator's scratch: the class rows by a flag per non-empty key, its
// exclusive scan and a scatter (key order, no sort); the instance rows by a radix sort of the dynamic points' records by label (histogram
// bank 2, like the overlap report's tree: the query chains of nodes announced ahead keep bank 0), run heads, their scan, and one atomic
// per row and counter of a wavefront.
static void bc_fill(const std::vector<uint32_t> &rows, size_t n, bool instances, erasor_eval_class_row *out) {
    for (size_t r = 0; r < n; ++r) {
        const uint32_t *v = &rows[r * EV_ROW];
        erasor_eval_class_row &o = out[r];
        o.key = v[0];
        const uint32_t sem = v[0] & 0xFFFFu;
        o.is_dynamic = (instances || (v[0] < EV_KEY_OOR && sem >= 252u && sem <= 259u)) ? 1u : 0u;
        o.n_gt = v[1 + EV_K_GT];
        o.n_within = v[1 + EV_K_WITHIN];
        o.n_preserved = v[1 + EV_K_KEPT];
        o.n_tied = v[1 + EV_K_TIED];
        o.n_est = v[1 + EV_K_EST];
    }
}

static int bc_run(erasor_hip_handle *h, const float4 *gt, uint32_t n_gt, const float4 *est, uint32_t n_est, double voxelsize,
                  erasor_eval_class_row *classes, size_t cap_classes, size_t *n_classes, erasor_eval_class_row *instances, size_t cap_instances,
                  size_t *n_instances, erasor_eval_result *res) {
    uint32_t n_rec = 0;
    int rc = ev_run(h, gt, n_gt, est, n_est, voxelsize, nullptr, res, &n_rec);
    if (rc) return rc;
    auto &E = h->ev;
    const size_t n_scan = std::max<size_t>(EV_NKEYS, n_rec) + 1;
    if (ensure(h, E.bc_flag, n_scan) || ensure(h, E.bc_pl, n_scan) || ensure(h, E.bc_tops, n_scan / 1024 + 4) ||
        ensure(h, E.bc_crows, (size_t)EV_NKEYS * EV_ROW))
        return ERASOR_E_NO_DEVICE;
    LAUNCH(h, h->stream, "ev_rows", k_ev_class_flags, cdiv(EV_NKEYS, 256), 256, (const uint32_t *)E.bc_tab.p, E.bc_flag.p);
    scan_u32(h, h->stream, E.bc_flag.p, E.bc_pl.p, E.bc_tops.p, EV_NKEYS, EV_NKEYS, nullptr, E.bc_cur.p + 1, "ev_rows");
    LAUNCH(h, h->stream, "ev_rows", k_ev_class_rows, cdiv(EV_NKEYS, 256), 256, (const uint32_t *)E.bc_tab.p, (const uint32_t *)E.bc_flag.p,
           (const uint32_t *)E.bc_pl.p, (const uint32_t *)E.bc_tops.p, E.bc_crows.p);
    uint32_t n_cls = 0;
    HIPC(h, hipMemcpyAsync(&n_cls, E.bc_cur.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    uint32_t n_inst = 0;
    if (n_rec) {
        const size_t n1 = (size_t)n_rec + 1;
        if (ensure(h, E.nn_ka, n1) || ensure(h, E.nn_kb, n1) || ensure(h, E.nn_va, n1) || ensure(h, E.nn_vb, n1) || ensure(h, E.bc_irows, n1 * EV_ROW))
            return ERASOR_E_NO_DEVICE;
        const uint32_t *skeys = nullptr, *sperm = nullptr;
        if (radix_sort(h, h->stream, 2, E.bc_ikey.p, n_rec, nullptr, 32, E.nn_ka.p, E.nn_kb.p, E.nn_va.p, E.nn_vb.p, &skeys, &sperm, "ev_rows"))
            return ERASOR_E_NO_DEVICE;
        LAUNCH(h, h->stream, "ev_rows", k_ev_run_heads, cdiv(n_rec, 256), 256, skeys, n_rec, E.bc_flag.p);
        scan_u32(h, h->stream, E.bc_flag.p, E.bc_pl.p, E.bc_tops.p, n_rec, n_rec, nullptr, E.bc_cur.p + 2, "ev_rows");
        HIPC(h, hipMemsetAsync(E.bc_irows.p, 0, (size_t)n_rec * EV_ROW * sizeof(uint32_t), h->stream));
        LAUNCH(h, h->stream, "ev_rows", k_ev_inst_rows, cdiv(n_rec, 256), 256, skeys, sperm, (const uint32_t *)E.bc_ival.p, (const uint32_t *)E.bc_flag.p,
               (const uint32_t *)E.bc_pl.p, (const uint32_t *)E.bc_tops.p, n_rec, E.bc_irows.p);
        HIPC(h, hipMemcpyAsync(&n_inst, E.bc_cur.p + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPC(h, hipStreamSynchronize(h->stream));
    *n_classes = n_cls;
    *n_instances = n_inst;
    if (n_cls > cap_classes || n_inst > cap_instances) return ERASOR_E_CAPACITY;  // (the counts and res are written: size and call again)
    std::vector<uint32_t> rows((size_t)std::max(n_cls, n_inst) * EV_ROW);
    if ((rc = d2h(h, rows.data(), E.bc_crows.p, (size_t)n_cls * EV_ROW * sizeof(uint32_t)))) return rc;
    bc_fill(rows, n_cls, false, classes);
    if ((rc = d2h(h, rows.data(), E.bc_irows.p, (size_t)n_inst * EV_ROW * sizeof(uint32_t)))) return rc;
    bc_fill(rows, n_inst, true, instances);
    return ERASOR_OK;
}

static int bc_check_rows(erasor_hip_handle *h, const erasor_eval_class_row *classes, size_t cap_classes, size_t *n_classes,
                         const erasor_eval_class_row *instances, size_t cap_instances, size_t *n_instances) {
    if (!n_classes || !n_instances || (!classes && cap_classes) || (!instances && cap_instances)) {
        h->err = "erasor_hip_evaluate_by_class: NULL row count, or a NULL row array with a capacity > 0";
        return ERASOR_E_INVALID;
    }
    *n_classes = 0;
    *n_instances = 0;
    return ERASOR_OK;
}

int erasor_hip_evaluate_clouds_by_class(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *est_xyzi,
                                        size_t n_est, int est_is_device, double voxel_leaf, double voxelsize, erasor_eval_class_row *classes,
                                        size_t cap_classes, size_t *n_classes, erasor_eval_class_row *instances, size_t cap_instances,
                                        size_t *n_instances, erasor_eval_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    EvPair p;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, false, res);
    if (rc || (rc = bc_check_rows(h, classes, cap_classes, n_classes, instances, cap_instances, n_instances)) ||
        (rc = ev_pair_clouds(h, "erasor_hip_evaluate_clouds_by_class", gt_xyzi, n_gt, gt_is_device, est_xyzi, n_est, est_is_device, voxel_leaf, &p)))
        return rc;
    return bc_run(h, p.g, p.ng, p.e, p.ne, voxelsize, classes, cap_classes, n_classes, instances, cap_instances, n_instances, res);
}

int erasor_hip_evaluate_map_by_class(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, double voxel_leaf, double voxelsize,
                                     erasor_eval_class_row *classes, size_t cap_classes, size_t *n_classes, erasor_eval_class_row *instances,
                                     size_t cap_instances, size_t *n_instances, erasor_eval_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    EvPair p;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, false, res);
    if (rc || (rc = bc_check_rows(h, classes, cap_classes, n_classes, instances, cap_instances, n_instances)) ||
        (rc = ev_pair_map(h, "erasor_hip_evaluate_map_by_class", gt_xyzi, n_gt, gt_is_device, voxel_leaf, &p)))
        return rc;
    return bc_run(h, p.g, p.ng, p.e, p.ne, voxelsize, classes, cap_classes, n_classes, instances, cap_instances, n_instances, res);
}

// ---- bird's-eye images (erasor_hip_render_*; kernels: render.hip.h) ----
// Like ev_run: the main stream, behind whatever a collected step launched ahead there; scratch of the renderer's own (h->ev.rd_*).
static constexpr uint32_t RD_MAX_EDGE = 16384u;
static constexpr uint64_t RD_MAX_PIXELS = 1ull << 26;

static int rd_check_view(erasor_hip_handle *h, const erasor_render_view *v) {
    if (!v) {
        h->err = "erasor_hip_render: view is NULL";
        return ERASOR_E_INVALID;
    }
    if (!(v->res > 0) || !std::isfinite(v->res) || !std::isfinite(v->x0) || !std::isfinite(v->y0) || !std::isfinite(v->z_lo) || !std::isfinite(v->z_hi)) {
        h->err = "erasor_hip_render: the view needs a finite res > 0 and finite x0, y0, z_lo, z_hi";
        return ERASOR_E_INVALID;
    }
    if (v->width < 1 || v->height < 1 || v->width > RD_MAX_EDGE || v->height > RD_MAX_EDGE || (uint64_t)v->width * v->height > RD_MAX_PIXELS) {
        h->err = "erasor_hip_render: the view needs 1 <= width, height <= 16384 and width * height <= 2^26 (got " + std::to_string(v->width) + " x " +
                 std::to_string(v->height) + ")";
        return ERASOR_E_INVALID;
    }
    return ERASOR_OK;
}

// the kernels' view and mode from the caller's
static RdView rd_view(const erasor_render_view *view) {
    RdView v;
    v.x0 = view->x0;
    v.y0 = view->y0;
    v.res = view->res;
    v.z_lo = view->z_lo;
    v.z_hi = view->z_hi;
    v.width = view->width;
    v.height = view->height;
    v.tiles_x = cdiv(view->width, RD_TILE);
    v.background = view->background & 0xFFFFFFu;
    return v;
}
static RdMode rd_mode(int mode, int32_t target_class, int32_t target_instance) {
    RdMode m;
    m.mode = (uint32_t)mode;
    m.target_class = mode == ERASOR_RENDER_LABEL ? target_class : -1;
    m.target_instance = target_instance;
    for (uint32_t c = 0; c < RD_NCAT; ++c) m.palette[c] = ERASOR_RENDER_PALETTE[c];
    return m;
}
static void rd_stats(const unsigned long long c[RD_NCTR], uint64_t n, erasor_render_stats *stats) {
    erasor_render_stats s;
    memset(&s, 0, sizeof(s));
    s.n_points = n;
    s.n_outside = c[RD_C_OUTSIDE];
    s.n_nonfinite = c[RD_C_NONFINITE];
    for (uint32_t k = 0; k < RD_NCAT; ++k) {
        s.cat_points[k] = c[RD_C_CATPTS + k];
        s.cat_pixels[k] = c[RD_C_CATPIX + k];
        s.n_drawn += s.cat_points[k];
        s.n_pixels_hit += s.cat_pixels[k];
    }
    *stats = s;
}

// the view fitted to pts[0 .. n) (device); see erasor_hip_render_fit
static int rd_fit(erasor_hip_handle *h, const float4 *pts, uint32_t n, double res, uint32_t margin, uint32_t background, erasor_render_view *view) {
    auto &E = h->ev;
    if (!view) {
        h->err = "erasor_hip_render_fit: view is NULL";
        return ERASOR_E_INVALID;
    }
    if (!(res > 0) || !std::isfinite(res) || margin < 1 || margin > 1024) {
        h->err = "erasor_hip_render_fit: res must be a finite number > 0 and margin_px in 1 .. 1024";
        return ERASOR_E_INVALID;
    }
    if (ensure(h, E.rd_zb, (size_t)n + 1) || ensure(h, E.rd_bb, 4) || ensure(h, E.rd_ctr, RD_NCTR) || ensure(h, E.nn_hist, OV_SEL_MAX * 256))
        return ERASOR_E_NO_DEVICE;
    HIPC(h, hipMemsetAsync(E.rd_bb.p, 0xFF, 2 * sizeof(uint32_t), h->stream));
    HIPC(h, hipMemsetAsync(E.rd_bb.p + 2, 0, 2 * sizeof(uint32_t), h->stream));
    HIPC(h, hipMemsetAsync(E.rd_ctr.p, 0, sizeof(unsigned long long), h->stream));
    if (n) LAUNCH(h, h->stream, "render_fit", k_rd_fit, cdiv(n, 2048), 256, pts, n, E.rd_zb.p, E.rd_bb.p, E.rd_ctr.p);
    uint32_t bb[4];
    unsigned long long nfin = 0;
    HIPC(h, hipMemcpyAsync(bb, E.rd_bb.p, sizeof(bb), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipMemcpyAsync(&nfin, E.rd_ctr.p, sizeof(nfin), hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (!nfin) {
        h->err = "erasor_hip_render_fit: the cloud has no finite point";
        return ERASOR_E_INVALID;
    }
    auto inv = [](uint32_t k) {  // (rd_zinv on the host)
        const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
        float f;
        memcpy(&f, &b, sizeof(f));
        return (double)f;
    };
    const double mn[2] = {inv(bb[0]), inv(bb[1])}, mx[2] = {inv(bb[2]), inv(bb[3])};
    double o[2], sz[2];
    for (int a = 0; a < 2; ++a) {
        o[a] = floor(mn[a] / res) * res - (double)margin * res;
        sz[a] = floor((mx[a] - o[a]) / res) + 1.0 + (double)margin;
    }
    if (!std::isfinite(o[0]) || !std::isfinite(o[1]) || !(sz[0] <= RD_MAX_EDGE) || !(sz[1] <= RD_MAX_EDGE) || !(sz[0] * sz[1] <= (double)RD_MAX_PIXELS)) {
        // the smallest res that fits: the sizes at res r are about span / r + 2 * margin + 2
        const double sx = mx[0] - mn[0], sy = mx[1] - mn[1], pad = 2.0 * margin + 2.0;
        double lo = res, hi = res;
        auto fits = [&](double r) {
            const double w = sx / r + pad, hh = sy / r + pad;
            return w <= RD_MAX_EDGE && hh <= RD_MAX_EDGE && w * hh <= (double)RD_MAX_PIXELS;
        };
        while (!fits(hi) && hi < 1e300) hi *= 2;
        for (int it = 0; it < 60; ++it) {
            const double mid = 0.5 * (lo + hi);
            (fits(mid) ? hi : lo) = mid;
        }
        char buf[256];
        snprintf(buf, sizeof(buf), "erasor_hip_render_fit: at res %g the image would be %.0f x %.0f pixels (limits: 16384 per edge, 2^26 in all); "
                 "the smallest res that fits is about %.3g", res, sz[0], sz[1], hi * 1.001);
        h->err = buf;
        return ERASOR_E_INVALID;
    }
    // z_lo / z_hi: the values at ranks floor(0.02 (n - 1)) and floor(0.98 (n - 1)) of the finite heights
    uint64_t rk[OV_SEL_MAX];
    rk[0] = (uint64_t)floor(0.02 * (double)(nfin - 1));
    rk[1] = (uint64_t)floor(0.98 * (double)(nfin - 1));
    for (uint32_t t = 2; t < OV_SEL_MAX; ++t) rk[t] = rk[0];
    double sel[OV_SEL_MAX];
    const int rc = ov_select(h, E.rd_zb.p, n, rk, sel, 24);
    if (rc) return rc;
    unsigned long long kz[2];
    memcpy(kz, sel, sizeof(kz));
    memset(view, 0, sizeof(*view));
    view->x0 = o[0];
    view->y0 = o[1];
    view->res = res;
    view->width = (uint32_t)sz[0];
    view->height = (uint32_t)sz[1];
    view->z_lo = inv((uint32_t)kz[0]);
    view->z_hi = inv((uint32_t)kz[1]);
    view->background = background & 0xFFFFFFu;
    return ERASOR_OK;
}

// pts[0 .. n) (device; code: the evaluator's per-point codes for ERASOR_RENDER_EVAL) into rgb and stats
static int rd_run(erasor_hip_handle *h, const float4 *pts, uint32_t n, const uint8_t *code, int mode, int32_t target_class, int32_t target_instance,
                  const erasor_render_view *view, void *rgb, int rgb_is_device, erasor_render_stats *stats, hipEvent_t ev_begin = nullptr,
                  hipEvent_t ev_end = nullptr) {  // (ev_begin / ev_end: recorded around the clears and the launches, for the hooks' timing)
    auto &E = h->ev;
    const int rc = rd_check_view(h, view);
    if (rc) return rc;
    const RdView v = rd_view(view);
    const RdMode m = rd_mode(mode, target_class, target_instance);
    const uint32_t ntiles = v.tiles_x * cdiv(view->height, RD_TILE);
    const size_t bytes = (size_t)view->width * view->height * 3;
    if (ensure(h, E.rd_ctr, RD_NCTR) || ensure(h, E.rd_cnt, (size_t)ntiles + 1) || ensure(h, E.rd_pl, (size_t)ntiles + 1) ||
        ensure(h, E.rd_tops, ntiles / 1024 + 4) || ensure(h, E.rd_tile, (size_t)n + 1) || ensure(h, E.rd_rec, (size_t)n + 1) ||
        ensure(h, E.rd_srt, (size_t)n + 1) || ensure(h, E.rd_img, bytes + 4))
        return ERASOR_E_NO_DEVICE;
    if (ev_begin) HIPC(h, hipEventRecord(ev_begin, h->stream));
    HIPC(h, hipMemsetAsync(E.rd_ctr.p, 0, RD_NCTR * sizeof(unsigned long long), h->stream));
    HIPC(h, hipMemsetAsync(E.rd_cnt.p, 0, ((size_t)ntiles + 1) * sizeof(uint32_t), h->stream));
    if (n) LAUNCH(h, h->stream, "render_bin", k_rd_bin, cdiv(n, 256), 256, pts, n, code, v, m, E.rd_tile.p, E.rd_rec.p, E.rd_cnt.p, E.rd_ctr.p);
    scan_u32(h, h->stream, E.rd_cnt.p, E.rd_pl.p, E.rd_tops.p, ntiles + 1, ntiles + 1, nullptr, nullptr, "render_scan");
    LAUNCH(h, h->stream, "render_scan", k_ev_offsets, cdiv(ntiles + 1, 256), 256, (const uint32_t *)E.rd_pl.p, (const uint32_t *)E.rd_tops.p, ntiles + 1, E.rd_cnt.p,
           E.rd_pl.p);
    if (n)
        LAUNCH(h, h->stream, "render_scatter", k_rd_scatter, cdiv(n, 256), 256, (const uint32_t *)E.rd_tile.p, (const unsigned long long *)E.rd_rec.p, n, E.rd_pl.p,
               E.rd_srt.p);
    LAUNCH(h, h->stream, "render_resolve", k_rd_resolve, ntiles, 256, (const unsigned long long *)E.rd_srt.p, (const uint32_t *)E.rd_cnt.p, v, m, E.rd_img.p,
           E.rd_ctr.p);
    if (ev_end) HIPC(h, hipEventRecord(ev_end, h->stream));
    unsigned long long c[RD_NCTR];
    HIPC(h, hipMemcpyAsync(c, E.rd_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    if (rgb) HIPC(h, hipMemcpyAsync(rgb, E.rd_img.p, bytes, rgb_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPC(h, hipStreamSynchronize(h->stream));
    if (stats) rd_stats(c, n, stats);
    return ERASOR_OK;
}

int erasor_hip_render_fit(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, double res, uint32_t margin_px, uint32_t background,
                          erasor_render_view *view) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    int rc = check_cloud(h, "erasor_hip_render_fit", BAD_CLOUD, xyzi, n);
    if (rc) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    if ((rc = ev_input(h, xyzi, n, is_device, h->ev.rd_pts, &p))) return rc;
    return rd_fit(h, p, (uint32_t)n, res, margin_px, background, view);
}
int erasor_hip_render_fit_map(erasor_hip_handle *h, double res, uint32_t margin_px, uint32_t background, erasor_render_view *view) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    const int rc = map_on_device(h, "erasor_hip_render_fit_map", h->ev.rd_map, &p, &n);
    if (rc) return rc;
    return rd_fit(h, p, n, res, margin_px, background, view);
}

static int rd_check_mode(erasor_hip_handle *h, int mode) {
    if (mode != ERASOR_RENDER_LABEL && mode != ERASOR_RENDER_HEIGHT) {
        h->err = "erasor_hip_render: mode must be ERASOR_RENDER_LABEL or ERASOR_RENDER_HEIGHT (the error map: erasor_hip_render_eval_*)";
        return ERASOR_E_INVALID;
    }
    return ERASOR_OK;
}
int erasor_hip_render_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, int mode, int32_t target_class, int32_t target_instance,
                             const erasor_render_view *view, void *rgb, int rgb_is_device, erasor_render_stats *stats) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    int rc = rd_check_mode(h, mode);
    if (rc || (rc = rd_check_view(h, view)) || (rc = check_cloud(h, "erasor_hip_render_clouds", BAD_CLOUD, xyzi, n))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    if ((rc = ev_input(h, xyzi, n, is_device, h->ev.rd_pts, &p))) return rc;
    return rd_run(h, p, (uint32_t)n, nullptr, mode, target_class, target_instance, view, rgb, rgb_is_device, stats);
}
int erasor_hip_render_map(erasor_hip_handle *h, int mode, int32_t target_class, int32_t target_instance, const erasor_render_view *view, void *rgb,
                          int rgb_is_device, erasor_render_stats *stats) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    int rc = rd_check_mode(h, mode);
    if (rc || (rc = rd_check_view(h, view))) return rc;
    HIPC(h, hipSetDevice(h->device));
    const float4 *p = nullptr;
    uint32_t n = 0;
    if ((rc = map_on_device(h, "erasor_hip_render_map", h->ev.rd_map, &p, &n))) return rc;
    return rd_run(h, p, n, nullptr, mode, target_class, target_instance, view, rgb, rgb_is_device, stats);
}

// the evaluation of a pair as erasor_hip_evaluate_* runs it, its codes left in h->ev.code, then the ground truth drawn by them
static int rd_eval(erasor_hip_handle *h, const EvPair &p, double voxelsize, const erasor_render_view *view, void *rgb, int rgb_is_device,
                   erasor_render_stats *stats, erasor_eval_result *res) {
    const int rc = ev_run(h, p.g, p.ng, p.e, p.ne, voxelsize, nullptr, res, nullptr, true);
    if (rc) return rc;
    return rd_run(h, p.g, p.ng, h->ev.code.p, ERASOR_RENDER_EVAL, -1, -1, view, rgb, rgb_is_device, stats);
}
int erasor_hip_render_eval_clouds(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *est_xyzi, size_t n_est,
                                  int est_is_device, double voxel_leaf, double voxelsize, const erasor_render_view *view, void *rgb,
                                  int rgb_is_device, erasor_render_stats *stats, erasor_eval_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    EvPair p;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, false, res);
    if (rc || (rc = rd_check_view(h, view)) ||
        (rc = ev_pair_clouds(h, "erasor_hip_render_eval_clouds", gt_xyzi, n_gt, gt_is_device, est_xyzi, n_est, est_is_device, voxel_leaf, &p)))
        return rc;
    return rd_eval(h, p, voxelsize, view, rgb, rgb_is_device, stats, res);
}
int erasor_hip_render_eval_map(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, double voxel_leaf, double voxelsize,
                               const erasor_render_view *view, void *rgb, int rgb_is_device, erasor_render_stats *stats, erasor_eval_result *res) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    EvPair p;
    int rc = ev_check_args(h, voxel_leaf, voxelsize, false, res);
    if (rc || (rc = rd_check_view(h, view)) || (rc = ev_pair_map(h, "erasor_hip_render_eval_map", gt_xyzi, n_gt, gt_is_device, voxel_leaf, &p))) return rc;
    return rd_eval(h, p, voxelsize, view, rgb, rgb_is_device, stats, res);
}

#ifdef ERASOR_HIP_TEST_HOOKS
// rd_run's image and counters by the other rasteriser (one 64-bit atomic max per point on a key image in device memory): the comparison
// of MEASUREMENTS.md.  Mode LABEL or HEIGHT; tiled != 0: the shipped kernels (rd_run) instead, timed the same way; ms (optional): device
// time between one event before the clears and one after the last kernel -- the same bracket for both.
int erasor_hip_debug_render_atomic(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, int mode, const erasor_render_view *view,
                                   void *rgb, erasor_render_stats *stats, int tiled, double *ms) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    int rc = rd_check_mode(h, mode);
    if (rc || (rc = rd_check_view(h, view)) || (rc = check_cloud(h, "erasor_hip_debug_render_atomic", BAD_CLOUD, xyzi, n))) return rc;
    auto &E = h->ev;
    const float4 *p = nullptr;
    HIPC(h, hipSetDevice(h->device));
    if ((rc = ev_input(h, xyzi, n, is_device, E.rd_pts, &p))) return rc;
    if (tiled) {
        hipEvent_t a, b;
        HIPC(h, hipEventCreate(&a));
        HIPC(h, hipEventCreate(&b));
        rc = rd_run(h, p, (uint32_t)n, nullptr, mode, -1, -1, view, rgb, 0, stats, a, b);
        float t = 0.f;
        if (!rc && hipEventElapsedTime(&t, a, b) != hipSuccess) rc = ERASOR_E_NO_DEVICE;
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        if (ms) *ms = t;
        return rc;
    }
    const RdView v = rd_view(view);
    const RdMode m = rd_mode(mode, -1, -1);
    const size_t npix = (size_t)view->width * view->height;
    DBuf<unsigned long long> keyimg;
    if (ensure(h, keyimg, npix + 1) || ensure(h, E.rd_ctr, RD_NCTR) || ensure(h, E.rd_img, npix * 3 + 4)) return ERASOR_E_NO_DEVICE;
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, h->stream);
    (void)hipMemsetAsync(E.rd_ctr.p, 0, RD_NCTR * sizeof(unsigned long long), h->stream);
    (void)hipMemsetAsync(keyimg.p, 0, npix * sizeof(unsigned long long), h->stream);
    if (n)
        hipLaunchKernelGGL(k_rd_atomic_points, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, p, (uint32_t)n, (const uint8_t *)nullptr, v, m, keyimg.p,
                           E.rd_ctr.p);
    hipLaunchKernelGGL(k_rd_atomic_pixels, dim3(cdiv(npix, 256)), dim3(256), 0, h->stream, (const unsigned long long *)keyimg.p, v, m, E.rd_img.p,
                       E.rd_ctr.p);
    (void)hipEventRecord(b, h->stream);
    unsigned long long c[RD_NCTR];
    (void)hipMemcpyAsync(c, E.rd_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream);
    if (rgb) (void)hipMemcpyAsync(rgb, E.rd_img.p, npix * 3, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e_ = hipStreamSynchronize(h->stream);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, a, b);
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    release(keyimg);
    if (e_ != hipSuccess) return ERASOR_E_NO_DEVICE;
    if (ms) *ms = t;
    if (stats) rd_stats(c, n, stats);
    return ERASOR_OK;
}
#endif

#ifdef ERASOR_HIP_TEST_HOOKS
// test hook: the bounding-volume tree of a cloud (x y z i rows, host or device) as nn_build builds it for overlap, align_frames,
// label_map and static_complement: P, the points in key order with their original indices, the sorted Morton keys, the boxes of all 2P
// nodes (node 0 is never written: its rows come back as they lie in the scratch).  cap_nodes: the rows lo / hi hold.
int erasor_hip_debug_nn_tree(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, uint32_t *P_out, float *pts, uint32_t *idx,
                             uint32_t *keys, float *lo, float *hi, size_t cap_nodes) {
    NOFLY(h);
    if (!h || !xyzi || !n || n > MAX_POINTS || !P_out || !pts || !idx || !keys || !lo || !hi) return ERASOR_E_INVALID;
    HIPC(h, hipSetDevice(h->device));
    auto &E = h->ev;
    const float4 *g = nullptr;
    int rc = ev_input(h, xyzi, n, is_device, E.gt, &g);
    if (rc) return rc;
    NnTree T;
    if ((rc = nn_build(h, g, (uint32_t)n, "erasor_hip_debug_nn_tree", "cloud", "point(s)", &T))) return rc;
    *P_out = T.n_pad;
    if (2 * (size_t)T.n_pad > cap_nodes) return ERASOR_E_CAPACITY;
    if ((rc = d2h(h, pts, T.pts, n * sizeof(float4))) || (rc = d2h(h, idx, T.idx, n * sizeof(uint32_t))) ||
        (rc = d2h(h, keys, E.dbg_skeys, n * sizeof(uint32_t))) || (rc = d2h(h, lo, T.lo, 2 * (size_t)T.n_pad * sizeof(float4))) ||
        (rc = d2h(h, hi, T.hi, 2 * (size_t)T.n_pad * sizeof(float4))))
        return rc;
    return ERASOR_OK;
}

// test hook: k_nn_query (f32 == 0: overlap's float64 search) or k_lm_query (f32 != 0: label_map's float32 search) of n_q queries over
// the tree of a cloud, built as above, with every query's effort beside the kernel's own outputs: effort[2 * i] = leaves opened,
// effort[2 * i + 1] = leaf points tested.  f32 == 0: dist / nearest as erasor_hip_overlap_clouds returns them per point; f32 != 0:
// rows = k_lm_query's output (x, y, z, the nearest point's w), *n_tied its FM_TIED counter.  Queries must be finite.
int erasor_hip_debug_nn_effort(erasor_hip_handle *h, const float *tree_xyzi, size_t n, const float *query_xyzi, size_t n_q, int f32, double *dist,
                               uint32_t *nearest, float *rows, uint64_t *n_tied, uint32_t *effort) {
    NOFLY(h);
    if (!h || !tree_xyzi || !n || n > MAX_POINTS || !query_xyzi || !n_q || n_q > MAX_POINTS || !effort) return ERASOR_E_INVALID;
    if (f32 ? (!rows || !n_tied) : (!dist || !nearest)) return ERASOR_E_INVALID;
    HIPC(h, hipSetDevice(h->device));
    auto &E = h->ev;
    const float4 *g = nullptr, *q = nullptr;
    int rc;
    if ((rc = ev_input(h, tree_xyzi, n, 0, E.gt, &g)) || (rc = ev_input(h, query_xyzi, n_q, 0, E.est, &q))) return rc;
    const uint32_t nt = (uint32_t)n, nq = (uint32_t)n_q;
    if (ensure(h, E.fm_ctr, FM_NCTR) || ensure(h, E.nn_dbits, n_q + 1) || ensure(h, E.nn_near, n_q + 1) ||
        ensure(h, E.fm_out, n_q + 1))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    if ((rc = nn_build(h, g, nt, "erasor_hip_debug_nn_effort", "cloud", "point(s)", &T))) return rc;
    HIPC(h, hipMemsetAsync(E.fm_ctr.p, 0, FM_NCTR * sizeof(unsigned long long), h->stream));
    uint32_t *d_eff = nullptr;  // (the query grid's lanes past n_q never search: 2 * n_q entries are all that is written)
    HIPC(h, hipMalloc((void **)&d_eff, 2 * n_q * sizeof(uint32_t)));
    (void)hipMemsetAsync(d_eff, 0xFF, 2 * n_q * sizeof(uint32_t), h->stream);
    hipLaunchKernelGGL(k_nn_set_effort, dim3(1), dim3(1), 0, h->stream, d_eff);
    if (f32)
        LAUNCH(h, h->stream, "lm_query", k_lm_query, cdiv(nq, NN_QBLOCK), NN_QBLOCK, q, nq, T, E.fm_out.p, E.fm_ctr.p);
    else
        LAUNCH(h, h->stream, "ov_query", k_nn_query, cdiv(nq, NN_QBLOCK), NN_QBLOCK, q, nq, T, 0.5, 1.0, 2.0, E.nn_dbits.p, E.nn_near.p, E.nn_ctr.p);
    hipLaunchKernelGGL(k_nn_set_effort, dim3(1), dim3(1), 0, h->stream, (uint32_t *)nullptr);
    unsigned long long c[FM_NCTR], co[OV_NCTR];
    rc = d2h(h, effort, d_eff, 2 * n_q * sizeof(uint32_t));
    (void)hipFree(d_eff);
    if (rc || (rc = d2h(h, c, E.fm_ctr.p, sizeof(c))) || (rc = d2h(h, co, E.nn_ctr.p, sizeof(co)))) return rc;
    if (c[FM_NON_FINITE] || co[OV_NON_FINITE]) {
        h->err = "erasor_hip_debug_nn_effort: non-finite query";
        return ERASOR_E_INVALID;
    }
    if (f32) {
        *n_tied = c[FM_TIED];
        return d2h(h, rows, E.fm_out.p, n_q * sizeof(float4));
    }
    if ((rc = d2h(h, dist, E.nn_dbits.p, n_q * sizeof(double)))) return rc;
    return d2h(h, nearest, E.nn_near.p, n_q * sizeof(uint32_t));
}

// test hook: the labelling's bounded search (k_ls_query's static pass: one frame, identity transforms) of n_q finite queries over the
// tree of a cloud, built as above: codes[i] = 0 when a tree point lies within tau of query i, else 1, and the search's effort beside it,
// effort[2 * i] = leaves opened, effort[2 * i + 1] = leaf points tested -- to set against erasor_hip_debug_nn_effort's on the same input.
int erasor_hip_debug_ls_effort(erasor_hip_handle *h, const float *tree_xyzi, size_t n, const float *query_xyzi, size_t n_q, double tau, uint8_t *codes,
                               uint32_t *effort) {
    NOFLY(h);
    if (!h || !tree_xyzi || !n || n > MAX_POINTS || !query_xyzi || !n_q || n_q > MAX_POINTS || !codes || !effort || !(tau > 0) || !std::isfinite(tau))
        return ERASOR_E_INVALID;
    HIPC(h, hipSetDevice(h->device));
    auto &E = h->ev;
    const float4 *g = nullptr, *q = nullptr;
    int rc;
    if ((rc = ev_input(h, tree_xyzi, n, 0, E.gt, &g)) || (rc = ev_input(h, query_xyzi, n_q, 0, E.est, &q))) return rc;
    const uint32_t nt = (uint32_t)n, nq = (uint32_t)n_q, grid = cdiv(nq, NN_QBLOCK);
    if (ensure(h, E.al_off, 2) || ensure(h, E.al_wg, (size_t)grid + 1) || ensure(h, E.al_xf, 1) ||
        ensure(h, E.al_ctr, LS_NCTR) || ensure(h, E.code, n_q + 1))
        return ERASOR_E_NO_DEVICE;
    NnTree T;
    if ((rc = nn_build(h, g, nt, "erasor_hip_debug_ls_effort", "cloud", "point(s)", &T))) return rc;
    const uint32_t off[2] = {0, nq};
    const Xf one = to_xf(AL_IDENTITY);
    HIPC(h, hipMemcpyAsync(E.al_off.p, off, sizeof(off), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.al_wg.p, 0, ((size_t)grid + 1) * sizeof(uint32_t), h->stream));
    HIPC(h, hipMemcpyAsync(E.al_xf.p, &one, sizeof(Xf), hipMemcpyHostToDevice, h->stream));
    HIPC(h, hipMemsetAsync(E.al_ctr.p, 0, LS_NCTR * sizeof(unsigned long long), h->stream));
    uint32_t *d_eff = nullptr;
    HIPC(h, hipMalloc((void **)&d_eff, 2 * n_q * sizeof(uint32_t)));
    (void)hipMemsetAsync(d_eff, 0xFF, 2 * n_q * sizeof(uint32_t), h->stream);
    hipLaunchKernelGGL(k_nn_set_effort, dim3(1), dim3(1), 0, h->stream, d_eff);
    rc = ls_pass(h, q, nq, nullptr, 0, 1, one, T, ls_bound(tau), LS_STATIC, LS_DYNAMIC, 1u, nullptr);
    hipLaunchKernelGGL(k_nn_set_effort, dim3(1), dim3(1), 0, h->stream, (uint32_t *)nullptr);
    if (!rc) rc = d2h(h, effort, d_eff, 2 * n_q * sizeof(uint32_t));
    (void)hipFree(d_eff);
    unsigned long long c[LS_NCTR];
    if (rc || (rc = d2h(h, c, E.al_ctr.p, sizeof(c)))) return rc;
    if (c[LS_NON_FINITE]) {
        h->err = "erasor_hip_debug_ls_effort: non-finite query";
        return ERASOR_E_INVALID;
    }
    return d2h(h, codes, E.code.p, n_q);
}

// what ev_run / evm_run left in the evaluator's scratch: the bucket count, the bucket offsets and the scattered points and indices
static int dbg_ev_dump(erasor_hip_handle *h, size_t n, uint32_t *nb_out, uint32_t *off, size_t cap_off, float *pts, uint32_t *idx) {
    auto &E = h->ev;
    *nb_out = E.dbg_nb;
    if ((size_t)E.dbg_nb + 1 > cap_off) return ERASOR_E_CAPACITY;
    int rc;
    if ((rc = d2h(h, off, E.cnt.p, ((size_t)E.dbg_nb + 1) * sizeof(uint32_t))) || (rc = d2h(h, pts, E.pts.p, n * sizeof(float4))) ||
        (rc = d2h(h, idx, E.idx.p, n * sizeof(uint32_t))))
        return rc;
    return ERASOR_OK;
}

// test hook: the hashed grid of an estimate (n > 0 host rows) at a voxel size, built by erasor_hip_evaluate_clouds' own path (ev_run, an
// empty ground truth): nb, off[nb + 1], the scattered points and their indices
int erasor_hip_debug_ev_grid(erasor_hip_handle *h, const float *est_xyzi, size_t n, double voxelsize, uint32_t *nb_out, uint32_t *off, size_t cap_off,
                             float *pts, uint32_t *idx) {
    if (!h || !est_xyzi || !n || !nb_out || !off || !pts || !idx) return ERASOR_E_INVALID;
    erasor_eval_result res;
    const int rc = erasor_hip_evaluate_clouds(h, nullptr, 0, 0, est_xyzi, n, 0, 0.0, voxelsize, nullptr, &res);
    if (rc) return rc;
    return dbg_ev_dump(h, n, nb_out, off, cap_off, pts, idx);
}

// test hook: the combined table of k estimates (host rows; some may be empty, not all), built by erasor_hip_evaluate_many's own path
// (evm_run, an empty ground truth): as above over all estimates back to back (idx: combined indices), and tab[4 * j ..] = estimate j's
// (first point, points, first bucket, bucket mask)
int erasor_hip_debug_ev_grid_many(erasor_hip_handle *h, const void *const *est_xyzi, const size_t *n_est, size_t k, double voxelsize, uint32_t *nb_out,
                                  uint32_t *off, size_t cap_off, float *pts, uint32_t *idx, uint32_t *tab) {
    if (!h || !est_xyzi || !n_est || !k || !nb_out || !off || !pts || !idx || !tab) return ERASOR_E_INVALID;
    std::vector<erasor_eval_result> rows(k);
    const int rc = erasor_hip_evaluate_many(h, nullptr, 0, 0, est_xyzi, n_est, nullptr, k, 0.0, voxelsize, rows.data());
    if (rc) return rc;
    size_t n = 0;
    for (size_t j = 0; j < k; ++j) {
        const EvmEst &e = h->ev.dbg_tab[j];
        tab[4 * j] = e.off;
        tab[4 * j + 1] = e.n;
        tab[4 * j + 2] = e.base;
        tab[4 * j + 3] = e.mask;
        n += n_est[j];
    }
    if (!n) return ERASOR_E_INVALID;
    return dbg_ev_dump(h, n, nb_out, off, cap_off, pts, idx);
}
#endif  // ERASOR_HIP_TEST_HOOKS

}  // extern "C"

// ---- a parameter sweep: every configuration over one sequence, each one's saved map scored by PR / RR (erasor_hip_sweep) ----
// What the shim's OfflineMapUpdater + save_static_map + evaluate_saved_map do for one configuration (demo_main.cpp --config <yaml> n
// <gt>): node j (0-based) is stepped iff (j + 1) % removal_interval == 0 (OMU.cpp:206-209), the map after the last node is voxelised by
// voxelize_preserving_labels at save_leaf (main_in_your_env.cpp:123), and that map is evaluated against the GT as given.  The map, the
// scans and the GT go to the device once.  Configurations run in waves of worker handles on the caller's device, one host thread each,
// every worker with ONE query stream (two such handles keep the device's four compute pipes busy, DESIGN "Several handles on one GPU");
// a worker takes its map from the shared copy, steps the shared scans in place, voxelises its final map into a buffer of the sweep's and is
// destroyed before the next wave.  Then the saved maps are scored in groups by evm_run, in the caller handle's evaluator scratch.
namespace {
constexpr int SWEEP_LOOKAHEAD = 6;  // nodes announced ahead by a worker (the offline driver's default)
struct SweepIn {
    int device = 0;
    const float4 *map = nullptr;
    size_t n_map = 0;
    const float4 *scans = nullptr;
    const uint64_t *offsets = nullptr;
    size_t n_nodes = 0;
    const float *Tl = nullptr, *Tb = nullptr, *To = nullptr;
    double save_leaf = 0;
};
struct SweepJob {
    erasor_params p;
    int status = ERASOR_OK;
    uint32_t n_steps = 0;
    uint64_t n_map_final = 0;
    float4 *saved = nullptr;  // the saved map (hipMalloc of the sweep's), n_saved points
    uint32_t n_saved = 0;
    double run_ms = 0;
};

// a worker handle's device memory for a map of n_map points and scans of at most max_scan points: per slot of alloc_map's capacity the
// map-sized scratch, the outskirts store and both F buffers, per scan point the query sides, plus the saved map; rounded up (a handle
// with a 9.8 M-point map took 5.49 GB after four steps of 245 k-point scans, this gives 5.6 GB)
uint64_t sweep_need(size_t n_map, uint64_t max_scan) {
    const uint64_t cap = (uint64_t)n_map + std::max<uint64_t>(n_map / 4, 1u << 20);
    return cap * 420 + max_scan * 8 * 96 + (uint64_t)n_map * 24 + (64ull << 20);
}

void sweep_one(const SweepIn &in, SweepJob &J) {
    if (hipSetDevice(in.device) != hipSuccess) {
        J.status = ERASOR_E_NO_DEVICE;
        return;
    }
    const int ri = J.p.removal_interval;
    if (ri < 1) {  // (the shim takes stack_count % removal_interval)
        J.status = ERASOR_E_INVALID;
        return;
    }
    std::vector<const void *> ptrs;
    std::vector<size_t> np;
    std::vector<float> Tb, To;
    for (size_t j = 0; j < in.n_nodes; ++j) {
        if ((j + 1) % (size_t)ri != 0) continue;  // OMU.cpp:206-209
        ptrs.push_back(in.scans + in.offsets[j]);
        np.push_back((size_t)(in.offsets[j + 1] - in.offsets[j]));
        Tb.insert(Tb.end(), in.Tb + 16 * j, in.Tb + 16 * j + 16);
        To.insert(To.end(), in.To + 16 * j, in.To + 16 * j + 16);
    }
    J.n_steps = (uint32_t)ptrs.size();
    erasor_hip_handle *h = nullptr;
    int rc = create_handle(&J.p, in.device, 1, &h);
    if (rc) {
        J.status = rc;
        return;
    }
    rc = erasor_hip_set_map_device(h, in.map, in.n_map);
    if (!rc && !ptrs.empty()) {
        size_t announced = 0;
        const auto t0 = std::chrono::steady_clock::now();
        rc = erasor_hip_run_nodes(h, ptrs.data(), np.data(), ptrs.size(), 1, in.Tl, Tb.data(), To.data(), 0, ptrs.size(), SWEEP_LOOKAHEAD, &announced,
                                  nullptr);
        J.run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    size_t n_final = 0;
    if (!rc) rc = map_to_device(h, h->ev.map, &n_final);
    if (!rc && n_final > MAX_POINTS) rc = ERASOR_E_CAPACITY;
    uint32_t nq = (uint32_t)n_final;
    const float4 *src = h->ev.map.p;
    if (!rc && in.save_leaf > 0 && n_final) {
        rc = voxelize_device(h, h->ev.map.p, (uint32_t)n_final, in.save_leaf, &nq);
        src = h->q[h->qi].query.p;
    }
    if (!rc) {
        J.n_map_final = n_final;
        if (hipMalloc((void **)&J.saved, ((size_t)nq + 1) * sizeof(float4)) != hipSuccess) {
            J.saved = nullptr;
            rc = ERASOR_E_NO_DEVICE;
        } else if ((nq && hipMemcpyAsync(J.saved, src, (size_t)nq * sizeof(float4), hipMemcpyDeviceToDevice, h->stream) != hipSuccess) ||
                   hipStreamSynchronize(h->stream) != hipSuccess) {
            rc = ERASOR_E_NO_DEVICE;
        }
        J.n_saved = nq;
    }
    J.status = rc;
    erasor_hip_destroy(h);
}

// hipMemGetInfo, looked up at run time in the library that provides the HIP runtime: a runtime that does not export it gets no memory
// check (every wave is then `concurrency` wide)
using MemInfoFn = hipError_t (*)(size_t *, size_t *);
MemInfoFn mem_info_fn() {
    static const MemInfoFn fn = [] {
        Dl_info info;
        if (!dladdr((void *)&hipGetDeviceCount, &info) || !info.dli_fname) return (MemInfoFn) nullptr;
        void *lib = dlopen(info.dli_fname, RTLD_LAZY | RTLD_NOLOAD);
        return lib ? (MemInfoFn)dlsym(lib, "hipMemGetInfo") : (MemInfoFn) nullptr;
    }();
    return fn;
}

// a sweep-owned device buffer (freed on every return)
struct SweepBuf {
    void *p = nullptr;
    ~SweepBuf() {
        if (p) (void)hipFree(p);
    }
};
}  // namespace

int erasor_hip_sweep(erasor_hip_handle *h, const erasor_params *configs, size_t n_configs, const void *map_xyzi, size_t n_map, int map_is_device,
                     const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_nodes, int scans_are_device,
                     const float T_lidar2body[16], const float *T_body2origin, const float *T_origin2body, const void *gt_xyzi, size_t n_gt,
                     int gt_is_device, double save_leaf, double voxelsize, int concurrency, int eval_batch, erasor_sweep_row *rows) {
    NOFLY(h);
    if (!h) return ERASOR_E_INVALID;
    const char *who = "erasor_hip_sweep";
    auto fail = [&](const char *why) { return invalid(h, who, why); };
    if (n_configs > 256) return fail("more than 256 configurations");
    if (n_configs && (!configs || !rows)) return fail("configs or rows is NULL");
    if (concurrency < 1 || concurrency > 4) return fail("concurrency must be 1..4");
    if (eval_batch < 0) return fail("eval_batch must be >= 0");
    if (!(voxelsize > 0) || !std::isfinite(voxelsize)) return fail("voxelsize must be a finite number > 0");
    if (!(save_leaf >= 0) || !std::isfinite(save_leaf)) return fail("save_leaf must be 0 or a finite number > 0");
    int rc = check_cloud(h, who, "NULL map or more than 2^30 map points", map_xyzi, n_map);
    if (rc || (rc = check_cloud(h, who, "NULL ground truth or more than 2^30 points", gt_xyzi, n_gt))) return rc;
    if (!offsets) return fail("offsets is NULL (n_nodes + 1 entries)");
    if ((rc = check_scan_offsets(h, who, scans_xyzi, n_scan_points, offsets, n_nodes))) return rc;
    if (!T_lidar2body || (n_nodes && (!T_body2origin || !T_origin2body))) return fail("a pose array is NULL");
    if (!all_finite(T_lidar2body, 16)) return fail("non-finite entry in T_lidar2body");
    if (!all_finite(T_body2origin, n_nodes * 16) || !all_finite(T_origin2body, n_nodes * 16))
        return fail("non-finite entry in T_body2origin or T_origin2body");
    HIPC(h, hipSetDevice(h->device));
    // the shared inputs, on the device once
    SweepBuf b_map, b_scans, b_gt;
    auto upload = [&](const void *src, size_t n, int is_device, SweepBuf &b, const float4 **out) -> int {
        *out = (const float4 *)src;
        if (is_device || !n) return ERASOR_OK;
        HIPC(h, hipMalloc(&b.p, n * sizeof(float4)));
        HIPC(h, hipMemcpyAsync(b.p, src, n * sizeof(float4), hipMemcpyHostToDevice, h->stream));
        HIPC(h, hipStreamSynchronize(h->stream));
        *out = (const float4 *)b.p;
        return ERASOR_OK;
    };
    SweepIn in;
    in.device = h->device;
    const float4 *d_gt = nullptr;
    if ((rc = upload(map_xyzi, n_map, map_is_device, b_map, &in.map)) || (rc = upload(scans_xyzi, n_scan_points, scans_are_device, b_scans, &in.scans)) ||
        (rc = upload(gt_xyzi, n_gt, gt_is_device, b_gt, &d_gt)))
        return rc;
    // non-finite map / GT points: the GT side of evm_run with no estimate counts them
    for (int c = 0; c < 2; ++c) {
        const float4 *cl = c ? d_gt : in.map;
        const size_t n = c ? n_gt : n_map;
        if (!n) continue;
        if ((rc = evm_run(h, who, cl, (uint32_t)n, nullptr, 0, voxelsize, nullptr))) {
            if (rc == ERASOR_E_INVALID) h->err = std::string(who) + ": non-finite coordinate (NaN / Inf) in the " + (c ? "ground truth" : "map");
            return rc;
        }
    }
    in.n_map = n_map;
    in.offsets = offsets;
    in.n_nodes = n_nodes;
    in.Tl = T_lidar2body;
    in.Tb = T_body2origin;
    in.To = T_origin2body;
    in.save_leaf = save_leaf;
    uint64_t max_scan = 0;
    for (size_t f = 0; f < n_nodes; ++f) max_scan = std::max<uint64_t>(max_scan, offsets[f + 1] - offsets[f]);
    std::vector<SweepJob> jobs(n_configs);
    for (size_t i = 0; i < n_configs; ++i) jobs[i].p = configs[i];
    struct FreeSaved {
        std::vector<SweepJob> &jobs;
        ~FreeSaved() {
            for (auto &J : jobs)
                if (J.saved) (void)hipFree(J.saved);
        }
    } free_saved{jobs};
    // waves of `concurrency` workers, as many as the free device memory takes (at least one, else that configuration fails on its own)
    const MemInfoFn mem_info = mem_info_fn();
    const uint64_t need = sweep_need(n_map, max_scan);
    for (size_t next = 0; next < n_configs;) {
        size_t free_b = ~(size_t)0, total_b = 0;
        if (mem_info) HIPC(h, mem_info(&free_b, &total_b));
        std::vector<size_t> wave;
        uint64_t budget = free_b;
        while (next < n_configs && (int)wave.size() < concurrency && need <= budget) {
            budget -= need;
            wave.push_back(next++);
        }
        if (wave.empty()) {
            jobs[next++].status = ERASOR_E_NO_DEVICE;
            continue;
        }
        std::vector<std::thread> th;
        for (size_t i : wave) th.emplace_back(sweep_one, std::cref(in), std::ref(jobs[i]));
        for (auto &t : th) t.join();
    }
    HIPC(h, hipSetDevice(h->device));
    // the saved maps against the GT, in groups of eval_batch (0: all), each group one evm_run
    std::vector<size_t> ok;
    for (size_t i = 0; i < n_configs; ++i)
        if (jobs[i].status == ERASOR_OK) ok.push_back(i);
    std::vector<erasor_eval_result> ev(n_configs);
    memset(ev.data(), 0, ev.size() * sizeof(erasor_eval_result));
    auto &E = h->ev;
    for (size_t b = 0; b < ok.size();) {
        std::vector<size_t> grp;
        uint64_t total = 0;
        while (b < ok.size() && (eval_batch == 0 || (int)grp.size() < eval_batch) &&
               (grp.empty() || total + jobs[ok[b]].n_saved <= 0x7FFFFFFFull)) {
            total += jobs[ok[b]].n_saved;
            grp.push_back(ok[b++]);
        }
        int grc = ensure(h, E.em_cat, total + 1) ? ERASOR_E_NO_DEVICE : ERASOR_OK;
        std::vector<uint32_t> ne;
        uint64_t off = 0;
        for (size_t i : grp) {
            if (!grc && jobs[i].n_saved &&
                hipMemcpyAsync(E.em_cat.p + off, jobs[i].saved, (size_t)jobs[i].n_saved * sizeof(float4), hipMemcpyDeviceToDevice, h->stream) != hipSuccess)
                grc = ERASOR_E_NO_DEVICE;
            ne.push_back(jobs[i].n_saved);
            off += jobs[i].n_saved;
        }
        if (!grc && hipStreamSynchronize(h->stream) != hipSuccess) grc = ERASOR_E_NO_DEVICE;
        std::vector<erasor_eval_result> r(grp.size());
        if (!grc) grc = evm_run(h, who, d_gt, (uint32_t)n_gt, ne.data(), grp.size(), voxelsize, r.data());
        for (size_t q = 0; q < grp.size(); ++q) {
            if (grc) jobs[grp[q]].status = grc;
            else ev[grp[q]] = r[q];
        }
    }
    for (size_t i = 0; i < n_configs; ++i) {
        erasor_sweep_row &R = rows[i];
        memset(&R, 0, sizeof(R));
        R.params = configs[i];
        R.status = jobs[i].status;
        R.n_steps = jobs[i].n_steps;
        if (jobs[i].status == ERASOR_OK) {
            R.n_map_final = jobs[i].n_map_final;
            R.n_saved = jobs[i].n_saved;
            R.eval = ev[i];
        }
        R.run_ms = jobs[i].run_ms;
    }
    return ERASOR_OK;
}
