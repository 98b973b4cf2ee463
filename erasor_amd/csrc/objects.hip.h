// objects.hip.h — the decision per object (erasor_hip_object_vote_clouds / _map): a removal method's per-point votes spread over the
// clusters they fall on, fragments reverted.  The step decides by bin, the see-through check by pixel vote, the carving by voxel
// log-odds -- one point at a time; this joins their votes with the clustering (cluster.hip.h) and the ground mask (ground.hip.h).
//
// The contract (restated on the host by erasor_amd/evalmap.py, object_vote / object_vote_brute; the device equals it byte for byte):
//   * point i is voted iff votes[i] >= vote_thr, ground iff ground[i] != 0;
//   * ground points are outside the graph (adjacent to nothing, in no cluster): kept if ground_keep, otherwise removed iff voted;
//   * over the other points adjacency is k_cl_unite's predicate, a cluster a connected component, its `first` the lowest index it
//     contains in the GIVEN cloud's indexing;
//   * per cluster, in this order: NOT_OBJECT (n_points < min_size, or max_size != 0 and n_points > max_size, or max_extent > 0 and
//     (double)max - (double)min > max_extent on some axis), REMOVED (n_voted >= min_voted and (double)n_voted >= remove_ratio *
//     (double)n_points), REVERTED (n_voted > 0 and (double)n_voted <= revert_ratio * (double)n_points), UNCHANGED;
//   * one row per touched cluster (n_voted > 0) in increasing `first`.
// Integer atomics, ballots and boxes only: no float sum, one float64 product per cluster and test, nothing depends on scheduling.
//
// The passes (host: obj_run in analysis_host.hip.h):
//   k_obj_flags    one point per lane: the class byte (voted, ground), the non-ground flag for the compaction, and n_voted, n_ground
//                  and the non-finite points from a wavefront ballot and a popcount, one atomic per wavefront and counter;
//   k_obj_compact  after scan_u32 over the non-ground flags: the non-ground rows, stably, and the source index of every one of them.
//                  Stable, so a cluster's lowest compacted index is its lowest original index.  No ground mask: skipped, the index map
//                  is the identity;
//   the grid, the forest and the unite over the compacted cloud: k_ev_hist / k_ev_offsets / k_ev_scatter and k_cl_unite as they are
//                  (k_obj_init: every point its own tree, this table's rows at their identities);
//   k_obj_table    root[j] and point j into its root's row, aggregated per wavefront as k_cl_table does: one atomic per distinct root
//                  and counter, the box of up to CL_BOX_ROUNDS shared roots reduced across the lanes first -- behind the ground mask
//                  the common input is one or a few enormous clusters and many small ones;
//   k_obj_decide   one root per lane: the decision in float64 as the contract words it, the touched flag, the clusters' totals;
//   k_obj_apply    after scan_u32 over the touched flags (compacted-index order is `first` order): one ORIGINAL point per lane, its mask
//                  byte, row index and keep flag; a non-ground point's compacted index is what the first scan left at its place.  The
//                  points' totals from ballots, one atomic per wavefront and counter;
//   k_obj_rows     the touched roots' rows, `first` mapped back through the index map;
//   the kept cloud is the project's stable compaction (k_f_compact) over the keep flags.
#ifndef ERASOR_OBJECTS_HIP_H
#define ERASOR_OBJECTS_HIP_H

namespace ek {

// a row of the table, per compacted index (used at the roots): the counts, the box's min / max keys (fkey_ord)
enum : uint32_t { OB_T_N = 0, OB_T_VOTED, OB_T_DYN, OB_T_VDYN, OB_T_OOR, OB_T_MIN, OB_T_MAX = OB_T_MIN + 3, OB_TROW = OB_T_MAX + 3 };
// a row as the caller gets it (erasor_object_row): first, n_points, n_voted, n_dynamic, n_voted_dynamic, n_label_out_of_range,
// min_xyz[3], max_xyz[3], decision
static constexpr uint32_t OB_ROW = 13;
enum : uint32_t {
    OB_C_VOTED = 0, OB_C_GROUND, OB_C_NON_FINITE, OB_C_CLUSTERS, OB_C_TOUCHED, OB_C_REMOVED_CL, OB_C_REVERTED_CL, OB_C_NOT_OBJECT, OB_C_LARGEST,
    OB_C_REMOVED, OB_C_GROWN, OB_C_GROWN_DYN, OB_C_REVERTED, OB_C_REVERTED_DYN, OB_C_GROUND_REV, OB_C_GROUND_REV_DYN, OB_NCTR
};
enum : uint32_t { OB_UNCHANGED = 0, OB_REMOVED = 1, OB_REVERTED = 2, OB_NOT_OBJECT = 3 };
enum : uint8_t { OB_CLS_VOTED = 1, OB_CLS_GROUND = 2 };
static constexpr uint32_t OB_NONE = 0xFFFFFFFFu;

struct ObDecide {
    uint32_t min_size, max_size, min_voted;  // min_size >= 1; max_size == 0: no upper limit
    double max_extent, remove_ratio, revert_ratio;
};

// the wavefront's count of `mine` from one ballot, added by lane 0 (every lane of the wavefront must call this)
__device__ __forceinline__ void ob_commit(unsigned long long *ctr, uint32_t which, bool mine) {
    const uint64_t m = __ballot(mine);
    if ((threadIdx.x & 63u) == 0 && m != 0ull) atomicAdd(&ctr[which], (unsigned long long)__popcll(m));
}

// (1) cls[i] = voted | ground << 1, ng[i] = point i is in the graph (ng may be NULL: no ground mask); ctr zeroed by the host
__global__ __launch_bounds__(256) void k_obj_flags(const float4 *__restrict__ pts, uint32_t n, const uint8_t *__restrict__ votes,
                                                    const uint8_t *__restrict__ ground, uint32_t vote_thr, uint8_t *__restrict__ cls,
                                                    uint32_t *__restrict__ ng, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool voted = false, gnd = false, bad = false;
    if (i < n) {
        voted = (uint32_t)votes[i] >= vote_thr;
        gnd = ground != nullptr && ground[i] != 0;
        bad = !ev_finite(pts[i]);
        cls[i] = (uint8_t)((voted ? OB_CLS_VOTED : 0) | (gnd ? OB_CLS_GROUND : 0));
        if (ng) ng[i] = gnd ? 0u : 1u;
    }
    ob_commit(ctr, OB_C_VOTED, voted);
    ob_commit(ctr, OB_C_GROUND, gnd);
    ob_commit(ctr, OB_C_NON_FINITE, bad);
}

// (2) after scan_u32 over ng: the rows in the graph, in the order given, and where each came from
__global__ __launch_bounds__(256) void k_obj_compact(const float4 *__restrict__ pts, uint32_t n, const uint32_t *__restrict__ ng,
                                                      const uint32_t *__restrict__ pl, const uint32_t *__restrict__ tops, float4 *__restrict__ dst,
                                                      uint32_t *__restrict__ src) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !ng[i]) return;
    const uint32_t s = pl[i] + tops[i >> 10];
    dst[s] = pts[i];
    src[s] = i;
}

// (3) every compacted point its own tree; the table's rows at their identities
__global__ __launch_bounds__(256) void k_obj_init(uint32_t m, uint32_t *__restrict__ parent, uint32_t *__restrict__ tab) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    parent[j] = j;
    uint32_t *r = tab + (size_t)j * OB_TROW;
    r[OB_T_N] = r[OB_T_VOTED] = r[OB_T_DYN] = r[OB_T_VDYN] = r[OB_T_OOR] = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        r[OB_T_MIN + c] = 0xFFFFFFFFu;
        r[OB_T_MAX + c] = 0u;
    }
}

// (4) root[j], and compacted point j into its root's row (src NULL: the index map is the identity).  Every lane of the wavefront stays
// to the end.
__global__ __launch_bounds__(256) void k_obj_table(const float4 *__restrict__ pts, uint32_t m, const uint32_t *__restrict__ parent,
                                                    const uint8_t *__restrict__ cls, const uint32_t *__restrict__ src, uint32_t *__restrict__ root,
                                                    uint32_t *__restrict__ tab) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = j < m;
    uint32_t r = 0, oor = 0, k[3] = {0u, 0u, 0u};
    bool dyn = false, voted = false;
    if (valid) {
        r = j;
        for (uint32_t q = parent[r]; q != r; q = parent[r]) r = q;
        root[j] = r;
        const float4 p = pts[j];
        dyn = ev_is_dynamic(p.w, oor);
        voted = (cls[src ? src[j] : j] & OB_CLS_VOTED) != 0;
        k[0] = fkey_ord(p.x), k[1] = fkey_ord(p.y), k[2] = fkey_ord(p.z);
    }
    const uint64_t peers = match_any(r, valid, 32);
    const uint64_t m_dyn = __ballot(valid && dyn), m_oor = __ballot(valid && oor != 0u), m_vot = __ballot(valid && voted);
    if (valid && (peers & lanemask_lt()) == 0ull) {
        uint32_t *row = tab + (size_t)r * OB_TROW;
        const uint32_t nv = (uint32_t)__popcll(peers & m_vot), nd = (uint32_t)__popcll(peers & m_dyn), no = (uint32_t)__popcll(peers & m_oor),
                       nvd = (uint32_t)__popcll(peers & m_vot & m_dyn);
        atomicAdd(&row[OB_T_N], (uint32_t)__popcll(peers));
        if (nv) atomicAdd(&row[OB_T_VOTED], nv);
        if (nd) atomicAdd(&row[OB_T_DYN], nd);
        if (nvd) atomicAdd(&row[OB_T_VDYN], nvd);
        if (no) atomicAdd(&row[OB_T_OOR], no);
    }
    bool pending = valid;
    uint64_t todo = __ballot(valid && __popcll(peers) > 1);
    for (int round = 0; todo != 0ull && round < CL_BOX_ROUNDS; ++round) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const uint32_t rk = __builtin_amdgcn_readlane(r, lead);
        const bool in = valid && r == rk;
        const uint64_t mk = __ballot(in);
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            const uint32_t mn = wave_minmax_u<false>(in ? k[c] : 0xFFFFFFFFu), mx = wave_minmax_u<true>(in ? k[c] : 0u);
            if (lane == lead) {
                atomicMin(&tab[(size_t)rk * OB_TROW + OB_T_MIN + c], mn);
                atomicMax(&tab[(size_t)rk * OB_TROW + OB_T_MAX + c], mx);
            }
        }
        if (in) pending = false;
        todo &= ~mk;
    }
    if (pending) {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            atomicMin(&tab[(size_t)r * OB_TROW + OB_T_MIN + c], k[c]);
            atomicMax(&tab[(size_t)r * OB_TROW + OB_T_MAX + c], k[c]);
        }
    }
}

// the decision of the cluster whose table row is t, in the contract's order
__device__ __forceinline__ uint32_t ob_decision(const uint32_t *t, const ObDecide &d) {
    const uint32_t n = t[OB_T_N], nv = t[OB_T_VOTED];
    bool gate = n < d.min_size || (d.max_size != 0u && n > d.max_size);
    if (d.max_extent > 0.0) {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c)
            gate = gate || ((double)fkey_inv(t[OB_T_MAX + c]) - (double)fkey_inv(t[OB_T_MIN + c]) > d.max_extent);
    }
    if (gate) return OB_NOT_OBJECT;
    const double dn = (double)n, dv = (double)nv;
    if (nv >= d.min_voted && dv >= d.remove_ratio * dn) return OB_REMOVED;
    if (nv > 0u && dv <= d.revert_ratio * dn) return OB_REVERTED;
    return OB_UNCHANGED;
}

// (5) code[j] = the decision of the cluster rooted at j, touched[j] = j is the root of a touched cluster; the clusters' totals
__global__ __launch_bounds__(256) void k_obj_decide(uint32_t m, const uint32_t *__restrict__ root, const uint32_t *__restrict__ tab, ObDecide d,
                                                     uint32_t *__restrict__ code, uint32_t *__restrict__ touched,
                                                     unsigned long long *__restrict__ ctr) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    bool is_root = false, tch = false;
    uint32_t dec = OB_UNCHANGED, cnt = 0;
    if (j < m) {
        is_root = root[j] == j;
        if (is_root) {
            const uint32_t *t = tab + (size_t)j * OB_TROW;
            cnt = t[OB_T_N];
            tch = t[OB_T_VOTED] != 0u;
            dec = ob_decision(t, d);
        }
        code[j] = dec;
        touched[j] = tch ? 1u : 0u;
    }
    ob_commit(ctr, OB_C_CLUSTERS, is_root);
    ob_commit(ctr, OB_C_TOUCHED, tch);
    ob_commit(ctr, OB_C_REMOVED_CL, tch && dec == OB_REMOVED);
    ob_commit(ctr, OB_C_REVERTED_CL, tch && dec == OB_REVERTED);
    ob_commit(ctr, OB_C_NOT_OBJECT, tch && dec == OB_NOT_OBJECT);
    const uint32_t big = wave_minmax_u<true>(cnt);
    if ((threadIdx.x & 63u) == 0 && big) atomicMax(&ctr[OB_C_LARGEST], (unsigned long long)big);
}

// (6) after scan_u32 over touched (tpl / ttops): one ORIGINAL point per lane.  ng / gpl / gtops: the first scan (NULL: no ground mask,
// the compacted index is the point's own).  mask[i] = 1 kept / 0 removed, ids[i] = its cluster's row or OB_NONE, keep[i] = mask as a
// flag for the kept cloud's compaction; the points' totals.
__global__ __launch_bounds__(256) void k_obj_apply(const float4 *__restrict__ pts, uint32_t n, const uint8_t *__restrict__ cls,
                                                    const uint32_t *__restrict__ gpl, const uint32_t *__restrict__ gtops, const uint32_t *__restrict__ root,
                                                    const uint32_t *__restrict__ code, const uint32_t *__restrict__ touched,
                                                    const uint32_t *__restrict__ tpl, const uint32_t *__restrict__ ttops, uint32_t ground_keep,
                                                    uint8_t *__restrict__ mask, uint32_t *__restrict__ ids, uint32_t *__restrict__ keep,
                                                    unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    bool voted = false, gnd = false, kept = true, dyn = false;
    if (valid) {
        const uint8_t c = cls[i];
        voted = (c & OB_CLS_VOTED) != 0, gnd = (c & OB_CLS_GROUND) != 0;
        uint32_t oor = 0, id = OB_NONE;
        dyn = ev_is_dynamic(pts[i].w, oor);
        if (gnd) {
            kept = ground_keep != 0u || !voted;
        } else {
            const uint32_t j = gpl ? gpl[i] + gtops[i >> 10] : i;
            const uint32_t r = root[j], dec = code[r];
            kept = dec == OB_REMOVED ? false : dec == OB_REVERTED ? true : !voted;
            if (touched[r]) id = tpl[r] + ttops[r >> 10];
        }
        mask[i] = kept ? 1 : 0;
        ids[i] = id;
        keep[i] = kept ? 1u : 0u;
    }
    const bool grown = valid && !voted && !kept, rev = valid && voted && !gnd && kept, grev = valid && voted && gnd && kept;
    ob_commit(ctr, OB_C_REMOVED, valid && !kept);
    ob_commit(ctr, OB_C_GROWN, grown);
    ob_commit(ctr, OB_C_GROWN_DYN, grown && dyn);
    ob_commit(ctr, OB_C_REVERTED, rev);
    ob_commit(ctr, OB_C_REVERTED_DYN, rev && dyn);
    ob_commit(ctr, OB_C_GROUND_REV, grev);
    ob_commit(ctr, OB_C_GROUND_REV_DYN, grev && dyn);
}

// (7) the touched roots' rows in `first` order (src NULL: the index map is the identity)
__global__ __launch_bounds__(256) void k_obj_rows(uint32_t m, const uint32_t *__restrict__ touched, const uint32_t *__restrict__ tpl,
                                                   const uint32_t *__restrict__ ttops, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ code,
                                                   const uint32_t *__restrict__ src, uint32_t *__restrict__ rows) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || !touched[j]) return;
    const uint32_t *t = tab + (size_t)j * OB_TROW;
    uint32_t *o = rows + (size_t)(tpl[j] + ttops[j >> 10]) * OB_ROW;
    o[0] = src ? src[j] : j;
    o[1] = t[OB_T_N];
    o[2] = t[OB_T_VOTED];
    o[3] = t[OB_T_DYN];
    o[4] = t[OB_T_VDYN];
    o[5] = t[OB_T_OOR];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        o[6 + c] = __float_as_uint(fkey_inv(t[OB_T_MIN + c]));
        o[9 + c] = __float_as_uint(fkey_inv(t[OB_T_MAX + c]));
    }
    o[12] = code[j];
}

}  // namespace ek

#endif  // ERASOR_OBJECTS_HIP_H
