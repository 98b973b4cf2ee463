// cluster.hip.h — Euclidean clustering of a cloud: the connected components of "closer than tol", listed and filtered by size
// (erasor_hip_cluster_clouds / _map).  What users of a cleaned map do next on the host with a KD-tree and a region-growing loop
// (pcl::EuclideanClusterExtraction): what a run removed as objects, the small floating fragments it left (drop every cluster below n
// points), how many ghost objects remain rather than how many ghost points.
//
// The contract (restated on the host by erasor_amd/evalmap.py, cluster / cluster_brute; the device equals it byte for byte):
//   * points i and j are adjacent iff ((dx*dx + dy*dy) + dz*dz) <= tol*tol with dx = (double)x_i - (double)x_j (dy, dz alike), all in
//     float64, left to right, no fused multiply-add: symmetric bit for bit;
//   * a cluster is a connected component of that graph, named by `first`, the lowest point index it contains;
//   * a cluster is listed when min_size <= n_points and (max_size == 0 or n_points <= max_size); one row per listed cluster in
//     increasing `first`: the counts and the bounding box, taken in float32's total order (-0.0 below +0.0), the floats as bits.
// No centroid: a float sum depends on the order of its terms, a box and a count do not -- nothing here depends on scheduling.
// Up to the metric at the very edge d == tol this is the partition pcl::EuclideanClusterExtraction's region growing produces (PCL
// measures in float32); PCL is not a dependency of this project and the contract is not pinned against it.
//
// Grid.  The points are bucketed by evaluate.hip.h's builders (k_ev_hist, the scan, k_ev_offsets, k_ev_scatter) at the cell edge
// CL_CELL_MARGIN * tol, and a point tests the 27 cells around its own.  Hash collisions and the 2^30 clamp only add candidates: the
// predicate decides.  The margin -- see CL_CELL_MARGIN -- is what makes 27 cells enough although floor((double)v / cell) is rounded.
//
// Unite (k_cl_unite): one point per lane, candidates of LOWER original index only (each adjacent pair is met once, by its higher
// point).  parent[] is a union-find forest with parent[x] <= x throughout: a union hooks the LARGER root under the smaller one with an
// atomicCAS that succeeds only while that root still is a root, so the root of a finished component is its lowest index.  find halves
// paths with atomicMin (a parent only ever decreases, to an ancestor).  No lane waits for another: a union retries only after its own
// CAS failed, which means somebody else hooked that root -- the number of roots and the parent values only go down, which bounds
// every loop by the data.  parent[] is written by other workgroups, on other XCDs, during the launch: every read of it in there is an
// agent-scope atomic load (cl_load), never a plain one; behind the kernel boundary plain loads are fine.
//
// Known hazard, stated and not solved: the unite pass tests all pairs inside a cell neighbourhood, so an unvoxelised cloud with
// thousands of points per tol-cell is quadratic there.
//
// Then: k_cl_table flattens (root[i] = find(i), plain loads) and accumulates the table on the root's row -- counts by atomicAdd, the box
// by atomicMin / atomicMax on fkey_ord keys, aggregated per wavefront where lanes share a root --; k_cl_flags decides the listed
// clusters and the result's counters; an exclusive scan of the flags ranks them, k_cl_rows writes the rows in `first` order, k_cl_ids
// every point's row index; the kept cloud is the project's stable compaction (k_f_compact).
#ifndef ERASOR_CLUSTER_HIP_H
#define ERASOR_CLUSTER_HIP_H

namespace ek {

// The cell edge is CL_CELL_MARGIN * tol = (1 + 2^-10) * tol.  Why 27 cells then suffice: an adjacent pair has fl(dx*dx) <= fl(tol*tol)
// (sums of non-negative terms round monotonically), so the computed |dx| <= tol * (1 + 2^-52), and the exact difference of the two
// coordinates, which the subtraction rounded by 2^-53 at most, is <= tol * (1 + 2^-51).  Its two quotients v / cell differ by at most
// (1 + 2^-51) / (1 + 2^-10) < 1 - 2^-10 + 2^-19 in exact arithmetic; each is rounded with a relative error of 2^-53, and below the
// clamp |v / cell| <= 2^30 + 2, so each moves by less than 2^-22 (the clamp itself never widens a difference).  The rounded quotients
// therefore differ by less than 1 - 2^-10 + 2^-19 + 2^-21 < 1, and floor() of two numbers less than 1 apart differs by at most 1.
// An edge of exactly tol has no such room: at tol = 0.5 the points -1.4e-45 and 0.5 are adjacent (their difference rounds to 0.5) and
// lie in cells -1 and 1.
static constexpr double CL_CELL_MARGIN = 1.0009765625;

// a row of the table, per point index (used at the roots): count, dynamic, labels out of range, the box's min / max keys (fkey_ord)
enum : uint32_t { CL_T_N = 0, CL_T_DYN, CL_T_OOR, CL_T_MIN, CL_T_MAX = CL_T_MIN + 3, CL_TROW = CL_T_MAX + 3 };
// a row as the caller gets it (erasor_cluster_row): first, n_points, n_dynamic, n_label_out_of_range, min_xyz[3], max_xyz[3]
static constexpr uint32_t CL_ROW = 10;
enum : uint32_t { CL_C_CLUSTERS = 0, CL_C_LISTED, CL_C_POINTS_LISTED, CL_C_SINGLETONS, CL_C_LARGEST, CL_NCTR };
static constexpr uint32_t CL_NONE = 0xFFFFFFFFu;
static constexpr int CL_BOX_ROUNDS = 8;  // root groups of a wavefront whose box is reduced across lanes; lanes of further groups add their own

// parent[] inside k_cl_unite: written by other workgroups during the launch, so read at agent scope (a host compiler has no scopes)
__device__ __forceinline__ uint32_t cl_load(const uint32_t *p) {
#if defined(__HIPCC__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// the root of x's tree, halving the path on the way (parent[x] only decreases, to an ancestor of x)
__device__ __forceinline__ uint32_t cl_find(uint32_t *parent, uint32_t x) {
    uint32_t p = cl_load(&parent[x]);
    while (p != x) {
        const uint32_t gp = cl_load(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

// one tree out of a's and b's: the larger root under the smaller.  A failed CAS means another lane hooked that root: go on from there.
__device__ __forceinline__ void cl_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(&parent[hi], hi, lo);
        if (old == hi) return;
        a = old;  // (an ancestor-to-be of hi, below it)
        b = lo;
    }
}

// (1) every point its own tree; the table's rows at their identities
__global__ __launch_bounds__(256) void k_cl_init(uint32_t n, uint32_t *__restrict__ parent, uint32_t *__restrict__ tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    uint32_t *r = tab + (size_t)i * CL_TROW;
    r[CL_T_N] = r[CL_T_DYN] = r[CL_T_OOR] = 0u;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        r[CL_T_MIN + c] = 0xFFFFFFFFu;
        r[CL_T_MAX + c] = 0u;
    }
}

// (2) one point per lane against the bucketed points (bpts / idx / off: k_ev_scatter's) of the 27 cells around its own, lower indices only
__global__ __launch_bounds__(256) void k_cl_unite(const float4 *__restrict__ pts, uint32_t n, const float4 *__restrict__ bpts,
                                                   const uint32_t *__restrict__ idx, const uint32_t *__restrict__ off, uint32_t mask, double cell,
                                                   double tol2, uint32_t *parent) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    const int32_t cx = ev_cell(p.x, cell), cy = ev_cell(p.y, cell), cz = ev_cell(p.z, cell);
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t b = ev_bucket(cx + dx, cy + dy, cz + dz, mask);
                const uint32_t e = off[b + 1];
                for (uint32_t s = off[b]; s < e; ++s) {
                    const uint32_t j = idx[s];
                    if (j >= i) continue;
                    const float4 q = bpts[s];
                    const double ex = px - (double)q.x, ey = py - (double)q.y, ez = pz - (double)q.z;
                    if ((ex * ex + ey * ey) + ez * ez <= tol2) cl_unite(parent, i, j);  // (NaN: never adjacent)
                }
            }
}

// (3) root[i], and point i into its root's row: one atomicAdd per distinct root of the wavefront and counter; the box of up to
// CL_BOX_ROUNDS roots shared by several lanes is reduced across the wavefront first, every other lane adds its own key.  Every lane of
// the wavefront stays to the end.
__global__ __launch_bounds__(256) void k_cl_table(const float4 *__restrict__ pts, uint32_t n, const uint32_t *__restrict__ parent,
                                                   uint32_t *__restrict__ root, uint32_t *__restrict__ tab) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = i < n;
    uint32_t r = 0, oor = 0, k[3] = {0u, 0u, 0u};
    bool dyn = false;
    if (valid) {
        r = i;
        for (uint32_t q = parent[r]; q != r; q = parent[r]) r = q;
        root[i] = r;
        const float4 p = pts[i];
        dyn = ev_is_dynamic(p.w, oor);
        k[0] = fkey_ord(p.x), k[1] = fkey_ord(p.y), k[2] = fkey_ord(p.z);
    }
    const uint64_t peers = match_any(r, valid, 32);
    const uint64_t m_dyn = __ballot(valid && dyn), m_oor = __ballot(valid && oor != 0u);
    if (valid && (peers & lanemask_lt()) == 0ull) {
        uint32_t *row = tab + (size_t)r * CL_TROW;
        const uint32_t nd = (uint32_t)__popcll(peers & m_dyn), no = (uint32_t)__popcll(peers & m_oor);
        atomicAdd(&row[CL_T_N], (uint32_t)__popcll(peers));
        if (nd) atomicAdd(&row[CL_T_DYN], nd);
        if (no) atomicAdd(&row[CL_T_OOR], no);
    }
    bool pending = valid;
    uint64_t todo = __ballot(valid && __popcll(peers) > 1);
    for (int round = 0; todo != 0ull && round < CL_BOX_ROUNDS; ++round) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const uint32_t rk = __builtin_amdgcn_readlane(r, lead);
        const bool in = valid && r == rk;
        const uint64_t m = __ballot(in);
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            const uint32_t mn = wave_minmax_u<false>(in ? k[c] : 0xFFFFFFFFu), mx = wave_minmax_u<true>(in ? k[c] : 0u);
            if (lane == lead) {
                atomicMin(&tab[(size_t)rk * CL_TROW + CL_T_MIN + c], mn);
                atomicMax(&tab[(size_t)rk * CL_TROW + CL_T_MAX + c], mx);
            }
        }
        if (in) pending = false;
        todo &= ~m;
    }
    if (pending) {
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            atomicMin(&tab[(size_t)r * CL_TROW + CL_T_MIN + c], k[c]);
            atomicMax(&tab[(size_t)r * CL_TROW + CL_T_MAX + c], k[c]);
        }
    }
}

// (4) flag[i] = point i is the root of a listed cluster; the result's counters (ctr: [CL_NCTR], zeroed by the host).  min_size >= 1;
// max_size == 0: no upper limit.
__global__ __launch_bounds__(256) void k_cl_flags(uint32_t n, const uint32_t *__restrict__ root, const uint32_t *__restrict__ tab, uint32_t min_size,
                                                   uint32_t max_size, uint32_t *__restrict__ flag, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t is_root = 0, listed = 0, cnt = 0;
    if (i < n) {
        is_root = root[i] == i ? 1u : 0u;
        cnt = is_root ? tab[(size_t)i * CL_TROW + CL_T_N] : 0u;
        listed = (is_root && min_size <= cnt && (max_size == 0u || cnt <= max_size)) ? 1u : 0u;
        flag[i] = listed;
    }
    ev_commit(ctr, CL_C_CLUSTERS, is_root);
    ev_commit(ctr, CL_C_LISTED, listed);
    ev_commit(ctr, CL_C_POINTS_LISTED, listed ? cnt : 0u);
    ev_commit(ctr, CL_C_SINGLETONS, cnt == 1u ? 1u : 0u);
    const uint32_t big = wave_minmax_u<true>(cnt);
    if ((threadIdx.x & 63u) == 0 && big) atomicMax(&ctr[CL_C_LARGEST], (unsigned long long)big);
}

// (5) after scan_u32 over the flags: the listed roots' rows in `first` order, and lrank[i] = the row of root i (CL_NONE: not listed)
__global__ __launch_bounds__(256) void k_cl_rows(uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pl,
                                                  const uint32_t *__restrict__ tops, const uint32_t *__restrict__ tab, uint32_t *__restrict__ rows,
                                                  uint32_t *__restrict__ lrank) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!flag[i]) {
        lrank[i] = CL_NONE;
        return;
    }
    const uint32_t r = pl[i] + tops[i >> 10];
    lrank[i] = r;
    const uint32_t *t = tab + (size_t)i * CL_TROW;
    uint32_t *o = rows + (size_t)r * CL_ROW;
    o[0] = i;
    o[1] = t[CL_T_N];
    o[2] = t[CL_T_DYN];
    o[3] = t[CL_T_OOR];
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
        o[4 + c] = __float_as_uint(fkey_inv(t[CL_T_MIN + c]));
        o[7 + c] = __float_as_uint(fkey_inv(t[CL_T_MAX + c]));
    }
}

// (6) ids[i] = the row of point i's cluster (CL_NONE: not listed), keep[i] = it has one (the kept cloud's flags)
__global__ __launch_bounds__(256) void k_cl_ids(uint32_t n, const uint32_t *__restrict__ root, const uint32_t *__restrict__ lrank,
                                                 uint32_t *__restrict__ ids, uint32_t *__restrict__ keep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = lrank[root[i]];
    ids[i] = r;
    keep[i] = r != CL_NONE ? 1u : 0u;
}

}  // namespace ek

#endif  // ERASOR_CLUSTER_HIP_H
