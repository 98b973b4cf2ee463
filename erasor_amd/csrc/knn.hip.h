// knn.hip.h — every point's k nearest neighbours inside its own cloud, the number of points within a radius of it, and the density
// filters built on both (erasor_hip_knn_* / erasor_hip_radius_count_* / erasor_hip_density_filter_*).  What users of a cleaned map do
// next on the host with a KD-tree over the whole map: pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval, to drop the single
// returns in the air, the thin shells dynamic removal leaves behind and the stray centroids at the rim of a reverted bin.
//
// The contract (restated on the host by erasor_amd/evalmap.py: knn / knn_brute, radius_count / radius_count_brute, density_filter -- the
// host restatement; the device equals it byte for byte):
//   * distance: ex = (double)x_i - (double)x_j (ey, ez alike), d2 = (ex*ex + ey*ey) + ez*ez in float64, left to right, no fused
//     multiply-add; d = sqrt(d2), correctly rounded;
//   * the neighbour order of point i: every j != i by (d2, j) ascending -- a total order, so "the k nearest" is one defined list under
//     any number of ties and duplicates.  Self is excluded by INDEX: an identical point at another index is a neighbour at distance 0;
//   * knn, 1 <= k <= 32: the first k entries of that order; kth = the k-th distance; mean = (((0.0 + d_0) + d_1) + ... + d_{k-1}) /
//     (double)k, summed in list order.  A point with fewer than k other points has its missing entries padded with index 0xFFFFFFFF and
//     distance +inf, kth = mean = +inf, and is counted in n_short;
//   * radius count: the number of j != i with d2 <= r*r (r*r formed once, in float64);
//   * the statistics of a score (min, median, p90, p99, max) are exact order statistics over the finite scores, taken as the overlap
//     report takes them (nearest.hip.h: the radix select, numpy's interpolation);
//   * the filters keep a point iff score <= thr (never an infinite score; a NaN thr keeps nothing), thr given (ABS) or thr = m + mul *
//     (1.4826 * mad) from the median m and the median absolute deviation mad of the finite scores (MAD), or iff count >= min_neighbors.
// Not offered: PCL's mean + mul * sigma.  Sigma is a float sum whose value depends on the order of its terms; a median and a MAD do
// not, so nothing here depends on scheduling.  Up to that rule and PCL's float32 metric, MEAN / MAD is StatisticalOutlierRemoval's
// selection and COUNT is RadiusOutlierRemoval's; PCL is not a dependency of this project and nothing is pinned against it.
//
// Search (k_kn_query).  The tree is nearest.hip.h's, built by its builders over the cloud itself.  One query per lane, taken in the
// tree's sorted (Morton) order so that a wavefront walks neighbouring leaves; results go to the point's original index.  The traversal
// is nearest.hip.h's nn_walk (depth first, nearer child first, the pending siblings on a per-lane stack), at the stride KN_QBLOCK; the
// visitor KnList keeps the lane's k best (d2, j) sorted ascending; a candidate enters when it is lexicographically below the list's
// last entry (or the list is not full), by insertion from the end.  Its bound is the list's last d2 once the list is FULL, so a node is
// pruned only then, and only when the node's lower bound is STRICTLY greater.
//
// Why that is exact, with no epsilon (nn_walk's argument, for k): the bound, the list's last d2, only decreases.  A point that belongs
// to the final list has d2 <= the final last d2 <= the last d2 at any moment, so a box pruned on lb > last d2 holds no such point; and
// because the prune is strict, every point AT the k-th d2 is visited, so among equal d2 the index decides.  While the list is not full
// the bound is +inf and nothing is pruned: any point may still be needed.
//
// Where the list lives.  List and stack are indexed at run time; a per-thread array would go to scratch memory.  They are LDS arrays,
// lane-minor ([entry][lane]: consecutive lanes in consecutive banks).  An entry is 12 B (d2 as float64, j as uint32), the stack
// NN_STACK words.  The kernel is instantiated by k class (k <= 8, <= 16, <= 32) at KN_QBLOCK = 128 lanes, so a small k does not pay for 32
// entries: per workgroup 128 * (KC * 12 + 26 * 4) B = 25 600 / 37 888 / 62 464 B, which by arithmetic against the CU's 163 840 B of LDS
// is 6 / 4 / 2 workgroups (12 / 8 / 4 wavefronts) per CU.  (256 lanes at k = 32 would be 124 928 B: one workgroup per CU, the same 4
// wavefronts in one piece.)
//
// Finish: at the end of the search the lane walks its sorted list once: d = sqrt(d2), the sequential sum, kth, mean, and, when asked for,
// the neighbour lists at the point's original index.
//
// Radius count (k_kn_count): one point per lane over the 27 cells of evaluate.hip.h's hashed grid at the cell edge CL_CELL_MARGIN * r;
// cluster.hip.h's margin argument carries over word for word (the predicate is the same).  All j != i are counted, not only lower
// indices -- and counted ONCE: two of the 27 cells may hash to the same bucket, so a bucket that an earlier cell of the 27 named is
// skipped.  Other cells' points in a bucket are only more candidates: the predicate decides.
//
// Known hazards, stated and not solved: the count tests every point of a cell neighbourhood, so thousands of points per
// r-cell are quadratic there, as in cluster.hip.h; and m identical points make every one of them visit all m in the search, because
// the strict prune visits every tie.
#ifndef ERASOR_KNN_HIP_H
#define ERASOR_KNN_HIP_H

namespace ek {

static constexpr uint32_t KN_QBLOCK = 128;  // lanes per workgroup of k_kn_query
static constexpr uint32_t KN_MAX_K = 32;
static constexpr uint32_t KN_NONE = 0xFFFFFFFFu;

// counters of one call (zeroed by the host, the *_MIN ones set to all ones): one 64-bit atomic per wavefront and counter
enum : uint32_t {
    KN_C_SHORT = 0,    // points with fewer than k other points
    KN_C_KTH_MIN,      // the smallest / largest finite score's bit pattern (scores are >= +0: unsigned order is numeric order)
    KN_C_KTH_MAX,
    KN_C_MEAN_MIN,
    KN_C_MEAN_MAX,
    KN_C_KEPT,         // the filter: points kept, points removed by label
    KN_C_REMOVED_DYNAMIC,
    KN_C_REMOVED_STATIC,
    KN_NCTR
};

// the wavefront's smallest and largest bit pattern among the lanes with `valid` into ctr[lo_at] / ctr[hi_at]: the high words first, then
// the low words of the lanes that hold that high word (every lane of the wavefront must call this)
__device__ __forceinline__ void kn_commit_range(unsigned long long *ctr, uint32_t lo_at, uint32_t hi_at, unsigned long long bits, bool valid) {
    const uint32_t h = (uint32_t)(bits >> 32), l = (uint32_t)bits;
    const bool any = __ballot(valid) != 0ull;
    const uint32_t xh = wave_minmax_u<true>(valid ? h : 0u);
    const uint32_t xl = wave_minmax_u<true>(valid && h == xh ? l : 0u);
    const uint32_t nh = wave_minmax_u<false>(valid ? h : 0xFFFFFFFFu);
    const uint32_t nl = wave_minmax_u<false>(valid && h == nh ? l : 0xFFFFFFFFu);
    if ((threadIdx.x & 63u) == 0 && any) {
        atomicMax(&ctr[hi_at], ((unsigned long long)xh << 32) | xl);
        atomicMin(&ctr[lo_at], ((unsigned long long)nh << 32) | nl);
    }
}

// visitor: the k best (d2, j) of the query at sorted position s, ascending in the lane's column t of the LDS list ld / li
// ([entry][KN_QBLOCK]).  The bound is the list's last d2 once the list is full and +inf before: nothing is pruned, everything enters.
// (It carries no effort counters: no test hook reads this search's.)
struct KnList {
    typedef double real;
    static constexpr bool FIXED = false;
    double qx, qy, qz;
    uint32_t s, k, t;
    double *ld;
    uint32_t *li;
    uint32_t cnt = 0, worst_j = KN_NONE;
    double worst = __builtin_huge_val();
    __device__ __forceinline__ double lb(const float4 &l, const float4 &u) const { return nn_lb(l, u, qx, qy, qz); }
    __device__ __forceinline__ double bound() const { return worst; }
    // a leaf's points, except the query itself (by position, which is by index)
    __device__ __forceinline__ bool leaf(const NnTree &T, uint32_t b, uint32_t e) {
        for (uint32_t c = b; c < e; ++c) {
            if (c == s) continue;
            const float4 p = T.pts[c];
            const double ex = qx - (double)p.x, ey = qy - (double)p.y, ez = qz - (double)p.z;
            const double d2 = (ex * ex + ey * ey) + ez * ez;
            if (!(d2 <= worst)) continue;
            const uint32_t j = T.idx[c];
            if (cnt == k && d2 == worst && j > worst_j) continue;
            // insertion from the end: the entries above (d2, j) move up one place, the last one drops out when the list is full.  The
            // loop walks the new entry's place in the lane's column (entry * KN_QBLOCK + t), not the entry number: with the number the
            // compiler keeps apart the loop's two exits and the search is 4 % slower at k = 8 (MEASUREMENTS.md, Density)
            uint32_t at = (cnt < k ? cnt : k - 1) * KN_QBLOCK + t;
            while (at >= KN_QBLOCK) {
                const double pd = ld[at - KN_QBLOCK];
                const uint32_t pj = li[at - KN_QBLOCK];
                if (pd < d2 || (pd == d2 && pj < j)) break;
                ld[at] = pd;
                li[at] = pj;
                at -= KN_QBLOCK;
            }
            ld[at] = d2;
            li[at] = j;
            if (cnt < k) ++cnt;
            if (cnt == k) {
                worst = ld[(k - 1) * KN_QBLOCK + t];
                worst_j = li[(k - 1) * KN_QBLOCK + t];
            }
        }
        return false;
    }
};

// One query per lane, in the tree's sorted order: lane s asks for the k nearest other points of T.pts[s] (original index T.idx[s]).  T:
// the tree nearest.hip.h built over the cloud (T.n > 0, every point finite).  kth_bits / mean_bits: the two scores'
// bit patterns at the point's original index; nbr_idx / nbr_dist ([n][k], optional): its neighbour lists.  KC: the list's capacity, k <= KC.
template <uint32_t KC>
__global__ __launch_bounds__(KN_QBLOCK) void k_kn_query(NnTree T, uint32_t k, unsigned long long *__restrict__ kth_bits,
                                                         unsigned long long *__restrict__ mean_bits, uint32_t *__restrict__ nbr_idx,
                                                         double *__restrict__ nbr_dist, unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * KN_QBLOCK];  // [depth][lane]
    __shared__ double ld[KC * KN_QBLOCK];              // [entry][lane]: the list's d2 ...
    __shared__ uint32_t li[KC * KN_QBLOCK];            // ... and original index
    const uint32_t t = threadIdx.x, s = blockIdx.x * KN_QBLOCK + t;
    uint32_t is_short = 0;
    unsigned long long kb = 0ull, mb = 0ull;
    bool scored = false;
    if (s < T.n) {
        const float4 q = T.pts[s];
        const uint32_t self = T.idx[s];
        KnList v{(double)q.x, (double)q.y, (double)q.z, s, k, t, ld, li};
        nn_walk<KN_QBLOCK>(v, T, stack, t);
        const uint32_t cnt = v.cnt;
        // the finishing pass over the sorted list: distances, the sequential sum, the padding
        double sum = 0.0, last = __builtin_huge_val();
        for (uint32_t e = 0; e < k; ++e) {
            const bool have = e < cnt;
            const double d = have ? sqrt(ld[e * KN_QBLOCK + t]) : __builtin_huge_val();
            if (have) {
                sum = sum + d;
                last = d;
            }
            if (nbr_idx) nbr_idx[(size_t)self * k + e] = have ? li[e * KN_QBLOCK + t] : KN_NONE;
            if (nbr_dist) nbr_dist[(size_t)self * k + e] = d;
        }
        is_short = cnt < k ? 1u : 0u;
        scored = !is_short;
        const double kth = scored ? last : __builtin_huge_val(), mean = scored ? sum / (double)k : __builtin_huge_val();
        kb = __builtin_bit_cast(unsigned long long, kth);
        mb = __builtin_bit_cast(unsigned long long, mean);
        kth_bits[self] = kb;
        mean_bits[self] = mb;
    }
    ev_commit(ctr, KN_C_SHORT, is_short);
    kn_commit_range(ctr, KN_C_KTH_MIN, KN_C_KTH_MAX, kb, scored);
    kn_commit_range(ctr, KN_C_MEAN_MIN, KN_C_MEAN_MAX, mb, scored);
}

// One point per lane against the bucketed points (bpts / idx / off: k_ev_scatter's, at the cell edge CL_CELL_MARGIN * r) of the 27 cells
// around its own: count[i] = the number of j != i with d2 <= r2, and the same as a float64 bit pattern in score_bits[i].
__global__ __launch_bounds__(256) void k_kn_count(const float4 *__restrict__ pts, uint32_t n, const float4 *__restrict__ bpts,
                                                   const uint32_t *__restrict__ idx, const uint32_t *__restrict__ off, uint32_t mask, double cell,
                                                   double r2, uint32_t *__restrict__ count, unsigned long long *__restrict__ score_bits,
                                                   unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bits = 0ull;
    if (i < n) {
        const float4 p = pts[i];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        const int32_t cx = ev_cell(p.x, cell), cy = ev_cell(p.y, cell), cz = ev_cell(p.z, cell);
        uint32_t bk[27];  // (every loop over it is unrolled: registers, not scratch)
#pragma unroll
        for (int c = 0; c < 27; ++c) bk[c] = ev_bucket(cx + c % 3 - 1, cy + (c / 3) % 3 - 1, cz + c / 9 - 1, mask);
        uint32_t m = 0;
#pragma unroll
        for (int c = 0; c < 27; ++c) {
            bool seen = false;  // a bucket an earlier cell named has been counted already
#pragma unroll
            for (int c2 = 0; c2 < c; ++c2) seen = seen || bk[c2] == bk[c];
            if (seen) continue;
            const uint32_t e = off[bk[c] + 1];
            for (uint32_t s = off[bk[c]]; s < e; ++s) {
                if (idx[s] == i) continue;
                const float4 q = bpts[s];
                const double ex = px - (double)q.x, ey = py - (double)q.y, ez = pz - (double)q.z;
                if ((ex * ex + ey * ey) + ez * ez <= r2) ++m;
            }
        }
        count[i] = m;
        bits = __builtin_bit_cast(unsigned long long, (double)m);
        score_bits[i] = bits;
    }
    kn_commit_range(ctr, KN_C_KTH_MIN, KN_C_KTH_MAX, bits, i < n);
}

// dev[i] = |score_i - m| as a bit pattern; +inf where the score is not finite (above every rank of the select over the scored points)
__global__ __launch_bounds__(256) void k_kn_absdev(const unsigned long long *__restrict__ score_bits, uint32_t n, double m,
                                                    unsigned long long *__restrict__ dev) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = __builtin_bit_cast(double, score_bits[i]);
    dev[i] = __builtin_bit_cast(unsigned long long, isfinite(s) ? fabs(s - m) : __builtin_huge_val());
}

// The filter's decision per point: by_count ? count[i] >= min_neighbors : the score is finite and <= thr (a NaN thr keeps nothing).
// flag (uint32, for the compaction's scan) and mask (uint8, the caller's); kept and removed-by-label counters per wavefront.
__global__ __launch_bounds__(256) void k_kn_keep(const float4 *__restrict__ pts, uint32_t n, const unsigned long long *__restrict__ score_bits,
                                                  const uint32_t *__restrict__ count, uint32_t by_count, double thr, uint32_t min_neighbors,
                                                  uint32_t *__restrict__ flag, uint8_t *__restrict__ mask, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t keep = 0, rd = 0, rs = 0;
    if (i < n) {
        if (by_count) {
            keep = count[i] >= min_neighbors ? 1u : 0u;
        } else {
            const double s = __builtin_bit_cast(double, score_bits[i]);
            keep = (isfinite(s) && s <= thr) ? 1u : 0u;
        }
        flag[i] = keep;
        mask[i] = (uint8_t)keep;
        if (!keep) {
            uint32_t oor = 0;
            if (ev_is_dynamic(pts[i].w, oor)) rd = 1; else rs = 1;
        }
    }
    ev_commit(ctr, KN_C_KEPT, keep);
    ev_commit(ctr, KN_C_REMOVED_DYNAMIC, rd);
    ev_commit(ctr, KN_C_REMOVED_STATIC, rs);
}

}  // namespace ek

#endif  // ERASOR_KNN_HIP_H
