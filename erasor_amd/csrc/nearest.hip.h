// nearest.hip.h — the exact nearest ground-truth point of every estimated point, however far away: analysis_runner.py's overlap_report
// (scripts/analysis_runner.py:53-71) on the device.
//
// The reference fits NearestNeighbors(kd_tree) on the ground truth (GT) and queries the estimate: for every estimated point the distance
// to its nearest GT point, then the median / p90 / p99 / max of those distances and the fractions below 0.5*v, v and 2*v.  Unlike PR / RR
// (evaluate.hip.h: only neighbours within 0.866 cell edges matter, a 27-cell grid is exact there) the report needs the TRUE nearest
// distance of every point -- `max` is printed, and a misaligned map puts most points more than a cell away.
//
// Index: a bounding-volume tree over the GT.  30-bit Morton keys (10 bits per axis over the GT's bounding box; an axis of zero extent
// gets cell 0: planar, linear and single-point clouds) sorted stably by radix_sort, the points gathered in key order with their original
// index, leaves of NN_LEAF consecutive sorted points with the exact float AABB of their points, and an implicit complete binary tree over
// the leaf count padded to a power of two P (heap order: node 1 is the root, node k has children 2k and 2k+1, leaf l is node P + l).
// Nodes without points have the empty box lo = +inf, hi = -inf.  The tree only decides the ORDER of the search, never its answer.
//
// Query: one estimated point per lane, depth first, nearer child first, the pending siblings on a per-lane stack in LDS (a runtime-
// indexed per-lane array would live in scratch).  A node is pruned only when its lower bound is STRICTLY greater than the best d^2 so
// far, so every point at the minimum d^2 is visited and ties go to the smaller GT index.  Leaf points: d^2 in float64 exactly as
// k_ev_query / cKDTree compute it, ex = (double)q.x - (double)p.x, d^2 = (ex*ex + ey*ey) + ez*ez (the library builds with
// -ffp-contract=off: no fused multiply-add).  d = sqrt(d^2) with the correctly rounded float64 sqrt tests/test_gpu_hooks.py pins.
//
// Why the pruning is exact, with no epsilon: the lower bound of a box is formed by the same operations, per axis gap = (double)lo - q if
// q < lo, q - (double)hi if q > hi, else 0, and lb = (gx*gx + gy*gy) + gz*gz.  For a point p of the box and q < lo: p.x - q >= lo - q
// exactly, and rounding is monotone, so fl(p.x - q) >= fl(lo - q) = gx >= 0; fl(q - p.x) = -fl(p.x - q), so ex*ex = fl(p.x - q)^2 >=
// gx*gx (the product of non-negative values is monotone after rounding too).  The same holds for q > hi, and gx = 0 <= |ex| inside.
// Sums of non-negative terms are monotone in each term, so lb <= d^2(p) for every p in the box: what nn_walk, the one traversal every
// search of the tree shares, needs of a lower bound (its own part of the argument is stated there, once).
//
// Order statistics: the distances' float64 bit patterns stay on the device (every d >= +0, so unsigned order is numeric order) and an
// exact radix select finds the ranks the median and the two percentiles need: 8 passes of 8-bit digits from the top, all target ranks in
// the same pass; each pass is one histogram launch with 256 LDS counters per still-active prefix and one global add per non-zero bin and
// workgroup, and only those histograms go to the host, which picks the next digit of every target.
//
// label_map and calc_complement (third-party maps without labels, the static points a method lost) search the same tree in FLANN's
// float32 metric instead: k_lm_query / k_cp_query, below k_nn_query, where the exactness argument is restated for float.
#ifndef ERASOR_NEAREST_HIP_H
#define ERASOR_NEAREST_HIP_H

namespace ek {

// counters of one overlap report (one 64-bit atomic per wavefront and counter)
enum : uint32_t {
    OV_BELOW_HALF = 0,  // d < 0.5 * voxelsize
    OV_BELOW_ONE,       // d < voxelsize
    OV_BELOW_TWO,       // d < 2 * voxelsize
    OV_MAX_BITS,        // the bit pattern of the largest d (atomicMax: d >= +0)
    OV_NON_FINITE,      // points with a non-finite coordinate (the host refuses the report)
    OV_NCTR
};

static constexpr uint32_t NN_LEAF = 32;     // sorted points per leaf
static constexpr uint32_t NN_QBLOCK = 256;  // lanes per workgroup of k_nn_query
static constexpr uint32_t NN_STACK = 26;    // stack entries per lane: one per level below the root, at most 2^25 leaves (2^30 points)
static constexpr uint32_t OV_SEL_MAX = 6;   // target ranks of one select: two for the median, two for each percentile

// 10 bits of v spread to every third bit
__device__ __forceinline__ uint32_t nn_spread10(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// the 10-bit cell of v on an axis of the box [lo, hi]; zero extent (and anything non-finite) gives cell 0
__device__ __forceinline__ uint32_t nn_cell10(float v, float lo, float hi) {
    const double ext = (double)hi - (double)lo;
    if (!(ext > 0.0)) return 0u;
    double t = ((double)v - (double)lo) / ext * 1024.0;
    if (!(t >= 0.0)) t = 0.0;
    if (t > 1023.0) t = 1023.0;
    return (uint32_t)t;
}

// (1) Morton key of every GT point over the box k_bbox left in bb (fkey_ord order); counts the non-finite points
__global__ __launch_bounds__(256) void k_nn_keys(const float4 *__restrict__ gt, uint32_t n, const uint32_t *__restrict__ bb,
                                                  uint32_t *__restrict__ key, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < n) {
        const float4 p = gt[i];
        bad = ev_finite(p) ? 0u : 1u;
        const uint32_t cx = nn_cell10(p.x, fkey_inv(bb[0]), fkey_inv(bb[3]));
        const uint32_t cy = nn_cell10(p.y, fkey_inv(bb[1]), fkey_inv(bb[4]));
        const uint32_t cz = nn_cell10(p.z, fkey_inv(bb[2]), fkey_inv(bb[5]));
        key[i] = nn_spread10(cx) | (nn_spread10(cy) << 1) | (nn_spread10(cz) << 2);
    }
    ev_commit(ctr, OV_NON_FINITE, bad);
}

// (2) the points in key order, with their original index beside them
__global__ __launch_bounds__(256) void k_nn_gather(const float4 *__restrict__ gt, uint32_t n, const uint32_t *__restrict__ perm,
                                                    float4 *__restrict__ pts, uint32_t *__restrict__ idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = perm[i];
    pts[i] = gt[j];
    idx[i] = j;
}

// (3) one lane per sorted point, NN_LEAF lanes per leaf: the leaf's exact float AABB by a butterfly over the half-wavefront.  The grid
// covers all P leaves; leaves past the last point get the empty box.  lo / hi: [2P] (node P + l is leaf l).
__global__ __launch_bounds__(256) void k_nn_leaves(const float4 *__restrict__ pts, uint32_t n, uint32_t n_pad, float4 *__restrict__ lo,
                                                    float4 *__restrict__ hi) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const float inf = __builtin_huge_valf();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    if (i < n) {
        const float4 p = pts[i];
        mn[0] = mx[0] = p.x;
        mn[1] = mx[1] = p.y;
        mn[2] = mx[2] = p.z;
    }
#pragma unroll
    for (int m = NN_LEAF / 2; m >= 1; m >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], m));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], m));
        }
    }
    const uint32_t leaf = i / NN_LEAF;
    if ((i % NN_LEAF) == 0 && leaf < n_pad) {
        lo[n_pad + leaf] = make_float4(mn[0], mn[1], mn[2], 0.0f);
        hi[n_pad + leaf] = make_float4(mx[0], mx[1], mx[2], 0.0f);
    }
}

// (4) one level of the tree, bottom-up: nodes [first, 2 * first) from their children
__global__ __launch_bounds__(256) void k_nn_level(float4 *__restrict__ lo, float4 *__restrict__ hi, uint32_t first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= first) return;
    const uint32_t k = first + i;
    const float4 a = lo[2 * k], b = lo[2 * k + 1], c = hi[2 * k], d = hi[2 * k + 1];
    lo[k] = make_float4(fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z), 0.0f);
    hi[k] = make_float4(fmaxf(c.x, d.x), fmaxf(c.y, d.y), fmaxf(c.z, d.z), 0.0f);
}

#ifdef ERASOR_HIP_TEST_HOOKS
// test hooks only: when set, every search also writes the leaves it opened and the leaf points it tested to nn_effort[2 * i], [2 * i + 1],
// i = blockIdx.x * NN_QBLOCK + t (the query's index in k_nn_query / k_lm_query).  The product library has none of this.
__device__ uint32_t *nn_effort = nullptr;
__global__ void k_nn_set_effort(uint32_t *p) { nn_effort = p; }
#endif

// the lower bound of d^2 from q to any point of the box [l, u] (exact: see the header)
__device__ __forceinline__ double nn_lb(const float4 &l, const float4 &u, double qx, double qy, double qz) {
    const double gx = qx < (double)l.x ? (double)l.x - qx : (qx > (double)u.x ? qx - (double)u.x : 0.0);
    const double gy = qy < (double)l.y ? (double)l.y - qy : (qy > (double)u.y ? qy - (double)u.y : 0.0);
    const double gz = qz < (double)l.z ? (double)l.z - qz : (qz > (double)u.z ? qz - (double)u.z : 0.0);
    return (gx * gx + gy * gy) + gz * gz;
}

// The tree as the searches see it, one value passed to every query kernel: pts / idx the points in key order and their original
// indices ([n]), lo / hi the boxes of all 2 * n_pad nodes.  n == 0: n_pad = 1, nothing built, and no search may start.
struct NnTree {
    const float4 *pts;
    const uint32_t *idx;
    const float4 *lo, *hi;
    uint32_t n, n_pad;
};

#ifdef ERASOR_HIP_TEST_HOOKS
// a finished visitor's effort counts into nn_effort at the query's slot, when the hook is set
template <class V>
__device__ __forceinline__ void nn_put_effort(const V &v, size_t slot) {
    if (nn_effort) {
        nn_effort[2 * slot] = v.n_leaves;
        nn_effort[2 * slot + 1] = v.n_points;
    }
}
#endif

// THE traversal, shared by every search of the tree (T.n > 0): depth first from the root, nearer child first, the pending siblings at
// stack[depth * STRIDE + t] (the workgroup's [NN_STACK][STRIDE] LDS array, t: the lane's column).  The visitor V supplies what differs:
//   real                 the arithmetic of its bounds (double or float);
//   lb(l, u)             a lower bound of its d^2 from the query to every point of the box [l, u];
//   bound()              the current bound: a box is pruned only when lb is STRICTLY greater;
//   leaf(T, b, e)        the sorted points b .. e of a reached leaf (at least one); returns true to end the search at once;
//   FIXED                the bound never changes, so a popped sibling, which passed it when it was pushed, is taken untested.
// Why no search loses a point it needs: a box is skipped only on lb > bound, lb <= d^2(p) for every p of the box, and the bound never
// grows, so a skipped box holds no point with d^2 <= the bound at that moment or later; because the prune is strict every point AT the
// bound is visited, and the visitor's tie rule sees it.  Empty boxes (lo = +inf > hi) are never entered.  The order of visit -- the child
// with the smaller lb first, the left one on equal lb -- decides only the effort, never the answer.
template <uint32_t STRIDE, class V>
__device__ __forceinline__ void nn_walk(V &v, const NnTree &T, uint32_t *stack, uint32_t t) {
    typedef typename V::real real;
    const real inf = (real)__builtin_huge_val();
    uint32_t node = 1, sp = 0;
    for (;;) {
        if (node >= T.n_pad) {  // a leaf: its points (a leaf that is reached holds at least one)
            const uint32_t b = (node - T.n_pad) * NN_LEAF, e = b + NN_LEAF < T.n ? b + NN_LEAF : T.n;
            if (v.leaf(T, b, e)) return;
        } else {
            const uint32_t c = 2 * node;
            const float4 l0 = T.lo[c], u0 = T.hi[c], l1 = T.lo[c + 1], u1 = T.hi[c + 1];
            const real d0 = l0.x <= u0.x ? v.lb(l0, u0) : inf;  // (empty boxes: never entered)
            const real d1 = l1.x <= u1.x ? v.lb(l1, u1) : inf;
            const bool v0 = l0.x <= u0.x && !(d0 > v.bound()), v1 = l1.x <= u1.x && !(d1 > v.bound());
            if (v0 && v1) {
                const uint32_t near = d1 < d0 ? c + 1 : c;
                stack[sp * STRIDE + t] = near ^ 1u;  // (sp < the tree's depth <= NN_STACK - 1: one entry per level above)
                ++sp;
                node = near;
                continue;
            }
            if (v0 || v1) {
                node = v0 ? c : c + 1;
                continue;
            }
        }
        if constexpr (V::FIXED) {
            if (!sp) return;
            --sp;
            node = stack[sp * STRIDE + t];
        } else {
            bool more = false;  // the next pending sibling that may still hold a point within the bound, which has shrunk since the push
            while (sp) {
                --sp;
                const uint32_t k = stack[sp * STRIDE + t];
                if (!(v.lb(T.lo[k], T.hi[k]) > v.bound())) {
                    node = k;
                    more = true;
                    break;
                }
            }
            if (!more) return;
        }
    }
}

// visitor: the exact float64 1-NN.  The bound is the best d^2 so far, so every point at the minimum is visited and ties go to the
// smaller original index.
struct NnBestF64 {
    typedef double real;
    static constexpr bool FIXED = false;
    double qx, qy, qz;
    double best = __builtin_huge_val();
    uint32_t best_i = 0xFFFFFFFFu;
#ifdef ERASOR_HIP_TEST_HOOKS
    uint32_t n_leaves = 0, n_points = 0;  // leaves opened, and e - b of each
#endif
    __device__ __forceinline__ double lb(const float4 &l, const float4 &u) const { return nn_lb(l, u, qx, qy, qz); }
    __device__ __forceinline__ double bound() const { return best; }
    __device__ __forceinline__ bool leaf(const NnTree &T, uint32_t b, uint32_t e) {
#ifdef ERASOR_HIP_TEST_HOOKS
        ++n_leaves;
        n_points += e - b;
#endif
        for (uint32_t s = b; s < e; ++s) {
            const float4 p = T.pts[s];
            const double ex = qx - (double)p.x, ey = qy - (double)p.y, ez = qz - (double)p.z;
            const double d2 = (ex * ex + ey * ey) + ez * ez;
            if (d2 <= best) {
                const uint32_t j = T.idx[s];
                if (d2 < best || j < best_i) {
                    best = d2;
                    best_i = j;
                }
            }
        }
        return false;
    }
};

// the exact float64 1-NN of q over the tree (T.n > 0, q finite): the best d^2, and in *best_i the smallest original index at it.
// stack: the workgroup's [NN_STACK][NN_QBLOCK] LDS array, t: the lane's column.  k_nn_query and k_al_query (align.hip.h) share it.
__device__ __forceinline__ double nn_search_f64(double qx, double qy, double qz, const NnTree &T, uint32_t *stack, uint32_t t, uint32_t *best_i) {
    NnBestF64 v{qx, qy, qz};
    nn_walk<NN_QBLOCK>(v, T, stack, t);
#ifdef ERASOR_HIP_TEST_HOOKS
    nn_put_effort(v, (size_t)(blockIdx.x * NN_QBLOCK + t));
#endif
    *best_i = v.best_i;
    return v.best;
}

// (5) one estimated point per lane: its nearest GT point (d^2, then the smaller original index), d = sqrt(d^2) as a bit pattern in
// dbits, the original index in nearest (optional), the three threshold counters and the maximum.  T.n > 0.
__global__ __launch_bounds__(NN_QBLOCK) void k_nn_query(const float4 *__restrict__ est, uint32_t n_est, NnTree T, double half, double one, double two,
                                                         unsigned long long *__restrict__ dbits, uint32_t *__restrict__ nearest,
                                                         unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * NN_QBLOCK];  // [depth][lane]: consecutive lanes in consecutive banks
    const uint32_t t = threadIdx.x, i = blockIdx.x * NN_QBLOCK + t;
    uint32_t bh = 0, b1 = 0, b2 = 0, bad = 0;
    unsigned long long bits = 0ull;
    if (i < n_est) {
        const float4 q = est[i];
        if (!ev_finite(q)) {
            bad = 1;
            dbits[i] = 0ull;
            if (nearest) nearest[i] = 0xFFFFFFFFu;
        } else {
            uint32_t best_i;
            const double best = nn_search_f64((double)q.x, (double)q.y, (double)q.z, T, stack, t, &best_i);
            const double d = sqrt(best);
            bh = d < half ? 1u : 0u;
            b1 = d < one ? 1u : 0u;
            b2 = d < two ? 1u : 0u;
            bits = __builtin_bit_cast(unsigned long long, d);
            dbits[i] = bits;
            if (nearest) nearest[i] = best_i;
        }
    }
    ev_commit(ctr, OV_BELOW_HALF, bh);
    ev_commit(ctr, OV_BELOW_ONE, b1);
    ev_commit(ctr, OV_BELOW_TWO, b2);
    ev_commit(ctr, OV_NON_FINITE, bad);
    // the wavefront's largest bit pattern: the high words first, then the low words of the lanes that hold the largest high word
    const uint32_t whi = wave_minmax_u<true>((uint32_t)(bits >> 32));
    const uint32_t wlo = wave_minmax_u<true>((uint32_t)(bits >> 32) == whi ? (uint32_t)bits : 0u);
    const unsigned long long wmax = ((unsigned long long)whi << 32) | wlo;
    if ((t & 63u) == 0 && wmax) atomicMax(&ctr[OV_MAX_BITS], wmax);
}

// ---- the same tree searched in FLANN's metric: label_map (fill_removert_intensity.cpp:24-59, compare_map.cpp:77-110) and calc_complement
// (compare_complement.cpp:43-75) query a pcl::KdTreeFLANN, K = 1, whose distance is L2_Simple in float32: r = 0; r += dx*dx; r += dy*dy;
// r += dz*dz with dx = q.x - p.x in float (FLANN's L2_Simple; no fused multiply-add: -ffp-contract=off), and
// whose ties go to the lowest index.  The traversal, the LDS stack and the strict pruning are nn_walk's; only the visitor's arithmetic differs.
//
// Why the pruning stays exact in float: the lower bound is formed by the same float operations on the box gaps, gx = l.x - q.x if
// q.x < l.x, q.x - u.x if q.x > u.x, else 0, and lb = ((0 + gx*gx) + gy*gy) + gz*gz.  For a point p of the box and q.x < l.x:
// p.x - q.x >= l.x - q.x exactly, and rounding to nearest is monotone, so fl(p.x - q.x) >= fl(l.x - q.x) = gx >= 0; fl(q.x - p.x) =
// -fl(p.x - q.x) (rounding to nearest is symmetric), so fl(dx*dx) >= fl(gx*gx).  The same holds for q.x > u.x, and gx = 0 <= |dx|
// inside.  Sums of non-negative floats are monotone in each term after rounding, so lb <= d^2(p) for every p of the box, as nn_walk
// requires.  Nothing here relies on gradual underflow, but the answer does: a difference of
// 1e-20 squares to a subnormal, which flushing would tie with an exact 0.  The library keeps f32 denormals (hipcc's default for
// gfx950: the kernels' float denorm mode is "flush none"), as the host's float arithmetic does.
//
// Ties: the label a query takes depends on the tie rule only when the points at its minimum d^2 carry different intensity bits; those
// queries are counted (FM_TIED), in the spirit of the evaluator's n_tied.

// counters of one label_map / static_complement call (one 64-bit atomic per wavefront and counter)
enum : uint32_t {
    FM_TIED = 0,     // label_map: queries whose minimum d^2 is shared by medium points of different intensity bits
    FM_GT_STATIC,    // static_complement: static ground-truth points
    FM_LOST,         // static_complement: static ground-truth points whose nearest estimated point is farther than the threshold
    FM_LABEL_OOR,    // static_complement: intensities that are not finite or outside [0, 2^32): decoded as static
    FM_NON_FINITE,   // query points with a non-finite coordinate (the host refuses the call)
    FM_NCTR
};

// the float lower bound of d^2 from q to any point of the box [l, u] (exact: see above)
__device__ __forceinline__ float nn_lb_f32(const float4 &l, const float4 &u, float qx, float qy, float qz) {
    const float gx = qx < l.x ? l.x - qx : (qx > u.x ? qx - u.x : 0.0f);
    const float gy = qy < l.y ? l.y - qy : (qy > u.y ? qy - u.y : 0.0f);
    const float gz = qz < l.z ? l.z - qz : (qz > u.z ? qz - u.z : 0.0f);
    float r = 0.0f;
    r += gx * gx;
    r += gy * gy;
    r += gz * gz;
    return r;
}

// visitor: the exact float32 1-NN in FLANN's metric: best d^2, the smallest original index at it, that point's w bits, and whether the
// points at the minimum carry more than one w bit pattern.  The bound is the best d^2 so far.
struct NnF32 {
    float d2;
    uint32_t idx, w;
    bool mixed;
};
struct NnBestF32 {
    typedef float real;
    static constexpr bool FIXED = false;
    float qx, qy, qz;
    NnF32 b{__builtin_huge_valf(), 0xFFFFFFFFu, 0u, false};
#ifdef ERASOR_HIP_TEST_HOOKS
    uint32_t n_leaves = 0, n_points = 0;  // leaves opened, and e - s0 of each
#endif
    __device__ __forceinline__ float lb(const float4 &l, const float4 &u) const { return nn_lb_f32(l, u, qx, qy, qz); }
    __device__ __forceinline__ float bound() const { return b.d2; }
    __device__ __forceinline__ bool leaf(const NnTree &T, uint32_t s0, uint32_t e) {
#ifdef ERASOR_HIP_TEST_HOOKS
        ++n_leaves;
        n_points += e - s0;
#endif
        for (uint32_t s = s0; s < e; ++s) {
            const float4 p = T.pts[s];
            const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
            float r = 0.0f;
            r += dx * dx;
            r += dy * dy;
            r += dz * dz;
            if (r <= b.d2) {
                const uint32_t j = T.idx[s], w = __float_as_uint(p.w);
                if (r < b.d2) {
                    b.d2 = r;
                    b.idx = j;
                    b.w = w;
                    b.mixed = false;
                } else {  // the same d^2: the smaller index is the answer, a second bit pattern makes the query tied
                    // (idx == ~0u: no candidate yet -- a first point whose d^2 overflowed to +inf equals the seed, not a point)
                    if (b.idx != 0xFFFFFFFFu && w != b.w) b.mixed = true;
                    if (j < b.idx) {
                        b.idx = j;
                        b.w = w;
                    }
                }
            }
        }
        return false;
    }
};

// the exact float32 1-NN of q over the tree (T.n > 0, q finite).  stack: the workgroup's [NN_STACK][NN_QBLOCK] LDS array.
__device__ __forceinline__ NnF32 nn_search_f32(float qx, float qy, float qz, const NnTree &T, uint32_t *stack, uint32_t t) {
    NnBestF32 v{qx, qy, qz};
    nn_walk<NN_QBLOCK>(v, T, stack, t);
#ifdef ERASOR_HIP_TEST_HOOKS
    nn_put_effort(v, (size_t)(blockIdx.x * NN_QBLOCK + t));
#endif
    return v.b;
}

// label_map: one centroid per lane; the row out[i] = (centroid x, y, z, w of its nearest medium point, copied as bits).  T.n > 0.
__global__ __launch_bounds__(NN_QBLOCK) void k_lm_query(const float4 *__restrict__ cent, uint32_t n_q, NnTree T, float4 *__restrict__ out,
                                                         unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * NN_QBLOCK];
    const uint32_t t = threadIdx.x, i = blockIdx.x * NN_QBLOCK + t;
    uint32_t tied = 0, bad = 0;
    if (i < n_q) {
        const float4 q = cent[i];
        if (!ev_finite(q)) {
            bad = 1;
            out[i] = q;
        } else {
            const NnF32 b = nn_search_f32(q.x, q.y, q.z, T, stack, t);
            out[i] = make_float4(q.x, q.y, q.z, __uint_as_float(b.w));
            tied = b.mixed ? 1u : 0u;
        }
    }
    ev_commit(ctr, FM_TIED, tied);
    ev_commit(ctr, FM_NON_FINITE, bad);
}

// static_complement: one ground-truth point per lane; lost[i] = 1 when the point is static and its nearest estimated point's float
// d^2, widened to double, is > thr (calc_complement's `pointNKNSquaredDistance[0] > 0.03`: a float against a double literal).  T.n == 0:
// every static point is lost (d^2 = +inf).
__global__ __launch_bounds__(NN_QBLOCK) void k_cp_query(const float4 *__restrict__ gt, uint32_t n_gt, NnTree T, double thr, uint32_t *__restrict__ lost,
                                                         unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * NN_QBLOCK];
    const uint32_t t = threadIdx.x, i = blockIdx.x * NN_QBLOCK + t;
    uint32_t sta = 0, ls = 0, oor = 0, bad = 0;
    if (i < n_gt) {
        const float4 q = gt[i];
        if (!ev_finite(q)) {
            bad = 1;
        } else if (!ev_is_dynamic(q.w, oor)) {
            sta = 1;
            const float d2 = T.n ? nn_search_f32(q.x, q.y, q.z, T, stack, t).d2 : __builtin_huge_valf();
            ls = (double)d2 > thr ? 1u : 0u;
        }
        lost[i] = ls;
    }
    ev_commit(ctr, FM_GT_STATIC, sta);
    ev_commit(ctr, FM_LOST, ls);
    ev_commit(ctr, FM_LABEL_OOR, oor);
    ev_commit(ctr, FM_NON_FINITE, bad);
}

// one pass of the radix select: the values whose bits above `shift + 8` equal one of the prefixes, counted by prefix and by the 8-bit
// digit at `shift`.  hist: [n][256], zeroed by the host.
struct OvSelect {
    unsigned long long pref[OV_SEL_MAX];
    uint32_t n;
    int shift;
};
__global__ __launch_bounds__(256) void k_ov_select_hist(const unsigned long long *__restrict__ v, uint32_t count, OvSelect s,
                                                         uint32_t *__restrict__ hist) {
    __shared__ uint32_t c[OV_SEL_MAX * 256];
    for (uint32_t j = threadIdx.x; j < OV_SEL_MAX * 256; j += blockDim.x) c[j] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
        const unsigned long long x = v[i];
        const unsigned long long top = s.shift >= 56 ? 0ull : x >> (s.shift + 8);
        const uint32_t d = (uint32_t)(x >> s.shift) & 0xFFu;
        bool done = false;
#pragma unroll
        for (uint32_t k = 0; k < OV_SEL_MAX; ++k) {  // (unrolled: the prefixes stay in registers, no scratch)
            if (!done && k < s.n && top == s.pref[k]) {
                atomicAdd(&c[k * 256 + d], 1u);
                done = true;
            }
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < s.n * 256; j += blockDim.x)
        if (c[j]) atomicAdd(&hist[j], c[j]);
}

}  // namespace ek

#endif  // ERASOR_NEAREST_HIP_H
