// evaluate.hip.h — Preservation Rate / Rejection Rate of a cleaned map against a labelled ground-truth map, on the device.
//
// Replaces the reference's evaluator (scripts/analysis_runner.py:74-105, restated on the host in erasor_amd/evalmap.py): for every
// ground-truth (GT) point the nearest estimated point (1-NN, Euclidean, what cKDTree.query(k=1) returns); the GT point is kept if that
// distance is < voxelsize*sqrt(3)/2.  Labels: uint32(intensity) & 0xFFFF, classes 252..259 are dynamic (analysis_runner.py:14,44-47).
//
// The estimated map is indexed by a uniform grid of cell edge `voxelsize` hashed into a power-of-two bucket table (histogram -> exclusive
// scan -> scatter of (point, original index)).  The threshold is 0.866 cell edges, so every estimated point within it of a GT point lies
// in the 27 cells around that point's cell -- also when the cell coordinates of the two are a few ulps off their exact values (a margin of
// 0.134 cell edges).  Whenever the nearest estimated point is within the threshold, the minimum over those 27 cells IS the global minimum.
// Hash collisions only add candidates, and the order inside a bucket does not matter: the query decides by (d^2, estimated index).
//
// Distances are computed in float64 exactly as cKDTree does: dx = (double)gt.x - (double)est.x, d^2 = (dx*dx + dy*dy) + dz*dz, left to
// right (the library builds with -ffp-contract=off: no fused multiply-add).  The comparison is sqrt(d^2) < thr with the correctly rounded
// float64 square root: on gfx950 hipcc expands sqrt(double) (the llvm.sqrt.f64 lowering) into v_ldexp_f64 scaling of tiny inputs,
// v_rsq_f64, two Newton-Raphson steps on v_fma_f64, the inverse scaling and a v_cmp_class_f64 fix-up for 0 / inf -- no v_sqrt_f64 --
// and tests/test_gpu_hooks.py pins that device sqrt against the host's bit for bit.
#ifndef ERASOR_EVALUATE_HIP_H
#define ERASOR_EVALUATE_HIP_H

namespace ek {

// counters of one evaluation (one 64-bit atomic per wavefront and counter)
enum : uint32_t {
    EV_GT_STATIC = 0,
    EV_GT_DYNAMIC,
    EV_EST_STATIC,
    EV_EST_DYNAMIC,
    EV_KEPT_STATIC,
    EV_KEPT_DYNAMIC,
    EV_TIED,            // GT points within the threshold whose minimum d^2 is shared by candidates of both classes
    EV_LABEL_OOR,       // intensities that are not finite or outside [0, 2^32): decoded as static
    EV_NON_FINITE,      // points with a non-finite coordinate (the host refuses the evaluation)
    EV_NCTR
};
// per GT point (optional): 0 not within the threshold, 1 kept static, 2 kept dynamic, 3 within the threshold but the class differs
enum : uint8_t { EV_OUT = 0, EV_KEPT_S = 1, EV_KEPT_D = 2, EV_CLASS_DIFFERS = 3 };

static constexpr double EV_CELL_CLAMP = 1073741824.0;  // 2^30: cell coordinates are clamped (neighbours +-1 stay in int32)

// label decode of evalmap.labels: numeric cast to uint32, & 0xFFFF, dynamic = 252..259.  Values the cast is not defined for are static.
__device__ __forceinline__ bool ev_is_dynamic(float w, uint32_t &oor) {
    if (!(w >= 0.0f && w < 4294967296.0f)) {  // (NaN fails both)
        oor = 1u;
        return false;
    }
    const uint32_t sem = (uint32_t)w & 0xFFFFu;
    return sem >= 252u && sem <= 259u;
}

__device__ __forceinline__ int32_t ev_cell(float v, double cell) {
    double f = floor((double)v / cell);
    if (!(f >= -EV_CELL_CLAMP)) f = -EV_CELL_CLAMP;  // (NaN lands here: such a point is refused by the host anyway)
    if (f > EV_CELL_CLAMP) f = EV_CELL_CLAMP;
    return (int32_t)f;
}

__device__ __forceinline__ uint32_t ev_bucket(int32_t cx, int32_t cy, int32_t cz, uint32_t mask) {
    uint32_t k = ((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u);
    k ^= k >> 16;  // (murmur3 finaliser: neighbouring cells spread over the table)
    k *= 0x85EBCA6Bu;
    k ^= k >> 13;
    k *= 0xC2B2AE35u;
    k ^= k >> 16;
    return k & mask;
}

__device__ __forceinline__ bool ev_finite(const float4 &p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// lane 0 of each wavefront adds the wavefront's count (every lane of the wavefront must call this)
__device__ __forceinline__ void ev_commit(unsigned long long *ctr, uint32_t which, uint32_t mine) {
    const uint32_t s = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0 && s) atomicAdd(&ctr[which], (unsigned long long)s);
}

// (1) bucket of every estimated point + histogram of the buckets; est label counters.  cnt: [nb + 1], zeroed by the host.
__global__ __launch_bounds__(256) void k_ev_hist(const float4 *__restrict__ est, uint32_t n, double cell, uint32_t mask,
                                                  uint32_t *__restrict__ bucket_of, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t dyn = 0, sta = 0, oor = 0, bad = 0;
    if (i < n) {
        const float4 p = est[i];
        bad = ev_finite(p) ? 0u : 1u;
        const uint32_t b = ev_bucket(ev_cell(p.x, cell), ev_cell(p.y, cell), ev_cell(p.z, cell), mask);
        bucket_of[i] = b;
        atomicAdd(&cnt[b], 1u);
        if (ev_is_dynamic(p.w, oor)) dyn = 1; else sta = 1;
    }
    ev_commit(ctr, EV_EST_DYNAMIC, dyn);
    ev_commit(ctr, EV_EST_STATIC, sta);
    ev_commit(ctr, EV_LABEL_OOR, oor);
    ev_commit(ctr, EV_NON_FINITE, bad);
}

// (2) after scan_u32 over cnt[0 .. nb]: off[b] = start of bucket b (off[nb] = n), cursor[b] = the same (the scatter's slot counter).
// off may be cnt itself, cursor may be pl itself (each thread reads its own entries before it writes them).
__global__ __launch_bounds__(256) void k_ev_offsets(const uint32_t *pl, const uint32_t *__restrict__ tops, uint32_t nb1, uint32_t *off,
                                                     uint32_t *cursor) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb1) return;
    const uint32_t o = pl[b] + tops[b >> 10];
    off[b] = o;
    cursor[b] = o;
}

// (3) (point, original index) into its bucket's range; the order inside a bucket is whatever the atomics give
__global__ __launch_bounds__(256) void k_ev_scatter(const float4 *__restrict__ est, uint32_t n, const uint32_t *__restrict__ bucket_of,
                                                     uint32_t *__restrict__ cursor, float4 *__restrict__ pts, uint32_t *__restrict__ idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = atomicAdd(&cursor[bucket_of[i]], 1u);
    pts[s] = est[i];
    idx[s] = i;
}

// k_ev_query's search for the GT point g, for the breakdown kernels: the minimum (d^2, estimated index) over the 27 buckets around its
// cell, the class of that estimated point, and the classes seen at the minimum d^2.  The caller starts with best = +inf, best_i = ~0u
// and the flags false.  k_ev_query keeps its own copy of this loop: calling the function changes its register allocation and schedule,
// and that kernel's code object stays as it was.
__device__ __forceinline__ void ev_nearest(const float4 &g, const float4 *pts, const uint32_t *idx, const uint32_t *off, uint32_t mask, double cell, double &best, uint32_t &best_i,
                                           bool &best_dyn, bool &at_min_s, bool &at_min_d) {
    const double gx = (double)g.x, gy = (double)g.y, gz = (double)g.z;
    const int32_t cx = ev_cell(g.x, cell), cy = ev_cell(g.y, cell), cz = ev_cell(g.z, cell);
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t b = ev_bucket(cx + dx, cy + dy, cz + dz, mask);
                const uint32_t e = off[b + 1];
                for (uint32_t s = off[b]; s < e; ++s) {
                    const float4 p = pts[s];
                    const double ex = gx - (double)p.x, ey = gy - (double)p.y, ez = gz - (double)p.z;
                    const double d2 = (ex * ex + ey * ey) + ez * ez;
                    if (!(d2 <= best)) continue;  // (NaN never wins)
                    uint32_t o_ = 0;
                    const bool e_dyn = ev_is_dynamic(p.w, o_);
                    const uint32_t j = idx[s];
                    if (d2 < best) {
                        best = d2;
                        best_i = j;
                        best_dyn = e_dyn;
                        at_min_s = !e_dyn;
                        at_min_d = e_dyn;
                    } else {  // the same d^2: the smaller index is the answer, both classes are remembered
                        if (j < best_i) {
                            best_i = j;
                            best_dyn = e_dyn;
                        }
                        at_min_s = at_min_s || !e_dyn;
                        at_min_d = at_min_d || e_dyn;
                    }
                }
            }
}

// (4) one GT point per lane: the minimum (d^2, estimated index) over the 27 buckets around its cell, then the counters
__global__ __launch_bounds__(256) void k_ev_query(const float4 *__restrict__ gt, uint32_t n_gt, const float4 *__restrict__ pts,
                                                   const uint32_t *__restrict__ idx, const uint32_t *__restrict__ off, uint32_t mask, uint32_t n_est,
                                                   double cell, double thr, uint8_t *__restrict__ code, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t gs = 0, gd = 0, ks = 0, kd = 0, tied = 0, oor = 0, bad = 0;
    if (i < n_gt) {
        const float4 g = gt[i];
        bad = ev_finite(g) ? 0u : 1u;
        const bool g_dyn = ev_is_dynamic(g.w, oor);
        gd = g_dyn ? 1u : 0u;
        gs = 1u - gd;
        double best = __builtin_huge_val();
        uint32_t best_i = 0xFFFFFFFFu;
        bool best_dyn = false, at_min_s = false, at_min_d = false;  // classes seen at the current minimum d^2
        if (n_est) {
            const double gx = (double)g.x, gy = (double)g.y, gz = (double)g.z;
            const int32_t cx = ev_cell(g.x, cell), cy = ev_cell(g.y, cell), cz = ev_cell(g.z, cell);
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const uint32_t b = ev_bucket(cx + dx, cy + dy, cz + dz, mask);
                        const uint32_t e = off[b + 1];
                        for (uint32_t s = off[b]; s < e; ++s) {
                            const float4 p = pts[s];
                            const double ex = gx - (double)p.x, ey = gy - (double)p.y, ez = gz - (double)p.z;
                            const double d2 = (ex * ex + ey * ey) + ez * ez;
                            if (!(d2 <= best)) continue;  // (NaN never wins)
                            uint32_t o_ = 0;
                            const bool e_dyn = ev_is_dynamic(p.w, o_);
                            const uint32_t j = idx[s];
                            if (d2 < best) {
                                best = d2;
                                best_i = j;
                                best_dyn = e_dyn;
                                at_min_s = !e_dyn;
                                at_min_d = e_dyn;
                            } else {  // the same d^2: the smaller index is the answer, both classes are remembered
                                if (j < best_i) {
                                    best_i = j;
                                    best_dyn = e_dyn;
                                }
                                at_min_s = at_min_s || !e_dyn;
                                at_min_d = at_min_d || e_dyn;
                            }
                        }
                    }
        }
        uint8_t c = EV_OUT;
        if (best_i != 0xFFFFFFFFu && sqrt(best) < thr) {
            if (!g_dyn && !best_dyn) {
                c = EV_KEPT_S;
                ks = 1;
            } else if (g_dyn && best_dyn) {
                c = EV_KEPT_D;
                kd = 1;
            } else {
                c = EV_CLASS_DIFFERS;
            }
            tied = (at_min_s && at_min_d) ? 1u : 0u;
        }
        if (code) code[i] = c;
    }
    ev_commit(ctr, EV_GT_STATIC, gs);
    ev_commit(ctr, EV_GT_DYNAMIC, gd);
    ev_commit(ctr, EV_KEPT_STATIC, ks);
    ev_commit(ctr, EV_KEPT_DYNAMIC, kd);
    ev_commit(ctr, EV_TIED, tied);
    ev_commit(ctr, EV_LABEL_OOR, oor);
    ev_commit(ctr, EV_NON_FINITE, bad);
}

// ---- the breakdown by class and by dynamic instance (erasor_hip_evaluate_*_by_class) ----
// Class key of a label: uint32(intensity) & 0xFFFF, or EV_KEY_OOR where the cast is not defined (ev_is_dynamic's decode).  A dense table
// holds EV_KC counters per key; an instance row holds its label and the same counters.  Dynamic points with a label in range are also
// appended to a list of (label, counter bits) records, which the host sorts into instance rows.
static constexpr uint32_t EV_KEY_OOR = 0x10000u, EV_NKEYS = 0x10001u;
enum : uint32_t { EV_K_GT = 0, EV_K_WITHIN, EV_K_KEPT, EV_K_TIED, EV_K_EST, EV_KC };  // counter columns (bit c of a record: column c)
static constexpr uint32_t EV_ROW = 1 + EV_KC;                                           // a row: key, then the counters

__device__ __forceinline__ uint32_t ev_key(float w) { return (w >= 0.0f && w < 4294967296.0f) ? ((uint32_t)w & 0xFFFFu) : EV_KEY_OOR; }

// tab[row * stride + c] += the number of lanes with this row and bit c set, for c < EV_KC.  The lanes holding the same row are grouped
// (match_any) and the lowest of them adds the group's counts: one atomic per distinct row and counter of the wavefront, never one per
// lane.  Every lane of the wavefront must call this (row_bits: bits of the row numbers, for match_any's fallback).
__device__ __forceinline__ void ev_add_rows(uint32_t *tab, uint32_t stride, uint32_t row, bool valid, uint32_t bits, int row_bits) {
    const uint64_t peers = match_any(row, valid, row_bits);
    const bool leader = valid && (peers & lanemask_lt()) == 0ull;
#pragma unroll
    for (uint32_t c = 0; c < EV_KC; ++c) {
        const uint32_t n = (uint32_t)__popcll(peers & __ballot(valid && ((bits >> c) & 1u)));
        if (leader && n) atomicAdd(&tab[(size_t)row * stride + c], n);
    }
}

// appends (label, bits) of the lanes with `take` set to ikey / ival at the cursor *cur: one atomic per wavefront (every lane calls this)
__device__ __forceinline__ void ev_append(uint32_t *cur, uint32_t *__restrict__ ikey, uint32_t *__restrict__ ival, bool take, uint32_t label,
                                          uint32_t bits) {
    const uint64_t m = __ballot(take);
    if (m == 0ull) return;
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0) base = atomicAdd(cur, (uint32_t)__popcll(m));
    base = __builtin_amdgcn_readfirstlane(base);
    if (take) {
        const uint32_t s = base + (uint32_t)__popcll(m & lanemask_lt());
        ikey[s] = label;
        ival[s] = bits;
    }
}

// (1') k_ev_hist, plus each estimated point's class (column EV_K_EST of tab) and the records of its dynamic points.  cur: [1], zeroed.
__global__ __launch_bounds__(256) void k_ev_hist_keys(const float4 *__restrict__ est, uint32_t n, double cell, uint32_t mask,
                                                       uint32_t *__restrict__ bucket_of, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr,
                                                       uint32_t *__restrict__ tab, uint32_t *__restrict__ cur, uint32_t *__restrict__ ikey,
                                                       uint32_t *__restrict__ ival) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t dyn = 0, sta = 0, oor = 0, bad = 0, key = 0, label = 0;
    if (i < n) {
        const float4 p = est[i];
        bad = ev_finite(p) ? 0u : 1u;
        const uint32_t b = ev_bucket(ev_cell(p.x, cell), ev_cell(p.y, cell), ev_cell(p.z, cell), mask);
        bucket_of[i] = b;
        atomicAdd(&cnt[b], 1u);
        if (ev_is_dynamic(p.w, oor)) dyn = 1; else sta = 1;
        key = ev_key(p.w);
        if (dyn) label = (uint32_t)p.w;
    }
    ev_commit(ctr, EV_EST_DYNAMIC, dyn);
    ev_commit(ctr, EV_EST_STATIC, sta);
    ev_commit(ctr, EV_LABEL_OOR, oor);
    ev_commit(ctr, EV_NON_FINITE, bad);
    ev_add_rows(tab, EV_KC, key, i < n, 1u << EV_K_EST, 17);
    ev_append(cur, ikey, ival, dyn != 0, label, 1u << EV_K_EST);
}

// (4') k_ev_query's decision and counters (no per-point codes), plus each GT point's (class, within, kept, tied) in tab and the records
// of its dynamic points
__global__ __launch_bounds__(256) void k_ev_query_keys(const float4 *__restrict__ gt, uint32_t n_gt, const float4 *__restrict__ pts,
                                                        const uint32_t *__restrict__ idx, const uint32_t *__restrict__ off, uint32_t mask, uint32_t n_est,
                                                        double cell, double thr, unsigned long long *__restrict__ ctr, uint32_t *__restrict__ tab,
                                                        uint32_t *__restrict__ cur, uint32_t *__restrict__ ikey, uint32_t *__restrict__ ival) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t gs = 0, gd = 0, ks = 0, kd = 0, tied = 0, oor = 0, bad = 0, key = 0, label = 0, bits = 0;
    if (i < n_gt) {
        const float4 g = gt[i];
        bad = ev_finite(g) ? 0u : 1u;
        const bool g_dyn = ev_is_dynamic(g.w, oor);
        gd = g_dyn ? 1u : 0u;
        gs = 1u - gd;
        key = ev_key(g.w);
        if (g_dyn) label = (uint32_t)g.w;
        double best = __builtin_huge_val();
        uint32_t best_i = 0xFFFFFFFFu;
        bool best_dyn = false, at_min_s = false, at_min_d = false;
        if (n_est) ev_nearest(g, pts, idx, off, mask, cell, best, best_i, best_dyn, at_min_s, at_min_d);
        bits = 1u << EV_K_GT;
        if (best_i != 0xFFFFFFFFu && sqrt(best) < thr) {
            if (!g_dyn && !best_dyn) ks = 1;
            else if (g_dyn && best_dyn) kd = 1;
            tied = (at_min_s && at_min_d) ? 1u : 0u;
            bits |= (1u << EV_K_WITHIN) | ((ks | kd) << EV_K_KEPT) | (tied << EV_K_TIED);
        }
    }
    ev_commit(ctr, EV_GT_STATIC, gs);
    ev_commit(ctr, EV_GT_DYNAMIC, gd);
    ev_commit(ctr, EV_KEPT_STATIC, ks);
    ev_commit(ctr, EV_KEPT_DYNAMIC, kd);
    ev_commit(ctr, EV_TIED, tied);
    ev_commit(ctr, EV_LABEL_OOR, oor);
    ev_commit(ctr, EV_NON_FINITE, bad);
    ev_add_rows(tab, EV_KC, key, i < n_gt, bits, 17);
    ev_append(cur, ikey, ival, gd != 0, label, bits);
}

// (5) class rows: flag[k] = key k was seen in either cloud (scan_u32 then numbers the rows in key order)
__global__ __launch_bounds__(256) void k_ev_class_flags(const uint32_t *__restrict__ tab, uint32_t *__restrict__ flag) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= EV_NKEYS) return;
    flag[k] = (tab[(size_t)k * EV_KC + EV_K_GT] | tab[(size_t)k * EV_KC + EV_K_EST]) ? 1u : 0u;
}

// (6) ... and the scatter: rows[r] = (k, its counters) at r = the exclusive scan of the flags
__global__ __launch_bounds__(256) void k_ev_class_rows(const uint32_t *__restrict__ tab, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pl,
                                                        const uint32_t *__restrict__ tops, uint32_t *__restrict__ rows) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= EV_NKEYS || !flag[k]) return;
    const uint32_t r = pl[k] + tops[k >> 10];
    rows[(size_t)r * EV_ROW] = k;
#pragma unroll
    for (uint32_t c = 0; c < EV_KC; ++c) rows[(size_t)r * EV_ROW + 1 + c] = tab[(size_t)k * EV_KC + c];
}

// (7) instance rows, over the records sorted by label (skey, perm from radix_sort): head[j] = a run of labels starts at j
__global__ __launch_bounds__(256) void k_ev_run_heads(const uint32_t *__restrict__ skey, uint32_t n, uint32_t *__restrict__ head) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    head[j] = (j == 0 || skey[j] != skey[j - 1]) ? 1u : 0u;
}

// (8) ... after scan_u32 over the heads: record j belongs to row (exclusive scan + head - 1); the head writes the label, the lanes of a
// run add their counter bits with one atomic per row and counter (rows: zeroed by the host)
__global__ __launch_bounds__(256) void k_ev_inst_rows(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ ival,
                                                       const uint32_t *__restrict__ head, const uint32_t *__restrict__ pl, const uint32_t *__restrict__ tops,
                                                       uint32_t n, uint32_t *__restrict__ rows) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t r = 0, bits = 0;
    if (j < n) {
        const uint32_t h = head[j];
        r = pl[j] + tops[j >> 10] + h - 1u;
        bits = ival[perm[j]];
        if (h) rows[(size_t)r * EV_ROW] = skey[j];
    }
    ev_add_rows(rows + 1, EV_ROW, r, j < n, bits, 32);
}

// ---- K estimates against one ground truth in one set of launches (erasor_hip_evaluate_many) ----
// The estimates lie back to back in one array.  Estimate j owns the bucket range [base, base + mask] of one combined table; its buckets
// are k_ev_hist's (a power of two >= its size, at least 1024), so with the combined offsets `off + base` it is searched exactly as
// k_ev_query searches a table of its own.  k_ev_offsets and k_ev_scatter build the combined table unchanged; the scatter stores the
// combined index off_j + i, which orders the points of one estimate as their own index i does.
struct EvmEst {
    uint32_t off;   // first point of the estimate in the combined array
    uint32_t n;     // its points
    uint32_t base;  // first bucket of its range
    uint32_t mask;  // its bucket count - 1
    uint32_t blk0;  // first workgroup of k_evm_hist on it (entry k, after the last estimate: the grid)
    uint32_t pad_[3];
};

// (1) every estimate's buckets and their histogram, one workgroup never straddling two estimates; estimate counters per estimate in
// ctr[j * EV_NCTR ..].  cnt: [buckets + 1], zeroed by the host.
__global__ __launch_bounds__(256) void k_evm_hist(const float4 *__restrict__ est, const EvmEst *__restrict__ tab, uint32_t k, double cell,
                                                   uint32_t *__restrict__ bucket_of, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr) {
    uint32_t lo = 0, hi = k;  // the block's estimate: the last j with blk0_j <= blockIdx.x (empty estimates share the next one's blk0)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid].blk0 <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const EvmEst e = tab[lo];
    const uint32_t i = (blockIdx.x - e.blk0) * blockDim.x + threadIdx.x;
    uint32_t dyn = 0, sta = 0, oor = 0, bad = 0;
    if (i < e.n) {
        const float4 p = est[e.off + i];
        bad = ev_finite(p) ? 0u : 1u;
        const uint32_t b = e.base + ev_bucket(ev_cell(p.x, cell), ev_cell(p.y, cell), ev_cell(p.z, cell), e.mask);
        bucket_of[e.off + i] = b;
        atomicAdd(&cnt[b], 1u);
        if (ev_is_dynamic(p.w, oor)) dyn = 1; else sta = 1;
    }
    unsigned long long *c = ctr + (size_t)lo * EV_NCTR;
    ev_commit(c, EV_EST_DYNAMIC, dyn);
    ev_commit(c, EV_EST_STATIC, sta);
    ev_commit(c, EV_LABEL_OOR, oor);
    ev_commit(c, EV_NON_FINITE, bad);
}

// ev_nearest with the GT point's cell given (computed once for all estimates)
__device__ __forceinline__ void evm_nearest(const float4 &g, int32_t cx, int32_t cy, int32_t cz, const float4 *pts, const uint32_t *idx, const uint32_t *off,
                                            uint32_t mask, double &best, uint32_t &best_i, bool &best_dyn, bool &at_min_s, bool &at_min_d) {
    const double gx = (double)g.x, gy = (double)g.y, gz = (double)g.z;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t b = ev_bucket(cx + dx, cy + dy, cz + dz, mask);
                const uint32_t e = off[b + 1];
                for (uint32_t s = off[b]; s < e; ++s) {
                    const float4 p = pts[s];
                    const double ex = gx - (double)p.x, ey = gy - (double)p.y, ez = gz - (double)p.z;
                    const double d2 = (ex * ex + ey * ey) + ez * ez;
                    if (!(d2 <= best)) continue;  // (NaN never wins)
                    uint32_t o_ = 0;
                    const bool e_dyn = ev_is_dynamic(p.w, o_);
                    const uint32_t j = idx[s];
                    if (d2 < best) {
                        best = d2;
                        best_i = j;
                        best_dyn = e_dyn;
                        at_min_s = !e_dyn;
                        at_min_d = e_dyn;
                    } else {
                        if (j < best_i) {
                            best_i = j;
                            best_dyn = e_dyn;
                        }
                        at_min_s = at_min_s || !e_dyn;
                        at_min_d = at_min_d || e_dyn;
                    }
                }
            }
}

// (2) one GT point per lane, read and placed in its cell once, then k_ev_query's decision against estimates
// [blockIdx.y * per_y, + per_y) one after the other (the host launches per_y = 1, see evm_run).  Kept / tied counters in ctr[j * EV_NCTR ..]; the GT's own counters (classes,
// labels out of range, non-finite points) once, by the blocks of blockIdx.y == 0, in row k.
__global__ __launch_bounds__(256) void k_evm_query(const float4 *__restrict__ gt, uint32_t n_gt, const float4 *__restrict__ pts,
                                                    const uint32_t *__restrict__ idx, const uint32_t *__restrict__ off, const EvmEst *__restrict__ tab,
                                                    uint32_t k, uint32_t per_y, double cell, double thr, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n_gt;
    uint32_t gs = 0, gd = 0, oor = 0, bad = 0;
    bool g_dyn = false;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    int32_t cx = 0, cy = 0, cz = 0;
    if (live) {
        g = gt[i];
        bad = ev_finite(g) ? 0u : 1u;
        g_dyn = ev_is_dynamic(g.w, oor);
        gd = g_dyn ? 1u : 0u;
        gs = 1u - gd;
        cx = ev_cell(g.x, cell);
        cy = ev_cell(g.y, cell);
        cz = ev_cell(g.z, cell);
    }
    if (blockIdx.y == 0) {
        unsigned long long *c = ctr + (size_t)k * EV_NCTR;
        ev_commit(c, EV_GT_STATIC, gs);
        ev_commit(c, EV_GT_DYNAMIC, gd);
        ev_commit(c, EV_LABEL_OOR, oor);
        ev_commit(c, EV_NON_FINITE, bad);
    }
    const uint32_t j0 = blockIdx.y * per_y, j1 = min(k, j0 + per_y);
    for (uint32_t j = j0; j < j1; ++j) {
        const EvmEst e = tab[j];
        uint32_t ks = 0, kd = 0, tied = 0;
        if (live && e.n) {
            double best = __builtin_huge_val();
            uint32_t best_i = 0xFFFFFFFFu;
            bool best_dyn = false, at_min_s = false, at_min_d = false;
            evm_nearest(g, cx, cy, cz, pts, idx, off + e.base, e.mask, best, best_i, best_dyn, at_min_s, at_min_d);
            if (best_i != 0xFFFFFFFFu && sqrt(best) < thr) {
                if (!g_dyn && !best_dyn) ks = 1;
                else if (g_dyn && best_dyn) kd = 1;
                tied = (at_min_s && at_min_d) ? 1u : 0u;
            }
        }
        unsigned long long *c = ctr + (size_t)j * EV_NCTR;
        ev_commit(c, EV_KEPT_STATIC, ks);
        ev_commit(c, EV_KEPT_DYNAMIC, kd);
        ev_commit(c, EV_TIED, tied);
    }
}

}  // namespace ek

#endif  // ERASOR_EVALUATE_HIP_H
