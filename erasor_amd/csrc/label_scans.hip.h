// label_scans.hip.h — every scan's points labelled static or moving from a cleaned map, all frames in one call
// (erasor_hip_label_scans_*): what users of a cleaned map do next, carry the result back to the scans (moving-object-segmentation
// labels, the cleaned scans for re-localisation).
//
// Frame f is put into the map frame as align.hip.h puts it (T_lidar2body, then the frame's T_body2origin, xform's association).  A
// point is static (0) when the static map has a point at float64 distance d < tau from it; else dynamic (1) when no raw map was given
// or the raw map has such a point; else unknown (2); a point with a non-finite coordinate after the transforms is dropped (255).
//
// The question is "is there a map point within tau", not "where is the nearest one": nn_exists_f64 runs nearest.hip.h's shared
// traversal, nn_walk, (depth first, nearer child first, the pending siblings on the per-lane LDS stack) with the bound FIXED at T2,
// the largest double whose correctly rounded sqrt is < tau (the host finds it with nextafter), and returns at the first leaf point
// with d^2 <= T2.
//
// Why this equals the host's answer (evalmap.label_scans), with no epsilon: its d is sqrt(min d^2), d^2 = (ex*ex + ey*ey) + ez*ez in
// float64 (what cKDTree returns; nearest.hip.h reproduces it bit for bit), and the correctly rounded sqrt is monotone, so d < tau <=>
// min d^2 <= T2 <=> some map point has d^2 <= T2.  The walker prunes a box only when nn_lb, its exact lower bound (nearest.hip.h's
// header), is > T2, and a sibling that passed the fixed bound when it was pushed still passes it when it is popped: no point with
// d^2 <= T2 is ever skipped.
//
// Why it never works harder than the exact search (nn_search_f64: the same walker, the bound its best d^2) on the same tree: until the
// exact search meets its first point with d^2 <= T2 its bound is > T2, so it enters every box this search enters (and more), in the
// same order -- where both children pass here both pass there and the nearer is the same; where one passes here it is the one with the
// smaller bound, which the exact search takes first too.  At that first point this search stops; the exact one goes on.  When no such
// point exists the exact search's bound stays > T2 throughout.
//
// k_ls_query: one scan point per lane.  The static pass runs over all points with k_al_query's frame lookup (the host gives every
// workgroup the frames it touches).  With a raw map the points the static pass left are compacted into a list of their indices (a flag
// per point, the project's two-level scan, a scatter) and the raw pass runs over that list alone, one left point per lane, against the
// raw map's tree built in the SAME scratch: one tree resident at a time.  Counters per frame: one atomic per frame, counter and
// wavefront, on ballots, as in k_al_query.
//
// The split (the rows of one code, as given, frame by frame in scan order) is a stable compaction over the concatenated scans: frames
// are consecutive ranges, so the global order is the per-frame order; a flag per point, the scan, k_f_compact's scatter, and the
// per-frame offsets from the frames' counters.
#ifndef ERASOR_LABEL_SCANS_HIP_H
#define ERASOR_LABEL_SCANS_HIP_H

namespace ek {

// counters of one frame (LS_NCTR per frame): n[gt moving][code] at gt * 3 + code, then the two below
enum : uint32_t {
    LS_NON_FINITE = 6,  // points dropped: a non-finite coordinate after the two transforms
    LS_LABEL_OOR,       // kept points whose intensity is not finite or outside [0, 2^32): decoded as static
    LS_NCTR
};

enum : uint8_t { LS_STATIC = 0, LS_DYNAMIC = 1, LS_UNKNOWN = 2, LS_DROPPED = 255 };

// visitor: is there a tree point with float64 d^2 <= T2?  The bound is FIXED at T2 and the search ends at the first such point.
struct NnExistsF64 {
    typedef double real;
    static constexpr bool FIXED = true;
    double qx, qy, qz, T2;
    bool found = false;
#ifdef ERASOR_HIP_TEST_HOOKS
    uint32_t n_leaves = 0, n_points = 0;  // leaves opened, points tested up to and including the hit
#endif
    __device__ __forceinline__ double lb(const float4 &l, const float4 &u) const { return nn_lb(l, u, qx, qy, qz); }
    __device__ __forceinline__ double bound() const { return T2; }
    __device__ __forceinline__ bool leaf(const NnTree &T, uint32_t b, uint32_t e) {
#ifdef ERASOR_HIP_TEST_HOOKS
        ++n_leaves;
#endif
        for (uint32_t s = b; s < e; ++s) {
            const float4 p = T.pts[s];
            const double ex = qx - (double)p.x, ey = qy - (double)p.y, ez = qz - (double)p.z;
            const double d2 = (ex * ex + ey * ey) + ez * ez;
#ifdef ERASOR_HIP_TEST_HOOKS
            ++n_points;
#endif
            if (d2 <= T2) {
                found = true;
                break;
            }
        }
        return found;
    }
};

// is there a tree point with float64 d^2 <= T2 from q (T.n > 0, q finite)?  stack: the workgroup's [NN_STACK][NN_QBLOCK] LDS array,
// t: the lane's column; slot: the query's index for the test hook's effort counts.
__device__ __forceinline__ bool nn_exists_f64(double qx, double qy, double qz, double T2, const NnTree &T, uint32_t *stack, uint32_t t,
                                             uint32_t slot) {
    NnExistsF64 v{qx, qy, qz, T2};
    nn_walk<NN_QBLOCK>(v, T, stack, t);
#ifdef ERASOR_HIP_TEST_HOOKS
    nn_put_effort(v, (size_t)slot);
#else
    (void)slot;
#endif
    return v.found;
}

// one pass of the labelling, one scan point per lane.  list == nullptr: the pass over all n points (wg: [grid + 1], the frame of every
// workgroup's first point, as in k_al_query); else the pass over the n_list left points list[0 .. n_list), ascending.  off: [n_frames +
// 1]; Tb: [n_frames].  A point with a tree point within the bound gets code_hit, the others code_miss; a dropped point LS_DROPPED (first
// pass).  count_miss == 0: the missed points are not counted (a later pass decides them) and left[i] says whether point i is one (left:
// [n], first pass with a raw map to come, else nullptr).  ctr: [n_frames][LS_NCTR], zeroed by the host.  T.n == 0: nothing is hit; T.idx is not read.
__global__ __launch_bounds__(NN_QBLOCK) void k_ls_query(const float4 *__restrict__ scans, uint32_t n, const uint32_t *__restrict__ list,
                                                         uint32_t n_list, const uint32_t *__restrict__ off, uint32_t n_frames,
                                                         const uint32_t *__restrict__ wg, Xf Tl, const Xf *__restrict__ Tb, NnTree T,
                                                         double T2, uint32_t code_hit, uint32_t code_miss, uint32_t count_miss, uint8_t *__restrict__ codes,
                                                         uint32_t *__restrict__ left, unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * NN_QBLOCK];  // [depth][lane], as in k_nn_query
    const uint32_t t = threadIdx.x, j = blockIdx.x * NN_QBLOCK + t;
    const bool valid = list ? j < n_list : j < n;
    uint32_t f = 0, which = LS_NCTR, oor = 0;  // which: the counter this lane adds to (LS_NCTR: none)
    if (valid) {
        const uint32_t i = list ? list[j] : j;
        f = al_frame_of(off, i, list ? 0u : wg[blockIdx.x], list ? n_frames - 1 : wg[blockIdx.x + 1]);
        const float4 s = scans[i];
        const float4 q = xform(Tb[f], xform(Tl, s));
        if (!ev_finite(q)) {  // (first pass only: a left point is finite)
            which = LS_NON_FINITE;
            codes[i] = LS_DROPPED;
            if (left) left[i] = 0u;
        } else {
            const bool hit = T.n && nn_exists_f64((double)q.x, (double)q.y, (double)q.z, T2, T, stack, t, j);
            const uint32_t gt = ev_is_dynamic(s.w, oor) ? 1u : 0u;
            codes[i] = (uint8_t)(hit ? code_hit : code_miss);
            if (left) left[i] = hit ? 0u : 1u;
            if (hit || count_miss) which = gt * 3u + (hit ? code_hit : code_miss);
            else oor = 0u;  // (the pass that decides the point counts its label)
        }
    }
    // one round per frame present in the wavefront (usually one): one atomic per frame and counter, on ballots
    uint64_t todo = __ballot(valid);
    while (todo) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const uint32_t fk = __builtin_amdgcn_readlane(f, lead);
        const bool in = valid && f == fk;
        const uint64_t mine = __ballot(in);
        unsigned long long *c = ctr + (size_t)fk * LS_NCTR;
        const bool leader = (t & 63u) == lead;
#pragma unroll
        for (uint32_t k = 0; k < LS_NCTR; ++k) {
            const uint32_t cnt = (uint32_t)__popcll(__ballot(in && (k == LS_LABEL_OOR ? oor != 0u : which == k)));
            if (leader && cnt) atomicAdd(&c[k], (unsigned long long)cnt);
        }
        todo &= ~mine;
    }
}

// the left points' indices, ascending: list[rank of i among the flagged] = i (flag's scan in pl / tops, as k_f_compact reads it)
__global__ __launch_bounds__(256) void k_ls_list(uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pl,
                                                  const uint32_t *__restrict__ tops, uint32_t *__restrict__ list) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) list[pl[i] + tops[i >> 10]] = i;
}

// the split's flags: the points of one code
__global__ __launch_bounds__(256) void k_ls_flag(const uint8_t *__restrict__ codes, uint32_t n, uint32_t code, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = codes[i] == code ? 1u : 0u;
}

}  // namespace ek

#endif  // ERASOR_LABEL_SCANS_HIP_H
