// visibility.hip.h — the see-through check: every scan becomes a range image, every map point is voted on by every image
// (erasor_hip_visibility_*).  The reference has no such pass: ERASOR rejects by its bin-wise height test alone, and the reference only
// compares its result against Removert's and OctoMap's maps (README.md:214, compare_results.launch; the panels of img/<seq>/README.md),
// the two methods that argue from visibility -- a map point that later scans look straight through was not static.  This is that
// argument, so that the comparison's other side can be produced, scored (evaluate), drawn (render_eval) and intersected with ERASOR's
// output here.
//
// The contract (the normative text is erasor_amd/evalmap.py: visibility / visibility_brute; the device equals it byte for byte).
// Float64 on the float32 coordinates, every operation a separate IEEE operation in the order written, and only + - * /, sqrt and
// comparisons: the pixel grid is data, two tables of tangents (erasor_visibility.col_tan / row_tan), so no pixel needs atan2, whose last
// bit at sector boundaries kernels.hip.h and the shim already had to document.
//   * the pixel of (x, y, z) in a lidar frame is evalmap.visibility_column's and _vis_pixels': a = |x|, b = |y|, t = min / max, j = the
//     number of col_tan entries <= t; the quadrant from x < 0 and y < 0, the octant o = 2 q + odd with odd = (a < b) in quadrants 0 and
//     2 and !(a < b) in 1 and 3; column o M + j in an even octant, o M + (M - 1) - j mirrored in an odd one (M = W / 8); row = (the
//     number of row_tan entries <= z / sqrt(x x + y y)) - 1; rho = sqrt((x x + y y) + z z);
//   * the gates, in this order: a non-finite coordinate, on the axis (a == b == 0), rho outside [min_range, max_range], a row outside
//     0 .. H - 1 (out of view);
//   * a scan point that passes puts the bits of (float)rho into its pixel by an integer atomic minimum (non-negative floats order as
//     their bits: the image does not depend on the order of the points); an empty pixel is all ones;
//   * a map point p goes into frame f as q = ((r0 x + r1 y) + r2 z) + t per row of the frame's 12 doubles (the host's rigid inverse of
//     T_body2origin . T_lidar2body); where it passes the gates it is in view, and with m = margin_abs + margin_rel rho the non-empty
//     pixels r of the (2 w + 1)^2 window around its own (columns wrap, rows clip) decide: HIT (some rho - m <= r <= rho + m), else
//     OCCLUDED (some r < rho - m), else NO RETURN (all empty), else THROUGH; with normals a THROUGH becomes GRAZING when
//     |n . v| < min_cos sqrt(v . v), v = p - the frame's origin, unless the normal is NaN;
//   * the decision: removed iff through >= min_through and (double)through > hit_weight (double)hit.
//
// k_vis_image: one scan point per lane, all frames of a batch in one launch; a lane finds its frame with al_frame_of over its
// workgroup's frame span, as k_al_query does.  The drop counters and the count of pixels filled (the atomic minimum that found the
// pixel empty: exactly one per filled pixel, whatever the order) go through LDS counters per frame of the span and are added once per
// frame and workgroup; a workgroup that spans more than VI_SLOTS frames (frames of a handful of points) adds per lane instead.
// k_vis_vote: one map point per lane, the point and its normal loaded once, a loop over the batch's frames whose 12 doubles and origin
// are uniform reads; the range gate rejects before any table search or gather; both tables sit in LDS and are binary-searched; the four
// votes stay in registers and are added to the lane's own row at the end with a plain load and store (the lane owns the row); the
// verdict counts of a frame are a ballot per verdict and wavefront into LDS counters, flushed once per frame and workgroup.
// k_vis_decide: the keep flag, the mask and the removed dynamic / static counts per wavefront; the kept cloud is the project's stable
// compaction (scan_u32 + k_f_compact), as density_filter's.
//
// Resources (the compiler's report for gfx950): k_vis_image 24 VGPRs, 6 784 B of LDS; k_vis_vote 46 VGPRs, 9 216 B of LDS; no scratch,
// 8 wavefronts per SIMD for both (MEASUREMENTS.md "Visibility").
#ifndef ERASOR_VISIBILITY_HIP_H
#define ERASOR_VISIBILITY_HIP_H

namespace ek {

static constexpr uint32_t VIS_EMPTY = 0xFFFFFFFFu;  // an empty pixel
static constexpr uint32_t VIS_MAX_W = 4096, VIS_MAX_H = 256;
static constexpr uint32_t VIS_TAB = VIS_MAX_W / 8 - 1 + VIS_MAX_H + 1;  // both tables back to back: col_tan [M - 1], row_tan [H + 1]
static constexpr uint32_t VI_SLOTS = 32;    // k_vis_image: frames of a workgroup's span with LDS counters
static constexpr uint32_t VV_FCHUNK = 128;  // k_vis_vote: frames between two flushes of the LDS counters

// the gates of a point (the first that rejects)
enum : uint32_t { VIS_OK = 0, VIS_G_NON_FINITE, VIS_G_AXIS, VIS_G_RANGE, VIS_G_VIEW };
// the verdicts of a map point in a frame, and "not in view"
enum : uint32_t { VIS_HIT = 0, VIS_OCCLUDED, VIS_NO_RETURN, VIS_THROUGH, VIS_GRAZING, VIS_NVERDICT, VIS_NOT_IN_VIEW = VIS_NVERDICT };
// counters of one frame (VIS_NCTR per frame, zeroed by the host): the scan's drops by gate, the pixels filled, the map points in view
// and their verdicts
static constexpr uint32_t VIS_C_NON_FINITE = 0, VIS_C_AXIS = 1, VIS_C_RANGE = 2, VIS_C_VIEW = 3, VIS_C_PIXELS = 4, VIS_C_IN_VIEW = 5,
                          VIS_C_VERDICT = 6 /* + the verdict */, VIS_NCTR = VIS_C_VERDICT + (uint32_t)VIS_NVERDICT;
static constexpr uint32_t VI_NCTR = VIS_C_PIXELS + 1;      // what k_vis_image counts
static constexpr uint32_t VV_NCTR = VIS_NCTR - VI_NCTR;    // what k_vis_vote counts
// counters of the decision: the rarer events (the kept points and those never in view are what is left of n; counting those instead
// cost 3.6 ms where this costs 0.2 .. 0.4 ms, MEASUREMENTS.md "Visibility")
enum : uint32_t { VD_C_REMOVED_DYNAMIC = 0, VD_C_REMOVED_STATIC, VD_C_SEEN, VD_NCTR };

struct VisParams {
    uint32_t W, H, M, window;
    double min_range, max_range, margin_abs, margin_rel, min_cos;
};
// a frame: the map-to-lidar transform (per row r0, r1, r2, t) and the lidar's origin in the map frame
struct VisFrame {
    double m[12];
    double o[3];
    double pad;
};
// a map point's votes
struct alignas(8) VisVote {
    uint16_t in_view, hit, through, occluded;
};

// the number of entries of tab[0 .. n) that are <= v (tab strictly increasing, v not NaN)
__device__ __forceinline__ uint32_t vis_count_le(const double *tab, uint32_t n, double v) {
    uint32_t lo = 0, hi = n;  // entries below lo are <= v, entries from hi on are > v
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (tab[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// both tables into LDS (every lane of the workgroup calls this; a barrier follows)
__device__ __forceinline__ void vis_load_tabs(double *tab, const double *__restrict__ tabs, const VisParams &P) {
    const uint32_t nt = (P.M - 1) + (P.H + 1);
    for (uint32_t j = threadIdx.x; j < nt; j += blockDim.x) tab[j] = tabs[j];
    __syncthreads();
}

// The gates and the pixel of a finite point in a lidar frame: evalmap.visibility_column and _vis_pixels, operation by operation.
// tab: col_tan then row_tan.  *rho is set unless the point is on the axis; *col and *row when VIS_OK is returned.
__device__ __forceinline__ uint32_t vis_pixel(double x, double y, double z, const VisParams &P, const double *tab, double *rho, uint32_t *col,
                                              uint32_t *row) {
    const double a = fabs(x), b = fabs(y);
    if (a == 0.0 && b == 0.0) return VIS_G_AXIS;
    const double xy = x * x + y * y;
    const double r = sqrt(xy + z * z);
    *rho = r;
    if (!(r >= P.min_range && r <= P.max_range)) return VIS_G_RANGE;  // (before any table search)
    const bool swap = a < b;
    const double t = swap ? a / b : b / a;
    const uint32_t j = vis_count_le(tab, P.M - 1, t);
    const uint32_t q = x < 0 ? (y < 0 ? 2u : 1u) : (y < 0 ? 3u : 0u);
    const bool odd = (q & 1u) ? !swap : swap;
    const uint32_t o = 2 * q + (odd ? 1u : 0u);
    const double s = z / sqrt(xy);
    const uint32_t r1 = vis_count_le(tab + (P.M - 1), P.H + 1, s);  // the row + 1
    if (r1 == 0 || r1 > P.H) return VIS_G_VIEW;
    *col = odd ? o * P.M + (P.M - 1) - j : o * P.M + j;
    *row = r1 - 1;
    return VIS_OK;
}

// (1) one scan point per lane: workgroup blockIdx.x covers the points (b0 + blockIdx.x) * 256 .. of the concatenated scans, of which
// [lo, hi) belong to the batch's frames [f0, f1).  off: [n_frames + 1] point offsets; wg: wg[b] the frame of point b * 256 (the last
// frame after the last point), over ALL workgroups of the scans.  img: [f1 - f0][H][W], all ones; ctr: [n_frames][VIS_NCTR].
__global__ __launch_bounds__(256) void k_vis_image(const float4 *__restrict__ scans, uint32_t lo, uint32_t hi, uint32_t b0,
                                                    const uint32_t *__restrict__ off, const uint32_t *__restrict__ wg, uint32_t f0, uint32_t f1,
                                                    VisParams P, const double *__restrict__ tabs, uint32_t *__restrict__ img,
                                                    unsigned long long *__restrict__ ctr) {
    __shared__ double tab[VIS_TAB];
    __shared__ uint32_t lc[VI_SLOTS * VI_NCTR];  // [frame of the span][counter]
    const uint32_t t = threadIdx.x, b = b0 + blockIdx.x, i = b * 256u + t;
    for (uint32_t j = t; j < VI_SLOTS * VI_NCTR; j += 256u) lc[j] = 0u;
    vis_load_tabs(tab, tabs, P);
    // the frames this workgroup touches, inside the batch
    const uint32_t fa = wg[b] > f0 ? wg[b] : f0, fz = wg[b + 1] < f1 - 1 ? wg[b + 1] : f1 - 1;
    const bool local = fz < fa + VI_SLOTS;
    if (i >= lo && i < hi) {
        const uint32_t f = al_frame_of(off, i, fa, fz);
        const float4 p = scans[i];
        uint32_t c;  // the counter this point adds to, VI_NCTR: none
        if (!ev_finite(p)) {
            c = VIS_C_NON_FINITE;
        } else {
            double rho = 0.0;
            uint32_t col = 0, row = 0;
            const uint32_t g = vis_pixel((double)p.x, (double)p.y, (double)p.z, P, tab, &rho, &col, &row);
            if (g == VIS_OK) {
                const uint32_t bits = __builtin_bit_cast(uint32_t, (float)rho);
                const uint32_t old = atomicMin(&img[((size_t)(f - f0) * P.H + row) * P.W + col], bits);
                c = old == VIS_EMPTY ? VIS_C_PIXELS : VI_NCTR;  // (exactly one minimum finds a filled pixel empty)
            } else {
                c = g - VIS_G_NON_FINITE;  // (the gates' counters are in the gates' order)
            }
        }
        if (c < VI_NCTR) {
            if (local) atomicAdd(&lc[(f - fa) * VI_NCTR + c], 1u);
            else atomicAdd(&ctr[(size_t)f * VIS_NCTR + c], 1ull);
        }
    }
    __syncthreads();
    if (local && fz >= fa) {
        const uint32_t m = (fz - fa + 1) * VI_NCTR;
        for (uint32_t j = t; j < m; j += 256u)
            if (lc[j]) atomicAdd(&ctr[(size_t)(fa + j / VI_NCTR) * VIS_NCTR + j % VI_NCTR], (unsigned long long)lc[j]);
    }
}

// (2) one map point per lane against the frames [f0, f1) of a batch.  nrm: [n][3] the map's normals, or NULL (no incidence gate);
// frames: [n_frames]; img: the batch's images; votes: [n], the lane's own row, added to; ctr: [n_frames][VIS_NCTR].
__global__ __launch_bounds__(256) void k_vis_vote(const float4 *__restrict__ map, uint32_t n, const float *__restrict__ nrm,
                                                   const VisFrame *__restrict__ frames, uint32_t f0, uint32_t f1, VisParams P,
                                                   const double *__restrict__ tabs, const uint32_t *__restrict__ img, VisVote *__restrict__ votes,
                                                   unsigned long long *__restrict__ ctr) {
    __shared__ double tab[VIS_TAB];
    __shared__ uint32_t lc[VV_FCHUNK * VV_NCTR];  // [frame of the chunk][in view, the verdicts]
    const uint32_t t = threadIdx.x, i = blockIdx.x * 256u + t;
    for (uint32_t j = t; j < VV_FCHUNK * VV_NCTR; j += 256u) lc[j] = 0u;
    vis_load_tabs(tab, tabs, P);
    bool fin = false, gated = false;
    double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    if (i < n) {
        const float4 p = map[i];
        fin = ev_finite(p);
        px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        if (nrm) {
            nx = (double)nrm[(size_t)i * 3 + 0], ny = (double)nrm[(size_t)i * 3 + 1], nz = (double)nrm[(size_t)i * 3 + 2];
            gated = nx == nx;  // (a NaN normal gates nothing)
        }
    }
    const uint32_t w = P.window, HW = P.H * P.W;
    uint32_t n_in = 0, n_hit = 0, n_thr = 0, n_occ = 0;
    for (uint32_t fc = f0; fc < f1; fc += VV_FCHUNK) {
        const uint32_t fe = fc + VV_FCHUNK < f1 ? fc + VV_FCHUNK : f1;
        for (uint32_t f = fc; f < fe; ++f) {  // (uniform over the workgroup)
            uint32_t v = VIS_NOT_IN_VIEW;
            if (fin) {
                const VisFrame &F = frames[f];
                const double qx = ((F.m[0] * px + F.m[1] * py) + F.m[2] * pz) + F.m[3];
                const double qy = ((F.m[4] * px + F.m[5] * py) + F.m[6] * pz) + F.m[7];
                const double qz = ((F.m[8] * px + F.m[9] * py) + F.m[10] * pz) + F.m[11];
                double rho = 0.0;
                uint32_t col = 0, row = 0;
                if (vis_pixel(qx, qy, qz, P, tab, &rho, &col, &row) == VIS_OK) {
                    const double m = P.margin_abs + P.margin_rel * rho;
                    const double lo = rho - m, hi = rho + m;
                    const uint32_t *im = img + (size_t)(f - f0) * HW;
                    bool hit = false, occ = false, some = false;
                    const uint32_t ra = row >= w ? row - w : 0u, rz = row + w < P.H ? row + w : P.H - 1;  // rows clip
                    for (uint32_t rr = ra; rr <= rz; ++rr) {
                        for (uint32_t dc = 0; dc <= 2 * w; ++dc) {
                            uint32_t cc = col + P.W + dc - w;  // columns wrap (w <= 2 < W)
                            if (cc >= P.W) cc -= P.W;
                            if (cc >= P.W) cc -= P.W;
                            const uint32_t bits = im[rr * P.W + cc];
                            if (bits != VIS_EMPTY) {
                                const double r = (double)__builtin_bit_cast(float, bits);
                                some = true;
                                hit = hit || (lo <= r && r <= hi);
                                occ = occ || r < lo;
                            }
                        }
                    }
                    v = hit ? VIS_HIT : (occ ? VIS_OCCLUDED : (!some ? VIS_NO_RETURN : VIS_THROUGH));
                    if (v == VIS_THROUGH && gated) {
                        const double vx = px - F.o[0], vy = py - F.o[1], vz = pz - F.o[2];
                        const double dot = (nx * vx + ny * vy) + nz * vz;
                        const double vv = (vx * vx + vy * vy) + vz * vz;
                        if (fabs(dot) < P.min_cos * sqrt(vv)) v = VIS_GRAZING;
                    }
                    ++n_in;
                    n_hit += v == VIS_HIT ? 1u : 0u;
                    n_thr += v == VIS_THROUGH ? 1u : 0u;
                    n_occ += v == VIS_OCCLUDED ? 1u : 0u;
                }
            }
            // the frame's counts: a ballot per verdict and wavefront
            const uint64_t in = __ballot(v != VIS_NOT_IN_VIEW);
            if (in) {
                uint32_t *c = lc + (f - fc) * VV_NCTR;
                const bool lead = (t & 63u) == 0;
                if (lead) atomicAdd(&c[0], (uint32_t)__popcll(in));
#pragma unroll
                for (uint32_t k = 0; k < VIS_NVERDICT; ++k) {
                    const uint32_t cnt = (uint32_t)__popcll(__ballot(v == k));
                    if (lead && cnt) atomicAdd(&c[1 + k], cnt);
                }
            }
        }
        __syncthreads();
        const uint32_t m = (fe - fc) * VV_NCTR;
        for (uint32_t j = t; j < m; j += 256u) {
            const uint32_t x = lc[j];
            if (x) {
                atomicAdd(&ctr[(size_t)(fc + j / VV_NCTR) * VIS_NCTR + VIS_C_IN_VIEW + j % VV_NCTR], (unsigned long long)x);
                lc[j] = 0u;
            }
        }
        __syncthreads();
    }
    if (i < n && n_in) {
        VisVote r = votes[i];
        r.in_view = (uint16_t)(r.in_view + n_in);
        r.hit = (uint16_t)(r.hit + n_hit);
        r.through = (uint16_t)(r.through + n_thr);
        r.occluded = (uint16_t)(r.occluded + n_occ);
        votes[i] = r;
    }
}

// (3) the decision per map point: flag (uint32, for the compaction's scan) and mask (uint8, the caller's), 1 = kept; the counters per
// wavefront, removed points by label as k_kn_keep counts them, and the points in view of some frame
__global__ __launch_bounds__(256) void k_vis_decide(const float4 *__restrict__ map, uint32_t n, const VisVote *__restrict__ votes, uint32_t min_through,
                                                     double hit_weight, uint32_t *__restrict__ flag, uint8_t *__restrict__ mask,
                                                     unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rd = 0, rs = 0, seen = 0;
    if (i < n) {
        const VisVote r = votes[i];
        const bool removed = (uint32_t)r.through >= min_through && (double)r.through > hit_weight * (double)r.hit;
        seen = r.in_view ? 1u : 0u;
        flag[i] = removed ? 0u : 1u;
        mask[i] = removed ? (uint8_t)0 : (uint8_t)1;
        if (removed) {
            uint32_t oor = 0;
            if (ev_is_dynamic(map[i].w, oor)) rd = 1; else rs = 1;
        }
    }
    ev_commit(ctr, VD_C_REMOVED_DYNAMIC, rd);
    ev_commit(ctr, VD_C_REMOVED_STATIC, rs);
    ev_commit(ctr, VD_C_SEEN, seen);
}

}  // namespace ek

#endif  // ERASOR_VISIBILITY_HIP_H
