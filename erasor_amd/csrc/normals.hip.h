// normals.hip.h — every point's surface normal, curvature and covariance eigenvalues from its k nearest neighbours inside its own
// cloud (erasor_hip_normals_*).  What users of a cleaned map compute next on the host with pcl::NormalEstimation over a KD-tree of the
// whole map; what a point-to-plane registration, a shaded rendering and telling a wall from scatter all start from.
//
// The contract (restated on the host by erasor_amd/evalmap.py: normals / normals_brute / _jacobi3; the device equals it byte for byte).
// Everything is float64 on the float32 coordinates, every operation a separate IEEE operation in the order written:
//   * the neighbourhood of point i: the point itself first, then its k nearest other points in knn.hip.h's order, (d2, j) ascending,
//     self excluded by index: m = k + 1 points, 2 <= k <= 32.  A point with fewer than k other points is SHORT: its normal, curvature
//     and eigenvalues are NaN and it is counted in n_short;
//   * centroid, per axis: s = ((0.0 + p_self) + p_n0) + ... in list order, c = s / (double)m;
//   * covariance: for each neighbourhood point in the same order e = p - c, and cxx = cxx + ex*ex (cxy, cxz, cyy, cyz, czz alike), each
//     from 0.0; after the loop each entry divided by (double)m (PCL's scale); tr = (cxx + cyy) + czz, taken before the solve;
//   * a point is DEGENERATE if !(tr > 0) (all m points identical): NaN outputs, counted in n_degenerate;
//   * the eigen-solve: cyclic Jacobi on the symmetric 3x3 with the pivots (0,1), (0,2), (1,2) and the rotation of the 4x4 solve of
//     refine_poses (theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrt(theta*theta + 1)), c = 1 / sqrt(t*t + 1), s = t c;
//     A <- A J, A <- Jt A, apq = 0, V <- V J); a pivot that is exactly 0 is skipped; it stops when the three off-diagonals are exactly 0
//     before a sweep, or after 32 sweeps.  A division that overflows gives +-inf, a value like any other.  The eigenvalues are the
//     diagonal, listed ascending by (value, column index); the normal is the column of V of the first one, not renormalised;
//   * n_ambiguous counts the points whose two smallest eigenvalues are exactly equal (an exactly collinear neighbourhood: the normal
//     is defined by the rules above, but arbitrary);
//   * curvature = fabs(l0) / tr (PCL's);
//   * orientation: with a viewpoint v (three finite float64) s = ((vx-px)*nx + (vy-py)*ny) + (vz-pz)*nz and the normal is negated iff
//     s < 0; without one ("up") iff nz < 0, or nz == 0 and ny < 0, or nz == ny == 0 and nx < 0.  n_flipped counts the negations;
//   * outputs: the normal's float64 components rounded once to float32; curvature and the three eigenvalues (ascending) as float64;
//     the statistics of the finite curvatures as knn.hip.h takes a score's.
// Not offered: a radius neighbourhood (its point count is unbounded, so the list has no fixed LDS size, and the sums' terms would have
// no bounded order) and MLS smoothing -- knn.hip.h's reason about sums whose value depends on the order of their terms.  PCL is not a
// dependency of this project and nothing is pinned against it.
//
// Search (k_nm_query): knn.hip.h's, unchanged -- one query per lane in the tree's sorted order, nn_walk at the stride KN_QBLOCK with the
// visitor KnList and its [entry][lane] list in LDS.  The finishing pass then walks the lane's sorted list twice (centroid, covariance),
// fetching the neighbours' coordinates from the cloud by their original indices, and solves in registers: the six entries of A and
// the nine of V are named scalars and the three pivots are written out, so nothing is indexed at run time and nothing goes to scratch.
//
// Resources (the compiler's report for gfx950, KC = 8 / 16 / 32): 62 / 62 / 62 VGPRs, 0 B of scratch, LDS 25 600 / 37 888 / 62 464 B
// per workgroup -- k_kn_query's at the same KC (128 * (KC * 12 + 26 * 4) B), so by the same arithmetic against the CU's 163 840 B
// 6 / 4 / 2 workgroups (12 / 8 / 4 wavefronts) per CU; the registers would allow 8 wavefronts per SIMD and do not bind.
//
// Inherited hazards, stated and not solved: m identical points make every one of them visit all m in the search, and a
// crowded cell is walked point by point.
#ifndef ERASOR_NORMALS_HIP_H
#define ERASOR_NORMALS_HIP_H

namespace ek {

static constexpr uint32_t NM_MIN_K = 2;
static constexpr uint32_t NM_SWEEPS = 32;

// counters of one call (zeroed by the host, NM_C_CURV_MIN set to all ones): one 64-bit atomic per wavefront and counter
enum : uint32_t {
    NM_C_SHORT = 0,    // points with fewer than k other points
    NM_C_DEGENERATE,   // points whose covariance has no positive trace
    NM_C_AMBIGUOUS,    // points whose two smallest eigenvalues are equal
    NM_C_FLIPPED,      // normals negated by the orientation rule
    NM_C_CURV_MIN,     // the smallest / largest curvature's bit pattern (curvatures are >= +0: unsigned order is numeric order)
    NM_C_CURV_MAX,
    NM_NCTR
};

// one Jacobi rotation on the pivot (p, q) of a symmetric 3x3, r the third index: app, aqq, apq and the two entries apr, aqr beside them,
// and the columns p and q of V.  A pivot that is exactly 0 is skipped.
__device__ __forceinline__ void nm_rotate(double &app, double &aqq, double &apq, double &apr, double &aqr, double &v0p, double &v0q, double &v1p,
                                          double &v1q, double &v2p, double &v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    // A <- A J, then A <- Jt A: the four entries of the pivot's block, and the two beside it
    const double bpp = c * app - s * apq, bpq = s * app + c * apq;
    const double bqp = c * apq - s * aqq, bqq = s * apq + c * aqq;
    const double npr = c * apr - s * aqr, nqr = s * apr + c * aqr;
    app = c * bpp - s * bqp;
    aqq = s * bpq + c * bqq;
    apq = 0.0;
    apr = npr;
    aqr = nqr;
    // V <- V J
    const double n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const double n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const double n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    v0p = n0p, v0q = n0q, v1p = n1p, v1q = n1q, v2p = n2p, v2q = n2q;
}

// One query per lane, in the tree's sorted order, as k_kn_query: lane s finds the k nearest other points of T.pts[s] (original index
// T.idx[s]) and from them and itself the normal, curvature and eigenvalues of that point.  T: the tree over pts[0 .. T.n) (T.n > 0, every
// point finite); pts: the cloud in its original order.  view: 1 with the viewpoint (vx, vy, vz), 0 for "up".  curv_bits ([n]): the
// curvature's bit pattern at the point's original index; nrm ([n][3]) and eig ([n][3]): optional.  KC: the list's capacity, k <= KC.
template <uint32_t KC>
__global__ __launch_bounds__(KN_QBLOCK) void k_nm_query(NnTree T, const float4 *__restrict__ pts, uint32_t k, uint32_t view, double vx, double vy,
                                                         double vz, float *__restrict__ nrm, unsigned long long *__restrict__ curv_bits,
                                                         double *__restrict__ eig, unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * KN_QBLOCK];  // [depth][lane]
    __shared__ double ld[KC * KN_QBLOCK];              // [entry][lane]: the list's d2 ...
    __shared__ uint32_t li[KC * KN_QBLOCK];            // ... and original index
    const uint32_t t = threadIdx.x, s = blockIdx.x * KN_QBLOCK + t;
    uint32_t is_short = 0, is_degenerate = 0, is_ambiguous = 0, is_flipped = 0;
    unsigned long long cb = 0ull;
    bool scored = false;
    if (s < T.n) {
        const float4 q = T.pts[s];
        const uint32_t self = T.idx[s];
        const double px = (double)q.x, py = (double)q.y, pz = (double)q.z;
        KnList v{px, py, pz, s, k, t, ld, li};
        nn_walk<KN_QBLOCK>(v, T, stack, t);
        const double nan = __builtin_nan("");
        double nx = nan, ny = nan, nz = nan, curv = nan, l0 = nan, l1 = nan, l2 = nan;
        is_short = v.cnt < k ? 1u : 0u;
        if (!is_short) {
            const double m = (double)(k + 1);
            // the centroid: the point itself, then the list in its order
            double sx = 0.0 + px, sy = 0.0 + py, sz = 0.0 + pz;
            for (uint32_t e = 0; e < k; ++e) {
                const float4 p = pts[li[e * KN_QBLOCK + t]];
                sx = sx + (double)p.x;
                sy = sy + (double)p.y;
                sz = sz + (double)p.z;
            }
            const double cx = sx / m, cy = sy / m, cz = sz / m;
            // the covariance, in the same order
            double ex = px - cx, ey = py - cy, ez = pz - cz;
            double a00 = 0.0 + ex * ex, a01 = 0.0 + ex * ey, a02 = 0.0 + ex * ez, a11 = 0.0 + ey * ey, a12 = 0.0 + ey * ez, a22 = 0.0 + ez * ez;
            for (uint32_t e = 0; e < k; ++e) {
                const float4 p = pts[li[e * KN_QBLOCK + t]];
                ex = (double)p.x - cx, ey = (double)p.y - cy, ez = (double)p.z - cz;
                a00 = a00 + ex * ex;
                a01 = a01 + ex * ey;
                a02 = a02 + ex * ez;
                a11 = a11 + ey * ey;
                a12 = a12 + ey * ez;
                a22 = a22 + ez * ez;
            }
            a00 = a00 / m, a01 = a01 / m, a02 = a02 / m, a11 = a11 / m, a12 = a12 / m, a22 = a22 / m;
            const double tr = (a00 + a11) + a22;
            is_degenerate = tr > 0 ? 0u : 1u;
            if (!is_degenerate) {
                double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
                for (uint32_t sweep = 0; sweep < NM_SWEEPS; ++sweep) {
                    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
                    nm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0,1), beside it column 2
                    nm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0,2), beside it column 1
                    nm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1,2), beside it column 0
                }
                // ascending by (value, column): the ranks of columns 0 and 1 (column 2 has the one that is left)
                const uint32_t r0 = (a11 < a00 ? 1u : 0u) + (a22 < a00 ? 1u : 0u);
                const uint32_t r1 = (a00 <= a11 ? 1u : 0u) + (a22 < a11 ? 1u : 0u);
                l0 = r0 == 0 ? a00 : (r1 == 0 ? a11 : a22);
                l1 = r0 == 1 ? a00 : (r1 == 1 ? a11 : a22);
                l2 = r0 == 2 ? a00 : (r1 == 2 ? a11 : a22);
                nx = r0 == 0 ? v00 : (r1 == 0 ? v01 : v02);
                ny = r0 == 0 ? v10 : (r1 == 0 ? v11 : v12);
                nz = r0 == 0 ? v20 : (r1 == 0 ? v21 : v22);
                is_ambiguous = l0 == l1 ? 1u : 0u;
                curv = fabs(l0) / tr;
                bool flip;
                if (view) {
                    const double sd = ((vx - px) * nx + (vy - py) * ny) + (vz - pz) * nz;
                    flip = sd < 0;
                } else {
                    flip = nz < 0 || (nz == 0 && (ny < 0 || (ny == 0 && nx < 0)));
                }
                if (flip) nx = -nx, ny = -ny, nz = -nz;
                is_flipped = flip ? 1u : 0u;
                scored = true;
            }
        }
        cb = __builtin_bit_cast(unsigned long long, curv);
        curv_bits[self] = cb;
        if (nrm) {
            nrm[(size_t)self * 3 + 0] = (float)nx;
            nrm[(size_t)self * 3 + 1] = (float)ny;
            nrm[(size_t)self * 3 + 2] = (float)nz;
        }
        if (eig) {
            eig[(size_t)self * 3 + 0] = l0;
            eig[(size_t)self * 3 + 1] = l1;
            eig[(size_t)self * 3 + 2] = l2;
        }
    }
    ev_commit(ctr, NM_C_SHORT, is_short);
    ev_commit(ctr, NM_C_DEGENERATE, is_degenerate);
    ev_commit(ctr, NM_C_AMBIGUOUS, is_ambiguous);
    ev_commit(ctr, NM_C_FLIPPED, is_flipped);
    kn_commit_range(ctr, NM_C_CURV_MIN, NM_C_CURV_MAX, cb, scored);
}

}  // namespace ek

#endif  // ERASOR_NORMALS_HIP_H
