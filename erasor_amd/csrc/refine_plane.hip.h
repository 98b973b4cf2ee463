// refine_plane.hip.h — every frame's pose refined point-to-plane against the map's own normals, all frames side by side
// (erasor_hip_refine_poses_plane_*).  refine.hip.h moves a frame onto the map's points; on surfaces that converges linearly and stops a
// fraction of the sampling step off, because a scan never samples the map's own points.  Here the residual is the distance to the plane
// through the nearest map point, so a frame slides freely along a surface and only its distance to it counts.
//
// The contract (restated on the host by erasor_amd/evalmap.py: refine_poses_plane / refine_plane_frame_sums / refine_plane_solve /
// _jacobi6; the device equals it byte for byte).  Float64 on the float32 inputs, every operation a separate IEEE operation:
//   * once per call the map's normals N[j] (3 x float32) and curvature C[j] (float64) are what normals.hip.h gives for the map with
//     k = normals_k and no viewpoint; they stay on the device (E.nm_nrm, E.nm_curv) and the map's one tree serves that pass and every
//     iteration.  The orientation rule cannot matter: flipping n negates J and r together -- each is a sum of products with one factor
//     from n, and (-a + -b) + -c = -((a + b) + c) exactly -- so every summed product J[a]*J[b], J[a]*r and r*r is unchanged bit for bit;
//   * per scan point, as in refine.hip.h: p = xform(T_lidar2body, row) in float32, q' = R p and q = q' + t in float64; a non-finite
//     point has no query and is counted; nn_search_f64 gives j and d2, ties to the lowest index;
//   * a CANDIDATE: d2 <= gate2 (max_dist * max_dist, formed by the host).  A PAIR: a candidate whose N[j] has three finite components
//     and C[j] <= max_curvature.  Any other candidate is UNUSABLE: counted, and +0.0 in every sum;
//   * for a pair n = (double)N[j], m = (double)map[j], e = q - m, r = (ex*nx + ey*ny) + ez*nz, c = q' x n
//     (cx = q'y*nz - q'z*ny, cy = q'z*nx - q'x*nz, cz = q'x*ny - q'y*nx) and J = (cx, cy, cz, nx, ny, nz);
//   * its RFP_NSUM = 29 sums: 0..20 J[a]*J[b] for a <= b (upper triangle, row-major), 21..26 J[a]*r, 27 r*r, 28 d2, added by
//     refine.hip.h's rule (rf_reduce per chunk of 256 from the frame's own first point, k_rf_partials over the chunks from 0.0);
//   * the solve is the host's (analysis_host.hip.h, rfp_solve): the symmetric 6x6 A from sums 0..20 and b = -S[21..26], cyclic Jacobi,
//     a pseudo-inverse over the eigen-directions with lambda_i > rank_tol * lambda_max, a rotation from the half vector without
//     trigonometry.  The eigenvalues mix radians and metres (the first three rows of J are lengths, the last three pure numbers), as
//     every 6-DoF degeneracy test does: rank_tol is therefore a parameter, and lambda_ratio is reported beside the rank.
//
// k_rfp_query is k_rf_query's shape: one scan point per lane, one chunk per workgroup, live[f] uniform over the workgroup, the walk's
// 26 KB stack reused for the tree across the wavefronts -- RFP_GROUP = 10 components at a time (20 KB; 29 x 256 doubles do not fit at
// once), so three groups and six barriers.  The 29 sums are formed only after the walk, from j, d2, q' and q: the walk's registers are
// dead by then, and the sums are indexed by constants only.  Three integer counters per frame, one atomic per wavefront each; no float
// atomics.
//
// Resources (the compiler's report for gfx950): k_rfp_query 119 VGPRs, 0 B of scratch, no spilled register, LDS 26 624 B per workgroup
// (the stack) -- 4 wavefronts per SIMD by the registers, 6 workgroups (24 wavefronts) per CU by the LDS; k_rf_query beside it: 130
// VGPRs and 3 wavefronts per SIMD, the same before and after its reduction moved into rf_reduce.
#ifndef ERASOR_REFINE_PLANE_HIP_H
#define ERASOR_REFINE_PLANE_HIP_H

namespace ek {

static constexpr uint32_t RFP_NSUM = 29;   // J[a]*J[b], a <= b row-major (0..20), J[a]*r (21..26), r*r (27), d2 (28)
static constexpr uint32_t RFP_GROUP = 10;  // components that cross the wavefronts together

// counters of one frame (RFP_NCTR per frame)
enum : uint32_t {
    RFP_PAIRS = 0,   // candidates with a usable normal
    RFP_NON_FINITE,  // points without a query, as RF_NON_FINITE
    RFP_UNUSABLE,    // candidates whose map point has a non-finite normal or a curvature above max_curvature
    RFP_NCTR
};

// One scan point per lane, one chunk per workgroup; arguments as k_rf_query's.  nrm: [T.n][3], curv_bits: [T.n] (the curvature's bit
// pattern), both at the map's own indices, as k_nm_query leaves them.  part: [grid][RFP_NSUM]; ctr: [n_frames][RFP_NCTR], zeroed by the
// host.  T.n > 0.
__global__ __launch_bounds__(NN_QBLOCK) void k_rfp_query(const float4 *__restrict__ scans, const uint32_t *__restrict__ off,
                                                          const RfChunk *__restrict__ chunks, Xf Tl, const RfPose *__restrict__ pose,
                                                          const uint32_t *__restrict__ live, const float4 *__restrict__ map,
                                                          const float *__restrict__ nrm, const unsigned long long *__restrict__ curv_bits, NnTree T,
                                                          double gate2, double max_curv, double *__restrict__ part,
                                                          unsigned long long *__restrict__ ctr) {
    __shared__ unsigned long long lds[NN_STACK * NN_QBLOCK / 2];  // the walk's stack, then the tree's rows
    uint32_t *stack = (uint32_t *)lds;                            // [depth][lane], as in k_nn_query
    double *red = (double *)lds;                                  // [component of the group][lane]
    const uint32_t t = threadIdx.x;
    const RfChunk ck = chunks[blockIdx.x];
    const uint32_t f = ck.frame;
    if (!live[f]) return;  // (uniform over the workgroup)
    const uint32_t i = off[f] + ck.chunk * RF_CHUNK + t;
    uint32_t bad = 0, j = 0;
    bool cand = false;
    double rx = 0.0, ry = 0.0, rz = 0.0, qx = 0.0, qy = 0.0, qz = 0.0, d2 = 0.0;
    if (i < off[f + 1]) {
        const RfPose P = pose[f];
        const float4 p = xform(Tl, scans[i]);
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        rx = (P.R[0] * px + P.R[1] * py) + P.R[2] * pz;
        ry = (P.R[3] * px + P.R[4] * py) + P.R[5] * pz;
        rz = (P.R[6] * px + P.R[7] * py) + P.R[8] * pz;
        qx = rx + P.t[0], qy = ry + P.t[1], qz = rz + P.t[2];
        if (!ev_finite(p) || !(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
            bad = 1;
        } else {
            d2 = nn_search_f64(qx, qy, qz, T, stack, t, &j);
            cand = d2 <= gate2;
        }
    }
    // the walk is over: what is live from here on is j, d2, q' and q
    double v[RFP_NSUM];
#pragma unroll
    for (uint32_t c = 0; c < RFP_NSUM; ++c) v[c] = 0.0;
    uint32_t pair = 0, unusable = 0;
    if (cand) {
        const double nx = (double)nrm[(size_t)j * 3 + 0], ny = (double)nrm[(size_t)j * 3 + 1], nz = (double)nrm[(size_t)j * 3 + 2];
        const double cv = __builtin_bit_cast(double, curv_bits[j]);
        if (isfinite(nx) && isfinite(ny) && isfinite(nz) && cv <= max_curv) {
            const float4 m = map[j];
            const double ex = qx - (double)m.x, ey = qy - (double)m.y, ez = qz - (double)m.z;
            const double r = (ex * nx + ey * ny) + ez * nz;
            const double J[6] = {ry * nz - rz * ny, rz * nx - rx * nz, rx * ny - ry * nx, nx, ny, nz};
            pair = 1;
            uint32_t k = 0;
#pragma unroll
            for (uint32_t a = 0; a < 6; ++a) {
#pragma unroll
                for (uint32_t b = a; b < 6; ++b) v[k++] = J[a] * J[b];
            }
#pragma unroll
            for (uint32_t a = 0; a < 6; ++a) v[21 + a] = J[a] * r;
            v[27] = r * r;
            v[28] = d2;
        } else {
            unusable = 1;
        }
    }
    ev_commit(ctr + (size_t)f * RFP_NCTR, RFP_PAIRS, pair);
    ev_commit(ctr + (size_t)f * RFP_NCTR, RFP_NON_FINITE, bad);
    ev_commit(ctr + (size_t)f * RFP_NCTR, RFP_UNUSABLE, unusable);
    rf_reduce<RFP_NSUM, RFP_GROUP>(v, red, t, part + (size_t)blockIdx.x * RFP_NSUM);
}

}  // namespace ek

#endif  // ERASOR_REFINE_PLANE_HIP_H
