// refine.hip.h — every frame's pose refined against the map, all frames side by side: point-to-point ICP with a fixed correspondence
// gate (erasor_hip_refine_poses_*).  What the reference leaves to the user: its README's first pitfall is a pose that does not put
// pose_i · pcds/00000<i>.pcd onto dense_global_map.pcd, and align.hip.h only reports it.
//
// The cloud matched is the one align.hip.h checks, body2origin(tf_lidar2body · scan) (OfflineMapUpdater.cpp:238-242, :441-449), with
// the frame's pose as the unknown: p = xform(T_lidar2body, scan row) in float32 once, then q' = R·p and q = q' + t in float64 with the
// frame's current (R, t), each row as ((a*x + b*y) + c*z).  nn_search_f64 (nearest.hip.h) gives q's nearest map point j and d^2, ties
// to the lowest index; the pair counts when d^2 <= gate2 (max_dist * max_dist, formed once by the host), with m' = map[j] - t.
//
// k_rf_query gathers, per chunk of RF_CHUNK points of ONE frame, the sums Horn's closed form needs -- Σq' (3), Σm' (3), Σq'm'ᵀ (9) and
// Σd^2: RF_NSUM doubles -- and the count of pairs.  The order of every addition is fixed, so the sums have one answer: the frame's points
// in scan order, cut into chunks of 256 from the frame's own first point (a workgroup lies in one frame; chunk: the table the host
// writes, al_put_frames' per-workgroup table in its place); lanes without a pair hold +0.0; inside a chunk the halving tree
// v[i] += v[i + s], s = 128, 64 through LDS and s = 32 .. 1 by shuffles inside wavefront 0.  k_rf_partials then adds a frame's chunk
// partials one after another in chunk order from 0.0, one lane per (frame, component).  No float atomics; the counts are integer
// atomics, one per wavefront.  The chunk's tree is rf_reduce and the second launch takes its component count as a template parameter:
// refine_plane.hip.h adds its 29 sums by the same rule.
//
// LDS: the walk's [NN_STACK][NN_QBLOCK] stack (26 KB) is dead once every lane has its neighbour, and the tree over the wavefronts
// reuses it, RF_GROUP components at a time ([RF_GROUP][256] doubles = 16 KB).  A frame that has ended is frozen: its workgroups return
// on live[f] == 0 (uniform over the workgroup) and its sums are not read.
#ifndef ERASOR_REFINE_HIP_H
#define ERASOR_REFINE_HIP_H

namespace ek {

static constexpr uint32_t RF_CHUNK = 256;  // points per chunk: part of the sums' definition, not a launch parameter
static constexpr uint32_t RF_NSUM = 16;    // Σq' (0..2), Σm' (3..5), Σq'm'ᵀ row-major (6..14), Σd^2 (15)
static constexpr uint32_t RF_GROUP = 8;    // components that cross the wavefronts together
static_assert(NN_QBLOCK == RF_CHUNK, "a query workgroup covers one chunk");
static_assert(RF_GROUP * RF_CHUNK * sizeof(double) <= NN_STACK * NN_QBLOCK * sizeof(uint32_t), "the tree fits the walk's stack");

// counters of one frame (RF_NCTR per frame)
enum : uint32_t {
    RF_PAIRS = 0,   // pairs within the gate
    RF_NON_FINITE,  // points without a query: a non-finite coordinate after T_lidar2body, or after the frame's pose
    RF_NCTR
};

// a frame's pose in float64: R row-major, then t
struct RfPose {
    double R[9], t[3];
};

// the workgroup's chunk: its frame and the chunk's number inside the frame
struct RfChunk {
    uint32_t frame, chunk;
};

// The chunk's defined sum of every lane's NSUM values v, stored by lane 0 to out[0 .. NSUM): the halving tree v[i] += v[i + s].  Every lane
// of the workgroup (RF_CHUNK lanes) calls it with the walk over; red: the workgroup's LDS, [GROUP][RF_CHUNK] doubles.  GROUP components
// cross the wavefronts together (the last group may be short); which ones travel together does not change a sum.
template <uint32_t NSUM, uint32_t GROUP>
__device__ __forceinline__ void rf_reduce(double (&v)[NSUM], double *red, uint32_t t, double *__restrict__ out) {
    static_assert(GROUP * RF_CHUNK * sizeof(double) <= NN_STACK * NN_QBLOCK * sizeof(uint32_t), "the tree fits the walk's stack");
    // s = 128, 64: lanes [s, 2s) hand their values to lanes [0, s), a group of components at a time
    __syncthreads();  // (every lane's walk is over: the stack is free)
#pragma unroll
    for (uint32_t g = 0; g < NSUM; g += GROUP) {
        if (t >= 128) {
#pragma unroll
            for (uint32_t c = 0; c < GROUP; ++c)
                if (g + c < NSUM) red[c * RF_CHUNK + t] = v[g + c];
        }
        __syncthreads();
        if (t < 128) {
#pragma unroll
            for (uint32_t c = 0; c < GROUP; ++c)
                if (g + c < NSUM) v[g + c] += red[c * RF_CHUNK + t + 128];
            if (t >= 64) {
#pragma unroll
                for (uint32_t c = 0; c < GROUP; ++c)
                    if (g + c < NSUM) red[c * RF_CHUNK + t] = v[g + c];
            }
        }
        __syncthreads();
        if (t < 64) {
#pragma unroll
            for (uint32_t c = 0; c < GROUP; ++c)
                if (g + c < NSUM) v[g + c] += red[c * RF_CHUNK + t + 64];
        }
        // (the next group writes rows [128, 256) first, which nobody reads after the barrier above, and rows [64, 128) only after
        // its own first barrier, behind wavefront 0's reads here)
    }
    if (t >= 64) return;
    // s = 32 .. 1 inside wavefront 0: lane i < s takes lane i + s (the other lanes' values are not used again)
#pragma unroll
    for (uint32_t s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (uint32_t c = 0; c < NSUM; ++c) v[c] += __shfl_down(v[c], s);
    }
    if (t == 0) {
#pragma unroll
        for (uint32_t c = 0; c < NSUM; ++c) out[c] = v[c];
    }
}

// (1) one scan point per lane, one chunk per workgroup.  off: [n_frames + 1]; chunks: [grid]; pose, live: [n_frames]; map: the points
// the tree was built over, in their own order.  part: [grid][RF_NSUM]; ctr: [n_frames][RF_NCTR], zeroed by the host.  T.n > 0.
__global__ __launch_bounds__(NN_QBLOCK) void k_rf_query(const float4 *__restrict__ scans, const uint32_t *__restrict__ off,
                                                         const RfChunk *__restrict__ chunks, Xf Tl, const RfPose *__restrict__ pose,
                                                         const uint32_t *__restrict__ live, const float4 *__restrict__ map, NnTree T, double gate2,
                                                         double *__restrict__ part, unsigned long long *__restrict__ ctr) {
    __shared__ unsigned long long lds[NN_STACK * NN_QBLOCK / 2];  // the walk's stack, then the tree's rows
    uint32_t *stack = (uint32_t *)lds;                            // [depth][lane], as in k_nn_query
    double *red = (double *)lds;                                  // [component of the group][lane]
    const uint32_t t = threadIdx.x;
    const RfChunk ck = chunks[blockIdx.x];
    const uint32_t f = ck.frame;
    if (!live[f]) return;  // (uniform over the workgroup)
    const uint32_t i = off[f] + ck.chunk * RF_CHUNK + t;
    double v[RF_NSUM];
#pragma unroll
    for (uint32_t c = 0; c < RF_NSUM; ++c) v[c] = 0.0;
    uint32_t pair = 0, bad = 0;
    if (i < off[f + 1]) {
        const RfPose P = pose[f];
        const float4 p = xform(Tl, scans[i]);
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        const double rx = (P.R[0] * px + P.R[1] * py) + P.R[2] * pz;
        const double ry = (P.R[3] * px + P.R[4] * py) + P.R[5] * pz;
        const double rz = (P.R[6] * px + P.R[7] * py) + P.R[8] * pz;
        const double qx = rx + P.t[0], qy = ry + P.t[1], qz = rz + P.t[2];
        if (!ev_finite(p) || !(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
            bad = 1;
        } else {
            uint32_t j;
            const double d2 = nn_search_f64(qx, qy, qz, T, stack, t, &j);
            if (d2 <= gate2) {
                const float4 m = map[j];
                const double mx = (double)m.x - P.t[0], my = (double)m.y - P.t[1], mz = (double)m.z - P.t[2];
                pair = 1;
                v[0] = rx, v[1] = ry, v[2] = rz;
                v[3] = mx, v[4] = my, v[5] = mz;
                v[6] = rx * mx, v[7] = rx * my, v[8] = rx * mz;
                v[9] = ry * mx, v[10] = ry * my, v[11] = ry * mz;
                v[12] = rz * mx, v[13] = rz * my, v[14] = rz * mz;
                v[15] = d2;
            }
        }
    }
    ev_commit(ctr + (size_t)f * RF_NCTR, RF_PAIRS, pair);
    ev_commit(ctr + (size_t)f * RF_NCTR, RF_NON_FINITE, bad);
    rf_reduce<RF_NSUM, RF_GROUP>(v, red, t, part + (size_t)blockIdx.x * RF_NSUM);
}

// (2) one lane per (frame, component): the frame's chunk partials, one after another in chunk order, from 0.0.  cb: [n_frames + 1],
// cb[f] the frame's first chunk; part: [chunks][NSUM]; sums: [n_frames][NSUM], written for live frames only.
template <uint32_t NSUM>
__global__ __launch_bounds__(256) void k_rf_partials(const double *__restrict__ part, const uint32_t *__restrict__ cb,
                                                      const uint32_t *__restrict__ live, uint32_t n_frames, double *__restrict__ sums) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_frames * NSUM) return;
    const uint32_t f = k / NSUM, c = k % NSUM;
    if (!live[f]) return;
    double s = 0.0;
    for (uint32_t b = cb[f]; b < cb[f + 1]; ++b) s += part[(size_t)b * NSUM + c];
    sums[k] = s;
}

}  // namespace ek

#endif  // ERASOR_REFINE_HIP_H
