// align.hip.h — every frame's pose checked against the map, all frames in one call: the reference README's first pitfall check
// ("pose_i · pcds/00000<i>.pcd must overlay correctly on dense_global_map.pcd ... most points should sit within 0.5 × voxel_size of
// the dense map"), frame by frame, on the device (erasor_hip_align_frames_*).
//
// The cloud checked is the one the reference builds in every callback for RViz, ptr_query_viz = body2origin(tf_lidar2body · scan)
// (OfflineMapUpdater.cpp:238-242, :441-449): the scan as given, T_lidar2body then the frame's T_body2origin, each with xform's
// association (kernels.hip.h).  Each frame's row is the overlap report (nearest.hip.h) of those points against the map; the map's tree
// is nn_build's, built once.
//
// k_al_query: one scan point per lane, all frames in one launch.  The frames are consecutive ranges of the concatenated scans (offsets);
// the host gives every workgroup the frame of its first point and of the first point after it, so a lane binary-searches only the
// frames its workgroup touches (usually one).  A point with a non-finite coordinate after the transforms is dropped: its distance bits
// are the all-ones sentinel, which sorts above every finite distance, so a rank below the frame's count of kept points never reaches
// it.  Counters per frame: one atomic per frame and wavefront (a wavefront usually lies in one frame; the few that straddle frames
// take one round per frame, on ballots).
//
// k_al_select: one workgroup per frame runs nearest.hip.h's exact radix select on the frame's distance bits on its own: 8 passes of
// 8-bit digits from the top, the six target ranks in the same pass, at most OV_SEL_MAX x 256 LDS counters, and wavefront 0 picks every
// target's next digit from them.  The host then applies numpy's formulas to the six values of every frame (ov_percentile_ranks /
// ov_lerp in erasor_hip.hip), with no round trip per frame.
#ifndef ERASOR_ALIGN_HIP_H
#define ERASOR_ALIGN_HIP_H

namespace ek {

// counters of one frame (AL_NCTR per frame)
enum : uint32_t {
    AL_BELOW_HALF = 0,  // d < 0.5 * voxelsize
    AL_BELOW_ONE,       // d < voxelsize
    AL_BELOW_TWO,       // d < 2 * voxelsize
    AL_MAX_BITS,        // the bit pattern of the frame's largest d
    AL_NON_FINITE,      // points dropped: a non-finite coordinate after the two transforms
    AL_NCTR
};

static constexpr unsigned long long AL_DROPPED = ~0ull;  // distance bits of a dropped point

// the six target ranks of one frame's select and its count of kept points (0: no select)
struct AlRanks {
    unsigned long long rk[OV_SEL_MAX];
    unsigned long long n;
    unsigned long long pad;
};

// the largest frame in [a, z] whose first point is <= i: the frame holding point i (empty frames start where the next does)
__device__ __forceinline__ uint32_t al_frame_of(const uint32_t *__restrict__ off, uint32_t i, uint32_t a, uint32_t z) {
    while (a < z) {
        const uint32_t m = (a + z + 1) / 2;
        if (off[m] <= i) a = m;
        else z = m - 1;
    }
    return a;
}

// (1) one scan point per lane.  off: [n_frames + 1] point offsets; wg: [grid + 1], wg[b] the frame of point b * NN_QBLOCK (wg[grid]:
// the last frame); Tb: [n_frames] poses.  dbits: [n] distance bits; ctr: [n_frames][AL_NCTR], zeroed by the host.  T.n > 0.
__global__ __launch_bounds__(NN_QBLOCK) void k_al_query(const float4 *__restrict__ scans, uint32_t n, const uint32_t *__restrict__ off,
                                                         const uint32_t *__restrict__ wg, Xf Tl, const Xf *__restrict__ Tb, NnTree T, double half,
                                                         double one, double two, unsigned long long *__restrict__ dbits,
                                                         unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t stack[NN_STACK * NN_QBLOCK];  // [depth][lane], as in k_nn_query
    const uint32_t t = threadIdx.x, i = blockIdx.x * NN_QBLOCK + t;
    const bool valid = i < n;
    uint32_t f = 0, flags = 0;  // flags: bit c set for counter c < AL_MAX_BITS, and bit AL_NON_FINITE
    unsigned long long bits = 0ull;
    if (valid) {
        f = al_frame_of(off, i, wg[blockIdx.x], wg[blockIdx.x + 1]);  // (the frames its workgroup touches)
        const float4 q = xform(Tb[f], xform(Tl, scans[i]));
        if (!ev_finite(q)) {
            flags = 1u << AL_NON_FINITE;
            dbits[i] = AL_DROPPED;
        } else {
            uint32_t best_i;
            const double d = sqrt(nn_search_f64((double)q.x, (double)q.y, (double)q.z, T, stack, t, &best_i));
            flags = (d < half ? 1u << AL_BELOW_HALF : 0u) | (d < one ? 1u << AL_BELOW_ONE : 0u) | (d < two ? 1u << AL_BELOW_TWO : 0u);
            bits = __builtin_bit_cast(unsigned long long, d);
            dbits[i] = bits;
        }
    }
    // one round per frame present in the wavefront (usually one): the frame's lanes' counts and largest bit pattern, one atomic each
    uint64_t todo = __ballot(valid);
    while (todo) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
        const uint32_t fk = __builtin_amdgcn_readlane(f, lead);
        const bool in = valid && f == fk;
        const uint64_t mine = __ballot(in);
        unsigned long long *c = ctr + (size_t)fk * AL_NCTR;
        const uint32_t whi = wave_minmax_u<true>(in ? (uint32_t)(bits >> 32) : 0u);
        const uint32_t wlo = wave_minmax_u<true>(in && (uint32_t)(bits >> 32) == whi ? (uint32_t)bits : 0u);
        const unsigned long long wmax = ((unsigned long long)whi << 32) | wlo;
        const bool leader = (t & 63u) == lead;
#pragma unroll
        for (uint32_t k = 0; k < AL_NCTR; ++k) {
            if (k == AL_MAX_BITS) continue;
            const uint32_t cnt = (uint32_t)__popcll(mine & __ballot(in && ((flags >> k) & 1u)));
            if (leader && cnt) atomicAdd(&c[k], (unsigned long long)cnt);
        }
        if (leader && wmax) atomicMax(&c[AL_MAX_BITS], wmax);
        todo &= ~mine;
    }
}

// (2) one workgroup of 256 lanes per frame: the values at the frame's six target ranks (val: [n_frames][OV_SEL_MAX], written only for
// frames with kept points)
__global__ __launch_bounds__(256) void k_al_select(const unsigned long long *__restrict__ dbits, const uint32_t *__restrict__ off,
                                                    const AlRanks *__restrict__ ranks, unsigned long long *__restrict__ val) {
    __shared__ uint32_t c[OV_SEL_MAX * 256];                                          // [distinct prefix][digit]
    __shared__ unsigned long long pref[OV_SEL_MAX], left[OV_SEL_MAX], upref[OV_SEL_MAX];  // per target; the distinct prefixes
    __shared__ uint32_t slot[OV_SEL_MAX], nu;                                         // per target: its prefix's row of c
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    if (ranks[f].n == 0) return;  // (uniform over the workgroup)
    const uint32_t b = off[f], e = off[f + 1];
    if (t < OV_SEL_MAX) {
        pref[t] = 0ull;
        left[t] = ranks[f].rk[t];
    }
    __syncthreads();
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (t == 0) {
            uint32_t m = 0;
            for (uint32_t k = 0; k < OV_SEL_MAX; ++k) {
                uint32_t j = 0;
                while (j < m && upref[j] != pref[k]) ++j;
                if (j == m) upref[m++] = pref[k];
                slot[k] = j;
            }
            nu = m;
        }
        for (uint32_t j = t; j < OV_SEL_MAX * 256; j += 256) c[j] = 0u;
        __syncthreads();
        const uint32_t m = nu;
        unsigned long long up[OV_SEL_MAX];
#pragma unroll
        for (uint32_t k = 0; k < OV_SEL_MAX; ++k) up[k] = upref[k];
        for (uint32_t i = b + t; i < e; i += 256) {
            const unsigned long long x = dbits[i];
            const unsigned long long top = shift >= 56 ? 0ull : x >> (shift + 8);
            const uint32_t d = (uint32_t)(x >> shift) & 0xFFu;
            bool done = false;
#pragma unroll
            for (uint32_t k = 0; k < OV_SEL_MAX; ++k) {  // (unrolled: the prefixes stay in registers, no scratch)
                if (!done && k < m && top == up[k]) {
                    atomicAdd(&c[k * 256 + d], 1u);
                    done = true;
                }
            }
        }
        __syncthreads();
        if (t < 64) {  // wavefront 0: every target's digit, from a scan of its row (four digits per lane)
            for (uint32_t k = 0; k < OV_SEL_MAX; ++k) {
                const uint32_t *row = c + slot[k] * 256;
                const uint32_t s = row[4 * t] + row[4 * t + 1] + row[4 * t + 2] + row[4 * t + 3];
                const uint32_t incl = esort::wave_incl_scan(s), excl = incl - s;
                const unsigned long long L = left[k];  // (< the prefix's count <= 2^30)
                const uint64_t hit = __ballot(excl <= L && L < incl);
                const uint32_t lane = hit ? (uint32_t)__builtin_ctzll(hit) : 63u;
                if (t == lane) {
                    unsigned long long cum = excl;
                    uint32_t d = 4 * t;
                    while (d < 4 * t + 3 && L >= cum + row[d]) cum += row[d++];
                    left[k] = L - cum;
                    pref[k] = (pref[k] << 8) | d;
                }
            }
        }
        __syncthreads();
    }
    if (t < OV_SEL_MAX) val[(size_t)f * OV_SEL_MAX + t] = pref[t];
}

}  // namespace ek

#endif  // ERASOR_ALIGN_HIP_H
