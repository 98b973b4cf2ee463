// ground.hip.h — every scan's ground, patch by patch, and the map's ground points by vote (erasor_hip_ground_scans /
// erasor_hip_ground_votes_*).  The project fits the ground only where the reference does: per bin, inside a step, for the bins the Scan
// Ratio Test reverts (revert_bins.hip.h).  This is R-GPF (erasor.cpp:183-294: extract_initial_seeds_, estimate_plane_, the loop of
// extract_ground) run on every polar patch of every scan, as the reference's author runs it in the follow-up (Patchwork), with the
// uprightness gate the reference carries commented out (erasor.cpp:286) and an elevation / flatness gate per ring.
//
// The contract (the normative text is erasor_amd/evalmap.py: ground_scans / ground_votes and their *_brute twins; the device equals it
// byte for byte).  Float64 on the float32 coordinates, every operation a separate IEEE operation in the order written:
//   * the patch of (x, y, z): the sector is visibility.hip.h's column over col_tan; r = sqrt(x x + y y), ring = (the number of ring_edge
//     entries <= r) - 1.  The gates, in this order: a non-finite coordinate (code 255); on the axis or a ring outside 0 .. R - 1 (out of
//     range, code 2).  A patch is (frame, ring, sector); its points are kept in scan order, j = 0 .. m - 1;
//   * m < min_points: SPARSE, the points' code 2;
//   * seeds: the candidates z >= min_z ascending by (z, j), -0.0 equal to +0.0; lpr = (((0.0 + z_0) + z_1) + ...) / k over the first
//     k = min(num_lpr, candidates); none: DEGENERATE; the seeds are z >= min_z and z < lpr + th_seeds;
//   * iters times: the member count n and the nine raw moments x y z xx xy xz yy yz zz over ALL the patch's points in patch order by
//     refine.hip.h's rule -- chunks of 256 from the patch's first point, a non-member holds +0.0, the halving tree v[i] += v[i + s] for
//     s = 128 .. 1, the chunks' partials one after another from 0.0; n < 3: DEGENERATE; mean = S / n, cov_ab = S_ab / n - mean_a mean_b,
//     tr = (cxx + cyy) + czz; !(tr > 0): DEGENERATE; normals.hip.h's Jacobi solve, the eigenvalues ascending by (value, column), the
//     normal the first one's column, negated iff nz < 0; d = -((nx mx + ny my) + nz mz); the new members:
//     ((nx x + ny y) + nz z) + d < th_dist;
//   * then nz < uprightness: REJECTED_UPRIGHT; else mean_z > elevation[ring] and !(l0 / tr <= flatness[ring]): REJECTED_ELEVATION;
//   * codes: 1 a member of an OK patch, 0 judged and not one (or any point of a REJECTED patch), 2 not judged, 255 non-finite.
//
// k_gr_key: one point per lane over all frames of a batch: the gates, the ring (a square root and a binary search of ring_edge in LDS),
// the sector, the patch key ((frame * R + ring) * S + sector; the batch's patch count for a point without a patch), one integer atomic
// into the patch's count per run of equal keys inside the wavefront; the per-frame drop counters are aggregated per wavefront (a
// ballot per frame the wavefront touches) before any atomic.  The keys then go through the project's stable radix sort, whose permutation lists every patch's points in scan order, and
// the counts through scan_u32, which gives every patch's first place in it: an empty patch costs its table row and nothing else.
// k_gr_fit: three launches, one per size class, each walking the patch table with a grid stride and taking the patches of its class:
//   * m <= GR_WAVE_POINTS: one wavefront (a workgroup of 64 lanes), a point per lane, no barrier and no LDS traffic between lanes;
//   * m <= GR_SMALL_POINTS / m <= GR_LDS_POINTS: a workgroup of 256 with the coordinates in 12 KiB / 48 KiB of LDS (with the tree's
//     9 KiB: 7 / 2 workgroups per CU of 160 KiB);
//   * m > GR_LDS_POINTS: the large class's workgroup reads every point from memory through the permutation in every pass instead -- the
//     same operations in the same order, so the same bytes.
// Lane t owns the points j = t, t + BS, ...: it alone writes and reads their LDS slots, so the cache needs no barrier.  The num_lpr
// lowest come out exactly, one per round: the minimum of the 64-bit order keys (z's order-preserving bit pattern, then j) above the last
// one taken.  Every lane then carries the same sums and solves the same 3x3 in registers (nm_rotate), so the control flow stays uniform.
// No float atomics; the counters are integer atomics, one per patch and counter.
// The map form puts k_gr_gather_flag / k_gr_gather_put in front (every map point into every frame of the batch, rounded to float32,
// the ring gate, the project's stable compaction over all frames of the batch at once, the map index kept) and k_gr_vote behind (one
// 32-bit integer atomic per judged point into the map point's pair of uint16), then k_gr_decide.
#ifndef ERASOR_GROUND_HIP_H
#define ERASOR_GROUND_HIP_H

namespace ek {

static constexpr uint32_t GR_WAVE_POINTS = ERASOR_GROUND_WAVE_POINTS;    // size class 0: one wavefront
static constexpr uint32_t GR_SMALL_POINTS = ERASOR_GROUND_SMALL_POINTS;  // size class 1: a workgroup, 12 KiB of coordinates
static constexpr uint32_t GR_LDS_POINTS = ERASOR_GROUND_LDS_POINTS;      // size class 2: a workgroup, 48 KiB; beyond: from memory
static constexpr uint32_t GR_CHUNK = 256;                                // points per chunk of the sums: part of their definition
static constexpr uint32_t GR_NSUM = 9;                                   // x y z xx xy xz yy yz zz
static constexpr uint32_t GR_MAX_RINGS = ERASOR_GROUND_MAX_RINGS, GR_MAX_SECTORS = ERASOR_GROUND_MAX_SECTORS;
static constexpr uint32_t GR_TAB = (GR_MAX_RINGS + 1) + (GR_MAX_SECTORS / 8 - 1);  // what k_gr_key keeps in LDS: ring_edge, col_tan
static constexpr uint32_t GR_MAX_PATCHES = 1u << 20;                     // patches of one batch (the host cuts the frames)
static_assert(RF_CHUNK == GR_CHUNK, "the sums follow refine.hip.h's rule");

// counters of one frame (GR_NCTR per frame, zeroed by the host)
enum : uint32_t {
    GR_C_NON_FINITE = 0, GR_C_RANGE, GR_C_POINTS /* the map form: points gathered */, GR_C_JUDGED, GR_C_GROUND, GR_C_GROUND_DYNAMIC,
    GR_C_PATCHES, GR_C_STATUS /* + the status: SPARSE .. REJECTED_ELEVATION */, GR_NCTR = GR_C_STATUS + 6
};
// counters of the map form's decision
enum : uint32_t { GD_C_GROUND_DYNAMIC = 0, GD_C_GROUND_STATIC, GD_C_UNSEEN, GD_NCTR };

struct GrParams {
    uint32_t R, S, M, num_lpr, iters, min_points;
    double th_seeds, th_dist, min_z, uprightness;
};

// z's bit pattern in an order that unsigned comparison keeps (-0.0 as +0.0), and back
__device__ __forceinline__ uint32_t gr_zkey(float z) {
    const uint32_t b = __float_as_uint(z == 0.0f ? 0.0f : z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float gr_zval(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// the patch of a finite point: false when it has none (on the axis, ring out of range).  tab: ring_edge [R + 1], then col_tan [M - 1]
__device__ __forceinline__ bool gr_patch_of(double x, double y, const GrParams &P, const double *tab, uint32_t *ring, uint32_t *sector) {
    const double a = fabs(x), b = fabs(y);
    if (a == 0.0 && b == 0.0) return false;
    const double r = sqrt(x * x + y * y);
    const uint32_t r1 = vis_count_le(tab, P.R + 1, r);  // the ring + 1
    if (r1 == 0 || r1 > P.R) return false;
    const bool swap = a < b;
    const double t = swap ? a / b : b / a;
    const uint32_t j = vis_count_le(tab + (P.R + 1), P.M - 1, t);
    const uint32_t q = x < 0 ? (y < 0 ? 2u : 1u) : (y < 0 ? 3u : 0u);
    const bool odd = (q & 1u) ? !swap : swap;
    const uint32_t o = 2 * q + (odd ? 1u : 0u);
    *ring = r1 - 1;
    *sector = odd ? o * P.M + (P.M - 1) - j : o * P.M + j;
    return true;
}

// (1) one point per lane: the points lo + k, k < n (n = *n_dev when given), of the frames whose offsets are off[0 .. nb] (absolute point
// indices).  key: [n] by k; cnt: [nb R S + 1], zeroed; codes: by absolute index; ctr: the batch's first frame's counters.
__global__ __launch_bounds__(256) void k_gr_key(const float4 *__restrict__ pts, uint32_t lo, uint32_t n_host, const uint32_t *__restrict__ n_dev,
                                                 const uint32_t *__restrict__ off, uint32_t nb, GrParams P, const double *__restrict__ tabs,
                                                 uint32_t *__restrict__ key, uint32_t *__restrict__ cnt, uint8_t *__restrict__ codes,
                                                 unsigned long long *__restrict__ ctr) {
    __shared__ double tab[GR_TAB];
    const uint32_t t = threadIdx.x, k = blockIdx.x * 256u + t;
    const uint32_t n = n_dev ? *n_dev : n_host;
    if (blockIdx.x * 256u >= n) return;  // (the map form sizes the grid by the bound of n: most of its workgroups have no point)
    for (uint32_t j = t; j < (P.R + 1) + (P.M - 1); j += 256u) tab[j] = tabs[j];
    __syncthreads();
    uint32_t f = 0, c = 2;  // the drop counter this point adds to, 2: none
    const uint32_t none = nb * P.R * P.S;  // the key of a point without a patch
    uint32_t kv = none;
    if (k < n) {
        const uint32_t i = lo + k;
        f = al_frame_of(off, i, 0u, nb - 1);
        const float4 p = pts[i];
        if (!ev_finite(p)) {
            codes[i] = (uint8_t)ERASOR_GROUND_CODE_NON_FINITE;
            c = GR_C_NON_FINITE;
        } else {
            uint32_t ring = 0, sector = 0;
            if (gr_patch_of((double)p.x, (double)p.y, P, tab, &ring, &sector)) {
                kv = (f * P.R + ring) * P.S + sector;
            } else {
                codes[i] = (uint8_t)ERASOR_GROUND_CODE_NOT_JUDGED;
                c = GR_C_RANGE;
            }
        }
        key[k] = kv;
    }
    // the patches' counts: neighbours in a scan, and in a map, mostly share a patch, so the first lane of every run of equal keys inside
    // the wavefront adds the run's length (integer adds: the counts do not depend on how the runs fall)
    {
        const uint32_t ln = t & 63u, prev = __shfl_up(kv, 1u);
        const bool edge = ln == 0 || prev != kv;
        const uint64_t edges = __ballot(edge);
        if (edge && kv != none) {
            const uint64_t above = ln == 63u ? 0ull : (edges >> (ln + 1)) << (ln + 1);
            const uint32_t end = above ? (uint32_t)__ffsll((long long)above) - 1u : 64u;
            atomicAdd(&cnt[kv], end - ln);
        }
    }
    // the drops, per frame the wavefront touches: one ballot per counter, one atomic per frame and counter
    uint64_t pend = __ballot(c < 2);
    const uint32_t lane = t & 63u;
    while (pend) {  // (uniform over the wavefront)
        const int src = __ffsll((long long)pend) - 1;
        const uint32_t fc = __shfl(f, src);
        const bool mine = c < 2 && f == fc;
        const uint64_t m0 = __ballot(mine && c == GR_C_NON_FINITE), m1 = __ballot(mine && c == GR_C_RANGE);
        if (lane == (uint32_t)src) {
            if (m0) atomicAdd(&ctr[(size_t)fc * GR_NCTR + GR_C_NON_FINITE], (unsigned long long)__popcll(m0));
            if (m1) atomicAdd(&ctr[(size_t)fc * GR_NCTR + GR_C_RANGE], (unsigned long long)__popcll(m1));
        }
        pend &= ~(m0 | m1);
    }
}

// the smallest v of the workgroup, in every lane.  wm: BS / 64 words of LDS
template <uint32_t BS>
__device__ __forceinline__ unsigned long long gr_block_min(unsigned long long v, unsigned long long *wm, uint32_t t) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t ol = __shfl_xor((uint32_t)v, s), oh = __shfl_xor((uint32_t)(v >> 32), s);
        const unsigned long long o = ((unsigned long long)oh << 32) | ol;
        v = o < v ? o : v;
    }
    if constexpr (BS > 64) {
        if ((t & 63u) == 0) wm[t >> 6] = v;
        __syncthreads();
        v = wm[0];
#pragma unroll
        for (uint32_t w = 1; w < BS / 64; ++w) v = wm[w] < v ? wm[w] : v;
        __syncthreads();
    }
    return v;
}

// the workgroup's sum of x, in every lane.  ws: BS / 64 words of LDS
template <uint32_t BS>
__device__ __forceinline__ uint32_t gr_block_sum(uint32_t x, uint32_t *ws, uint32_t t) {
    uint32_t s = wave_sum(x);
    if constexpr (BS > 64) {
        if ((t & 63u) == 0) ws[t >> 6] = s;
        __syncthreads();
        s = 0;
#pragma unroll
        for (uint32_t w = 0; w < BS / 64; ++w) s += ws[w];
        __syncthreads();
    }
    return s;
}

// One chunk's defined sums added to tot, in every lane: lane t holds the chunk's rows t, t + BS, ... in v.  A wavefront: rows 128 apart
// and 64 apart meet in the lane's own registers, the rest by shuffles.  A workgroup of 256: s = 128, 64 through red ([GR_NSUM][128]),
// s = 32 .. 1 by shuffles in wavefront 0, lane 0's sums through bc.
template <uint32_t BS>
__device__ __forceinline__ void gr_chunk_sum(double (&v)[GR_CHUNK / BS][GR_NSUM], double *red, double *bc, uint32_t t, double (&tot)[GR_NSUM]) {
    if constexpr (BS == 64) {
#pragma unroll
        for (uint32_t c = 0; c < GR_NSUM; ++c) {
            v[0][c] += v[2][c];  // s = 128: rows [0, 64) take [128, 192), rows [64, 128) take [192, 256)
            v[1][c] += v[3][c];
            v[0][c] += v[1][c];  // s = 64
        }
#pragma unroll
        for (uint32_t s = 32; s >= 1; s >>= 1) {
#pragma unroll
            for (uint32_t c = 0; c < GR_NSUM; ++c) v[0][c] += __shfl_down(v[0][c], s);
        }
#pragma unroll
        for (uint32_t c = 0; c < GR_NSUM; ++c) tot[c] = tot[c] + __shfl(v[0][c], 0);
    } else {
        static_assert(BS == 64 || BS == GR_CHUNK, "a wavefront or a workgroup of one chunk");
        if (t >= 128) {
#pragma unroll
            for (uint32_t c = 0; c < GR_NSUM; ++c) red[c * 128 + (t - 128)] = v[0][c];
        }
        __syncthreads();
        if (t < 128) {
#pragma unroll
            for (uint32_t c = 0; c < GR_NSUM; ++c) v[0][c] += red[c * 128 + t];
        }
        __syncthreads();
        if (t >= 64 && t < 128) {
#pragma unroll
            for (uint32_t c = 0; c < GR_NSUM; ++c) red[c * 128 + (t - 64)] = v[0][c];
        }
        __syncthreads();
        if (t < 64) {
#pragma unroll
            for (uint32_t c = 0; c < GR_NSUM; ++c) v[0][c] += red[c * 128 + t];
#pragma unroll
            for (uint32_t s = 32; s >= 1; s >>= 1) {
#pragma unroll
                for (uint32_t c = 0; c < GR_NSUM; ++c) v[0][c] += __shfl_down(v[0][c], s);
            }
            if (t == 0) {
#pragma unroll
                for (uint32_t c = 0; c < GR_NSUM; ++c) bc[c] = v[0][c];
            }
        }
        __syncthreads();  // (bc is read here and written again only behind the next chunk's three barriers; red likewise)
#pragma unroll
        for (uint32_t c = 0; c < GR_NSUM; ++c) tot[c] = tot[c] + bc[c];
    }
}

// (2) the fit: workgroup b takes the patches b, b + gridDim.x, ... of its size class CLS (0: m <= GR_WAVE_POINTS, BS = 64; 1: m <=
// GR_SMALL_POINTS; 2: the rest; CAP: the points its LDS holds).  perm: the sorted permutation (k of the batch's points, patch by
// patch in scan order); cnt, pl, tops: the patches' counts and their scan; patches: the batch's table rows, zeroed, or NULL; tabs: ring_edge,
// col_tan, elevation [R], flatness [R]; ctr: the batch's first frame's counters.
template <uint32_t BS, uint32_t CAP, uint32_t CLS>
__global__ __launch_bounds__(BS) void k_gr_fit(const float4 *__restrict__ pts, uint32_t lo, const uint32_t *__restrict__ perm,
                                                const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ pl, const uint32_t *__restrict__ tops,
                                                uint32_t n_patches, GrParams P, const double *__restrict__ tabs, uint8_t *__restrict__ codes,
                                                erasor_ground_patch *__restrict__ patches, unsigned long long *__restrict__ ctr) {
    constexpr uint32_t NV = GR_CHUNK / BS;
    __shared__ float lx[CAP], ly[CAP], lz[CAP];
    __shared__ double red[BS == 64 ? 1 : GR_NSUM * 128];
    __shared__ double bc[GR_NSUM];
    __shared__ unsigned long long wm[4];
    __shared__ uint32_t ws[4];
    const uint32_t t = threadIdx.x;
    const double *elev = tabs + (P.R + 1) + (P.M - 1), *flat = elev + P.R;
    for (uint32_t p = blockIdx.x; p < n_patches; p += gridDim.x) {
        const uint32_t m = cnt[p];
        const uint32_t cls = m <= GR_WAVE_POINTS ? 0u : (m <= GR_SMALL_POINTS ? 1u : 2u);
        if (m == 0 || cls != CLS) continue;  // (uniform over the workgroup, as everything below)
        const uint32_t s0 = pl[p] + tops[p >> 10];
        const uint32_t fl = p / (P.R * P.S), ring = (p / P.S) % P.R;
        unsigned long long *cf = ctr + (size_t)fl * GR_NCTR;
        const uint32_t *pj = perm + s0;
        if (m < P.min_points) {
            for (uint32_t j = t; j < m; j += BS) codes[lo + pj[j]] = (uint8_t)ERASOR_GROUND_CODE_NOT_JUDGED;
            if (t == 0) {
                if (patches) {
                    patches[p].status = ERASOR_GROUND_SPARSE;
                    patches[p].n_points = m;
                }
                atomicAdd(&cf[GR_C_PATCHES], 1ull);
                atomicAdd(&cf[GR_C_STATUS + (uint32_t)ERASOR_GROUND_SPARSE], 1ull);
            }
            continue;
        }
        const bool in_lds = m <= CAP;
        if (in_lds)
            for (uint32_t j = t; j < m; j += BS) {  // (lane t alone writes and reads the slots j = t, t + BS, ...)
                const float4 q = pts[lo + pj[j]];
                lx[j] = q.x, ly[j] = q.y, lz[j] = q.z;
            }
        // the lowest-point height: the num_lpr smallest order keys, one per round
        unsigned long long last = 0ull;
        bool first = true;
        double zsum = 0.0;
        uint32_t nc = 0;
        for (uint32_t r = 0; r < P.num_lpr; ++r) {
            unsigned long long best = ~0ull;
            for (uint32_t j = t; j < m; j += BS) {
                const float z = in_lds ? lz[j] : pts[lo + pj[j]].z;
                if ((double)z >= P.min_z) {
                    const unsigned long long kk = ((unsigned long long)gr_zkey(z) << 32) | j;
                    if ((first || kk > last) && kk < best) best = kk;
                }
            }
            best = gr_block_min<BS>(best, wm, t);
            if (best == ~0ull) break;
            zsum = zsum + (double)gr_zval((uint32_t)(best >> 32));
            ++nc;
            last = best;
            first = false;
        }
        uint32_t status = ERASOR_GROUND_OK;
        double nx = 0.0, ny = 0.0, nz = 0.0, d = 0.0, mz = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0, tr = 0.0;
        if (nc == 0) status = ERASOR_GROUND_DEGENERATE;
        const double thr = nc ? zsum / (double)nc + P.th_seeds : 0.0;
        for (uint32_t it = 0; it < P.iters && status == ERASOR_GROUND_OK; ++it) {
            double tot[GR_NSUM];
#pragma unroll
            for (uint32_t c = 0; c < GR_NSUM; ++c) tot[c] = 0.0;
            uint32_t mine = 0;
            for (uint32_t c0 = 0; c0 < m; c0 += GR_CHUNK) {
                double v[NV][GR_NSUM];
#pragma unroll
                for (uint32_t e = 0; e < NV; ++e) {
                    const uint32_t j = c0 + e * BS + t;
                    bool mem = false;
                    double x = 0.0, y = 0.0, z = 0.0;
                    if (j < m) {
                        if (in_lds) {
                            x = (double)lx[j], y = (double)ly[j], z = (double)lz[j];
                        } else {
                            const float4 q = pts[lo + pj[j]];
                            x = (double)q.x, y = (double)q.y, z = (double)q.z;
                        }
                        mem = it == 0 ? (z >= P.min_z && z < thr) : (((nx * x + ny * y) + nz * z) + d < P.th_dist);
                    }
                    mine += mem ? 1u : 0u;
                    v[e][0] = mem ? x : 0.0, v[e][1] = mem ? y : 0.0, v[e][2] = mem ? z : 0.0;
                    v[e][3] = mem ? x * x : 0.0, v[e][4] = mem ? x * y : 0.0, v[e][5] = mem ? x * z : 0.0;
                    v[e][6] = mem ? y * y : 0.0, v[e][7] = mem ? y * z : 0.0, v[e][8] = mem ? z * z : 0.0;
                }
                gr_chunk_sum<BS>(v, red, bc, t, tot);
            }
            const uint32_t nm = gr_block_sum<BS>(mine, ws, t);
            if (nm < 3) {
                status = ERASOR_GROUND_DEGENERATE;
                break;
            }
            const double nn = (double)nm;
            const double mx = tot[0] / nn, my = tot[1] / nn;
            mz = tot[2] / nn;
            double a00 = tot[3] / nn - mx * mx, a01 = tot[4] / nn - mx * my, a02 = tot[5] / nn - mx * mz;
            double a11 = tot[6] / nn - my * my, a12 = tot[7] / nn - my * mz, a22 = tot[8] / nn - mz * mz;
            tr = (a00 + a11) + a22;
            if (!(tr > 0)) {
                status = ERASOR_GROUND_DEGENERATE;
                break;
            }
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
            for (uint32_t sweep = 0; sweep < NM_SWEEPS; ++sweep) {
                if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
                nm_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
                nm_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
                nm_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
            }
            const uint32_t r0 = (a11 < a00 ? 1u : 0u) + (a22 < a00 ? 1u : 0u);
            const uint32_t r1 = (a00 <= a11 ? 1u : 0u) + (a22 < a11 ? 1u : 0u);
            l0 = r0 == 0 ? a00 : (r1 == 0 ? a11 : a22);
            l1 = r0 == 1 ? a00 : (r1 == 1 ? a11 : a22);
            l2 = r0 == 2 ? a00 : (r1 == 2 ? a11 : a22);
            nx = r0 == 0 ? v00 : (r1 == 0 ? v01 : v02);
            ny = r0 == 0 ? v10 : (r1 == 0 ? v11 : v12);
            nz = r0 == 0 ? v20 : (r1 == 0 ? v21 : v22);
            if (nz < 0) nx = -nx, ny = -ny, nz = -nz;
            d = -((nx * mx + ny * my) + nz * mz);
        }
        if (status == ERASOR_GROUND_OK) {
            if (nz < P.uprightness) status = ERASOR_GROUND_REJECTED_UPRIGHT;
            else if (mz > elev[ring] && !(l0 / tr <= flat[ring])) status = ERASOR_GROUND_REJECTED_ELEVATION;
        }
        // the codes, and the patch's ground points
        uint32_t g = 0, gd = 0;
        for (uint32_t j = t; j < m; j += BS) {
            const uint32_t i = lo + pj[j];
            uint8_t code = (uint8_t)ERASOR_GROUND_CODE_NOT_JUDGED;
            if (status == ERASOR_GROUND_OK) {
                double x, y, z;
                if (in_lds) {
                    x = (double)lx[j], y = (double)ly[j], z = (double)lz[j];
                } else {
                    const float4 q = pts[i];
                    x = (double)q.x, y = (double)q.y, z = (double)q.z;
                }
                const bool mem = ((nx * x + ny * y) + nz * z) + d < P.th_dist;
                code = mem ? (uint8_t)ERASOR_GROUND_CODE_GROUND : (uint8_t)ERASOR_GROUND_CODE_NOT;
                if (mem) {
                    uint32_t oor = 0;
                    ++g;
                    gd += ev_is_dynamic(pts[i].w, oor) ? 1u : 0u;
                }
            } else if (status != ERASOR_GROUND_DEGENERATE) {
                code = (uint8_t)ERASOR_GROUND_CODE_NOT;
            }
            codes[i] = code;
        }
        g = gr_block_sum<BS>(g, ws, t);
        gd = gr_block_sum<BS>(gd, ws, t);
        if (t == 0) {
            const bool judged = status != ERASOR_GROUND_DEGENERATE;
            if (patches) {
                erasor_ground_patch row;
                row.status = status, row.n_points = m, row.n_ground = g, row.reserved = 0;
                row.normal[0] = judged ? nx : 0.0, row.normal[1] = judged ? ny : 0.0, row.normal[2] = judged ? nz : 0.0;
                row.d = judged ? d : 0.0, row.mean_z = judged ? mz : 0.0;
                row.eig[0] = judged ? l0 : 0.0, row.eig[1] = judged ? l1 : 0.0, row.eig[2] = judged ? l2 : 0.0;
                patches[p] = row;
            }
            atomicAdd(&cf[GR_C_PATCHES], 1ull);
            if (status != ERASOR_GROUND_OK) atomicAdd(&cf[GR_C_STATUS + status], 1ull);
            if (judged) atomicAdd(&cf[GR_C_JUDGED], (unsigned long long)m);
            if (g) atomicAdd(&cf[GR_C_GROUND], (unsigned long long)g);
            if (gd) atomicAdd(&cf[GR_C_GROUND_DYNAMIC], (unsigned long long)gd);
        }
    }
}

// ---- the map form ----

// a map point in a frame: q = ((r0 x + r1 y) + r2 z) + t per row, rounded to float32, with the map point's intensity
__device__ __forceinline__ float4 gr_into_frame(const float4 &p, const VisFrame &F) {
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    float4 q;
    q.x = (float)(((F.m[0] * px + F.m[1] * py) + F.m[2] * pz) + F.m[3]);
    q.y = (float)(((F.m[4] * px + F.m[5] * py) + F.m[6] * pz) + F.m[7]);
    q.z = (float)(((F.m[8] * px + F.m[9] * py) + F.m[10] * pz) + F.m[11]);
    q.w = p.w;
    return q;
}

// whether a frame gathers a map point: finite before and after the transform, and in a patch
__device__ __forceinline__ bool gr_gathered(const float4 &p, const VisFrame &F, const GrParams &P, const double *tab) {
    if (!ev_finite(p)) return false;
    const float4 q = gr_into_frame(p, F);
    if (!ev_finite(q)) return false;
    uint32_t ring, sector;
    return gr_patch_of((double)q.x, (double)q.y, P, tab, &ring, &sector);
}

// (3) one (frame of the batch, map point) pair per lane, frame-major: flag [nb * n]; blockIdx.y: the frame
__global__ __launch_bounds__(256) void k_gr_gather_flag(const float4 *__restrict__ map, uint32_t n, const VisFrame *__restrict__ frames, GrParams P,
                                                         const double *__restrict__ tabs, uint32_t *__restrict__ flag) {
    __shared__ double tab[GR_TAB];
    const uint32_t t = threadIdx.x, i = blockIdx.x * 256u + t, fl = blockIdx.y;
    for (uint32_t j = t; j < (P.R + 1) + (P.M - 1); j += 256u) tab[j] = tabs[j];
    __syncthreads();
    if (i >= n) return;
    flag[(size_t)fl * n + i] = gr_gathered(map[i], frames[fl], P, tab) ? 1u : 0u;
}

// (4) the stable compaction: cloud and midx by the flags' scan (pl, tops); off[fl] = the frame's first place (off[nb], the total, is the
// scan's own output).  A flagged point is transformed again: cheaper than keeping nb * n rounded points between the two launches.
__global__ __launch_bounds__(256) void k_gr_gather_put(const float4 *__restrict__ map, uint32_t n, const VisFrame *__restrict__ frames,
                                                        const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pl,
                                                        const uint32_t *__restrict__ tops, float4 *__restrict__ cloud, uint32_t *__restrict__ midx,
                                                        uint32_t *__restrict__ off) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, fl = blockIdx.y;
    if (i >= n) return;
    const uint32_t g = fl * n + i, pos = pl[g] + tops[g >> 10];
    if (i == 0) off[fl] = pos;
    if (!flag[g]) return;
    cloud[pos] = gr_into_frame(map[i], frames[fl]);
    midx[pos] = i;
}

// (5) the frames' gathered counts from their offsets
__global__ __launch_bounds__(256) void k_gr_count_frames(const uint32_t *__restrict__ off, uint32_t nb, unsigned long long *__restrict__ ctr) {
    const uint32_t fl = blockIdx.x * 256u + threadIdx.x;
    if (fl < nb) ctr[(size_t)fl * GR_NCTR + GR_C_POINTS] = off[fl + 1] - off[fl];
}

// (6) the votes: one gathered point per lane; a map point's word holds seen in its low and ground in its high half (an integer atomic:
// a map point meets every frame once, and at most 65535 frames)
__global__ __launch_bounds__(256) void k_gr_vote(const uint8_t *__restrict__ codes, const uint32_t *__restrict__ midx, const uint32_t *__restrict__ n_dev,
                                                  uint32_t *__restrict__ votes) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= *n_dev) return;
    const uint8_t c = codes[k];
    if (c <= (uint8_t)ERASOR_GROUND_CODE_GROUND) atomicAdd(&votes[midx[k]], c == (uint8_t)ERASOR_GROUND_CODE_GROUND ? 0x10001u : 1u);
}

// (7) the decision per map point: mask (1 = ground) and the flag of the rows asked for (keep: the ground, else the rest)
__global__ __launch_bounds__(256) void k_gr_decide(const float4 *__restrict__ map, uint32_t n, const uint32_t *__restrict__ votes, uint32_t min_votes,
                                                    double ratio, uint32_t keep, uint32_t *__restrict__ flag, uint8_t *__restrict__ mask,
                                                    unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t gd = 0, gs = 0, unseen = 0;
    if (i < n) {
        const uint32_t v = votes[i], seen = v & 0xFFFFu, gr = v >> 16;
        const bool ground = gr >= min_votes && (double)gr > ratio * (double)seen;
        unseen = seen ? 0u : 1u;
        flag[i] = (ground == (keep != 0)) ? 1u : 0u;
        mask[i] = ground ? (uint8_t)1 : (uint8_t)0;
        if (ground) {
            uint32_t oor = 0;
            if (ev_is_dynamic(map[i].w, oor)) gd = 1; else gs = 1;
        }
    }
    ev_commit(ctr, GD_C_GROUND_DYNAMIC, gd);
    ev_commit(ctr, GD_C_GROUND_STATIC, gs);
    ev_commit(ctr, GD_C_UNSEEN, unseen);
}

}  // namespace ek

#endif  // ERASOR_GROUND_HIP_H
