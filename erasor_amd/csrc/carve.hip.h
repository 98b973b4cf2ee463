// carve.hip.h — carving free space: every ray of every scan walked through the map's voxels, the voxels' clamped log-odds integrated
// (erasor_hip_carve_*).  The reference has no such pass: it only compares ERASOR's map with those of OctoMap and Peopleremover
// (compare_results.launch, src/utils/compare_map.cpp, the panels of img/<seq>/README.md, scripts/semantickitti2bag/analysis_octomap.py),
// the two methods that put the map into a voxel grid and walk every ray through it.  This is that argument, so that the comparison's
// other side can be produced, scored (evaluate), drawn (render_eval) and set beside visibility's and ERASOR's output here.
//
// The contract (the normative text is erasor_amd/evalmap.py: carve / carve_brute; the device equals it byte for byte).
// Coordinates are float64 on the float32 inputs.  Every operation is a separate IEEE operation in the order written.  Only + - * /,
// sqrt, floor and comparisons are used.  The log-odds are float32.
// Voxels.
//   - A finite point lies in cell c = floor(x / voxel) per axis.
//   - A map point with a non-finite coordinate lies in no voxel.  It is kept, gets zero votes and log-odds l_init, and is counted as
//     n_map_non_finite.
//   - The map voxels are the cells that hold at least one finite map point.  Only they carry state.
// Rays.
//   - The forward matrix of frame f is the M of visibility_transforms: T_body2origin[f] . T_lidar2body, upper three rows, float32
//     entries widened.
//   - The ray's origin o is M's column 3.
//   - A scan point (x, y, z) in the lidar frame has rho = sqrt((x x + y y) + z z).
//   - The gates, in this order: a non-finite coordinate, then rho outside [min_range, max_range].  Both are dropped and counted per
//     frame.
//   - The end point is e_i = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3].
//   - Under a rigid M the end lies within max_range of the origin, so at most 4097 cells away per axis.  A ray whose end cell is not
//     within 4098 cells of the origin's cell on every axis (a matrix that stretches, or an end that is not finite) is dropped and
//     counted as out of range: this keeps every walk below 3 * 4098 steps whatever the matrix.
// Traversal.
//   - c0 = cell(o), c1 = cell(e), n_a = |c1_a - c0_a|, step_a = +-1, N = n_x + n_y + n_z.
//   - For an axis with n_a > 0: d_a = e_a - o_a; tMax_a = ((c0_a + (step_a > 0 ? 1 : 0)) * voxel - o_a) / d_a; tDelta_a = voxel / |d_a|.
//   - An axis with no steps left never moves.
//   - Each of the N steps moves the axis with the smallest tMax among the axes that still have steps left.  Ties go to x before y
//     before z.
//   - After the move, c_a += step_a, the steps left on that axis drop by one, and tMax_a += tDelta_a.
//   - So the walk visits V_0 = c0 ... V_N = c1, and always ends in c1 whatever the rounding.
//   - Free evidence: V_i for 0 <= i <= N - 1 - stop_short.
//   - Hit evidence: V_N.
//   - n_steps of a ray is max(0, N - stop_short).
// One update per voxel and scan, hits first (OctoMap's insertPointCloud rule).
//   - In frame f a map voxel is hit if any ray of f ends in it.
//   - Otherwise it is free if any ray of f has it as free evidence.
//   - Otherwise it is untouched.
// Integration, per map voxel, frames in index order.
//   - L starts at l_init.
//   - A hit frame: L = min(L + l_hit, l_max), and hits += 1.
//   - A free frame: L = max(L + l_miss, l_min), and misses += 1.
//   - Everything is float32.
//   - The log-odds are parameters.  No kernel calls log.
// Decision.  A map point is removed iff its voxel's L < l_thr.  Every point of a voxel shares its voxel's fate.
//
// The occupancy structure: a hash table with one entry per 4 x 4 x 4 block of voxels (c >> 2 per axis, arithmetic), open addressing
// with linear probing, a power of two of at least twice the point count.  An entry holds the block's coordinates, a 64-bit mask of its
// map voxels (bit (cx & 3) | (cy & 3) << 2 | (cz & 3) << 4) and a base, so that a voxel's dense index is base + popcount(the mask below
// its bit); the per-voxel state (L, hits and misses, a word of frame bits for hits and one for free evidence) is dense over the voxels.
// Built with 32-bit atomics only: k_cv_claim claims a slot by a compare-and-swap of (point index + 1) into the owner word -- a lane
// that finds the slot taken compares blocks by recomputing the owner point's block from its immutable coordinates, never waiting for
// another lane -- and sets the voxel's bit in a half of the mask; k_cv_slots writes every taken slot's coordinates and popcount with
// plain stores; scan_u32 gives the bases (k_cv_base).  Every probe loop is bounded by the capacity.
// k_cv_walk: one scan point per lane over all frames of a batch of at most 32 (the frame by al_frame_of, as k_vis_image); transforms,
// gates and walks the point.  The current block's coordinates, mask and base stay in registers and memory is read only when the block
// coordinate changes: most voxels on a ray are empty and cost nothing.  A map voxel on the way gets the frame's bit in its free word
// (loaded first, the atomic skipped when the bit is there), the end voxel in its hit word; precedence is resolved afterwards, so both
// share the launch.  The loop's bound, max(0, N - stop_short) <= 3 * 4098, is known when the lane enters it.
// k_cv_integrate: one voxel per lane; free & ~hit, then the batch's bits in frame order through the integration; clears the words; the
// frame's distinct-voxel counts by ballot into LDS counters, flushed once per frame and workgroup.
// k_cv_gather: every point's voxel state, keep flag and mask, the removed counts by label per wavefront (as k_vis_decide); the kept
// cloud is the project's stable compaction (scan_u32 + k_f_compact).
//
// Resources (the compiler's report for gfx950): k_cv_claim 38 VGPRs; k_cv_slots 32; k_cv_base 7; k_cv_fill 3; k_cv_walk 54 VGPRs and
// 640 B of LDS; k_cv_integrate 15 VGPRs and 256 B of LDS; k_cv_gather 30 VGPRs; no LDS in the others, no scratch and no spill in any of
// them, 8 wavefronts per SIMD for all (MEASUREMENTS.md "Carve").
#ifndef ERASOR_CARVE_HIP_H
#define ERASOR_CARVE_HIP_H

namespace ek {

static constexpr uint32_t CV_BATCH = 32;          // frames per batch: one bit each in a voxel's two words
static constexpr double CV_CELL_LIMIT = 268435456.0;  // 2^28: a finite map point's or a frame origin's cell coordinate stays inside +- this
static constexpr double CV_MAX_REACH = 4098.0;    // cells between a ray's origin and its end, per axis
static constexpr uint32_t CV_NONE = 0xFFFFFFFFu;  // the slot of a map point that lies in no voxel
static constexpr uint32_t CV_SLOTS_GRID = 2048;   // workgroups of k_cv_slots at most (a grid-stride loop)
// counters of one frame (CV_NCTR per frame, zeroed by the host)
static constexpr uint32_t CV_C_NON_FINITE = 0, CV_C_RANGE = 1, CV_C_RAYS = 2, CV_C_END = 3, CV_C_STEPS = 4, CV_C_VHIT = 5, CV_C_VFREE = 6, CV_NCTR = 8;
static constexpr uint32_t CW_NCTR = CV_C_STEPS + 1;  // what k_cv_walk counts
// counters of the call
enum : uint32_t { CG_C_NON_FINITE = 0, CG_C_BAD_CELL, CG_C_BLOCKS, CG_C_TOUCHED, CG_C_REMOVED_DYNAMIC, CG_C_REMOVED_STATIC, CG_NCTR };

struct alignas(16) CvBlock {
    int32_t bx, by, bz;  // the block's coordinates (k_cv_slots)
    uint32_t base;       // the dense index of its first map voxel (k_cv_base)
    uint32_t mlo, mhi;   // the mask of its map voxels
    uint32_t owner;      // 0: empty; else 1 + the index of the map point that claimed the slot
    uint32_t pad;
};
struct CvParams {
    double voxel, min_range, max_range;
    float l_init, l_hit, l_miss, l_min, l_max, l_thr;
    uint32_t stop_short, pad;
};
// a frame: the forward matrix (per row M[i][0 .. 3]) and the cell of its origin
struct CvFrame {
    double m[12];
    int32_t c0[3];
    int32_t pad;
};

// the cell and the block of a finite map point whose cell is inside the limit; false otherwise
__device__ __forceinline__ bool cv_point_cell(const float4 &p, double voxel, int32_t *cx, int32_t *cy, int32_t *cz) {
    const double fx = floor((double)p.x / voxel), fy = floor((double)p.y / voxel), fz = floor((double)p.z / voxel);
    if (!(fabs(fx) < CV_CELL_LIMIT && fabs(fy) < CV_CELL_LIMIT && fabs(fz) < CV_CELL_LIMIT)) return false;
    *cx = (int32_t)fx, *cy = (int32_t)fy, *cz = (int32_t)fz;
    return true;
}
__device__ __forceinline__ uint32_t cv_bit(int32_t cx, int32_t cy, int32_t cz) {
    return (uint32_t)(cx & 3) | ((uint32_t)(cy & 3) << 2) | ((uint32_t)(cz & 3) << 4);
}

// (1) one map point per lane: its block's slot claimed or found, its voxel's bit set.  tab: [capmask + 1], zeroed by the host;
// slot_of: [n]
__global__ __launch_bounds__(256) void k_cv_claim(const float4 *__restrict__ map, uint32_t n, double voxel, CvBlock *__restrict__ tab, uint32_t capmask,
                                                   uint32_t *__restrict__ slot_of, unsigned long long *__restrict__ gctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t nf = 0, bad = 0;
    if (i < n) {
        const float4 p = map[i];
        int32_t cx = 0, cy = 0, cz = 0;
        uint32_t slot = CV_NONE;
        if (!ev_finite(p)) {
            nf = 1;
        } else if (!cv_point_cell(p, voxel, &cx, &cy, &cz)) {
            bad = 1;
        } else {
            const int32_t bx = cx >> 2, by = cy >> 2, bz = cz >> 2;
            uint32_t s = ev_bucket(bx, by, bz, capmask);
            for (uint32_t probe = 0; probe <= capmask; ++probe) {  // (the table is at most half full: this ends long before)
                const uint32_t old = atomicCAS(&tab[s].owner, 0u, i + 1u);
                if (old == 0u) {
                    slot = s;
                    break;
                }
                int32_t ox = 0, oy = 0, oz = 0;
                cv_point_cell(map[old - 1u], voxel, &ox, &oy, &oz);  // (an owner passed both checks)
                if ((ox >> 2) == bx && (oy >> 2) == by && (oz >> 2) == bz) {
                    slot = s;
                    break;
                }
                s = (s + 1u) & capmask;
            }
            if (slot != CV_NONE) {
                const uint32_t bit = cv_bit(cx, cy, cz);
                uint32_t *half = bit < 32u ? &tab[slot].mlo : &tab[slot].mhi;
                const uint32_t m = 1u << (bit & 31u);
                atomicOr(half, m);
            }
        }
        slot_of[i] = slot;
    }
    ev_commit(gctr, CG_C_NON_FINITE, nf);
    ev_commit(gctr, CG_C_BAD_CELL, bad);
}

// (2) the slots in a grid-stride loop: a taken slot's coordinates (its owner's block) and the number of its map voxels.  cnt:
// [capmask + 1].  The taken slots are counted per lane over the loop and added once per wavefront at the end: one add per wavefront
// of a launch with one slot per lane queued a third of a million adds on one address (EXPERIMENTS.md "Carve").
__global__ __launch_bounds__(256) void k_cv_slots(const float4 *__restrict__ map, double voxel, CvBlock *__restrict__ tab, uint32_t capmask,
                                                   uint32_t *__restrict__ cnt, unsigned long long *__restrict__ gctr) {
    uint32_t taken = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s <= capmask; s += gridDim.x * blockDim.x) {
        const uint32_t o = tab[s].owner;
        uint32_t c = 0;
        if (o) {
            int32_t cx = 0, cy = 0, cz = 0;
            cv_point_cell(map[o - 1u], voxel, &cx, &cy, &cz);
            tab[s].bx = cx >> 2, tab[s].by = cy >> 2, tab[s].bz = cz >> 2;
            c = (uint32_t)__popc(tab[s].mlo) + (uint32_t)__popc(tab[s].mhi);
            ++taken;
        }
        cnt[s] = c;
    }
    ev_commit(gctr, CG_C_BLOCKS, taken);
}

// (3) after scan_u32 over cnt: every slot's base
__global__ __launch_bounds__(256) void k_cv_base(CvBlock *__restrict__ tab, uint32_t capmask, const uint32_t *__restrict__ pl, const uint32_t *__restrict__ tops) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= capmask) tab[s].base = pl[s] + tops[s >> 10];
}

// every voxel's log-odds at the start
__global__ __launch_bounds__(256) void k_cv_fill(float *__restrict__ L, uint32_t n, float v) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) L[i] = v;
}

// the block a walk is in: its coordinates, the mask of its map voxels (0: no such block in the table) and its base
struct CvCur {
    int32_t bx, by, bz;
    uint32_t base;
    uint64_t mask;
};
__device__ __forceinline__ void cv_lookup(const CvBlock *__restrict__ tab, uint32_t capmask, int32_t bx, int32_t by, int32_t bz, CvCur &c) {
    c.bx = bx, c.by = by, c.bz = bz;
    c.mask = 0ull;
    c.base = 0u;
    uint32_t s = ev_bucket(bx, by, bz, capmask);
    for (uint32_t probe = 0; probe <= capmask; ++probe) {
        const uint4 k = *reinterpret_cast<const uint4 *>(&tab[s]);             // bx, by, bz, base
        const uint4 m = *(reinterpret_cast<const uint4 *>(&tab[s]) + 1);       // mlo, mhi, owner
        if (m.z == 0u) return;
        if ((int32_t)k.x == bx && (int32_t)k.y == by && (int32_t)k.z == bz) {
            c.mask = (uint64_t)m.x | ((uint64_t)m.y << 32);
            c.base = k.w;
            return;
        }
        s = (s + 1u) & capmask;
    }
}
// the dense index of voxel (cx, cy, cz), or CV_NONE; the block is looked up when it is not the current one
__device__ __forceinline__ uint32_t cv_voxel(const CvBlock *__restrict__ tab, uint32_t capmask, int32_t cx, int32_t cy, int32_t cz, CvCur &c) {
    const int32_t bx = cx >> 2, by = cy >> 2, bz = cz >> 2;
    if (bx != c.bx || by != c.by || bz != c.bz) cv_lookup(tab, capmask, bx, by, bz, c);
    if (c.mask == 0ull) return CV_NONE;
    const uint32_t bit = cv_bit(cx, cy, cz);
    if (!((c.mask >> bit) & 1ull)) return CV_NONE;
    return c.base + (uint32_t)__popcll(c.mask & ((1ull << bit) - 1ull));
}

// (4) one scan point per lane: workgroup blockIdx.x covers the points (b0 + blockIdx.x) * 256 .. of the concatenated scans, of which
// [lo, hi) belong to the batch's frames [f0, f1), f1 - f0 <= CV_BATCH.  off, wg: as k_vis_image takes them.  wfree, whit: [n_voxels]
// the frame bits of the batch, zero at the start; ctr: [n_frames][CV_NCTR].
__global__ __launch_bounds__(256) void k_cv_walk(const float4 *__restrict__ scans, uint32_t lo, uint32_t hi, uint32_t b0, const uint32_t *__restrict__ off,
                                                  const uint32_t *__restrict__ wg, uint32_t f0, uint32_t f1, CvParams P,
                                                  const CvFrame *__restrict__ frames, const CvBlock *__restrict__ tab, uint32_t capmask,
                                                  uint32_t *__restrict__ wfree, uint32_t *__restrict__ whit, unsigned long long *__restrict__ ctr) {
    __shared__ uint32_t lc[CV_BATCH * CW_NCTR];  // [frame of the span][counter]
    const uint32_t t = threadIdx.x, b = b0 + blockIdx.x, i = b * 256u + t;
    for (uint32_t j = t; j < CV_BATCH * CW_NCTR; j += 256u) lc[j] = 0u;
    __syncthreads();
    // the frames this workgroup touches, inside the batch (at most CV_BATCH)
    const uint32_t fa = wg[b] > f0 ? wg[b] : f0, fz = wg[b + 1] < f1 - 1 ? wg[b + 1] : f1 - 1;
    if (i >= lo && i < hi) {
        const uint32_t f = al_frame_of(off, i, fa, fz);
        const float4 p = scans[i];
        uint32_t *c = lc + (f - fa) * CW_NCTR;
        if (!ev_finite(p)) {
            atomicAdd(&c[CV_C_NON_FINITE], 1u);
        } else {
            const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
            const double rho = sqrt((x * x + y * y) + z * z);
            const CvFrame &F = frames[f];
            const double ox = F.m[3], oy = F.m[7], oz = F.m[11];
            const double ex = ((F.m[0] * x + F.m[1] * y) + F.m[2] * z) + ox;
            const double ey = ((F.m[4] * x + F.m[5] * y) + F.m[6] * z) + oy;
            const double ez = ((F.m[8] * x + F.m[9] * y) + F.m[10] * z) + oz;
            int32_t cx = F.c0[0], cy = F.c0[1], cz = F.c0[2];
            const double gx = floor(ex / P.voxel), gy = floor(ey / P.voxel), gz = floor(ez / P.voxel);
            const bool reach = fabs(gx - (double)cx) <= CV_MAX_REACH && fabs(gy - (double)cy) <= CV_MAX_REACH && fabs(gz - (double)cz) <= CV_MAX_REACH;
            if (!(rho >= P.min_range && rho <= P.max_range) || !reach) {
                atomicAdd(&c[CV_C_RANGE], 1u);
            } else {
                const int32_t c1x = (int32_t)gx, c1y = (int32_t)gy, c1z = (int32_t)gz;
                const int32_t sx = c1x > cx ? 1 : -1, sy = c1y > cy ? 1 : -1, sz = c1z > cz ? 1 : -1;
                uint32_t lx = (uint32_t)(c1x > cx ? c1x - cx : cx - c1x), ly = (uint32_t)(c1y > cy ? c1y - cy : cy - c1y),
                         lz = (uint32_t)(c1z > cz ? c1z - cz : cz - c1z);
                const uint32_t N = lx + ly + lz, n_free = N > P.stop_short ? N - P.stop_short : 0u;
                double tx = 0.0, ty = 0.0, tz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0;
                if (lx) {
                    const double d = ex - ox;
                    tx = ((double)(cx + (sx > 0 ? 1 : 0)) * P.voxel - ox) / d;
                    dx = P.voxel / fabs(d);
                }
                if (ly) {
                    const double d = ey - oy;
                    ty = ((double)(cy + (sy > 0 ? 1 : 0)) * P.voxel - oy) / d;
                    dy = P.voxel / fabs(d);
                }
                if (lz) {
                    const double d = ez - oz;
                    tz = ((double)(cz + (sz > 0 ? 1 : 0)) * P.voxel - oz) / d;
                    dz = P.voxel / fabs(d);
                }
                const uint32_t fbit = 1u << (f - f0);
                CvCur cur;
                cur.bx = cur.by = cur.bz = (int32_t)0x80000000;  // (no block: |c >> 2| < 2^27)
                cur.base = 0u;
                cur.mask = 0ull;
                for (uint32_t k = 0; k < n_free; ++k) {  // V_k, then the move to V_(k+1): k < N, so a step is left
                    const uint32_t v = cv_voxel(tab, capmask, cx, cy, cz, cur);
                    if (v != CV_NONE && !(wfree[v] & fbit)) atomicOr(&wfree[v], fbit);
                    const bool mx = lx && (!ly || tx <= ty) && (!lz || tx <= tz);
                    const bool my = !mx && ly && (!lz || ty <= tz);
                    if (mx) {
                        cx += sx, --lx, tx += dx;
                    } else if (my) {
                        cy += sy, --ly, ty += dy;
                    } else {
                        cz += sz, --lz, tz += dz;
                    }
                }
                const uint32_t v = cv_voxel(tab, capmask, c1x, c1y, c1z, cur);
                if (v != CV_NONE) {
                    if (!(whit[v] & fbit)) atomicOr(&whit[v], fbit);
                    atomicAdd(&c[CV_C_END], 1u);
                }
                atomicAdd(&c[CV_C_RAYS], 1u);
                if (n_free) atomicAdd(&c[CV_C_STEPS], n_free);
            }
        }
    }
    __syncthreads();
    if (fz >= fa) {
        const uint32_t m = (fz - fa + 1) * CW_NCTR;
        for (uint32_t j = t; j < m; j += 256u)
            if (lc[j]) atomicAdd(&ctr[(size_t)(fa + j / CW_NCTR) * CV_NCTR + j % CW_NCTR], (unsigned long long)lc[j]);
    }
}

// (5) one voxel per lane after a batch's walk: nb = the batch's frames, from f0.  hm: hits | misses << 16
__global__ __launch_bounds__(256) void k_cv_integrate(uint32_t n_voxels, uint32_t f0, uint32_t nb, CvParams P, float *__restrict__ L, uint32_t *__restrict__ hm,
                                                       uint32_t *__restrict__ wfree, uint32_t *__restrict__ whit, unsigned long long *__restrict__ ctr,
                                                       unsigned long long *__restrict__ gctr) {
    __shared__ uint32_t lc[CV_BATCH * 2];  // [frame of the batch][hit, free]
    const uint32_t t = threadIdx.x, v = blockIdx.x * 256u + t;
    if (t < CV_BATCH * 2) lc[t] = 0u;
    __syncthreads();
    uint32_t h = 0, fr = 0, touched = 0;
    if (v < n_voxels) {
        h = whit[v];
        fr = wfree[v];
        if (h) whit[v] = 0u;
        if (fr) wfree[v] = 0u;
        fr &= ~h;  // hits first
        if (h | fr) {
            float l = L[v];
            const uint32_t old = hm[v];
            uint32_t hits = old & 0xFFFFu, misses = old >> 16;
            for (uint32_t k = 0; k < nb; ++k) {
                if ((h >> k) & 1u) {
                    const float s = l + P.l_hit;
                    l = s < P.l_max ? s : P.l_max;
                    ++hits;
                } else if ((fr >> k) & 1u) {
                    const float s = l + P.l_miss;
                    l = s > P.l_min ? s : P.l_min;
                    ++misses;
                }
            }
            L[v] = l;
            hm[v] = hits | (misses << 16);
            touched = old == 0u ? 1u : 0u;
        }
    }
    if (__ballot((h | fr) != 0u)) {  // (uniform over the wavefront)
        const bool lead = (t & 63u) == 0;
        for (uint32_t k = 0; k < nb; ++k) {
            const uint32_t ch = (uint32_t)__popcll(__ballot((h >> k) & 1u)), cf = (uint32_t)__popcll(__ballot((fr >> k) & 1u));
            if (lead && ch) atomicAdd(&lc[2 * k], ch);
            if (lead && cf) atomicAdd(&lc[2 * k + 1], cf);
        }
    }
    ev_commit(gctr, CG_C_TOUCHED, touched);
    __syncthreads();
    if (t < nb * 2 && lc[t]) atomicAdd(&ctr[(size_t)(f0 + t / 2) * CV_NCTR + CV_C_VHIT + (t & 1u)], (unsigned long long)lc[t]);
}

// (6) every map point's voxel state and fate: votes (hits | misses << 16), logodds, flag (uint32, for the compaction's scan) and mask
// (uint8), 1 = kept; the removed points by label per wavefront
__global__ __launch_bounds__(256) void k_cv_gather(const float4 *__restrict__ map, uint32_t n, const uint32_t *__restrict__ slot_of,
                                                    const CvBlock *__restrict__ tab, CvParams P, const float *__restrict__ L, const uint32_t *__restrict__ hm,
                                                    uint32_t *__restrict__ votes, float *__restrict__ logodds, uint32_t *__restrict__ flag,
                                                    uint8_t *__restrict__ mask, unsigned long long *__restrict__ gctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t rd = 0, rs = 0;
    if (i < n) {
        const uint32_t s = slot_of[i];
        uint32_t vt = 0;
        float l = P.l_init;
        bool removed = false;
        const float4 p = map[i];
        if (s != CV_NONE) {
            int32_t cx = 0, cy = 0, cz = 0;
            cv_point_cell(p, P.voxel, &cx, &cy, &cz);
            const CvBlock B = tab[s];
            const uint64_t m = (uint64_t)B.mlo | ((uint64_t)B.mhi << 32);
            const uint32_t v = B.base + (uint32_t)__popcll(m & ((1ull << cv_bit(cx, cy, cz)) - 1ull));
            vt = hm[v];
            l = L[v];
            removed = l < P.l_thr;
        }
        votes[i] = vt;
        logodds[i] = l;
        flag[i] = removed ? 0u : 1u;
        mask[i] = removed ? (uint8_t)0 : (uint8_t)1;
        if (removed) {
            uint32_t oor = 0;
            if (ev_is_dynamic(p.w, oor)) rd = 1; else rs = 1;
        }
    }
    ev_commit(gctr, CG_C_REMOVED_DYNAMIC, rd);
    ev_commit(gctr, CG_C_REMOVED_STATIC, rs);
}

}  // namespace ek

#endif  // ERASOR_CARVE_HIP_H
