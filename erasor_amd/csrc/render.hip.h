// render.hip.h — bird's-eye (top-down, orthographic) images of XYZI clouds, rasterised on the device.
//
// Replaces what the reference looks at in RViz: src/utils/viz_kitti_map.cpp:27-82,118-125 (one map as static / dynamic / one chosen class or
// instance) and src/utils/compare_map.cpp:65-96 (ground truth and the methods' maps split into static and dynamic points, side by side),
// plus the error map no reference tool draws: every ground-truth point coloured by what the evaluator (evaluate.hip.h) decided for it.
//
// The image is a function of the point SET: every point has a priority (its category's) and a height, the winner of a pixel is the
// largest (priority, z) with z in float32's total order, and the colour depends on (category, z) only -- equal winners give equal
// colours, so the order of the points and of the atomics never shows.  The same on the host: erasor_amd/evalmap.py (render / render_eval).
//
// Shape (cdna_hip_programming.md Guideline 12 and Appendix B 'Scatter / gather': a store pass plus a per-destination pass, not one
// 64-bit global atomic per point scattered over a key image of up to 512 MB):
//   k_rd_bin      one point per lane: category, pixel, tile (64 x 64 pixels) and the 47-bit record (priority, ordered z, pixel in tile);
//                 tile histogram with one atomic per distinct tile of a wavefront (match_any); the point counters per workgroup
//   scan_u32      tile offsets
//   k_rd_scatter  records into their tile's range (one atomic per distinct tile of a wavefront; the order inside a tile is free)
//   k_rd_resolve  one workgroup per tile: LDS atomic max over 4096 keys (32 KiB), shading, the tile's RGB rows with plain stores
//                 (32-bit where the row is aligned), the pixels won per category with one global add per category and tile
// Every pixel of the image is written by exactly one workgroup (empty tiles write the background): no clear pass.
#ifndef ERASOR_RENDER_HIP_H
#define ERASOR_RENDER_HIP_H

namespace ek {

enum : uint32_t { RD_LABEL = 0, RD_HEIGHT = 1, RD_EVAL = 2 };
static constexpr uint32_t RD_TILE = 64, RD_TPIX = RD_TILE * RD_TILE, RD_NCAT = 8;
// counters of one render: [RD_C_CATPTS + c] points drawn of category c, [RD_C_CATPIX + c] pixels won by it
enum : uint32_t { RD_C_OUTSIDE = 0, RD_C_NONFINITE = 1, RD_C_CATPTS = 2, RD_C_CATPIX = RD_C_CATPTS + RD_NCAT, RD_NCTR = RD_C_CATPIX + RD_NCAT };
static constexpr uint32_t RD_NO_TILE = 0xFFFFFFFFu;

struct RdView {
    double x0, y0, res, z_lo, z_hi;
    uint32_t width, height, tiles_x, background;
};
struct RdMode {
    uint32_t mode;
    int32_t target_class, target_instance;  // RD_LABEL: < 0 = none / any
    uint32_t palette[RD_NCAT];              // 0xRRGGBB per category
};

// first category of a mode; category = base + priority - 1 (include/erasor_hip.h: ERASOR_RENDER_CAT_*)
__host__ __device__ __forceinline__ uint32_t rd_cat_base(uint32_t mode) { return mode == RD_LABEL ? 0u : mode == RD_HEIGHT ? 3u : 4u; }

// float32's total order as an unsigned key (-0.0 below +0.0) and back
__device__ __forceinline__ uint32_t rd_zord(float z) {
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rd_zinv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// priority (1..4) of a point within its mode
__device__ __forceinline__ uint32_t rd_priority(const float4 &p, const RdMode &m, const uint8_t *__restrict__ code, uint32_t i) {
    if (m.mode == RD_HEIGHT) return 1u;
    uint32_t oor = 0;
    const bool dyn = ev_is_dynamic(p.w, oor);
    if (m.mode == RD_LABEL) {
        if (!dyn) return 1u;
        const uint32_t lab = (uint32_t)p.w;  // (in range: the point is dynamic)
        const bool target = m.target_class >= 0 && (lab & 0xFFFFu) == (uint32_t)m.target_class &&
                            (m.target_instance < 0 || (lab >> 16) == (uint32_t)m.target_instance);
        return target ? 3u : 2u;
    }
    const uint8_t c = code[i];
    if (c == EV_KEPT_S) return 1u;  // static kept
    if (c == EV_KEPT_D) return 4u;  // dynamic left
    return dyn ? 2u : 3u;           // dynamic removed : static lost
}

// column and image row (north up) of a finite point; false when it is off the image.  float64 from the float32 coordinates, every
// operation on its own, the range test on the doubles.
__device__ __forceinline__ bool rd_pixel(const float4 &p, const RdView &v, uint32_t &col, uint32_t &row) {
    const double fx = floor(((double)p.x - v.x0) / v.res), fy = floor(((double)p.y - v.y0) / v.res);
    if (!(fx >= 0.0 && fx < (double)v.width && fy >= 0.0 && fy < (double)v.height)) return false;
    col = (uint32_t)fx;
    row = v.height - 1u - (uint32_t)fy;
    return true;
}

// A workgroup's point counters -- outside, non-finite, drawn per priority 1..4 -- into ctr: a ballot per counter and wavefront, summed in
// LDS, then ONE 64-bit add per workgroup and non-zero counter (six adds per wavefront on the same few addresses were most of this
// kernel's time: memory-side atomics, one line).  Every lane of the workgroup calls this.
__device__ __forceinline__ void rd_commit_points(unsigned long long *__restrict__ ctr, uint32_t mode, uint32_t outside, uint32_t bad, uint32_t prio) {
    __shared__ uint32_t sum[6];
    if (threadIdx.x < 6) sum[threadIdx.x] = 0u;
    __syncthreads();
    const bool flag[6] = {outside != 0u, bad != 0u, prio == 1u, prio == 2u, prio == 3u, prio == 4u};
#pragma unroll
    for (uint32_t c = 0; c < 6; ++c) {
        const uint32_t w = (uint32_t)__popcll(__ballot(flag[c]));
        if ((threadIdx.x & 63u) == 0 && w) atomicAdd(&sum[c], w);
    }
    __syncthreads();
    if (threadIdx.x < 6 && sum[threadIdx.x])
        atomicAdd(&ctr[threadIdx.x < 2 ? threadIdx.x : RD_C_CATPTS + rd_cat_base(mode) + threadIdx.x - 2u], (unsigned long long)sum[threadIdx.x]);
}

// (1) per point: tile and record; tile histogram (cnt: [tiles + 1], zeroed by the host); counters
__global__ __launch_bounds__(256) void k_rd_bin(const float4 *__restrict__ pts, uint32_t n, const uint8_t *__restrict__ code, RdView v, RdMode m,
                                                 uint32_t *__restrict__ tile_of, unsigned long long *__restrict__ rec, uint32_t *__restrict__ cnt,
                                                 unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t tile = RD_NO_TILE, prio = 0, outside = 0, bad = 0;
    if (i < n) {
        const float4 p = pts[i];
        unsigned long long r = 0ull;
        uint32_t col = 0, row = 0;
        if (!ev_finite(p)) {
            bad = 1;
        } else if (!rd_pixel(p, v, col, row)) {
            outside = 1;
        } else {
            prio = rd_priority(p, m, code, i);
            tile = (row / RD_TILE) * v.tiles_x + col / RD_TILE;
            r = ((unsigned long long)prio << 44) | ((unsigned long long)rd_zord(p.z) << 12) | ((row % RD_TILE) * RD_TILE + col % RD_TILE);
        }
        tile_of[i] = tile;
        rec[i] = r;
    }
    const bool drawn = tile != RD_NO_TILE;
    const uint64_t peers = match_any(tile, drawn, 32);
    if (drawn && (peers & lanemask_lt()) == 0ull) atomicAdd(&cnt[tile], (uint32_t)__popcll(peers));
    rd_commit_points(ctr, m.mode, outside, bad, prio);
}

// (2) after scan_u32 and k_ev_offsets over cnt: every drawn point's record into its tile's range (cursor[t]: the tile's next free slot)
__global__ __launch_bounds__(256) void k_rd_scatter(const uint32_t *__restrict__ tile_of, const unsigned long long *__restrict__ rec, uint32_t n,
                                                     uint32_t *__restrict__ cursor, unsigned long long *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t tile = i < n ? tile_of[i] : RD_NO_TILE;
    const bool valid = tile != RD_NO_TILE;
    const uint64_t peers = match_any(tile, valid, 32);
    const uint64_t lt = lanemask_lt();
    uint32_t base = 0;
    if (valid && (peers & lt) == 0ull) base = atomicAdd(&cursor[tile], (uint32_t)__popcll(peers));
    base = __shfl(base, valid ? (int)__builtin_ctzll(peers) : (int)(threadIdx.x & 63u));  // (the group's lowest lane made the reservation)
    if (valid) out[base + (uint32_t)__popcll(peers & lt)] = rec[i];
}

// shade of a height: s = z_hi > z_lo ? clamp((z - z_lo) / (z_hi - z_lo), 0, 1) : 1, factor 0.35 + 0.65 * s
__device__ __forceinline__ double rd_factor(float z, const RdView &v) {
    double s = 1.0;
    if (v.z_hi > v.z_lo) {
        s = ((double)z - v.z_lo) / (v.z_hi - v.z_lo);
        s = s < 0.0 ? 0.0 : s;
        s = s > 1.0 ? 1.0 : s;
    }
    return 0.35 + 0.65 * s;
}
__device__ __forceinline__ uint8_t rd_channel(uint32_t base, double f) { return (uint8_t)floor((double)base * f + 0.5); }

// (3) one workgroup per tile: off[t] .. off[t + 1] are its records.  img: height x width x 3 bytes, 4-byte aligned.
__global__ __launch_bounds__(256) void k_rd_resolve(const unsigned long long *__restrict__ recs, const uint32_t *__restrict__ off, RdView v, RdMode m,
                                                     uint8_t *__restrict__ img, unsigned long long *__restrict__ ctr) {
    __shared__ unsigned long long key[RD_TPIX];
    __shared__ uint8_t rgb[RD_TPIX * 3];
    __shared__ uint32_t won[4];
    const uint32_t t = blockIdx.x, tid = threadIdx.x;
    const uint32_t b = off[t], e = off[t + 1];
    for (uint32_t p = tid; p < RD_TPIX; p += 256) key[p] = 0ull;
    if (tid < 4) won[tid] = 0u;
    __syncthreads();
    for (uint32_t s = b + tid; s < e; s += 256) {
        const unsigned long long r = recs[s];
        atomicMax(&key[(uint32_t)r & (RD_TPIX - 1u)], r >> 12);
    }
    __syncthreads();
    const uint32_t bg[3] = {(v.background >> 16) & 0xFFu, (v.background >> 8) & 0xFFu, v.background & 0xFFu};
    const uint32_t cat0 = rd_cat_base(m.mode);
    uint32_t mine[4] = {0u, 0u, 0u, 0u};
    for (uint32_t p = tid; p < RD_TPIX; p += 256) {
        const unsigned long long k = key[p];
        uint32_t c3[3] = {bg[0], bg[1], bg[2]};
        if (k != 0ull) {
            const uint32_t prio = (uint32_t)(k >> 32);
            const uint32_t base = m.palette[cat0 + prio - 1u];
            const double f = rd_factor(rd_zinv((uint32_t)k), v);
            c3[0] = rd_channel((base >> 16) & 0xFFu, f);
            c3[1] = rd_channel((base >> 8) & 0xFFu, f);
            c3[2] = rd_channel(base & 0xFFu, f);
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) mine[q] += prio == q + 1u ? 1u : 0u;
        }
        rgb[p * 3 + 0] = (uint8_t)c3[0];
        rgb[p * 3 + 1] = (uint8_t)c3[1];
        rgb[p * 3 + 2] = (uint8_t)c3[2];
    }
    if (e > b) {  // (uniform over the workgroup)
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t s = wave_sum(mine[q]);
            if ((tid & 63u) == 0 && s) atomicAdd(&won[q], s);
        }
    }
    __syncthreads();
    if (tid < 4 && won[tid]) atomicAdd(&ctr[RD_C_CATPIX + cat0 + tid], (unsigned long long)won[tid]);
    // the tile's rows: row r of the tile is bytes [g0, g0 + len) of the image; lane j of a row takes the aligned word at (g0 & ~3) + 4 j
    const uint32_t px0 = (t % v.tiles_x) * RD_TILE, py0 = (t / v.tiles_x) * RD_TILE;
    const uint32_t w = min(RD_TILE, v.width - px0), hgt = min(RD_TILE, v.height - py0);
    const uint32_t len = w * 3u;
    constexpr uint32_t WPR = RD_TILE * 3 / 4 + 1;  // words a row of 192 bytes can touch
    for (uint32_t idx = tid; idx < hgt * WPR; idx += 256) {
        const uint32_t r = idx / WPR, j = idx % WPR;
        const size_t g0 = ((size_t)(py0 + r) * v.width + px0) * 3u;
        const size_t wa = (g0 & ~(size_t)3) + 4u * j;
        if (wa >= g0 + len) continue;
        const uint8_t *src = rgb + (size_t)r * RD_TILE * 3;
        if (wa >= g0 && wa + 4 <= g0 + len) {
            const uint32_t o = (uint32_t)(wa - g0);
            *(uint32_t *)(img + wa) = (uint32_t)src[o] | ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16) | ((uint32_t)src[o + 3] << 24);
        } else {
            for (uint32_t q = 0; q < 4; ++q)
                if (wa + q >= g0 && wa + q < g0 + len) img[wa + q] = src[wa + q - g0];
        }
    }
}

// The other rasteriser (test hook only, for the comparison in MEASUREMENTS.md): one 64-bit atomic max per point on a key image in
// device memory, then a pass over the pixels.
#ifdef ERASOR_HIP_TEST_HOOKS
__global__ __launch_bounds__(256) void k_rd_atomic_points(const float4 *__restrict__ pts, uint32_t n, const uint8_t *__restrict__ code, RdView v, RdMode m,
                                                           unsigned long long *__restrict__ keyimg, unsigned long long *__restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t prio = 0, outside = 0, bad = 0;
    if (i < n) {
        const float4 p = pts[i];
        uint32_t col = 0, row = 0;
        if (!ev_finite(p)) {
            bad = 1;
        } else if (!rd_pixel(p, v, col, row)) {
            outside = 1;
        } else {
            prio = rd_priority(p, m, code, i);
            atomicMax(&keyimg[(size_t)row * v.width + col], ((unsigned long long)prio << 32) | rd_zord(p.z));
        }
    }
    rd_commit_points(ctr, m.mode, outside, bad, prio);
}
__global__ __launch_bounds__(256) void k_rd_atomic_pixels(const unsigned long long *__restrict__ keyimg, RdView v, RdMode m, uint8_t *__restrict__ img,
                                                           unsigned long long *__restrict__ ctr) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x, npix = (size_t)v.width * v.height;
    const uint32_t cat0 = rd_cat_base(m.mode);
    uint32_t prio = 0;
    if (p < npix) {
        const unsigned long long k = keyimg[p];
        uint32_t c3[3] = {(v.background >> 16) & 0xFFu, (v.background >> 8) & 0xFFu, v.background & 0xFFu};
        if (k != 0ull) {
            prio = (uint32_t)(k >> 32);
            const uint32_t base = m.palette[cat0 + prio - 1u];
            const double f = rd_factor(rd_zinv((uint32_t)k), v);
            c3[0] = rd_channel((base >> 16) & 0xFFu, f);
            c3[1] = rd_channel((base >> 8) & 0xFFu, f);
            c3[2] = rd_channel(base & 0xFFu, f);
        }
        img[p * 3 + 0] = (uint8_t)c3[0];
        img[p * 3 + 1] = (uint8_t)c3[1];
        img[p * 3 + 2] = (uint8_t)c3[2];
    }
    // (the pixels won per priority, one add per workgroup and counter, as rd_commit_points does it)
    __shared__ uint32_t sum[4];
    if (threadIdx.x < 4) sum[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 1; q <= 4; ++q) {
        const uint32_t w = (uint32_t)__popcll(__ballot(prio == q));
        if ((threadIdx.x & 63u) == 0 && w) atomicAdd(&sum[q - 1], w);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sum[threadIdx.x]) atomicAdd(&ctr[RD_C_CATPIX + cat0 + threadIdx.x], (unsigned long long)sum[threadIdx.x]);
}
#endif

// ---- the view fitted to a cloud (erasor_hip_render_fit) ----
// zb[i] = the ordered height of point i as a 64-bit value for the exact radix select (k_ov_select_hist), ~0 for a non-finite point (above
// every rank of the finite ones); bb: ordered keys min x, min y (start ~0), max x, max y (start 0); ctr[0]: finite points.
// Eight points per lane: the box costs four atomics per wavefront.
__global__ __launch_bounds__(256) void k_rd_fit(const float4 *__restrict__ pts, uint32_t n, unsigned long long *__restrict__ zb, uint32_t *__restrict__ bb,
                                                 unsigned long long *__restrict__ ctr) {
    uint32_t mnx = 0xFFFFFFFFu, mny = 0xFFFFFFFFu, mxx = 0u, mxy = 0u, fin = 0;
    for (uint32_t k = 0; k < 8; ++k) {
        const uint32_t i = blockIdx.x * 2048u + k * 256u + threadIdx.x;
        if (i >= n) break;
        const float4 p = pts[i];
        if (ev_finite(p)) {
            const uint32_t kx = rd_zord(p.x), ky = rd_zord(p.y);
            mnx = min(mnx, kx);
            mny = min(mny, ky);
            mxx = max(mxx, kx);
            mxy = max(mxy, ky);
            zb[i] = (unsigned long long)rd_zord(p.z);
            ++fin;
        } else {
            zb[i] = ~0ull;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, d));
        mny = min(mny, __shfl_xor(mny, d));
        mxx = max(mxx, __shfl_xor(mxx, d));
        mxy = max(mxy, __shfl_xor(mxy, d));
    }
    const uint32_t s = wave_sum(fin);
    if ((threadIdx.x & 63u) == 0 && s) {
        atomicMin(&bb[0], mnx);
        atomicMin(&bb[1], mny);
        atomicMax(&bb[2], mxx);
        atomicMax(&bb[3], mxy);
        atomicAdd(&ctr[0], (unsigned long long)s);
    }
}

}  // namespace ek

#endif  // ERASOR_RENDER_HIP_H
