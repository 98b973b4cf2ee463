// The pose refinement under the host sanitizers: a stand-alone program that is linked with erasor_hip.hip compiled against the CPU
// stand-in of the HIP runtime (tests/cpp/simt_emu), both with -fsanitize=address,undefined.  Device buffers are heap blocks and a
// workgroup's LDS arrays are static arrays there, so an access past one shows -- the chunk partials, the per-frame sums and counters,
// the tree across the wavefronts in the walk's stack.  One call with frames of 0, 1, 63 .. 65, 255 .. 257, 511 .. 513 and 1025 points (no
// frame boundary on a multiple of 256 of the buffer), the rows in a heap block of exactly n_frames entries, then without rows and
// without a summary, then against the handle's map.  TEST INFRASTRUCTURE ONLY (tests/test_refine_sanitized.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/erasor_hip.h"

static int fail(const char *what, erasor_hip_handle *h, int rc) {
    printf("FAILED: %s (rc %d: %s)\n", what, rc, h ? erasor_hip_last_error(h) : "");
    return 1;
}

int main() {
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    int rc = erasor_hip_create(&p, 0, &h);
    if (rc) return fail("erasor_hip_create", nullptr, rc);
    // a map of 5 000 points in a 16 m box, flattened towards a floor and two walls
    uint32_t seed = 12345u;
    auto unit = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / 16777216.0f;
    };
    std::vector<float> map;
    for (int i = 0; i < 5000; ++i) {
        float x = 16.0f * unit() - 8.0f, y = 16.0f * unit() - 8.0f, z = 4.0f * unit();
        if (i % 3 == 0) z *= 0.01f;
        if (i % 3 == 1) x = 8.0f + 0.01f * x;
        if (i % 3 == 2) y = 8.0f + 0.01f * y;
        const float row[4] = {x, y, z, 40.0f};
        map.insert(map.end(), row, row + 4);
    }
    const size_t sizes[12] = {1, 63, 0, 64, 65, 255, 256, 257, 511, 512, 513, 1025};
    std::vector<float> scans, Tb;
    std::vector<uint64_t> off{0};
    size_t at = 0;
    for (size_t f = 0; f < 12; ++f) {
        for (size_t k = 0; k < sizes[f]; ++k, at = (at + 7) % 5000) scans.insert(scans.end(), map.begin() + 4 * at, map.begin() + 4 * at + 4);
        off.push_back(scans.size() / 4);
        if (f && off.back() % 256 == 0) return fail("a frame boundary on a chunk boundary", nullptr, (int)f);
        // the map's own points under a pose a little off the identity (frame 3: the identity itself)
        const float d = f == 3 ? 0.0f : 0.01f * (float)(f + 1);
        const float T[16] = {1, -0.2f * d, 0, d, 0.2f * d, 1, 0, -d, 0, 0, 1, 0.5f * d, 0, 0, 0, 1};
        Tb.insert(Tb.end(), T, T + 16);
    }
    const size_t n = scans.size() / 4;
    const erasor_refine_params prm = {0.6, 1e-4, 1e-5, 3, 1};
    erasor_refine_row *rows = (erasor_refine_row *)malloc(12 * sizeof(erasor_refine_row));  // (exactly n_frames entries)
    erasor_refine_summary sum;
    rc = erasor_hip_refine_poses_clouds(h, map.data(), map.size() / 4, 0, scans.data(), n, off.data(), 12, 0, nullptr, Tb.data(), &prm, rows, &sum);
    if (rc) return fail("refine_poses_clouds", h, rc);
    uint64_t by_status = 0;
    for (int s = 0; s < 4; ++s) by_status += sum.n_status[s];
    if (sum.n_frames != 12 || by_status != 12 || sum.n_status[ERASOR_REFINE_NO_POINTS] != 1 || rows[2].status != ERASOR_REFINE_NO_POINTS)
        return fail("the summary", h, (int)by_status);
    for (size_t f = 0; f < 12; ++f)
        if (rows[f].n_points != sizes[f] || rows[f].n_non_finite != 0 || rows[f].T[15] != 1.0 || (sizes[f] && !(rows[f].rms_last <= rows[f].rms_first)))
            return fail("a row", h, (int)f);
    if (rows[3].status != ERASOR_REFINE_CONVERGED || rows[3].iters != 1 || rows[3].rms_last != 0.0 || rows[3].moved_t != 0.0)
        return fail("the frame that was right", h, (int)rows[3].status);
    const double t10 = rows[10].T[3];
    rc = erasor_hip_refine_poses_clouds(h, map.data(), map.size() / 4, 0, scans.data(), n, off.data(), 12, 0, nullptr, Tb.data(), &prm, nullptr, &sum);
    if (rc || sum.n_frames != 12) return fail("no rows", h, rc);
    rc = erasor_hip_refine_poses_clouds(h, map.data(), map.size() / 4, 0, scans.data(), n, off.data(), 12, 0, nullptr, Tb.data(), &prm, rows, nullptr);
    if (rc || rows[10].T[3] != t10) return fail("no summary", h, rc);
    // the handle's map, and a T_lidar2body
    rc = erasor_hip_set_map(h, map.data(), map.size() / 4);
    if (rc) return fail("set_map", h, rc);
    const float Tl[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.05f, 0, 0, 0, 1};
    rc = erasor_hip_refine_poses_map(h, scans.data(), n, off.data(), 12, 0, Tl, Tb.data(), &prm, rows, &sum);
    if (rc || sum.n_frames != 12 || rows[11].n_points != 1025) return fail("refine_poses_map", h, rc);
    free(rows);
    erasor_hip_destroy(h);
    printf("ALL OK\n");
    return 0;
}
