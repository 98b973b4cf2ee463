// The k nearest neighbours, the radius counts and the density filters under the host sanitizers: a stand-alone program that is linked
// with erasor_hip.hip compiled against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu), both with -fsanitize=address,undefined.
// Device buffers are heap blocks and a workgroup's LDS arrays are static arrays there, so an access past one shows.  It searches a lattice
// with 300 copies of one point in it (ties everywhere) at k = 1, 8, 9, 32 with every output, a cloud shorter than k, and runs every filter
// with a mask, a kept cloud and a kept buffer one row short.  TEST INFRASTRUCTURE ONLY (tests/test_knn_sanitized.py).
#include <algorithm>
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
    // a 13 x 13 x 13 lattice at 0.5 m (2 197 points: 69 leaves, padded to 128), then 300 copies of its first point
    std::vector<float> c;
    for (int x = 0; x < 13; ++x)
        for (int y = 0; y < 13; ++y)
            for (int z = 0; z < 13; ++z) {
                const float row[4] = {0.5f * x, 0.5f * y, 0.5f * z, (float)(250 + (x + y + z) % 12)};
                c.insert(c.end(), row, row + 4);
            }
    for (int k = 0; k < 300; ++k) c.insert(c.end(), c.begin(), c.begin() + 4);
    const size_t n = c.size() / 4;
    for (uint32_t k : {1u, 8u, 9u, 32u}) {
        std::vector<uint32_t> ni(n * k);
        std::vector<double> nd(n * k), kth(n), mean(n);
        erasor_knn_result r;
        rc = erasor_hip_knn_clouds(h, c.data(), n, 0, k, ni.data(), nd.data(), kth.data(), mean.data(), &r);
        if (rc) return fail("knn", h, rc);
        // the copies are each other's neighbours at distance 0, lowest indices first; point 0 is one of them
        const uint32_t first = ni[0], want = (uint32_t)(n - 300);
        if (r.n_points != n || r.n_short != 0 || r.kth.n_scored != n || first != want || nd[0] != 0.0 || kth[n - 1] != 0.0 || !(r.kth.max >= 0.5))
            return fail("knn's result", h, (int)k);
    }
    {  // fewer than k other points: padding
        std::vector<uint32_t> ni(5 * 32);
        std::vector<double> nd(5 * 32), kth(5), mean(5);
        erasor_knn_result r;
        rc = erasor_hip_knn_clouds(h, c.data(), 5, 0, 32, ni.data(), nd.data(), kth.data(), mean.data(), &r);
        if (rc) return fail("the short cloud", h, rc);
        if (r.n_short != 5 || r.kth.n_scored != 0 || ni[4] != 0xFFFFFFFFu || ni[3] == 0xFFFFFFFFu || !std::isinf(nd[31]) || !std::isinf(mean[4]))
            return fail("the short cloud's result", h, 0);
    }
    std::vector<uint32_t> cnt(n);
    erasor_score_stats st;
    rc = erasor_hip_radius_count_clouds(h, c.data(), n, 0, 0.5, cnt.data(), &st);
    if (rc) return fail("radius_count", h, rc);
    // an inner lattice point has its 6 axis neighbours; point 0, a corner, has 3 and the 300 copies
    if (st.n_scored != n || cnt[0] != 303 || cnt[(6 * 13 + 6) * 13 + 6] != 6 || st.max != (double)*std::max_element(cnt.begin(), cnt.end()) ||
        st.min != (double)*std::min_element(cnt.begin(), cnt.end()))
        return fail("radius_count's result", h, (int)cnt[0]);
    for (int score = 0; score < 3; ++score)
        for (int rule = 0; rule < 2; ++rule) {
            erasor_density_filter f = {score, rule, 8, 7, 0.5, 0.5, 1.0};
            std::vector<uint8_t> mask(n);
            std::vector<float> kept(4 * n);
            erasor_density_result r;
            rc = erasor_hip_density_filter_clouds(h, c.data(), n, 0, &f, mask.data(), kept.data(), n, &r);
            if (rc) return fail("density_filter", h, rc);
            size_t nk = 0;
            for (uint8_t m : mask) nk += m;
            if (r.n_points != n || nk != r.n_kept || r.n_kept + r.n_removed != n || r.n_removed_dynamic + r.n_removed_static != r.n_removed || r.n_kept == 0)
                return fail("density_filter's result", h, score * 2 + rule);
            std::vector<float> tight(4 * (r.n_kept - 1) + 4);
            rc = erasor_hip_density_filter_clouds(h, c.data(), n, 0, &f, mask.data(), tight.data(), r.n_kept - 1, &r);
            if (rc != ERASOR_E_CAPACITY) return fail("the short kept buffer", h, rc);
            tight.resize(4 * r.n_kept);
            rc = erasor_hip_density_filter_clouds(h, c.data(), n, 0, &f, nullptr, tight.data(), r.n_kept, &r);
            if (rc || !std::equal(tight.begin(), tight.end(), kept.begin())) return fail("the exact kept buffer", h, rc);
        }
    erasor_hip_destroy(h);
    printf("ALL OK\n");
    return 0;
}
