// The clustering's host code and kernels under the host sanitizers: a stand-alone program that is linked with erasor_hip.hip compiled
// against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu), both with -fsanitize=address,undefined.  Device buffers are heap
// blocks there, so an access past one shows.  It clusters a shuffled chain (one cluster, long union-find paths) and 300 identical
// points (every atomic on one row), with every output asked for, then with a short row buffer.  TEST INFRASTRUCTURE ONLY
// (tests/test_cluster_sanitized.py).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
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
    // a chain of 4 096 points 0.45 m apart, shuffled, labels around the dynamic range
    const size_t n = 4096;
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::mt19937 rng(7);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<float> chain(4 * n);
    for (size_t i = 0; i < n; ++i) {
        chain[4 * i] = 0.45f * (float)order[i];
        chain[4 * i + 1] = chain[4 * i + 2] = 0.f;
        chain[4 * i + 3] = (float)(250 + order[i] % 12);
    }
    std::vector<uint32_t> ids(n);
    std::vector<erasor_cluster_row> rows(n);
    std::vector<float> kept(4 * n);
    erasor_cluster_result r;
    rc = erasor_hip_cluster_clouds(h, chain.data(), n, 0, 0.5, 1, 0, ids.data(), rows.data(), rows.size(), kept.data(), n, &r);
    if (rc) return fail("the chain", h, rc);
    if (r.n_clusters != 1 || r.n_listed != 1 || r.largest != n || rows[0].first != 0 || rows[0].n_points != n || rows[0].min_xyz[0] != 0.f ||
        rows[0].max_xyz[0] != 0.45f * (float)(n - 1) || !std::all_of(ids.begin(), ids.end(), [](uint32_t v) { return v == 0; }) || kept != chain)
        return fail("the chain's result", h, 0);
    // at tol 0.4 every point is alone: 4 096 rows do not fit a buffer of 10, which is refused with res filled
    rc = erasor_hip_cluster_clouds(h, chain.data(), n, 0, 0.4, 1, 0, ids.data(), rows.data(), 10, nullptr, 0, &r);
    if (rc != ERASOR_E_CAPACITY || r.n_clusters != n || r.n_singletons != n) return fail("the short row buffer", h, rc);
    // 300 identical points
    std::vector<float> dup(4 * 300);
    for (size_t i = 0; i < 300; ++i) {
        dup[4 * i] = 1.5f, dup[4 * i + 1] = -2.25f, dup[4 * i + 2] = 0.125f, dup[4 * i + 3] = 252.f;
    }
    rc = erasor_hip_cluster_clouds(h, dup.data(), 300, 0, 0.5, 2, 300, ids.data(), rows.data(), rows.size(), kept.data(), n, &r);
    if (rc) return fail("the duplicates", h, rc);
    if (r.n_clusters != 1 || r.n_points_listed != 300 || rows[0].n_dynamic != 300 || rows[0].min_xyz[1] != -2.25f || rows[0].max_xyz[2] != 0.125f)
        return fail("the duplicates' result", h, 0);
    erasor_hip_destroy(h);
    printf("ALL OK\n");
    return 0;
}
