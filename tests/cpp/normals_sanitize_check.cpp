// Surface normals, curvature and eigenvalues under the host sanitizers: a stand-alone program that is linked with erasor_hip.hip compiled
// against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu), both with -fsanitize=address,undefined.  Device buffers are heap
// blocks and a workgroup's LDS arrays are static arrays there, so an access past one shows.  It runs a lattice with 300 copies of one
// point in it (ties everywhere, degenerate neighbourhoods among them) at k = 2, 8, 9, 32 with every combination of outputs in exactly
// sized buffers, a cloud shorter than k, and both orientation rules.  TEST INFRASTRUCTURE ONLY (tests/test_normals_sanitized.py).
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
    const double view[3] = {3.0, 3.0, 40.0};
    for (uint32_t k : {2u, 8u, 9u, 32u})
        for (int use = 0; use < 8; ++use)
            for (int oriented = use == 7 ? 0 : (use >> 1) & 1; oriented <= (use == 7 ? 1 : (use >> 1) & 1); ++oriented) {  // (both rules with every output)
                // exactly sized buffers: one element past any of them is the sanitizer's
                std::vector<float> nrm(use & 1 ? 3 * n : 0);
                std::vector<double> curv(use & 2 ? n : 0), eig(use & 4 ? 3 * n : 0);
                erasor_normals_result r;
                rc = erasor_hip_normals_clouds(h, c.data(), n, 0, k, oriented ? view : nullptr, use & 1 ? nrm.data() : nullptr,
                                               use & 2 ? curv.data() : nullptr, use & 4 ? eig.data() : nullptr, &r);
                if (rc) return fail("normals", h, rc);
                // the 301 points at the lattice's first corner see only each other: no extent
                if (r.n_points != n || r.n_short != 0 || r.n_degenerate != 301 || r.curvature.n_scored != n - 301 || !(r.curvature.min >= 0) ||
                    !(r.curvature.max <= 1.0 / 3.0 + 1e-9))
                    return fail("normals' result", h, (int)k);
                if ((use & 1) && (!std::isnan(nrm[0]) || !std::isnan(nrm[3 * n - 1]) || std::isnan(nrm[3 * 1000]))) return fail("the normals", h, (int)k);
                if ((use & 2) && (!std::isnan(curv[n - 1]) || !(curv[1000] >= 0))) return fail("the curvature", h, (int)k);
                if ((use & 4) && (!std::isnan(eig[0]) || !(eig[3 * 1000] <= eig[3 * 1000 + 1] && eig[3 * 1000 + 1] <= eig[3 * 1000 + 2])))
                    return fail("the eigenvalues", h, (int)k);
                if (oriented && (use & 1) && !(nrm[3 * 1000 + 2] >= 0 || nrm[3 * 1000] != 0 || nrm[3 * 1000 + 1] != 0)) return fail("the orientation", h, (int)k);
            }
    {  // fewer than k other points: everything NaN
        std::vector<float> nrm(3 * 5);
        std::vector<double> curv(5), eig(3 * 5);
        erasor_normals_result r;
        rc = erasor_hip_normals_clouds(h, c.data() + 4, 5, 0, 32, nullptr, nrm.data(), curv.data(), eig.data(), &r);
        if (rc) return fail("the short cloud", h, rc);
        if (r.n_short != 5 || r.n_degenerate != 0 || r.curvature.n_scored != 0 || !std::isnan(nrm[14]) || !std::isnan(curv[4]) || !std::isnan(eig[14]) ||
            !std::isnan(r.curvature.median))
            return fail("the short cloud's result", h, 0);
    }
    {  // no points at all
        erasor_normals_result r;
        rc = erasor_hip_normals_clouds(h, nullptr, 0, 0, 8, view, nullptr, nullptr, nullptr, &r);
        if (rc || r.n_points != 0 || r.n_short != 0 || !std::isnan(r.curvature.max)) return fail("the empty cloud", h, rc);
    }
    erasor_hip_destroy(h);
    printf("ALL OK\n");
    return 0;
}
