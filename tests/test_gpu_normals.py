"""Surface normals, curvature and covariance eigenvalues on the device (erasor_hip_normals_*, kernel in normals.hip.h) against their host
restatement evalmap.normals, byte for byte (NaNs as bit patterns), and against the pure-Python normals_brute where n <= 300.  Known
answers on lattices in the axis planes, a tilted plane against its analytic normal (near the origin and 10 and 100 km out), ties at
the k-th place in every index permutation and one float32 step beside it, every list class at every size around the leaf, wavefront,
workgroup and tree padding, short clouds, degenerate, collinear and signed-zero neighbourhoods, both orientation rules, every
combination of outputs with guard words, the refusals, the synthetic world, a 200 000-point cloud, and the handle's map with a step
after it.  tests/test_normals_on_cpu.py re-runs this file against the CPU stand-in."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import erasor_amd
import scenarios
from erasor_amd import evalmap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_CPU = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))
E_INVALID, E_STATE = -1, -4
RESULT_KEYS = evalmap.NORMALS_RESULT_FIELDS + ("k", "curvature_stats")


@pytest.fixture(scope="module")
def gpu_mod():
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def same_numbers(a, b):
    """two dicts of ints and floats with the same keys and values, NaN equal to NaN"""
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or
                                        (type(a[k]) is type(b[k]) and a[k] == b[k]) for k in a)


def assert_same_normals(got, want, what):
    """(normals, curvature, eigenvalues, result) twice: the same bytes and the same numbers"""
    assert tuple(got[3].keys()) == RESULT_KEYS and tuple(want[3].keys()) == RESULT_KEYS, (what, got[3].keys())
    for key in RESULT_KEYS[:-1]:
        assert got[3][key] == want[3][key], (what, key, got[3], want[3])
    assert same_numbers(got[3]["curvature_stats"], want[3]["curvature_stats"]), (what, got[3], want[3])
    for j, (name, dt, bits) in enumerate((("normals", np.float32, np.uint32), ("curvature", np.float64, np.uint64), ("eigenvalues", np.float64, np.uint64))):
        g, w = got[j], want[j]
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((np.ascontiguousarray(g).view(bits) != np.ascontiguousarray(w).view(bits)).reshape(len(g), -1).any(1))
            assert False, (what, name, len(bad), bad[:5], g[bad[:2]], w[bad[:2]])


def check(g, cloud, k, viewpoint=None, what=""):
    """the device against the host restatement (and the pure-Python one on a small cloud); what the host restatement returned"""
    want = evalmap.normals(cloud, k, viewpoint)
    assert_same_normals(g.normals(cloud, k, viewpoint, eigenvalues=True), want, (what, k, viewpoint))
    if len(cloud) <= 300:
        assert_same_normals(evalmap.normals_brute(cloud, k, viewpoint), want, (what, k, viewpoint, "the pure-Python restatement"))
    return want


def all_nan(a):
    return np.isnan(a).all()


# ---- 1. known answers that do not depend on the restatement ----
def axis_lattice(axis, rows=5, cols=4, const=1.7, spacing=0.2):
    """rows x cols points, `spacing` apart, in the plane where coordinate `axis` is the float32 `const`"""
    u, v = np.meshgrid(np.arange(rows) * spacing, np.arange(cols) * spacing, indexing="ij")
    xyz = np.zeros((rows * cols, 3), np.float32)
    xyz[:, (axis + 1) % 3], xyz[:, (axis + 2) % 3], xyz[:, axis] = u.ravel() - 0.3, v.ravel() + 2.1, np.float32(const)
    return xyz


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_lattice_in_an_axis_plane_has_the_axis_as_its_normal_exactly(handle, axis):
    """the constant coordinate c is a float32, so the sums 1 c, 2 c, ... m c are exact in float64 (m <= 33 adds six bits to c's 24) and
    so is (m c) / m: the centred coordinate is exactly 0, the three covariance entries with it are exactly 0, the two pivots touching
    that axis are skipped, its column of V stays the unit vector and its eigenvalue is exactly 0"""
    for rows, cols, k in ((3, 3, 8), (5, 4, 8), (6, 7, 16), (7, 7, 32)):
        xyz = axis_lattice(axis, rows, cols)
        c, m = np.float64(xyz[0, axis]), k + 1
        s = np.float64(0.0)
        for _ in range(m):
            s = s + c
        assert s / np.float64(m) == c and c != 1.7  # (checked here, on the host: exact for the float32 nearest 1.7)
        nrm, curv, eig, res = check(handle, xyzi(xyz), k, what=("lattice", axis, rows, cols))
        e = np.zeros(3, np.float32)
        e[axis] = 1.0
        assert (nrm == e).all() and not np.signbit(nrm).any(), nrm[:3]
        assert (curv == 0.0).all() and (eig[:, 0] == 0.0).all() and (eig[:, 1] > 0).all()
        assert res["n_ambiguous"] == 0 and res["n_flipped"] == 0 and res["n_short"] == 0 and res["n_degenerate"] == 0
        assert res["curvature_stats"] == {"n_scored": rows * cols, "min": 0.0, "median": 0.0, "p90": 0.0, "p99": 0.0, "max": 0.0}


# ---- 2. a tilted plane, near the origin and far from it ----
PLANE_A, PLANE_B = 0.3, -0.45
STEP_AT_10M = float(np.spacing(np.float32(10.0)))  # 9.5e-7 m


def tilted_plane(n, seed, shift=0.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-10, 10, (n, 2))
    z = PLANE_A * xy[:, 0] + PLANE_B * xy[:, 1]
    return xyzi(np.stack([xy[:, 0], xy[:, 1], z], 1) + shift)


def angles_to_the_plane_normal(nrm):
    a = np.array([-PLANE_A, -PLANE_B, 1.0])
    a /= np.linalg.norm(a)
    n = nrm.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(n, a), axis=1), np.abs(n @ a))


def check_plane(handle, cloud, bound, what):
    k = 16
    extent = evalmap.knn(cloud, k)["kth"]
    assert extent.min() >= 0.1, extent.min()  # the bound below is the coordinates' step over this extent
    nrm, curv, eig, res = check(handle, cloud, k, what=what)
    ang = angles_to_the_plane_normal(nrm)
    assert ang.max() <= bound, (what, ang.max(), bound)
    assert res["n_short"] == res["n_degenerate"] == 0 and (nrm[:, 2] > 0).all() and res["curvature_stats"]["n_scored"] == len(cloud)
    return nrm


def test_a_tilted_plane_against_its_analytic_normal(handle):
    """z = a x + b y on random xy within +-10 m, stored as float32: every coordinate is off the plane by at most float32's step at 10 m,
    about 1e-6 m, and the neighbourhood's extent is >= 0.1 m (asserted), so the fitted normal is within 1e-6 / 0.1 = 1e-5 rad"""
    check_plane(handle, tilted_plane(1500, 1), 1e-5, "tilted plane")


@pytest.mark.parametrize("shift", [1e4, 1e5])
def test_the_tilted_plane_far_from_the_origin(handle, shift):
    """the same plane shifted on each axis: the bytes still agree, and the analytic bound grows with float32's step out there"""
    cloud = tilted_plane(1500, 2, shift)
    step = float(np.spacing(np.float32(shift + 16.0)))
    assert step > 500 * STEP_AT_10M
    check_plane(handle, cloud, 1e-5 * step / STEP_AT_10M, ("tilted plane at", shift))


# ---- 3. ties at the k-th place ----
AXES = np.float64([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
PERMS = list(itertools.permutations(range(6)))


def tie_groups(mode):
    """720 groups of seven points, 16 m apart on a grid of whole metres: a centre and, behind it in the index order, the six points 1 m
    from it along the axes, in every permutation.  mode "nearer": the group's last point is one float32 step nearer to the centre;
    "farther": the group's first axis point is one step farther away"""
    xyz = np.zeros((len(PERMS), 7, 3), np.float32)
    for g, perm in enumerate(PERMS):
        centre = np.float32([16.0 * (g % 27), 16.0 * (g // 27), 32.0])
        xyz[g, 0] = centre
        pts = (centre + AXES[list(perm)]).astype(np.float32)
        slot = {"same": None, "nearer": 5, "farther": 0}[mode]
        if slot is not None:
            ax = int(np.flatnonzero(AXES[perm[slot]])[0])
            outward = np.float32(np.inf) * np.float32(AXES[perm[slot]][ax])
            pts[slot, ax] = np.nextafter(pts[slot, ax], centre[ax] if mode == "nearer" else outward)
        xyz[g, 1:] = pts
    return xyz


@pytest.mark.parametrize("mode", ["same", "nearer", "farther"])
def test_six_neighbours_at_one_distance_with_k_3_in_every_index_permutation(handle, mode):
    """k = 3 of six candidates at one distance: the index decides which three enter the neighbourhood, and with them the normal.  One
    float32 step nearer, the last candidate is always in, and first; one step farther, the first candidate is always out."""
    groups = tie_groups(mode)
    cloud = xyzi(groups.reshape(-1, 3))
    want = evalmap.normals(cloud, 3)
    nbr = evalmap.knn(cloud, 3, True)["nbr_idx"][0::7].astype(np.int64) - 7 * np.arange(len(PERMS))[:, None]
    assert (nbr == {"same": [1, 2, 3], "nearer": [6, 1, 2], "farther": [2, 3, 4]}[mode]).all(), nbr[:3]
    assert_same_normals(handle.normals(cloud, 3, eigenvalues=True), want, ("ties", mode))
    # each group on its own, in pure Python: its centre's normal is the one the whole cloud gives it
    distinct = set()
    for g in range(len(PERMS)):
        alone = evalmap.normals_brute(xyzi(groups[g]), 3)
        assert alone[0][0].tobytes() == want[0][7 * g].tobytes() and alone[1][0].tobytes() == want[1][7 * g].tobytes(), (mode, g)
        distinct.add(want[0][7 * g].tobytes())
    assert len(distinct) >= 4  # (the membership shows in the normal: the case tells the permutations apart)


# ---- 4. list classes and sizes ----
def blob(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-4, 4, (n, 3)) * [1, 1, 0.2]
    xyz[::9] = np.round(xyz[::9])  # lattice points among them: ties and duplicates
    return xyzi(xyz, rng.integers(240, 270, n))


@pytest.mark.parametrize("k", [2, 8, 9, 16, 17, 32])
def test_every_list_class_at_sizes_around_the_leaf_the_wavefront_the_workgroup_and_the_tree_padding(handle, k):
    sizes = sorted({1, 2, 3, k, k + 1, k + 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257})
    for n in sizes:
        nrm, curv, eig, res = check(handle, blob(n, 100 * k + n), k, what=("size", n))
        if n - 1 < k:
            assert res["n_short"] == n and all_nan(nrm) and all_nan(curv) and all_nan(eig) and res["curvature_stats"]["n_scored"] == 0
        else:
            assert res["n_short"] == 0 and res["curvature_stats"]["n_scored"] + res["n_degenerate"] == n


# ---- 5. degenerate and ambiguous neighbourhoods ----
def test_300_copies_of_one_point_are_all_degenerate(handle):
    nrm, curv, eig, res = check(handle, xyzi(np.tile([[1.5, -2.25, 0.125]], (300, 1))), 8, what="copies")
    assert res["n_degenerate"] == 300 and res["n_short"] == 0 and all_nan(nrm) and all_nan(curv) and all_nan(eig)
    assert res["curvature_stats"]["n_scored"] == 0 and math.isnan(res["curvature_stats"]["max"])


def test_copies_of_one_point_inside_a_lattice(handle):
    g = np.stack(np.meshgrid(*[np.arange(6) * 0.5] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([g, np.tile(g[100:101], (300, 1))])
    perm = np.random.default_rng(6).permutation(len(xyz))
    nrm, curv, eig, res = check(handle, xyzi(xyz[perm]), 8, what="copies in a lattice")
    copies = (xyz[perm] == g[100]).all(1)
    assert copies.sum() == 301 and res["n_degenerate"] == 301 and np.isnan(curv[copies]).all() and np.isfinite(curv[~copies]).all()
    assert res["curvature_stats"]["n_scored"] == len(xyz) - 301


def test_an_exactly_collinear_row_is_counted_as_ambiguous(handle):
    """forty points a quarter metre apart on a line along x: only cxx is not zero, so the two smallest eigenvalues are both exactly 0, the
    order (value, column) picks column 1 and the normal is (0, 1, 0) -- defined, arbitrary, and counted"""
    xyz = np.zeros((40, 3))
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = np.arange(40) * 0.25 - 3.0, 1.5, -2.0
    for k in (2, 8, 32):
        nrm, curv, eig, res = check(handle, xyzi(xyz), k, what="collinear")
        assert res["n_ambiguous"] == 40 and res["n_degenerate"] == 0 and (nrm == np.float32([0, 1, 0])).all() and (curv == 0).all()
        assert (eig[:, :2] == 0).all() and (eig[:, 2] > 0).all()


def test_coplanar_points_with_negative_zero_coordinates(handle):
    xyz = axis_lattice(2, 6, 6, const=0.0)
    xyz[::2, 2] = -0.0
    xyz[:, 0] -= xyz[7, 0]
    xyz[7::5, 0] *= np.float32(-1.0)
    assert np.signbit(xyz[:, 2]).sum() == 18 and (xyz[:, 2] == 0).all() and np.signbit(xyz[xyz[:, 0] == 0, 0]).any()
    for vp in (None, (0.3, -0.2, 5.0), (0.3, -0.2, -5.0)):
        nrm, curv, eig, res = check(handle, xyzi(xyz), 8, vp, what="signed zeros")
        assert (np.abs(nrm) == np.float32([0, 0, 1])).all() and (curv == 0).all() and res["n_flipped"] == (36 if vp and vp[2] < 0 else 0)


# ---- 6. orientation ----
def test_a_viewpoint_on_either_side_of_a_plane_flips_every_normal_and_only_its_sign(handle):
    lattice = xyzi(axis_lattice(2, 6, 6))
    above, below = check(handle, lattice, 8, (0.5, 2.5, 9.0), "above"), check(handle, lattice, 8, (0.5, 2.5, -9.0), "below")
    assert above[3]["n_flipped"] == 0 and below[3]["n_flipped"] == 36 and (below[0] == -above[0]).all() and (above[0][:, 2] == 1).all()
    assert above[1].tobytes() == below[1].tobytes() and above[2].tobytes() == below[2].tobytes()
    # a tilted plane: each normal is turned by exactly one of the two viewpoints
    cloud = tilted_plane(600, 3)
    up, down = check(handle, cloud, 16, (0.0, 0.0, 50.0), "above"), check(handle, cloud, 16, (0.0, 0.0, -50.0), "below")
    assert up[3]["n_flipped"] + down[3]["n_flipped"] == 600 and (up[0] == -down[0]).all() and (up[0][:, 2] > 0).all()
    assert (np.signbit(up[0]) != np.signbit(down[0])).all() and up[1].tobytes() == down[1].tobytes()


def test_a_viewpoint_in_the_plane_flips_nothing(handle):
    xyz = axis_lattice(2, 6, 6)
    vp = (0.123, 2.2, float(xyz[0, 2]))  # vz - pz == 0 and nx == ny == 0: s == 0 exactly
    nrm, curv, eig, res = check(handle, xyzi(xyz), 8, vp, "in the plane")
    assert res["n_flipped"] == 0 and (nrm == np.float32([0, 0, 1])).all()


def test_the_up_rule_on_horizontal_normals(handle):
    """nine points (n = k + 1: one neighbourhood) in a vertical plane through a diagonal of the xy axes, on multiples of a quarter, so
    every sum is exact: cxy == +-cxx, one rotation by exactly 45 degrees, nz == 0 exactly.  Along x == y the solve's normal is
    (c, -s, 0): ny < 0, turned; along x == -y it is (s, c, 0): kept.  In the plane x = const it is (1, 0, 0): nz == ny == 0, kept."""
    i, j = (v.ravel() for v in np.meshgrid(np.arange(-1, 2) * 0.25, np.arange(-1, 2) * 0.25, indexing="ij"))
    for sign, flipped in ((1.0, 9), (-1.0, 0)):
        xyz = np.stack([i + 2.0, sign * i - 1.0, j + 0.5], 1)
        nrm, curv, eig, res = check(handle, xyzi(xyz), 8, what=("diagonal", sign))
        assert res["n_flipped"] == flipped and (nrm[:, 2] == 0).all() and (nrm[:, 1] > 0).all()
        assert (np.signbit(nrm[:, 2]) == bool(flipped)).all()  # (all three components are negated: a turned 0.0 is -0.0)
        assert (nrm[:, 0] == -sign * nrm[:, 1]).all() and (curv == 0).all() and len({r.tobytes() for r in nrm}) == 1
    nrm, curv, eig, res = check(handle, xyzi(axis_lattice(0, 3, 3)), 8, what="x = const")
    assert res["n_flipped"] == 0 and (nrm == np.float32([1, 0, 0])).all() and not np.signbit(nrm).any()


# ---- 7. buffers ----
def test_every_combination_of_outputs_and_the_words_behind_them(handle, gpu_mod):
    cloud = blob(257, 5)
    n, k = len(cloud), 9
    want = evalmap.normals(cloud, k, (1.0, 2.0, 3.0))
    L, vp = gpu_mod.lib(), (C.c_double * 3)(1.0, 2.0, 3.0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for use in itertools.product((False, True), repeat=3):
        nrm, curv, eig = np.full(3 * n + 4, 7.0, np.float32), np.full(n + 4, 7.0), np.full(3 * n + 4, 7.0)
        bufs = [b if u else None for b, u in zip((nrm, curv, eig), use)]
        res = gpu_mod.NormalsResult()
        res.n_points = 12345
        rc = L.erasor_hip_normals_clouds(handle._h, p(cloud), C.c_size_t(n), C.c_int(0), C.c_uint32(k), vp, p(bufs[0]), p(bufs[1]), p(bufs[2]), C.byref(res))
        assert rc == 0, (use, L.erasor_hip_last_error(handle._h))
        for j, (b, u, m) in enumerate(zip((nrm, curv, eig), use, (3 * n, n, 3 * n))):
            assert (b[m:] == 7.0).all(), (use, j)  # the guard words
            assert b[:m].tobytes() == want[j].tobytes() if u else (b[:m] == 7.0).all(), (use, j)
        assert [getattr(res, f) for f in evalmap.NORMALS_RESULT_FIELDS] == [want[3][f] for f in evalmap.NORMALS_RESULT_FIELDS]
        assert same_numbers(res.curvature.as_dict(), want[3]["curvature_stats"])


# ---- 8. refusals and the struct's layout ----
def test_refusals_each_with_its_code_and_its_sentence(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    cloud = blob(200, 4)
    L, p, n = gpu_mod.lib(), cloud.ctypes.data_as(C.c_void_p), C.c_size_t(len(cloud))
    err = lambda: L.erasor_hip_last_error(g._h).decode()
    res = gpu_mod.NormalsResult()

    def clouds(k, vp=None, r=res, ptr=p, count=n):
        v = None if vp is None else (C.c_double * 3)(*vp)
        return L.erasor_hip_normals_clouds(g._h, ptr, count, C.c_int(0), C.c_uint32(k), v, None, None, None, None if r is None else C.byref(r))

    for k in (0, 1, 33):
        assert clouds(k) == E_INVALID and err() == "erasor_hip_normals_clouds: k must be within 2 .. 32"
        assert L.erasor_hip_normals_map(g._h, C.c_uint32(k), None, None, None, None, C.byref(res)) == E_INVALID
        assert err() == "erasor_hip_normals_map: k must be within 2 .. 32"
    assert clouds(8, r=None) == E_INVALID and err() == "erasor_hip_normals_clouds: res is NULL"
    assert L.erasor_hip_normals_map(g._h, C.c_uint32(8), None, None, None, None, None) == E_INVALID and err() == "erasor_hip_normals_map: res is NULL"
    for bad in (float("nan"), float("inf"), float("-inf")):
        for at in range(3):
            vp = [1.0, 2.0, 3.0]
            vp[at] = bad
            assert clouds(8, vp) == E_INVALID and err() == "erasor_hip_normals_clouds: viewpoint must be three finite numbers"
            with pytest.raises(gpu_mod.ErasorError) as e:
                g.normals(cloud, 8, vp)
            assert e.value.rc == E_INVALID
            with pytest.raises(ValueError):
                evalmap.normals(cloud, 8, vp)
    for bad in (np.nan, np.inf):
        c = cloud.copy()
        c[5, 1] = bad
        assert clouds(8, ptr=c.ctypes.data_as(C.c_void_p)) == E_INVALID
        assert err() == "erasor_hip_normals_clouds: non-finite coordinate (NaN / Inf) in 1 point(s)"
    for count, ptr in ((C.c_size_t(2 ** 30 + 1), p), (C.c_size_t(3), None)):
        assert clouds(8, ptr=ptr, count=count) == E_INVALID and err() == "erasor_hip_normals_clouds: NULL cloud or more than 2^30 points"
    for k in (1, 33):
        with pytest.raises(ValueError):
            evalmap.normals(cloud, k)
    # the handle's map: none yet
    assert L.erasor_hip_normals_map(g._h, C.c_uint32(8), None, None, None, None, C.byref(res)) == E_STATE and "no map" in err()
    # n == 0: all zero, statistics NaN, status OK
    empty = np.zeros((0, 4), np.float32)
    got, want = g.normals(empty, 5, eigenvalues=True), evalmap.normals(empty, 5)
    assert_same_normals(got, want, "empty")
    assert got[3]["n_points"] == 0 and got[3]["curvature_stats"]["n_scored"] == 0 and math.isnan(got[3]["curvature_stats"]["min"])
    assert g.normals(cloud, 8)[2] is None and g.normals(cloud, 8)[3]["n_short"] == 0  # the handle is fine after the refusals
    # the header's layout
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(erasor_normals_result), '
            'offsetof(erasor_normals_result, n_flipped), offsetof(erasor_normals_result, curvature));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    R = gpu_mod.NormalsResult
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [C.sizeof(R), R.n_flipped.offset, R.curvature.offset] == [88, 32, 40]


# ---- 9. worlds ----
def test_the_synthetic_world_with_and_without_a_viewpoint(handle):
    sc = scenarios.small(n_frames=3, az=60) if ON_CPU else scenarios.small()
    m = np.ascontiguousarray(sc["map"], np.float32)
    cloud = np.ascontiguousarray(m[:: max(1, len(m) // (2500 if ON_CPU else 20000))])
    assert len(cloud) > (1000 if ON_CPU else 15000)
    up = check(handle, cloud, 16, what="world")
    seen = check(handle, cloud, 16, (float(m[:, 0].mean()), float(m[:, 1].mean()), 2.0), "world, a viewpoint")
    assert up[3]["n_short"] == 0 and up[3]["curvature_stats"]["n_scored"] > 0.9 * len(cloud) and (up[0][np.isfinite(up[1]), 2] >= 0).all()
    assert 0 < seen[3]["n_flipped"] < len(cloud) and up[1].tobytes() == seen[1].tobytes()
    # the ground is flat: most normals point up
    assert (up[0][:, 2] > 0.9).mean() > 0.3
    # the same from a device buffer
    p = handle.device_array(cloud)
    try:
        assert_same_normals(handle.normals((p, len(cloud)), 16, eigenvalues=True), up, "device cloud")
    finally:
        handle.device_free(p)


def test_random_world_of_200000_points_at_k_8(handle):
    rng = np.random.default_rng(11)
    cloud = xyzi(rng.uniform(0, 41.0, (200000, 3)), rng.integers(0, 300, 200000))
    cloud[::1000, :3] = cloud[0, :3]  # 200 copies of one point among them
    want = check(handle, cloud, 8, what="random world")
    assert want[3]["n_degenerate"] == 200 and want[3]["curvature_stats"]["n_scored"] == 199800


def test_the_map_call_a_step_and_the_map_call_again(gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, plain = (gpu_mod.Erasor(scenarios.to_product_params(sc["params"])) for _ in range(2))
    for e in (g, plain):
        e.set_map(sc["map"])
        for f in range(n - 1):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    k = 4 if ON_CPU else 8
    for f in (n - 1, n):
        m = np.ascontiguousarray(g.get_map(), np.float32)
        assert_same_normals(g.normals_map(k, eigenvalues=True), evalmap.normals(m, k), ("normals_map before step", f))
        assert_same_normals(g.normals_map(k, (0.0, 0.0, 1.0), eigenvalues=True), evalmap.normals(m, k, (0.0, 0.0, 1.0)), ("normals_map, a viewpoint", f))
        assert g.get_map().tobytes() == m.tobytes()  # the map itself stays as it is
        # the step after the call is the uninterrupted run's
        a = g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        b = plain.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        assert a.as_dict() == b.as_dict() and g.get_map().tobytes() == plain.get_map().tobytes()
    m = np.ascontiguousarray(g.get_map(), np.float32)
    assert_same_normals(g.normals_map(k, eigenvalues=True), evalmap.normals(m, k), "normals_map after the steps")
