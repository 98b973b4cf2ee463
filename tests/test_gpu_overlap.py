"""The estimate-to-ground-truth overlap report on the device (erasor_hip_overlap_clouds / erasor_hip_overlap_map, kernels in
nearest.hip.h) against the reference's overlap_report (scripts/analysis_runner.py:53-71): its golden numbers and text, per-point
distances against scipy's cKDTree and nearest indices against brute force, the handle's map after real steps, steps after the report,
errors, the offline driver's --analyze mode, and the bench's full-size map.  tests/test_overlap_on_cpu.py re-runs part of this file
against the CPU stand-in."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
from scipy.spatial import cKDTree

import scenarios
from erasor_amd import evalmap, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("n_est", "n_below_half", "n_below_one", "n_below_two", "median", "p90", "p99", "max", "frac_half", "frac_one", "frac_two")


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "overlap_golden.npz"))
    fields = [str(f) for f in z["fields"]]
    return [(str(z["name%d" % k]), z["gt%d" % k], z["est%d" % k], float(z["vs%d" % k]), dict(zip(fields, z["res%d" % k].tolist())),
             str(z["text%d" % k])) for k in range(int(z["n_cases"]))]


def assert_same_bits(r, ref, what=""):
    for k in FIELDS:
        a, b = np.float64(r[k]), np.float64(ref[k])
        assert a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b)), (what, k, r[k], ref[k])


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.full((len(xyz), 1), w, np.float32)], 1)


def sphere_lattice(n2):
    """every integer point at squared distance n2 from the origin: all of them tie for a query at the centre"""
    r = int(np.ceil(np.sqrt(n2)))
    g = np.arange(-r, r + 1)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    m = x * x + y * y + z * z == n2
    return np.stack([x[m], y[m], z[m]], 1).astype(np.float64)


def per_point_cases():
    rng = np.random.default_rng(11)
    cases = {name: (gt, est) for name, gt, est, _, _, _ in golden()}
    line = np.zeros((1500, 3), np.float32)
    line[:, 0] = rng.uniform(-50, 50, 1500).astype(np.float32)
    cases["gt_on_a_line"] = (xyzi(line), xyzi(rng.uniform(-60, 60, (900, 3))))
    cases["single_gt_point"] = (xyzi([[1.5, -2.0, 0.25]]), xyzi(rng.uniform(-100, 100, (700, 3))))
    s = sphere_lattice(2 * 3 * 5 * 7 * 11)  # (2310: a few hundred lattice points, a dozen leaves)
    s = s[rng.permutation(len(s))] * 0.25 + np.array([100.0, -50.0, 2.0])
    centre = np.array([[100.0, -50.0, 2.0]] * 3 + [[100.25, -50.0, 2.0]])
    cases["sphere_centre_ties"] = (xyzi(s), xyzi(np.concatenate([centre, rng.uniform(80, 120, (200, 3))])))
    return cases


CASES = per_point_cases()


def brute_force(gt, est):
    """(d, smallest GT index at the minimum d^2), d^2 in float64 as cKDTree and the device form it"""
    g = gt[:, :3].astype(np.float64)
    e = est[:, :3].astype(np.float64)
    ex = e[:, None, 0] - g[None, :, 0]
    ey = e[:, None, 1] - g[None, :, 1]
    ez = e[:, None, 2] - g[None, :, 2]
    d2 = (ex * ex + ey * ey) + ez * ez
    m = d2.min(1)
    return np.sqrt(m), np.argmax(d2 == m[:, None], 1).astype(np.uint32)


# ---- 1. golden: the reference's own overlap_report (tests/golden/overlap_golden.npz, make_overlap_golden.py) ----
@pytest.mark.parametrize("device_inputs", [False, True])
def test_golden_numbers_of_the_reference_report(handle, device_inputs):
    for name, gt, est, vs, ref, text in golden():
        if device_inputs:
            pg, pe = handle.device_array(gt), handle.device_array(est)
            try:
                r = handle.overlap((pg, len(gt)), (pe, len(est)), vs)
            finally:
                handle.device_free(pg)
                handle.device_free(pe)
        else:
            r = handle.overlap(gt, est, vs)
        assert_same_bits(r, ref, name)
        assert "\n".join(evalmap.overlap_lines(r, vs)) + "\n" == text, name


# ---- 2. per point: distances against cKDTree, nearest indices against brute force ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_per_point_distances_match_ckdtree(handle, name):
    gt, est = CASES[name]
    r = handle.overlap(gt, est, 0.2, per_point=True)
    d, _ = cKDTree(gt[:, :3].astype(np.float64)).query(est[:, :3].astype(np.float64), k=1)
    same = r["dist"].view(np.uint64) == d.view(np.uint64)
    assert same.all(), "%s: %d of %d distances differ (first at %s: %r vs %r)" % (
        name, (~same).sum(), len(d), np.argwhere(~same)[:3].ravel().tolist(), r["dist"][~same][:3], d[~same][:3])
    assert_same_bits(r, evalmap.overlap(gt[:, :3], est[:, :3], 0.2), name)
    if len(gt) <= 5000 and len(est) <= 2000:
        bd, bi = brute_force(gt, est)
        assert (r["dist"].view(np.uint64) == bd.view(np.uint64)).all(), name
        assert (r["nearest"] == bi).all(), (name, np.argwhere(r["nearest"] != bi)[:5].ravel())
    if name == "sphere_centre_ties":
        assert (r["nearest"][:3] == 0).all() and r["dist"][0] == np.sqrt(2310 * 0.0625)


def test_per_point_nearest_breaks_ties_towards_the_smaller_index(handle):
    gt = xyzi([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [5, 5, 5], [-1, 0, 0], [0, 0, 0.5]])
    est = xyzi([[0, 0, 0], [0, 0, 0.5], [-1, 0, 0], [3, 3, 3]])
    r = handle.overlap(gt, est, 0.2, per_point=True)
    assert r["nearest"].tolist() == [5, 5, 1, 3]
    assert r["dist"].tolist() == [0.5, 0.0, 0.0, float(np.sqrt(12.0))]


# ---- 3. voxel_leaf: the host voxelisation followed by evalmap.overlap ----
def test_voxel_leaf_matches_host_voxelisation(handle):
    name, gt, est, vs, _, _ = golden()[0]  # (not the outliers' case: a grid that wide overflows PCL's indices, a pass-through)
    for leaf in (1.0, 2.5):  # (the fixture's points are ~0.5 m apart: leaves that merge some of them)
        r = handle.overlap(gt, est, vs, voxel_leaf=leaf)
        vg, ve = handle.voxelize_preserving_labels(gt, leaf), handle.voxelize_preserving_labels(est, leaf)
        assert r["n_est"] == len(ve) < len(est)
        assert_same_bits(r, evalmap.overlap(vg[:, :3], ve[:, :3], vs), leaf)


# ---- 4. the handle's map ----
@pytest.mark.parametrize("large_scale", [False, True])
def test_overlap_map_after_steps(gpu_mod, large_scale):
    import copy
    sc = scenarios.small()
    p = copy.copy(sc["params"])
    if large_scale:
        p.is_large_scale, p.submap_size = 1, 25.0
    g = gpu_mod.Erasor(scenarios.to_product_params(p))
    g.set_map(sc["map"])
    for f in range(12):
        g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    m = g.get_map()
    r = g.overlap_map(sc["map"], 0.2)
    assert r["n_est"] == len(m)
    assert_same_bits(r, evalmap.overlap(sc["map"][:, :3], m[:, :3], 0.2))
    rv = g.overlap_map(sc["map"], 0.2, voxel_leaf=0.2)
    vg, vm = g.voxelize_preserving_labels(sc["map"], 0.2), g.voxelize_preserving_labels(m, 0.2)
    assert_same_bits(rv, evalmap.overlap(vg[:, :3], vm[:, :3], 0.2))


# ---- 5. no interference with later steps ----
def test_overlap_between_steps_leaves_later_steps_bit_identical(gpu_mod):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import orc
    from test_gpu_parity import compare_step
    sc = scenarios.small()
    g, o = gpu_mod.Erasor(scenarios.to_product_params(sc["params"])), orc.Oracle(sc["params"])
    g.set_map(sc["map"])
    o.set_map(sc["map"])
    n, ahead = 8, 2
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"][:n]]
    Tb, To = sc["T_b2o"], sc["T_o2b"]
    for j in range(ahead):
        g.prefetch(scans[j], sc["T_l2b"], Tb[j], To[j])
    gt = sc["map"][::2].copy()
    for k in range(n):
        if k + ahead < n:
            g.prefetch(scans[k + ahead], sc["T_l2b"], Tb[k + ahead], To[k + ahead])
        rg = g.step(scans[k], sc["T_l2b"], Tb[k], To[k])
        ro = o.step(scans[k], sc["T_l2b"], Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
        # between steps, nodes announced ahead: the report in the evaluator's scratch, its tree sort in a radix bank of its own
        assert_same_bits(g.overlap_map(gt, 0.2), evalmap.overlap(gt[:, :3], o.get_map()[:, :3], 0.2))
        g.overlap(gt, scans[k], 0.2, per_point=True)
        g.evaluate_map(gt, 0.2)
        if k % 3 == 1:
            g.overlap_map(gt, 0.2, voxel_leaf=0.2)
    assert g.get_map().shape == o.get_map().shape


# ---- 6. errors and the struct layout ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    E_INVALID, E_STATE = -1, -4
    g = gpu_mod.Erasor(gpu_mod.params_default())
    a = xyzi(np.random.default_rng(1).uniform(-3, 3, (100, 3)))
    for vs in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.overlap(a, a, vs)
        assert e.value.rc == E_INVALID
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.overlap(a, a, 0.2, voxel_leaf=0.2, per_point=True)
    assert e.value.rc == E_INVALID and "per-point" in str(e.value)
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.overlap(np.zeros((0, 4), np.float32), a, 0.2)
    assert e.value.rc == E_INVALID and "empty ground truth" in str(e.value)
    bad = a.copy()
    bad[7, 1] = np.nan
    for gt, est in ((bad, a), (a, bad)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.overlap(gt, est, 0.2)
        assert e.value.rc == E_INVALID and "non-finite" in str(e.value)
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.overlap(gt, est, 0.2, voxel_leaf=0.2)
        assert e.value.rc == E_INVALID
    pb = g.device_array(bad)
    try:
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.overlap((pb, len(bad)), a, 0.2)
        assert e.value.rc == E_INVALID
    finally:
        g.device_free(pb)
    r = g.overlap(a, np.zeros((0, 4), np.float32), 0.2)
    assert r["n_est"] == 0 and r["n_below_two"] == 0 and all(np.isnan(r[k]) for k in FIELDS[4:])
    r = g.overlap(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), 0.2)
    assert r["n_est"] == 0 and np.isnan(r["max"])
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.overlap_map(a, 0.2)
    assert e.value.rc == E_STATE  # no map
    r = g.overlap(a, a, 0.2)  # the handle is fine after the refusals
    assert r["n_below_half"] == 100 and r["max"] == 0.0
    # a step in flight: the NOFLY guard
    sc = scenarios.small()
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    for call in (lambda: g.overlap(a, a, 0.2), lambda: g.overlap_map(a, 0.2)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            call()
        assert e.value.rc == E_STATE
    g.step_wait()
    g.overlap_map(a, 0.2)
    # the header's layout
    offs = ", ".join("offsetof(erasor_overlap_result, %s)" % k for k in FIELDS)
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu' + ' %zu' * len(FIELDS) + '\\n", '
            'sizeof(erasor_overlap_result), ' + offs + ');return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = gpu_mod.OverlapResult
    assert got == [C.sizeof(R)] + [getattr(R, k).offset for k in FIELDS]


# ---- the offline driver ----
def test_offline_driver_analyze_mode(gpu_mod, tmp_path):
    shim_dir = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
    shim = C.CDLL(os.path.join(shim_dir, "liberasor_shim.so"))
    shim.erasor_shim_save_pcd.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_int]
    shim.erasor_shim_save_pcd.restype = C.c_int
    demo = os.path.join(shim_dir, "erasor_offline_demo")
    for name, gt, est, vs, _, text in golden():
        gt, est = np.ascontiguousarray(gt), np.ascontiguousarray(est)
        fg, fe = tmp_path / ("%s_gt.pcd" % name), tmp_path / ("%s_est.pcd" % name)
        assert shim.erasor_shim_save_pcd(str(fg).encode(), gt.ctypes.data, len(gt), 1) == 0
        assert shim.erasor_shim_save_pcd(str(fe).encode(), est.ctypes.data, len(est), 1) == 0
        out = subprocess.run([demo, "--analyze", str(fg), str(fe), repr(vs)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        assert lines[0] == "GT : %s" % fg and lines[1] == "Est: %s" % fe, out.stdout
        assert "\n".join(lines[2:4]) + "\n" == text, (name, out.stdout, text)
        assert lines[4].startswith("|   gt_S |") and lines[6].startswith("| "), out.stdout  # the PR / RR row follows
    out = subprocess.run([demo, "--analyze", str(fg), str(fe), "0.2", "0.2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.splitlines()[2].startswith("est->GT dist: median="), out.stdout + out.stderr


# ---- 7. full size: the bench's world ----
@pytest.mark.timeout(900)
def test_full_size_overlap_map_matches_evalmap(gpu_mod):
    w = synth.World(seed=20210305 + 5, length=1000.0, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    lid = synth.Lidar.hdl64(2000)
    m = w.sample_map(spacing=0.2, frames=range(0, 320, 2))
    assert len(m) > 9_000_000
    p = gpu_mod.params_default()
    synth.apply_params(p, "05", max_range=80.0, num_rings=20, num_sectors=108)
    g = gpu_mod.Erasor(p)
    g.set_map(m)
    Tl = gpu_mod.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    jr = np.random.default_rng(7)
    for k in range(3):
        p7 = w.pose(k * 3, 1.0, x0=300.0, jitter_rng=jr)
        Tb = gpu_mod.geopose2eigen(p7)
        g.step(w.cast(p7, lid, k * 3), Tl, Tb, gpu_mod.invert_rigid(Tb))
    est = g.get_map()
    # the ground truth: the map moved rigidly by 0.2 m and 0.5 deg of yaw about its centre, plus far outliers
    rng = np.random.default_rng(3)
    c, s = np.cos(np.radians(0.5)), np.sin(np.radians(0.5))
    ctr = m[:, :3].astype(np.float64).mean(0)
    xyz = m[:, :3].astype(np.float64) - ctr
    gt = m.copy()
    gt[:, 0] = (c * xyz[:, 0] - s * xyz[:, 1] + ctr[0] + 0.2).astype(np.float32)
    gt[:, 1] = (s * xyz[:, 0] + c * xyz[:, 1] + ctr[1]).astype(np.float32)
    far = rng.uniform(-1, 1, (2000, 3)) * np.array([3000.0, 3000.0, 200.0]) + ctr
    gt = np.concatenate([gt, xyzi(far)])
    pg = g.device_array(gt)
    try:
        g.overlap_map((pg, len(gt)), 0.2)  # (first call: allocations)
        t0 = time.perf_counter()
        r = g.overlap_map((pg, len(gt)), 0.2)
        t_dev = time.perf_counter() - t0
    finally:
        g.device_free(pg)
    t0 = time.perf_counter()
    ref = evalmap.overlap(gt[:, :3], est[:, :3], 0.2)
    t_host = time.perf_counter() - t0
    print("\nfull size: %d-pt ground truth, %d-pt map: overlap_map %.1f ms, evalmap.overlap (cKDTree, every core) %.1f ms\n%s" % (
        len(gt), len(est), t_dev * 1e3, t_host * 1e3, "\n".join(evalmap.overlap_lines(r, 0.2))))
    assert_same_bits(r, ref)
    assert r["n_est"] == len(est) and r["median"] > 0.05
