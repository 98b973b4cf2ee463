"""PR / RR of a cleaned map on the device (erasor_hip_evaluate_clouds / erasor_hip_evaluate_map, kernels in evaluate.hip.h) against
the reference's protocol (scripts/analysis_runner.py:74-105): the golden vectors written by the reference's own evaluator, per-point
decisions against scipy's cKDTree, the handle's map after real steps, steps after an evaluation, errors, the offline driver's --eval
mode, and the bench's full-size map.  tests/test_evaluate_on_cpu.py re-runs part of this file against the CPU stand-in."""
import ctypes as C
import os
import re
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
KEYS = ("gt_static", "gt_dynamic", "est_static", "est_dynamic", "preserved_static", "preserved_dynamic", "PR", "RR", "F1")
COUNTS = KEYS[:6]
STATIC, DYNAMIC = 40.0, 252.0


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def assert_same_result(r, ref, tol=0.0):
    for k in COUNTS:
        assert r[k] == ref[k], (k, r[k], ref[k])
    for k in ("PR", "RR", "F1"):
        assert abs(r[k] - ref[k]) <= tol, (k, r[k], ref[k])


def reference_codes(gt, est, voxelsize):
    """the per-ground-truth-point decision of evalmap.evaluate (cKDTree 1-NN), as ERASOR_EVAL_* codes"""
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    est = np.asarray(est, np.float32).reshape(-1, 4)
    if len(est) == 0 or len(gt) == 0:
        return np.zeros(len(gt), np.uint8)
    d, idx = cKDTree(est[:, :3].astype(np.float64)).query(gt[:, :3].astype(np.float64), k=1)
    inside = d < voxelsize * np.sqrt(3) / 2
    g_dyn = np.isin(evalmap.labels(gt[:, 3]), evalmap.DYNAMIC_CLASSES)
    e_dyn = np.isin(evalmap.labels(est[:, 3]), evalmap.DYNAMIC_CLASSES)[np.minimum(idx, len(est) - 1)]
    codes = np.where(g_dyn == e_dyn, np.where(g_dyn, 2, 1), 3).astype(np.uint8)
    codes[~inside] = 0
    return codes


def cloud(xyz, lab):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.broadcast_to(np.asarray(lab, np.float32).reshape(-1, 1), (len(xyz), 1))], 1).astype(np.float32)


def threshold_pairs(rng, n, voxelsize, origin):
    """n ground-truth / estimate pairs, 5 m apart, whose float64 distance (cKDTree's formula) lies a few ulps either side of the
    threshold -- chosen on the host so that its sqrt lands on each side"""
    thr = voxelsize * np.sqrt(3) / 2
    gts, ests = [], []
    for k in range(n):
        g = (np.asarray(origin, np.float64) + np.array([5.0 * k, 0.0, 0.0]) + rng.uniform(-1, 1, 3)).astype(np.float32)
        u = rng.normal(size=3)
        u[0] = np.sign(u[0]) * max(abs(u[0]), 0.5)  # (the walk below moves x)
        u /= np.linalg.norm(u)
        e0 = (g.astype(np.float64) + u * thr).astype(np.float32)
        # walk the estimate's x by float32 ulps until the host decision is on the side we want
        want_inside = k % 2 == 0
        e = e0.copy()
        for _ in range(64):
            dd = g.astype(np.float64) - e.astype(np.float64)
            dist = np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])
            if (dist < thr) == want_inside:
                break
            toward = g[0] if want_inside else (np.float32(2 * e[0] - g[0]))
            e[0] = np.nextafter(e[0], toward, dtype=np.float32)
        dd = g.astype(np.float64) - e.astype(np.float64)
        dist = np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])
        # (a few float32 ulps of the coordinates away from the threshold: the closest the two clouds can come to it)
        assert (dist < thr) == want_inside and abs(dist - thr) <= 8 * float(np.spacing(np.abs(g).max())), (dist, thr)
        gts.append(g)
        ests.append(e)
    return np.array(gts), np.array(ests)


def per_point_cases():
    """seeded fixtures with no opposite-class ties by construction"""
    rng = np.random.default_rng(20261015)
    cases = {}
    # mixed: random clutter, duplicates (same label), exact multiples of the cell edge, negative and +-1e4 m coordinates, and
    # ground-truth / estimate pairs a few ulps either side of the threshold
    n = 4000
    gxyz = rng.uniform(-25, 25, (n, 3)).astype(np.float32)
    gxyz[: n // 8] = (np.round(gxyz[: n // 8] / 0.25) * 0.25).astype(np.float32)          # on multiples of 0.25 (exact in float32)
    gxyz[n // 8: n // 4] = (np.round(gxyz[n // 8: n // 4] / 0.2) * 0.2).astype(np.float32)  # on (rounded) multiples of 0.2
    gxyz[n // 4: n // 4 + 300] += np.float32(1e4)
    gxyz[n // 4 + 300: n // 4 + 600] -= np.float32(1e4)
    glab = np.where(rng.uniform(size=n) < 0.3, rng.choice([252.0, 255.0, 259.0], n), rng.choice([40.0, 50.0, 251.0, 260.0], n)).astype(np.float32)
    glab[:50] += np.float32(65536.0 * 3)  # instance bits above the 16 label bits
    keep = rng.uniform(size=n) < 0.75
    exyz = gxyz[keep] + rng.normal(0, 0.08, (int(keep.sum()), 3)).astype(np.float32)
    exyz[:200] = gxyz[keep][:200]  # some exact hits
    elab = glab[keep].copy()
    flip = rng.uniform(size=len(elab)) < 0.1
    elab[flip] = STATIC
    est = cloud(exyz, elab)
    est = np.concatenate([est, est[:300]])  # duplicate points, same labels
    gt = cloud(gxyz, glab)
    for vs, org in ((0.2, (100.0, 100.0, 0.0)), (0.25, (-9990.0, 40.0, -3.0))):
        tg, te = threshold_pairs(rng, 40, vs, org)
        lab = np.where(np.arange(40) % 4 < 2, STATIC, DYNAMIC)
        cases["mixed_vs%.2f" % vs] = (np.concatenate([gt, cloud(tg, lab)]), np.concatenate([est, cloud(te, lab)]), vs)
    small = cloud(rng.uniform(-5, 5, (700, 3)), rng.choice([STATIC, DYNAMIC], 700))
    near = small.copy()
    near[:, :3] += rng.normal(0, 0.05, (700, 3)).astype(np.float32)
    cases["empty_estimate"] = (small, np.zeros((0, 4), np.float32), 0.2)
    cases["empty_ground_truth"] = (np.zeros((0, 4), np.float32), near, 0.2)
    cases["no_dynamic"] = (cloud(small[:, :3], STATIC), cloud(near[:, :3], STATIC), 0.2)
    cases["all_dynamic"] = (cloud(small[:, :3], 254.0), cloud(near[:, :3], 254.0), 0.2)
    cases["estimate_is_ground_truth"] = (small, small.copy(), 0.2)
    cases["estimate_is_a_subset"] = (small, small[::3].copy(), 0.2)
    return cases


CASES = per_point_cases()


# ---- 1. golden: the reference's own evaluator (tests/golden/eval_golden.npz, make_eval_golden.py) ----
@pytest.mark.parametrize("device_inputs", [False, True])
def test_golden_vectors_of_the_reference_evaluator(handle, device_inputs):
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval_golden.npz"))
    for case in range(4):
        gt, est, res = z["gt%d" % case], z["est%d" % case], z["res%d" % case]
        ref = dict(zip(KEYS, [int(v) for v in res[:6]] + [float(v) for v in res[6:]]))
        if device_inputs:
            pg, pe = handle.device_array(gt), handle.device_array(est)
            try:
                r = handle.evaluate((pg, len(gt)), (pe, len(est)), 0.2)
            finally:
                handle.device_free(pg)
                handle.device_free(pe)
        else:
            r = handle.evaluate(gt, est, 0.2)
        assert_same_result(r, ref, tol=1e-9)
        assert r["n_tied"] == 0 and r["n_label_out_of_range"] == 0


# ---- 2. per point against cKDTree ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_per_point_decisions_match_ckdtree(handle, name):
    gt, est, vs = CASES[name]
    r = handle.evaluate(gt, est, vs, per_point=True)
    codes = reference_codes(gt, est, vs)
    assert r["n_tied"] == 0, "the fixture has no opposite-class ties by construction"
    same = r["per_point"] == codes
    assert same.all(), "%s: %d of %d codes differ (first at %s: %s vs %s)" % (name, (~same).sum(), len(codes), np.argwhere(~same)[:3].ravel().tolist(),
                                                                             r["per_point"][~same][:3], codes[~same][:3])
    g_dyn = np.isin(evalmap.labels(gt[:, 3]), evalmap.DYNAMIC_CLASSES)
    if (~g_dyn).any():
        assert_same_result(r, evalmap.evaluate_clouds(gt, est, vs))
    else:  # (evalmap divides by the static count: without static ground truth PR is 0 here, the rest as evalmap computes it)
        e_dyn = np.isin(evalmap.labels(est[:, 3]), evalmap.DYNAMIC_CLASSES)
        nd, kd = int(g_dyn.sum()), int((codes == 2).sum())
        rr = (nd - kd) / nd * 100.0 if nd else 0.0
        assert_same_result(r, {"gt_static": 0, "gt_dynamic": nd, "est_static": int((~e_dyn).sum()), "est_dynamic": int(e_dyn.sum()),
                               "preserved_static": 0, "preserved_dynamic": kd, "PR": 0.0, "RR": rr, "F1": 0.0})
    if name == "no_dynamic":
        assert r["RR"] == 0.0 and r["gt_dynamic"] == 0
    if name == "estimate_is_ground_truth":
        assert r["preserved_static"] == r["gt_static"] and r["preserved_dynamic"] == r["gt_dynamic"] and r["RR"] == 0.0


def test_threshold_pairs_land_on_both_sides(handle):
    rng = np.random.default_rng(5)
    tg, te = threshold_pairs(rng, 60, 0.2, (0.0, 0.0, 0.0))
    r = handle.evaluate(cloud(tg, STATIC), cloud(te, STATIC), 0.2, per_point=True)
    assert (r["per_point"] == np.where(np.arange(60) % 2 == 0, 1, 0)).all()


def test_device_inputs_and_per_point_codes(handle):
    gt, est, vs = CASES["mixed_vs0.20"]
    pg, pe = handle.device_array(gt), handle.device_array(est)
    try:
        r = handle.evaluate((pg, len(gt)), (pe, len(est)), vs, per_point=True)
        r2 = handle.evaluate((pg, len(gt)), est, vs, voxel_leaf=0.2)
    finally:
        handle.device_free(pg)
        handle.device_free(pe)
    assert (r["per_point"] == reference_codes(gt, est, vs)).all()
    assert_same_result(r2, handle.evaluate(gt, est, vs, voxel_leaf=0.2))


def test_equidistant_points_of_both_classes_are_reported_as_tied(handle):
    gt = cloud([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [20.0, 0.0, 0.0]], [STATIC, DYNAMIC, STATIC])
    est = cloud([[0.05, 0.0, 0.0], [-0.05, 0.0, 0.0], [10.05, 0.0, 0.0], [9.95, 0.0, 0.0], [20.05, 0, 0], [19.95, 0, 0]],
                [STATIC, DYNAMIC, DYNAMIC, STATIC, STATIC, STATIC])
    r = handle.evaluate(gt, est, 0.2, per_point=True)
    assert r["n_tied"] == 2  # the third point's two candidates share a class
    assert r["per_point"][2] == 1
    assert r["per_point"][0] == 1 and r["per_point"][1] == 2  # the smaller estimated index is the answer


def test_labels_out_of_range_are_static_and_counted(handle):
    gt = cloud([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], 0.0)
    gt[:, 3] = [np.nan, np.inf, -1.0, 252.0 + 65536.0]
    est = gt.copy()
    est[:, 3] = [252.0, 252.0, 252.0, 252.0]
    r = handle.evaluate(gt, est, 0.2, per_point=True)
    assert r["n_label_out_of_range"] == 3 and r["gt_static"] == 3 and r["gt_dynamic"] == 1 and r["est_dynamic"] == 4
    assert list(r["per_point"]) == [3, 3, 3, 2]


# ---- 3. the handle's map ----
def _pair(gpu_mod, p):
    from oracle import orc
    return gpu_mod.Erasor(scenarios.to_product_params(p)), orc.Oracle(p)


@pytest.mark.parametrize("large_scale,steps", [(False, 2), (False, 12), (True, 12)])
def test_evaluate_map_follows_the_end_to_end_protocol(gpu_mod, large_scale, steps):
    """test_pr_rr_end_to_end's protocol (save_static_map's voxelisation at 0.2, the labelled initial map as ground truth), with the
    handle's resident map evaluated in place"""
    import copy
    from oracle import orc
    sc = scenarios.small()
    p = copy.copy(sc["params"])
    if large_scale:
        p.is_large_scale, p.submap_size = 1, 25.0
    g = gpu_mod.Erasor(scenarios.to_product_params(p))
    g.set_map(sc["map"])
    for f in range(steps):
        g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    m = g.get_map()
    r = g.evaluate_map(sc["map"], 0.2, voxel_leaf=0.2)
    ref = evalmap.evaluate_clouds(orc.voxelize_preserving_labels(sc["map"], 0.2), orc.voxelize_preserving_labels(m, 0.2), 0.2)
    assert_same_result(r, ref)
    r0 = g.evaluate_map(sc["map"], 0.2)
    assert_same_result(r0, evalmap.evaluate_clouds(sc["map"], m, 0.2))
    if steps == 12:
        assert r["RR"] > 50.0 and r["PR"] > 90.0, r


# ---- 4. no interference with later steps ----
def test_evaluations_between_steps_leave_later_steps_bit_identical(gpu_mod):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_parity import compare_step
    sc = scenarios.small()
    g, o = _pair(gpu_mod, sc["params"])
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
        # between steps, nodes announced ahead: the evaluator in its own scratch, and (every third step) with the voxelisation
        r = g.evaluate_map(gt, 0.2)
        assert_same_result(r, evalmap.evaluate_clouds(gt, o.get_map(), 0.2))
        g.evaluate(gt, scans[k], 0.2, per_point=True)
        if k % 3 == 1:
            g.evaluate_map(gt, 0.2, voxel_leaf=0.2)
    assert g.get_map().shape == o.get_map().shape


# ---- 5. errors and the struct layout ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    E_INVALID, E_STATE = -1, -4
    g = gpu_mod.Erasor(gpu_mod.params_default())
    a = cloud(np.random.default_rng(1).uniform(-3, 3, (100, 3)), STATIC)
    for vs in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.evaluate(a, a, vs)
        assert e.value.rc == E_INVALID
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.evaluate(a, a, 0.2, voxel_leaf=0.2, per_point=True)
    assert e.value.rc == E_INVALID and "per_gt" in str(e.value)
    bad = a.copy()
    bad[7, 1] = np.nan
    for gt, est in ((bad, a), (a, bad)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.evaluate(gt, est, 0.2)
        assert e.value.rc == E_INVALID and "non-finite" in str(e.value)
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.evaluate(gt, est, 0.2, voxel_leaf=0.2)
        assert e.value.rc == E_INVALID
    pb = g.device_array(bad)
    try:
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.evaluate((pb, len(bad)), a, 0.2)
        assert e.value.rc == E_INVALID
    finally:
        g.device_free(pb)
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.evaluate_map(a, 0.2)
    assert e.value.rc == E_STATE  # no map
    assert g.evaluate(a, a, 0.2)["preserved_static"] == 100  # the handle is fine after the refusals
    # a step in flight: the NOFLY guard
    sc = scenarios.small()
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    for call in (lambda: g.evaluate(a, a, 0.2), lambda: g.evaluate_map(a, 0.2)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            call()
        assert e.value.rc == E_STATE
    g.step_wait()
    g.evaluate_map(a, 0.2)
    # the header's layout
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(erasor_eval_result), '
            'offsetof(erasor_eval_result, n_tied), offsetof(erasor_eval_result, PR), offsetof(erasor_eval_result, RR), offsetof(erasor_eval_result, F1));'
            'return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = gpu_mod.EvalResult
    assert got == [C.sizeof(R), R.n_tied.offset, R.PR.offset, R.RR.offset, R.F1.offset]


# ---- the offline driver ----
def test_offline_driver_eval_mode(gpu_mod, tmp_path):
    shim_dir = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
    shim = C.CDLL(os.path.join(shim_dir, "liberasor_shim.so"))
    shim.erasor_shim_save_pcd.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_int]
    shim.erasor_shim_save_pcd.restype = C.c_int
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval_golden.npz"))
    gt, est = np.ascontiguousarray(z["gt2"]), np.ascontiguousarray(z["est2"])
    fg, fe = tmp_path / "gt.pcd", tmp_path / "est.pcd"
    assert shim.erasor_shim_save_pcd(str(fg).encode(), gt.ctypes.data, len(gt), 1) == 0
    assert shim.erasor_shim_save_pcd(str(fe).encode(), est.ctypes.data, len(est), 0) == 0
    demo = os.path.join(shim_dir, "erasor_offline_demo")
    for leaf in (0.0, 0.2):
        out = subprocess.run([demo, "--eval", str(fg), str(fe), "0.2", str(leaf)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        row = [ln for ln in out.stdout.splitlines() if re.match(r"^\|\s*\d", ln)]
        assert len(row) == 1, out.stdout
        v = [s.strip() for s in row[0].strip("|").split("|")]
        if leaf:
            ref = evalmap.evaluate_clouds(gpu_mod.Erasor(gpu_mod.params_default()).voxelize_preserving_labels(gt, 0.2),
                                          gpu_mod.Erasor(gpu_mod.params_default()).voxelize_preserving_labels(est, 0.2), 0.2)
        else:
            ref = evalmap.evaluate_clouds(gt, est, 0.2)
        assert [int(x) for x in v[:6]] == [ref[k] for k in COUNTS]
        assert v[6:] == ["%.3f" % ref["PR"], "%.3f" % ref["RR"], "%.4f" % ref["F1"]]


# ---- 6. full size: the bench's world ----
@pytest.mark.timeout(900)
def test_full_size_map_matches_evalmap(gpu_mod):
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
    pg = g.device_array(m)
    try:
        g.evaluate_map((pg, len(m)), 0.2)  # (first call: allocations)
        t0 = time.perf_counter()
        r = g.evaluate_map((pg, len(m)), 0.2)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        rv = g.evaluate_map((pg, len(m)), 0.2, voxel_leaf=0.2)
        t_dev_vox = time.perf_counter() - t0
    finally:
        g.device_free(pg)
    t0 = time.perf_counter()
    ref = evalmap.evaluate_clouds(m, est, 0.2)
    t_host = time.perf_counter() - t0
    print("\nfull size: %d-pt ground truth, %d-pt map: evaluate_map %.1f ms (voxel_leaf 0.2: %.1f ms), evalmap (cKDTree, every core) %.1f ms; "
          "tied %d" % (len(m), len(est), t_dev * 1e3, t_dev_vox * 1e3, t_host * 1e3, r["n_tied"]))
    if r["n_tied"]:  # (which of two equidistant points of both classes cKDTree answers with is not defined)
        for k in ("preserved_static", "preserved_dynamic"):
            assert abs(r[k] - ref[k]) <= r["n_tied"], (k, r[k], ref[k], r["n_tied"])
    else:
        assert_same_result(r, ref)
    assert rv["gt_static"] + rv["gt_dynamic"] < len(m)
