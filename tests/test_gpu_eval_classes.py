"""PR / RR broken down by semantic class and by dynamic instance on the device (erasor_hip_evaluate_clouds_by_class /
erasor_hip_evaluate_map_by_class, kernels k_ev_*_keys onwards in evaluate.hip.h) against the host oracle evalmap.evaluate_by_class:
mixed fixtures, ties, the invariants that tie the rows to erasor_eval_result, key extremes, voxel_leaf, the handle's map, steps after a
breakdown, errors and sizing, the offline driver's --eval-classes mode, and the bench's full-size map.
tests/test_eval_classes_on_cpu.py re-runs part of this file against the CPU stand-in."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import scenarios
from erasor_amd import evalmap, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("gt_static", "gt_dynamic", "est_static", "est_dynamic", "preserved_static", "preserved_dynamic", "n_tied")
ROW_COUNTS = ("n_gt", "n_within", "n_preserved", "n_tied", "n_est")
OOR = 0x10000


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def cloud(xyz, lab):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.broadcast_to(np.asarray(lab, np.float32).reshape(-1, 1), (len(xyz), 1))], 1).astype(np.float32)


def inst(sem, k):
    """the intensity of instance k of class sem: (k << 16) | sem, exact in float32 for k < 256"""
    return np.float32(k * 65536 + sem)


def assert_rows_match(a, b, what):
    """device rows `a` against oracle rows `b`: the same keys; identical counters where the device row has no tie, else n_preserved
    within n_tied of the oracle's"""
    assert len(a) == len(b), (what, a["key"][:20], b["key"][:20])
    assert (a["key"] == b["key"]).all() and (a["is_dynamic"] == b["is_dynamic"]).all(), what
    for ra, rb in zip(a, b):
        if ra["n_tied"] == 0:
            assert all(ra[k] == rb[k] for k in ROW_COUNTS), (what, ra, rb)
            for k in ("PR", "RR"):
                assert (np.isnan(ra[k]) and np.isnan(rb[k])) or ra[k] == rb[k], (what, k, ra, rb)
        else:
            assert all(ra[k] == rb[k] for k in ("n_gt", "n_within", "n_est")), (what, ra, rb)
            assert abs(int(ra["n_preserved"]) - int(rb["n_preserved"])) <= int(ra["n_tied"]), (what, ra, rb)


def assert_invariants(r, plain=None):
    """the rows sum to the result's counters; the instances of each dynamic class sum to its row; equal to a separate evaluate()"""
    c, i = r["classes"], r["instances"]
    assert (np.diff(c["key"].astype(np.int64)) > 0).all() and (np.diff(i["key"].astype(np.int64)) > 0).all()
    dyn = c["is_dynamic"] != 0
    assert int(c["n_gt"][~dyn].sum()) == r["gt_static"] and int(c["n_gt"][dyn].sum()) == r["gt_dynamic"]
    assert int(c["n_est"][~dyn].sum()) == r["est_static"] and int(c["n_est"][dyn].sum()) == r["est_dynamic"]
    assert int(c["n_preserved"][~dyn].sum()) == r["preserved_static"] and int(c["n_preserved"][dyn].sum()) == r["preserved_dynamic"]
    assert int(c["n_tied"].sum()) == r["n_tied"]
    assert ((c["n_gt"] > 0) | (c["n_est"] > 0)).all() and ((i["n_gt"] > 0) | (i["n_est"] > 0)).all()
    assert (c["n_within"] <= c["n_gt"]).all() and (c["n_preserved"] <= c["n_within"]).all() and (c["n_tied"] <= c["n_within"]).all()
    sem = (i["key"] & 0xFFFF).astype(np.int64)
    assert ((sem >= 252) & (sem <= 259)).all() and (i["is_dynamic"] == 1).all()
    for row in c[dyn]:
        m = sem == int(row["key"])
        for k in ROW_COUNTS:
            assert int(i[k][m].sum()) == int(row[k]), (int(row["key"]), k)
    assert not (set(sem.tolist()) - set(c["key"][dyn].tolist()))
    if plain is not None:
        for k in plain:
            a, b = r[k], plain[k]
            assert a == b or (isinstance(a, float) and np.isnan(a) and np.isnan(b)), (k, a, b)


def check(h, gt, est, vs=0.2, **kw):
    r = h.evaluate_by_class(gt, est, vs, **kw)
    assert_invariants(r, h.evaluate(gt, est, vs, **kw))
    return r


def fixtures():
    rng = np.random.default_rng(20261016)
    cases = {}
    # mixed static classes, all 8 dynamic classes with several instances each, instance bits on static labels too
    n = 3000
    xyz = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    stat = rng.choice([0.0, 1.0, 10.0, 40.0, 44.0, 48.0, 50.0, 70.0, 72.0, 80.0, 99.0, 251.0, 260.0], n)
    stat = np.where(rng.uniform(size=n) < 0.1, stat + 65536.0 * rng.integers(1, 5, n), stat)
    dyn = np.array([inst(252 + s, k) for s, k in zip(rng.integers(0, 8, n), rng.integers(0, 6, n))], np.float32)
    lab = np.where(rng.uniform(size=n) < 0.35, dyn, stat).astype(np.float32)
    gt = cloud(xyz, lab)
    keep = rng.uniform(size=n) < 0.7
    est = gt[keep].copy()
    est[:, :3] += rng.normal(0, 0.07, (len(est), 3)).astype(np.float32)
    flip = rng.uniform(size=len(est)) < 0.08
    est[flip, 3] = np.where(rng.uniform(size=int(flip.sum())) < 0.5, np.float32(40.0), inst(254, 77))  # (254 / instance 77: estimate only)
    est = np.concatenate([est, est[:100]])  # duplicate points, same labels
    cases["mixed"] = (gt, est)
    # ties: estimated pairs of both classes at exactly the same distance of a GT point, and same-class pairs
    g, e = [], []
    for k in range(40):
        c = np.array([3.0 * k, 1.0, 0.5], np.float32)
        g.append(np.r_[c, inst(252 + k % 8, k % 3) if k % 2 else np.float32(40.0)])
        lab2 = (np.float32(50.0), inst(255, 1)) if k % 4 < 2 else (np.float32(40.0), np.float32(48.0))
        e.append(np.r_[c + np.float32([0.0625, 0, 0]), lab2[0]])
        e.append(np.r_[c - np.float32([0.0625, 0, 0]), lab2[1]])
    cases["ties"] = (np.array(g, np.float32), np.array(e, np.float32))
    return cases


CASES = fixtures()


# ---- 1. oracle equality (host and device inputs) and 2. the invariants ----
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("device_inputs", [False, True])
def test_rows_match_the_oracle_and_sum_to_the_result(handle, name, device_inputs):
    gt, est = CASES[name]
    ref = evalmap.evaluate_by_class(gt, est, 0.2)
    if device_inputs:
        pg, pe = handle.device_array(gt), handle.device_array(est)
        try:
            r = handle.evaluate_by_class((pg, len(gt)), (pe, len(est)), 0.2)
        finally:
            handle.device_free(pg)
            handle.device_free(pe)
    else:
        r = handle.evaluate_by_class(gt, est, 0.2)
    assert_invariants(r, handle.evaluate(gt, est, 0.2))
    for k in COUNTS:
        assert r[k] == ref[k], (k, r[k], ref[k])
    assert_rows_match(r["classes"], ref["classes"], name + " classes")
    assert_rows_match(r["instances"], ref["instances"], name + " instances")
    if name == "mixed":
        assert {252 + s for s in range(8)} <= set(r["classes"]["key"].tolist())
        assert len(r["instances"]) > 40 and r["n_tied"] == 0
        e77 = r["instances"][r["instances"]["key"] == 77 * 65536 + 254]
        assert len(e77) == 1 and e77["n_gt"][0] == 0 and e77["n_est"][0] > 0  # an estimate-only instance
    if name == "ties":
        assert r["n_tied"] == 20 and ref["n_tied"] == 20  # (k % 4 < 2: a static and a dynamic point at the same distance)


# ---- 3. key extremes ----
def test_one_class_everywhere(handle):
    rng = np.random.default_rng(3)
    xyz = rng.uniform(-10, 10, (6000, 3)).astype(np.float32)
    gt = cloud(xyz, 40.0)
    r = check(handle, gt, cloud(xyz[::2] + np.float32(0.01), 40.0))
    assert len(r["classes"]) == 1 and len(r["instances"]) == 0
    row = r["classes"][0]
    assert row["key"] == 40 and row["n_gt"] == 6000 and row["n_est"] == 3000 and row["n_preserved"] == r["preserved_static"]
    dy = check(handle, cloud(xyz, inst(252, 9)), cloud(xyz[::3], inst(252, 9)))
    assert len(dy["instances"]) == 1 and dy["instances"][0]["n_gt"] == 6000 and dy["instances"][0]["n_est"] == 2000


def test_every_key_once_and_labels_out_of_range(handle):
    n = 65536
    xyz = np.stack([np.arange(n) % 256, np.arange(n) // 256, np.zeros(n)], 1).astype(np.float32)
    lab = (np.arange(n, dtype=np.float64) + 65536.0 * (np.arange(n) % 3)).astype(np.float32)
    bad = np.array([np.nan, -1.0, 4294967296.0, np.inf, -np.inf], np.float32)
    gt = np.concatenate([cloud(xyz, lab), cloud([[0.0, -5.0 - k, 0.0] for k in range(5)], bad)])
    est = gt[::2].copy()
    r = check(handle, gt, est)
    c = r["classes"]
    assert len(c) == 65537 and (c["key"] == np.arange(65537)).all()
    assert (c["n_gt"][:65536] == 1).all() and c[-1]["key"] == OOR and c[-1]["n_gt"] == 5 and c[-1]["is_dynamic"] == 0
    assert r["n_label_out_of_range"] == 5 + 3
    ref = evalmap.evaluate_by_class(gt, est, 0.2)
    assert_rows_match(c, ref["classes"], "every key")
    assert_rows_match(r["instances"], ref["instances"], "every key instances")


def test_empty_clouds(handle):
    gt, est = CASES["mixed"]
    r = check(handle, gt, np.zeros((0, 4), np.float32))
    assert (r["classes"]["n_within"] == 0).all() and (r["classes"]["n_est"] == 0).all()
    assert_rows_match(r["classes"], evalmap.evaluate_by_class(gt, np.zeros((0, 4), np.float32))["classes"], "empty estimate")
    r = check(handle, np.zeros((0, 4), np.float32), est)
    assert (r["classes"]["n_gt"] == 0).all() and int(r["classes"]["n_est"].sum()) == len(est)
    assert (r["instances"]["n_gt"] == 0).all() and int(r["instances"]["n_est"].sum()) == r["est_dynamic"]
    r = check(handle, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32))
    assert len(r["classes"]) == 0 and len(r["instances"]) == 0


# ---- 4. voxel_leaf ----
def test_voxel_leaf_against_the_oracle_on_voxelised_clouds(handle):
    gt, est = CASES["mixed"]
    r = check(handle, gt, est, voxel_leaf=0.2)
    ref = evalmap.evaluate_by_class(handle.voxelize_preserving_labels(gt, 0.2), handle.voxelize_preserving_labels(est, 0.2), 0.2)
    for k in COUNTS:
        assert r[k] == ref[k], k
    assert_rows_match(r["classes"], ref["classes"], "voxel_leaf classes")
    assert_rows_match(r["instances"], ref["instances"], "voxel_leaf instances")


# ---- 5. the handle's map ----
@pytest.mark.parametrize("large_scale", [False, True])
def test_evaluate_map_by_class_after_twelve_steps(gpu_mod, large_scale):
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
    for leaf in (0.0, 0.2):
        r = g.evaluate_map_by_class(sc["map"], 0.2, voxel_leaf=leaf)
        assert_invariants(r, g.evaluate_map(sc["map"], 0.2, voxel_leaf=leaf))
        ref = g.evaluate_by_class(sc["map"], m, 0.2, voxel_leaf=leaf)
        for k in ("classes", "instances"):
            assert r[k].tobytes() == ref[k].tobytes(), (leaf, k)
    ho = evalmap.evaluate_by_class(sc["map"], m, 0.2)
    r = g.evaluate_map_by_class(sc["map"], 0.2)
    assert_rows_match(r["classes"], ho["classes"], "map classes")
    assert_rows_match(r["instances"], ho["instances"], "map instances")
    assert r["gt_dynamic"] > 0 and len(r["instances"]) > 0


def test_breakdowns_between_steps_leave_later_steps_bit_identical(gpu_mod):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_parity import compare_step
    from oracle import orc
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
        # between steps, nodes announced ahead: the breakdown in the evaluator's scratch and histogram bank (voxel_leaf 0)
        r = g.evaluate_map_by_class(gt, 0.2)
        assert_invariants(r, g.evaluate_map(gt, 0.2))
        g.evaluate_by_class(gt, scans[k], 0.2)
    assert g.get_map().shape == o.get_map().shape


# ---- 6. errors, sizing and the struct layout ----
def test_errors_sizing_and_struct_layout(gpu_mod, handle, tmp_path):
    E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
    L = gpu_mod.lib()
    gt, est = CASES["mixed"]
    a = cloud(np.random.default_rng(1).uniform(-3, 3, (100, 3)), 40.0)
    for vs in (0.0, -0.2, float("nan")):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.evaluate_by_class(a, a, vs)
        assert e.value.rc == E_INVALID
    bad = a.copy()
    bad[7, 1] = np.nan
    for g_, e_ in ((bad, a), (a, bad)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.evaluate_by_class(g_, e_, 0.2)
        assert e.value.rc == E_INVALID and "non-finite" in str(e.value)
    with pytest.raises(gpu_mod.ErasorError) as e:
        gpu_mod.Erasor(gpu_mod.params_default()).evaluate_map_by_class(a, 0.2)
    assert e.value.rc == E_STATE
    nc, ni, r = C.c_size_t(7), C.c_size_t(7), gpu_mod.EvalResult()
    # NULL clouds with points, NULL counts, a NULL array with a capacity
    args = lambda gp, ep, rows, cap, pnc: (handle._h, gp, C.c_size_t(len(gt)), C.c_int(0), ep, C.c_size_t(len(est)), C.c_int(0), C.c_double(0.0),
                                           C.c_double(0.2), rows, C.c_size_t(cap), pnc, None, C.c_size_t(0), C.byref(ni), C.byref(r))
    pg, pe = gt.ctypes.data_as(C.c_void_p), est.ctypes.data_as(C.c_void_p)
    assert L.erasor_hip_evaluate_clouds_by_class(*args(None, pe, None, 0, C.byref(nc))) == E_INVALID
    assert L.erasor_hip_evaluate_clouds_by_class(*args(pg, None, None, 0, C.byref(nc))) == E_INVALID
    assert L.erasor_hip_evaluate_clouds_by_class(*args(pg, pe, None, 0, None)) == E_INVALID
    assert L.erasor_hip_evaluate_clouds_by_class(*args(pg, pe, None, 5, C.byref(nc))) == E_INVALID
    # the size query: NULL arrays with capacity 0 -> ERASOR_E_CAPACITY with the counts and the result
    full = handle.evaluate_by_class(gt, est, 0.2)
    assert L.erasor_hip_evaluate_clouds_by_class(*args(pg, pe, None, 0, C.byref(nc))) == E_CAPACITY
    assert nc.value == len(full["classes"]) and ni.value == len(full["instances"]) and r.as_dict() == handle.evaluate(gt, est, 0.2)
    # classes fit, instances one short
    cls = np.zeros(nc.value, gpu_mod.CLASS_ROW_DTYPE)
    ins = np.zeros(ni.value, gpu_mod.CLASS_ROW_DTYPE)
    call = lambda cap_i: L.erasor_hip_evaluate_clouds_by_class(handle._h, pg, C.c_size_t(len(gt)), C.c_int(0), pe, C.c_size_t(len(est)), C.c_int(0),
                                                                C.c_double(0.0), C.c_double(0.2), cls.ctypes.data_as(C.c_void_p), C.c_size_t(len(cls)),
                                                                C.byref(nc), ins.ctypes.data_as(C.c_void_p), C.c_size_t(cap_i), C.byref(ni), C.byref(r))
    assert call(len(ins) - 1) == E_CAPACITY and ni.value == len(ins)
    assert call(len(ins)) == 0
    for k in gpu_mod.CLASS_ROW_DTYPE.names:
        assert (cls[k] == full["classes"][k]).all() and (ins[k] == full["instances"][k]).all(), k
    # the header's layout
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %u\\n", '
            'sizeof(erasor_eval_class_row), offsetof(erasor_eval_class_row, is_dynamic), offsetof(erasor_eval_class_row, n_gt), '
            'offsetof(erasor_eval_class_row, n_within), offsetof(erasor_eval_class_row, n_preserved), offsetof(erasor_eval_class_row, n_tied), '
            'offsetof(erasor_eval_class_row, n_est), ERASOR_EVAL_KEY_LABEL_OUT_OF_RANGE);return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R = gpu_mod.ClassRow
    assert got == [C.sizeof(R), R.is_dynamic.offset, R.n_gt.offset, R.n_within.offset, R.n_preserved.offset, R.n_tied.offset, R.n_est.offset,
                   gpu_mod.EVAL_KEY_LABEL_OUT_OF_RANGE]
    assert gpu_mod.CLASS_ROW_DTYPE.itemsize == C.sizeof(R)
    assert all(gpu_mod.CLASS_ROW_DTYPE.fields[k][1] == getattr(R, k).offset for k in gpu_mod.CLASS_ROW_DTYPE.names)


# ---- 7. the offline driver ----
def test_offline_driver_eval_classes_mode(gpu_mod, tmp_path):
    shim_dir = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
    shim = C.CDLL(os.path.join(shim_dir, "liberasor_shim.so"))
    shim.erasor_shim_save_pcd.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_int]
    shim.erasor_shim_save_pcd.restype = C.c_int
    gt, est = (np.ascontiguousarray(a) for a in CASES["mixed"])
    fg, fe = tmp_path / "gt.pcd", tmp_path / "est.pcd"
    assert shim.erasor_shim_save_pcd(str(fg).encode(), gt.ctypes.data, len(gt), 1) == 0
    assert shim.erasor_shim_save_pcd(str(fe).encode(), est.ctypes.data, len(est), 1) == 0
    demo = os.path.join(shim_dir, "erasor_offline_demo")
    h = gpu_mod.Erasor(gpu_mod.params_default())
    for leaf in (0.0, 0.2):
        plain = subprocess.run([demo, "--eval", str(fg), str(fe), "0.2", str(leaf)], capture_output=True, text=True, timeout=120)
        out = subprocess.run([demo, "--eval-classes", str(fg), str(fe), "0.2", str(leaf)], capture_output=True, text=True, timeout=120)
        assert plain.returncode == 0 and out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        assert lines[: len(plain.stdout.splitlines())] == plain.stdout.splitlines()
        g2, e2 = (h.voxelize_preserving_labels(gt, 0.2), h.voxelize_preserving_labels(est, 0.2)) if leaf else (gt, est)
        ref = evalmap.evaluate_by_class(g2, e2, 0.2)
        rows = [[s.strip() for s in ln.strip("|").split("|")] for ln in lines if re.match(r"^\|\s*\d+ \| ", ln)]
        rows = [v for v in rows if len(v) == 6]
        assert len(rows) == len(ref["classes"]), out.stdout
        for v, rr in zip(rows, ref["classes"]):
            key = int(v[0])
            assert key == rr["key"] and v[1] == evalmap.SEMANTIC_KITTI_NAMES.get(key, "-")
            assert int(v[2]) == rr["n_gt"] and int(v[3]) == rr["n_preserved"] and int(v[5]) == rr["n_est"]
            rate = rr["RR"] if rr["is_dynamic"] else rr["PR"]
            assert v[4] == ("RR" if rr["is_dynamic"] else "PR") + " %7.3f" % rate
        ins = ref["instances"][ref["instances"]["n_gt"] > 0]
        gone = ins["n_gt"] - ins["n_preserved"]
        want = "dynamic instances in the ground truth: %d; fully removed %d, >= 90%% removed %d, >= 50%% removed %d, not removed %d" % (
            len(ins), (gone == ins["n_gt"]).sum(), (gone * 10 >= ins["n_gt"] * 9).sum(), (gone * 2 >= ins["n_gt"]).sum(), (gone == 0).sum())
        assert want in lines, out.stdout


# ---- 8. full size: the bench's world ----
@pytest.mark.timeout(1200)
def test_full_size_map_by_class_matches_the_oracle(gpu_mod):
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
        g.evaluate_map_by_class((pg, len(m)), 0.2)  # (first call: allocations)
        g.evaluate_map((pg, len(m)), 0.2)
        t0 = time.perf_counter()
        plain = g.evaluate_map((pg, len(m)), 0.2)
        t_plain = time.perf_counter() - t0
        t0 = time.perf_counter()
        r = g.evaluate_map_by_class((pg, len(m)), 0.2)
        t_dev = time.perf_counter() - t0
    finally:
        g.device_free(pg)
    assert_invariants(r, plain)
    t0 = time.perf_counter()
    ref = evalmap.evaluate_by_class(m, est, 0.2)
    t_host = time.perf_counter() - t0
    print("\nfull size: %d-pt ground truth, %d-pt map: evaluate_map_by_class %.1f ms, evaluate_map %.1f ms, evalmap.evaluate_by_class %.1f ms; "
          "%d classes, %d instances, tied %d" % (len(m), len(est), t_dev * 1e3, t_plain * 1e3, t_host * 1e3, len(r["classes"]), len(r["instances"]),
                                                  r["n_tied"]))
    assert_rows_match(r["classes"], ref["classes"], "full-size classes")
    assert_rows_match(r["instances"], ref["instances"], "full-size instances")
    assert len(r["instances"]) > 0
