"""Maps without labels on the device: label_map (erasor_hip_label_map; src/utils/fill_removert_intensity.cpp:24-59) and calc_complement
(erasor_hip_static_complement; src/utils/compare_complement.cpp:43-75), kernels in nearest.hip.h, against the host oracle
(oracle/orc.voxel_grid for the centroids, evalmap.label_from / evalmap.static_complement for FLANN's float32 1-NN): a labelled
world, fixtures where float32 and float64 pick different points, far and degenerate clouds, the complement's threshold, relabelling a
cleaned map end to end, steps after the calls, errors, the offline driver's --label / --complement modes and the bench's full-size
map.  tests/test_label_map_on_cpu.py re-runs part of this file against the CPU stand-in."""
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
from oracle import orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
LABEL_FIELDS = ("n_src", "n_out", "n_tied", "passthrough")
COMPLEMENT_FIELDS = ("n_gt", "n_gt_static", "n_lost", "n_label_out_of_range")


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def label_oracle(src, medium, leaf):
    """orc.voxel_grid's centroids (the input itself when VoxelGrid's indices overflow, as PCL returns it), labelled by label_from"""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 4)
    cent, _, _, overflow = orc.voxel_grid(src, leaf)
    if overflow:
        cent = src.copy()
    rows, info = evalmap.label_from(cent, medium)
    return rows, dict(info, n_src=len(src), n_out=len(rows), passthrough=int(overflow))


def assert_label_matches(handle, src, medium, leaf, device_inputs=False, what=""):
    if device_inputs:
        ps, pm = handle.device_array(src), handle.device_array(medium)
        try:
            rows, info = handle.label_map((ps, len(src)), (pm, len(medium)), leaf)
        finally:
            handle.device_free(ps)
            handle.device_free(pm)
    else:
        rows, info = handle.label_map(src, medium, leaf)
    ref, ref_info = label_oracle(src, medium, leaf)
    assert {k: info[k] for k in LABEL_FIELDS} == {k: ref_info[k] for k in LABEL_FIELDS}, what
    same = (bits(rows) == bits(ref)).all(1)
    assert same.all(), "%s: %d of %d rows differ (first %s: %r vs %r)" % (what, (~same).sum(), len(same), np.argwhere(~same)[:3].ravel().tolist(),
                                                                        rows[~same][:2], ref[~same][:2])
    return rows, info


def world_clouds():
    """a dense labelled sample of a synthetic world (the medium) and a sparser sample of the same world with its labels zeroed"""
    w = synth.World(seed=20210311, length=60.0)
    medium = w.sample_map(spacing=0.1, frames=range(0, 20, 4), x_range=(0.0, 24.0))
    src = w.sample_map(spacing=0.2, frames=range(0, 20, 4), x_range=(0.0, 24.0))
    src[:, 3] = 0.0
    return np.ascontiguousarray(src), np.ascontiguousarray(medium)


# ---- 1. a labelled world: rows and n_tied against the oracle ----
@pytest.mark.parametrize("leaf", [0.2, 0.5])
@pytest.mark.parametrize("device_inputs", [False, True])
def test_label_map_of_a_world_matches_the_oracle(handle, leaf, device_inputs):
    src, medium = world_clouds()
    rows, info = assert_label_matches(handle, src, medium, leaf, device_inputs, "world leaf %g" % leaf)
    assert info["n_out"] < len(src) and not info["passthrough"]
    assert len(np.unique(rows[:, 3])) > 5  # (ground, facades, cars, poles, moving objects' trails)


# ---- 2. the metric is FLANN's float32, not float64 ----
def float_metric_triple(centre, rng):
    """(query, point B, point A) near `centre`: float64 d^2 makes A strictly nearer, float32 d^2 puts B at or below A.  B is A moved
    by a few ulps in one coordinate."""
    while True:
        q = (centre + rng.uniform(-3, 3, (100000, 3))).astype(np.float32)
        a = (q + rng.uniform(-0.3, 0.3, (len(q), 3))).astype(np.float32)
        b = a.copy()
        r, k = np.arange(len(q)), rng.integers(0, 3, len(q))
        b[r, k] = (a[r, k].view(np.int32) + rng.integers(-3, 4, len(q)).astype(np.int32)).view(np.float32)
        d64 = lambda p: ((q.astype(np.float64) - p.astype(np.float64)) ** 2).sum(1)
        pick = np.nonzero((d64(a) < d64(b)) & (evalmap._l2_simple(q, b) <= evalmap._l2_simple(q, a)))[0]
        if len(pick):
            return q[pick[0]], b[pick[0]], a[pick[0]]


def test_the_metric_is_float32_with_the_lowest_index_on_ties(handle):
    rng = np.random.default_rng(5)
    src, med = [], []
    for k in range(6):  # (each triple 40 m from the others, each query alone in its voxel)
        q, b, a = float_metric_triple(np.array([40.0 * k, 0.0, 0.0]), rng)
        src.append(q)
        med += [(b, 100.0 + k), (a, 200.0 + k)]  # B has the lower index
    src = xyzi(np.array(src), 0.0)
    medium = np.array([np.append(p, lab) for p, lab in med], np.float32)
    # the fixture is what it claims: cKDTree (float64) picks A, float32 picks B
    _, i64 = cKDTree(medium[:, :3].astype(np.float64)).query(src[:, :3].astype(np.float64), k=1)
    i32, _, _ = evalmap.nearest_f32(medium[:, :3], src[:, :3])
    assert (i64 == 2 * np.arange(len(src)) + 1).all() and (i32 == 2 * np.arange(len(src))).all()
    rows, info = assert_label_matches(handle, src, medium, 0.2, what="float metric")
    o = np.argsort(rows[:, 0])  # (rows come in voxel order; the triples lie along x)
    assert rows[o, 3].tolist() == [100.0 + k for k in range(len(src))]
    assert (bits(rows[o, :3]) == bits(src[:, :3])).all()  # (a lone point's centroid is the point)
    # duplicates: the lowest index wins; only a duplicate with different intensity bits is a tie
    p = np.array([[1.0, 2.0, 3.0], [30.0, 2.0, 3.0], [60.0, 2.0, 3.0]], np.float32)
    medium = np.concatenate([xyzi(p[[0]], 7.0), xyzi(p[[1]], 9.0), xyzi(p[[0]], 5.0), xyzi(p[[1]], 9.0), xyzi(p[[2]], 11.0),
                             xyzi(p[[2]], 6.0), xyzi(p[[2]], 11.0)])
    rows, info = assert_label_matches(handle, xyzi(p, 0.0), medium, 0.2, what="duplicates")
    assert rows[np.argsort(rows[:, 0]), 3].tolist() == [7.0, 9.0, 11.0] and info["n_tied"] == 2


# ---- 3. far and degenerate clouds ----
def degenerate_cases():
    rng = np.random.default_rng(17)
    pts = rng.uniform(-20, 20, (3000, 3))
    labels = rng.integers(0, 300, 3000).astype(np.float32)
    near = xyzi(rng.uniform(-25, 25, (4000, 3)), 0.0)
    cases = {"far_queries": (xyzi(rng.uniform(-1, 1, (500, 3)) * 3000.0 + np.array([4000.0, -2500.0, 100.0]), 0.0), xyzi(pts, labels))}
    plane = pts.copy()
    plane[:, 2] = 1.5
    cases["planar_medium"] = (near, xyzi(plane, labels))
    line = pts.copy()
    line[:, 1:] = 0.0
    cases["linear_medium"] = (near, xyzi(line, labels))
    cases["single_point_medium"] = (near, xyzi([[0.5, -0.5, 2.0]], 77.0))
    return cases


@pytest.mark.parametrize("name", sorted(degenerate_cases()))
def test_far_and_degenerate_clouds_match_the_oracle(handle, name):
    src, medium = degenerate_cases()[name]
    rows, info = assert_label_matches(handle, src, medium, 0.2, what=name)
    if name == "single_point_medium":
        assert (rows[:, 3] == 77.0).all()


def test_subnormal_differences_are_not_flushed(handle):
    # A is 1e-20 from the query: its d^2 (1e-40) is a float32 subnormal, which flush-to-zero would tie with B's exact 0 -- and the
    # lower index (A) would win.  Unflushed, B is strictly nearer.
    a2 = np.float32(1e-20) * np.float32(1e-20)
    assert 0 < a2 < np.finfo(np.float32).tiny
    medium = np.concatenate([xyzi([[1e-20, 0.0, 0.0]], 1.0), xyzi([[0.0, 0.0, 0.0]], 2.0), xyzi([[0.0, 1e-20, 0.0]], 3.0)])
    src = xyzi([[0.0, 0.0, 0.0]], 0.0)
    rows, info = assert_label_matches(handle, src, medium, 0.2, what="subnormal")
    assert rows[:, 3].tolist() == [2.0] and info["n_tied"] == 0
    # the complement: a static ground-truth point 1e-20 from the only estimated point is not lost, its d^2 (1e-40) is not > 0.03
    rows, info = assert_complement_matches(handle, xyzi([[0.0, 0.0, 0.0]], 0.0), xyzi([[1e-20, 0.0, 0.0]], 40.0), what="subnormal")
    assert info["n_lost"] == 0 and info["n_gt_static"] == 1


def test_voxel_index_overflow_labels_the_input_as_it_is(handle):
    rng = np.random.default_rng(23)
    src = xyzi(rng.uniform(-1, 1, (600, 3)) * np.array([4000.0, 4000.0, 50.0]), 0.0)
    medium = xyzi(rng.uniform(-1, 1, (5000, 3)) * np.array([4000.0, 4000.0, 50.0]), rng.integers(1, 260, 5000))
    rows, info = assert_label_matches(handle, src, medium, 0.001, what="overflow")
    assert info["passthrough"] == 1 and info["n_out"] == len(src)
    assert (bits(rows[:, :3]) == bits(src[:, :3])).all()


def test_empty_and_invalid_label_inputs(gpu_mod, handle):
    rng = np.random.default_rng(29)
    a = xyzi(rng.uniform(-3, 3, (100, 3)), 40.0)
    empty = np.zeros((0, 4), np.float32)
    rows, info = handle.label_map(empty, a, 0.2)
    assert rows.shape == (0, 4) and info == {"n_src": 0, "n_out": 0, "n_tied": 0, "passthrough": 0}
    rows, info = handle.label_map(empty, empty, 0.2)
    assert rows.shape == (0, 4) and info["n_out"] == 0
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.label_map(a, empty, 0.2)
    assert e.value.rc == E_INVALID and "empty medium" in str(e.value)
    for leaf in (0.0, -0.2, float("nan"), float("inf")):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.label_map(a, a, leaf)
        assert e.value.rc == E_INVALID
    for k in range(3):
        bad = a.copy()
        bad[7, k] = (np.nan, np.inf, -np.inf)[k]
        for s, m in ((bad, a), (a, bad)):
            with pytest.raises(gpu_mod.ErasorError) as e:
                handle.label_map(s, m, 0.2)
            assert e.value.rc == E_INVALID and "non-finite" in str(e.value)
    rows, info = handle.label_map(a, a, 0.2)  # the handle is fine after the refusals
    assert info["n_out"] == len(rows) > 0 and (rows[:, 3] == 40.0).all()


# ---- 4. the complement against evalmap.static_complement ----
def assert_complement_matches(handle, est, gt, device_inputs=False, what=""):
    if device_inputs:
        pe, pg = handle.device_array(est), handle.device_array(gt)
        try:
            rows, info = handle.static_complement((pe, len(est)), (pg, len(gt)))
        finally:
            handle.device_free(pe)
            handle.device_free(pg)
    else:
        rows, info = handle.static_complement(est, gt)
    ref, ref_info = evalmap.static_complement(est, gt)
    assert info == ref_info, what
    assert rows.shape == ref.shape and (bits(rows) == bits(ref)).all(), what
    return rows, info


@pytest.mark.parametrize("device_inputs", [False, True])
def test_complement_of_a_world_matches_the_oracle(handle, device_inputs):
    _, gt = world_clouds()
    rng = np.random.default_rng(31)
    keep = rng.random(len(gt)) < 0.7
    est = gt[keep].copy()
    est[:, :3] += rng.normal(0, 0.08, (len(est), 3)).astype(np.float32)  # (jittered: distances on both sides of the threshold)
    est[:, 3] = 0.0
    rows, info = assert_complement_matches(handle, est, gt, device_inputs, "world")
    assert 0 < info["n_lost"] < info["n_gt_static"] < info["n_gt"]


def threshold_offsets():
    """(dx, dy) float32 pairs whose FLANN d^2 from the origin is exactly 0.03f (not lost: 0.0299999993 as a double) and the next float
    up (lost), found by a search on the host"""
    t0 = np.float32(0.03)
    t1 = np.nextafter(t0, np.float32(1.0))
    base = np.float32(np.sqrt(0.015))
    xs = (base.view(np.int32) + np.arange(-1500, 1500, dtype=np.int32)).view(np.float32)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    q = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size, np.float32)], 1)
    d2 = evalmap._l2_simple(q, np.zeros_like(q))
    out = []
    for t in (t0, t1):
        i = np.nonzero(d2 == t)[0]
        assert len(i) >= 2, t
        out.append(q[i[:2], :2])
    assert float(t0) < 0.03 < float(t1)
    return out


def test_complement_threshold_static_dynamic_and_instance_bits(handle):
    at, above = threshold_offsets()
    est, gt, expect = [], [], []
    for k, (dx, dy) in enumerate(np.concatenate([at, above])):
        e = np.array([0.0, 0.0, 10.0 * k], np.float32)  # (z apart: dz = 0 exactly for each pair, 10 m from the others)
        est.append(xyzi(e, 0.0))
        gt.append(xyzi([[dx, dy, e[2]]], 40.0 + (k << 16)))  # (static, with instance bits)
        expect.append(k >= 2)
    # dynamic points far from everything never appear; out-of-range intensities are static and counted
    far = [[500.0, 0.0, 0.0], [500.0, 50.0, 0.0], [500.0, 100.0, 0.0], [500.0, 150.0, 0.0], [500.0, 200.0, 0.0], [500.0, 250.0, 0.0]]
    labels = [252.0, 259.0 + (7 << 16), 255.0 + (1 << 16), 251.0, -1.0, 5e9]
    for p, lab in zip(far, labels):
        gt.append(xyzi([p], lab))
        expect.append(lab in (251.0, -1.0, 5e9))
    nan_label = xyzi([[500.0, 300.0, 0.0]], np.nan)
    gt.append(nan_label)
    expect.append(True)
    est, gt = np.concatenate(est), np.concatenate(gt)
    # the pairs are what they claim on the host
    d2 = evalmap._l2_simple(gt[:4, :3], est[:4, :3])
    assert d2[0] == d2[1] == np.float32(0.03) and d2[2] == d2[3] == np.nextafter(np.float32(0.03), np.float32(1))
    rows, info = assert_complement_matches(handle, est, gt, what="threshold")
    assert (bits(rows) == bits(gt[np.array(expect)])).all()
    assert info == {"n_gt": len(gt), "n_gt_static": 4 + 4, "n_lost": 2 + 4, "n_label_out_of_range": 3}
    # an empty estimate: every static point, in order
    rows, info = assert_complement_matches(handle, np.zeros((0, 4), np.float32), gt, what="empty estimate")
    assert info["n_lost"] == info["n_gt_static"] == 8


def test_complement_empty_and_invalid_inputs(gpu_mod, handle):
    a = xyzi(np.random.default_rng(37).uniform(-3, 3, (100, 3)), 40.0)
    rows, info = handle.static_complement(a, np.zeros((0, 4), np.float32))
    assert rows.shape == (0, 4) and info == {"n_gt": 0, "n_gt_static": 0, "n_lost": 0, "n_label_out_of_range": 0}
    bad = a.copy()
    bad[3, 2] = np.nan
    for e_, g_ in ((bad, a), (a, bad)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.static_complement(e_, g_)
        assert e.value.rc == E_INVALID and "non-finite" in str(e.value)
    rows, info = handle.static_complement(a, a)
    assert rows.shape == (0, 4) and info["n_gt_static"] == 100


# ---- 5. end to end: a cleaned map, its labels erased, relabelled and evaluated ----
def test_relabelled_cleaned_map_evaluates_as_the_oracle_labelled_one(gpu_mod):
    sc = scenarios.small()
    g = gpu_mod.Erasor(scenarios.to_product_params(sc["params"]))
    g.set_map(sc["map"])
    for f in range(6):
        g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    cleaned = g.get_map()
    cleaned[:, 3] = 0.0
    dense = sc["map"]
    rows, info = g.label_map(cleaned, dense, 0.2)
    ref, _ = label_oracle(cleaned, dense, 0.2)
    assert (bits(rows) == bits(ref)).all()
    r = g.evaluate(dense, rows, 0.2)
    want = evalmap.evaluate_clouds(dense, ref, 0.2)
    assert {k: r[k] for k in want} == want
    assert 0 < r["preserved_static"] < r["gt_static"]


# ---- 6. no interference with later steps ----
def test_label_and_complement_between_steps_leave_later_steps_bit_identical(gpu_mod):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
    dense = sc["map"][::2].copy()
    for k in range(n):
        if k + ahead < n:
            g.prefetch(scans[k + ahead], sc["T_l2b"], Tb[k + ahead], To[k + ahead])
        rg = g.step(scans[k], sc["T_l2b"], Tb[k], To[k])
        ro = o.step(scans[k], sc["T_l2b"], Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
        # between steps, nodes announced ahead: the complement in the evaluator's scratch, the tree's sort in a radix bank of its own;
        # label_map voxelises (it drops the announcements, whose steps then run their own chains)
        m = o.get_map()
        rows, info = g.static_complement(m, dense)
        ref, ref_info = evalmap.static_complement(m, dense)
        assert info == ref_info and (bits(rows) == bits(ref)).all()
        if k % 3 == 1:
            rows, _ = g.label_map(scans[k], dense, 0.2)
            ref, _ = label_oracle(scans[k], dense, 0.2)
            assert (bits(rows) == bits(ref)).all()
    assert g.get_map().shape == o.get_map().shape


# ---- 7. errors, the struct layout and the offline driver ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    a = xyzi(np.random.default_rng(41).uniform(-3, 3, (300, 3)), 40.0)
    lib, h = gpu_mod.lib(), g._h
    # a caller buffer too small: ERASOR_E_CAPACITY, the result filled first; NULL: the counts only
    out = np.zeros((2, 4), np.float32)
    r = gpu_mod.LabelResult()
    rc = lib.erasor_hip_label_map(h, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0,
                                  C.c_double(0.2), out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out)), C.byref(r))
    assert rc == E_CAPACITY and r.n_out > 2 and r.n_src == len(a)
    r2 = gpu_mod.LabelResult()
    assert lib.erasor_hip_label_map(h, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0,
                                    C.c_double(0.2), None, C.c_size_t(0), C.byref(r2)) == 0
    assert r2.n_out == r.n_out
    far = a.copy()
    far[:, 0] += 100.0
    c = gpu_mod.ComplementResult()
    rc = lib.erasor_hip_static_complement(h, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, far.ctypes.data_as(C.c_void_p),
                                          C.c_size_t(len(far)), 0, out.ctypes.data_as(C.c_void_p), C.c_size_t(len(out)), C.byref(c))
    assert rc == E_CAPACITY and c.n_lost == len(far)
    assert lib.erasor_hip_static_complement(h, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, far.ctypes.data_as(C.c_void_p),
                                            C.c_size_t(len(far)), 0, None, C.c_size_t(0), C.byref(c)) == 0 and c.n_lost == len(far)
    assert lib.erasor_hip_label_map(h, None, C.c_size_t(5), 0, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, C.c_double(0.2), None,
                                    C.c_size_t(0), C.byref(r)) == E_INVALID
    assert lib.erasor_hip_label_map(h, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0,
                                    C.c_double(0.2), None, C.c_size_t(0), None) == E_INVALID
    assert lib.erasor_hip_static_complement(h, a.ctypes.data_as(C.c_void_p), C.c_size_t(len(a)), 0, None, C.c_size_t(3), 0, None, C.c_size_t(0),
                                            C.byref(c)) == E_INVALID
    # a step in flight: the NOFLY guard
    sc = scenarios.small()
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    for call in (lambda: g.label_map(a, a, 0.2), lambda: g.static_complement(a, a)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            call()
        assert e.value.rc == E_STATE
    g.step_wait()
    g.static_complement(a, a)
    # the header's layout
    for R, name, fields in ((gpu_mod.LabelResult, "erasor_label_result", LABEL_FIELDS), (gpu_mod.ComplementResult, "erasor_complement_result",
                                                                                         COMPLEMENT_FIELDS)):
        offs = ", ".join("offsetof(%s, %s)" % (name, k) for k in fields)
        code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu' + ' %zu' * len(fields) + '\\n", '
                'sizeof(' + name + '), ' + offs + ');return 0;}\n')
        src, exe = tmp_path / (name + ".c"), tmp_path / name
        src.write_text(code)
        subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
        got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
        assert got == [C.sizeof(R)] + [getattr(R, k).offset for k in fields], name


def read_ascii_pcd(path):
    lines = open(path).read().splitlines()
    k = lines.index("DATA ascii")
    assert lines[k - 1] == "POINTS %d" % (len(lines) - k - 1)
    return np.array([[float(v) for v in l.split()] for l in lines[k + 1:]], np.float64).reshape(-1, 4)


def as_printed(rows):
    """rows as save_pcd_ascii prints them (%.8g) and a reader parses them back"""
    return np.array([[float("%.8g" % v) for v in r] for r in np.asarray(rows, np.float32).astype(np.float64)]).reshape(-1, 4)


def test_offline_driver_label_and_complement_modes(gpu_mod, tmp_path):
    shim_dir = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
    shim = C.CDLL(os.path.join(shim_dir, "liberasor_shim.so"))
    shim.erasor_shim_save_pcd.argtypes = [C.c_char_p, C.c_void_p, C.c_long, C.c_int]
    shim.erasor_shim_save_pcd.restype = C.c_int
    demo = os.path.join(shim_dir, "erasor_offline_demo")
    rng = np.random.default_rng(43)
    medium = xyzi(rng.uniform(-10, 10, (4000, 3)), rng.integers(1, 260, 4000))
    mp = medium.copy()
    mp[:, :3] += rng.normal(0, 0.05, (len(mp), 3)).astype(np.float32)
    mp = np.ascontiguousarray(mp[rng.random(len(mp)) < 0.8])
    mp[:, 3] = 0.0
    fm, fd = tmp_path / "method_map.pcd", tmp_path / "dense.pcd"
    assert shim.erasor_shim_save_pcd(str(fm).encode(), mp.ctypes.data, len(mp), 1) == 0
    assert shim.erasor_shim_save_pcd(str(fd).encode(), medium.ctypes.data, len(medium), 1) == 0
    for leaf in (None, 0.5):
        out = subprocess.run([demo, "--label", str(fm), str(fd)] + ([] if leaf is None else [repr(leaf)]), capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        ref, info = label_oracle(mp, medium, 0.2 if leaf is None else leaf)
        assert out.stdout.splitlines()[0] == "%d - > %d" % (len(mp), len(ref)), out.stdout
        got = read_ascii_pcd(tmp_path / "method_map_w_label.pcd")
        assert got.shape == ref.shape and (got == as_printed(ref)).all()
    fl, fo = tmp_path / "method_map_w_label.pcd", tmp_path / "lost.pcd"
    labelled = np.ascontiguousarray(read_ascii_pcd(fl).astype(np.float32))
    out = subprocess.run([demo, "--complement", str(fl), str(fd), str(fo)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    ref, info = evalmap.static_complement(labelled, medium)
    assert out.stdout.splitlines()[0] == "%d of %d static ground-truth point(s) lost" % (info["n_lost"], info["n_gt_static"]), out.stdout
    got = read_ascii_pcd(fo)
    assert info["n_lost"] > 0 and got.shape == ref.shape and (got == as_printed(ref)).all()


# ---- 8. full size: the bench's world ----
@pytest.mark.timeout(900)
def test_full_size_label_map_and_complement_match_the_oracle(gpu_mod):
    w = synth.World(seed=20210305 + 5, length=1000.0, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    m = w.sample_map(spacing=0.2, frames=range(0, 320, 2))
    assert len(m) > 9_000_000
    dense = w.sample_map(spacing=0.15, frames=range(0, 320, 2), x_range=(0.0, 1000.0))  # (the labelled sample: denser, another jitter)
    src = m.copy()
    src[:, 3] = 0.0
    g = gpu_mod.Erasor(gpu_mod.params_default())
    ps, pd = g.device_array(src), g.device_array(dense)
    try:
        g.label_map((ps, len(src)), (pd, len(dense)), 0.2)  # (first calls: allocations)
        t0 = time.perf_counter()
        rows, info = g.label_map((ps, len(src)), (pd, len(dense)), 0.2)
        t_lm = time.perf_counter() - t0
        g.static_complement((ps, len(src)), (pd, len(dense)))
        t0 = time.perf_counter()
        lost, cinfo = g.static_complement((ps, len(src)), (pd, len(dense)))
        t_cp = time.perf_counter() - t0
    finally:
        g.device_free(ps)
        g.device_free(pd)
    t0 = time.perf_counter()
    ref, ref_info = label_oracle(src, dense, 0.2)
    t_lm_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref_lost, ref_cinfo = evalmap.static_complement(src, dense)
    t_cp_host = time.perf_counter() - t0
    print("\nfull size: %d-pt map, %d-pt labelled sample: label_map %.1f ms (host oracle %.1f ms), static_complement %.1f ms "
          "(host oracle %.1f ms)\n%s\n%s" % (len(src), len(dense), t_lm * 1e3, t_lm_host * 1e3, t_cp * 1e3, t_cp_host * 1e3, info, cinfo))
    assert {k: info[k] for k in LABEL_FIELDS} == {k: ref_info[k] for k in LABEL_FIELDS}
    assert (bits(rows) == bits(ref)).all()
    assert cinfo == ref_cinfo and (bits(lost) == bits(ref_lost)).all()
    assert info["n_out"] < len(src) and 0 < cinfo["n_lost"] < cinfo["n_gt_static"]
