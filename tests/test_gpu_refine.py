"""Every frame's pose refined against the map on the device (erasor_hip_refine_poses_clouds / _map, kernels in refine.hip.h) against the
host restatement evalmap.refine_poses: the poses, the rows and the summary byte for byte -- on the small world with host and device scans
and both kinds of map, at every frame size around the wavefront and chunk boundaries, on ties, at the gate itself, with a frozen frame
beside a running one, with dropped points, too few pairs and a degenerate map; steps and tickets after the call, errors and the struct
layout.  tests/test_refine_on_cpu.py re-runs this file against the CPU stand-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_world as rw
import scenarios
from erasor_amd import evalmap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the CPU stand-in runs the kernels four to five orders of magnitude slower: thinner scans there, the same code paths
ON_CPU = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


@pytest.fixture(scope="module")
def small_world():
    """the map, the scans, the true and the given poses, and the restatement's answer (computed once)"""
    m = rw.world()
    scans, T_true, T_given = rw.frames(m, n_frames=3 if ON_CPU else 6, every=24 if ON_CPU else 1)
    kw = dict(max_iters=4) if ON_CPU else {}
    return m, scans, T_true, T_given, kw, evalmap.refine_poses(m[:, :3], scans, T_given, **kw)


def bits(x):
    return np.float64(x).tobytes()


def same_bits(a, b):
    return bits(a) == bits(b) or (np.isnan(a) and np.isnan(b))  # (a NaN's sign and payload are not part of the contract)


def assert_same(got, ref, what=""):
    (T, rows, summ), (rT, rrows, rsumm) = got, ref
    assert T.shape == rT.shape and len(rows) == len(rrows), what
    for f in range(len(rows)):
        for k in evalmap.REFINE_ROW_FIELDS:
            assert type(rows[f][k]) is type(rrows[f][k]) and same_bits(rows[f][k], rrows[f][k]), (what, "frame", f, k, rows[f][k], rrows[f][k])
        assert all(same_bits(a, b) for a, b in zip(T[f].reshape(-1), rT[f].reshape(-1))), (what, "frame", f, "T", T[f], rT[f], rows[f], rrows[f])
    assert list(summ) == list(evalmap.REFINE_SUMMARY_FIELDS)
    for k in evalmap.REFINE_SUMMARY_FIELDS:
        a, b = np.asarray(summ[k], np.float64).reshape(-1), np.asarray(rsumm[k], np.float64).reshape(-1)
        assert len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b)), (what, "summary", k, summ[k], rsumm[k])


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.full((len(xyz), 1), w, np.float32)], 1)


def widened(T):
    return np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)


# ---- 1. the small world ----
@pytest.mark.parametrize("device_scans", [False, True])
@pytest.mark.parametrize("against", ["clouds", "map"])
def test_small_world_matches_the_host_restatement(gpu_mod, small_world, against, device_scans):
    m, scans, T_true, T_given, kw, ref = small_world
    g = gpu_mod.Erasor(gpu_mod.params_default())
    if against == "map":
        g.set_map(m)
    mm = None if against == "map" else m
    if device_scans:
        offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])])
        p = g.device_array(np.concatenate(scans))
        try:
            got = g.refine_poses((p, offs), T_given, map=mm, **kw)
        finally:
            g.device_free(p)
    else:
        got = g.refine_poses(scans, T_given, map=mm, **kw)
    assert_same(got, ref, (against, device_scans))
    if not ON_CPU:  # (what the call is for: the restatement's own recovery is tests/test_evalmap_refine.py's)
        assert got[2]["n_status"] == [len(scans), 0, 0, 0]
        assert max(rw.pose_error(got[0][f], T_true[f])[0] for f in range(len(scans))) < 1e-6


# ---- 2. every frame size around the wavefront and chunk boundaries, in one call ----
SIZES = (1, 63, 0, 64, 65, 255, 256, 257, 511, 512, 513, 1025)


def test_frame_sizes_in_one_call(handle):
    ends = np.cumsum(SIZES)
    assert sorted(SIZES) == [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025] and not any(e % 256 == 0 for e in ends)
    rng = np.random.default_rng(17)
    m = xyzi(np.concatenate([rng.uniform(-8, 8, (3000, 3)) * [1, 1, 0.01], rng.uniform(-8, 8, (1500, 3)) * [0.01, 1, 0.3] + [8, 0, 2.4],
                             rng.uniform(-8, 8, (1500, 3)) * [1, 0.01, 0.3] + [0, 8, 2.4]]))
    scans, poses = [], []
    for n in SIZES:
        Tt = rw.pose(rw.rot(0.0, 0.01, rng.uniform(-3, 3)), rng.uniform(-1, 1, 3))
        sub = m[rng.choice(len(m), n, replace=False), :3].astype(np.float64)
        scans.append(xyzi((sub - Tt[:3, 3]) @ Tt[:3, :3]).reshape(-1, 4))
        poses.append((rw.pose(rw.rot(0.004, -0.006, 0.008), [0.05, -0.04, 0.03]) @ Tt).astype(np.float32))
    Tl = np.eye(4, dtype=np.float32)
    Tl[2, 3] = 0.25
    for T_l2b, iters in ((None, 3), (Tl, 1)):
        kw = dict(max_dist=0.6, max_iters=iters, min_pairs=1)
        got = handle.refine_poses(scans, poses, T_l2b, map=m, **kw)
        assert_same(got, evalmap.refine_poses(m[:, :3], scans, poses, T_l2b, **kw), ("sizes", iters))
    rows = got[1]
    assert [r["n_points"] for r in rows] == list(SIZES) and rows[2]["status"] == 3 and rows[2]["iters"] == 0
    assert all(r["n_pairs_first"] > 0 for f, r in enumerate(rows) if SIZES[f] >= 63)


# ---- 3. ties: the lowest map index wins ----
def test_ties_go_to_the_lowest_map_index(handle):
    g = np.arange(5.0)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[np.random.default_rng(6).permutation(len(lattice))]  # (so that the lowest index is no corner in particular)
    c = np.arange(4.0) + 0.5
    cells = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)                 # 8 map points at d2 = 0.75
    faces = np.stack(np.meshgrid(c, np.arange(1.0, 4.0), np.arange(1.0, 4.0), indexing="ij"), -1).reshape(-1, 3)  # 2 at d2 = 0.25
    scans = [xyzi(cells), xyzi(faces), xyzi(np.concatenate([faces[:, [1, 0, 2]], cells, faces[:, [2, 1, 0]]]))]
    poses = [np.eye(4, dtype=np.float32)] * 3
    kw = dict(max_dist=1.0, max_iters=2, min_pairs=1)
    ref = evalmap.refine_poses(lattice, scans, poses, **kw)
    assert_same(handle.refine_poses(scans, poses, map=xyzi(lattice), **kw), ref, "ties")
    assert [r["n_pairs_first"] for r in ref[1]] == [64, 36, 136] and bits(ref[1][0]["rms_first"]) == bits(np.sqrt(0.75))
    # the tie rule is in the answer: the highest index instead gives other poses

    def highest(map64, tree, q):
        d2 = evalmap.pair_d2(q[:, None, :], map64[None, :, :])
        j = d2.shape[1] - 1 - np.argmin(d2[:, ::-1], axis=1)
        return d2[np.arange(len(q)), j], j

    other = evalmap.refine_poses(lattice, scans, poses, nearest=highest, **kw)
    assert other[0].tobytes() != ref[0].tobytes()


# ---- 4. the gate itself: d2 == max_dist^2, one float64 step below, one above ----
def f32_near(x, span):
    """the float32 values from `span` steps below x to `span` above"""
    x = np.float32(x)
    lo = x
    for _ in range(span):
        lo = np.nextafter(lo, np.float32(-np.inf))
    out = [lo]
    for _ in range(2 * span):
        out.append(np.nextafter(out[-1], np.float32(np.inf)))
    return out


def point_at_d2(x, target):
    """a float32 point (x, y, z) whose d2 from the origin, (x*x + y*y) + z*z in float64, is exactly `target` (>= x*x)"""
    x = float(np.float32(x))
    for y in f32_near(np.sqrt(max(target - x * x, 0.0)), 3):
        s = x * x + float(y) * float(y)
        if s > target:
            continue
        for z in f32_near(np.sqrt(target - s), 40):
            if s + float(z) * float(z) == target:
                return [x, float(y), float(z)]
    raise AssertionError("no float32 point at that d2")


def test_the_gate_counts_a_pair_at_exactly_max_dist(handle):
    max_dist = 1.5
    gate2 = max_dist * max_dist
    below, above = float(np.nextafter(gate2, 0.0)), float(np.nextafter(gate2, np.inf))
    at = [1.5, 0.0, 0.0]
    lo = point_at_d2(np.nextafter(np.float32(1.5), np.float32(0)), below)
    hi = point_at_d2(1.5, above)
    for pt, want in ((at, gate2), (lo, below), (hi, above)):
        assert (pt[0] * pt[0] + pt[1] * pt[1]) + pt[2] * pt[2] == want and want in (gate2, below, above)
    m = xyzi([[0.0, 0.0, 0.0]])  # a lone map point
    scans = [xyzi([at]), xyzi([lo]), xyzi([hi]), xyzi([hi, at, lo, hi]), xyzi([np.negative(hi), hi])]
    poses = [np.eye(4, dtype=np.float32)] * len(scans)
    kw = dict(max_dist=max_dist, max_iters=2, min_pairs=1)
    ref = evalmap.refine_poses(m[:, :3], scans, poses, **kw)
    got = handle.refine_poses(scans, poses, map=m, **kw)
    assert_same(got, ref, "gate")
    assert [r["n_pairs_first"] for r in got[1]] == [1, 1, 0, 2, 0]
    # (frame 3's second update, with all four points paired, is `lo`'s 6e-4 m off the axis: parity only)
    assert [got[1][f]["status"] for f in (0, 1, 2, 4)] == [0, 0, 2, 2] and got[1][3]["n_pairs_last"] == 4
    assert bits(got[1][0]["rms_first"]) == bits(1.5) and got[1][0]["rms_last"] == 0.0  # (one pair: the update puts it on the map point)


# ---- 5. stopping: a frame that ends at once beside one that runs to the limit ----
def test_a_frozen_frame_beside_a_running_one(handle):
    m = rw.world()[::7 if ON_CPU else 2]
    exact = m[np.random.default_rng(2).choice(len(m), 700, replace=False)]  # the map's own points under the identity: nothing to correct
    scans, T_true, T_given = rw.frames(m, n_frames=1, every=8 if ON_CPU else 2)
    ident = np.eye(4, dtype=np.float32)
    kw = dict(max_iters=3, eps_t=1e-12, eps_r=1e-12)
    ref = evalmap.refine_poses(m[:, :3], [exact, scans[0]], [ident, T_given[0]], **kw)
    got = handle.refine_poses([exact, scans[0]], [ident, T_given[0]], map=m, **kw)
    assert_same(got, ref, "frozen + running")
    T, rows, summ = got
    assert rows[0]["status"] == 0 and rows[0]["iters"] == 1 and rows[1]["status"] == 1 and rows[1]["iters"] == 3 and summ["n_status"] == [1, 1, 0, 0]
    assert T[0].tobytes() == np.eye(4).tobytes() and rows[0]["moved_t"] == 0.0 and rows[0]["moved_r"] == 0.0 and rows[0]["rms_last"] == 0.0
    assert rows[1]["rms_last"] < rows[1]["rms_first"]
    # the frozen frame's row is the row it has alone, and after one iteration: the other frame's later iterations did not touch it
    for frames, poses, k in (([exact], [ident], kw), ([exact, scans[0]], [ident, T_given[0]], dict(kw, max_iters=1))):
        T1, rows1, _ = handle.refine_poses(frames, poses, map=m, **k)
        assert T1[0].tobytes() == T[0].tobytes() and str(rows1[0]) == str(rows[0])


# ---- 6. rows and poses that are not finite, too few pairs, a degenerate map ----
def test_non_finite_rows_and_poses_are_dropped_and_counted(handle):
    rng = np.random.default_rng(5)
    m = xyzi(rng.uniform(-6, 6, (4000, 3)) * [1, 1, 0.2])
    pts = m[rng.choice(len(m), 300, replace=False)].copy()
    pts[:, :3] += np.float32(0.02)
    holes = pts.copy()
    holes[::7, 1] = np.nan
    holes[3::11, 2] = np.inf
    holes[5, 0] = -np.inf
    inf_pose = np.eye(4, dtype=np.float32)
    inf_pose[1, 3] = np.inf
    big = np.eye(4, dtype=np.float32)  # (the pose is applied in float64: only an infinite entry takes a point's query away)
    big[0, 0] = -np.inf
    ident = np.eye(4, dtype=np.float32)
    scans = [holes, pts, np.full((5, 4), np.nan, np.float32), pts[:100], pts]
    poses = [ident, inf_pose, ident, big, ident]
    kw = dict(max_dist=0.5, max_iters=3, min_pairs=20)
    ref = evalmap.refine_poses(m[:, :3], scans, poses, **kw)
    got = handle.refine_poses(scans, poses, map=m, **kw)
    assert_same(got, ref, "non-finite")
    T, rows, summ = got
    n_bad = int((~np.isfinite(holes[:, :3]).all(1)).sum())
    assert [r["n_non_finite"] for r in rows] == [n_bad, 300, 5, 100, 0] and n_bad > 60
    assert [r["status"] for r in rows] == [ref[1][0]["status"], 3, 3, 3, ref[1][4]["status"]] and rows[0]["status"] in (0, 1)
    assert rows[0]["n_pairs_first"] == 300 - n_bad and rows[4]["n_pairs_first"] == 300
    for f in (1, 2, 3):  # the pose as given, widened
        assert T[f].tobytes() == widened(poses[f]).tobytes() and rows[f]["iters"] == 0 and np.isnan(rows[f]["rms_first"])
    assert summ["n_status"][3] == 3


def test_a_frame_far_from_the_map_keeps_its_pose(handle):
    rng = np.random.default_rng(12)
    m = xyzi(rng.uniform(-5, 5, (2000, 3)))
    near = m[:400].copy()
    far = m[400:700].copy()
    far[:, 0] += np.float32(100.0)
    T_far = rw.pose(rw.rot(0.01, 0.02, 0.3), [0.123456789, -0.2, 0.05]).astype(np.float32)
    kw = dict(max_dist=1.0, max_iters=2)
    got = handle.refine_poses([far, near, near[:99]], [T_far, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)], map=m, **kw)
    assert_same(got, evalmap.refine_poses(m[:, :3], [far, near, near[:99]], [T_far, np.eye(4), np.eye(4)], **kw), "far")
    T, rows, summ = got
    assert rows[0]["status"] == 2 and rows[0]["n_pairs_first"] == 0 and rows[0]["n_non_finite"] == 0 and T[0].tobytes() == widened(T_far).tobytes()
    assert rows[1]["status"] == 0 and rows[2]["status"] == 2 and rows[2]["n_pairs_first"] == 99  # (the default min_pairs: 100)
    assert rows[2]["rms_first"] == 0.0 and T[2].tobytes() == np.eye(4).tobytes()


def test_a_single_plane_map_parity_only(handle):
    rng = np.random.default_rng(30)
    m = xyzi(np.concatenate([rng.uniform(-6, 6, (3000, 2)), np.zeros((3000, 1))], 1))
    scans, poses = [], []
    for n in (500, 300):
        sub = m[rng.choice(len(m), n, replace=False), :3].astype(np.float64)
        scans.append(xyzi(sub))
        poses.append(rw.pose(rw.rot(0.01, -0.01, 0.01), [0.05, 0.03, 0.04]).astype(np.float32))
    kw = dict(max_dist=0.5, max_iters=4, min_pairs=10)
    assert_same(handle.refine_poses(scans, poses, map=m, **kw), evalmap.refine_poses(m[:, :3], scans, poses, **kw), "plane")


# ---- 7. no side effects on the run ----
def test_refine_between_steps_leaves_later_steps_and_tickets_intact(gpu_mod):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import orc
    from test_gpu_parity import compare_step
    sc = scenarios.small()
    g, o = gpu_mod.Erasor(scenarios.to_product_params(sc["params"])), orc.Oracle(sc["params"])
    g.set_map(sc["map"])
    o.set_map(sc["map"])
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
    n, ahead = len(scans), 2
    Tl, Tb, To = sc["T_l2b"], sc["T_b2o"], sc["T_o2b"]
    kw = dict(max_iters=2, max_dist=0.5)
    tickets = {}
    for j in range(ahead):
        tickets[j] = g.prefetch_node_rows(scans[j], 3, Tl, Tb[j], To[j])
    for k in range(n):
        if k + ahead < n:
            tickets[k + ahead] = g.prefetch_node_rows(scans[k + ahead], 3, Tl, Tb[k + ahead], To[k + ahead])
        if k % 3 == 0:  # with nodes announced ahead: the call works in the evaluator's scratch, its tree sort in a radix bank of its own
            some = [k, min(n - 1, k + 1)]
            got = g.refine_poses([scans[f][::4] for f in some], [Tb[f] for f in some], Tl, **kw)
            assert_same(got, evalmap.refine_poses(o.get_map()[:, :3], [scans[f][::4] for f in some], [Tb[f] for f in some], Tl, **kw), ("step", k))
        rg = g.step_ticket(tickets.pop(k), Tb[k], To[k])
        ro = o.step(scans[k], Tl, Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
    assert g.get_map().shape == o.get_map().shape


# ---- 8. errors and the struct layout ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    E_INVALID, E_STATE = -1, -4
    lib = gpu_mod.lib()
    g = gpu_mod.Erasor(gpu_mod.params_default())
    rng = np.random.default_rng(2)
    m = xyzi(rng.uniform(-3, 3, (100, 3)))
    scans = [xyzi(rng.uniform(-3, 3, (n, 3))) for n in (10, 20)]
    poses = [np.eye(4, dtype=np.float32)] * 2

    def refused(rc, *a, **kw):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.refine_poses(*a, **kw)
        assert e.value.rc == rc, str(e.value)
        return str(e.value)

    for it in (0, 65, 1000):
        assert "max_iters" in refused(E_INVALID, scans, poses, map=m, max_iters=it)
    for name in ("max_dist", "eps_t", "eps_r"):
        for v in (0.0, -0.5, float("nan"), float("inf")):
            assert name in refused(E_INVALID, scans, poses, map=m, **{name: v})
    Tl = np.eye(4, dtype=np.float32)
    Tl[0, 0] = np.inf
    assert "T_lidar2body" in refused(E_INVALID, scans, poses, Tl, map=m)
    bad_map = m.copy()
    bad_map[3, 0] = np.nan
    assert "non-finite" in refused(E_INVALID, scans, poses, map=bad_map)
    assert "empty map" in refused(E_INVALID, scans, poses, map=np.zeros((0, 4), np.float32))
    # the offsets and the optional outputs, through the C ABI
    cat = np.ascontiguousarray(np.concatenate(scans))
    rows = (gpu_mod.RefineRow * 4)()
    Tb = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (4, 1))
    summ = gpu_mod.RefineSummary()
    prm = gpu_mod.RefineParams(1.0, 1e-4, 1e-5, 2, 1)

    def call(offs, n_pts=len(cat), rows=rows, summ=C.byref(summ), prm=C.byref(prm)):
        offs = np.ascontiguousarray(offs, np.uint64)
        return lib.erasor_hip_refine_poses_clouds(g._h, m.ctypes.data_as(C.c_void_p), C.c_size_t(len(m)), C.c_int(0), cat.ctypes.data_as(C.c_void_p),
                                                  C.c_size_t(n_pts), offs.ctypes.data_as(C.c_void_p), C.c_size_t(len(offs) - 1), C.c_int(0), None,
                                                  Tb.ctypes.data_as(C.c_void_p), prm, rows, summ)

    def message():
        return lib.erasor_hip_last_error(g._h).decode()

    assert call([0, 10, 30]) == 0 and rows[1].n_points == 20 and summ.n_frames == 2 and rows[0].T[15] == 1.0
    assert call([0, 10, 30], rows=None) == 0 and call([0, 10, 30], summ=None) == 0 and call([0, 10, 30], rows=None, summ=None) == 0
    assert call([0, 10, 30], prm=None) == E_INVALID and "params" in message()
    assert call([1, 10, 30]) == E_INVALID and "offsets" in message()
    assert call([0, 20, 10, 30]) == E_INVALID and "offsets decrease" in message()
    assert call([0, 10, 29]) == E_INVALID and "last offset" in message()
    assert call([0, 10, 30], n_pts=2**30) == E_INVALID and message()
    assert call([0], n_pts=0) == 0 and summ.n_frames == 0  # no frames: nothing to do
    # the handle's map: none yet
    assert "no map" in refused(E_STATE, scans, poses)
    # a step in flight: the NOFLY guard
    sc = scenarios.small(n_frames=2, az=60)
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    refused(E_STATE, scans, poses)
    refused(E_STATE, scans, poses, map=m)
    g.step_wait()
    T, rows2, _ = g.refine_poses(scans, poses, map=m, min_pairs=1, max_iters=1)  # the handle is fine after the refusals
    assert [r["n_points"] for r in rows2] == [10, 20]
    # the header's layout
    R, P, S = gpu_mod.RefineRow, gpu_mod.RefineParams, gpu_mod.RefineSummary
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
            'sizeof(erasor_refine_row), sizeof(erasor_refine_params), sizeof(erasor_refine_summary), offsetof(erasor_refine_row, status), '
            'offsetof(erasor_refine_row, n_points), offsetof(erasor_refine_row, rms_first), offsetof(erasor_refine_row, moved_r), '
            'offsetof(erasor_refine_params, max_iters), offsetof(erasor_refine_summary, sum_d2_first));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(R), C.sizeof(P), C.sizeof(S), R.status.offset, R.n_points.offset, R.rms_first.offset, R.moved_r.offset, P.max_iters.offset,
                   S.sum_d2_first.offset]
