"""Every frame's pose refined point-to-plane against the map's normals on the device (erasor_hip_refine_poses_plane_clouds / _map, kernel
in refine_plane.hip.h) against the host restatement evalmap.refine_poses_plane: the poses, the rows and the summary byte for byte -- on the
designed lattices with host and device scans and both kinds of map, at every frame size around the wavefront and chunk boundaries, at the
curvature gate itself, on map points without a normal, with a frozen frame beside a running one, with dropped points and a far frame, on
a frame that constrains one direction only, on ties; steps and tickets after the call, errors and the struct layout.
tests/test_refine_plane_on_cpu.py re-runs this file against the CPU stand-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_plane_world as pw
import refine_world as rw
import scenarios
from erasor_amd import evalmap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the CPU stand-in runs the kernels four to five orders of magnitude slower: smaller maps there, the same code paths
ON_CPU = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))
xyzi = pw.xyzi


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def three_planes(side):
    return pw.lattices(side)["three perpendicular planes"][0]


def bits(x):
    return np.float64(x).tobytes()


def same_bits(a, b):
    return bits(a) == bits(b) or (np.isnan(a) and np.isnan(b))  # (a NaN's sign and payload are not part of the contract)


def assert_same(got, ref, what=""):
    (T, rows, summ), (rT, rrows, rsumm) = got, ref
    assert T.shape == rT.shape and len(rows) == len(rrows), what
    for f in range(len(rows)):
        assert list(rows[f]) == list(evalmap.REFINE_PLANE_ROW_FIELDS)
        for k in evalmap.REFINE_PLANE_ROW_FIELDS:
            assert type(rows[f][k]) is type(rrows[f][k]) and same_bits(rows[f][k], rrows[f][k]), (what, "frame", f, k, rows[f][k], rrows[f][k])
        assert all(same_bits(a, b) for a, b in zip(T[f].reshape(-1), rT[f].reshape(-1))), (what, "frame", f, "T", T[f], rT[f], rows[f], rrows[f])
    assert list(summ) == list(evalmap.REFINE_PLANE_SUMMARY_FIELDS)
    for k in evalmap.REFINE_PLANE_SUMMARY_FIELDS:
        a, b = np.asarray(summ[k], np.float64).reshape(-1), np.asarray(rsumm[k], np.float64).reshape(-1)
        assert len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b)), (what, "summary", k, summ[k], rsumm[k])


def widened(T):
    return np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)


# ---- 1. the designed lattices: ranks 3, 3, 5 and 6 ----
KW = dict(k=8, max_dist=0.5)


@pytest.fixture(scope="module")
def lattice_refs():
    """name -> (map XYZI, scan, T_given, rank, the restatement's answer), computed once"""
    out = {}
    for name, (m, rank) in pw.lattices().items():
        scan, Tg = pw.own_points_scan(m)
        out[name] = (xyzi(m), scan, Tg, rank, evalmap.refine_poses_plane(m, [scan], [Tg], **KW))
    return out


@pytest.mark.parametrize("device_scans", [False, True])
@pytest.mark.parametrize("against", ["clouds", "map"])
def test_lattices_match_the_host_restatement(gpu_mod, lattice_refs, against, device_scans):
    for name, (m, scan, Tg, rank, ref) in lattice_refs.items():
        assert 576 <= len(m) <= 1728
        g = gpu_mod.Erasor(gpu_mod.params_default())
        if against == "map":
            g.set_map(m)
        mm = None if against == "map" else m
        if device_scans:
            p = g.device_array(scan)
            try:
                got = g.refine_poses_plane((p, np.array([0, len(scan)])), [Tg], map=mm, **KW)
            finally:
                g.device_free(p)
        else:
            got = g.refine_poses_plane([scan], [Tg], map=mm, **KW)
        assert_same(got, ref, (name, against, device_scans))
        assert got[1][0]["rank"] == rank and got[1][0]["status"] == 0 and got[2]["n_map_no_normal"] == 0


# ---- 2. every frame size around the wavefront and chunk boundaries, in one call ----
SIZES = (1, 63, 0, 64, 65, 255, 256, 257, 511, 512, 513, 1025)


def test_frame_sizes_in_one_call(handle):
    ends = np.cumsum(SIZES)
    assert sorted(SIZES) == [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025] and not any(e % 256 == 0 for e in ends)
    rng = np.random.default_rng(17)
    m = xyzi(three_planes(30 if ON_CPU else 45))  # 6 075 map points (2 700 on the stand-in)
    scans, poses = [], []
    for n in SIZES:
        Tt = rw.pose(rw.rot(0.0, 0.01, rng.uniform(-3, 3)), rng.uniform(-1, 1, 3))
        sub = m[rng.choice(len(m), n, replace=False), :3].astype(np.float64)
        scans.append(xyzi((sub - Tt[:3, 3]) @ Tt[:3, :3]).reshape(-1, 4))
        poses.append((rw.pose(rw.rot(0.004, -0.006, 0.008), [0.05, -0.04, 0.03]) @ Tt).astype(np.float32))
    Tl = np.eye(4, dtype=np.float32)
    Tl[2, 3] = 0.25
    for T_l2b, iters in ((None, 3), (Tl, 1)):
        kw = dict(k=8, max_dist=0.6, max_iters=iters, min_pairs=1)
        got = handle.refine_poses_plane(scans, poses, T_l2b, map=m, **kw)
        assert_same(got, evalmap.refine_poses_plane(m[:, :3], scans, poses, T_l2b, **kw), ("sizes", iters))
    rows = got[1]
    assert [r["n_points"] for r in rows] == list(SIZES) and rows[2]["status"] == 3 and rows[2]["iters"] == 0 and rows[2]["rank"] == 0
    assert all(r["n_pairs_first"] > 0 for f, r in enumerate(rows) if SIZES[f] >= 63)


# ---- 3. the curvature gate itself: max_curvature at one map point's curvature, one float64 step below, one above ----
def test_the_curvature_gate_at_one_map_points_curvature(handle):
    rng = np.random.default_rng(23)
    ball = rng.normal(size=(300, 3))
    ball = ball / np.linalg.norm(ball, axis=1)[:, None] * rng.uniform(0.0, 1.0, (300, 1)) ** (1 / 3) * 1.5 + [3.0, 3.0, 4.0]
    planes = three_planes(16 if ON_CPU else 24)
    m = xyzi(np.concatenate([planes, ball]))
    _, curv, _, _ = evalmap.normals(m, 8)
    cb = curv[len(planes):]
    star = len(planes) + int(np.argsort(cb)[len(cb) // 2])  # the ball's median curvature: points on either side of it
    c_at = float(curv[star])
    assert 0.0 < c_at < 1 / 3 and (curv == c_at).sum() == 1
    c_below, c_above = float(np.nextafter(c_at, 0.0)), float(np.nextafter(c_at, 1.0))
    # the scan: the map's own points under the identity, and three more beside the chosen one
    extra = m[star, :3] + np.float32(1e-3) * np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    scan = xyzi(np.concatenate([m[:, :3], extra]))
    m64 = m[:, :3].astype(np.float64)
    d2, j = evalmap.nearest_f64(m64, evalmap.cKDTree(m64), scan[:, :3].astype(np.float64))
    n_star = int(((j == star) & (d2 <= 0.25)).sum())
    assert n_star == 4
    ident = [np.eye(4, dtype=np.float32)]
    got = {}
    for c in (c_below, c_at, c_above):
        kw = dict(k=8, max_dist=0.5, max_curvature=c, max_iters=1, min_pairs=1)
        got[c] = handle.refine_poses_plane([scan], ident, map=m, **kw)
        assert_same(got[c], evalmap.refine_poses_plane(m[:, :3], [scan], ident, **kw), ("curvature", c))
    u = {c: got[c][1][0]["n_unusable_first"] for c in got}
    p = {c: got[c][1][0]["n_pairs_first"] for c in got}
    assert u[c_below] - u[c_at] == n_star == p[c_at] - p[c_below] and u[c_at] == u[c_above] and p[c_at] == p[c_above]
    assert u[c_at] == int((cb > c_at).sum()) > 100 and p[c_at] + u[c_at] == len(scan)


# ---- 4. map points without a normal ----
def test_map_points_without_a_normal_are_unusable_and_counted(handle):
    k = 8
    planes = three_planes(12)
    clump = np.tile([[9.0, 9.0, 9.0]], (k + 1, 1))  # k + 1 identical points: each one's neighbourhood is the clump, its covariance zero
    m = xyzi(np.concatenate([planes[:200], clump, planes[200:]]))
    rng = np.random.default_rng(3)
    on_planes = m[rng.choice(len(m), 300, replace=False)].copy()
    on_clump = xyzi(np.array([9.0, 9.0, 9.0]) + rng.uniform(-0.1, 0.1, (40, 3)))
    scans = [np.concatenate([on_planes[:150], on_clump, on_planes[150:]]), on_clump, on_planes]
    poses = [np.eye(4, dtype=np.float32)] * 3
    kw = dict(k=k, max_dist=0.5, max_iters=2, min_pairs=1)
    ref = evalmap.refine_poses_plane(m[:, :3], scans, poses, **kw)
    got = handle.refine_poses_plane(scans, poses, map=m, **kw)
    assert_same(got, ref, "clump")
    T, rows, summ = got
    n_on_clump = int((on_planes[:, 0] == 9.0).sum())
    assert summ["n_map_no_normal"] == k + 1
    assert rows[0]["n_unusable_first"] == 40 + n_on_clump and rows[0]["n_pairs_first"] == 300 - n_on_clump
    assert rows[1]["n_unusable_first"] == 40 and rows[1]["n_pairs_first"] == 0 and rows[1]["status"] == 2 and rows[1]["rank"] == 0
    assert T[1].tobytes() == np.eye(4).tobytes() and rows[2]["n_unusable_first"] == n_on_clump
    # a map with no more points than k: no normal at all
    tiny = m[:k]
    ref = evalmap.refine_poses_plane(tiny[:, :3], [tiny, tiny[:3]], poses[:2], **kw)
    got = handle.refine_poses_plane([tiny, tiny[:3]], poses[:2], map=tiny, **kw)
    assert_same(got, ref, "no normals")
    assert got[2]["n_map_no_normal"] == k and got[2]["n_status"] == [0, 0, 2, 0, 0]
    assert [r["n_unusable_first"] for r in got[1]] == [k, 3] and [r["n_unusable_last"] for r in got[1]] == [k, 3]
    assert got[0][0].tobytes() == np.eye(4).tobytes()


# ---- 5. stopping: a frame that ends at once beside one that runs to the limit ----
def test_a_frozen_frame_beside_a_running_one(handle):
    m = xyzi(three_planes(16 if ON_CPU else 32))
    exact = m[np.random.default_rng(2).choice(len(m), 700, replace=False)]  # the map's own points under the identity: nothing to correct
    moved, T_given = pw.own_points_scan(m[:, :3], rows=slice(None, None, 3))
    ident = np.eye(4, dtype=np.float32)
    kw = dict(k=8, max_dist=0.5, max_iters=3, eps_t=1e-300, eps_r=1e-300)  # (only an update of exactly nothing ends a frame)
    ref = evalmap.refine_poses_plane(m[:, :3], [exact, moved], [ident, T_given], **kw)
    got = handle.refine_poses_plane([exact, moved], [ident, T_given], map=m, **kw)
    assert_same(got, ref, "frozen + running")
    T, rows, summ = got
    assert rows[0]["status"] == 0 and rows[0]["iters"] == 1 and rows[1]["status"] == 1 and rows[1]["iters"] == 3 and summ["n_status"] == [1, 1, 0, 0, 0]
    assert T[0].tobytes() == np.eye(4).tobytes() and rows[0]["moved_t"] == 0.0 and rows[0]["moved_r"] == 0.0 and rows[0]["rms_plane_last"] == 0.0
    assert rows[1]["rms_plane_last"] < rows[1]["rms_plane_first"] and rows[0]["rank"] == 6 == rows[1]["rank"]
    # the frozen frame's row is the row it has alone, and after one iteration: the other frame's later iterations did not touch it
    for frames, poses, k in (([exact], [ident], kw), ([exact, moved], [ident, T_given], dict(kw, max_iters=1))):
        T1, rows1, _ = handle.refine_poses_plane(frames, poses, map=m, **k)
        assert T1[0].tobytes() == T[0].tobytes() and str(rows1[0]) == str(rows[0])


# ---- 6. rows and poses that are not finite, a frame far from the map ----
def test_non_finite_rows_and_poses_are_dropped_and_counted(handle):
    rng = np.random.default_rng(5)
    m = xyzi(three_planes(16 if ON_CPU else 32))
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
    kw = dict(k=8, max_dist=0.5, max_iters=3, min_pairs=20)
    ref = evalmap.refine_poses_plane(m[:, :3], scans, poses, **kw)
    got = handle.refine_poses_plane(scans, poses, map=m, **kw)
    assert_same(got, ref, "non-finite")
    T, rows, summ = got
    n_bad = int((~np.isfinite(holes[:, :3]).all(1)).sum())
    assert [r["n_non_finite"] for r in rows] == [n_bad, 300, 5, 100, 0] and n_bad > 60
    assert [r["status"] for r in rows] == [ref[1][0]["status"], 3, 3, 3, ref[1][4]["status"]] and rows[0]["status"] in (0, 1)
    assert rows[0]["n_pairs_first"] == 300 - n_bad and rows[4]["n_pairs_first"] == 300
    for f in (1, 2, 3):  # the pose as given, widened
        assert T[f].tobytes() == widened(poses[f]).tobytes() and rows[f]["iters"] == 0 and np.isnan(rows[f]["rms_plane_first"]) and rows[f]["rank"] == 0
    assert summ["n_status"][3] == 3


def test_a_frame_far_from_the_map_keeps_its_pose(handle):
    m = xyzi(three_planes(16 if ON_CPU else 32))
    near = m[:400].copy()
    far = m[400:700].copy()
    far[:, 0] += np.float32(100.0)
    T_far = rw.pose(rw.rot(0.01, 0.02, 0.3), [0.123456789, -0.2, 0.05]).astype(np.float32)
    ident = np.eye(4, dtype=np.float32)
    kw = dict(k=8, max_dist=1.0, max_iters=2)
    got = handle.refine_poses_plane([far, near, near[:99]], [T_far, ident, ident], map=m, **kw)
    assert_same(got, evalmap.refine_poses_plane(m[:, :3], [far, near, near[:99]], [T_far, ident, ident], **kw), "far")
    T, rows, summ = got
    assert rows[0]["status"] == 2 and rows[0]["n_pairs_first"] == 0 and rows[0]["n_non_finite"] == 0 and T[0].tobytes() == widened(T_far).tobytes()
    assert rows[0]["rank"] == 0 and np.isnan(rows[0]["lambda_ratio"]) and rows[0]["n_unusable_first"] == 0
    assert rows[1]["status"] == 0 and rows[2]["status"] == 2 and rows[2]["n_pairs_first"] == 99  # (the default min_pairs: 100)
    assert rows[2]["rms_plane_first"] == 0.0 and T[2].tobytes() == np.eye(4).tobytes()


# ---- 7. a frame that constrains one direction only ----
def test_one_point_at_the_body_origin_moves_along_the_normal_only(handle):
    """ERASOR_REFINE_DEGENERATE needs a solve whose lambda_max is not > 0.  A pair's J holds its normal, a unit vector, so the trace of A
    is at least the number of pairs and float32 inputs cannot overflow a product: the status is not reachable through the interface
    (tests/test_evalmap_refine_plane.py solves all-zero sums directly).  The nearest thing is a frame of one point at the body origin on
    a map whose normal there is exactly (0, 0, 1): q' = 0, J = (0, 0, 0, 0, 0, 1), rank 1, and the update moves t along z only."""
    m = xyzi(pw.lattices()["one plane"][0])
    T0 = rw.pose(rw.rot(0.02, -0.01, 0.5), [1.1, 2.2, 0.0703125]).astype(np.float32)
    scan = xyzi([[0.0, 0.0, 0.0]])
    kw = dict(k=8, max_dist=0.5, min_pairs=1)
    ref = evalmap.refine_poses_plane(m[:, :3], [scan], [T0], **kw)
    got = handle.refine_poses_plane([scan], [T0], map=m, **kw)
    assert_same(got, ref, "one point")
    T, rows, summ = got
    r = rows[0]
    assert r["status"] == 0 and r["iters"] == 2 and r["rank"] == 1 and r["lambda_ratio"] == 0.0 and summ["n_status"] == [1, 0, 0, 0, 0]
    want = widened(T0)
    want[2, 3] = 0.0  # r = qz - 0 exactly, the update is -r, the second update is zero
    assert T[0].tobytes() == want.tobytes() and bits(r["moved_t"]) == bits(0.0703125)
    assert bits(r["rms_plane_first"]) == bits(0.0703125) and r["rms_plane_last"] == 0.0


# ---- 8. ties: the lowest map index wins ----
def test_ties_go_to_the_lowest_map_index(handle):
    g = np.arange(5.0)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lattice = lattice[np.random.default_rng(6).permutation(len(lattice))]  # (so that the lowest index is no corner in particular)
    c = np.arange(4.0) + 0.5
    cells = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)                 # 8 map points at d2 = 0.75
    faces = np.stack(np.meshgrid(c, np.arange(1.0, 4.0), np.arange(1.0, 4.0), indexing="ij"), -1).reshape(-1, 3)  # 2 at d2 = 0.25
    scans = [xyzi(cells), xyzi(faces), xyzi(np.concatenate([faces[:, [1, 0, 2]], cells, faces[:, [2, 1, 0]]]))]
    poses = [np.eye(4, dtype=np.float32)] * 3
    kw = dict(k=6, max_dist=1.0, max_iters=2, min_pairs=1)
    ref = evalmap.refine_poses_plane(lattice, scans, poses, **kw)
    assert_same(handle.refine_poses_plane(scans, poses, map=xyzi(lattice), **kw), ref, "ties")
    assert [r["n_pairs_first"] for r in ref[1]] == [64, 36, 136] and bits(ref[1][0]["rms_first"]) == bits(np.sqrt(0.75))
    # the tie rule is in the answer: the highest index instead gives other poses

    def highest(map64, tree, q):
        d2 = evalmap.pair_d2(q[:, None, :], map64[None, :, :])
        j = d2.shape[1] - 1 - np.argmin(d2[:, ::-1], axis=1)
        return d2[np.arange(len(q)), j], j

    other = evalmap.refine_poses_plane(lattice, scans, poses, nearest=highest, **kw)
    assert other[0].tobytes() != ref[0].tobytes()


# ---- 9. no side effects on the run ----
def test_refine_plane_between_steps_leaves_later_steps_and_tickets_intact(gpu_mod):
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
            got = g.refine_poses_plane([scans[f][::4] for f in some], [Tb[f] for f in some], Tl, **kw)
            assert_same(got, evalmap.refine_poses_plane(o.get_map()[:, :3], [scans[f][::4] for f in some], [Tb[f] for f in some], Tl, **kw), ("step", k))
        rg = g.step_ticket(tickets.pop(k), Tb[k], To[k])
        ro = o.step(scans[k], Tl, Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
    assert g.get_map().shape == o.get_map().shape


# ---- 10. errors and the struct layout ----
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
            g.refine_poses_plane(*a, **kw)
        assert e.value.rc == rc, str(e.value)
        return str(e.value)

    for it in (0, 65, 1000):
        assert "max_iters" in refused(E_INVALID, scans, poses, map=m, max_iters=it)
    for name in ("max_dist", "eps_t", "eps_r", "max_curvature"):
        for v in (0.0, -0.5, float("nan"), float("inf")):
            assert name in refused(E_INVALID, scans, poses, map=m, **{name: v})
    for v in (-1e-300, 1.0, 2.0, float("nan"), float("inf")):
        assert "rank_tol" in refused(E_INVALID, scans, poses, map=m, rank_tol=v)
    for v in (0, 1, 33, 1000):
        assert "normals_k" in refused(E_INVALID, scans, poses, map=m, k=v)
    Tl = np.eye(4, dtype=np.float32)
    Tl[0, 0] = np.inf
    assert "T_lidar2body" in refused(E_INVALID, scans, poses, Tl, map=m)
    bad_map = m.copy()
    bad_map[3, 0] = np.nan
    assert "non-finite" in refused(E_INVALID, scans, poses, map=bad_map)
    assert "empty map" in refused(E_INVALID, scans, poses, map=np.zeros((0, 4), np.float32))
    # the ends of the ranges are in
    T, rows2, _ = g.refine_poses_plane(scans, poses, map=m, rank_tol=0.0, k=2, max_iters=1, min_pairs=1)
    T, rows2, _ = g.refine_poses_plane(scans, poses, map=m, rank_tol=float(np.nextafter(1.0, 0.0)), k=32, max_iters=64, min_pairs=1)
    assert rows2[0]["rank"] <= 1
    # the offsets and the optional outputs, through the C ABI
    cat = np.ascontiguousarray(np.concatenate(scans))
    rows = (gpu_mod.RefinePlaneRow * 4)()
    Tb = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (4, 1))
    summ = gpu_mod.RefinePlaneSummary()
    prm = gpu_mod.RefinePlaneParams(1.0, 1e-4, 1e-5, 2, 1, 8, 1.0, 1e-9)

    def call(offs, n_pts=len(cat), rows=rows, summ=C.byref(summ), prm=C.byref(prm)):
        offs = np.ascontiguousarray(offs, np.uint64)
        return lib.erasor_hip_refine_poses_plane_clouds(g._h, m.ctypes.data_as(C.c_void_p), C.c_size_t(len(m)), C.c_int(0),
                                                        cat.ctypes.data_as(C.c_void_p), C.c_size_t(n_pts), offs.ctypes.data_as(C.c_void_p),
                                                        C.c_size_t(len(offs) - 1), C.c_int(0), None, Tb.ctypes.data_as(C.c_void_p), prm, rows, summ)

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
    T, rows2, _ = g.refine_poses_plane(scans, poses, map=m, min_pairs=1, max_iters=1)  # the handle is fine after the refusals
    assert [r["n_points"] for r in rows2] == [10, 20]
    # the header's layout
    R, P, S = gpu_mod.RefinePlaneRow, gpu_mod.RefinePlaneParams, gpu_mod.RefinePlaneSummary
    probe = [("sizeof(erasor_refine_plane_row)", C.sizeof(R)), ("sizeof(erasor_refine_plane_params)", C.sizeof(P)),
             ("sizeof(erasor_refine_plane_summary)", C.sizeof(S))]
    probe += [("offsetof(erasor_refine_plane_row, %s)" % k, getattr(R, k).offset) for k, _ in R._fields_]
    probe += [("offsetof(erasor_refine_plane_params, %s)" % k, getattr(P, k).offset) for k, _ in P._fields_]
    probe += [("offsetof(erasor_refine_plane_summary, %s)" % k, getattr(S, k).offset) for k, _ in S._fields_]
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){' +
            "".join('printf("%%zu\\n", (size_t)%s);' % e for e, _ in probe) + "return ERASOR_REFINE_DEGENERATE == 4 ? 0 : 1;}\n")
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [v for _, v in probe]
    assert evalmap.REFINE_DEGENERATE == 4
