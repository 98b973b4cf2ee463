"""Every frame's pose checked against the map on the device (erasor_hip_align_frames_clouds / _map, kernels in align.hip.h) against the
host oracle evalmap.align_frames: bit for bit on the small scenario with host and device scans, edge cases at wavefront boundaries and
with dropped points, the faults it is there to find (a moved or turned pose, the wrong lidar-to-body convention, poses one index off),
steps after the check, errors and the struct layout, the offline driver's --align mode, and the bench's full-size map.
tests/test_align_on_cpu.py re-runs part of this file against the CPU stand-in."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import scenarios
from erasor_amd import evalmap, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("n_est", "n_below_half", "n_below_one", "n_below_two", "median", "p90", "p99", "max", "frac_half", "frac_one", "frac_two")
ROW_FIELDS = ("n_points", "n_non_finite") + FIELDS
# the CPU stand-in runs the kernels four to five orders of magnitude slower: a shorter scenario there, the same code paths
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
def sc():
    return scenarios.small()


def same_bits(a, b):
    a, b = np.float64(a), np.float64(b)
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


def assert_same(rows, summary, ref, what=""):
    ref_rows, ref_summary = ref
    assert len(rows) == len(ref_rows), what
    for f, (r, q) in enumerate(zip(rows, ref_rows)):
        for k in ROW_FIELDS:
            assert same_bits(r[k], q[k]), (what, "frame", f, k, r[k], q[k])
    for k in FIELDS:
        assert same_bits(summary[k], ref_summary[k]), (what, "summary", k, summary[k], ref_summary[k])


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.full((len(xyz), 1), w, np.float32)], 1)


def flagged(rows):
    """the README's "most points" rule: a frame with 50 % or fewer of its points below 0.5 * v"""
    return [not (r["frac_half"] > 50.0) for r in rows]


# ---- 1. exactness ----
@pytest.mark.parametrize("device_scans", [False, True])
@pytest.mark.parametrize("against", ["clouds", "map"])
def test_rows_and_summary_match_the_host_oracle(gpu_mod, sc, against, device_scans):
    g = gpu_mod.Erasor(scenarios.to_product_params(sc["params"]))
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
    ref = evalmap.align_frames(sc["map"][:, :3], scans, sc["T_b2o"], sc["T_l2b"], 0.2)
    if against == "map":
        g.set_map(sc["map"])
    m = None if against == "map" else sc["map"]
    if device_scans:
        cat = np.concatenate(scans)
        offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])])
        p = g.device_array(cat)
        try:
            rows, summary = g.align_frames((p, offs), sc["T_b2o"], sc["T_l2b"], map=m, voxelsize=0.2)
        finally:
            g.device_free(p)
    else:
        rows, summary = g.align_frames(scans, sc["T_b2o"], sc["T_l2b"], map=m, voxelsize=0.2)
    assert_same(rows, summary, ref, (against, device_scans))
    assert summary["n_est"] == sum(len(s) for s in scans) and rows[0]["n_non_finite"] == 0
    assert 0.0 <= summary["median"] < 0.2


# ---- 2. edge cases ----
def edge_frames():
    rng = np.random.default_rng(5)
    frames, poses = [], []
    ident = np.eye(4, dtype=np.float32)

    def add(pts, T=ident):
        frames.append(xyzi(pts) if len(pts) else np.zeros((0, 4), np.float32))
        poses.append(np.asarray(T, np.float32))

    add(np.zeros((0, 3)))                                        # empty
    add(rng.uniform(-20, 20, (1, 3)))                            # one point
    add(np.tile([[3.1, -2.2, 0.7]], (700, 1)))                  # identical points: every rank ties
    for n in (1, 63, 64, 65):                                    # wavefront boundaries (and frames that straddle them)
        add(rng.uniform(-20, 20, (n, 3)))
    nan_pts = rng.uniform(-20, 20, (300, 3))
    nan_pts[::7, 1] = np.nan
    nan_pts[3::11, 2] = np.inf
    nan_pts[5, 0] = -np.inf
    add(nan_pts)                                                 # NaN / Inf points: dropped and counted
    big = np.diag([1e38, 1e38, 1e38, 1.0]).astype(np.float32)
    add(rng.uniform(5, 20, (200, 3)), big)                       # the pose overflows every coordinate to Inf
    add(np.full((5, 3), np.nan))                                 # every point dropped
    half = rng.uniform(0.5, 20, (130, 3))
    half[::2] *= 1000.0
    add(half, big * np.float32(0.1))                             # every other point overflows
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.31, -0.12, 0.05]
    add(rng.uniform(-20, 20, (1000, 3)), T)                      # several workgroups
    add(np.zeros((0, 3)))                                        # empty at the end
    return frames, poses


@pytest.mark.parametrize("map_kind", ["cloud", "one_point"])
def test_edge_cases_match_the_host_oracle(gpu_mod, handle, map_kind):
    rng = np.random.default_rng(9)
    m = xyzi(rng.uniform(-25, 25, (5000, 3))) if map_kind == "cloud" else xyzi([[1.0, 2.0, -0.5]])
    frames, poses = edge_frames()
    Tl = np.eye(4, dtype=np.float32)
    Tl[2, 3] = 1.73
    for T_l2b in (Tl, None):
        ref = evalmap.align_frames(m[:, :3], frames, poses, T_l2b, 0.25)
        rows, summary = handle.align_frames(frames, poses, T_l2b, map=m, voxelsize=0.25)
        assert_same(rows, summary, ref, (map_kind, T_l2b is None))
    assert [r["n_points"] for r in rows] == [len(f) for f in frames]
    assert rows[0]["n_est"] == 0 and np.isnan(rows[0]["median"]) and np.isnan(rows[-1]["max"])
    assert rows[7]["n_non_finite"] == 300 - rows[7]["n_est"] > 40
    assert rows[8]["n_non_finite"] == 200 and rows[8]["n_est"] == 0 and np.isnan(rows[8]["frac_half"])
    assert rows[9]["n_non_finite"] == 5 and rows[10]["n_non_finite"] == 65 and rows[10]["n_est"] == 65
    assert rows[2]["median"] == rows[2]["p99"] == rows[2]["max"]


def test_no_frames_and_a_handle_map(gpu_mod, sc):
    g = gpu_mod.Erasor(scenarios.to_product_params(sc["params"]))
    rows, summary = g.align_frames([], np.zeros((0, 4, 4), np.float32), map=sc["map"])
    assert rows == [] and summary["n_est"] == 0 and np.isnan(summary["median"])
    g.set_map(sc["map"])
    rows, summary = g.align_frames([], np.zeros((0, 4, 4), np.float32))
    assert rows == [] and summary["n_below_half"] == 0
    # empty frames against an empty map: nothing to measure, nothing refused
    rows, summary = g.align_frames([np.zeros((0, 4), np.float32)] * 2, [np.eye(4)] * 2, map=np.zeros((0, 4), np.float32))
    assert [r["n_est"] for r in rows] == [0, 0] and np.isnan(summary["p90"])


# ---- 3. what it is for ----
def test_it_finds_a_moved_or_turned_pose_the_wrong_convention_and_shifted_poses(gpu_mod, sc):
    g = gpu_mod.Erasor(scenarios.to_product_params(sc["params"]))
    g.set_map(sc["map"])
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
    n = len(scans)
    Tb = [np.asarray(t, np.float32).reshape(4, 4) for t in sc["T_b2o"]]

    def check(poses, T_l2b=sc["T_l2b"]):
        rows, summary = g.align_frames(scans, poses, T_l2b)
        ref = evalmap.align_frames(sc["map"][:, :3], scans, poses, T_l2b, 0.2)
        assert_same(rows, summary, ref)
        return rows, summary

    good, good_sum = check(Tb)
    assert not any(flagged(good)), [r["frac_half"] for r in good]
    bad = n // 2
    moved = [t.copy() for t in Tb]
    moved[bad][1, 3] += 1.0  # 1 m across the street (along it, the ground and the facades still overlay: 67 % stay within 0.5 * v)
    turned = [t.copy() for t in Tb]
    c, s = np.cos(np.radians(3.0)), np.sin(np.radians(3.0))  # 3 degrees of pitch
    turned[bad][:3, :3] = (np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64) @ turned[bad][:3, :3].astype(np.float64)).astype(np.float32)
    for poses in (moved, turned):
        rows, _ = check(poses)
        assert flagged(rows) == [f == bad for f in range(n)], [r["frac_half"] for r in rows]
        assert rows[bad]["median"] > good[bad]["median"] and rows[bad]["p90"] > good[bad]["p90"]
        for f in range(n):
            if f != bad:
                assert rows[f] == good[f]
    # tf/lidar2body left out (the README's convention mix-up): the scans sit 1.73 m low
    _, none_sum = check(Tb, None)
    assert none_sum["frac_half"] < 0.25 * good_sum["frac_half"] and none_sum["median"] > 5 * good_sum["median"]
    # poses one index off (pitfall 3): every frame gets worse
    shifted, _ = check(Tb[1:] + Tb[-1:])
    for f in range(n - 1):
        assert shifted[f]["frac_half"] < good[f]["frac_half"] and shifted[f]["median"] > good[f]["median"], f


# ---- 4. no side effects on the run ----
def test_align_between_steps_leaves_later_steps_and_tickets_intact(gpu_mod, sc):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import orc
    from test_gpu_parity import compare_step
    g, o = gpu_mod.Erasor(scenarios.to_product_params(sc["params"])), orc.Oracle(sc["params"])
    g.set_map(sc["map"])
    o.set_map(sc["map"])
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
    n, ahead = len(scans), 2
    Tl, Tb, To = sc["T_l2b"], sc["T_b2o"], sc["T_o2b"]
    tickets = {}
    for j in range(ahead):
        tickets[j] = g.prefetch_node_rows(scans[j], 3, Tl, Tb[j], To[j])
    for k in range(n):
        if k + ahead < n:
            tickets[k + ahead] = g.prefetch_node_rows(scans[k + ahead], 3, Tl, Tb[k + ahead], To[k + ahead])
        # with nodes announced ahead: the check works in the evaluator's scratch, its tree sort in a radix bank of its own
        some = list(range(max(0, k - 1), min(n, k + 2)))
        rows, summary = g.align_frames([scans[f] for f in some], [Tb[f] for f in some], Tl)
        assert_same(rows, summary, evalmap.align_frames(o.get_map()[:, :3], [scans[f] for f in some], [Tb[f] for f in some], Tl, 0.2))
        rg = g.step_ticket(tickets.pop(k), Tb[k], To[k])
        ro = o.step(scans[k], Tl, Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
    assert g.get_map().shape == o.get_map().shape


# ---- 5. errors and the struct layout ----
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
            g.align_frames(*a, **kw)
        assert e.value.rc == rc, str(e.value)
        return str(e.value)

    for vs in (0.0, -0.2, float("nan"), float("inf")):
        refused(E_INVALID, scans, poses, map=m, voxelsize=vs)
    for bad_at in ((0, 0, 3), (1, 2, 1)):
        p = [t.copy() for t in poses]
        p[bad_at[0]][bad_at[1], bad_at[2]] = np.nan
        assert "non-finite" in refused(E_INVALID, scans, p, map=m)
    Tl = np.eye(4, dtype=np.float32)
    Tl[0, 0] = np.inf
    assert "T_lidar2body" in refused(E_INVALID, scans, poses, Tl, map=m)
    bad_map = m.copy()
    bad_map[3, 0] = np.nan
    assert "non-finite" in refused(E_INVALID, scans, poses, map=bad_map)
    assert "empty map" in refused(E_INVALID, scans, poses, map=np.zeros((0, 4), np.float32))
    # the offsets, through the C ABI: offsets[0] != 0, decreasing, a last offset other than the point count, more than 65536 frames
    cat = np.ascontiguousarray(np.concatenate(scans))
    rows = (gpu_mod.AlignRow * 70000)()
    Tb = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (70000, 1))
    summ = gpu_mod.OverlapResult()

    def call(offs, n_pts=len(cat), n_frames=None, T=Tb, vs=0.2):
        offs = np.ascontiguousarray(offs, np.uint64)
        nf = len(offs) - 1 if n_frames is None else n_frames
        return lib.erasor_hip_align_frames_clouds(g._h, m.ctypes.data_as(C.c_void_p), C.c_size_t(len(m)), C.c_int(0), cat.ctypes.data_as(C.c_void_p),
                                                  C.c_size_t(n_pts), offs.ctypes.data_as(C.c_void_p), C.c_size_t(nf), C.c_int(0), None,
                                                  T.ctypes.data_as(C.c_void_p), C.c_double(vs), rows, C.byref(summ))

    assert call([0, 10, 30]) == 0 and rows[1].r.n_est == 20 and summ.n_est == 30
    assert call([1, 10, 30]) == E_INVALID
    assert call([0, 20, 10, 30]) == E_INVALID
    assert call([0, 10, 29]) == E_INVALID
    assert call([0, 10, 31]) == E_INVALID
    assert call([0, 10, 30], n_pts=2**30) == E_INVALID
    many = np.zeros(65538, np.uint64)
    many[-1] = len(cat)
    assert call(many) == E_INVALID and "65536" in gpu_mod.lib().erasor_hip_last_error(g._h).decode()
    many = np.zeros(65537, np.uint64)
    many[-1] = len(cat)
    assert call(many) == 0 and rows[65535].r.n_est == 30 and rows[0].n_points == 0  # exactly 65536 frames
    assert lib.erasor_hip_align_frames_clouds(g._h, m.ctypes.data_as(C.c_void_p), C.c_size_t(2**30), C.c_int(0), cat.ctypes.data_as(C.c_void_p),
                                              C.c_size_t(len(cat)), np.array([0, 30], np.uint64).ctypes.data_as(C.c_void_p), C.c_size_t(1),
                                              C.c_int(0), None, Tb.ctypes.data_as(C.c_void_p), C.c_double(0.2), rows, None) == E_INVALID
    # the handle's map: none yet
    assert "no map" in refused(E_STATE, scans, poses)
    # a step in flight: the NOFLY guard
    sc = scenarios.small(n_frames=2, az=60)
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    refused(E_STATE, scans, poses)
    refused(E_STATE, scans, poses, map=m)
    g.step_wait()
    rows2, _ = g.align_frames(scans, poses)  # the handle is fine after the refusals
    assert [r["n_est"] for r in rows2] == [10, 20]
    # the header's layout
    R, O = gpu_mod.AlignRow, gpu_mod.OverlapResult
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", '
            'sizeof(erasor_align_row), offsetof(erasor_align_row, n_points), offsetof(erasor_align_row, n_non_finite), '
            'offsetof(erasor_align_row, r), sizeof(erasor_overlap_result));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(R), R.n_points.offset, R.n_non_finite.offset, R.r.offset, C.sizeof(O)]


# ---- 6. the offline driver ----
def write_ascii_pcd(path, pts):
    pts = np.asarray(pts, np.float32)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
            "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(pts), len(pts)))
    with open(path, "w") as f:
        f.write(head)
        for p in pts:
            f.write("%r %r %r %r\n" % tuple(float(v) for v in p))


def test_offline_driver_align_mode(gpu_mod, sc, tmp_path):
    shim_dir = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
    demo = os.path.join(shim_dir, "erasor_offline_demo")
    d = tmp_path / "seq"
    (d / "pcds").mkdir(parents=True)
    n = min(len(sc["scans"]), 5)
    for k in range(n):
        write_ascii_pcd(d / "pcds" / ("%06d.pcd" % k), sc["scans"][k])
    write_ascii_pcd(d / "dense_global_map.pcd", sc["map"])
    with open(d / "poses_lidar2body.csv", "w") as f:
        f.write("index,timestamp,x,y,z,qx,qy,qz,qw\n")
        for k in range(n):
            f.write("%d,%d,%s\n" % (k, 1000 + k, ",".join(repr(float(v)) for v in sc["poses"][k])))
    yaml = d / "rosparam.yaml"
    yaml.write_text('data_dir: "%s"\ninit_idx: 0\ntf:\n     lidar2body: [0.0, 0.0, %r, 0.0, 0.0, 0.0, 1.0]\n' % (d, float(synth.LIDAR_HEIGHT)))
    out = subprocess.run([demo, "--align", str(yaml), str(n), "0.2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    # the poses the run uses: the CSV's, after callback_node's eigen2geoPose / geoPose2eigen round trip
    shim = C.CDLL(os.path.join(shim_dir, "liberasor_shim.so"))
    shim.erasor_shim_load_poses.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    shim.erasor_shim_load_poses.restype = C.c_long
    T, geo, Tb = np.zeros((n, 16), np.float32), np.zeros((n, 7)), np.zeros((n, 16), np.float32)
    assert shim.erasor_shim_load_poses(str(d / "poses_lidar2body.csv").encode(), T.ctypes.data, geo.ctypes.data, Tb.ctypes.data, n) == n
    Tl = gpu_mod.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    scans = [np.ascontiguousarray(sc["scans"][k], np.float32) for k in range(n)]
    within = []
    for T_l2b in (Tl, None):  # convention (B): poses in the body frame, the extrinsic in tf; then (A): the identity
        rows, summary = evalmap.align_frames(sc["map"][:, :3], scans, Tb, T_l2b, 0.2)
        for k, r in enumerate(rows):
            want = "%6d  n=%d  median=%.4fm  p90=%.4fm  <0.5*v %.2f%%  <1*v %.2f%%  <2*v %.2f%%%s" % (
                k, r["n_points"], r["median"], r["p90"], r["frac_half"], r["frac_one"], r["frac_two"],
                "" if r["frac_half"] > 50.0 else "  <- check this pose")
            assert want in lines, (want, out.stdout)
        text = evalmap.overlap_lines(summary, 0.2)
        i = lines.index(text[0])
        assert lines[i + 1] == text[1], out.stdout
        within.append(summary["frac_one"])
    assert within[0] > within[1]
    assert lines[-1].startswith("convention: (B)") and lines[-1].endswith("(B) fits better"), out.stdout


# ---- 7. full size: the bench's world ----
@pytest.mark.timeout(1200)
def test_full_size_against_the_bench_map(gpu_mod):
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
    n_frames = 24
    scans, Tb = [], []
    for k in range(n_frames):
        p7 = w.pose(k * 3, 1.0, x0=300.0, jitter_rng=jr)
        Tb.append(gpu_mod.geopose2eigen(p7))
        scans.append(np.ascontiguousarray(w.cast(p7, lid, k * 3), np.float32))
    g.align_frames(scans[:2], Tb[:2], Tl)  # (first call: allocations)
    t0 = time.perf_counter()
    rows, summary = g.align_frames(scans, Tb, Tl)
    t_dev = time.perf_counter() - t0
    sub = list(range(0, n_frames, 6))
    t0 = time.perf_counter()
    ref_rows, ref_sum = evalmap.align_frames(m[:, :3], [scans[f] for f in sub], [Tb[f] for f in sub], Tl, 0.2)
    t_host = time.perf_counter() - t0
    rows_sub, sum_sub = g.align_frames([scans[f] for f in sub], [Tb[f] for f in sub], Tl)
    n_pts = sum(len(s) for s in scans)
    print("\nfull size: %d-pt map, %d frames, %d scan points: align_frames_map %.1f ms; evalmap.align_frames on %d frames (%d points) "
          "%.1f ms\n%s" % (len(m), n_frames, n_pts, t_dev * 1e3, len(sub), sum(len(scans[f]) for f in sub), t_host * 1e3,
                           "\n".join(evalmap.overlap_lines(summary, 0.2))))
    assert_same(rows_sub, sum_sub, (ref_rows, ref_sum))
    for j, f in enumerate(sub):
        assert rows[f] == rows_sub[j]
    assert summary["n_est"] == n_pts and not any(flagged(rows))
    assert t_dev < 5.0  # (generous: the check is a small part of a run)
