"""Every scan's points labelled static / dynamic / unknown from a cleaned map on the device (erasor_hip_label_scans_clouds / _map, kernels
in label_scans.hip.h) against the host oracle evalmap.label_scans: byte for byte on the small scenario after its steps (host and device
scans, a caller map and the handle's, with and without a raw map, the split on each code), edge shapes at wavefront, workgroup and leaf
boundaries, points at the threshold, exact properties, the bounded search's effort against the exact search's on the same tree, errors
and the struct layout, a step and a ticket after the call.  tests/test_label_scans_on_cpu.py re-runs part of this file against the CPU
stand-in."""
import contextlib
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import erasor_amd
import hooks
import hooks_label_scans
import scenarios
from erasor_amd import evalmap, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_CPU = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))  # (the CPU stand-in is orders of magnitude slower: a shorter scenario, the same paths)
NN_LEAF, NN_QBLOCK, SCAN_BLOCK = 32, 256, 1024
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


@contextlib.contextmanager
def hooked(gpu_mod):
    """a handle of the hooks build; closed before the product library is back in place"""
    with hooks.hooks_library():
        g = gpu_mod.Erasor(gpu_mod.params_default())
        try:
            yield g
        finally:
            g.close()


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def oracle(static, frames, poses, Tl, raw, tau, split):
    return evalmap.label_scans(static[:, :3], frames, poses, Tl, raw_xyz=None if raw is None else raw[:, :3], tau=tau, split=split)


def assert_same(got, ref, what):
    assert len(got) == len(ref), what
    assert len(got[0]) == len(ref[0]), what
    for f, (a, b) in enumerate(zip(got[0], ref[0])):
        assert a.dtype == np.uint8 and a.tobytes() == b.tobytes(), (what, "codes of frame", f, np.flatnonzero(a != b)[:5] if len(a) == len(b) else (len(a), len(b)))
    assert got[1] == ref[1], (what, "rows", [(f, a, b) for f, (a, b) in enumerate(zip(got[1], ref[1])) if a != b][:3])
    assert got[2] == ref[2], (what, "summary", got[2], ref[2])
    if len(ref) == 4:
        for f, (a, b) in enumerate(zip(got[3], ref[3])):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, "split rows of frame", f, a.shape, b.shape)


def check(g, static, raw, frames, poses, Tl, tau, what):
    """the call without a split and with the split on every code against the oracle; what the plain call returned"""
    plain = None
    for split in (None, 0, 1) + ((2,) if raw is not None else ()):
        got = g.label_scans(frames, poses, Tl, static_map=static, raw_map=raw, tau=tau, split=split)
        assert_same(got, oracle(static, frames, poses, Tl, raw, tau, split), (what, "split", split))
        plain = got if split is None else plain
    return plain


# ---- 1. exactness on the small scenario after its steps ----
@pytest.fixture(scope="module")
def stepped(gpu_mod):
    sc = scenarios.small(n_frames=3, az=60) if ON_CPU else scenarios.small()
    g = gpu_mod.Erasor(scenarios.to_product_params(sc["params"]))
    g.set_map(sc["map"])
    for f in range(len(sc["scans"])):
        g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    cleaned = np.ascontiguousarray(g.get_map(), np.float32)
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]

    @functools.lru_cache(maxsize=None)
    def reference(with_raw, split):  # (computed once, shared by the cases)
        return oracle(cleaned, scans, sc["T_b2o"], sc["T_l2b"], sc["map"] if with_raw else None, evalmap.label_tau(0.2), split)

    return g, sc, cleaned, reference


@pytest.mark.parametrize("with_raw", [True, False], ids=["raw", "no_raw"])
@pytest.mark.parametrize("device_scans", [False, True], ids=["host_scans", "device_scans"])
@pytest.mark.parametrize("against", ["clouds", "map"])
def test_codes_rows_summary_and_split_match_the_host_oracle(gpu_mod, stepped, against, device_scans, with_raw):
    g, sc, cleaned, reference = stepped
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
    raw = sc["map"] if with_raw else None
    sm = None if against == "map" else cleaned
    p = None
    if device_scans:
        p = g.device_array(np.concatenate(scans))
        arg = (p, np.concatenate([[0], np.cumsum([len(s) for s in scans])]))
    else:
        arg = scans
    try:
        for split in (None, 0, 1) + ((2,) if with_raw else ()):
            got = g.label_scans(arg, sc["T_b2o"], sc["T_l2b"], static_map=sm, raw_map=raw, voxelsize=0.2, split=split)
            assert_same(got, reference(with_raw, split), (against, device_scans, with_raw, split))
    finally:
        if p is not None:
            g.device_free(p)
    summary = got[2]
    n_pts = sum(len(s) for s in scans)
    assert summary["n_points"] == n_pts and summary["n_non_finite"] == 0 and sum(summary["n"][0]) + sum(summary["n"][1]) == n_pts
    # the scenario has moving objects and the cleaned map lost (most of) them: the scans' moving points are found, most points are static
    assert summary["n"][0][0] > 0.8 * sum(summary["n"][0]) and summary["n"][1][1] + summary["n"][1][2] > 0
    assert evalmap.moving_iou(summary)["TP"] == summary["n"][1][1]


# ---- 2. edge shapes ----
def small_maps(seed=9):
    rng = np.random.default_rng(seed)
    static = xyzi(rng.uniform(-6, 6, (300, 3)))
    raw = np.concatenate([static, xyzi(rng.uniform(-9, 9, (200, 3)), 252.0)])
    return static, raw


def queries(rng, n):
    w = rng.choice(np.array([40.0, 252.0, 70.0, 65536.0 * 5 + 255.0, 259.0, 251.0, 260.0], np.float32), n)
    return xyzi(rng.uniform(-9, 9, (n, 3)), w)


SIZE_SETS = {
    "wavefront": [0, 1, 63, 64, 65],
    "query_block": [NN_QBLOCK - 1, NN_QBLOCK, NN_QBLOCK + 1],
    "empty_frames": [0, 5, 0, 0, 7, 0],
    "one_wavefront_three_frames": [30, 10, 40],
    "scan_blocks": [SCAN_BLOCK - 1, 1, 1, SCAN_BLOCK - NN_QBLOCK, NN_QBLOCK + 1, 3],
}


@pytest.mark.parametrize("name", list(SIZE_SETS))
def test_frame_sizes_at_wavefront_workgroup_and_scan_block_edges(handle, name):
    rng = np.random.default_rng(31)
    static, raw = small_maps()
    frames = [queries(rng, n) for n in SIZE_SETS[name]]
    poses = []
    for f in range(len(frames)):
        T = EYE.copy()
        T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        poses.append(T)
    Tl = EYE.copy()
    Tl[2, 3] = 0.25
    for r in (None, raw):
        got = check(handle, static, r, frames, poses, Tl, 1.0, (name, r is not None))
    assert [r["n_points"] for r in got[1]] == SIZE_SETS[name]
    if name == "scan_blocks":  # every code occurs on both sides of every boundary
        allc = np.concatenate(got[0])
        assert all(len(set(allc[b - 60:b].tolist())) == 3 and len(set(allc[b:b + 60].tolist())) == 3 for b in (NN_QBLOCK, SCAN_BLOCK))
        assert len(allc) > 2 * SCAN_BLOCK and len(set(allc[2 * SCAN_BLOCK - 60:2 * SCAN_BLOCK].tolist())) == 3


def test_frames_of_one_code_and_compaction_counts_at_every_boundary(handle):
    """a frame whose points are all static, all dynamic, all unknown: the split's ranks then ARE the indices, so every workgroup (256) and
    scan block (1024) boundary of the compaction carries a count equal to its position"""
    rng = np.random.default_rng(32)
    static, raw = small_maps()
    n = 2 * SCAN_BLOCK + 7
    all_static = xyzi(static[rng.integers(0, len(static), n), :3], 252.0)
    all_dynamic = xyzi(raw[300 + rng.integers(0, 200, n), :3] + np.float32(50.0))  # (moved out of the static map's reach, below)
    all_unknown = xyzi(rng.uniform(200, 300, (n, 3)))
    far_raw = raw.copy()
    far_raw[300:, :3] += np.float32(50.0)
    frames = [all_static, all_dynamic, all_unknown, all_static[:1], all_unknown[:65]]
    got = check(handle, static, far_raw, frames, [EYE] * 5, None, 0.4, "one code")
    assert [set(c.tolist()) for c in got[0]] == [{0}, {1}, {2}, {0}, {2}]
    assert got[1][0]["n"] == [[0, 0, 0], [n, 0, 0]] and got[1][1]["n"] == [[0, n, 0], [0, 0, 0]] and got[1][2]["n"] == [[0, 0, n], [0, 0, 0]]


def edge_frames():
    """NaN / Inf points and overflowing poses (tests/test_gpu_align.py's constructions, rebuilt)"""
    rng = np.random.default_rng(5)
    frames, poses = [], []

    def add(pts, T=EYE):
        frames.append(xyzi(pts, 252.0) if len(pts) else np.zeros((0, 4), np.float32))
        poses.append(np.asarray(T, np.float32))

    add(np.zeros((0, 3)))
    add(np.tile([[3.1, -2.2, 0.7]], (300, 1)))                   # identical points
    nan_pts = rng.uniform(-8, 8, (300, 3))
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
    add(rng.uniform(-8, 8, (600, 3)), T)                         # several workgroups
    bad_w = xyzi(rng.uniform(-8, 8, (40, 3)))
    bad_w[:, 3] = np.tile(np.array([np.nan, -1.0, 4294967296.0, np.inf, 252.0, 4294967040.0, -0.0, 65536.0 + 252.0], np.float32), 5)
    frames.append(bad_w)                                         # labels out of range: static, and counted
    poses.append(EYE)
    add(np.zeros((0, 3)))
    return frames, poses


def test_dropped_points_overflowing_poses_and_labels_out_of_range(handle):
    static, raw = small_maps()
    frames, poses = edge_frames()
    Tl = EYE.copy()
    Tl[2, 3] = 1.73
    for T_l2b in (Tl, None):
        for r in (raw, None):
            got = check(handle, static, r, frames, poses, T_l2b, 1.0, ("edge", T_l2b is None, r is not None))
    rows = got[1]
    assert rows[2]["n_non_finite"] > 40 and rows[3]["n_non_finite"] == 200 and rows[4]["n_non_finite"] == 5 and rows[5]["n_non_finite"] == 65
    assert set(got[0][3].tolist()) == {255} and rows[7]["n_label_out_of_range"] == 20
    assert got[2]["n_non_finite"] == sum(int((c == 255).sum()) for c in got[0])


def threshold_queries(p, tau):
    """points exactly at tau from p, and one float32 step either side, on each axis and on diagonals"""
    p = np.asarray(p, np.float32)
    out = []
    t = np.float32(tau)
    for axis in range(3):
        for sign in (-1, 1):
            at = p[axis] + np.float32(sign) * t
            for v in (np.nextafter(at, np.float32(-np.inf)), at, np.nextafter(at, np.float32(np.inf))):
                q = p.copy()
                q[axis] = v
                out.append(q)
    for d in ([0.6, 0.8, 0.0], [0.0, 0.6, 0.8], [0.8, 0.0, -0.6], [3 / 13, 4 / 13, 12 / 13], [-2 / 3, 1 / 3, 2 / 3]):
        at = p + t * np.asarray(d, np.float32)
        for k in range(3):
            for v in (np.nextafter(at[k], np.float32(-np.inf)), at[k], np.nextafter(at[k], np.float32(np.inf))):
                q = at.copy()
                q[k] = v
                out.append(q)
    return np.asarray(out, np.float32)


@pytest.mark.parametrize("tau", [0.5, 0.2 * np.sqrt(3) / 2, 0.25, 1.0])
def test_points_at_the_threshold_and_one_float32_step_either_side(handle, tau):
    for p in ([0.0, 0.0, 0.0], [1.0, -2.0, 0.5], [17.25, 3.0, -0.125]):
        static = xyzi([p])
        q = xyzi(threshold_queries(p, tau))
        raw = xyzi([[p[0], p[1], p[2] + 100.0]])
        got = check(handle, static, raw, [q], [EYE], None, float(tau), ("threshold", tau, p))
        if p == [0.0, 0.0, 0.0] and tau in (0.5, 0.25, 1.0):  # (tau a float32: the axis points land exactly on it -- at tau is not static)
            assert got[0][0][:18].tolist() == [2, 2, 0, 0, 2, 2] * 3
    # the issue's three hand-computed queries
    q = xyzi([[0.5, 0, 0], [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0], [np.float32(0.3), np.float32(0.4), 0]])
    assert handle.label_scans([q], [EYE], static_map=xyzi([[0, 0, 0]]), tau=0.5)[0][0].tolist() == [1, 0, 1]


@pytest.mark.parametrize("n_static", [1, NN_LEAF - 1, NN_LEAF, NN_LEAF + 1])
def test_static_maps_of_one_point_and_around_one_leaf(handle, n_static):
    rng = np.random.default_rng(40 + n_static)
    static = xyzi(rng.uniform(-3, 3, (n_static, 3)))
    raw = xyzi(rng.uniform(-4, 4, (NN_LEAF + 1, 3)))
    frames = [queries(rng, 200) * np.float32([0.4, 0.4, 0.4, 1.0]), queries(rng, 70) * np.float32([0.4, 0.4, 0.4, 1.0])]
    got = check(handle, static, raw, frames, [EYE, EYE], None, 1.2, ("n_static", n_static))
    assert {0, 1} <= set(np.concatenate(got[0]).tolist())


def test_an_empty_static_map_and_an_empty_raw_map(handle):
    rng = np.random.default_rng(43)
    static, raw = small_maps()
    empty = np.zeros((0, 4), np.float32)
    frames = [queries(rng, 300), np.zeros((0, 4), np.float32), queries(rng, 10)]
    poses = [EYE] * 3
    got = check(handle, empty, raw, frames, poses, None, 1.0, "empty static")
    assert 0 not in set(np.concatenate(got[0]).tolist()) and {1, 2} <= set(np.concatenate(got[0]).tolist())
    got = check(handle, static, empty, frames, poses, None, 1.0, "empty raw")
    assert set(np.concatenate(got[0]).tolist()) == {0, 2}
    got = check(handle, empty, empty, frames, poses, None, 1.0, "both empty")
    assert set(np.concatenate(got[0]).tolist()) == {2}
    got = check(handle, empty, None, frames, poses, None, 1.0, "empty static, no raw")
    assert set(np.concatenate(got[0]).tolist()) == {1}
    # no frames at all, and empty frames only
    codes, rows, summary, clouds = handle.label_scans([], np.zeros((0, 4, 4), np.float32), static_map=static, raw_map=raw, split=1)
    assert codes == [] and rows == [] and clouds == [] and summary == oracle(static, [], [], None, raw, 1.0, None)[2]
    check(handle, static, raw, [np.zeros((0, 4), np.float32)] * 2, [EYE] * 2, None, 1.0, "empty frames")


# ---- 3. exact properties ----
def test_a_frame_against_itself_shrinking_tau_and_the_overlap_reports_distances(handle):
    rng = np.random.default_rng(51)
    static, raw = small_maps()
    frame = queries(rng, 700)
    T = np.asarray(erasor_amd.geopose2eigen([1.5, -2.0, 0.3, 0.0, 0.0, 0.38268343, 0.92387953]), np.float32).reshape(4, 4)
    Tl = EYE.copy()
    Tl[2, 3] = 1.73
    # a frame labelled against itself, put into the map frame: all static, whatever tau
    in_map = xyzi(evalmap._xform(T, evalmap._xform(Tl, frame[:, :3])))
    for tau in (1e-6, 0.1):
        codes, rows, summary = handle.label_scans([frame], [T], Tl, static_map=in_map, tau=tau)
        assert set(codes[0].tolist()) == {0} and sum(summary["n"][0]) + sum(summary["n"][1]) == 700
    # shrinking tau never turns a non-static point static
    prev = None
    for tau in (3.0, 1.5, 1.0, 0.7, 0.4, 0.2, 0.05):
        codes = check(handle, static, raw, [frame], [T], Tl, tau, ("shrinking", tau))[0][0]
        if prev is not None:
            assert not ((codes == 0) & (prev != 0)).any()
        prev = codes
    # codes == 0 is the overlap report's per-point distance < tau on the same input
    for tau in (1.0, 0.35):
        codes = handle.label_scans([frame], [EYE], static_map=static, tau=tau)[0][0]
        dist = handle.overlap(static, frame, 0.2, per_point=True)["dist"]
        assert ((codes == 0) == (dist < tau)).all() and (codes == 0).tobytes() == (dist < tau).tobytes()


# ---- 4. the bounded search's effort ----
@functools.lru_cache(maxsize=None)
def world_slice(n, spacing=0.25, seed=20210311):
    w = synth.World(seed=seed, length=60.0)
    m = w.sample_map(spacing=spacing, frames=range(0, 20, 4), x_range=(0.0, 30.0))
    assert len(m) >= n, (len(m), n)
    return np.ascontiguousarray(m[np.random.default_rng(n).permutation(len(m))[:n]], np.float32)


def dup_runs(seed, n_runs=14):
    rng = np.random.default_rng(seed)
    place = rng.uniform(-10, 10, (n_runs, 3)).astype(np.float32)
    rows = [xyzi(np.repeat(place[r][None], int(rng.integers(40, 201)), 0)) for r in range(n_runs)]
    c = np.concatenate(rows)
    return np.ascontiguousarray(c[rng.permutation(len(c))]), place


def effort_fixtures():
    """tests/test_gpu_spatial_index.py's kinds of geometry, rebuilt"""
    rng = np.random.default_rng(21)
    n_q = 300 if ON_CPU else 2049
    u = xyzi(np.random.default_rng(41).uniform(-20, 20, (5000, 3)))
    w = world_slice(5000)
    scan = world_slice(n_q, spacing=0.4).copy()
    scan[:, :3] += rng.normal(0, 0.03, (len(scan), 3)).astype(np.float32)
    d, place = dup_runs(42)
    qd = np.concatenate([xyzi(place), xyzi(place[rng.integers(0, len(place), n_q - len(place))] + rng.normal(0, 0.5, (n_q - len(place), 3)))])
    far = rng.normal(0, 1, (n_q, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * rng.choice([1e4, 1e5, 1e6, 1e7], (n_q, 1))
    return [("uniform_inside", u, xyzi(rng.uniform(-20, 20, (n_q, 3)))), ("world_scan", w, scan), ("far_outside", u, xyzi(far)),
            ("dup_runs", d, qd)]


@pytest.mark.parametrize("name", [f[0] for f in effort_fixtures()])
def test_bounded_search_never_works_harder_than_the_exact_search(gpu_mod, name):
    """For every query, on the same tree: the bounded search opens no more leaves and tests no more leaf points than nn_search_f64, and
    decides as its distance does.  A condition, not a measurement: both share the traversal order (label_scans.hip.h's header)."""
    cloud, q = {f[0]: f[1:] for f in effort_fixtures()}[name]
    with hooked(gpu_mod) as g:
        exact = hooks.debug_nn_effort(g, cloud, q, False)
        for tau in (0.05, 0.2 * np.sqrt(3) / 2, 0.6, 2.5, 1e5):
            got = hooks_label_scans.debug_ls_effort(g, cloud, q, tau)
            worse = np.flatnonzero((got["effort"] > exact["effort"]).any(1))
            assert len(worse) == 0, (name, tau, worse[:5], got["effort"][worse[:5]], exact["effort"][worse[:5]])
            assert ((got["codes"] == 0) == (exact["dist"] < tau)).all(), (name, tau)
            print("EFFORT %s tau %.4g: %d queries, %d static; leaves %d (exact %d), leaf points %d (exact %d)" % (
                name, tau, len(q), int((got["codes"] == 0).sum()), got["effort"][:, 0].sum(), exact["effort"][:, 0].sum(),
                got["effort"][:, 1].sum(), exact["effort"][:, 1].sum()))


# ---- 5. errors and the struct layout ----
def test_errors_capacity_and_struct_layout(gpu_mod, tmp_path):
    E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
    lib = gpu_mod.lib()
    g = gpu_mod.Erasor(gpu_mod.params_default())
    rng = np.random.default_rng(2)
    m = xyzi(rng.uniform(-3, 3, (100, 3)))
    scans = [xyzi(rng.uniform(-3, 3, (n, 3))) for n in (10, 20)]
    poses = [np.eye(4, dtype=np.float32)] * 2

    def refused(rc, *a, **kw):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.label_scans(*a, **kw)
        assert e.value.rc == rc, str(e.value)
        return str(e.value)

    for tau in (0.0, -0.2, float("nan"), float("inf")):
        assert "tau" in refused(E_INVALID, scans, poses, static_map=m, tau=tau)
    for split in (3, -1, 255):
        assert "split_code" in refused(E_INVALID, scans, poses, static_map=m, raw_map=m, split=split)
    assert "raw map" in refused(E_INVALID, scans, poses, static_map=m, split=2)
    p = [t.copy() for t in poses]
    p[1][2, 1] = np.nan
    assert "non-finite" in refused(E_INVALID, scans, p, static_map=m)
    Tl = np.eye(4, dtype=np.float32)
    Tl[0, 0] = np.inf
    assert "T_lidar2body" in refused(E_INVALID, scans, poses, Tl, static_map=m)
    bad_map = m.copy()
    bad_map[3, 0] = np.nan
    assert "static map point" in refused(E_INVALID, scans, poses, static_map=bad_map)
    assert "raw map point" in refused(E_INVALID, [xyzi([[50.0, 50.0, 50.0]])], poses[:1], static_map=m, raw_map=bad_map)
    # the offsets and the split's capacity, through the C ABI
    cat = np.ascontiguousarray(np.concatenate(scans))
    rows = (gpu_mod.ScanLabelRow * 70000)()
    Tb = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (70000, 1))
    summ = gpu_mod.ScanLabelRow()
    codes = np.zeros(64, np.uint8)
    out = np.full((64, 4), -7.0, np.float32)
    out_offs = np.zeros(70001, np.uint64)

    def call(offs, n_pts=len(cat), tau=1.0, split=None, cap=0, n_static=len(m)):
        offs = np.ascontiguousarray(offs, np.uint64)
        return lib.erasor_hip_label_scans_clouds(
            g._h, m.ctypes.data_as(C.c_void_p), C.c_size_t(n_static), C.c_int(0), None, C.c_size_t(0), C.c_int(0), C.c_int(0),
            cat.ctypes.data_as(C.c_void_p), C.c_size_t(n_pts), offs.ctypes.data_as(C.c_void_p), C.c_size_t(len(offs) - 1), C.c_int(0), None,
            Tb.ctypes.data_as(C.c_void_p), C.c_double(tau), codes.ctypes.data_as(C.c_void_p), C.c_int(0 if split is None else split),
            None if split is None else out.ctypes.data_as(C.c_void_p), C.c_size_t(cap), None if split is None else out_offs.ctypes.data_as(C.c_void_p),
            rows, C.byref(summ))

    ref = oracle(m, scans, poses, None, None, 1.0, 0)
    assert call([0, 10, 30]) == 0 and rows[1].as_dict() == ref[1][1] and summ.as_dict() == ref[2]
    assert call([1, 10, 30]) == E_INVALID
    assert call([0, 20, 10, 30]) == E_INVALID
    assert call([0, 10, 29]) == E_INVALID
    assert call([0, 10, 30], n_pts=2**30) == E_INVALID
    assert call([0, 10, 30], n_static=2**30) == E_INVALID
    many = np.zeros(65538, np.uint64)
    many[-1] = len(cat)
    assert call(many) == E_INVALID and "65536" in lib.erasor_hip_last_error(g._h).decode()
    n_static_rows = sum(len(c) for c in ref[3])
    assert 1 < n_static_rows < 30
    assert call([0, 10, 30], split=0, cap=30) == 0
    assert out[:n_static_rows].tobytes() == np.concatenate(ref[3]).tobytes() and (out[n_static_rows:] == -7.0).all()
    assert out_offs[:3].tolist() == [0, len(ref[3][0]), n_static_rows]
    assert call([0, 10, 30], split=0, cap=n_static_rows) == 0  # exactly enough
    # too small: ERASOR_E_CAPACITY, with the rows, the summary, the codes and the offsets filled first
    for k in range(2):
        rows[k].n_points = 0
    codes[:] = 99
    out_offs[:] = 0
    assert call([0, 10, 30], split=0, cap=n_static_rows - 1) == E_CAPACITY
    assert [rows[k].as_dict() for k in range(2)] == ref[1] and summ.as_dict() == ref[2]
    assert codes[:30].tobytes() == np.concatenate(ref[0]).tobytes() and out_offs[:3].tolist() == [0, len(ref[3][0]), n_static_rows]
    # the handle's map: none yet
    assert "no map" in refused(E_STATE, scans, poses)
    # a step in flight: the NOFLY guard
    sc = scenarios.small(n_frames=2, az=60)
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    refused(E_STATE, scans, poses)
    refused(E_STATE, scans, poses, static_map=m)
    g.step_wait()
    assert [r["n_points"] for r in g.label_scans(scans, poses)[1]] == [10, 20]  # the handle is fine after the refusals
    # the header's layout
    R = gpu_mod.ScanLabelRow
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", '
            'sizeof(erasor_scan_label_row), offsetof(erasor_scan_label_row, n_points), offsetof(erasor_scan_label_row, n_non_finite), '
            'offsetof(erasor_scan_label_row, n_label_out_of_range), offsetof(erasor_scan_label_row, n), '
            'sizeof(((erasor_scan_label_row *)0)->n[0]));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(R), R.n_points.offset, R.n_non_finite.offset, R.n_label_out_of_range.offset, R.n.offset, 3 * 8] and C.sizeof(R) == 72


# ---- 6. no side effects on the run ----
def test_label_scans_between_steps_leaves_later_steps_and_tickets_intact(gpu_mod):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import orc
    from test_gpu_parity import compare_step
    sc = scenarios.small()
    g, o = gpu_mod.Erasor(scenarios.to_product_params(sc["params"])), orc.Oracle(sc["params"])
    g.set_map(sc["map"])
    o.set_map(sc["map"])
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
    n, ahead = (3 if ON_CPU else 5), 2
    Tl, Tb, To = sc["T_l2b"], sc["T_b2o"], sc["T_o2b"]
    tau = evalmap.label_tau(0.2)
    tickets = {}
    for j in range(ahead):
        tickets[j] = g.prefetch_node_rows(scans[j], 3, Tl, Tb[j], To[j])
    for k in range(n):
        if k + ahead < n:
            tickets[k + ahead] = g.prefetch_node_rows(scans[k + ahead], 3, Tl, Tb[k + ahead], To[k + ahead])
        # with nodes announced ahead: the call works in the evaluator's scratch, its trees' sorts in a radix bank of their own
        some = list(range(max(0, k - 1), min(n, k + 1)))
        got = g.label_scans([scans[f] for f in some], [Tb[f] for f in some], Tl, raw_map=sc["map"], split=1)
        assert_same(got, oracle(o.get_map(), [scans[f] for f in some], [Tb[f] for f in some], Tl, sc["map"], tau, 1), ("between steps", k))
        rg = g.step_ticket(tickets.pop(k), Tb[k], To[k])
        ro = o.step(scans[k], Tl, Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
    assert g.get_map().shape == o.get_map().shape
