"""The see-through check on the device (erasor_hip_visibility_*, kernels in visibility.hip.h) against its normative host text
evalmap.visibility, byte for byte -- votes, mask, kept cloud, frame rows and result -- and against the pure-Python visibility_brute where
the map has at most 300 points.  Known answers that do not rest on the restatement (one return on the x axis and six map points, under
the identity and under a yawed and translated pose), the margin band at its exact ends and one float32 step either side, the pixel edges
of exactly representable tables in all eight octants and at both row ends, both signs of zero, windows 0 .. 2 with the only return at
every corner, the column wrap and the row clipping, the priority of a hit, the minimum in every order of its points, every size around
a wavefront and a workgroup, batches one below, at and above the image budget, the incidence gate at its exact threshold, the decision
at its edges, a ray-cast scene whose answer follows from how it is built, every combination of outputs with guard words, the refusals,
the struct's layout, the handle's map with a step after it, and the synthetic world.  tests/test_visibility_on_cpu.py re-runs this file
against the CPU stand-in."""
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
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
THROUGH, HIT, OCCLUDED, NO_RETURN, UNSEEN = (1, 0, 1, 0), (1, 1, 0, 0), (1, 0, 0, 1), (1, 0, 0, 0), (0, 0, 0, 0)  # a point's row after one frame
EYE = np.eye(4, dtype=np.float32)


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


def grid_of(width, height, col_tan, row_tan):
    return {"width": width, "height": height, "col_tan": np.asarray(col_tan, np.float64), "row_tan": np.asarray(row_tan, np.float64)}


G8 = grid_of(8, 1, [], [-0.5, 0.5])  # one column per octant, one row
NARROW = dict(min_range=0.5, max_range=100.0, margin_abs=0.25, margin_rel=0.0, window=0, k=0, min_through=1, hit_weight=1.0)


def assert_same(got, want, what):
    """(votes, mask, kept, rows, result) twice: the same bytes and the same numbers"""
    for j, (name, dt) in enumerate((("votes", np.uint16), ("mask", np.uint8), ("kept", np.float32))):
        g, w = got[j], want[j]
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(1))
            assert False, (what, name, len(bad), bad[:5], g[bad[:3]], w[bad[:3]])
    assert got[3] == want[3], (what, "rows", [(f, a, b) for f, (a, b) in enumerate(zip(got[3], want[3])) if a != b][:3])
    assert tuple(got[4].keys()) == evalmap.VISIBILITY_RESULT_FIELDS and got[4] == want[4], (what, got[4], want[4])
    for r in got[3]:
        assert tuple(r.keys()) == evalmap.VISIBILITY_ROW_FIELDS


def check(g, cloud, scans, T, grid, Tl=None, what="", budget=0, **kw):
    """the device against the normative text (and the pure-Python one on a small map); what the normative text returned"""
    want = evalmap.visibility(cloud, scans, T, Tl, grid, **kw)
    assert_same(g.visibility(scans, T, Tl, cloud, grid, image_budget_bytes=budget, **kw), want, what)
    if len(cloud) <= 300 and sum(len(s) for s in scans) <= 2000:
        assert_same(evalmap.visibility_brute(cloud, scans, T, Tl, grid, **kw), want, (what, "the pure-Python restatement"))
    return want


def step32(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


def yaw90(tx=0.0, ty=0.0, tz=0.0):
    """a quarter turn about z and a translation: exact in float32"""
    T = np.float32([[0, -1, 0, tx], [1, 0, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]])
    return T


def moved(T, xyz):
    """T applied to points whose images are exactly representable (quarter turns, small dyadic numbers)"""
    p = np.asarray(xyz, np.float64)
    out = p @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]
    assert (out.astype(np.float32) == out).all()
    return out.astype(np.float32)


# ---- 1. known answers that do not rest on the restatement ----
SIX = [(5, 0, 0), (10, 0, 0), (15, 0, 0), (0, 10, 0), (200, 0, 0), (0, 0, 5)]
SIX_ROWS = [THROUGH, HIT, OCCLUDED, NO_RETURN, UNSEEN, UNSEEN]  # through, hit, occluded, no return, out of range, on the axis


@pytest.mark.parametrize("pose", ["identity", "yawed and translated", "through T_lidar2body"])
def test_one_return_on_the_x_axis_and_six_map_points(handle, pose):
    scan = xyzi([(10, 0, 0)])
    Tb = {"identity": EYE, "yawed and translated": yaw90(3.0, -2.0, 1.5), "through T_lidar2body": yaw90(0.0, 0.0, 0.0)}[pose]
    Tl = np.float32([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 1.25], [0, 0, 0, 1]]) if pose == "through T_lidar2body" else None
    world = np.asarray(Tb, np.float64) @ (np.eye(4) if Tl is None else np.asarray(Tl, np.float64))
    cloud = xyzi(moved(world, SIX), [40, 252, 40, 40, 40, 40])
    want = check(handle, cloud, [scan], Tb[None], G8, Tl, what=pose, **NARROW)
    votes, mask, kept, rows, res = handle.visibility([scan], Tb[None], Tl, cloud, G8, **NARROW)
    assert votes.tolist() == [list(r) for r in SIX_ROWS]
    assert mask.tolist() == [0, 1, 1, 1, 1, 1] and kept.tobytes() == cloud[1:].tobytes()
    assert rows == [dict(n_points=1, n_non_finite=0, n_on_axis=0, n_out_of_range=0, n_out_of_view=0, n_pixels=1, n_map_in_view=4, n_hit=1, n_occluded=1,
                         n_no_return=1, n_through=1, n_grazing=0)]
    assert res == dict(n_points=6, n_never_in_view=2, n_kept=5, n_removed=1, n_removed_dynamic=0, n_removed_static=1, n_map_no_normal=0, n_in_view=4,
                       n_hit=1, n_occluded=1, n_no_return=1, n_through=1, n_grazing=0) == want[4]


def test_the_scan_points_that_are_dropped_are_counted_by_their_gate(handle):
    scan = xyzi([(10, 0, 0), (np.nan, 0, 0), (0, np.inf, 1), (0, 0, 3), (-0.0, 0.0, -2), (0.25, 0, 0), (101, 0, 0), (1, 0, 1), (1, 0, -0.5), (1, 0, 0.5),
                 (1, 0, step32(0.5, False))])
    want = check(handle, xyzi(SIX), [scan], EYE[None], G8, what="drops", **NARROW)
    r = want[3][0]
    assert (r["n_points"], r["n_non_finite"], r["n_on_axis"], r["n_out_of_range"], r["n_out_of_view"], r["n_pixels"]) == (11, 2, 2, 2, 2, 1)


# ---- 2. the margin band ----
@pytest.mark.parametrize("rel", [False, True])
def test_the_margin_band_at_its_exact_ends_and_one_step_either_side(handle, rel):
    """margin_rel = 0: m = 0.25, a return at 10: rho - m = 10 at rho = 10.25, rho + m = 10 at rho = 9.75.  margin_rel = 0.125, margin_abs =
    0: 0.875 rho = 7 and 1.125 rho = 9 at rho = 8, every product exact in float64.  On the axis rho = |x| exactly."""
    kw = dict(NARROW, margin_abs=0.0, margin_rel=0.125) if rel else NARROW
    for ret, at, beyond in ((7.0, 8.0, OCCLUDED), (9.0, 8.0, THROUGH)) if rel else ((10.0, 10.25, OCCLUDED), (10.0, 9.75, THROUGH)):
        up = beyond == OCCLUDED  # the band's far end is left by going up, its near end by going down
        xs = [at, step32(at, up), step32(at, not up)]
        want = check(handle, xyzi([(x, 0, 0) for x in xs]), [xyzi([(ret, 0, 0)])], EYE[None], G8, what=("band", rel, ret), **kw)
        assert want[0].tolist() == [list(HIT), list(beyond), list(HIT)], (rel, ret, want[0])


# ---- 3. pixel edges ----
QUARTERS = grid_of(32, 2, [0.25, 0.5, 0.75], [-0.5, 0.0, 0.5])
OCTANTS = [(sx, sy, swap) for sx in (1, -1) for sy in (1, -1) for swap in (False, True)]


def in_octant(major, minor, sx, sy, swap, z=0.0):
    return (sx * minor, sy * major, z) if swap else (sx * major, sy * minor, z)


@pytest.mark.parametrize("sx,sy,swap", OCTANTS)
def test_a_ratio_on_a_column_edge_belongs_to_the_column_above_it(handle, sx, sy, swap):
    """returns at (8, 8 e) for every table entry e, t == e exactly: the map point at half the range in the same direction is seen through,
    and so is the one a float32 step further from the axis; the one a step nearer to it lies in the column before, which is empty"""
    for e in (0.25, 0.5, 0.75):
        scan = xyzi([in_octant(8.0, 8.0 * e, sx, sy, swap)])
        probes = [in_octant(4.0, m, sx, sy, swap) for m in (4.0 * e, step32(4.0 * e, True), step32(4.0 * e, False))]
        want = check(handle, xyzi(probes), [scan], EYE[None], QUARTERS, what=("column edge", sx, sy, swap, e), **NARROW)
        assert want[0].tolist() == [list(THROUGH), list(THROUGH), list(NO_RETURN)], (e, want[0])
    # the diagonal itself (t == 1) and the two axes of the octant's quadrant (t == 0), a return on each
    scan = xyzi([in_octant(8.0, 8.0, sx, sy, swap), in_octant(8.0, 0.0, sx, sy, swap)])
    probes = [in_octant(4.0, 4.0, sx, sy, swap), in_octant(4.0, 0.0, sx, sy, swap), in_octant(4.0, -0.0, sx, sy, swap), in_octant(4.0, 3.5, sx, sy, swap)]
    want = check(handle, xyzi(probes), [scan], EYE[None], QUARTERS, what=("diagonal and axis", sx, sy, swap), **NARROW)
    assert want[0].tolist() == [list(THROUGH), list(THROUGH), list(THROUGH), list(THROUGH if not swap else NO_RETURN)], want[0]


def test_the_columns_of_the_eight_octants_follow_each_other(handle):
    """one return in the middle of every column of QUARTERS and W = 16, a map point under each: every column is filled once"""
    for grid, ratios in ((QUARTERS, (0.125, 0.375, 0.625, 0.875)), (grid_of(16, 1, [0.5], [-1.0, 1.0]), (0.25, 0.75)), (G8, (0.5,))):
        dirs = [in_octant(8.0, 8.0 * r, sx, sy, swap) for sx, sy, swap in OCTANTS for r in ratios]
        cols = evalmap.visibility_column(np.float64([d[0] for d in dirs]), np.float64([d[1] for d in dirs]), grid["col_tan"], grid["width"])
        assert sorted(cols.tolist()) == list(range(grid["width"]))
        want = check(handle, xyzi(np.float32(dirs) / 2), [xyzi(dirs)], EYE[None], grid, what=("all columns", grid["width"]), **NARROW)
        assert want[3][0]["n_pixels"] == grid["width"] and (want[0] == THROUGH).all()


@pytest.mark.parametrize("height", [1, 2])
def test_a_tangent_on_a_row_edge_belongs_to_the_row_above_it(handle, height):
    """x = 4, y = 0: sqrt(x x + y y) = 4 exactly and s = z / 4.  Rows [-0.5, 0) and [0, 0.5) (H = 2) or [-0.5, 0.5) (H = 1)."""
    grid = grid_of(8, height, [], [-0.5, 0.0, 0.5] if height == 2 else [-0.5, 0.5])
    zs = [-2.0, step32(-2.0, False), step32(-2.0, True), 0.0, -0.0, step32(0.0, False), 2.0, step32(2.0, False)]
    # the map points' rows: 0 (the bottom edge is in), out, 0, the row above 0, the same, 0, out (the top edge is out), the top row
    top = height - 1
    rows = [0, None, 0, top, top, 0, None, top]
    scan = xyzi([(8.0, 0.0, -2.0), (8.0, 0.0, 2.0)] if height == 2 else [(8.0, 0.0, 0.0)])  # a return in every row, twice as far
    want = check(handle, xyzi([(4.0, 0.0, z) for z in zs]), [scan], EYE[None], grid, what=("row edge", height), **dict(NARROW, margin_abs=0.0))
    assert want[3][0]["n_pixels"] == height
    assert want[0].tolist() == [list(UNSEEN if r is None else THROUGH) for r in rows], want[0]


# ---- 4. windows ----
def centre(grid, row, col, rho):
    """a point of range rho in the middle of a pixel of a uniform grid made by visibility_grid (the test's own trigonometry: far from every edge)"""
    W, H = grid["width"], grid["height"]
    el = math.atan(grid["row_tan"][0]) + (row + 0.5) * (math.atan(grid["row_tan"][-1]) - math.atan(grid["row_tan"][0])) / H
    az = (col + 0.5) * 2 * math.pi / W
    p = (rho * math.cos(el) * math.cos(az), rho * math.cos(el) * math.sin(az), rho * math.sin(el))
    assert int(evalmap.visibility_column(np.float64([p[0]]), np.float64([p[1]]), grid["col_tan"], W)[0]) == col
    return p


@pytest.mark.parametrize("w", [0, 1, 2])
def test_the_only_return_at_every_corner_of_the_window_and_just_outside_it(handle, gpu_mod, w):
    """a map point in pixel (r0, c0) at range 5, the scan's only return at (r0 + dr, c0 + dc) at range 10: seen through iff |dr| <= w and
    |dc| <= w, with the columns wrapping between W - 1 and 0 and the rows clipped at 0 and H - 1"""
    grid = gpu_mod.visibility_grid(16, 5, -25.0, 25.0)
    W, H = 16, 5
    for r0, c0 in ((2, 5), (0, 0), (4, 15), (0, 15), (4, 0)):
        offs = [(dr, dc) for dr in (-w - 1, -w, 0, w, w + 1) for dc in (-w - 1, -w, 0, w, w + 1)]
        offs = sorted(set((dr, dc) for dr, dc in offs if 0 <= r0 + dr < H))
        scans = [xyzi([centre(grid, r0 + dr, (c0 + dc) % W, 10.0)]) for dr, dc in offs]
        cloud = xyzi([centre(grid, r0, c0, 5.0)])
        want = check(handle, cloud, scans, np.stack([EYE] * len(scans)), grid, what=("window", w, r0, c0), **dict(NARROW, window=w, max_range=50.0))
        inside = sum(1 for dr, dc in offs if abs(dr) <= w and abs(dc) <= w)
        assert want[0].tolist() == [[len(offs), 0, inside, 0]], (w, r0, c0, want[0])
        assert [r["n_through"] for r in want[3]] == [1 if abs(dr) <= w and abs(dc) <= w else 0 for dr, dc in offs]
    # rows do not wrap: the return in the top row says nothing about a point in the bottom row
    want = check(handle, xyzi([centre(grid, 0, 3, 5.0)]), [xyzi([centre(grid, 4, 3, 10.0)])], EYE[None], grid, what="rows clip", **dict(NARROW, window=2))
    assert want[0].tolist() == [list(NO_RETURN)]


def test_a_hit_and_an_occluder_in_one_window_give_a_hit(handle, gpu_mod):
    grid = gpu_mod.visibility_grid(16, 5, -25.0, 25.0)
    cloud = xyzi([centre(grid, 2, 5, 10.0)])
    near, same, far = centre(grid, 1, 4, 3.0), centre(grid, 3, 6, 10.0), centre(grid, 2, 5, 20.0)
    for returns, verdict in (([near, same, far], HIT), ([near, far], OCCLUDED), ([far], THROUGH), ([same], HIT), ([], NO_RETURN)):
        for order in itertools.permutations(returns):
            want = check(handle, cloud, [xyzi(list(order)) if order else np.zeros((0, 4), np.float32)], EYE[None], grid, what=("priority", len(order)),
                         **dict(NARROW, window=1))
            assert want[0].tolist() == [list(verdict)]


# ---- 5. the minimum ----
def test_five_returns_in_one_pixel_in_every_order_leave_the_nearest(handle):
    """with both margins 0 only a map point at exactly the stored range is a hit: the one at the smallest range; the one at the second
    smallest is occluded by it.  One frame per permutation, all in one call."""
    ranges = [7.0, 5.5, 9.25, float(step32(5.5, True)), 30.0]
    perms = list(itertools.permutations(ranges))
    scans = [xyzi([(r, 0, 0) for r in p]) for p in perms]
    cloud = xyzi([(5.5, 0, 0), (step32(5.5, True), 0, 0), (7.0, 0, 0), (5.0, 0, 0)])
    kw = dict(NARROW, margin_abs=0.0)
    want = check(handle, cloud, scans, np.stack([EYE] * len(perms)), G8, what="min over permutations", **kw)
    n = len(perms)
    assert want[0].tolist() == [[n, n, 0, 0], [n, 0, 0, n], [n, 0, 0, n], [n, 0, n, 0]]
    assert all(r["n_pixels"] == 1 and r["n_points"] == 5 for r in want[3])
    # duplicates of the nearest
    want = check(handle, cloud, [xyzi([(5.5, 0, 0)] * 3 + [(7.0, 0, 0)] * 2)], EYE[None], G8, what="duplicates", **kw)
    assert want[0].tolist() == [list(HIT), list(OCCLUDED), list(OCCLUDED), list(THROUGH)] and want[3][0]["n_pixels"] == 1


# ---- 6. sizes ----
def blob(n, seed, span=12.0, labels=True):
    rng = np.random.default_rng(seed)
    return xyzi(rng.uniform(-span, span, (n, 3)) * [1, 1, 0.25], rng.integers(245, 265, n) if labels else 40.0)


SMALL_GRID = grid_of(16, 2, [0.5], [-0.75, 0.0, 0.75])
LOOSE = dict(min_range=1.0, max_range=14.0, margin_abs=0.5, margin_rel=0.02, window=1, k=0, min_through=1, hit_weight=1.0)


def frames_of(sizes, seed):
    scans = [blob(n, seed + 17 * f, labels=False) for f, n in enumerate(sizes)]
    T = np.stack([EYE] * len(sizes)).copy()
    for f in range(len(sizes)):
        T[f, :3, 3] = [0.5 * f - 1.0, 0.25 * (f % 3), 0.125 * f]
    return scans, T


@pytest.mark.parametrize("n_map", [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_map_size_around_a_wavefront_and_a_workgroup(handle, n_map):
    scans, T = frames_of([0, 1, 64, 257, 40], 3)
    scans[4][:, :3] *= 100.0  # a frame whose points are all dropped (out of range)
    want = check(handle, blob(n_map, n_map), scans, T, SMALL_GRID, what=("n_map", n_map), **LOOSE)
    assert want[4]["n_points"] == n_map and want[3][4]["n_out_of_range"] == 40 and want[3][4]["n_pixels"] == 0 and want[3][0]["n_points"] == 0
    if n_map >= 63:
        assert want[4]["n_through"] > 0 and want[4]["n_hit"] > 0 and want[4]["n_occluded"] > 0 and want[4]["n_no_return"] > 0 and want[4]["n_removed"] > 0


def test_no_frames_and_empty_everything(handle):
    want = check(handle, blob(70, 1), [], np.zeros((0, 4, 4), np.float32), SMALL_GRID, what="no frames", **LOOSE)
    assert want[3] == [] and want[4]["n_never_in_view"] == 70 and want[4]["n_kept"] == 70
    check(handle, blob(0, 1), [], np.zeros((0, 4, 4), np.float32), SMALL_GRID, what="nothing", **LOOSE)
    # many tiny frames: more frames in one image workgroup than it has counters for
    scans, T = frames_of([3] * 70 + [0] * 5 + [1] * 60, 5)
    want = check(handle, blob(100, 2), scans, T, SMALL_GRID, what="tiny frames", **LOOSE)
    assert sum(r["n_points"] for r in want[3]) == 270


@pytest.mark.parametrize("images", [1, 2, 3])
def test_batches_below_at_and_above_the_image_budget_vote_as_one_batch_does(handle, images):
    image_bytes = SMALL_GRID["width"] * SMALL_GRID["height"] * 4
    cloud = blob(257, 9)
    for n_frames in sorted({max(images - 1, 1), images, images + 1, 2 * images + 1}):
        scans, T = frames_of([90 + 7 * f for f in range(n_frames)], 21)
        one = handle.visibility(scans, T, None, cloud, SMALL_GRID, **LOOSE)
        want = check(handle, cloud, scans, T, SMALL_GRID, what=("budget", images, n_frames), budget=images * image_bytes, **LOOSE)
        assert_same(one, want, ("one batch", images, n_frames))
        # a budget below one image still takes one image at a time
        assert_same(handle.visibility(scans, T, None, cloud, SMALL_GRID, image_budget_bytes=1, **LOOSE), want, ("one image", n_frames))


# ---- 7. the incidence gate ----
def lattice():
    u, v = np.meshgrid(np.arange(9) * 0.5 - 2.0, np.arange(9) * 0.5 - 2.0, indexing="ij")
    return np.stack([u.ravel(), v.ravel(), np.zeros(81)], 1).astype(np.float32)


def looking_from(origin, plane):
    """the pose of a lidar at `origin` (no rotation) and a scan that has a return twice as far behind every point of the plane"""
    T = EYE.copy()
    T[:3, 3] = origin
    local = plane.astype(np.float64) - np.float64(origin)
    assert (local.astype(np.float32) == local).all() and (np.abs(local[:, :2]).max(1) > 0).all()
    return T, xyzi(2.0 * local)


def test_the_incidence_gate_on_a_lattice_plane(handle):
    """a 9 x 9 lattice in z = 0 has the normal (0, 0, 1) exactly (tests/test_gpu_normals.py).  From (-3, 0.25, 4) the point (0, 0.25, 0)
    ... is not on the lattice, so the lidar stands at (-3, 0, 4) shifted by a quarter: see below."""
    plane = lattice()
    grid = grid_of(8, 1, [], [-1000.0, 1000.0])
    kw = dict(min_range=0.25, max_range=100.0, margin_abs=0.125, margin_rel=0.0, window=0, min_through=1, hit_weight=1.0)
    down = looking_from((0.25, 0.25, 4.0), plane)      # every cosine >= 4 / sqrt(16 + 2 * 2.25^2) > 0.78
    along = looking_from((-10.25, 0.25, 0.125), plane)  # every cosine <= 0.125 / 8.25 < 0.02
    cloud = xyzi(plane)
    for k, name in ((0, "ungated"), (8, "gated")):
        want = check(handle, cloud, [down[1], along[1]], np.stack([down[0], along[0]]), grid, what=("lattice", name), k=k, min_cos=0.25, **kw)
        assert want[3][0]["n_through"] == 81 and want[3][0]["n_grazing"] == 0
        assert (want[3][1]["n_through"], want[3][1]["n_grazing"]) == ((81, 0) if k == 0 else (0, 81))
        assert want[4]["n_map_no_normal"] == 0 and (want[0][:, 2] == (2 if k == 0 else 1)).all()
    # the exact threshold: from (-3, 0, 4) the point (0, 0, 0) has v = (3, 0, -4), |n . v| = 4 and sqrt(v . v) = 5; 4 / 5 is no binary
    # number, but the double nearest 0.8 times 5 rounds to exactly 4 -- not below it, so the see-through counts -- and its neighbours do not
    T, scan = looking_from((-3.0, 0.0, 4.0), plane)
    at = int(np.flatnonzero((plane == 0).all(1))[0])
    assert 0.8 * 5.0 == 4.0 and np.nextafter(0.8, 1.0) * 5.0 > 4.0 and np.nextafter(0.8, 0.0) * 5.0 < 4.0
    for min_cos, through in ((0.8, 1), (float(np.nextafter(0.8, 1.0)), 0), (float(np.nextafter(0.8, 0.0)), 1)):
        want = check(handle, cloud, [scan], T[None], grid, what=("min_cos", min_cos), k=8, min_cos=min_cos, **kw)
        assert want[0][at].tolist() == [1, 0, through, 0]


def test_a_point_without_a_normal_is_not_gated(handle):
    """fewer than k other points: the normal is NaN, the grazing see-through counts and the point stays removable"""
    grid = grid_of(8, 1, [], [-1000.0, 1000.0])
    kw = dict(min_range=0.25, max_range=100.0, margin_abs=0.125, margin_rel=0.0, window=0, min_through=1, hit_weight=1.0)
    cloud = xyzi(lattice()[:5])
    T, scan = looking_from((-10.25, 0.25, 0.125), lattice()[:5])
    want = check(handle, cloud, [scan], T[None], grid, what="NaN normals", k=8, min_cos=0.25, **kw)
    assert want[4]["n_map_no_normal"] == 5 and want[4]["n_through"] == 5 and want[4]["n_grazing"] == 0 and want[4]["n_removed"] == 5


# ---- 8. the decision ----
def test_the_decision_at_its_edges_and_the_removed_points_by_label(handle):
    """a map point at (5, 0, 0): a frame with a return at 10 sees through it, one with a return at 5 hits it, an empty one says nothing"""
    see, hit, none = xyzi([(10, 0, 0)]), xyzi([(5, 0, 0)]), np.zeros((0, 4), np.float32)
    labels = [251, 252, 259, 260, 252 + (7 << 16), np.nan, -1.0]
    cloud = xyzi([(5, 0, 0)] * len(labels), labels)
    scans = [see, hit, see, none, hit, see]  # through 3, hit 2
    T = np.stack([EYE] * len(scans))
    for min_through, weight, removed in ((3, 1.0, True), (4, 1.0, False), (3, 1.5, False), (3, float(np.nextafter(1.5, 0.0)), True), (0, 0.0, True),
                                         (1, 2.0, False)):
        want = check(handle, cloud, scans, T, G8, what=("decision", min_through, weight), **dict(NARROW, min_through=min_through, hit_weight=weight))
        assert want[0].tolist() == [[6, 2, 3, 0]] * len(labels)  # (in view of the empty frame too)
        assert (want[1] == (0 if removed else 1)).all()
        assert (want[4]["n_removed"], want[4]["n_removed_dynamic"], want[4]["n_removed_static"]) == ((7, 3, 4) if removed else (0, 0, 0))
    # no see-through at all is never removed, whatever the weights
    want = check(handle, cloud, [hit, none], T[:2], G8, what="nothing through", **dict(NARROW, min_through=0, hit_weight=0.0))
    assert want[4]["n_removed"] == 0


# ---- 9. a scene whose answer follows from how it is built ----
def cast(grid, box):
    """the returns of one noise-free scan, rays through the pixel centres of `grid` from the origin: the ground z = -1.5, a wall x = 12 and
    optionally a box; lidar-frame points in float32 and whether each came from the box"""
    W, H = grid["width"], grid["height"]
    pts, on_box, ray = [], [], []
    el0, el1 = math.atan(grid["row_tan"][0]), math.atan(grid["row_tan"][-1])
    for row in range(H):
        el = el0 + (row + 0.5) * (el1 - el0) / H
        for col in range(W):
            az = (col + 0.5) * 2 * math.pi / W
            d = np.float64([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
            best, from_box = math.inf, False
            if d[2] < 0:
                best = -1.5 / d[2]
            if d[0] > 0 and 12.0 / d[0] < best and -1.5 <= 12.0 / d[0] * d[2] <= 4.0:
                best = 12.0 / d[0]
            if box is not None:
                lo, hi = np.float64(box[0]), np.float64(box[1])
                with np.errstate(divide="ignore"):
                    t0, t1 = (lo - 0.0) / d, (hi - 0.0) / d
                near, far = np.minimum(t0, t1).max(), np.maximum(t0, t1).min()
                if 0 < near <= far and near < best:
                    best, from_box = near, True
            if best < 60.0:
                pts.append(best * d)
                on_box.append(from_box)
                ray.append(row * W + col)
    return xyzi(pts), np.array(on_box), np.array(ray)


BOX = ((5.0, -1.0, -1.25), (6.0, 1.0, 0.5))  # (it hovers a quarter of a metre: the ground just behind its lower edge is out of the margin)


def test_a_box_that_stood_before_a_wall_in_the_first_frame_only(handle, gpu_mod):
    """Six frames from one place, each a quarter turn further (the pixel mapping and the rays are symmetric under quarter turns, and a
    quarter turn is exact in float32, so every frame casts the same rays into the world): frame 0 sees a box, the others the ground and
    the wall behind it.  The map is the union of all returns.  A box point is hit once and seen through five times: removed.  A wall or
    ground point is hit by every frame, or occluded by the box in frame 0: kept.  Exactly."""
    grid = gpu_mod.visibility_grid(64, 16, -20.0, 10.0)
    Tl = np.float32([[1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 1, 1.0], [0, 0, 0, 1]])
    turns = [np.linalg.matrix_power(np.float64(yaw90())[:3, :3], f % 4) for f in range(6)]
    T = np.stack([EYE] * 6).copy()
    scans, world, is_box = [], [], []
    # what the construction keeps in band: behind every box return the boxless scan has a return, well beyond the margin
    (with_box, from_box, ray_b), (without, _, ray_w) = cast(grid, BOX), cast(grid, None)
    behind = {r: np.linalg.norm(p[:3]) for r, p in zip(ray_w.tolist(), without)}
    assert all(behind.get(r, 0.0) > np.linalg.norm(p[:3]) + 0.2 for r, p in zip(ray_b[from_box].tolist(), with_box[from_box]))
    for f, R in enumerate(turns):
        T[f, :3, :3] = R
        T[f, :3, 3] = -(R @ np.float64(Tl[:3, 3]))  # the lidar stays at the world's origin
        local, from_box, _ = cast(grid, BOX if f == 0 else None)
        # the scene is fixed in the world: the scan of a turned lidar is the turned-back scan of the unturned one
        local[:, :3] = (local[:, :3].astype(np.float64) @ R).astype(np.float32)
        scans.append(local)
        world.append(xyzi(local[:, :3].astype(np.float64) @ R.T, np.where(from_box, 252.0, 40.0)))
        is_box.append(from_box)
    cloud, is_box = np.concatenate(world), np.concatenate(is_box)
    assert is_box.sum() > 20 and len(cloud) > 2000
    kw = dict(min_range=0.5, max_range=60.0, margin_abs=0.05, margin_rel=0.0, window=0, k=0, min_through=2, hit_weight=1.0)
    want = check(handle, cloud, scans, T, grid, Tl, what="box scene", **kw)
    assert (want[1] == np.where(is_box, 0, 1)).all()
    assert (want[0][is_box] == [6, 1, 5, 0]).all() and (want[0][~is_box, 2] == 0).all() and (want[0][~is_box, 0] == 6).all()
    assert want[4]["n_removed"] == want[4]["n_removed_dynamic"] == int(is_box.sum()) and want[4]["n_removed_static"] == 0
    assert want[2].tobytes() == cloud[~is_box].tobytes()


# ---- 10. the interface ----
def raw_call(gpu_mod, g, cloud, scans, T, grid, kw, outs, budget=0, map_call=False, cap=None):
    """erasor_hip_visibility_clouds / _map through ctypes with the buffers given (None: NULL); the return code"""
    L = gpu_mod.lib()
    cat = np.ascontiguousarray(np.concatenate(scans) if scans else np.zeros((0, 4), np.float32), np.float32)
    offs = np.zeros(len(scans) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in scans])
    col, row = np.ascontiguousarray(grid["col_tan"], np.float64), np.ascontiguousarray(grid["row_tan"], np.float64)
    prm = gpu_mod.Visibility(grid["width"], grid["height"], col.ctypes.data_as(C.POINTER(C.c_double)), row.ctypes.data_as(C.POINTER(C.c_double)),
                             kw["min_range"], kw["max_range"], kw["margin_abs"], kw["margin_rel"], kw["window"], kw["k"], kw.get("min_cos", 0.25),
                             kw["min_through"], 0, kw["hit_weight"], budget)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    Tb = np.ascontiguousarray(T, np.float32)
    votes, mask, kept, rows, res = outs
    head = () if map_call else (p(cloud), C.c_size_t(len(cloud)), C.c_int(0))
    fn = L.erasor_hip_visibility_map if map_call else L.erasor_hip_visibility_clouds
    return fn(g._h, *head, p(cat), C.c_size_t(len(cat)), p(offs), C.c_size_t(len(scans)), C.c_int(0), None, p(Tb), C.byref(prm), p(votes), p(mask), p(kept),
              C.c_size_t(len(cloud) if cap is None else cap), rows, None if res is None else C.byref(res))


def test_every_combination_of_outputs_and_the_words_behind_them(handle, gpu_mod):
    cloud = blob(257, 9)
    scans, T = frames_of([90, 0, 130], 21)
    want = evalmap.visibility(cloud, scans, T, None, SMALL_GRID, **LOOSE)
    n, nk, nf = len(cloud), want[4]["n_kept"], len(scans)
    assert 0 < nk < n
    for use in itertools.product((False, True), repeat=5):
        votes, mask, kept = np.full(4 * n + 8, 0x7777, np.uint16), np.full(n + 8, 0x77, np.uint8), np.full(4 * n + 8, 7.0, np.float32)
        rows, res = (gpu_mod.VisibilityRow * (nf + 1))(), gpu_mod.VisibilityResult()
        rows[nf].n_points = res.n_points = 12345
        outs = [b if u else None for b, u in zip((votes, mask, kept, rows, res), use)]
        assert raw_call(gpu_mod, handle, cloud, scans, T, SMALL_GRID, LOOSE, outs) == 0, (use, gpu_mod.lib().erasor_hip_last_error(handle._h))
        for b, u, m, w, fill in ((votes, use[0], 4 * n, want[0], 0x7777), (mask, use[1], n, want[1], 0x77), (kept, use[2], 4 * nk, want[2], 7.0)):
            assert (b[m:] == fill).all(), use  # the guard words
            assert b[:m].tobytes() == w.tobytes() if u else (b[:m] == fill).all(), use
        assert rows[nf].n_points == 12345
        assert [rows[f].as_dict() for f in range(nf)] == want[3] if use[3] else all(rows[f].n_points == 0 for f in range(nf))
        assert res.as_dict() == want[4] if use[4] else res.n_points == 12345
    # a kept cloud that does not fit: the result first, then the code
    res = gpu_mod.VisibilityResult()
    kept = np.full(4 * n, 7.0, np.float32)
    assert raw_call(gpu_mod, handle, cloud, scans, T, SMALL_GRID, LOOSE, [None, None, kept, None, res], cap=nk - 1) == E_CAPACITY
    assert res.as_dict() == want[4] and (kept == 7.0).all()


def test_refusals_each_with_its_code_and_the_struct_layout(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    cloud = blob(100, 4)
    scans, T = frames_of([50, 60], 2)
    L = gpu_mod.lib()
    err = lambda: L.erasor_hip_last_error(g._h).decode()
    none = [None] * 5

    def refused(sentence, grid=SMALL_GRID, scans=scans, T=T, **kw):
        assert raw_call(gpu_mod, g, cloud, scans, T, grid, dict(LOOSE, **kw), none) == E_INVALID, sentence
        assert err() == "erasor_hip_visibility_clouds: " + sentence, err()

    for W in (0, 4, 12, 4104):
        refused("width must be a multiple of 8 within 8 .. 4096", grid_of(W, 2, [0.5], [-1, 0, 1]))
    for H in (0, 257):
        refused("height must be within 1 .. 256", grid_of(16, H, [0.5], [-1, 0, 1]))
    for col in ([0.5, 0.5], [0.6, 0.5], [0.0, 0.5], [0.5, 1.0], [np.nan, 0.5]):
        refused("col_tan must be strictly increasing within (0, 1)", grid_of(24, 2, col, [-1, 0, 1]))
    for row in ([-1, 0, 0], [0, -1, 1], [-1, 0, np.inf], [np.nan, 0, 1]):
        refused("row_tan must be finite and strictly increasing", grid_of(16, 2, [0.5], row))
    for lo, hi in ((5.0, 5.0), (6.0, 5.0), (-1.0, 5.0), (np.nan, 5.0), (1.0, np.inf)):
        refused("0 <= min_range < max_range, both finite", min_range=lo, max_range=hi)
    for kw in (dict(margin_abs=-0.1), dict(margin_rel=-0.1), dict(margin_abs=np.inf), dict(margin_rel=np.nan)):
        refused("the margins must be finite numbers >= 0", **kw)
    refused("window must be 0, 1 or 2", window=3)
    for k in (1, 33):
        refused("k must be 0 or within 2 .. 32", k=k)
    for kw in (dict(min_cos=np.nan), dict(hit_weight=np.inf), dict(hit_weight=-1.0)):
        refused("min_cos must be finite and hit_weight a finite number >= 0", **kw)
    many = [np.zeros((0, 4), np.float32)] * 65536
    refused("more than 65535 frames", scans=many, T=np.stack([EYE] * 65536))
    bad = T.copy()
    bad[1, 0, 3] = np.inf
    refused("non-finite entry in T_body2origin", T=bad)
    # offsets that are not monotone, params NULL
    cat, offs = np.concatenate(scans), np.uint64([0, 70, 50])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    col, row = np.float64([0.5]), np.float64([-1, 0, 1])
    prm = gpu_mod.Visibility(16, 2, col.ctypes.data_as(C.POINTER(C.c_double)), row.ctypes.data_as(C.POINTER(C.c_double)), 1.0, 14.0, 0.5, 0.02, 1, 0, 0.25, 1, 0,
                             1.0, 0)
    args = lambda o, q: (g._h, p(cloud), C.c_size_t(100), C.c_int(0), p(cat), C.c_size_t(110), p(o), C.c_size_t(2), C.c_int(0), None, p(T), q, None, None, None,
                         C.c_size_t(0), None, None)
    assert L.erasor_hip_visibility_clouds(*args(offs, C.byref(prm))) == E_INVALID and err() == "erasor_hip_visibility_clouds: offsets decrease"
    assert L.erasor_hip_visibility_clouds(*args(np.uint64([0, 50, 110]), None)) == E_INVALID and err() == "erasor_hip_visibility_clouds: params is NULL"
    # with normals a non-finite map point is the normals' refusal; without them it is merely never in view
    c = cloud.copy()
    c[5, 1] = np.nan
    assert raw_call(gpu_mod, g, c, scans, T, SMALL_GRID, dict(LOOSE, k=8), none) == E_INVALID
    assert err() == "erasor_hip_visibility_clouds: non-finite coordinate (NaN / Inf) in 1 map point(s)"
    with pytest.raises(ValueError):
        evalmap.visibility(c, scans, T, None, SMALL_GRID, **dict(LOOSE, k=8))
    want = check(g, c, scans, T, SMALL_GRID, what="a NaN map point", **LOOSE)
    assert want[0][5].tolist() == [0, 0, 0, 0] and want[1][5] == 1
    # the handle's map: none yet -- the error normals_map gives
    res = gpu_mod.NormalsResult()
    assert L.erasor_hip_normals_map(g._h, C.c_uint32(8), None, None, None, None, C.byref(res)) == E_STATE
    sentence = err().split(": ", 1)[1]
    assert raw_call(gpu_mod, g, cloud, scans, T, SMALL_GRID, LOOSE, none, map_call=True) == E_STATE and err() == "erasor_hip_visibility_map: " + sentence
    for kw in (dict(window=3), dict(k=1), dict(min_range=9.0, max_range=2.0)):
        with pytest.raises(ValueError):
            evalmap.visibility(cloud, scans, T, None, SMALL_GRID, **dict(LOOSE, **kw))
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.visibility(scans, T, None, cloud, SMALL_GRID, **dict(LOOSE, **kw))
        assert e.value.rc == E_INVALID
    for bad in (-1, 2 ** 32):  # (no uint32: the call and its normative text refuse it alike, before anything runs)
        for fn in (lambda kw: evalmap.visibility(cloud, scans, T, None, SMALL_GRID, **kw), lambda kw: g.visibility(scans, T, None, cloud, SMALL_GRID, **kw)):
            with pytest.raises(ValueError):
                fn(dict(LOOSE, min_through=bad))
    check(g, cloud, scans, T, SMALL_GRID, what="after the refusals", **LOOSE)  # the handle is fine
    # the header's layout
    fields = ("width", "height", "col_tan", "row_tan", "min_range", "max_range", "margin_abs", "margin_rel", "window", "k", "min_cos", "min_through",
              "hit_weight", "image_budget_bytes")
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu", sizeof(erasor_visibility), '
            'sizeof(erasor_visibility_row), sizeof(erasor_visibility_result));' +
            "".join('printf(" %%zu", offsetof(erasor_visibility, %s));' % f for f in fields) +
            'printf(" %zu %zu\\n", offsetof(erasor_visibility_row, n_grazing), offsetof(erasor_visibility_result, n_grazing));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    V, R, S = gpu_mod.Visibility, gpu_mod.VisibilityRow, gpu_mod.VisibilityResult
    mirror = [C.sizeof(V), C.sizeof(R), C.sizeof(S)] + [getattr(V, f).offset for f in fields] + [R.n_grazing.offset, S.n_grazing.offset]
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == mirror
    assert mirror[:3] == [96, 96, 104] and mirror[-2:] == [88, 96]


def test_the_map_call_a_step_and_the_map_call_again(gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, plain = (gpu_mod.Erasor(scenarios.to_product_params(sc["params"])) for _ in range(2))
    for e in (g, plain):
        e.set_map(sc["map"])
        for f in range(n - 1):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    grid = gpu_mod.visibility_grid(64 if ON_CPU else 256, 16, -25.0, 5.0)
    scans, T = sc["scans"][:3], np.stack(sc["T_b2o"][:3])
    kw = dict(min_range=1.0, max_range=60.0, margin_abs=0.2, margin_rel=0.01, window=1, k=4 if ON_CPU else 8, min_cos=0.25, min_through=1, hit_weight=1.0)
    for f in (n - 1, n):
        m = np.ascontiguousarray(g.get_map(), np.float32)
        want = evalmap.visibility(m, scans, T, sc["T_l2b"], grid, **kw)
        assert_same(g.visibility(scans, T, sc["T_l2b"], None, grid, **kw), want, ("the handle's map before step", f))
        assert_same(g.visibility(scans, T, sc["T_l2b"], m, grid, **kw), want, ("the same map given", f))
        assert g.get_map().tobytes() == m.tobytes()  # the map itself stays as it is
        # the step after the call is the uninterrupted run's
        a = g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        b = plain.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        assert a.as_dict() == b.as_dict() and g.get_map().tobytes() == plain.get_map().tobytes()


# ---- 11. the synthetic world ----
def test_the_synthetic_world(handle, gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    m = np.ascontiguousarray(sc["map"], np.float32)
    cloud = np.ascontiguousarray(m[:: max(1, len(m) // 3000)])
    assert len(cloud) > 1000
    grid = gpu_mod.visibility_grid(128, 16, -25.0, 5.0)
    scans, T = sc["scans"][:4], np.stack(sc["T_b2o"][:4])
    kw = dict(min_range=1.0, max_range=60.0, margin_abs=0.2, margin_rel=0.01, window=1, min_cos=0.25, min_through=2, hit_weight=1.0)
    plain = check(handle, cloud, scans, T, grid, sc["T_l2b"], what="world", k=0, **kw)
    gated = check(handle, cloud, scans, T, grid, sc["T_l2b"], what="world, gated", k=8, **kw)
    assert plain[4]["n_in_view"] > len(cloud) and plain[4]["n_hit"] > 0 and plain[4]["n_through"] > 0 and plain[4]["n_occluded"] > 0
    assert gated[4]["n_through"] + gated[4]["n_grazing"] == plain[4]["n_through"] and gated[4]["n_hit"] == plain[4]["n_hit"]
    # the same from device buffers, in two batches
    p = handle.device_array(cloud)
    cat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32).reshape(-1, 4) for s in scans]))
    q = handle.device_array(cat)
    try:
        offs = np.cumsum([0] + [len(s) for s in scans])
        got = handle.visibility((q, offs), T, sc["T_l2b"], (p, len(cloud)), grid, k=8, image_budget_bytes=2 * 128 * 16 * 4, **kw)
        assert_same(got, gated, "device buffers")
    finally:
        handle.device_free(p)
        handle.device_free(q)
