"""The ground on the device (erasor_hip_ground_scans / _votes_*, kernels in ground.hip.h) against its normative host text
evalmap.ground_scans / ground_votes, byte for byte -- codes, rows, patch table, votes, mask, kept rows and result -- and against the
pure-Python *_brute twins where the input is small.  Known answers that do not rest on the restatement: a dyadic lattice on z = -1.75
under a box (normal exactly (0, 0, 1), d = 1.75), the same plane tilted about x and about y, a wall alone in a patch.  The grid's edges
one float32 step either side in all eight octants; the seeds (equal z in every permutation, the count around num_lpr, num_lpr 1 and 64,
min_z at a point's z, no candidate); th_dist, uprightness, elevation and flatness at their exact ends, taken from the host text;
degenerate patches in every iteration; every patch size around min_points, a wavefront, the sums' chunk and the size classes; batches of
1 .. 65 frames with empty and non-finite frames; every combination of outputs with guard words; the map form and its budget; the refusals
and the struct layout; the handle's map with a step before and after; the synthetic world.  tests/test_ground_on_cpu.py re-runs this
file against the CPU stand-in."""
import ctypes as C
import itertools
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
EYE = np.eye(4, dtype=np.float32)
G1 = evalmap.ground_grid(1, 8, 0.5, 64.0)  # one ring, eight sectors of 45 degrees: a cloud with 0 < y < x is one patch
OK, SPARSE, DEGENERATE, UPRIGHT, ELEVATION = (evalmap.GROUND_OK, evalmap.GROUND_SPARSE, evalmap.GROUND_DEGENERATE,
                                              evalmap.GROUND_REJECTED_UPRIGHT, evalmap.GROUND_REJECTED_ELEVATION)


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


def step32(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


def step64(v, up):
    return float(np.nextafter(np.float64(v), np.inf if up else -np.inf))


def assert_same_scans(got, want, what):
    """(codes, rows, result, patches) twice: the same bytes and the same numbers"""
    assert got[0].dtype == np.uint8 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    if got[0].tobytes() != want[0].tobytes():
        bad = np.flatnonzero(got[0] != want[0])
        assert False, (what, "codes", len(bad), bad[:5], got[0][bad[:5]], want[0][bad[:5]])
    assert got[1] == want[1], (what, "rows", [(f, a, b) for f, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:3])
    assert got[2] == want[2], (what, got[2], want[2])
    for r in got[1]:
        assert tuple(r.keys()) == evalmap.GROUND_ROW_FIELDS
    assert (got[3] is None) == (want[3] is None)
    if got[3] is not None:
        assert got[3].dtype == evalmap.GROUND_PATCH_DTYPE and got[3].shape == want[3].shape
        if got[3].tobytes() != want[3].tobytes():
            bad = np.flatnonzero(got[3].reshape(-1) != want[3].reshape(-1))
            assert False, (what, "patches", len(bad), bad[:3], got[3].reshape(-1)[bad[:2]], want[3].reshape(-1)[bad[:2]])


def check(g, scans, grid=G1, what="", patches=True, **kw):
    """the device against the normative text (and the pure-Python one on a small input); what the normative text returned"""
    want = evalmap.ground_scans(scans, grid, patches=patches, **kw)
    assert_same_scans(g.ground_scans(scans, grid, patches=patches, **kw), want, what)
    if sum(len(s) for s in scans) <= 1500:
        assert_same_scans(evalmap.ground_scans_brute(scans, grid, patches=patches, **kw), want, (what, "the pure-Python restatement"))
    return want


def assert_same_votes(got, want, what):
    """(votes, mask, kept rows, rows, result) twice"""
    for j, (name, dt) in enumerate((("votes", np.uint16), ("mask", np.uint8), ("kept", np.float32))):
        a, b = got[j], want[j]
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(1))
            assert False, (what, name, len(bad), bad[:5], a[bad[:3]], b[bad[:3]])
    assert got[3] == want[3], (what, "rows", [(f, a, b) for f, (a, b) in enumerate(zip(got[3], want[3])) if a != b][:3])
    assert tuple(got[4].keys()) == evalmap.GROUND_VOTES_RESULT_FIELDS and got[4] == want[4], (what, got[4], want[4])
    for r in got[3]:
        assert tuple(r.keys()) == evalmap.GROUND_VOTES_ROW_FIELDS


def check_votes(g, cloud, T, Tl=None, grid=G1, what="", **kw):
    want = evalmap.ground_votes(cloud, T, Tl, grid, **kw)
    assert_same_votes(g.ground_votes(T, Tl, cloud, grid, **kw), want, what)
    return want


def floor(n, seed, noise=0.02, z0=-1.75, label=40.0):
    """n points of a noisy floor at z0 inside sector 0 of G1 (0 < y < x)"""
    r = np.random.default_rng(seed)
    x = r.uniform(4, 30, n)
    y = r.uniform(0.05, 0.9, n) * x
    z = z0 + r.normal(0, noise, n)
    return xyzi(np.stack([x, y, z], 1), label)


def status_of(want, f=0, ring=0, sector=0):
    return int(want[3]["status"][f, ring, sector])


# ---- 1. known answers ----
def lattice(tilt_x=0.0, tilt_y=0.0):
    """16 x 16 dyadic points of the plane z = -1.75 + tilt_x * y + tilt_y * x inside sector 0, under a box of 27 points"""
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    x, y = 4.0 + i.reshape(-1) / 4.0, 0.125 + j.reshape(-1) / 8.0
    pl = lambda x, y: -1.75 + tilt_x * y + tilt_y * x
    bx, by, bz = np.meshgrid(6.0 + np.arange(3) / 4.0, 1.0 + np.arange(3) / 4.0, np.arange(3) / 4.0, indexing="ij")
    bx, by, bz = bx.reshape(-1), by.reshape(-1), bz.reshape(-1)
    box = np.stack([bx, by, pl(bx, by) + 0.5 + bz], 1)  # (its lowest layer is not below lpr + th_seeds)
    return xyzi(np.concatenate([np.stack([x, y, pl(x, y)], 1), box])), 256


def test_a_dyadic_lattice_under_a_box_is_the_plane_exactly(handle):
    scan, n = lattice()
    want = check(handle, [scan], what="lattice")
    row = want[3][0, 0, 0]
    assert row["status"] == OK and row["n_points"] == len(scan) and row["n_ground"] == n
    assert row["normal"].tolist() == [0.0, 0.0, 1.0] and row["d"] == 1.75 and row["mean_z"] == -1.75 and row["eig"][0] == 0.0
    assert (want[0][:n] == 1).all() and (want[0][n:] == 0).all()
    assert want[1][0]["n_ground"] == n and want[1][0]["n_judged"] == len(scan) and want[1][0]["n_patches"] == 1


@pytest.mark.parametrize("tilt_x,tilt_y", [(0.25, 0.0), (0.0, 0.125), (-0.125, 0.0625)])
def test_the_same_plane_tilted(handle, tilt_x, tilt_y):
    scan, n = lattice(tilt_x, tilt_y)
    want = check(handle, [scan], what="tilted")
    row = want[3][0, 0, 0]
    nrm = np.float64([-tilt_y, -tilt_x, 1.0]) / np.sqrt(1.0 + tilt_x * tilt_x + tilt_y * tilt_y)
    assert row["status"] == OK and row["n_ground"] == n and np.abs(row["normal"] - nrm).max() < 1e-12 and abs(row["d"] - 1.75 * nrm[2]) < 1e-12
    assert (want[0][:n] == 1).all() and (want[0][n:] == 0).all()


def test_a_wall_alone_in_a_patch_is_rejected_as_not_upright(handle):
    y, z = np.meshgrid(1.0 + np.arange(12) / 8.0, -1.75 + np.arange(12) / 4.0, indexing="ij")
    wall = xyzi(np.stack([np.full(144, 10.0), y.reshape(-1), z.reshape(-1)], 1))
    want = check(handle, [wall], what="wall")
    row = want[3][0, 0, 0]
    assert row["status"] == UPRIGHT and row["n_ground"] == 0 and abs(row["normal"][2]) < 1e-9 and abs(abs(row["normal"][0]) - 1.0) < 1e-9
    assert (want[0] == 0).all() and want[1][0]["n_rejected_upright"] == 1 and want[1][0]["n_judged"] == 144 and want[1][0]["n_ground"] == 0


# ---- 2. the grid's edges ----
def test_points_one_step_either_side_of_every_ring_and_sector_edge(handle):
    grid = evalmap.ground_grid(3, 16, 1.0, 4.0)  # ring edges 1 2 3 4; sector edges every 22.5 degrees
    t8 = np.float32(np.tan(np.pi / 8))
    pts = []
    for sx, sy, swap in itertools.product((1, -1), (1, -1), (False, True)):  # the eight octants
        put = lambda a, b: pts.append((sx * b, sy * a, -1.75) if swap else (sx * a, sy * b, -1.75))
        for r in (1.0, 2.0, 3.0, 4.0):  # the ring edges along the octant's axis and along its diagonal
            for v in (step32(r, False), np.float32(r), step32(r, True)):
                put(v, 0.0)
            d = np.float32(r / np.sqrt(2.0))
            for v in (step32(d, False), d, step32(d, True)):
                put(v, d)
        for b in (np.float32(0.0), step32(0.0, True), step32(2.5 * t8, False), np.float32(2.5 * t8), step32(2.5 * t8, True), step32(2.5, False),
                  np.float32(2.5)):  # the sector edges at 0, 22.5 and 45 degrees
            put(np.float32(2.5), b)
    pts += [(0.0, 0.0, -1.75), (0.0, 0.0, 0.0), (-0.0, 0.0, 1.0)]  # on the axis
    scan = xyzi(pts)
    want = check(handle, [scan], grid, what="edges", min_points=3)
    ring, sec = evalmap.ground_patch_of(scan[:, 0].astype(np.float64), scan[:, 1].astype(np.float64), grid)
    assert want[1][0]["n_out_of_range"] == int((ring < 0).sum()) and (ring[-3:] == -1).all() and (want[0][ring < 0] == 2).all()
    assert 0 < (ring < 0).sum() < len(scan) and len(np.unique(sec[ring >= 0])) == 16 and len(np.unique(ring[ring >= 0])) == 3
    for rg, sc in set(zip(ring[ring >= 0].tolist(), sec[ring >= 0].tolist())):
        assert want[3][0, rg, sc]["n_points"] == int(((ring == rg) & (sec == sc)).sum())
    # r equal to the first and the last edge: in, and out
    ends = xyzi([(1.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, -4.0, 0.0)])
    r2, _ = evalmap.ground_patch_of(ends[:, 0].astype(np.float64), ends[:, 1].astype(np.float64), grid)
    assert r2.tolist() == [0, -1, 0, -1]
    check(handle, [ends], grid, what="the first and the last edge", min_points=3)


# ---- 3. the seeds ----
def test_equal_heights_in_every_permutation(handle):
    base = floor(6, 11)
    base[:, 2] = [-1.75, -1.75, -0.0, 0.0, -1.75, 0.0]
    scans = [np.ascontiguousarray(base[list(p)]) for p in itertools.permutations(range(6))]
    want = check(handle, scans, what="permutations", patches=True, min_points=6, num_lpr=4, min_z=-2.0)
    assert len(scans) == 720 and len({status_of(want, f) for f in range(720)}) == 1
    check(handle, scans[:24], what="permutations, only the zeros are candidates", min_points=6, num_lpr=2, min_z=0.0)


@pytest.mark.parametrize("n_cand", [9, 10, 11])
def test_a_candidate_count_below_at_and_above_num_lpr(handle, n_cand):
    s = floor(30, 3, noise=0.1)
    order = np.argsort(s[:, 2], kind="stable")
    min_z = float(s[order[30 - n_cand], 2])  # the n_cand highest are the candidates
    want = check(handle, [s], what=n_cand, min_z=min_z, th_seeds=5.0)
    assert int((s[:, 2].astype(np.float64) >= min_z).sum()) == n_cand and status_of(want) in (OK, UPRIGHT)


@pytest.mark.parametrize("num_lpr", [1, 64])
def test_num_lpr_at_its_ends(handle, num_lpr):
    s = floor(100, 4, noise=0.2)
    a = check(handle, [s], what=num_lpr, num_lpr=num_lpr, th_seeds=0.1)
    b = evalmap.ground_scans([s], G1, num_lpr=10, th_seeds=0.1, patches=True)
    assert a[3].tobytes() != b[3].tobytes()  # (the lowest-point height matters here)


def test_min_z_at_a_points_height_and_one_step_either_side(handle):
    s = floor(40, 6, noise=0.1)
    z = float(np.sort(s[:, 2])[20])
    got = [check(handle, [s], what=("min_z", k), iters=1, min_z=v) for k, v in enumerate((float(step32(z, False)), z, float(step32(z, True))))]
    assert got[0][3].tobytes() == got[1][3].tobytes() != got[2][3].tobytes()  # z >= min_z: the point is a candidate at its own height


def test_no_candidate_at_all(handle):
    s = floor(40, 7)
    want = check(handle, [s], what="no candidate", min_z=0.0)
    assert status_of(want) == DEGENERATE and (want[0] == 2).all() and want[1][0]["n_degenerate"] == 1 and want[1][0]["n_judged"] == 0


# ---- 4. the thresholds at their exact ends ----
def last_plane(s, ring=0, **kw):
    g, R, prm = evalmap._ground_args(G1, *[kw.get(k, v) for k, v in evalmap.GROUND_DEFAULTS.items()], None, None, 1)
    return evalmap.ground_fit(s[:, :3].astype(np.float64), ring, prm)


def test_th_dist_at_a_points_residual(handle):
    s = floor(60, 8, noise=0.05)
    _, _, plane = last_plane(s, iters=1, th_dist=0.15)  # (one iteration: the plane comes from the seeds alone)
    (nx, ny, nz), d = plane[0], plane[1]
    res = [((nx * float(p[0]) + ny * float(p[1])) + nz * float(p[2])) + d for p in s]
    j = int(np.argsort(res)[40])
    n_g = [check(handle, [s], what=("th_dist", k), iters=1, th_dist=v)[1][0]["n_ground"] for k, v in
           enumerate((step64(res[j], False), res[j], step64(res[j], True)))]
    assert n_g == [40, 40, 41]  # one-sided and strict: the point joins only above its own residual


def test_uprightness_at_the_normals_z(handle):
    s = floor(60, 9, noise=0.05)
    st, _, plane = last_plane(s)
    nz = plane[0][2]
    assert st == OK and 0.9 < nz < 1.0
    got = [status_of(check(handle, [s], what=("uprightness", k), uprightness=v)) for k, v in enumerate((step64(nz, False), nz, step64(nz, True)))]
    assert got == [OK, OK, UPRIGHT]


def test_elevation_and_flatness_at_their_exact_ends(handle):
    s = floor(60, 10, noise=0.05)
    st, _, plane = last_plane(s)
    mean_z, ratio = plane[2], plane[3][0] / plane[4]
    assert st == OK and ratio > 0
    tab = lambda v: np.float64([v])
    for k, (el, fl, expect) in enumerate(((mean_z, 0.0, OK), (step64(mean_z, True), 0.0, OK), (step64(mean_z, False), 0.0, ELEVATION),
                                          (step64(mean_z, False), ratio, OK), (step64(mean_z, False), step64(ratio, True), OK),
                                          (step64(mean_z, False), step64(ratio, False), ELEVATION), (-np.inf, np.inf, OK), (-np.inf, -np.inf, ELEVATION))):
        want = check(handle, [s], what=("elevation", k), elevation=tab(el), flatness=tab(fl))
        assert status_of(want) == expect, (k, status_of(want))
        assert want[1][0]["n_rejected_elevation"] == (expect == ELEVATION) and (want[1][0]["n_ground"] > 0) == (expect == OK)


# ---- 5. degenerate patches ----
@pytest.mark.parametrize("iteration,kw", [(1, dict(min_z=None)), (2, dict(th_dist=-1.0)), (3, dict(th_dist=-0.05))])
def test_members_dropping_below_three(handle, iteration, kw):
    s = floor(40, 5, noise=0.05)
    if iteration == 1:
        kw = dict(min_z=float(np.sort(s[:, 2])[38]))  # two candidates: two seeds
    if iteration > 1:
        assert status_of(evalmap.ground_scans([s], G1, patches=True, iters=iteration - 1, **kw)) != DEGENERATE
    want = check(handle, [s], what=("degenerate in iteration", iteration), iters=iteration, **kw)
    assert status_of(want) == DEGENERATE and (want[0] == 2).all() and want[3][0, 0, 0]["n_ground"] == 0 and not want[3][0, 0, 0]["normal"].any()


def test_identical_and_collinear_points(handle):
    same = xyzi(np.tile([[4.0, 1.0, -1.75]], (16, 1)))
    i = np.arange(16)
    line = xyzi(np.stack([4.0 + i / 4.0, np.full(16, 1.0), np.full(16, -1.75)], 1))
    want = check(handle, [same, line], what="identical, collinear")
    assert status_of(want, 0) == DEGENERATE and status_of(want, 1) == UPRIGHT  # (a line's normal is arbitrary; here it is (0, 1, 0))
    assert want[3][1, 0, 0]["normal"].tolist() == [0.0, 1.0, 0.0] and want[3][1, 0, 0]["eig"][1] == 0.0


# ---- 6. the sizes ----
W, SM, LDS = evalmap.GROUND_WAVE_POINTS, evalmap.GROUND_SMALL_POINTS, evalmap.GROUND_LDS_POINTS
SIZES = [1, 2, 3, 9, 10, 11, W - 1, W, W + 1, 255, 256, 257, 511, 512, 513, SM - 1, SM, SM + 1, LDS - 1, LDS, LDS + 1]


def test_the_size_classes_mirror_the_header(gpu_mod):
    assert (W, SM, LDS) == (gpu_mod.GROUND_WAVE_POINTS, gpu_mod.GROUND_SMALL_POINTS, gpu_mod.GROUND_LDS_POINTS) == (64, 1024, 4096)
    text = open(os.path.join(ROOT, "include", "erasor_hip.h")).read()
    for name, v in (("WAVE", W), ("SMALL", SM), ("LDS", LDS)):
        assert "#define ERASOR_GROUND_%s_POINTS %du" % (name, v) in text


def test_every_patch_size_around_every_edge(handle):
    scans = [floor(n, 100 + n, noise=0.03) for n in SIZES]
    for k, s in enumerate(scans):
        s[::7, 2] += 1.0  # (some points off the floor: both codes)
        s[3::11, 3] = 252.0
    want = check(handle, scans, what="sizes")
    for f, n in enumerate(SIZES):
        assert want[3][f, 0, 0]["n_points"] == n and status_of(want, f) == (SPARSE if n < 10 else OK), (n, status_of(want, f))
        if n >= 10:
            assert 0 < want[1][f]["n_ground_dynamic"] < want[1][f]["n_ground"] < n
    # the same sizes side by side in one frame (eight sectors, three calls), so that a launch holds every class at once
    for k in range(0, len(SIZES), 8):
        parts = []
        for o, s in enumerate(scans[k:k + 8]):
            a = o * (np.pi / 4)
            c, sn = np.cos(a), np.sin(a)
            p = s.copy()
            p[:, 0], p[:, 1] = np.float32(c * s[:, 0] - sn * s[:, 1]), np.float32(sn * s[:, 0] + c * s[:, 1])
            parts.append(p)
        frame = np.ascontiguousarray(np.concatenate(parts)[np.random.default_rng(k).permutation(sum(len(p) for p in parts))])
        w2 = check(handle, [frame], what=("side by side", k))
        assert sorted(w2[3][0, 0]["n_points"].tolist())[-len(parts):] == sorted(len(p) for p in parts)


def test_one_patch_holding_the_whole_scan_streams_from_memory(handle):
    n = 3 * LDS + 100 if ON_CPU else 40 * LDS + 100
    s = floor(n, 77, noise=0.03)
    s[::5, 2] += 0.7
    want = check(handle, [s], what="whole scan", num_lpr=64)
    assert want[3][0, 0, 0]["n_points"] == n and status_of(want) == OK and 0 < want[1][0]["n_ground"] < n


# ---- 7. the batches ----
@pytest.mark.parametrize("n_frames", [1, 2, 63, 64, 65])
def test_batches_with_empty_and_non_finite_frames(handle, n_frames):
    scans = [floor(12 + (7 * f) % 90, 200 + f, noise=0.03) for f in range(n_frames)]
    empty = np.zeros((0, 4), np.float32)
    if n_frames >= 2:
        scans[0] = empty
        scans[-1] = empty
    if n_frames >= 63:
        scans[31] = empty
        scans[32] = empty
        bad = floor(20, 1)
        bad[:, 0], bad[3, 1], bad[5, 2] = np.nan, np.inf, -np.inf
        scans[40] = bad
        scans[41][2, 2] = np.nan
    want = check(handle, scans, what=n_frames)
    if n_frames >= 63:
        assert want[1][40]["n_non_finite"] == 20 and want[1][40]["n_patches"] == 0 and want[1][41]["n_non_finite"] == 1
        assert (want[0][int(sum(len(s) for s in scans[:40])):][:20] == 255).all()
    # more than one batch of frames: the finest grid, whose table is cut after 32 frames
    if n_frames == 65:
        fine = evalmap.ground_grid(64, 512, 0.5, 64.0)
        w2 = check(handle, scans, fine, what="the finest grid", patches=False, min_points=3)
        assert w2[2]["n_patches"] > 65


def test_nothing_at_all(handle):
    want = check(handle, [], what="no frame")
    assert want[0].shape == (0,) and want[1] == [] and want[2]["n_frames"] == 0 and want[3].shape == (0, 1, 8)
    want = check(handle, [np.zeros((0, 4), np.float32)] * 3, what="three empty frames")
    assert want[2]["n_points"] == 0 and not want[3]["status"].any()
    g = handle
    v = check_votes(g, np.zeros((0, 4), np.float32), np.stack([EYE] * 2), what="an empty map")
    assert v[0].shape == (0, 2) and v[4]["n_points"] == 0
    v = check_votes(g, floor(50, 1), np.zeros((0, 4, 4), np.float32), what="no frame", keep=0)
    assert v[4]["n_unseen"] == 50 and v[4]["n_kept"] == 50 and len(v[2]) == 50


# ---- 8. the interface ----
def params_of(gpu_mod, kept, grid=G1, **kw):
    a = dict(evalmap.GROUND_DEFAULTS, elevation=None, flatness=None, min_votes=1, ratio=0.5, keep=1, work_budget_bytes=0)
    a.update(kw)
    g = gpu_mod.Erasor._ground_params(None, grid, a["num_lpr"], a["th_seeds"], a["th_dist"], a["iters"], a["min_points"], a["min_z"], a["uprightness"],
                                      a["elevation"], a["flatness"], kept, a["min_votes"], a["ratio"], a["keep"], a["work_budget_bytes"])
    return g[0]


def raw_scans(gpu_mod, g, scans, prm, outs):
    """erasor_hip_ground_scans through ctypes with the buffers given (None: NULL); the return code"""
    cat = np.ascontiguousarray(np.concatenate(scans) if scans else np.zeros((0, 4), np.float32), np.float32)
    offs = np.zeros(len(scans) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in scans])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    codes, rows, patches, res = outs
    return gpu_mod.lib().erasor_hip_ground_scans(g._h, p(cat), C.c_size_t(len(cat)), p(offs), C.c_size_t(len(scans)), C.c_int(0),
                                                 None if prm is None else C.byref(prm), p(codes), rows, p(patches), None if res is None else C.byref(res))


def raw_votes(gpu_mod, g, cloud, T, prm, outs, cap=None, map_call=False):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    Tb = np.ascontiguousarray(T, np.float32)
    votes, mask, kept, rows, res = outs
    head = () if map_call else (p(cloud), C.c_size_t(len(cloud)), C.c_int(0))
    fn = gpu_mod.lib().erasor_hip_ground_votes_map if map_call else gpu_mod.lib().erasor_hip_ground_votes_clouds
    return fn(g._h, *head, None, p(Tb), C.c_size_t(len(Tb)), None if prm is None else C.byref(prm), p(votes), p(mask), p(kept),
              C.c_size_t(len(cloud) if cap is None else cap), rows, None if res is None else C.byref(res))


def world_patch(seed, n=300):
    """a floor with a box on it and labelled wheels in it, seen from three poses"""
    c = floor(n, seed, noise=0.02, z0=0.0)
    c[::6, 2] += 0.8
    c[::9, 3] = 252.0
    T = np.stack([EYE] * 3)
    T[:, 2, 3] = 1.75
    T[1, 0, 3], T[2, 1, 3] = 1.0, -1.0
    return c, T


def test_every_combination_of_outputs_and_the_words_behind_them(handle, gpu_mod):
    scans = [floor(90, 21), np.zeros((0, 4), np.float32), floor(130, 22)]
    scans[2][::4, 2] += 1.0
    want = evalmap.ground_scans(scans, G1, patches=True)
    n, nf, npatch = sum(len(s) for s in scans), 3, 3 * 8
    kept = []
    prm = params_of(gpu_mod, kept)
    for use in itertools.product((False, True), repeat=4):
        codes = np.full(n + 8, 0x77, np.uint8)
        patches = np.full((npatch + 1) * 80, 0x77, np.uint8)
        rows, res = (gpu_mod.GroundRow * (nf + 1))(), gpu_mod.GroundResult()
        rows[nf].n_points = res.n_points = 12345
        outs = [b if u else None for b, u in zip((codes, rows, patches, res), use)]
        assert raw_scans(gpu_mod, handle, scans, prm, outs) == 0, (use, gpu_mod.lib().erasor_hip_last_error(handle._h))
        assert (codes[n:] == 0x77).all() and (patches[npatch * 80:] == 0x77).all() and rows[nf].n_points == 12345, use
        assert codes[:n].tobytes() == want[0].tobytes() if use[0] else (codes == 0x77).all(), use
        assert [rows[f].as_dict() for f in range(nf)] == want[1] if use[1] else all(rows[f].n_points == 0 for f in range(nf)), use
        assert patches[:npatch * 80].tobytes() == want[3].tobytes() if use[2] else (patches == 0x77).all(), use
        assert {k: v for k, v in res.as_dict().items() if k in want[2]} == want[2] if use[3] else res.n_points == 12345, use
    # the map form
    cloud, T = world_patch(31)
    wv = evalmap.ground_votes(cloud, T, None, G1)
    n, nk = len(cloud), wv[4]["n_kept"]
    assert 0 < nk < n and 0 < wv[4]["n_ground_dynamic"] < wv[4]["n_ground"]
    for use in itertools.product((False, True), repeat=5):
        votes, mask, out = np.full(2 * n + 8, 0x7777, np.uint16), np.full(n + 8, 0x77, np.uint8), np.full(4 * n + 8, 7.0, np.float32)
        rows, res = (gpu_mod.GroundRow * (nf + 1))(), gpu_mod.GroundResult()
        rows[nf].n_points = res.n_points = 12345
        outs = [b if u else None for b, u in zip((votes, mask, out, rows, res), use)]
        assert raw_votes(gpu_mod, handle, cloud, T, prm, outs) == 0, (use, gpu_mod.lib().erasor_hip_last_error(handle._h))
        for b, u, m, w, fill in ((votes, use[0], 2 * n, wv[0], 0x7777), (mask, use[1], n, wv[1], 0x77), (out, use[2], 4 * nk, wv[2], 7.0)):
            assert (b[m:] == fill).all(), use
            assert b[:m].tobytes() == w.tobytes() if u else (b[:m] == fill).all(), use
        assert rows[nf].n_points == 12345
        assert [rows[f].as_dict(gathered=True) for f in range(nf)] == wv[3] if use[3] else all(rows[f].n_points == 0 for f in range(nf))
        assert (res.n_map_ground, res.n_map_unseen, res.n_kept) == (wv[4]["n_ground"], wv[4]["n_unseen"], nk) if use[4] else res.n_points == 12345
    # rows that do not fit: the result first, then the code
    res = gpu_mod.GroundResult()
    out = np.full(4 * n, 7.0, np.float32)
    assert raw_votes(gpu_mod, handle, cloud, T, prm, [None, None, out, None, res], cap=nk - 1) == E_CAPACITY
    assert (res.n_map_ground, res.n_kept, res.n_map_points) == (wv[4]["n_ground"], nk, n) and (out == 7.0).all()


def test_refusals_each_naming_its_argument_and_the_struct_layout(gpu_mod, tmp_path):
    # (the handle is closed here, not left to the collector: pytest.raises keeps the frame, and with it the handle, in a reference cycle,
    # and a handle must be destroyed by the library that made it -- tests/hooks.py puts another build in the library's place for a while)
    g = gpu_mod.Erasor(gpu_mod.params_default())
    try:
        refusals(gpu_mod, tmp_path, g)
    finally:
        g.close()


def refusals(gpu_mod, tmp_path, g):
    scans = [floor(50, 1), floor(60, 2)]
    cloud, T = world_patch(3, 100)
    L = gpu_mod.lib()
    err = lambda: L.erasor_hip_last_error(g._h).decode()
    none4, none5 = [None] * 4, [None] * 5

    def refused(sentence, grid=G1, **kw):
        kept = []
        prm = params_of(gpu_mod, kept, grid, **kw)
        assert raw_scans(gpu_mod, g, scans, prm, none4) == E_INVALID, sentence
        assert err() == "erasor_hip_ground_scans: " + sentence, err()
        assert raw_votes(gpu_mod, g, cloud, T, prm, none5) == E_INVALID, sentence
        assert err() == "erasor_hip_ground_votes_clouds: " + sentence, err()

    edge = lambda *v: dict(G1, ring_edge=np.float64(v))
    refused("n_rings must be within 1 .. 64", edge(1.0))
    refused("n_rings must be within 1 .. 64", dict(G1, ring_edge=np.arange(66.0)))
    for S in (0, 4, 12, 520):
        refused("n_sectors must be a multiple of 8 within 8 .. 512", dict(G1, n_sectors=S, col_tan=np.zeros(max(S // 8 - 1, 0))))
    for e in (edge(1.0, 1.0), edge(2.0, 1.0), edge(-0.5, 1.0), edge(0.0, np.inf), edge(np.nan, 1.0)):
        refused("ring_edge must be finite, strictly increasing and start at >= 0", e)
    for col in ((0.0,), (1.0,), (np.nan,)):
        refused("col_tan must be strictly increasing within (0, 1)", dict(G1, n_sectors=16, col_tan=np.float64(col)))
    refused("col_tan must be strictly increasing within (0, 1)", dict(G1, n_sectors=24, col_tan=np.float64([0.5, 0.5])))
    refused("elevation and flatness must not hold a NaN", elevation=np.float64([np.nan]))
    refused("elevation and flatness must not hold a NaN", flatness=np.float64([np.nan]))
    for v in (0, 65):
        refused("num_lpr must be within 1 .. 64", num_lpr=v)
    for v in (0, 17):
        refused("iters must be within 1 .. 16", iters=v)
    refused("min_points must be at least 3", min_points=2)
    for k in ("th_seeds", "th_dist", "min_z", "uprightness"):
        for v in (np.nan, np.inf):
            refused("th_seeds, th_dist, min_z and uprightness must be finite", **{k: v})
    refused("ratio must be finite", ratio=np.nan)
    # the arguments beside the parameters
    kept = []
    prm = params_of(gpu_mod, kept)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cat = np.concatenate(scans)
    sc = lambda o, n_f, q, n=110, pts=p(cat): L.erasor_hip_ground_scans(g._h, pts, C.c_size_t(n), None if o is None else p(o), C.c_size_t(n_f), C.c_int(0), q,
                                                                        None, None, None, None)
    good = np.uint64([0, 50, 110])
    assert sc(good, 2, None) == E_INVALID and err() == "erasor_hip_ground_scans: params is NULL"
    assert sc(None, 2, C.byref(prm)) == E_INVALID and err() == "erasor_hip_ground_scans: offsets is NULL (n_frames + 1 entries)"
    assert sc(np.uint64([0, 70, 50]), 2, C.byref(prm)) == E_INVALID and err() == "erasor_hip_ground_scans: offsets decrease"
    assert sc(np.uint64([1, 50, 110]), 2, C.byref(prm)) == E_INVALID and err() == "erasor_hip_ground_scans: offsets[0] must be 0"
    assert sc(np.uint64([0, 50, 100]), 2, C.byref(prm)) == E_INVALID and err() == "erasor_hip_ground_scans: the last offset is not the scans' point count"
    assert sc(good, 2, C.byref(prm), pts=None) == E_INVALID and err() == "erasor_hip_ground_scans: NULL scans"
    assert sc(np.uint64([0, (1 << 30) + 1]), 1, C.byref(prm), n=(1 << 30) + 1) == E_INVALID and err() == "erasor_hip_ground_scans: more than 2^30 scan points"
    many = np.zeros(65537, np.uint64)
    assert sc(many, 65536, C.byref(prm), n=0) == E_INVALID and err() == "erasor_hip_ground_scans: more than 65535 frames"
    assert sc(many, 65535, C.byref(prm), n=0) == 0
    vt = lambda Tb, n_f, Tl=None, cl=p(cloud), n=100: L.erasor_hip_ground_votes_clouds(g._h, cl, C.c_size_t(n), C.c_int(0), Tl, None if Tb is None else p(Tb),
                                                                                       C.c_size_t(n_f), C.byref(prm), None, None, None, C.c_size_t(0), None,
                                                                                       None)
    who = "erasor_hip_ground_votes_clouds: "
    assert vt(None, 3) == E_INVALID and err() == who + "T_body2origin is NULL"
    bad = T.copy()
    bad[1, 0, 3] = np.inf
    assert vt(bad, 3) == E_INVALID and err() == who + "non-finite entry in T_body2origin"
    bad_l = EYE.copy()
    bad_l[2, 3] = np.nan
    assert vt(T, 3, p(bad_l)) == E_INVALID and err() == who + "non-finite entry in T_lidar2body"
    assert vt(T, 3, cl=None) == E_INVALID and err() == who + "NULL map or more than 2^30 map points"
    assert vt(T, 3, n=(1 << 30) + 1) == E_INVALID and err() == who + "NULL map or more than 2^30 map points"
    assert vt(np.zeros((65536, 16), np.float32), 65536) == E_INVALID and err() == who + "more than 65535 frames"
    # the handle's map: none yet -- the error carve_map gives
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.carve(scans, T[:2], None, None)
    assert e.value.rc == E_STATE
    sentence = err().split(": ", 1)[1]
    assert raw_votes(gpu_mod, g, cloud, T, prm, none5, map_call=True) == E_STATE and err() == "erasor_hip_ground_votes_map: " + sentence
    # a step in flight: every entry point is refused, and the handle is fine after step_wait
    ssc = scenarios.small(n_frames=2, az=60)
    g.set_map(ssc["map"])
    g.step_async(ssc["scans"][0], T_l2b=ssc["T_l2b"], T_b2o=ssc["T_b2o"][0], T_o2b=ssc["T_o2b"][0])
    for rc in (raw_scans(gpu_mod, g, scans, prm, none4), raw_votes(gpu_mod, g, cloud, T, prm, none5), raw_votes(gpu_mod, g, cloud, T, prm, none5, map_call=True)):
        assert rc == E_STATE and "in flight" in err(), err()
    for fn, a in ((g.ground_scans, (scans,)), (g.ground_votes, (T, None, cloud)), (g.ground_votes, (T,))):
        with pytest.raises(gpu_mod.ErasorError) as e:
            fn(*a)
        assert e.value.rc == E_STATE and "in flight" in err()
    g.step_wait()
    m = np.ascontiguousarray(g.get_map(), np.float32)
    assert_same_votes(g.ground_votes(T, None, None, G1), evalmap.ground_votes(m, T, None, G1), "the handle's map after the refusals")
    # a grid table that is NULL
    for name, S in (("ring_edge", 8), ("ring_edge", 16), ("col_tan", 16)):
        k2 = []
        q = params_of(gpu_mod, k2, evalmap.ground_grid(1, S, 0.5, 64.0))
        setattr(q, name, None)
        assert raw_scans(gpu_mod, g, scans, q, none4) == E_INVALID and err() == "erasor_hip_ground_scans: ring_edge or col_tan is NULL"
        assert raw_votes(gpu_mod, g, cloud, T, q, none5) == E_INVALID and err() == "erasor_hip_ground_votes_clouds: ring_edge or col_tan is NULL"
    k2 = []
    q = params_of(gpu_mod, k2)
    q.col_tan = None  # (eight sectors have no column edge: the table is not read)
    assert raw_scans(gpu_mod, g, scans, q, none4) == 0
    # the host text refuses the same
    for kw in (dict(num_lpr=0), dict(iters=17), dict(min_points=2), dict(th_dist=np.nan), dict(elevation=[np.nan]), dict(grid=edge(2.0, 1.0))):
        kw = dict(dict(grid=G1), **kw)
        with pytest.raises(ValueError):
            evalmap.ground_scans(scans, **kw)
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.ground_scans(scans, **kw)
        assert e.value.rc == E_INVALID
    check(g, scans, what="after the refusals")  # the handle is fine
    # the header's layout
    fields = [k for k, _ in gpu_mod.Ground._fields_]
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu", sizeof(erasor_ground), '
            'sizeof(erasor_ground_row), sizeof(erasor_ground_patch), sizeof(erasor_ground_result));' +
            "".join('printf(" %%zu", offsetof(erasor_ground, %s));' % f for f in fields) +
            "".join('printf(" %%zu", offsetof(erasor_ground_patch, %s));' % f for f in ("status", "n_points", "n_ground", "normal", "d", "mean_z", "eig")) +
            'printf(" %zu %zu\\n", offsetof(erasor_ground_row, n_gathered), offsetof(erasor_ground_result, n_kept));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    V, R, P, S = gpu_mod.Ground, gpu_mod.GroundRow, gpu_mod.GroundPatch, gpu_mod.GroundResult
    dt = evalmap.GROUND_PATCH_DTYPE
    mirror = ([C.sizeof(V), C.sizeof(R), C.sizeof(P), C.sizeof(S)] + [getattr(V, f).offset for f in fields] +
              [dt.fields[f][1] for f in ("status", "n_points", "n_ground", "normal", "d", "mean_z", "eig")] + [R.n_gathered.offset, S.n_kept.offset])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == mirror
    assert mirror[:4] == [112, 96, 80, 144] and dt.itemsize == 80 and mirror[-2:] == [88, 136]
    assert [getattr(P, f).offset for f in ("status", "n_points", "n_ground", "normal", "d", "mean_z", "eig")] == mirror[-9:-2]
    assert tuple(k for k, _ in R._fields_) == evalmap.GROUND_VOTES_ROW_FIELDS


# ---- 9. the map form ----
def test_the_votes_are_the_scans_of_the_gathered_clouds(handle):
    cloud, T = world_patch(41, 400)
    cloud[5, 0] = np.nan          # a non-finite map point: gathered by no frame
    cloud[6, :2] = (500.0, 100.0)  # out of every frame's rings
    Tl = EYE.copy()
    Tl[:3, 3] = (0.25, 0.0, 0.5)
    want = check_votes(handle, cloud, T, Tl, what="votes")
    assert_same_votes(evalmap.ground_votes_brute(cloud, T, Tl, G1), want, "the pure-Python restatement")
    clouds, idx = evalmap.ground_gather(cloud, T, Tl, G1)
    codes, rows, res, _ = handle.ground_scans(clouds, G1)
    votes = np.zeros((len(cloud), 2), np.uint16)
    o = 0
    for f, ix in enumerate(idx):
        c = codes[o:o + len(ix)]
        o += len(ix)
        votes[ix[c <= 1], 0] += 1
        votes[ix[c == 1], 1] += 1
        assert {k: v for k, v in want[3][f].items() if k != "n_gathered"} == rows[f] and want[3][f]["n_gathered"] == len(ix)
    assert votes.tobytes() == want[0].tobytes() and (want[0][[5, 6]] == 0).all() and want[4]["n_unseen"] >= 2
    assert want[1].tobytes() == evalmap.ground_decide(votes, 1, 0.5).astype(np.uint8).tobytes() and 0 < want[4]["n_ground"] < len(cloud)
    # the rest instead of the ground
    rest = check_votes(handle, cloud, T, Tl, what="keep = 0", keep=0)
    assert len(rest[2]) + len(want[2]) == len(cloud) and rest[2].tobytes() == cloud[want[1] == 0].tobytes()


def test_the_work_budget_only_cuts_the_batches(handle):
    cloud, _ = world_patch(42, 500)
    T = np.stack([EYE] * 7)
    T[:, 2, 3] = 1.75
    T[:, 0, 3] = np.arange(7) * 0.5
    want = evalmap.ground_votes(cloud, T, None, G1)
    for budget in (1, len(cloud) * 16 * 2, len(cloud) * 16 * 3 + 5, 0):  # one frame per batch, two, three, all
        assert_same_votes(handle.ground_votes(T, None, cloud, G1, work_budget_bytes=budget), want, budget)


def test_ratio_and_min_votes_at_their_exact_ends(handle):
    cloud, _ = world_patch(43, 300)
    cloud[1::4, 2] += np.random.default_rng(5).uniform(0.05, 0.25, len(cloud[1::4])).astype(np.float32)  # (points about th_dist above the floor)
    T = np.stack([EYE] * 5)
    T[:, 2, 3] = 1.75
    T[:, 2, 3] += np.float32([0.0, 0.05, 0.1, 0.3, 0.6])  # (the sensor's height moves: the votes differ between frames)
    T[:, 0, 3] = np.arange(5) * 2.0
    base = evalmap.ground_votes(cloud, T, None, G1)
    v = base[0].astype(np.int64)
    mixed = np.flatnonzero((v[:, 1] > 0) & (v[:, 1] < v[:, 0]))
    assert len(mixed)
    i = int(mixed[0])
    seen, gr = int(v[i, 0]), int(v[i, 1])
    ratio = gr / seen
    for r, is_ground in ((ratio, float(gr) > ratio * float(seen)), (step64(ratio, False), True), (step64(ratio, True), False)):
        w = check_votes(handle, cloud, T, what=("ratio", r), ratio=r)
        assert bool(w[1][i]) == is_ground and w[0].tobytes() == base[0].tobytes()
    for mv, is_ground in ((gr, True), (gr + 1, False)):
        w = check_votes(handle, cloud, T, what=("min_votes", mv), min_votes=mv, ratio=0.0)
        assert bool(w[1][i]) == is_ground
    # a point no frame sees
    far = np.concatenate([cloud, xyzi([(900.0, 1.0, 0.0)])])
    w = check_votes(handle, far, T, what="unseen")
    assert (w[0][-1] == 0).all() and w[1][-1] == 0 and w[4]["n_unseen"] >= 1


def test_the_map_call_with_a_step_before_and_after_it(gpu_mod):
    from oracle import orc  # checker only
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, o = gpu_mod.Erasor(scenarios.to_product_params(sc["params"])), orc.Oracle(sc["params"])
    for e in (g, o):
        e.set_map(sc["map"])
        for f in range(n - 1):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    T = np.stack(sc["T_b2o"][:3])
    grid = evalmap.ground_grid(10, 16, 0.5, 80.0)
    for f in (n - 1, n):
        m = np.ascontiguousarray(g.get_map(), np.float32)
        assert m.tobytes() == np.ascontiguousarray(o.get_map(), np.float32).tobytes()
        want = evalmap.ground_votes(m, T, sc["T_l2b"], grid)
        assert_same_votes(g.ground_votes(T, sc["T_l2b"], None, grid), want, ("the handle's map before step", f))
        assert_same_votes(g.ground_votes(T, sc["T_l2b"], m, grid), want, ("the same map given", f))
        assert g.get_map().tobytes() == m.tobytes()  # the map itself stays as it is
        assert 0 < want[4]["n_ground"] < len(m)
        # the step after the call is the oracle's, bit for bit
        a = g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        b = o.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        assert a.n_map_rejected == b.n_map_rejected and a.n_reverted_bins == b.n_reverted_bins
        assert np.ascontiguousarray(g.get_map(), np.float32).tobytes() == np.ascontiguousarray(o.get_map(), np.float32).tobytes()
        assert (g.get_rejected_indices() == o.get_rejected_indices()).all() and (g.get_status() == o.get_status()).all()
    g.close()


# ---- 10. the synthetic world ----
def test_the_synthetic_world(handle):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    scans = sc["scans"][:3]
    grid = evalmap.ground_grid(10, 16, 0.5, 80.0)
    kw = dict(min_z=-1.72, elevation=np.full(10, -1.2), flatness=np.full(10, 1e-3))
    want = check(handle, scans, grid, what="world", **kw)
    assert set(np.unique(want[3]["status"]).tolist()) == {0, 1, 2, 3, 4, 5}  # every patch status
    o = 0
    for f, s in enumerate(scans):
        c = want[0][o:o + len(s)]
        o += len(s)
        assert (c == 0).any() and (c == 1).any() and 0 < want[1][f]["n_ground_dynamic"] < want[1][f]["n_ground"]
    # the defaults, and the same from a device buffer
    want = check(handle, scans, None, what="world, the default grid")
    cat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32).reshape(-1, 4) for s in scans]))
    q = handle.device_array(cat)
    try:
        offs = np.cumsum([0] + [len(s) for s in scans])
        assert_same_scans(handle.ground_scans((q, offs), None, patches=True), want, "device buffer")
    finally:
        handle.device_free(q)
