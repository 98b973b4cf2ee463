"""Carving free space on the device (erasor_hip_carve_*, kernels in carve.hip.h) against its normative host text evalmap.carve, byte for
byte -- votes, log-odds, mask, kept cloud, frame rows and result -- and against the pure-Python carve_brute where the input is small.
Known answers that do not rest on the restatement: the listed walks read back through a map with a point in every voxel of a cube, under
the identity, under a yawed and translated pose and through T_lidar2body; N = 0 and N = 1; long rays in all eight sign octants across
the grid's origin and many block borders; stop_short around N; the lidar's own voxel.  The occupancy structure: a full block and the
rank of its last bit, the eight blocks round the origin corner, two points in a voxel, a lattice of 8000 blocks that forces probing, a
non-finite map point.  Hits before misses within a frame and across two; the integration with the default log-odds, its clamps and its
order; batches of 1 .. 65 frames with an empty frame among them; every size around a wavefront and a workgroup; the gates at their exact
ends; every combination of outputs with guard words; the refusals and the struct layout; the handle's map with a step after it; the
synthetic world.  tests/test_carve_on_cpu.py re-runs this file against the CPU stand-in."""
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
LG = evalmap.carve_logodds()
L_HIT, L_MISS, L_MIN, L_MAX = (np.float32(LG[k]) for k in ("l_hit", "l_miss", "l_min", "l_max"))


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


def assert_same(got, want, what):
    """(votes, logodds, mask, kept, rows, result) twice: the same bytes and the same numbers"""
    for j, (name, dt) in enumerate((("votes", np.uint16), ("logodds", np.float32), ("mask", np.uint8), ("kept", np.float32))):
        g, w = got[j], want[j]
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(1))
            assert False, (what, name, len(bad), bad[:5], g[bad[:3]], w[bad[:3]])
    assert got[4] == want[4], (what, "rows", [(f, a, b) for f, (a, b) in enumerate(zip(got[4], want[4])) if a != b][:3])
    assert tuple(got[5].keys()) == evalmap.CARVE_RESULT_FIELDS and got[5] == want[5], (what, got[5], want[5])
    for r in got[4]:
        assert tuple(r.keys()) == evalmap.CARVE_ROW_FIELDS


def check(g, cloud, scans, T, Tl=None, what="", **kw):
    """the device against the normative text (and the pure-Python one on a small input); what the normative text returned"""
    want = evalmap.carve(cloud, scans, T, Tl, **kw)
    assert_same(g.carve(scans, T, Tl, cloud, **kw), want, what)
    if len(cloud) <= 400 and sum(len(s) for s in scans) <= 300 and kw.get("max_range", 80.0) / kw.get("voxel", 0.2) <= 100:
        assert_same(evalmap.carve_brute(cloud, scans, T, Tl, **kw), want, (what, "the pure-Python restatement"))
    return want


def step32(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


def yaw90(tx=0.0, ty=0.0, tz=0.0):
    """a quarter turn about z and a translation: exact in float32"""
    return np.float32([[0, -1, 0, tx], [1, 0, 0, ty], [0, 0, 1, tz], [0, 0, 0, 1]])


def centres(cells, voxel):
    """a point in the middle of every cell"""
    return ((np.asarray(cells, np.float64) + 0.5) * voxel).astype(np.float32)


def cube(lo, hi, voxel=1.0, shift=(0, 0, 0)):
    """(cells, cloud): one point in every voxel of the cube of cells lo .. hi per axis, moved by `shift` cells"""
    r = np.arange(lo, hi + 1)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) + np.asarray(shift)
    return cells, xyzi(centres(cells, voxel))


def votes_of(cells, walk, n_free):
    """the (hits, misses) a single ray leaves on `cells`: a miss on the first n_free voxels of the walk, a hit on its last"""
    out = np.zeros((len(cells), 2), np.uint16)
    index = {tuple(c): i for i, c in enumerate(np.asarray(cells).tolist())}
    for w in walk[:n_free]:
        if tuple(w) in index:
            out[index[tuple(w)], 1] = 1
    if tuple(walk[-1]) in index:
        out[index[tuple(walk[-1])]] = (1, 0)
    return out


def one_ray(pose, origin, end):
    """(T_body2origin, T_lidar2body, scan) that put the lidar at `origin` and its only return at `end` (small dyadic numbers: exact)"""
    o, e = np.float64(origin), np.float64(end)
    if pose == "identity":
        Tb, Tl, R = EYE.copy(), None, np.eye(3)
        Tb[:3, 3] = o
    elif pose == "yawed and translated":
        Tb, Tl = yaw90(*o), None
        R = np.float64(Tb[:3, :3])
    else:  # through T_lidar2body: the body turned, the lidar offset in the body so that it stands at `origin`
        Tb = yaw90(0.0, 0.0, 0.0)
        R = np.float64(Tb[:3, :3])
        Tl = EYE.copy()
        Tl[:3, 3] = R.T @ o
    p = R.T @ (e - o)
    assert (p.astype(np.float32) == p).all() and (o.astype(np.float32) == o).all()
    return Tb[None], Tl, [xyzi([p])]


# ---- 1. walks ----
WALKS = {
    "the diagonal (ties: x before y before z)": (1.0, (0.5, 0.5, 0.5), (2.5, 2.5, 2.5),
                                                 [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]),
    "towards negative x": (1.0, (0.5, 0.5, 0.5), (-1.5, 2.5, 0.5), [(0, 0, 0), (-1, 0, 0), (-1, 1, 0), (-2, 1, 0), (-2, 2, 0)]),
    "N = 0": (1.0, (0.5, 0.5, 0.5), (0.75, 0.25, 0.5), [(0, 0, 0)]),
    "N = 1": (1.0, (0.5, 0.5, 0.5), (1.25, 0.5, 0.5), [(0, 0, 0), (1, 0, 0)]),
}
WIDE = dict(min_range=0.125, max_range=80.0)


@pytest.mark.parametrize("pose", ["identity", "yawed and translated", "through T_lidar2body"])
@pytest.mark.parametrize("name", list(WALKS))
def test_a_known_walk_read_back_through_a_cube_of_map_voxels(handle, name, pose):
    voxel, o, e, listed = WALKS[name]
    shift = (3, -2, 1) if pose == "yawed and translated" else (0, 0, 0)  # (whole cells: the walk moves with the lidar)
    cells, cloud = cube(-3, 3, voxel, shift)
    T, Tl, scans = one_ray(pose, np.float64(o) + shift, np.float64(e) + shift)
    want = check(handle, cloud, scans, T, Tl, what=(name, pose), voxel=voxel, **WIDE)
    walk = np.asarray(listed) + shift
    assert (evalmap.carve_walk(np.float64(o) + shift, np.float64(e) + shift, voxel) == walk).all()
    assert (want[0] == votes_of(cells, walk, len(walk) - 1)).all(), (name, pose)
    assert want[4] == [dict(n_points=1, n_non_finite=0, n_out_of_range=0, n_rays=1, n_steps=len(walk) - 1, n_end_in_map=1, n_voxels_hit=1,
                            n_voxels_free=len(walk) - 1)]
    hit = (want[0][:, 0] == 1)
    assert hit.sum() == 1 and want[1][hit] == L_HIT and (want[1][want[0][:, 1] == 1] == L_MISS).all() and (want[1][want[0].sum(1) == 0] == 0).all()
    assert (want[2] == (want[0][:, 1] == 0)).all() and want[5]["n_removed"] == len(walk) - 1 == want[5]["n_voxels_touched"] - 1


def test_the_known_walk_at_a_fifth_of_a_metre(handle):
    cells = [(c, 0, 0) for c in range(-1, 6)]
    T = EYE[None].copy()
    T[0, :3, 3] = np.float32(0.1)
    want = check(handle, xyzi(centres(cells, 0.2)), [xyzi([(np.float32(0.6), 0, 0)])], T, what="0.1 -> 0.7", voxel=0.2, **WIDE)
    assert want[0].tolist() == [[0, 0], [0, 1], [0, 1], [0, 1], [1, 0], [0, 0], [0, 0]]  # it ends in cell 3


@pytest.mark.parametrize("sx,sy,sz", list(itertools.product((1, -1), repeat=3)))
def test_a_long_ray_across_the_origin_and_many_block_borders(handle, sx, sy, sz):
    """from one octant through the grid's origin into the opposite one, 79.7 m of the 80 at voxel = 0.2: negative cells, >> 2 and & 3 on both
    sides of zero.  The map: every second voxel of the walk (carve_walk, whose geometry tests/test_evalmap_carve.py checks by itself) and a
    neighbour of each that the ray does not enter."""
    s = np.float32([sx, sy, sz])
    o = (-s * np.float32([28.63, 18.67, 7.21])).astype(np.float32)
    p = (s * np.float32([64.43, 43.31, 18.13])).astype(np.float32)
    assert 79.5 < np.linalg.norm(p.astype(np.float64)) < 80.0
    walk = evalmap.carve_walk(o.astype(np.float64), p.astype(np.float64) + o.astype(np.float64), 0.2)
    on = walk[::2] if len(walk) % 2 else np.concatenate([walk[::2], walk[-1:]])
    walked = set(map(tuple, walk.tolist()))
    off = np.array([c for c in (on + [0, 0, 7]).tolist() if tuple(c) not in walked])
    cells = np.concatenate([on, off])
    T = EYE[None].copy()
    T[0, :3, 3] = o
    want = check(handle, xyzi(centres(cells, 0.2)), [xyzi([p])], T, what=("octant", sx, sy, sz), voxel=0.2, min_range=0.5, max_range=80.0)
    assert len(walk) > 600 and (walk.min(0) < -60).any() and (walk.max(0) > 60).any()
    assert (want[0] == votes_of(cells, walk, len(walk) - 1)).all()
    assert want[4][0]["n_steps"] == len(walk) - 1 and want[4][0]["n_voxels_free"] == len(on) - 1 and want[5]["n_voxels_touched"] == len(on)


@pytest.mark.parametrize("stop_short", [0, 1, 5, 6, 7])
def test_stop_short_around_the_number_of_steps(handle, stop_short):
    voxel, o, e, listed = WALKS["the diagonal (ties: x before y before z)"]  # N = 6
    cells, cloud = cube(-1, 3)
    T, Tl, scans = one_ray("identity", o, e)
    want = check(handle, cloud, scans, T, Tl, what=("stop_short", stop_short), voxel=voxel, stop_short=stop_short, **WIDE)
    n_free = max(0, 6 - stop_short)
    assert (want[0] == votes_of(cells, np.asarray(listed), n_free)).all()
    assert want[4][0]["n_steps"] == n_free == want[4][0]["n_voxels_free"] and want[4][0]["n_voxels_hit"] == 1


def test_the_lidars_own_voxel_in_the_map(handle):
    cloud = xyzi([(0.5, 0.5, 0.5)])
    T, Tl, leaves = one_ray("identity", (0.5, 0.5, 0.5), (4.5, 0.5, 0.5))
    _, _, stays = one_ray("identity", (0.5, 0.5, 0.5), (0.75, 0.75, 0.25))
    want = check(handle, cloud, leaves, T, Tl, what="a ray leaves it", voxel=1.0, **WIDE)
    assert want[0].tolist() == [[0, 1]] and want[4][0]["n_end_in_map"] == 0 and want[2].tolist() == [0]
    want = check(handle, cloud, stays, T, Tl, what="a ray ends in it", voxel=1.0, **WIDE)
    assert want[0].tolist() == [[1, 0]] and want[4][0]["n_end_in_map"] == 1 and want[4][0]["n_steps"] == 0 and want[2].tolist() == [1]


# ---- 2. the occupancy structure ----
def rays_to(origin, ends):
    """the pose of a lidar at `origin` (no rotation) and a scan with a return at every point of `ends`"""
    T = EYE.copy()
    T[:3, 3] = origin
    local = np.asarray(ends, np.float64) - np.float64(origin)
    assert (local.astype(np.float32) == local).all()
    return T[None], [xyzi(local)]


def test_a_full_block_and_the_rank_of_its_last_bit(handle):
    """a point in every voxel of the block of cells 4 .. 7 (voxel = 1), in a shuffled order; returns in the voxels whose bit index is odd:
    exactly those points are hit, bit 63 among them, so every voxel's rank below its bit is right"""
    r = np.arange(4, 8)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    cells = cells[np.random.default_rng(5).permutation(64)]
    bit = (cells[:, 0] & 3) | ((cells[:, 1] & 3) << 2) | ((cells[:, 2] & 3) << 4)
    T, scans = rays_to((5.5, 5.5, -3.5), centres(cells[bit % 2 == 1], 1.0))
    want = check(handle, xyzi(centres(cells, 1.0)), scans, T, what="one block", voxel=1.0, **WIDE)
    assert (want[5]["n_blocks"], want[5]["n_voxels"]) == (1, 64) and sorted(bit.tolist()) == list(range(64))
    assert (want[0][:, 0] == bit % 2).all() and (want[0][bit % 2 == 1, 1] == 0).all() and want[0][bit == 63].tolist() == [[1, 0]]
    assert want[4][0]["n_voxels_hit"] == 32 == want[4][0]["n_end_in_map"]


def test_the_eight_blocks_around_the_origin_corner(handle):
    cells = np.array(list(itertools.product((-1, 0), repeat=3)))
    T, Tl, scans = one_ray("identity", (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    want = check(handle, xyzi(centres(cells, 1.0)), scans, T, Tl, what="eight blocks", voxel=1.0, **WIDE)
    assert (want[5]["n_blocks"], want[5]["n_voxels"]) == (8, 8)
    assert (want[0] == votes_of(cells, [(-1, -1, -1), (0, -1, -1), (0, 0, -1), (0, 0, 0)], 3)).all()


def test_two_points_in_one_voxel_share_votes_and_fate(handle):
    cloud = xyzi([(2.25, 0.5, 0.5), (9.5, 0.5, 0.5), (2.75, 0.25, 0.75), (4.5, 0.5, 0.5)], [252, 40, 40, 40])
    T, Tl, scans = one_ray("identity", (0.5, 0.5, 0.5), (4.5, 0.5, 0.5))
    want = check(handle, cloud, scans, T, Tl, what="two in one", voxel=1.0, **WIDE)
    assert want[0].tolist() == [[0, 1], [0, 0], [0, 1], [1, 0]] and want[2].tolist() == [0, 1, 0, 1] and want[5]["n_voxels"] == 3
    assert (want[5]["n_removed"], want[5]["n_removed_dynamic"], want[5]["n_removed_static"]) == (2, 1, 1) and want[1][0] == want[1][2] == L_MISS


def test_a_lattice_of_eight_thousand_blocks_with_every_voxel_found(handle):
    """one map voxel in each of 20 x 20 x 20 blocks: 8000 entries in a table of 16384 slots, so slots collide and probing goes on past
    them.  A return in every one of them: every point is hit exactly once"""
    r = np.arange(20) * 4 - 36
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) + [1, 2, 3]
    T, scans = rays_to((0.5, 0.5, 0.5), centres(cells, 1.0))
    want = check(handle, xyzi(centres(cells, 1.0)), scans, T, what="lattice", voxel=1.0, **WIDE)
    assert (want[5]["n_blocks"], want[5]["n_voxels"], want[5]["n_voxels_touched"]) == (8000, 8000, 8000)
    assert (want[0] == [1, 0]).all() and want[4][0]["n_end_in_map"] == 8000 == want[4][0]["n_voxels_hit"] and want[4][0]["n_voxels_free"] == 0


def test_a_non_finite_map_point_lies_in_no_voxel(handle):
    cloud = xyzi([(2.5, 0.5, 0.5), (np.nan, 0.5, 0.5), (2.5, np.inf, 0.5), (2.5, 0.5, -np.inf)], 252)
    T, Tl, scans = one_ray("identity", (0.5, 0.5, 0.5), (4.5, 0.5, 0.5))
    lg = dict(LG, l_init=-0.5, l_min=-2.0, l_thr=-0.25)  # (even a start below the threshold removes only what lies in a voxel)
    want = check(handle, cloud, scans, T, Tl, what="non-finite map points", voxel=1.0, logodds=lg, **WIDE)
    assert want[0].tolist() == [[0, 1], [0, 0], [0, 0], [0, 0]] and want[2].tolist() == [0, 1, 1, 1] and (want[1][1:] == np.float32(-0.5)).all()
    assert (want[5]["n_map_non_finite"], want[5]["n_voxels"], want[5]["n_removed"]) == (3, 1, 1)
    assert want[3].view(np.uint32).tolist() == cloud[1:].view(np.uint32).tolist()  # kept as given, bit for bit


# ---- 3. precedence ----
def test_hits_come_before_misses_within_a_frame_and_not_across_frames(handle):
    cloud = xyzi([(3.5, 0.5, 0.5), (6.5, 0.5, 0.5)])
    T, Tl, near = one_ray("identity", (0.5, 0.5, 0.5), (3.5, 0.5, 0.5))
    _, _, far = one_ray("identity", (0.5, 0.5, 0.5), (6.5, 0.5, 0.5))
    both = [np.concatenate([near[0], far[0]])]
    want = check(handle, cloud, both, T, Tl, what="one frame", voxel=1.0, **WIDE)
    assert want[0].tolist() == [[1, 0], [1, 0]] and want[4][0]["n_voxels_hit"] == 2 and want[4][0]["n_voxels_free"] == 0
    assert_same(handle.carve([both[0][::-1].copy()], T, Tl, cloud, voxel=1.0, **WIDE), want, "the other order")
    want = check(handle, cloud, [near[0], far[0]], np.concatenate([T, T]), Tl, what="two frames", voxel=1.0, **WIDE)
    assert want[0].tolist() == [[1, 1], [1, 0]] and [r["n_voxels_free"] for r in want[4]] == [0, 1]
    assert want[1][0] == np.float32(L_HIT + L_MISS)


# ---- 4. the integration ----
BOX, WALL = xyzi([(4.0, 0, 0)]), xyzi([(9.0, 0, 0)])  # returns on one line from a lidar at (0.5, 0.5, 0.5)
LINE = xyzi([(4.5, 0.5, 0.5), (9.5, 0.5, 0.5)], [252, 40])  # the box voxel and the wall voxel
AT = EYE.copy()
AT[:3, 3] = 0.5


def line(g, seq, what, **kw):
    """the box voxel's (hits, misses, L, kept) after the frames of `seq`: True a return in the box, False one in the wall behind it,
    None a frame without points"""
    scans = [np.zeros((0, 4), np.float32) if s is None else BOX if s else WALL for s in seq]
    want = check(g, LINE, scans, np.stack([AT] * len(seq)), what=what, voxel=1.0, **dict(WIDE, **kw))
    return int(want[0][0, 0]), int(want[0][0, 1]), want[1][0], int(want[2][0])


def fold(seq):
    """the integration of the contract, by hand in float32"""
    l = np.float32(0)
    for s in seq:
        if s is not None:
            l = min(np.float32(l + L_HIT), L_MAX) if s else max(np.float32(l + L_MISS), L_MIN)
    return np.float32(l)


def test_a_box_return_then_wall_returns_behind_it(handle):
    """L = l_hit + k l_miss in float32, one addition per frame: 0.847 - 0.405 k first falls below 0 at k = 3"""
    k = next(k for k in range(1, 20) if evalmap.carve(LINE, [BOX] + [WALL] * k, np.stack([AT] * (k + 1)), voxel=1.0, **WIDE)[2][0] == 0)
    assert k == 3
    for n_miss, kept in ((k - 1, 1), (k, 0)):
        hits, misses, l, mask = line(handle, [True] + [False] * n_miss, ("box then wall", n_miss))
        assert (hits, misses, mask) == (1, n_miss, kept) and l == fold([True] + [False] * n_miss) and (l < 0) == (not kept)


def test_the_clamps_and_the_order_of_the_frames(handle):
    """20 hits saturate at l_max = 3.476, so 9 misses of 0.405 remove the voxel; unclamped it would take 42.  The misses first saturate at
    l_min, and the 20 hits after them end at l_max: kept."""
    unclamped = int(np.ceil(20 * float(L_HIT) / -float(L_MISS)))
    need = next(m for m in range(1, 60) if fold([True] * 20 + [False] * m) < 0)
    assert need == int(np.floor(float(L_MAX) / -float(L_MISS))) + 1 and need < unclamped // 4
    for m, kept in ((need - 1, 1), (need, 0)):
        hits, misses, l, mask = line(handle, [True] * 20 + [False] * m, ("clamped", m))
        assert (hits, misses, mask) == (20, m, kept) and l == fold([True] * 20 + [False] * m)
    hits, misses, l, mask = line(handle, [False] * need + [True] * 20, "reversed")
    assert (hits, misses, mask) == (20, need, 1) and l == L_MAX
    assert line(handle, [False] * 10, "the lower clamp")[2] == L_MIN


# ---- 5. batches ----
@pytest.mark.parametrize("n_frames", [1, 31, 32, 33, 64, 65])
def test_the_result_does_not_depend_on_where_a_batch_ends(handle, n_frames):
    seq = [None if f == 17 else (f * 7) % 5 < 2 for f in range(n_frames)]  # (frame 17: no points, in the middle of a batch)
    hits, misses, l, mask = line(handle, seq, ("frames", n_frames))
    assert (hits, misses) == (sum(s is True for s in seq), sum(s is False for s in seq)) and l == fold(seq) and mask == (0 if l < 0 else 1)
    # a threshold and clamps that make the order matter everywhere
    lg = dict(l_init=0.0, l_hit=0.75, l_miss=-0.5, l_min=-1.0, l_max=1.0, l_thr=0.25)
    line(handle, seq, ("frames, tight clamps", n_frames), logodds=lg)


# ---- 6. sizes ----
def blob(n, seed, span=6.0, labels=True):
    rng = np.random.default_rng(seed)
    return xyzi(rng.uniform(-span, span, (n, 3)) * [1, 1, 0.25], rng.integers(245, 265, n) if labels else 40.0)


def frames_of(sizes, seed):
    scans = [blob(n, seed + 17 * f, labels=False) for f, n in enumerate(sizes)]
    T = np.stack([EYE] * len(sizes)).copy()
    for f in range(len(sizes)):
        T[f, :3, 3] = [0.5 * f - 1.0, 0.25 * (f % 3), 0.125 * f]
    return scans, T


LOOSE = dict(voxel=0.5, min_range=1.0, max_range=8.0, stop_short=0)


@pytest.mark.parametrize("n_map", [0, 1, 63, 64, 65, 255, 256, 257])
def test_every_map_size_around_a_wavefront_and_a_workgroup(handle, n_map):
    scans, T = frames_of([0, 1, 63, 64, 65, 257], 3)
    want = check(handle, blob(n_map, n_map), scans, T, what=("n_map", n_map), **LOOSE)
    assert want[5]["n_points"] == n_map and [r["n_points"] for r in want[4]] == [0, 1, 63, 64, 65, 257] and want[5]["n_rays"] > 300
    if n_map >= 63:
        assert want[5]["n_voxels_free"] > 0 and want[5]["n_removed"] > 0 and 0 < want[5]["n_voxels"] <= n_map


def test_no_frames_and_empty_everything(handle):
    want = check(handle, blob(70, 1), [], np.zeros((0, 4, 4), np.float32), what="no frames", **LOOSE)
    assert want[4] == [] and want[5]["n_kept"] == 70 and want[5]["n_voxels_touched"] == 0 and (want[1] == 0).all()
    check(handle, blob(0, 1), [], np.zeros((0, 4, 4), np.float32), what="nothing", **LOOSE)
    # many tiny frames, empty ones among them: more than a batch in one workgroup of the walk
    scans, T = frames_of([3] * 70 + [0] * 5 + [1] * 60, 5)
    want = check(handle, blob(100, 2), scans, T, what="tiny frames", **LOOSE)
    assert sum(r["n_points"] for r in want[4]) == 270


# ---- 7. drops ----
def test_each_gate_is_counted_and_the_range_ends_are_inside(handle):
    lo, hi = 0.5, 80.0
    xs = [lo, step32(lo, False), step32(lo, True), hi, step32(hi, True), step32(hi, False)]  # on the x axis rho = |x| exactly
    scan = xyzi([(x, 0, 0) for x in xs] + [(np.nan, 1, 1), (1, -np.inf, 1), (1, 1, np.inf), (0, 0, 0), (3, 4, 0)])
    want = check(handle, xyzi([(79.9, 0.1, 0.1), (3.1, 4.1, 0.1)]), [scan], EYE[None], what="drops", voxel=0.2, min_range=lo, max_range=hi)
    r = want[4][0]
    assert (r["n_points"], r["n_non_finite"], r["n_out_of_range"], r["n_rays"]) == (11, 3, 3, 5) and r["n_end_in_map"] == 2
    # a matrix that stretches: the end is out of reach, the ray is dropped and nothing is walked
    T = EYE[None].copy()
    T[0, 0, 0] = 1.0e6
    want = check(handle, xyzi([(1.5, 0.5, 0.5)]), [xyzi([(3, 0, 0), (0, 3, 0)])], T, what="stretched", voxel=1.0, **WIDE)
    assert (want[4][0]["n_out_of_range"], want[4][0]["n_rays"]) == (1, 1)


# ---- 8. the interface ----
def raw_call(gpu_mod, g, cloud, scans, T, kw, outs, map_call=False, cap=None, lg=LG):
    """erasor_hip_carve_clouds / _map through ctypes with the buffers given (None: NULL); the return code"""
    L = gpu_mod.lib()
    cat = np.ascontiguousarray(np.concatenate(scans) if scans else np.zeros((0, 4), np.float32), np.float32)
    offs = np.zeros(len(scans) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in scans])
    prm = gpu_mod.Carve(kw["voxel"], kw["min_range"], kw["max_range"], *[lg[k] for k in evalmap.CARVE_LOGODDS_FIELDS], kw["stop_short"], 0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    Tb = np.ascontiguousarray(T, np.float32)
    votes, lo, mask, kept, rows, res = outs
    head = () if map_call else (p(cloud), C.c_size_t(len(cloud)), C.c_int(0))
    fn = L.erasor_hip_carve_map if map_call else L.erasor_hip_carve_clouds
    return fn(g._h, *head, p(cat), C.c_size_t(len(cat)), p(offs), C.c_size_t(len(scans)), C.c_int(0), None, p(Tb), C.byref(prm), p(votes), p(lo), p(mask),
              p(kept), C.c_size_t(len(cloud) if cap is None else cap), rows, None if res is None else C.byref(res))


def test_every_combination_of_outputs_and_the_words_behind_them(handle, gpu_mod):
    cloud = blob(257, 9)
    scans, T = frames_of([90, 0, 130], 21)
    want = evalmap.carve(cloud, scans, T, None, **LOOSE)
    n, nk, nf = len(cloud), want[5]["n_kept"], len(scans)
    assert 0 < nk < n and 0 < want[5]["n_removed_dynamic"] < want[5]["n_removed"]  # (the removed counts by label, both kinds)
    for use in itertools.product((False, True), repeat=6):
        votes, lo, mask = np.full(2 * n + 8, 0x7777, np.uint16), np.full(n + 8, 7.0, np.float32), np.full(n + 8, 0x77, np.uint8)
        kept = np.full(4 * n + 8, 7.0, np.float32)
        rows, res = (gpu_mod.CarveRow * (nf + 1))(), gpu_mod.CarveResult()
        rows[nf].n_points = res.n_points = 12345
        outs = [b if u else None for b, u in zip((votes, lo, mask, kept, rows, res), use)]
        assert raw_call(gpu_mod, handle, cloud, scans, T, LOOSE, outs) == 0, (use, gpu_mod.lib().erasor_hip_last_error(handle._h))
        for b, u, m, w, fill in ((votes, use[0], 2 * n, want[0], 0x7777), (lo, use[1], n, want[1], 7.0), (mask, use[2], n, want[2], 0x77),
                                 (kept, use[3], 4 * nk, want[3], 7.0)):
            assert (b[m:] == fill).all(), use  # the guard words
            assert b[:m].tobytes() == w.tobytes() if u else (b[:m] == fill).all(), use
        assert rows[nf].n_points == 12345
        assert [rows[f].as_dict() for f in range(nf)] == want[4] if use[4] else all(rows[f].n_points == 0 for f in range(nf))
        assert res.as_dict() == want[5] if use[5] else res.n_points == 12345
    # a kept cloud that does not fit: the result first, then the code
    res = gpu_mod.CarveResult()
    kept = np.full(4 * n, 7.0, np.float32)
    assert raw_call(gpu_mod, handle, cloud, scans, T, LOOSE, [None, None, None, kept, None, res], cap=nk - 1) == E_CAPACITY
    assert res.as_dict() == want[5] and (kept == 7.0).all()


def test_refusals_each_with_its_code_and_the_struct_layout(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    cloud = blob(100, 4)
    scans, T = frames_of([50, 60], 2)
    L = gpu_mod.lib()
    err = lambda: L.erasor_hip_last_error(g._h).decode()
    none = [None] * 6

    def refused(sentence, cloud=cloud, scans=scans, T=T, lg=LG, **kw):
        assert raw_call(gpu_mod, g, cloud, scans, T, dict(LOOSE, **kw), none, lg=lg) == E_INVALID, sentence
        assert err() == "erasor_hip_carve_clouds: " + sentence, err()

    for v in (0.0, -0.5, np.nan, np.inf):
        refused("voxel must be a finite number > 0", voxel=v)
    for lo, hi in ((5.0, 5.0), (6.0, 5.0), (-1.0, 5.0), (np.nan, 5.0), (1.0, np.inf)):
        refused("0 <= min_range < max_range, both finite", min_range=lo, max_range=hi)
    refused("max_range / voxel must not exceed 4096", voxel=0.01, max_range=80.0)
    refused("max_range / voxel must not exceed 4096", voxel=1.0, max_range=float(np.nextafter(4096.0, 5000.0)))
    for bad in (dict(l_hit=-0.125), dict(l_miss=0.125), dict(l_init=4.0), dict(l_init=-3.0), dict(l_thr=np.nan), dict(l_min=-np.inf), dict(l_max=np.inf)):
        refused("the log-odds must be finite, l_hit >= 0, l_miss <= 0 and l_min <= l_init <= l_max", lg=dict(LG, **bad))
    refused("stop_short must be within 0 .. 64", stop_short=65)
    many = [np.zeros((0, 4), np.float32)] * 65536
    refused("more than 65535 frames", scans=many, T=np.stack([EYE] * 65536))
    bad = T.copy()
    bad[1, 0, 3] = np.inf
    refused("non-finite entry in T_body2origin", T=bad)
    far = T.copy()
    far[1, 2, 3] = -0.5 * 2.0 ** 28
    refused("the origin of frame 1 lies in a cell whose coordinate reaches 2^28", T=far)
    far[1, 2, 3] = np.nextafter(np.float32(0.5 * 2.0 ** 28), np.float32(0))  # one step inside: fine
    assert raw_call(gpu_mod, g, cloud, scans, far, LOOSE, none) == 0
    c = cloud.copy()
    c[7, 1] = 0.5 * 2.0 ** 28
    c[9, 0] = -0.5 * 2.0 ** 28 - 64
    refused("2 map point(s) lie in a cell whose coordinate reaches 2^28", cloud=c)
    with pytest.raises(ValueError):
        evalmap.carve(c, scans, T, None, **LOOSE)
    c[9, 0] = 1.0
    c[7, 1] = np.nextafter(np.float32(0.5 * 2.0 ** 28), np.float32(0))
    check(g, c, scans, T, what="a map point one step inside the cell range", **LOOSE)
    bad_l = EYE.copy()
    bad_l[2, 3] = np.nan
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.carve(scans, T, bad_l, cloud, **LOOSE)
    assert e.value.rc == E_INVALID and err() == "erasor_hip_carve_clouds: non-finite entry in T_lidar2body"
    # offsets that are not monotone, params NULL
    cat, offs = np.concatenate(scans), np.uint64([0, 70, 50])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    prm = gpu_mod.Carve(0.5, 1.0, 8.0, *[LG[k] for k in evalmap.CARVE_LOGODDS_FIELDS], 0, 0)
    args = lambda o, q: (g._h, p(cloud), C.c_size_t(100), C.c_int(0), p(cat), C.c_size_t(110), p(o), C.c_size_t(2), C.c_int(0), None, p(T), q, None, None, None,
                         None, C.c_size_t(0), None, None)
    assert L.erasor_hip_carve_clouds(*args(offs, C.byref(prm))) == E_INVALID and err() == "erasor_hip_carve_clouds: offsets decrease"
    assert L.erasor_hip_carve_clouds(*args(np.uint64([0, 50, 110]), None)) == E_INVALID and err() == "erasor_hip_carve_clouds: params is NULL"
    big = C.c_size_t((1 << 30) + 1)
    assert L.erasor_hip_carve_clouds(g._h, p(cloud), big, C.c_int(0), p(cat), C.c_size_t(110), p(np.uint64([0, 50, 110])), C.c_size_t(2), C.c_int(0), None,
                                     p(T), C.byref(prm), None, None, None, None, C.c_size_t(0), None, None) == E_INVALID
    assert err() == "erasor_hip_carve_clouds: NULL map or more than 2^30 map points"
    # the handle's map: none yet -- the error visibility_map gives
    grid = gpu_mod.visibility_grid(16, 2, -10.0, 10.0)
    with pytest.raises(gpu_mod.ErasorError) as e:
        g.visibility(scans, T, None, None, grid)
    assert e.value.rc == E_STATE
    sentence = err().split(": ", 1)[1]
    assert raw_call(gpu_mod, g, cloud, scans, T, LOOSE, none, map_call=True) == E_STATE and err() == "erasor_hip_carve_map: " + sentence
    for kw in (dict(voxel=0.0), dict(stop_short=65), dict(min_range=9.0, max_range=2.0), dict(logodds=dict(LG, l_miss=1.0))):
        with pytest.raises(ValueError):
            evalmap.carve(cloud, scans, T, None, **dict(LOOSE, **kw))
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.carve(scans, T, None, cloud, **dict(LOOSE, **kw))
        assert e.value.rc == E_INVALID
    check(g, cloud, scans, T, what="after the refusals", **LOOSE)  # the handle is fine
    # the header's layout
    fields = ("voxel", "min_range", "max_range", "l_init", "l_hit", "l_miss", "l_min", "l_max", "l_thr", "stop_short", "reserved")
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu", sizeof(erasor_carve), '
            'sizeof(erasor_carve_row), sizeof(erasor_carve_result));' +
            "".join('printf(" %%zu", offsetof(erasor_carve, %s));' % f for f in fields) +
            'printf(" %zu %zu\\n", offsetof(erasor_carve_row, n_voxels_free), offsetof(erasor_carve_result, n_voxels_free));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    V, R, S = gpu_mod.Carve, gpu_mod.CarveRow, gpu_mod.CarveResult
    mirror = [C.sizeof(V), C.sizeof(R), C.sizeof(S)] + [getattr(V, f).offset for f in fields] + [R.n_voxels_free.offset, S.n_voxels_free.offset]
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == mirror
    assert mirror[:3] == [56, 64, 136] and mirror[-2:] == [56, 128]
    assert tuple(k for k, _ in R._fields_) == evalmap.CARVE_ROW_FIELDS and tuple(k for k, _ in S._fields_) == evalmap.CARVE_RESULT_FIELDS


def test_the_map_call_a_step_and_the_map_call_again(gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, plain = (gpu_mod.Erasor(scenarios.to_product_params(sc["params"])) for _ in range(2))
    for e in (g, plain):
        e.set_map(sc["map"])
        for f in range(n - 1):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    scans, T = sc["scans"][:3], np.stack(sc["T_b2o"][:3])
    kw = dict(voxel=0.4, min_range=1.0, max_range=60.0, stop_short=1)
    for f in (n - 1, n):
        m = np.ascontiguousarray(g.get_map(), np.float32)
        want = evalmap.carve(m, scans, T, sc["T_l2b"], **kw)
        assert_same(g.carve(scans, T, sc["T_l2b"], None, **kw), want, ("the handle's map before step", f))
        assert_same(g.carve(scans, T, sc["T_l2b"], m, **kw), want, ("the same map given", f))
        assert g.get_map().tobytes() == m.tobytes()  # the map itself stays as it is
        # the step after the call is the uninterrupted run's
        a = g.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        b = plain.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        assert a.as_dict() == b.as_dict() and g.get_map().tobytes() == plain.get_map().tobytes()


# ---- 9. the synthetic world ----
def test_the_synthetic_world(handle, gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    m = np.ascontiguousarray(sc["map"], np.float32)
    cloud = np.ascontiguousarray(m[:: max(1, len(m) // 6000)])
    assert len(cloud) > 1000
    scans, T = sc["scans"][:4], np.stack(sc["T_b2o"][:4])
    kw = dict(voxel=0.4, min_range=1.0, max_range=60.0, stop_short=1)
    want = check(handle, cloud, scans, T, sc["T_l2b"], what="world", **kw)
    res = want[5]
    assert res["n_removed_dynamic"] > 0 and res["n_voxels_free"] > 0 and res["n_voxels_hit"] > 0 and res["n_end_in_map"] > 0
    assert res["n_rays"] > 1000 and res["n_steps"] > 10 * res["n_rays"] and 0 < res["n_blocks"] <= res["n_voxels"] <= len(cloud)
    # the same from device buffers
    p = handle.device_array(cloud)
    cat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32).reshape(-1, 4) for s in scans]))
    q = handle.device_array(cat)
    try:
        offs = np.cumsum([0] + [len(s) for s in scans])
        assert_same(handle.carve((q, offs), T, sc["T_l2b"], (p, len(cloud)), **kw), want, "device buffers")
    finally:
        handle.device_free(p)
        handle.device_free(q)
