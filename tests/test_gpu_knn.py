"""k nearest neighbours, radius counts and the density filters on the device (erasor_hip_knn_* / _radius_count_* / _density_filter_*,
kernels in knn.hip.h) against their host restatement evalmap.knn / radius_count / density_filter (and the all-pairs knn_brute /
radius_count_brute): byte for byte in neighbour lists, distances, scores, counts, mask, kept cloud and result.  Ties at the k-th place,
one float32 step at the k-th place, at the radius and at the threshold, pairs a radius apart at every cell border, duplicates, short
clouds, every size around the leaf, wavefront, workgroup and tree padding, k = 1 and the radius count on one padded tree, degenerate boxes, the prefix property, the sequential mean,
every score with every rule, the buffers, the errors and the struct layout, the synthetic world, a 200 000-point cloud, the handle's
map and a step after it.  tests/test_knn_on_cpu.py re-runs this file against the CPU stand-in."""
import ctypes as C
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
NONE = evalmap.KNN_NONE
CELL_MARGIN = 1.0009765625  # cluster.hip.h: CL_CELL_MARGIN
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4


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


def steps(v, k):
    """the float32 values k steps above (below: k < 0) each of v"""
    v = np.asarray(v, np.float32).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def same_numbers(a, b):
    """two dicts of ints and floats with the same keys and values, NaN equal to NaN"""
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or
                                        (type(a[k]) is type(b[k]) and a[k] == b[k]) for k in a)


def assert_same_knn(got, want, what):
    assert got.keys() == want.keys(), what
    for key in ("n_points", "n_short", "k"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in ("kth_stats", "mean_stats"):
        assert same_numbers(got[key], want[key]), (what, key, got[key], want[key])
    for key, dt in (("kth", np.float64), ("mean", np.float64), ("nbr_idx", np.uint32), ("nbr_dist", np.float64)):
        if key in want:
            assert got[key].dtype == dt and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
            if got[key].tobytes() != want[key].tobytes():
                bits = np.uint64 if dt == np.float64 else np.uint32
                bad = np.flatnonzero((got[key].view(bits) != want[key].view(bits)).reshape(len(got[key]), -1).any(1))
                assert False, (what, key, bad[:5], got[key][bad[:2]], want[key][bad[:2]])


def check_knn(g, cloud, k, ref=evalmap.knn, what=""):
    """the device against the host restatement; what the host restatement returned"""
    want = ref(cloud, k, True)
    assert_same_knn(g.knn(cloud, k, True), want, (what, k))
    return want


def check_count(g, cloud, r, ref=evalmap.radius_count, what=""):
    want = ref(cloud, r)
    cnt, st = g.radius_count(cloud, r)
    assert cnt.dtype == np.uint32 and cnt.shape == want[0].shape and cnt.tobytes() == want[0].tobytes(), (what, r, np.flatnonzero(cnt != want[0])[:5])
    assert same_numbers(st, want[1]), (what, r, st, want[1])
    return want


def assert_same_filter(got, want, what):
    assert same_numbers(got[2], want[2]), (what, got[2], want[2])
    assert got[0].dtype == np.uint8 and got[0].shape == want[0].shape and got[0].tobytes() == want[0].tobytes(), (what, "mask")
    if want[1] is None:
        assert got[1] is None, what
    else:
        assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes(), (what, "kept cloud", got[1].shape, want[1].shape)


def check_filter(g, cloud, what="", **kw):
    want = evalmap.density_filter(cloud, **kw)
    assert_same_filter(g.density_filter(cloud, **kw), want, (what, kw))
    return want


def filler(n, seed, lo=60.0, hi=100.0):
    """n points far from the origin, on every side of it"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))


# ---- 1. ties at the k-th place ----
AXES = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_six_neighbours_at_one_distance_the_lowest_indices_win(handle, k):
    """the six points at +-1 on the axes around a query at the origin lie in different octants of the tree (far filler points on every
    side spread them over its leaves); they are all at d2 == 1, so the k lowest indices among them are the answer, wherever they sit
    in the cloud.  A prune on lb >= the list's last d2 drops some of them."""
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        n = 400
        xyz = filler(n, seed).astype(np.float32)
        at = rng.permutation(n)[:7]
        xyz[at[0]] = 0.0
        xyz[at[1:]] = AXES[rng.permutation(6)]
        cloud = xyzi(xyz)
        want = check_knn(handle, cloud, k, ref=evalmap.knn_brute, what=("ties", seed))
        assert want["nbr_idx"][at[0]].tolist() == sorted(at[1:].tolist())[:k] and (want["nbr_dist"][at[0]] == 1.0).all()
        assert_same_knn(evalmap.knn(cloud, k, True), want, ("ties, the tree version", seed, k))


# ---- 2. one float32 step ----
@pytest.mark.parametrize("k", [1, 5, 8, 9, 32])
def test_one_float32_step_between_the_kth_and_the_next_neighbour(handle, k):
    """k - 1 near points, then two points whose x differs by one float32 step, in either index order and on each axis: the nearer one is
    the k-th neighbour"""
    rng = np.random.default_rng(k)
    for base in (0.0, 700.0):
        for axis in range(3):
            for swap in (False, True):
                near = rng.uniform(-0.2, 0.2, (k - 1, 3))
                a, b = np.zeros(3, np.float32), np.zeros(3, np.float32)
                a[axis] = 0.75
                b[axis] = steps(np.float32(0.75 + base), 1) - np.float32(base)
                pair = [b, a] if swap else [a, b]
                xyz = np.concatenate([[np.zeros(3)], near, pair, filler(200, 7, 20, 40)]) + base
                xyz = xyz.astype(np.float32)
                want = check_knn(handle, xyzi(xyz), k, ref=evalmap.knn_brute, what=("step", base, axis, swap))
                d = want["nbr_dist"][0]
                assert d[k - 1] > (d[k - 2] if k > 1 else 0.0)
                w1 = evalmap.knn_brute(xyzi(xyz), min(k + 1, 32), True)
                if k < 32:
                    assert w1["nbr_dist"][0][k] > d[k - 1] and {int(w1["nbr_idx"][0][k - 1]), int(w1["nbr_idx"][0][k])} == {k, k + 1}


@pytest.mark.parametrize("r", [0.2, 0.5, 1.0, 0.3])
def test_pairs_one_float32_step_either_side_of_the_radius(handle, r):
    """pairs whose distance is r to within a few float32 steps along each axis, at the origin and far out, 16 m beside one another:
    counts of 1 inside, 0 outside, and one edge between them"""
    K = np.arange(-3, 4)
    for base in (0.0, -r / 2, 1e3, -1e5):
        for axis in range(3):
            pts = []
            for m, s in enumerate(K):
                lo = np.full(3, base, np.float32)
                lo[(axis + 1) % 3] += np.float32(16.0 * m)
                hi = lo.copy()
                hi[axis] = steps(np.float32(lo[axis] + np.float32(r)), int(s))
                pts += [lo, hi]
            cnt = check_count(handle, xyzi(pts), r, ref=evalmap.radius_count_brute, what=("edge", base, axis))[0]
            assert (cnt[0::2] == cnt[1::2]).all() and cnt[0] == 1 and cnt[-1] == 0 and (np.diff(cnt[0::2].astype(int)) <= 0).all(), cnt
            if r in (0.5, 1.0):
                assert cnt[6] == 1 and cnt[8] == 0  # d == r exactly counts, one step outside does not


@pytest.mark.parametrize("r", [0.5, 0.3])
def test_pairs_a_radius_apart_at_every_cell_border(handle, r):
    """pairs the predicate counts, as far apart as it allows along one axis, the lower point a few float32 steps around k * r and around
    k * (the cell edge in use), k from -2^20 to 2^20: a 27-cell search must meet every pair, and meet it once"""
    ks = np.unique(np.concatenate([np.array([s * (2 ** e + j) for s in (-1, 1) for e in range(0, 21) for j in (-1, 0, 1)]), np.arange(-40, 41),
                                   np.linspace(-2 ** 20, 2 ** 20, 97).astype(np.int64)])).astype(np.float64)
    ks = ks[np.abs(ks) <= 2 ** 20]
    for edge in (r, r * CELL_MARGIN):
        for axis in range(3):
            lo = np.concatenate([steps((ks * edge).astype(np.float32), s) for s in range(-2, 3)])
            hi = (lo.astype(np.float64) + r).astype(np.float32)
            z = lo * 0
            for _ in range(3):  # the largest float32 the predicate still counts from lo
                far = ~evalmap.cluster_adjacent(np.stack([lo, z, z], 1), np.stack([hi, z, z], 1), r)
                hi = np.where(far, np.nextafter(hi, np.float32(-np.inf)), hi)
            nxt = np.nextafter(hi, np.float32(np.inf))
            hi = np.where(evalmap.cluster_adjacent(np.stack([lo, z, z], 1), np.stack([nxt, z, z], 1), r), nxt, hi)
            ok = evalmap.cluster_adjacent(np.stack([lo, z, z], 1), np.stack([hi, z, z], 1), r) & (hi > lo)
            lo, hi = lo[ok], hi[ok]
            n = len(lo)
            assert n > 900
            xyz = np.zeros((2 * n, 3), np.float32)
            xyz[0::2, axis], xyz[1::2, axis] = lo, hi
            xyz[0::2, (axis + 1) % 3] = xyz[1::2, (axis + 1) % 3] = 4.0 * np.arange(n)  # (pairs 4 m apart: r <= 1)
            cnt, st = handle.radius_count(xyzi(xyz), r)
            assert (cnt == 1).all(), (r, edge, axis, np.flatnonzero(cnt != 1)[:5])
            assert st == {"n_scored": 2 * n, "min": 1.0, "median": 1.0, "p90": 1.0, "p99": 1.0, "max": 1.0}


def test_an_absolute_threshold_at_a_points_score_and_just_below_it(handle):
    rng = np.random.default_rng(3)
    cloud = xyzi(rng.uniform(-3, 3, (500, 3)), rng.integers(245, 265, 500))
    for score in ("kth", "mean"):
        s = evalmap.knn(cloud, 6)[score]
        for i in (0, 17, int(np.argmin(s)), int(np.argmax(s))):
            at = check_filter(handle, cloud, ("at", score, i), score=score, k=6, rule="abs", thr=float(s[i]))
            below = check_filter(handle, cloud, ("below", score, i), score=score, k=6, rule="abs", thr=float(np.nextafter(s[i], -np.inf)))
            assert at[0][i] == 1 and below[0][i] == 0 and at[2]["n_kept"] == below[2]["n_kept"] + int((s == s[i]).sum())


# ---- 3. duplicates ----
@pytest.mark.parametrize("k", [1, 8, 32])
def test_identical_points_are_neighbours_at_distance_zero(handle, k):
    for m in (2, k, k + 1, k + 2, 200):
        xyz = np.concatenate([filler(150, m, 5, 9), np.tile([[1.5, -2.25, 0.125]], (m, 1))])
        perm = np.random.default_rng(m).permutation(len(xyz))
        cloud = xyzi(xyz[perm])
        want = check_knn(handle, cloud, k, ref=evalmap.knn_brute, what=("duplicates", m))
        dup = np.flatnonzero(perm >= 150)
        for i in dup[:3].tolist() + dup[-3:].tolist():
            others = [j for j in dup.tolist() if j != i][:k]
            assert want["nbr_idx"][i][:len(others)].tolist() == others and (want["nbr_dist"][i][:len(others)] == 0).all()
        assert_same_knn(evalmap.knn(cloud, k, True), want, ("duplicates, the tree version", m, k))


def test_a_ball_of_4096_identical_points(handle):
    """every query visits all 4096 (the strict prune visits every tie): the tie hazard, bounded"""
    n = 1024 if ON_CPU else 4096
    cloud = xyzi(np.tile([[3.0, 3.0, 3.0]], (n, 1)), 252)
    got = handle.knn(cloud, 32, True)
    want_idx = np.array([[j for j in range(33) if j != i][:32] for i in range(n)], np.uint32)
    assert got["nbr_idx"].tobytes() == want_idx.tobytes() and not got["nbr_dist"].any() and not got["kth"].any() and not got["mean"].any()
    assert got["n_short"] == 0 and got["kth_stats"] == {"n_scored": n, "min": 0.0, "median": 0.0, "p90": 0.0, "p99": 0.0, "max": 0.0}
    res = handle.density_filter(cloud, "mean", k=32, rule="mad", mul=0.0, keep=False)[2]
    assert res["n_kept"] == n and res["m"] == 0.0 and res["mad"] == 0.0 and res["thr"] == 0.0  # mad == 0: everything at m is kept


# ---- 4. short clouds ----
@pytest.mark.parametrize("k", [1, 8, 32])
def test_clouds_with_fewer_than_k_other_points(handle, k):
    rng = np.random.default_rng(k)
    for n in (1, 2, k, k + 1):
        cloud = xyzi(rng.uniform(-1, 1, (n, 3)), 253)
        want = check_knn(handle, cloud, k, ref=evalmap.knn_brute, what=("short", n))
        short = n - 1 < k
        assert want["n_short"] == (n if short else 0) and np.isinf(want["kth"]).all() == short
        if short:
            assert (want["nbr_idx"][:, n - 1:] == NONE).all() and np.isinf(want["nbr_dist"][:, n - 1:]).all() and np.isinf(want["mean"]).all()
            assert (want["nbr_idx"][:, :n - 1] != NONE).all() and want["kth_stats"]["n_scored"] == 0 and math.isnan(want["kth_stats"]["median"])
        for score in ("kth", "mean"):
            w = check_filter(handle, cloud, ("short", n), score=score, k=k, rule="mad", mul=1.0)
            assert (w[2]["n_kept"] == 0 and math.isnan(w[2]["thr"]) and w[2]["n_removed_dynamic"] == n) if short else w[2]["n_kept"] >= (n + 1) // 2
            check_filter(handle, cloud, ("short, abs", n), score=score, k=k, rule="abs", thr=10.0)


# ---- 5. sizes ----
SIZES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049]


def blob(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-4, 4, (n, 3))
    xyz[::9] = np.round(xyz[::9])  # lattice points among them: ties and duplicates
    return xyzi(xyz, rng.integers(240, 270, n))


@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_leaf_the_wavefront_the_workgroup_and_the_tree_padding(handle, n, k):
    cloud = blob(n, 1000 + n)
    check_knn(handle, cloud, k, what=("size", n))
    if k == 8:
        check_count(handle, cloud, 0.9, what=("size", n))


@pytest.mark.parametrize("k", [2, 7, 9, 16, 17, 31])
def test_every_list_class_at_257_points(handle, k):
    check_knn(handle, blob(257, k), k, ref=evalmap.knn_brute, what="k classes")


def test_the_nearest_other_point_and_the_radius_count_agree_on_a_padded_tree(handle):
    """1025 points: 33 leaves under a tree padded to 64, so whole subtrees are empty boxes.  Among them 40 identical points (every one of
    them ties with 39 others at distance 0) and, far outside, three points 0.5 apart on a line (the middle one ties between its two
    neighbours).  knn(k = 1) is the float64 nearest OTHER point as the all-pairs restatement gives it, and radius_count(0.5) > 0 holds
    exactly where that distance is <= 0.5 -- a distance the tail hits with equality."""
    rng = np.random.default_rng(1025)
    xyz = rng.uniform(-4, 4, (1025, 3)).astype(np.float32)
    at = rng.permutation(1025)
    dup, tail = at[:40], at[40:43]
    xyz[dup] = [1.5, -2.25, 0.125]
    xyz[tail] = [[20.0, 20.0, 20.0], [20.5, 20.0, 20.0], [21.0, 20.0, 20.0]]
    cloud, r = xyzi(xyz), 0.5
    want = evalmap.knn_brute(cloud, 1, True)
    d, j = want["nbr_dist"][:, 0], want["nbr_idx"][:, 0]
    near = d <= r
    # the case itself, on the host alone: r is hit with equality, both sides of it occur, and the count's predicate (d2 <= r * r) says the same
    assert (d[tail] == r).all() and j[tail[1]] == min(tail[0], tail[2]) and (d[dup] == 0).all() and 43 < near.sum() < 1025 - 43
    assert all(j[i] == min(k for k in dup if k != i) for i in dup)
    assert ((evalmap.radius_count_brute(cloud, r)[0] > 0) == near).all()
    got = handle.knn(cloud, 1, True)
    assert got["nbr_idx"][:, 0].tobytes() == j.tobytes(), np.flatnonzero(got["nbr_idx"][:, 0] != j)[:5]
    assert got["nbr_dist"][:, 0].tobytes() == d.tobytes(), np.flatnonzero(got["nbr_dist"][:, 0] != d)[:5]
    cnt = handle.radius_count(cloud, r)[0]
    assert ((cnt > 0) == near).all(), np.flatnonzero((cnt > 0) != near)[:5]


# ---- 6. degenerate boxes ----
@pytest.mark.parametrize("shape", ["line", "plane", "point"])
def test_points_on_a_line_in_a_plane_and_at_one_place_with_an_outlier(handle, shape):
    rng = np.random.default_rng(5)
    xyz = np.zeros((300, 3))
    if shape == "line":
        xyz[:, 1] = rng.uniform(-5, 5, 300)
    elif shape == "plane":
        xyz[:, [0, 2]] = rng.uniform(-5, 5, (300, 2))
    else:
        xyz[:] = [2.0, -1.0, 0.5]
    xyz[137] = [1e6, -1e6, 1e6]
    cloud = xyzi(xyz)
    for k in (1, 8, 32):
        want = check_knn(handle, cloud, k, ref=evalmap.knn_brute, what=shape)
        assert want["kth"][137] > 1e6 and want["kth_stats"]["max"] == want["kth"][137]
    cnt = check_count(handle, cloud, 0.5, ref=evalmap.radius_count_brute, what=shape)[0]
    assert cnt[137] == 0
    w = check_filter(handle, cloud, shape, score="mean", k=8, rule="mad", mul=3.0)
    assert w[0][137] == 0


# ---- 7. the prefix property, determinism, the mean ----
def test_the_first_eight_of_thirty_two_are_the_eight_and_two_runs_agree(handle):
    cloud = blob(3000, 77)
    a, b, c = handle.knn(cloud, 32, True), handle.knn(cloud, 8, True), handle.knn(cloud, 32, True)
    assert a["nbr_idx"][:, :8].tobytes() == b["nbr_idx"].tobytes() and a["nbr_dist"][:, :8].tobytes() == b["nbr_dist"].tobytes()
    assert b["kth"].tobytes() == a["nbr_dist"][:, 7].tobytes()
    assert_same_knn(c, a, "a second run")
    # without the lists: the same scores
    d = handle.knn(cloud, 32)
    assert "nbr_idx" not in d and d["kth"].tobytes() == a["kth"].tobytes() and d["mean"].tobytes() == a["mean"].tobytes()


def test_the_mean_is_summed_in_list_order(handle):
    """eight neighbours on the x axis from 2e-7 m to 998 m (float32 values; their float64 sum needs more than 53 bits): summing from the
    far end, or pairwise, rounds differently from the list order"""
    d = np.float32([2.0723335580896673e-07, 2.627641890740051e-07, 4.2249038756381196e-07, 0.5983953475952148, 0.6327766180038452,
                    1.5256928205490112, 948.5191040039062, 998.07373046875])
    xyz = np.zeros((9, 3), np.float32)
    xyz[1:, 0] = d
    cloud = xyzi(np.concatenate([xyz, filler(100, 9, 5e4, 6e4)]).astype(np.float32))
    want = check_knn(handle, cloud, 8, ref=evalmap.knn_brute, what="mean")
    dd = want["nbr_dist"][0]
    seq = np.float64(0.0)
    for v in dd:
        seq = seq + v
    assert want["mean"][0] == seq / 8.0
    back = np.float64(0.0)
    for v in dd[::-1]:
        back = back + v
    pair = ((dd[0] + dd[1]) + (dd[2] + dd[3])) + ((dd[4] + dd[5]) + (dd[6] + dd[7]))
    assert back != seq and pair != seq  # (the case tells the orders apart)


# ---- 8. the filter ----
def filter_cloud():
    rng = np.random.default_rng(21)
    xyz = np.concatenate([rng.uniform(-3, 3, (1500, 3)) * [1, 1, 0.05], rng.uniform(-8, 8, (60, 3))])
    w = rng.integers(245, 265, len(xyz)).astype(np.float32)
    w[::50] = np.nan
    w[7], w[8], w[9] = -1.0, 4294967296.0, np.float32(252 + (3 << 16))
    c = xyzi(xyz, w)
    c[3::40, 0] = -0.0  # signed zeros, copied as bits
    return c


@pytest.mark.parametrize("score,rule", [("kth", "abs"), ("kth", "mad"), ("mean", "abs"), ("mean", "mad"), ("count", "abs"), ("count", "mad")])
def test_every_score_with_every_rule(handle, score, rule):
    cloud = filter_cloud()
    for k, thr, mul, radius, mn in ((8, 0.35, 2.0, 0.4, 3), (1, 0.1, 0.0, 0.2, 1), (32, 0.9, 5.0, 1.0, 40)):
        w = check_filter(handle, cloud, "filter", score=score, k=k, radius=radius, rule=rule, thr=thr, mul=mul, min_neighbors=mn)
        r = w[2]
        assert 0 < r["n_kept"] < len(cloud) and r["n_removed_dynamic"] + r["n_removed_static"] == r["n_removed"] and r["n_removed_dynamic"] > 0
        assert np.signbit(w[1][:, 0]).any() and np.isnan(w[1][:, 3]).any()
        # counts only
        got = handle.density_filter(cloud, score=score, k=k, radius=radius, rule=rule, thr=thr, mul=mul, min_neighbors=mn, keep=False)
        assert got[1] is None and same_numbers(got[2], r) and got[0].tobytes() == w[0].tobytes()
    # min_neighbors 0 keeps everything, a huge one nothing
    if score == "count":
        assert check_filter(handle, cloud, score="count", radius=0.4, min_neighbors=0)[2]["n_kept"] == len(cloud)
        assert check_filter(handle, cloud, score="count", radius=0.4, min_neighbors=2 ** 31)[2]["n_kept"] == 0


def raw_filter(gpu_mod, g, cloud, f, mask, kept, cap, res, n=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return gpu_mod.lib().erasor_hip_density_filter_clouds(g._h, p(cloud), C.c_size_t(len(cloud) if n is None else n), C.c_int(0),
                                                          None if f is None else C.byref(f), p(mask), p(kept), C.c_size_t(cap),
                                                          None if res is None else C.byref(res))


def test_a_kept_buffer_one_row_too_small(handle, gpu_mod):
    cloud = filter_cloud()
    want = evalmap.density_filter(cloud, "mean", k=8, rule="mad", mul=2.0)
    nk = want[2]["n_kept"]
    f = gpu_mod.DensityFilter(1, 1, 8, 0, 0.0, 0.0, 2.0)
    res = gpu_mod.DensityResult()
    mask = np.zeros(len(cloud), np.uint8)
    kept = np.full((nk, 4), 7.0, np.float32)
    assert raw_filter(gpu_mod, handle, cloud, f, mask, kept, nk - 1, res) == E_CAPACITY
    assert same_numbers(res.as_dict(), want[2]) and mask.tobytes() == want[0].tobytes() and (kept == 7.0).all()
    assert raw_filter(gpu_mod, handle, cloud, f, None, kept, nk, res) == 0 and kept.tobytes() == want[1].tobytes()
    assert raw_filter(gpu_mod, handle, cloud, f, None, None, 0, res) == 0 and same_numbers(res.as_dict(), want[2])


# ---- 9. errors and struct layout ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    cloud = blob(300, 4)

    def refused(rc, fn, *a, **kw):
        with pytest.raises(gpu_mod.ErasorError) as e:
            fn(*a, **kw)
        assert e.value.rc == rc, str(e.value)
        return str(e.value)

    for k in (0, 33, -1, 1000):
        assert refused(E_INVALID, g.knn, cloud, k).endswith("erasor_hip_knn_clouds: k must be within 1 .. 32")
        assert refused(E_INVALID, g.density_filter, cloud, "kth", k=k).endswith("erasor_hip_density_filter_clouds: k must be within 1 .. 32")
    for r in (0.0, -0.5, float("nan"), float("inf")):
        assert refused(E_INVALID, g.radius_count, cloud, r).endswith("erasor_hip_radius_count_clouds: radius must be a finite number > 0")
        assert refused(E_INVALID, g.density_filter, cloud, "count", radius=r).endswith("radius must be a finite number > 0")
    for v in (-0.5, float("nan"), float("inf")):
        assert refused(E_INVALID, g.density_filter, cloud, "kth", k=4, rule="abs", thr=v).endswith("thr must be a finite number >= 0")
        assert refused(E_INVALID, g.density_filter, cloud, "mean", k=4, rule="mad", mul=v).endswith("mul must be a finite number >= 0")
    assert refused(E_INVALID, g.density_filter, cloud, "sigma").endswith("unknown score (ERASOR_DENSITY_KTH, _MEAN or _COUNT)")
    assert refused(E_INVALID, g.density_filter, cloud, 3).endswith("unknown score (ERASOR_DENSITY_KTH, _MEAN or _COUNT)")
    assert refused(E_INVALID, g.density_filter, cloud, "mean", rule="sigma").endswith("unknown rule (ERASOR_DENSITY_ABS or _MAD)")
    assert refused(E_INVALID, g.density_filter, cloud, "count", rule=2).endswith("unknown rule (ERASOR_DENSITY_ABS or _MAD)")
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            c = cloud.copy()
            c[5, col] = bad
            for fn, a in ((g.knn, (4,)), (g.radius_count, (0.5,)), (g.density_filter, ("kth",)), (g.density_filter, ("count",))):
                assert refused(E_INVALID, fn, c, *a).endswith("non-finite coordinate (NaN / Inf) in 1 point(s)")
    L, p = gpu_mod.lib(), cloud.ctypes.data_as(C.c_void_p)
    kr, st, dr, f = gpu_mod.KnnResult(), gpu_mod.ScoreStats(), gpu_mod.DensityResult(), gpu_mod.DensityFilter(0, 0, 4, 0, 0.5, 0.5, 1.0)
    n = C.c_size_t(len(cloud))
    err = lambda: L.erasor_hip_last_error(g._h).decode()
    # more than 2^30 points, a NULL cloud
    for big, ptr in ((C.c_size_t(2 ** 30 + 1), p), (C.c_size_t(3), None)):
        assert L.erasor_hip_knn_clouds(g._h, ptr, big, 0, C.c_uint32(4), None, None, None, None, C.byref(kr)) == E_INVALID
        assert err() == "erasor_hip_knn_clouds: NULL cloud or more than 2^30 points"
        assert L.erasor_hip_radius_count_clouds(g._h, ptr, big, 0, C.c_double(0.5), None, C.byref(st)) == E_INVALID
        assert L.erasor_hip_density_filter_clouds(g._h, ptr, big, 0, C.byref(f), None, None, C.c_size_t(0), C.byref(dr)) == E_INVALID
    # res NULL, filter NULL
    assert L.erasor_hip_knn_clouds(g._h, p, n, 0, C.c_uint32(4), None, None, None, None, None) == E_INVALID and err() == "erasor_hip_knn_clouds: res is NULL"
    assert L.erasor_hip_radius_count_clouds(g._h, p, n, 0, C.c_double(0.5), None, None) == E_INVALID and err().endswith("res is NULL")
    assert L.erasor_hip_density_filter_clouds(g._h, p, n, 0, C.byref(f), None, None, C.c_size_t(0), None) == E_INVALID and err().endswith("res is NULL")
    assert L.erasor_hip_density_filter_clouds(g._h, p, n, 0, None, None, None, C.c_size_t(0), C.byref(dr)) == E_INVALID and err().endswith("filter is NULL")
    assert L.erasor_hip_knn_map(g._h, C.c_uint32(4), None, None, None, None, None) == E_INVALID
    # neighbour lists with n * k > 2^30 (refused before anything is read: the device pointer is never followed)
    dummy = np.zeros(4, np.uint32)
    assert L.erasor_hip_knn_clouds(g._h, p, C.c_size_t(2 ** 25 + 1), 1, C.c_uint32(32), dummy.ctypes.data_as(C.c_void_p), None, None, None,
                                   C.byref(kr)) == E_INVALID and err() == "erasor_hip_knn_clouds: neighbour lists need n * k <= 2^30"
    # N = 0: everything zero or NaN
    empty = np.zeros((0, 4), np.float32)
    assert_same_knn(g.knn(empty, 5, True), evalmap.knn(empty, 5, True), "empty")
    cnt, s = g.radius_count(empty, 0.5)
    assert len(cnt) == 0 and same_numbers(s, evalmap.radius_count(empty, 0.5)[1]) and s["n_scored"] == 0 and math.isnan(s["max"])
    for score in ("kth", "mean", "count"):
        for rule in ("abs", "mad"):
            assert_same_filter(g.density_filter(empty, score, rule=rule), evalmap.density_filter(empty, score, rule=rule), ("empty", score, rule))
    # the handle's map: none yet; then a step in flight
    for fn, a in ((g.knn_map, (4,)), (g.radius_count_map, (0.5,)), (g.density_filter_map, ())):
        assert "no map" in refused(E_STATE, fn, *a)
    sc = scenarios.small(n_frames=2, az=60)
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    for fn, a in ((g.knn, (cloud, 4)), (g.knn_map, (4,)), (g.radius_count, (cloud, 0.5)), (g.radius_count_map, (0.5,)), (g.density_filter, (cloud,)),
                  (g.density_filter_map, ())):
        assert "in flight" in refused(E_STATE, fn, *a)
    g.step_wait()
    assert g.knn(cloud, 4)["n_short"] == 0  # the handle is fine after the refusals
    # the header's layout
    S, K, F, R = gpu_mod.ScoreStats, gpu_mod.KnnResult, gpu_mod.DensityFilter, gpu_mod.DensityResult
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
            'sizeof(erasor_score_stats), sizeof(erasor_knn_result), sizeof(erasor_density_filter), sizeof(erasor_density_result), '
            'offsetof(erasor_score_stats, max), offsetof(erasor_knn_result, mean), offsetof(erasor_density_filter, min_neighbors), '
            'offsetof(erasor_density_filter, radius), offsetof(erasor_density_filter, mul), offsetof(erasor_density_result, m), '
            'offsetof(erasor_density_result, max), ERASOR_DENSITY_KTH, ERASOR_DENSITY_MEAN, ERASOR_DENSITY_COUNT, ERASOR_DENSITY_ABS, '
            'ERASOR_DENSITY_MAD);return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(S), C.sizeof(K), C.sizeof(F), C.sizeof(R), S.max.offset, K.mean.offset, F.min_neighbors.offset, F.radius.offset, F.mul.offset,
                   R.m.offset, R.max.offset] + [gpu_mod.DENSITY_SCORES[s] for s in ("kth", "mean", "count")] + [gpu_mod.DENSITY_RULES[s] for s in ("abs", "mad")]
    assert (C.sizeof(S), C.sizeof(K), C.sizeof(F), C.sizeof(R)) == (48, 112, 40, 120)
    assert gpu_mod.DENSITY_SCORES == evalmap.DENSITY_SCORES and gpu_mod.DENSITY_RULES == evalmap.DENSITY_RULES and gpu_mod.KNN_NONE == NONE


# ---- 10. worlds ----
def sprinkled_world():
    sc = scenarios.small(n_frames=3, az=60) if ON_CPU else scenarios.small()
    m = np.ascontiguousarray(sc["map"], np.float32)
    rng = np.random.default_rng(8)
    lo, hi = m[:, :3].min(0), m[:, :3].max(0)
    air = xyzi(rng.uniform(lo, hi + [0, 0, 6.0], (300, 3)), rng.choice([40.0, 252.0, 259.0], 300))
    return np.ascontiguousarray(np.concatenate([m, air])[rng.permutation(len(m) + 300)])


def test_the_voxelised_synthetic_map_with_sprinkled_points(handle):
    world = sprinkled_world()
    cloud = np.ascontiguousarray(handle.voxelize_preserving_labels(world, 0.2), np.float32)
    assert len(cloud) > 1500
    check_knn(handle, cloud, 8, what="world")
    check_count(handle, cloud, 0.5, what="world")
    for kw in (dict(score="mean", k=8, rule="mad", mul=2.0), dict(score="kth", k=8, rule="abs", thr=0.6), dict(score="count", radius=0.5, min_neighbors=3)):
        w = check_filter(handle, cloud, "world", **kw)
        assert 0 < w[2]["n_removed"] < len(cloud)
    # the same from a device buffer
    p = handle.device_array(cloud)
    try:
        assert_same_filter(handle.density_filter((p, len(cloud)), "mean", k=8, rule="mad", mul=2.0), evalmap.density_filter(cloud, "mean", k=8, rule="mad", mul=2.0),
                           "device cloud")
    finally:
        handle.device_free(p)


def test_random_world_of_200000_points_at_k_16(handle):
    rng = np.random.default_rng(11)
    cloud = xyzi(rng.uniform(0, 41.0, (200000, 3)), rng.integers(0, 300, 200000))
    cloud[::1000, :3] = cloud[0, :3]  # 200 copies of one point among them
    want = check_knn(handle, cloud, 16, what="random world")
    assert want["kth_stats"]["n_scored"] == 200000 and want["kth_stats"]["min"] == 0.0
    check_filter(handle, cloud, "random world", score="mean", k=16, rule="mad", mul=2.0)
    check_count(handle, cloud, 0.5, what="random world")


def test_the_map_calls_and_the_step_after_them(gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, plain = (gpu_mod.Erasor(scenarios.to_product_params(sc["params"])) for _ in range(2))
    for e in (g, plain):
        e.set_map(sc["map"])
        for f in range(n):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    # a node announced ahead, then the calls: the map's answers are those of the map read back
    ticket = g.prefetch_node_rows(np.ascontiguousarray(sc["scans"][n], np.float32), 3, sc["T_l2b"], sc["T_b2o"][n], sc["T_o2b"][n])
    m = np.ascontiguousarray(g.get_map(), np.float32)
    k = 4 if ON_CPU else 8
    assert_same_knn(g.knn_map(k, True), evalmap.knn(m, k, True), "knn_map")
    cnt, st = g.radius_count_map(0.4)
    want = evalmap.radius_count(m, 0.4)
    assert cnt.tobytes() == want[0].tobytes() and same_numbers(st, want[1])
    assert_same_filter(g.density_filter_map("mean", k=k, rule="mad", mul=2.0), evalmap.density_filter(m, "mean", k=k, rule="mad", mul=2.0), "density_filter_map")
    assert_same_filter(g.density_filter_map("count", radius=0.4, min_neighbors=4, keep=False),
                       evalmap.density_filter(m, "count", radius=0.4, min_neighbors=4, keep=False), "density_filter_map, count")
    assert g.get_map().tobytes() == m.tobytes()  # the map itself stays as it is
    # the announcement and the last step's clouds are untouched: the next step is the uninterrupted run's
    a = g.step_ticket(ticket, sc["T_b2o"][n], sc["T_o2b"][n])
    b = plain.step(sc["scans"][n], sc["T_l2b"], sc["T_b2o"][n], sc["T_o2b"][n])
    assert a.as_dict() == b.as_dict()
    assert g.get_map().tobytes() == plain.get_map().tobytes()
    for which in (gpu_mod.CLOUD_MAP_REJECTED, gpu_mod.CLOUD_STATIC_ESTIMATE):
        assert g.get_cloud(which).tobytes() == plain.get_cloud(which).tobytes()
