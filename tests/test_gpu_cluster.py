"""Euclidean clustering on the device (erasor_hip_cluster_clouds / _map, kernels in cluster.hip.h) against its host restatement
evalmap.cluster / cluster_brute: byte for byte in rows, ids, kept cloud and result.  The predicate at its edge, the grid's cell margin,
chains in every order, contention on one row, every size around the wavefront, workgroup and scan-block edges, bucket collisions and
the clamp, the table's box and counters, the size limits and the buffers, the errors and the struct layout, the synthetic world, the
handle's map, a step after the call, the residue and the driver.  tests/test_cluster_on_cpu.py re-runs this file against the CPU
stand-in."""
import ctypes as C
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
NONE = evalmap.CLUSTER_NONE
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


def assert_same(got, want, what):
    rows, ids, kept, res = got
    assert res == want[3], (what, res, want[3])
    assert rows.dtype == evalmap.CLUSTER_ROW_DTYPE and rows.dtype == want[0].dtype, what
    assert rows.shape == want[0].shape and rows.tobytes() == want[0].tobytes(), (what, "rows", rows[:3], want[0][:3])
    assert ids.dtype == np.uint32 and ids.shape == want[1].shape and ids.tobytes() == want[1].tobytes(), (what, "ids", np.flatnonzero(ids != want[1])[:5])
    assert kept.shape == want[2].shape and kept.tobytes() == want[2].tobytes(), (what, "kept cloud", kept.shape, want[2].shape)


def check(g, cloud, tol, min_size=1, max_size=0, ref=evalmap.cluster, what=""):
    """the device against the host restatement; what the host restatement returned"""
    want = ref(cloud, tol, min_size, max_size)
    assert_same(g.cluster(cloud, tol, min_size, max_size, ids=True, keep=True), want, what)
    return want


def steps(v, k):
    """the float32 values k steps above (below: k < 0) each of v"""
    v = np.asarray(v, np.float32).copy()
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


# ---- 1. the predicate at its edge ----
@pytest.mark.parametrize("tol", [0.2, 0.5, 1.0, 0.3])
def test_pairs_at_the_edge_of_the_predicate(handle, tol):
    """pairs whose distance is tol to within a few float32 steps, along each axis and the space diagonal, at the origin, across zero and
    far out: the pair at d <= tol is one cluster, the next step outside is two.  cluster_brute decides; both outcomes must occur."""
    K = np.arange(-3, 4)
    for base in (0.0, -tol / 2, 1e3, -1e3, 1e5, -1e5):
        for direction in range(4):
            a = np.full(3, base, np.float32)
            d = np.zeros(3, np.float32)
            if direction < 3:
                d[direction] = tol
            else:
                d[:] = tol / np.sqrt(3.0)
            if direction < 3:
                # the seven pairs in one cloud, 16 m (a power of two: exact at every offset used) beside one another along an axis
                # the pairs do not span
                pts = []
                for m, k in enumerate(K):
                    shift = np.zeros(3, np.float32)
                    shift[(direction + 1) % 3] = 16.0 * m
                    lo = a + shift
                    hi = lo + d
                    hi[direction] = steps(hi[direction], int(k))
                    pts += [lo, hi]
                want = check(handle, xyzi(pts), tol, ref=evalmap.cluster_brute, what=("edge", tol, base, direction))
                joined = want[1][0::2] == want[1][1::2]
            else:
                # the diagonal pair spans every axis: a cloud per pair, x stepped two float32 steps at a time (steps of the coordinate,
                # or of the displacement where the pair straddles zero and the coordinate's own steps are far finer)
                joined = []
                for k in 2 * K:
                    hi = a + d
                    hi[0] = steps(hi[0], int(k)) if abs(hi[0]) >= abs(d[0]) else a[0] + steps(d[0], int(k))
                    want = check(handle, xyzi([a, hi]), tol, ref=evalmap.cluster_brute, what=("edge", tol, base, "diagonal", k))
                    joined.append(want[3]["n_clusters"] == 1)
                joined = np.asarray(joined)
            assert joined[0] and not joined[-1], (tol, base, direction, joined)  # the innermost pair is joined, the outermost is not
            assert (np.diff(joined.astype(int)) <= 0).all(), (tol, base, direction, joined)  # and one edge between them
            if direction < 3 and tol in (0.5, 1.0):
                assert joined[3] and not joined[4], (tol, base, direction)  # d == tol exactly is joined, one step outside is not


# ---- 2. the cell margin ----
@pytest.mark.parametrize("tol", [0.5, 1.0, 0.3, 0.2])
def test_pairs_a_tolerance_apart_at_every_cell_border(handle, tol):
    """pairs the predicate joins, as far apart as it allows along one axis (exactly tol where float32 can say it), the lower point a few
    float32 steps around k * tol and around k * (the cell edge in use), k from -2^20 to 2^20: a 27-cell search must meet every pair."""
    ks = np.unique(np.concatenate([np.array([s * (2 ** e + j) for s in (-1, 1) for e in range(0, 21) for j in (-1, 0, 1)]), np.arange(-40, 41),
                                   np.linspace(-2 ** 20, 2 ** 20, 97).astype(np.int64)])).astype(np.float64)
    ks = ks[np.abs(ks) <= 2 ** 20]
    for edge in (tol, tol * CELL_MARGIN):
        for axis in range(3):
            lo = np.concatenate([steps((ks * edge).astype(np.float32), s) for s in range(-2, 3)])
            hi = (lo.astype(np.float64) + tol).astype(np.float32)
            # the largest float32 the predicate still joins to lo
            for _ in range(3):
                far = ~evalmap.cluster_adjacent(np.stack([lo, lo * 0, lo * 0], 1), np.stack([hi, lo * 0, lo * 0], 1), tol)
                hi = np.where(far, np.nextafter(hi, np.float32(-np.inf)), hi)
            nxt = np.nextafter(hi, np.float32(np.inf))
            grow = evalmap.cluster_adjacent(np.stack([lo, lo * 0, lo * 0], 1), np.stack([nxt, lo * 0, lo * 0], 1), tol)
            hi = np.where(grow, nxt, hi)
            ok = evalmap.cluster_adjacent(np.stack([lo, lo * 0, lo * 0], 1), np.stack([hi, lo * 0, lo * 0], 1), tol) & (hi > lo)
            lo, hi = lo[ok], hi[ok]
            n = len(lo)
            assert n > 900
            xyz = np.zeros((2 * n, 3), np.float32)
            xyz[0::2, axis], xyz[1::2, axis] = lo, hi
            xyz[0::2, (axis + 1) % 3] = xyz[1::2, (axis + 1) % 3] = 4.0 * np.arange(n)  # (pairs 4 m apart: tol <= 1)
            want = check(handle, xyzi(xyz), tol, ref=evalmap.cluster_brute, what=("margin", tol, edge, axis))
            assert want[3]["n_clusters"] == n and want[3]["largest"] == 2 and want[3]["n_singletons"] == 0


# ---- 3. chains ----
def line(n, tol, f=0.9):
    return np.stack([np.arange(n) * (f * tol), np.zeros(n), np.zeros(n)], 1).astype(np.float32)


def spiral(n, tol):
    th = np.zeros(n)
    for i in range(1, n):
        th[i] = th[i - 1] + 0.85 * tol / (2.0 + 0.3 * th[i - 1])
    r = 2.0 + 0.3 * th
    return np.stack([r * np.cos(th), r * np.sin(th), 0.01 * th], 1).astype(np.float32)


@pytest.mark.parametrize("order", ["increasing", "decreasing", "shuffled"])
@pytest.mark.parametrize("shape", ["line", "spiral"])
def test_a_chain_is_one_cluster_in_every_order(handle, shape, order):
    n, tol = 4096, 0.5
    xyz = line(n, tol) if shape == "line" else spiral(n, tol)
    assert evalmap.cluster_adjacent(xyz[:-1], xyz[1:], tol).all()
    perm = {"increasing": np.arange(n), "decreasing": np.arange(n)[::-1], "shuffled": np.random.default_rng(3).permutation(n)}[order]
    want = check(handle, xyzi(xyz[perm], np.arange(n) % 7 + 250), tol, what=(shape, order))
    assert want[3]["n_clusters"] == 1 and want[0]["first"].tolist() == [0] and want[0]["n_points"].tolist() == [n]
    # one link stretched just past tol: two clusters
    cut = 2500
    far = xyz.copy()
    if shape == "line":
        far[cut:, 0] += np.float32(0.1 * tol)
        while evalmap.cluster_adjacent(far[cut - 1:cut], far[cut:cut + 1], tol)[0]:
            far[cut:, 0] = steps(far[cut:, 0], 1)
    else:
        far = np.delete(far, cut, 0)  # (a missing point: a link of 1.7 tol)
    want = check(handle, xyzi(far[perm[perm < len(far)]]), tol, what=(shape, order, "cut"))
    assert want[3]["n_clusters"] == 2 and sorted(want[0]["n_points"].tolist()) == sorted([cut, len(far) - cut])


def test_two_interleaved_chains_that_never_touch(handle):
    n, tol = 2048, 0.5
    a, b = line(n, tol), line(n, tol)
    b[:, 1] = 2 * tol
    xyz = np.empty((2 * n, 3), np.float32)
    xyz[0::2], xyz[1::2] = a, b
    want = check(handle, xyzi(xyz), tol, what="interleaved")
    assert want[0]["first"].tolist() == [0, 1] and want[0]["n_points"].tolist() == [n, n]
    assert (want[1] == np.arange(2 * n) % 2).all()


# ---- 4. contention: every atomic of the table on one row ----
def test_identical_points_and_a_crowded_ball_are_one_cluster(handle):
    rng = np.random.default_rng(5)
    dup = xyzi(np.tile(np.float32([1.5, -2.25, 0.125]), (300, 1)), rng.integers(250, 262, 300))
    want = check(handle, dup, 0.5, what="duplicates")
    assert want[3]["n_clusters"] == 1 and want[0]["n_points"].tolist() == [300]
    side = 0.5 / np.sqrt(3.0) * 0.99
    ball = xyzi(rng.uniform(0, side, (5000, 3)) + [10.0, 20.0, -3.0], rng.integers(250, 262, 5000))  # 12.5 M pair tests
    want = check(handle, ball, 0.5, what="ball")
    assert want[3]["n_clusters"] == 1 and want[3]["largest"] == 5000


# ---- 5. sizes ----
def isolated(n, tol):
    i = np.arange(n)
    return xyzi(np.stack([(i % 50) * 3.0 * tol, ((i // 50) % 50) * 3.0 * tol, (i // 2500) * 3.0 * tol], 1), i % 5 + 250)


SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


@pytest.mark.parametrize("n", SIZES + [2047, 2048, 2049, 3071, 3072, 3073])
def test_sizes_of_isolated_points(handle, n):
    want = check(handle, isolated(n, 0.5), 0.5, what=("isolated", n))
    assert want[3]["n_clusters"] == n == want[3]["n_singletons"] and (want[1] == np.arange(n)).all()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_of_one_cluster_and_of_adjacent_pairs(handle, n):
    want = check(handle, xyzi(line(n, 0.5, 0.5), np.arange(n) % 3 + 251), 0.5, what=("one cluster", n))
    assert want[3]["n_clusters"] == min(n, 1) and want[3]["largest"] == n
    pairs = isolated(n, 0.5)
    pairs[1::2, :3] = pairs[0:2 * (n // 2):2, :3] + np.float32([0, 0, 0.25])
    want = check(handle, pairs, 0.5, what=("pairs", n))
    assert want[3]["n_clusters"] == (n + 1) // 2 and want[3]["n_singletons"] == n % 2


def test_hundred_thousand_isolated_points(handle):
    want = check(handle, isolated(100000, 0.5), 0.5, what="100 000 isolated")
    assert want[3]["n_clusters"] == 100000


# ---- 6. collisions and the clamp ----
def test_far_points_sharing_a_bucket_are_never_joined(handle):
    far = [[i * 1e6, j * 1e6, k * 1e6] for i in (-1, 0, 1) for j in (-1, 1) for k in (0, 1)]
    far += [[1e9, 0, 0], [1.1e9, 0, 0], [-3e9, 5e9, 0], [-3.5e9, 5e9, 0], [1e30, 1e30, 1e30], [-1e30, 1e30, 1e30]]  # beyond the 2^30-cell clamp
    for tol in (0.5, 1e-3):
        want = check(handle, xyzi(far), tol, ref=evalmap.cluster_brute, what=("far", tol))
        assert want[3]["n_clusters"] == len(far)
    # 1 024 buckets and a few thousand occupied cells: every bucket is shared
    want = check(handle, isolated(3000, 0.2), 0.2, what="shared buckets")
    assert want[3]["n_clusters"] == 3000


# ---- 7. the table ----
def test_the_box_finds_its_extremes_at_every_position(handle):
    rng = np.random.default_rng(7)
    base = rng.uniform(-0.05, 0.05, (70, 3)).astype(np.float32)
    for e in range(70):
        xyz = base.copy()
        pos = [(e + 11 * k) % 70 for k in range(6)]
        for a in range(3):
            xyz[pos[a], a] = -0.1 - 0.001 * e
            xyz[pos[3 + a], a] = 0.1 + 0.002 * e
        want = check(handle, xyzi(xyz + np.float32([3, -7, 1])), 0.5, ref=evalmap.cluster_brute, what=("extremes", e))
        assert want[3]["n_clusters"] == 1
        assert want[0]["min_xyz"][0].tolist() == [float(np.float32(xyz[pos[a], a] + np.float32([3, -7, 1])[a])) for a in range(3)]


def test_signed_zeros_labels_and_out_of_range_intensities(handle, gpu_mod):
    # -0.0 sorts below +0.0 in each coordinate, whichever comes first
    for flip in (False, True):
        z = np.float32([0.0, -0.0] if flip else [-0.0, 0.0])
        xyz = np.zeros((64 + 6, 3), np.float32)
        xyz[:, 0] = np.resize(z, 70)
        xyz[:, 1] = np.resize(z[::-1], 70)
        xyz[:, 2] = np.resize(np.float32([0.0, 0.0, -0.0]), 70)
        want = check(handle, xyzi(xyz), 0.2, what=("zeros", flip))
        assert np.signbit(want[0]["min_xyz"][0]).all() and not np.signbit(want[0]["max_xyz"][0]).any()
    w = np.float32([251, 252, 259, 260, 252 + (5 << 16), 259 + (65535 << 16), 40, np.nan, -1.0, 4294967296.0, np.inf, -np.inf, 4294967040.0, 0.0])
    rng = np.random.default_rng(8)
    cloud = xyzi(np.concatenate([rng.uniform(0, 0.1, (140, 3)), rng.uniform(0, 0.1, (70, 3)) + 5.0]), np.resize(w, 210))
    want = check(handle, cloud, 0.5, what="labels")
    assert want[0]["n_points"].tolist() == [140, 70] and want[0]["n_dynamic"].tolist() == [40, 20] and want[0]["n_label_out_of_range"].tolist() == [50, 25]


# ---- 8. the limits and the buffers ----
def sized_clusters():
    """clusters of 1 .. 6 points, three of each, their points interleaved through the cloud"""
    pts, rng = [], np.random.default_rng(9)
    for c in range(18):
        for _ in range(c % 6 + 1):
            pts.append([4.0 * c + rng.uniform(0, 0.2), rng.uniform(0, 0.2), rng.uniform(0, 0.2)])
    pts = np.asarray(pts, np.float32)
    return xyzi(pts[rng.permutation(len(pts))], rng.integers(250, 262, len(pts)))


@pytest.mark.parametrize("limits", [(0, 0), (1, 0), (3, 0), (1, 3), (3, 3), (2, 4), (4, 2), (6, 6), (7, 0), (1, 1), (2 ** 40, 0), (1, 2 ** 40)])
def test_size_limits_ids_and_the_kept_cloud(handle, limits):
    cloud = sized_clusters()
    want = check(handle, cloud, 0.5, *limits, what=limits)
    lo, hi = max(limits[0], 1), limits[1]
    n_listed = sum(3 for s in range(1, 7) if lo <= s and (hi == 0 or s <= hi))
    assert want[3]["n_listed"] == n_listed and want[3]["n_clusters"] == 18 and want[3]["n_singletons"] == 3 and want[3]["largest"] == 6
    assert ((want[1] == NONE).sum() == len(cloud) - want[3]["n_points_listed"]) and want[2].tobytes() == cloud[want[1] != NONE].tobytes()


def raw_call(gpu_mod, g, cloud, tol, mn, mx, ids, rows, cap_rows, kept, cap_kept, res, n=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return gpu_mod.lib().erasor_hip_cluster_clouds(g._h, p(cloud), C.c_size_t(len(cloud) if n is None else n), C.c_int(0), C.c_double(tol), C.c_size_t(mn),
                                                   C.c_size_t(mx), p(ids), p(rows), C.c_size_t(cap_rows), p(kept), C.c_size_t(cap_kept), C.byref(res))


def test_counts_only_and_buffers_too_small(handle, gpu_mod):
    cloud = sized_clusters()
    want = evalmap.cluster(cloud, 0.5, 2, 5)
    nl, nk = want[3]["n_listed"], want[3]["n_points_listed"]
    assert nl == 12 and 0 < nk < len(cloud)
    res = gpu_mod.ClusterResult()
    assert raw_call(gpu_mod, handle, cloud, 0.5, 2, 5, None, None, 0, None, 0, res) == 0 and res.as_dict() == want[3]  # counts only
    rows = np.zeros(nl + 2, gpu_mod.CLUSTER_ROW_DTYPE)
    kept = np.full((nk + 2, 4), -7.0, np.float32)
    ids = np.full(len(cloud), 12345, np.uint32)
    assert raw_call(gpu_mod, handle, cloud, 0.5, 2, 5, ids, rows, nl, kept, nk, res) == 0  # exactly enough
    assert rows[:nl].tobytes() == want[0].tobytes() and rows[nl:].tobytes() == bytes(80) and ids.tobytes() == want[1].tobytes()
    assert kept[:nk].tobytes() == want[2].tobytes() and (kept[nk:] == -7.0).all()
    for cap_rows, cap_kept in ((nl - 1, nk), (nl, nk - 1), (0, 0)):
        res = gpu_mod.ClusterResult()
        ids[:] = 12345
        assert raw_call(gpu_mod, handle, cloud, 0.5, 2, 5, ids, rows, cap_rows, kept, cap_kept, res) == E_CAPACITY
        assert res.as_dict() == want[3] and ids.tobytes() == want[1].tobytes()  # filled first
    # one buffer alone
    assert raw_call(gpu_mod, handle, cloud, 0.5, 2, 5, None, None, 0, kept, nk, res) == 0 and kept[:nk].tobytes() == want[2].tobytes()
    assert raw_call(gpu_mod, handle, cloud, 0.5, 2, 5, None, rows, nl, None, 0, res) == 0 and rows[:nl].tobytes() == want[0].tobytes()


# ---- 9. errors and the struct layout ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    cloud = sized_clusters()

    def refused(rc, fn, *a, **kw):
        with pytest.raises(gpu_mod.ErasorError) as e:
            fn(*a, **kw)
        assert e.value.rc == rc, str(e.value)
        return str(e.value)

    for tol in (0.0, -0.5, float("nan"), float("inf")):
        assert "tol" in refused(E_INVALID, g.cluster, cloud, tol)
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            c = cloud.copy()
            c[5, col] = bad
            assert "non-finite" in refused(E_INVALID, g.cluster, c, 0.5)
    res = gpu_mod.ClusterResult()
    assert raw_call(gpu_mod, g, cloud, 0.5, 1, 0, None, None, 0, None, 0, res, n=2 ** 30 + 1) == E_INVALID
    assert raw_call(gpu_mod, g, None, 0.5, 1, 0, None, None, 0, None, 0, res, n=3) == E_INVALID
    assert gpu_mod.lib().erasor_hip_cluster_clouds(g._h, cloud.ctypes.data_as(C.c_void_p), C.c_size_t(len(cloud)), C.c_int(0), C.c_double(0.5), C.c_size_t(1),
                                                   C.c_size_t(0), None, None, C.c_size_t(0), None, C.c_size_t(0), None) == E_INVALID  # res NULL
    # N = 0: zero clusters
    rows, ids, kept, r = g.cluster(np.zeros((0, 4), np.float32), 0.5, keep=True)
    assert len(rows) == 0 and len(ids) == 0 and len(kept) == 0 and r == dict.fromkeys(evalmap.CLUSTER_RESULT_FIELDS, 0)
    # the handle's map: none yet; then a step in flight
    assert "no map" in refused(E_STATE, g.cluster_map, 0.5)
    sc = scenarios.small(n_frames=2, az=60)
    g.set_map(sc["map"])
    g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
    refused(E_STATE, g.cluster, cloud, 0.5)
    refused(E_STATE, g.cluster_map, 0.5)
    g.step_wait()
    assert g.cluster(cloud, 0.5)[3]["n_clusters"] == 18  # the handle is fine after the refusals
    # the header's layout
    R, S = gpu_mod.ClusterRow, gpu_mod.ClusterResult
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
            'sizeof(erasor_cluster_row), sizeof(erasor_cluster_result), offsetof(erasor_cluster_row, n_dynamic), offsetof(erasor_cluster_row, min_xyz), '
            'offsetof(erasor_cluster_row, max_xyz), offsetof(erasor_cluster_result, n_listed), offsetof(erasor_cluster_result, largest));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(R), C.sizeof(S), R.n_dynamic.offset, R.min_xyz.offset, R.max_xyz.offset, S.n_listed.offset, S.largest.offset]
    assert C.sizeof(R) == 40 == gpu_mod.CLUSTER_ROW_DTYPE.itemsize == evalmap.CLUSTER_ROW_DTYPE.itemsize and C.sizeof(S) == 48


# ---- 10. worlds ----
def dynamic_points(cloud):
    c = np.ascontiguousarray(cloud, np.float32)
    return np.ascontiguousarray(c[np.isin(evalmap.labels(c[:, 3]), evalmap.DYNAMIC_CLASSES)])


def test_the_synthetic_worlds_moving_objects(handle):
    sc = scenarios.small(n_frames=3, az=60) if ON_CPU else scenarios.small()
    dyn = dynamic_points(sc["map"])
    assert len(dyn) > 100
    want = check(handle, dyn, 0.5, what="dynamic points")
    assert 1 <= want[3]["n_clusters"] < len(dyn) / 4 and (want[0]["n_dynamic"] == want[0]["n_points"]).all()
    want = check(handle, dyn, 0.5, 10, 0, what="dynamic points, small fragments dropped")
    assert want[3]["n_points_listed"] <= len(dyn)
    # the same from a device buffer
    p = handle.device_array(dyn)
    try:
        assert_same(handle.cluster((p, len(dyn)), 0.5, 10, 0, keep=True), want, "device cloud")
    finally:
        handle.device_free(p)


def test_random_world_of_200000_points(handle):
    rng = np.random.default_rng(11)
    cloud = xyzi(rng.uniform(0, 41.0, (200000, 3)), rng.integers(0, 300, 200000))
    want = check(handle, cloud, 0.5, what="random world")
    assert want[3]["largest"] > 20 and want[3]["n_singletons"] > 1000
    check(handle, cloud, 0.5, 5, 100, what="random world with limits")


def test_cluster_map_and_the_step_after_it(gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, plain = (gpu_mod.Erasor(scenarios.to_product_params(sc["params"])) for _ in range(2))
    for e in (g, plain):
        e.set_map(sc["map"])
        for f in range(n):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    # a node announced ahead, then the call: the map's clusters are those of the map read back
    ticket = g.prefetch_node_rows(np.ascontiguousarray(sc["scans"][n], np.float32), 3, sc["T_l2b"], sc["T_b2o"][n], sc["T_o2b"][n])
    m = np.ascontiguousarray(g.get_map(), np.float32)
    tol = 0.3 if ON_CPU else 0.5
    got = g.cluster_map(tol, 5, 0, ids=True, keep=True)
    assert_same(got, evalmap.cluster(m, tol, 5, 0), "cluster_map")
    assert_same(g.cluster(m, tol, 5, 0, keep=True), got, "cluster(get_map())")
    # the announcement and the last step's clouds are untouched: the next step is the uninterrupted run's
    a = g.step_ticket(ticket, sc["T_b2o"][n], sc["T_o2b"][n])
    b = plain.step(sc["scans"][n], sc["T_l2b"], sc["T_b2o"][n], sc["T_o2b"][n])
    assert a.as_dict() == b.as_dict()
    assert g.get_map().tobytes() == plain.get_map().tobytes()
    for which in (gpu_mod.CLOUD_MAP_REJECTED, gpu_mod.CLOUD_STATIC_ESTIMATE):
        assert g.get_cloud(which).tobytes() == plain.get_cloud(which).tobytes()


def test_residue_is_the_host_composition(handle):
    sc = scenarios.small(n_frames=3, az=60) if ON_CPU else scenarios.small()
    gt = np.ascontiguousarray(sc["map"], np.float32)
    dyn = np.isin(evalmap.labels(gt[:, 3]), evalmap.DYNAMIC_CLASSES)
    # an estimate that lost most moving points and some static ones
    keep = np.where(dyn, np.arange(len(gt)) % 3 == 0, np.arange(len(gt)) % 7 != 0)
    est = np.ascontiguousarray(gt[keep])
    rows, ids, pts, res = handle.residue(gt, est, tol=0.5, voxelsize=0.2, min_size=2)
    code, _ = evalmap.eval_codes(gt, est, 0.2)
    left = np.ascontiguousarray(gt[code == 2])
    assert len(left) > 10 and pts.tobytes() == left.tobytes()
    want = evalmap.cluster(left, 0.5, 2)
    assert res == want[3] and rows.tobytes() == want[0].tobytes() and ids.tobytes() == want[1].tobytes()
    assert (rows["n_dynamic"] == rows["n_points"]).all()


def test_driver_prints_the_clusters_and_writes_the_kept_cloud(tmp_path):
    from test_label_scans_driver import DEMO, ensure_demo, read_pcd_binary, write_pcd_binary
    ensure_demo()
    cloud = sized_clusters()
    write_pcd_binary(tmp_path / "c.pcd", cloud)
    out = subprocess.run([DEMO, "--clusters", str(tmp_path / "c.pcd"), "0.5", "2", "5", str(tmp_path / "kept.pcd")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows, _, kept, r = evalmap.cluster(cloud, 0.5, 2, 5)
    lines = out.stdout.splitlines()
    assert lines[0] == "clusters: n=%d  clusters=%d  listed=%d  points listed=%d  singletons=%d  largest=%d" % tuple(r[k] for k in evalmap.CLUSTER_RESULT_FIELDS)
    big = rows[np.argsort(-rows["n_points"].astype(np.int64), kind="stable")][0]
    assert lines[1].startswith("  first=%d  n=%d  dynamic=%d " % (big["first"], big["n_points"], big["n_dynamic"])), lines[1]
    assert len(lines) == 1 + len(rows) + 1 and read_pcd_binary(tmp_path / "kept.pcd").tobytes() == kept.tobytes()
