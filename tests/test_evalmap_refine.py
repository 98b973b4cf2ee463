"""evalmap.refine_poses, the host restatement of Erasor.refine_poses, on its own (no GPU): its pieces against independent forms -- the
defined sum against explicit loops, the Jacobi eigenvectors against numpy, the whole call against a brute-force ICP with a dense distance
matrix --, the statuses, and that it recovers known pose errors on the small world (tests/refine_world.py) to a measured bound."""
import math

import numpy as np
import pytest

import refine_world as rw
from erasor_amd import evalmap

# The worst remaining error of the six frames of the small world, measured with this file on the CPU (MEASUREMENTS.md, "Refine"):
# 5.3e-8 m and 3.7e-9 rad.  The input is noise-free (every scan point IS a map point, rounded to float32 in the body frame), so only that
# rounding and the stopping rule remain; the test allows ten times the measured figures.
MEASURED_T, MEASURED_R = 5.3e-8, 3.7e-9


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.full((len(xyz), 1), w, np.float32)], 1)


def loop_tree_sum(v):
    """the defined order with explicit loops over Python floats"""
    n, k = v.shape
    out = []
    for c in range(k):
        total = 0.0
        for lo in range(0, n, 256):
            x = [float(a) for a in v[lo:lo + 256, c]] + [0.0] * (256 - len(v[lo:lo + 256]))
            s = 128
            while s >= 1:
                for i in range(s):
                    x[i] = x[i] + x[i + s]
                s //= 2
            total = total + x[0]
        out.append(total)
    return np.array(out)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_the_defined_sum_equals_the_explicit_loops(n):
    rng = np.random.default_rng(n)
    v = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-8, 8, (n, 3))
    assert evalmap.refine_tree_sum(v).tobytes() == loop_tree_sum(v).tobytes()


def test_jacobi_finds_the_eigenvectors():
    rng = np.random.default_rng(4)
    for _ in range(20):
        B = rng.normal(size=(4, 4))
        A0 = (B + B.T) / 2
        A = [[float(x) for x in row] for row in A0]
        V = np.array(evalmap._jacobi4(A))
        lam = np.array([A[i][i] for i in range(4)])
        assert all(A[i][j] == 0.0 for i in range(4) for j in range(i + 1, 4))  # the stopping rule was reached, not the sweep limit
        assert np.allclose(np.sort(lam), np.linalg.eigvalsh(A0), atol=1e-13)
        assert np.allclose(A0 @ V, V * lam[None, :], atol=1e-13) and np.allclose(V.T @ V, np.eye(4), atol=1e-14)
    # a zero matrix: no rotation at all, the first eigenvector is w = 1 (the identity update)
    assert evalmap._jacobi4([[0.0] * 4 for _ in range(4)]) == [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]


def test_one_solve_recovers_a_rigid_motion_exactly_paired():
    rng = np.random.default_rng(8)
    p = rng.uniform(-5, 5, (50, 3))
    Rt, tt = rw.rot(0.2, -0.1, 0.7), np.array([0.5, -1.0, 0.25])
    m = p @ Rt.T + tt
    v = np.zeros((50, 16))
    v[:, 0:3], v[:, 3:6] = p, m
    v[:, 6:15] = (p[:, :, None] * m[:, None, :]).reshape(50, 9)
    S = [float(s) for s in evalmap.refine_tree_sum(v)]
    R, t, st, sr = evalmap.refine_solve(S, 50, [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], [0.0, 0.0, 0.0])
    assert np.allclose(np.array(R).reshape(3, 3), Rt, atol=1e-13) and np.allclose(t, tt, atol=1e-12)
    assert abs(st - np.linalg.norm(tt)) < 1e-12 and sr > 0.5


def brute_nearest(map64, tree, q):
    """every pair in a dense matrix, the first of equal minima"""
    d2 = evalmap.pair_d2(q[:, None, :], map64[None, :, :])
    j = np.argmin(d2, axis=1)
    return d2[np.arange(len(q)), j], j


def brute_refine(m, scans, Tg, Tl, max_dist, eps_t, eps_r, max_iters, min_pairs):
    """an ICP of its own around a dense distance matrix, loop_tree_sum and the restatement's solve: (T, statuses, iterations)"""
    m64 = np.asarray(m, np.float32).astype(np.float64)
    out, stat, its = [], [], []
    for f, s in enumerate(scans):
        p32 = evalmap._xform(np.eye(4, dtype=np.float32) if Tl is None else Tl, np.asarray(s, np.float32)[:, :3])
        p = p32.astype(np.float64)
        T0 = np.asarray(Tg[f], np.float32).reshape(4, 4).astype(np.float64)
        R, t = [float(x) for x in T0[:3, :3].reshape(9)], [float(x) for x in T0[:3, 3]]
        status, n_it = 1, 0
        for it in range(1, max_iters + 1):
            v = np.zeros((len(p), 16))
            pairs = 0
            for i in range(len(p)):
                r = [(R[3 * a] * p[i, 0] + R[3 * a + 1] * p[i, 1]) + R[3 * a + 2] * p[i, 2] for a in range(3)]
                q = np.array([r[a] + t[a] for a in range(3)])
                e = q[None, :] - m64
                d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                j = int(np.argmin(d2))
                if d2[j] <= max_dist * max_dist:
                    mm = [float(m64[j, a]) - t[a] for a in range(3)]
                    v[i] = r + mm + [r[a] * mm[b] for a in range(3) for b in range(3)] + [float(d2[j])]
                    pairs += 1
            if pairs < max(min_pairs, 1):
                status = 2
                break
            R, t, st, sr = evalmap.refine_solve([float(x) for x in loop_tree_sum(v)], pairs, R, t)
            n_it = it
            if st <= eps_t and sr <= eps_r:
                status = 0
                break
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = np.array(R).reshape(3, 3), t
        out.append(T)
        stat.append(status)
        its.append(n_it)
    return np.array(out), stat, its


def test_the_restatement_equals_a_brute_force_icp_on_tiny_inputs():
    rng = np.random.default_rng(21)
    m = np.concatenate([rng.uniform(-4, 4, (500, 3)) * [1, 1, 0.02], rng.uniform(-4, 4, (300, 3)) * [0.02, 1, 0.5] + [4, 0, 2],
                        rng.uniform(-4, 4, (300, 3)) * [1, 0.02, 0.5] + [0, 4, 2]]).astype(np.float32)
    scans, Tg = [], []
    for n in (40, 257, 300):
        Tt = rw.pose(rw.rot(0.01, -0.02, rng.uniform(-3, 3)), rng.uniform(-1, 1, 3))
        sub = m[rng.choice(len(m), n, replace=False)].astype(np.float64)
        scans.append(xyzi((sub - Tt[:3, 3]) @ Tt[:3, :3]))
        Tg.append((rw.pose(rw.rot(0.01, 0.01, -0.015), [0.08, -0.05, 0.04]) @ Tt).astype(np.float32))
    scans.append(xyzi(rng.uniform(-1, 1, (30, 3)) + [0, 0, 50.0]))  # too far away for a pair
    Tg.append(np.eye(4, dtype=np.float32))
    Tl = np.eye(4, dtype=np.float32)
    Tl[2, 3] = 0.5
    for T_l2b in (None, Tl):
        kw = dict(max_dist=0.7, eps_t=1e-5, eps_r=1e-6, max_iters=8, min_pairs=10)
        T, rows, summ = evalmap.refine_poses(m, scans, Tg, T_l2b, **kw)
        T2, rows2, summ2 = evalmap.refine_poses(m, scans, Tg, T_l2b, nearest=brute_nearest, **kw)
        Tb, stat, its = brute_refine(m, scans, Tg, T_l2b, **kw)
        assert T.tobytes() == T2.tobytes() == Tb.tobytes()
        assert str(rows) == str(rows2)  # (by text: NaN fields)
        assert [r["status"] for r in rows] == stat and [r["iters"] for r in rows] == its
        assert rows[3]["status"] == evalmap.REFINE_FEW_PAIRS and rows[3]["iters"] == 0 and np.isnan(rows[3]["rms_first"])
        assert T[3].tobytes() == np.eye(4).tobytes()
        assert summ["n_status"][2] == 1 and summ["n_frames"] == 4 and summ == summ2


def test_nearest_breaks_ties_towards_the_lowest_index():
    g = np.arange(4.0)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(1)
    lattice = lattice[rng.permutation(len(lattice))]
    from scipy.spatial import cKDTree
    q = np.array([[0.5, 0.5, 0.5], [1.5, 2.5, 0.5], [1.0, 1.0, 1.5], [2.5, 2.0, 2.0], [1.0, 2.0, 3.0]])
    d2, j = evalmap.nearest_f64(lattice, cKDTree(lattice), q)
    d2b, jb = brute_nearest(lattice, None, q)
    assert d2.tobytes() == d2b.tobytes() and list(j) == list(jb)
    assert list(d2) == [0.75, 0.75, 0.25, 0.25, 0.0]


def test_statuses_and_refusals():
    m = xyzi(np.random.default_rng(0).uniform(-3, 3, (400, 3)))[:, :3]
    bad = np.eye(4, dtype=np.float32)
    bad[0, 3] = np.inf
    scans = [np.zeros((0, 4), np.float32), xyzi([[np.nan, 0, 0], [0, np.inf, 0]]), xyzi([[0.1, 0.2, 0.3]] * 5), xyzi(m[:50])]
    T, rows, summ = evalmap.refine_poses(m, scans, [np.eye(4, dtype=np.float32)] * 2 + [bad] + [np.eye(4, dtype=np.float32)], min_pairs=10, max_iters=1)
    assert [r["status"] for r in rows] == [3, 3, 3, 0] and [r["n_non_finite"] for r in rows] == [0, 2, 5, 0]
    assert rows[3]["iters"] == 1 and rows[3]["rms_last"] == 0.0 and rows[3]["moved_t"] == 0.0 and rows[3]["moved_r"] == 0.0
    assert np.isinf(T[2, 0, 3]) and T[2, 1, 1] == 1.0 and summ["n_status"] == [1, 0, 0, 3]
    for kw in (dict(max_iters=0), dict(max_iters=65), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(eps_t=-1.0), dict(eps_r=float("inf"))):
        with pytest.raises(ValueError):
            evalmap.refine_poses(m, scans, [np.eye(4)] * 4, **kw)
    with pytest.raises(ValueError):
        evalmap.refine_poses(np.zeros((0, 3)), scans, [np.eye(4)] * 4)


@pytest.fixture(scope="module")
def recovered():
    m = rw.world()
    scans, T_true, T_given = rw.frames(m)
    T, rows, summ = evalmap.refine_poses(m[:, :3], scans, T_given)
    return m, scans, T_true, T_given, T, rows, summ


def test_it_recovers_the_pose_errors_of_the_small_world(recovered):
    m, scans, T_true, T_given, T, rows, summ = recovered
    assert 18000 < len(m) < 25000 and len(scans) == 6
    worst_t = worst_r = 0.0
    for f in range(len(scans)):
        e0 = rw.pose_error(T_given[f].astype(np.float64), T_true[f])
        e1 = rw.pose_error(T[f], T_true[f])
        print("frame %d: given %.3f m %.3f deg -> %.3g m %.3g rad in %d iterations" % (f, e0[0], math.degrees(e0[1]), e1[0], e1[1], rows[f]["iters"]))
        assert 0.1 < e0[0] <= 0.3 + 1e-6 and math.radians(0.9) < e0[1] <= math.radians(2.0) + 1e-6
        worst_t, worst_r = max(worst_t, e1[0]), max(worst_r, e1[1])
    print("worst remaining error: %.3g m, %.3g rad" % (worst_t, worst_r))
    assert worst_t <= 10 * MEASURED_T and worst_r <= 10 * MEASURED_R
    assert summ["n_status"] == [6, 0, 0, 0] and all(r["rms_last"] < 1e-5 < 0.1 < r["rms_first"] for r in rows)
    assert summ["sum_d2_last"] < 1e-6 * summ["sum_d2_first"]


def test_no_frame_fits_the_map_worse_afterwards(recovered):
    m, scans, T_true, T_given, T, rows, summ = recovered
    before, _ = evalmap.align_frames(m[:, :3], scans, T_given, None, 0.2)
    after, _ = evalmap.align_frames(m[:, :3], scans, T.astype(np.float32), None, 0.2)
    for b, a in zip(before, after):
        assert a["frac_half"] >= b["frac_half"]
    assert min(a["frac_half"] for a in after) > 99.0 > 40.0 > max(b["frac_half"] for b in before)
