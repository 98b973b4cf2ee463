"""The host restatement of the point-to-plane pose refinement (evalmap.refine_poses_plane) on its own: the ranks of designed lattices whose
normals are exact axis vectors, what a single plane leaves untouched, a map without normals, rank_tol = 0, recovery where the
point-to-point refinement is biased, and the normals' orientation, which cannot matter.  No GPU."""
import numpy as np
import pytest

import refine_plane_world as pw
import refine_world as rw
from erasor_amd import evalmap

KW = dict(k=8, max_dist=0.5)


@pytest.fixture(scope="module")
def lattice_runs():
    """name -> (map, scan, T_given, the restatement's answer), computed once"""
    out = {}
    for name, (m, _) in pw.lattices().items():
        scan, Tg = pw.own_points_scan(m)
        out[name] = (m, scan, Tg, evalmap.refine_poses_plane(m, [scan], [Tg], **KW))
    return out


# ---- the designed lattices ----
@pytest.mark.parametrize("name", list(pw.lattices()))
def test_lattice_normals_are_exact_axis_vectors_and_the_rank_is_the_planes(lattice_runs, name):
    m, scan, Tg, (T, rows, summ) = lattice_runs[name]
    want_rank = pw.lattices()[name][1]
    nrm, curv, _, res = evalmap.normals(pw.xyzi(m), 8)
    assert res["n_ambiguous"] == 0 and res["n_short"] == 0 and res["n_degenerate"] == 0
    axes = {(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)}
    assert set(map(tuple, nrm.tolist())) <= axes and len(set(map(tuple, nrm.tolist()))) == {3: 1, 5: 2, 6: 3}[want_rank]
    assert (curv == 0.0).all()
    r = rows[0]
    assert r["rank"] == want_rank and r["status"] == evalmap.REFINE_CONVERGED and r["n_pairs_first"] == len(m) and r["n_unusable_first"] == 0
    assert summ["n_map_no_normal"] == 0 and summ["n_status"] == [1, 0, 0, 0, 0]
    assert (r["lambda_ratio"] == 0.0) == (want_rank < 6) and 0.0 <= r["lambda_ratio"] < 1.0
    assert r["rms_plane_last"] < 1e-6 < r["rms_plane_first"]


def test_numpy_eigh_gives_the_same_ranks(lattice_runs):
    """the prototype's check: the normal equations under the given pose, solved by numpy's eigh and not by _jacobi6"""
    for name, (m, scan, Tg, _) in lattice_runs.items():
        m64 = m.astype(np.float64)
        nrm, curv, _, _ = evalmap.normals(pw.xyzi(m), 8)
        T0 = Tg.astype(np.float64)
        S, pairs, bad, unusable = evalmap.refine_plane_frame_sums(m64, evalmap.cKDTree(m64), nrm, curv, scan[:, :3], T0[:3, :3].reshape(-1).tolist(),
                                                                  T0[:3, 3].tolist(), 0.25, 1.0)
        A = np.zeros((6, 6))
        A[np.triu_indices(6)] = S[:21]
        A = A + np.triu(A, 1).T
        lam = np.linalg.eigvalsh(A)
        assert int((lam > 1e-9 * lam.max()).sum()) == pw.lattices()[name][1], (name, lam)
        assert pairs == len(m) and bad == 0 and unusable == 0


def test_one_plane_leaves_the_in_plane_translation_and_the_yaw_alone(lattice_runs):
    m, scan, Tg, (T, rows, summ) = lattice_runs["one plane"]
    # every normal is (0, 0, 1): J = (q'y, -q'x, 0, 0, 0, 1), so the columns of the yaw and of t's x and y are exactly zero ...
    m64 = m.astype(np.float64)
    nrm, curv, _, _ = evalmap.normals(pw.xyzi(m), 8)
    T0 = Tg.astype(np.float64)
    R0, t0 = T0[:3, :3].reshape(-1).tolist(), T0[:3, 3].tolist()
    S, _, _, _ = evalmap.refine_plane_frame_sums(m64, evalmap.cKDTree(m64), nrm, curv, scan[:, :3], R0, t0, 0.25, 1.0)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            assert (S[k] == 0.0) == (a in (2, 3, 4) or b in (2, 3, 4)), (a, b, S[k])
            k += 1
    assert S[23] == 0.0 and S[24] == 0.0 and S[25] == 0.0
    # ... the update has no component along them: the quaternion's z is exactly zero (D's yaw-only entries xy +- wz hold no wz) ...
    R1, t1, st, sr, rank, ratio = evalmap.refine_plane_solve([float(s) for s in S], R0, t0, 1e-9)
    assert rank == 3 and ratio == 0.0 and t1[0] == t0[0] and t1[1] == t0[1] and t1[2] != t0[2] and st > 0.0
    # ... and t's in-plane components come back bit for bit after every iteration
    assert rows[0]["iters"] >= 2
    assert T[0][0, 3].tobytes() == np.float64(Tg[0, 3]).tobytes() and T[0][1, 3].tobytes() == np.float64(Tg[1, 3]).tobytes()
    assert T[0][2, 3] != np.float64(Tg[2, 3])
    # a frame that is wrong only by a yaw and an in-plane shift has nothing to correct: r is exactly zero and the pose is kept bit for bit
    scan2, Tg2 = pw.own_points_scan(m, T_true=rw.pose(np.eye(3), [0.0, 0.0, 0.0]), T_err=rw.pose(rw.rot(0.0, 0.0, 0.004), [0.004, -0.003, 0.0]))
    T2, rows2, _ = evalmap.refine_poses_plane(m, [scan2], [Tg2], **KW)
    assert T2[0].tobytes() == Tg2.astype(np.float64).tobytes() and rows2[0]["status"] == 0 and rows2[0]["iters"] == 1 and rows2[0]["rank"] == 3
    assert rows2[0]["rms_plane_first"] == 0.0 and rows2[0]["rms_first"] > 0.0


def test_three_planes_converge(lattice_runs):
    m, scan, Tg, (T, rows, summ) = lattice_runs["three perpendicular planes"]
    et, er = rw.pose_error(T[0], pw.T_TRUE)
    e0t, e0r = rw.pose_error(Tg.astype(np.float64), pw.T_TRUE)
    print("three planes: %d iterations, left %.3g m %.3g rad (given %.3g m %.3g rad)" % (rows[0]["iters"], et, er, e0t, e0r))
    # measured with the restatement: 2 iterations, 2.4e-8 m and 4.7e-9 rad left (float32 scan coordinates: 6e-8 at these sizes); ten times that
    assert rows[0]["iters"] <= 3 and et < 2.4e-7 and er < 4.7e-8 and e0t > 5e-3 and e0r > 3e-3


def test_a_map_without_normals_gives_few_pairs_and_keeps_the_pose():
    m = pw.plane(2, 0.0, 3)[:8].astype(np.float32)  # 8 points, k = 8: every point is short of neighbours
    scan, Tg = pw.own_points_scan(m)
    T, rows, summ = evalmap.refine_poses_plane(m, [scan], [Tg], min_pairs=1, **KW)
    r = rows[0]
    assert r["status"] == evalmap.REFINE_FEW_PAIRS and r["iters"] == 0 and r["n_pairs_first"] == 0 and r["n_unusable_first"] == 8 == r["n_unusable_last"]
    assert r["rank"] == 0 and np.isnan(r["lambda_ratio"]) and np.isnan(r["rms_first"]) and np.isnan(r["rms_plane_first"])
    assert T[0].tobytes() == Tg.astype(np.float64).tobytes() and summ["n_map_no_normal"] == 8 and summ["n_status"] == [0, 0, 1, 0, 0]


def test_rank_tol_zero_on_a_single_plane(lattice_runs):
    """rank_tol = 0 keeps every direction with a positive eigenvalue.  On the lattice plane the three null directions' rows and columns
    of A are exactly zero, no rotation touches them and their eigenvalues are exactly 0.0: the rank is 3 under both, and so is every
    bit of the answer.  A plane whose normals are not exact has tiny positive eigenvalues instead; there the two differ."""
    m, scan, Tg, ref = lattice_runs["one plane"]
    zero = evalmap.refine_poses_plane(m, [scan], [Tg], rank_tol=0.0, **KW)
    assert zero[1][0]["rank"] == 3 and str(zero[1]) == str(ref[1]) and zero[0].tobytes() == ref[0].tobytes()
    # tilted a little, the same plane's normals carry rounding: the null directions' eigenvalues are tiny, and positive or negative
    Rt = rw.rot(0.3, -0.2, 0.1)
    tilted = (m.astype(np.float64) @ Rt.T).astype(np.float32)
    scan_t, Tg_t = pw.own_points_scan(tilted)
    r9 = evalmap.refine_poses_plane(tilted, [scan_t], [Tg_t], max_iters=1, **KW)[1][0]
    r0 = evalmap.refine_poses_plane(tilted, [scan_t], [Tg_t], max_iters=1, rank_tol=0.0, **KW)[1][0]
    print("tilted plane: rank %d at 1e-9, %d at 0, lambda_ratio %.3g" % (r9["rank"], r0["rank"], r9["lambda_ratio"]))
    # (the restatement gives 3 and 6 here, with lambda_ratio 3.9e-16)
    assert r9["rank"] == 3 and 3 < r0["rank"] <= 6 and abs(r9["lambda_ratio"]) < 1e-9


def test_a_solve_without_a_positive_eigenvalue_is_degenerate():
    """status 4 (REFINE_DEGENERATE): what refine_plane_solve answers when lambda_max is not > 0.  A pair's J holds a unit normal, so sums
    of real pairs never get there; the rule is checked on the solve itself"""
    R, t = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.5, -0.25, 2.0]
    for S in ([0.0] * 29, [0.0] * 21 + [1.0] * 8, [float("nan")] * 29):
        R1, t1, st, sr, rank, ratio = evalmap.refine_plane_solve(S, R, t, 1e-9)
        assert (R1, t1, st, sr, rank) == (R, t, 0.0, 0.0, 0) and np.isnan(ratio)
    assert evalmap.REFINE_DEGENERATE == 4 and len(evalmap.REFINE_PLANE_ROW_FIELDS) == 16 and len(evalmap.REFINE_PLANE_SUMMARY_FIELDS) == 9


# ---- recovery where point-to-point is biased ----
@pytest.fixture(scope="module")
def biased():
    m, surfaces = pw.biased_world()
    scans, T_true, T_given, seen = pw.biased_frames(surfaces)
    return m, scans, T_true, T_given, seen, evalmap.refine_poses(m[:, :3], scans, T_given), evalmap.refine_poses_plane(m[:, :3], scans, T_given)


def test_plane_refinement_recovers_what_point_to_point_leaves(biased):
    m, scans, T_true, T_given, seen, p2p, pl = biased
    worst_t = worst_r = 0.0
    for f in range(len(scans)):
        # the frame sees the ground and both walls, and the restatement says so: all six directions held, none of them weakly
        assert min(seen[f]) > 500 and pl[1][f]["rank"] == 6 and pl[1][f]["lambda_ratio"] > 1e-3, (seen[f], pl[1][f])
        (at, ar), (bt, br) = rw.pose_error(p2p[0][f], T_true[f]), rw.pose_error(pl[0][f], T_true[f])
        print("frame %d: point-to-point %d iterations, %.4f m %.5f rad left; point-to-plane %d iterations, %.4f m %.5f rad left" % (
            f, p2p[1][f]["iters"], at, ar, pl[1][f]["iters"], bt, br))
        assert bt < at and br < ar
        assert pl[1][f]["status"] == evalmap.REFINE_CONVERGED and pl[1][f]["iters"] < p2p[1][f]["iters"]
        worst_t, worst_r = max(worst_t, bt), max(worst_r, br)
    # measured with the restatement (MEASUREMENTS.md "Refine"): 1.68 mm and 75 urad at the worst of the three frames, after 4 iterations
    # each (the point-to-point refinement: 10.9 to 15.9 mm and 0.9 to 2.5 mrad after 20); ten times that
    assert worst_t < 1.68e-2 and worst_r < 7.5e-4


# ---- the normals' orientation cannot matter ----
def test_flipping_the_map_normals_changes_no_bit(biased):
    m, scans, T_true, T_given, seen, _, ref = biased  # (no NaN in these rows: str() compares every bit)
    rng = np.random.default_rng(8)
    flips = []

    def flip(nrm, curv):
        s = rng.random(len(nrm)) < 0.5
        flips.append(int(s.sum()))
        return np.where(s[:, None], -nrm, nrm)

    got = evalmap.refine_poses_plane(m[:, :3], scans, T_given, normals_hook=flip)
    assert flips and 0.4 * len(m) < flips[0] < 0.6 * len(m)
    assert got[0].tobytes() == ref[0].tobytes() and str(got[1]) == str(ref[1]) and str(got[2]) == str(ref[2])
