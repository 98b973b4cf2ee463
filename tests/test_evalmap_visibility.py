"""evalmap.visibility, the normative text of the see-through check, against its pure-Python check visibility_brute on random small inputs;
the pixel mapping going once round the circle on integer-ratio directions (no trigonometry here: the directions are lattice points
sorted by exact cross products); the frame transforms against numpy's inverse; the decision rule at its edges.  No GPU needed."""
import functools
from fractions import Fraction

import numpy as np
import pytest

from erasor_amd import evalmap


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def random_case(seed):
    rng = np.random.default_rng(seed)
    W, H = int(rng.choice([8, 16, 40])), int(rng.integers(1, 5))
    M = W // 8
    grid = {"width": W, "height": H, "col_tan": np.sort(rng.uniform(0.05, 0.95, M - 1)), "row_tan": np.sort(rng.uniform(-1.0, 1.0, H + 1))}
    n_frames = int(rng.integers(0, 5))
    cloud = xyzi(rng.uniform(-9, 9, (int(rng.integers(0, 120)), 3)) * [1, 1, 0.3], rng.integers(248, 264, 1)[0])
    if len(cloud) > 3 and seed % 3 == 0:
        cloud[1, :3] = cloud[2, :3]
    scans, T = [], np.zeros((n_frames, 4, 4), np.float32)
    for f in range(n_frames):
        s = xyzi(rng.uniform(-9, 9, (int(rng.integers(0, 90)), 3)) * [1, 1, 0.3])
        if len(s) > 4:
            s[0, 0] = np.nan
            s[1, :2] = 0.0
            s[2, :3] *= 50
            s[3, :3] = rng.integers(-3, 4, 3)  # lattice directions: ties with the tables are possible
        scans.append(s)
        a = rng.uniform(-np.pi, np.pi)
        T[f] = np.eye(4)
        T[f, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[f, :3, 3] = rng.uniform(-2, 2, 3) * [1, 1, 0.2]
    Tl = None if seed % 2 else np.float32([[1, 0, 0, 0.3], [0, 1, 0, -0.1], [0, 0, 1, 1.7], [0, 0, 0, 1]])
    kw = dict(min_range=float(rng.uniform(0, 2)), max_range=float(rng.uniform(6, 14)), margin_abs=float(rng.uniform(0, 0.6)),
              margin_rel=float(rng.choice([0.0, 0.03])), window=int(rng.integers(0, 3)), k=int(rng.choice([0, 0, 3, 8])), min_cos=float(rng.uniform(0, 0.9)),
              min_through=int(rng.integers(0, 3)), hit_weight=float(rng.choice([0.0, 0.5, 1.0, 2.0])))
    return cloud, scans, T, Tl, grid, kw


@pytest.mark.parametrize("seed", range(24))
def test_the_vectorised_text_equals_the_point_by_point_one(seed):
    cloud, scans, T, Tl, grid, kw = random_case(seed)
    a = evalmap.visibility(cloud, scans, T, Tl, grid, **kw)
    b = evalmap.visibility_brute(cloud, scans, T, Tl, grid, **kw)
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert a[3] == b[3] and a[4] == b[4]
    assert tuple(a[4].keys()) == evalmap.VISIBILITY_RESULT_FIELDS and all(tuple(r.keys()) == evalmap.VISIBILITY_ROW_FIELDS for r in a[3])
    votes, mask, kept, rows, res = a
    assert votes.dtype == np.uint16 and votes.shape == (len(cloud), 4) and mask.dtype == np.uint8 and kept.tobytes() == cloud[mask == 1].tobytes()
    assert (votes[:, 0] >= votes[:, 1] + votes[:, 2] + votes[:, 3]).all() and res["n_in_view"] == int(votes[:, 0].sum())
    assert res["n_in_view"] == res["n_hit"] + res["n_occluded"] + res["n_no_return"] + res["n_through"] + res["n_grazing"]
    assert res["n_kept"] + res["n_removed"] == len(cloud) and res["n_removed"] == res["n_removed_dynamic"] + res["n_removed_static"]
    for r in rows:
        assert r["n_pixels"] <= r["n_points"] - r["n_non_finite"] - r["n_on_axis"] - r["n_out_of_range"] - r["n_out_of_view"]
    if kw["k"] == 0:
        assert res["n_grazing"] == 0 and res["n_map_no_normal"] == 0


def round_the_circle(R):
    """every lattice direction (x, y) != 0 with |x|, |y| <= R, counter-clockwise from +x, by exact integer comparisons"""
    half = lambda p: 0 if (p[1] > 0 or (p[1] == 0 and p[0] > 0)) else 1
    def cmp(p, q):
        if half(p) != half(q):
            return half(p) - half(q)
        c = p[0] * q[1] - p[1] * q[0]
        return -1 if c > 0 else (1 if c < 0 else 0)
    return sorted([(x, y) for x in range(-R, R + 1) for y in range(-R, R + 1) if (x, y) != (0, 0)], key=functools.cmp_to_key(cmp))


@pytest.mark.parametrize("width,col_tan", [(8, []), (16, [0.5]), (32, [0.25, 0.5, 0.75]), (40, [0.125, 0.3125, 0.5, 0.8125])])
def test_the_columns_follow_each_other_once_round_the_circle(width, col_tan):
    dirs = round_the_circle(16)
    col = evalmap.visibility_column(np.float64([d[0] for d in dirs]), np.float64([d[1] for d in dirs]), np.float64(col_tan), width)
    assert col[0] == 0 and (np.diff(col) >= 0).all() and (np.diff(col) <= 1).all()  # never back, never a column skipped
    assert sorted(set(col.tolist())) == list(range(width))                           # all W of them, each one run of directions
    # the same column for every length of a direction and for both signs of a zero
    for s in (0.5, 3.0):
        again = evalmap.visibility_column(np.float64([s * d[0] for d in dirs]), np.float64([s * d[1] for d in dirs]), np.float64(col_tan), width)
        assert (again == col).all()
    neg = lambda v: -0.0 if v == 0 else float(v)
    again = evalmap.visibility_column(np.float64([neg(d[0]) for d in dirs]), np.float64([neg(d[1]) for d in dirs]), np.float64(col_tan), width)
    assert (again == col).all()
    # against the rule in exact arithmetic: a direction on an inner edge (its ratio equal to a table entry) starts the next column in an
    # octant that runs outward from an axis and ends the previous one in a mirrored octant
    M = width // 8
    for (x, y), c in zip(dirs, col.tolist()):
        a, b = abs(x), abs(y)
        t = Fraction(min(a, b), max(a, b))
        j = sum(1 for e in col_tan if Fraction(e) <= t)
        q = (2 if y < 0 else 1) if x < 0 else (3 if y < 0 else 0)
        odd = (a >= b) if q & 1 else (a < b)
        assert c == (2 * q + odd) * M + ((M - 1 - j) if odd else j), (x, y)
    assert evalmap.visibility_column(np.float64([0.0, -0.0]), np.float64([-0.0, 0.0]), np.float64(col_tan), width).tolist() == [-1, -1]


def test_the_uniform_grid_and_its_checks():
    g = evalmap.visibility_grid(64, 16, -24.8, 2.0)
    assert g["col_tan"].shape == (7,) and g["row_tan"].shape == (17,) and (np.diff(g["col_tan"]) > 0).all() and (np.diff(g["row_tan"]) > 0).all()
    assert 0 < g["col_tan"][0] and g["col_tan"][-1] < 1 and abs(g["col_tan"][3] - np.tan(np.pi / 8)) < 1e-15
    assert abs(g["row_tan"][0] - np.tan(np.radians(-24.8))) < 1e-15 and abs(g["row_tan"][-1] - np.tan(np.radians(2.0))) < 1e-15
    assert evalmap.visibility_grid(8, 1, -1, 1)["col_tan"].shape == (0,)
    for W, H in ((0, 1), (12, 1), (4104, 1), (8, 0), (8, 257)):
        with pytest.raises(ValueError):
            evalmap.visibility_grid(W, H, -10, 10)
    with pytest.raises(ValueError):
        evalmap.visibility_grid(8, 4, 10, -10)
    for bad in (dict(col_tan=[0.5, 0.5, 0.7]), dict(col_tan=[0.0, 0.5, 0.7]), dict(col_tan=[0.2, 0.5, 1.0]), dict(col_tan=[0.2, 0.5]),
                dict(row_tan=[0, 0, 1]), dict(row_tan=[0, 1, np.inf]), dict(row_tan=[0, 1])):
        with pytest.raises(ValueError):
            evalmap.check_visibility_grid(dict({"width": 32, "height": 2, "col_tan": [0.25, 0.5, 0.75], "row_tan": [-1, 0, 1]}, **bad))


def test_the_frame_transforms_are_the_rigid_inverse_summed_in_index_order():
    rng = np.random.default_rng(5)
    T = np.zeros((6, 4, 4), np.float32)
    for f in range(6):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T[f, :3, :3], T[f, :3, 3], T[f, 3, 3] = q, rng.uniform(-50, 50, 3), 1
    Tl = np.float32([[0, -1, 0, 0.3], [1, 0, 0, -0.1], [0, 0, 1, 1.7], [0, 0, 0, 1]])
    m, org = evalmap.visibility_transforms(T, Tl)
    for f in range(6):
        M = T[f].astype(np.float64) @ Tl.astype(np.float64)
        assert np.allclose(m[f].reshape(3, 4), np.linalg.inv(M)[:3], atol=1e-5) and np.allclose(org[f], M[:3, 3], atol=1e-12)
        # the sums as the text orders them
        A, B = T[f].astype(np.float64), Tl.astype(np.float64)
        M01 = (A[0, 0] * B[0, 1] + A[0, 1] * B[1, 1]) + A[0, 2] * B[2, 1]
        M03 = ((A[0, 0] * B[0, 3] + A[0, 1] * B[1, 3]) + A[0, 2] * B[2, 3]) + A[0, 3]
        assert m[f, 4] == M01 and org[f, 0] == M03
    m1, org1 = evalmap.visibility_transforms(T)
    assert (org1 == T[:, :3, 3].astype(np.float64)).all()
    bad = T.copy()
    bad[2, 1, 1] = np.inf
    with pytest.raises(ValueError):
        evalmap.visibility_transforms(bad)


def test_the_decision_rule_at_its_edges():
    votes = np.uint16([[9, 0, 0, 0], [9, 0, 1, 0], [9, 0, 2, 0], [9, 2, 2, 0], [9, 1, 2, 0], [9, 2, 3, 0], [9, 65535, 65535, 0], [9, 0, 65535, 0]])
    assert evalmap.visibility_decide(votes, 2, 1.0).tolist() == [False, False, True, False, True, True, False, True]
    assert evalmap.visibility_decide(votes, 3, 1.0).tolist() == [False, False, False, False, False, True, False, True]
    assert evalmap.visibility_decide(votes, 0, 0.0).tolist() == [False, True, True, True, True, True, True, True]  # through > 0 still
    assert evalmap.visibility_decide(votes, 2, 1.5).tolist() == [False, False, True, False, True, False, False, True]  # 3 > 1.5 * 2 is false
    assert evalmap.visibility_decide(votes, 2, float(np.nextafter(1.5, 0))).tolist() == [False, False, True, False, True, True, False, True]
    for kw in (dict(window=3), dict(k=1), dict(k=33), dict(min_range=5.0, max_range=5.0), dict(margin_abs=-1.0), dict(margin_rel=np.nan), dict(hit_weight=-1.0),
               dict(min_cos=np.inf)):
        with pytest.raises(ValueError):
            evalmap.visibility(xyzi([(1, 2, 3)]), [], np.zeros((0, 4, 4)), None, evalmap.visibility_grid(8, 1, -10, 10), **kw)
    with pytest.raises(ValueError):
        evalmap.visibility(xyzi([(1, 2, 3)]), [np.zeros((0, 4))] * 65536, np.zeros((65536, 4, 4)), None, evalmap.visibility_grid(8, 1, -10, 10))
