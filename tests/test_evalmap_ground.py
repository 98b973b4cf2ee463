"""The normative host text of the ground (evalmap.ground_scans / ground_votes) against its pure-Python restatements (*_brute) on random
small scenes, and the known answers that do not rest on either: a dyadic lattice on z = -1.75 under a box (normal exactly (0, 0, 1),
d = 1.75), a wall alone in a patch, the patch mapping at its edges, the seeds' order, the sum's chunk rule, the decision and the grid's
refusals.  No GPU."""
import itertools

import numpy as np
import pytest

from erasor_amd import evalmap

EYE = np.eye(4, dtype=np.float32)
G1 = evalmap.ground_grid(1, 8, 0.5, 64.0)


def same_scans(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2] == b[2] and a[3].tobytes() == b[3].tobytes()


def scene(seed, n):
    """a noisy floor 1.75 m below the sensor with boxes, walls and labelled points on it"""
    rng = np.random.default_rng(seed)
    r, az = 30.0 * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(-np.pi, np.pi, n)
    z = -1.75 + rng.normal(0, 0.03, n) + 0.02 * r * np.cos(az)
    z[::6] += rng.uniform(0.2, 2.0, len(z[::6]))
    s = np.stack([r * np.cos(az), r * np.sin(az), z, rng.choice([40.0, 252.0, 255.0, 72.0], n)], 1).astype(np.float32)
    if n > 10:
        s[3, seed % 3] = [np.nan, np.inf, -np.inf][seed % 3]
        s[5, :2] = 0.0
    return s


@pytest.mark.parametrize("seed", range(6))
def test_ground_scans_equals_its_scalar_restatement_on_random_small_scenes(seed):
    sizes = [[0], [1, 40], [300, 0, 520], [257, 256, 255], [700], [64, 65, 63, 10, 9]][seed]
    scans = [scene(10 * seed + k, n) for k, n in enumerate(sizes)]
    grid = [None, evalmap.ground_grid(3, 8, 0.5, 40.0), evalmap.ground_grid(2, 16, 1.0, 35.0), G1, evalmap.ground_grid(5, 24, 0.0, 30.0),
            {"n_sectors": 8, "col_tan": [], "ring_edge": [0.0, 2.7, 12.3, 44.2, 74.0]}][seed]
    kw = [dict(), dict(num_lpr=1, iters=1), dict(th_seeds=0.2, th_dist=0.05, min_points=3), dict(num_lpr=64, iters=16), dict(min_z=-1.8, uprightness=0.99),
          dict(elevation=[-1.0, -1.7, -1.8, -1.9], flatness=[0.0, 1e-4, 1e-3, 1.0])][seed]
    a = evalmap.ground_scans(scans, grid, patches=True, **kw)
    assert same_scans(a, evalmap.ground_scans_brute(scans, grid, patches=True, **kw))
    assert a[0].dtype == np.uint8 and len(a[0]) == sum(sizes) and a[2]["n_frames"] == len(scans)
    assert all(tuple(r.keys()) == evalmap.GROUND_ROW_FIELDS for r in a[1]) and evalmap.ground_scans(scans, grid, **kw)[3] is None
    for f, (s, r) in enumerate(zip(scans, a[1])):
        c = a[0][sum(sizes[:f]):sum(sizes[:f + 1])]
        assert r["n_points"] == len(s) and r["n_non_finite"] == int((c == 255).sum()) and r["n_ground"] == int((c == 1).sum())
        assert r["n_judged"] == int((c <= 1).sum()) and r["n_ground"] == int(a[3]["n_ground"][f].sum())
        st = a[3]["status"][f]
        assert r["n_patches"] == int((st != 0).sum()) and r["n_sparse"] == int((st == 2).sum()) and r["n_degenerate"] == int((st == 3).sum())
        assert int(a[3]["n_points"][f].sum()) == len(s) - r["n_non_finite"] - r["n_out_of_range"]


@pytest.mark.parametrize("seed", range(4))
def test_ground_votes_equals_its_scalar_restatement_and_the_scans_of_the_gathered_clouds(seed):
    m = scene(100 + seed, [0, 60, 400, 300][seed])
    m[:, 2] += 1.75
    n_f = [2, 3, 4, 0][seed]
    T = np.stack([EYE] * n_f).copy() if n_f else np.zeros((0, 4, 4), np.float32)
    for f in range(n_f):
        a = 0.4 * f
        T[f, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[f, :3, 3] = (0.5 * f, -0.25 * f, 1.5)
    Tl = None if seed % 2 else np.float32([[1, 0, 0, 0.3], [0, 1, 0, -0.1], [0, 0, 1, 0.25], [0, 0, 0, 1]])
    grid = evalmap.ground_grid(3, 8, 0.5, 40.0)
    kw = dict(min_votes=1 + seed % 2, ratio=[0.5, 0.0, 0.75, 0.5][seed], keep=seed % 2)
    a = evalmap.ground_votes(m, T, Tl, grid, **kw)
    b = evalmap.ground_votes_brute(m, T, Tl, grid, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and a[4] == b[4]
    assert a[0].dtype == np.uint16 and a[0].shape == (len(m), 2) and tuple(a[4].keys()) == evalmap.GROUND_VOTES_RESULT_FIELDS
    clouds, idx = evalmap.ground_gather(m, T, Tl, grid)
    codes = evalmap.ground_scans(clouds, grid)[0]
    votes, o = np.zeros((len(m), 2), np.uint16), 0
    for ix in idx:
        c = codes[o:o + len(ix)]
        o += len(ix)
        votes[ix[c <= 1], 0] += 1
        votes[ix[c == 1], 1] += 1
    gr = evalmap.ground_decide(votes, kw["min_votes"], kw["ratio"])
    assert votes.tobytes() == a[0].tobytes() and gr.astype(np.uint8).tobytes() == a[1].tobytes()
    assert a[2].tobytes() == m[gr if kw["keep"] else ~gr].tobytes() and a[4]["n_unseen"] == int((votes[:, 0] == 0).sum())
    assert (votes[:, 1] <= votes[:, 0]).all() and (votes[:, 0] <= n_f).all()


def lattice():
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    x, y = 4.0 + i.reshape(-1) / 4.0, 0.125 + j.reshape(-1) / 8.0
    bx, by, bz = (v.reshape(-1) for v in np.meshgrid(6.0 + np.arange(3) / 4.0, 1.0 + np.arange(3) / 4.0, np.arange(3) / 4.0, indexing="ij"))
    p = np.concatenate([np.stack([x, y, np.full(256, -1.75)], 1), np.stack([bx, by, -1.25 + bz], 1)])
    return np.concatenate([p, np.full((len(p), 1), 40.0)], 1).astype(np.float32)


def test_a_dyadic_lattice_under_a_box_and_a_wall():
    s = lattice()
    for fn in (evalmap.ground_scans, evalmap.ground_scans_brute):
        codes, rows, res, tab = fn([s], G1, patches=True)
        row = tab[0, 0, 0]
        assert row["status"] == evalmap.GROUND_OK and row["normal"].tolist() == [0.0, 0.0, 1.0] and row["d"] == 1.75 and row["n_ground"] == 256
        assert (codes[:256] == 1).all() and (codes[256:] == 0).all() and rows[0]["n_judged"] == len(s)
    y, z = np.meshgrid(1.0 + np.arange(12) / 8.0, -1.75 + np.arange(12) / 4.0, indexing="ij")
    wall = np.stack([np.full(144, 10.0), y.reshape(-1), z.reshape(-1), np.full(144, 40.0)], 1).astype(np.float32)
    codes, rows, res, tab = evalmap.ground_scans([wall], G1, patches=True)
    assert tab[0, 0, 0]["status"] == evalmap.GROUND_REJECTED_UPRIGHT and (codes == 0).all() and rows[0]["n_rejected_upright"] == 1


def test_the_patch_mapping_at_its_edges():
    grid = evalmap.ground_grid(3, 16, 1.0, 4.0)
    assert grid["ring_edge"].tolist() == [1.0, 2.0, 3.0, 4.0] and len(grid["col_tan"]) == 1
    f = lambda x, y: tuple(int(v[0]) for v in evalmap.ground_patch_of([x], [y], grid))
    below = float(np.nextafter(np.float32(1.0), np.float32(0)))
    assert f(1.0, 0.0) == (0, 0) and f(below, 0.0)[0] == -1 and f(4.0, 0.0)[0] == -1 and f(float(np.nextafter(np.float32(4.0), np.float32(0))), 0.0) == (2, 0)
    assert f(0.0, 0.0)[0] == -1 and f(-0.0, 0.0)[0] == -1
    assert f(2.0, 0.0) == (1, 0) and f(0.0, 2.0) == (1, 3) and f(-2.0, 0.0) == (1, 7) and f(0.0, -2.0) == (1, 12)
    assert f(2.0, -1e-30) == (1, 15) and f(2.0, 2.0) == (1, 1) and f(-2.0, 2.0) == (1, 6)  # (an edge belongs to exactly one sector)
    secs = {f(2.5 * np.cos(a), 2.5 * np.sin(a))[1] for a in (np.arange(16) + 0.5) * (np.pi / 8)}
    assert secs == set(range(16))


def test_the_seeds_do_not_depend_on_the_order_of_equal_heights_and_the_sum_follows_the_chunk_rule():
    prm = evalmap._ground_args(G1, 3, 0.5, 0.15, 1, 6, -3.03, 0.0, None, None, 1)[2]
    base = np.float64([[4, 1, -1.75], [5, 2, -1.75], [6, 1, -0.0], [7, 3, 0.0], [8, 2, -1.75], [9, 4, -1.5]])
    got = set()
    for p in itertools.permutations(range(6)):
        st, mem, plane = evalmap.ground_fit(base[list(p)], 0, prm)
        st2, mem2, plane2 = evalmap.ground_fit_brute(base[list(p)], 0, prm)
        assert st == st2 and (mem == mem2).all() and plane == plane2
        got.add((st, frozenset(p[i] for i in np.flatnonzero(mem))))  # (position i of the permuted patch holds point p[i])
    assert len(got) == 1  # the same points are ground whatever their order
    # the sum: a halving tree inside a chunk of 256, the chunks one after another -- not the sum from left to right
    assert evalmap._tree_sum_brute([1e16, 1.0, -1e16, 1.0]) == 2.0 and ((1e16 + 1.0) + -1e16) + 1.0 == 1.0
    v = [0.0] * 258
    v[0], v[256], v[257] = 1e16, 1.0, -1e16
    assert evalmap._tree_sum_brute(v) == 0.0 and evalmap._tree_sum_brute(v[:257]) == 1e16
    r = np.random.default_rng(1).normal(0, 1, 600)
    assert evalmap._tree_sum_brute(r.tolist()) == float(evalmap.refine_tree_sum(r.reshape(-1, 1))[0])


def test_the_decision_at_its_exact_ends():
    votes = np.uint16([[0, 0], [4, 2], [4, 3], [3, 3], [5, 1]])
    assert evalmap.ground_decide(votes, 1, 0.5).tolist() == [False, False, True, True, False]  # strictly more than ratio * seen
    assert evalmap.ground_decide(votes, 3, 0.5).tolist() == [False, False, True, True, False]
    assert evalmap.ground_decide(votes, 4, 0.0).tolist() == [False] * 5 and evalmap.ground_decide(votes, 0, -1.0).tolist() == [False, True, True, True, True]
    assert evalmap.ground_decide(votes, 1, 0.0).tolist() == [False, True, True, True, True]


def test_the_grid_and_the_parameters_are_checked():
    g = evalmap.ground_grid()
    assert g["n_sectors"] == 64 and len(g["ring_edge"]) == 21 and len(g["col_tan"]) == 7 and g["ring_edge"][0] == 0.5 and g["ring_edge"][-1] == 80.0
    assert g["col_tan"].tobytes() == evalmap.visibility_grid(64, 1, -1.0, 1.0)["col_tan"].tobytes()
    for bad in (dict(n_rings=0), dict(n_rings=65), dict(n_sectors=12), dict(n_sectors=520), dict(min_range=-1.0), dict(min_range=5.0, max_range=5.0)):
        with pytest.raises(ValueError):
            evalmap.ground_grid(**bad)
    for bad in (dict(g, ring_edge=[1.0]), dict(g, ring_edge=[2.0, 1.0]), dict(g, ring_edge=[0.0, np.inf]), dict(g, col_tan=g["col_tan"][:3]),
                dict(g, col_tan=g["col_tan"][::-1]), dict(g, n_sectors=8)):
        with pytest.raises(ValueError):
            evalmap.check_ground_grid(bad)
    s = [lattice()]
    for bad in (dict(num_lpr=0), dict(num_lpr=65), dict(iters=0), dict(iters=17), dict(min_points=2), dict(th_seeds=np.nan), dict(th_dist=np.inf),
                dict(min_z=np.nan), dict(uprightness=np.inf), dict(elevation=[0.0, 1.0]), dict(flatness=[np.nan])):
        with pytest.raises(ValueError):
            evalmap.ground_scans(s, G1, **bad)
    with pytest.raises(ValueError):
        evalmap.ground_votes(s[0], np.stack([EYE]), None, G1, ratio=np.nan)
    assert evalmap.GROUND_PATCH_DTYPE.itemsize == 80 and evalmap.GROUND_DEFAULTS["min_z"] == -3.03
