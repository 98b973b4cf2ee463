"""The normative host text of the free-space carving (evalmap.carve) against its scalar pure-Python restatement (carve_brute) on random
small scenes, and the traversal itself (carve_walk): on thousands of random float32 rays at four voxel sizes consecutive voxels are
face-adjacent, the list has N + 1 entries and ends in the end's cell, and every voxel touches the segment (a slab test with 1e-9 of slack,
which belongs to this test's own geometry, not to the product); the known walks, the tie rule among them.  No GPU."""
import numpy as np
import pytest

from erasor_amd import evalmap

EYE = np.eye(4, dtype=np.float32)


def assert_same(got, want, what):
    for j, (name, dt) in enumerate((("votes", np.uint16), ("logodds", np.float32), ("mask", np.uint8), ("kept", np.float32))):
        g, w = got[j], want[j]
        assert g.dtype == dt and w.dtype == dt and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)
    assert got[4] == want[4] and got[5] == want[5], (what, got[5], want[5])
    assert tuple(got[5].keys()) == evalmap.CARVE_RESULT_FIELDS and all(tuple(r.keys()) == evalmap.CARVE_ROW_FIELDS for r in got[4])


@pytest.mark.parametrize("seed", range(8))
def test_carve_equals_its_scalar_restatement_on_random_small_scenes(seed):
    rng = np.random.default_rng(seed)
    n = [0, 1, 40, 200, 300, 120, 257, 64][seed]
    m = np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.integers(248, 263, (n, 1))], 1).astype(np.float32)
    if n > 10:
        m[3, seed % 3] = [np.nan, np.inf, -np.inf][seed % 3]
        m[7] = m[8]  # two points in one voxel
    n_f = [1, 2, 3, 5, 0, 4, 3, 6][seed]
    scans = [rng.uniform(-4, 4, (int(rng.integers(0, 50)), 4)).astype(np.float32) for _ in range(n_f)]
    for s in scans[:1]:
        if len(s) > 2:
            s[0, 0], s[1, :3] = np.nan, 0.01  # a non-finite point and one below min_range
    T = np.stack([EYE] * n_f).copy() if n_f else np.zeros((0, 4, 4), np.float32)
    for f in range(n_f):
        a = 0.4 * f
        T[f, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[f, :3, 3] = rng.uniform(-1, 1, 3)
    Tl = None if seed % 2 else np.float32([[1, 0, 0, 0.3], [0, 1, 0, -0.1], [0, 0, 1, 0.7], [0, 0, 0, 1]])
    kw = dict(voxel=[0.2, 0.1, 0.25, 1.0][seed % 4], min_range=0.5, max_range=5.0, stop_short=seed % 3)
    lg = None if seed % 3 else dict(l_init=0.25, l_hit=0.5, l_miss=-0.75, l_min=-1.0, l_max=1.0, l_thr=-0.25)
    a = evalmap.carve(m, scans, T, Tl, logodds=lg, **kw)
    assert_same(evalmap.carve_brute(m, scans, T, Tl, logodds=lg, **kw), a, seed)
    res = a[5]
    assert res["n_points"] == n and res["n_kept"] + res["n_removed"] == n and res["n_removed_dynamic"] + res["n_removed_static"] == res["n_removed"]
    assert res["n_scan_points"] == sum(len(s) for s in scans) == res["n_non_finite"] + res["n_out_of_range"] + res["n_rays"]
    assert a[3].tobytes() == m[a[2] == 1].tobytes()
    assert evalmap.carve(m, scans, T, Tl, logodds=lg, keep=False, **kw)[3] is None


@pytest.mark.parametrize("voxel", [0.2, 0.1, 0.25, 1.0])
def test_three_thousand_random_rays_walk_face_to_face_along_their_segment(voxel):
    rng = np.random.default_rng(int(voxel * 100))
    o = rng.uniform(-20, 20, (3000, 3)).astype(np.float32).astype(np.float64)
    e = (o + rng.normal(0, 1, (3000, 3)) * rng.uniform(0.01, 12, (3000, 1))).astype(np.float32).astype(np.float64)
    e[::50, 1] = o[::50, 1]  # rays in an axis plane
    e[::75, 1:] = o[::75, 1:]  # and along an axis
    n_voxels = 0
    for a, b in zip(o, e):
        w = evalmap.carve_walk(a, b, voxel)
        c0, c1 = np.floor(a / voxel).astype(np.int64), np.floor(b / voxel).astype(np.int64)
        assert len(w) == np.abs(c1 - c0).sum() + 1 and (w[0] == c0).all() and (w[-1] == c1).all()
        assert (np.abs(np.diff(w, axis=0)).sum(1) == 1).all()
        # the slab test: the segment's parameter interval inside each voxel's box, grown by the slack, is not empty
        lo, hi = w * voxel - 1e-9, (w + 1) * voxel + 1e-9
        d = b - a
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - a) / d, (hi - a) / d
        par = d == 0
        inside = (a >= lo) & (a <= hi)
        assert inside[:, par].all()
        tn = np.where(par, -np.inf, np.minimum(t0, t1)).max(1)
        tf = np.where(par, np.inf, np.maximum(t0, t1)).min(1)
        assert (np.maximum(tn, 0.0) <= np.minimum(tf, 1.0)).all(), (a, b)
        n_voxels += len(w)
    assert n_voxels > 3000


def test_the_known_walks():
    w = evalmap.carve_walk((0.5, 0.5, 0.5), (2.5, 2.5, 2.5), 1.0)
    assert w.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1], [2, 1, 1], [2, 2, 1], [2, 2, 2]]  # ties: x before y before z
    w = evalmap.carve_walk((0.5, 0.5, 0.5), (-1.5, 2.5, 0.5), 1.0)
    assert w.tolist() == [[0, 0, 0], [-1, 0, 0], [-1, 1, 0], [-2, 1, 0], [-2, 2, 0]]
    w = evalmap.carve_walk((0.1, 0.1, 0.1), (0.7, 0.1, 0.1), 0.2)
    assert w[-1].tolist() == [3, 0, 0] and len(w) == 4
    assert evalmap.carve_walk((0.3, 0.3, 0.3), (0.4, 0.35, 0.3), 1.0).tolist() == [[0, 0, 0]]  # N = 0


def test_the_default_log_odds_and_the_refusals():
    lg = evalmap.carve_logodds()
    assert tuple(lg.keys()) == evalmap.CARVE_LOGODDS_FIELDS and lg["l_init"] == 0.0 and lg["l_thr"] == 0.0
    assert lg["l_hit"] == float(np.float32(np.log(0.7 / 0.3))) and lg["l_miss"] == float(np.float32(np.log(0.4 / 0.6)))
    assert lg["l_min"] < lg["l_miss"] < 0 < lg["l_hit"] < lg["l_max"]
    m, s = np.zeros((3, 4), np.float32), [np.ones((2, 4), np.float32)]
    for kw in (dict(voxel=0.0), dict(voxel=np.nan), dict(min_range=5.0, max_range=5.0), dict(min_range=-1.0), dict(voxel=0.01, max_range=80.0),
               dict(stop_short=65), dict(stop_short=-1), dict(logodds=dict(lg, l_hit=-0.1)), dict(logodds=dict(lg, l_miss=0.1)),
               dict(logodds=dict(lg, l_init=9.0)), dict(logodds=dict(lg, l_thr=np.nan))):
        with pytest.raises(ValueError):
            evalmap.carve(m, s, EYE[None], None, **kw)
    far = m.copy()
    far[1, 2] = 0.2 * 2.0 ** 28
    with pytest.raises(ValueError):
        evalmap.carve(far, s, EYE[None])
    T = EYE[None].copy()
    T[0, 0, 3] = -0.2 * 2.0 ** 28 - 1
    with pytest.raises(ValueError):
        evalmap.carve(m, s, T)
    T[0, 0, 3] = np.inf
    with pytest.raises(ValueError):
        evalmap.carve(m, s, T)
    evalmap.carve(m, s, EYE[None], None, voxel=80.0 / 4096, max_range=80.0)  # exactly 4096 cells is fine
