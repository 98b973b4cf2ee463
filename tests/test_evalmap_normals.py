"""evalmap.normals, the host restatement of Erasor.normals, without a GPU: the numpy version equals the pure-Python normals_brute byte
for byte on small designed clouds; lattices in the axis planes have their known answers; and the Jacobi solve (_jacobi3, and its
all-rows-at-once form) agrees with numpy.linalg.eigh on twenty thousand random neighbourhoods wherever the smallest eigenvalue is
separated from the next."""
import numpy as np
import pytest

from erasor_amd import evalmap


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([xyz, np.full((len(xyz), 1), w, np.float32)], 1))


def same(a, b):
    assert a[3].keys() == b[3].keys() and repr(a[3]) == repr(b[3]), (a[3], b[3])
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def designed_clouds():
    rng = np.random.default_rng(1)
    blob = rng.uniform(-4, 4, (150, 3)) * [1, 1, 0.1]
    blob[::9] = np.round(blob[::9])
    u, v = (a.ravel() for a in np.meshgrid(np.arange(5) * 0.2, np.arange(4) * 0.2, indexing="ij"))
    lattice = np.stack([u - 0.3, v + 2.1, np.full(20, 1.7)], 1)
    line = np.stack([np.arange(40) * 0.25 - 3.0, np.full(40, 1.5), np.full(40, -2.0)], 1)
    copies = np.concatenate([blob[:60], np.tile([[1.5, -2.25, 0.125]], (40, 1))])[rng.permutation(100)]
    axes = np.float64([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) + [16.0, 32.0, 48.0]
    zeros = lattice.copy()
    zeros[:, 2] = 0.0
    zeros[::2, 2] = -0.0
    far = blob + 1e5
    return {"blob": blob, "lattice": lattice, "line": line, "copies": copies, "ties": axes, "signed zeros": zeros, "far": far, "few": blob[:5]}


@pytest.mark.parametrize("name", list(designed_clouds()))
def test_the_numpy_version_equals_the_pure_python_one_byte_for_byte(name):
    cloud = xyzi(designed_clouds()[name])
    for k in (2, 3, 8, 17, 32):
        for vp in (None, (0.5, -1.0, 30.0), (1e5, 1e5, 0.0)):
            same(evalmap.normals(cloud, k, vp), evalmap.normals_brute(cloud, k, vp))


def test_short_degenerate_and_ambiguous_points_are_counted():
    d = designed_clouds()
    n, c, e, r = evalmap.normals(xyzi(d["few"]), 8)
    assert r["n_short"] == 5 and np.isnan(n).all() and np.isnan(c).all() and np.isnan(e).all() and r["curvature_stats"]["n_scored"] == 0
    n, c, e, r = evalmap.normals(xyzi(np.tile([[1.0, 2.0, 3.0]], (30, 1))), 4)
    assert r["n_degenerate"] == 30 and r["n_short"] == 0 and np.isnan(n).all() and n.dtype == np.float32
    n, c, e, r = evalmap.normals(xyzi(d["line"]), 8)
    assert r["n_ambiguous"] == 40 and (n == np.float32([0, 1, 0])).all() and (c == 0).all() and (e[:, :2] == 0).all()
    for k in (0, 1, 33, 2.0):
        with pytest.raises(ValueError):
            evalmap.normals(xyzi(d["blob"]), k)
    for vp in ((0, 0), (0, 0, float("nan")), (float("inf"), 0, 0)):
        with pytest.raises(ValueError):
            evalmap.normals(xyzi(d["blob"]), 8, vp)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_lattice_in_an_axis_plane_has_the_axis_as_its_normal_exactly(axis):
    u, v = (a.ravel() for a in np.meshgrid(np.arange(6) * 0.2, np.arange(7) * 0.2, indexing="ij"))
    xyz = np.zeros((42, 3), np.float32)
    xyz[:, (axis + 1) % 3], xyz[:, (axis + 2) % 3], xyz[:, axis] = u - 0.3, v + 2.1, np.float32(1.7)
    for k in (8, 16, 32):
        for fn in (evalmap.normals, evalmap.normals_brute):
            n, c, e, r = fn(xyzi(xyz), k)
            want = np.zeros(3, np.float32)
            want[axis] = 1.0
            assert (n == want).all() and not np.signbit(n).any() and (c == 0).all() and (e[:, 0] == 0).all() and (e[:, 1] > 0).all()
            assert r["n_ambiguous"] == 0 and r["n_flipped"] == 0
        below = [0.0, 0.0, 0.0]
        below[axis] = -5.0
        n, c, e, r = evalmap.normals(xyzi(xyz), k, below)
        assert (n == -want).all() and r["n_flipped"] == 42


# ---- the solve against numpy.linalg.eigh ----
N_DRAWS = 20000


def random_neighbourhoods():
    """per m = 3 .. 33: float32 neighbourhoods of m points -- generic, flat (one extent exactly or nearly 0), thin, needle-shaped (two
    small extents) and far from the origin, each turned by a random rotation"""
    rng = np.random.default_rng(20240607)
    per_m = -(-N_DRAWS // 31)
    out = []
    for m in range(3, 34):
        p = rng.normal(size=(per_m, m, 3))
        kind = rng.integers(0, 5, per_m)
        scale = np.ones((per_m, 3))
        scale[kind == 1, 2] = rng.choice([0.0, 1e-6, 1e-3], (kind == 1).sum())   # flat
        scale[kind == 2, 2] = 10.0 ** rng.uniform(-3, -0.5, (kind == 2).sum())   # thin
        scale[kind == 3, 1] = 10.0 ** rng.uniform(-2.5, -0.3, (kind == 3).sum())  # needle
        scale[kind == 3, 2] = scale[kind == 3, 1] * rng.uniform(0.05, 1.0, (kind == 3).sum())
        p = p * scale[:, None, :] * rng.uniform(0.05, 2.0, (per_m, 1, 1))
        q, _ = np.linalg.qr(rng.normal(size=(per_m, 3, 3)))
        p = np.einsum("nmj,nij->nmi", p, q)
        p[kind == 4] += rng.choice([1e3, 1e4, -1e5], ((kind == 4).sum(), 1, 3))  # far-offset
        out.append(p.astype(np.float32).astype(np.float64))
    return out


def covariances(p):
    """the contract's covariance of every neighbourhood in p (cnt, m, 3), in list order: [xx, xy, xz, yy, yz, zz]"""
    cnt, m, _ = p.shape
    s = np.zeros((cnt, 3))
    for j in range(m):
        s = s + p[:, j]
    c = s / np.float64(m)
    a = [np.zeros(cnt) for _ in range(6)]
    for j in range(m):
        e = p[:, j] - c
        for t, term in enumerate((e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1], e[:, 1] * e[:, 2], e[:, 2] * e[:, 2])):
            a[t] = a[t] + term
    return np.stack([x / np.float64(m) for x in a], 1)


def test_the_jacobi_solve_against_numpy_eigh_on_twenty_thousand_neighbourhoods():
    """Wherever the gap l1 - l0 >= 1e-3 l2: 1 - |n . n_ref| <= 1e-12 and |l0 - w0| <= 1e-12 w2.  Rounding gives about 1e-15 (over this draw's
    17 972 such cases the worst 1 - |dot| was 1.0e-15 and the worst |l0 - w0| 1.1e-15 w2; every solve ended with its off-diagonals exactly
    zero), so 1e-12 has three orders of margin.  Below the gap the
    smallest eigenvector is ill-conditioned and the two solvers may differ: those cases are left out of this comparison only, and must be
    fewer than 30 % of the draw (here 2 028 of 20 000)."""
    cov = np.concatenate([covariances(p) for p in random_neighbourhoods()])
    cov = cov[(cov[:, 0] + cov[:, 3]) + cov[:, 5] > 0][:N_DRAWS]
    assert len(cov) >= N_DRAWS - 5
    full = cov[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    w, vec = np.linalg.eigh(full)
    l0, nrm = np.zeros(len(cov)), np.zeros((len(cov), 3))
    for i, row in enumerate(cov.tolist()):
        A = [[row[0], row[1], row[2]], [row[1], row[3], row[4]], [row[2], row[4], row[5]]]
        V = evalmap._jacobi3(A)
        assert A[0][1] == 0.0 and A[0][2] == 0.0 and A[1][2] == 0.0  # converged: every off-diagonal exactly zero
        j = min(range(3), key=lambda c: (A[c][c], c))
        l0[i], nrm[i] = A[j][j], (V[0][j], V[1][j], V[2][j])
    # the all-rows-at-once form does the same operations
    a = [cov[:, t].copy() for t in range(6)]
    v = evalmap._jacobi3_rows(a, np.ones(len(cov), bool))
    d = np.stack([a[0], a[3], a[5]], 1)
    first = np.argmin(d, 1)  # (the first of equal minima: the lowest column)
    rows = np.arange(len(cov))
    assert d[rows, first].tobytes() == l0.tobytes()
    assert np.stack([np.stack(v[3 * r:3 * r + 3], 1)[rows, first] for r in range(3)], 1).tobytes() == nrm.tobytes()
    gap = (w[:, 1] - w[:, 0]) >= 1e-3 * w[:, 2]
    assert (~gap).mean() < 0.30 and gap.sum() >= 15000, ((~gap).mean(), gap.sum())
    dot = np.abs(np.einsum("ni,ni->n", nrm, vec[:, :, 0]))
    assert (1.0 - dot[gap]).max() <= 1e-12, (1.0 - dot[gap]).max()
    assert (np.abs(l0 - w[:, 0])[gap] <= 1e-12 * w[gap, 2]).all(), (np.abs(l0 - w[:, 0])[gap] / w[gap, 2]).max()
