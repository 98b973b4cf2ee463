"""The two spatial indexes tested AS INDEXES: the bounding-volume tree of nearest.hip.h (nn_build in analysis_host.hip.h: Morton keys,
the 30-bit radix sort, leaves of 32 points, the per-lane depth-first search) behind overlap, align_frames, label_map and
static_complement, and the hashed uniform grid of evaluate.hip.h (k_ev_hist / k_ev_offsets / k_ev_scatter, and evaluate_many's combined
table) behind evaluate, evaluate_by_class and evaluate_many.

Both are built so that their ANSWER does not depend on the index being any good ("the tree only decides the ORDER of the search", "hash
collisions only add candidates"), so a test that compares answers passes on a broken index that merely turns an O(log n) query into an
O(n) one.  Here the structure itself (1, 2) and the search's effort (3) are compared with plain numpy / Python restatements written in
this file, through the dump hooks of tests/hooks.py; then the public calls run at the structural boundary sizes (4), on adversarial
geometry (5) and where every float32 d^2 overflows (6), against brute force over all pairs.  The references are never the library,
never evalmap.nearest_f32, and cKDTree only for the overlap report's eleven fields (evalmap.overlap / evalmap.align_frames), whose
per-point distances and indices are compared with brute force beside them.  tests/test_spatial_index_on_cpu.py re-runs part of this file against the CPU stand-in."""
import contextlib
import functools
import os

import numpy as np
import pytest

import hooks
from erasor_amd import evalmap, synth
from oracle import orc

pytestmark = pytest.mark.gpu

NN_LEAF, NN_QBLOCK = 32, 256
ON_CPU = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))
REPORT_FIELDS = ("n_est", "n_below_half", "n_below_one", "n_below_two", "median", "p90", "p99", "max", "frac_half", "frac_one", "frac_two")
SEEDS = (11, 12)
N_SKIPPED = [0]  # queries a test left out because brute force could not decide them: asserted to stay 0


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


@contextlib.contextmanager
def hooked(gpu_mod):
    """a handle of the hooks build; closed before the product library is back in place"""
    with hooks.hooks_library():
        g = gpu_mod.Erasor(gpu_mod.params_default())
        try:
            yield g
        finally:
            g.close()


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.float64(a), np.float64(b)
    return a.tobytes() == b.tobytes() or (np.isnan(a) and np.isnan(b))


@functools.lru_cache(maxsize=None)
def world_slice(n, spacing=0.25, seed=20210311):
    """n points of a synthetic street (ground, facades, cars, poles, trails of moving objects), labelled"""
    w = synth.World(seed=seed, length=60.0)
    m = w.sample_map(spacing=spacing, frames=range(0, 20, 4), x_range=(0.0, 30.0))
    assert len(m) >= n, (len(m), n)
    return np.ascontiguousarray(m[np.random.default_rng(n).permutation(len(m))[:n]], np.float32)


def uniform_cloud(n, seed, half=20.0, labels=(40.0, 50.0, 252.0, 70.0)):
    rng = np.random.default_rng(seed)
    return xyzi(rng.uniform(-half, half, (n, 3)), rng.choice(np.asarray(labels, np.float32), n))


# ------------------------------------------------------------------------------------------------------------------------------------
# brute force over all pairs, in the two metrics
# ------------------------------------------------------------------------------------------------------------------------------------
def d2_f64(q, t):
    """(dx*dx + dy*dy) + dz*dz in float64, dx = (double)q.x - (double)t.x: rows of q against all of t"""
    q, t = q.astype(np.float64), t.astype(np.float64)
    with np.errstate(over="ignore"):
        e = [q[:, None, a] - t[None, :, a] for a in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def d2_f32(q, t):
    """FLANN's L2_Simple in float32, operation by operation: r = 0; r += dx*dx; r += dy*dy; r += dz*dz with dx = q.x - t.x"""
    q, t = q.astype(np.float32), t.astype(np.float32)
    with np.errstate(over="ignore"):
        r = np.zeros((len(q), len(t)), np.float32)
        for a in range(3):
            d = q[:, None, a] - t[None, :, a]
            r = r + d * d
        return r


def brute(tree_xyz, q_xyz, metric, key=None):
    """per query: the minimum d^2 over ALL tree points, the smallest tree index at it, and whether the points at the minimum carry more
    than one value of `key`"""
    t = np.ascontiguousarray(tree_xyz, np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(q_xyz, np.float32).reshape(-1, 3)
    n_q = len(q)
    best = np.zeros(n_q, np.float32 if metric is d2_f32 else np.float64)
    idx = np.zeros(n_q, np.int64)
    mixed = np.zeros(n_q, bool)
    step = max(1, 2_000_000 // max(len(t), 1))
    for s in range(0, n_q, step):
        d2 = metric(q[s:s + step], t)
        N_SKIPPED[0] += int(np.isnan(d2).any(1).sum())  # (a NaN d^2 would leave the minimum undecided: finite inputs never give one)
        m = d2.min(1)
        at = d2 == m[:, None]
        i = at.argmax(1)  # (the first True: the smallest index)
        best[s:s + step], idx[s:s + step] = m, i
        if key is not None:
            k = np.asarray(key)
            mixed[s:s + step] = (at & (k[None, :] != k[i][:, None])).any(1)
    return best, idx, mixed


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the tree's structure, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------
def restated_keys(xyz):
    """the 30-bit Morton key of every point over the cloud's bounding box: per axis (v - lo) / ext * 1024 in float64, truncated, clamped to
    [0, 1023], an axis of zero extent giving cell 0; bit b of the x / y / z cell at bit 3b / 3b + 1 / 3b + 2"""
    v = xyz.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = hi - lo
    key = np.zeros(len(v), np.uint32)
    for a in range(3):
        if ext[a] > 0.0:
            t = (v[:, a] - lo[a]) / ext[a] * 1024.0
            t = np.minimum(np.where(t >= 0.0, t, 0.0), 1023.0)
            c = t.astype(np.uint32)
        else:
            c = np.zeros(len(v), np.uint32)
        for b in range(10):
            key |= ((c >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + a)
    return key


def check_tree(cloud, d, what):
    n = len(cloud)
    n_leaves = max(1, -(-n // NN_LEAF))
    P = 1
    while P < n_leaves:
        P *= 2
    assert d["P"] == P, (what, d["P"], P)
    key = restated_keys(cloud[:, :3])
    order = np.argsort(key, kind="stable")
    assert np.array_equal(d["keys"], key[order]), (what, "sorted keys", np.flatnonzero(d["keys"] != key[order])[:5])
    assert np.array_equal(d["idx"], order.astype(np.uint32)), (what, "permutation", np.flatnonzero(d["idx"] != order)[:5])
    assert np.array_equal(bits(d["pts"]), bits(cloud[order])), (what, "gathered points")
    lo, hi = d["lo"], d["hi"]
    assert lo.shape == (2 * P, 4) and hi.shape == (2 * P, 4)
    inf = np.float32(np.inf)
    for leaf in range(P):
        s = cloud[order][leaf * NN_LEAF:(leaf + 1) * NN_LEAF, :3]
        e_lo = s.min(0) if len(s) else np.full(3, inf)
        e_hi = s.max(0) if len(s) else np.full(3, -inf)
        assert np.array_equal(lo[P + leaf, :3], e_lo) and np.array_equal(hi[P + leaf, :3], e_hi), (what, "leaf", leaf, lo[P + leaf], hi[P + leaf])
    for k in range(P - 1, 0, -1):
        assert np.array_equal(lo[k, :3], np.minimum(lo[2 * k, :3], lo[2 * k + 1, :3])), (what, "node", k)
        assert np.array_equal(hi[k, :3], np.maximum(hi[2 * k, :3], hi[2 * k + 1, :3])), (what, "node", k)
    assert (bits(lo[1:, 3]) == 0).all() and (bits(hi[1:, 3]) == 0).all(), (what, "w fields")


def outlier_cloud(n, seed):
    """a box stretched by one outlier: nearly all keys are equal and the stable sort leaves input order"""
    c = uniform_cloud(n, seed, half=5.0)
    c[n // 3, :3] = (1e7, -1e7, 1e7)
    return c


def dup_runs(seed, n_runs=14):
    """runs of 40 to 200 exact duplicates with shuffled indices and different labels inside a run (runs span leaves and buckets), and
    the runs' places"""
    rng = np.random.default_rng(seed)
    place = rng.uniform(-10, 10, (n_runs, 3)).astype(np.float32)
    rows = []
    for r in range(n_runs):
        m = int(rng.integers(40, 201))
        lab = rng.choice(np.array([40.0, 252.0, 50.0, 65536.0 * 3 + 252.0], np.float32), m)
        if r % 3 == 0:
            lab[:] = 40.0  # (a run with one label: never tied)
        rows.append(xyzi(np.repeat(place[r][None], m, 0), lab))
    c = np.concatenate(rows)
    return np.ascontiguousarray(c[rng.permutation(len(c))]), place


def structure_fixtures():
    rng = np.random.default_rng(7)
    fx = [("uniform", uniform_cloud(3000, 1)), ("world", world_slice(3000)), ("planar", xyzi(np.c_[rng.uniform(-9, 9, (700, 2)), np.full(700, 1.5)])),
          ("linear", xyzi(np.c_[np.full(300, -2.0), rng.uniform(0, 50, 300), np.full(300, 0.25)])), ("single", xyzi([[3.0, -4.0, 5.0]])),
          ("identical", xyzi(np.tile([[1.25, -7.5, 0.125]], (100, 1)))), ("outlier", outlier_cloud(1500, 2)), ("dup_runs", dup_runs(3)[0])]
    at_max = uniform_cloud(500, 3, half=4.0)
    at_max[::7, 0], at_max[::5, 1], at_max[::3, 2] = 4.0, 4.0, 4.0  # (t = 1024 exactly: clamped to cell 1023)
    at_max[1, :3] = -4.0
    fx.append(("at_box_max", at_max))
    tiny = xyzi(rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, 1.1754944e-38, 1e-30, -1e-30], np.float32), (400, 3)))
    fx.append(("signed_zero_subnormal", tiny))
    huge = xyzi(rng.uniform(-3e38, 3e38, (600, 3)))
    huge[0, :3], huge[1, :3] = 3e38, -3e38
    fx.append(("extent_3e38", huge))
    for n in (1, 31, 32, 33, 1023, 1024, 1025, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1):
        fx.append(("n%d" % n, uniform_cloud(n, 100 + n)))
    return fx


@pytest.mark.parametrize("name", [f[0] for f in structure_fixtures()])
def test_tree_structure_bit_for_bit(gpu_mod, name):
    cloud = dict(structure_fixtures())[name]
    with hooked(gpu_mod) as g:
        check_tree(cloud, hooks.debug_nn_tree(g, cloud), name)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the grid's structure
# ------------------------------------------------------------------------------------------------------------------------------------
def restated_cells(xyz, cell):
    f = np.floor(xyz.astype(np.float64) / np.float64(cell))
    return np.clip(f, -2.0 ** 30, 2.0 ** 30).astype(np.int64).astype(np.int32)


def restated_bucket(c, mask):
    """ev_bucket in uint32 arithmetic: the three cell coordinates times their primes, xor-ed, through murmur3's finaliser, masked"""
    u = np.ascontiguousarray(c, np.int32).view(np.uint32).astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    k = ((u[:, 0] * np.uint64(73856093)) & m32) ^ ((u[:, 1] * np.uint64(19349663)) & m32) ^ ((u[:, 2] * np.uint64(83492791)) & m32)
    k ^= k >> np.uint64(16)
    k = (k * np.uint64(0x85EBCA6B)) & m32
    k ^= k >> np.uint64(13)
    k = (k * np.uint64(0xC2B2AE35)) & m32
    k ^= k >> np.uint64(16)
    return (k & np.uint64(mask)).astype(np.int64)


def sized_nb(n):
    """the host code's rule: a power of two >= the estimate's size, at least 1024"""
    nb = 1024
    while nb < n:
        nb *= 2
    return nb


def check_grid(est, cell, nb, off, pts, idx, base, first, what):
    """estimate `est` in the table rows off[base .. base + nb]: pts / idx are the table's scattered arrays, `first` the estimate's first
    point in them (its indices are stored as first + i)"""
    n = len(est)
    assert nb == sized_nb(n) and nb & (nb - 1) == 0, (what, nb, n)
    b = restated_bucket(restated_cells(est[:, :3], cell), nb - 1)
    hist = np.bincount(b, minlength=nb)
    o = off[base:base + nb + 1].astype(np.int64)
    assert np.array_equal(o - o[0], np.concatenate([[0], np.cumsum(hist)])), (what, "offsets are not the exclusive scan of the histogram")
    assert o[0] == first and o[nb] == first + n, (what, o[0], o[nb])
    seg_idx = idx[first:first + n].astype(np.int64) - first
    assert np.array_equal(np.sort(seg_idx), np.arange(n)), (what, "indices are not a permutation")
    # each bucket's slice holds exactly its members (as a set): the bucket of slot s is the one whose range holds s
    slot_bucket = np.repeat(np.arange(nb), hist)
    assert np.array_equal(b[seg_idx], slot_bucket), (what, "a point lies in another bucket's slice")
    assert np.array_equal(bits(pts[first:first + n]), bits(est[seg_idx])), (what, "scattered points are not their rows")
    return hist


def grid_fixtures():
    rng = np.random.default_rng(9)
    v = 0.2
    fx = [("uniform", uniform_cloud(5000, 4), v), ("world", world_slice(3000), v), ("negative", uniform_cloud(1500, 5, half=3.0) - np.float32([50, 70, 9, 0]), v)]
    k = rng.integers(-40, 40, (1200, 3)).astype(np.float64)
    faces = (k * v).astype(np.float32)
    faces[::3] = np.nextafter(faces[::3], np.float32(-np.inf))
    faces[1::3] = np.nextafter(faces[1::3], np.float32(np.inf))
    fx.append(("cell_faces", xyzi(faces), v))
    far = uniform_cloud(900, 6, half=1.0)
    far[::2, :3] *= np.float32(3e9)   # (coordinate / voxelsize beyond 2^30: clamped)
    far[1::4, 0] = -2.5e30
    fx.append(("beyond_clamp", far, v))
    fx.append(("one_cell", xyzi(rng.uniform(0.01, 0.19, (1500, 3))), v))
    for n in (1, 1023, 1024, 1025, 2047, 2048, 2049):
        fx.append(("n%d" % n, uniform_cloud(n, 200 + n, half=8.0), v))
    return fx


@pytest.mark.parametrize("name", [f[0] for f in grid_fixtures()])
def test_grid_structure(gpu_mod, name):
    est, v = {f[0]: f[1:] for f in grid_fixtures()}[name]
    with hooked(gpu_mod) as g:
        d = hooks.debug_ev_grid(g, est, v)
    hist = check_grid(est, v, d["nb"], d["off"], d["pts"], d["idx"], 0, 0, name)
    if name == "one_cell":
        assert hist.max() == len(est)
    if name == "uniform":
        assert hist.max() <= 12  # (5000 points over 8192 buckets: Poisson with mean 0.6; 12 in one bucket has probability < 1e-9)


def test_grid_structure_of_evaluate_many(gpu_mod):
    ests = [uniform_cloud(1025, 31, half=6.0), np.zeros((0, 4), np.float32), uniform_cloud(700, 32, half=6.0)]
    with hooked(gpu_mod) as g:
        d = hooks.debug_ev_grid_many(g, ests, 0.2)
    first = base = 0
    for j, e in enumerate(ests):
        nb = int(d["tab"][j, 3]) + 1
        assert d["tab"][j, :3].tolist() == [first, len(e), base], (j, d["tab"][j])
        if len(e):
            check_grid(e, 0.2, nb, d["off"], d["pts"], d["idx"], base, first, "estimate %d" % j)
        else:
            assert nb == 1024 and (d["off"][base:base + nb + 1] == first).all()
        first, base = first + len(e), base + nb
    assert d["nb"] == base and d["off"][base] == first


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the search's effort is what the algorithm says, and is necessary
# ------------------------------------------------------------------------------------------------------------------------------------
def restated_search(tree, q, f32):
    """The depth-first search over a dumped tree, restated: the nearer child first (the left one on equal bounds), the sibling stacked, a
    node entered or popped only when its lower bound is not strictly greater than the best d^2 so far, float64 arithmetic
    ((gx*gx + gy*gy) + gz*gz) or float32 (r = 0; r += gx*gx; ...).  Returns (best d^2, smallest index at it, opened leaves in order,
    leaf points tested)."""
    P, n = tree["P"], len(tree["idx"])
    if f32:
        F = np.float32
        LO, HI, PT, Q = tree["lo"], tree["hi"], tree["pts"][:, :3], [np.float32(x) for x in q]
    else:
        F = float
        LO, HI, PT, Q = tree["lo"].astype(np.float64).tolist(), tree["hi"].astype(np.float64).tolist(), tree["pts64"], [float(x) for x in q]
    zero = F(0.0)

    def lb(k):
        g = []
        for a in range(3):
            l, u, x = LO[k][a], HI[k][a], Q[a]
            g.append(l - x if x < l else (x - u if x > u else zero))
        if f32:
            r = zero
            for a in range(3):
                r = r + g[a] * g[a]
            return r
        return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]

    best, best_i = F(np.inf), 0xFFFFFFFF
    node, stack, opened, tested = 1, [], [], 0
    while True:
        descend = False
        if node >= P:
            b = (node - P) * NN_LEAF
            e = min(b + NN_LEAF, n)
            opened.append(node - P)
            tested += e - b
            p = PT[b:e]
            if f32:
                d2 = np.zeros(e - b, np.float32)
                for a in range(3):
                    d = Q[a] - p[:, a]
                    d2 = d2 + d * d
            else:
                ex, ey, ez = Q[0] - p[:, 0], Q[1] - p[:, 1], Q[2] - p[:, 2]
                d2 = (ex * ex + ey * ey) + ez * ez
            m = d2.min()
            if m <= best:
                j = int(tree["idx"][b:e][d2 == m].min())
                if m < best or j < best_i:
                    best, best_i = F(m), j
        else:
            c = 2 * node
            ok0, ok1 = LO[c][0] <= HI[c][0], LO[c + 1][0] <= HI[c + 1][0]
            d0 = lb(c) if ok0 else F(np.inf)
            d1 = lb(c + 1) if ok1 else F(np.inf)
            v0, v1 = ok0 and not d0 > best, ok1 and not d1 > best
            if v0 and v1:
                near = c + 1 if d1 < d0 else c
                stack.append(near ^ 1)
                node, descend = near, True
            elif v0 or v1:
                node, descend = (c if v0 else c + 1), True
        if descend:
            continue
        more = False
        while stack:
            k = stack.pop()
            if not lb(k) > best:
                node, more = k, True
                break
        if not more:
            return best, best_i, opened, tested


def necessary_leaves(tree, q, best, f32):
    """N(q): the leaves whose box lower bound is <= the final best d^2 (from brute force), for every query, as a (queries x leaves) mask"""
    P, n = tree["P"], len(tree["idx"])
    n_leaves = -(-n // NN_LEAF)
    lo, hi = tree["lo"][P:P + n_leaves, :3], tree["hi"][P:P + n_leaves, :3]
    T = np.float32 if f32 else np.float64
    qq, lo, hi = q[:, None, :3].astype(T), lo[None].astype(T), hi[None].astype(T)
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.where(qq < lo, lo - qq, np.where(qq > hi, qq - hi, T(0)))
        if f32:
            r = np.zeros(g.shape[:2], np.float32)
            for a in range(3):
                r = r + g[..., a] * g[..., a]
        else:
            r = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    return r <= best[:, None]


def effort_fixtures():
    rng = np.random.default_rng(21)
    n_q = 300 if ON_CPU else 2049
    u = uniform_cloud(5000, 41)
    w = world_slice(5000)
    scan = world_slice(n_q, spacing=0.4)
    scan[:, :3] += rng.normal(0, 0.03, (len(scan), 3)).astype(np.float32)
    d, place = dup_runs(42)
    qd = np.concatenate([xyzi(place), xyzi(place[rng.integers(0, len(place), n_q - len(place))] + rng.normal(0, 0.5, (n_q - len(place), 3)))])
    far = rng.normal(0, 1, (n_q, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * rng.choice([1e4, 1e5, 1e6, 1e7], (n_q, 1))
    return [("uniform_inside", u, xyzi(rng.uniform(-20, 20, (n_q, 3)))), ("world_scan", w, scan), ("far_outside", u, xyzi(far)),
            ("dup_runs", d, qd)]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", [f[0] for f in effort_fixtures()])
def test_search_effort_equals_the_restated_search_and_covers_the_necessary_leaves(gpu_mod, name, f32):
    """The kernel's per-query counts of opened leaves and tested leaf points EQUAL the restated search's (the search is deterministic per
    lane: no margin).  The inclusion N(q) <= opened is asserted on the restated search's set of leaves, whose size and point count the
    kernel's counts equal.  The printed ratio sum(opened) / sum(|N|) is the overhead of the search order (MEASUREMENTS.md); it is
    recorded, not asserted."""
    cloud, q = {f[0]: f[1:] for f in effort_fixtures()}[name]
    with hooked(gpu_mod) as g:
        tree = hooks.debug_nn_tree(g, cloud)
        out = hooks.debug_nn_effort(g, cloud, q, f32)
    check_tree(cloud, tree, name)
    tree["pts64"] = tree["pts"][:, :3].astype(np.float64)
    metric = d2_f32 if f32 else d2_f64
    wbits = bits(cloud[:, 3])
    best, idx, mixed = brute(cloud[:, :3], q[:, :3], metric, wbits)
    need = necessary_leaves(tree, q, best, f32)
    n_open = n_need = 0
    with np.errstate(over="ignore"):
        for i in range(len(q)):
            b, bi, opened, tested = restated_search(tree, q[i, :3], f32)
            assert (b, bi) == (best[i], idx[i]), (name, i, b, bi, best[i], idx[i])
            assert out["effort"][i].tolist() == [len(opened), tested], (name, "query", i, out["effort"][i], len(opened), tested)
            assert len(set(opened)) == len(opened)
            missing = set(np.flatnonzero(need[i]).tolist()) - set(opened)
            assert not missing, (name, "query", i, "necessary leaves never opened", sorted(missing)[:5])
            n_open += len(opened)
            n_need += int(need[i].sum())
    if f32:
        assert np.array_equal(bits(out["rows"][:, 3]), wbits[idx]) and out["n_tied"] == int(mixed.sum())
    else:
        assert np.array_equal(bits(out["dist"]), bits(np.sqrt(best))) and np.array_equal(out["nearest"], idx.astype(np.uint32))
    print("EFFORT %s %s: tree %d points / %d leaves, %d queries, opened %d, necessary %d, ratio %.3f, points tested per query %.1f"
          % (name, "f32" if f32 else "f64", len(cloud), -(-len(cloud) // NN_LEAF), len(q), n_open, n_need, n_open / n_need,
             out["effort"][:, 1].mean()))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4 / 5. the public calls against brute force
# ------------------------------------------------------------------------------------------------------------------------------------
def is_dynamic(w):
    w = np.asarray(w, np.float32)
    inr = (w >= 0) & (w < np.float32(4294967296.0))
    sem = np.where(inr, w, np.float32(0)).astype(np.uint32) & 0xFFFF
    return inr & (sem >= 252) & (sem <= 259), ~inr


def check_overlap(handle, tree, q, what, voxelsize=0.3):
    r = handle.overlap(tree, q, voxelsize=voxelsize, per_point=True)
    d2, idx, _ = brute(tree[:, :3], q[:, :3], d2_f64)
    assert np.array_equal(bits(r["dist"]), bits(np.sqrt(d2))), (what, "distance bits", np.flatnonzero(bits(r["dist"]) != bits(np.sqrt(d2)))[:5])
    assert np.array_equal(r["nearest"], idx.astype(np.uint32)), (what, "nearest index", np.flatnonzero(r["nearest"] != idx)[:5])
    ref = evalmap.overlap(tree[:, :3], q[:, :3], voxelsize)
    for k in REPORT_FIELDS:
        assert same_bits(r[k], ref[k]), (what, k, r[k], ref[k])


def check_label_map(handle, tree, q, what, leaf=1e-3):
    """every source point its own voxel (or VoxelGrid's index overflow, which returns the input): the centroids are the points"""
    _, first = np.unique(q[:, :3], axis=0, return_index=True)
    src = np.ascontiguousarray(q[np.sort(first)])
    src[:, 3] = 0.0
    cent, _, _, overflow = orc.voxel_grid(src, leaf)
    if overflow:
        cent = src.copy()
    assert len(cent) == len(src), (what, "the fixture's points share voxels", len(cent), len(src))
    wbits = bits(tree[:, 3])
    _, idx, mixed = brute(tree[:, :3], cent[:, :3], d2_f32, wbits)
    rows, info = handle.label_map(src, tree, leaf)
    assert (info["n_src"], info["n_out"], info["passthrough"]) == (len(src), len(cent), int(overflow)), (what, info)
    assert np.array_equal(bits(rows[:, :3]), bits(cent[:, :3])), (what, "centroids")
    bad = np.flatnonzero(bits(rows[:, 3]) != wbits[idx])
    assert len(bad) == 0, (what, "labels", len(bad), bad[:5], rows[bad[:3]], tree[idx[bad[:3]]])
    assert info["n_tied"] == int(mixed.sum()), (what, "n_tied", info["n_tied"], int(mixed.sum()))


def check_complement(handle, tree, q, what):
    dyn, oor = is_dynamic(q[:, 3])
    static = ~dyn
    d2, _, _ = brute(tree[:, :3], q[:, :3], d2_f32)
    lost = static & (d2.astype(np.float64) > 0.03)
    rows, info = handle.static_complement(tree, q)
    assert info == {"n_gt": len(q), "n_gt_static": int(static.sum()), "n_lost": int(lost.sum()), "n_label_out_of_range": int(oor.sum())}, (what, info)
    assert np.array_equal(bits(rows), bits(q[lost])), (what, "lost rows")


def brute_evaluate(gt, est, voxelsize):
    """codes and counters from float64 brute force with the sqrt(d^2) < thr rule; n_tied: GT points within the threshold whose minimum is
    shared by estimated points of both classes"""
    g_dyn, g_oor = is_dynamic(gt[:, 3])
    e_dyn, e_oor = is_dynamic(est[:, 3])
    code = np.zeros(len(gt), np.uint8)
    tied = np.zeros(len(gt), bool)
    if len(est) and len(gt):
        d2, idx, mixed = brute(est[:, :3], gt[:, :3], d2_f64, e_dyn)
        within = np.sqrt(d2) < voxelsize * np.sqrt(3) / 2
        b_dyn = e_dyn[idx]
        code[within & ~g_dyn & ~b_dyn] = 1
        code[within & g_dyn & b_dyn] = 2
        code[within & (g_dyn != b_dyn)] = 3
        tied = within & mixed
    ctr = {"gt_static": int((~g_dyn).sum()), "gt_dynamic": int(g_dyn.sum()), "est_static": int((~e_dyn).sum()), "est_dynamic": int(e_dyn.sum()),
           "preserved_static": int((code == 1).sum()), "preserved_dynamic": int((code == 2).sum()), "n_tied": int(tied.sum()),
           "n_label_out_of_range": int(g_oor.sum() + e_oor.sum())}
    return code, tied, ctr


def check_evaluate(handle, gt, est, what, voxelsize=0.3):
    code, tied, ctr = brute_evaluate(gt, est, voxelsize)
    r = handle.evaluate(gt, est, voxelsize=voxelsize, per_point=True)
    assert np.array_equal(r["per_point"], code), (what, "codes", np.flatnonzero(r["per_point"] != code)[:5])
    assert {k: r[k] for k in ctr} == ctr, (what, {k: r[k] for k in ctr}, ctr)
    many = handle.evaluate_many(gt, [est, est[: max(1, len(est) // 2)]], voxelsize=voxelsize)
    assert {k: many[0][k] for k in ctr} == ctr, (what, "evaluate_many")
    bc = handle.evaluate_by_class(gt, est, voxelsize=voxelsize)
    assert {k: bc[k] for k in ctr} == ctr, (what, "evaluate_by_class", {k: bc[k] for k in ctr}, ctr)
    oor = is_dynamic(gt[:, 3])[1]
    key = np.where(oor, 0x10000, np.where(oor, np.float32(0), gt[:, 3]).astype(np.uint32) & 0xFFFF).astype(np.int64)
    rows = {int(c["key"]): c for c in bc["classes"]}
    for k in np.unique(key):
        m = key == k
        got = tuple(int(rows[int(k)][f]) for f in ("n_gt", "n_within", "n_preserved", "n_tied"))
        assert got == (int(m.sum()), int((code[m] != 0).sum()), int(np.isin(code[m], (1, 2)).sum()), int(tied[m].sum())), (what, "class", k, got)
    return code, tied


def check_all_calls(handle, tree, q, what, voxelsize=0.3):
    check_overlap(handle, tree, q, what, voxelsize)
    check_label_map(handle, tree, q, what)
    check_complement(handle, tree, q, what)
    check_evaluate(handle, q, tree, what, voxelsize)


TREE_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1)
QUERY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
SIZE_PAIRS = [(TREE_SIZES[i % 14], QUERY_COUNTS[(i + 3 * (i // 14)) % 8]) for i in range(28)]
assert all(sum(t == a for t, _ in SIZE_PAIRS) >= 2 for a in TREE_SIZES) and all(sum(c == b for _, c in SIZE_PAIRS) >= 2 for b in QUERY_COUNTS)


def boundary_clouds(n_tree, n_q):
    tree = uniform_cloud(n_tree, 1000 + n_tree, half=6.0)
    rng = np.random.default_rng(n_tree * 7 + n_q)
    q = uniform_cloud(n_q, 2000 + n_q, half=6.5, labels=(40.0, 252.0, 72.0, -1.0))
    on = rng.integers(0, n_q, max(1, n_q // 8))
    q[on, :3] = tree[rng.integers(0, n_tree, len(on)), :3]  # (some queries exactly on tree points)
    return tree, q


@pytest.mark.parametrize("n_tree,n_q", SIZE_PAIRS, ids=["%s-tree%d-q%d" % ("small" if t <= 1025 else "large", t, c) for t, c in SIZE_PAIRS])
def test_boundary_sizes_through_the_tree_calls(handle, n_tree, n_q):
    tree, q = boundary_clouds(n_tree, n_q)
    what = "tree %d, %d queries" % (n_tree, n_q)
    check_overlap(handle, tree, q, what)
    check_label_map(handle, tree, q, what)
    check_complement(handle, tree, q, what)


@pytest.mark.parametrize("n_est", [1, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("n_gt", [257, 1000])
def test_boundary_sizes_through_the_evaluator(handle, n_est, n_gt):
    est, gt = boundary_clouds(n_est, n_gt)
    est[:, :3] *= np.float32(0.25)  # (dense enough that most GT points have an estimated point within the threshold)
    gt[:, :3] *= np.float32(0.25)
    code, _ = check_evaluate(handle, gt, est, "estimate %d, gt %d" % (n_est, n_gt))
    if n_est >= 1023:
        assert (code != 0).sum() > n_gt // 4 and (code == 0).sum() > 0


def test_frame_borders_at_every_lane_position(handle):
    """frame lengths that put frame borders at the lane positions of a wavefront and of a workgroup, against evalmap.align_frames"""
    lens = [1, 63, 1, 191, 0, 257, 64, 62, 2, 255, 1, 256, 0, 0, 65, 127, 129, 3]
    m = uniform_cloud(1025, 51, half=6.0)
    rng = np.random.default_rng(52)
    frames = [uniform_cloud(n, 300 + i, half=6.0) for i, n in enumerate(lens)]
    poses = []
    for i in range(len(lens)):
        T = np.eye(4, dtype=np.float32)
        a = rng.uniform(-0.2, 0.2)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        poses.append(T)
    rows, summary = handle.align_frames(frames, poses, None, map=m, voxelsize=0.5)
    ref_rows, ref_summary = evalmap.align_frames(m[:, :3], frames, poses, None, 0.5)
    assert len(rows) == len(ref_rows)
    for f, (r, e) in enumerate(zip(rows, ref_rows)):
        for k in REPORT_FIELDS + ("n_points", "n_non_finite"):
            assert same_bits(r[k], e[k]), ("frame", f, k, r[k], e[k])
    for k in REPORT_FIELDS:
        assert same_bits(summary[k], ref_summary[k]), ("summary", k, summary[k], ref_summary[k])


# ---- 5. adversarial geometry, seeded and fixed ----
def gen_dup_runs(seed):
    tree, place = dup_runs(seed)
    rng = np.random.default_rng(seed + 1)
    near = place[rng.integers(0, len(place), 300)] + rng.normal(0, 0.4, (300, 3))
    return tree, np.concatenate([xyzi(place, 40.0), xyzi(near, rng.choice(np.float32([40.0, 252.0]), 300))])


def gen_lattice(seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    tree = xyzi(g * 0.25, rng.choice(np.float32([40.0, 252.0, 50.0]), len(g)))
    tree = tree[rng.permutation(len(tree))]
    centres = (g[(np.abs(g) < 4).all(1)] + 0.5) * 0.25  # (eight lattice points at the same distance, exactly: 0.125 is a power of two)
    q = np.concatenate([xyzi(g * 0.25, 40.0), xyzi(centres, 252.0)])
    return np.ascontiguousarray(tree), q[rng.permutation(len(q))]


def gen_mixed_scales(seed):
    rng = np.random.default_rng(seed)
    cl = [rng.normal(0, s, (400, 3)) + c for s, c in ((1e-3, (0.5, 0.5, 0.5)), (1.0, (10.0, 0.0, 0.0)), (1e6, (0.0, 0.0, 0.0)))]
    tree = xyzi(np.concatenate(cl), rng.choice(np.float32([40.0, 252.0]), 1200))
    qs = [rng.normal(0, s, (150, 3)) + c for s, c in ((2e-3, (0.5, 0.5, 0.5)), (2.0, (10.0, 0.0, 0.0)), (2e6, (0.0, 0.0, 0.0)))]
    return tree[rng.permutation(1200)], xyzi(np.concatenate(qs), rng.choice(np.float32([40.0, 252.0]), 450))


def gen_sheet_and_outlier(seed):
    rng = np.random.default_rng(seed)
    sheet = np.c_[rng.uniform(-8, 8, (1500, 2)), np.full(1500, 0.5)]
    tree = xyzi(np.concatenate([sheet, [[1e7, 1e7, 1e7]]]), rng.choice(np.float32([40.0, 252.0]), 1501))
    q = np.concatenate([np.c_[rng.uniform(-9, 9, (400, 2)), rng.uniform(0, 1, 400)], [[9e6, 9e6, 9e6], [5e6, 5e6, 5e6]]])
    return tree[rng.permutation(1501)], xyzi(q, rng.choice(np.float32([40.0, 252.0]), len(q)))


def gen_exact_queries(seed):
    rng = np.random.default_rng(seed)
    base = uniform_cloud(600, seed, half=5.0, labels=(40.0, 252.0))
    dup = base[rng.integers(0, 600, 300)].copy()
    dup[:, 3] = rng.choice(np.float32([40.0, 252.0]), 300)  # (a duplicate of a tree point, often with the other class)
    tree = np.concatenate([base, dup])
    tree = np.ascontiguousarray(tree[rng.permutation(len(tree))])
    q = tree[rng.integers(0, len(tree), 500)].copy()
    q[:, 3] = rng.choice(np.float32([40.0, 252.0]), 500)
    return tree, q


def gen_far_queries(seed):
    rng = np.random.default_rng(seed)
    tree = uniform_cloud(2000, seed, half=10.0, labels=(40.0, 252.0))
    d = rng.normal(0, 1, (400, 3))
    d = d / np.linalg.norm(d, axis=1)[:, None] * rng.choice([1e4, 1e5, 1e6, 1e7], (400, 1))
    d[::9, 1:] = 0.0  # (along an axis: many box bounds tie)
    return tree, xyzi(d, rng.choice(np.float32([40.0, 252.0]), 400))


GENERATORS = {"dup_runs": gen_dup_runs, "lattice": gen_lattice, "mixed_scales": gen_mixed_scales, "sheet_and_outlier": gen_sheet_and_outlier,
              "exact_queries": gen_exact_queries, "far_queries": gen_far_queries}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_adversarial_geometry_through_every_call(handle, gen, seed):
    tree, q = GENERATORS[gen](seed)
    check_all_calls(handle, tree, q, "%s seed %d" % (gen, seed))
    if gen in ("dup_runs", "lattice", "exact_queries"):
        _, _, mixed = brute(tree[:, :3], q[:, :3], d2_f32, bits(tree[:, 3]))
        assert mixed.sum() > 20  # (the fixture is what it claims: massive ties between different labels)


def face_offsets(g, thr):
    """for the float32 coordinate g: the largest float32 e > g with sqrt((g - e)^2) < thr in float64 and the next float up (>= thr),
    found by a search on the host"""
    c = np.float32(np.float64(g) + thr)
    cand = np.sort((np.array([c], np.float32).view(np.int32) + np.arange(-6, 7, dtype=np.int32)).view(np.float32))
    d = np.sqrt((np.float64(g) - cand.astype(np.float64)) ** 2)
    inside = d < thr
    assert inside[0] and not inside[-1] and (np.diff(inside.astype(int)) <= 0).all()
    k = int(inside.sum())
    return cand[k - 1], cand[k]


@pytest.mark.parametrize("voxelsize", [0.2, 0.25])
def test_evaluator_points_on_cell_faces_and_at_the_threshold(handle, voxelsize):
    """ground-truth points at k * voxelsize +- {0, 1 ulp} on one axis (cell faces, also on the negative side), each paired with an
    estimated point just inside or just outside voxelsize * sqrt(3) / 2 across that face"""
    thr = voxelsize * np.sqrt(3) / 2
    gt, est, expect = [], [], []
    row = 0
    for axis in range(3):
        for k in range(-5, 6):
            face = np.float32(k * voxelsize)
            for g in (np.nextafter(face, np.float32(-np.inf)), face, np.nextafter(face, np.float32(np.inf))):
                for which, e in enumerate(face_offsets(g, thr)):
                    for sign in (1.0, -1.0):
                        p = np.zeros(3, np.float32)
                        p[[a for a in range(3) if a != axis]] = (3.0 * (row % 40) + 1.0, 3.0 * (row // 40) + 1.0)  # (pairs 3 m apart)
                        pg, pe = p.copy(), p.copy()
                        pg[axis] = g
                        pe[axis] = np.float32(g) + sign * (np.float32(e) - np.float32(g))
                        d = np.sqrt((np.float64(pg[axis]) - np.float64(pe[axis])) ** 2)
                        if (d < thr) != (which == 0):  # (the mirrored offset rounded across the threshold: brute force still decides it)
                            which = 0 if d < thr else 1
                        gt.append(np.append(pg, 40.0))
                        est.append(np.append(pe, 40.0))
                        expect.append(1 if which == 0 else 0)
                        row += 1
    gt, est = np.ascontiguousarray(gt, np.float32), np.ascontiguousarray(est, np.float32)
    code, _ = check_evaluate(handle, gt, est, "faces v=%g" % voxelsize, voxelsize)
    assert code.tolist() == expect and 0 < sum(expect) < len(expect)


def test_no_generated_query_was_left_out():
    assert N_SKIPPED[0] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. float32 overflow: every d^2 is +inf
# ------------------------------------------------------------------------------------------------------------------------------------
def overflow_clouds(labels, half=5.0):
    """a medium around the origin (half = 1e17: wider than any relative margin around a query 2e19 m away) and queries of which some have
    every coordinate difference above 2e19 m (their float32 d^2 to every medium point is +inf), mixed with ordinary ones"""
    rng = np.random.default_rng(61)
    medium = uniform_cloud(300, 62, half=half, labels=labels)
    q = uniform_cloud(200, 63, half=6.0)
    far = np.arange(0, 200, 3)
    q[far, :3] = rng.choice(np.float32([-1.0, 1.0]), (len(far), 3)) * rng.uniform(2.1e19, 6e19, (len(far), 3)).astype(np.float32)
    assert np.isinf(d2_f32(q[far, :3], medium[:, :3])).all() and np.isfinite(q).all()
    return medium, q, far


@pytest.mark.parametrize("half", [5.0, 1e17])
def test_label_map_where_every_float32_distance_overflows(handle, half):
    """the contract is the lowest index among the points at the minimum float32 d^2: at +inf that is medium point 0, and a medium with one
    single label has no ties"""
    medium, q, far = overflow_clouds((77.0,), half)
    rows, info = handle.label_map(q, medium, 1e-3)
    assert info["passthrough"] == 1 and info["n_out"] == len(q)
    assert (rows[:, 3] == 77.0).all() and info["n_tied"] == 0, info
    check_label_map(handle, medium, q, "overflow, one label")
    medium, q, far = overflow_clouds((77.0, 252.0), half)
    medium[0, 3], medium[1, 3] = 77.0, 252.0
    _, idx, mixed = brute(medium[:, :3], q[:, :3], d2_f32, bits(medium[:, 3]))
    assert (idx[far] == 0).all() and mixed[far].all() and not mixed[np.setdiff1d(np.arange(len(q)), far)].any()
    rows, info = handle.label_map(q, medium, 1e-3)
    assert info["n_tied"] == len(far), (info, len(far))
    assert (rows[far, 3] == 77.0).all()
    check_label_map(handle, medium, q, "overflow, two labels")


@pytest.mark.parametrize("half", [5.0, 1e17])
def test_label_from_on_the_host_where_every_float32_distance_overflows(half):
    for labels in ((77.0,), (77.0, 252.0)):
        medium, q, far = overflow_clouds(labels, half)
        medium[0, 3] = 77.0
        wbits = bits(medium[:, 3])
        _, idx, mixed = brute(medium[:, :3], q[:, :3], d2_f32, wbits)
        rows, info = evalmap.label_from(q, medium)
        assert np.array_equal(bits(rows[:, 3]), wbits[idx]) and info["n_tied"] == int(mixed.sum()), (labels, info, int(mixed.sum()))


@pytest.mark.parametrize("half", [5.0, 1e17])
def test_static_complement_where_every_float32_distance_overflows(handle, half):
    medium, q, far = overflow_clouds((40.0, 252.0), half)
    q[:, 3] = 40.0
    d2, _, _ = brute(medium[:, :3], q[:, :3], d2_f32)
    assert np.isinf(d2[far]).all()  # (so every such point is lost in the expectation check_complement forms)
    check_complement(handle, medium, q, "overflow")
    rows, info = handle.static_complement(medium, q)
    assert info["n_lost"] >= len(far) and np.isin(bits(q[far, 0]), bits(rows[:, 0])).all()
