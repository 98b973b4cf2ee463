"""Test infrastructure: the designed scenes of the decision per object (evalmap.object_vote, Erasor.object_vote), shared by
tests/test_evalmap_object_vote.py, tests/test_gpu_object_vote.py and tests/test_object_vote_driver.py.  A plain module like hooks.py."""
import numpy as np

from erasor_amd import evalmap

ROW = evalmap.OBJECT_ROW_DTYPE
UNCHANGED, REMOVED, REVERTED, NOT_OBJECT = evalmap.OBJECT_UNCHANGED, evalmap.OBJECT_REMOVED, evalmap.OBJECT_REVERTED, evalmap.OBJECT_NOT_OBJECT


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def lattice(nx, ny, nz, step, origin):
    """nx * ny * nz points `step` apart from `origin`, x fastest"""
    k = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (k * np.float64(step) + np.asarray(origin, np.float64)).astype(np.float32)


KNOWN_PARAMS = dict(tol=0.3, remove_ratio=0.5, revert_ratio=0.05, max_size=500)


def known_scene():
    """(cloud, votes, ground): a 16 x 16 ground lattice at 0.25 m with 10 of its points voted; box A (5 x 5 x 5 at 0.2 m, moving-car
    labels, 80 voted), box B (125 points, 3 voted), box C (125 points, 40 voted) and wall D (30 x 1 x 30 at 0.1 m, 600 voted), more
    than 2 m from one another, their bottoms 0.2 m (within the tolerance 0.3) above the lattice"""
    parts = [lattice(16, 16, 1, 0.25, (0, 0, 0)), lattice(5, 5, 5, 0.2, (0, 0, 0.2)), lattice(5, 5, 5, 0.2, (2.95, 0, 0.2)),
             lattice(5, 5, 5, 0.2, (0, 2.95, 0.2)), lattice(30, 1, 30, 0.1, (3.0, 3.75, 0.2))]
    n_voted = [10, 80, 3, 40, 600]
    labels = [40.0, 252.0, 40.0, 40.0, 50.0]
    cloud = np.concatenate([xyzi(p, w) for p, w in zip(parts, labels)])
    votes, ground = [], []
    for i, (p, k) in enumerate(zip(parts, n_voted)):
        v = np.zeros(len(p), np.uint8)
        v[(np.arange(k) * 7919) % len(p) if i else np.arange(k) * 25] = 1  # (7919 is coprime to 125 and 900: k distinct points)
        assert v.sum() == k
        votes.append(v)
        ground.append(np.full(len(p), 1 if i == 0 else 0, np.uint8))
    return cloud, np.concatenate(votes), np.concatenate(ground)


def known_answer(ground_keep=True):
    """mask, rows and result of known_scene() under KNOWN_PARAMS with the ground mask, written out by hand"""
    cloud, votes, ground = known_scene()
    mask = (votes == 0).astype(np.uint8)
    mask[:256] = 1 if ground_keep else mask[:256]  # the ground: kept, or removed where voted
    mask[256:381] = 0                              # A: 80 of 125 >= 62.5 -> removed, all of it
    mask[381:506] = 1                              # B: 3 of 125 <= 6.25 -> reverted
    #                                                C: 40 of 125 -> unchanged; D: 900 > max_size -> not an object: their votes stand
    rows = np.zeros(4, ROW)
    rows["first"] = [256, 381, 506, 631]
    rows["n_points"] = [125, 125, 125, 900]
    rows["n_voted"] = [80, 3, 40, 600]
    rows["n_dynamic"] = [125, 0, 0, 0]
    rows["n_voted_dynamic"] = [80, 0, 0, 0]
    f = np.float32
    rows["min_xyz"] = [[0, 0, f(0.2)], [f(2.95), 0, f(0.2)], [0, f(2.95), f(0.2)], [3, f(3.75), f(0.2)]]
    rows["max_xyz"] = [[f(0.8), f(0.8), f(1.0)], [f(3.75), f(0.8), f(1.0)], [f(0.8), f(3.75), f(1.0)],
                       [f(3.0 + 29 * 0.1), f(3.75), f(0.2 + 29 * 0.1)]]
    rows["decision"] = [REMOVED, REVERTED, UNCHANGED, NOT_OBJECT]
    res = dict(n_points=1531, n_ground=256, n_clusters=4, n_touched=4, n_removed_clusters=1, n_reverted_clusters=1, n_not_object=1, n_voted=733,
               n_removed=125 + 40 + 600 + (0 if ground_keep else 10), n_grown=45, n_grown_dynamic=45, n_reverted=3, n_reverted_dynamic=0,
               n_ground_reverted=10 if ground_keep else 0, n_ground_reverted_dynamic=0, largest=900)
    return mask, rows, res


def bridge_scene():
    """two non-ground points 0.5 m apart, each within tol = 0.3 of the one ground point between them"""
    return xyzi([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]]), np.uint8([1, 0, 0]), np.uint8([0, 1, 0])


def random_case(seed):
    """(cloud, votes, ground or None, parameters): up to 2000 points in a box that gives clusters of many sizes, random votes 0 .. 3,
    a random ground mask, random parameters inside their ranges"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 2001))
    tol = float(rng.choice([0.2, 0.3, 0.5]))
    side = tol * (n / rng.uniform(0.3, 1.5)) ** (1 / 3)
    cloud = xyzi(rng.uniform(0, side, (n, 3)), rng.integers(245, 265, n))
    votes = (rng.integers(0, 4, n) * (rng.uniform(0, 1, n) < rng.uniform(0.1, 0.9))).astype(np.uint8)
    ground = None if seed % 4 == 0 else (rng.uniform(0, 1, n) < rng.uniform(0, 0.6)).astype(np.uint8)
    remove = float(rng.choice([0.25, 0.3, 0.5, 0.7, 1.0]))
    prm = dict(tol=tol, vote_thr=int(rng.integers(1, 4)), min_size=int(rng.integers(0, 4)), max_size=int(rng.choice([0, 5, 50])),
               max_extent=float(rng.choice([0.0, 2 * tol, 6 * tol])), remove_ratio=remove, revert_ratio=float(rng.choice([0.0, 0.1, 0.2])) * remove,
               min_voted=int(rng.integers(0, 4)), ground_keep=bool(rng.integers(0, 2)))
    return cloud, votes, ground, prm


def assert_same(got, want, what=""):
    """(mask, rows, ids, kept, result) byte for byte"""
    mask, rows, ids, kept, res = got
    assert res == want[4], (what, res, want[4])
    assert mask.dtype == np.uint8 and mask.shape == want[0].shape and mask.tobytes() == want[0].tobytes(), (what, "mask", np.flatnonzero(mask != want[0])[:5])
    assert rows.dtype == ROW and rows.shape == want[1].shape and rows.tobytes() == want[1].tobytes(), (what, "rows", rows[:3], want[1][:3])
    assert ids.dtype == np.uint32 and ids.shape == want[2].shape and ids.tobytes() == want[2].tobytes(), (what, "ids", np.flatnonzero(ids != want[2])[:5])
    assert kept.shape == want[3].shape and kept.tobytes() == want[3].tobytes(), (what, "kept cloud", kept.shape, want[3].shape)
