"""The worlds of the point-to-plane refinement's tests (tests/test_evalmap_refine_plane.py, tests/test_gpu_refine_plane.py): designed
lattices whose normals come out as exact axis vectors and whose rank is known, and a ground with two walls that the scans sample at
another step than the map does -- where a point-to-point refinement is biased.  A plain module, like refine_world.py."""
import numpy as np

import refine_world as rw

STEP = 0.25  # the lattices' step: dyadic, like the planes' offsets, so that every centroid and every covariance entry across a plane is exact


def plane(axis, offset, side=24, low=0.0):
    """side x side points at STEP on the plane `axis` = offset; the two in-plane coordinates start at 0 and (a wall's z) at `low`"""
    g = np.arange(side) * STEP
    a, b = np.meshgrid(g, g, indexing="ij")
    a, b, c = a.reshape(-1), b.reshape(-1) + low, np.full(side * side, float(offset))
    return np.stack({0: [c, a, b], 1: [a, c, b], 2: [a, b, c]}[axis], 1)


def lattices(side=24):
    """name -> (map xyz float32, the rank a frame on it has): the planes at least 1 m apart, so that no neighbourhood of k = 8 mixes two"""
    ground, above = plane(2, 0.0, side), plane(2, 2.0, side)
    wall_x, wall_y = plane(0, -1.0, side, 1.0), plane(1, -1.0, side, 1.0)
    return {"one plane": (ground.astype(np.float32), 3), "two parallel planes": (np.concatenate([ground, above]).astype(np.float32), 3),
            "two perpendicular planes": (np.concatenate([ground, wall_x]).astype(np.float32), 5),
            "three perpendicular planes": (np.concatenate([ground, wall_x, wall_y]).astype(np.float32), 6)}


T_TRUE = rw.pose(rw.rot(0.0, 0.0, 0.3), [1.0, 2.0, 0.5])
T_ERR = rw.pose(rw.rot(0.003, -0.002, 0.004), [0.004, -0.003, 0.005])  # a few mm and mrad


def own_points_scan(m, T_true=T_TRUE, T_err=T_ERR, rows=None):
    """(scan XYZI float32, T_given float32): the map's own points (rows: which) in the body frame of T_true, handed over with T_err in
    front of the pose"""
    xyz = np.asarray(m, np.float64)[:, :3]
    if rows is not None:
        xyz = xyz[rows]
    body = (xyz - T_true[:3, 3]) @ T_true[:3, :3]
    return np.concatenate([body, np.full((len(body), 1), 40.0)], 1).astype(np.float32), (T_err @ T_true).astype(np.float32)


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.full((len(xyz), 1), w, np.float32)], 1)


# ---- a ground and two walls: the map sampled at 0.2 m, the scans at 0.27 m, both with jitter inside the surface ----
def _surfaces(step, rng, jitter):
    g = np.arange(-12.0, 12.0 + 1e-9, step)
    h = np.arange(step, 4.0 + 1e-9, step)
    out = []
    for axis, us, vs in ((2, g, g), (0, g, h), (1, g, h)):
        u, v = np.meshgrid(us, vs, indexing="ij")
        u = u.reshape(-1) + rng.uniform(-jitter, jitter, u.size)
        v = v.reshape(-1) + rng.uniform(-jitter, jitter, v.size)
        out.append(np.stack({2: [u, v, np.zeros_like(u)], 0: [np.full_like(u, 12.0), u, v], 1: [u, np.full_like(u, 12.0), v]}[axis], 1))
    return out


def biased_world(seed=21):
    """the map (XYZI float32) at 0.2 m and the three surfaces sampled again at 0.27 m (float64 xyz each: ground, wall across x, wall across y)"""
    rng = np.random.default_rng(seed)
    m = xyzi(np.concatenate(_surfaces(0.2, rng, 0.05)))
    return m, _surfaces(0.27, rng, 0.05)


def biased_frames(surfaces, n_frames=3, seed=4, reach=15.0, every=1):
    """(scans, T_true, T_given, seen): frames as refine_world.frames makes them -- the same pose errors, up to 0.3 m and 2 degrees --
    whose sensor stands where the ground and both walls lie within `reach`; seen[f]: the points of each surface in scan f"""
    rng = np.random.default_rng(seed)
    scans, true, given, seen = [], [], [], []
    for _ in range(n_frames):
        Tt = rw.pose(rw.rot(rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-np.pi, np.pi)), [rng.uniform(0, 7), rng.uniform(0, 7), 1.7])
        parts = [s[np.linalg.norm(s - Tt[:3, 3], axis=1) < reach][::every] for s in surfaces]
        xyz = np.concatenate(parts)
        body = (xyz - Tt[:3, 3]) @ Tt[:3, :3]
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = np.radians(2.0) * rng.uniform(0.5, 1.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Re = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        dt = rng.normal(size=3)
        dt *= 0.3 * rng.uniform(0.5, 1.0) / np.linalg.norm(dt)
        scans.append(xyzi(body))
        true.append(Tt)
        given.append(rw.pose(Re @ Tt[:3, :3], Tt[:3, 3] + dt).astype(np.float32))
        seen.append([len(p) for p in parts])
    return scans, np.array(true), np.array(given), seen
