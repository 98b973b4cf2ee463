"""The small world of the pose-refinement tests (tests/test_evalmap_refine.py, tests/test_gpu_refine.py): a ground plane, two perpendicular
walls and a few boxes on a 0.2 m lattice with jitter, about 20 k points; frames that see the map points within 15 m of their sensor,
moved into the body frame by the true pose and handed over with a pose that is wrong by up to 0.3 m and 2 degrees.  A plain module."""
import numpy as np

STEP = 0.2


def _grid(u, v):
    a, b = np.meshgrid(u, v, indexing="ij")
    return a.reshape(-1), b.reshape(-1)


def world(seed=11, jitter=0.1):
    # (jitter of half a lattice step: with less, the ground's 0.2 m period gives ICP a local minimum one step off for a 0.3 m error)
    rng = np.random.default_rng(seed)
    parts = []
    g = np.arange(-12.0, 12.0 + 1e-9, STEP)
    x, y = _grid(g, g)
    parts.append(np.stack([x, y, np.zeros_like(x)], 1))                        # the ground
    h = np.arange(STEP, 4.0 + 1e-9, STEP)
    y, z = _grid(g, h)
    parts.append(np.stack([np.full_like(y, 12.0), y, z], 1))                    # a wall across x
    x, z = _grid(g, h)
    parts.append(np.stack([x, np.full_like(x, 12.0), z], 1))                    # a wall across y
    for cx, cy, sx, sy, sz in ((-5.0, 3.0, 2.0, 1.4, 1.6), (4.0, -6.0, 1.2, 3.0, 2.2), (6.0, 5.0, 2.4, 2.0, 1.0), (-7.0, -7.0, 1.6, 1.6, 2.8)):
        bx, by, bz = np.arange(0, sx + 1e-9, STEP), np.arange(0, sy + 1e-9, STEP), np.arange(STEP, sz + 1e-9, STEP)
        for xs in (0.0, sx):
            y, z = _grid(by, bz)
            parts.append(np.stack([np.full_like(y, cx + xs), cy + y, z], 1))
        for ys in (0.0, sy):
            x, z = _grid(bx, bz)
            parts.append(np.stack([cx + x, np.full_like(x, cy + ys), z], 1))
        x, y = _grid(bx, by)
        parts.append(np.stack([cx + x, cy + y, np.full_like(x, sz)], 1))       # the lid
    pts = np.concatenate(parts)
    pts = pts + rng.uniform(-jitter, jitter, pts.shape)
    return np.concatenate([pts, np.full((len(pts), 1), 40.0)], 1).astype(np.float32)


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def frames(m, n_frames=6, seed=3, every=1, reach=15.0, max_t=0.3, max_deg=2.0):
    """(scans, T_true float64, T_given float32): scan f is the map's points within `reach` of sensor f (every `every`-th of them), in the
    body frame of T_true[f]; T_given[f] is T_true[f] with an error of up to max_t metres and max_deg degrees in front of it"""
    rng = np.random.default_rng(seed)
    xyz = m[:, :3].astype(np.float64)
    scans, true, given = [], [], []
    for f in range(n_frames):
        yaw = rng.uniform(-np.pi, np.pi)
        Tt = pose(rot(rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), yaw), [rng.uniform(-6, 6), rng.uniform(-6, 6), 1.7])
        seen = xyz[np.linalg.norm(xyz - Tt[:3, 3], axis=1) < reach][::every]
        body = (seen - Tt[:3, 3]) @ Tt[:3, :3]  # R^t (x - t)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = np.radians(max_deg) * rng.uniform(0.5, 1.0)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Re = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        dt = rng.normal(size=3)
        dt *= max_t * rng.uniform(0.5, 1.0) / np.linalg.norm(dt)
        Tg = pose(Re @ Tt[:3, :3], Tt[:3, 3] + dt)
        scans.append(np.concatenate([body, np.full((len(body), 1), 40.0)], 1).astype(np.float32))
        true.append(Tt)
        given.append(Tg.astype(np.float32))
    return scans, np.array(true), np.array(given)


def pose_error(T, T_true):
    """(|t - t_true|, the angle of R R_true^t) of one pose"""
    dR = T[:3, :3] @ T_true[:3, :3].T
    s = 0.5 * np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])  # (sin: exact near zero, unlike acos)
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.arctan2(s, (np.trace(dR) - 1) / 2))
