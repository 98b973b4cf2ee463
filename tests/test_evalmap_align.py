"""evalmap.align_frames, the host oracle of Erasor.align_frames: its transform is the CPU oracle's pcl::transformPointCloud bit for bit,
and its rows are overlap() of each frame's transformed, finite points."""
import numpy as np

import scenarios
from erasor_amd import evalmap
from oracle import orc


def test_the_transform_is_the_oracles_bit_for_bit():
    sc = scenarios.small(n_frames=3)
    for f, scan in enumerate(sc["scans"]):
        scan = np.ascontiguousarray(scan, np.float32)
        want = orc.transform(orc.transform(scan, sc["T_l2b"]), sc["T_b2o"][f])[:, :3]
        got = evalmap._xform(sc["T_b2o"][f], evalmap._xform(sc["T_l2b"], scan[:, :3]))
        assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all(), f


def test_rows_are_the_overlap_of_each_frames_finite_points():
    rng = np.random.default_rng(4)
    m = rng.uniform(-10, 10, (2000, 3)).astype(np.float32)
    a = np.concatenate([rng.uniform(-10, 10, (50, 3)), np.full((50, 1), 7.0)], 1).astype(np.float32)
    b = a.copy()
    b[::5, 0] = np.nan
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.5, -0.25, 2.0]
    Tl = np.eye(4, dtype=np.float32)
    Tl[2, 3] = -2.0
    rows, summary = evalmap.align_frames(m, [a, b, a[:0]], [T, T, T], Tl, 0.2)
    keep = b[~np.isnan(b[:, 0])]
    assert rows[0] == dict(evalmap.overlap(m, evalmap._xform(T, evalmap._xform(Tl, a[:, :3])), 0.2), n_points=50, n_non_finite=0)
    assert rows[1]["n_non_finite"] == 10 and rows[1]["n_points"] == 50 and rows[1]["n_est"] == len(keep) == 40
    assert rows[2]["n_est"] == 0 and np.isnan(rows[2]["median"])
    assert summary["n_est"] == 90
    ident, _ = evalmap.align_frames(m, [a], [np.eye(4)], None, 0.2)
    assert ident[0]["median"] == evalmap.overlap(m, a[:, :3], 0.2)["median"]
