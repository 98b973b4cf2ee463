"""Generates tests/golden/overlap_golden.npz by running the REFERENCE's own overlap report (scripts/analysis_runner.py:
overlap_report, its stdout captured) on seeded clouds, next to the exact numbers of the same NearestNeighbors(kd_tree) + numpy calls.

usage: python tests/golden/make_overlap_golden.py <reference checkout>

Only runs where a reference checkout exists; the fixture travels, the reference does not."""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
from sklearn.neighbors import NearestNeighbors

sys.path.insert(0, os.path.join(sys.argv[1], "scripts"))
import analysis_runner as ar  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("n_est", "n_below_half", "n_below_one", "n_below_two", "median", "p90", "p99", "max", "frac_half", "frac_one", "frac_two")


def numbers(gt_xyz, est_xyz, voxelsize):
    """overlap_report's computation, value by value"""
    d, _ = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(gt_xyz).kneighbors(est_xyz)
    d = d.reshape(-1)
    half, one = 0.5 * voxelsize, voxelsize
    return [len(d), np.sum(d < half), np.sum(d < one), np.sum(d < 2 * one), np.median(d), np.percentile(d, 90), np.percentile(d, 99),
            d.max(), np.mean(d < half) * 100, np.mean(d < one) * 100, np.mean(d < 2 * one) * 100]


def yaw(xyz, deg, t, centre=(0.0, 0.0, 0.0)):
    """rotated by `deg` about the vertical through `centre`, then moved by t"""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    o = np.asarray(centre)
    return ((xyz.astype(np.float64) - o) @ R.T + o + np.asarray(t)).astype(np.float32)


def street(rng, n, origin=(0.0, 0.0, 0.0)):
    """a ground plane with a few walls and poles, 60 m x 20 m"""
    g = rng.uniform([-30, -10, -0.05], [30, 10, 0.05], (n, 3))
    w = rng.uniform(size=n) < 0.35
    g[w, 1] = np.where(rng.uniform(size=w.sum()) < 0.5, -10.0, 10.0) + rng.normal(0, 0.02, w.sum())
    g[w, 2] = rng.uniform(0, 4, w.sum())
    return (g + np.asarray(origin)).astype(np.float32)


def main():
    rng = np.random.default_rng(20261015)
    cases = []
    gt = street(rng, 3001)
    cases.append(("aligned_3cm", gt, (gt[::2] + rng.normal(0, 0.03, (1501, 3))).astype(np.float32), 0.2))
    gt = street(rng, 3000)
    cases.append(("misaligned_0.35m_1.5deg", gt, yaw(gt[1::2] + rng.normal(0, 0.02, (1500, 3)).astype(np.float32), 1.5, (0.35, 0.0, 0.0)), 0.2))
    gt = street(rng, 2800)
    est = (gt[:2400] + rng.normal(0, 0.03, (2400, 3))).astype(np.float32)
    out = rng.choice(2400, 24, replace=False)  # 1 % outliers, 50 - 5000 m from the street
    dirs = rng.normal(size=(24, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    est[out] = (gt[out] + dirs * np.exp(rng.uniform(np.log(50), np.log(5000), (24, 1)))).astype(np.float32)
    cases.append(("outliers_1pct", gt, est, 0.2))
    gt = street(rng, 2000)
    gt = np.concatenate([gt, gt[:300]])  # exact duplicates in the GT
    est = (gt[500:1700] + rng.normal(0, 0.05, (1200, 3))).astype(np.float32)
    est[:400] = gt[:400]  # estimated points ON ground-truth points (d = 0), some of them on duplicates
    est = np.concatenate([est, est[:100]])  # and duplicates in the estimate
    cases.append(("duplicates_and_exact_hits", gt, est, 0.25))
    gt = street(rng, 2500, origin=(4.0e5, 5.0e6, 40.0))
    cases.append(("utm_scale", gt, yaw(gt[::3], 0.2, (0.1, -0.05, 0.0), (4.0e5, 5.0e6, 40.0)) + rng.normal(0, 0.02, (834, 3)).astype(np.float32), 0.2))
    gt = street(rng, 2000)
    cases.append(("even_n", gt, (gt[:1000] + rng.normal(0, 0.1, (1000, 3))).astype(np.float32), 0.1))
    gt = street(rng, 1500)
    cases.append(("single_estimate", gt, np.array([[1.0, 2.0, 0.5]], np.float32), 0.2))
    gt = rng.uniform([-20, -20, 0], [20, 20, 0], (2000, 3)).astype(np.float32)  # planar: every z is 0
    est = (gt[::2] + rng.normal(0, 0.1, (1000, 3))).astype(np.float32)
    est = np.concatenate([est, np.array([[0.0, 0.0, 3.0]], np.float32)])
    cases.append(("planar_gt", gt, est, 0.2))

    out = {}
    for k, (name, gt, est, vs) in enumerate(cases):
        buf = io.StringIO()
        with redirect_stdout(buf):
            ar.overlap_report(gt, est, voxelsize=vs)
        out["name%d" % k] = np.array(name)
        out["gt%d" % k] = np.concatenate([gt, np.full((len(gt), 1), 40.0, np.float32)], 1)
        out["est%d" % k] = np.concatenate([est, np.full((len(est), 1), 40.0, np.float32)], 1)
        out["vs%d" % k] = np.float64(vs)
        out["res%d" % k] = np.array(numbers(gt, est, vs), np.float64)
        out["text%d" % k] = np.array(buf.getvalue())
        print(name, len(gt), len(est))
        print(buf.getvalue(), end="")
    out["n_cases"] = np.int64(len(cases))
    out["fields"] = np.array(FIELDS)
    np.savez_compressed(os.path.join(HERE, "overlap_golden.npz"), **out)


if __name__ == "__main__":
    main()
