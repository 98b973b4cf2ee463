#!/usr/bin/env python3
"""Timing of the pose refinement (MEASUREMENTS.md, "Refine") on the bench's synthetic seq-05 world: scans cast from the world, their poses
put wrong by a known amount, refined against the sampled map.

  python tools/refine_bench.py [--spacing 0.2] [--length 400] [--frames 12] [--az 2000] [--iters 8] [--runs 3] [--host-frames 2] [--no-host]
                               [--plane] [--out FILE.json]

On the one input:
  (a) Erasor.refine_poses with its defaults: median wall time of --runs calls after a warm-up call (scans and map on the host: the copies
      are in the time), the statuses, the iterations, and the device time per kernel group from the library's event brackets
      (Erasor.profiling) in a second set of calls -- rf_query is the search and the chunk sums, rf_partials the second launch, ov_tree the
      tree;
  (b) the cost of one iteration: refine_poses held to exactly --iters and to exactly 1 iteration (eps so small that no frame stops), the
      difference divided by --iters - 1, beside Erasor.align_frames on the same scans, poses and map in the same run (one iteration searches
      what one align_frames searches);
  (c) evalmap.refine_poses, the host restatement, on the first --host-frames frames: wall time, and the device result on those frames
      compared with it byte for byte.
--no-host skips (c) (for a run under a profiler).
  (d) with --plane, Erasor.refine_poses_plane on the same input in the same run, beside the rows above: the wall time at its defaults, the
      iterations, ranks and statuses, the translation errors and frac_half after it; the call held to exactly --iters and to 1 iteration
      and the cost of one iteration from their difference; rfp_query per launch, rfp_partials and the one-off normals pass (nm_query) from
      the event brackets.  Its host restatement is not run here: evalmap.normals over the whole map is minutes of numpy."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import erasor_amd  # noqa: E402
from erasor_amd import evalmap, synth  # noqa: E402


def median_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def wrong_by(T, rng, max_t, max_deg):
    """T (16 float32, row-major) with a rotation of up to max_deg about a random axis and a shift of up to max_t in front of it"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = np.radians(max_deg) * rng.uniform(0.5, 1.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    dt = rng.normal(size=3)
    E[:3, 3] = dt * max_t * rng.uniform(0.5, 1.0) / np.linalg.norm(dt)
    E[:3, 3] += T[:3, 3] - E[:3, :3] @ T[:3, 3]  # (the rotation about the sensor, not about the origin)
    return (E @ T).astype(np.float32)


def same(a, b):
    return bool(np.asarray(a).tobytes() == np.asarray(b).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--length", type=float, default=400.0)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--az", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--plane", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    erasor_amd.build()
    w = synth.World(seed=20210305 + 5, length=a.length, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    lid = synth.Lidar.hdl64(a.az)
    m = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2)), np.float32)
    Tl = erasor_amd.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    jr, er = np.random.default_rng(7), np.random.default_rng(8)
    scans, T_true, T_given = [], [], []
    for k in range(a.frames):
        p7 = w.pose(k * 3, 1.0, x0=min(300.0, a.length / 2), jitter_rng=jr)
        T_true.append(erasor_amd.geopose2eigen(p7))
        T_given.append(wrong_by(T_true[-1], er, 0.3, 1.0))
        scans.append(np.ascontiguousarray(w.cast(p7, lid, k * 3), np.float32))
    g = erasor_amd.Erasor(erasor_amd.params_default())
    g.set_map(m)
    row = {"spacing": a.spacing, "length": a.length, "map_points": int(len(m)), "frames": a.frames, "scan_points": int(sum(len(s) for s in scans))}
    out = {}
    # (a) the call as a user makes it
    row["a_refine_wall_ms"] = median_ms(lambda: out.__setitem__("r", g.refine_poses(scans, T_given, Tl)), a.runs)
    g.profiling(1)
    g.profile_reset()
    for _ in range(a.runs):
        g.refine_poses(scans, T_given, Tl)
    row["a_refine_device_ms_per_kernel"] = {k: v[0] / a.runs for k, v in g.profile_get().items()}
    g.profiling(0)
    T, rows, summ = out["r"]
    row["a_summary"] = summ
    row["a_iters"] = [r["iters"] for r in rows]
    err0 = [float(np.linalg.norm(np.asarray(T_given[f], np.float64).reshape(4, 4)[:3, 3] - np.asarray(T_true[f], np.float64).reshape(4, 4)[:3, 3]))
            for f in range(a.frames)]
    err1 = [float(np.linalg.norm(T[f][:3, 3] - np.asarray(T_true[f], np.float64).reshape(4, 4)[:3, 3])) for f in range(a.frames)]
    row["a_translation_error_m_given_median_max"] = [float(np.median(err0)), float(np.max(err0))]
    row["a_translation_error_m_refined_median_max"] = [float(np.median(err1)), float(np.max(err1))]
    before, _ = g.align_frames(scans, T_given, Tl)
    after, _ = g.align_frames(scans, T.astype(np.float32), Tl)
    row["a_frac_half_before_min_median"] = [float(np.min([r["frac_half"] for r in before])), float(np.median([r["frac_half"] for r in before]))]
    row["a_frac_half_after_min_median"] = [float(np.min([r["frac_half"] for r in after])), float(np.median([r["frac_half"] for r in after]))]
    # (b) one iteration against one align_frames
    tiny = dict(eps_t=1e-300, eps_r=1e-300)
    t_n = median_ms(lambda: out.__setitem__("n", g.refine_poses(scans, T_given, Tl, max_iters=a.iters, **tiny)), a.runs)
    t_1 = median_ms(lambda: g.refine_poses(scans, T_given, Tl, max_iters=1, **tiny), a.runs)
    t_al = median_ms(lambda: g.align_frames(scans, T_given, Tl), a.runs)
    assert all(r["iters"] == a.iters for r in out["n"][1] if r["status"] == 1)
    row["b_refine_%d_iters_wall_ms" % a.iters] = t_n
    row["b_refine_1_iter_wall_ms"] = t_1
    row["b_align_frames_wall_ms"] = t_al
    row["b_ms_per_iteration"] = (t_n[0] - t_1[0]) / max(a.iters - 1, 1)
    row["b_iteration_over_align_frames"] = row["b_ms_per_iteration"] / t_al[0]
    # the two query kernels alone, by the event brackets: --iters + 1 launches of rf_query (the last evaluates) against one al_query
    g.profiling(1)
    g.profile_reset()
    g.refine_poses(scans, T_given, Tl, max_iters=a.iters, **tiny)
    prof_r = {k: v[0] for k, v in g.profile_get().items()}
    g.profile_reset()
    g.align_frames(scans, T_given, Tl)
    prof_a = {k: v[0] for k, v in g.profile_get().items()}
    g.profiling(0)
    row["b_rf_query_device_ms_per_launch"] = prof_r.get("rf_query", 0.0) / (a.iters + 1)
    row["b_rf_partials_device_ms_per_launch"] = prof_r.get("rf_partials", 0.0) / (a.iters + 1)
    row["b_al_query_device_ms"] = prof_a.get("al_query", 0.0)
    row["b_align_device_ms_per_kernel"] = prof_a
    # (c) the host restatement
    if not a.no_host and a.host_frames > 0:
        sub = list(range(min(a.host_frames, a.frames)))
        dev = g.refine_poses([scans[f] for f in sub], [T_given[f] for f in sub], Tl)
        t0 = time.perf_counter()
        ref = evalmap.refine_poses(m[:, :3], [scans[f] for f in sub], [T_given[f] for f in sub], Tl)
        row["c_host_frames"] = len(sub)
        row["c_host_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["c_device_wall_ms_same_frames"] = median_ms(lambda: g.refine_poses([scans[f] for f in sub], [T_given[f] for f in sub], Tl), a.runs)
        row["c_equal_to_host"] = same(dev[0], ref[0]) and str(dev[1]) == str(ref[1]) and str(dev[2]) == str(ref[2])
    # (d) point-to-plane on the same input
    if a.plane:
        row["d_plane_wall_ms"] = median_ms(lambda: out.__setitem__("p", g.refine_poses_plane(scans, T_given, Tl)), a.runs)
        Tp, prows, psumm = out["p"]
        row["d_summary"] = psumm
        row["d_iters"] = [r["iters"] for r in prows]
        row["d_rank"] = [r["rank"] for r in prows]
        row["d_lambda_ratio_min"] = float(np.min([r["lambda_ratio"] for r in prows]))
        row["d_rms_plane_last_median"] = float(np.median([r["rms_plane_last"] for r in prows]))
        err2 = [float(np.linalg.norm(Tp[f][:3, 3] - np.asarray(T_true[f], np.float64).reshape(4, 4)[:3, 3])) for f in range(a.frames)]
        row["d_translation_error_m_refined_median_max"] = [float(np.median(err2)), float(np.max(err2))]
        after_p, _ = g.align_frames(scans, Tp.astype(np.float32), Tl)
        row["d_frac_half_after_min_median"] = [float(np.min([r["frac_half"] for r in after_p])), float(np.median([r["frac_half"] for r in after_p]))]
        p_n = median_ms(lambda: out.__setitem__("pn", g.refine_poses_plane(scans, T_given, Tl, max_iters=a.iters, **tiny)), a.runs)
        p_1 = median_ms(lambda: g.refine_poses_plane(scans, T_given, Tl, max_iters=1, **tiny), a.runs)
        assert all(r["iters"] == a.iters for r in out["pn"][1] if r["status"] == 1)
        row["d_plane_%d_iters_wall_ms" % a.iters] = p_n
        row["d_plane_1_iter_wall_ms"] = p_1
        row["d_ms_per_iteration"] = (p_n[0] - p_1[0]) / max(a.iters - 1, 1)
        row["d_iteration_over_point_to_point"] = row["d_ms_per_iteration"] / row["b_ms_per_iteration"]
        row["d_wall_over_point_to_point"] = row["d_plane_wall_ms"][0] / row["a_refine_wall_ms"][0]
        g.profiling(1)
        g.profile_reset()
        g.refine_poses_plane(scans, T_given, Tl, max_iters=a.iters, **tiny)
        prof_p = {k: v[0] for k, v in g.profile_get().items()}
        g.profiling(0)
        row["d_rfp_query_device_ms_per_launch"] = prof_p.get("rfp_query", 0.0) / (a.iters + 1)
        row["d_rfp_partials_device_ms_per_launch"] = prof_p.get("rfp_partials", 0.0) / (a.iters + 1)
        row["d_nm_query_device_ms"] = prof_p.get("nm_query", 0.0)
        row["d_rfp_query_over_rf_query"] = row["d_rfp_query_device_ms_per_launch"] / max(row["b_rf_query_device_ms_per_launch"], 1e-9)
        row["d_plane_device_ms_per_kernel"] = prof_p
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
