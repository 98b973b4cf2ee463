#!/usr/bin/env python3
"""Timing of the k nearest neighbours, the radius counts and the density filters (MEASUREMENTS.md, "Density") on the bench's synthetic
seq-05 map, voxelised at 0.2 m.

  python tools/knn_bench.py [--spacing 0.2] [--length 1000] [--k 16] [--radius 0.5] [--runs 5] [--no-host] [--out FILE.json]

On the one cloud:
  (a) Erasor.knn (scores only, then with the neighbour lists), Erasor.radius_count and Erasor.density_filter (mean / MAD, and count): median
      wall time of --runs calls after a warm-up call (the cloud on the host: the copy is in the time), knn again from a device buffer, and
      the device time per kernel group from the library's event brackets (Erasor.profiling) in a second set of calls -- kn_query is the
      search, ov_tree the tree, ov_select the order statistics;
  (b) evalmap.knn, evalmap.radius_count and evalmap.density_filter, the host restatement (cKDTree proposes, the float64 predicate decides),
      wall time, and the device results compared with them byte for byte;
  (c) Erasor.cluster at --radius on the same cloud, for scale.
The k class's workgroups per CU are arithmetic, not a measurement: 163 840 B of LDS per CU over 128 * (KC * 12 + 104) B per workgroup.
--no-host skips (b) (for a run under a profiler)."""
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


def same(a, b):
    return bool(np.asarray(a).tobytes() == np.asarray(b).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--length", type=float, default=1000.0)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    erasor_amd.build()
    w = synth.World(seed=20210305 + 5, length=a.length, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    raw = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2)), np.float32)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    cloud = np.ascontiguousarray(g.voxelize_preserving_labels(raw, 0.2), np.float32)
    kc = 8 if a.k <= 8 else (16 if a.k <= 16 else 32)
    lds = 128 * (kc * 12 + 104)
    row = {"spacing": a.spacing, "length": a.length, "k": a.k, "radius": a.radius, "raw_points": int(len(raw)), "points": int(len(cloud)),
           "list_class": kc, "lds_bytes_per_workgroup": lds, "workgroups_per_cu_by_lds": 163840 // lds}
    out = {}
    calls = {
        "knn": lambda: out.__setitem__("knn", g.knn(cloud, a.k)),
        "knn_with_lists": lambda: out.__setitem__("knn_l", g.knn(cloud, a.k, True)),
        "radius_count": lambda: out.__setitem__("rc", g.radius_count(cloud, a.radius)),
        "density_filter_mean_mad": lambda: out.__setitem__("sor", g.density_filter(cloud, "mean", k=a.k, rule="mad", mul=2.0)),
        "density_filter_count": lambda: out.__setitem__("ror", g.density_filter(cloud, "count", radius=a.radius, min_neighbors=3)),
        "cluster": lambda: out.__setitem__("cl", g.cluster(cloud, a.radius)),
    }
    for name, fn in calls.items():
        row["a_" + name + "_wall_ms"] = median_ms(fn, a.runs)
        g.profiling(1)
        g.profile_reset()
        for _ in range(a.runs):
            fn()
        row["a_" + name + "_device_ms_per_kernel"] = {k: v[0] / a.runs for k, v in g.profile_get().items()}
        g.profiling(0)
    p = g.device_array(cloud)
    row["a_knn_device_input_wall_ms"] = median_ms(lambda: g.knn((p, len(cloud)), a.k), a.runs)
    g.device_free(p)
    row["knn_result"] = {k: out["knn"][k] for k in ("n_points", "n_short", "kth_stats", "mean_stats")}
    row["density_filter_mean_mad_result"] = out["sor"][2]
    row["density_filter_count_result"] = out["ror"][2]
    if not a.no_host:
        t0 = time.perf_counter()
        ref = evalmap.knn(cloud, a.k, True)
        row["b_host_knn_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["knn_equal_to_host"] = all(same(out["knn_l"][k], ref[k]) for k in ("kth", "mean", "nbr_idx", "nbr_dist")) and same(out["knn"]["kth"], ref["kth"])
        t0 = time.perf_counter()
        ref = evalmap.radius_count(cloud, a.radius)
        row["b_host_radius_count_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["radius_count_equal_to_host"] = same(out["rc"][0], ref[0]) and str(out["rc"][1]) == str(ref[1])
        t0 = time.perf_counter()
        ref = evalmap.density_filter(cloud, "mean", k=a.k, rule="mad", mul=2.0)
        row["b_host_density_filter_mean_mad_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["density_filter_equal_to_host"] = same(out["sor"][0], ref[0]) and same(out["sor"][1], ref[1]) and str(out["sor"][2]) == str(ref[2])
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
