#!/usr/bin/env python3
"""Timing of the surface normals (MEASUREMENTS.md, "Normals") against the k nearest neighbours at the same k on the same cloud: the
bench's synthetic seq-05 map, voxelised at 0.2 m, as tools/knn_bench.py takes it.

  python tools/normals_bench.py [--spacing 0.2] [--length 1000] [--k 16] [--runs 7] [--no-host] [--out FILE.json]

On the one cloud:
  (a) Erasor.normals (normals and curvature; then with the eigenvalues; then towards a viewpoint) and Erasor.knn (scores only): after a
      warm-up call of each, --runs rounds that alternate the calls, each timed by the host clock around the call -- every call ends in
      the device-to-host copy of its results, a synchronise -- and the median, smallest and largest per call.  The cloud is on the host:
      the copy in is in both times.  normals again from a device buffer;
  (b) the device time per kernel group from the library's event brackets (Erasor.profiling) in a second set of calls: nm_query is the
      search with its finishing pass, kn_query knn's search, ov_tree the tree both build, ov_select the order statistics (one score for
      normals, two for knn);
  (c) evalmap.normals, the host restatement (cKDTree proposes, the float64 predicate decides, numpy does the arithmetic): wall time, and
      the device results compared with it byte for byte.
The expectation is knn's time plus a finishing pass; the ratio is printed, not gated.  --no-host skips (c)."""
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


def alternating_ms(calls, runs):
    """every call once to warm up, then `runs` rounds in turn: {name: (median, min, max)} in ms"""
    for fn in calls.values():
        fn()
    t = {name: [] for name in calls}
    for _ in range(runs):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            t[name].append((time.perf_counter() - t0) * 1e3)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in t.items()}


def same(a, b):
    return bool(np.asarray(a).tobytes() == np.asarray(b).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--length", type=float, default=1000.0)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    erasor_amd.build()
    w = synth.World(seed=20210305 + 5, length=a.length, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    raw = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2)), np.float32)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    cloud = np.ascontiguousarray(g.voxelize_preserving_labels(raw, 0.2), np.float32)
    view = (float(cloud[:, 0].mean()), float(cloud[:, 1].mean()), float(cloud[:, 2].max()) + 10.0)
    kc = 8 if a.k <= 8 else (16 if a.k <= 16 else 32)
    lds = 128 * (kc * 12 + 104)
    row = {"spacing": a.spacing, "length": a.length, "k": a.k, "runs": a.runs, "raw_points": int(len(raw)), "points": int(len(cloud)), "list_class": kc,
           "lds_bytes_per_workgroup": lds, "workgroups_per_cu_by_lds": 163840 // lds}
    out = {}
    calls = {
        "knn": lambda: out.__setitem__("knn", g.knn(cloud, a.k)),
        "normals": lambda: out.__setitem__("nm", g.normals(cloud, a.k)),
        "normals_with_eigenvalues": lambda: out.__setitem__("nm_e", g.normals(cloud, a.k, eigenvalues=True)),
        "normals_towards_a_viewpoint": lambda: out.__setitem__("nm_v", g.normals(cloud, a.k, view)),
    }
    for name, t in alternating_ms(calls, a.runs).items():
        row["a_" + name + "_wall_ms"] = t
    row["a_normals_over_knn"] = row["a_normals_wall_ms"][0] / row["a_knn_wall_ms"][0]
    p = g.device_array(cloud)
    dev = {"knn": lambda: g.knn((p, len(cloud)), a.k), "normals": lambda: g.normals((p, len(cloud)), a.k)}
    for name, t in alternating_ms(dev, a.runs).items():
        row["a_" + name + "_device_input_wall_ms"] = t
    g.device_free(p)
    for name in ("knn", "normals"):
        g.profiling(1)
        g.profile_reset()
        for _ in range(a.runs):
            calls[name]()
        row["b_" + name + "_device_ms_per_kernel"] = {k: v[0] / a.runs for k, v in g.profile_get().items()}
        g.profiling(0)
    row["b_nm_query_over_kn_query"] = row["b_normals_device_ms_per_kernel"].get("nm_query", float("nan")) / row["b_knn_device_ms_per_kernel"].get(
        "kn_query", float("nan"))
    row["normals_result"] = out["nm"][3]
    if not a.no_host:
        t0 = time.perf_counter()
        ref = evalmap.normals(cloud, a.k)
        row["c_host_normals_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["normals_equal_to_host"] = all(same(out["nm_e"][j], ref[j]) for j in range(3)) and same(out["nm"][0], ref[0]) and str(out["nm"][3]) == str(ref[3])
        refv = evalmap.normals(cloud, a.k, view)
        row["normals_towards_a_viewpoint_equal_to_host"] = same(out["nm_v"][0], refv[0]) and same(out["nm_v"][1], refv[1]) and str(out["nm_v"][3]) == str(refv[3])
        row["c_host_over_device"] = row["c_host_normals_wall_ms"] / row["a_normals_wall_ms"][0]
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
