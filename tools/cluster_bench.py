#!/usr/bin/env python3
"""Timing of the Euclidean clustering (MEASUREMENTS.md, "Clustering") on the bench's synthetic seq-05 map.

  python tools/cluster_bench.py [--spacing 0.2] [--length 1000] [--tol 0.5] [--runs 5] [--no-host] [--out FILE.json]

Two inputs, both at --tol: (dyn) the map's dynamic points, the moving objects' trails; (map) the whole map voxelised at 0.2 m.  Per input:
  (a) Erasor.cluster with the ids: median wall time of --runs calls after a warm-up call (the cloud on the host: the copy is in the
      time), the same from a device buffer, and the device time per kernel group from the library's event brackets (Erasor.profiling)
      in a second set of calls -- cl_unite's share of it is the unite pass;
  (b) evalmap.cluster, the host restatement (cKDTree.query_pairs, the predicate in numpy, connected_components), wall time, and the
      device result compared with it byte for byte.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--length", type=float, default=1000.0)
    ap.add_argument("--tol", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    erasor_amd.build()
    w = synth.World(seed=20210305 + 5, length=a.length, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    raw = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2)), np.float32)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    inputs = {"dyn": np.ascontiguousarray(raw[np.isin(evalmap.labels(raw[:, 3]), evalmap.DYNAMIC_CLASSES)]),
              "map": np.ascontiguousarray(g.voxelize_preserving_labels(raw, 0.2), np.float32)}
    row = {"spacing": a.spacing, "length": a.length, "tol": a.tol, "raw_points": int(len(raw))}
    for name, cloud in inputs.items():
        out = {}

        def call(c=cloud):
            out["r"] = g.cluster(c, a.tol)

        r = {"points": int(len(cloud))}
        r["a_cluster_wall_ms"] = median_ms(call, a.runs)
        p = g.device_array(cloud)
        r["a_cluster_device_input_wall_ms"] = median_ms(lambda: g.cluster((p, len(cloud)), a.tol), a.runs)
        g.device_free(p)
        r["result"] = out["r"][3]
        g.profiling(1)
        g.profile_reset()
        for _ in range(a.runs):
            call()
        dev = {k: v[0] / a.runs for k, v in g.profile_get().items() if k.startswith("cl_")}
        g.profiling(0)
        r["device_ms_per_kernel"] = dev
        r["unite_share"] = dev.get("cl_unite", 0.0) / max(sum(dev.values()), 1e-12)
        if not a.no_host:
            t0 = time.perf_counter()
            ref = evalmap.cluster(cloud, a.tol)
            r["b_host_restatement_wall_ms"] = (time.perf_counter() - t0) * 1e3
            r["equal_to_host"] = bool(out["r"][3] == ref[3] and out["r"][0].tobytes() == ref[0].tobytes() and out["r"][1].tobytes() == ref[1].tobytes())
        row[name] = r
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
