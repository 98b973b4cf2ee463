#!/usr/bin/env python3
"""Timing and scores of the free-space carving (MEASUREMENTS.md, "Carve") on the benchmark's config-2 world: the synthetic seq-05 street
with config/seq_05.yaml's parameters, its sampled map and the first --frames of its scans, cast as bench.py casts them.

  python tools/carve_bench.py [--frames 20,200] [--length 1000] [--spacing 0.2] [--az 2000] [--voxel 0.2] [--max-range 80] [--stop-short 0]
                              [--runs 3] [--host-points 20000] [--host-frames 2] [--host-stride 8] [--no-host] [--no-erasor] [--out FILE.json]

For every frame count, on the one input:
  (a) Erasor.carve at its defaults (map and scans on the host: the copies in and the copy of the outputs back are in the time): the
      median wall time of --runs calls after a warm-up call, and the device time per kernel group from the library's event brackets
      (Erasor.profiling) in a second set of calls -- cv_claim, cv_slots, cv_scan, cv_base and cv_fill the block table and the voxels'
      start (once a call), cv_walk and cv_integrate the two launches of every batch of 32 frames, cv_gather and cv_keep the points'
      fate and the compaction -- and from cv_walk's time the rays and the voxel steps per second;
  (b) Erasor.visibility at its defaults (1024 x 64, k = 0) on the same input in the same run: its wall time;
  (c) PR / RR / F1 (Erasor.evaluate against the labelled map itself) of carve's kept cloud, of visibility's, of the untouched map and,
      unless --no-erasor, of the map an ERASOR run over the same scans leaves;
  (d) unless --no-host, evalmap.carve, the normative host text, on a cut-down input (every n-th map point up to --host-points, every
      --host-stride-th point of the first --host-frames frames): wall time, the device's time on the same input, and the outputs
      compared byte for byte.
Nothing is gated: these are recorded numbers."""
import argparse
import json
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import erasor_amd  # noqa: E402
from erasor_amd import evalmap, synth  # noqa: E402

_CAST = None


def _cast_init(world, lidar, poses):
    global _CAST
    _CAST = (world, lidar, poses)


def _cast_one(k):
    world, lidar, poses = _CAST
    return world.cast(poses[k], lidar, k)


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


def rates(r):
    return {k: r[k] for k in ("PR", "RR", "F1", "gt_static", "gt_dynamic", "preserved_static", "preserved_dynamic")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="20,200")
    ap.add_argument("--length", type=float, default=1000.0)
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--az", type=int, default=2000)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--max-range", type=float, default=80.0)
    ap.add_argument("--stop-short", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=20000)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--host-stride", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-erasor", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    counts = sorted(int(v) for v in a.frames.split(","))
    erasor_amd.build()
    # the world, its map and its scans: on the host, before anything opens the device (the casting workers are fresh interpreters)
    w = synth.World(seed=20210305 + 5, length=a.length, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    lid = synth.Lidar.hdl64(a.az)
    jr = np.random.default_rng(1234)
    poses = [w.pose(k, 1.0, x0=300.0, jitter_rng=jr) for k in range(counts[-1])]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(min(16, len(poses)), initializer=_cast_init, initargs=(w, lid, poses)) as pool:
        scans = [np.ascontiguousarray(s, np.float32) for s in pool.map(_cast_one, range(len(poses)))]
    t_cast = time.perf_counter() - t0
    m = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2), step=1.0), np.float32)
    Tl = erasor_amd.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    Tb = [erasor_amd.geopose2eigen(p7) for p7 in poses]
    grid = erasor_amd.visibility_grid(1024, 64, -24.8, 2.0)  # an HDL-64E's field of view
    kw = dict(voxel=a.voxel, max_range=a.max_range, stop_short=a.stop_short)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    rows_out = []
    head = {"length": a.length, "spacing": a.spacing, "az": a.az, "map_points": int(len(m)), "runs": a.runs, "cast_s": t_cast, "min_range": 0.5,
            "logodds": evalmap.carve_logodds(), **kw}
    untouched = rates(g.evaluate(m, m))
    for n in counts:
        sc, T = scans[:n], np.stack([np.asarray(t, np.float32).reshape(4, 4) for t in Tb[:n]])
        row = dict(head, frames=n, scan_points=int(sum(len(s) for s in sc)), untouched_map=untouched)
        out = {}
        call = lambda: out.__setitem__("carve", g.carve(sc, T, Tl, m, **kw))
        row["a_wall_ms"] = median_ms(call, a.runs)
        g.profiling(1)
        g.profile_reset()
        for _ in range(a.runs):
            call()
        prof = {name: (v[0] / a.runs, v[1] / a.runs) for name, v in g.profile_get().items()}
        g.profiling(0)
        row["a_device_ms_per_kernel"] = {name: v[0] for name, v in prof.items()}
        row["a_launches"] = {name: v[1] for name, v in prof.items()}
        res = out["carve"][5]
        walk_s = prof.get("cv_walk", (float("nan"),))[0] / 1e3
        row["a_rays_per_s"], row["a_steps_per_s"] = res["n_rays"] / walk_s, res["n_steps"] / walk_s
        row["a_result"] = res
        row["c_carve_kept"] = rates(g.evaluate(m, out["carve"][3]))
        # (b) the see-through check on the same input
        row["b_visibility_wall_ms"] = median_ms(lambda: out.__setitem__("vis", g.visibility(sc, T, Tl, m, grid)), a.runs)
        row["b_visibility_result"] = out["vis"][4]
        row["c_visibility_kept"] = rates(g.evaluate(m, out["vis"][2]))
        both = out["carve"][2].astype(bool) & out["vis"][1].astype(bool)
        row["c_both_kept"] = rates(g.evaluate(m, np.ascontiguousarray(m[both])))
        # (c) an ERASOR run over the same scans
        if not a.no_erasor:
            p = erasor_amd.params_default()
            synth.apply_params(p, "05")
            e = erasor_amd.Erasor(p)
            e.set_map(m)
            t0 = time.perf_counter()
            for f in range(n):
                e.step(sc[f], Tl, Tb[f], erasor_amd.invert_rigid(Tb[f]))
            row["c_erasor_run_s"] = time.perf_counter() - t0
            est = np.ascontiguousarray(e.get_map(), np.float32)
            e.close()
            row["c_erasor"] = rates(g.evaluate(m, est))
            row["c_erasor_points"] = int(len(est))
        # (d) the normative text on a cut-down input
        if not a.no_host:
            cut = np.ascontiguousarray(m[:: max(1, len(m) // a.host_points)])
            hs, hT = [np.ascontiguousarray(s[:: a.host_stride]) for s in sc[: a.host_frames]], T[: a.host_frames]
            t0 = time.perf_counter()
            ref = evalmap.carve(cut, hs, hT, Tl, **kw)
            row["d_host_wall_ms"] = (time.perf_counter() - t0) * 1e3
            row["d_device_wall_ms"] = median_ms(lambda: out.__setitem__("cut", g.carve(hs, hT, Tl, cut, **kw)), a.runs)
            got = out["cut"]
            row["d_equal_to_host"] = all(same(got[j], ref[j]) for j in range(4)) and got[4] == ref[4] and got[5] == ref[5]
            row["d_host_points"], row["d_host_frames"], row["d_host_rays"], row["d_host_steps"] = int(len(cut)), len(hs), ref[5]["n_rays"], ref[5]["n_steps"]
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
