#!/usr/bin/env python3
"""Timing and scores of the see-through check (MEASUREMENTS.md, "Visibility") on the benchmark's config-2 world: the synthetic seq-05
street with config/seq_05.yaml's parameters, its sampled map and the first --frames of its scans, cast as bench.py casts them.

  python tools/visibility_bench.py [--frames 20,200] [--length 1000] [--spacing 0.2] [--az 2000] [--width 1024] [--height 64] [--k 0,16]
                                   [--runs 3] [--host-points 20000] [--host-frames 4] [--no-host] [--no-erasor] [--out FILE.json]

For every frame count, on the one input:
  (a) Erasor.visibility at its defaults (map and scans on the host: the copies in and the copy of the outputs back are in the time),
      for every k of --k: the median wall time of --runs calls after a warm-up call, and the device time per kernel group from the
      library's event brackets (Erasor.profiling) in a second set of calls -- vis_image the range images, vis_vote the votes,
      vis_decide and vis_keep the decision and the compaction, nm_query and ov_tree the one-off normals pass (k > 0);
  (b) Erasor.align_frames on the same scans, poses and map in the same run: its wall time and al_query per frame beside vis_vote per
      frame (the vote does no tree walk);
  (c) PR / RR / F1 (Erasor.evaluate against the labelled map itself) of the kept cloud, of the untouched map and, unless --no-erasor, of
      the map an ERASOR run over the same scans leaves;
  (d) unless --no-host, evalmap.visibility, the normative host text, on a cut-down input (every n-th map point up to --host-points,
      the first --host-frames frames): wall time, the device's time on the same input, and the outputs compared byte for byte.
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
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--k", default="0,16")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=20000)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-erasor", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    counts = sorted(int(v) for v in a.frames.split(","))
    ks = [int(v) for v in a.k.split(",")]
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
    grid = erasor_amd.visibility_grid(a.width, a.height, -24.8, 2.0)  # an HDL-64E's field of view
    g = erasor_amd.Erasor(erasor_amd.params_default())
    rows_out = []
    head = {"length": a.length, "spacing": a.spacing, "az": a.az, "map_points": int(len(m)), "width": a.width, "height": a.height, "runs": a.runs,
            "cast_s": t_cast, "defaults": evalmap.VISIBILITY_DEFAULTS, "image_budget_bytes": erasor_amd.VISIBILITY_IMAGE_BUDGET}
    untouched = rates(g.evaluate(m, m))
    for n in counts:
        sc, T = scans[:n], np.stack([np.asarray(t, np.float32).reshape(4, 4) for t in Tb[:n]])
        row = dict(head, frames=n, scan_points=int(sum(len(s) for s in sc)), untouched_map=untouched)
        out = {}
        for k in ks:
            tag = "k%d" % k
            call = lambda: out.__setitem__(tag, g.visibility(sc, T, Tl, m, grid, k=k))
            row["a_%s_wall_ms" % tag] = median_ms(call, a.runs)
            g.profiling(1)
            g.profile_reset()
            for _ in range(a.runs):
                call()
            prof = {name: (v[0] / a.runs, v[1] / a.runs) for name, v in g.profile_get().items()}
            g.profiling(0)
            row["a_%s_device_ms_per_kernel" % tag] = {name: v[0] for name, v in prof.items()}
            row["a_%s_launches" % tag] = {name: v[1] for name, v in prof.items()}
            row["a_%s_vote_ms_per_frame" % tag] = prof.get("vis_vote", (float("nan"),))[0] / n
            row["a_%s_result" % tag] = out[tag][4]
            row["c_%s_kept" % tag] = rates(g.evaluate(m, out[tag][2]))
        # (b) align_frames on the same input
        row["b_align_wall_ms"] = median_ms(lambda: g.align_frames(sc, T, Tl, m), a.runs)
        g.profiling(1)
        g.profile_reset()
        for _ in range(a.runs):
            g.align_frames(sc, T, Tl, m)
        row["b_align_device_ms_per_kernel"] = {name: v[0] / a.runs for name, v in g.profile_get().items()}
        g.profiling(0)
        row["b_al_query_ms_per_frame"] = row["b_align_device_ms_per_kernel"].get("al_query", float("nan")) / n
        # (c) an ERASOR run over the same scans, and what both keep
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
            hs, hT = sc[: a.host_frames], T[: a.host_frames]
            for k in ks:
                t0 = time.perf_counter()
                ref = evalmap.visibility(cut, hs, hT, Tl, grid, k=k)
                row["d_k%d_host_wall_ms" % k] = (time.perf_counter() - t0) * 1e3
                row["d_k%d_device_wall_ms" % k] = median_ms(lambda: out.__setitem__("cut", g.visibility(hs, hT, Tl, cut, grid, k=k)), a.runs)
                got = out["cut"]
                row["d_k%d_equal_to_host" % k] = all(same(got[j], ref[j]) for j in range(3)) and got[3] == ref[3] and got[4] == ref[4]
            row["d_host_points"], row["d_host_frames"] = int(len(cut)), len(hs)
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
