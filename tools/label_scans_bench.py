#!/usr/bin/env python3
"""Timing of the scans' labelling (MEASUREMENTS.md, "Labelling the scans") on the bench's config-2 map and its scans.

  python tools/label_scans_bench.py [--spacing 0.2] [--frames 24] [--host-frames 4] [--runs 5] [--no-host] [--out FILE.json]

The cleaned map is the map's points with a static label (what a perfect run leaves), the raw map is the whole map.  Per run:
  (a) Erasor.label_scans of all frames against the cleaned map, without and with the raw map: median wall time of --runs calls after a
      warm-up call (maps and scans on the host: the copies are in the time), and the device time per kernel group from the library's
      event brackets (Erasor.profiling) in a second set of calls;
  (b) Erasor.align_frames on the same input against the cleaned map: what getting the same decision from exact distances costs (the
      exact nearest-neighbour search per point, plus the report's selects);
  (c) evalmap.label_scans, the host oracle (cKDTree on every host core), on the first --host-frames frames, wall time, and the device
      result of those frames compared with it byte for byte.
--no-host skips (c) (for a run under a profiler)."""
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
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    erasor_amd.build()
    w = synth.World(seed=20210305 + 5, length=1000.0, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    raw = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2)), np.float32)
    static = np.ascontiguousarray(raw[~np.isin(evalmap.labels(raw[:, 3]), evalmap.DYNAMIC_CLASSES)])
    lid = synth.Lidar.hdl64(2000)
    Tl = erasor_amd.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    jr = np.random.default_rng(7)
    scans, Tb = [], []
    for k in range(a.frames):
        p7 = w.pose(k * 3, 1.0, x0=300.0, jitter_rng=jr)
        Tb.append(erasor_amd.geopose2eigen(p7))
        scans.append(np.ascontiguousarray(w.cast(p7, lid, k * 3), np.float32))
    p = erasor_amd.params_default()
    synth.apply_params(p, "05", max_range=80.0, num_rings=20, num_sectors=108)
    g = erasor_amd.Erasor(p)
    tau = evalmap.label_tau(0.2)
    row = {"spacing": a.spacing, "static_points": int(len(static)), "raw_points": int(len(raw)), "frames": a.frames,
           "scan_points": int(sum(len(s) for s in scans)), "tau": tau}
    out = {}

    def call(with_raw):
        out[with_raw] = g.label_scans(scans, Tb, Tl, static_map=static, raw_map=raw if with_raw else None, tau=tau)

    row["a_label_scans_wall_ms"] = median_ms(lambda: call(False), a.runs)
    row["a_label_scans_raw_wall_ms"] = median_ms(lambda: call(True), a.runs)
    row["summary"], row["summary_raw"] = out[False][2], out[True][2]
    row["moving"] = evalmap.moving_iou(out[True][2])
    row["b_align_frames_wall_ms"] = median_ms(lambda: g.align_frames(scans, Tb, Tl, map=static, voxelsize=0.2), a.runs)
    g.profiling(1)
    g.profile_reset()
    for _ in range(a.runs):
        call(True)
        g.align_frames(scans, Tb, Tl, map=static, voxelsize=0.2)
    row["device_ms_per_kernel"] = {k: v[0] / a.runs for k, v in g.profile_get().items() if k.startswith(("ls_", "al_", "ov_"))}
    g.profiling(0)
    if not a.no_host:
        nh = min(a.host_frames, a.frames)
        t0 = time.perf_counter()
        ref = evalmap.label_scans(static[:, :3], scans[:nh], Tb[:nh], Tl, raw_xyz=raw[:, :3], tau=tau)
        row["c_host_oracle_wall_ms"] = (time.perf_counter() - t0) * 1e3
        row["c_host_frames"], row["c_host_scan_points"] = nh, int(sum(len(s) for s in scans[:nh]))
        row["equal_to_host"] = all(x.tobytes() == y.tobytes() for x, y in zip(out[True][0][:nh], ref[0])) and out[True][1][:nh] == ref[1]
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
