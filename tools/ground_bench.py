#!/usr/bin/env python3
"""Timing and scores of the ground segmentation (MEASUREMENTS.md, "Ground") on the benchmark's config-2 world: the synthetic seq-05 street
with config/seq_05.yaml's parameters, its sampled map and the first --frames of its scans, cast as bench.py casts them.

  python tools/ground_bench.py [--frames 20,200] [--length 1000] [--spacing 0.2] [--az 2000] [--rings 20] [--sectors 64] [--max-range 80]
                               [--runs 3] [--host-points 20000] [--host-frames 2] [--host-stride 8] [--no-host] [--out FILE.json]

For every frame count, on the one input:
  (a) Erasor.ground_scans and Erasor.ground_votes at their defaults (scans and map on the host: the copies in and the copy of the outputs
      back are in the time): the median wall time of --runs calls after a warm-up call, and the device time per kernel group from the
      library's event brackets (Erasor.profiling) in a second set of calls -- gr_key, gr_scan, gr_sort and the three gr_fit_* launches of
      every batch; gr_gather, gr_vote, gr_decide and gr_keep of the map form;
  (b) Erasor.visibility at its defaults (1024 x 64, k = 0) on the same input in the same run: its wall time -- the expectation is "about
      one visibility call at the same frame count";
  (c) the share of the map's LABEL_ROAD / LABEL_SIDEWALK points called ground, and of its other points, over the whole map and over the
      points that at least one frame judged;
  (d) PR / RR / F1 (Erasor.evaluate against the labelled map itself) of carve's kept cloud and of visibility's, and of the same with the
      ground points put back (removed & ~ground): what the mask is for;
  (e) unless --no-host, evalmap.ground_scans / ground_votes, the normative host text, on a cut-down input (every n-th map point up to
      --host-points, every --host-stride-th point of the first --host-frames frames): wall time, the device's time on the same input,
      and the outputs compared byte for byte.
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


def profiled(g, call, runs):
    g.profiling(1)
    g.profile_reset()
    for _ in range(runs):
        call()
    prof = {name: v[0] / runs for name, v in g.profile_get().items()}
    g.profiling(0)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="20,200")
    ap.add_argument("--length", type=float, default=1000.0)
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--az", type=int, default=2000)
    ap.add_argument("--rings", type=int, default=20)
    ap.add_argument("--sectors", type=int, default=64)
    ap.add_argument("--max-range", type=float, default=80.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-points", type=int, default=20000)
    ap.add_argument("--host-frames", type=int, default=2)
    ap.add_argument("--host-stride", type=int, default=8)
    ap.add_argument("--no-host", action="store_true")
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
    vgrid = erasor_amd.visibility_grid(1024, 64, -24.8, 2.0)  # an HDL-64E's field of view
    grid = erasor_amd.ground_grid(a.rings, a.sectors, 0.5, a.max_range)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    sem = evalmap._decode(m[:, 3])[0]
    flat = (sem == synth.LABEL_ROAD) | (sem == synth.LABEL_SIDEWALK)
    head = {"length": a.length, "spacing": a.spacing, "az": a.az, "map_points": int(len(m)), "map_road_or_sidewalk": int(flat.sum()), "runs": a.runs,
            "cast_s": t_cast, "rings": a.rings, "sectors": a.sectors, "min_range": 0.5, "max_range": a.max_range, **evalmap.GROUND_DEFAULTS}
    rows_out = []
    for n in counts:
        sc, T = scans[:n], np.stack([np.asarray(t, np.float32).reshape(4, 4) for t in Tb[:n]])
        row = dict(head, frames=n, scan_points=int(sum(len(s) for s in sc)))
        out = {}
        scans_call = lambda: out.__setitem__("scans", g.ground_scans(sc, grid))
        votes_call = lambda: out.__setitem__("votes", g.ground_votes(T, Tl, m, grid))
        row["a_scans_wall_ms"] = median_ms(scans_call, a.runs)
        row["a_scans_device_ms_per_kernel"] = profiled(g, scans_call, a.runs)
        row["a_scans_result"] = out["scans"][2]
        row["a_votes_wall_ms"] = median_ms(votes_call, a.runs)
        row["a_votes_device_ms_per_kernel"] = profiled(g, votes_call, a.runs)
        row["a_votes_result"] = out["votes"][4]
        ground = out["votes"][1].astype(bool)
        # (b) the see-through check on the same input
        row["b_visibility_wall_ms"] = median_ms(lambda: out.__setitem__("vis", g.visibility(sc, T, Tl, m, vgrid)), a.runs)
        # (c) what is called ground
        row["c_share_of_road_and_sidewalk_called_ground"] = float(ground[flat].mean()) if flat.any() else None
        row["c_share_of_other_points_called_ground"] = float(ground[~flat].mean()) if (~flat).any() else None
        seen = out["votes"][0][:, 0] > 0  # (most of a kilometre of map is in no frame's patches: the same shares among the points some frame judged)
        row["c_seen"] = int(seen.sum())
        row["c_share_of_seen_road_and_sidewalk_called_ground"] = float(ground[flat & seen].mean()) if (flat & seen).any() else None
        row["c_share_of_seen_other_points_called_ground"] = float(ground[~flat & seen].mean()) if (~flat & seen).any() else None
        # (d) the other analyses with and without the mask
        out["carve"] = g.carve(sc, T, Tl, m)
        for name, kept in (("carve", out["carve"][2].astype(bool)), ("visibility", out["vis"][1].astype(bool))):
            removed = ~kept
            row["d_%s_kept" % name] = rates(g.evaluate(m, np.ascontiguousarray(m[kept])))
            row["d_%s_kept_with_ground_put_back" % name] = rates(g.evaluate(m, np.ascontiguousarray(m[~(removed & ~ground)])))
            row["d_%s_removed" % name], row["d_%s_removed_and_not_ground" % name] = int(removed.sum()), int((removed & ~ground).sum())
        # (e) the normative text on a cut-down input
        if not a.no_host:
            cut = np.ascontiguousarray(m[:: max(1, len(m) // a.host_points)])
            hs, hT = [np.ascontiguousarray(s[:: a.host_stride]) for s in sc[: a.host_frames]], T[: a.host_frames]
            t0 = time.perf_counter()
            ref = evalmap.ground_scans(hs, grid, patches=True)
            row["e_host_scans_wall_ms"] = (time.perf_counter() - t0) * 1e3
            row["e_device_scans_wall_ms"] = median_ms(lambda: out.__setitem__("cut", g.ground_scans(hs, grid, patches=True)), a.runs)
            got = out["cut"]
            row["e_scans_equal_to_host"] = same(got[0], ref[0]) and got[1] == ref[1] and got[2] == ref[2] and same(got[3], ref[3])
            t0 = time.perf_counter()
            ref = evalmap.ground_votes(cut, hT, Tl, grid)
            row["e_host_votes_wall_ms"] = (time.perf_counter() - t0) * 1e3
            row["e_device_votes_wall_ms"] = median_ms(lambda: out.__setitem__("cutv", g.ground_votes(hT, Tl, cut, grid)), a.runs)
            got = out["cutv"]
            row["e_votes_equal_to_host"] = all(same(got[j], ref[j]) for j in range(3)) and got[3] == ref[3] and got[4] == ref[4]
            row["e_host_points"], row["e_host_frames"], row["e_host_scan_points"] = int(len(cut)), len(hs), int(sum(len(s) for s in hs))
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
