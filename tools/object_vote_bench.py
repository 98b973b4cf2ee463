#!/usr/bin/env python3
"""Scores and timing of the decision per object (MEASUREMENTS.md, "Objects") on the benchmark's config-2 world: the synthetic seq-05
street with its sampled map and the first --frames of its scans, cast as bench.py casts them -- tools/carve_bench.py's and
tools/ground_bench.py's input.

  python tools/object_vote_bench.py [--frames 200] [--length 1000] [--spacing 0.2] [--az 2000] [--tols 0.3,0.5] [--ratios 0.3,0.5]
                                    [--max-size 0] [--runs 3] [--host-length 10] [--no-host] [--out FILE.json]

In one run: Erasor.visibility, Erasor.carve and Erasor.ground_votes at their defaults on the one input.  Then Erasor.object_vote with the
votes of each method alone and with their sum at vote_thr = 2 (both methods agree), each with and without the ground mask, at every
tolerance of --tols and every remove_ratio of --ratios (revert_ratio 0, the other parameters at their defaults).  For each:
  * PR / RR (Erasor.evaluate against the labelled map itself) before -- the per-point votes applied as they are -- and after;
  * the ghost objects Erasor.residue counts (tol 0.5) before and after;
  * n_grown_dynamic / n_grown and the result's other counts;
  * the wall time, map, votes and mask on the host, all copies included: the median of --runs calls after a warm-up call;
  * the device time per kernel group from the library's event brackets (Erasor.profiling) in one further call;
and, per tolerance, the wall time of Erasor.cluster on the same non-ground rows (and on all rows) in the same run: the expectation is
that a call costs about what that costs.  Unless --no-host, evalmap.object_vote, the normative host text, runs on a cut-down input (the
map's rows whose x lies within --host-length metres of the first pose) and every output is compared byte for byte.
The world is synthetic and noise-free: the scores say nothing about real data.  Nothing is gated: these are recorded numbers."""
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


def rates(r):
    return {k: r[k] for k in ("PR", "RR", "F1", "preserved_static", "preserved_dynamic")}


def profiled(g, call):
    g.profiling(1)
    g.profile_reset()
    call()
    prof = {name: v[0] for name, v in g.profile_get().items()}
    g.profiling(0)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--length", type=float, default=1000.0)
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--az", type=int, default=2000)
    ap.add_argument("--tols", default="0.3,0.5")
    ap.add_argument("--ratios", default="0.3,0.5")
    ap.add_argument("--max-size", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-length", type=float, default=10.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tols, ratios = [float(v) for v in a.tols.split(",")], [float(v) for v in a.ratios.split(",")]
    erasor_amd.build()
    # the world, its map and its scans: on the host, before anything opens the device (the casting workers are fresh interpreters)
    w = synth.World(seed=20210305 + 5, length=a.length, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    lid = synth.Lidar.hdl64(a.az)
    jr = np.random.default_rng(1234)
    poses = [w.pose(k, 1.0, x0=300.0, jitter_rng=jr) for k in range(a.frames)]
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(min(16, len(poses)), initializer=_cast_init, initargs=(w, lid, poses)) as pool:
        sc = [np.ascontiguousarray(s, np.float32) for s in pool.map(_cast_one, range(len(poses)))]
    t_cast = time.perf_counter() - t0
    m = np.ascontiguousarray(w.sample_map(spacing=a.spacing, frames=range(0, 320, 2), step=1.0), np.float32)
    Tl = erasor_amd.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    T = np.stack([np.asarray(erasor_amd.geopose2eigen(p7), np.float32).reshape(4, 4) for p7 in poses])
    g = erasor_amd.Erasor(erasor_amd.params_default())
    vis = g.visibility(sc, T, Tl, m, erasor_amd.visibility_grid(1024, 64, -24.8, 2.0))
    carve = g.carve(sc, T, Tl, m, keep=False)
    gv = g.ground_votes(T, Tl, m)
    ground = np.ascontiguousarray(gv[1], np.uint8)
    kept_masks = {"visibility": np.ascontiguousarray(vis[1], np.uint8), "carve": np.ascontiguousarray(carve[2], np.uint8)}
    votes = {k: erasor_amd.votes_from_masks(v) for k, v in kept_masks.items()}
    votes["both"] = erasor_amd.votes_from_masks(*kept_masks.values())
    thr = {"visibility": 1, "carve": 1, "both": 2}
    head = {"frames": a.frames, "length": a.length, "spacing": a.spacing, "az": a.az, "map_points": int(len(m)), "scan_points": int(sum(len(s) for s in sc)),
            "ground_points": int((ground != 0).sum()), "cast_s": t_cast, "runs": a.runs, "max_size": a.max_size}
    print(json.dumps(head), flush=True)
    rows_out = [head]
    # the clustering alone on the same rows, per tolerance
    not_ground = np.ascontiguousarray(m[ground == 0])
    for tol in tols:
        row = {"cluster_tol": tol, "cluster_non_ground_rows": int(len(not_ground))}
        out = {}
        row["cluster_non_ground_wall_ms"] = median_ms(lambda: out.__setitem__("c", g.cluster(not_ground, tol)), a.runs)
        row["cluster_non_ground_result"] = out["c"][3]
        row["cluster_all_rows_wall_ms"] = median_ms(lambda: out.__setitem__("c", g.cluster(m, tol)), a.runs)
        row["cluster_all_rows_result"] = out["c"][3]
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    before = {}
    for name, v in votes.items():
        kept = np.ascontiguousarray(m[v < thr[name]])
        before[name] = {"removed": int(len(m) - len(kept)), **rates(g.evaluate(m, kept)), "ghost_objects": g.residue(m, kept, tol=0.5)[3]["n_clusters"]}
        before[name + " & ~ground"] = {"removed": int(((v >= thr[name]) & (ground == 0)).sum()),
                                       **rates(g.evaluate(m, np.ascontiguousarray(m[(v < thr[name]) | (ground != 0)])))}
    print(json.dumps({"before": before}), flush=True)
    rows_out.append({"before": before})
    for name, v in votes.items():
        for use_ground in (True, False):
            for tol in tols:
                for ratio in ratios:
                    prm = dict(tol=tol, vote_thr=thr[name], remove_ratio=ratio, max_size=a.max_size)
                    out = {}
                    call = lambda: out.__setitem__("r", g.object_vote(m, v, ground if use_ground else None, **prm))  # noqa: E731
                    row = {"votes": name, "ground_mask": use_ground, **prm, "wall_ms": median_ms(call, a.runs), "device_ms_per_kernel": profiled(g, call)}
                    mask, rows, _, kept, res = out["r"]
                    row["result"] = res
                    row["grown_dynamic_share"] = res["n_grown_dynamic"] / res["n_grown"] if res["n_grown"] else None
                    row["decisions"] = np.bincount(rows["decision"], minlength=4).tolist()
                    row["after"] = {**rates(g.evaluate(m, kept)), "ghost_objects": g.residue(m, kept, tol=0.5)[3]["n_clusters"]}
                    print(json.dumps(row), flush=True)
                    rows_out.append(row)
    # the normative text on a cut-down input
    if not a.no_host:
        x0 = float(T[0][0, 3])
        sel = np.abs(m[:, 0] - x0) <= a.host_length
        cut, cg = np.ascontiguousarray(m[sel]), np.ascontiguousarray(ground[sel])
        for name, v in votes.items():
            prm = dict(tol=tols[-1], vote_thr=thr[name], remove_ratio=ratios[0], revert_ratio=0.1 * ratios[0], max_size=2000)
            cv = np.ascontiguousarray(v[sel])
            t0 = time.perf_counter()
            ref = evalmap.object_vote(cut, cv, cg, **prm)
            t_host = (time.perf_counter() - t0) * 1e3
            out = {}
            t_dev = median_ms(lambda: out.__setitem__("r", g.object_vote(cut, cv, cg, **prm)), a.runs)
            got = out["r"]
            row = {"host_votes": name, "host_points": int(len(cut)), **prm, "host_wall_ms": t_host, "device_wall_ms": t_dev, "host_result": ref[4],
                   "equal_to_host": all(np.asarray(got[j]).tobytes() == np.asarray(ref[j]).tobytes() for j in range(4)) and got[4] == ref[4]}
            print(json.dumps(row), flush=True)
            rows_out.append(row)
    g.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
