#!/usr/bin/env python3
"""The first steps of a fresh handle, one line per step (Erasor.step_log): period on the device's clock, mode, allocations and stream /
event creations, and what the overlap decision (overlap_auto.h) was doing -- the table of MEASUREMENTS.md, "cold start".

The sequence is bench.py's (same world, map, scans and look-ahead); like bench.py it runs the warm-up block and the timed block on a
fresh handle, `run_block(0, W)` then `run_block(W, K)`:

    python tools/cold_start.py --workload seq05 --steps 25 --warmup 5

--lib PATH loads another build of the library (to set two builds side by side on one box); --blocks prints, beside the table, the
mean period of every block of the decision's schedule and the relative difference between the two blocks of either mode (what
OVA_MARGIN is derived from)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_sequence(workload, steps, warmup, lib=None):
    import torch
    import bench
    import erasor_amd
    from erasor_amd import synth
    from erasor_amd import dist as ed
    if lib:
        erasor_amd.LIB_PATH = os.path.abspath(lib)
        erasor_amd._lib = None
    args = bench.parse_args(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--workload", workload])
    wl = bench.WORKLOADS[workload]
    n_frames = steps + warmup + args.lookahead
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lidar = bench.make_lidar(wl, args)
    x_end = ed.shard_frames(0, 1, n_frames)[0] + n_frames
    length = max(args.street_length, x_end + 150.0)
    per_m = length / args.street_length
    world = synth.World(seed=20210305 + 5, length=length, n_streets=args.streets, street_gap=50.0, n_moving=int(round(10 * per_m)),
                        n_peds=int(round(6 * per_m)))
    P = bench.make_params(wl, args)
    m = world.sample_map(spacing=wl["spacing"], frames=range(0, max(320, int(x_end - 20.0) + 2), 2), step=1.0)
    d_map = torch.from_numpy(m).to(dev)
    x0, _ = ed.shard_frames(0, 1, n_frames)
    return bench.Sequence(args, P, world, lidar, d_map, int(d_map.shape[0]), x0, n_frames, dev, 0, wl["l2b_z"], 1234), d_map


def block_means(log):
    """mean sampled period (without the largest sample) of every run of sampled steps that share block and mode"""
    runs = []
    for e in log:
        if not e["sampled"]:
            continue
        key = (e["ova_block"], e["ova_mode"])
        if not runs or runs[-1][0] != key:
            runs.append((key, []))
        runs[-1][1].append(e["period_us"])
    out = []
    for (blk, mode), p in runs:
        p = sorted(p)
        kept = p[:-1] if len(p) > 1 else p
        out.append({"block": blk, "mode": mode, "samples": len(p), "mean_us": float(np.mean(kept)), "max_us": p[-1]})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="seq05")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of liberasor_hip.so")
    ap.add_argument("--blocks", action="store_true", help="also print the schedule's block means and the drift between blocks of one mode")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the table")
    a = ap.parse_args(argv)
    import torch
    seq, _keep = build_sequence(a.workload, a.steps, a.warmup, a.lib)
    torch.cuda.synchronize()
    seq.run_block(0, a.warmup)
    seq.run_block(a.warmup, a.steps)
    torch.cuda.synchronize()
    log = seq.g.step_log()
    mode, p_plain, p_ov = seq.g.overlap_auto()
    blocks = block_means(log)
    if a.json:
        print(json.dumps({"workload": a.workload, "steps": a.steps, "warmup": a.warmup, "log": log, "blocks": blocks,
                          "decision": {"mode": mode, "plain_us": p_plain, "overlapped_us": p_ov}}))
        return
    print("# %s: %d warm-up + %d steps on a fresh handle; decision now: %s (plain %.1f us, overlapped %.1f us)"
          % (a.workload, a.warmup, a.steps, "overlapped" if mode else "plain", p_plain, p_ov))
    sp = seq.g.stream_pipes()
    print("# streams (me * 4 + pipe; main, q0, q1, early): %s; %d pad(s) kept, %d different pipe(s) seen" % (sp["pipes"], sp["n_pads"], sp["distinct_seen"]))
    print("| step | period us | layout | took ahead | deep | alloc | free | create | grown | decision: mode block skip | sampled |")
    print("|---:|---:|---|---|---|---:|---:|---:|---|---|---|")
    for e in log:
        print("| %d | %.1f | %s | %s | %s | %d | %d | %d | %s | %s %d %d | %s |"
              % (e["step"] - 1, e["period_us"], "reserved" if e["reserved"] else "dense", "yes" if e["use_ov"] else "no", "yes" if e["deep"] else "no",
                 e["n_alloc"], e["n_free"], e["n_create"], ("", "scratch", "outskirts", "both")[e["grown"] & 3], "O" if e["ova_mode"] else "P", e["ova_block"], e["ova_skip"], "yes" if e["sampled"] else ""))
    if a.blocks:
        print("# blocks: " + "; ".join("%d %s %.1f us (%d samples, max %.1f)" % (b["block"], "O" if b["mode"] else "P", b["mean_us"], b["samples"], b["max_us"])
                                       for b in blocks))
        by = {b["block"]: b["mean_us"] for b in blocks}
        for x, y in ((0, 3), (1, 2)):
            if x in by and y in by:
                print("# drift, block %d against %d: %+.2f %%" % (x, y, 100.0 * (by[y] - by[x]) / by[x]))


if __name__ == "__main__":
    main()
