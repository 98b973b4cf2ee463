#!/usr/bin/env python3
"""Timing of the bird's-eye renderer (MEASUREMENTS.md, "Bird's-eye images") on the bench's maps.

  python tools/render_bench.py [--spacing 0.2] [--res 0.2 0.05] [--runs 7] [--no-host] [--out FILE.json]

Per map and resolution:
  (a) what a user could do before: Erasor.get_map() (device -> host copy of the map) + evalmap.render on the host, wall time;
  (b) Erasor.render_map: median wall time of --runs calls after a warm-up call, and the device time per kernel group from the
      library's event brackets (Erasor.profiling), in a second set of calls so that the brackets do not sit in the wall times;
  (c) the other rasteriser (one 64-bit atomic max per point on a key image in device memory; a test hook of the library built with
      `make -C erasor_amd/csrc hooks`) against the shipped kernels, on the same device cloud, alternating: device time of each between
      one event before its clears and one after its last kernel, images compared;
  (d) per kernel group, the bytes it must move over its device time.
--spacing 0.2 is bench config 2's map (9.8 M points), --spacing 0.1 config 4's (39.2 M).  A resolution the fit refuses (the image
would be beyond the limits) is reported, and the smallest one that fits, as the refusal names it, is measured in its place.
--no-host skips (a) and the comparison with the host image (for a run under a profiler)."""
import argparse
import ctypes as C
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


def bench_map(spacing):
    w = synth.World(seed=20210305 + 5, length=1000.0, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    return w.sample_map(spacing=spacing, frames=range(0, 320, 2))


def median_ms(fn, runs):
    fn()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def other_rasteriser(m, view, runs):
    """(device ms of the atomic rasteriser, device ms of the shipped kernels, images equal) through the hooks library"""
    path = os.path.join(ROOT, "tests", "_build", "liberasor_hip_hooks.so")
    if not os.path.exists(path):
        return None
    L = C.CDLL(path)
    L.erasor_hip_last_error.restype = C.c_char_p
    L.erasor_hip_last_error.argtypes = [C.c_void_p]
    L.erasor_hip_destroy.argtypes = [C.c_void_p]
    p = erasor_amd.Params()
    L.erasor_hip_params_default(C.byref(p))
    h = C.c_void_p()
    assert L.erasor_hip_create(C.byref(p), 0, C.byref(h)) == 0
    d = C.c_void_p()
    assert L.erasor_hip_device_alloc(h, C.c_size_t(m.nbytes), C.byref(d)) == 0
    assert L.erasor_hip_device_upload(h, d, m.ctypes.data_as(C.c_void_p), C.c_size_t(m.nbytes)) == 0
    v = erasor_amd.RenderView.of(view)
    a = np.empty((v.height, v.width, 3), np.uint8)
    b = np.empty_like(a)
    sa, sb = erasor_amd.RenderStats(), erasor_amd.RenderStats()
    ms = C.c_double(0)
    ta, tb = [], []
    for k in range(runs + 1):  # (alternating; the first pair is the warm-up)
        for tiled, img, st, t in ((0, a, sa, ta), (1, b, sb, tb)):
            rc = L.erasor_hip_debug_render_atomic(h, d, C.c_size_t(len(m)), 1, 0, C.byref(v), img.ctypes.data_as(C.c_void_p), C.byref(st),
                                                  C.c_int(tiled), C.byref(ms))
            assert rc == 0, L.erasor_hip_last_error(h)
            if k:
                t.append(ms.value)
    same = bool((a == b).all()) and sa.as_dict() == sb.as_dict()
    L.erasor_hip_device_free(h, d)
    L.erasor_hip_destroy(h)
    return {"atomic_device_ms": statistics.median(ta), "atomic_min_max": [min(ta), max(ta)], "tiled_device_ms": statistics.median(tb),
            "tiled_min_max": [min(tb), max(tb)], "images_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=0.2)
    ap.add_argument("--res", type=float, nargs="+", default=[0.2, 0.05])
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    erasor_amd.build()
    m = bench_map(a.spacing)
    p = erasor_amd.params_default()
    synth.apply_params(p, "05", max_range=80.0, num_rings=20, num_sectors=108)
    g = erasor_amd.Erasor(p)
    g.set_map(m)
    rows = []
    todo = list(a.res)
    while todo:
        res = todo.pop(0)
        row = {"spacing": a.spacing, "map_points": int(len(m)), "res": res}
        try:
            view = g.render_fit(None, res)
        except erasor_amd.ErasorError as e:
            row["refused"] = str(e)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if "about" in str(e):  # (the smallest resolution that fits, in its place)
                todo.insert(0, float(str(e).rsplit("about", 1)[1]))
            continue
        row["width"], row["height"] = view["width"], view["height"]
        t0 = time.perf_counter()
        host = g.get_map()
        t1 = time.perf_counter()
        row["a_get_map_ms"] = (t1 - t0) * 1e3
        if not a.no_host:
            img_h, st_h = evalmap.render(host, view)
            row["a_host_render_ms"] = (time.perf_counter() - t1) * 1e3
        out = {}

        def call():
            out["r"] = g.render_map(view)

        row["b_render_map_wall_ms"] = median_ms(call, a.runs)
        if not a.no_host:
            row["equal_to_host"] = bool((out["r"][0] == img_h).all()) and out["r"][1] == st_h
        row["b_fit_wall_ms"] = median_ms(lambda: g.render_fit(None, res), a.runs)
        g.profiling(1)
        g.profile_reset()
        for _ in range(a.runs):
            g.render_map(view)
        prof = {k: v[0] / a.runs for k, v in g.profile_get().items() if k.startswith("render") or k == "replicate"}
        g.profiling(0)
        row["b_device_ms_per_kernel"] = prof
        n, npix, ntiles = len(m), view["width"] * view["height"], -(-view["width"] // 64) * -(-view["height"] // 64)
        must = {"render_bin": n * (16 + 12) + ntiles * 4, "render_scatter": n * (12 + 8), "render_resolve": n * 8 + npix * 3 + ntiles * 8}
        row["d_gbps"] = {k: must[k] / (prof[k] * 1e-3) / 1e9 for k in must if prof.get(k)}
        row["c_other"] = other_rasteriser(np.ascontiguousarray(host), view, a.runs)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
