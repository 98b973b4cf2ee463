"""Test infrastructure: the library's test hooks, called through a copy of the library that was built with them
(-DERASOR_HIP_TEST_HOOKS -> tests/_build/liberasor_hip_hooks.so).  The product library does not export these entry points and the
package has no wrapper for them any more (round 4)."""
import contextlib
import ctypes as C
import os

import numpy as np

import erasor_amd

HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS_LIB = os.path.join(HERE, "_build", "liberasor_hip_hooks.so")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@contextlib.contextmanager
def hooks_library():
    """inside the block erasor_amd loads the hooks build instead of the product library (under ERASOR_TEST_SIMT_LIB the CPU stand-in
    build, which is compiled with the hooks, is in place already)"""
    if os.environ.get("ERASOR_TEST_SIMT_LIB"):
        yield
        return
    # (built here, by the tests that need it -- `make hooks`; the product build, plain `make`, neither compiles nor writes it)
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(HERE), "erasor_amd", "csrc"), "-s", "hooks"])
    keep = (erasor_amd.LIB_PATH, erasor_amd._lib)
    erasor_amd.LIB_PATH, erasor_amd._lib = HOOKS_LIB, None
    try:
        yield
    finally:
        erasor_amd.LIB_PATH, erasor_amd._lib = keep


def probe_math(g, x, y):
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    o = [np.zeros_like(x) for _ in range(3)]
    g._check(erasor_amd.lib().erasor_hip_probe_math(g._h, _p(x), _p(y), C.c_size_t(len(x)), _p(o[0]), _p(o[1]), _p(o[2])))
    return o


def probe_bin_keys(g, pts):
    pts = np.ascontiguousarray(pts, np.float32)
    kf = np.zeros(len(pts), np.uint32)
    ke = np.zeros(len(pts), np.uint32)
    ctr = np.zeros(4, np.uint32)
    g._check(erasor_amd.lib().erasor_hip_probe_bin_keys(g._h, _p(pts), C.c_size_t(len(pts)), _p(kf), _p(ke), _p(ctr)))
    return kf, ke, ctr


def exact_sort_u32(g, keys, vals):
    keys = np.ascontiguousarray(keys, np.uint32).copy()
    vals = np.ascontiguousarray(vals, np.uint32).copy()
    nf = C.c_uint32(0)
    g._check(erasor_amd.lib().erasor_hip_exact_sort_u32(g._h, _p(keys), _p(vals), C.c_size_t(len(keys)), C.byref(nf)))
    return keys, vals, int(nf.value)


def radix_sort_u32(g, keys, bits):
    keys = np.ascontiguousarray(keys, np.uint32)
    ko = np.zeros_like(keys)
    po = np.zeros_like(keys)
    g._check(erasor_amd.lib().erasor_hip_radix_sort_u32(g._h, _p(keys), C.c_size_t(len(keys)), C.c_int(bits), _p(ko), _p(po)))
    return ko, po


def debug_rebuild_outskirts(g):
    g._check(erasor_amd.lib().erasor_hip_debug_rebuild_outskirts(g._h))


def debug_store_state(g, records=True):
    """the map store between steps (read-only): nF, nFv, o_begin, capO, o_valid; the last step's n_o_read, n_leaving, o_new_begin and
    scan_path (1 / 2: one-launch / two-level chunk scan run by the step, 3 / 4: launched ahead, 5 / 6: overlapped); scan_one_max, chunk;
    "rec": the OMeta records of the chunks [o_begin / chunk, capO / chunk) as (xmin, xmax, ymin, ymax), valid, known (None without records)"""
    out = np.zeros(12, np.uint64)
    n = C.c_size_t(0)
    g._check(erasor_amd.lib().erasor_hip_debug_store_state(g._h, _p(out), C.c_void_p(None), C.c_size_t(0), C.byref(n)))
    names = ("nF", "nFv", "o_begin", "capO", "o_valid", "n_o_read", "n_leaving", "o_new_begin", "scan_path", "use_ometa", "scan_one_max", "chunk")
    st = {k: int(v) for k, v in zip(names, out)}
    st["rec"] = None
    if records and st["use_ometa"]:
        rec = np.zeros((max(n.value, 1), 8), np.uint32)
        g._check(erasor_amd.lib().erasor_hip_debug_store_state(g._h, _p(out), _p(rec), C.c_size_t(len(rec)), C.byref(n)))
        rec = rec[: n.value]
        st["rec"] = {"box": rec[:, :4].copy().view(np.float32), "valid": rec[:, 4].copy(), "known": rec[:, 5].copy()}
    return st


def debug_set_scan_one_max(g, n):
    """stores of more than n chunks take the two-level chunk scan (0: the default, 16384)"""
    g._check(erasor_amd.lib().erasor_hip_debug_set_scan_one_max(g._h, C.c_uint32(n)))


def debug_nn_tree(g, cloud):
    """the bounding-volume tree nn_build builds over `cloud` (N x 4 rows): P, the points in key order, their original indices,
    the sorted Morton keys, lo / hi of the 2P nodes (node 0 is unused)"""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    n = len(cloud)
    cap = 4 * (n // 32 + 1) + 4  # (at least 2P: P < 2 * ceil(n / 32))
    P = C.c_uint32(0)
    pts, idx, keys = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    lo, hi = np.zeros((cap, 4), np.float32), np.zeros((cap, 4), np.float32)
    g._check(erasor_amd.lib().erasor_hip_debug_nn_tree(g._h, _p(cloud), C.c_size_t(n), C.c_int(0), C.byref(P), _p(pts), _p(idx), _p(keys), _p(lo),
                                                       _p(hi), C.c_size_t(cap)))
    P = int(P.value)
    return {"P": P, "pts": pts, "idx": idx, "keys": keys, "lo": lo[: 2 * P], "hi": hi[: 2 * P]}


def debug_nn_effort(g, tree, queries, f32):
    """k_nn_query (f32 False) or k_lm_query (f32 True) of `queries` over the tree of `tree`, with effort[i] = (leaves opened, leaf points
    tested) of query i beside the kernel's outputs: "dist" / "nearest", or "rows" / "n_tied" """
    tree = np.ascontiguousarray(tree, np.float32).reshape(-1, 4)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 4)
    nq = len(q)
    dist, near = np.zeros(nq, np.float64), np.zeros(nq, np.uint32)
    rows, tied, effort = np.zeros((nq, 4), np.float32), C.c_uint64(0), np.zeros((nq, 2), np.uint32)
    g._check(erasor_amd.lib().erasor_hip_debug_nn_effort(g._h, _p(tree), C.c_size_t(len(tree)), _p(q), C.c_size_t(nq), C.c_int(int(f32)), _p(dist),
                                                         _p(near), _p(rows), C.byref(tied), _p(effort)))
    out = {"effort": effort}
    out.update({"rows": rows, "n_tied": int(tied.value)} if f32 else {"dist": dist, "nearest": near})
    return out


def debug_ev_grid(g, est, voxelsize):
    """the evaluator's hashed grid over `est` (N x 4 rows): nb, off[nb + 1], the scattered points and their original indices"""
    est = np.ascontiguousarray(est, np.float32).reshape(-1, 4)
    n = len(est)
    cap = 2 * max(n, 1024) + 2
    nb = C.c_uint32(0)
    off, pts, idx = np.zeros(cap, np.uint32), np.zeros((n, 4), np.float32), np.zeros(n, np.uint32)
    g._check(erasor_amd.lib().erasor_hip_debug_ev_grid(g._h, _p(est), C.c_size_t(n), C.c_double(voxelsize), C.byref(nb), _p(off), C.c_size_t(cap),
                                                       _p(pts), _p(idx)))
    return {"nb": int(nb.value), "off": off[: nb.value + 1], "pts": pts, "idx": idx}


def debug_ev_grid_many(g, ests, voxelsize):
    """evaluate_many's combined table over `ests`: as debug_ev_grid over all estimates back to back, plus "tab": one
    (first point, points, first bucket, bucket mask) row per estimate"""
    ests = [np.ascontiguousarray(e, np.float32).reshape(-1, 4) for e in ests]
    k, n = len(ests), sum(len(e) for e in ests)
    cap = sum(2 * max(len(e), 1024) for e in ests) + 2
    ptrs = (C.c_void_p * k)(*[_p(e) for e in ests])
    sizes = (C.c_size_t * k)(*[len(e) for e in ests])
    nb = C.c_uint32(0)
    off, pts, idx, tab = np.zeros(cap, np.uint32), np.zeros((n, 4), np.float32), np.zeros(n, np.uint32), np.zeros((k, 4), np.uint32)
    g._check(erasor_amd.lib().erasor_hip_debug_ev_grid_many(g._h, ptrs, sizes, C.c_size_t(k), C.c_double(voxelsize), C.byref(nb), _p(off),
                                                            C.c_size_t(cap), _p(pts), _p(idx), _p(tab)))
    return {"nb": int(nb.value), "off": off[: nb.value + 1], "pts": pts, "idx": idx, "tab": tab}


SORT_STATE = ("cnt0", "cnt1", "cnt2", "small_cnt", "nseg0", "nseg1", "ntiles0", "ntiles1", "n", "wide_levels", "level_launches", "mid_run",
              "final_grid", "n_sort_fallback", "n_voxel_overflow", "sort_qoverflow", "err", "run_tiles")


def debug_sort_queues(g):
    """what the last exact sort of the handle's query side -- exact_sort_u32, or the sort inside a voxelisation -- left behind (read-only):
    EsQueues and WideState, what run_exact_sort launched (keys, wide levels, k_esort_level launches, whether k_esort_mid ran,
    k_esort_final's grid), the chain's counters, and the (first, last, depth) records of the finisher's queue ("small") and of the three
    level queues ("q0", "q1", "q2") up to their counts.  After a sort that ran k_esort_mid, q0 is what that kernel was given."""
    st = np.zeros(len(SORT_STATE), np.uint32)
    g._check(erasor_amd.lib().erasor_hip_debug_sort_queues(g._h, _p(st), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_void_p(None),
                                                           C.c_size_t(0)))
    out = {k: int(v) for k, v in zip(SORT_STATE, st)}
    cap = max(1, min(65536, max(out["cnt0"], out["cnt1"], out["cnt2"], out["small_cnt"])))
    rec = [np.zeros((cap, 3), np.int32) for _ in range(4)]
    g._check(erasor_amd.lib().erasor_hip_debug_sort_queues(g._h, _p(st), _p(rec[0]), _p(rec[1]), _p(rec[2]), _p(rec[3]), C.c_size_t(cap)))
    for name, r, k in zip(("small", "q0", "q1", "q2"), rec, ("small_cnt", "cnt0", "cnt1", "cnt2")):
        out[name] = r[: min(out[k], cap)].astype(np.int64)
    return out
