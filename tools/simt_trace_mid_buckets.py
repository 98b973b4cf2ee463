#!/usr/bin/env python3
"""A traced scenario for tools/simt_trace_diff.py that no test of the suite covers: 30 rings x 100 sectors = 3000 bins, i.e. between 2176
and 4096 buckets, where the map's scatter is k_mb_scatter_w<MBW_NB_MAX> -- on the step's own site and, with the steps overlapped, on the
site launched ahead.  scenarios.small(), four steps, two nodes announced ahead with pose and both transforms, every step against the oracle.

    SIMT_EMU_TRACE=1 python tools/simt_trace_mid_buckets.py <liberasor_hip_simt.so> 2> trace      (the library: tests/simt.py)"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("ERASOR_HIP_OVERLAP", "1")
os.environ["ERASOR_TEST_SIMT_LIB"] = sys.argv[1]
import numpy as np  # noqa: E402
import erasor_amd  # noqa: E402

erasor_amd.LIB_PATH = sys.argv[1]
erasor_amd._lib = None
import scenarios  # noqa: E402
import test_gpu_parity as T  # noqa: E402

sc = scenarios.small()
p = copy.copy(sc["params"])
p.num_rings, p.num_sectors = 30, 100
g, o = T.make_pair(erasor_amd, p)
g.set_map(sc["map"])
o.set_map(sc["map"])
scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
N = 4
for j in range(2):
    g.prefetch(scans[j], sc["T_l2b"], sc["T_b2o"][j], sc["T_o2b"][j])
for k in range(N):
    if k + 2 < N:
        g.prefetch(scans[k + 2], sc["T_l2b"], sc["T_b2o"][k + 2], sc["T_o2b"][k + 2])
    rg = g.step(scans[k], sc["T_l2b"], sc["T_b2o"][k], sc["T_o2b"][k])
    ro = o.step(scans[k], sc["T_l2b"], sc["T_b2o"][k], sc["T_o2b"][k])
    T.compare_step(g, o, rg, ro)
print("MID-BUCKETS-OK overlapped steps launched / taken: %d / %d" % g.overlap_counts())
