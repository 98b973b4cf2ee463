"""Where a handle's streams land (erasor_hip_stream_pipes): the rehearsal at handle creation steers the early stream of overlapped steps
onto a compute pipe that main, q0 and q1 do not have, and nothing of it changes a result.  Twelve deep steps with the overlap forced,
every one against the oracle.  Each case in a process of its own: the switches are read once."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = """
import sys
import json
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import erasor_amd
import scenarios
import test_gpu_parity as T
from oracle import orc
sc = scenarios.small()
nf = len(sc["scans"])
N = 12
order = [k %% nf if (k // nf) %% 2 == 0 else nf - 1 - k %% nf for k in range(N)]  # down the street and back
scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
LA = 4  # four nodes announced ahead: deep enough for overlapped steps


class Run:
    def __init__(self):
        self.g = erasor_amd.Erasor(scenarios.to_product_params(sc["params"]))
        self.o = orc.Oracle(sc["params"])
        self.g.set_map(sc["map"])
        self.o.set_map(sc["map"])
        self.k = 0
        for j in range(LA):
            self.announce(j)

    def announce(self, j):
        f = order[j]
        self.g.prefetch(scans[f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])

    def step(self):
        k = self.k
        if k + LA < N:
            self.announce(k + LA)
        f = order[k]
        rg = self.g.step(scans[f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        ro = self.o.step(scans[f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
        T.compare_step(self.g, self.o, rg, ro, full=(k %% 4 == 0 or k == N - 1))
        self.k += 1

    def report(self):
        return {"log": self.g.step_log(), "pipes": self.g.stream_pipes(), "overlap_counts": self.g.overlap_counts()}


%(body)s
"""

ONE = """
r = Run()
for _ in range(N):
    r.step()
print("PLACEMENT " + json.dumps([r.report()]))
"""

# two handles stepped alternately; the first is destroyed (its pads go with it), then a third is created and stepped
TWO = """
a, b = Run(), Run()
for _ in range(N):
    a.step()
    b.step()
ra, rb = a.report(), b.report()
a.g.close()
c = Run()
for _ in range(N):
    c.step()
print("PLACEMENT " + json.dumps([ra, rb, c.report()]))
"""


def run_worker(tmp_path, body, env_extra):
    script = tmp_path / "stream_placement_worker.py"
    script.write_text(WORKER % {"root": ROOT, "body": body})
    env = dict(dict(os.environ, ERASOR_HIP_OVERLAP="1", ERASOR_HIP_PLACEMENT_LOG="1"), **env_extra)
    env = {k: v for k, v in env.items() if v is not None}  # (None: the variable is removed)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0 and "PLACEMENT " in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    reps = json.loads(out.stdout.split("PLACEMENT ", 1)[1].splitlines()[0])
    print("\n".join(line for line in out.stderr.splitlines() if "placement:" in line))
    for r in reps:
        print(r["pipes"], r["overlap_counts"], [e["n_create"] for e in r["log"]])
    return reps


def skip_on_the_cpu_stand_in():
    if os.environ.get("ERASOR_TEST_SIMT_LIB"):
        pytest.skip("no hardware queues on the CPU stand-in: every pipe is unknown and nothing is steered (tests/test_stream_place.py checks the rule)")


@pytest.mark.gpu
def test_the_early_stream_gets_a_pipe_of_its_own_and_every_step_matches_the_oracle(tmp_path):
    """Twelve overlapped steps against the oracle.  All four pipes are known; where the rehearsal saw four different pipes the early
    stream's is none of the other three; at most three pads; the early stream is still the first step's creation (with the copy stream
    of the host scans)."""
    skip_on_the_cpu_stand_in()
    (r,) = run_worker(tmp_path, ONE, {})
    p = r["pipes"]
    assert len(p["pipes"]) == 4 and all(0 <= v <= 15 for v in p["pipes"]), p
    if p["distinct_seen"] >= 4:
        assert p["pipes"][3] not in p["pipes"][:3], p
    assert 0 <= p["n_pads"] <= 3
    log = r["log"]
    assert len(log) == 12 and log[0]["n_create"] == 2 and sum(e["n_create"] for e in log[1:]) == 0
    assert any(e["reserved"] for e in log) and r["overlap_counts"][1] > 0, "the steps did overlap"


@pytest.mark.gpu
def test_one_query_stream_places_nothing(tmp_path):
    """ERASOR_HIP_QSTREAMS=1, the overlap left to the handle (forced, a step overlaps whatever the handle has): no rehearsal, no pad, no
    early stream; every step plain and equal to the oracle's"""
    skip_on_the_cpu_stand_in()
    (r,) = run_worker(tmp_path, ONE, {"ERASOR_HIP_QSTREAMS": "1", "ERASOR_HIP_OVERLAP": None})
    assert r["pipes"]["n_pads"] == 0 and r["pipes"]["pipes"][3] == -1, r["pipes"]
    assert all(e["reserved"] == 0 and e["use_ov"] == 0 for e in r["log"]) and r["overlap_counts"] == [0, 0]


@pytest.mark.gpu
def test_the_switch_leaves_the_handle_as_it_was(tmp_path):
    """ERASOR_HIP_NO_PLACEMENT=1: no pad; the overlapped steps match the oracle"""
    skip_on_the_cpu_stand_in()
    (r,) = run_worker(tmp_path, ONE, {"ERASOR_HIP_NO_PLACEMENT": "1"})
    assert r["pipes"]["n_pads"] == 0 and r["pipes"]["pipes"] == [-1, -1, -1, -1], r["pipes"]
    assert r["log"][0]["n_create"] == 2 and any(e["reserved"] for e in r["log"])


@pytest.mark.gpu
def test_two_handles_stepped_alternately_then_a_third(tmp_path):
    """Two handles in one process, stepped in turn, both against the oracle; the first is destroyed and takes its pads with it; a third
    handle created afterwards steps against the oracle too.  Where a handle's streams land beside another's is not asserted."""
    skip_on_the_cpu_stand_in()
    reps = run_worker(tmp_path, TWO, {})
    assert len(reps) == 3
    for r in reps:
        assert len(r["log"]) == 12 and 0 <= r["pipes"]["n_pads"] <= 3
        assert r["log"][0]["n_create"] == 2 and sum(e["n_create"] for e in r["log"][1:]) == 0
