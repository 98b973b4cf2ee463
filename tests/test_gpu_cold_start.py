"""A fresh handle's first steps through the per-step record (erasor_hip_step_log): a change of mode costs no allocation and no stream,
the record's periods are the ones the overlap decision averaged, and a handle with one query stream never prepares the overlapped mode.
Each case in a process of its own with ERASOR_HIP_OVERLAP removed (the switch is read once; the suite forces the overlap)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = """
import sys
import json
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import os
os.environ.pop("ERASOR_HIP_OVERLAP", None)  # (the handle decides)
import erasor_amd
import scenarios
import test_gpu_parity as T
from oracle import orc
sc = scenarios.small()
g = erasor_amd.Erasor(scenarios.to_product_params(sc["params"]))
o = orc.Oracle(sc["params"])
g.set_map(sc["map"])
o.set_map(sc["map"])
nf = len(sc["scans"])
order = [k %% nf if (k // nf) %% 2 == 0 else nf - 1 - k %% nf for k in range(30)]  # down the street and back
scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"]]
LA = 4  # (the handle considers overlapping only for a caller that announces at least three nodes beyond the step's own)
for j in range(LA):
    g.prefetch(scans[order[j]], sc["T_l2b"], sc["T_b2o"][order[j]], sc["T_o2b"][order[j]])
for k, f in enumerate(order):
    if k + LA < len(order):
        f2 = order[k + LA]
        g.prefetch(scans[f2], sc["T_l2b"], sc["T_b2o"][f2], sc["T_o2b"][f2])
    rg = g.step(scans[f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    ro = o.step(scans[f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    T.compare_step(g, o, rg, ro, full=(k %% 5 == 0))
print("COLD-START " + json.dumps({"log": g.step_log(), "auto": g.overlap_auto(), "overlap_counts": g.overlap_counts()}))
"""


def run_worker(tmp_path, env_extra):
    import json
    script = tmp_path / "cold_start_worker.py"
    script.write_text(WORKER % (ROOT, ROOT))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=280, env=dict(os.environ, **env_extra))
    assert out.returncode == 0 and "COLD-START " in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    r = json.loads(out.stdout.split("COLD-START ", 1)[1].splitlines()[0])
    for e in r["log"]:
        print(e)
    print(r["auto"], r["overlap_counts"])
    return r


def skip_on_the_cpu_stand_in():
    if os.environ.get("ERASOR_TEST_SIMT_LIB"):
        pytest.skip("30 steps: most of an hour on the CPU stand-in")


@pytest.mark.gpu
def test_a_change_of_mode_allocates_nothing_and_the_record_holds_the_sampled_periods(tmp_path):
    """30 deep steps, every one against the oracle: the handle samples both modes.  From the record: both layouts occur; a step whose
    layout differs from the previous step's made no allocation, no free and created no stream or event (the early stream is there since
    the first deep step: created before the first step's record closes, with the copy stream of the host scans); the periods marked as
    sampled, mode by mode without each mode's largest, give exactly the two means erasor_hip_overlap_auto reports.  Which mode wins on
    this small scene is not asserted."""
    skip_on_the_cpu_stand_in()
    r = run_worker(tmp_path, {})
    log = r["log"]
    assert [e["step"] for e in log] == list(range(1, 31))
    assert all(e["deep"] for e in log[:26]), "four nodes are announced beyond every step but the last four"
    layouts = [e["reserved"] for e in log]
    assert 0 in layouts and 1 in layouts
    changes = [k for k in range(1, len(log)) if layouts[k] != layouts[k - 1]]
    assert changes
    for k in changes:
        assert (log[k]["n_alloc"], log[k]["n_free"], log[k]["n_create"]) == (0, 0, 0), (k, log[k])
    assert log[0]["n_create"] == 2 and sum(e["n_create"] for e in log[1:]) == 0, "the copy stream and the early stream, both before the first step ends"
    assert log[0]["period_us"] == 0 and all(e["period_us"] > 0 for e in log[1:])
    # the decision's own arithmetic, from the record
    blocks = {}
    for e in log:
        if e["sampled"]:
            assert e["deep"] and e["ova_skip"] == 0 and e["ova_block"] < 4
            assert e["reserved"] == e["ova_mode"] == (1 if e["ova_block"] in (1, 2) else 0)
            blocks.setdefault(e["ova_block"], []).append(e["period_us"])
    mode, p_plain, p_ov = r["auto"]
    assert p_plain > 0 and p_ov > 0 and sorted(blocks) in ([0, 1], [0, 1, 2, 3])
    assert all(len(v) == 4 for v in blocks.values())
    kept = {0: [], 1: []}
    for b, v in blocks.items():
        kept[1 if b in (1, 2) else 0] += v
    kept = {m: sorted(v)[:-1] for m, v in kept.items()}  # (a mode's mean leaves out its largest sample)
    assert abs(sum(kept[0]) / len(kept[0]) - p_plain) <= 1e-9 * p_plain
    assert abs(sum(kept[1]) / len(kept[1]) - p_ov) <= 1e-9 * p_ov
    launched, taken = r["overlap_counts"]
    assert 0 < taken < 30 and taken == sum(e["use_ov"] for e in log)


@pytest.mark.gpu
def test_one_query_stream_never_prepares_the_overlapped_mode(tmp_path):
    """ERASOR_HIP_QSTREAMS=1 (several handles on one GPU: main + one query stream each): no early stream -- the only creation is the
    copy stream of the host scans --, every step plain, nothing launched ahead beside a per-bin launch; every step against the oracle."""
    skip_on_the_cpu_stand_in()
    r = run_worker(tmp_path, {"ERASOR_HIP_QSTREAMS": "1"})
    log = r["log"]
    assert len(log) == 30
    assert all(e["reserved"] == 0 and e["use_ov"] == 0 for e in log)
    assert log[0]["n_create"] == 1 and sum(e["n_create"] for e in log[1:]) == 0
    assert r["overlap_counts"] == [0, 0]
