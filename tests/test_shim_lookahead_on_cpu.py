"""erasor::OfflineMapUpdater's look-ahead state machine (announce_upcoming / announce_next / announce_next_deferred / callback_node with
and without a ticket) under the removal_interval gate, explored on the CPU: tests/cpp/shim_lookahead_check.cpp drives the shim by six
caller policies against tests/cpp/fake_erasor_hip.cpp, a recording stand-in that implements the announcement contract of
erasor_hip.hip and nothing else (tests/test_gpu_shim_lookahead.py pins it to the real library).  No GPU.

Every script (policy, removal_interval, lookahead, seed; N = 3 * interval + lookahead + 3 nodes) must satisfy
  (a) nothing throws;
  (b) the processed callbacks are exactly the nodes with (node + 1) % interval == 0, in order, each on its own cloud with its own
      T_body2origin and T_origin2body;
  (c) window / greedy / greedy_deferred: every ungated node that was given a ticket, or whose deferred hand-over was accepted, is stepped
      by that ticket (stepped_by_ticket()), and the updater drops nothing (announcements_dropped());
  (d) under those three, from the second processed node on every ungated node is stepped by ticket;
  (e) after every call outstanding() equals the number of announcements the library holds.
Against the shim before capacity was tested ahead of the gate, greedy at removal_interval 2 threw for every lookahead 2 .. 7
("not the ticket of the oldest announced scan"): the node refused by the gate while the pipeline was full was retried and staged under
the next node's callback number."""
import os

import pytest

import shim_lookahead as sl

N_SCANS = 40  # >= 3 * 9 + 7 + 3: every node of every script has a cloud and a pose of its own


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lookahead_data"))
    m, scans = sl.toy_data(d, N_SCANS)
    return d, m, scans


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """linked against the stand-in built as a liberasor_hip.so in the temporary directory, as the GPU test links the real one"""
    d = str(tmp_path_factory.mktemp("lookahead_fake"))
    sl.build_fake_lib(d)
    return sl.build_driver(os.path.join(d, "shim_lookahead_check"), libdir=d)


def _run_and_collect(exe, toy, tmp_path, policy, intervals, lookaheads, n_seeds, env=None):
    d, m, scans = toy
    bad, n = [], 0
    for iv in intervals:
        scripts, out = sl.run_driver(exe, d, str(tmp_path / ("%s_%d_" % (policy, iv))), N_SCANS, iv, lookaheads, policy, 1000 * iv, n_seeds, env=env)
        assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
        for s in scripts:
            n += 1
            assert s.n_nodes == sl.n_nodes(iv, s.lookahead)
            f = sl.failures(s) + sl.stand_in_failures(s, m, scans)
            if f:
                bad.append(sl.tag(s) + ": " + " | ".join(f[:3]))
    assert n == len(intervals) * len(lookaheads) * n_seeds
    return bad, n


@pytest.mark.parametrize("policy", sl.FIXED_POLICIES + ("random",))
def test_every_caller_policy_at_every_interval_and_lookahead(driver, toy, tmp_path, policy):
    """removal_interval 1 .. 9 x lookahead 1 .. 7; `random` with 200 fixed seeds per interval"""
    bad, n = _run_and_collect(driver, toy, tmp_path, policy, list(range(1, 10)), list(range(1, 8)), 200 if policy == "random" else 1)
    assert not bad, "%d of %d scripts:\n%s" % (len(bad), n, "\n".join(bad[:40]))


def test_the_scripted_callers_are_clean_under_address_and_undefined_behaviour_sanitizers(toy, tmp_path):
    """The same driver, shim and stand-in compiled into ONE plain executable with -fsanitize=address,undefined (nothing is preloaded).  The
    driver frees the cloud of an announce_next_deferred hand-over as soon as the callback has returned: a later read of it ends the run."""
    exe = sl.build_driver(str(tmp_path / "shim_lookahead_check_san"), libdir=None, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    for policy in sl.FIXED_POLICIES + ("random",):
        bad, n = _run_and_collect(exe, toy, tmp_path, policy, [1, 2, 3, 8], [1, 2, 7], 20 if policy == "random" else 1, env=env)
        assert not bad, "%s: %d of %d scripts:\n%s" % (policy, len(bad), n, "\n".join(bad[:40]))


@pytest.mark.timeout(7200)  # (pytest.ini's 300 s is for the device; the stand-in takes seconds per step)
@pytest.mark.skipif(not (os.environ.get("ERASOR_SIMT_MORE") or os.environ.get("ERASOR_SIMT_ALL")), reason="~6 minutes: ERASOR_SIMT_MORE=1")
def test_the_scripted_callers_pass_on_the_cpu_stand_in_of_the_library(tmp_path):
    """tests/test_gpu_shim_lookahead.py against erasor_hip.hip itself, compiled for the CPU stand-in of the HIP runtime -- the mechanism of
    tests/test_full_step_on_cpu.py::test_the_cpp_shim_suite_passes_on_the_cpu_stand_in, in a test of its own --, on a reduced key: greedy
    and greedy_deferred at removal_interval 2 with lookahead 1, 2, 3 (16 steps each), against the oracle and against the recording stand-in
    of the C ABI."""
    import shutil
    import subprocess
    import sys
    import simt
    simt.build_oracle()
    d = str(tmp_path / "shim")
    os.makedirs(d)
    shutil.copy(simt.build_simt_lib(tmp_path), os.path.join(d, "liberasor_hip.so"))
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=os.path.join(d, "liberasor_hip.so"), ERASOR_TEST_SHIM_DIR=d)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(sl.HERE, "test_gpu_shim_lookahead.py"), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                          "-k", "scripted_callers and greedy and interval2"], capture_output=True, text=True, timeout=3600, cwd=sl.ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and "2 passed" in tail, out.stdout[-4000:] + out.stderr[-2000:]
