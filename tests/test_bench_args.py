"""bench.py's command line, without a GPU: a plain run does only what its headline needs; --full adds every other leg, and
the --no-* options still leave single legs of a --full run out."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("no_cpu_baseline", "no_pr_rr", "no_callback_bench", "no_extra_workloads")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_plain_run_leaves_every_other_leg_out():
    a = _bench().parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert not a.full and all(getattr(a, f) for f in LEGS)
    assert (a.gpus, a.steps, a.warmup, a.repeats, a.workload, a.mode) == (1, 20, 5, 1, "seq05", "replicas")


def test_full_runs_what_the_no_options_leave():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert a.full and not any(getattr(a, f) for f in LEGS)
    a = b.parse_args(["--full", "--no-pr-rr", "--no-callback-bench"])
    assert a.no_pr_rr and a.no_callback_bench and not a.no_cpu_baseline and not a.no_extra_workloads


def test_the_other_workload_passes_of_full_are_full_runs_of_their_own():
    b = _bench()
    verified = b.parse_args(b.extra_pass_cmd("large_scale_05", ["--cpu-steps", "1"], True)[2:])
    assert verified.full and not verified.no_cpu_baseline and verified.verify_all  # every step replayed on the oracle
    assert verified.no_extra_workloads and verified.no_pr_rr and verified.no_callback_bench and verified.cpu_steps == 1
    timed = b.parse_args(b.extra_pass_cmd("ouster128", [], False)[2:])
    assert timed.full and timed.no_cpu_baseline and timed.verify_prefix_seconds == 4 and timed.repeats == 7
