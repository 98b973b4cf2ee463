"""The offline driver's --denoise and --density modes (erasor_offline_demo).  On a GPU: the printed counts and statistics and the written
cloud are those of the Python call (which the GPU suite holds to evalmap.density_filter / knn).  Without one: bad arguments end with
status 2 before anything is read or launched, and a missing input file is an I/O error, status 3."""
import subprocess

import numpy as np
import pytest

import erasor_amd
from test_label_scans_driver import DEMO, ensure_demo, read_pcd_binary, write_pcd_binary


def run(*args):
    return subprocess.run([DEMO] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def small_cloud():
    rng = np.random.default_rng(31)
    xyz = np.concatenate([rng.uniform(-3, 3, (1200, 3)) * [1, 1, 0.05], rng.uniform(-8, 8, (50, 3))])
    c = np.concatenate([xyz, rng.integers(245, 265, (len(xyz), 1))], 1).astype(np.float32)
    c[5, 3] = -1.0
    c[6, 0] = -0.0
    return np.ascontiguousarray(c)


def stats_line(name, r):
    return "  %s: min=%.9g  median=%.9g  p90=%.9g  p99=%.9g  max=%.9g" % ((name,) + tuple(r[k] for k in ("min", "median", "p90", "p99", "max")))


@pytest.mark.parametrize("args", [
    ("--denoise",), ("--denoise", "in.pcd"), ("--denoise", "in.pcd", "out.pcd"), ("--denoise", "in.pcd", "out.pcd", "sor"),
    ("--denoise", "in.pcd", "out.pcd", "sor", "8"), ("--denoise", "in.pcd", "out.pcd", "sor", "0", "2"), ("--denoise", "in.pcd", "out.pcd", "sor", "33", "2"),
    ("--denoise", "in.pcd", "out.pcd", "sor", "8", "-1"), ("--denoise", "in.pcd", "out.pcd", "sor", "8", "nan"), ("--denoise", "in.pcd", "out.pcd", "sor", "8.5", "2"),
    ("--denoise", "in.pcd", "out.pcd", "ror", "0", "3"), ("--denoise", "in.pcd", "out.pcd", "ror", "-0.5", "3"), ("--denoise", "in.pcd", "out.pcd", "ror", "0.5", "-3"),
    ("--denoise", "in.pcd", "out.pcd", "ror", "inf", "3"), ("--denoise", "in.pcd", "out.pcd", "kth", "8", "far"), ("--denoise", "in.pcd", "out.pcd", "kth", "40", "0.5"),
    ("--denoise", "in.pcd", "out.pcd", "sigma", "8", "2"), ("--denoise", "in.pcd", "out.pcd", "sor", "8", "2", "more"),
    ("--density",), ("--density", "cloud.pcd"), ("--density", "cloud.pcd", "0"), ("--density", "cloud.pcd", "33"), ("--density", "cloud.pcd", "many"),
    ("--density", "cloud.pcd", "8", "more"),
])
def test_bad_arguments_exit_with_status_2(args):
    ensure_demo()
    assert run(*args).returncode == 2


def test_a_missing_input_file_is_not_a_usage_error(tmp_path):
    ensure_demo()
    assert run("--denoise", "/nonexistent/in.pcd", tmp_path / "out.pcd", "sor", "8", "2").returncode == 3
    assert run("--density", "/nonexistent/cloud.pcd", "8").returncode == 3
    assert not (tmp_path / "out.pcd").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("how,a,b", [("sor", 8, 2.0), ("ror", 0.4, 3), ("kth", 4, 0.3)])
def test_denoise_prints_the_result_and_writes_the_kept_cloud(tmp_path, how, a, b):
    ensure_demo()
    cloud = small_cloud()
    write_pcd_binary(tmp_path / "in.pcd", cloud)
    out = run("--denoise", tmp_path / "in.pcd", tmp_path / "out.pcd", how, a, b)
    assert out.returncode == 0, out.stdout + out.stderr
    g = erasor_amd.Erasor(erasor_amd.params_default())
    kw = {"sor": dict(score="mean", k=a, rule="mad", mul=b), "ror": dict(score="count", radius=a, min_neighbors=b), "kth": dict(score="kth", k=a, rule="abs", thr=b)}[how]
    _, kept, r = g.density_filter(cloud, **kw)
    assert 0 < r["n_kept"] < len(cloud)
    lines = out.stdout.splitlines()
    assert lines[0] == "denoise: n=%d  kept=%d  removed=%d (dynamic %d, static %d)  short=%d  scored=%d" % tuple(
        r[k] for k in ("n_points", "n_kept", "n_removed", "n_removed_dynamic", "n_removed_static", "n_short", "n_scored"))
    assert lines[1] == stats_line({"sor": "mean", "ror": "count", "kth": "kth"}[how], r)
    assert lines[2] == "  m=%.9g  mad=%.9g  thr=%.9g" % (r["m"], r["mad"], r["thr"])
    assert lines[3] == "saved %s" % (tmp_path / "out.pcd") and len(lines) == 4
    assert read_pcd_binary(tmp_path / "out.pcd").tobytes() == kept.tobytes()


@pytest.mark.gpu
def test_density_prints_the_statistics(tmp_path):
    ensure_demo()
    cloud = small_cloud()
    write_pcd_binary(tmp_path / "c.pcd", cloud)
    out = run("--density", tmp_path / "c.pcd", 8)
    assert out.returncode == 0, out.stdout + out.stderr
    r = erasor_amd.Erasor(erasor_amd.params_default()).knn(cloud, 8)
    assert out.stdout.splitlines() == ["density: n=%d  k=8  short=%d  scored=%d" % (r["n_points"], r["n_short"], r["kth_stats"]["n_scored"]),
                                       stats_line("kth", r["kth_stats"]), stats_line("mean", r["mean_stats"])]
