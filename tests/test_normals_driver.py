"""The offline driver's --normals mode (erasor_offline_demo).  On a GPU: the printed counts and statistics are those of the Python call
(which the GPU suite holds to evalmap.normals) and the written cloud's eight fields are the input rows, the normals and the curvature
cast to float32, byte for byte; with a viewpoint and without one.  Without a GPU: bad arguments end with status 2 before anything is
read or launched, and a missing input file is an I/O error, status 3, with nothing written."""
import subprocess

import numpy as np
import pytest

import erasor_amd
from test_label_scans_driver import DEMO, ensure_demo, write_pcd_binary

FIELDS = "x y z intensity normal_x normal_y normal_z curvature"


def run(*args):
    return subprocess.run([DEMO] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def small_cloud():
    rng = np.random.default_rng(41)
    xyz = np.concatenate([rng.uniform(-3, 3, (1200, 3)) * [1, 1, 0.05], rng.uniform(-8, 8, (50, 3)), np.tile([[5.0, 5.0, 5.0]], (20, 1))])
    c = np.concatenate([xyz, rng.integers(245, 265, (len(xyz), 1))], 1).astype(np.float32)
    c[5, 3] = -1.0
    c[6, 0] = -0.0
    return np.ascontiguousarray(c)


def read_pcd_normals(path):
    """the eight-field binary file: (n, 8) float32"""
    raw = open(path, "rb").read()
    head, body = raw.split(b"DATA binary\n", 1)
    lines = head.decode().splitlines()
    get = lambda key: [ln for ln in lines if ln.startswith(key + " ")][0][len(key) + 1:]
    assert get("FIELDS") == FIELDS and get("SIZE") == "4 4 4 4 4 4 4 4" and get("TYPE") == "F F F F F F F F" and get("COUNT") == "1 1 1 1 1 1 1 1"
    n = int(get("POINTS"))
    assert int(get("WIDTH")) == n and get("HEIGHT") == "1" and len(body) == 32 * n, (path, n, len(body))
    return np.frombuffer(body, np.float32).reshape(n, 8)


@pytest.mark.parametrize("args", [
    ("--normals",), ("--normals", "in.pcd"), ("--normals", "in.pcd", "out.pcd"), ("--normals", "in.pcd", "out.pcd", "1"),
    ("--normals", "in.pcd", "out.pcd", "0"), ("--normals", "in.pcd", "out.pcd", "33"), ("--normals", "in.pcd", "out.pcd", "8.5"),
    ("--normals", "in.pcd", "out.pcd", "many"), ("--normals", "in.pcd", "out.pcd", "8", "1.0"), ("--normals", "in.pcd", "out.pcd", "8", "1.0", "2.0"),
    ("--normals", "in.pcd", "out.pcd", "8", "1.0", "2.0", "nan"), ("--normals", "in.pcd", "out.pcd", "8", "inf", "2.0", "3.0"),
    ("--normals", "in.pcd", "out.pcd", "8", "1.0", "up", "3.0"), ("--normals", "in.pcd", "out.pcd", "8", "1.0", "2.0", "3.0", "more"),
])
def test_bad_arguments_exit_with_status_2(args):
    ensure_demo()
    assert run(*args).returncode == 2


def test_a_missing_input_file_is_not_a_usage_error(tmp_path):
    ensure_demo()
    assert run("--normals", "/nonexistent/in.pcd", tmp_path / "out.pcd", "8").returncode == 3
    assert run("--normals", "/nonexistent/in.pcd", tmp_path / "out.pcd", "8", "0", "0", "10").returncode == 3
    assert not (tmp_path / "out.pcd").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("k,vp", [(8, None), (16, (0.5, -0.25, 30.0)), (2, (0.0, 0.0, -7.5))])
def test_normals_prints_the_result_and_writes_the_eight_fields(tmp_path, k, vp):
    ensure_demo()
    cloud = small_cloud()
    write_pcd_binary(tmp_path / "in.pcd", cloud)
    out = run("--normals", tmp_path / "in.pcd", tmp_path / "out.pcd", k, *([] if vp is None else [repr(v) for v in vp]))
    assert out.returncode == 0, out.stdout + out.stderr
    nrm, curv, _, r = erasor_amd.Erasor(erasor_amd.params_default()).normals(cloud, k, vp)
    st = r["curvature_stats"]
    assert r["n_degenerate"] == 20 and 0 < r["n_flipped"] < len(cloud)
    assert out.stdout.splitlines() == [
        "normals: n=%d  k=%d  short=%d  degenerate=%d  ambiguous=%d  flipped=%d  scored=%d" % (
            r["n_points"], k, r["n_short"], r["n_degenerate"], r["n_ambiguous"], r["n_flipped"], st["n_scored"]),
        "  curvature: min=%.9g  median=%.9g  p90=%.9g  p99=%.9g  max=%.9g" % tuple(st[f] for f in ("min", "median", "p90", "p99", "max")),
        "saved %s" % (tmp_path / "out.pcd")]
    want = np.concatenate([cloud, nrm, curv.astype(np.float32)[:, None]], 1)
    assert read_pcd_normals(tmp_path / "out.pcd").tobytes() == np.ascontiguousarray(want, np.float32).tobytes()
