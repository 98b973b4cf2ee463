"""The offline driver's --objects mode (erasor_offline_demo).  On a GPU: the scene whose answer is written out by hand, as PCD files --
the raw map, the ground cloud and a method's kept cloud -- gives the printed result and the kept cloud of evalmap.object_vote.  Without
one: bad arguments end with status 2 before anything is read or launched, and a missing input file is an I/O error, status 3."""
import subprocess

import numpy as np
import pytest

import object_scenes as S
from erasor_amd import evalmap
from test_label_scans_driver import DEMO, ensure_demo, read_pcd_binary, write_pcd_binary

GOOD = ["raw.pcd", "-", "out.pcd", "0.3", "1", "0.5", "0.05", "500", "kept.pcd"]


def run(*args):
    return subprocess.run([DEMO] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def changed(k, v):
    a = list(GOOD)
    a[k] = v
    return a


@pytest.mark.parametrize("args", [
    [], GOOD[:3], GOOD[:8], changed(3, "0"), changed(3, "-0.3"), changed(3, "nan"), changed(3, "wide"), changed(4, "0"), changed(4, "256"), changed(4, "1.5"),
    changed(5, "0"), changed(5, "1.1"), changed(5, "half"), changed(6, "-0.1"), changed(6, "0.5"), changed(6, "0.7"), changed(6, "1"), changed(7, "-1"),
    changed(7, "many"), GOOD + ["--tau", "0"], GOOD + ["--tau", "-1"], GOOD + ["--tau", "near"], GOOD[:8] + ["--tau", "0.1"],
])
def test_bad_arguments_exit_with_status_2(args):
    ensure_demo()
    out = run("--objects", *args)
    assert out.returncode == 2 and "usage" in out.stderr


def test_a_missing_input_file_is_not_a_usage_error(tmp_path):
    ensure_demo()
    cloud, _, _ = S.known_scene()
    write_pcd_binary(tmp_path / "raw.pcd", cloud)
    a = [tmp_path / "raw.pcd", "-", tmp_path / "out.pcd"] + GOOD[3:8]
    for args, name in ((changed(0, "/nonexistent/raw.pcd"), "raw.pcd"), (a + ["/nonexistent/kept.pcd"], "kept.pcd"),
                       ([a[0], "/nonexistent/ground.pcd"] + a[2:] + [tmp_path / "raw.pcd"], "ground.pcd"),
                       (a + [tmp_path / "raw.pcd", "/nonexistent/kept2.pcd", "--tau", "0.05"], "kept2.pcd")):
        out = run("--objects", *args)
        assert out.returncode == 3 and "cannot read" in out.stderr and name in out.stderr, (args, out.stderr)
    assert not (tmp_path / "out.pcd").exists()


@pytest.mark.gpu
def test_objects_prints_the_result_and_writes_the_kept_cloud(tmp_path):
    ensure_demo()
    cloud, votes, ground = S.known_scene()
    write_pcd_binary(tmp_path / "raw.pcd", cloud)
    write_pcd_binary(tmp_path / "ground.pcd", cloud[ground != 0])
    write_pcd_binary(tmp_path / "kept.pcd", cloud[votes == 0])  # a method's kept cloud: a subset of the raw map
    # (the wall's points are 0.1 m apart, below the default tau: a removed point is voted only when no kept point is that near)
    out = run("--objects", tmp_path / "raw.pcd", tmp_path / "ground.pcd", tmp_path / "out.pcd", 0.3, 1, 0.5, 0.05, 500, tmp_path / "kept.pcd", "--tau", 0.05)
    assert out.returncode == 0, out.stdout + out.stderr
    mask, rows, res = S.known_answer()
    want = evalmap.object_vote(cloud, votes, ground, **S.KNOWN_PARAMS)
    assert want[4] == res and want[0].tobytes() == mask.tobytes()
    lines = out.stdout.splitlines()
    assert lines[0] == "objects: n=1531  ground=256  clusters=4  touched=4  removed=1  reverted=1  not objects=1  largest=900"
    assert lines[1] == "points: voted=733  removed=765  grown=45 (dynamic 45)  reverted=3 (dynamic 0)  ground reverted=10 (dynamic 0)"
    assert lines[2].startswith("  first=631  n=900  voted=600  dynamic=0 (0.0%)  not an object  box=[3.000 3.750 0.200]..[5.900 3.750 3.100]")
    assert lines[3].startswith("  first=256  n=125  voted=80  dynamic=125 (100.0%)  removed  ")
    assert lines[4].startswith("  first=381  n=125  voted=3  dynamic=0 (0.0%)  reverted  ") and lines[5].startswith("  first=506  n=125  voted=40  ")
    assert lines[6:10] == ["unchanged: clusters=1  points=125  dynamic=0 (0.0%)", "removed: clusters=1  points=125  dynamic=125 (100.0%)",
                           "reverted: clusters=1  points=125  dynamic=0 (0.0%)", "not an object: clusters=1  points=900  dynamic=0 (0.0%)"]
    assert lines[10] == "saved %s" % (tmp_path / "out.pcd") and len(lines) == 11
    assert read_pcd_binary(tmp_path / "out.pcd").tobytes() == want[3].tobytes() == cloud[mask != 0].tobytes()
    # two methods and their majority: the same kept cloud twice and the raw map once is vote_thr 2 of 3
    out = run("--objects", tmp_path / "raw.pcd", tmp_path / "ground.pcd", tmp_path / "out2.pcd", 0.3, 2, 0.5, 0.05, 500, tmp_path / "kept.pcd",
              tmp_path / "raw.pcd", tmp_path / "kept.pcd", "--tau", 0.05)
    assert out.returncode == 0, out.stdout + out.stderr
    assert read_pcd_binary(tmp_path / "out2.pcd").tobytes() == want[3].tobytes()
    # a method that removed everything: its empty kept cloud votes every raw point out, and only the ground stays
    write_pcd_binary(tmp_path / "none.pcd", cloud[:0])
    out = run("--objects", tmp_path / "raw.pcd", tmp_path / "ground.pcd", tmp_path / "out3.pcd", 0.3, 1, 0.5, 0.05, 500, tmp_path / "none.pcd", "--tau", 0.05)
    assert out.returncode == 0, out.stdout + out.stderr
    all_voted = evalmap.object_vote(cloud, np.ones(len(cloud), np.uint8), ground, **S.KNOWN_PARAMS)
    assert out.stdout.splitlines()[1].startswith("points: voted=1531  removed=1275  grown=0 ") and all_voted[4]["n_removed"] == 1275
    assert read_pcd_binary(tmp_path / "out3.pcd").tobytes() == all_voted[3].tobytes() == cloud[ground != 0].tobytes()
