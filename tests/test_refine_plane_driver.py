"""The offline driver's --refine-plane mode (erasor_offline_demo) on a tiny written-out sequence, as tests/test_refine_driver.py checks
--refine: the printed rows are the host restatement's (evalmap.refine_poses_plane, with evalmap.align_frames before and after), rank,
lambda_ratio and the plane rms included, and the pose file it writes reads back, through the project's own reader, as the refined poses
-- the lines of the frames it did not refine untouched.  Too few arguments: status 2; a missing input: a file error, not a usage error;
both without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import erasor_amd
import refine_world as rw
from erasor_amd import evalmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
DEMO = os.path.join(LIBDIR, "erasor_offline_demo")
STATUS = ("converged", "iteration limit", "too few pairs", "no finite points", "degenerate")


def ensure_demo():
    erasor_amd.build()
    cmd = ["make", "-C", os.path.join(ROOT, "erasor_amd", "csrc", "shim"), "-s"]
    if os.environ.get("ERASOR_TEST_SHIM_DIR"):
        cmd.append("LIBDIR=" + LIBDIR)
    subprocess.check_call(cmd)
    assert os.path.exists(DEMO)


def write_pcd_binary(path, c):
    with open(path, "wb") as f:
        f.write(("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                 "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (len(c), len(c))).encode())
        f.write(np.ascontiguousarray(c, np.float32).tobytes())


def load_poses(path, n):
    """(the file's poses, the poses after callback_node's round trip) through the shim's reader"""
    shim = C.CDLL(os.path.join(LIBDIR, "liberasor_shim.so"))
    shim.erasor_shim_load_poses.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    shim.erasor_shim_load_poses.restype = C.c_long
    T, geo, Tb = np.zeros((n, 16), np.float32), np.zeros((n, 7)), np.zeros((n, 16), np.float32)
    assert shim.erasor_shim_load_poses(str(path).encode(), T.ctypes.data, geo.ctypes.data, Tb.ctypes.data, n) == n
    return T.reshape(n, 4, 4), Tb.reshape(n, 4, 4)


def test_too_few_arguments_launch_nothing(tmp_path):
    ensure_demo()
    assert subprocess.run([DEMO, "--refine-plane", str(tmp_path / "a.yaml")], capture_output=True, timeout=60).returncode == 2
    assert subprocess.run([DEMO, "--refine-plane"], capture_output=True, timeout=60).returncode == 2


def test_a_missing_input_is_a_file_error(tmp_path):
    ensure_demo()
    out = subprocess.run([DEMO, "--refine-plane", str(tmp_path / "missing.yaml"), str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "cannot read" in out.stderr and "missing.yaml" in out.stderr
    # the YAML is there, the pose file is not
    (tmp_path / "seq").mkdir()
    yaml = tmp_path / "seq" / "rosparam.yaml"
    yaml.write_text('data_dir: "%s"\ninit_idx: 0\ntf:\n     lidar2body: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]\n' % (tmp_path / "seq"))
    out = subprocess.run([DEMO, "--refine-plane", str(yaml), str(tmp_path / "out.csv")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "poses_lidar2body.csv" in out.stderr and not (tmp_path / "out.csv").exists()


@pytest.mark.gpu
def test_driver_prints_the_restatements_rows_and_writes_a_pose_file_that_reads_back(tmp_path):
    ensure_demo()
    m = rw.world()[::3]
    n_all, n = 4, 3  # four frames on file, the first three refined
    scans, T_true, T_given = rw.frames(m, n_frames=n_all, every=10)
    far = scans[2].copy()
    far[:, 2] += np.float32(60.0)  # frame 2 sees nothing of the map: it keeps its pose and its line
    scans[2] = far
    d = tmp_path / "seq"
    (d / "pcds").mkdir(parents=True)
    for k in range(n_all):
        write_pcd_binary(d / "pcds" / ("%06d.pcd" % k), scans[k])
    write_pcd_binary(d / "dense_global_map.pcd", m)
    pose_lines = ["index,timestamp,x,y,z,qx,qy,qz,qw"]
    for k in range(n_all):
        T = T_given[k].astype(np.float64)
        q = Rotation.from_matrix(T[:3, :3]).as_quat()
        pose_lines.append("%d,%d,%s" % (k, 1000 + k, ",".join(repr(float(v)) for v in list(T[:3, 3]) + list(q))))
    (d / "poses_lidar2body.csv").write_text("\n".join(pose_lines) + "\n")
    yaml = d / "rosparam.yaml"
    yaml.write_text('data_dir: "%s"\ninit_idx: 0\ntf:\n     lidar2body: [0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0]\n' % d)
    out_csv = tmp_path / "refined.csv"
    out = subprocess.run([DEMO, "--refine-plane", str(yaml), str(out_csv), str(n), "0.8", "30", "12"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    # the poses the driver starts from: the CSV's, after callback_node's eigen2geoPose / geoPose2eigen round trip
    _, Tb = load_poses(d / "poses_lidar2body.csv", n_all)
    Tl = erasor_amd.geopose2eigen([0, 0, 0.25, 0, 0, 0, 1])
    T, rows, summ = evalmap.refine_poses_plane(m[:, :3], scans[:n], Tb[:n], Tl, k=12, max_dist=0.8, max_iters=30)
    before, _ = evalmap.align_frames(m[:, :3], scans[:n], Tb[:n], Tl, 0.2)
    after, _ = evalmap.align_frames(m[:, :3], scans[:n], T.astype(np.float32), Tl, 0.2)
    for k, r in enumerate(rows):
        flag = "" if r["status"] == 0 and not r["moved_t"] > 0.8 else (
            "  <- not converged: check this pose" if r["status"] != 0 else "  <- moved more than max_dist: check this pose")
        want = ("%6d  n=%d  <0.5*v %.2f%% -> %.2f%%  %s after %d  pairs %d -> %d  rms %.4fm -> %.4fm  moved %.4fm %.5frad"
                "  rank %d  lambda_ratio %.3g  plane rms %.4fm -> %.4fm%s%s") % (
            k, r["n_points"], before[k]["frac_half"], after[k]["frac_half"], STATUS[r["status"]], r["iters"], r["n_pairs_first"], r["n_pairs_last"],
            r["rms_first"], r["rms_last"], r["moved_t"], r["moved_r"], r["rank"], r["lambda_ratio"], r["rms_plane_first"], r["rms_plane_last"], flag,
            "  <- only %d of 6 directions constrained" % r["rank"] if r["status"] <= 1 and r["rank"] < 6 else "")
        assert want in lines, (want, out.stdout)
    assert [r["rank"] for r in rows] == [6, 6, 0] and "map points without one" in lines[0]
    assert [r["status"] for r in rows] == [0, 0, 2] and lines[-1] == "wrote %s" % out_csv
    assert lines[-2].startswith("summary: 2 converged, 0 at the iteration limit, 1 with too few pairs, 0 without finite points, 0 degenerate; "
                                "pairs %d -> %d, " % (summ["n_pairs_first"], summ["n_pairs_last"])) and ", plane rms " in lines[-2]
    # the file: the header, the index and timestamp of every line, and the lines of frames 2 (too few pairs) and 3 (not refined) as they were
    got = out_csv.read_text().splitlines()
    assert len(got) == len(pose_lines) and got[0] == pose_lines[0] and got[3] == pose_lines[3] and got[4] == pose_lines[4]
    assert all(g.split(",")[:2] == p.split(",")[:2] and len(g.split(",")) == 9 for g, p in zip(got[1:], pose_lines[1:]))
    # ... and it reads back, through the reader the run uses, as the refined poses: float32 of a unit quaternion's matrix
    T_file, T_run = load_poses(out_csv, n_all)
    for k in range(2):
        assert np.abs(T_file[k].astype(np.float64) - T[k]).max() < 2e-6 and np.abs(T_run[k].astype(np.float64) - T[k]).max() < 4e-6
        want = T_true[k] @ np.linalg.inv(Tl.astype(np.float64).reshape(4, 4))  # (the scans were cast from T_true with no lidar offset)
        assert rw.pose_error(T_run[k].astype(np.float64), want)[0] < 1e-3 < 0.1 < rw.pose_error(Tb[k].astype(np.float64), want)[0]
    assert T_file[3].tobytes() == load_poses(d / "poses_lidar2body.csv", n_all)[0][3].tobytes()
