"""The offline driver's --carve mode (erasor_offline_demo) on a tiny written-out sequence: the frame rows and the result it prints and the
kept cloud it saves are those of evalmap.carve (and of Erasor.carve) on the same map, scans and poses -- the poses after callback_node's
round trip, read through the project's own reader, and OctoMap's default log-odds, whose expression the driver restates with C's log.
Too few or malformed arguments: status 2; a missing input: a file error, not a usage error; both without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import erasor_amd
from erasor_amd import evalmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
DEMO = os.path.join(LIBDIR, "erasor_offline_demo")


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


def read_pcd_binary(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"DATA binary\n", 1)
    n = int([l for l in head.decode().splitlines() if l.startswith("POINTS")][0].split()[1])
    return np.frombuffer(body, np.float32).reshape(n, 4)


def load_poses(path, n):
    """the poses after callback_node's round trip, through the shim's reader"""
    shim = C.CDLL(os.path.join(LIBDIR, "liberasor_shim.so"))
    shim.erasor_shim_load_poses.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    shim.erasor_shim_load_poses.restype = C.c_long
    T, geo, Tb = np.zeros((n, 16), np.float32), np.zeros((n, 7)), np.zeros((n, 16), np.float32)
    assert shim.erasor_shim_load_poses(str(path).encode(), T.ctypes.data, geo.ctypes.data, Tb.ctypes.data, n) == n
    return Tb.reshape(n, 4, 4)


def write_sequence(d, n_all):
    """map points on three cylinders around the origin, labelled; scans whose returns lie on those and on a fourth one beyond them, so
    that rays end in map voxels and pass through others"""
    rng = np.random.default_rng(8)
    az, z = rng.uniform(-np.pi, np.pi, 900), rng.uniform(-2.0, 1.0, 900)
    r = rng.choice([6.0, 9.0, 14.0], 900)
    m = np.ascontiguousarray(np.stack([r * np.cos(az), r * np.sin(az), z, rng.choice([40.0, 252.0, 72.0], 900)], 1).astype(np.float32))
    (d / "pcds").mkdir(parents=True)
    write_pcd_binary(d / "dense_global_map.pcd", m)
    lines, scans = ["index,timestamp,x,y,z,qx,qy,qz,qw"], []
    for k in range(n_all):
        a, zz = rng.uniform(-np.pi, np.pi, 400), rng.uniform(-2.0, 1.0, 400)
        rr = rng.choice([6.0, 9.0, 14.0, 20.0], 400) + rng.normal(0, 0.02, 400)
        s = np.stack([rr * np.cos(a), rr * np.sin(a), zz - 0.25, np.zeros(400)], 1).astype(np.float32)
        s[0, 0], s[1, :3] = np.nan, 0.1  # one point of every scan is not finite and one is too near
        scans.append(s)
        write_pcd_binary(d / "pcds" / ("%06d.pcd" % k), s)
        q = Rotation.from_euler("z", 0.3 * k).as_quat()
        lines.append("%d,%d,%s" % (k, 1000 + k, ",".join(repr(float(v)) for v in [0.2 * k, -0.1 * k, 0.0] + list(q))))
    (d / "poses_lidar2body.csv").write_text("\n".join(lines) + "\n")
    yaml = d / "rosparam.yaml"
    yaml.write_text('data_dir: "%s"\ninit_idx: 0\ntf:\n     lidar2body: [0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0]\n' % d)
    return yaml, m, scans


def test_too_few_or_malformed_arguments_launch_nothing(tmp_path):
    ensure_demo()
    y, o = str(tmp_path / "a.yaml"), str(tmp_path / "o.pcd")
    for args in ([], [y], [y, "-"], [y, "-", o, "x"], [y, "-", o, "-3"], [y, "-", o, "3", "0"], [y, "-", o, "3", "-0.2"], [y, "-", o, "3", "nan"],
                 [y, "-", o, "3", "0.2", "0.5"], [y, "-", o, "3", "0.2", "0.25"], [y, "-", o, "3", "0.01", "80"], [y, "-", o, "3", "0.2", "80", "65"],
                 [y, "-", o, "3", "0.2", "80", "1.5"], [y, "-", o, "3", "0.2", "80", "1", "extra"]):
        assert subprocess.run([DEMO, "--carve"] + args, capture_output=True, timeout=60).returncode == 2, args
    assert not os.path.exists(o)


def test_a_missing_input_is_a_file_error(tmp_path):
    ensure_demo()
    out = subprocess.run([DEMO, "--carve", str(tmp_path / "missing.yaml"), "-", str(tmp_path / "o.pcd")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "cannot read" in out.stderr and "missing.yaml" in out.stderr
    yaml, _, _ = write_sequence(tmp_path / "seq", 1)
    out = subprocess.run([DEMO, "--carve", str(yaml), str(tmp_path / "no_map.pcd"), str(tmp_path / "o.pcd")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no_map.pcd" in out.stderr and not (tmp_path / "o.pcd").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), ("0.25", "15", "2")])
def test_driver_prints_the_restatements_rows_and_saves_its_kept_cloud(tmp_path, args):
    ensure_demo()
    n_all, n = 4, 3  # four frames on file, the first three used
    yaml, m, scans = write_sequence(tmp_path / "seq", n_all)
    out_pcd = tmp_path / "kept.pcd"
    out = subprocess.run([DEMO, "--carve", str(yaml), "-", str(out_pcd), str(n)] + list(args), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    Tb = load_poses(tmp_path / "seq" / "poses_lidar2body.csv", n_all)
    Tl = erasor_amd.geopose2eigen([0, 0, 0.25, 0, 0, 0, 1])
    kw = dict(voxel=float(args[0]), max_range=float(args[1]), stop_short=int(args[2])) if args else {}  # (otherwise the documented defaults)
    want = evalmap.carve(m, scans[:n], Tb[:n], Tl, **kw)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    votes, lo, mask, kept, rows, res = g.carve(scans[:n], Tb[:n], Tl, m, **kw)
    assert rows == want[4] and res == want[5] and kept.tobytes() == want[3].tobytes() and lo.tobytes() == want[1].tobytes()
    assert res["n_removed"] > 0 and res["n_end_in_map"] > 0 and res["n_voxels_free"] > 0 and res["n_non_finite"] == n and res["n_out_of_range"] >= n
    for f, r in enumerate(rows):
        line = "%6d  n=%d  dropped %d non-finite, %d out of range  rays %d  steps %d  ends in the map %d  voxels hit %d, free %d" % (
            f, r["n_points"], r["n_non_finite"], r["n_out_of_range"], r["n_rays"], r["n_steps"], r["n_end_in_map"], r["n_voxels_hit"], r["n_voxels_free"])
        assert lines[1 + f] == line, (line, out.stdout)
    assert lines[0].startswith("3 frames against ") and lines[0].endswith(
        "(900 points), voxel %s, range 0.5 .. %s, stop_short %s:" % ((args[0], args[1], args[2]) if args else ("0.2", "80", "0")))
    assert lines[4] == "carve: n=%d  non-finite=%d  voxels=%d in %d blocks, touched %d  kept=%d  removed=%d (dynamic %d, static %d)" % (
        res["n_points"], res["n_map_non_finite"], res["n_voxels"], res["n_blocks"], res["n_voxels_touched"], res["n_kept"], res["n_removed"],
        res["n_removed_dynamic"], res["n_removed_static"])
    assert lines[5] == "  rays: %d of %d points (dropped %d non-finite, %d out of range)  steps %d  ends in the map %d  voxel hits %d, misses %d" % (
        res["n_rays"], res["n_scan_points"], res["n_non_finite"], res["n_out_of_range"], res["n_steps"], res["n_end_in_map"], res["n_voxels_hit"],
        res["n_voxels_free"])
    assert lines[6] == "saved %s" % out_pcd
    assert read_pcd_binary(out_pcd).tobytes() == kept.tobytes()
