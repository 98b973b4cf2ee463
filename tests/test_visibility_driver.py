"""The offline driver's --visibility mode (erasor_offline_demo) on a tiny written-out sequence: the frame rows and the result it prints and
the kept cloud it saves are those of the Python call (Erasor.visibility) on the same map, scans and poses -- the poses after
callback_node's round trip, read through the project's own reader, and the edge tables from visibility_grid, whose expressions the
driver restates with C's tan.  Too few or malformed arguments: status 2; a missing input: a file error, not a usage error; both without
a GPU."""
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
    """a wall of map points around the origin, labelled; scans that see part of it, some returns short of it and some beyond"""
    rng = np.random.default_rng(8)
    az, z = rng.uniform(-np.pi, np.pi, 900), rng.uniform(-2.0, 1.0, 900)
    az = np.where(np.abs(az) < 0.6, az + np.pi, az)  # (nothing of the wall ahead, where the strip of ground below lies)
    r = rng.choice([6.0, 9.0, 14.0], 900)
    m = np.stack([r * np.cos(az), r * np.sin(az), z, rng.choice([40.0, 252.0, 72.0], 900)], 1).astype(np.float32)
    # a strip of ground ahead, seen by frame 0 from 1.75 m above with a return behind every point of it: from 8 m on the incidence is
    # beyond min_cos = 0.25 (1.75 / 8.2 = 0.21), so with k > 0 those see-throughs are grazing
    gx, gy = np.meshgrid(np.arange(6.0, 12.5, 0.5), np.arange(-2.0, 2.5, 0.5), indexing="ij")
    strip = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -1.5), np.full(gx.size, 40.0)], 1).astype(np.float32)
    m = np.ascontiguousarray(np.concatenate([m, strip]))
    (d / "pcds").mkdir(parents=True)
    write_pcd_binary(d / "dense_global_map.pcd", m)
    lines, scans = ["index,timestamp,x,y,z,qx,qy,qz,qw"], []
    for k in range(n_all):
        a, zz = rng.uniform(-np.pi, np.pi, 400), rng.uniform(-2.0, 1.0, 400)
        rr = rng.choice([6.0, 9.0, 14.0, 20.0], 400) + rng.normal(0, 0.02, 400)
        s = np.stack([rr * np.cos(a), rr * np.sin(a), zz - 0.25, np.zeros(400)], 1).astype(np.float32)
        if k == 0:  # (frame 0: no rotation, the lidar 0.25 m above the origin; its other returns are not ahead)
            s = s[np.abs(a) >= 0.6]
            behind = strip.copy()
            behind[:, :3] = 1.5 * (strip[:, :3] - np.float32([0, 0, 0.25]))
            s = np.ascontiguousarray(np.concatenate([s, behind]))
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
    for args in ([], [y], [y, "-"], [y, "-", o, "3", "64"], [y, "-", o, "3", "64", "16", "-20"], [y, "-", o, "3", "60", "16", "-20", "10"],
                 [y, "-", o, "3", "64", "0", "-20", "10"], [y, "-", o, "3", "64", "16", "10", "-20"], [y, "-", o, "3", "64", "16", "-20", "10", "3"],
                 [y, "-", o, "3", "64", "16", "-20", "10", "1", "1"], [y, "-", o, "3", "64", "16", "-20", "10", "1", "8", "extra"]):
        assert subprocess.run([DEMO, "--visibility"] + args, capture_output=True, timeout=60).returncode == 2, args
    assert not os.path.exists(o)


def test_a_missing_input_is_a_file_error(tmp_path):
    ensure_demo()
    out = subprocess.run([DEMO, "--visibility", str(tmp_path / "missing.yaml"), "-", str(tmp_path / "o.pcd")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "cannot read" in out.stderr and "missing.yaml" in out.stderr
    yaml, _, _ = write_sequence(tmp_path / "seq", 1)
    out = subprocess.run([DEMO, "--visibility", str(yaml), str(tmp_path / "no_map.pcd"), str(tmp_path / "o.pcd")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no_map.pcd" in out.stderr and not (tmp_path / "o.pcd").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 6])
def test_driver_prints_the_python_calls_rows_and_saves_its_kept_cloud(tmp_path, k):
    ensure_demo()
    n_all, n = 4, 3  # four frames on file, the first three used
    yaml, m, scans = write_sequence(tmp_path / "seq", n_all)
    out_pcd = tmp_path / "kept.pcd"
    out = subprocess.run([DEMO, "--visibility", str(yaml), "-", str(out_pcd), str(n), "64", "8", "-22.5", "12.5", "1", str(k)], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    Tb = load_poses(tmp_path / "seq" / "poses_lidar2body.csv", n_all)
    Tl = erasor_amd.geopose2eigen([0, 0, 0.25, 0, 0, 0, 1])
    grid = erasor_amd.visibility_grid(64, 8, -22.5, 12.5)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    votes, mask, kept, rows, res = g.visibility(scans[:n], Tb[:n], Tl, m, grid, window=1, k=k)  # (the other parameters: the documented defaults)
    want = evalmap.visibility(m, scans[:n], Tb[:n], Tl, grid, window=1, k=k)
    assert rows == want[3] and res == want[4] and kept.tobytes() == want[2].tobytes()
    assert res["n_removed"] > 0 and res["n_hit"] > 0 and res["n_occluded"] > 0 and (k == 0 or res["n_grazing"] > 0)
    for f, r in enumerate(rows):
        line = ("%6d  n=%d  dropped %d non-finite, %d on the axis, %d out of range, %d out of view  pixels %d  map in view %d: hit %d, occluded %d, "
                "no return %d, through %d, grazing %d") % (f, r["n_points"], r["n_non_finite"], r["n_on_axis"], r["n_out_of_range"], r["n_out_of_view"],
                                                           r["n_pixels"], r["n_map_in_view"], r["n_hit"], r["n_occluded"], r["n_no_return"], r["n_through"],
                                                           r["n_grazing"])
        assert lines[1 + f] == line, (line, out.stdout)
    assert lines[0].startswith("3 frames against ") and lines[0].endswith("(1017 points), 64 x 8 pixels between -22.5 and 12.5 degrees, window 1, k %d:" % k)
    assert lines[4] == "visibility: n=%d  never in view=%d  kept=%d  removed=%d (dynamic %d, static %d)  without a normal=%d" % (
        res["n_points"], res["n_never_in_view"], res["n_kept"], res["n_removed"], res["n_removed_dynamic"], res["n_removed_static"], res["n_map_no_normal"])
    assert lines[5] == "  verdicts: in view %d  hit %d  occluded %d  no return %d  through %d  grazing %d" % (
        res["n_in_view"], res["n_hit"], res["n_occluded"], res["n_no_return"], res["n_through"], res["n_grazing"])
    assert lines[6] == "saved %s" % out_pcd
    assert read_pcd_binary(out_pcd).tobytes() == kept.tobytes()
