"""The offline driver's --label-scans mode (erasor_offline_demo) on a tiny written-out sequence: the printed rows and summary are the host
oracle's (evalmap.label_scans / moving_iou), the .label files decode to its codes and the .pcd files hold its static rows, bit for
bit; with a raw map and without one.  Too few arguments: status 2, without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import erasor_amd
import scenarios
from erasor_amd import evalmap, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
DEMO = os.path.join(LIBDIR, "erasor_offline_demo")
MOS_ID = {0: 9, 1: 251, 2: 0, 255: 0}  # the driver's .label values: static, moving, unlabeled


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
    n = int([ln for ln in head.decode().splitlines() if ln.startswith("POINTS")][0].split()[1])
    assert len(body) == 16 * n, (path, n, len(body))
    return np.frombuffer(body, np.float32).reshape(n, 4)


def test_too_few_arguments_launch_nothing(tmp_path):
    ensure_demo()
    assert subprocess.run([DEMO, "--label-scans", str(tmp_path / "a.yaml"), "static.pcd", "-"], capture_output=True, timeout=60).returncode == 2


@pytest.mark.gpu
def test_driver_prints_the_oracles_summary_and_writes_its_codes_and_static_rows(tmp_path):
    ensure_demo()
    sc = scenarios.small()
    n = 3
    d, out_dir = tmp_path / "seq", tmp_path / "out"
    (d / "pcds").mkdir(parents=True)
    out_dir.mkdir()
    scans = []
    for k in range(n):
        s = np.ascontiguousarray(sc["scans"][k], np.float32)
        dyn = np.isin(evalmap.labels(s[:, 3]), evalmap.DYNAMIC_CLASSES)
        s = np.ascontiguousarray(np.concatenate([s[~dyn][::60], s[dyn][::4]]))  # a few hundred points, the moving ones among them
        s[1, 0] = np.nan                                                        # one point dropped
        scans.append(s)
        write_pcd_binary(d / "pcds" / ("%06d.pcd" % k), s)
    m = np.ascontiguousarray(sc["map"], np.float32)
    m_dyn = np.isin(evalmap.labels(m[:, 3]), evalmap.DYNAMIC_CLASSES)
    raw, static = np.ascontiguousarray(m[::3]), np.ascontiguousarray(m[~m_dyn][::5])
    write_pcd_binary(tmp_path / "static.pcd", static)
    write_pcd_binary(tmp_path / "raw.pcd", raw)
    with open(d / "poses_lidar2body.csv", "w") as f:
        f.write("index,timestamp,x,y,z,qx,qy,qz,qw\n")
        for k in range(n):
            f.write("%d,%d,%s\n" % (k, 1000 + k, ",".join(repr(float(v)) for v in sc["poses"][k])))
    yaml = d / "rosparam.yaml"
    yaml.write_text('data_dir: "%s"\ninit_idx: 0\ntf:\n     lidar2body: [0.0, 0.0, %r, 0.0, 0.0, 0.0, 1.0]\n' % (d, float(synth.LIDAR_HEIGHT)))
    # the poses the run uses: the CSV's, after callback_node's eigen2geoPose / geoPose2eigen round trip
    shim = C.CDLL(os.path.join(LIBDIR, "liberasor_shim.so"))
    shim.erasor_shim_load_poses.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    shim.erasor_shim_load_poses.restype = C.c_long
    T, geo, Tb = np.zeros((n, 16), np.float32), np.zeros((n, 7)), np.zeros((n, 16), np.float32)
    assert shim.erasor_shim_load_poses(str(d / "poses_lidar2body.csv").encode(), T.ctypes.data, geo.ctypes.data, Tb.ctypes.data, n) == n
    Tl = erasor_amd.geopose2eigen([0, 0, synth.LIDAR_HEIGHT, 0, 0, 0, 1])
    for raw_arg, raw_xyz, tau_args, tau in ((str(tmp_path / "raw.pcd"), raw[:, :3], [str(n), "0.3"], 0.3), ("-", None, [], evalmap.label_tau(0.2))):
        for f in out_dir.iterdir():
            f.unlink()
        out = subprocess.run([DEMO, "--label-scans", str(yaml), str(tmp_path / "static.pcd"), raw_arg, str(out_dir)] + tau_args, capture_output=True,
                             text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        codes, rows, summary, clouds = evalmap.label_scans(static[:, :3], scans, Tb, Tl, raw_xyz=raw_xyz, tau=tau, split=0)
        for k, r in enumerate(rows):
            by_code = [r["n"][0][c] + r["n"][1][c] for c in range(3)]
            want = "%6d  n=%d  static=%d  dynamic=%d  unknown=%d  dropped=%d  moving IoU=%.4f" % (
                k, r["n_points"], by_code[0], by_code[1], by_code[2], r["n_non_finite"], evalmap.moving_iou(r)["IoU"])
            assert want in lines, (want, out.stdout)
            got = np.fromfile(out_dir / ("%06d.label" % k), "<u4")
            assert got.tolist() == [MOS_ID[int(c)] for c in codes[k]]
            assert read_pcd_binary(out_dir / ("%06d.pcd" % k)).tobytes() == clouds[k].tobytes()
        s = evalmap.moving_iou(summary)
        want = ["summary: n=%d  dropped=%d  labels out of range=%d" % (summary["n_points"], summary["n_non_finite"], summary["n_label_out_of_range"]),
                "  own label static: static=%d dynamic=%d unknown=%d" % tuple(summary["n"][0]),
                "  own label moving: static=%d dynamic=%d unknown=%d" % tuple(summary["n"][1]),
                "  moving: TP=%d FP=%d FN=%d  IoU=%.6f  precision=%.6f  recall=%.6f" % (s["TP"], s["FP"], s["FN"], s["IoU"], s["precision"], s["recall"])]
        assert lines[-4:] == want, out.stdout
        assert summary["n_non_finite"] == n and s["TP"] > 0 and summary["n"][0][0] > 0
        assert (raw_xyz is None) == (summary["n"][0][2] + summary["n"][1][2] == 0)
