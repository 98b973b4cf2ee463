"""The offline driver's bird's-eye modes (erasor_offline_demo --render / --render-compare / --render-eval) and the shim's PPM writer:
the file's header and size without a GPU; on the GPU (marked gpu) the written images against Erasor.render / render_eval on the same
tiny PCDs, the panel count of --render-compare and the printed evaluation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import erasor_amd

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


def clouds():
    rng = np.random.default_rng(20261016)
    n = 3000
    gt = np.zeros((n, 4), np.float32)
    gt[:, :2] = rng.uniform(-12, 12, (n, 2))
    gt[:, 2] = rng.normal(0, 1, n)
    gt[:, 3] = rng.choice([40.0, 70.0, 252.0, 65536.0 * 2 + 253.0], n, p=[0.5, 0.3, 0.1, 0.1])
    dyn = (gt[:, 3].astype(np.uint32) & 0xFFFF) >= 252
    est = np.concatenate([gt[~dyn][::2], gt[dyn][::3]])
    return gt, np.ascontiguousarray(est)


def test_the_shims_ppm_writer_header_and_size(tmp_path):
    ensure_demo()
    shim = C.CDLL(os.path.join(LIBDIR, "liberasor_shim.so"))
    shim.erasor_shim_write_ppm.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
    shim.erasor_shim_write_ppm.restype = C.c_int
    img = np.random.default_rng(1).integers(0, 256, (5, 7, 3)).astype(np.uint8)
    p = tmp_path / "a.ppm"
    assert shim.erasor_shim_write_ppm(str(p).encode(), img.ctypes.data, 7, 5) == 0
    raw = p.read_bytes()
    assert raw[:11] == b"P6\n7 5\n255\n" and len(raw) == 11 + 5 * 7 * 3
    assert (erasor_amd.read_ppm(str(p)) == img).all()
    assert shim.erasor_shim_write_ppm(str(tmp_path / "no_such_dir" / "a.ppm").encode(), img.ctypes.data, 7, 5) == -1
    # too few arguments: status 2, nothing launched
    for mode in ("--render", "--render-compare", "--render-eval"):
        assert subprocess.run([DEMO, mode, str(p)], capture_output=True, timeout=60).returncode == 2


@pytest.mark.gpu
def test_driver_render_modes_write_the_images_the_library_renders(tmp_path):
    ensure_demo()
    gt, est = clouds()
    fg, fe = tmp_path / "gt.pcd", tmp_path / "est.pcd"
    write_pcd_binary(fg, gt)
    write_pcd_binary(fe, est)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    v = g.render_fit(gt, 0.25)
    # --render: viz_kitti_map's picture, with a class and an instance
    out = subprocess.run([DEMO, "--render", str(tmp_path / "m.ppm"), str(fg), "0.25", "253", "2"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    img, st = g.render(gt, v, target_class=253, target_instance=2)
    got = erasor_amd.read_ppm(str(tmp_path / "m.ppm"))
    assert got.shape == (v["height"], v["width"], 3) and (got == img).all() and st["cat_points"][2] > 0
    assert "%u x %u pixels" % (v["width"], v["height"]) in out.stdout and "points %d drawn %d" % (len(gt), st["n_drawn"]) in out.stdout
    # --render-compare: one panel per file, all in the first one's view
    out = subprocess.run([DEMO, "--render-compare", str(tmp_path / "c.ppm"), "0.25", str(fg), str(fe), str(fg)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = erasor_amd.read_ppm(str(tmp_path / "c.ppm"))
    want = erasor_amd.hstack_panels([g.render(gt, v)[0], g.render(est, v)[0], g.render(gt, v)[0]], gap=4)
    assert got.shape == want.shape == (v["height"], 3 * v["width"] + 8, 3) and (got == want).all()
    assert "3 panel(s)" in out.stdout and out.stdout.count("panel ") == 3
    # --render-eval: --eval's table and the error map
    out = subprocess.run([DEMO, "--render-eval", str(tmp_path / "e.ppm"), str(fg), str(fe), "0.2", "0", "0.25"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    img, st, ev = g.render_eval(gt, est, v)
    assert (erasor_amd.read_ppm(str(tmp_path / "e.ppm")) == img).all()
    plain = subprocess.run([DEMO, "--eval", str(fg), str(fe)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout in out.stdout
    assert "dynamic left" in out.stdout and str(ev["preserved_dynamic"]) in out.stdout
