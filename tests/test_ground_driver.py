"""The offline driver's --ground and --ground-map modes (erasor_offline_demo) on a tiny written-out sequence: the frame rows and the
results they print and the files they write -- the codes and the non-ground points per frame, the map's ground points and the rest --
are those of evalmap.ground_scans / ground_votes (and of Erasor.ground_*) on the same scans, map and poses: the poses after
callback_node's round trip, read through the project's own reader, and the uniform grid, whose expressions the driver restates with C's
tan.  Too few or malformed arguments: status 2; a missing input: a file error, not a usage error; both without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import erasor_amd
from erasor_amd import evalmap
from test_carve_driver import DEMO, ensure_demo, load_poses, read_pcd_binary, write_pcd_binary
from scipy.spatial.transform import Rotation


def write_sequence(d, n_all):
    """a labelled floor with boxes on it as the map; scans of that floor (1.75 m below the lidar) with returns from the boxes' height"""
    rng = np.random.default_rng(9)
    n = 6000
    r, az = 20.0 * np.sqrt(rng.uniform(0.01, 1.0, n)), rng.uniform(-np.pi, np.pi, n)
    z = -1.5 + rng.normal(0, 0.02, n)
    z[::7] += rng.uniform(0.3, 1.5, len(z[::7]))
    m = np.ascontiguousarray(np.stack([r * np.cos(az), r * np.sin(az), z, rng.choice([40.0, 252.0, 72.0], n)], 1).astype(np.float32))
    (d / "pcds").mkdir(parents=True)
    write_pcd_binary(d / "dense_global_map.pcd", m)
    lines, scans = ["index,timestamp,x,y,z,qx,qy,qz,qw"], []
    for k in range(n_all):
        rr, a = 25.0 * np.sqrt(rng.uniform(0.0, 1.0, 700)), rng.uniform(-np.pi, np.pi, 700)
        zz = -1.75 + rng.normal(0, 0.02, 700)
        zz[::5] += rng.uniform(0.3, 1.5, len(zz[::5]))
        s = np.stack([rr * np.cos(a), rr * np.sin(a), zz, rng.choice([40.0, 252.0], 700)], 1).astype(np.float32)
        s[0, 0], s[1, :2] = np.nan, 0.0  # one point of every scan is not finite and one is on the axis
        scans.append(s)
        write_pcd_binary(d / "pcds" / ("%06d.pcd" % k), s)
        q = Rotation.from_euler("z", 0.3 * k).as_quat()
        lines.append("%d,%d,%s" % (k, 1000 + k, ",".join(repr(float(v)) for v in [0.2 * k, -0.1 * k, 0.0] + list(q))))
    (d / "poses_lidar2body.csv").write_text("\n".join(lines) + "\n")
    yaml = d / "rosparam.yaml"
    yaml.write_text('data_dir: "%s"\ninit_idx: 0\ntf:\n     lidar2body: [0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0]\n' % d)
    return yaml, m, scans


def row_line(f, r, gathered=False):
    line = ("%6d  n=%d  dropped %d non-finite, %d out of range  judged %d  ground %d (dynamic %d)  patches %d: sparse %d, degenerate %d, "
            "not upright %d, elevated %d") % (f, r["n_points"], r["n_non_finite"], r["n_out_of_range"], r["n_judged"], r["n_ground"],
                                              r["n_ground_dynamic"], r["n_patches"], r["n_sparse"], r["n_degenerate"], r["n_rejected_upright"],
                                              r["n_rejected_elevation"])
    return line + ("  gathered %d" % r["n_gathered"] if gathered else "")


def test_too_few_or_malformed_arguments_launch_nothing(tmp_path):
    ensure_demo()
    y, o, o2 = str(tmp_path / "a.yaml"), str(tmp_path / "o"), str(tmp_path / "o2.pcd")
    for args in ([], [y], [y, o, "x"], [y, o, "-3"], [y, o, "3", "4"], [y, o, "3", "4", "16"], [y, o, "3", "0", "16", "30"], [y, o, "3", "65", "16", "30"],
                 [y, o, "3", "4", "12", "30"], [y, o, "3", "4", "520", "30"], [y, o, "3", "4", "16", "0.5"], [y, o, "3", "4", "16", "nan"],
                 [y, o, "3", "4", "16", "30", "extra"]):
        assert subprocess.run([DEMO, "--ground"] + args, capture_output=True, timeout=60).returncode == 2, args
    for args in ([], [y], [y, "-"], [y, "-", o2], [y, "-", o2, o2, "x"], [y, "-", o2, o2, "3", "-1"], [y, "-", o2, o2, "3", "1", "nan"],
                 [y, "-", o2, o2, "3", "1", "0.5", "extra"]):
        assert subprocess.run([DEMO, "--ground-map"] + args, capture_output=True, timeout=60).returncode == 2, args
    assert not os.path.exists(o) and not os.path.exists(o2)


def test_a_missing_input_is_a_file_error(tmp_path):
    ensure_demo()
    for mode, tail in (("--ground", [str(tmp_path)]), ("--ground-map", ["-", str(tmp_path / "g.pcd"), str(tmp_path / "r.pcd")])):
        out = subprocess.run([DEMO, mode, str(tmp_path / "missing.yaml")] + tail, capture_output=True, text=True, timeout=60)
        assert out.returncode == 3 and "cannot read" in out.stderr and "missing.yaml" in out.stderr
    yaml, _, _ = write_sequence(tmp_path / "seq", 1)
    out = subprocess.run([DEMO, "--ground-map", str(yaml), str(tmp_path / "no_map.pcd"), str(tmp_path / "g.pcd"), str(tmp_path / "r.pcd")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "no_map.pcd" in out.stderr and not (tmp_path / "g.pcd").exists()
    os.remove(tmp_path / "seq" / "pcds" / "000000.pcd")
    out = subprocess.run([DEMO, "--ground", str(yaml), str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 3 and "000000.pcd" in out.stderr and not (tmp_path / "000000.ground").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), ("4", "16", "30")])
def test_ground_prints_the_restatements_rows_and_writes_codes_and_the_rest(tmp_path, args):
    ensure_demo()
    n_all, n = 4, 3  # four frames on file, the first three used
    yaml, _, scans = write_sequence(tmp_path / "seq", n_all)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    out = subprocess.run([DEMO, "--ground", str(yaml), str(out_dir), str(n)] + list(args), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    grid = evalmap.ground_grid(int(args[0]), int(args[1]), 0.5, float(args[2])) if args else evalmap.ground_grid()
    want = evalmap.ground_scans(scans[:n], grid)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    codes, rows, res, _ = g.ground_scans(scans[:n], grid)
    assert codes.tobytes() == want[0].tobytes() and rows == want[1] and res == want[2]
    assert res["n_non_finite"] == n and res["n_out_of_range"] >= n and (not args or (res["n_ground"] > 0 and res["n_ground_dynamic"] > 0))
    assert lines[0] == "3 frames, %s rings x %s sectors between 0.5 and %s m:" % ((args[0], args[1], args[2]) if args else ("20", "64", "80"))
    o = 0
    for f, r in enumerate(rows):
        assert lines[1 + f] == row_line(f, r), (lines[1 + f], out.stdout)
        c = codes[o:o + len(scans[f])]
        o += len(scans[f])
        assert (out_dir / ("%06d.ground" % f)).read_bytes() == c.tobytes()
        assert read_pcd_binary(out_dir / ("%06d.pcd" % f)).tobytes() == scans[f][c != 1].tobytes()
    assert lines[4] == ("ground: frames=%d  n=%d  non-finite=%d  out of range=%d  judged=%d  ground=%d (dynamic %d)  patches=%d: sparse %d, degenerate %d, "
                        "not upright %d, elevated %d") % (3, res["n_points"], res["n_non_finite"], res["n_out_of_range"], res["n_judged"], res["n_ground"],
                                                          res["n_ground_dynamic"], res["n_patches"], res["n_sparse"], res["n_degenerate"],
                                                          res["n_rejected_upright"], res["n_rejected_elevation"])
    assert not (out_dir / "000003.ground").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), ("2", "0.75")])
def test_ground_map_prints_the_rows_and_saves_the_ground_and_the_rest(tmp_path, args):
    ensure_demo()
    n_all, n = 4, 3
    yaml, m, _ = write_sequence(tmp_path / "seq", n_all)
    gp, rp = tmp_path / "ground.pcd", tmp_path / "rest.pcd"
    out = subprocess.run([DEMO, "--ground-map", str(yaml), "-", str(gp), str(rp), str(n)] + list(args), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    Tb = load_poses(tmp_path / "seq" / "poses_lidar2body.csv", n_all)
    Tl = erasor_amd.geopose2eigen([0, 0, 0.25, 0, 0, 0, 1])
    kw = dict(min_votes=int(args[0]), ratio=float(args[1])) if args else {}
    want = evalmap.ground_votes(m, Tb[:n], Tl, None, **kw)
    g = erasor_amd.Erasor(erasor_amd.params_default())
    votes, mask, kept, rows, res = g.ground_votes(Tb[:n], Tl, m, None, **kw)
    assert votes.tobytes() == want[0].tobytes() and mask.tobytes() == want[1].tobytes() and kept.tobytes() == want[2].tobytes()
    assert rows == want[3] and res == want[4] and 0 < res["n_ground_dynamic"] < res["n_ground"] < len(m)
    assert lines[0].startswith("3 frames against ") and lines[0].endswith("(6000 points), min_votes %s, ratio %s:" % (args if args else ("1", "0.5")))
    for f, r in enumerate(rows):
        assert lines[1 + f] == row_line(f, r, gathered=True), (lines[1 + f], out.stdout)
    assert lines[4] == "ground-map: n=%d  ground=%d (dynamic %d, static %d)  unseen=%d  gathered=%d  judged=%d" % (
        res["n_points"], res["n_ground"], res["n_ground_dynamic"], res["n_ground_static"], res["n_unseen"], res["n_gathered"], res["n_judged"])
    assert lines[5:] == ["saved %s" % gp, "saved %s" % rp]
    assert read_pcd_binary(gp).tobytes() == m[mask == 1].tobytes() and read_pcd_binary(rp).tobytes() == m[mask == 0].tobytes()
