"""The offline driver's sweep grid (erasor_offline_demo --sweep) expanded on the host through erasor_shim_expand_grid: the Cartesian
product of the grid file's flow lists in file order with the last axis varying fastest, scalars overriding the base file, lists of ints
and floats, a key a grid may not set, the 256-configuration limit.  CPU only: no kernel is launched."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BASE = """erasor:
    max_range: 80.0
    num_rings: 20
    num_sectors: 108
    max_h: 3.1
    min_h: -0.5
    scan_ratio_threshold: 0.2
    minimum_num_pts: 5
    version: 3
MapUpdater:
    data_name: "05"
    env: "outdoor"
    query_voxel_size: 0.2
    removal_interval: 2
large_scale:
    is_large_scale: false
    submap_size: 200.0
data_dir: "/data/05"
init_idx: 3
tf:
    lidar2body: [0.0, 0.0, 1.73, 0, 0.0, 0.0, 1.0]
"""


@pytest.fixture(scope="module")
def shim():
    import erasor_amd
    erasor_amd.build()
    lib = C.CDLL(os.path.join(ROOT, "erasor_amd", "liberasor_shim.so"))
    lib.erasor_shim_expand_grid.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    lib.erasor_shim_expand_grid.restype = C.c_int
    return lib


def expand(shim, tmp_path, grid, cap=1 << 22):
    b, g = tmp_path / "base.yaml", tmp_path / "grid.yaml"
    b.write_text(BASE)
    g.write_text(grid)
    buf = C.create_string_buffer(cap)
    rc = shim.erasor_shim_expand_grid(str(b).encode(), str(g).encode(), buf, cap)
    if rc < 0:
        return rc, buf.value.decode()
    blocks = [blk for blk in buf.value.decode().split("\n\n") if blk.strip()]
    return rc, [dict(line.split("=", 1) for line in blk.strip().split("\n")) for blk in blocks]


def test_axes_in_file_order_last_fastest(shim, tmp_path):
    rc, cfgs = expand(shim, tmp_path, "erasor:\n    scan_ratio_threshold: [0.1, 0.2, 0.3]\n    max_h: [2.8, 3.2]\n")
    assert rc > 0 and len(cfgs) == 6
    got = [(float(c["scan_ratio_threshold"]), float(c["max_h"])) for c in cfgs]
    assert got == [(0.1, 2.8), (0.1, 3.2), (0.2, 2.8), (0.2, 3.2), (0.3, 2.8), (0.3, 3.2)]
    for c in cfgs:  # everything else is the base file's
        assert c["num_sectors"] == "108" and float(c["min_h"]) == -0.5 and c["removal_interval"] == "2" and c["init_idx"] == "3"
        assert c["data_dir"] == "/data/05" and c["lidar2body"].split(",")[2] == "1.73" and float(c["voi_max_range"]) == 80.0


def test_scalars_override_the_base_and_lists_of_ints(shim, tmp_path):
    grid = ("MapUpdater:\n    removal_interval: [1, 2, 3]\nerasor:\n    minimum_num_pts: 7\n    version: [2, 3]\n"
            "large_scale:\n    is_large_scale: true\n    submap_size: 25\n")
    rc, cfgs = expand(shim, tmp_path, grid)
    assert rc > 0 and len(cfgs) == 6
    assert [(c["removal_interval"], c["version"]) for c in cfgs] == [("1", "2"), ("1", "3"), ("2", "2"), ("2", "3"), ("3", "2"), ("3", "3")]
    for c in cfgs:
        assert c["minimum_num_pts"] == "7" and c["is_large_scale"] == "1" and float(c["submap_size"]) == 25.0


def test_max_range_sets_the_voi_radius_too(shim, tmp_path):
    rc, cfgs = expand(shim, tmp_path, "erasor:\n    max_range: [60, 80.5]\n")
    assert [(float(c["max_range"]), float(c["voi_max_range"])) for c in cfgs] == [(60.0, 60.0), (80.5, 80.5)]


def test_no_axis_is_one_configuration(shim, tmp_path):
    rc, cfgs = expand(shim, tmp_path, "erasor:\n    max_h: 2.9\n")
    assert len(cfgs) == 1 and float(cfgs[0]["max_h"]) == 2.9


@pytest.mark.parametrize("key", ["MapUpdater:\n    data_name: [a, b]", "erasor:\n    not_a_parameter: [1, 2]", "tf:\n    lidar2body: 1",
                                 "data_dir: /x", "MapUpdater:\n    initial_map_path: /m.pcd"])
def test_unknown_keys_are_refused_by_name(shim, tmp_path, key):
    rc, msg = expand(shim, tmp_path, key + "\n")
    assert rc == -2
    assert msg.startswith("/") and msg.split("/")[-1] == key.split(":")[-2].strip().split("\n")[-1].strip()


def test_256_configurations_at_most(shim, tmp_path):
    rc, cfgs = expand(shim, tmp_path, "erasor:\n    max_h: [%s]\n    min_h: [%s]\n" % (", ".join("%d" % (i + 1) for i in range(16)),
                                                                                     ", ".join("-%d" % i for i in range(16))))
    assert rc > 0 and len(cfgs) == 256
    assert (cfgs[17]["max_h"], cfgs[17]["min_h"]) == ("2", "-1")
    rc, _ = expand(shim, tmp_path, "erasor:\n    max_h: [%s]\n    min_h: [%s]\n" % (", ".join("%d" % (i + 1) for i in range(16)),
                                                                                   ", ".join("-%d" % i for i in range(17))))
    assert rc == -3
