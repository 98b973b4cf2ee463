"""erasor::OfflineMapUpdater's look-ahead under the removal_interval gate, on the GPU: the scripted callers of
tests/cpp/shim_lookahead_check.cpp (tests/test_shim_lookahead_on_cpu.py explores them exhaustively against a stand-in) linked to the real
liberasor_hip.so.  Per (policy, removal_interval) one process runs lookahead 1, 2, 3, 4, 7; N = 3 * interval + lookahead + 3 nodes, node k
brings scan and pose k % 12 of scenarios.small().  Every script:
  (a) throws nothing;
  (b) per processed callback the two rejected clouds and the counts of the result block, and the final map, equal the oracle's bit for
      bit -- the oracle steps exactly the ungated nodes;
  (c), (d) keeps its look-ahead (window / greedy / greedy_deferred: every ticket is stepped, nothing is dropped, every ungated node
      behind the first processed one is stepped by ticket);
  (e) leaves, line for line, the call log the same script leaves against tests/cpp/fake_erasor_hip.cpp (built here): outstanding() and
      the library's own count after every call included.  That pins the stand-in to the real library.
Then erasor_offline_demo --config at removal_interval 8 (the reference's config/seq_05.yaml) with ERASOR_DEMO_LOOKAHEAD 1, 3 and 7."""
import functools
import os
import subprocess

import numpy as np
import pytest

import scenarios
import shim_lookahead as sl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# as tests/test_gpu_shim.py: a directory with the tests' CPU stand-in build of liberasor_hip.so (tests/test_full_step_on_cpu.py)
ON_STAND_IN = bool(os.environ.get("ERASOR_TEST_SHIM_DIR"))
LIBDIR = os.environ.get("ERASOR_TEST_SHIM_DIR") or os.path.join(ROOT, "erasor_amd")
DEMO = os.path.join(LIBDIR, "erasor_offline_demo")
LOOKAHEADS = (1, 2, 3) if ON_STAND_IN else (1, 2, 3, 4, 7)  # (the stand-in takes seconds per step: a reduced key runs there)
INTERVALS = (1, 2, 3, 4, 8)
N_SCANS = 12
RANDOM_SEEDS = 4  # per interval: seeds 1000 * interval .. + 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def oracle_steps(interval):
    """the oracle over the ungated nodes of the longest script of this interval: per step the two rejected clouds, the result block's counts
    and the map behind it (the expectation depends on the interval and on how many nodes a script has, not on policy or lookahead)"""
    from oracle import orc
    sc = scenarios.small()
    o = orc.Oracle(sc["params"])
    o.set_map(sc["map"])
    steps = []
    for node in range(sl.n_nodes(interval, max(LOOKAHEADS))):
        if (node + 1) % interval != 0:
            continue  # "PASS!" (OMU.cpp:206-209)
        k = node % N_SCANS
        r = o.step(sc["scans"][k], sc["T_l2b"], sc["T_b2o"][k], sc["T_o2b"][k]).as_dict()
        steps.append(dict(node=node, map_rejected=bits(o.get_cloud(4)), query_rejected=bits(o.get_cloud(5)), counts=r, map=bits(o.get_map())))
    return bits(sc["map"]), steps


U64 = ("n_map_in", "n_voi", "n_outskirts", "n_query", "n_static_estimate", "n_complement", "n_map_rejected", "n_curr_rejected", "n_ground",
       "n_map_out", "n_static", "n_dynamic")


def oracle_failures(s):
    map0, steps = oracle_steps(s.interval)
    bad = []
    for j, c in enumerate(s.callbacks):
        want = steps[j]
        if c["node"] != want["node"]:
            bad.append("(b) processed callback %d is node %d, the oracle's is node %d" % (j, c["node"], want["node"]))
            break
        for nm in ("map_rejected", "query_rejected"):
            if c[nm].shape != want[nm].shape or not np.array_equal(c[nm], want[nm]):
                bad.append("(b) node %d: %s differs from the oracle's" % (c["node"], nm))
        got = dict(zip(U64, (int(v) for v in c["last"])))
        if got != {k: want["counts"][k] for k in U64}:
            bad.append("(b) node %d: result block %s, the oracle's %s" % (c["node"], got, want["counts"]))
    if not s.threw:
        want_map = steps[len(s.callbacks) - 1]["map"] if s.callbacks else map0
        if s.final_map is None or s.final_map.shape != want_map.shape or not np.array_equal(s.final_map, want_map):
            bad.append("(b) the final map differs from the oracle's")
    return bad


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """the data, the driver linked to the real library, and the driver linked to the stand-in"""
    from oracle import orc
    orc.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "erasor_amd", "csrc", "shim"), "-s"] + (["LIBDIR=" + LIBDIR] if ON_STAND_IN else []))
    sc = scenarios.small()
    data = str(tmp_path_factory.mktemp("lookahead_data"))
    sl.write_data(data, sc["map"], sc["scans"][:N_SCANS], sc["poses"][:N_SCANS])
    bin_dir = str(tmp_path_factory.mktemp("lookahead_bin"))
    real = sl.build_driver(os.path.join(bin_dir, "shim_lookahead_check"), libdir=LIBDIR)
    fake_dir = str(tmp_path_factory.mktemp("lookahead_fake"))
    sl.build_fake_lib(fake_dir)
    fake = sl.build_driver(os.path.join(fake_dir, "shim_lookahead_check"), libdir=fake_dir)
    return data, real, fake


@pytest.mark.parametrize("interval", INTERVALS, ids=lambda i: "interval%d" % i)
@pytest.mark.parametrize("policy", sl.FIXED_POLICIES + ("random",))
def test_scripted_callers_match_the_oracle_and_the_stand_in(setup, tmp_path, policy, interval):
    data, real, fake = setup
    seed0, n_seeds = (1000 * interval, RANDOM_SEEDS) if policy == "random" else (0, 1)
    timeout = 3000 if ON_STAND_IN else 120
    got, _ = sl.run_driver(real, data, str(tmp_path / "real_"), N_SCANS, interval, LOOKAHEADS, policy, seed0, n_seeds, timeout=timeout)
    ref, _ = sl.run_driver(fake, data, str(tmp_path / "fake_"), N_SCANS, interval, LOOKAHEADS, policy, seed0, n_seeds, timeout=120)
    bad = []
    for s, f in zip(got, ref):
        assert s.n_nodes == sl.n_nodes(interval, s.lookahead) and (s.lookahead, s.seed) == (f.lookahead, f.seed)
        why = sl.failures(s) + oracle_failures(s)
        if s.log != f.log:
            k = next((i for i, (a, b) in enumerate(zip(s.log, f.log)) if a != b), min(len(s.log), len(f.log)))
            why.append("(e) call log, line %d: `%s` here, `%s` against the stand-in" % (k, s.log[k] if k < len(s.log) else "", f.log[k] if k < len(f.log) else ""))
        if why:
            bad.append(sl.tag(s) + ": " + " | ".join(why[:4]))
    assert not bad, "\n".join(bad)


def _write_sequence_dir(d, sc, n, interval):
    """<d>/dense_global_map.pcd, pcds/, poses_lidar2body.csv, cfg.yaml in the reference's layout (node k: scan and pose k % 12)"""
    from erasor_amd import synth
    os.makedirs(os.path.join(d, "pcds"))
    os.makedirs(os.path.join(d, "out"))
    sl.write_pcd_binary(os.path.join(d, "dense_global_map.pcd"), sc["map"])
    with open(os.path.join(d, "poses_lidar2body.csv"), "w") as f:
        f.write("index, timestamp, x, y, z, qx, qy, qz, qw\n")
        for k in range(n):
            sl.write_pcd_binary(os.path.join(d, "pcds", "%06d.pcd" % k), sc["scans"][k % N_SCANS])
            f.write("%d, %.2f, %s\n" % (k, 0.1 * k, ", ".join("%.9f" % v for v in sc["poses"][k % N_SCANS])))
    sp = synth.SEQ_PARAMS["05"]
    with open(os.path.join(d, "cfg.yaml"), "w") as f:
        f.write("erasor:\n")
        for key in ("max_range", "num_rings", "num_sectors", "min_h", "max_h", "th_bin_max_h", "scan_ratio_threshold", "minimum_num_pts",
                    "gf_dist_thr", "gf_iter", "gf_num_lpr", "gf_th_seeds_height"):
            f.write("    %s: %s\n" % (key, sp[key]))
        f.write("    rejection_ratio: 0\n    version: 3\n\nMapUpdater:\n    data_name: \"05\"\n    env: \"outdoor\"\n")
        f.write("    save_path: \"%s\"\n    query_voxel_size: 0.2\n    map_voxel_size: 0.05\n    removal_interval: %d\n\n" % (os.path.join(d, "out"), interval))
        f.write("data_dir: \"%s\"\ninit_idx: 0\ninterval: 2\nvoxel_size: 0.075\n" % d)
        f.write("tf:\n     lidar2body: [0.0, 0.0, %s, 0, 0.0, 0.0, 1.0]\n\nverbose: false\n" % synth.LIDAR_HEIGHT)
    return os.path.join(d, "cfg.yaml")


def test_the_offline_driver_at_the_references_interval_8(setup, tmp_path):
    """erasor_offline_demo --config over 27 nodes at removal_interval 8 with 1, 3 and 7 nodes announced ahead: the three saved maps are
    byte-identical, and they are the oracle's map after its three steps (nodes 7, 15, 23), voxelised and written as save_static_map
    writes it (ASCII, %.8g: compared as text)."""
    import ctypes as C
    from oracle import orc
    sc = scenarios.small()
    n, interval = 27, 8
    saved = []
    for la in (1, 3, 7):
        d = str(tmp_path / ("la%d" % la))
        os.makedirs(d)
        cfg = _write_sequence_dir(d, sc, n, interval)
        out = subprocess.run([DEMO, "--config", cfg], capture_output=True, text=True, timeout=300, env=dict(os.environ, ERASOR_DEMO_LOOKAHEAD=str(la)))
        assert out.returncode == 0, out.stdout + out.stderr
        saved.append(open(os.path.join(d, "out", "05_result.pcd"), "rb").read())
    assert saved[0] == saved[1] == saved[2]
    # the oracle, fed with the transforms the driver derives from the csv
    shim = C.CDLL(os.path.join(LIBDIR, "liberasor_shim.so"))
    shim.erasor_shim_load_poses.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    shim.erasor_shim_load_poses.restype = C.c_long
    T, geo, R = np.zeros((n, 16), np.float32), np.zeros((n, 7), np.float64), np.zeros((n, 16), np.float32)
    assert shim.erasor_shim_load_poses(os.path.join(str(tmp_path / "la1"), "poses_lidar2body.csv").encode(), T.ctypes.data, geo.ctypes.data, R.ctypes.data, n) == n
    o = orc.Oracle(sc["params"])
    o.set_map(sc["map"])
    for k in (7, 15, 23):
        Tb = np.ascontiguousarray(R[k].reshape(4, 4))
        o.step(sc["scans"][k % N_SCANS], sc["T_l2b"], Tb, orc.invert4(Tb))
    ref = orc.voxelize_preserving_labels(o.get_map(), 0.2)
    body = saved[0].decode().split("DATA ascii\n")[1].splitlines()
    assert body == ["%.8g %.8g %.8g %.8g" % tuple(float(v) for v in row) for row in ref]
