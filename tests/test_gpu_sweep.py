"""K estimates against one ground truth (erasor_hip_evaluate_many, kernels k_evm_* in evaluate.hip.h) and the parameter sweep built on it
(erasor_hip_sweep): row for row equal to erasor_hip_evaluate_clouds and to a plain single-handle loop of the existing API, against the CPU
oracle, independent of the scheduling, a failing configuration in its own row, the caller's handle untouched, and the offline driver's
--sweep / --eval-many modes.  tests/test_sweep_on_cpu.py re-runs part of this file against the CPU stand-in."""
import copy
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scenarios
from erasor_amd import evalmap

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = ("gt_static", "gt_dynamic", "est_static", "est_dynamic", "preserved_static", "preserved_dynamic", "n_tied", "n_label_out_of_range")
E_INVALID, E_STATE, E_UNSUPPORTED = -1, -4, -5
# the CPU stand-in (tests/test_sweep_on_cpu.py) steps ~100 times slower and cannot drive two handles from two host threads: there the
# sweeps run on tests/simt_full_step.py's small scene, one worker at a time, over two nodes and four of the six configurations (a step
# takes seconds there, whatever the map's size)
SIMT = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))
N_NODES = 2 if SIMT else 6  # nodes of the scene stepped by the sweep tests


def scene():
    """scenarios.small(); on the CPU stand-in the small shape tests/simt_full_step.py steps there"""
    return scenarios.small(n_frames=6, az=120, length=60.0) if SIMT else scenarios.small()


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


def cloud(xyz, lab):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return np.concatenate([xyz, np.broadcast_to(np.asarray(lab, np.float32).reshape(-1, 1), (len(xyz), 1))], 1).astype(np.float32)


def same_row(a, b, what):
    for k in COUNTS + ("PR", "RR", "F1"):
        assert a[k] == b[k], (what, k, a[k], b[k])


def fixtures():
    """one GT and seven estimates of very different sizes: a noisy subset, an empty one, one point, equidistant pairs of both classes,
    a dense copy with duplicates, labels out of range, a sparse subset"""
    rng = np.random.default_rng(20261016)
    n = 3000
    xyz = rng.uniform(-15, 15, (n, 3))
    lab = rng.choice([40.0, 48.0, 10.0, 252.0, 253.0, 259.0, 65536.0 + 44.0], n)
    gt = cloud(xyz, lab)
    # equidistant pairs: a GT point at c, estimated points at c +- 1/16 in x, of both classes (and of one class)
    c = np.array([[3.0 * k, -20.0, 0.5] for k in range(24)], np.float32)
    gt_t = cloud(c, [40.0 if k % 2 else 252.0 for k in range(24)])
    off = np.float32([0.0625, 0, 0])
    tie = np.concatenate([cloud(c + off, [40.0 if k % 4 < 2 else 48.0 for k in range(24)]),
                          cloud(c - off, [252.0 if k % 4 < 2 else 10.0 for k in range(24)])])
    gt = np.concatenate([gt, gt_t, cloud([[0, 0, -30], [1, 0, -30], [2, 0, -30]], [-1.0, 5e9, np.inf])])
    base = gt[rng.uniform(size=len(gt)) < 0.7].copy()
    base[:, :3] += rng.normal(0, 0.07, (len(base), 3)).astype(np.float32)
    dense = np.concatenate([gt, gt[:1500]])
    dense[:, :3] += rng.normal(0, 0.03, (len(dense), 3)).astype(np.float32)
    oor = gt[::3].copy()
    oor[::5, 3] = -7.0
    oor[1::5, 3] = 4.5e9
    ests = [base, np.zeros((0, 4), np.float32), gt[5:6].copy(), tie, dense, oor, gt[::11].copy()]
    return gt, ests


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("leaf", [0.0, 0.2])
def test_evaluate_many_rows_match_evaluate_clouds(gpu_mod, handle, k, leaf):
    gt, ests = fixtures()
    ests = ests[:k] if k < 7 else ests
    # host and device inputs mixed: the GT and every other estimate on the device
    ptrs = []

    def dev(a):
        if not len(a):
            return a
        ptrs.append(handle.device_array(np.ascontiguousarray(a, np.float32)))
        return ptrs[-1], len(a)

    args = [dev(e) if j % 2 else e for j, e in enumerate(ests)]
    g = dev(gt) if k != 3 else gt
    try:
        rows = handle.evaluate_many(g, args, 0.2, voxel_leaf=leaf)
        assert len(rows) == len(ests)
        for j, e in enumerate(ests):
            same_row(rows[j], handle.evaluate(gt, e, 0.2, voxel_leaf=leaf), "estimate %d" % j)
    finally:
        for p in ptrs:
            handle.device_free(p)
    if leaf == 0.0:
        assert rows[0]["n_label_out_of_range"] >= 2
        if k >= 4:
            assert rows[3]["n_tied"] > 0 and rows[1]["est_static"] + rows[1]["est_dynamic"] == 0
        for j, e in enumerate(ests):  # the host oracle where its answer is defined: no tie, no label out of range, a non-empty estimate
            if len(e) and rows[j]["n_tied"] == 0:
                ok = np.isfinite(gt[:, 3]) & (gt[:, 3] >= 0) & (gt[:, 3] < 2 ** 32)
                mine = handle.evaluate_many(gt[ok], [e], 0.2)[0]
                if mine["n_label_out_of_range"] == 0:
                    ref = evalmap.evaluate_clouds(gt[ok], e, 0.2)
                    for key in ("gt_static", "gt_dynamic", "est_static", "est_dynamic", "preserved_static", "preserved_dynamic", "PR", "RR", "F1"):
                        assert mine[key] == ref[key], (j, key, mine[key], ref[key])


def test_evaluate_many_errors_and_struct_sizes(gpu_mod, handle):
    gt, ests = fixtures()
    bad = ests[0].copy()
    bad[17, 1] = np.nan
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.evaluate_many(gt, [ests[0], ests[2], bad], 0.2)
    assert e.value.rc == E_INVALID and "estimate 2" in str(e.value)
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.evaluate_many(gt, [bad, ests[0]], 0.2, voxel_leaf=0.2)
    assert e.value.rc == E_INVALID and "estimate 0" in str(e.value)
    for vs in (0.0, -1.0, float("nan")):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.evaluate_many(gt, ests[:2], vs)
        assert e.value.rc == E_INVALID
    assert handle.evaluate_many(gt, [], 0.2) == []
    assert gpu_mod.lib().erasor_hip_evaluate_many(handle._h, None, C.c_size_t(0), 0, None, None, None, C.c_size_t(0), C.c_double(0.0),
                                                  C.c_double(0.2), None) == 0
    assert C.sizeof(gpu_mod.EvalResult) == 88 and C.sizeof(gpu_mod.Params) == 160
    assert C.sizeof(gpu_mod.SweepRow) == 160 + 8 + 16 + 88 + 8 + 32
    assert gpu_mod.SweepRow.status.offset == 160 and gpu_mod.SweepRow.eval.offset == 184 and gpu_mod.SweepRow.run_ms.offset == 272


# ---- the sweep ----
def sweep_configs(sc):
    """version 2 and 3, removal_interval 1 / 2 / 3, two scan_ratio_thresholds, max_h, map_voxel_size, large-scale with submap_size 25"""
    p0 = scenarios.to_product_params(sc["params"])
    out = []
    for kw in (dict(removal_interval=1), dict(version=2, removal_interval=2), dict(removal_interval=3, scan_ratio_threshold=0.1),
               dict(removal_interval=1, scan_ratio_threshold=0.3, max_h=2.5), dict(removal_interval=1, map_voxel_size=0.1),
               dict(removal_interval=2, is_large_scale=1, submap_size=25.0)):
        p = copy.copy(p0)
        for k, v in kw.items():
            setattr(p, k, v)
        out.append(p)
    return [out[i] for i in (0, 1, 2, 5)] if SIMT else out


def single_run(gpu_mod, sc, p, gt, n=N_NODES):
    """one configuration with the existing API only: set_map, the gated steps, voxelize_preserving_labels(get_map(), 0.2), evaluate"""
    g = gpu_mod.Erasor(p)
    g.set_map(sc["map"])
    steps = 0
    for j in range(n):
        if (j + 1) % p.removal_interval == 0:
            g.step(sc["scans"][j], sc["T_l2b"], sc["T_b2o"][j], sc["T_o2b"][j])
            steps += 1
    m = g.get_map()
    saved = g.voxelize_preserving_labels(m, 0.2)
    r = g.evaluate(gt, saved, 0.2)
    g.close()
    return dict(n_steps=steps, n_map_final=len(m), n_saved=len(saved), eval=r, saved=saved)


def run_sweep(h, sc, configs, n=N_NODES, **kw):
    if SIMT:
        kw["concurrency"] = 1
    return h.sweep(configs, sc["map"], sc["scans"][:n], sc["T_l2b"], sc["T_b2o"][:n], sc["T_o2b"][:n], sc["map"], **kw)


def same_sweep_row(a, b, what):
    assert a["status"] == 0, (what, a["status"])
    for k in ("n_steps", "n_map_final", "n_saved"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    same_row(a["eval"], b["eval"], what)


@pytest.fixture(scope="module")
def sweep_case(gpu_mod):
    sc = scene()
    configs = sweep_configs(sc)
    ref = [single_run(gpu_mod, sc, p, sc["map"]) for p in configs]
    return sc, configs, ref


def test_sweep_rows_equal_one_configuration_at_a_time(gpu_mod, handle, sweep_case):
    sc, configs, ref = sweep_case
    rows = run_sweep(handle, sc, configs)
    assert len(rows) == len(configs)
    for i, (r, s) in enumerate(zip(rows, ref)):
        same_sweep_row(r, s, "config %d" % i)
        assert r["params"]["removal_interval"] == configs[i].removal_interval and r["params"]["version"] == configs[i].version
        assert (r["run_ms"] > 0) == (r["n_steps"] > 0)
    assert [r["n_steps"] for r in rows] == [N_NODES // p.removal_interval for p in configs]
    if not SIMT:
        assert len({(r["eval"]["preserved_static"], r["eval"]["preserved_dynamic"]) for r in rows}) >= 3  # the parameters matter


def test_sweep_matches_the_cpu_oracle(gpu_mod, handle, sweep_case):
    from oracle import orc
    sc, configs, ref = sweep_case
    for i in (1, 5):
        po = orc.Params()
        C.memmove(C.byref(po), C.byref(configs[i]), C.sizeof(po))
        o = orc.Oracle(po)
        o.set_map(sc["map"])
        for j in range(N_NODES):
            if (j + 1) % po.removal_interval == 0:
                o.step(sc["scans"][j], sc["T_l2b"], sc["T_b2o"][j], sc["T_o2b"][j])
        saved = orc.voxelize_preserving_labels(o.get_map(), 0.2)
        r = evalmap.evaluate_clouds(sc["map"], saved, 0.2)
        assert ref[i]["n_saved"] == len(saved)
        for k in ("gt_static", "gt_dynamic", "est_static", "est_dynamic", "preserved_static", "preserved_dynamic", "PR", "RR", "F1"):
            assert ref[i]["eval"][k] == r[k], (i, k, ref[i]["eval"][k], r[k])
        assert ref[i]["eval"]["n_tied"] == 0


def test_sweep_scheduling_does_not_change_results(gpu_mod, handle, sweep_case):
    sc, configs, ref = sweep_case
    for conc, batch in () if SIMT else ((1, 1), (2, 2), (4, 0), (3, 4)):
        rows = run_sweep(handle, sc, configs, concurrency=conc, eval_batch=batch)
        for i, (r, s) in enumerate(zip(rows, ref)):
            same_sweep_row(r, s, "config %d, concurrency %d, eval_batch %d" % (i, conc, batch))
    # (on the stand-in: only this one, scored in pairs)
    perm = [2, 0, 3, 1] if SIMT else [4, 0, 5, 2, 1, 3]
    rows = run_sweep(handle, sc, [configs[i] for i in perm], concurrency=2, eval_batch=2 if SIMT else 0)
    for r, i in zip(rows, perm):
        same_sweep_row(r, ref[i], "permuted config %d" % i)


def test_a_failing_configuration_keeps_to_its_row(gpu_mod, handle, sweep_case):
    sc, configs, ref = sweep_case
    v4 = copy.copy(configs[0])
    v4.version = 4
    rows = run_sweep(handle, sc, configs[:3] + [v4] + configs[3:], concurrency=2)
    assert rows[3]["status"] == E_UNSUPPORTED and rows[3]["n_saved"] == 0
    for r, s, i in zip(rows[:3] + rows[4:], ref, range(6)):
        same_sweep_row(r, s, "config %d beside version 4" % i)


def test_sweep_argument_errors(gpu_mod, handle, sweep_case):
    sc, configs, _ = sweep_case
    for kw in (dict(concurrency=0), dict(concurrency=5), dict(voxelsize=0.0), dict(save_leaf=-0.1)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            run_sweep(handle, sc, configs[:1], **kw)
        assert e.value.rc == E_INVALID, kw
    with pytest.raises(gpu_mod.ErasorError) as e:
        run_sweep(handle, sc, configs[:1] * 257)
    assert e.value.rc == E_INVALID
    Tb = [t.copy() for t in sc["T_b2o"][:N_NODES]]
    Tb[2][0] = np.nan
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.sweep(configs[:1], sc["map"], sc["scans"][:N_NODES], sc["T_l2b"], Tb, sc["T_o2b"][:N_NODES], sc["map"])
    assert e.value.rc == E_INVALID
    gt = sc["map"].copy()
    gt[5, 2] = np.inf
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.sweep(configs[:1], sc["map"], sc["scans"][:N_NODES], sc["T_l2b"], sc["T_b2o"][:N_NODES], sc["T_o2b"][:N_NODES], gt)
    assert e.value.rc == E_INVALID and "ground truth" in str(e.value)
    assert run_sweep(handle, sc, []) == []
    # save_leaf 0: the final map evaluated as it is
    r = run_sweep(handle, sc, configs[:1], save_leaf=0.0)[0]
    assert r["n_saved"] == r["n_map_final"]


def test_sweep_leaves_the_caller_handle_untouched(gpu_mod, sweep_case):
    from test_gpu_parity import compare_step
    from oracle import orc
    sc, configs, ref = sweep_case
    g = gpu_mod.Erasor(scenarios.to_product_params(sc["params"]))
    o = orc.Oracle(sc["params"])
    g.set_map(sc["map"])
    o.set_map(sc["map"])
    n, ahead = 6, 2
    scans = [np.ascontiguousarray(s, np.float32) for s in sc["scans"][:n]]
    Tb, To = sc["T_b2o"], sc["T_o2b"]
    for j in range(ahead):
        g.prefetch(scans[j], sc["T_l2b"], Tb[j], To[j])
    free = []
    for k in range(n):
        if k + ahead < n:
            g.prefetch(scans[k + ahead], sc["T_l2b"], Tb[k + ahead], To[k + ahead])
        rg = g.step(scans[k], sc["T_l2b"], Tb[k], To[k])
        ro = o.step(scans[k], sc["T_l2b"], Tb[k], To[k])
        compare_step(g, o, rg, ro, full=False)
        if k in (1, 3):  # a sweep between two steps, with nodes announced ahead
            rows = run_sweep(g, sc, configs[:2], concurrency=2)
            for i in range(2):
                same_sweep_row(rows[i], ref[i], "sweep between steps, config %d" % i)
            free.append(_free_bytes())
    assert g.get_map().shape == o.get_map().shape
    if free[0] is not None:
        assert free[1] == free[0], free  # a second identical sweep: nothing left behind


def _free_bytes():
    try:
        import torch
        if not torch.cuda.is_available():
            return None
        return torch.cuda.mem_get_info(0)[0]
    except Exception:
        return None


# ---- the offline driver ----
def _eval_rows(text):
    """every analysis_runner row (the nine numbers) printed in text"""
    out = []
    for line in text.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) >= 9 and re.fullmatch(r"[0-9.]+", cells[-1] or "x") and re.fullmatch(r"\d+", cells[-9] or "x"):
            out.append(cells)
    return out


def test_driver_sweep_and_eval_many(gpu_mod, tmp_path):
    from test_gpu_shim import DEMO, _write_sequence_dir, ensure_demo, write_pcd_binary
    ensure_demo()
    sc = scenarios.small()
    d = str(tmp_path / "seq")
    os.makedirs(d)
    cfg = _write_sequence_dir(d, sc, 5, 0, "05")
    gt = os.path.join(d, "dense_global_map.pcd")
    grid = str(tmp_path / "grid.yaml")
    with open(grid, "w") as f:
        f.write("erasor:\n    scan_ratio_threshold: [0.1, 0.2, 0.3]\n    max_h: [2.5, 3.1]\nMapUpdater:\n    removal_interval: 1\n")
    out = subprocess.run([DEMO, "--sweep", cfg, grid, gt, "100", "0.2", "2"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = _eval_rows(out.stdout)
    assert len(rows) == 6, out.stdout
    f1 = [float(r[-1]) for r in rows]
    assert f1 == sorted(f1, reverse=True)
    assert "best configuration" in out.stdout and "scan_ratio_threshold:" in out.stdout
    for r in rows:
        srt, mh = r[0], r[1]
        y = str(tmp_path / ("cfg_%s_%s.yaml" % (srt, mh)))
        text = re.sub(r"(\n\s+scan_ratio_threshold:) [^\n]*", r"\1 %s" % srt, open(cfg).read())
        text = re.sub(r"(\n\s+max_h:) [^\n]*", r"\1 %s" % mh, text)
        open(y, "w").write(text)
        one = subprocess.run([DEMO, "--config", y, "100", gt], capture_output=True, text=True, timeout=900)
        assert one.returncode == 0, one.stdout + one.stderr
        tail = one.stdout.split("PR / RR of the saved static map")[1]
        assert _eval_rows(tail)[0] == r[2:], (r, _eval_rows(tail)[0])
    # --eval-many: one row per estimate, each --eval's
    _, ests = fixtures()
    paths = []
    for j, e in enumerate([ests[0], ests[3], ests[6]]):
        paths.append(str(tmp_path / ("est%d.pcd" % j)))
        write_pcd_binary(paths[-1], e)
    gtf = str(tmp_path / "gt.pcd")
    write_pcd_binary(gtf, fixtures()[0])
    many = subprocess.run([DEMO, "--eval-many", "0.2", "0", gtf] + paths, capture_output=True, text=True, timeout=300)
    assert many.returncode == 0, many.stdout + many.stderr
    mrows = _eval_rows(many.stdout)
    assert len(mrows) == 3
    for p, r in zip(paths, mrows):
        one = subprocess.run([DEMO, "--eval", gtf, p, "0.2", "0"], capture_output=True, text=True, timeout=300)
        assert one.returncode == 0
        assert _eval_rows(one.stdout)[0] == r
    bad = str(tmp_path / "bad.yaml")
    open(bad, "w").write("erasor:\n    max_h: [2.5, 3.1]\nMapUpdater:\n    data_name: [a, b]\n")
    out = subprocess.run([DEMO, "--sweep", cfg, bad, gt], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "/MapUpdater/data_name" in out.stderr

