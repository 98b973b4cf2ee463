"""Bird's-eye images on the device (erasor_hip_render_*, kernels in erasor_amd/csrc/render.hip.h) against the host oracle
(evalmap.render_fit / render / render_eval): every byte of the image and every statistic.  No pixel is ever left out of a comparison:
the winner of a pixel is the largest (priority, z), and the colour depends on (category, z) only.
tests/test_render_on_cpu.py re-runs this file, except the full-size case, against the CPU stand-in."""
import ctypes as C

import numpy as np
import pytest

import scenarios
from erasor_amd import evalmap, synth

pytestmark = pytest.mark.gpu

BG = 0x0A0A14


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    return gpu_mod.Erasor(gpu_mod.params_default())


@pytest.fixture(scope="module")
def world():
    s = scenarios.small()
    return s


def same(dev, orc, what=""):
    img_d, st_d = dev[0], dev[1]
    img_o, st_o = orc[0], orc[1]
    assert img_d.shape == img_o.shape and img_d.dtype == np.uint8, what
    assert (img_d == img_o).all(), (what, int((img_d != img_o).any(2).sum()), "pixels differ")
    assert st_d == st_o, (what, st_d, st_o)


def lattice(res, x0, nx, ny, seed):
    """points exactly on pixel edges: x = float32(x0 + k * res)"""
    rng = np.random.default_rng(seed)
    kx, ky = np.meshgrid(np.arange(nx), np.arange(ny))
    c = np.zeros((nx * ny, 4), np.float32)
    c[:, 0] = (x0 + kx.ravel() * res).astype(np.float32)
    c[:, 1] = (-x0 + ky.ravel() * res).astype(np.float32)
    c[:, 2] = rng.normal(size=len(c)).astype(np.float32)
    c[:, 3] = rng.choice([40.0, 252.0, 65536.0 * 3 + 253.0], len(c)).astype(np.float32)
    return c


def test_three_modes_on_a_synth_world_host_and_device_inputs(handle, world):
    m = world["map"]
    v = handle.render_fit(m, 0.2, 2, BG)
    assert v == evalmap.render_fit(m, 0.2, 2, BG)
    dyn = m[synth.is_dynamic(m[:, 3])]
    lab = int(dyn[0, 3]) if len(dyn) else 252
    for kw in (dict(mode="label"), dict(mode="height"), dict(mode="label", target_class=lab & 0xFFFF),
               dict(mode="label", target_class=lab & 0xFFFF, target_instance=lab >> 16)):
        same(handle.render(m, v, **kw), evalmap.render(m, v, **kw), str(kw))
    img, st = handle.render(m, v)
    assert st["n_outside"] == 0 and st["n_nonfinite"] == 0 and st["n_drawn"] == len(m) and st["cat_points"][1] == len(dyn) > 0
    # a view fitted on the fly, and a device input
    same(handle.render(m, res=0.5), evalmap.render(m, evalmap.render_fit(m, 0.5)), "view=None")
    p = handle.device_array(m)
    try:
        assert handle.render_fit((p, len(m)), 0.2, 2, BG) == v
        same(handle.render((p, len(m)), v), (img, st), "device input")
    finally:
        handle.device_free(p)
    # the error map
    est = m[~synth.is_dynamic(m[:, 3])][::2]
    est = np.concatenate([est, dyn[::3]])
    d = handle.render_eval(m, est, v)
    o = evalmap.render_eval(m, est, v)
    same(d, o, "eval")
    for k in ("gt_static", "gt_dynamic", "preserved_static", "preserved_dynamic"):
        assert d[2][k] == o[2][k], k
    assert len(np.unique(d[0].reshape(-1, 3), axis=0)) > 20  # (a picture, not a constant)


def test_order_independence(handle, world):
    m = world["map"]
    v = evalmap.render_fit(m, 0.1, 2, BG)
    first = handle.render(m, v)
    rng = np.random.default_rng(20261016)
    for other in (m[::-1], m[rng.permutation(len(m))]):
        again = handle.render(other, v)
        assert (again[0] == first[0]).all() and again[1] == first[1]
    same(first, evalmap.render(m, v))


@pytest.mark.parametrize("res", [0.2, 0.1])
def test_points_on_pixel_edges(handle, res):
    c = lattice(res, -37.0, 150, 90, 5)
    v = evalmap.render_fit(c, res, 1, BG)
    assert handle.render_fit(c, res, 1, BG) == v
    d = handle.render(c, v)
    same(d, evalmap.render(c, v), "lattice")
    assert d[1]["n_outside"] == 0
    # a view whose edges the points lie on: x0 on a point, x0 + width * res on another
    v2 = evalmap.render_view(float(np.float32(-37.0 + 10 * res)), float(np.float32(37.0 + 10 * res)), res, 100, 60, -1.0, 1.0, BG)
    d2 = handle.render(c, v2)
    same(d2, evalmap.render(c, v2), "edges")
    assert d2[1]["n_outside"] > 0


def test_extremes_of_the_tile_sort(handle):
    rng = np.random.default_rng(9)
    n = 20000
    # all points in one pixel
    c = np.zeros((n, 4), np.float32)
    c[:, :2] = rng.uniform(5.0, 5.1, (n, 2))
    c[:, 2] = rng.normal(size=n)
    c[:, 3] = rng.choice([40.0, 252.0], n)
    v = evalmap.render_view(0.0, 0.0, 0.2, 70, 70, -1.0, 1.0, BG)
    d = handle.render(c, v)
    same(d, evalmap.render(c, v), "one pixel")
    assert d[1]["n_pixels_hit"] == 1 and d[1]["n_drawn"] == n
    # ties: every point the same (priority, z) -- equal winners, equal colours
    c[:, 2], c[:, 3] = 0.25, 40.0
    same(handle.render(c, v), evalmap.render(c, v), "ties")
    # all points in one tile (64 x 64 pixels), a view of several tiles
    c = np.zeros((n, 4), np.float32)
    c[:, :2] = rng.uniform(12.8, 25.6, (n, 2))
    c[:, 2] = rng.normal(size=n)
    v = evalmap.render_view(0.0, 0.0, 0.2, 200, 200, -1.0, 1.0, BG)
    same(handle.render(c, v, mode="height"), evalmap.render(c, v, mode="height"), "one tile")
    # one point per tile
    kx, ky = np.meshgrid(np.arange(40), np.arange(30))
    c = np.zeros((1200, 4), np.float32)
    c[:, 0] = kx.ravel() * 12.8 + rng.uniform(0, 12.7, 1200)
    c[:, 1] = ky.ravel() * 12.8 + rng.uniform(0, 12.7, 1200)
    c[:, 2] = rng.normal(size=1200)
    v = evalmap.render_view(0.0, 0.0, 0.2, 40 * 64, 30 * 64, -1.0, 1.0, BG)
    d = handle.render(c, v, mode="height")
    same(d, evalmap.render(c, v, mode="height"), "one point per tile")
    assert d[1]["n_pixels_hit"] == 1200


@pytest.mark.parametrize("w,h", [(1, 1), (1, 130), (130, 1), (65, 63), (127, 129), (16384, 3), (3, 16384)])
def test_image_sizes(handle, w, h):
    rng = np.random.default_rng(w * 7 + h)
    n = 5000
    res = 0.25
    c = np.zeros((n, 4), np.float32)
    c[:, 0] = rng.uniform(-1.0, w * res + 1.0, n)
    c[:, 1] = rng.uniform(-1.0, h * res + 1.0, n)
    c[:, 2] = rng.normal(size=n)
    c[:, 3] = rng.choice([0.0, 259.0], n)
    c[::97, rng.integers(0, 3)] = np.nan
    c[5::131, 1] = np.inf
    v = evalmap.render_view(0.0, 0.0, res, w, h, -2.0, 2.0, BG)
    d = handle.render(c, v)
    same(d, evalmap.render(c, v), (w, h))
    assert d[1]["n_nonfinite"] > 0 and d[1]["n_points"] == d[1]["n_drawn"] + d[1]["n_outside"] + d[1]["n_nonfinite"]


def test_empty_cloud_errors_and_limits(gpu_mod, handle):
    v = evalmap.render_view(0.0, 0.0, 0.5, 9, 5, 0.0, 1.0, 0x123456)
    img, st = handle.render(np.zeros((0, 4), np.float32), v)
    assert (img == [0x12, 0x34, 0x56]).all() and img.shape == (5, 9, 3)
    assert st == {"n_points": 0, "n_drawn": 0, "n_outside": 0, "n_nonfinite": 0, "n_pixels_hit": 0, "cat_points": [0] * 8, "cat_pixels": [0] * 8}
    c = np.array([[1, 1, 1, 0], [2, 2, 2, 0]], np.float32)
    for bad in (dict(res=0.0), dict(res=-1.0), dict(res=float("nan")), dict(res=float("inf")), dict(width=0), dict(height=0), dict(width=16385),
                dict(height=16385), dict(width=8193, height=8192), dict(x0=float("nan")), dict(z_hi=float("inf"))):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.render(c, dict(v, **bad))
        assert e.value.rc == -1, bad
    handle.render(c, dict(v, width=8192, height=8192))  # (2^26 pixels: the limit itself)
    for cloud, kw in ((np.zeros((0, 4), np.float32), {}), (np.full((3, 4), np.nan, np.float32), {}), (c, dict(res=0.0)), (c, dict(margin=0))):
        with pytest.raises(gpu_mod.ErasorError) as e:
            handle.render_fit(cloud, **kw)
        assert e.value.rc == -1
    wide = np.array([[0, 0, 0, 0], [5000, 100, 0, 0]], np.float32)
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.render_fit(wide, 0.2)
    assert e.value.rc == -1 and "smallest res that fits" in str(e.value)
    hint = float(str(e.value).rsplit("about", 1)[1])
    assert 5000 / 16384 < hint < 5000 / 16384 * 1.02
    assert handle.render_fit(wide, hint)["width"] <= 16384
    with pytest.raises(ValueError):
        handle.render(c, v, mode="eval")
    r = C.c_int(gpu_mod.lib().erasor_hip_render_clouds(handle._h, c.ctypes.data_as(C.c_void_p), C.c_size_t(2), C.c_int(0), C.c_int(2), C.c_int32(-1),
                                                       C.c_int32(-1), C.byref(gpu_mod.RenderView.of(v)), None, C.c_int(0), None))
    assert r.value == -1
    fresh = gpu_mod.Erasor(gpu_mod.params_default())
    for fn in (lambda: fresh.render_map(v), lambda: fresh.render_fit(None), lambda: fresh.render_eval_map(c, v)):
        with pytest.raises(gpu_mod.ErasorError) as e:
            fn()
        assert e.value.rc == -4
    assert C.sizeof(gpu_mod.RenderView) == 56 and C.sizeof(gpu_mod.RenderStats) == 5 * 8 + 2 * 64


def test_render_eval_counts_and_voxel_leaf(gpu_mod, handle, world):
    m = world["map"]
    dynm = synth.is_dynamic(m[:, 3])
    rng = np.random.default_rng(4)
    est = np.concatenate([m[~dynm][rng.uniform(size=int((~dynm).sum())) < 0.8], m[dynm][::2]])
    v = handle.render_fit(m, 0.2, 2, BG)
    img, st, ev = handle.render_eval(m, est, v)
    assert st["n_outside"] == 0 and st["n_drawn"] == len(m)
    assert st["cat_points"][4:] == [ev["preserved_static"], ev["gt_dynamic"] - ev["preserved_dynamic"], ev["gt_static"] - ev["preserved_static"],
                                    ev["preserved_dynamic"]]
    assert min(st["cat_points"][4:]) > 0
    plain = handle.evaluate(m, est, 0.2, per_point=True)
    assert {k: ev[k] for k in plain if k != "per_point"} == {k: plain[k] for k in plain if k != "per_point"}
    code = plain["per_point"]
    assert st["cat_points"][4] == int((code == 1).sum()) and st["cat_points"][7] == int((code == 2).sum())
    assert st["cat_points"][5] == int((dynm & (code != 2)).sum()) and st["cat_points"][6] == int((~dynm & (code != 1)).sum())
    # the image from those codes, by the oracle's rasteriser
    prio = np.where(code == 1, 1, np.where(code == 2, 4, np.where(dynm, 2, 3))).astype(np.int64)
    same((img, st), evalmap._raster(np.ascontiguousarray(m), prio, evalmap.RENDER_EVAL, v), "eval from the device's own codes")
    # voxel_leaf: the voxelised ground truth is drawn
    img2, st2, ev2 = handle.render_eval(m, est, v, voxel_leaf=0.2)
    gv, evx = handle.voxelize_preserving_labels(m, 0.2), handle.voxelize_preserving_labels(est, 0.2)
    assert ev2 == handle.evaluate(m, est, 0.2, voxel_leaf=0.2) and st2["n_points"] == len(gv) == ev2["gt_static"] + ev2["gt_dynamic"]
    same((img2, st2), handle.render_eval(gv, evx, v)[:2], "voxel_leaf")
    assert st2["n_outside"] == 0
    assert st2["cat_points"][4:] == [ev2["preserved_static"], ev2["gt_dynamic"] - ev2["preserved_dynamic"],
                                     ev2["gt_static"] - ev2["preserved_static"], ev2["preserved_dynamic"]]


@pytest.mark.parametrize("large_scale", [0, 1])
def test_resident_map_after_steps(gpu_mod, world, large_scale):
    p = scenarios.to_product_params(world["params"])
    p.is_large_scale = large_scale
    p.submap_size = 60.0
    g = gpu_mod.Erasor(p)
    g.set_map(world["map"])
    for k in range(3):
        g.prefetch(world["scans"][k + 1], world["T_l2b"]) if k < 2 else None
        g.step(world["scans"][k], world["T_l2b"], world["T_b2o"][k], world["T_o2b"][k])
        if k == 1:  # a render between two steps, with a scan announced: the announcement and the step's clouds stay
            before = [g.get_cloud(w) for w in (gpu_mod.CLOUD_MAP_REJECTED, gpu_mod.CLOUD_STATIC_ESTIMATE, gpu_mod.CLOUD_QUERY_VOI)]
            g.render_map(res=0.2)
            g.render_eval_map(world["map"], res=0.2)
            after = [g.get_cloud(w) for w in (gpu_mod.CLOUD_MAP_REJECTED, gpu_mod.CLOUD_STATIC_ESTIMATE, gpu_mod.CLOUD_QUERY_VOI)]
            assert all(a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all() for a, b in zip(before, after))
    # (the step after the render consumed its announcement: same result as an undisturbed run)
    ref = gpu_mod.Erasor(p)
    ref.set_map(world["map"])
    for k in range(3):
        ref.step(world["scans"][k], world["T_l2b"], world["T_b2o"][k], world["T_o2b"][k])
    m = g.get_map()
    assert (m.view(np.uint32) == ref.get_map().view(np.uint32)).all()
    v = g.render_fit(None, 0.2, 2, BG)
    assert v == evalmap.render_fit(m, 0.2, 2, BG)
    d = g.render_map(v)
    same(d, evalmap.render(m, v), "render_map")
    assert d[1]["n_points"] == len(m) == g.map_size() and d[1]["n_outside"] == 0
    same(g.render_map(v, mode="height"), evalmap.render(m, v, mode="height"), "render_map height")
    gt = world["map"]
    vg = g.render_fit(gt, 0.2, 2, BG)
    a, b = g.render_eval_map(gt, vg), g.render_eval(gt, m, vg)
    assert (a[0] == b[0]).all() and a[1] == b[1] and a[2] == b[2] == g.evaluate_map(gt, 0.2)
    same(a, evalmap.render_eval(gt, m, vg), "render_eval_map")


def test_fit_of_a_cloud_with_non_finite_points(gpu_mod, handle):
    """the order statistics are taken over the finite points only: ranks over their count, the others above every rank"""
    rng = np.random.default_rng(21)
    n = 5001
    c = np.zeros((n, 4), np.float32)
    c[:, :2] = rng.uniform(-30, 30, (n, 2))
    c[:, 2] = rng.normal(0, 3, n)
    c[rng.permutation(n)[:1500], 2] = np.nan          # 30 % of the heights
    c[rng.permutation(n)[:300], 0] = np.inf
    c[rng.permutation(n)[:300], 1] = -np.inf
    c[7, :3] = [1e30, 2.0, 1e30]                       # a finite outlier would widen the view beyond the limits: keep it non-finite
    c[7, 0] = np.nan
    want = evalmap.render_fit(c, 0.1, 2, BG)
    assert handle.render_fit(c, 0.1, 2, BG) == want
    fin = c[np.isfinite(c[:, :3]).all(1)]
    assert 3000 < len(fin) < n and want == evalmap.render_fit(fin, 0.1, 2, BG)
    assert handle.render_fit(fin, 0.1, 2, BG) == want
    same(handle.render(c, want), evalmap.render(c, want), "non-finite")
    with pytest.raises(gpu_mod.ErasorError) as e:
        handle.render_fit(c, 0.1, 1025)
    assert e.value.rc == -1
    assert handle.render_fit(c, 0.1, 1024) == evalmap.render_fit(c, 0.1, 1024)


def test_every_entry_refuses_a_handle_with_a_step_in_flight(gpu_mod, world):
    g = gpu_mod.Erasor(scenarios.to_product_params(world["params"]))
    g.set_map(world["map"])
    c = world["map"][:1000]
    v = evalmap.render_fit(c, 0.2)
    g.step_async(world["scans"][0], T_l2b=world["T_l2b"], T_b2o=world["T_b2o"][0], T_o2b=world["T_o2b"][0])
    try:
        for fn in (lambda: g.render_fit(c), lambda: g.render_fit(None), lambda: g.render(c, v), lambda: g.render_map(v),
                   lambda: g.render_eval(c, c, v), lambda: g.render_eval_map(c, v)):
            with pytest.raises(gpu_mod.ErasorError) as e:
                fn()
            assert e.value.rc == -4 and "in flight" in str(e.value)
    finally:
        g.step_wait()
    same(g.render_map(v), evalmap.render(g.get_map(), v), "after the wait")


@pytest.mark.timeout(1200)
def test_full_size_bench_map(gpu_mod):
    """the 9.8 M-point map of bench config 2 at res 0.2, every byte against the oracle"""
    w = synth.World(seed=20210305 + 5, length=1000.0, n_streets=5, street_gap=50.0, n_moving=10, n_peds=6)
    m = w.sample_map(spacing=0.2, frames=range(0, 320, 2))
    assert len(m) > 9_000_000
    p = gpu_mod.params_default()
    synth.apply_params(p, "05", max_range=80.0, num_rings=20, num_sectors=108)
    g = gpu_mod.Erasor(p)
    g.set_map(m)
    v = g.render_fit(None, 0.2, 2, BG)
    assert v == evalmap.render_fit(m, 0.2, 2, BG)
    d = g.render_map(v)
    same(d, evalmap.render(m, v), "full size")
    assert d[1]["n_outside"] == 0 and d[1]["n_drawn"] == len(m)
    print("full size: %d points into %d x %d pixels, %d hit" % (len(m), v["width"], v["height"], d[1]["n_pixels_hit"]))
