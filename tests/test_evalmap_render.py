"""The host oracle of the bird's-eye renderer (erasor_amd/evalmap.py: render_fit / render / render_eval; write_ppm / read_ppm /
hstack_panels in erasor_amd), pinned with hand-computed answers.  No GPU."""
import numpy as np
import pytest

import erasor_amd
from erasor_amd import evalmap

BG = 0x102030
S, D, T = 40.0, 252.0, 253.0  # a static class, a dynamic class, the target's (dynamic) class
PAL = evalmap.RENDER_PALETTE


def rgb(c):
    return [(c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF]


def test_each_rule_decides_one_pixel_of_a_4_by_3_image():
    # x0 = 10, y0 = -1, res = 0.5: columns cover x in [10, 12), rows y in [-1, 0.5); z_hi <= z_lo: every colour is its base colour
    v = evalmap.render_view(10.0, -1.0, 0.5, 4, 3, 0.0, 0.0, BG)
    pts = np.array([
        # pixel (col 0, cy 0): priority beats height -- the dynamic point is lower and still wins
        [10.1, -0.9, 5.0, S], [10.2, -0.8, -5.0, D],
        # pixel (col 1, cy 0): height decides within a category (both static, z 1 < z 2)
        [10.6, -0.9, 1.0, S], [10.7, -0.9, 2.0, S],
        # pixel (col 2, cy 1): two static points at -0.0 and +0.0.  Which of them wins cannot be seen in a colour (both shade alike
        # whatever z_lo / z_hi are): the rule -0.0 < +0.0 is pinned on the key, in test_negative_zero_loses_to_positive_zero
        [11.2, -0.4, -0.0, S], [11.3, -0.4, 0.0, S],
        # exactly on x0: inside (col 0, cy 2); exactly on x0 + width * res = 12: outside
        [10.0, 0.2, 0.0, T], [12.0, 0.2, 0.0, S],
        # a NaN z is dropped
        [11.7, 0.2, np.nan, S],
    ], np.float32)
    img, st = evalmap.render(pts, v, "label", target_class=253)
    want = np.empty((3, 4, 3), np.uint8)
    want[:] = rgb(BG)
    want[2, 0] = rgb(PAL[1])  # image row = height - 1 - cy
    want[2, 1] = rgb(PAL[0])
    want[1, 2] = rgb(PAL[0])
    want[0, 0] = rgb(PAL[2])
    assert (img == want).all(), (img, want)
    assert st == {"n_points": 9, "n_drawn": 7, "n_outside": 1, "n_nonfinite": 1, "n_pixels_hit": 4,
                  "cat_points": [5, 1, 1, 0, 0, 0, 0, 0], "cat_pixels": [2, 1, 1, 0, 0, 0, 0, 0]}
    # the same points in any order give the same image
    rng = np.random.default_rng(3)
    for _ in range(5):
        img2, st2 = evalmap.render(pts[rng.permutation(len(pts))], v, "label", target_class=253)
        assert (img2 == img).all() and st2 == st
    # without a target the point on x0 is plain dynamic; with another instance asked for, too
    assert (evalmap.render(pts, v, "label")[0][0, 0] == rgb(PAL[1])).all()
    assert (evalmap.render(pts, v, "label", 253, 7)[0][0, 0] == rgb(PAL[1])).all()
    assert (evalmap.render(pts, v, "label", 253, 0)[0][0, 0] == rgb(PAL[2])).all()
    # mode "height": one category, whatever the label
    img_h, st_h = evalmap.render(pts, v, "height")
    assert st_h["cat_points"] == [0, 0, 0, 7, 0, 0, 0, 0] and st_h["cat_pixels"] == [0, 0, 0, 4, 0, 0, 0, 0]
    assert (img_h[2, 0] == rgb(PAL[3])).all()


def test_negative_zero_loses_to_positive_zero():
    # the order the rasteriser compares heights in (the winner of a pixel is the largest key): float32's total order
    k = evalmap.z_order(np.array([-0.0, 0.0, -1.0, 1.0, -np.inf, np.inf], np.float32)).astype(np.int64)
    assert k[0] < k[1] and k[2] < k[0] and k[1] < k[3] and k[4] < k[2] and k[3] < k[5]
    back = evalmap.z_from_order(k.astype(np.uint32))
    assert (back.view(np.uint32) == np.array([-0.0, 0.0, -1.0, 1.0, -np.inf, np.inf], np.float32).view(np.uint32)).all()


def test_shade_formula():
    # channel = floor(base * (0.35 + 0.65 * s) + 0.5)
    z = np.array([0.0, 10.0, -3.0, 12.0, 5.0], np.float32)
    got = evalmap.shade(200, z, 0.0, 10.0)
    # s = 0, 1, clamp -> 0, clamp -> 1, 0.5: 200 * 0.35 = 70, 200, 70, 200, 200 * 0.675 = 135
    assert got.tolist() == [70, 200, 70, 200, 135]
    assert evalmap.shade(255, z, 0.0, 10.0).tolist() == [89, 255, 89, 255, 172]  # 89.25 + .5 -> 89; 172.125 + .5 -> 172
    assert evalmap.shade(200, z, 3.0, 3.0).tolist() == [200] * 5  # z_hi <= z_lo: s = 1
    assert evalmap.shade(200, z, 4.0, 3.0).tolist() == [200] * 5


def test_fit_order_statistics_and_extent():
    # 101 points: z = 0 .. 98 plus one outlier at each end; ranks floor(0.02 * 100) = 2 and floor(0.98 * 100) = 98 of the ascending z
    z = np.concatenate([[-1000.0], np.arange(99, dtype=np.float64), [1000.0]])
    rng = np.random.default_rng(5)
    x = rng.uniform(3.0, 7.0, 101)
    y = rng.uniform(-2.0, 2.0, 101)
    x[0], x[1], y[0], y[1] = 3.0, 7.0, -2.0, 2.0
    c = np.stack([x, y, z, np.zeros(101)], 1).astype(np.float32)
    c = c[rng.permutation(101)]
    c = np.concatenate([c, [[np.nan, 0, 0, 0], [0, np.inf, 0, 0], [0, 0, np.nan, 0]]]).astype(np.float32)  # (not finite: ignored)
    v = evalmap.render_fit(c, res=0.5, margin=2, background=BG)
    assert v["z_lo"] == 1.0 and v["z_hi"] == 97.0  # ascending: -1000, 0, 1, ..., 97, 98, 1000
    assert v["x0"] == 3.0 - 1.0 and v["y0"] == -2.0 - 1.0 and v["res"] == 0.5 and v["background"] == BG
    assert v["width"] == int((7.0 - 2.0) / 0.5) + 1 + 2 and v["height"] == int((2.0 + 3.0) / 0.5) + 1 + 2
    _, st = evalmap.render(c, v, "height")
    assert st["n_outside"] == 0 and st["n_nonfinite"] == 3 and st["n_drawn"] == 101
    with pytest.raises(ValueError):
        evalmap.render_fit(c[-3:], 0.5)
    with pytest.raises(ValueError):
        evalmap.render_fit(c, 1e-4)  # 40000 pixels wide
    with pytest.raises(ValueError):
        evalmap.render_fit(np.zeros((0, 4), np.float32), 0.5)
    with pytest.raises(ValueError):
        evalmap.render_fit(c, 0.5, margin=1025)


def test_fit_contains_points_on_pixel_edges():
    rng = np.random.default_rng(11)
    for res in (0.05, 0.1, 0.2, 0.25, 1.0):
        for margin in (1, 2):
            k = rng.integers(-300, 300, (500, 2))
            c = np.zeros((500, 4), np.float32)
            c[:, :2] = (k * res).astype(np.float32)
            c[:, 2] = rng.normal(size=500)
            v = evalmap.render_fit(c, res, margin)
            img, st = evalmap.render(c, v, "height")
            assert st["n_outside"] == 0 and st["n_drawn"] == 500, (res, margin, st)
            img2, _ = evalmap.render(c[::-1], v, "height")
            assert (img == img2).all()


def test_render_eval_categories():
    # GT: two static, two dynamic; the estimate keeps one of each (same place, same class)
    gt = np.array([[0.25, 0.25, 0, S], [1.25, 0.25, 0, S], [0.25, 1.25, 0, D], [1.25, 1.25, 0, D]], np.float32)
    est = gt[[0, 2]].copy()
    v = evalmap.render_view(0.0, 0.0, 1.0, 2, 2, 0.0, 0.0, BG)
    img, st, ev = evalmap.render_eval(gt, est, v, voxelsize=0.2)
    want = np.array([[rgb(PAL[7]), rgb(PAL[5])], [rgb(PAL[4]), rgb(PAL[6])]], np.uint8)  # (north up: y = 1.25 is image row 0)
    assert (img == want).all()
    assert st["cat_points"] == [0, 0, 0, 0, 1, 1, 1, 1]
    assert st["cat_points"][4:] == [ev["preserved_static"], ev["gt_dynamic"] - ev["preserved_dynamic"],
                                    ev["gt_static"] - ev["preserved_static"], ev["preserved_dynamic"]]
    # a dynamic point left behind on top of a higher static point in the same pixel: the error is on top
    gt2 = np.array([[0.25, 0.25, 9.0, S], [0.75, 0.75, -9.0, D]], np.float32)
    img2, _, _ = evalmap.render_eval(gt2, gt2, evalmap.render_view(0.0, 0.0, 1.0, 1, 1, 0.0, 0.0, BG))
    assert (img2[0, 0] == rgb(PAL[7])).all()


def test_ppm_round_trip_and_panels(tmp_path):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    p = str(tmp_path / "a.ppm")
    erasor_amd.write_ppm(p, img)
    raw = open(p, "rb").read()
    assert raw.startswith(b"P6\n7 5\n255\n") and len(raw) == len(b"P6\n7 5\n255\n") + 5 * 7 * 3
    back = erasor_amd.read_ppm(p)
    assert back.dtype == np.uint8 and back.shape == (5, 7, 3) and (back == img).all()
    open(p, "wb").write(b"P6\n# a comment\n7 5\n255\n" + img.tobytes())
    assert (erasor_amd.read_ppm(p) == img).all()
    open(p, "wb").write(b"P5\n7 5\n255\n" + img.tobytes())
    with pytest.raises(ValueError):
        erasor_amd.read_ppm(p)
    a, b = img, rng.integers(0, 256, (5, 3, 3)).astype(np.uint8)
    out = erasor_amd.hstack_panels([a, b, a], gap=4, background=0x010203)
    assert out.shape == (5, 7 + 4 + 3 + 4 + 7, 3)
    assert (out[:, :7] == a).all() and (out[:, 11:14] == b).all() and (out[:, 18:] == a).all()
    assert (out[:, 7:11] == [1, 2, 3]).all() and (out[:, 14:18] == [1, 2, 3]).all()
    assert erasor_amd.hstack_panels([a], gap=9).shape == a.shape
    with pytest.raises(ValueError):
        erasor_amd.hstack_panels([a, b[:4]])
