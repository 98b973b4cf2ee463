"""evalmap.label_scans / moving_iou, the host oracle of Erasor.label_scans, on answers computed by hand: the strict threshold at one
float32 step either side, the 2 x 3 table and the IoU formula on a six-point frame, a frame whose points are all dropped, no frames.
No GPU needed."""
import numpy as np
import pytest

from erasor_amd import evalmap

EYE = np.eye(4, dtype=np.float32)


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def test_the_threshold_is_strict_at_one_float32_step_either_side():
    origin = np.zeros((1, 3), np.float32)
    below = np.nextafter(np.float32(0.5), np.float32(0))
    q = xyzi([[0.5, 0, 0], [below, 0, 0], [np.float32(0.3), np.float32(0.4), 0]])
    codes, rows, summary = evalmap.label_scans(origin, [q], [EYE], tau=0.5)
    # d == tau: not static; one step below: static; float32(0.3)^2 + float32(0.4)^2 = 0.25000001...: d = 0.50000001 > tau
    assert codes[0].tolist() == [1, 0, 1]
    d = np.sqrt(np.float64(np.float32(0.3)) ** 2 + np.float64(np.float32(0.4)) ** 2)
    assert d > 0.5 and d - 0.5 < 2e-8
    assert rows[0]["n"] == [[1, 2, 0], [0, 0, 0]] and summary == rows[0]
    # the same on each axis, and through the poses: a translation of the frame moves the point onto the threshold
    for axis in range(3):
        p = np.zeros((3, 3), np.float32)
        p[:, axis] = [-0.5, -below, np.nextafter(np.float32(0.5), np.float32(1))]
        assert evalmap.label_scans(origin, [xyzi(p)], [EYE], tau=0.5)[0][0].tolist() == [1, 0, 1]
    T = EYE.copy()
    T[0, 3] = 0.25
    assert evalmap.label_scans(origin, [xyzi([[0.25, 0, 0], [0.125, 0, 0]])], [T], tau=0.5)[0][0].tolist() == [1, 0]
    assert evalmap.label_scans(origin, [xyzi([[0.25, 0, 0], [0.125, 0, 0]])], [EYE], T, tau=0.5)[0][0].tolist() == [1, 0]


def test_the_squared_bound_decides_as_the_distance_does():
    for tau in (0.5, 0.2 * np.sqrt(3) / 2, 0.1, 1.0, 3.3, 1e-3):
        t2 = evalmap.label_bound(tau)
        assert np.sqrt(t2) < tau <= np.sqrt(np.nextafter(t2, np.inf))
        assert 0 <= (np.float64(tau) * np.float64(tau) - t2) / np.spacing(t2) <= 2
    assert evalmap.label_tau(0.2) == 0.2 * np.sqrt(3) / 2


def six_point_frame():
    """static map: a point at the origin; raw map: the origin and (10, 0, 0); tau = 0.5
    point            own label      code
    (0.1, 0, 0)      static (40)    0
    (0, 0.2, 0)      moving (252)   0  -> FN
    (10, 0.1, 0)     moving (259)   1  -> TP
    (10, 0, 0.3)     static (70)    1  -> FP
    (20, 0, 0)       moving (65536 * 7 + 253: instance bits ignored)  2 -> FN
    (30, 0, 0)       -1 (out of range: static, counted)               2"""
    pts = xyzi([[0.1, 0, 0], [0, 0.2, 0], [10, 0.1, 0], [10, 0, 0.3], [20, 0, 0], [30, 0, 0]], [40.0, 252.0, 259.0, 70.0, 65536.0 * 7 + 253.0, -1.0])
    smap = np.zeros((1, 3), np.float32)
    raw = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    return pts, smap, raw


def test_the_table_and_the_iou_formula_on_a_six_point_frame():
    pts, smap, raw = six_point_frame()
    codes, rows, summary, clouds = evalmap.label_scans(smap, [pts], [EYE], raw_xyz=raw, tau=0.5, split=1)
    assert codes[0].tolist() == [0, 0, 1, 1, 2, 2]
    assert rows[0] == {"n_points": 6, "n_non_finite": 0, "n_label_out_of_range": 1, "n": [[1, 1, 1], [1, 1, 1]]} and summary == rows[0]
    assert clouds[0].tobytes() == pts[2:4].tobytes()
    s = evalmap.moving_iou(summary)
    assert (s["TP"], s["FP"], s["FN"]) == (1, 1, 2)
    assert s["IoU"] == 1 / 4 and s["precision"] == 1 / 2 and s["recall"] == 1 / 3
    # without a raw map: everything that is not static is dynamic
    codes, rows, summary = evalmap.label_scans(smap, [pts], [EYE], tau=0.5)
    assert codes[0].tolist() == [0, 0, 1, 1, 1, 1] and rows[0]["n"] == [[1, 2, 0], [1, 2, 0]]
    s = evalmap.moving_iou(summary)
    assert (s["TP"], s["FP"], s["FN"]) == (2, 2, 1) and s["IoU"] == 2 / 5
    # an empty raw map that is given: everything that is not static is unknown; an empty static map: nothing is static
    assert evalmap.label_scans(smap, [pts], [EYE], raw_xyz=np.zeros((0, 3)), tau=0.5)[0][0].tolist() == [0, 0, 2, 2, 2, 2]
    assert evalmap.label_scans(np.zeros((0, 3)), [pts], [EYE], raw_xyz=raw, tau=0.5)[0][0].tolist() == [1, 1, 1, 1, 2, 2]
    # the static test comes first: a point only the cleaned map holds is static
    assert evalmap.label_scans(smap, [pts[:1]], [EYE], raw_xyz=raw[1:], tau=0.5)[0][0].tolist() == [0]
    for k in range(3):
        assert evalmap.label_scans(smap, [pts], [EYE], raw_xyz=raw, tau=0.5, split=k)[3][0].tobytes() == pts[2 * k:2 * k + 2].tobytes()
    nan = evalmap.moving_iou({"n": [[5, 0, 0], [0, 0, 0]]})
    assert np.isnan(nan["IoU"]) and np.isnan(nan["precision"]) and np.isnan(nan["recall"])
    with pytest.raises(ValueError):
        evalmap.label_scans(smap, [pts], [EYE], tau=0.5, split=2)
    with pytest.raises(ValueError):
        evalmap.label_scans(smap, [pts], [EYE], tau=0.0)


def test_a_frame_with_all_points_dropped_and_no_frames():
    smap = np.zeros((1, 3), np.float32)
    bad = xyzi([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], 252.0)
    big = np.diag([1e38, 1e38, 1e38, 1.0]).astype(np.float32)
    codes, rows, summary, clouds = evalmap.label_scans(smap, [bad, xyzi([[5.0, 6.0, 7.0]])], [EYE, big], raw_xyz=smap, split=0)
    assert codes[0].tolist() == [255, 255, 255] and codes[1].tolist() == [255]
    assert rows[0] == {"n_points": 3, "n_non_finite": 3, "n_label_out_of_range": 0, "n": [[0, 0, 0], [0, 0, 0]]}
    assert summary["n_points"] == 4 and summary["n_non_finite"] == 4 and [len(c) for c in clouds] == [0, 0]
    assert np.isnan(evalmap.moving_iou(summary)["IoU"])
    codes, rows, summary, clouds = evalmap.label_scans(smap, [], np.zeros((0, 4, 4), np.float32), split=1)
    assert codes == [] and rows == [] and clouds == []
    assert summary == {"n_points": 0, "n_non_finite": 0, "n_label_out_of_range": 0, "n": [[0, 0, 0], [0, 0, 0]]}
