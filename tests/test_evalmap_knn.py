"""evalmap.knn / radius_count / density_filter, the host restatement of the device's density analyses: the tree versions against every
pair by the predicate (knn_brute, radius_count_brute) on uniform clouds, integer lattices, 15-fold duplicates and the smallest clouds;
answers written by hand; and the MAD rule's arithmetic on hand-made scores.  No GPU."""
import math

import numpy as np
import pytest

from erasor_amd import evalmap

NONE = evalmap.KNN_NONE


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def same_numbers(a, b):
    return a.keys() == b.keys() and all((isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in a)


def same_knn(a, b):
    assert a.keys() == b.keys() and (a["n_points"], a["n_short"], a["k"]) == (b["n_points"], b["n_short"], b["k"])
    assert same_numbers(a["kth_stats"], b["kth_stats"]) and same_numbers(a["mean_stats"], b["mean_stats"])
    for key in ("kth", "mean", "nbr_idx", "nbr_dist"):
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key


def clouds(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return xyzi(rng.uniform(-5, 5, (n, 3)))
    if kind == "lattice":
        return xyzi(rng.integers(0, 6, (n, 3)))  # ties everywhere, and duplicates
    base = rng.uniform(-5, 5, (max(n // 15, 1), 3))
    return xyzi(np.repeat(base, 15, 0)[rng.permutation(len(base) * 15)][:n])  # 15-fold duplicates


@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("kind", ["uniform", "lattice", "duplicates"])
def test_the_tree_versions_equal_every_pair_by_the_predicate(kind, k):
    for n in (1500, 700):
        c = clouds(kind, n, 10 * k + n)
        same_knn(evalmap.knn(c, k, True), evalmap.knn_brute(c, k, True))
        for r in (0.4, 1.0, 2.5):
            a, b = evalmap.radius_count(c, r), evalmap.radius_count_brute(c, r)
            assert a[0].dtype == np.uint32 and a[0].tobytes() == b[0].tobytes() and same_numbers(a[1], b[1])


@pytest.mark.parametrize("k", [1, 8, 32])
def test_the_smallest_clouds(k):
    for n in (0, 1, 2, k, k + 1):
        c = clouds("uniform", n, n)
        a = evalmap.knn(c, k, True)
        same_knn(a, evalmap.knn_brute(c, k, True))
        short = n - 1 < k
        assert a["n_points"] == n and a["n_short"] == (n if short else 0) and a["nbr_idx"].shape == (n, k)
        if short and n:
            assert (a["nbr_idx"][:, n - 1:] == NONE).all() and np.isinf(a["nbr_dist"][:, n - 1:]).all() and np.isinf(a["kth"]).all() and np.isinf(a["mean"]).all()
            assert a["kth_stats"]["n_scored"] == 0 and math.isnan(a["mean_stats"]["p90"])
        x, y = evalmap.radius_count(c, 1.0), evalmap.radius_count_brute(c, 1.0)
        assert x[0].tobytes() == y[0].tobytes() and same_numbers(x[1], y[1])


def test_answers_written_by_hand():
    # a row of points on the x axis at 0, 1, 3, 6, and a duplicate of the first at the end
    c = xyzi([[0, 0, 0], [1, 0, 0], [3, 0, 0], [6, 0, 0], [0, 0, 0]])
    a = evalmap.knn(c, 2, True)
    assert a["nbr_idx"].tolist() == [[4, 1], [0, 4], [1, 0], [2, 1], [0, 1]]  # (equal d2: the lower index first; self by index only)
    assert a["nbr_dist"].tolist() == [[0, 1], [1, 1], [2, 3], [3, 5], [0, 1]]
    assert a["kth"].tolist() == [1, 1, 3, 5, 1] and a["mean"].tolist() == [0.5, 1, 2.5, 4, 0.5] and a["n_short"] == 0
    assert a["kth_stats"] == {"n_scored": 5, "min": 1.0, "median": 1.0, "p90": float(np.percentile([1.0, 1, 1, 3, 5], 90)),
                              "p99": float(np.percentile([1.0, 1, 1, 3, 5], 99)), "max": 5.0}
    assert abs(a["kth_stats"]["p90"] - 4.2) < 1e-12 and abs(a["kth_stats"]["p99"] - 4.92) < 1e-12
    cnt, st = evalmap.radius_count(c, 1.0)
    assert cnt.tolist() == [2, 2, 0, 0, 2] and st["n_scored"] == 5 and st["median"] == 2.0 and st["min"] == 0.0
    assert evalmap.radius_count(c, np.nextafter(1.0, 0))[0].tolist() == [1, 0, 0, 0, 1]
    # the count filter and the labels of what it removes
    c[:, 3] = [252, 40, 259, 40, 40]
    mask, kept, res = evalmap.density_filter(c, "count", radius=1.0, min_neighbors=1)
    assert mask.tolist() == [1, 1, 0, 0, 1] and kept.tobytes() == c[[0, 1, 4]].tobytes()
    assert (res["n_kept"], res["n_removed"], res["n_removed_dynamic"], res["n_removed_static"], res["n_short"], res["thr"]) == (3, 2, 1, 1, 0, 1.0)
    assert math.isnan(res["m"]) and math.isnan(res["mad"])
    mask, kept, res = evalmap.density_filter(c, "kth", k=2, rule="abs", thr=3.0, keep=False)
    assert mask.tolist() == [1, 1, 1, 0, 1] and kept is None and res["thr"] == 3.0 and res["max"] == 5.0


def test_the_mad_rule_on_hand_made_scores():
    inf = np.inf
    # odd n: m = 3, dev = 2 1 0 1 6, mad = 1, thr = 3 + 2 * 1.4826
    keep, m, mad, thr = evalmap.density_threshold([1.0, 2.0, 3.0, 4.0, 9.0], "mad", mul=2.0)
    assert (m, mad, thr) == (3.0, 1.0, 3.0 + 2.0 * (1.4826 * 1.0)) and keep.tolist() == [True, True, True, True, False]
    # even n: m = (2 + 4) / 2, dev = 2 1 1 7, mad = (1 + 2) / 2
    keep, m, mad, thr = evalmap.density_threshold([1.0, 2.0, 4.0, 10.0], "mad", mul=1.0)
    assert (m, mad, thr) == (3.0, 1.5, 3.0 + 1.0 * (1.4826 * 1.5)) and keep.tolist() == [True, True, True, False]
    # all scores equal: mad == 0, everything at m is kept, whatever the multiplier
    for mul in (0.0, 1.0, 1e300):
        keep, m, mad, thr = evalmap.density_threshold([0.25] * 6, "mad", mul=mul)
        assert (m, mad, thr) == (0.25, 0.0, 0.25) and keep.all()
    # infinite scores are outside the statistics and are never kept, even by an infinite threshold
    keep, m, mad, thr = evalmap.density_threshold([inf, 1.0, 2.0, 3.0, inf], "mad", mul=0.0)
    assert (m, mad, thr) == (2.0, 1.0, 2.0) and keep.tolist() == [False, True, True, False, False]
    keep, m, mad, thr = evalmap.density_threshold([inf, 1.0, 1e308, 1.7e308], "mad", mul=1e10)
    assert thr == inf and keep.tolist() == [False, True, True, True]
    # no finite score: NaN statistics, a NaN threshold, nothing kept
    for s in ([inf, inf, inf], []):
        keep, m, mad, thr = evalmap.density_threshold(s, "mad", mul=1.0)
        assert math.isnan(m) and math.isnan(mad) and math.isnan(thr) and not keep.any()
    # the absolute rule: <= thr
    keep, m, mad, thr = evalmap.density_threshold([0.5, np.nextafter(0.5, 1), inf], "abs", thr=0.5)
    assert keep.tolist() == [True, False, False] and math.isnan(m) and thr == 0.5


def test_refusals():
    c = clouds("uniform", 10, 0)
    for k in (0, 33, -1, 2.5):
        with pytest.raises(ValueError):
            evalmap.knn(c, k)
    for r in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            evalmap.radius_count(c, r)
    bad = c.copy()
    bad[3, 1] = np.nan
    for fn in (lambda: evalmap.knn(bad, 2), lambda: evalmap.radius_count(bad, 1.0), lambda: evalmap.density_filter(bad),
               lambda: evalmap.density_filter(c, "sigma"), lambda: evalmap.density_filter(c, "mean", rule="sigma"),
               lambda: evalmap.density_filter(c, "mean", k=4, rule="abs", thr=-1.0), lambda: evalmap.density_filter(c, "kth", k=4, rule="mad", mul=np.nan)):
        with pytest.raises(ValueError):
            fn()
