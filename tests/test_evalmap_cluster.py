"""evalmap.cluster, the host restatement of the device's Euclidean clustering, against answers written by hand (two blobs and a bridge
point, a chain, duplicates, the size limits, the -0.0 box) and against cluster_brute (every pair by the predicate) on random clouds.
No GPU."""
import numpy as np
import pytest

from erasor_amd import evalmap

NONE = evalmap.CLUSTER_NONE


def xyzi(xyz, w=40.0):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    w = np.broadcast_to(np.asarray(w, np.float32), (len(xyz),)).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([xyz, w], 1))


def row(first, n, dyn, oor, lo, hi):
    r = np.zeros(1, evalmap.CLUSTER_ROW_DTYPE)
    r["first"], r["n_points"], r["n_dynamic"], r["n_label_out_of_range"], r["min_xyz"], r["max_xyz"] = first, n, dyn, oor, lo, hi
    return r[0]


def test_two_blobs_and_a_bridge_point():
    a = [[0, 0, 0], [0.3, 0, 0], [0, 0.3, 0]]
    b = [[1.0, 0, 0], [1.3, 0, 0], [1.0, 0.25, 0]]
    cloud = xyzi([a[0], b[0], a[1], b[1], a[2], b[2]], [252, 40, 40, 259, -1, 40])
    rows, ids, kept, res = evalmap.cluster(cloud, 0.4)
    assert res == {"n_points": 6, "n_clusters": 2, "n_listed": 2, "n_points_listed": 6, "n_singletons": 0, "largest": 3}
    assert ids.tolist() == [0, 1, 0, 1, 0, 1] and kept.tobytes() == cloud.tobytes()
    assert rows[0] == row(0, 3, 1, 1, [0, 0, 0], np.float32([0.3, 0.3, 0])) and rows[1] == row(1, 3, 1, 0, [1, 0, 0], np.float32([1.3, 0.25, 0]))
    # a bridge point joins them; it comes last and the cluster keeps its name
    bridged = np.concatenate([cloud, xyzi([[0.65, 0, 0]])])
    rows, ids, kept, res = evalmap.cluster(bridged, 0.4)
    assert res["n_clusters"] == 1 and res["largest"] == 7 and ids.tolist() == [0] * 7
    assert rows[0] == row(0, 7, 2, 1, [0, 0, 0], np.float32([1.3, 0.3, 0]))
    # exactly at the tolerance: joined; the predicate is <=
    assert evalmap.cluster(xyzi([[0, 0, 0], [0.5, 0, 0]]), 0.5)[3]["n_clusters"] == 1
    assert evalmap.cluster(xyzi([[0, 0, 0], [np.nextafter(np.float32(0.5), np.float32(1)), 0, 0]]), 0.5)[3]["n_clusters"] == 2


def test_a_chain_duplicates_and_names_by_lowest_index():
    n = 200
    xyz = np.stack([np.arange(n) * 0.45, np.zeros(n), np.zeros(n)], 1)
    for perm in (np.arange(n), np.arange(n)[::-1], np.random.default_rng(1).permutation(n)):
        rows, ids, _, res = evalmap.cluster(xyzi(xyz[perm]), 0.5)
        assert res["n_clusters"] == 1 and rows["first"].tolist() == [0] and (ids == 0).all()
    # the chain cut in two: the clusters are numbered by their lowest index, whichever half holds it
    xyz[120:, 0] += 1.0
    perm = np.random.default_rng(2).permutation(n)
    rows, ids, _, res = evalmap.cluster(xyzi(xyz[perm]), 0.5)
    assert res["n_clusters"] == 2 and rows["first"].tolist() == [0, int(np.flatnonzero((perm < 120) != (perm[0] < 120))[0])]
    assert ((ids == 0) == ((perm < 120) == (perm[0] < 120))).all()
    dup = xyzi(np.tile([[1.0, 2.0, 3.0]], (50, 1)), 253)
    rows, ids, _, res = evalmap.cluster(dup, 1e-6)
    assert res["n_clusters"] == 1 and rows[0] == row(0, 50, 50, 0, [1, 2, 3], [1, 2, 3])


def test_size_limits_ids_and_kept_cloud():
    # clusters of 1, 2, 3 and 4 points, interleaved
    pts = [[10.0 * c + 0.1 * k, 0, 0] for k in range(4) for c in range(4) if k <= c]
    cloud = xyzi(pts, np.arange(len(pts)))
    size_of = [1, 2, 3, 4]
    for mn, mx, listed in ((1, 0, [0, 1, 2, 3]), (0, 0, [0, 1, 2, 3]), (2, 0, [1, 2, 3]), (2, 3, [1, 2]), (3, 3, [2]), (4, 2, []), (5, 0, []), (1, 1, [0])):
        rows, ids, kept, res = evalmap.cluster(cloud, 0.5, mn, mx)
        assert rows["n_points"].tolist() == [size_of[c] for c in listed] and rows["first"].tolist() == listed
        assert res == {"n_points": 10, "n_clusters": 4, "n_listed": len(listed), "n_points_listed": sum(size_of[c] for c in listed),
                       "n_singletons": 1, "largest": 4}
        c_of = np.array([c for k in range(4) for c in range(4) if k <= c])
        want = np.array([listed.index(c) if c in listed else NONE for c in c_of], np.uint32)
        assert ids.tolist() == want.tolist() and kept.tobytes() == cloud[want != NONE].tobytes()


def test_the_box_orders_signed_zeros_and_copies_bits():
    cloud = xyzi([[0.0, -0.0, 0.0], [-0.0, 0.0, 0.0], [0.0, 0.0, -1e-45]])
    rows = evalmap.cluster(cloud, 0.1)[0]
    assert rows["min_xyz"].view(np.uint32).tolist() == [[0x80000000, 0x80000000, 0x80000001]]
    assert rows["max_xyz"].view(np.uint32).tolist() == [[0, 0, 0]]


def test_labels_and_out_of_range_intensities():
    w = np.float32([251, 252, 259, 260, 252 + (7 << 16), np.nan, -1, 4294967296.0, np.inf, 0])
    rows = evalmap.cluster(xyzi(np.zeros((10, 3)), w), 0.5)[0]
    assert rows["n_dynamic"].tolist() == [3] and rows["n_label_out_of_range"].tolist() == [4]


def test_refusals_and_the_empty_cloud():
    for tol in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            evalmap.cluster(xyzi([[0, 0, 0]]), tol)
    with pytest.raises(ValueError):
        evalmap.cluster(xyzi([[0, np.nan, 0]]), 0.5)
    rows, ids, kept, res = evalmap.cluster(np.zeros((0, 4), np.float32), 0.5)
    assert len(rows) == len(ids) == len(kept) == 0 and res == dict.fromkeys(evalmap.CLUSTER_RESULT_FIELDS, 0)
    assert evalmap.cluster_brute(np.zeros((0, 4), np.float32), 0.5)[3] == res


@pytest.mark.parametrize("seed,n,span,tol,limits", [(1, 1500, 4.0, 0.5, (1, 0)), (2, 2500, 9.0, 0.5, (2, 40)), (3, 800, 1.0, 0.2, (3, 0)),
                                                    (4, 2000, 1e5, 300.0, (1, 5)), (5, 1200, 0.5, 0.02, (1, 0))])
def test_the_tree_version_equals_every_pair_by_the_predicate(seed, n, span, tol, limits):
    rng = np.random.default_rng(seed)
    cloud = xyzi(rng.uniform(-span, span, (n, 3)), rng.integers(240, 270, n))
    k = len(cloud[3::7])
    cloud[:7 * k:7, :3] = cloud[3::7, :3]  # duplicates among them
    a, b = evalmap.cluster(cloud, tol, *limits), evalmap.cluster_brute(cloud, tol, *limits)
    assert a[3] == b[3] and 1 < a[3]["n_clusters"] < n
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
