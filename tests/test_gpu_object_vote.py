"""The decision per object on the device (erasor_hip_object_vote_clouds / _map, kernels in objects.hip.h) against its host text
evalmap.object_vote / object_vote_brute: byte for byte in mask, rows, ids, kept cloud and result.  A scene whose answer is written out
by hand, the ground outside the graph, the predicate's edge through the compaction, every decision at its edge and their order, the
vote threshold, ground points at every position of the indexing, every size around the wavefront, workgroup and scan-block edges,
contention on one root, many rows and short buffers, the handle's map with a step after it, the errors and the struct layout, and a
synthetic world with the carving's votes and the ground's mask.  tests/test_object_vote_on_cpu.py re-runs this file against the CPU
stand-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import erasor_amd
import object_scenes as S
import scenarios
from erasor_amd import evalmap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_CPU = bool(os.environ.get("ERASOR_TEST_SIMT_LIB"))
NONE = evalmap.OBJECT_NONE
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
xyzi = S.xyzi


@pytest.fixture(scope="module")
def gpu_mod():
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


@pytest.fixture(scope="module")
def handle(gpu_mod):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    yield g
    g.close()


def check(g, cloud, votes, ground=None, ref=evalmap.object_vote, what="", **prm):
    """the device against the host text; what the host text returned"""
    want = ref(cloud, votes, ground, **prm)
    S.assert_same(g.object_vote(cloud, votes, ground, **prm), want, (what, prm))
    return want


# ---- 1. the known answer ----
@pytest.mark.parametrize("ground_keep", [True, False])
def test_known_answer(handle, ground_keep):
    cloud, votes, ground = S.known_scene()
    want = check(handle, cloud, votes, ground, ground_keep=ground_keep, **S.KNOWN_PARAMS)
    mask, rows, res = S.known_answer(ground_keep)
    assert want[4] == res and want[0].tobytes() == mask.tobytes() and want[1].tobytes() == rows.tobytes()
    assert want[1]["decision"].tolist() == [S.REMOVED, S.REVERTED, S.UNCHANGED, S.NOT_OBJECT] and res["n_grown"] == 45
    assert want[3].tobytes() == cloud[mask != 0].tobytes()


def test_known_scene_without_the_ground_mask_is_one_cluster(handle):
    cloud, votes, _ = S.known_scene()
    want = check(handle, cloud, votes, None, **S.KNOWN_PARAMS)
    assert len(want[1]) == 1 and want[1]["first"][0] == 0 and want[1]["n_points"][0] == 1531 and want[1]["n_voted"][0] == 733
    assert want[1]["decision"][0] == S.NOT_OBJECT and want[4]["n_clusters"] == 1 and want[4]["n_removed"] == 733 and want[4]["n_grown"] == 0


# ---- 2. the ground is outside the graph ----
def test_ground_is_outside_the_graph(handle):
    cloud, votes, ground = S.bridge_scene()
    a = check(handle, cloud, votes, ground, ref=evalmap.object_vote_brute, tol=0.3)
    b = check(handle, cloud, votes, None, ref=evalmap.object_vote_brute, tol=0.3)
    assert a[4]["n_clusters"] == 2 and a[0].tolist() == [0, 1, 1] and a[2].tolist() == [0, NONE, NONE]
    assert b[4]["n_clusters"] == 1 and b[0].tolist() == [0, 1, 1] and b[2].tolist() == [0, 0, 0]


# ---- 3. the predicate's edge, through the compaction ----
@pytest.mark.parametrize("tol", [0.5, 1.0])
def test_the_edge_pair_with_ground_points_interleaved(handle, tol):
    """cluster's edge pair -- exactly tol apart, and one float32 step further -- with a ground point that would bridge it between the
    two and ground points around them"""
    far = np.nextafter(np.float32(tol), np.float32(np.inf))
    pts = [[-5, 0, 0], [0, 0, 0], [tol / 2, 0, 0], [tol, 0, 0], [-5, 16, 0], [0, 16, 0], [tol / 2, 16, 0], [far, 16, 0], [9, 9, 9]]
    ground = np.uint8([1, 0, 1, 0, 1, 0, 1, 0, 1])
    votes = np.uint8([0, 1, 1, 1, 0, 1, 0, 0, 1])
    want = check(handle, xyzi(pts), votes, ground, ref=evalmap.object_vote_brute, tol=tol)
    assert want[4]["n_clusters"] == 3 and want[1]["first"].tolist() == [1, 5] and want[1]["n_points"].tolist() == [2, 1]
    assert want[2].tolist() == [NONE, 0, NONE, 0, NONE, 1, NONE, NONE, NONE]
    want = check(handle, xyzi(pts), votes, None, ref=evalmap.object_vote_brute, tol=tol)
    assert want[4]["n_clusters"] == 5  # the bridges join both pairs; the three far points stay alone


# ---- 4. the decisions at their edges ----
def blobs(sizes, n_voted):
    """one cluster per entry: sizes[c] points 0.01 m apart on a line from x = 0.1, 8 m from the next cluster, the first n_voted[c] of
    them voted; the clusters' points interleaved round-robin through the cloud.  Returns (cloud, votes, cluster of every point)"""
    own = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)])
    k = np.concatenate([np.arange(s) for s in sizes])
    order = np.lexsort((own, k))  # (point 0 of every cluster, then point 1 of every cluster that has one, ...)
    own, k = own[order], k[order]
    cloud = xyzi(np.stack([0.1 + 0.01 * k, 8.0 * own, np.zeros(len(k))], 1), 252.0)
    return cloud, (k < np.asarray(n_voted)[own]).astype(np.uint8), own


def around(n, ratio, ge):
    """the n_voted values on and one either side of ratio * n: ge: the lowest k with k >= ratio * n, else the highest with k <= ratio * n"""
    t = np.float64(ratio) * np.float64(n)
    edge = min(k for k in range(n + 1) if np.float64(k) >= t) if ge else max(k for k in range(n + 1) if np.float64(k) <= t)
    return [k for k in (edge - 1, edge, edge + 1) if 0 <= k <= n]


@pytest.mark.parametrize("ratio", [0.5, 0.25, 0.3, 0.7, 1 / 3, 1.0])
def test_remove_ratio_at_its_edge(handle, ratio):
    sizes, nv = [], []
    for n in (3, 7, 10, 64):
        for k in around(n, ratio, True):
            sizes.append(n)
            nv.append(k)
    cloud, votes, own = blobs(sizes, nv)
    want = check(handle, cloud, votes, tol=0.5, remove_ratio=ratio)
    dec = dict(zip(own[want[1]["first"]].tolist(), want[1]["decision"].tolist()))
    seen = set()
    for c, (n, k) in enumerate(zip(sizes, nv)):
        removed = k >= 1 and np.float64(k) >= np.float64(ratio) * np.float64(n)
        assert dec.get(c, None) == (None if k == 0 else S.REMOVED if removed else S.UNCHANGED), (ratio, n, k)
        seen.add(bool(removed))
    assert seen == {True, False}


@pytest.mark.parametrize("ratio", [0.5, 0.25, 0.3, 0.7, 1 / 3])
def test_revert_ratio_at_its_edge(handle, ratio):
    sizes, nv = [], []
    for n in (3, 7, 10, 64):
        for k in around(n, ratio, False):
            sizes.append(n)
            nv.append(k)
    cloud, votes, own = blobs(sizes, nv)
    want = check(handle, cloud, votes, tol=0.5, remove_ratio=1.0, revert_ratio=ratio)
    dec = dict(zip(own[want[1]["first"]].tolist(), want[1]["decision"].tolist()))
    seen = set()
    for c, (n, k) in enumerate(zip(sizes, nv)):
        reverted = 0 < k < n and np.float64(k) <= np.float64(ratio) * np.float64(n)
        assert dec.get(c, None) == (None if k == 0 else S.REMOVED if k == n else S.REVERTED if reverted else S.UNCHANGED), (ratio, n, k)
        seen.add(bool(reverted))
    assert seen == {True, False}
    assert want[4]["n_reverted"] == sum(k for n, k in zip(sizes, nv) if 0 < k < n and np.float64(k) <= np.float64(ratio) * np.float64(n))


def test_gates_min_voted_and_the_order_of_the_tests(handle):
    n = 10
    cloud, votes, _ = blobs([n], [6])
    one = lambda **kw: check(handle, cloud, votes, tol=0.5, **kw)[1]["decision"].tolist()  # noqa: E731
    assert one(min_voted=6) == [S.REMOVED] and one(min_voted=7) == [S.UNCHANGED] and one(min_voted=2 ** 40) == [S.UNCHANGED]
    assert one(max_size=n) == [S.REMOVED] and one(max_size=n - 1) == [S.NOT_OBJECT] and one(max_size=2 ** 40) == [S.REMOVED]
    assert one(min_size=n) == [S.REMOVED] and one(min_size=n + 1) == [S.NOT_OBJECT] and one(min_size=0) == [S.REMOVED]
    # max_extent: exactly the box side -- a float64 difference of float32 values -- and one float32 step less
    x = cloud[:, 0]
    side = np.float64(x.max()) - np.float64(x.min())
    less = float(np.nextafter(np.float32(side), np.float32(-np.inf)))
    assert less < side
    assert one(max_extent=float(side)) == [S.REMOVED] and one(max_extent=less) == [S.NOT_OBJECT]
    # a cluster that passes the ratio (all of it voted) and fails a gate gets code 3, and its votes stand
    cloud, votes, _ = blobs([n], [n])
    want = check(handle, cloud, votes, tol=0.5, max_size=n - 1)
    assert want[1]["decision"].tolist() == [S.NOT_OBJECT] and want[4]["n_not_object"] == 1 and want[4]["n_removed_clusters"] == 0 and not want[0].any()
    # ... and one that would be reverted
    cloud, votes, _ = blobs([64], [1])
    want = check(handle, cloud, votes, tol=0.5, revert_ratio=0.1, min_size=65)
    assert want[1]["decision"].tolist() == [S.NOT_OBJECT] and want[4]["n_reverted"] == 0 and want[0].sum() == 63
    assert check(handle, cloud, votes, tol=0.5, revert_ratio=0.1)[1]["decision"].tolist() == [S.REVERTED]


# ---- 5. the vote threshold ----
@pytest.mark.parametrize("thr", [1, 2, 255])
def test_vote_threshold(handle, thr):
    v = np.uint8([0, 1, 2, 254, 255])
    cloud = xyzi(np.stack([np.arange(5) * 4.0, np.zeros(5), np.zeros(5)], 1))
    want = check(handle, cloud, v, tol=0.5, vote_thr=thr)
    assert want[0].tolist() == (v < thr).astype(int).tolist() and want[4]["n_voted"] == int((v >= thr).sum()) == want[4]["n_touched"]


# ---- 6. the indexing ----
@pytest.mark.parametrize("pattern", ["GPPP", "PGPP", "PPGP", "PPPG", "GPGPGPG", "GGPPPGG", "PPP"])
def test_ground_points_at_every_position_of_a_cluster(handle, pattern):
    is_g = np.array([ch == "G" for ch in pattern])
    cloud = xyzi(np.stack([np.where(is_g, 0.1, 0.0) + 0.05 * np.arange(len(pattern)), np.zeros(len(pattern)), np.zeros(len(pattern))], 1), 253.0)
    votes = np.ones(len(pattern), np.uint8)
    votes[np.flatnonzero(~is_g)[1]] = 0  # (the cluster's second point is not voted: 2 of 3 -> removed, one point grown)
    want = check(handle, cloud, votes, is_g.astype(np.uint8), ref=evalmap.object_vote_brute, tol=0.5)
    first = int(np.flatnonzero(~is_g)[0])
    assert want[1]["first"].tolist() == [first] and want[1]["n_points"].tolist() == [3] and want[1]["decision"].tolist() == [S.REMOVED]
    assert want[2].tolist() == [NONE if g else 0 for g in is_g] and want[0].tolist() == [1 if g else 0 for g in is_g]
    assert want[4]["n_grown"] == 1 and want[4]["n_ground_reverted"] == int(is_g.sum())
    if not is_g.any():  # no point ground: the mask array of zeros and no array are the same call
        S.assert_same(handle.object_vote(cloud, votes, None, tol=0.5), want, "no mask array")


def test_all_ground_n_zero_and_n_one(handle):
    cloud, votes, _ = S.bridge_scene()
    for keep in (True, False):
        want = check(handle, cloud, votes, np.ones(3, np.uint8), tol=0.3, ground_keep=keep)
        assert want[4]["n_clusters"] == 0 and want[4]["n_ground"] == 3 and want[0].tolist() == ([1, 1, 1] if keep else [0, 1, 1]) and len(want[1]) == 0
    z = np.zeros((0, 4), np.float32)
    for ground in (None, np.zeros(0, np.uint8)):
        want = check(handle, z, np.zeros(0, np.uint8), ground, tol=0.5)
        assert want[4] == dict.fromkeys(evalmap.OBJECT_RESULT_FIELDS, 0)
    for v, g in ((0, 0), (1, 0), (0, 1), (1, 1)):
        want = check(handle, xyzi([[1, 2, 3]]), np.uint8([v]), np.uint8([g]), tol=0.5)
        assert want[0].tolist() == [0 if v and not g else 1] and want[2].tolist() == [0 if v and not g else NONE]


# ---- 7. sizes ----
def mixed(n, tol=0.5):
    """n points: adjacent pairs on a 3 tol grid and, from the middle on, one chain; every third point is ground (and lies where it would
    bridge its neighbours); two of five points voted"""
    i = np.arange(n)
    xyz = np.stack([(i // 2 % 40) * 3.0 * tol, (i // 80) * 3.0 * tol, (i % 2) * 0.5 * tol], 1)
    chain = i >= n // 2
    xyz[chain] = np.stack([(i[chain] - n // 2) * 0.45 * tol, np.full(chain.sum(), -50.0), np.zeros(chain.sum())], 1)
    return xyzi(xyz, i % 4 + 250), (i % 5 < 2).astype(np.uint8), (i % 3 == 0).astype(np.uint8)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_sizes_with_every_third_point_ground(handle, n):
    cloud, votes, ground = mixed(n)
    want = check(handle, cloud, votes, ground, tol=0.5, remove_ratio=0.5, revert_ratio=0.25, max_size=n // 4, what=("mixed", n))
    assert want[4]["n_ground"] == (n + 2) // 3 and want[4]["n_clusters"] > 1
    if n >= 255:
        assert want[4]["n_touched"] > 8 and want[4]["n_removed_clusters"] > 0 and want[4]["n_not_object"] == 1
    check(handle, cloud, votes, None, tol=0.5, revert_ratio=0.25, what=("mixed, no mask", n))


# ---- 8. contention: every wavefront's tally on one root ----
def test_a_crowded_ball_counts_exactly(handle):
    rng = np.random.default_rng(5)
    n, side = 4096, 0.5 / np.sqrt(3.0) * 0.99
    i = np.arange(n + n // 4)
    ground = (i % 5 == 4).astype(np.uint8)  # (n non-ground points, a ground point after every fourth)
    assert int((ground == 0).sum()) == n
    k = np.cumsum(ground == 0) - 1  # the running number of the non-ground points
    cloud = xyzi(rng.uniform(0, side, (len(i), 3)) + [10.0, 20.0, -3.0], np.where(k % 4 < 2, 252.0, 40.0))
    votes = (k % 2 == 0).astype(np.uint8)
    want = check(handle, cloud, votes, ground, tol=0.5, what="ball")
    assert want[4]["n_clusters"] == 1 and want[4]["largest"] == n
    r = want[1][0]
    assert (r["first"], r["n_points"], r["n_voted"], r["n_dynamic"], r["n_voted_dynamic"], r["decision"]) == (0, n, n // 2, n // 2, n // 4, S.REMOVED)
    assert want[4]["n_grown"] == n // 2 and want[4]["n_grown_dynamic"] == n // 4 and want[4]["n_removed"] == n


# ---- 9. many rows, short buffers ----
def many_pairs(n_pairs=3000):
    i = np.arange(2 * n_pairs)
    p = i // 2
    cloud = xyzi(np.stack([(p % 60) * 2.0, (p // 60) * 2.0, (i % 2) * 0.25], 1), i % 3 + 251)
    votes = ((p % 2 == 0) & ((i % 2 == 0) | (p % 4 == 0))).astype(np.uint8)  # every other pair touched: one vote, or both
    return cloud, votes


def raw_call(gpu_mod, g, cloud, votes, ground, prm, mask, ids, rows, cap_rows, kept, cap_kept, res, n=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return gpu_mod.lib().erasor_hip_object_vote_clouds(g._h, p(cloud), C.c_size_t(len(cloud) if n is None else n), C.c_int(0), p(votes), p(ground),
                                                       None if prm is None else C.byref(prm), p(mask), p(ids), p(rows), C.c_size_t(cap_rows), p(kept),
                                                       C.c_size_t(cap_kept), None if res is None else C.byref(res))


def params(gpu_mod, tol=0.5, vote_thr=1, min_size=1, max_size=0, max_extent=0.0, remove_ratio=0.5, revert_ratio=0.0, min_voted=1, ground_keep=1):
    return gpu_mod.ObjectVoteParams(tol=tol, max_extent=max_extent, remove_ratio=remove_ratio, revert_ratio=revert_ratio, min_size=min_size,
                                    max_size=max_size, min_voted=min_voted, vote_thr=vote_thr, ground_keep=ground_keep)


def test_many_rows_in_first_order_and_buffers_too_small(handle, gpu_mod):
    cloud, votes = many_pairs()
    want = check(handle, cloud, votes, tol=0.5, remove_ratio=1.0, what="pairs")
    nr, nk = want[4]["n_touched"], len(want[3])
    assert nr == 1500 and (np.diff(want[1]["first"].astype(np.int64)) > 0).all() and want[1]["first"].tolist() == list(range(0, 6000, 4))
    assert set(want[1]["decision"].tolist()) == {S.REMOVED, S.UNCHANGED} and 0 < nk < len(cloud)
    P = params(gpu_mod, remove_ratio=1.0)
    res = gpu_mod.ObjectVoteResult()
    assert raw_call(gpu_mod, handle, cloud, votes, None, P, None, None, None, 0, None, 0, res) == 0 and res.as_dict() == want[4]  # counts only
    rows = np.zeros(nr + 2, gpu_mod.OBJECT_ROW_DTYPE)
    kept = np.full((nk + 2, 4), -7.0, np.float32)
    mask = np.full(len(cloud), 9, np.uint8)
    ids = np.full(len(cloud), 12345, np.uint32)
    assert raw_call(gpu_mod, handle, cloud, votes, None, P, mask, ids, rows, nr, kept, nk, res) == 0  # exactly enough
    assert rows[:nr].tobytes() == want[1].tobytes() and rows[nr:].tobytes() == bytes(2 * rows.itemsize)
    assert mask.tobytes() == want[0].tobytes() and ids.tobytes() == want[2].tobytes()
    assert kept[:nk].tobytes() == want[3].tobytes() and (kept[nk:] == -7.0).all()
    for cap_rows, cap_kept in ((nr - 1, nk), (nr, nk - 1), (0, 0)):
        res = gpu_mod.ObjectVoteResult()
        mask[:], ids[:] = 9, 12345
        assert raw_call(gpu_mod, handle, cloud, votes, None, P, mask, ids, rows, cap_rows, kept, cap_kept, res) == E_CAPACITY
        assert res.as_dict() == want[4] and mask.tobytes() == want[0].tobytes() and ids.tobytes() == want[2].tobytes()  # filled first
    # one buffer alone
    assert raw_call(gpu_mod, handle, cloud, votes, None, P, None, None, None, 0, kept, nk, res) == 0 and kept[:nk].tobytes() == want[3].tobytes()
    assert raw_call(gpu_mod, handle, cloud, votes, None, P, None, None, rows, nr, None, 0, res) == 0 and rows[:nr].tobytes() == want[1].tobytes()


# ---- 10. the handle's map ----
def test_object_vote_map_and_the_step_after_it(gpu_mod):
    sc = scenarios.small(n_frames=4, az=60) if ON_CPU else scenarios.small()
    n = 3
    g, plain = (gpu_mod.Erasor(scenarios.to_product_params(sc["params"])) for _ in range(2))
    for e in (g, plain):
        e.set_map(sc["map"])
        for f in range(n):
            e.step(sc["scans"][f], sc["T_l2b"], sc["T_b2o"][f], sc["T_o2b"][f])
    ticket = g.prefetch_node_rows(np.ascontiguousarray(sc["scans"][n], np.float32), 3, sc["T_l2b"], sc["T_b2o"][n], sc["T_o2b"][n])
    m = np.ascontiguousarray(g.get_map(), np.float32)
    rng = np.random.default_rng(4)
    votes = (rng.uniform(0, 1, len(m)) < 0.2).astype(np.uint8) * rng.integers(1, 4, len(m)).astype(np.uint8)
    ground = (m[:, 2] < np.median(m[:, 2])).astype(np.uint8)
    prm = dict(tol=0.3, vote_thr=2, remove_ratio=0.3, revert_ratio=0.1, max_size=200)
    got = g.object_vote_map(votes, ground, **prm)
    want = evalmap.object_vote(m, votes, ground, **prm)
    S.assert_same(got, want, "object_vote_map")
    S.assert_same(g.object_vote(m, votes, ground, **prm), want, "object_vote(get_map())")
    assert want[4]["n_touched"] > 10 and want[4]["n_removed_clusters"] > 0
    for wrong in (len(m) - 1, len(m) + 1):
        with pytest.raises(gpu_mod.ErasorError) as e:
            g.object_vote_map(np.resize(votes, wrong), None, **prm)
        assert e.value.rc == E_INVALID and "map's size" in str(e.value)
    # the announcement and the last step's clouds are untouched: the next step is the uninterrupted run's
    a = g.step_ticket(ticket, sc["T_b2o"][n], sc["T_o2b"][n])
    b = plain.step(sc["scans"][n], sc["T_l2b"], sc["T_b2o"][n], sc["T_o2b"][n])
    assert a.as_dict() == b.as_dict()
    assert g.get_map().tobytes() == plain.get_map().tobytes()
    for which in (gpu_mod.CLOUD_MAP_REJECTED, gpu_mod.CLOUD_STATIC_ESTIMATE):
        assert g.get_cloud(which).tobytes() == plain.get_cloud(which).tobytes()
    g.close()
    plain.close()


# ---- 11. errors and the struct layout ----
def test_errors_and_struct_layout(gpu_mod, tmp_path):
    g = gpu_mod.Erasor(gpu_mod.params_default())
    try:
        cloud, votes, ground = S.bridge_scene()

        def refused(rc, fn, *a, **kw):
            with pytest.raises(gpu_mod.ErasorError) as e:
                fn(*a, **kw)
            assert e.value.rc == rc, str(e.value)
            return str(e.value)

        for tol in (0.0, -0.5, float("nan"), float("inf")):
            assert "tol" in refused(E_INVALID, g.object_vote, cloud, votes, ground, tol=tol)
        for r in (0.0, -0.1, 1.5, float("nan")):
            assert "remove_ratio" in refused(E_INVALID, g.object_vote, cloud, votes, ground, remove_ratio=r)
        for kw in (dict(revert_ratio=-0.1), dict(revert_ratio=1.0, remove_ratio=1.0), dict(revert_ratio=0.5), dict(revert_ratio=0.6),
                   dict(revert_ratio=float("nan"))):
            assert "revert_ratio" in refused(E_INVALID, g.object_vote, cloud, votes, ground, **kw)
        for thr in (0, 256, 2 ** 31):
            assert "vote_thr" in refused(E_INVALID, g.object_vote, cloud, votes, ground, vote_thr=thr)
        for ext in (-1.0, float("inf"), float("nan")):
            assert "max_extent" in refused(E_INVALID, g.object_vote, cloud, votes, ground, max_extent=ext)
        assert "one entry per point" in refused(E_INVALID, g.object_vote, cloud, votes[:2], ground)
        assert "one entry per point" in refused(E_INVALID, g.object_vote, cloud, votes, ground[:2])
        for bad in (np.nan, np.inf, -np.inf):
            for row in range(3):  # (row 1 is the ground point: refused as any other)
                c = cloud.copy()
                c[row, row] = bad
                assert "non-finite" in refused(E_INVALID, g.object_vote, c, votes, ground)
        P, res = params(gpu_mod), gpu_mod.ObjectVoteResult()
        assert raw_call(gpu_mod, g, cloud, votes, ground, P, None, None, None, 0, None, 0, res, n=2 ** 30 + 1) == E_INVALID
        assert raw_call(gpu_mod, g, None, votes, ground, P, None, None, None, 0, None, 0, res, n=3) == E_INVALID
        assert raw_call(gpu_mod, g, cloud, None, ground, P, None, None, None, 0, None, 0, res) == E_INVALID  # votes NULL
        assert raw_call(gpu_mod, g, cloud, votes, ground, None, None, None, None, 0, None, 0, res) == E_INVALID  # params NULL
        assert raw_call(gpu_mod, g, cloud, votes, ground, P, None, None, None, 0, None, 0, None) == E_INVALID  # res NULL
        assert raw_call(gpu_mod, g, cloud, votes, ground, params(gpu_mod, tol=0.3), None, None, None, 0, None, 0, res) == 0 and res.n_clusters == 2
        # the handle's map: none yet; then a step in flight
        assert "no map" in refused(E_STATE, g.object_vote_map, votes)
        sc = scenarios.small(n_frames=2, az=60)
        g.set_map(sc["map"])
        g.step_async(sc["scans"][0], T_l2b=sc["T_l2b"], T_b2o=sc["T_b2o"][0], T_o2b=sc["T_o2b"][0])
        refused(E_STATE, g.object_vote, cloud, votes, ground)
        refused(E_STATE, g.object_vote_map, votes)
        g.step_wait()
        assert g.object_vote(cloud, votes, ground, tol=0.3)[4]["n_clusters"] == 2  # the handle is fine after the refusals
    finally:
        g.close()
    # the header's layout
    P, R, T = gpu_mod.ObjectVoteParams, gpu_mod.ObjectRow, gpu_mod.ObjectVoteResult
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "erasor_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
            'sizeof(erasor_object_vote_params), sizeof(erasor_object_row), sizeof(erasor_object_vote_result), offsetof(erasor_object_vote_params, max_extent), '
            'offsetof(erasor_object_vote_params, revert_ratio), offsetof(erasor_object_vote_params, min_size), offsetof(erasor_object_vote_params, min_voted), '
            'offsetof(erasor_object_vote_params, vote_thr), offsetof(erasor_object_vote_params, ground_keep), offsetof(erasor_object_row, n_voted_dynamic), '
            'offsetof(erasor_object_row, min_xyz), offsetof(erasor_object_row, decision), offsetof(erasor_object_vote_result, n_removed), '
            'offsetof(erasor_object_vote_result, largest));return 0;}\n')
    src, exe = tmp_path / "p.c", tmp_path / "p"
    src.write_text(code)
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(P), C.sizeof(R), C.sizeof(T), P.max_extent.offset, P.revert_ratio.offset, P.min_size.offset, P.min_voted.offset, P.vote_thr.offset,
                   P.ground_keep.offset, R.n_voted_dynamic.offset, R.min_xyz.offset, R.decision.offset, T.n_removed.offset, T.largest.offset]
    assert C.sizeof(P) == 64 and C.sizeof(R) == 52 == gpu_mod.OBJECT_ROW_DTYPE.itemsize == evalmap.OBJECT_ROW_DTYPE.itemsize and C.sizeof(T) == 128
    assert gpu_mod.OBJECT_ROW_DTYPE == evalmap.OBJECT_ROW_DTYPE
    assert (gpu_mod.OBJECT_UNCHANGED, gpu_mod.OBJECT_REMOVED, gpu_mod.OBJECT_REVERTED, gpu_mod.OBJECT_NOT_OBJECT, gpu_mod.OBJECT_NONE) == (0, 1, 2, 3, NONE)
    m = gpu_mod.votes_from_masks(np.uint8([1, 0, 0, 1]), np.uint8([1, 1, 0, 0]), np.uint8([1, 1, 0, 1]))
    assert m.dtype == np.uint8 and m.tolist() == [0, 1, 3, 1]
    assert gpu_mod.votes_from_masks(*[np.uint8([0, 1])] * 300).tolist() == [255, 0]  # saturating


# ---- 12. the synthetic world: the carving's votes, the ground's mask ----
def test_the_synthetic_world_with_carve_votes_and_the_ground_mask(handle, gpu_mod):
    nf = 8
    sc = scenarios.small(n_frames=nf, az=200)
    m = np.ascontiguousarray(sc["map"], np.float32)
    T = np.stack(sc["T_b2o"][:nf])
    assert 20000 < len(m) < 60000
    kept_mask = evalmap.carve(m, sc["scans"][:nf], T, sc["T_l2b"], voxel=0.2, keep=False)[2]
    ground = evalmap.ground_votes(m, T, sc["T_l2b"])[1]
    votes = gpu_mod.votes_from_masks(kept_mask)
    want = check(handle, m, votes, ground, tol=0.3, remove_ratio=0.3, max_size=100, what="world")
    # a condition on the input, not a measurement: every decision but the revert occurs, and objects grow
    assert {S.UNCHANGED, S.REMOVED, S.NOT_OBJECT} <= set(want[1]["decision"].tolist()) and want[4]["n_grown"] > 0
    assert 0 < want[4]["n_ground"] < len(m) and want[4]["n_reverted"] == 0
    want = check(handle, m, votes, ground, tol=0.3, remove_ratio=0.3, revert_ratio=0.1, max_size=100, ground_keep=False, what="world, reverting")
    assert want[4]["n_ground_reverted"] == 0
    # the same from a device buffer
    p = handle.device_array(m)
    try:
        S.assert_same(handle.object_vote((p, len(m)), votes, ground, tol=0.3, remove_ratio=0.3, revert_ratio=0.1, max_size=100, ground_keep=False), want, "device cloud")
    finally:
        handle.device_free(p)
