"""The host text of the decision per object (evalmap.object_vote) against its tree-free restatement (object_vote_brute: a plain flood
fill) and against answers written out by hand: the designed scenes, 20 random clouds with random votes, ground and parameters, the
refusals, and the degenerate setting in which the call is evalmap.cluster plus the votes.  No GPU."""
import numpy as np
import pytest

import object_scenes as S
from erasor_amd import evalmap


def both(cloud, votes, ground=None, **prm):
    want = evalmap.object_vote_brute(cloud, votes, ground, **prm)
    S.assert_same(evalmap.object_vote(cloud, votes, ground, **prm), want, prm)
    return want


@pytest.mark.parametrize("ground_keep", [True, False])
def test_known_answer(ground_keep):
    cloud, votes, ground = S.known_scene()
    mask, rows, ids, kept, res = both(cloud, votes, ground, ground_keep=ground_keep, **S.KNOWN_PARAMS)
    w_mask, w_rows, w_res = S.known_answer(ground_keep)
    assert res == w_res
    assert mask.tobytes() == w_mask.tobytes() and rows.tobytes() == w_rows.tobytes()
    assert kept.tobytes() == cloud[w_mask != 0].tobytes()
    want_ids = np.full(len(cloud), evalmap.OBJECT_NONE, np.uint32)
    for r, (lo, hi) in enumerate([(256, 381), (381, 506), (506, 631), (631, 1531)]):
        want_ids[lo:hi] = r
    assert ids.tobytes() == want_ids.tobytes()


def test_without_the_ground_mask_the_known_scene_is_one_cluster():
    cloud, votes, _ = S.known_scene()
    mask, rows, ids, kept, res = both(cloud, votes, None, **S.KNOWN_PARAMS)
    assert len(rows) == 1 and rows["first"][0] == 0 and rows["n_points"][0] == 1531 and rows["n_voted"][0] == 733 and rows["decision"][0] == S.NOT_OBJECT
    assert res["n_clusters"] == 1 and res["n_ground"] == 0 and res["n_removed"] == 733 and res["n_grown"] == 0 and (ids == 0).all()
    assert mask.tobytes() == (votes == 0).astype(np.uint8).tobytes()


def test_ground_is_outside_the_graph():
    cloud, votes, ground = S.bridge_scene()
    a = both(cloud, votes, ground, tol=0.3)
    b = both(cloud, votes, None, tol=0.3)
    assert a[4]["n_clusters"] == 2 and a[0].tolist() == [0, 1, 1] and a[2].tolist() == [0, evalmap.OBJECT_NONE, evalmap.OBJECT_NONE]
    # (without the mask: one cluster of three with one vote, 1 >= 0.5 * 3 is false -> unchanged, only the voted point goes)
    assert b[4]["n_clusters"] == 1 and b[0].tolist() == [0, 1, 1] and b[2].tolist() == [0, 0, 0] and b[1]["decision"].tolist() == [S.UNCHANGED]
    # with it the voted point is a cluster of its own, all of it voted -> removed
    assert a[1]["decision"].tolist() == [S.REMOVED] and a[1]["first"].tolist() == [0]


@pytest.mark.parametrize("seed", range(20))
def test_random_clouds(seed):
    cloud, votes, ground, prm = S.random_case(seed)
    both(cloud, votes, ground, **prm)


def test_every_decision_occurs_in_the_random_clouds():
    seen = set()
    for seed in range(20):
        cloud, votes, ground, prm = S.random_case(seed)
        seen |= set(evalmap.object_vote(cloud, votes, ground, **prm)[1]["decision"].tolist())
    assert seen == {S.UNCHANGED, S.REMOVED, S.REVERTED, S.NOT_OBJECT}


def test_degenerate_setting_is_cluster_and_the_votes():
    """ground=None, remove_ratio=1, min_voted huge, revert_ratio=0: the mask is votes < vote_thr and the touched clusters are cluster's"""
    for seed in (1, 2, 3):
        cloud, votes, _, prm = S.random_case(seed)
        thr = prm["vote_thr"]
        mask, rows, ids, kept, res = both(cloud, votes, None, tol=prm["tol"], vote_thr=thr, remove_ratio=1.0, revert_ratio=0.0, min_voted=2 ** 40)
        assert mask.tobytes() == (votes < thr).astype(np.uint8).tobytes() and res["n_grown"] == 0 and res["n_reverted"] == 0
        c_rows, c_ids, _, c_res = evalmap.cluster(cloud, prm["tol"])
        assert res["n_clusters"] == c_res["n_clusters"] and res["largest"] == c_res["largest"]
        touched = np.isin(c_rows["first"], rows["first"])
        assert touched.sum() == len(rows) == len(np.unique(c_ids[votes >= thr]))
        for f in ("first", "n_points", "n_dynamic", "n_label_out_of_range", "min_xyz", "max_xyz"):
            assert rows[f].tobytes() == c_rows[f][touched].tobytes(), f
        assert (rows["decision"] == S.UNCHANGED).all()


def test_n_zero_and_all_ground():
    z = np.zeros((0, 4), np.float32)
    mask, rows, ids, kept, res = both(z, np.zeros(0, np.uint8), None, tol=0.5)
    assert len(mask) == len(rows) == len(ids) == len(kept) == 0 and res == dict.fromkeys(evalmap.OBJECT_RESULT_FIELDS, 0)
    cloud, votes, _ = S.bridge_scene()
    for keep in (True, False):
        got = both(cloud, votes, np.ones(3, np.uint8), tol=0.3, ground_keep=keep)
        assert got[4]["n_clusters"] == 0 and got[0].tolist() == ([1, 1, 1] if keep else [0, 1, 1]) and (got[2] == evalmap.OBJECT_NONE).all()


def test_refusals():
    cloud, votes, ground = S.bridge_scene()
    bad = [dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(remove_ratio=0.0), dict(remove_ratio=1.5),
           dict(remove_ratio=float("nan")), dict(revert_ratio=-0.1), dict(revert_ratio=1.0, remove_ratio=1.0), dict(revert_ratio=0.5), dict(revert_ratio=0.6),
           dict(revert_ratio=float("nan")), dict(vote_thr=0), dict(vote_thr=256), dict(max_extent=-1.0), dict(max_extent=float("inf")),
           dict(max_extent=float("nan"))]
    for fn in (evalmap.object_vote, evalmap.object_vote_brute):
        for kw in bad:
            with pytest.raises(ValueError):
                fn(cloud, votes, ground, **kw)
        with pytest.raises(ValueError):
            fn(cloud, votes[:2], ground)
        with pytest.raises(ValueError):
            fn(cloud, votes, ground[:2])
        for v in (np.nan, np.inf, -np.inf):
            c = cloud.copy()
            c[1, 2] = v  # (a ground point's coordinate: refused as any other)
            with pytest.raises(ValueError):
                fn(c, votes, ground)
