"""The per-bin launch (revert_bins.hip.h: k_revert_bins_srt, and its unfused twins k_rgpf2 / k_binvox2) at every SIZE CLASS of a reverted bin.

Which code runs for a reverted bin depends on point counts alone:
  M  = map points of the bin:        exact-sort leaves (16 / 64 keys) | lds_esort_sync_call2 (<= 2048) | lds_esort_sync_call4 (<= 4096, four keys
                                     per thread, the whole LDS pool) | rg_rare_call (> 4096: global scratch, block_esort, rgpf_after_sort)
  m  = cc + ng, the voxelised cloud: the same two sorts (beyond 2048 the cloud is staged a second time behind the sort) | bv_rare_call (> 4096);
                                     coordinates and ground list taken from LDS (in_lds = 1) or, behind a rare R-GPF, from global memory (in_lds = 0)
  ng = the ground list:              covariance product rows in chunks of 896 elements, double-buffered; a fit is skipped when two successive
                                     classifications agree
One reverted bin in a world of 1 ring x 4 sectors puts the kernel on any of these paths, and the oracle answers such a step in
milliseconds.  Every case here states the class it is meant to hit, asserts it ON THE ORACLE'S numbers (a case whose inputs miss their class
fails; nothing in this file is skipped), and then compares the HIP path with the oracle bit for bit (compare_step(full=True): every cloud,
index, count, status, and the plane of every R-GPF iteration).  No tolerances.
"""
import functools
import os

import numpy as np
import pytest

import test_oracle_known_answers as ka
from test_gpu_parity import I4, compare_step, gpu_mod, make_pair, same  # noqa: F401  (gpu_mod: the module's fixture)

pytestmark = pytest.mark.gpu

ESYNC_MAX, PB_CAP, RG2_CH = 2048, 4096, 896  # (kernels.hip.h / revert_bins.hip.h)
EDGE = 0.05                                  # [rad] every point keeps this distance from a sector edge: n_ambiguous stays 0
KINDS_CONVERGING = ("plane", "ties", "canopy")  # the second classification repeats the first: the third fit is skipped
LABELS = np.array([40.0, 44.0, 48.0, 50.0, 70.0, 71.0, 252.0, 259.0], np.float32)


# ---------------------------------------------------------------------------------------------
# 1. inputs: one bin's map points and scan points, deterministic, in a chosen sector
# ---------------------------------------------------------------------------------------------
def median_of_3_killer(n):
    """the adversary sequence of test_exact_sort_heapsort_fallback_on_median_of_3_killer (n even)"""
    a = np.zeros(n, np.uint32)
    k = n // 2
    for i in range(1, k + 1):
        if i & 1:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


@functools.lru_cache(maxsize=None)
def _lattice(pitch, jitter, seed):
    """jittered lattice points of the first quadrant inside the bin (0.3 <= r <= 9.8, EDGE + 0.01 away from both axes), in a seeded random
    order: the first M of them are a bin of M points, and the bins of different M are nested"""
    rng = np.random.default_rng(seed)
    n = int(10.0 / pitch) + 1
    gx, gy = np.meshgrid(np.arange(n) * pitch + 0.5 * pitch, np.arange(n) * pitch + 0.5 * pitch, indexing="ij")
    xy = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-jitter, jitter, (n * n, 2))
    xy = xy.astype(np.float32).astype(np.float64)
    r, th = np.hypot(xy[:, 0], xy[:, 1]), np.arctan2(xy[:, 1], xy[:, 0])
    xy = xy[(r >= 0.3) & (r <= 9.8) & (th >= EDGE + 0.01) & (th <= np.pi / 2 - EDGE - 0.01)]
    return xy[rng.permutation(len(xy))]


@functools.lru_cache(maxsize=None)
def _map_candidates(kind, seed, order="shuffled"):
    """(x, y, z, label) of every lattice point for a map kind; point i's height does not depend on how many points the bin takes.
    order "shuffled": a bin of any size covers the whole quadrant; "radial": the innermost points first, a bin is as dense as the lattice"""
    xy = _lattice(0.07, 0.01, 1000 + seed)
    if order == "radial":
        xy = xy[np.argsort(np.hypot(xy[:, 0], xy[:, 1]), kind="stable")]
    rng = np.random.default_rng(2000 + seed)
    n = len(xy)
    r = np.hypot(xy[:, 0], xy[:, 1])
    raised = np.linspace(0.3, 1.2, 8)  # the bin is taller than 0.5 m: the v3 gate (erasor.cpp:511) lets R-GPF run
    if kind in ("plane", "ties"):
        z = 0.03 * r + rng.normal(0, 0.02, n)
        z[:8] = raised
        if kind == "ties":
            z = np.round(z * 16) / 16  # many equal heights: the introsort's tie order decides the order of the float32 sums
    elif kind == "bowl":
        z = 0.012 * (r - 5.0) ** 2 + rng.normal(0, 0.08, n)  # the classification keeps changing: no fit is skipped
        z[:8] = raised
    elif kind == "canopy":
        z = rng.uniform(0.6, 1.4, n)  # large M, small ng
        low = np.arange(n) % 8 == 0
        z[low] = 0.01 * r[low] + rng.normal(0, 0.02, n)[low]
    else:
        raise ValueError(kind)
    lab = LABELS[rng.integers(0, len(LABELS), n)]
    return np.column_stack([xy, z, lab]).astype(np.float32)


def rotate(pts, sector):
    """a 90 degree turn per sector: (x, y) -> (-y, x), exact in float32"""
    pts = pts.copy()
    for _ in range(sector % 4):
        pts[:, 0], pts[:, 1] = -pts[:, 1].copy(), pts[:, 0].copy()
    return pts


def map_bin(kind, M, sector=0, seed=0, order="shuffled"):
    if kind == "killer":  # heights follow the adversary sequence IN INPUT ORDER (a one-bin map keeps its order through the stable bucketing)
        pts = _map_candidates("plane", seed, order)[:M].copy()
        pts[:, 2] = (median_of_3_killer(M).astype(np.float64) * (1.2 / M)).astype(np.float32)
    else:
        pts = _map_candidates(kind, seed, order)[:M].copy()
    assert len(pts) == M, "the lattice is too small for %d points" % M
    return rotate(pts, sector)


def scan_bin(cc, sector=0, seed=0):
    """cc flat points (z = 0): the Scan Ratio Test sees zero height on the scan side, every bin with a map taller than 0.5 m reverts"""
    xy = _lattice(0.1, 0.0, 3000 + seed)[:cc]
    assert len(xy) == cc, "the lattice is too small for %d scan points" % cc
    lab = LABELS[np.random.default_rng(4000 + seed).integers(0, len(LABELS), cc)]
    return rotate(np.column_stack([xy, np.zeros(cc), lab]).astype(np.float32), sector)


# ---------------------------------------------------------------------------------------------
# handles: one per parameter variant, reused across cases with set_map
# ---------------------------------------------------------------------------------------------
_pairs = {}


def pair(gpu_mod, profiled=False, **kw):
    key = (profiled,) + tuple(sorted(kw.items()))
    if key not in _pairs:
        g, o = make_pair(gpu_mod, ka.one_bin_params(**kw))
        if profiled:
            g.profiling(1)  # every launch on its own: R-GPF and the per-bin voxelisation apart (k_rgpf2, k_binvox2)
        _pairs[key] = (g, o)
    return _pairs[key]


@functools.lru_cache(maxsize=None)
def _oracle(**kw):
    from oracle import orc
    return orc.Oracle(ka.one_bin_params(**kw))


def oracle_ng(kind, M, seed=0, **kw):
    """the ground count R-GPF leaves for a bin (it does not depend on the scan)"""
    o = _oracle(**kw)
    o.set_map(map_bin(kind, M, seed=seed))
    r = o.step(scan_bin(40), I4, I4, I4)
    assert r.n_reverted_bins == 1
    return int(r.n_ground)


@functools.lru_cache(maxsize=None)
def find_bin_for_ng(kind, target):
    """(M, seed) of a bin whose ground list has exactly `target` elements, searched on the oracle.  The bins of one seed are nested, so ng
    grows with M almost monotonically: a bisection to where it crosses the target, then the neighbourhood; a count that this seed's bins
    step over is looked for in the next seed's"""
    for seed in range(8):
        lo, hi = 16, 9000
        while hi - lo > 1:  # (ng(lo) < target <= ng(hi), up to the few places where ng steps back)
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if oracle_ng(kind, mid, seed) >= target else (mid, hi)
        for M in range(max(16, hi - 12), hi + 13):
            if oracle_ng(kind, M, seed) == target:
                return M, seed
    raise AssertionError("no %s bin with a ground list of %d elements" % (kind, target))


# ---------------------------------------------------------------------------------------------
# what a case is, asserted on the oracle
# ---------------------------------------------------------------------------------------------
def size_class(n):
    return 0 if n <= ESYNC_MAX else (1 if n <= PB_CAP else 2)


def bin_facts(o, ro, sector):
    """(M, cc) of a sector's bin from the oracle's R-POD (1 ring: the bin index is the sector)"""
    return int(o.get_bins(0)[0][sector]), int(o.get_bins(1)[0][sector])


def distinct_planes(o, k=0):
    _, n, d = o.get_planes()
    return len({(n[k, i].tobytes(), d[k, i].tobytes()) for i in range(n.shape[1])})


def assert_clean(ro, n_rev):
    assert ro.n_reverted_bins == n_rev, ro.as_dict()
    assert ro.n_ambiguous == 0 and ro.n_voxel_overflow == 0 and ro.n_degenerate_plane == 0, ro.as_dict()


def fits_intended(kind, M):
    """distinct planes among the gf_iter = 3 iterations = 1 + the iterations that really fit: the seeds' plane, the plane of the first
    classification, and a third only where the second classification differs from the first (otherwise the fit is skipped).  plane, ties
    and canopy bins converge after one iteration; bowl and killer bins keep changing -- once they have points enough for it: a bowl of
    the exact-sort leaves' sizes (16 to 65 points, eight of them raised) has converged by then as well"""
    return 2 if kind in KINDS_CONVERGING or M <= 65 else 3


def assert_one_bin_case(o, ro, kind, M, cc, sector=0, m_class=None, ng=None):
    """the oracle's own numbers say that this step is the case it claims to be"""
    assert_clean(ro, 1)
    assert bin_facts(o, ro, sector) == (M, cc), (bin_facts(o, ro, sector), M, cc)
    if ng is not None:
        assert ro.n_ground == ng, (ro.n_ground, ng)
    if m_class is not None:
        assert size_class(cc + int(ro.n_ground)) == m_class, (cc, ro.n_ground, m_class)
    assert distinct_planes(o) == fits_intended(kind, M), (kind, M, o.get_planes()[1:])


def run_one_bin(gpu_mod, kind, M, cc, sector=0, m_class=None, ng=None, seed=0, order="shuffled", **kw):
    g, o = pair(gpu_mod, **kw)
    mp, sc = map_bin(kind, M, sector, seed, order), scan_bin(cc, sector)
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(sc, I4, I4, I4)
    assert_one_bin_case(o, ro, kind, M, cc, sector, m_class, ng)
    rg = g.step(sc, I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)
    return rg, ro


def sid(M):
    """ids of the cases the CPU stand-in runs too (tests/test_full_step_on_cpu.py selects `standin`): M <= 4097"""
    return "standin" if M <= PB_CAP + 1 else "device"


# ---------------------------------------------------------------------------------------------
# 2. one bin at every class
# ---------------------------------------------------------------------------------------------
M_SWEEP = (16, 17, 64, 65, 1023, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 9000)


@pytest.mark.parametrize("kind,M", [pytest.param(k, M, id="%s-%d-%s" % (k, M, sid(M))) for k in ("plane", "ties", "bowl") for M in M_SWEEP])
def test_map_points_around_every_sort_class(gpu_mod, kind, M):
    """M across the exact-sort leaves (16, 64), the two LDS sorts (2048, 4096) and into the global-scratch path; cc = 40, so the voxelised
    cloud follows M through its own classes a few dozen points ahead (and with in_lds = 0 behind the rare R-GPF)"""
    # plane and ties bins leave all but their raised points on the ground (m ~ M + 32: it crosses 2048 and 4096 before M does); a bowl
    # leaves about seven eighths (m stays a class behind from 2047 on)
    m_class = size_class(M + 32) if kind != "bowl" else size_class(M * 7 // 8 + 40)
    run_one_bin(gpu_mod, kind, M, 40, sector=M % 4, m_class=m_class)


@pytest.mark.parametrize("M,cc,m_class", [pytest.param(M, cc, c, id="%d-%d-standin" % (M, cc)) for M, cc, c in (
    (1200, 840, 0), (1200, 860, 1), (1200, 900, 1), (2048, 2030, 1), (2048, 2100, 2), (3000, 3000, 2))])
def test_voxelised_cloud_straddles_its_classes_while_the_bin_stays_in_lds(gpu_mod, M, cc, m_class):
    """R-GPF in LDS (in_lds = 1), m = cc + ng on either side of 2048 and 4096 (a plane bin of 1200 points leaves 1194 on the ground:
    860 scan points already make 2054, so 840 stand for the side below)"""
    run_one_bin(gpu_mod, "plane", M, cc, m_class=m_class)


@pytest.mark.parametrize("M,m", [pytest.param(M, m, id="%d-m%d-standin" % (M, m)) for M, m in ((1200, 2047), (1200, 2048), (1200, 2049), (2048, 4095),
                                                                                                  (2048, 4096), (2048, 4097))])
def test_voxelised_cloud_exactly_at_the_class_borders(gpu_mod, M, m):
    """cc chosen from the oracle's ground count so that m = cc + ng lands ON the border, one below and one above"""
    ng = oracle_ng("plane", M)
    rg, ro = run_one_bin(gpu_mod, "plane", M, m - ng, ng=ng, m_class=size_class(m))
    assert (m - ng) + ro.n_ground == m


@pytest.mark.parametrize("M,cc,m_class", [pytest.param(4097, 40, 0, id="4097-40-standin"), pytest.param(9000, 40, 0, id="9000-40-device"),
                                          pytest.param(4000, 3700, 2, id="4000-3700-standin")])
def test_canopy_bins_put_the_two_stages_in_different_classes(gpu_mod, M, cc, m_class):
    """a sparse ground under a canopy (ng ~ M / 8): M > 4096 with a small cloud -- R-GPF on the rare path, the voxelisation in LDS fetching
    from global memory (in_lds = 0); M = 4000 with 3700 scan points -- R-GPF in LDS, the voxelisation on the rare path"""
    run_one_bin(gpu_mod, "canopy", M, cc, m_class=m_class)


@pytest.mark.parametrize("kind,ng", [pytest.param(k, n, id="%s-ng%d-standin" % (k, n)) for k in ("plane", "bowl")
                                     for n in (RG2_CH - 1, RG2_CH, RG2_CH + 1, 2 * RG2_CH, 2 * RG2_CH + 1, 3 * RG2_CH + 1)])
def test_ground_list_lengths_around_the_product_row_chunks(gpu_mod, kind, ng):
    """ng on both sides of 896, 1792 and 2688: one, two, three and four sets of covariance product rows, the last of them one element long;
    plane: the third fit is skipped, bowl: every iteration fits (lists of other lengths in between)"""
    M, seed = find_bin_for_ng(kind, ng)
    assert M <= PB_CAP, "the chunks under test are those of the LDS-resident fit"
    run_one_bin(gpu_mod, kind, M, 40, ng=ng, seed=seed)


@pytest.mark.parametrize("kind,M", [pytest.param(k, M, id="%s-%d-standin" % (k, M)) for k in ("plane", "ties", "bowl") for M in (2049, 4096, 4097)])
def test_many_points_per_voxel_at_the_upper_classes(gpu_mod, kind, M):
    """map_voxel_size = 0.2: several points share a voxel (the bin takes the lattice's innermost points, 0.07 m apart), so ties in the second exact sort decide the order of the centroid sums"""
    g, o = pair(gpu_mod, map_voxel_size=0.2)
    rg, ro = run_one_bin(gpu_mod, kind, M, 40, sector=1, order="radial", map_voxel_size=0.2)
    cloud = np.concatenate([scan_bin(40, 1), o.get_cloud(6)])[:, :3]  # (curr + reverted ground: what the bin voxelises)
    n_vox = len(np.unique(np.floor(cloud.astype(np.float64) / 0.2).astype(np.int64), axis=0))
    assert len(cloud) == 40 + ro.n_ground and n_vox < len(cloud) / 3, "voxels were meant to hold several points each"


# ---------------------------------------------------------------------------------------------
# 3. the heapsort fallback inside the per-bin sort
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [pytest.param(M, id="%d-%s" % (M, sid(M))) for M in (1000, 2048, 4096, 6000)])
def test_depth_budget_runs_out_inside_the_per_bin_sort(gpu_mod, M):
    """heights in the order of the median-of-3 adversary: the introsort's depth budget runs out in lds_esort_sync (two keys per thread:
    1000, 2048; four: 4096) and in the rare path's block_esort (6000).  The oracle calls the real std::sort and counts nothing, so the
    device's own counter is the evidence that the fallback ran -- and parity that it ran right."""
    rg, ro = run_one_bin(gpu_mod, "killer", M, 40, sector=2)
    assert rg.n_sort_fallback > 0, "depth limit was never hit: the fallback is not exercised"


# ---------------------------------------------------------------------------------------------
# 4. several classes in one launch
# ---------------------------------------------------------------------------------------------
MIXED = (("ties", 300, 40), ("bowl", 3000, 1500), ("plane", 5000, 200), ("canopy", 9000, 2500))  # (kind, M, cc) of sectors 0..3


@functools.lru_cache(maxsize=None)
def mixed_clouds():
    rng = np.random.default_rng(77)
    mp = np.concatenate([map_bin(k, M, s, seed=s) for s, (k, M, _) in enumerate(MIXED)])
    sc = np.concatenate([scan_bin(cc, s, seed=s) for s, (_, _, cc) in enumerate(MIXED)])
    return mp[rng.permutation(len(mp))], sc[rng.permutation(len(sc))]  # (shuffled: the bucketing sorts the bins out)


def sector_of(pts):
    return (np.floor(np.arctan2(pts[:, 1], pts[:, 0]) % (2 * np.pi) / (np.pi / 2))).astype(int)


def assert_mixed_case(o, ro, per_bin_ng=True):
    assert_clean(ro, len(MIXED))
    bins, n, d = o.get_planes()
    ng = np.bincount(sector_of(o.get_cloud(6)), minlength=4) if per_bin_ng else None
    for s, (kind, M, cc) in enumerate(MIXED):
        assert bin_facts(o, ro, s) == (M, cc)
        k = int(np.flatnonzero(bins == s)[0])
        assert distinct_planes(o, k) == fits_intended(kind, M), (s, kind)
    if per_bin_ng:
        assert int(ng.sum()) == ro.n_ground
        # R-GPF: LDS, LDS, rare, rare; the voxelisation: all three classes, the last two with in_lds = 0
        assert [size_class(M) for _, M, _ in MIXED] == [0, 1, 2, 2]
        assert [size_class(cc + int(ng[s])) for s, (_, _, cc) in enumerate(MIXED)] == [0, 2, 2, 1], ng.tolist()


def test_four_bins_of_different_classes_in_one_launch(gpu_mod):
    """four workgroups, all reverted: two on the rare R-GPF path, two in LDS, voxelisations of all three classes -- the rare ones share the
    global scratch through moff / qoff and vox_base / h_base"""
    g, o = pair(gpu_mod)
    mp, sc = mixed_clouds()
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(sc, I4, I4, I4)
    assert_mixed_case(o, ro)
    compare_step(g, o, g.step(sc, I4, I4, I4), ro, full=True)


# ---------------------------------------------------------------------------------------------
# 5. the same bins through every launch variant
# ---------------------------------------------------------------------------------------------
VARIANT_CASES = [pytest.param(("plane", 2049, 40), id="2049-standin"), pytest.param(("plane", 4097, 40), id="4097-standin"),
                 pytest.param(("plane", 3000, 3000), id="3000-3000-standin"), pytest.param("mixed", id="mixed-device")]


def variant_clouds(case):
    if case == "mixed":
        return mixed_clouds()
    kind, M, cc = case
    return map_bin(kind, M, 3), scan_bin(cc, 3)


def assert_variant_case(o, ro, case):
    if case == "mixed":
        assert_mixed_case(o, ro, per_bin_ng=False)
    else:
        kind, M, cc = case
        assert_one_bin_case(o, ro, kind, M, cc, 3, m_class=size_class(cc + M - 8))


def two_sites(gpu_mod, case):
    """the case's bins at the origin and again 40 m down the x axis (max range 10 m: the second site starts in the outskirts), the poses of
    the two steps, the scan (the same at both poses)"""
    mp, sc = variant_clouds(case)
    far = mp.copy()
    far[:, 0] += np.float32(40.0)
    T2 = gpu_mod.geopose2eigen([40.0, 0, 0, 0, 0, 0, 1])
    return np.concatenate([mp, far]), sc, [(I4, I4), (T2, gpu_mod.invert_rigid(T2))]


def run_two_sites(g, o, case, mp, sc, poses, check=compare_step):
    g.set_map(mp)
    o.set_map(mp)
    l0, u0 = g.overlap_counts()
    # both nodes announced with both transforms before the first step: the second step's front runs beside the first step's per-bin launch
    for Tb, To in poses:
        g.prefetch(sc, I4, Tb, To)
    for k, (Tb, To) in enumerate(poses):
        ro = o.step(sc, I4, Tb, To)
        assert_variant_case(o, ro, case)
        assert ro.n_voi == len(mp) // 2  # (the other site lies in the outskirts)
        rg = g.step(sc, I4, Tb, To)
        check(g, o, rg, ro)
        same(g.get_map(), o.get_map(), "map after step %d" % k)
    l1, u1 = g.overlap_counts()
    return l1 - l0, u1 - u0


@pytest.mark.parametrize("case", VARIANT_CASES)
def test_two_announced_steps_carry_bins_of_these_sizes(gpu_mod, case):
    """plain and overlapped steps: where the suite forces the overlap (conftest.py) the second step's front is launched beside the first
    step's per-bin launch, so the reserved layout (mc + cc places per reverted bin, holes) and the late write-back carry bins of these
    sizes.  Twice over: a handle that has to grow its scratch between the two steps drops the passes launched ahead and runs the step's
    own (the plain order, checked like the other); the second time round nothing grows and the passes are taken."""
    g, o = pair(gpu_mod)
    clouds = two_sites(gpu_mod, case)
    run_two_sites(g, o, case, *clouds)
    launched, taken = run_two_sites(g, o, case, *clouds)
    if os.environ.get("ERASOR_HIP_OVERLAP") == "1":
        assert (launched, taken) == (1, 1), (launched, taken)


@pytest.mark.parametrize("case", VARIANT_CASES)
def test_unfused_launches_at_these_sizes(gpu_mod, case):
    """erasor_hip_profiling(1): k_rgpf2 and k_binvox2 instead of the fused per-bin launch"""
    g, o = pair(gpu_mod, profiled=True)
    mp, sc = variant_clouds(case)
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(sc, I4, I4, I4)
    assert_variant_case(o, ro, case)
    compare_step(g, o, g.step(sc, I4, I4, I4), ro, full=True)


@pytest.mark.parametrize("case", VARIANT_CASES)
def test_v2_reverts_bins_of_these_sizes(gpu_mod, case):
    """v2 (erasor.cpp:383): the bin is reverted where its map is taller than th_bin_max_h -- 0.75 m, below every kind's highest point"""
    g, o = pair(gpu_mod, version=2, th_bin_max_h=0.75)
    mp, sc = variant_clouds(case)
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(sc, I4, I4, I4)
    assert_variant_case(o, ro, case)
    compare_step(g, o, g.step(sc, I4, I4, I4), ro, full=True)


NO_OVERLAP_WORKER = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import os
import erasor_amd
if os.environ.get("ERASOR_TEST_SIMT_LIB"):  # (the CPU stand-in build, when the suite itself runs on it)
    erasor_amd.LIB_PATH = os.environ["ERASOR_TEST_SIMT_LIB"]
    erasor_amd._lib = None
import test_gpu_bin_sizes as B
assert os.environ["ERASOR_HIP_OVERLAP"] == "0"
g, o = B.pair(erasor_amd)
launched, taken = B.run_two_sites(g, o, "mixed", *B.two_sites(erasor_amd, "mixed"))
assert taken == 0, (launched, taken)
print("NO-OVERLAP-OK")
"""


def test_mixed_bins_in_a_process_that_never_overlaps(gpu_mod, tmp_path):
    """ERASOR_HIP_OVERLAP=0 is read once, so in a process of its own: the dense layout of the VoI-resident region with bins of these sizes"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "no_overlap_worker.py"
    script.write_text(NO_OVERLAP_WORKER % (root, root))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=280, env=dict(os.environ, ERASOR_HIP_OVERLAP="0"))
    assert out.returncode == 0 and "NO-OVERLAP-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
