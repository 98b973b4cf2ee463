"""The voxelisation chain (voxelize_preserving_labels: k_bbox, k_voxel_keys_es, the device-wide exact std::sort, run detection, k_centroids,
k_query_nn; k_xyz_hash_keys / k_dup_label_passthrough for a cloud VoxelGrid refuses) on every route of its sort and of its label search.

Three judges, every comparison bit for bit:
  * the device (the hooks build: the sort on its own through hooks.exact_sort_u32, its queues through hooks.debug_sort_queues);
  * the oracle (orc.voxelize_preserving_labels, orc.std_sort_u32) -- whose 1-NN is the same shell search as the device's;
  * model() below: float32 arithmetic as PCL's, the real std::sort for the order inside a voxel, and a BRUTE-FORCE nearest neighbour
    over all input points -- no grid, no shells, nothing shared with either.  Used wherever points x voxels allows it.

Clouds are built from key sequences (key_cloud): the voxel keys of the cloud ARE the sequence, so every input pattern of the sort alone
is also an input of the whole chain; the output depends on the sort's tie order through the rounding of the float32 centroid sums, and
every such case asserts that itself (the model with a stable order must differ from the model proper).

census(): how many segments each stage of the sort took, derived from the queues the sort leaves behind.  The census is a function of
the input; the cases of ROUTES assert it exactly (figures: MEASUREMENTS.md, "Routes of the exact sort").

Ids end in `standin` (at most ~8200 points: also run on the CPU stand-in, tests/test_full_step_on_cpu.py) or `device`."""
import copy

import numpy as np
import pytest

import hooks
import scenarios
from test_gpu_parity import compare_step, make_pair, same

pytestmark = pytest.mark.gpu

F = np.float32
ES_LMAX, ES_MID_LMAX, WTILE, WTILES_MAX, WSEG_MAX = 2048, 8192, 2048, 8192, 1024  # (kernels.hip.h)
N_LAST_WIDE = WTILES_MAX * WTILE + 1  # the largest n that takes the wide levels; one more takes the level queue


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()
    with hooks.hooks_library():
        yield erasor_amd


@pytest.fixture(scope="module")
def g(gpu_mod):
    # (closed HERE, while the hooks build is still the loaded library: the two builds' handles differ in layout, and a handle must be
    # destroyed by the build that made it)
    h = gpu_mod.Erasor(gpu_mod.params_default())
    yield h
    h.close()


def tag(n):
    return "standin" if n <= 8200 else "device"


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
MODEL_MAX = 1 << 28  # points x voxels up to which the brute-force label search is affordable (a second or two)


def model(cloud, leaf, stable=False, nn=True):
    """voxelize_preserving_labels restated: float32 throughout, std::sort's order inside a voxel (stable: a stable sort's instead),
    sequential float32 centroid sums, brute-force L2_Simple nearest neighbour with the lowest index on ties.
    nn=False: the centroids only (labels 0).  Returns (rows, info); info: keys, the runs' (begin, end) in sorted order, order, passthrough, n_tied (points at the minimum per voxel)"""
    from oracle import orc
    pts = np.ascontiguousarray(cloud, F).reshape(-1, 4)
    n = len(pts)
    if n == 0:
        return np.zeros((0, 4), F), {"passthrough": False}
    xyz = pts[:, :3]
    inv = F(1) / F(leaf)
    mn, mx = xyz.min(0), xyz.max(0)
    ext = ((mx - mn) * inv).astype(np.int64) + 1  # VoxelGrid's own check: (dx * dy * dz) > INT_MAX, from the float32 extent
    if int(ext[0]) * int(ext[1]) * int(ext[2]) > 2 ** 31 - 1:
        # the cloud comes back as it is; the label search finds every point itself or, at distance 0, its first duplicate (-0.0 == 0.0)
        canon = np.ascontiguousarray(xyz + F(0))
        _, first, inverse = np.unique(canon.view(np.dtype((np.void, 12))).ravel(), return_index=True, return_inverse=True)
        out = pts.copy()
        out[:, 3] = pts[first[inverse.ravel()], 3]
        return out, {"passthrough": True}
    min_b = np.floor(mn * inv).astype(np.int64)
    div_b = np.floor(mx * inv).astype(np.int64) - min_b + 1
    ijk = (np.floor(xyz * inv) - min_b.astype(F)).astype(np.int64)
    keys = (ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]).astype(np.uint32)
    idx = np.arange(n, dtype=np.uint32)
    if stable:
        order = np.argsort(keys, kind="stable")
        skeys = keys[order]
    else:
        skeys, order = orc.std_sort_u32(keys, idx)
    heads = np.flatnonzero(np.concatenate([[True], skeys[1:] != skeys[:-1]]))
    ends = np.concatenate([heads[1:], [n]])
    cent, zero = np.zeros((len(heads), 3), F), np.zeros((1, 3), F)
    for v, (s, e) in enumerate(zip(heads, ends)):
        # (the sums start at +0.0, as CentroidPoint's do: a voxel of -0.0 coordinates has the centroid +0.0)
        cent[v] = np.add.accumulate(np.concatenate([zero, xyz[order[s:e]]]), axis=0, dtype=F)[-1] / F(e - s)
    label = np.zeros(len(heads), F)
    n_tied = np.zeros(len(heads), np.int64)
    step = max(1, (1 << 22) // n)
    for v0 in range(0, len(heads) if nn else 0, step):
        c = cent[v0:v0 + step]
        d = c[:, None, 0] - xyz[None, :, 0]
        r = d * d
        d = c[:, None, 1] - xyz[None, :, 1]
        r = r + d * d
        d = c[:, None, 2] - xyz[None, :, 2]
        r = r + d * d
        assert r.dtype == F
        near = np.argmin(r, axis=1)  # (the first minimum: the lowest index)
        label[v0:v0 + step] = pts[near, 3]
        n_tied[v0:v0 + step] = (r == r[np.arange(len(c)), near][:, None]).sum(1)
    rows = np.column_stack([cent, label]).astype(F)
    return rows, {"passthrough": False, "keys": keys, "runs": (heads, ends), "order": order, "n_tied": n_tied, "min_b": min_b, "div_b": div_b,
                  "inv": inv, "ukeys": skeys[heads]}


def judge(g, cloud, leaf, what, use_model=True):
    """device against oracle and (where it is affordable) the model: all bit for bit.  Returns the model's (rows, info) or None"""
    from oracle import orc
    cloud = np.ascontiguousarray(cloud, F)
    got = g.voxelize_preserving_labels(cloud, leaf)
    want = orc.voxelize_preserving_labels(cloud, leaf)
    same(got, want, what + ": device against oracle")
    if not use_model:
        return None
    rows, info = model(cloud, leaf)
    same(want, rows, what + ": oracle against model")
    same(got, rows, what + ": device against model")
    return rows, info


# ---------------------------------------------------------------------------------------------
# key sequences and the clouds made of them
# ---------------------------------------------------------------------------------------------
def adversary(n):
    """the median-of-3 adversary (Musser): quadratic for a median-of-3 quicksort, so introsort's depth budget runs out"""
    a = np.zeros(n, np.uint32)
    k = n // 2
    for i in range(1, k + 1):
        if i & 1:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


def key_pattern(pattern, n):
    rng = np.random.default_rng(1000 + n)
    i = np.arange(n, dtype=np.int64)
    if pattern == "equal":
        k = np.full(n, 7)
    elif pattern == "two":
        k = rng.integers(0, 2, n)
    elif pattern == "v37":
        k = rng.integers(0, 37, n)
    elif pattern == "asc29":
        k = i % 29
    elif pattern == "desc29":
        k = 28 - i % 29
    elif pattern == "organ":
        k = np.minimum(i, n - 1 - i)
    elif pattern == "organ4":  # (an organ pipe of eight keys per value: in the plain one a value's TWO keys sum to the same centroid in either order)
        k = np.minimum(i, n - 1 - i) // 4
    elif pattern == "distinct_asc":
        k = i
    elif pattern == "distinct_desc":
        k = n - 1 - i
    elif pattern == "adversary":
        k = adversary(n)
    elif pattern == "adversary8":
        k = adversary(n) // 8
    elif pattern == "uniform32":
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        k[: min(n, 2)] = [0, 0xFFFFFFFF][: min(n, 2)]
    else:
        raise KeyError(pattern)
    return np.asarray(k).astype(np.uint32)


PATTERNS = ("equal", "two", "v37", "asc29", "desc29", "organ", "organ4", "distinct_asc", "distinct_desc", "adversary", "adversary8", "uniform32")
# the patterns with ties whose tie order shows in the centroids (the plain organ pipe's does not: organ4 stands in for it)
TIED = ("equal", "two", "v37", "asc29", "desc29", "organ4", "adversary8")
SIZES = (0, 1, 16, 17, 64, 65, 2047, 2048, 2049, 2050, 4096, 4097, 4098, 8192, 8193, 8194, 16383, 16384, 16385, 65537)


def key_cloud(keys, leaf=0.5, seed=0):
    """a cloud whose voxel keys are `keys` (up to their minimum): point i at x = (key_i + u) * leaf, u in [0.2, 0.8]; y, z scattered the
    same way inside one cell; random labels"""
    keys = np.asarray(keys, np.uint32)
    rng = np.random.default_rng(seed + len(keys))
    u = rng.uniform(0.2, 0.8, (len(keys), 3))
    u[:, 0] += keys
    return np.column_stack([u * leaf, rng.integers(1, 250, len(keys))]).astype(F)


def census(st):
    """segments per stage of the exact sort, from what hooks.debug_sort_queues read back.  mid_*: segments k_esort_mid partitioned (in LDS:
    <= 8192 keys, in global memory: longer); refused: segments of wide size that went to queue 0 before the last wide level (no slot or
    no tiles left in the next wide list); fin_*: segments k_esort_final took (in LDS: <= 2048 keys; global: longer); exhausted: segments
    of more than 16 keys that arrived there with no depth budget left (heapsort), exhausted_long: those of them longer than 2048"""
    n = st["n"]
    small = st["small"]
    ln = lambda r: r[:, 1] - r[:, 0]
    c = {"wide_levels": st["wide_levels"], "level_launches": st["level_launches"], "mid_run": st["mid_run"], "final_grid": st["final_grid"],
         "mid_lds": 0, "mid_global": 0, "refused": 0}
    rest = np.zeros((0, 3), np.int64)
    if st["mid_run"]:
        q0 = st["q0"]
        part = (q0[:, 2] > 0) & (ln(q0) > ES_LMAX)
        c["mid_lds"] = int((part & (ln(q0) <= ES_MID_LMAX)).sum())
        c["mid_global"] = int((part & (ln(q0) > ES_MID_LMAX)).sum())
        depth0 = 2 * (int(n).bit_length() - 1)
        c["refused"] = int((q0[:, 2] > depth0 - st["wide_levels"]).sum())
    else:
        rest = st["q%d" % (st["level_launches"] % 3)]  # (what the levels left long: the finisher's global path)
    fin = np.concatenate([small, rest])
    c["fin_lds"] = int((ln(fin) <= ES_LMAX).sum())
    c["fin_global"] = int((ln(fin) > ES_LMAX).sum())
    c["exhausted"] = int(((fin[:, 2] == 0) & (ln(fin) > 16)).sum())
    c["exhausted_long"] = int(((fin[:, 2] == 0) & (ln(fin) > ES_LMAX)).sum())
    # whatever the route, the finisher's segments are a partition of [0, n)
    if n:
        f = fin[np.argsort(fin[:, 0], kind="stable")]
        assert f[0, 0] == 0 and f[-1, 1] == n and (f[1:, 0] == f[:-1, 1]).all() and (ln(f) > 0).all(), "the finisher's segments do not tile [0, n)"
    else:
        assert len(fin) == 0
    return c


def route_invariants(n, c):
    """what follows from n alone (run_exact_sort)"""
    wide = ES_LMAX < n <= N_LAST_WIDE
    assert (c["wide_levels"] > 0) == wide and c["mid_run"] == int(wide), (n, c)
    if wide:
        assert c["wide_levels"] == min((n // (ES_LMAX + 1)).bit_length() - 1 + 4, 16) and c["level_launches"] == 0, (n, c)
    assert c["level_launches"] == (12 if n > N_LAST_WIDE else 0), (n, c)
    assert c["final_grid"] == (128 if n <= 1 << 20 else 2048), (n, c)
    if n <= ES_LMAX:
        assert c["fin_lds"] == (1 if n else 0) and c["fin_global"] == 0, (n, c)


# The routes, proven taken: the exact census of one case per route.  Measured once (the CPU stand-in and the device agree: the census
# is a function of the input as long as the wide list refuses nothing for want of a slot, see the 12 M-key case), asserted exactly since.
ROUTES = {
    # below WIDE_MIN: straight to the LDS finisher
    'equal-2048-standin': dict(wide_levels=0, level_launches=0, mid_run=0, final_grid=128, mid_lds=0, mid_global=0, refused=0, fin_lds=1, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # the first wide size: one tile
    'v37-2049-standin': dict(wide_levels=4, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=0, refused=0, fin_lds=2, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # two tiles
    'v37-2050-standin': dict(wide_levels=4, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=0, refused=0, fin_lds=2, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # two tiles, the last size of four wide levels
    'uniform32-4097-standin': dict(wide_levels=4, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=0, refused=0, fin_lds=4, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # three tiles, five wide levels
    'uniform32-4098-standin': dict(wide_levels=5, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=0, refused=0, fin_lds=4, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # k_esort_mid in LDS
    'organ-4096-standin': dict(wide_levels=4, level_launches=0, mid_run=1, final_grid=128, mid_lds=1, mid_global=0, refused=0, fin_lds=11, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=16),
    # the finisher's global path: a segment of more than 2048 keys without depth budget (heapsort in place)
    'adversary-4097-standin': dict(wide_levels=4, level_launches=0, mid_run=1, final_grid=128, mid_lds=1, mid_global=0, refused=0, fin_lds=24, fin_global=1, exhausted=1, exhausted_long=1, n_fallback=1),
    # mid in LDS, then the finisher's global path
    'organ-8193-standin': dict(wide_levels=5, level_launches=0, mid_run=1, final_grid=128, mid_lds=1, mid_global=0, refused=0, fin_lds=26, fin_global=1, exhausted=2, exhausted_long=1, n_fallback=27),
    # k_esort_mid in global memory (segments of more than 8192 keys), depth exhausted there
    'adversary-30000-device': dict(wide_levels=7, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=2, refused=0, fin_lds=74, fin_global=2, exhausted=3, exhausted_long=2, n_fallback=74),
    # the same, three long heapsorts
    'adversary-40000-device': dict(wide_levels=8, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=2, refused=0, fin_lds=84, fin_global=3, exhausted=5, exhausted_long=3, n_fallback=85),
    # the same with ties
    'adversary8-40000-device': dict(wide_levels=8, level_launches=0, mid_run=1, final_grid=128, mid_lds=0, mid_global=2, refused=0, fin_lds=80, fin_global=1, exhausted=1, exhausted_long=1, n_fallback=98),
    # the wide list does NOT run out of slots here (refused 0): 372 segments for k_esort_mid, 48 of them beyond its LDS
    'uniform32-4000000-device': dict(wide_levels=14, level_launches=0, mid_run=1, final_grid=2048, mid_lds=324, mid_global=48, refused=0, fin_lds=3435, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # 8192 tiles: the last wide size; one child found no tiles left
    'below2p20-16777217-device': dict(wide_levels=16, level_launches=0, mid_run=1, final_grid=2048, mid_lds=544, mid_global=79, refused=1, fin_lds=14421, fin_global=0, exhausted=0, exhausted_long=0, n_fallback=0),
    # the level-queue route: no wide level, no mid kernel, 1413 segments finished in global memory
    'below2p20-16777218-device': dict(wide_levels=0, level_launches=12, mid_run=0, final_grid=2048, mid_lds=0, mid_global=0, refused=0, fin_lds=1244, fin_global=1413, exhausted=0, exhausted_long=0, n_fallback=0),
}


def check_sort(g, keys, case):
    from oracle import orc
    keys = np.ascontiguousarray(keys, np.uint32)
    vals = np.arange(len(keys), dtype=np.uint32)
    gk, gv, nf = hooks.exact_sort_u32(g, keys, vals)
    st = hooks.debug_sort_queues(g)
    assert st["n"] == len(keys) and st["sort_qoverflow"] == 0
    c = census(st)
    c["n_fallback"] = nf
    print("CENSUS %s %r" % (case, c))
    ok, ov = orc.std_sort_u32(keys, vals)
    same(gk, ok, "keys")
    same(gv, ov, "tie order (the permutation of std::sort)")
    route_invariants(len(keys), c)
    if case in ROUTES:
        assert c == ROUTES[case], (case, c, ROUTES[case])
    return c


# ---------------------------------------------------------------------------------------------
# (a) the sort alone, (b) its routes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["%s-%d-%s" % (p, n, tag(n)) for p in PATTERNS for n in SIZES])
def test_sort_alone(g, case):
    pattern, n = case.split("-")[0], int(case.split("-")[1])
    check_sort(g, key_pattern(pattern, n), case)


@pytest.mark.parametrize("case", ["adversary-30000-device", "adversary-40000-device", "adversary8-40000-device"])
def test_sort_adversary_leaves_long_segments_without_depth_budget(g, case):
    """the adversary at a few tens of thousands of keys: the wide levels peel two keys off per partition, so what reaches queue 0 is still
    tens of thousands of keys long -- k_esort_mid works on it in global memory, its depth budget runs out there, and k_esort_final
    heapsorts a segment far longer than its LDS capacity in place"""
    pattern, n = case.split("-")[0], int(case.split("-")[1])
    c = check_sort(g, key_pattern(pattern, n), case)
    if pattern == "adversary":
        assert c["mid_global"] >= 1 and c["exhausted_long"] >= 1 and c["n_fallback"] >= 1, c


@pytest.mark.parametrize("n", [4000000, 12000000], ids=["4m-device", "12m_overfills_the_wide_list-device"])
def test_sort_millions_of_keys_over_the_whole_range(g, n):
    """Keys over the whole 32-bit range.  At 4 000 000 the wide list does NOT run out (measured: the segments of wide size peak below
    its 1024 slots; 6 and 8 million keys do not overfill it either); what k_esort_mid is given there are the 372 unlucky subtrees still
    long after fourteen levels.  At 12 000 000 keys more than 1024 segments are of wide size at once: the next wide list refuses those
    beyond its slots, queue 0 and k_esort_mid take them.  WHICH segments find a slot is decided by the order of the workgroups' atomics,
    and a refused segment is not split by the later wide levels, so there the counts of k_esort_mid's segments are not a function of the
    input (two runs: 201 and 208 refused, 734 + 178 and 773 + 145 segments for k_esort_mid); the finisher's segments are -- they are
    the nodes of std::sort's own partition tree -- and the permutation is."""
    k = np.random.default_rng(4).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    c = check_sort(g, k, "uniform32-%d-device" % n)
    assert (c["refused"] >= 1) == (n == 12000000) and c["mid_lds"] + c["mid_global"] >= c["refused"], c
    if n == 12000000:
        assert (c["wide_levels"], c["fin_lds"], c["fin_global"], c["exhausted"], c["n_fallback"]) == (16, 10340, 0, 0, 0), c


@pytest.mark.parametrize("n", [N_LAST_WIDE, N_LAST_WIDE + 1], ids=["last_wide_size-device", "level_queue-device"])
def test_sort_around_8192_tiles(g, n):
    """n = 8192 * 2048 + 1: the last size of the wide path (8192 tiles, preL / preR full); one key more: no wide level, no mid kernel --
    twelve k_esort_level launches and the finisher's global path for what is still long (the route of a config-4 map save)"""
    k = np.random.default_rng(n).integers(0, 1 << 20, n).astype(np.uint32)
    c = check_sort(g, k, "below2p20-%d-device" % n)
    if n > N_LAST_WIDE:
        assert c["wide_levels"] == 0 and c["mid_run"] == 0 and c["level_launches"] == 12 and c["fin_global"] >= 1, c
    else:  # (refused: the two children of the 8192-tile segment need 8193 tiles between them -- the second finds none left)
        assert c["wide_levels"] == 16 and c["mid_run"] == 1 and c["refused"] >= 1, c


# ---------------------------------------------------------------------------------------------
# (c) the whole chain
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["%s-%d-%s" % (p, n, tag(n)) for p in TIED for n in (2048, 2049, 4097, 8193, 40000)])
def test_chain_on_key_sequence_clouds(g, case):
    pattern, n = case.split("-")[0], int(case.split("-")[1])
    keys = key_pattern(pattern, n)
    cloud = key_cloud(keys)
    full = n * len(np.unique(keys)) <= MODEL_MAX  # (beyond it the model judges the centroids, the oracle alone the labels)
    rows, info = model(cloud, 0.5, nn=full)
    assert np.array_equal(info["keys"].astype(np.int64) - int(info["keys"].min()), keys.astype(np.int64) - int(keys.min())), "the cloud's keys"
    # the case is sensitive to the sort's tie order: with a stable sort's order inside the voxels the model's own output differs
    stable_rows, _ = model(cloud, 0.5, stable=True, nn=False)
    assert (rows[:, :3].view(np.uint32) != stable_rows[:, :3].view(np.uint32)).any(), "blind to tie order: replace this case"
    from oracle import orc
    got = g.voxelize_preserving_labels(cloud, 0.5)
    st = hooks.debug_sort_queues(g)
    assert st["n"] == n and st["n_voxel_overflow"] == 0
    route_invariants(n, census(st))
    same(got, orc.voxelize_preserving_labels(cloud, 0.5), "device against oracle")
    same(got[:, :3], rows[:, :3], "device against model: centroids")
    if full:
        same(got, rows, "device against model")


@pytest.mark.parametrize("case", ["%s-%d-standin" % (k, n) for k in ("own_voxel_each", "one_voxel") for n in (1023, 1024, 1025, 4096, 4097)])
def test_chain_run_detection_at_its_tiles(g, case):
    kind, n = case.split("-")[0], int(case.split("-")[1])
    rng = np.random.default_rng(n)
    if kind == "own_voxel_each":
        cloud = key_cloud(rng.permutation(n))
    else:
        cloud = key_cloud(np.zeros(n, np.uint32))
    rows, info = judge(g, cloud, 0.5, "%s n=%d" % (kind, n))
    assert len(rows) == (n if kind == "own_voxel_each" else 1)


@pytest.mark.parametrize("runs", [(1023, 10, 500), (1024, 10, 500), (1000, 24, 1023, 5, 3000), (1, 1022, 1, 1024, 1)],
                         ids=["starts_on_last_key-standin", "ends_on_last_key-standin", "both_two_tiles-standin", "single_keys_at_the_edges-standin"])
def test_chain_runs_that_start_or_end_on_the_last_key_of_a_tile(g, runs):
    keys = np.repeat(np.arange(len(runs)), runs)
    keys = np.random.default_rng(5).permutation(keys)
    rows, info = judge(g, key_cloud(keys), 0.5, "runs %r" % (runs,))
    heads, ends = info["runs"]
    assert tuple(ends - heads) == tuple(runs)
    assert any(h % 1024 == 1023 for h in heads) or any(e % 1024 == 0 for e in ends[:-1])


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 1], ids=["2p20-device", "2p20_plus_1-device"])
def test_chain_at_the_size_where_run_detection_and_the_final_grid_switch(g, n):
    """1024 tiles of 1024 keys: k_run_count / k_run_emit and a final grid of 128; one point more: k_run_heads / scan_u32 / k_run_begin and
    a final grid of 2048.  Street-sized cloud at leaf 0.2, about one point per voxel; the oracle judges (the model would take minutes)"""
    rng = np.random.default_rng(n)
    cloud = np.column_stack([rng.uniform(-110, 110, n), rng.uniform(-90, 90, n), rng.uniform(-2, 4, n), rng.integers(1, 250, n)]).astype(F)
    judge(g, cloud, 0.2, "n=%d" % n, use_model=False)
    st = hooks.debug_sort_queues(g)
    c = census(st)
    route_invariants(n, c)
    assert st["n"] == n and st["run_tiles"] == (1024 if n == 1 << 20 else 1025) and c["final_grid"] == (128 if n == 1 << 20 else 2048), c


@pytest.mark.parametrize("leaf", [0.05, 0.2, 1.0], ids=["leaf_0.05-standin", "leaf_0.2-standin", "leaf_1.0-standin"])
def test_chain_key_geometry(g, leaf):
    rng = np.random.default_rng(int(leaf * 100))
    lf = float(F(leaf))
    # points exactly on cell faces, both signs (k * leaf in float32), with -0.0 and +0.0 among them
    k = rng.integers(-6, 7, (600, 3))
    faces = (k.astype(F) * F(leaf)).astype(F)
    faces[:5] = [[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [lf, -lf, -0.0]]
    on_faces = np.column_stack([faces, rng.integers(1, 250, len(faces))]).astype(F)
    judge(g, on_faces, leaf, "points on cell faces")
    mixed = on_faces.copy()
    mixed[::2, :3] += rng.uniform(-0.49, 0.49, (len(mixed[::2]), 3)).astype(F) * F(leaf)
    judge(g, mixed, leaf, "on faces and beside them")
    # all-negative cloud
    neg = np.column_stack([rng.uniform(-9, -1, (700, 3)) * leaf * 3, rng.integers(1, 250, 700)]).astype(F)
    judge(g, neg, leaf, "all negative")
    # an axis one cell thick (each axis in turn)
    for a in range(3):
        flat = np.column_stack([rng.uniform(-8, 8, (700, 3)) * leaf * 2, rng.integers(1, 250, 700)]).astype(F)
        flat[:, a] = (rng.uniform(0.1, 0.9, 700) * leaf + 3 * leaf).astype(F)
        rows, info = judge(g, flat, leaf, "axis %d one cell thick" % a)
        assert info["div_b"][a] == 1


@pytest.mark.parametrize("cells", [1290, 1291], ids=["largest_grid_accepted-standin", "first_grid_refused-standin"])
def test_chain_at_the_largest_grid_voxelgrid_accepts(g, cells):
    """1290^3 < 2^31 - 1 < 1291^3 cells at leaf 1.0: the first is voxelised, the second comes back as it went in (pass-through), counted"""
    rng = np.random.default_rng(cells)
    xyz = rng.uniform(0.5, cells - 0.5, (300, 3))
    xyz[0], xyz[1] = 0.5, cells - 0.5
    xyz[2:40] = xyz[40:78] + rng.uniform(-0.2, 0.2, (38, 3))  # (some voxels hold more than one point)
    cloud = np.column_stack([xyz, rng.integers(1, 250, 300)]).astype(F)
    cloud = np.concatenate([cloud, cloud[100:110] * [1, 1, 1, 0] + [0, 0, 0, 251]]).astype(F)  # exact duplicates with other labels
    rows, info = judge(g, cloud, 1.0, "%d cells per axis" % cells)
    st = hooks.debug_sort_queues(g)
    if cells == 1290:
        assert not info["passthrough"] and tuple(info["div_b"]) == (1290, 1290, 1290) and st["n_voxel_overflow"] == 0 and len(rows) < len(cloud)
    else:
        assert info["passthrough"] and st["n_voxel_overflow"] >= 1 and len(rows) == len(cloud)
        same(rows[:, :3], cloud[:, :3], "the cloud as it went in")
        assert (rows[-10:, 3] == cloud[100:110, 3]).all(), "a duplicate takes the label of the first point with its coordinates"


def _voxel_of(info, p, leaf):
    ijk = (np.floor(np.asarray(p, F) * info["inv"]) - info["min_b"].astype(F)).astype(np.int64)
    key = ijk[0] + ijk[1] * info["div_b"][0] + ijk[2] * info["div_b"][0] * info["div_b"][1]
    return int(np.flatnonzero(info["ukeys"] == key)[0])


@pytest.mark.parametrize("case", ["two_clusters-standin"])
def test_label_from_a_neighbouring_voxel(g, case):
    """a two-cluster voxel: its centroid lies between the clusters, nearest a point of the voxel below"""
    rng = np.random.default_rng(11)
    own = np.concatenate([rng.uniform(0.01, 0.05, (6, 3)) + [0, 0.02, 0.4], rng.uniform(0.01, 0.05, (6, 3)) + [0.93, 0.02, 0.4]])
    other = [[0.5, -0.04, 0.45], [2.5, 0.5, 0.5], [-1.5, 1.5, 0.5], [0.5, 0.5, 1.5]]
    cloud = np.column_stack([np.concatenate([own, other]), np.arange(1, 17)]).astype(F)
    rows, info = judge(g, cloud, 1.0, "two clusters")
    v = _voxel_of(info, cloud[0, :3], 1.0)
    assert rows[v, 3] == 13.0, "the label of the neighbour's point (index 12)"


@pytest.mark.parametrize("first", ["neighbour", "own"], ids=["neighbour_first-standin", "own_first-standin"])
def test_label_tie_between_an_own_point_and_a_neighbours(g, first):
    """centroid (0.75, 0.5, 0.5); the own point (0.5, 0.5, 0.5) and the neighbouring voxel's (1.0, 0.5, 0.5), which lies on its cell's face,
    are both exactly 0.25 away: the lower index wins, whichever voxel holds it"""
    own = [[0.5, 0.5, 0.5], [0.875, 0.75, 0.5], [0.875, 0.25, 0.5]]
    nb = [[1.0, 0.5, 0.5]]
    far = [[3.5, 0.5, 0.5], [-2.5, 1.5, 1.5]]
    xyz = (nb + own + far) if first == "neighbour" else (own + nb + far)
    cloud = np.column_stack([xyz, np.arange(1, len(xyz) + 1)]).astype(F)
    rows, info = judge(g, cloud, 1.0, "tie own / neighbour")
    v = _voxel_of(info, [0.5, 0.5, 0.5], 1.0)
    same(rows[v, :3], np.array([0.75, 0.5, 0.5], F), "the centroid")
    assert info["n_tied"][v] == 2, "the model confirms the tie"
    assert rows[v, 3] == 1.0, "the lowest index wins"


@pytest.mark.parametrize("case", ["%s-%d-standin" % (k, o) for k in ("opposite", "two_axes") for o in (0, 1)])
def test_label_tie_between_two_neighbours(g, case):
    kind, order = case.split("-")[0], int(case.split("-")[1])
    """the own points sit in opposite corners, farther from the centroid (0.46875 on every axis) than two points of neighbouring voxels
    that are exactly equally far: on opposite sides along x, or on the faces x = 1 and y = 1"""
    own = [[0.0, 0.0, 0.0], [0.9375, 0.9375, 0.9375]]
    c = 0.46875
    nb = [[-0.0625, c, c], [1.0, c, c]] if kind == "opposite" else [[1.0, c, c], [c, 1.0, c]]
    if order:
        nb = nb[::-1]
    far = [[3.5, 0.5, 0.5], [-2.5, 1.5, 1.5]]
    xyz = own + far + nb
    cloud = np.column_stack([xyz, np.arange(1, len(xyz) + 1)]).astype(F)
    rows, info = judge(g, cloud, 1.0, "tie between neighbours")
    v = _voxel_of(info, [0.0, 0.0, 0.0], 1.0)
    same(rows[v, :3], np.array([c, c, c], F), "the centroid")
    assert info["n_tied"][v] == 2, "the model confirms the tie"
    assert rows[v, 3] == 5.0, "the lower index of the two wins"


@pytest.mark.parametrize("case", ["grid_4x3x3-standin"])
def test_label_search_on_the_grids_corners_edges_and_faces(g, case):
    """every cell of a 4 x 3 x 3 grid filled: voxels on the grid's corners, edges, faces and inside, their shells clipped accordingly"""
    rng = np.random.default_rng(12)
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    xyz = np.concatenate([(cells + rng.uniform(0.02, 0.98, cells.shape)) * 0.2 for _ in range(4)])
    # clusters in two corners of each cell pull the centroids towards the cells' middles, away from the own points
    xyz = np.concatenate([xyz, (cells + 0.03) * 0.2, (cells + 0.97) * 0.2])
    cloud = np.column_stack([xyz - [7, 3, 1], rng.integers(1, 250, len(xyz))]).astype(F)
    cloud = cloud[rng.permutation(len(cloud))]
    rows, info = judge(g, cloud, 0.2, "filled grid")
    assert len(rows) == 36 and tuple(info["div_b"]) == (4, 3, 3)


@pytest.mark.parametrize("where", [(3000.0, -2000.0, 40.0), (-9000.0, 7000.0, 300.0)], ids=["drift_40_cells-device", "larger_offset-device"])
def test_label_search_of_a_crowded_voxel_far_from_the_origin(g, where):
    """60 000 points in one 0.05 m voxel far from the origin: the sequential float32 sum leaves the voxel -- the centroid lies cells
    away from the cell it belongs to, beyond the grid even (the 400 labelled neighbours span +-7 cells): the stage-0 exit must not
    fire, the shells run to maxrho, d2c prunes with its margins at a distance"""
    rng = np.random.default_rng(13)
    leaf = 0.05
    crowd = np.asarray(where) + rng.uniform(0.01, 0.04, (60000, 3))
    near = np.asarray(where) + rng.uniform(-7, 8, (400, 3)) * leaf
    cloud = np.column_stack([np.concatenate([crowd, near]), rng.integers(1, 250, 60400)]).astype(F)
    cloud = cloud[rng.permutation(len(cloud))]
    rows, info = judge(g, cloud, leaf, "crowded voxel")
    heads, ends = info["runs"]
    v = int(np.argmax(ends - heads))
    assert ends[v] - heads[v] >= 60000
    own = np.array([info["ukeys"][v] % info["div_b"][0], info["ukeys"][v] // info["div_b"][0] % info["div_b"][1],
                    info["ukeys"][v] // (info["div_b"][0] * info["div_b"][1])], np.int64)
    at = (np.floor(rows[v, :3] * info["inv"]) - info["min_b"].astype(F)).astype(np.int64)
    drift = int(np.abs(at - own).max())
    print("DRIFT %r: the centroid's cell %r, its voxel's %r, grid %r" % (where, at.tolist(), own.tolist(), info["div_b"].tolist()))
    assert drift >= 2, "the centroid did not leave its voxel's neighbourhood"
    if where[0] < 0:
        assert ((at < 0) | (at >= info["div_b"])).any(), "the centroid did not leave the grid"


def _wide_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-4000, 4000, (n, 3)), rng.integers(1, 250, n)]).astype(F)


@pytest.mark.parametrize("case", ["%s-%d-standin" % (d, n) for d in ("no_duplicates", "duplicate_groups") for n in (1, 2047, 2048, 2049, 6000)])
def test_passthrough_chain(g, case):
    dups, n = case.split("-")[0], int(case.split("-")[1])
    """leaf 1e-3 on a cloud 8 km wide: VoxelGrid refuses it (a single point it voxelises: the model decides which), every point keeps
    its place and takes the label of the first point with its coordinates"""
    cloud = _wide_cloud(n, n)
    rng = np.random.default_rng(n + 1)
    if dups == "duplicate_groups" and n > 1:
        # groups of 2 to 100 members, far apart in index, each member with a label of its own
        free = rng.permutation(n)
        at = 0
        for size in (2, 3, 17, 64, 100):
            if at + size > n // 2:
                break
            members = free[at:at + size]
            cloud[members, :3] = cloud[members[0], :3]
            at += size
        # a -0.0 / +0.0 pair: equal under the comparison that defines a duplicate
        a, b = free[at], free[at + 1]
        cloud[a, :3] = [0.0, -0.0, 12.5]
        cloud[b, :3] = [-0.0, 0.0, 12.5]
    rows, info = judge(g, cloud, 1e-3, "%s n=%d" % (dups, n))
    assert info["passthrough"] == (n > 1) and len(rows) == n
    if dups == "duplicate_groups" and n > 1:
        assert (rows[:, 3] != cloud[:, 3]).sum() >= 1, "labels were replaced"
        assert rows[max(a, b), 3] == cloud[min(a, b), 3], "-0.0 == +0.0"
    else:
        same(rows, cloud, "no duplicates: the cloud itself")


# ---------------------------------------------------------------------------------------------
# (d) shared launches with scans of very different sizes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query_voxel_size", [0.2, 0.04], ids=["voxelising-device", "one_set_both_modes-device"])
def test_shared_launches_with_unequal_scans(gpu_mod, query_voxel_size):
    """One handle, chains shared in fours (chain_batch(4, 1)), eight nodes announced as far ahead as the handle holds them (seven at a
    time), both transforms with each.  The scans: two whole ones and six cut to 1, 5, 2048, 2049, 4097 and 9000 points, ordered so that
    the set of four that forms holds 2049, 9000, 4097 points and a whole scan (wl and every grid of the shared launches are sized by the
    longest; a chain shorter than WIDE_MIN goes alone).  At query_voxel_size 0.04 VoxelGrid refuses the wide scans of that set and takes
    the one cropped to a 10 m box: one set holds both outcomes, the refused chains are redone as pass-throughs by their steps."""
    sc = scenarios.small()
    p = copy.copy(sc["params"])
    p.query_voxel_size = query_voxel_size
    gg, o = make_pair(gpu_mod, p)
    try:
        _shared_launches(gg, o, sc, query_voxel_size)
    finally:
        gg.close()  # (by the hooks build that made it, see the fixture g)


def _shared_launches(gg, o, sc, query_voxel_size):
    gg.set_map(sc["map"])
    o.set_map(sc["map"])
    gg.chain_batch(4, 1)
    cuts = [None, 2049, 9000, 4097, None, 1, 2048, 5]
    scans = []
    for k, c in enumerate(cuts):
        s = np.ascontiguousarray(sc["scans"][k], F)
        if c == 4097 and query_voxel_size < 0.1:
            s = s[(np.abs(s[:, 0]) < 5) & (np.abs(s[:, 1]) < 5)]
            assert len(s) >= 4097
        scans.append(np.ascontiguousarray(s[:c] if c else s))
    n, ahead = len(scans), 6
    Tl, Tb, To = sc["T_l2b"], sc["T_b2o"], sc["T_o2b"]
    for j in range(ahead):
        gg.prefetch(scans[j], Tl, Tb[j], To[j])
    overflowed = []
    for k in range(n):
        if k + ahead < n:
            gg.prefetch(scans[k + ahead], Tl, Tb[k + ahead], To[k + ahead])
        rg = gg.step(scans[k], Tl, Tb[k], To[k])
        ro = o.step(scans[k], Tl, Tb[k], To[k])
        overflowed.append(ro.n_voxel_overflow > 0)
        compare_step(gg, o, rg, ro, full=True)
    sets, chains = gg.chain_batch_counts()
    assert sets >= 1 and chains > 2 * sets, "no set of three or more chains formed: %r" % ((sets, chains),)
    if query_voxel_size < 0.1:
        assert any(overflowed[1:5]) and not all(overflowed[1:5]), "the set of four should hold both modes: %r" % (overflowed,)
    else:
        assert not any(overflowed)
