"""The stable bucketing of the map's VoI and of the voxelised scan by R-POD key, and the bin statistics read from it (kernels.hip.h:
k_mb_hist, k_mb_colscan, k_mb_scatter_w<2176> / <4096>, k_mb_scatter, k_qb_hist / k_qb_scan / k_qb_scatter and their shared-launch forms,
the LSD radix passes with k_gather and k_bin_offsets, k_bin_stats, k_bin_stats_srt; erasor_hip.hip: bucket_tiles, launch_bucket_table /
_scatter, key_bits) on DESIGNED KEY SEQUENCES: a case states the R-POD key (sector * R + ring, or B for the complement) of every map
point in map order, so it decides how many buckets there are, how many tiles the VoI has and where a run of equal keys ends.

The code changes path on three numbers:
  buckets   nbk = B + 1 (B + 2 in an overlapped step): <= 2176 k_mb_scatter_w<2176>, <= 4096 k_mb_scatter_w<4096>, <= 12288 k_mb_scatter,
            beyond that the radix passes; B + 2 > 4096 leaves the scatter and the statistics of an overlapped step to the step itself;
            k_qb_scan walks buckets in rounds of 1024, k_mb_colscan takes 16 per workgroup, key_bits grows at every power of two
  tiles     4096 keys per map tile (512 per wavefront, in strips of 64), 1024 per scan tile; the column scan takes 64 tiles per wavefront
            scan and 256 per round (a second round from 1 048 577 points on); k_qb_scatter sums the earlier tiles four at a time; the
            grids are sized from the previous step's VoI (at least 64 tiles), beyond that the tiles are walked with a grid stride
  positions lanes with equal keys are grouped, the highest lane of a group bumps the counter, waves take their turn in index order

The world: an R x S grid with rings 2 m wide, max_range = 2 R, identity poses, min_h / max_h = -5 / 5.  Point j of key k lies well
inside its cell (0.15 .. 0.85 m of the ring, 0.25 .. 0.75 of the sector), a point of the complement bucket has z = +-7.  The scan gives
every bin fewer than minimum_num_pts points unless a case says otherwise: every bin is LITTLE_NUM and the map is kept whole.

Every case (run_design) asserts ON THE ORACLE'S numbers that it is the case it claims to be (n_voi the designed length, n_outskirts,
n_ambiguous, n_voxel_overflow and the bin counts as designed), then that the oracle agrees with a model in plain numpy that shares
nothing with it (counts by bincount, float32 extrema, the static estimate as map[argsort(keys, stable)], the complement in map order),
then compare_step(full=True): bit-exact, no tolerances.  A case whose inputs miss fails; nothing is skipped.

The axes are NOT crossed unless a test says so: each is varied against a default for the others (the `mixed` sequence, two tiles + 1
point, v3, one plain step on the suite's overlapped path).

On the scan side the order is VoxelGrid's, not the caller's: a scan is built of one point per 0.05 m voxel, layer of voxels by layer,
and the model states the order VoxelGrid leaves (z-major, then y, then x); the oracle's voxelised scan must equal it.  In v3 the
bucketed scan shows only in get_bins(1); the same scans therefore also run in v2 with minimum_num_pts = 1, where every scan bin joins
the map whole and map_arranged_ IS the bucketed scan.  What a cell can hold in 0.05 m voxels bounds the sequences there (SCAN_BIG_KINDS).

828 cases; the whole file takes 8.3 to 10.6 s on one MI355X (pytest's figure, three runs), the slowest case 2.8 s (a process of its own), the
1 048 577-point case 0.2 s.  The 202 cases whose ids end in `standin` run on the CPU stand-in (tests/test_full_step_on_cpu.py with
ERASOR_SIMT_MORE=1; 11 minutes in a process of their own on an 8-core host with other runs beside it).  MEASUREMENTS.md lists which cases
each of five one-line faults of the kernels turns red.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_oracle_known_answers as ka
from test_gpu_parity import I4, compare_step, gpu_mod, make_pair, same  # noqa: F401  (gpu_mod: the module's fixture)

pytestmark = pytest.mark.gpu

RING = 2.0            # [m] ring width
INF_H = 10000000000000.0  # erasor.h: a bin without points has max_h = -INF_H, min_h = +INF_H
MB_TILE, QB_TILE = 4096, 1024
F32 = np.float32
G1, G2, G3 = 0.6180339887498949, 0.7548776662466927, 0.41421356237309515  # (irrational steps: no two points of a cell coincide)


def grid_params(R, S, **kw):
    return ka.one_bin_params(num_rings=R, num_sectors=S, max_range=RING * R, **kw)


def bin_index(R, S, keys):
    keys = np.asarray(keys, np.int64)
    return (keys % R) * S + keys // R


# ---------------------------------------------------------------------------------------------
# 1. the designed world and the independent model
# ---------------------------------------------------------------------------------------------
def occurrence(keys):
    """for every element its rank among the elements of the same key that come before it"""
    keys = np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    first = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if len(sk) else np.zeros(0, np.int64)
    rank = np.arange(len(sk)) - np.repeat(first, np.diff(np.r_[first, len(sk)]))
    occ = np.empty(len(sk), np.int64)
    occ[order] = rank
    return occ


def place(R, S, keys, z=None):
    """the cloud of a key sequence: point j lies in the cell of keys[j] (key B: in cell j mod B, above or below the height gate)"""
    keys = np.asarray(keys, np.int64)
    n, B = len(keys), R * S
    assert n == 0 or (0 <= keys.min() and keys.max() <= B)
    j = np.arange(n)
    comp = keys == B
    cell = np.where(comp, j % B, keys)
    occ = occurrence(cell)
    sector, ring = np.divmod(cell, R)
    r = ring * RING + 0.15 + 0.7 * np.modf(occ * G1 + 0.137 * (cell % 7))[0]
    th = (sector + 0.25 + 0.5 * np.modf(occ * G2 + 0.31)[0]) * (2 * ka.PI_REF / S)
    if z is None:
        z = -4.0 + 8.0 * np.modf(j * G3)[0]
    z = np.where(comp, np.where(j % 2 == 0, 7.0, -7.0), np.asarray(z, np.float64))
    return np.column_stack([r * np.cos(th), r * np.sin(th), z, 40.0 + cell % 32]).astype(F32)


def little_scan(R, S):
    """two points in bin 0 and one in bin B - 1: fewer than minimum_num_pts in every bin"""
    return place(R, S, [0, 0, R * S - 1][:3 if R * S > 1 else 2], z=[0.1, 0.4, 0.2][:3 if R * S > 1 else 2])


def model(R, S, mp, keys):
    """what a step with identity poses makes of the map `mp` whose points have the keys `keys`, from numpy alone:
    (count, min_h, max_h) per bin as get_bins gives them, map_voi, static_estimate, complement"""
    keys = np.asarray(keys, np.int64)
    B = R * S
    inh = keys < B
    at = bin_index(R, S, keys[inh])
    cnt = np.bincount(at, minlength=B).astype(np.uint32)
    mn, mx = np.full(B, np.inf, F32), np.full(B, -np.inf, F32)
    np.minimum.at(mn, at, mp[inh, 2])
    np.maximum.at(mx, at, mp[inh, 2])
    mn64 = np.where(cnt > 0, mn.astype(np.float64), INF_H)
    mx64 = np.where(cnt > 0, mx.astype(np.float64), -INF_H)
    static = mp[inh][np.argsort(keys[inh], kind="stable")]
    return (cnt, mn64, mx64), mp, static, mp[~inh]


def assert_model(o, ro, R, S, mp, keys, n_outskirts=0, map_kept=True):
    """checks 1 and 2 of a case: the oracle's step is the designed one, and the oracle agrees with the model"""
    (cnt, mn, mx), voi, static, comp = model(R, S, mp, keys)
    assert ro.n_voi == len(keys), (ro.n_voi, len(keys))
    assert ro.n_outskirts == n_outskirts and ro.n_ambiguous == 0 and ro.n_voxel_overflow == 0, ro.as_dict()
    got = o.get_bins(0)
    assert np.array_equal(got[0], cnt), ("points per bin", np.flatnonzero(got[0] != cnt)[:8].tolist())
    assert np.array_equal(got[1], mn), ("min_h per bin", np.flatnonzero(got[1] != mn)[:8].tolist())
    assert np.array_equal(got[2], mx), ("max_h per bin", np.flatnonzero(got[2] != mx)[:8].tolist())
    same(o.get_cloud(1), voi, "map_voi: the map, in map order")
    if map_kept:
        assert ro.n_reverted_bins == 0 and ro.n_map_rejected == 0, ro.as_dict()
        same(o.get_cloud(2), static, "static_estimate: the in-height points in stable key order")
        same(o.get_cloud(3), comp, "complement: the out-of-height points in map order")
        if n_outskirts == 0:
            same(o.get_map(), np.concatenate([static, comp]), "map_arranged_")


_pairs = {}


def pair(gpu_mod, R, S, profiled=False, **kw):
    key = (R, S, profiled) + tuple(sorted(kw.items()))
    if key not in _pairs:
        g, o = make_pair(gpu_mod, grid_params(R, S, **kw))
        if profiled:
            g.profiling(1)
        _pairs[key] = (g, o, grid_params(R, S, **kw))
    return _pairs[key]


def run_keys(g, o, R, S, keys):
    """set_map and one step on the map of a key sequence: the three checks"""
    mp, sc = place(R, S, keys), little_scan(R, S)
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(sc, I4, I4, I4)
    assert_model(o, ro, R, S, mp, keys)
    rg = g.step(sc, I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)
    return mp, rg, ro


def run_design(gpu_mod, R, S, keys, profiled=False, **kw):
    g, o, p = pair(gpu_mod, R, S, profiled, **kw)
    return run_keys(g, o, R, S, keys)


# ---------------------------------------------------------------------------------------------
# 2. key sequences
# ---------------------------------------------------------------------------------------------
RUNS = (63, 64, 65, 511, 512, 513, 4097)
KINDS = ("bucket0", "last_bucket", "complement", "round_robin", "descending", "alternating", "ends_only", "in_order", "mixed") + tuple(
    "runs%d" % L for L in RUNS)


def sequence(kind, B, n):
    """n keys in [0, B]"""
    j = np.arange(n, dtype=np.int64)
    nb = B + 1
    if kind == "bucket0":
        return np.zeros(n, np.int64)
    if kind == "last_bucket":
        return np.full(n, B - 1, np.int64)
    if kind == "complement":
        return np.full(n, B, np.int64)
    if kind == "round_robin":        # every lane of a wavefront holds another key (B >= 63)
        return j % nb
    if kind == "descending":
        return B - (j * nb) // max(n, 1)
    if kind == "alternating":
        return np.where(j % 2 == 0, B // 3, (2 * B) // 3 + (B > 1))
    if kind == "ends_only":          # buckets 0, B - 1 and B, in a seeded order
        return np.array([0, B - 1, B], np.int64)[np.random.default_rng(n).integers(0, 3, n)]
    if kind == "in_order":           # the production case: the map as a step left it
        return np.sort(np.random.default_rng(n + 1).integers(0, nb, n))
    if kind.startswith("runs"):      # runs of equal keys, L long: their ends slide across every strip, wavefront and tile boundary
        L = int(kind[4:])
        return ((j // L) * 37 + (j // L) ** 2 % 5) % nb
    if kind == "mixed":              # the default of the other axes: every kind of neighbourhood, every bucket, both ends, the complement
        rng = np.random.default_rng(B * 7 + n)
        k = rng.integers(0, nb, n)
        third = n // 3
        k[:third] = j[:third] % nb                                  # all lanes distinct
        k[third:2 * third] = ((j[third:2 * third] // 65) * 37) % nb  # runs that cross strips
        if n >= 3:
            k[0], k[n // 2], k[n - 1] = B, 0, B - 1
        return k
    raise KeyError(kind)


# ---------------------------------------------------------------------------------------------
# 3. the map side: bucket counts, VoI lengths, key sequences
# ---------------------------------------------------------------------------------------------
TABLE_GRIDS = ((25, 87), (34, 64), (46, 89), (63, 65), (64, 64), (17, 241), (11, 1117), (96, 128))
# B + 1 no multiple of 16 (k_mb_colscan's last workgroup is partial), B + 1 = 2 .. 64, and 1024, 1025, 2048, 2049 (k_qb_scan's rounds, key_bits)
SMALL_GRIDS = ((1, 1), (1, 2), (3, 5), (1, 16), (3, 7), (7, 9), (8, 8), (11, 93), (32, 32), (23, 89), (32, 64))
assert [R * S + 1 for R, S in SMALL_GRIDS] == [2, 3, 16, 17, 22, 64, 65, 1024, 1025, 2048, 2049]
assert [R * S for R, S in TABLE_GRIDS] == [2175, 2176, 4094, 4095, 4096, 4097, 12287, 12288]
DEFAULT_N = 2 * MB_TILE + 1
# What the CPU stand-in of tests/test_full_step_on_cpu.py re-runs (ids ending in `standin`): cases of at most three map tiles on grids of
# at most ~4100 bins -- and of those a part: a step costs the stand-in about a second per 400 bins whatever the VoI's length, so the
# grids of 4095 and more bins get the lengths and sequences that differ most, the grid of 2175 bins nearly everything.
STANDIN_POINTS = 3 * MB_TILE
HEAVY_GRIDS = ((63, 65), (64, 64), (17, 241))


def tag(R, S, n, heavy_too=False):
    ok = n <= STANDIN_POINTS and (R * S <= 2200 or (heavy_too and (R, S) in HEAVY_GRIDS))
    return "standin" if ok else "device"


@pytest.mark.parametrize("R,S", [pytest.param(R, S, id="%dx%d-%s" % (R, S, tag(R, S, DEFAULT_N, True))) for R, S in TABLE_GRIDS + SMALL_GRIDS])
def test_every_bucket_count_class(gpu_mod, R, S):
    """axis 1, against the default sequence and length: each grid at a bucket-count edge.  Then a second step on the map the first left --
    the VoI already in bucket order, the production case, with the grids sized by a real step's VoI"""
    g, o, p = pair(gpu_mod, R, S)
    keys = sequence("mixed", R * S, DEFAULT_N)
    assert set((0, R * S - 1, R * S)) <= set(keys.tolist())
    mp, rg, ro = run_keys(g, o, R, S, keys)
    left = np.concatenate([np.sort(keys[keys < R * S], kind="stable"), keys[keys == R * S]])
    mp2 = o.get_map()
    ro = o.step(little_scan(R, S), I4, I4, I4)
    assert_model(o, ro, R, S, mp2, left)
    rg = g.step(little_scan(R, S), I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)


POINTS = (0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8192, 8193)
TILES = tuple(t * MB_TILE + d for t in (63, 64, 65) for d in (-1, 0, 1))
LENGTH_GRIDS = ((25, 87), (63, 65), (64, 64))


@pytest.mark.parametrize("R,S,n", [pytest.param(R, S, n, id="%dx%d-n%d-%s" % (R, S, n, tag(R, S, n, n in (MB_TILE + 1, 2 * MB_TILE + 1)))) for R, S in LENGTH_GRIDS
                                   for n in POINTS + TILES])
def test_voi_lengths(gpu_mod, R, S, n):
    """axis 2, against the default sequence, on the three scatter kernels: lengths around a strip, a wavefront's share, a tile and two, and
    around 64 tiles (one wavefront scan of the column scan, and the smallest grid bucket_tiles gives)"""
    run_design(gpu_mod, R, S, sequence("mixed", R * S, n))


def test_a_voi_of_256_tiles_and_one_point(gpu_mod):
    """1 048 577 points on 34 x 64: the smallest VoI that reaches the column scan's second round of 256 tiles (run[j] carried over) --
    the only case of its size"""
    keys = sequence("mixed", 34 * 64, 256 * MB_TILE + 1)
    keys[-1] = 7  # (the one point of tile 256 lands in a bucket that every earlier tile has filled)
    run_design(gpu_mod, 34, 64, keys)


SEQ_LENGTHS = (MB_TILE - 1, MB_TILE, MB_TILE + 1, 3 * MB_TILE + 1)
SEQ_GRIDS = ((25, 87), (63, 65), (64, 64))
HEAVY_KINDS = ("round_robin", "alternating", "bucket0", "runs65", "runs513")
SEQ_CASES = [pytest.param(R, S, kind, n, id="%dx%d-%s-n%d-%s" % (R, S, kind, n, tag(R, S, n, n == MB_TILE + 1 and kind in HEAVY_KINDS)))
             for R, S in SEQ_GRIDS for kind in KINDS if kind != "mixed" for n in SEQ_LENGTHS]
# the routes beyond the counting sort's tables and the shared-table edge, at the two lengths that differ most
SEQ_CASES += [pytest.param(R, S, kind, n, id="%dx%d-%s-n%d-device" % (R, S, kind, n)) for R, S in ((17, 241), (11, 1117), (96, 128))
              for kind in KINDS if kind != "mixed" for n in (MB_TILE + 1, 3 * MB_TILE + 1)]


@pytest.mark.parametrize("R,S,kind,n", SEQ_CASES)
def test_key_sequences(gpu_mod, R, S, kind, n):
    """axis 3, crossed with the lengths of one tile -1 / +0 / +1 and three tiles + 1 and with the three scatter kernels (the fine grids: two
    lengths): where equal keys sit in the sequence"""
    run_design(gpu_mod, R, S, sequence(kind, R * S, n))


# ---------------------------------------------------------------------------------------------
# 4. bin statistics: an extremum at a chosen position of a bin
# ---------------------------------------------------------------------------------------------
SR, SS = 16, 4   # the statistics' grid: 64 bins whose outer cells hold more than a thousand 0.05 m voxels (the scan side needs them)
STAT_N = (1, 2, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 512, 513, 1025)
STAT_BINS = [s * SR + ring for s in range(SS) for ring in (9, 11, 13, 15)]      # the sixteen bins under test ...
FILL_BINS = [s * SR + ring for s in range(SS) for ring in (8, 10, 12, 14)]      # ... each between two bins whose heights lie beyond its own
LEAF = 0.05


def stat_positions(n):
    """(bin under test, "min" / "max", position) for the positions that a bin of n points has"""
    pos = [0, n - 1, n - 64, n - 65, 191, 192, 255, 256]
    out = []
    for t, key in enumerate(STAT_BINS):
        p = pos[t % 8]
        if 0 <= p < n:
            out.append((key, "min" if t < 8 else "max", p))
    return out


def voxel_order(pts):
    """the order PCL's VoxelGrid leaves one-point voxels in: by voxel index, z-major, then y, then x (float32 arithmetic as the filter's)"""
    ijk = np.floor(pts[:, :3] * (F32(1) / F32(LEAF))).astype(np.int64)
    assert len(np.unique(ijk, axis=0)) == len(pts), "two points share a voxel"
    return np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))


def lattice(key, n):
    """n places in the cell of `key` (grid SR x SS), 0.08 m apart radially and at least that along the arc: no two share a 0.05 m voxel"""
    sector, ring = divmod(key, SR)
    r0 = ring * RING + 0.15
    i = np.arange(n)
    row, col = i % 9, i // 9
    th = (sector + 0.25) * (2 * ka.PI_REF / SS) + col * 0.081 / r0
    assert n == 0 or th.max() <= (sector + 0.75) * (2 * ka.PI_REF / SS), "the cell is too small"
    r = r0 + 0.08 * row
    return np.column_stack([r * np.cos(th), r * np.sin(th)])


def stats_world(n, side):
    """(cloud, its keys) in the order that the bucketing sees: the map's own order (side 0), the voxelised scan's (side 1).  Every bin under
    test holds n points whose heights lie strictly inside (lo, hi) but for ONE at the stated position, the bin's unique minimum (or maximum);
    the bins before and behind it in key order hold heights beyond both, and so does the complement behind the last"""
    # side 1: every point of the bins under test in ONE layer of voxels (z in [0, 0.05)), so that the order inside a bin is the (y, x) order
    lo, hi, span = (F32(-1.5), F32(1.5), (-1.0, 1.0)) if side == 0 else (F32(0.01), F32(0.04), (0.02, 0.03))
    chosen = {key: (which, p) for key, which, p in stat_positions(n)}
    pts, keys = [], []
    for key in sorted(STAT_BINS + FILL_BINS):
        m = n if key in STAT_BINS else 4
        xy = lattice(key, m).astype(F32)
        if key in STAT_BINS:
            order = np.arange(m) if side == 0 else np.lexsort((np.floor(xy[:, 0] * F32(20)), np.floor(xy[:, 1] * F32(20))))
            z = np.empty(m)
            z[order] = span[0] + (span[1] - span[0]) * (0.05 + 0.9 * np.modf(np.arange(m) * G3)[0])
            if key in chosen:
                z[order[chosen[key][1]]] = lo if chosen[key][0] == "min" else hi
        else:
            z = np.array([-3.0, 3.0, 3.25, -3.25])  # (in layers of their own on the scan side)
        pts.append(np.column_stack([xy, z, np.full(m, 40.0 + key % 32)]))
        keys.append(np.full(m, key))
    comp = np.column_stack([lattice(STAT_BINS[0], 2), [7.0, -7.0], [41.0, 41.0]])
    pts, keys = np.concatenate(pts + [comp]).astype(F32), np.concatenate(keys + [np.full(2, SR * SS)])
    if side == 0:  # the bins' points dealt out in turn: the scatter has work to do, and keeps each bin's order
        order = np.lexsort((keys, occurrence(keys)))
    else:
        order = voxel_order(pts)
    return pts[order], keys[order]


def assert_positions(cloud, keys, n):
    """the designed extremum of every bin under test is unique and sits at the stated place of the bin, in the cloud's own order"""
    for key, which, pos in stat_positions(n):
        z = cloud[keys == key, 2]
        assert len(z) == n
        if n > 1:
            at = int(np.argmin(z) if which == "min" else np.argmax(z))
            zs = np.sort(z)
            assert at == pos and (zs[0] < zs[1] if which == "min" else zs[-1] > zs[-2]), (key, which, pos, at)


STAT_VARIANTS = {"v3": dict(), "v2": dict(version=2), "profiled": dict(profiled=True)}


@pytest.mark.parametrize("n", [pytest.param(n, id="n%d-standin" % n) for n in STAT_N])
@pytest.mark.parametrize("variant", list(STAT_VARIANTS))
def test_an_extremum_at_every_position_of_a_map_bin(gpu_mod, variant, n):
    """axis 4, map side: k_bin_stats_srt (v3), k_bin_stats (v2), and v3 with every launch on its own (profiling(1)).  Sixteen bins of n
    points each, in one step: the unique minimum (eight bins) or maximum (eight) at the first, the last, the n - 64th, the n - 65th, the
    191st .. 256th place -- where the loop of four loads ends and the loop of single loads begins.  The count comes from the offsets
    and is right whatever the loops do; the extrema are what a wrong bound spoils"""
    g, o, p = pair(gpu_mod, SR, SS, **STAT_VARIANTS[variant])
    mp, keys = stats_world(n, 0)
    assert_positions(mp, keys, n)
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(little_scan(SR, SS), I4, I4, I4)
    assert_model(o, ro, SR, SS, mp, keys)
    rg = g.step(little_scan(SR, SS), I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)


def assert_scan_model(o, ro, R, S, sc, keys):
    """the scan side of checks 1 and 2: `sc` in the voxelised scan's order, `keys` the keys of its points"""
    (cnt, mn, mx), voi, _, _ = model(R, S, sc, keys)
    assert ro.n_query == len(sc) and ro.n_ambiguous == 0 and ro.n_voxel_overflow == 0, ro.as_dict()
    same(o.get_cloud(0), voi, "query_voi: one point per voxel, in voxel order")
    got = o.get_bins(1)
    assert np.array_equal(got[0], cnt), ("scan points per bin", np.flatnonzero(got[0] != cnt)[:8].tolist())
    assert np.array_equal(got[1], mn) and np.array_equal(got[2], mx), "scan min_h / max_h per bin"


@pytest.mark.parametrize("n", [pytest.param(n, id="n%d-standin" % n) for n in STAT_N])
def test_an_extremum_at_every_position_of_a_scan_bin(gpu_mod, n):
    """axis 4, scan side (k_bin_stats on the bucketed scan, get_bins(1)): the same sixteen bins, their points more than a voxel's diagonal
    apart and in ONE layer of voxels, so that VoxelGrid keeps every point and leaves a bin's points in (y, x) order -- the position of the
    extremum in the bucketed bin is the designed one (asserted on the oracle's voxelised scan)"""
    g, o, p = pair(gpu_mod, SR, SS)
    sc, keys = stats_world(n, 1)
    assert_positions(sc, keys, n)
    mp = place(SR, SS, [1] * 5)  # (a bin that the scan leaves empty)
    raw = sc[np.random.default_rng(n).permutation(len(sc))]
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(raw, I4, I4, I4)
    assert_scan_model(o, ro, SR, SS, sc, keys)
    assert_model(o, ro, SR, SS, mp, [1] * 5)
    rg = g.step(raw, I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)


# ---------------------------------------------------------------------------------------------
# 5. the query side: key sequences of the voxelised scan
# ---------------------------------------------------------------------------------------------
LAYERS = 190  # layers of 0.05 m voxels between -4.75 m and 4.75 m


def scan_cloud(R, S, keys, max_ring=None):
    """(scan, keys), both in the order VoxelGrid leaves: a scan of one point per voxel whose voxels have the keys `keys` in the given order
    layer by layer -- consecutive keys share a layer of voxels (ceil(n / 190) a layer), the layers follow each other in z, and inside a
    layer the order is VoxelGrid's (y, x) order, which voxel_order states.  A cell takes nine points of a layer along its radius and as
    many such rows as its arc has room for, 0.08 m apart: more than a voxel's diagonal.  max_ring: fold the rings into [0, max_ring) (a
    grid 384 m wide has more 0.05 m voxels than VoxelGrid can index)"""
    keys = np.asarray(keys, np.int64).copy()
    n, B = len(keys), R * S
    if max_ring:
        inh = keys < B
        keys[inh] = keys[inh] // R * R + keys[inh] % R % max_ring
    j = np.arange(n)
    layer = j // max(1, -(-n // LAYERS))
    comp = keys == B
    layer = np.where(comp, LAYERS + 6 + layer % 20, layer)  # (the complement: twenty layers above the height gate, z > 5.05 m)
    cell = np.where(comp, (j * 101) % S * R + (max_ring or R) - 1, keys)   # (in the outermost ring: its cells are the widest)
    occ = occurrence(layer * B + cell)
    sector, ring = np.divmod(cell, R)
    r0 = ring * RING + 0.15
    th = (sector + 0.25) * (2 * ka.PI_REF / S) + (occ // 9) * 0.081 / r0
    assert n == 0 or (th <= (sector + 0.75) * (2 * ka.PI_REF / S)).all(), "a cell is too small for its share of a layer"
    r = r0 + 0.08 * (occ % 9)
    z = -4.725 + 0.05 * layer
    pts = np.column_stack([r * np.cos(th), r * np.sin(th), z, 40.0 + cell % 32]).astype(F32)
    order = voxel_order(pts)
    return pts[order], keys[order]


def stride_keys(B, n, step=2003):
    """every key another one for B + 1 elements on end, neighbours in the sequence far apart on the grid (cells of a fine grid are
    smaller than a voxel near the origin: neighbours in key order cannot share a layer of voxels there)"""
    assert np.gcd(step, B + 1) == 1
    return (np.arange(n, dtype=np.int64) * step) % (B + 1)


def scan_sequence(kind, B, n):
    return stride_keys(B, n) if kind == "stride" else sequence(kind, B, n)


def run_scan(g, o, R, S, sc, keys, mkeys, map_kept=True):
    """one step with the designed scan, handed over in a seeded order, on the map of the key sequence mkeys: the three checks"""
    mp = place(R, S, mkeys)
    raw = sc[np.random.default_rng(len(sc)).permutation(len(sc))]
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(raw, I4, I4, I4)
    assert_scan_model(o, ro, R, S, sc, keys)
    assert_model(o, ro, R, S, mp, mkeys, map_kept=map_kept)
    rg = g.step(raw, I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)
    return ro


SCAN_GRIDS = {(8, 8): None, (32, 32): None, (11, 1117): None, (96, 128): 20}  # B + 1 = 65, 1025, 12288 and the radix route (rings folded)
SCAN_SMALL, SCAN_BIG = (QB_TILE - 1, QB_TILE, QB_TILE + 1), (4 * QB_TILE + 1, 9 * QB_TILE + 5)
SCAN_KINDS = ("bucket0", "last_bucket", "complement", "round_robin", "alternating", "ends_only", "runs63", "runs64", "runs65", "runs511",
              "runs512", "runs513")
# (a 0.05 m voxel grid bounds what a cell holds: bucket 0 has room for nine voxels a layer, a cell of the 11 x 1117 grid is one voxel wide
# -- at five and ten tiles a bucket of an outer ring, two buckets in turn, and all buckets at a stride are what fits)
SCAN_BIG_KINDS = {(8, 8): ("last_bucket", "alternating", "stride", "round_robin"), (32, 32): ("last_bucket", "alternating", "stride"),
                  (11, 1117): ("stride",), (96, 128): ("last_bucket", "alternating", "stride")}


def scan_cases():
    out = []
    for (R, S) in SCAN_GRIDS:
        out += [(R, S, "round_robin", n) for n in (0, 1)]
        out += [(R, S, kind, n) for kind in SCAN_KINDS + (("descending",) if R < 96 else ()) for n in SCAN_SMALL]
        out += [(R, S, kind, n) for kind in SCAN_BIG_KINDS[(R, S)] for n in SCAN_BIG]
    return out


def scan_id(R, S, kind, n, version=3):
    return "%dx%d-%s-q%d-v%d-%s" % (R, S, kind, n, version, "standin" if R * S <= 64 and n <= SCAN_BIG[0] and version == 2 else "device")


@pytest.mark.parametrize("R,S,kind,n,version", [pytest.param(*c, v, id=scan_id(*c, v)) for v in (3, 2) for c in scan_cases()])
def test_key_sequences_of_the_voxelised_scan(gpu_mod, R, S, kind, n, version):
    """axis 5: k_qb_hist / k_qb_scan / k_qb_scatter (the radix passes on 96 x 128) on scans of 0, 1, one tile -1 / +0 / +1, 4 tiles + 1
    and 9 tiles + 5 voxels -- tiles 0 .. 9 see every leftover of the sum over the earlier tiles, four at a time.  The map: five points
    of the complement.  v3: a scan bin without map points is LITTLE_NUM and the map is kept; the bucketed scan shows in get_bins(1)
    alone.  v2 with minimum_num_pts = 1: every scan bin joins the map whole (action 3), so map_arranged_ IS the bucketed scan -- the
    model's sc[argsort(keys, stable)] -- followed by the complement"""
    kw = dict(version=2, minimum_num_pts=1) if version == 2 else {}
    g, o, p = pair(gpu_mod, R, S, **kw)
    sc, keys = scan_cloud(R, S, scan_sequence(kind, R * S, n), SCAN_GRIDS[(R, S)])
    assert len(sc) == n
    run_scan(g, o, R, S, sc, keys, [R * S] * 5, map_kept=version == 3)
    if version == 2:
        inh = keys < R * S
        same(o.get_map(), np.concatenate([sc[inh][np.argsort(keys[inh], kind="stable")], place(R, S, [R * S] * 5)]), "the bucketed scan in the map")


V2_CASES = [(R, S, kind, n) for (R, S) in SCAN_GRIDS for kind, n in (("runs63", QB_TILE + 1), ("alternating", QB_TILE - 1), ("runs512", QB_TILE))]


@pytest.mark.parametrize("R,S,kind,n", [pytest.param(*c, id=scan_id(*c, 2)) for c in V2_CASES])
def test_the_bucketed_scan_order_shows_in_the_map_of_v2(gpu_mod, R, S, kind, n):
    """axis 5, v2: a scan bin without map points joins the map whole (action 3), a bin whose map and scan are of like height is merged
    (action 2, scan points first) -- map_arranged_ holds the scan's points in bucketed order.  The map: points in every sixth of the scan's
    bins, so that some bins are scan-only, some are shared.  The model answers for counts and extrema, the oracle for the rest"""
    g, o, p = pair(gpu_mod, R, S, version=2)
    sc, keys = scan_cloud(R, S, scan_sequence(kind, R * S, n), SCAN_GRIDS[(R, S)])
    ro = run_scan(g, o, R, S, sc, keys, np.sort(keys[keys < R * S][::3])[::2], map_kept=False)
    assert ro.n_map_out > ro.n_map_in, "no scan bin joined the map: %r" % (ro.as_dict(),)


# ---------------------------------------------------------------------------------------------
# 6. the radix route's bin offsets (B + 1 > 12288: k_bin_offsets after the LSD passes and k_gather, on both sides)
# ---------------------------------------------------------------------------------------------
XR, XS = 96, 128
XB = XR * XS
OFFSET_CASES = {  # keys of the map (any ring) and of the scan (rings below 20)
    "empty": lambda n: np.zeros(0, np.int64),
    "first_key_above_0": lambda n: 5 + (np.arange(n) * 7) % 1000,
    "last_key_below_B": lambda n: (np.arange(n) * 11) % (XB - 4000),
    "long_gaps": lambda n: np.array([3, 4, 5000, 5001, 12200], np.int64)[(np.arange(n) * 3) % 5],
    "one_key": lambda n: np.full(n, 7000, np.int64),
    "one_key_and_the_complement": lambda n: np.where(np.arange(n) % 5 == 0, XB, 7000),
    "key_0_and_key_B-1": lambda n: np.where(np.arange(n) % 2 == 0, 0, XB - 1),
}


@pytest.mark.parametrize("case", [pytest.param(c, id=c + "-device") for c in OFFSET_CASES])
def test_bin_offsets_of_the_radix_route(gpu_mod, case):
    """axis 6: off[b] for every bucket from sorted keys alone -- no key at all, buckets empty before the first key, behind the last,
    and in long stretches between two keys.  The map: one tile + 1 points of those keys; the scan: 300 voxels of the same keys"""
    g, o, p = pair(gpu_mod, XR, XS)
    mkeys = OFFSET_CASES[case](MB_TILE + 1)
    sc, keys = scan_cloud(XR, XS, OFFSET_CASES[case](300 if len(mkeys) else 0), 20)
    run_scan(g, o, XR, XS, sc, keys, mkeys)


# ---------------------------------------------------------------------------------------------
# 7. one handle, several steps
# ---------------------------------------------------------------------------------------------
def assert_bins_model(o, ro, R, S, z, keys, n_outskirts):
    """checks 1 and 2 for a step away from the origin, where the VoI's x and y are rounded on their way into the body frame and back:
    the lengths, the counts and the extrema (z passes a translation unchanged), whatever the order of the points"""
    (cnt, mn, mx), _, _, _ = model(R, S, np.column_stack([z, z, z]).astype(F32), keys)
    assert (ro.n_voi, ro.n_outskirts, ro.n_ambiguous, ro.n_voxel_overflow) == (len(keys), n_outskirts, 0, 0), ro.as_dict()
    got = o.get_bins(0)
    assert np.array_equal(got[0], cnt) and np.array_equal(got[1], mn) and np.array_equal(got[2], mx), "counts / extrema per bin"


@pytest.mark.parametrize("R,S", [pytest.param(R, S, id="%dx%d-device" % (R, S)) for R, S in LENGTH_GRIDS])
def test_a_table_that_grows_shrinks_and_changes_its_buckets(gpu_mod, R, S):
    """axis 7, by set_map: a VoI of 2 tiles, of 74 tiles, of 2 tiles again (the table's rows beyond the second are stale), then two designs
    on disjoint sets of buckets (stale totals, stale rows), then nothing at all.  (set_map forgets the previous VoI's length: these steps
    size their grids by the table; the next test makes the same jump by pose)"""
    g, o, p = pair(gpu_mod, R, S)
    B = R * S
    even = 2 * (sequence("mixed", B // 2 - 1, 2 * MB_TILE))
    for keys in (sequence("mixed", B, 2 * MB_TILE), sequence("mixed", B, 73 * MB_TILE + 5), sequence("descending", B, 2 * MB_TILE - 3), even, even + 1,
                 np.zeros(0, np.int64), sequence("runs65", B, MB_TILE + 1)):
        run_keys(g, o, R, S, keys)


def pose_at(mod, x):
    T = mod.geopose2eigen([x, 0, 0, 0, 0, 0, 1])
    return T, mod.invert_rigid(T)


@pytest.mark.parametrize("R,S", [pytest.param(R, S, id="%dx%d-device" % (R, S)) for R, S in LENGTH_GRIDS])
def test_a_voi_of_74_tiles_after_one_of_2_takes_the_grid_stride(gpu_mod, R, S):
    """axis 7, by pose: a cluster of 2 tiles at the origin and one of 74 tiles three ranges away, stepped in turn.  bucket_tiles sizes the
    grids from the previous step's VoI -- 64 workgroups after the small cluster -- so k_mb_hist and the scatter walk the large one's 74
    tiles with a grid stride (tiles 64 .. 73 by workgroups 0 .. 9, whose LDS counters hold the first tile's counts).  Four steps as they
    come, then four with both transforms of the next two nodes announced: the table of an overlapped step is filled ahead"""
    g, o, p = pair(gpu_mod, R, S)
    B, dx = R * S, 3 * RING * R
    clusters = [sequence("mixed", B, 2 * MB_TILE), sequence("mixed", B, 73 * MB_TILE + 5)]
    clouds = [place(R, S, k) for k in clusters]
    far = clouds[1].copy()
    far[:, 0] += F32(dx)
    mp = np.concatenate([clouds[0], far])
    g.set_map(mp)
    o.set_map(mp)
    poses = [pose_at(gpu_mod, 0.0), pose_at(gpu_mod, dx)] * 4
    sc = little_scan(R, S)
    for k, (Tb, To) in enumerate(poses):
        if k >= 4:
            for j in ((k, k + 1) if k == 4 else (k + 1,)):
                if j < len(poses):
                    g.prefetch(sc, I4, *poses[j])
        ro = o.step(sc, I4, Tb, To)
        assert_bins_model(o, ro, R, S, clouds[k % 2][:, 2], clusters[k % 2], len(clusters[1 - k % 2]))
        rg = g.step(sc, I4, Tb, To)
        compare_step(g, o, rg, ro, full=True)


# ---------------------------------------------------------------------------------------------
# 8. overlapped steps: B + 2 buckets, the last one for the places a reverted bin has left
# ---------------------------------------------------------------------------------------------
OVERLAP_GRIDS = ((25, 87), (46, 89), (63, 65), (64, 64))  # B + 2 = 2177, 4096, 4097 (scatter and statistics left to the step) and 4098


def reverting_scan(R, S, mkeys, n_bins=40):
    """four voxels, 0.15 m apart in height, in each of the n_bins fullest bins of the map: where the map is more than 0.5 m tall the bin
    is reverted"""
    k, c = np.unique(mkeys[mkeys < R * S], return_counts=True)
    return scan_cloud(R, S, np.repeat(np.sort(k[np.argsort(-c, kind="stable")[:n_bins]]), 4))


def run_two_announced(mod, g, o, R, S, keys, reverting):
    """two announced steps (as test_gpu_scan_ratio.run_two_steps): the designed map at the origin, then the same scan three rings further;
    the map also holds a copy of itself moved by those three rings as far as it lies beyond the first step's range.  Returns (overlapped
    steps launched, taken)"""
    mp = place(R, S, keys)
    sc, skeys = reverting_scan(R, S, keys) if reverting else (little_scan(R, S), None)
    poses = [(I4, I4), pose_at(mod, 3 * RING)]
    far = mp.copy()
    far[:, 0] += F32(3 * RING)
    far = far[np.hypot(far[:, 0].astype(np.float64), far[:, 1].astype(np.float64)) > RING * R + 0.05]
    whole = np.concatenate([mp, far])
    g.set_map(whole)
    o.set_map(whole)
    l0, u0 = g.overlap_counts()
    for Tb, To in poses:
        g.prefetch(sc, I4, Tb, To)
    for k, (Tb, To) in enumerate(poses):
        ro = o.step(sc, I4, Tb, To)
        if k == 0:
            assert len(far) > 0
            assert_model(o, ro, R, S, mp, keys, n_outskirts=len(far), map_kept=not reverting)
            if reverting:
                assert_scan_model(o, ro, R, S, sc, skeys)
                assert ro.n_reverted_bins >= 8, ro.as_dict()
        else:
            assert 0 < ro.n_outskirts and 0 < ro.n_voi, "the second pose keeps a part of the world and leaves a part"
        rg = g.step(sc, I4, Tb, To)
        compare_step(g, o, rg, ro, full=True)
    l1, u1 = g.overlap_counts()
    return l1 - l0, u1 - u0


@pytest.mark.parametrize("reverting", [False, True], ids=["kept", "reverting"])
@pytest.mark.parametrize("R,S,kind", [pytest.param(R, S, kind, id="%dx%d-%s-%s" % (R, S, kind, tag(R, S, 0))) for R, S in OVERLAP_GRIDS for kind in ("mixed", "descending")])
def test_two_announced_steps_bucket_with_a_dead_bucket(gpu_mod, R, S, kind, reverting):
    """axis 8: the second step's table, scatter and statistics are launched beside the first step's per-bin launch, with B + 2 buckets.
    Twice over: a handle that has to grow its scratch between the two steps drops the passes launched ahead, the second time they are
    taken.  `reverting`: the first step reverts bins, whose places in the second step's VoI are dead and go to bucket B + 1"""
    g, o, p = pair(gpu_mod, R, S)
    keys = sequence(kind, R * S, 2 * MB_TILE + 1)
    run_two_announced(gpu_mod, g, o, R, S, keys, reverting)
    launched, taken = run_two_announced(gpu_mod, g, o, R, S, keys, reverting)
    if os.environ.get("ERASOR_HIP_OVERLAP") == "1":
        assert (launched, taken) == (1, 1), (launched, taken)


# ---------------------------------------------------------------------------------------------
# 9. chains that share their launches
# ---------------------------------------------------------------------------------------------
def run_shared_chains(g, o, R, S):
    """seven nodes announced six ahead on a handle that shares chains in fours (chain_batch(4, 1)): a small scan, then scans of 1023, 1024,
    1025 and 4097 voxels -- every voxel of the first three holds three equal points, a chain of fewer than 2049 points is never held
    back -- which form one set (k_qb_hist_b / _scan_b / _scatter_b, k_bin_stats_b: grids sized by the longest), then an empty scan and a
    small one, which go alone.  Returns the (sets, chains) formed"""
    B = R * S
    g.chain_batch(4, 1)
    scans = [(little_scan(R, S), None)]
    for kind, n in (("runs63", QB_TILE - 1), ("alternating", QB_TILE), ("round_robin", QB_TILE + 1), ("stride", 4 * QB_TILE + 1)):
        sc, keys = scan_cloud(R, S, scan_sequence(kind, B, n), SCAN_GRIDS.get((R, S)))
        raw = np.repeat(sc, 3 if n < 2049 else 1, axis=0)
        scans.append((raw[np.random.default_rng(n).permutation(len(raw))], keys))
    scans += [(np.zeros((0, 4), F32), np.zeros(0, np.int64)), (little_scan(R, S), None)]
    mp = place(R, S, sequence("mixed", B, MB_TILE + 1))
    g.set_map(mp)
    o.set_map(mp)
    s0, c0 = g.chain_batch_counts()
    ahead = 6
    for j in range(ahead):
        g.prefetch(scans[j][0], I4, I4, I4)
    for k, (raw, keys) in enumerate(scans):
        if k + ahead < len(scans):
            g.prefetch(scans[k + ahead][0], I4, I4, I4)
        ro = o.step(raw, I4, I4, I4)
        if keys is not None:  # the model: voxels per bin
            assert ro.n_query == len(keys) and ro.n_voxel_overflow == 0 and ro.n_ambiguous == 0, ro.as_dict()
            want = np.bincount(bin_index(R, S, keys[keys < B]), minlength=B)
            assert np.array_equal(o.get_bins(1)[0], want), "scan voxels per bin"
        rg = g.step(raw, I4, I4, I4)
        compare_step(g, o, rg, ro, full=True)
    s1, c1 = g.chain_batch_counts()
    g.chain_batch(2, 3)  # (the handle's defaults)
    return s1 - s0, c1 - c0


@pytest.mark.parametrize("R,S", [pytest.param(8, 8, id="8x8-standin"), pytest.param(32, 32, id="32x32-device"), pytest.param(11, 1117, id="11x1117-device")])
def test_four_chains_in_one_set_of_launches(gpu_mod, R, S):
    """axis 9: each scan is stepped and compared"""
    g, o, p = pair(gpu_mod, R, S)
    sets, chains = run_shared_chains(g, o, R, S)
    if os.environ.get("ERASOR_HIP_OVERLAP") == "1":  # (chains are held back for a set only while the steps overlap)
        assert (sets, chains) == (1, 4), (sets, chains)


# ---------------------------------------------------------------------------------------------
# 10. the same designs in a process whose steps never overlap (ERASOR_HIP_OVERLAP is read once)
# ---------------------------------------------------------------------------------------------
WORKER = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import os
import erasor_amd
if os.environ.get("ERASOR_TEST_SIMT_LIB"):  # (the CPU stand-in build, when the suite itself runs on it)
    erasor_amd.LIB_PATH = os.environ["ERASOR_TEST_SIMT_LIB"]
    erasor_amd._lib = None
import test_gpu_bucketing as T
assert os.environ["ERASOR_HIP_OVERLAP"] == "0"
small = sys.argv[1] == "few"
for R, S in T.OVERLAP_GRIDS[:2] if small else T.TABLE_GRIDS:
    T.test_every_bucket_count_class(erasor_amd, R, S)
for R, S in T.OVERLAP_GRIDS[:1] if small else T.OVERLAP_GRIDS:
    for kind in ("mixed",) if small else ("mixed", "descending"):
        for reverting in (False, True):
            g, o, p = T.pair(erasor_amd, R, S)
            assert T.run_two_announced(erasor_amd, g, o, R, S, T.sequence(kind, R * S, 2 * T.MB_TILE + 1), reverting) == (0, 0)
for R, S, kind, n in T.SEQ_CASES_PLAIN[:6] if small else T.SEQ_CASES_PLAIN:
    T.run_design(erasor_amd, R, S, T.sequence(kind, R * S, n))
g, o, p = T.pair(erasor_amd, 8, 8)
assert T.run_shared_chains(g, o, 8, 8) == (0, 0)
print("WORKER-OK")
"""
SEQ_CASES_PLAIN = [(R, S, kind, MB_TILE + 1) for R, S in SEQ_GRIDS for kind in ("round_robin", "runs65", "runs513", "bucket0", "complement", "in_order")]


@pytest.mark.parametrize("mode", [pytest.param("all", id="all-device"), pytest.param("few", id="few-standin")])
def test_the_same_designs_in_a_process_that_never_overlaps(gpu_mod, tmp_path, mode):
    """ERASOR_HIP_OVERLAP=0: no reserved layout, B + 1 buckets in every step, the dense write-back -- the bucket-count classes, the two
    announced steps, a few key sequences and the chains (which then go one by one)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "bucketing_worker.py"
    script.write_text(WORKER % (root, root))
    out = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=280, env=dict(os.environ, ERASOR_HIP_OVERLAP="0"))
    assert out.returncode == 0 and "WORKER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
