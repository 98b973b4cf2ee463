"""The Scan Ratio Test, the reverted-bin list and the output layouts built from it (kernels.hip.h: srt_first / srt_second, k_bin_stats_srt,
k_srt, k_srt4 / srt4_body, rev_select_call; k_layout / k_layout4; k_assemble_map<FOLD> with its tail workgroups; k_assemble_early;
k_assemble_late) on DESIGNED GRIDS: every bin of an R x S world gets a recipe (point counts and heights of its map and scan cloud), so a
case decides which bins a step reverts, where they sit in key order (key = sector * R + ring) and how many they are.

The code changes path with the number of reverted bins of a step:
  > 32    the dense write-back's 32 tail workgroups loop over the list             (k_assemble_map)
  > 128   several bins per workgroup in the per-bin launch and in k_assemble_late   (ERASOR_REV_GRID)
  > 256   more than one round of k_assemble_late's "thread r takes bin r" prefix; the late table the NEXT overlapped step stages in LDS
          (512 entries = 256 bins) falls back to global memory
  > 1024  ASM_RVMAX: the LDS prefix tables are given up, the prefixes are summed on the fly (k_assemble_map<FOLD> and k_assemble_late)
  B > 4096  k_srt (keys in rounds of 1024 with carries) and k_layout instead of k_srt4 / k_layout4
and with where they sit: srt4_body and rev_select_call give a thread four consecutive keys, read four status bytes as one word unless the
last thread's keys run past B, and take one block scan over 16 wavefronts.

Every case asserts ON THE ORACLE'S numbers that it is the case it claims to be (bin counts equal the design bin for bin, nothing
ambiguous, overflowing or degenerate, the designed bins reverted -- exactly those, in key order); a case whose inputs miss fails, nothing
is skipped.  srt_model restates erasor.cpp:438-595 (v3) and :332-434 (v2) in plain float64 Python from the designed counts and heights
alone, sharing no code with the oracle: a second opinion on the statuses.  Then compare_step(full=True): bit-exact, no tolerances.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import test_oracle_known_answers as ka
from test_gpu_parity import I4, compare_step, gpu_mod, make_pair, same  # noqa: F401  (gpu_mod: the module's fixture)

pytestmark = pytest.mark.gpu

RING = 2.0           # [m] ring width: a bin's map points sit at 0.15 .. 0.85 m of it, its scan points at 1.0 .. 1.6 m, 0.1 m apart -- no two
#                      points of a bin share a 0.05 m voxel whatever the sector's width (ring 0 included), none comes near a ring border
MAP_AT, SCAN_AT = (0.35, 0.45), 0.65   # fractions of the sector angle (map points alternate between two: no collinear bin)
INF_H = 10000000000000.0               # erasor.h: a bin without points has max_h = -INF_H, min_h = +INF_H
LITTLE_NUM, MERGE_BINS, MAP_IS_HIGHER, BLOCKED, CURR_IS_HIGHER = 0.0, 0.25, 0.5, 0.8, 1.0  # (NOT_ASSIGNED == LITTLE_NUM == 0.0)
F32 = np.float32


def up(x):
    return F32(np.nextafter(F32(x), F32(np.inf)))


def down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


# ---------------------------------------------------------------------------------------------
# 1. the designed grid and the independent model
# ---------------------------------------------------------------------------------------------
def bin_(mc, cc, mlo=0.0, mhi=0.0, clo=0.0, chi=0.0):
    """a bin's recipe: map count, scan count, lowest / highest map height, lowest / highest scan height (float32 values)"""
    return (int(mc), int(cc), F32(mlo), F32(mhi), F32(clo), F32(chi))


def heights(n, lo, hi):
    """n float32 heights with minimum lo and maximum hi exactly (n >= 2), all others strictly between: most near lo, one at 0.8 of the span"""
    lo, hi = F32(lo), F32(hi)
    if n == 0:
        return np.zeros(0, F32)
    f = 0.01 * (1 + np.arange(n) % 5)
    if n >= 4:
        f[-2] = 0.8
    z = (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * f).astype(F32)
    z = np.clip(z, lo, hi)
    z[0] = lo
    if n >= 2:
        z[-1] = hi
    return z


def grid_params(R, S, **kw):
    return ka.one_bin_params(num_rings=R, num_sectors=S, max_range=RING * R, **kw)


def grid_world(R, S, design):
    """(map, scan) of an R x S world for identity poses; design: {key: recipe} with key = sector * R + ring (a missing key: an empty bin)"""
    sector_size = 2 * ka.PI_REF / S
    mp, sc = [], []
    for key in sorted(design):
        mc, cc, mlo, mhi, clo, chi = design[key]
        sector, ring = divmod(key, R)
        assert 0 <= sector < S and mc <= 8 and cc <= 7
        lab = F32(40 + key % 32)
        for n, lo, hi, out, r0 in ((mc, mlo, mhi, mp, 0.15), (cc, clo, chi, sc, 1.0)):
            i = np.arange(n)
            r = ring * RING + r0 + 0.1 * i
            at = np.where(i % 2 == 0, MAP_AT[0], MAP_AT[1]) if out is mp else np.full(n, SCAN_AT)
            th = (sector + at) * sector_size
            out.append(np.column_stack([r * np.cos(th), r * np.sin(th), heights(n, lo, hi), np.full(n, lab)]))
    cat = lambda a: np.concatenate(a).astype(F32) if a else np.zeros((0, 4), F32)  # noqa: E731
    return cat(mp), cat(sc)


def srt_model(params, design):
    """(status of every bin indexed ring * S + sector, the reverted keys in key order) -- erasor.cpp:438-595 (v3), :332-434 (v2) restated
    from the designed counts and heights: C++ double arithmetic (0/0 = NaN, x/0 = inf, std::min(a, b) = b < a ? b : a)"""
    R, S, v3 = params.num_rings, params.num_sectors, params.version == 3
    thr, minimum = float(params.scan_ratio_threshold), int(params.minimum_num_pts)
    first = {}
    with np.errstate(all="ignore"):
        for key, (mc, cc, mlo, mhi, clo, chi) in design.items():
            m_max, m_min = (np.float64(mhi if mc > 1 else mlo), np.float64(mlo)) if mc else (np.float64(-INF_H), np.float64(INF_H))
            c_max, c_min = (np.float64(chi if cc > 1 else clo), np.float64(clo)) if cc else (np.float64(-INF_H), np.float64(INF_H))
            st, revert = LITTLE_NUM, False
            if (mc > 0 or not v3) and cc >= minimum:  # (v3: an empty map bin is LITTLE_NUM before anything else, :454)
                md, cd = m_max - m_min, c_max - c_min
                a, b = md / cd, cd / md
                ratio = b if b < a else a
                if cc > 0 and mc > 0:
                    if ratio < thr:
                        if md >= cd:
                            st = MAP_IS_HIGHER
                            revert = (md > 0.5) if v3 else (m_max > params.th_bin_max_h)
                        elif md <= cd:
                            st = CURR_IS_HIGHER
                    else:
                        st = MERGE_BINS
            first[key] = (st, revert)
    status = np.zeros(R * S, np.float64)
    for key, (st, revert) in first.items():
        sector, ring = divmod(key, R)
        if v3 and st == MAP_IS_HIGHER and not revert:
            st = LITTLE_NUM  # NOT_ASSIGNED (:537)
        if v3 and st == MERGE_BINS:
            # is_dynamic_obj_close(r, theta, 1, 1), :573-595: theta wraps by num_RINGS (kept); a candidate outside [0, S) is skipped
            cand = [j + R if j < 0 else (j - R if j >= S else j) for j in (sector - 1, sector, sector + 1)]
            for r in range(max(0, ring - 1), min(ring + 1, R - 1) + 1):
                for t in cand:
                    if (r == ring and t == sector) or t < 0 or t >= S:
                        continue
                    if first.get(t * R + r, (LITTLE_NUM, False))[0] == CURR_IS_HIGHER:
                        st = BLOCKED
        status[ring * S + sector] = st
    return status, sorted(k for k, (_, rv) in first.items() if rv)


def bin_index(R, S, keys):
    keys = np.asarray(keys, np.int64)
    return (keys % R) * S + keys // R


def assert_designed(o, ro, params, design, degenerate_ok=False):
    """the oracle's own numbers say that this step is the designed one; returns the model's reverted keys"""
    R, S = params.num_rings, params.num_sectors
    want = np.zeros((2, R * S), np.uint32)
    for key, rec in design.items():
        want[:, bin_index(R, S, key)] = rec[:2]
    for w in (0, 1):
        got = o.get_bins(w)[0]
        assert np.array_equal(got, want[w]), ("points per bin, cloud %d" % w, np.flatnonzero(got != want[w])[:8].tolist())
    assert ro.n_ambiguous == 0 and ro.n_voxel_overflow == 0, ro.as_dict()
    assert degenerate_ok or ro.n_degenerate_plane == 0, ro.as_dict()
    status, rev = srt_model(params, design)
    assert ro.n_reverted_bins == len(rev), (ro.n_reverted_bins, len(rev))
    assert np.array_equal(o.get_planes()[0], bin_index(R, S, rev)), "the reverted bins, in key order"
    st = o.get_status()
    assert np.array_equal(st, status), ("model and oracle disagree on bins", np.flatnonzero(st != status)[:8].tolist())
    return rev


# recipes -------------------------------------------------------------------------------------
def rev(k=0):       # ratio 0, the map higher, taller than 0.5 m (v3) and above th_bin_max_h = 0.75 (v2): REVERTED
    return bin_(5 + k % 3, 3 + k % 2, 0.0, 1.0 + 0.125 * (k % 4), 0.25, 0.25)


OTHERS = {  # what a bin that is not reverted may be (minimum_num_pts = 3, scan_ratio_threshold = 0.3)
    "little": lambda k: bin_(4 + k % 3, 2, 0.0, 1.0, 0.0, 0.0),         # cc < minimum_num_pts: LITTLE_NUM
    "merge": lambda k: bin_(4 + k % 3, 3 + k % 2, 0.0, 1.0, 0.0, 0.75),  # ratio 0.75: MERGE_BINS, or BLOCKED beside a CURR_IS_HIGHER bin
    "curr": lambda k: bin_(4 + k % 3, 3 + k % 3, 0.0, 0.125, 0.0, 1.5),  # the scan higher (v2: above th_bin_max_h, rejected)
    "low": lambda k: bin_(4 + k % 3, 3, 0.0, 0.5 - 0.125 * (k % 3), 0.0, 0.0),  # the map higher, but <= 0.5 m: NOT_ASSIGNED (v2: kept)
    "map_only": lambda k: bin_(1 + k % 4, 0, 0.0, 0.5),
    "scan_only": lambda k: bin_(0, 3 + k % 2, 0.0, 0.0, 0.0, 0.5),      # dropped (v3) / taken into the map (v2)
    "empty": lambda k: None,
}
OTHER_NAMES = ("little", "merge", "merge", "merge", "curr", "low", "low", "map_only", "scan_only", "empty")


def mixed_design(R, S, rev_keys, seed=5):
    """rev_keys reverted, every other bin a seeded mix of the other outcomes"""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(OTHER_NAMES), R * S)
    rev_keys = set(int(k) for k in rev_keys)
    design = {}
    for key in range(R * S):
        rec = rev(key) if key in rev_keys else OTHERS[OTHER_NAMES[pick[key]]](key)
        if rec is not None:
            design[key] = rec
    return design


# handles: one per grid and parameter variant ---------------------------------------------------
_pairs = {}


def pair(gpu_mod, R, S, profiled=False, **kw):
    key = (R, S, profiled) + tuple(sorted(kw.items()))
    if key not in _pairs:
        g, o = make_pair(gpu_mod, grid_params(R, S, **kw))
        if profiled:
            g.profiling(1)
        _pairs[key] = (g, o, grid_params(R, S, **kw))
    return _pairs[key]


def run_design(gpu_mod, R, S, design, profiled=False, degenerate_ok=False, **kw):
    g, o, p = pair(gpu_mod, R, S, profiled, **kw)
    mp, sc = grid_world(R, S, design)
    g.set_map(mp)
    o.set_map(mp)
    ro = o.step(sc, I4, I4, I4)
    rev_keys = assert_designed(o, ro, p, design, degenerate_ok)
    rg = g.step(sc, I4, I4, I4)
    compare_step(g, o, rg, ro, full=True)
    return g, o, rg, ro, rev_keys


# ---------------------------------------------------------------------------------------------
# 2. decision edges, on a grid
# ---------------------------------------------------------------------------------------------
ER, ES = 6, 10
TH_MAX_H = 0.75
H3, H8 = F32(0.3), F32(F32(0.3) + F32(0.5))  # two float32 heights, neither a round number, whose float64 difference is exactly 0.5
assert float(H8) - float(H3) == 0.5 and float(up(H8)) - float(H3) > 0.5
# (name, recipe, status v3, reverted v3, status v2, reverted v2) with minimum_num_pts = 3, scan_ratio_threshold = 0.25, th_bin_max_h = 0.75;
# a "merge" of v3 may turn BLOCKED beside a CURR_IS_HIGHER bin (the model says where)
EDGES = (
    ("cc_below_minimum", bin_(5, 2, 0, 1, 0, 0), LITTLE_NUM, 0, LITTLE_NUM, 0),
    ("cc_at_minimum", bin_(5, 3, 0, 1, 0, 0), MAP_IS_HIGHER, 1, MAP_IS_HIGHER, 1),
    ("scan_without_map", bin_(0, 4, 0, 0, 0, 1), LITTLE_NUM, 0, LITTLE_NUM, 0),          # v2: action 3, the scan points join the map
    ("map_without_scan", bin_(5, 0, 0, 1), LITTLE_NUM, 0, LITTLE_NUM, 0),
    ("ratio_at_threshold", bin_(5, 4, 0, 1, 0, 0.25), MERGE_BINS, 0, MERGE_BINS, 0),     # 0.25 < 0.25 is false
    ("ratio_below_threshold", bin_(5, 4, 0, 1, 0, down(0.25)), MAP_IS_HIGHER, 1, MAP_IS_HIGHER, 1),
    ("ratio_above_threshold", bin_(5, 4, 0, 1, 0, up(0.25)), MERGE_BINS, 0, MERGE_BINS, 0),
    ("ratio_at_threshold_scan_higher", bin_(5, 4, 0, 0.25, 0, 1), MERGE_BINS, 0, MERGE_BINS, 0),
    ("ratio_below_threshold_scan_higher", bin_(5, 4, 0, down(0.25), 0, 1), CURR_IS_HIGHER, 0, CURR_IS_HIGHER, 0),
    ("ratio_above_threshold_scan_higher", bin_(5, 4, 0, up(0.25), 0, 1), MERGE_BINS, 0, MERGE_BINS, 0),
    ("equal_spans", bin_(5, 5, 0.125, 0.875, 0.25, 1.0), MERGE_BINS, 0, MERGE_BINS, 0),  # ratio 1 (v2: action 2)
    ("flat_scan", bin_(6, 3, 0, 1, 0.5, 0.5), MAP_IS_HIGHER, 1, MAP_IS_HIGHER, 1),        # ratio 0
    ("flat_map", bin_(6, 3, 0.5, 0.5, 0, 1), CURR_IS_HIGHER, 0, CURR_IS_HIGHER, 0),       # ratio 0 (v2: action 4, chi = 1 > 0.75)
    ("both_flat", bin_(4, 4, 0.25, 0.25, 0.5, 0.5), MERGE_BINS, 0, MERGE_BINS, 0),        # 0 / 0: NaN < thr is false
    ("gate_exactly_half_a_metre", bin_(6, 3, H3, H8, 0, 0), LITTLE_NUM, 0, MAP_IS_HIGHER, 1),      # NOT_ASSIGNED; v2: 0.8 > 0.75
    ("gate_one_step_above", bin_(6, 3, H3, up(H8), 0, 0), MAP_IS_HIGHER, 1, MAP_IS_HIGHER, 1),
    ("map_top_at_th_bin_max_h", bin_(6, 3, 0.125, TH_MAX_H, 0, 0), MAP_IS_HIGHER, 1, MAP_IS_HIGHER, 0),   # v2 action 1: 0.75 > 0.75 is false
    ("map_top_one_step_above", bin_(6, 3, 0.125, up(TH_MAX_H), 0, 0), MAP_IS_HIGHER, 1, MAP_IS_HIGHER, 1),
    ("scan_top_at_th_bin_max_h", bin_(5, 4, 0, 0.125, -0.5, TH_MAX_H), CURR_IS_HIGHER, 0, CURR_IS_HIGHER, 0),  # v2 action 4: not rejected
    ("scan_top_one_step_above", bin_(5, 4, 0, 0.125, -0.5, up(TH_MAX_H)), CURR_IS_HIGHER, 0, CURR_IS_HIGHER, 0),  # rejected
)
EDGE_KW = dict(scan_ratio_threshold=0.25, th_bin_max_h=TH_MAX_H)
EDGE_OFFSETS = (0, 3, 7, 11, 13, 18)


def edge_design(offset):
    """the recipes laid over the whole grid, one after the other from key `offset` on: every edge bin has eight neighbours' worth of
    other edge bins around it, and over the offsets every recipe visits ring 0, ring R - 1, sector 0, sector S - 1 and the interior"""
    return {key: EDGES[(key + offset) % len(EDGES)][1] for key in range(ER * ES)}


def places(R, S, keys):
    out = set()
    for k in keys:
        s, r = divmod(k, R)
        out |= {"ring0"} if r == 0 else set()
        out |= {"ringR"} if r == R - 1 else set()
        out |= {"sector0"} if s == 0 else set()
        out |= {"sectorS"} if s == S - 1 else set()
        out |= {"interior"} if 0 < r < R - 1 and 0 < s < S - 1 else set()
    return out


def test_every_edge_recipe_visits_every_kind_of_place():
    for e in range(len(EDGES)):
        keys = [k for off in EDGE_OFFSETS for k in range(ER * ES) if (k + off) % len(EDGES) == e]
        assert places(ER, ES, keys) == {"ring0", "ringR", "sector0", "sectorS", "interior"}, EDGES[e][0]


@pytest.mark.parametrize("offset", [pytest.param(x, id="offset%d-standin" % x) for x in EDGE_OFFSETS])
@pytest.mark.parametrize("version", [3, 2])
def test_decision_edges_on_a_grid(gpu_mod, version, offset):
    """every edge of the Scan Ratio Test and of the two revert gates, each stated with the outcome derived by hand (EDGES), on a 6 x 10
    grid full of such bins; the model and the oracle agree with the hand-derived outcome, the device with the oracle"""
    design = edge_design(offset)
    g, o, rg, ro, rev_keys = run_design(gpu_mod, ER, ES, design, version=version, **EDGE_KW)
    st = o.get_status()
    for key in range(ER * ES):
        name, _, st3, rv3, st2, rv2 = EDGES[(key + offset) % len(EDGES)]
        want, rv = (st3, rv3) if version == 3 else (st2, rv2)
        got = st[bin_index(ER, ES, key)]
        assert got == want or (version == 3 and want == MERGE_BINS and got == BLOCKED), (name, key, got, want)
        assert (key in rev_keys) == bool(rv), (name, key)
    gate = [k for k in range(ER * ES) if EDGES[(k + offset) % len(EDGES)][0].startswith("gate_")]
    assert len(gate) >= 4 and min(gate) > 0, "the gate's bins are not key 0"
    if version == 2:  # action 2: the merged bin holds the scan points first, then the map points (erasor.cpp:296-307)
        e = [x[0] for x in EDGES].index("equal_spans")
        key = next(k for k in range(ER * ES) if (k + offset) % len(EDGES) == e)
        mp, sc = grid_world(ER, ES, {key: design[key]})
        m = o.get_map()
        at = int(np.flatnonzero((m == sc[0]).all(1))[0])
        same(m[at:at + len(sc) + len(mp)], np.concatenate([sc, mp]), "a merged bin in the map: scan points, then map points")
        # action 4: the scan points of the CURR_IS_HIGHER bins above th_bin_max_h, and only those, are in curr_rejected
        want = sum(rec[1] for _, rec, _, _, st2, _ in (EDGES[(k + offset) % len(EDGES)] for k in range(ER * ES))
                   if st2 == CURR_IS_HIGHER and rec[5] > F32(TH_MAX_H))
        assert len(o.get_cloud(5)) == want > 0


@pytest.mark.parametrize("version", [pytest.param(3, id="v3-standin"), pytest.param(2, id="v2-standin")])
def test_minimum_num_pts_zero_with_an_empty_scan_bin(gpu_mod, version):
    """minimum_num_pts = 0, cc = 0: the scan bin's heights are -/+INF_H, the quotients -0 and -inf, and the ratio is below every threshold
    -- the bin stays LITTLE_NUM because the scan bin is not occupied (erasor.cpp:469, 479); between bins that do decide"""
    design = {key: (bin_(5, 0, 0, 1) if key % 7 == 0 else EDGES[key % len(EDGES)][1]) for key in range(ER * ES)}
    g, o, rg, ro, rev_keys = run_design(gpu_mod, ER, ES, design, version=version, minimum_num_pts=0, **EDGE_KW)
    st = o.get_status()
    assert all(st[bin_index(ER, ES, key)] == LITTLE_NUM and key not in rev_keys for key in range(0, ER * ES, 7))
    assert places(ER, ES, range(0, ER * ES, 7)) == {"ring0", "ringR", "sector0", "sectorS", "interior"}


# MERGE beside CURR_IS_HIGHER -----------------------------------------------------------------
MERGE_REC, CURR_REC, FILL_REC = bin_(5, 4, 0, 1, 0, 0.75), bin_(5, 4, 0, 0.125, 0, 1.5), bin_(3, 0, 0, 0.25)
NEIGHBOUR_GRIDS = ((15, 60), (8, 8), (12, 5), (5, 1), (1, 1))  # R < S, R == S, R > S: the reference's wrap by num_rings leaves [0, S)


def neighbour_cases():
    """(R, S, merge (ring, sector), curr (ring, sector) or None): the eight neighbours of a bin in the centre; a bin at sector 0 and at
    sector S - 1 with the CURR_IS_HIGHER bin where a correct wrap would look, where the reference's wrap by num_rings looks, and beside"""
    out = []
    for R, S in NEIGHBOUR_GRIDS:
        rc, sc = R // 2, S // 2
        cases = [((rc, sc), None)]
        if R >= 3 and S >= 3:
            cases += [((rc, sc), (rc + dr, sc + ds)) for dr in (-1, 0, 1) for ds in (-1, 0, 1) if (dr, ds) != (0, 0)]
        for s0 in sorted({0, S - 1}):
            look = {(s0 - 1) % S, (s0 + 1) % S}                                       # a correct wrap
            look |= {t for t in (s0 - 1 + R, s0 + 1 - R, s0 - 1, s0 + 1) if 0 <= t < S}  # the reference's, and no wrap at all
            look |= {R - 1, S - R} & set(range(S))
            for t in sorted(look):
                for r in sorted({rc, min(rc + 1, R - 1), max(rc - 1, 0)}):
                    if (r, t) != (rc, s0):
                        cases.append(((rc, s0), (r, t)))
        out += [(R, S, m, c) for m, c in dict.fromkeys(cases)]
    return out


def _nid(c):
    R, S, m, cu = c
    return "%dx%d-merge%d.%d-curr%s-standin" % (R, S, m[0], m[1], "%d.%d" % cu if cu else "none")


@pytest.mark.parametrize("case", [pytest.param(c, id=_nid(c)) for c in neighbour_cases()])
def test_a_merge_candidate_beside_a_bin_where_the_scan_is_higher(gpu_mod, case):
    """is_dynamic_obj_close is kept bug-compatible (theta wraps by num_rings) and skips a wrapped candidate outside [0, S), where the
    reference reads out of bounds: one merge candidate, one CURR_IS_HIGHER bin, every other bin a plain map bin.  Whether the candidate is
    BLOCKED is derived here from the rule itself, then asked of the model, the oracle and the device."""
    R, S, (mr, ms), cu = case
    design = {key: FILL_REC for key in range(R * S)}
    design[ms * R + mr] = MERGE_REC
    blocked = False
    if cu is not None:
        design[cu[1] * R + cu[0]] = CURR_REC
        thetas = [ms - 1 + R if ms - 1 < 0 else ms - 1, ms, ms + 1 - R if ms + 1 >= S else ms + 1]
        blocked = abs(cu[0] - mr) <= 1 and cu[1] in thetas
    g, o, rg, ro, rev_keys = run_design(gpu_mod, R, S, design)
    assert o.get_status()[mr * S + ms] == (BLOCKED if blocked else MERGE_BINS), (case, blocked)
    assert rev_keys == []


# ---------------------------------------------------------------------------------------------
# 3. positions of the reverted bins in key order
# ---------------------------------------------------------------------------------------------
POSITION_GRIDS = ((64, 64), (7, 11), (9, 10), (13, 7), (1, 4), (1, 1))  # B = 4096, and B mod 4 = 1, 2, 3, 0, 1


def position_patterns(B):
    """{name: keys}; a pattern that needs keys the grid has not got is left out"""
    rng = np.random.default_rng(B)
    pats = {
        "none": [], "key0": [0], "last_key": [B - 1], "last_word": list(range((B - 1) // 4 * 4, B)), "all": list(range(B)),
        "every_second": list(range(0, B, 2)), "odd": list(range(1, B, 2)), "3mod4": list(range(3, B, 4)), "0mod4": list(range(0, B, 4)),
        "3and4mod4": sorted(set(range(3, B, 4)) | set(range(4, B, 4))),
        "255_256_257": [255, 256, 257], "1023_1024_1025": [1023, 1024, 1025], "every_256th": list(range(0, B, 256)),
        "every_256th_from_255": list(range(255, B, 256)), "random_third": sorted(rng.choice(B, B // 3, replace=False).tolist()),
    }
    return {n: k for n, k in pats.items() if all(x < B for x in k) and (k or n == "none") and not (n.startswith("every_256") and B <= 256)}


POSITION_CASES = [pytest.param(R, S, n, id="%dx%d-%s-%s" % (R, S, n, "standin" if R * S < 4096 else "device"))
                  for R, S in POSITION_GRIDS for n in position_patterns(R * S)]


@pytest.mark.parametrize("R,S,pattern", POSITION_CASES)
def test_reverted_bins_at_chosen_keys(gpu_mod, R, S, pattern):
    """the reverted bins exactly at the pattern's keys, the other bins a seeded mix of the other outcomes (out_off0 / out_offR / crej_off
    have something to count); v3, on the suite's overlapped path rev_select_call finds them"""
    keys = position_patterns(R * S)[pattern]
    g, o, rg, ro, rev_keys = run_design(gpu_mod, R, S, mixed_design(R, S, keys))
    assert rev_keys == keys


# ---------------------------------------------------------------------------------------------
# 4. list lengths around every threshold, through every launch variant
# ---------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4096)
LENGTHS_BIG, LENGTHS_V2 = (1, 129, 1025, 4200), (33, 129, 1025)
STANDIN_MAX = 129


@functools.lru_cache(maxsize=None)
def length_design(R, S, n_rev):
    keys = np.sort(np.random.default_rng(1000 + n_rev).choice(R * S, n_rev, replace=False))
    return mixed_design(R, S, keys.tolist(), seed=7)


def _lid(R, S, n, version=3):
    return "%dx%d-v%d-n%d-%s" % (R, S, version, n, "standin" if n <= STANDIN_MAX and R * S <= 4096 else "device")


LENGTH_CASES = ([pytest.param(64, 64, 3, n, id=_lid(64, 64, n)) for n in LENGTHS] + [pytest.param(70, 60, 3, n, id=_lid(70, 60, n)) for n in LENGTHS_BIG] +
                [pytest.param(64, 64, 2, n, id=_lid(64, 64, n, 2)) for n in LENGTHS_V2])


def length_kw(version):
    return dict(version=2, th_bin_max_h=TH_MAX_H) if version == 2 else {}


@pytest.mark.parametrize("R,S,version,n_rev", LENGTH_CASES)
def test_list_lengths_in_one_step(gpu_mod, R, S, version, n_rev):
    """variant a: the suite's default -- overlapped: the reserved layout, k_assemble_early, the self-selecting per-bin launch, k_assemble_late"""
    g, o, rg, ro, rev_keys = run_design(gpu_mod, R, S, length_design(R, S, n_rev), **length_kw(version))
    assert len(rev_keys) == n_rev == ro.n_reverted_bins


@pytest.mark.parametrize("R,S,version,n_rev", LENGTH_CASES)
def test_list_lengths_with_every_launch_on_its_own(gpu_mod, R, S, version, n_rev):
    """variant c: erasor_hip_profiling(1) -- k_srt4 with st1_in as a launch of its own, k_rgpf2 / k_binvox2, k_layout4, the dense
    k_assemble_map without FOLD"""
    g, o, rg, ro, rev_keys = run_design(gpu_mod, R, S, length_design(R, S, n_rev), profiled=True, **length_kw(version))
    assert len(rev_keys) == n_rev == ro.n_reverted_bins


def shifted_pose(mod, rings=3):
    T = mod.geopose2eigen([rings * RING, 0, 0, 0, 0, 0, 1])
    return T, mod.invert_rigid(T)


def run_two_steps(mod, g, o, p, R, S, design):
    """two announced steps: the designed one at the origin, then the same scan from a pose three rings further -- some of the first step's
    reverted bins leave the VoI, others stay.  The map also holds a copy of itself moved by those three rings, as far as the copy lies
    beyond the first step's range: outskirts of the first step that the second finds exactly where its scan expects the designed bins,
    so bins are reverted there and their rejected points have source indices behind every entry of the late table.  Both nodes are
    announced with both transforms before the first step.  Returns (overlapped steps launched, taken)"""
    mp, sc = grid_world(R, S, design)
    poses = [(I4, I4), shifted_pose(mod)]
    far = mp.copy()
    far[:, 0] += F32(poses[1][0][3])
    far = far[np.hypot(far[:, 0].astype(np.float64), far[:, 1].astype(np.float64)) > RING * R + 0.05]
    mp = np.concatenate([mp, far])
    g.set_map(mp)
    o.set_map(mp)
    l0, u0 = g.overlap_counts()
    for Tb, To in poses:
        g.prefetch(sc, I4, Tb, To)
    for k, (Tb, To) in enumerate(poses):
        ro = o.step(sc, I4, Tb, To)
        if k == 0:
            assert_designed(o, ro, p, design)
            assert ro.n_outskirts == len(far) > 0
            behind = ro.n_static_estimate + ro.n_complement  # (where the outskirts begin in the map this step leaves)
        else:
            assert 0 < ro.n_outskirts and 0 < ro.n_voi, "the second pose keeps a part of the world and leaves a part"
            if len(srt_model(p, design)[1]) >= 255:  # (a list that long has members in the thin strip of former outskirts)
                assert ro.n_map_rejected > 0 and o.get_rejected_indices().max() >= behind, "no rejected point came out of the former outskirts"
        rg = g.step(sc, I4, Tb, To)
        compare_step(g, o, rg, ro, full=True)
        same(g.get_map(), o.get_map(), "map after step %d" % k)
    l1, u1 = g.overlap_counts()
    return l1 - l0, u1 - u0


@pytest.mark.parametrize("R,S,version,n_rev", [pytest.param(R, S, 3, n, id="%dx%d-n%d-%s" % (R, S, n, "standin" if (R, n) in ((64, 33), (64, 129)) else "device"))
                                               for R, S, ns in ((64, 64, LENGTHS), (70, 60, LENGTHS_BIG)) for n in ns])
def test_list_lengths_in_two_announced_steps(gpu_mod, R, S, version, n_rev):
    """variant b: the doubled reservations, k_late_gather, and the second step's conversion of source indices through a late table of
    2 * n_rev entries -- in LDS up to 256 bins, in global memory beyond.  Twice over: a handle that has to grow its scratch between the
    two steps drops the passes launched ahead; the second time round they are taken"""
    g, o, p = pair(gpu_mod, R, S)
    design = length_design(R, S, n_rev)
    run_two_steps(gpu_mod, g, o, p, R, S, design)
    launched, taken = run_two_steps(gpu_mod, g, o, p, R, S, design)
    if os.environ.get("ERASOR_HIP_OVERLAP") == "1":  # (more than 4096 bins: no reserved layout, so no step is overlapped)
        assert (launched, taken) == ((1, 1) if R * S <= 4096 else (0, 0)), (launched, taken)


WORKER = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r + "/tests")
import os
import erasor_amd
if os.environ.get("ERASOR_TEST_SIMT_LIB"):  # (the CPU stand-in build, when the suite itself runs on it)
    erasor_amd.LIB_PATH = os.environ["ERASOR_TEST_SIMT_LIB"]
    erasor_amd._lib = None
elif os.environ.get("ALT_HOOKS_LIB"):       # (the product's sources with the test hooks compiled in: ERASOR_HIP_LEAVE_ALL is one)
    import subprocess
    import hooks
    subprocess.check_call(["make", "-C", os.path.join(os.path.dirname(os.path.dirname(hooks.HOOKS_LIB)), "..", "erasor_amd", "csrc"), "-s", "hooks"])
    erasor_amd.LIB_PATH = hooks.HOOKS_LIB
    erasor_amd._lib = None
import test_gpu_scan_ratio as T
lengths = [int(x) for x in sys.argv[2].split(",")]
if sys.argv[1].startswith("no_overlap"):
    assert os.environ["ERASOR_HIP_OVERLAP"] == "0"
    more = sys.argv[1] == "no_overlap_all"  # (the grid of more than 4096 bins and v2 as well)
    for R, S, version, ns in ((64, 64, 3, lengths), (70, 60, 3, T.LENGTHS_BIG if more else ()), (64, 64, 2, T.LENGTHS_V2 if more else ())):
        for n in ns:
            g, o, rg, ro, rev_keys = T.run_design(erasor_amd, R, S, T.length_design(R, S, n), **T.length_kw(version))
            assert len(rev_keys) == n
    assert g.overlap_counts()[1] == 0
else:
    assert os.environ["ERASOR_HIP_OVERLAP"] == "1" and os.environ["ERASOR_HIP_LEAVE_ALL"] == "1"
    g, o, p = T.pair(erasor_amd, 64, 64)
    for n in lengths:
        T.run_two_steps(erasor_amd, g, o, p, 64, 64, T.length_design(64, 64, n))
        launched, taken = T.run_two_steps(erasor_amd, g, o, p, 64, 64, T.length_design(64, 64, n))
        assert (launched, taken) == (1, 1), (n, launched, taken)
print("WORKER-OK")
"""


def run_worker(tmp_path, mode, lengths, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "scan_ratio_worker.py"
    script.write_text(WORKER % (root, root))
    out = subprocess.run([sys.executable, str(script), mode, ",".join(str(n) for n in lengths)], capture_output=True, text=True, timeout=280,
                         env=dict(os.environ, **env))
    assert out.returncode == 0 and "WORKER-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.parametrize("mode,lengths", [pytest.param("no_overlap_all", LENGTHS, id="all-device"),
                                          pytest.param("no_overlap", (0, 1, 32, 33, 129), id="few-standin")])
def test_list_lengths_in_a_process_that_never_overlaps(gpu_mod, tmp_path, mode, lengths):
    """variant d: ERASOR_HIP_OVERLAP=0 is read once, so in a process of its own, one for the whole list: the extra last workgroup of
    k_revert_bins_srt and the dense k_assemble_map<FOLD> with its 32 tail workgroups -- the only place where the tail loop (> 32 bins) and
    its ASM_RVMAX fallback (> 1024) run"""
    run_worker(tmp_path, mode, lengths, {"ERASOR_HIP_OVERLAP": "0"})


@pytest.mark.parametrize("lengths", [pytest.param((129, 1025), id="129-1025-device")])
def test_two_announced_steps_where_every_reverted_bin_may_leave(gpu_mod, tmp_path, lengths):
    """variant b with the hooks build's ERASOR_HIP_LEAVE_ALL=1: every reverted bin reserves places in the outskirts' order"""
    run_worker(tmp_path, "leave_all", lengths, {"ERASOR_HIP_OVERLAP": "1", "ERASOR_HIP_LEAVE_ALL": "1", "ALT_HOOKS_LIB": "1"})
