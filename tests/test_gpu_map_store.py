"""The MAP STORE at every chunk boundary and on both chunk-scan paths: k_voi_split, k_chunk_scan_one / _local / _top, k_voi_gather,
k_late_gather, k_o_commit, the OMeta chunk records and rebuild_outskirts (kernels.hip.h, the map chain of erasor_hip.hip).

The store is two regions of 1024-entry chunks (16 tiles of 64): the VoI-resident region F (dense float4, nF entries) and the outskirts
(right-aligned in a buffer of capO entries, tombstones where points entered a VoI, leaving points prepended in front of o_begin).  Which
code runs -- and which rank a point gets -- depends on where nF, o_begin and the chunk counts fall relative to 1, 4, 16, 64, 256 and 1024.
Every case here is an ordinary call sequence on a SYNTHETIC map built to order, and is compared with two references:

  * the CPU oracle, bit for bit (compare_step(full=True): map_voi pins the VoI order, get_map() the order of what left);
  * a few lines of numpy float64: a map point is inside iff (x - xc)^2 + (y - yc)^2 < r^2 (OMU.cpp:394, strict), which gives n_voi,
    n_outskirts and -- cases (e) -- the physical layout of the outskirts: [leaving points, in F order | the old entries, tombstones
    where points entered], dense and right-aligned (o_begin = capO - n_valid) after a rebuild.

Coordinates are odd multiples of 1/512 below 128 and the poses integer translations: the float32 round trip map -> body -> map is
exact, a point never moves, and nothing lies on a sector edge (1 ring x 4 sectors: the axes).  Most scans are empty or a few points in
a quadrant without map points: nothing reverts, and a step is VoI extraction, the round trip and reassembly.  No tolerance appears
anywhere in this file.  Ids of cases whose store has at most ~70 k entries contain `standin`: tests/test_full_step_on_cpu.py re-runs
them against the CPU stand-in of the HIP runtime (ERASOR_SIMT_MORE=1).
"""
import functools

import numpy as np
import pytest

import hooks
import test_oracle_known_answers as ka
from test_gpu_parity import I4, compare_step, make_pair, same  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK, TILE, GATHER_PIECE = 1024, 64, 256  # (kernels.hip.h: CHUNK, TILE, CHUNK_TILES / GATHER_SUB tiles)
R = 8.0                                    # the VoI radius of every case but (d)
EMPTY = np.zeros((0, 4), np.float32)
LABELS = np.array([40.0, 44.0, 48.0, 50.0, 70.0, 71.0, 252.0, 259.0], np.float32)  # (static and dynamic: the label tallies move with the points)


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()
    with hooks.hooks_library():
        yield erasor_amd
        # (the handles shared by the cases belong to the hooks build: they go before the package turns back to the product library)
        for g, _ in _pairs.values():
            g.close()
        _pairs.clear()
        _oracle_runs.cache_clear()


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def block(n, x0, y0=0.0, width=1024, tag=0):
    """n distinct points on a lattice of pitch 1/256 whose first point is (x0, y0) + 1/512, `width` to a row: x0 <= x < x0 + width / 256"""
    i = np.arange(n, dtype=np.int64)
    x = x0 + (2 * (i % width) + 1) / 512.0
    y = y0 + (2 * (i // width) + 1) / 512.0
    pts = np.column_stack([x, y, np.full(n, 0.5), LABELS[(i + tag) % len(LABELS)]]).astype(np.float32)
    assert np.array_equal(pts[:, 0].astype(np.float64), x) and np.array_equal(pts[:, 1].astype(np.float64), y), "not exact in float32"
    return pts


def pose(x, y):
    import erasor_amd
    Tb = erasor_amd.geopose2eigen([float(x), float(y), 0, 0, 0, 0, 1])
    return np.ascontiguousarray(Tb, np.float32), np.ascontiguousarray(erasor_amd.invert_rigid(Tb), np.float32)


def inside(pts, T, r=R):
    """the model: OMU.cpp:394 in float64, centre and radius as the oracle derives them (T_b2o[3], T_b2o[7], max_range^2)"""
    Tb = np.asarray(T[0], np.float32).reshape(16)
    dx, dy = pts[:, 0].astype(np.float64) - float(Tb[3]), pts[:, 1].astype(np.float64) - float(Tb[7])
    return dx * dx + dy * dy < float(r) * float(r)


_pairs = {}


def pair(gpu_mod, **kw):
    """one handle and one oracle per parameter set, reused with set_map"""
    d = dict(max_range=R, num_rings=1, num_sectors=4, min_h=-5.0, max_h=5.0, minimum_num_pts=3, scan_ratio_threshold=0.3,
             query_voxel_size=0.05, map_voxel_size=0.05, gf_num_lpr=2, num_lowest_pts=0)  # (test_oracle_known_answers.one_bin_params)
    d.update(kw)
    key = tuple(sorted(d.items()))
    if key not in _pairs:
        _pairs[key] = make_pair(gpu_mod, ka.params(**d))
    g, o = _pairs[key]
    hooks.debug_set_scan_one_max(g, 0)
    return g, o


def load(g, o, m):
    g.set_map(m)
    if o is not None:
        o.set_map(m)


def step(g, o, T, pre, scan=EMPTY, full=True, r=R):
    """one step of both, compared bit for bit, and the model's counts for the logical map `pre` the step starts from"""
    rg, ro = g.step(scan, I4, T[0], T[1]), o.step(scan, I4, T[0], T[1])
    n_in = int(inside(pre, T, r).sum())
    print("step at (%g, %g): model n_voi %d n_outskirts %d; hip %d %d; oracle %d %d" % (T[0].reshape(16)[3], T[0].reshape(16)[7], n_in, len(pre) - n_in,
                                                                                  rg.n_voi, rg.n_outskirts, ro.n_voi, ro.n_outskirts))
    assert (ro.n_voi, ro.n_outskirts) == (n_in, len(pre) - n_in), "oracle against the float64 model"
    assert (rg.n_voi, rg.n_outskirts) == (n_in, len(pre) - n_in), "HIP against the float64 model"
    compare_step(g, o, rg, ro, full=full)
    return rg


def chunks_of(st):
    """(nFchunks, nOchunks) of the store as the NEXT step will see it"""
    return -(-st["nF"] // CHUNK), st["capO"] // CHUNK - st["o_begin"] // CHUNK


A, FAR = (0, 0), (4000, 4000)


# ---------------------------------------------------------------------------------------------
# (a) extents: nF and o_begin on, just below and just above a chunk border; the borders of k_chunk_scan_one's 16-count threads
# ---------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)
BORDER = (1023, 1024, 1025, 2047, 2048, 2049)


def _extent_cases():
    cases = []
    for n_in in SIZES:
        for n_out in SIZES:
            tot = n_in + n_out
            if tot == 0:
                continue
            nF_edge = n_in in BORDER and n_out in (0, 1, 65, 1024, 2049)       # nF at k * 1024 - 1 / + 0 / + 1
            ob_edge = tot % CHUNK in (1023, 0, 1) and n_in in (1, 64, 1025)     # o_begin = capO - total at a chunk border, or one off
            small = tot <= 65 and (n_in in (0, 1) or n_out in (0, 1))           # degenerate stores
            if nF_edge or ob_edge or small:
                cases.append((n_in, n_out))
    # nFchunks == nchunks (no outskirts at all after a rebuild) and nFchunks = 0 (mod 16); nF one short of 16 chunks beside 1025 outside
    cases += [(16 * CHUNK, 0), (32 * CHUNK, 0), (16 * CHUNK - 1, 1025)]
    # chunk counts of the second step 1 + 4, 1 + 2, 1 + 3, 2 + 5: nchunks = 1, 3, 0 (mod 4) -- the uint4 fast path's tail --, and 3 again
    cases += [(1024, 3072), (1000, 1000), (1024, 2048 - 1), (1025, 5 * CHUNK - 1030)]
    return sorted(set(cases))


@pytest.mark.parametrize("n_in,n_out", _extent_cases(), ids=lambda v: "standin%d" % v)
def test_a_extents(gpu_mod, n_in, n_out):
    """[n_out points 10 r away | n_in points near the pose]: two steps at the same pose (the points enter from the outskirts, then sit in
    the VoI-resident region beside the tombstones they left), a forced rebuild (o_begin = capO - n_out: no outskirts chunk at all when
    n_out = 0) and a third step"""
    g, o = pair(gpu_mod)
    m = np.concatenate([block(n_out, 80.0, tag=3), block(n_in, 0.5)])
    assert int(inside(m, pose(*A)).sum()) == n_in
    load(g, o, m)
    s0 = hooks.debug_store_state(g)
    assert (s0["nF"], s0["capO"] - s0["o_begin"], s0["o_valid"]) == (0, len(m), len(m)) and s0["capO"] % CHUNK == 0
    step(g, o, pose(*A), m)
    s1 = hooks.debug_store_state(g)
    assert (s1["nF"], s1["nFv"], s1["o_begin"], s1["o_valid"]) == (n_in, n_in, s0["o_begin"], n_out), s1
    assert s1["scan_path"] == 1 and s1["n_leaving"] == 0
    step(g, o, pose(*A), m)
    hooks.debug_rebuild_outskirts(g)
    s2 = hooks.debug_store_state(g)
    assert (s2["nF"], s2["capO"] - s2["o_begin"], s2["o_valid"]) == (n_in, n_out, n_out), s2  # dense and right-aligned
    assert chunks_of(s2) == (-(-n_in // CHUNK), -(-n_out // CHUNK))
    same(g.get_map(), o.get_map(), "map after the forced rebuild")
    step(g, o, pose(*A), m)
    step(g, o, pose(*FAR), m)  # everything leaves: n_leaving = n_in, o_new_begin crosses as many chunk borders as that takes
    s3 = hooks.debug_store_state(g)
    assert (s3["nF"], s3["n_leaving"], s3["o_begin"]) == (0, n_in, s2["o_begin"] - n_in), s3


# ---------------------------------------------------------------------------------------------
# (b) patterns inside a chunk
# ---------------------------------------------------------------------------------------------
AP, AQ = (0, 0), (-6, 0)  # every point is inside AP's circle and in its first quadrant (ONE bin: the VoI-resident region keeps the map's order);
#                           AQ's circle takes the points with x < 1 and leaves those with x > 3


def _pattern(kind):
    n = 4096
    if kind == "all":
        return np.ones(1024, bool)
    if kind == "random":
        return np.random.default_rng(20240607).random(n) < 0.5
    return (np.arange(n) // int(kind)) % 2 == 0


@pytest.mark.parametrize("kind", ["1", "64", "256", "1024", "random", "all"], ids=lambda k: "standin-period-" + k)
def test_b_patterns_inside_a_chunk(gpu_mod, kind):
    """membership of AQ's VoI alternates along the map with a period of one point, one tile, one piece of k_voi_gather (GATHER_SUB), one
    chunk, or at random; `all`: one chunk whose voi count and valid count are both 1024 (bit 10 of both packed fields of cinfo).  Once
    with the pattern in the outskirts (a fresh store), once in the VoI-resident region (after a step from AP, which takes everything)"""
    g, o = pair(gpu_mod)
    sel = _pattern(kind)
    near, away = block(len(sel), 0.0, 0.25, width=256, tag=1), block(len(sel), 3.0, 0.25, width=256, tag=5)
    m = np.where(sel[:, None], near, away)
    assert np.array_equal(inside(m, pose(*AQ)), sel) and inside(m, pose(*AP)).all()
    for seq in ((AQ, AP, AQ), (AP, AQ, AP, AQ)):
        load(g, o, m)
        for P in seq:
            step(g, o, pose(*P), m)
        st = hooks.debug_store_state(g)
        assert st["nFv"] == int(sel.sum()) and st["o_valid"] == len(m) - int(sel.sum())


# ---------------------------------------------------------------------------------------------
# the physical model of the outskirts (cases c, e)
# ---------------------------------------------------------------------------------------------
class StoreModel:
    """the outskirts as they must lie in memory: xy[capO], valid[capO], o_begin; which chunk records are known"""

    def __init__(self, st, m):
        self.capO, self.o_begin = st["capO"], st["capO"] - len(m)
        self.xy = np.zeros((self.capO, 2), np.float64)
        self.valid = np.zeros(self.capO, bool)
        self.xy[self.o_begin:] = m[:, :2]
        self.valid[self.o_begin:] = True
        self.F = np.zeros((0, 2), np.float64)
        self.known = np.zeros(self.capO // CHUNK, bool)

    def chunk_ids(self):
        return np.arange(self.o_begin // CHUNK, self.capO // CHUNK)

    def reach(self, T, r, slack):
        """per chunk of the region: holds a VoI point; its valid-entry box comes within r * (1 + slack) of the pose"""
        Tb = np.asarray(T[0], np.float32).reshape(16)
        xc, yc = float(Tb[3]), float(Tb[7])
        ids = self.chunk_ids()
        holds, near = np.zeros(len(ids), bool), np.zeros(len(ids), bool)
        for k, a in enumerate(ids):
            v = self.valid[a * CHUNK:(a + 1) * CHUNK]
            if not v.any():
                continue
            p = self.xy[a * CHUNK:(a + 1) * CHUNK][v]
            d2 = (p[:, 0] - xc) ** 2 + (p[:, 1] - yc) ** 2
            holds[k] = (d2 < r * r).any()
            bx = max(p[:, 0].min() - xc, xc - p[:, 0].max(), 0.0)
            by = max(p[:, 1].min() - yc, yc - p[:, 1].max(), 0.0)
            near[k] = bx * bx + by * by <= (r * (1 + slack)) ** 2
        return holds, near

    def step(self, T, F_after, r=R):
        """what a step at T does to the outskirts; F_after: the VoI-resident region it leaves (the head of the oracle's map)"""
        Tb = np.asarray(T[0], np.float32).reshape(16)
        xc, yc = float(Tb[3]), float(Tb[7])
        leave = self.F[~((self.F[:, 0] - xc) ** 2 + (self.F[:, 1] - yc) ** 2 < r * r)]
        ent = self.valid & ((self.xy[:, 0] - xc) ** 2 + (self.xy[:, 1] - yc) ** 2 < r * r)
        self.known[self.chunk_ids()] = True  # (read or skipped: every chunk of the region has a record behind the pass)
        self.valid[ent] = False
        if len(leave):
            nb = self.o_begin - len(leave)
            self.known[nb // CHUNK:(self.o_begin - 1) // CHUNK + 1] = False  # the chunks that receive them: records void
            self.xy[nb:self.o_begin] = leave
            self.valid[nb:self.o_begin] = True
            self.o_begin = nb
        self.F = np.asarray(F_after[:, :2], np.float64)
        return len(leave), int(ent.sum())

    def rebuild(self, st):
        p = self.xy[self.valid]
        self.capO = st["capO"]
        self.xy, self.valid = np.zeros((self.capO, 2), np.float64), np.zeros(self.capO, bool)
        self.o_begin = self.capO - len(p)
        self.xy[self.o_begin:] = p
        self.valid[self.o_begin:] = True
        self.known = np.zeros(self.capO // CHUNK, bool)

    def check(self, g, st):
        """extents; the logical outskirts (the tail of the map); every record: known as the model says, a known record's box contains every
        valid entry of its chunk and its count is the model's"""
        assert (st["o_begin"], st["o_valid"], st["nFv"]) == (self.o_begin, int(self.valid.sum()), len(self.F)), (st, self.o_begin)
        tail = g.get_map()[st["nFv"]:, :2].astype(np.float64)
        assert np.array_equal(tail, self.xy[self.valid]), "the order of the outskirts"
        rec = st["rec"]
        assert rec is not None and len(rec["known"]) == len(self.chunk_ids())
        for k, a in enumerate(self.chunk_ids()):
            assert bool(rec["known"][k]) == bool(self.known[a]), ("known", int(a), k, int(rec["known"][k]))
            if not self.known[a]:
                continue
            v = self.valid[a * CHUNK:(a + 1) * CHUNK]
            assert int(rec["valid"][k]) == int(v.sum()), ("valid", int(a), int(rec["valid"][k]), int(v.sum()))
            if v.any():
                p, b = self.xy[a * CHUNK:(a + 1) * CHUNK][v], rec["box"][k].astype(np.float64)
                assert b[0] <= p[:, 0].min() and p[:, 0].max() <= b[1] and b[2] <= p[:, 1].min() and p[:, 1].max() <= b[3], ("box", int(a), b)


def model_step(g, o, mod, T, pre, quiet=False):
    """a step checked against the oracle, the counts, the layout model and -- n_o_read -- the skip rule: a chunk that holds a VoI point or
    has no record must be read; on a `quiet` pass (the pass before it, from the same pose, moved nothing: every record is fresh) nothing
    may be read whose valid entries' box stays beyond r * (1 + 1e-6) (the kernel's own margin is 1e-9 on r^2)"""
    holds, near = mod.reach(T, R, 1e-6)
    ids = mod.chunk_ids()
    must = holds | ~mod.known[ids]
    step(g, o, T, pre)
    st = hooks.debug_store_state(g)
    n_leave, n_enter = mod.step(T, o.get_map()[:st["nFv"]])
    print("  chunks %d, must be read %d, within reach %d, read %d; %d left, %d entered" % (len(ids), must.sum(), near.sum(), st["n_o_read"], n_leave, n_enter))
    assert st["n_leaving"] == n_leave
    assert st["n_o_read"] >= int(must.sum()), "a chunk with a VoI point, or without a record, was skipped"
    if quiet:
        assert n_leave == 0 and n_enter == 0
        assert st["n_o_read"] <= int(near.sum()), "chunks beyond the circle were read"
    mod.check(g, st)
    return st


# ---------------------------------------------------------------------------------------------
# (c) traffic: A -> B -> A -> A, exactly k points leave and m enter on the way to B
# ---------------------------------------------------------------------------------------------
TA, TB = (0, 0), (10, 0)


def traffic_map(k, m, pad):
    """[common to both circles | k points of A's circle only | pad + 2048 points far away | m points of B's circle only]; m = 1024: the
    store's last chunk enters B's VoI whole and is left fully tombstoned"""
    mp = np.concatenate([block(1500, 4.5, 0.25, 256), block(k, -3.0, 0.25, 256, tag=2), block(2048 + pad, 80.0, tag=4), block(m, 12.0, 0.25, 256, tag=6)])
    a, b = inside(mp, pose(*TA)), inside(mp, pose(*TB))
    assert (int((a & ~b).sum()), int((b & ~a).sum()), int((a & b).sum())) == (k, m, 1500)
    return mp


@pytest.mark.parametrize("k,m,pad", [(1, 1, 0), (1023, 1025, 1), (1024, 1024, 0), (1025, 1023, 1023), (3000, 3000, 5), (1, 3000, 1022), (3000, 1, 64)],
                         ids=lambda v: "standin%d" % v)
def test_c_traffic(gpu_mod, k, m, pad):
    """k = 1 .. 3000: o_new_begin crosses no, one or several chunk borders (the loop that voids the records of the receiving chunks);
    every step against the oracle, the counts and the layout model; then a forced rebuild and one more step"""
    g, o = pair(gpu_mod)
    mp = traffic_map(k, m, pad)
    load(g, o, mp)
    mod = StoreModel(hooks.debug_store_state(g), mp)
    for P in (TA, TB, TA, TA):
        model_step(g, o, mod, pose(*P), mp)
    if m == 1024:  # (the whole last chunk entered at B, came back to the front at A: its record counts no valid entry)
        st = hooks.debug_store_state(g)
        assert st["rec"]["valid"][-1] == 0 and st["rec"]["known"][-1] == 1
    hooks.debug_rebuild_outskirts(g)
    mod.rebuild(hooks.debug_store_state(g))
    same(g.get_map(), o.get_map(), "map after the forced rebuild")
    model_step(g, o, mod, pose(*TB), mp)


# ---------------------------------------------------------------------------------------------
# (d) the circle: d^2 < r^2, strictly, in float64
# ---------------------------------------------------------------------------------------------
def circle_points(cx, cy):
    """integer offsets with dx^2 + dy^2 == 25 exactly (outside), and their float32 neighbours on each side along the larger coordinate"""
    f = np.float32
    pts = []
    for dx, dy in ((3, 4), (4, 3), (5, 0), (0, -5)):
        x, y = f(cx + dx), f(cy + dy)
        pts.append((x, y))
        if abs(dy) > abs(dx):
            pts += [(x, np.nextafter(y, f(cy))), (x, np.nextafter(y, f(cy + 3 * dy)))]
        else:
            pts += [(np.nextafter(x, f(cx)), y), (np.nextafter(x, f(cx + 3 * dx)), y)]
    p = np.array(pts, np.float32)
    return np.column_stack([p, np.full(len(p), 0.5, np.float32), LABELS[np.arange(len(p)) % len(LABELS)]]).astype(np.float32)


@pytest.mark.parametrize("where", ["outskirts", "resident"])
@pytest.mark.parametrize("centre", [(0, 0), (16, -8)], ids=lambda c: "standin-at-%d-%d" % c)
def test_d_a_point_on_the_voi_circle_stays_outside(gpu_mod, centre, where):
    """r = 5: (3, 4), (4, 3), (5, 0), (0, -5) from the pose lie ON the circle and are not VoI points; the float32 neighbour towards the pose
    is, the one away from it is not.  `outskirts`: the outskirts half of k_voi_split decides (a fresh store); `resident`: a step from
    (1.5, -0.5) beside the pose, whose circle holds all twelve, brings them into the VoI-resident region first and the other half decides"""
    g, o = pair(gpu_mod, max_range=5.0, num_rings=15, num_sectors=60)
    cx, cy = centre
    m = np.concatenate([block(700, cx + 0.5, cy + 0.25, 64), circle_points(cx, cy), block(1100, cx + 40.0, cy, 64, tag=3)])
    P = pose(cx, cy)
    want = inside(m, P, 5.0)
    on = slice(700, 712)
    assert want[on].tolist() == [False, True, False] * 4 and int(want.sum()) == 704
    d2 = (m[on, 0].astype(np.float64) - cx) ** 2 + (m[on, 1].astype(np.float64) - cy) ** 2
    assert (d2[0::3] == 25.0).all() and (d2[1::3] < 25.0).all() and (d2[2::3] > 25.0).all()
    load(g, o, m)
    pre = m
    if where == "resident":
        P0 = pose(cx + 1.5, cy - 0.5)
        assert inside(m, P0, 5.0)[:712].all()
        step(g, o, P0, m, r=5.0)
        # (the round trip through P0's frame is exact for the lattice and for the four points ON the circle; a float32 neighbour may come
        # back one ulp off: the model takes the map as it lies now)
        pre = o.get_map()
        d2 = (pre[:, 0].astype(np.float64) - cx) ** 2 + (pre[:, 1].astype(np.float64) - cy) ** 2
        assert int((d2 == 25.0).sum()) >= 4 and int(((d2 < 25.0) & (d2 > 24.999)).sum()) >= 1 and int(((d2 > 25.0) & (d2 < 25.001)).sum()) >= 1
    n_in = int(inside(pre, P, 5.0).sum())
    n_on = int(((pre[:, 0].astype(np.float64) - cx) ** 2 + (pre[:, 1].astype(np.float64) - cy) ** 2 == 25.0).sum())
    assert (n_in, n_on) == (704, 4) if where == "outskirts" else n_on >= 4
    for _ in range(2):
        rg = step(g, o, P, pre, r=5.0)
        got = g.get_map()
        assert rg.n_voi == n_in and inside(got[:n_in], P, 5.0).all() and not inside(got[n_in:], P, 5.0).any()
        d2 = (got[n_in:, 0].astype(np.float64) - cx) ** 2 + (got[n_in:, 1].astype(np.float64) - cy) ** 2
        assert int((d2 == 25.0).sum()) == n_on, "the points on the circle are outskirts"


# ---------------------------------------------------------------------------------------------
# (e) the chunk records: what the pass skips
# ---------------------------------------------------------------------------------------------
def records_map():
    """[points near the pose | a band across A's circle | 20 chunks 10 r away | a band across B's circle]"""
    return np.concatenate([block(1500, 4.5, 0.25, 256), block(3 * CHUNK, 6.0, 0.25, 1024, tag=1), block(20 * CHUNK + 77, 80.0, 0.0, 2048, tag=2),
                           block(2 * CHUNK, 16.0, 0.25, 1024, tag=3)])


def test_e_records_standin_skip_what_lies_beyond_the_circle(gpu_mod):
    g, o = pair(gpu_mod)
    mp = records_map()
    # the model alone: a pass from A may read fewer than half of the chunks, or the upper bound shows nothing
    probe = StoreModel({"capO": 64 * CHUNK}, mp)
    _, near = probe.reach(pose(*TA), R, 1e-6)
    assert 0 < near.sum() < len(near) / 2, (near.sum(), len(near))
    load(g, o, mp)
    mod = StoreModel(hooks.debug_store_state(g), mp)
    model_step(g, o, mod, pose(*TA), mp)       # (every chunk is read: no record yet)
    hooks.debug_rebuild_outskirts(g)
    mod.rebuild(hooks.debug_store_state(g))
    st = model_step(g, o, mod, pose(*TA), mp)  # after a rebuild: every chunk again ...
    assert st["n_o_read"] == len(mod.chunk_ids())
    st = model_step(g, o, mod, pose(*TA), mp, quiet=True)  # ... and the second pass skips
    assert st["n_o_read"] < len(mod.chunk_ids()) / 2
    # after traffic: prepended chunks have no record and are read once, tombstoned chunks keep a right count
    for P in (TB, TA, TA):
        model_step(g, o, mod, pose(*P), mp)
    model_step(g, o, mod, pose(*TA), mp, quiet=True)
    for P in (TB, TB):
        model_step(g, o, mod, pose(*P), mp)
    model_step(g, o, mod, pose(*TB), mp, quiet=True)


# ---------------------------------------------------------------------------------------------
# (f) the two-level chunk scan at small size (the single-launch limit lowered), (g) the real border
# ---------------------------------------------------------------------------------------------
class Recorded:
    """one oracle step, kept: the getters compare_step asks for"""

    def __init__(self, o, ro):
        self.res = ro
        self.d = {("cloud", w): o.get_cloud(w) for w in range(7)}
        self.d["map"], self.d["rej"], self.d["planes"], self.d["status"] = o.get_map(), o.get_rejected_indices(), o.get_planes(), o.get_status()
        self.d["bins0"], self.d["bins1"] = o.get_bins(0), o.get_bins(1)

    get_cloud = lambda self, w: self.d[("cloud", w)]
    get_map = lambda self: self.d["map"]
    get_rejected_indices = lambda self: self.d["rej"]
    get_planes = lambda self: self.d["planes"]
    get_status = lambda self: self.d["status"]
    get_bins = lambda self, w: self.d["bins%d" % w]


SA, SB = (0, 0), (-4, 0)


def column(cx, cy):
    """six map points 1 m tall in a row: a bin that a flat scan reverts"""
    i = np.arange(6)
    return np.column_stack([cx + 0.3125 * i, np.full(6, cy), i / 5.0, np.full(6, 40.0)]).astype(np.float32)


def flat(cx, cy):
    i = np.arange(4)
    return np.column_stack([cx + 0.3125 * i, np.full(4, cy - 0.5), np.zeros(4), np.full(4, 44.0)]).astype(np.float32)


# scans in the body frame.  QUIET: two points in a quadrant without map points, nothing reverts.  REVERT: a flat patch under a 1 m column
# of the map in the LAST bin of the step's VoI (its reserved slots lie at the end of the VoI-resident region): at SA the column at
# (-2, -2.5), from SB the one at (2, -2.5) -- (6, -2.5) in its frame --, back at SA the one at (3, -4), which SB's circle does not hold
QUIET = [np.array([[-2.0, -2.5, 0.0, 40.0], [-2.5, -2.0, 0.0, 40.0]], np.float32)] * 3
REVERT = [flat(-2.0, -2.5), flat(6.0, -2.5), flat(3.0, -4.0)]
COLUMNS = np.concatenate([column(-2.0, -2.5), column(2.0, -2.5), column(3.0, -4.0)])


def two_level_map(nFc, nOc, small):
    """a store that, after a warm-up step and a rebuild, has nFc chunks in the VoI-resident region and nOc in the outskirts: [a band that
    enters at SB | far away | near SA (the last rows beyond SB's reach), three columns].  nFc = 0: the warm-up is at FAR, everything is
    outskirts and the points near SA lie in the LAST chunks"""
    w = 256 if small else 1024
    n_in = nFc * CHUNK - (5 if nFc % 2 else 0)  # (an odd count ends 5 short of its last chunk, an even one fills it)
    n_near = (n_in if nFc else (CHUNK + 11 if small else 3 * CHUNK + 11)) - len(COLUMNS)
    n_rest = nOc * CHUNK - 3 - (0 if nFc else n_near + len(COLUMNS))
    near = [block(n_near, 0.5, 0.0, w, tag=3), COLUMNS]
    if nOc == 0:
        return np.concatenate(near)
    assert n_rest >= 600
    return np.concatenate([block(600, -11.5, 0.25, 256, tag=1), block(n_rest - 600, 80.0, 0.0, 2048, tag=2)] + near)


class OracleRuns:
    """the oracle's answers for one store (warm-up included), by scan set; the ways of a store share them"""

    def __init__(self, o, nFc, nOc, small):
        self.o, self.mp = o, two_level_map(nFc, nOc, small)
        self.seq = [pose(*(SA if nFc else FAR)), pose(*SA), pose(*SB), pose(*SA)]
        self.runs = {}

    def get(self, kind):
        if kind not in self.runs:
            self.o.set_map(self.mp)
            out = []
            for T, s in zip(self.seq, [EMPTY] + (REVERT if kind == "revert" else QUIET)):
                ro = self.o.step(s, I4, T[0], T[1])
                out.append(Recorded(self.o, ro))
            self.runs[kind] = out
        return self.runs[kind]


@functools.lru_cache(maxsize=1)
def _oracle_runs(o, nFc, nOc, small):
    return OracleRuns(o, nFc, nOc, small)


def run_two_level(gpu_mod, nFc, nOc, limit, way, small=False):
    g, o = pair(gpu_mod)
    runs = _oracle_runs(o, nFc, nOc, small)
    mp, seq = runs.mp, runs.seq
    rec = runs.get("revert" if way == "overlapped" else "quiet")
    scans = [EMPTY] + (REVERT if way == "overlapped" else QUIET)
    To = lambda k: seq[k][1] if way == "overlapped" else None
    g.set_map(mp)
    hooks.debug_set_scan_one_max(g, limit)
    rg = g.step(EMPTY, I4, seq[0][0], seq[0][1])
    compare_step(g, rec[0], rg, rec[0].res, full=False)
    hooks.debug_rebuild_outskirts(g)
    st = hooks.debug_store_state(g, records=False)
    assert chunks_of(st) == (nFc, nOc), (st, nFc, nOc)
    l0, u0 = g.ahead_split_counts()
    o0, ou0 = g.overlap_counts()
    pre = rec[0].get_map()
    paths, n_rev = [], 0
    if way != "plain":
        g.prefetch(scans[1], I4, seq[1][0], To(1))
    for k in (1, 2, 3):
        if way != "plain" and k < 3:
            g.prefetch(scans[k + 1], I4, seq[k + 1][0], To(k + 1))
        rg = g.step(scans[k], I4, seq[k][0], seq[k][1])
        n_in = int(inside(pre, seq[k]).sum())
        print("step %d: model n_voi %d; hip %d; oracle %d; reverted bins %d" % (k, n_in, rg.n_voi, rec[k].res.n_voi, rec[k].res.n_reverted_bins))
        assert (rec[k].res.n_voi, rec[k].res.n_outskirts) == (n_in, len(pre) - n_in), "oracle against the float64 model"
        assert (rg.n_voi, rg.n_outskirts) == (n_in, len(pre) - n_in), "HIP against the float64 model"
        compare_step(g, rec[k], rg, rec[k].res, full=True)
        pre = rec[k].get_map()
        n_rev += rec[k].res.n_reverted_bins
        paths.append(hooks.debug_store_state(g, records=False)["scan_path"])
    l1, u1 = g.ahead_split_counts()
    o1, ou1 = g.overlap_counts()
    print("%s, limit %d, %d + %d chunks: chunk-scan paths %s; splits ahead %d launched / %d used, overlapped %d / %d" % (
        way, limit, nFc, nOc, paths, l1 - l0, u1 - u0, o1 - o0, ou1 - ou0))
    two = limit != 0  # (every store here has more chunks than every lowered limit, and fewer than the default)
    if way == "plain":
        assert paths == [2 if two else 1] * 3, paths
    elif way == "ahead":
        # (the rebuild voids nothing here: no pass was ahead of the first step; the two behind it were launched ahead and must be used)
        assert l1 - l0 == 2 and u1 - u0 >= 1, (l0, u0, l1, u1)
        # (on the small store the two-level scan cannot go ahead: its prefix arrays are sized in whole workgroups of 1024 chunks, which the
        # store's scratch does not hold; the split still goes ahead and the step runs the scan)
        assert ((4 if two else 3) in paths[1:] or small) and all(p in ((2, 4) if two else (1, 3)) for p in paths), paths
    else:
        assert n_rev >= 2, "the scans of the overlapped way must revert bins"
        assert o1 - o0 == 2 and ou1 - ou0 >= 1, (o0, ou0, o1, ou1)
        assert (6 if two else 5) in paths[1:] and all(p in ((2, 4, 6) if two else (1, 3, 5)) for p in paths), paths


STORES = [(nFc, n - nFc) for n in (1025, 2047, 2048, 2049) for nFc in (0, 1023, 1024, 1025)]


@pytest.mark.parametrize("limit", [1024, 0], ids=["two-level", "default-limit"])
@pytest.mark.parametrize("way", ["plain", "ahead", "overlapped"])
@pytest.mark.parametrize("nFc,nOc", STORES, ids=["F%d-O%d" % s for s in STORES])
def test_f_two_level_scan_at_small_size(gpu_mod, nFc, nOc, way, limit):
    """stores of 1025, 2047, 2048 and 2049 chunks with 0, 1023, 1024 and 1025 of them in the VoI-resident region (k_chunk_scan_top reads
    pvl[nFchunks] + topv[nFchunks >> 10]; the gathers add topv[c >> 10]), the single-launch limit lowered to 1024 chunks: run by the step
    itself, launched ahead behind the previous step (the next node announced with its pose), and overlapped (announced with both
    transforms).  With the limit at its default the same stores take k_chunk_scan_one.  Three steps each (SA, SB, SA: some points leave
    and come back, a band enters and leaves) against the oracle's answers, which the ways of one store share"""
    run_two_level(gpu_mod, nFc, nOc, limit, way)


@pytest.mark.parametrize("limit", [16, 64])
@pytest.mark.parametrize("way", ["plain", "ahead", "overlapped"])
@pytest.mark.parametrize("nFc,nOc", [(0, 68), (16, 52), (17, 48)], ids=["standin-F0-O68", "standin-F16-O52", "standin-F17-O48"])
def test_f_two_level_scan_on_a_small_store(gpu_mod, nFc, nOc, way, limit):
    """the same on a ~70 k-entry store with the limit at 16 and at 64 chunks"""
    run_two_level(gpu_mod, nFc, nOc, limit, way, small=True)


@pytest.mark.parametrize("n_total,paths", [(16383 * CHUNK, [1, 1]), (16384 * CHUNK + 1, [2, 2])], ids=["16384-chunks", "16385-chunks"])
def test_g_the_real_border_of_the_one_launch_scan(gpu_mod, n_total, paths):
    """the default limit: a store whose second step sees 1 + 16383 = 16384 chunks (the last one-launch size) and one of 16385 and then 16386
    (two levels).  16.8 M points, 270 MB on the host: the one case here that takes more than a few seconds (the time is in MEASUREMENTS.md)"""
    g, o = pair(gpu_mod)
    mp = np.concatenate([block(n_total - 1000, 80.0, 0.0, 2048, tag=2), block(1000, 0.5, 0.25, 256)])
    load(g, o, mp)
    got = []
    for _ in range(2):
        st = hooks.debug_store_state(g, records=False)
        print("chunks", chunks_of(st))
        step(g, o, pose(*SA), mp, full=False)
        got.append(hooks.debug_store_state(g, records=False)["scan_path"])
    assert sum(chunks_of(st)) == (16384 if paths == [1, 1] else 16386)
    assert got == paths, got
    g.set_map(EMPTY)  # (the handle is shared: give the memory back)
    o.set_map(EMPTY)
