"""What the offline analyses refuse, and with which words: every analysis entry point of the C ABI (evaluate, overlap, by_class, render_eval
and align_frames as _clouds / _map, evaluate_many, label_map, static_complement, render_fit / _fit_map, render_clouds / _map) called on
clouds of 8 points with exactly ONE fault, its return code and the full erasor_hip_last_error text compared with literals, and one valid
call of each.  The entry points share their argument checks and their loading of the clouds; this file pins what a caller sees of them.
The 2^30-point cases pass a valid pointer to 8 points: the count is refused before anything is read.
tests/test_analysis_errors_on_cpu.py re-runs this file against the CPU stand-in."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 8
BIG = 2 ** 30
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def gpu_mod():
    import erasor_amd
    erasor_amd.build()  # (a no-op under ERASOR_TEST_SIMT_LIB, see conftest.py)
    return erasor_amd


def clouds():
    rng = np.random.default_rng(7)
    gt = np.zeros((N, 4), np.float32)
    gt[:, :3] = rng.uniform(-1, 1, (N, 3))
    gt[:, 3] = [40, 40, 40, 40, 40, 252, 252, 65536 + 253]
    est = gt.copy()
    est[:, :3] += np.float32(0.01)
    return gt, est


GT_A, EST_A = clouds()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def g(gpu_mod):
    """[a handle with an 8-point map, a handle without a map]"""
    with_map, without = gpu_mod.Erasor(gpu_mod.params_default()), gpu_mod.Erasor(gpu_mod.params_default())
    with_map.set_map(EST_A)
    return {"map": with_map, "no map": without}


class World:
    """the valid arguments of every call, by name; a case replaces one of them"""

    def __init__(self, mod):
        self.mod = mod
        self.d = dict(
            gt=ptr(GT_A), n_gt=N, est=ptr(EST_A), n_est=N, leaf=0.0, vs=0.2,
            res=C.byref(mod.EvalResult()), ov_res=C.byref(mod.OverlapResult()), lm_res=C.byref(mod.LabelResult()),
            cp_res=C.byref(mod.ComplementResult()), per_gt=None, per_dist=None, per_near=None,
            # by_class
            classes=(mod.ClassRow * 1024)(), cap_classes=1024, n_classes=C.byref(C.c_size_t(0)), instances=(mod.ClassRow * 64)(), cap_instances=64,
            n_instances=C.byref(C.c_size_t(0)),
            # render
            view=C.byref(mod.RenderView(-2.0, -2.0, 0.5, 8, 8, -1.5, 1.5, 0, 0)), fit_view=C.byref(mod.RenderView()), mode=mod.RENDER_MODES["label"],
            rgb=(C.c_uint8 * (8 * 8 * 3))(), stats=C.byref(mod.RenderStats()), fit_res=0.5, margin=2,
            # align_frames: one frame of all 8 estimated points
            offsets=(C.c_uint64 * 2)(0, N), n_frames=1, Tl=None, Tb=(C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1),
            al_rows=(mod.AlignRow * 1)(), summary=C.byref(mod.OverlapResult()),
            # evaluate_many: two estimates
            ests=(C.c_void_p * 2)(ptr(EST_A), ptr(GT_A)), n_ests=(C.c_size_t * 2)(N, N), ests_dev=(C.c_int * 2)(0, 0), k=2,
            many_rows=(mod.EvalResult * 2)(),
            # label_map / static_complement
            lm_leaf=0.2, dst=(C.c_float * (4 * N))(), cap=N)

    def call(self, entry, h, over):
        a = dict(self.d, **over)
        z, d, i = C.c_size_t, C.c_double, C.c_int
        gt, est = (a["gt"], z(a["n_gt"]), i(0)), (a["est"], z(a["n_est"]), i(0))
        vox = (d(a["leaf"]), d(a["vs"]))
        rows = (a["classes"], z(a["cap_classes"]), a["n_classes"], a["instances"], z(a["cap_instances"]), a["n_instances"])
        img = (a["view"], a["rgb"], i(0), a["stats"])
        tgt = (i(a["mode"]), C.c_int32(-1), C.c_int32(-1))
        fit = (d(a["fit_res"]), C.c_uint32(a["margin"]), C.c_uint32(0), a["fit_view"])
        frames = (a["est"], z(a["n_est"]), a["offsets"], z(a["n_frames"]), i(0), a["Tl"], a["Tb"], d(a["vs"]), a["al_rows"], a["summary"])
        args = {
            "evaluate_clouds": (*gt, *est, *vox, a["per_gt"], a["res"]),
            "evaluate_map": (*gt, *vox, a["res"]),
            "overlap_clouds": (*gt, *est, *vox, a["per_dist"], a["per_near"], a["ov_res"]),
            "overlap_map": (*gt, *vox, a["ov_res"]),
            "evaluate_clouds_by_class": (*gt, *est, *vox, *rows, a["res"]),
            "evaluate_map_by_class": (*gt, *vox, *rows, a["res"]),
            "render_eval_clouds": (*gt, *est, *vox, *img, a["res"]),
            "render_eval_map": (*gt, *vox, *img, a["res"]),
            "align_frames_clouds": (*gt, *frames),  # (the ground truth as the map)
            "align_frames_map": frames,
            "evaluate_many": (*gt, a["ests"], a["n_ests"], a["ests_dev"], z(a["k"]), *vox, a["many_rows"]),
            "label_map": (*est, *gt, d(a["lm_leaf"]), a["dst"], z(a["cap"]), a["lm_res"]),  # (src = est, medium = gt)
            "static_complement": (*est, *gt, a["dst"], z(a["cap"]), a["cp_res"]),
            "render_fit": (*gt, *fit),
            "render_fit_map": fit,
            "render_clouds": (*gt, *tgt, *img),
            "render_map": (*tgt, *img),
        }[entry]
        lib = self.mod.lib()
        rc = getattr(lib, "erasor_hip_" + entry)(h._h, *args)
        return rc, (lib.erasor_hip_last_error(h._h) or b"").decode()


@pytest.fixture(scope="module")
def world(gpu_mod):
    return World(gpu_mod)


PAIR = ("evaluate_clouds", "overlap_clouds", "evaluate_clouds_by_class", "render_eval_clouds")
PAIR_MAP = ("evaluate_map", "overlap_map", "evaluate_map_by_class", "render_eval_map")
ALIGN = ("align_frames_clouds", "align_frames_map")
USES_MAP = PAIR_MAP + ("align_frames_map", "render_fit_map", "render_map")
ENTRIES = PAIR + PAIR_MAP + ALIGN + ("evaluate_many", "label_map", "static_complement", "render_fit", "render_fit_map", "render_clouds", "render_map")
RES = {"overlap_clouds": "ov_res", "overlap_map": "ov_res", "label_map": "lm_res", "static_complement": "cp_res", "evaluate_many": "many_rows",
       "align_frames_clouds": "al_rows", "align_frames_map": "al_rows"}
# the cloud arguments of every entry point: (pointer, count)
CLOUDS = {e: (("gt", "n_gt"), ("est", "n_est")) for e in PAIR + ("align_frames_clouds", "label_map", "static_complement")}
CLOUDS.update({e: (("gt", "n_gt"),) for e in PAIR_MAP + ("evaluate_many", "render_fit", "render_clouds")})
CLOUDS["align_frames_map"] = (("est", "n_est"),)
BIG_OFFSETS = (C.c_uint64 * 2)(0, BIG)  # (align_frames: the offsets of one frame of 2^30 points, so that the count is the only fault)


def cases():
    out = []
    add = lambda entry, what, over, handle="map": out.append((entry + ": " + what, entry, over, handle))
    for e in ENTRIES:
        add(e, "valid", {})
    for e in PAIR + PAIR_MAP + ("evaluate_many",):
        add(e, "valid, voxel_leaf 0.1", {"leaf": 0.1})
    for e in PAIR + PAIR_MAP + ALIGN + ("evaluate_many", "label_map", "static_complement"):
        add(e, "rows NULL" if e in ALIGN + ("evaluate_many",) else "res NULL", {RES.get(e, "res"): None})
    for e in PAIR + PAIR_MAP + ALIGN + ("evaluate_many",):
        add(e, "voxelsize 0", {"vs": 0.0})
        add(e, "voxelsize NaN", {"vs": NAN})
    for e in PAIR + PAIR_MAP + ("evaluate_many",):
        add(e, "voxel_leaf negative", {"leaf": -0.1})
        add(e, "voxel_leaf Inf", {"leaf": INF})
    add("label_map", "leaf 0", {"lm_leaf": 0.0})
    add("label_map", "leaf Inf", {"lm_leaf": INF})
    add("evaluate_clouds", "per_gt with voxel_leaf > 0", {"per_gt": (C.c_uint8 * N)(), "leaf": 0.1})
    add("overlap_clouds", "per_est_dist with voxel_leaf > 0", {"per_dist": (C.c_double * N)(), "leaf": 0.1})
    add("overlap_clouds", "per_est_nearest with voxel_leaf > 0", {"per_near": (C.c_uint32 * N)(), "leaf": 0.1})
    for e, slots in CLOUDS.items():
        for cl, cnt in slots:
            add(e, "NULL " + cl, {cl: None})
            big = {cnt: BIG}
            if e in ALIGN and cl == "est":
                big["offsets"] = BIG_OFFSETS
            add(e, cnt + " 2^30", big)
    add("evaluate_many", "NULL estimate 1", {"ests": (C.c_void_p * 2)(ptr(EST_A), None)})
    add("evaluate_many", "estimate 1 of 2^30", {"n_ests": (C.c_size_t * 2)(N, BIG)})
    add("evaluate_many", "est_xyzi NULL", {"ests": None})
    for e in USES_MAP:
        add(e, "no map", {}, "no map")
    add("overlap_clouds", "empty ground truth", {"n_gt": 0})
    add("overlap_map", "empty ground truth", {"n_gt": 0})
    add("label_map", "empty medium", {"n_gt": 0})
    for e in ("evaluate_clouds_by_class", "evaluate_map_by_class"):
        add(e, "n_classes NULL", {"n_classes": None})
        add(e, "n_instances NULL", {"n_instances": None})
    for e in ("render_clouds", "render_map", "render_eval_clouds", "render_eval_map"):
        add(e, "view NULL", {"view": None})
    for e in ("render_fit", "render_fit_map"):
        add(e, "view NULL", {"fit_view": None})
        add(e, "res 0", {"fit_res": 0.0})
    for e in ("render_clouds", "render_map"):
        add(e, "mode EVAL", {"mode": 2})
        add(e, "mode 7", {"mode": 7})
    return out


CASES = cases()

# (rc, erasor_hip_last_error) of every case; 0: the call succeeds
EXPECT = {
    'evaluate_clouds: valid': 0,
    'overlap_clouds: valid': 0,
    'evaluate_clouds_by_class: valid': 0,
    'render_eval_clouds: valid': 0,
    'evaluate_map: valid': 0,
    'overlap_map: valid': 0,
    'evaluate_map_by_class: valid': 0,
    'render_eval_map: valid': 0,
    'align_frames_clouds: valid': 0,
    'align_frames_map: valid': 0,
    'evaluate_many: valid': 0,
    'label_map: valid': 0,
    'static_complement: valid': 0,
    'render_fit: valid': 0,
    'render_fit_map: valid': 0,
    'render_clouds: valid': 0,
    'render_map: valid': 0,
    'evaluate_clouds: valid, voxel_leaf 0.1': 0,
    'overlap_clouds: valid, voxel_leaf 0.1': 0,
    'evaluate_clouds_by_class: valid, voxel_leaf 0.1': 0,
    'render_eval_clouds: valid, voxel_leaf 0.1': 0,
    'evaluate_map: valid, voxel_leaf 0.1': 0,
    'overlap_map: valid, voxel_leaf 0.1': 0,
    'evaluate_map_by_class: valid, voxel_leaf 0.1': 0,
    'render_eval_map: valid, voxel_leaf 0.1': 0,
    'evaluate_many: valid, voxel_leaf 0.1': 0,
    'evaluate_clouds: res NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'overlap_clouds: res NULL': (-1, 'erasor_hip_overlap: res is NULL'),
    'evaluate_clouds_by_class: res NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'render_eval_clouds: res NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'evaluate_map: res NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'overlap_map: res NULL': (-1, 'erasor_hip_overlap: res is NULL'),
    'evaluate_map_by_class: res NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'render_eval_map: res NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'align_frames_clouds: rows NULL': (-1, 'erasor_hip_align_frames_clouds: rows or T_body2origin is NULL'),
    'align_frames_map: rows NULL': (-1, 'erasor_hip_align_frames_map: rows or T_body2origin is NULL'),
    'evaluate_many: rows NULL': (-1, 'erasor_hip_evaluate: res is NULL'),
    'label_map: res NULL': (-1, 'erasor_hip_label_map: res is NULL'),
    'static_complement: res NULL': (-1, 'erasor_hip_static_complement: res is NULL'),
    'evaluate_clouds: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_clouds: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'overlap_clouds: voxelsize 0': (-1, 'erasor_hip_overlap: voxelsize must be a finite number > 0'),
    'overlap_clouds: voxelsize NaN': (-1, 'erasor_hip_overlap: voxelsize must be a finite number > 0'),
    'evaluate_clouds_by_class: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_clouds_by_class: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'render_eval_clouds: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'render_eval_clouds: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_map: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_map: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'overlap_map: voxelsize 0': (-1, 'erasor_hip_overlap: voxelsize must be a finite number > 0'),
    'overlap_map: voxelsize NaN': (-1, 'erasor_hip_overlap: voxelsize must be a finite number > 0'),
    'evaluate_map_by_class: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_map_by_class: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'render_eval_map: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'render_eval_map: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'align_frames_clouds: voxelsize 0': (-1, 'erasor_hip_align_frames_clouds: voxelsize must be a finite number > 0'),
    'align_frames_clouds: voxelsize NaN': (-1, 'erasor_hip_align_frames_clouds: voxelsize must be a finite number > 0'),
    'align_frames_map: voxelsize 0': (-1, 'erasor_hip_align_frames_map: voxelsize must be a finite number > 0'),
    'align_frames_map: voxelsize NaN': (-1, 'erasor_hip_align_frames_map: voxelsize must be a finite number > 0'),
    'evaluate_many: voxelsize 0': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_many: voxelsize NaN': (-1, 'erasor_hip_evaluate: voxelsize must be a finite number > 0'),
    'evaluate_clouds: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_clouds: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'overlap_clouds: voxel_leaf negative': (-1, 'erasor_hip_overlap: voxel_leaf must be 0 or a finite number > 0'),
    'overlap_clouds: voxel_leaf Inf': (-1, 'erasor_hip_overlap: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_clouds_by_class: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_clouds_by_class: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'render_eval_clouds: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'render_eval_clouds: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_map: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_map: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'overlap_map: voxel_leaf negative': (-1, 'erasor_hip_overlap: voxel_leaf must be 0 or a finite number > 0'),
    'overlap_map: voxel_leaf Inf': (-1, 'erasor_hip_overlap: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_map_by_class: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_map_by_class: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'render_eval_map: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'render_eval_map: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_many: voxel_leaf negative': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'evaluate_many: voxel_leaf Inf': (-1, 'erasor_hip_evaluate: voxel_leaf must be 0 or a finite number > 0'),
    'label_map: leaf 0': (-1, 'erasor_hip_label_map: leaf must be a finite number > 0'),
    'label_map: leaf Inf': (-1, 'erasor_hip_label_map: leaf must be a finite number > 0'),
    'evaluate_clouds: per_gt with voxel_leaf > 0': (-1, 'erasor_hip_evaluate: per_gt needs voxel_leaf == 0 (the codes would describe the voxelised ground truth)'),
    'overlap_clouds: per_est_dist with voxel_leaf > 0': (-1, 'erasor_hip_overlap: per-point outputs need voxel_leaf == 0 (they would describe the voxelised estimate)'),
    'overlap_clouds: per_est_nearest with voxel_leaf > 0': (-1, 'erasor_hip_overlap: per-point outputs need voxel_leaf == 0 (they would describe the voxelised estimate)'),
    'evaluate_clouds: NULL gt': (-1, 'erasor_hip_evaluate_clouds: NULL cloud or more than 2^30 points'),
    'evaluate_clouds: n_gt 2^30': (-1, 'erasor_hip_evaluate_clouds: NULL cloud or more than 2^30 points'),
    'evaluate_clouds: NULL est': (-1, 'erasor_hip_evaluate_clouds: NULL cloud or more than 2^30 points'),
    'evaluate_clouds: n_est 2^30': (-1, 'erasor_hip_evaluate_clouds: NULL cloud or more than 2^30 points'),
    'overlap_clouds: NULL gt': (-1, 'erasor_hip_overlap_clouds: NULL cloud or more than 2^30 points'),
    'overlap_clouds: n_gt 2^30': (-1, 'erasor_hip_overlap_clouds: NULL cloud or more than 2^30 points'),
    'overlap_clouds: NULL est': (-1, 'erasor_hip_overlap_clouds: NULL cloud or more than 2^30 points'),
    'overlap_clouds: n_est 2^30': (-1, 'erasor_hip_overlap_clouds: NULL cloud or more than 2^30 points'),
    'evaluate_clouds_by_class: NULL gt': (-1, 'erasor_hip_evaluate_clouds_by_class: NULL cloud or more than 2^30 points'),
    'evaluate_clouds_by_class: n_gt 2^30': (-1, 'erasor_hip_evaluate_clouds_by_class: NULL cloud or more than 2^30 points'),
    'evaluate_clouds_by_class: NULL est': (-1, 'erasor_hip_evaluate_clouds_by_class: NULL cloud or more than 2^30 points'),
    'evaluate_clouds_by_class: n_est 2^30': (-1, 'erasor_hip_evaluate_clouds_by_class: NULL cloud or more than 2^30 points'),
    'render_eval_clouds: NULL gt': (-1, 'erasor_hip_render_eval_clouds: NULL cloud or more than 2^30 points'),
    'render_eval_clouds: n_gt 2^30': (-1, 'erasor_hip_render_eval_clouds: NULL cloud or more than 2^30 points'),
    'render_eval_clouds: NULL est': (-1, 'erasor_hip_render_eval_clouds: NULL cloud or more than 2^30 points'),
    'render_eval_clouds: n_est 2^30': (-1, 'erasor_hip_render_eval_clouds: NULL cloud or more than 2^30 points'),
    'align_frames_clouds: NULL gt': (-1, 'erasor_hip_align_frames_clouds: NULL map or more than 2^30 map points'),
    'align_frames_clouds: n_gt 2^30': (-1, 'erasor_hip_align_frames_clouds: NULL map or more than 2^30 map points'),
    'align_frames_clouds: NULL est': (-1, 'erasor_hip_align_frames_clouds: NULL scans'),
    'align_frames_clouds: n_est 2^30': (-1, 'erasor_hip_align_frames_clouds: more than 2^30 scan points'),
    'label_map: NULL gt': (-1, 'erasor_hip_label_map: NULL cloud or more than 2^30 points'),
    'label_map: n_gt 2^30': (-1, 'erasor_hip_label_map: NULL cloud or more than 2^30 points'),
    'label_map: NULL est': (-1, 'erasor_hip_label_map: NULL cloud or more than 2^30 points'),
    'label_map: n_est 2^30': (-1, 'erasor_hip_label_map: NULL cloud or more than 2^30 points'),
    'static_complement: NULL gt': (-1, 'erasor_hip_static_complement: NULL cloud or more than 2^30 points'),
    'static_complement: n_gt 2^30': (-1, 'erasor_hip_static_complement: NULL cloud or more than 2^30 points'),
    'static_complement: NULL est': (-1, 'erasor_hip_static_complement: NULL cloud or more than 2^30 points'),
    'static_complement: n_est 2^30': (-1, 'erasor_hip_static_complement: NULL cloud or more than 2^30 points'),
    'evaluate_map: NULL gt': (-1, 'erasor_hip_evaluate_map: NULL cloud or more than 2^30 points'),
    'evaluate_map: n_gt 2^30': (-1, 'erasor_hip_evaluate_map: NULL cloud or more than 2^30 points'),
    'overlap_map: NULL gt': (-1, 'erasor_hip_overlap_map: NULL cloud or more than 2^30 points'),
    'overlap_map: n_gt 2^30': (-1, 'erasor_hip_overlap_map: NULL cloud or more than 2^30 points'),
    'evaluate_map_by_class: NULL gt': (-1, 'erasor_hip_evaluate_map_by_class: NULL cloud or more than 2^30 points'),
    'evaluate_map_by_class: n_gt 2^30': (-1, 'erasor_hip_evaluate_map_by_class: NULL cloud or more than 2^30 points'),
    'render_eval_map: NULL gt': (-1, 'erasor_hip_render_eval_map: NULL cloud or more than 2^30 points'),
    'render_eval_map: n_gt 2^30': (-1, 'erasor_hip_render_eval_map: NULL cloud or more than 2^30 points'),
    'evaluate_many: NULL gt': (-1, 'erasor_hip_evaluate_many: NULL ground truth or more than 2^30 points'),
    'evaluate_many: n_gt 2^30': (-1, 'erasor_hip_evaluate_many: NULL ground truth or more than 2^30 points'),
    'render_fit: NULL gt': (-1, 'erasor_hip_render_fit: NULL cloud or more than 2^30 points'),
    'render_fit: n_gt 2^30': (-1, 'erasor_hip_render_fit: NULL cloud or more than 2^30 points'),
    'render_clouds: NULL gt': (-1, 'erasor_hip_render_clouds: NULL cloud or more than 2^30 points'),
    'render_clouds: n_gt 2^30': (-1, 'erasor_hip_render_clouds: NULL cloud or more than 2^30 points'),
    'align_frames_map: NULL est': (-1, 'erasor_hip_align_frames_map: NULL scans'),
    'align_frames_map: n_est 2^30': (-1, 'erasor_hip_align_frames_map: more than 2^30 scan points'),
    'evaluate_many: NULL estimate 1': (-1, 'erasor_hip_evaluate_many: estimate 1: NULL cloud or more than 2^30 points'),
    'evaluate_many: estimate 1 of 2^30': (-1, 'erasor_hip_evaluate_many: estimate 1: NULL cloud or more than 2^30 points'),
    'evaluate_many: est_xyzi NULL': (-1, 'erasor_hip_evaluate_many: est_xyzi or n_est is NULL'),
    'evaluate_map: no map': (-4, 'erasor_hip_evaluate_map: the handle has no map (erasor_hip_set_map first)'),
    'overlap_map: no map': (-4, 'erasor_hip_overlap_map: the handle has no map (erasor_hip_set_map first)'),
    'evaluate_map_by_class: no map': (-4, 'erasor_hip_evaluate_map_by_class: the handle has no map (erasor_hip_set_map first)'),
    'render_eval_map: no map': (-4, 'erasor_hip_render_eval_map: the handle has no map (erasor_hip_set_map first)'),
    'align_frames_map: no map': (-4, 'erasor_hip_align_frames_map: the handle has no map (erasor_hip_set_map first)'),
    'render_fit_map: no map': (-4, 'erasor_hip_render_fit_map: the handle has no map (erasor_hip_set_map first)'),
    'render_map: no map': (-4, 'erasor_hip_render_map: the handle has no map (erasor_hip_set_map first)'),
    'overlap_clouds: empty ground truth': (-1, 'erasor_hip_overlap_clouds: empty ground truth (no nearest point to measure against)'),
    'overlap_map: empty ground truth': (-1, 'erasor_hip_overlap_map: empty ground truth (no nearest point to measure against)'),
    'label_map: empty medium': (-1, 'erasor_hip_label_map: empty medium (no labelled point to take a label from)'),
    'evaluate_clouds_by_class: n_classes NULL': (-1, 'erasor_hip_evaluate_by_class: NULL row count, or a NULL row array with a capacity > 0'),
    'evaluate_clouds_by_class: n_instances NULL': (-1, 'erasor_hip_evaluate_by_class: NULL row count, or a NULL row array with a capacity > 0'),
    'evaluate_map_by_class: n_classes NULL': (-1, 'erasor_hip_evaluate_by_class: NULL row count, or a NULL row array with a capacity > 0'),
    'evaluate_map_by_class: n_instances NULL': (-1, 'erasor_hip_evaluate_by_class: NULL row count, or a NULL row array with a capacity > 0'),
    'render_clouds: view NULL': (-1, 'erasor_hip_render: view is NULL'),
    'render_map: view NULL': (-1, 'erasor_hip_render: view is NULL'),
    'render_eval_clouds: view NULL': (-1, 'erasor_hip_render: view is NULL'),
    'render_eval_map: view NULL': (-1, 'erasor_hip_render: view is NULL'),
    'render_fit: view NULL': (-1, 'erasor_hip_render_fit: view is NULL'),
    'render_fit: res 0': (-1, 'erasor_hip_render_fit: res must be a finite number > 0 and margin_px in 1 .. 1024'),
    'render_fit_map: view NULL': (-1, 'erasor_hip_render_fit: view is NULL'),
    'render_fit_map: res 0': (-1, 'erasor_hip_render_fit: res must be a finite number > 0 and margin_px in 1 .. 1024'),
    'render_clouds: mode EVAL': (-1, 'erasor_hip_render: mode must be ERASOR_RENDER_LABEL or ERASOR_RENDER_HEIGHT (the error map: erasor_hip_render_eval_*)'),
    'render_clouds: mode 7': (-1, 'erasor_hip_render: mode must be ERASOR_RENDER_LABEL or ERASOR_RENDER_HEIGHT (the error map: erasor_hip_render_eval_*)'),
    'render_map: mode EVAL': (-1, 'erasor_hip_render: mode must be ERASOR_RENDER_LABEL or ERASOR_RENDER_HEIGHT (the error map: erasor_hip_render_eval_*)'),
    'render_map: mode 7': (-1, 'erasor_hip_render: mode must be ERASOR_RENDER_LABEL or ERASOR_RENDER_HEIGHT (the error map: erasor_hip_render_eval_*)'),
}


def test_every_case_has_its_expectation():
    assert sorted(EXPECT) == sorted(c[0] for c in CASES) and len(EXPECT) == len(CASES)


@pytest.mark.parametrize("name,entry,over,handle", CASES, ids=[c[0] for c in CASES])
def test_one_fault_one_code_one_sentence(g, world, name, entry, over, handle):
    rc, msg = world.call(entry, g[handle], over)
    want = EXPECT[name]
    if want == 0:
        assert rc == 0, (rc, msg)
    else:
        assert (rc, msg) == want
