"""erasor_amd — MI355X-native ERASOR hot path.

The product is `liberasor_hip.so` (hand-written HIP for gfx950, C ABI in include/erasor_hip.h) plus the
C++ shim in erasor_amd/csrc/shim (reference-compatible ERASOR / OfflineMapUpdater / erasor_utils
surface).  This Python package is plumbing only: a ctypes binding used by tests, bench.py and
__graft_entry__.py.  There is no CPU fallback: if the HIP library or a GPU is missing, calls fail loudly.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liberasor_hip.so")
_SRC_DIR = os.path.join(_HERE, "csrc")


class Params(C.Structure):
    """erasor_params (include/erasor_hip.h) — the reference's rosparam names (erasor.h:47-61, OMU.cpp:66-83)."""
    _fields_ = [
        ("max_range", C.c_double), ("num_rings", C.c_int32), ("num_sectors", C.c_int32),
        ("max_h", C.c_double), ("min_h", C.c_double), ("th_bin_max_h", C.c_double),
        ("scan_ratio_threshold", C.c_double), ("num_lowest_pts", C.c_int32),
        ("minimum_num_pts", C.c_int32), ("rejection_ratio", C.c_double),
        ("gf_dist_thr", C.c_double), ("gf_iter", C.c_int32), ("gf_num_lpr", C.c_int32),
        ("gf_th_seeds_height", C.c_double), ("map_voxel_size", C.c_double),
        ("version", C.c_int32), ("query_voxel_size", C.c_double),
        ("removal_interval", C.c_int32), ("voi_max_range", C.c_double),
        ("is_large_scale", C.c_int32), ("reserved0_", C.c_int32), ("submap_size", C.c_double),
        ("reserved_", C.c_int32 * 3),
    ]


class StepLogEntry(C.Structure):
    """erasor_step_log_entry (include/erasor_hip.h)"""
    _fields_ = [("step", C.c_uint64), ("period_us", C.c_double), ("n_alloc", C.c_uint32), ("n_free", C.c_uint32), ("n_create", C.c_uint32),
                ("reserved", C.c_uint8), ("use_ov", C.c_uint8), ("deep", C.c_uint8), ("sampled", C.c_uint8), ("ova_mode", C.c_uint8),
                ("ova_block", C.c_uint8), ("ova_skip", C.c_uint8), ("grown", C.c_uint8)]


class StepResult(C.Structure):
    """erasor_step_result (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "n_map_in", "n_voi", "n_outskirts", "n_query", "n_static_estimate", "n_complement",
        "n_map_rejected", "n_curr_rejected", "n_ground", "n_map_out", "n_static", "n_dynamic")] + [
        (k, C.c_uint32) for k in (
            "n_reverted_bins", "n_neg_sector", "n_ambiguous", "n_degenerate_plane",
            "n_voxel_overflow", "n_sort_fallback")] + [("reserved_", C.c_uint32 * 6)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved_"}


class EvalResult(C.Structure):
    """erasor_eval_result (include/erasor_hip.h): PR / RR of a cleaned map (scripts/analysis_runner.py:74-105)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "gt_static", "gt_dynamic", "est_static", "est_dynamic", "preserved_static", "preserved_dynamic",
        "n_tied", "n_label_out_of_range")] + [(k, C.c_double) for k in ("PR", "RR", "F1")]

    def as_dict(self):
        """evalmap.evaluate's keys plus the two diagnostics"""
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class OverlapResult(C.Structure):
    """erasor_overlap_result (include/erasor_hip.h): the estimate-to-ground-truth distances of overlap_report
    (scripts/analysis_runner.py:53-71)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_est", "n_below_half", "n_below_one", "n_below_two")] + [(k, C.c_double) for k in (
        "median", "p90", "p99", "max", "frac_half", "frac_one", "frac_two")]

    def as_dict(self):
        """evalmap.overlap's keys"""
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class AlignRow(C.Structure):
    """erasor_align_row (include/erasor_hip.h): one frame of align_frames"""
    _fields_ = [("n_points", C.c_uint64), ("n_non_finite", C.c_uint64), ("r", OverlapResult)]

    def as_dict(self):
        """evalmap.align_frames' row keys"""
        d = self.r.as_dict()
        d.update(n_points=int(self.n_points), n_non_finite=int(self.n_non_finite))
        return d


class RefineParams(C.Structure):
    """erasor_refine_params (include/erasor_hip.h)"""
    _fields_ = [("max_dist", C.c_double), ("eps_t", C.c_double), ("eps_r", C.c_double), ("max_iters", C.c_uint32), ("min_pairs", C.c_uint32)]


class RefineRow(C.Structure):
    """erasor_refine_row (include/erasor_hip.h): one frame of refine_poses"""
    _fields_ = [("T", C.c_double * 16), ("status", C.c_uint32), ("iters", C.c_uint32)] + [(k, C.c_uint64) for k in (
        "n_points", "n_non_finite", "n_pairs_first", "n_pairs_last")] + [(k, C.c_double) for k in ("rms_first", "rms_last", "moved_t", "moved_r")]

    def as_dict(self):
        """evalmap.refine_poses' row keys (the pose itself is returned beside the rows)"""
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_ if k != "T"}


class RefineSummary(C.Structure):
    """erasor_refine_summary (include/erasor_hip.h)"""
    _fields_ = [("n_frames", C.c_uint64), ("n_status", C.c_uint64 * 4), ("n_pairs_first", C.c_uint64), ("n_pairs_last", C.c_uint64),
                ("sum_d2_first", C.c_double), ("sum_d2_last", C.c_double)]

    def as_dict(self):
        """evalmap.refine_poses' summary keys"""
        return {"n_frames": int(self.n_frames), "n_status": [int(v) for v in self.n_status], "n_pairs_first": int(self.n_pairs_first),
                "n_pairs_last": int(self.n_pairs_last), "sum_d2_first": float(self.sum_d2_first), "sum_d2_last": float(self.sum_d2_last)}


class RefinePlaneParams(C.Structure):
    """erasor_refine_plane_params (include/erasor_hip.h)"""
    _fields_ = [("max_dist", C.c_double), ("eps_t", C.c_double), ("eps_r", C.c_double), ("max_iters", C.c_uint32), ("min_pairs", C.c_uint32),
                ("normals_k", C.c_uint32), ("max_curvature", C.c_double), ("rank_tol", C.c_double)]


class RefinePlaneRow(C.Structure):
    """erasor_refine_plane_row (include/erasor_hip.h): one frame of refine_poses_plane"""
    _fields_ = RefineRow._fields_ + [("rank", C.c_uint32), ("lambda_ratio", C.c_double), ("n_unusable_first", C.c_uint64),
                                     ("n_unusable_last", C.c_uint64), ("rms_plane_first", C.c_double), ("rms_plane_last", C.c_double)]

    def as_dict(self):
        """evalmap.refine_poses_plane's row keys (the pose itself is returned beside the rows)"""
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_ if k != "T"}


class RefinePlaneSummary(C.Structure):
    """erasor_refine_plane_summary (include/erasor_hip.h)"""
    _fields_ = [("n_frames", C.c_uint64), ("n_status", C.c_uint64 * 5), ("n_pairs_first", C.c_uint64), ("n_pairs_last", C.c_uint64),
                ("sum_d2_first", C.c_double), ("sum_d2_last", C.c_double), ("sum_r2_first", C.c_double), ("sum_r2_last", C.c_double),
                ("n_map_no_normal", C.c_uint64)]

    def as_dict(self):
        """evalmap.refine_poses_plane's summary keys"""
        return {k: ([int(v) for v in self.n_status] if k == "n_status" else float(getattr(self, k)) if t is C.c_double else int(getattr(self, k)))
                for k, t in self._fields_}


class ScanLabelRow(C.Structure):
    """erasor_scan_label_row (include/erasor_hip.h): one frame of label_scans, or their sum"""
    _fields_ = [("n_points", C.c_uint64), ("n_non_finite", C.c_uint64), ("n_label_out_of_range", C.c_uint64), ("n", (C.c_uint64 * 3) * 2)]

    def as_dict(self):
        """evalmap.label_scans' row keys"""
        return {"n_points": int(self.n_points), "n_non_finite": int(self.n_non_finite), "n_label_out_of_range": int(self.n_label_out_of_range),
                "n": [[int(self.n[g][k]) for k in range(3)] for g in range(2)]}


class ClusterRow(C.Structure):
    """erasor_cluster_row (include/erasor_hip.h): one listed cluster"""
    _fields_ = [(k, C.c_uint32) for k in ("first", "n_points", "n_dynamic", "n_label_out_of_range")] + [
        ("min_xyz", C.c_float * 3), ("max_xyz", C.c_float * 3)]


# the rows as numpy records (ClusterRow's layout; evalmap.CLUSTER_ROW_DTYPE)
CLUSTER_ROW_DTYPE = np.dtype([(k, np.uint32) for k in ("first", "n_points", "n_dynamic", "n_label_out_of_range")] + [
    ("min_xyz", np.float32, 3), ("max_xyz", np.float32, 3)])
CLUSTER_NONE = 0xFFFFFFFF  # ids of points whose cluster is not listed


class ClusterResult(C.Structure):
    """erasor_cluster_result (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_clusters", "n_listed", "n_points_listed", "n_singletons", "largest")]

    def as_dict(self):
        """evalmap.cluster's result keys"""
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ObjectVoteParams(C.Structure):
    """erasor_object_vote_params (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_double) for k in ("tol", "max_extent", "remove_ratio", "revert_ratio")] + [
        (k, C.c_uint64) for k in ("min_size", "max_size", "min_voted")] + [("vote_thr", C.c_uint32), ("ground_keep", C.c_uint32)]


class ObjectRow(C.Structure):
    """erasor_object_row (include/erasor_hip.h): one touched cluster"""
    _fields_ = [(k, C.c_uint32) for k in ("first", "n_points", "n_voted", "n_dynamic", "n_voted_dynamic", "n_label_out_of_range")] + [
        ("min_xyz", C.c_float * 3), ("max_xyz", C.c_float * 3), ("decision", C.c_uint32)]


# the rows as numpy records (ObjectRow's layout; evalmap.OBJECT_ROW_DTYPE), the decision codes and the id of a point without a row
OBJECT_ROW_DTYPE = np.dtype([(k, np.uint32) for k in ("first", "n_points", "n_voted", "n_dynamic", "n_voted_dynamic", "n_label_out_of_range")] + [
    ("min_xyz", np.float32, 3), ("max_xyz", np.float32, 3), ("decision", np.uint32)])
OBJECT_UNCHANGED, OBJECT_REMOVED, OBJECT_REVERTED, OBJECT_NOT_OBJECT = 0, 1, 2, 3
OBJECT_NONE = 0xFFFFFFFF


class ObjectVoteResult(C.Structure):
    """erasor_object_vote_result (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "n_points", "n_ground", "n_clusters", "n_touched", "n_removed_clusters", "n_reverted_clusters", "n_not_object", "n_voted", "n_removed",
        "n_grown", "n_grown_dynamic", "n_reverted", "n_reverted_dynamic", "n_ground_reverted", "n_ground_reverted_dynamic", "largest")]

    def as_dict(self):
        """evalmap.object_vote's result keys"""
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def votes_from_masks(*kept_masks):
    """the saturating uint8 count, per point, of the masks that say 0 (removed): the 1 = kept masks of visibility, carve and a step go
    straight in, and object_vote(vote_thr=2) of three of them is their majority"""
    if not kept_masks:
        raise ValueError("votes_from_masks: no mask")
    n = len(np.asarray(kept_masks[0]).reshape(-1))
    votes = np.zeros(n, np.uint16)
    for m in kept_masks:
        m = np.asarray(m).reshape(-1)
        if len(m) != n:
            raise ValueError("votes_from_masks: the masks differ in length")
        votes += (m == 0)
        np.minimum(votes, 255, out=votes)
    return votes.astype(np.uint8)


class ScoreStats(C.Structure):
    """erasor_score_stats (include/erasor_hip.h): a score's statistics over the points where it is finite"""
    _fields_ = [("n_scored", C.c_uint64)] + [(k, C.c_double) for k in ("min", "median", "p90", "p99", "max")]

    def as_dict(self):
        """evalmap.score_stats' keys"""
        return {"n_scored": int(self.n_scored), **{k: float(getattr(self, k)) for k in ("min", "median", "p90", "p99", "max")}}


class KnnResult(C.Structure):
    """erasor_knn_result (include/erasor_hip.h)"""
    _fields_ = [("n_points", C.c_uint64), ("n_short", C.c_uint64), ("kth", ScoreStats), ("mean", ScoreStats)]


class DensityFilter(C.Structure):
    """erasor_density_filter (include/erasor_hip.h)"""
    _fields_ = [("score", C.c_int32), ("rule", C.c_int32), ("k", C.c_uint32), ("min_neighbors", C.c_uint32), ("radius", C.c_double),
                ("thr", C.c_double), ("mul", C.c_double)]


class DensityResult(C.Structure):
    """erasor_density_result (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_kept", "n_removed", "n_removed_dynamic", "n_removed_static", "n_short", "n_scored")] + [
        (k, C.c_double) for k in ("m", "mad", "thr", "min", "median", "p90", "p99", "max")]

    def as_dict(self):
        """evalmap.density_filter's result keys"""
        return {k: (int if t is C.c_uint64 else float)(getattr(self, k)) for k, t in self._fields_}


class NormalsResult(C.Structure):
    """erasor_normals_result (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_short", "n_degenerate", "n_ambiguous", "n_flipped")] + [("curvature", ScoreStats)]


class Visibility(C.Structure):
    """erasor_visibility"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("col_tan", C.POINTER(C.c_double)), ("row_tan", C.POINTER(C.c_double)),
                ("min_range", C.c_double), ("max_range", C.c_double), ("margin_abs", C.c_double), ("margin_rel", C.c_double),
                ("window", C.c_uint32), ("k", C.c_uint32), ("min_cos", C.c_double), ("min_through", C.c_uint32), ("reserved", C.c_uint32),
                ("hit_weight", C.c_double), ("image_budget_bytes", C.c_uint64)]


class VisibilityRow(C.Structure):
    """erasor_visibility_row"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_non_finite", "n_on_axis", "n_out_of_range", "n_out_of_view", "n_pixels", "n_map_in_view",
                                          "n_hit", "n_occluded", "n_no_return", "n_through", "n_grazing")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class VisibilityResult(C.Structure):
    """erasor_visibility_result"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_never_in_view", "n_kept", "n_removed", "n_removed_dynamic", "n_removed_static",
                                          "n_map_no_normal", "n_in_view", "n_hit", "n_occluded", "n_no_return", "n_through", "n_grazing")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


VISIBILITY_IMAGE_BUDGET = 256 << 20  # ERASOR_VISIBILITY_IMAGE_BUDGET


def visibility_grid(width, height, el_bottom_deg, el_top_deg):
    """evalmap.visibility_grid, re-exported: the edge tables of a uniform width x height grid between two elevations, for Erasor.visibility"""
    from . import evalmap
    return evalmap.visibility_grid(width, height, el_bottom_deg, el_top_deg)

class Carve(C.Structure):
    """erasor_carve"""
    _fields_ = [("voxel", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("l_init", C.c_float), ("l_hit", C.c_float),
                ("l_miss", C.c_float), ("l_min", C.c_float), ("l_max", C.c_float), ("l_thr", C.c_float), ("stop_short", C.c_uint32),
                ("reserved", C.c_uint32)]


class CarveRow(C.Structure):
    """erasor_carve_row"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_non_finite", "n_out_of_range", "n_rays", "n_steps", "n_end_in_map", "n_voxels_hit",
                                          "n_voxels_free")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CarveResult(C.Structure):
    """erasor_carve_result"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_map_non_finite", "n_voxels", "n_blocks", "n_voxels_touched", "n_kept", "n_removed",
                                          "n_removed_dynamic", "n_removed_static", "n_scan_points", "n_non_finite", "n_out_of_range", "n_rays",
                                          "n_steps", "n_end_in_map", "n_voxels_hit", "n_voxels_free")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def carve_logodds(p_hit=0.7, p_miss=0.4, p_min=0.12, p_max=0.97, p_thr=0.5):
    """evalmap.carve_logodds, re-exported: OctoMap's log-odds from its probabilities (float32(log(p / (1 - p))), l_init = 0), for
    Erasor.carve"""
    from . import evalmap
    return evalmap.carve_logodds(p_hit, p_miss, p_min, p_max, p_thr)


class Ground(C.Structure):
    """erasor_ground"""
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("ring_edge", C.POINTER(C.c_double)), ("col_tan", C.POINTER(C.c_double)),
                ("elevation", C.POINTER(C.c_double)), ("flatness", C.POINTER(C.c_double)), ("num_lpr", C.c_uint32), ("iters", C.c_uint32),
                ("min_points", C.c_uint32), ("min_votes", C.c_uint32), ("th_seeds", C.c_double), ("th_dist", C.c_double), ("min_z", C.c_double),
                ("uprightness", C.c_double), ("ratio", C.c_double), ("keep", C.c_uint32), ("reserved", C.c_uint32),
                ("work_budget_bytes", C.c_uint64)]


class GroundRow(C.Structure):
    """erasor_ground_row"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_non_finite", "n_out_of_range", "n_judged", "n_ground", "n_ground_dynamic", "n_patches",
                                          "n_sparse", "n_degenerate", "n_rejected_upright", "n_rejected_elevation", "n_gathered")]

    def as_dict(self, gathered=False):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if gathered or k != "n_gathered"}


class GroundPatch(C.Structure):
    """erasor_ground_patch (evalmap.GROUND_PATCH_DTYPE)"""
    _fields_ = [("status", C.c_uint32), ("n_points", C.c_uint32), ("n_ground", C.c_uint32), ("reserved", C.c_uint32), ("normal", C.c_double * 3),
                ("d", C.c_double), ("mean_z", C.c_double), ("eig", C.c_double * 3)]


class GroundResult(C.Structure):
    """erasor_ground_result"""
    _fields_ = [(k, C.c_uint64) for k in ("n_frames", "n_points", "n_non_finite", "n_out_of_range", "n_judged", "n_ground", "n_ground_dynamic",
                                          "n_patches", "n_sparse", "n_degenerate", "n_rejected_upright", "n_rejected_elevation", "n_map_points",
                                          "n_map_ground", "n_map_ground_dynamic", "n_map_ground_static", "n_map_unseen", "n_kept")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# the fit's size classes and the default work budget (include/erasor_hip.h)
GROUND_WAVE_POINTS, GROUND_SMALL_POINTS, GROUND_LDS_POINTS = 64, 1024, 4096
GROUND_WORK_BUDGET = 256 << 20


def ground_grid(n_rings=20, n_sectors=64, min_range=0.5, max_range=80.0):
    """evalmap.ground_grid, re-exported: a uniform patch grid (n_sectors, col_tan, ring_edge) for Erasor.ground_scans / ground_votes"""
    from . import evalmap
    return evalmap.ground_grid(n_rings, n_sectors, min_range, max_range)


DENSITY_SCORES = {"kth": 0, "mean": 1, "count": 2}  # ERASOR_DENSITY_KTH / _MEAN / _COUNT
DENSITY_RULES = {"abs": 0, "mad": 1}                # ERASOR_DENSITY_ABS / _MAD
KNN_NONE = 0xFFFFFFFF  # the padding of a neighbour list


class LabelResult(C.Structure):
    """erasor_label_result (include/erasor_hip.h): label_map of a map without labels (fill_removert_intensity.cpp:24-59)"""
    _fields_ = [("n_src", C.c_uint64), ("n_out", C.c_uint64), ("n_tied", C.c_uint64), ("passthrough", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ComplementResult(C.Structure):
    """erasor_complement_result (include/erasor_hip.h): calc_complement's lost static points (compare_complement.cpp:43-75)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_gt", "n_gt_static", "n_lost", "n_label_out_of_range")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RenderView(C.Structure):
    """erasor_render_view (include/erasor_hip.h): the window of a bird's-eye image"""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("res", C.c_double), ("width", C.c_uint32), ("height", C.c_uint32),
                ("z_lo", C.c_double), ("z_hi", C.c_double), ("background", C.c_uint32), ("reserved_", C.c_uint32)]

    def as_dict(self):
        """evalmap.render_view's keys"""
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved_"}

    @classmethod
    def of(cls, v):
        """from a RenderView or a dict with evalmap.render_view's keys"""
        return v if isinstance(v, cls) else cls(**{k: v[k] for k, _ in cls._fields_ if k != "reserved_"})


class RenderStats(C.Structure):
    """erasor_render_stats (include/erasor_hip.h)"""
    _fields_ = [(k, C.c_uint64) for k in ("n_points", "n_drawn", "n_outside", "n_nonfinite", "n_pixels_hit")] + [
        ("cat_points", C.c_uint64 * 8), ("cat_pixels", C.c_uint64 * 8)]

    def as_dict(self):
        """evalmap.render's stats keys"""
        d = {k: int(getattr(self, k)) for k, _ in self._fields_[:5]}
        d["cat_points"] = [int(v) for v in self.cat_points]
        d["cat_pixels"] = [int(v) for v in self.cat_pixels]
        return d


RENDER_LABEL, RENDER_HEIGHT, RENDER_EVAL = 0, 1, 2
RENDER_MODES = {"label": RENDER_LABEL, "height": RENDER_HEIGHT}


def write_ppm(path, img):
    """an H x W x 3 uint8 image as a binary PPM (P6, maxval 255)"""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_ppm: the image must be H x W x 3")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def read_ppm(path):
    """a binary PPM (P6, maxval 255; comments allowed in the header) as an H x W x 3 uint8 array"""
    with open(path, "rb") as f:
        data = f.read()
    pos, tok = 0, []
    while len(tok) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while end < len(data) and not data[end:end + 1].isspace():
            end += 1
        tok.append(data[pos:end])
        pos = end
    if tok[0] != b"P6" or int(tok[3]) != 255:
        raise ValueError("read_ppm: not a binary PPM with maxval 255")
    w, h = int(tok[1]), int(tok[2])
    pos += 1  # (the single whitespace after maxval)
    if len(data) - pos < w * h * 3:
        raise ValueError("read_ppm: truncated file")
    return np.frombuffer(data, np.uint8, w * h * 3, pos).reshape(h, w, 3).copy()


def hstack_panels(imgs, gap=4, background=0):
    """images of one height side by side, left to right, `gap` pixels of `background` (0xRRGGBB) between neighbours"""
    imgs = [np.asarray(i, np.uint8) for i in imgs]
    if not imgs or any(i.ndim != 3 or i.shape[2] != 3 or i.shape[0] != imgs[0].shape[0] for i in imgs):
        raise ValueError("hstack_panels: H x W x 3 images of one height")
    h = imgs[0].shape[0]
    out = np.empty((h, sum(i.shape[1] for i in imgs) + gap * (len(imgs) - 1), 3), np.uint8)
    out[:] = [(background >> 16) & 0xFF, (background >> 8) & 0xFF, background & 0xFF]
    x = 0
    for i in imgs:
        out[:, x:x + i.shape[1]] = i
        x += i.shape[1] + gap
    return out


class SweepRow(C.Structure):
    """erasor_sweep_row (include/erasor_hip.h): one configuration of a sweep"""
    _fields_ = [("params", Params), ("status", C.c_int32), ("n_steps", C.c_uint32), ("n_map_final", C.c_uint64), ("n_saved", C.c_uint64),
                ("eval", EvalResult), ("run_ms", C.c_double), ("reserved_", C.c_uint32 * 8)]

    def as_dict(self):
        return {"params": params_dict(self.params), "status": int(self.status), "n_steps": int(self.n_steps),
                "n_map_final": int(self.n_map_final), "n_saved": int(self.n_saved), "run_ms": float(self.run_ms), "eval": self.eval.as_dict()}


def params_dict(p):
    """the fields of a Params as a dict of field -> value (the reserved ones left out)"""
    return {k: getattr(p, k) for k, _ in Params._fields_ if not k.startswith("reserved")}


def param_grid(base, **axes):
    """the Cartesian product of Params field lists, in keyword order, the last axis varying fastest: a list of copies of `base` with those
    fields set.  param_grid(p, scan_ratio_threshold=[0.1, 0.2, 0.3], max_h=[2.8, 3.2]) gives six Params."""
    import itertools
    names = [f for f, _ in Params._fields_]
    for k in axes:
        if k not in names or k.startswith("reserved"):
            raise ValueError("param_grid: %r is not a Params field" % k)
    out = []
    for combo in itertools.product(*[list(v) for v in axes.values()]):
        p = Params()
        C.memmove(C.byref(p), C.byref(base), C.sizeof(Params))
        for k, v in zip(axes, combo):
            setattr(p, k, v)
        out.append(p)
    return out


class ClassRow(C.Structure):
    """erasor_eval_class_row (include/erasor_hip.h): one row of the breakdown by class or by dynamic instance"""
    _fields_ = [("key", C.c_uint32), ("is_dynamic", C.c_uint32)] + [(k, C.c_uint64) for k in (
        "n_gt", "n_within", "n_preserved", "n_tied", "n_est")]


# the rows as numpy records (ClassRow's layout); Erasor.evaluate_by_class adds PR / RR per row (CLASS_ROW_DTYPE_PR)
CLASS_ROW_DTYPE = np.dtype([(k, np.uint32 if t is C.c_uint32 else np.uint64) for k, t in ClassRow._fields_])
CLASS_ROW_DTYPE_PR = np.dtype(CLASS_ROW_DTYPE.descr + [("PR", np.float64), ("RR", np.float64)])
EVAL_KEY_LABEL_OUT_OF_RANGE = 0x10000
N_CLASS_KEYS = 0x10001  # (every class key: a class array of this many rows always fits)


def class_rows_with_rates(rows):
    """rows (CLASS_ROW_DTYPE) plus evalmap.evaluate's rates per row: PR = n_preserved / n_gt * 100 on static rows, RR = (n_gt -
    n_preserved) / n_gt * 100 on dynamic rows; 0 without ground truth, NaN in the column that does not apply"""
    out = np.zeros(len(rows), CLASS_ROW_DTYPE_PR)
    for k in CLASS_ROW_DTYPE.names:
        out[k] = rows[k]
    n = rows["n_gt"].astype(np.float64)
    kept = rows["n_preserved"].astype(np.float64)
    dyn = rows["is_dynamic"] != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        pr = np.where(n > 0, kept / n * 100.0, 0.0)
        rr = np.where(n > 0, (n - kept) / n * 100.0, 0.0)
    out["PR"] = np.where(dyn, np.nan, pr)
    out["RR"] = np.where(dyn, rr, np.nan)
    return out


# per-ground-truth-point codes of Erasor.evaluate(per_point=True)
EVAL_OUT, EVAL_KEPT_STATIC, EVAL_KEPT_DYNAMIC, EVAL_CLASS_DIFFERS = 0, 1, 2, 3

CLOUD_QUERY_VOI, CLOUD_MAP_VOI, CLOUD_STATIC_ESTIMATE, CLOUD_COMPLEMENT = 0, 1, 2, 3
CLOUD_MAP_REJECTED, CLOUD_CURR_REJECTED, CLOUD_GROUND_VIZ, CLOUD_MAP = 4, 5, 6, 7

E_NO_DEVICE = -2
E_CAPACITY = -3


class ErasorError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__("erasor_hip rc=%d: %s" % (rc, msg))
        self.rc = rc


def build(force=False):
    """hipcc --offload-arch=gfx950 … -shared -> erasor_amd/liberasor_hip.so (cross-compiles without a GPU)."""
    srcs = [os.path.join(_SRC_DIR, f) for f in ("erasor_hip.hip", "analysis_host.hip.h", "kernels.hip.h", "evaluate.hip.h", "nearest.hip.h", "align.hip.h", "refine.hip.h", "label_scans.hip.h", "cluster.hip.h", "objects.hip.h", "knn.hip.h", "normals.hip.h", "refine_plane.hip.h", "visibility.hip.h", "carve.hip.h", "ground.hip.h", "render.hip.h", "revert_bins.hip.h",
                                                 "exact_sort.hip.h", "exact_sort_core.h", "overlap_auto.h", "stream_place.h")]
    srcs.append(os.path.join(_HERE, "..", "include", "erasor_hip.h"))
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["make", "-C", _SRC_DIR, "-s"])
    return LIB_PATH


_lib = None


def lib():
    """Load liberasor_hip.so.  Raises if it has not been built — there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ErasorError(E_NO_DEVICE, "liberasor_hip.so missing: run erasor_amd.build() (hipcc) first; no CPU fallback exists")
        l = C.CDLL(LIB_PATH)
        l.erasor_hip_version.restype = C.c_char_p
        l.erasor_hip_last_error.restype = C.c_char_p
        l.erasor_hip_last_error.argtypes = [C.c_void_p]
        l.erasor_hip_stream.restype = C.c_void_p
        l.erasor_hip_stream.argtypes = [C.c_void_p]
        l.erasor_hip_destroy.argtypes = [C.c_void_p]
        l.erasor_hip_destroy.restype = None
        _lib = l
    return _lib


def params_default():
    p = Params()
    rc = lib().erasor_hip_params_default(C.byref(p))
    assert rc == 0
    return p


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


Mat16 = C.c_float * 16


def c_mat(T):
    """a 4x4 row-major transform as a ctypes float[16], converted once: the step / prefetch wrappers take it as it is
    (the numpy -> ctypes conversion of three matrices costs ~10 us per call, a visible share of a 0.3 ms step)"""
    return T if isinstance(T, Mat16) else Mat16(*[float(v) for v in _f32(T).reshape(16)])


def _m(T):
    return T if isinstance(T, Mat16) else _p(_f32(T).reshape(16))


def geopose2eigen(pose7):
    """erasor_utils::geoPose2eigen (erasor_utils.cpp:35-55): tf::Matrix3x3(tf::Quaternion) evaluated in double with
    tf's association, each entry narrowed to float32.  pose7 = x y z qx qy qz qw.  Returns 16 floats, row-major."""
    px, py, pz, x, y, z, w = [float(v) for v in pose7]
    d = x * x + y * y + z * z + w * w
    s = 2.0 / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    T = np.array([1.0 - (yy + zz), xy - wz, xz + wy, px,
                  xy + wz, 1.0 - (xx + zz), yz - wx, py,
                  xz - wy, yz + wx, 1.0 - (xx + yy), pz,
                  0.0, 0.0, 0.0, 1.0], np.float64)
    return T.astype(np.float32)


def invert_rigid(T):
    """T_origin2body from T_body2origin: general 4x4 inverse in float64, narrowed to float32 (the caller owns this
    choice — the reference's Eigen SSE inverse (OMU.cpp:436) is not bit-reproducible across CPUs)."""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    return np.linalg.inv(T).astype(np.float32).reshape(16)


def replicate_map(handles, root=0):
    """erasor_hip_replicate_map: the map of handles[root] to every other handle (one per device) -- single-process RCCL broadcast over
    xGMI, or peer copies.  Returns the transport used (1 RCCL, 2 peer copies, 0 empty map)."""
    arr = (C.c_void_p * len(handles))(*[h._h for h in handles])
    t = C.c_int(0)
    rc = lib().erasor_hip_replicate_map(arr, C.c_int(len(handles)), C.c_int(root), C.byref(t))
    if rc != 0:
        raise ErasorError(rc, (lib().erasor_hip_last_error(handles[root]._h) or b"").decode())
    return t.value


class Erasor:
    """Handle of the HIP hot path (one GPU, one stream)."""

    def __init__(self, params, device=0):
        self.params = params
        self.B = params.num_rings * params.num_sectors
        self._h = C.c_void_p()
        rc = lib().erasor_hip_create(C.byref(params), C.c_int(device), C.byref(self._h))
        self._last_res = None
        if rc != 0:
            self._h = C.c_void_p()
            raise ErasorError(rc, "erasor_hip_create failed (no GPU / invalid parameters)")

    # -- lifetime --
    def close(self):
        if getattr(self, "_h", None):
            lib().erasor_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise ErasorError(rc, (lib().erasor_hip_last_error(self._h) or b"").decode())

    # -- map --
    def set_map(self, cloud):
        cloud = _f32(cloud).reshape(-1, 4)
        self._check(lib().erasor_hip_set_map(self._h, _p(cloud), C.c_size_t(len(cloud))))

    def set_map_device(self, dptr, n):
        self._check(lib().erasor_hip_set_map_device(self._h, C.c_void_p(dptr), C.c_size_t(n)))

    def map_size(self):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_map_size(self._h, C.byref(n)))
        return n.value

    def get_map(self):
        return self.get_cloud(CLOUD_MAP)

    # -- step --
    def prefetch(self, scan, T_l2b, T_b2o=None, T_o2b=None):
        """announce the next scan (host array): its query chain starts now, beside the step in flight.  With the node's pose its VoI
        split goes ahead as well; with T_o2b too (erasor_hip_announce_origin2body) the whole front of its step runs beside the per-bin
        launch of the step before it (overlapped steps)"""
        scan = _f32(scan).reshape(-1, 4)
        # every announced buffer stays alive until a step has consumed it (up to four scans can be outstanding; a freed
        # buffer's address could be handed to the next np.ascontiguousarray)
        self._keep = (getattr(self, "_keep", []) + [scan])[-4:]
        if T_b2o is None:
            self._check(lib().erasor_hip_prefetch_scan(self._h, _p(scan), C.c_size_t(len(scan)), C.c_int(0), _m(T_l2b)))
        else:
            self._check(lib().erasor_hip_prefetch_node(self._h, _p(scan), C.c_size_t(len(scan)), C.c_int(0), _m(T_l2b), _m(T_b2o)))
            if T_o2b is not None:
                self._check(lib().erasor_hip_announce_origin2body(self._h, _m(T_o2b)))
        return scan

    def prefetch_device(self, d_ptr, n, T_l2b, T_b2o=None, T_o2b=None):
        """announce the next scan (device buffer, read in place); with its pose the next step's VoI split is launched ahead"""
        if T_b2o is None:
            self._check(lib().erasor_hip_prefetch_scan(self._h, C.c_void_p(d_ptr), C.c_size_t(n), C.c_int(1), _m(T_l2b)))
        else:
            self._check(lib().erasor_hip_prefetch_node(self._h, C.c_void_p(d_ptr), C.c_size_t(n), C.c_int(1), _m(T_l2b), _m(T_b2o)))
            if T_o2b is not None:
                self._check(lib().erasor_hip_announce_origin2body(self._h, _m(T_o2b)))

    def step(self, scan, T_l2b, T_b2o, T_o2b):
        scan = _f32(scan).reshape(-1, 4)
        res = StepResult()
        self._check(lib().erasor_hip_step(self._h, _p(scan), C.c_size_t(len(scan)), _p(_f32(T_l2b).reshape(16)),
                                          _p(_f32(T_b2o).reshape(16)), _p(_f32(T_o2b).reshape(16)), C.byref(res)))
        self._last_res = res
        return res

    def step_device(self, dptr, n, T_l2b, T_b2o, T_o2b):
        res = StepResult()
        self._check(lib().erasor_hip_step_device(self._h, C.c_void_p(dptr), C.c_size_t(n), _m(T_l2b), _m(T_b2o), _m(T_o2b), C.byref(res)))
        self._last_res = res
        return res

    # -- host records in the caller's layout, announcements by ticket (erasor_hip_step_rows / _prefetch_node_rows / _step_ticket) --
    @staticmethod
    def _rows(rows):
        """rows: a C-contiguous 2-D array of 4-byte items, one record per row: x, y, z first; returns (array, stride in bytes)"""
        rows = np.ascontiguousarray(rows)
        assert rows.ndim == 2 and rows.itemsize == 4 and rows.shape[1] >= 4
        return rows, rows.shape[1] * 4

    def step_rows(self, rows, intensity_col, T_l2b, T_b2o, T_o2b):
        """a step on host records laid out like the caller has them (pcl::PointXYZI: 8 floats per row, intensity in column 4)"""
        rows, stride = self._rows(rows)
        res = StepResult()
        self._check(lib().erasor_hip_step_rows(self._h, _p(rows), C.c_size_t(len(rows)), C.c_size_t(stride), C.c_size_t(4 * intensity_col),
                                               _m(T_l2b), _m(T_b2o), _m(T_o2b), C.byref(res)))
        self._last_res = res
        return res

    def prefetch_node_rows(self, rows, intensity_col, T_l2b, T_b2o=None, T_o2b=None):
        """announce the next node (host records); returns its ticket.  The buffer is the caller's again on return."""
        rows, stride = self._rows(rows)
        t = C.c_uint64(0)
        self._check(lib().erasor_hip_prefetch_node_rows(self._h, _p(rows), C.c_size_t(len(rows)), C.c_size_t(stride), C.c_size_t(4 * intensity_col),
                                                        _m(T_l2b), None if T_b2o is None else _m(T_b2o), C.byref(t)))
        if T_b2o is not None and T_o2b is not None:
            self._check(lib().erasor_hip_announce_origin2body(self._h, _m(T_o2b)))
        return t.value

    def step_ticket(self, ticket, T_b2o, T_o2b):
        res = StepResult()
        self._check(lib().erasor_hip_step_ticket(self._h, C.c_uint64(ticket), _m(T_b2o), _m(T_o2b), C.byref(res)))
        self._last_res = res
        return res

    def step_async(self, scan, n=None, T_l2b=None, T_b2o=None, T_o2b=None, device=False):
        """first half of a step (erasor_hip_step_async): everything is enqueued, nothing is waited for.  scan: a host array, or a
        device pointer with its point count (device=True).  step_wait() collects the results."""
        if device:
            ptr, cnt = C.c_void_p(scan), C.c_size_t(n)
        else:
            scan = _f32(scan).reshape(-1, 4)
            self._fly_keep = scan  # (must stay valid until step_wait has returned)
            ptr, cnt = _p(scan), C.c_size_t(len(scan))
        self._check(lib().erasor_hip_step_async(self._h, ptr, cnt, C.c_int(1 if device else 0), _m(T_l2b), _m(T_b2o), _m(T_o2b)))

    def step_wait(self):
        res = StepResult()
        self._check(lib().erasor_hip_step_wait(self._h, C.byref(res)))
        self._fly_keep = None
        self._last_res = res
        return res

    def run_nodes(self, scan_ptrs, n_pts, T_l2b, Tb, To, first, count, lookahead, announced, device=True):
        """erasor_hip_run_nodes: nodes [first, first + count) of a sequence in ONE native call (the offline driver's loop).
        scan_ptrs / n_pts: ctypes arrays over the whole sequence (see node_arrays); announced: a ctypes c_size_t carried
        between calls.  Returns the list of StepResult."""
        res = (StepResult * count)()
        self._check(lib().erasor_hip_run_nodes(self._h, scan_ptrs, n_pts, C.c_size_t(len(n_pts)), C.c_int(1 if device else 0), _m(T_l2b), Tb, To,
                                               C.c_size_t(first), C.c_size_t(count), C.c_int(lookahead), C.byref(announced), res))
        self._last_res = res[count - 1] if count else None
        return list(res)

    @staticmethod
    def node_arrays(ptrs, sizes, Tb_list, To_list):
        """the arguments of run_nodes from Python lists: device (or host) pointers, point counts, 4x4 matrices"""
        n = len(ptrs)
        P = (C.c_void_p * n)(*ptrs)
        N = (C.c_size_t * n)(*sizes)
        Tb = (C.c_float * (16 * n))(*[float(v) for t in Tb_list for v in np.asarray(t, np.float32).reshape(16)])
        To = (C.c_float * (16 * n))(*[float(v) for t in To_list for v in np.asarray(t, np.float32).reshape(16)])
        return P, N, Tb, To

    def last_result(self):
        """erasor_step_result of the last collected step (kept by the wrapper)"""
        return self._last_res

    def step_done(self):
        return bool(lib().erasor_hip_step_done(self._h))

    # -- read-back --
    def get_cloud(self, which):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_get_cloud(self._h, which, None, C.c_size_t(0), C.byref(n)))
        out = np.empty((n.value, 4), np.float32)
        self._check(lib().erasor_hip_get_cloud(self._h, which, _p(out), C.c_size_t(n.value), C.byref(n)))
        return out

    def get_rejected_indices(self):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_get_rejected_indices(self._h, None, C.c_size_t(0), C.byref(n)))
        out = np.empty(n.value, np.uint64)
        self._check(lib().erasor_hip_get_rejected_indices(self._h, _p(out), C.c_size_t(n.value), C.byref(n)))
        return out

    def get_bins(self, which):
        cnt = np.zeros(self.B, np.uint32)
        mn = np.zeros(self.B, np.float64)
        mx = np.zeros(self.B, np.float64)
        self._check(lib().erasor_hip_get_bins(self._h, which, _p(cnt), _p(mn), _p(mx)))
        return cnt, mn, mx

    def get_status(self):
        st = np.zeros(self.B, np.float64)
        self._check(lib().erasor_hip_get_status(self._h, _p(st)))
        return st

    def get_planes(self):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_get_planes(self._h, None, None, None, C.c_size_t(0), C.byref(n)))
        nb, it = n.value, self.params.gf_iter
        bins = np.zeros(nb, np.uint32)
        normal = np.zeros((nb, it, 3), np.float32)
        d = np.zeros((nb, it), np.float64)
        if nb:
            self._check(lib().erasor_hip_get_planes(self._h, _p(bins), _p(normal), _p(d), C.c_size_t(nb), C.byref(n)))
        return bins, normal, d

    def voxelize_preserving_labels(self, cloud, leaf):
        cloud = _f32(cloud).reshape(-1, 4)
        out = np.empty((max(len(cloud), 1), 4), np.float32)
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_voxelize_preserving_labels(self._h, _p(cloud), C.c_size_t(len(cloud)), C.c_double(leaf), _p(out),
                                                                C.c_size_t(len(out)), C.byref(n)))
        return out[: n.value].copy()

    # -- PR / RR (scripts/analysis_runner.py:74-105; the same on the host: erasor_amd.evalmap) --
    def _eval_cloud(self, cloud, kept):
        """(pointer, point count, is_device) of a cloud argument: a host array (N x 4 float32 rows) or a (device pointer, n) pair"""
        if isinstance(cloud, tuple):
            ptr, n = cloud
            return C.c_void_p(ptr), C.c_size_t(n), C.c_int(1)
        a = _f32(cloud).reshape(-1, 4)
        kept.append(a)
        return _p(a), C.c_size_t(len(a)), C.c_int(0)

    def evaluate(self, gt, est, voxelsize=0.2, voxel_leaf=0.0, per_point=False):
        """PR / RR of the estimate `est` against the labelled ground truth `gt` on the device (erasor_hip_evaluate_clouds).  Each cloud is
        a host array of XYZI rows or a (device pointer, n) pair (device_array).  voxel_leaf > 0: both voxelised at that leaf first.
        Returns evalmap.evaluate's dict plus n_tied / n_label_out_of_range; per_point=True adds "per_point": one EVAL_* code per GT point."""
        kept = []
        g = self._eval_cloud(gt, kept)
        e = self._eval_cloud(est, kept)
        codes = np.zeros(max(g[1].value, 1), np.uint8) if per_point else None
        r = EvalResult()
        self._check(lib().erasor_hip_evaluate_clouds(self._h, *g, *e, C.c_double(voxel_leaf), C.c_double(voxelsize),
                                                     _p(codes) if per_point else None, C.byref(r)))
        out = r.as_dict()
        if per_point:
            out["per_point"] = codes[: g[1].value]
        return out

    def evaluate_map(self, gt, voxelsize=0.2, voxel_leaf=0.0):
        """PR / RR of the handle's current map (the get_map view, never copied to the host) against `gt` (erasor_hip_evaluate_map)"""
        kept = []
        g = self._eval_cloud(gt, kept)
        r = EvalResult()
        self._check(lib().erasor_hip_evaluate_map(self._h, *g, C.c_double(voxel_leaf), C.c_double(voxelsize), C.byref(r)))
        return r.as_dict()

    def evaluate_many(self, gt, ests, voxelsize=0.2, voxel_leaf=0.0):
        """evaluate(gt, e, voxelsize, voxel_leaf) for every estimate e of `ests`, from one index of all of them and one query
        (erasor_hip_evaluate_many).  Clouds as for evaluate.  Returns a list of evaluate's dicts, in the order of `ests`."""
        kept = []
        g = self._eval_cloud(gt, kept)
        es = [self._eval_cloud(e, kept) for e in ests]
        k = len(es)
        P = (C.c_void_p * max(k, 1))(*[e[0] for e in es])
        N = (C.c_size_t * max(k, 1))(*[e[1] for e in es])
        D = (C.c_int * max(k, 1))(*[e[2] for e in es])
        rows = (EvalResult * max(k, 1))()
        self._check(lib().erasor_hip_evaluate_many(self._h, *g, P, N, D, C.c_size_t(k), C.c_double(voxel_leaf), C.c_double(voxelsize), rows))
        return [rows[j].as_dict() for j in range(k)]

    def sweep(self, configs, map, scans, T_lidar2body, T_body2origin, T_origin2body, gt, voxelsize=0.2, save_leaf=0.2, concurrency=2,
              eval_batch=0):
        """every Params of `configs` over one sequence, each saved map scored against `gt` (erasor_hip_sweep): the removal_interval gate,
        the map after the last node voxelised at save_leaf, PR / RR with voxelsize.  map / gt: clouds as for evaluate; scans: a list of
        (n, 4) host arrays, or (device pointer, offsets) as align_frames takes them; T_body2origin / T_origin2body: one 4x4 per node.
        Returns one dict per configuration, in the order of `configs`: params (field -> value), status, n_steps, n_map_final, n_saved,
        run_ms and eval (evaluate's dict)."""
        kept = []
        m = self._eval_cloud(map, kept)
        g = self._eval_cloud(gt, kept)
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n = len(offs) - 1
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n, 16) if n else np.zeros((1, 16), np.float32))
        To = _f32(np.asarray(T_origin2body, np.float32).reshape(n, 16) if n else np.zeros((1, 16), np.float32))
        Tl = _f32(T_lidar2body).reshape(16)
        cfg = (Params * max(len(configs), 1))(*configs)
        rows = (SweepRow * max(len(configs), 1))()
        self._check(lib().erasor_hip_sweep(self._h, cfg, C.c_size_t(len(configs)), *m, q[0], q[1], _p(offs), C.c_size_t(n), C.c_int(q[2]),
                                           _p(Tl), _p(Tb), _p(To), *g, C.c_double(save_leaf), C.c_double(voxelsize), C.c_int(concurrency),
                                           C.c_int(eval_batch), rows))
        return [rows[i].as_dict() for i in range(len(configs))]

    # -- PR / RR by class and by dynamic instance (the same on the host: evalmap.evaluate_by_class) --
    def _by_class(self, fn, args, voxel_leaf, voxelsize):
        classes = np.zeros(N_CLASS_KEYS, CLASS_ROW_DTYPE)
        instances = np.zeros(4096, CLASS_ROW_DTYPE)
        nc, ni = C.c_size_t(0), C.c_size_t(0)
        r = EvalResult()
        for attempt in range(2):  # (a second call only when the instances did not fit: then with their exact count)
            rc = fn(self._h, *args, C.c_double(voxel_leaf), C.c_double(voxelsize), _p(classes), C.c_size_t(len(classes)), C.byref(nc),
                    _p(instances), C.c_size_t(len(instances)), C.byref(ni), C.byref(r))
            if rc != E_CAPACITY or attempt:
                break
            instances = np.zeros(max(ni.value, 1), CLASS_ROW_DTYPE)
        self._check(rc)
        out = r.as_dict()
        out["classes"] = class_rows_with_rates(classes[: nc.value])
        out["instances"] = class_rows_with_rates(instances[: ni.value])
        return out

    def evaluate_by_class(self, gt, est, voxelsize=0.2, voxel_leaf=0.0):
        """evaluate's dict plus its breakdown (erasor_hip_evaluate_clouds_by_class): "classes", one row per class key present in either
        cloud, and "instances", one row per whole dynamic label; numpy records with ClassRow's fields plus PR (static rows) / RR
        (dynamic rows).  Clouds and voxel_leaf as for evaluate."""
        kept = []
        g = self._eval_cloud(gt, kept)
        e = self._eval_cloud(est, kept)
        return self._by_class(lib().erasor_hip_evaluate_clouds_by_class, (*g, *e), voxel_leaf, voxelsize)

    def evaluate_map_by_class(self, gt, voxelsize=0.2, voxel_leaf=0.0):
        """evaluate_by_class of the handle's current map (the get_map view, never copied to the host) against `gt`
        (erasor_hip_evaluate_map_by_class)"""
        kept = []
        g = self._eval_cloud(gt, kept)
        return self._by_class(lib().erasor_hip_evaluate_map_by_class, g, voxel_leaf, voxelsize)

    # -- bird's-eye images (viz_kitti_map.cpp, compare_map.cpp as image files; the same on the host: evalmap.render / render_eval) --
    def render_fit(self, cloud=None, res=0.2, margin=2, background=0):
        """the view that contains every finite point of `cloud` (a cloud as for evaluate; None: the handle's map), as a dict with
        evalmap.render_view's keys (erasor_hip_render_fit / _fit_map)"""
        v = RenderView()
        if cloud is None:
            self._check(lib().erasor_hip_render_fit_map(self._h, C.c_double(res), C.c_uint32(margin), C.c_uint32(background), C.byref(v)))
        else:
            kept = []
            c = self._eval_cloud(cloud, kept)
            self._check(lib().erasor_hip_render_fit(self._h, *c, C.c_double(res), C.c_uint32(margin), C.c_uint32(background), C.byref(v)))
        return v.as_dict()

    @staticmethod
    def _render_args(view, mode, target_class, target_instance):
        v = RenderView.of(view)
        img = np.empty((v.height, v.width, 3), np.uint8)
        if mode is None:
            return v, img, (C.byref(v), _p(img), C.c_int(0))
        if mode not in RENDER_MODES:
            raise ValueError("render: mode must be 'label' or 'height'")
        tc = -1 if target_class is None else int(target_class)
        ti = -1 if target_instance is None else int(target_instance)
        return v, img, (C.c_int(RENDER_MODES[mode]), C.c_int32(tc), C.c_int32(ti), C.byref(v), _p(img), C.c_int(0))

    def render(self, cloud, view=None, res=0.2, mode="label", target_class=None, target_instance=None):
        """`cloud` (as for evaluate) as a bird's-eye image (erasor_hip_render_clouds): (uint8 array H x W x 3, stats dict).  view: a dict
        with evalmap.render_view's keys; None fits one at `res`.  mode "label": static / dynamic / target_class (and
        target_instance) by label; "height": one colour, for maps without labels."""
        if view is None:
            view = self.render_fit(cloud, res)
        v, img, tail = self._render_args(view, mode, target_class, target_instance)
        kept = []
        c = self._eval_cloud(cloud, kept)
        st = RenderStats()
        self._check(lib().erasor_hip_render_clouds(self._h, *c, *tail, C.byref(st)))
        return img, st.as_dict()

    def render_map(self, view=None, res=0.2, mode="label", target_class=None, target_instance=None):
        """render of the handle's current map (the get_map view, never copied to the host; erasor_hip_render_map)"""
        if view is None:
            view = self.render_fit(None, res)
        v, img, tail = self._render_args(view, mode, target_class, target_instance)
        st = RenderStats()
        self._check(lib().erasor_hip_render_map(self._h, *tail, C.byref(st)))
        return img, st.as_dict()

    def render_eval(self, gt, est, view=None, res=0.2, voxelsize=0.2, voxel_leaf=0.0):
        """the error map (erasor_hip_render_eval_clouds): evaluate(gt, est, voxelsize, voxel_leaf) and the ground truth drawn by its
        decision per point -- static kept grey, dynamic removed green, static lost blue, dynamic left red, errors on top.  Returns
        (image, stats, evaluate's dict).  view None: fitted to `gt` at `res`."""
        if view is None:
            view = self.render_fit(gt, res)
        v, img, tail = self._render_args(view, None, None, None)
        kept = []
        g = self._eval_cloud(gt, kept)
        e = self._eval_cloud(est, kept)
        st, r = RenderStats(), EvalResult()
        self._check(lib().erasor_hip_render_eval_clouds(self._h, *g, *e, C.c_double(voxel_leaf), C.c_double(voxelsize), *tail, C.byref(st),
                                                        C.byref(r)))
        return img, st.as_dict(), r.as_dict()

    def render_eval_map(self, gt, view=None, res=0.2, voxelsize=0.2, voxel_leaf=0.0):
        """render_eval with the handle's current map as the estimate (erasor_hip_render_eval_map)"""
        if view is None:
            view = self.render_fit(gt, res)
        v, img, tail = self._render_args(view, None, None, None)
        kept = []
        g = self._eval_cloud(gt, kept)
        st, r = RenderStats(), EvalResult()
        self._check(lib().erasor_hip_render_eval_map(self._h, *g, C.c_double(voxel_leaf), C.c_double(voxelsize), *tail, C.byref(st), C.byref(r)))
        return img, st.as_dict(), r.as_dict()

    # -- the estimate-to-ground-truth overlap report (scripts/analysis_runner.py:53-71; the same on the host: evalmap.overlap) --
    def overlap(self, gt, est, voxelsize=0.2, voxel_leaf=0.0, per_point=False):
        """overlap_report's numbers for the estimate `est` against the ground truth `gt` on the device (erasor_hip_overlap_clouds): the
        distance of every estimated point to its nearest ground-truth point, its median / p90 / p99 / max and the percentages below
        0.5*v, v and 2*v.  Clouds as for evaluate.  per_point=True (voxel_leaf 0 only) adds "dist" (float64, one per estimated point)
        and "nearest" (uint32: the smallest ground-truth index at that distance)."""
        kept = []
        g = self._eval_cloud(gt, kept)
        e = self._eval_cloud(est, kept)
        n_e = e[1].value
        dist = np.zeros(max(n_e, 1), np.float64) if per_point else None
        near = np.zeros(max(n_e, 1), np.uint32) if per_point else None
        r = OverlapResult()
        self._check(lib().erasor_hip_overlap_clouds(self._h, *g, *e, C.c_double(voxel_leaf), C.c_double(voxelsize),
                                                    _p(dist) if per_point else None, _p(near) if per_point else None, C.byref(r)))
        out = r.as_dict()
        if per_point:
            out["dist"] = dist[:n_e]
            out["nearest"] = near[:n_e]
        return out

    def overlap_map(self, gt, voxelsize=0.2, voxel_leaf=0.0):
        """overlap_report of the handle's current map (the get_map view, never copied to the host) against `gt`
        (erasor_hip_overlap_map)"""
        kept = []
        g = self._eval_cloud(gt, kept)
        r = OverlapResult()
        self._check(lib().erasor_hip_overlap_map(self._h, *g, C.c_double(voxel_leaf), C.c_double(voxelsize), C.byref(r)))
        return r.as_dict()

    # -- every frame's pose against the map before a run (the reference README's pitfalls 1, 3 and 5; on the host: evalmap.align_frames) --
    def align_frames(self, scans, T_body2origin, T_lidar2body=None, map=None, voxelsize=0.2):
        """overlap_report of every frame's scan, put into the map frame as the reference puts its RViz query (T_lidar2body, the identity
        when None, then T_body2origin[f]), against `map` (a cloud as for evaluate; None: the handle's current map), all frames in one call
        (erasor_hip_align_frames_clouds / _map).  scans: a list of (n, 4) host arrays, or the frames in one device buffer of the
        handle's device as (device pointer, offsets), offsets[f] the first row of frame f and offsets[-1] the row count.  Returns
        (rows, summary): per frame evalmap.overlap's keys plus n_points / n_non_finite, and the report of all frames' kept points
        together."""
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f = len(offs) - 1
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n_f, 16) if n_f else np.zeros((1, 16), np.float32))
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        rows = (AlignRow * max(n_f, 1))()
        summ = OverlapResult()
        tail = (q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), Tl, _p(Tb), C.c_double(voxelsize), rows, C.byref(summ))
        if map is None:
            self._check(lib().erasor_hip_align_frames_map(self._h, *tail))
        else:
            m = self._eval_cloud(map, kept)
            self._check(lib().erasor_hip_align_frames_clouds(self._h, *m, *tail))
        return [rows[f].as_dict() for f in range(n_f)], summ.as_dict()

    # -- every frame's pose refined against the map: point-to-point ICP (on the host: evalmap.refine_poses) --
    def refine_poses(self, scans, T_body2origin, T_lidar2body=None, map=None, max_dist=1.0, eps_t=1e-4, eps_r=1e-5, max_iters=20, min_pairs=100):
        """Every frame's T_body2origin refined against `map` (a cloud as for evaluate; None: the handle's current map) by point-to-point
        ICP, all frames side by side (erasor_hip_refine_poses_clouds / _map): per iteration every scan point's exact nearest map point,
        the pairs within max_dist, Horn's closed-form update, until the update is below eps_t (metres) and eps_r (radians) or max_iters
        updates were made; a frame with fewer than min_pairs pairs keeps its pose.  scans, poses and T_lidar2body as for align_frames.
        Returns (T_refined float64 [n, 4, 4], rows, summary) as evalmap.refine_poses does, bit for bit."""
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f = len(offs) - 1
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n_f, 16) if n_f else np.zeros((1, 16), np.float32))
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        prm = RefineParams(float(max_dist), float(eps_t), float(eps_r), int(max_iters), int(min_pairs))
        rows = (RefineRow * max(n_f, 1))()
        summ = RefineSummary()
        tail = (q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), Tl, _p(Tb), C.byref(prm), rows, C.byref(summ))
        if map is None:
            self._check(lib().erasor_hip_refine_poses_map(self._h, *tail))
        else:
            m = self._eval_cloud(map, kept)
            self._check(lib().erasor_hip_refine_poses_clouds(self._h, *m, *tail))
        T = np.array([list(rows[f].T) for f in range(n_f)], np.float64).reshape(n_f, 4, 4)
        return T, [rows[f].as_dict() for f in range(n_f)], summ.as_dict()

    # -- every frame's pose refined point-to-plane against the map's normals (on the host: evalmap.refine_poses_plane) --
    def refine_poses_plane(self, scans, T_body2origin, T_lidar2body=None, map=None, k=16, max_dist=1.0, max_curvature=1.0, rank_tol=1e-9,
                           eps_t=1e-4, eps_r=1e-5, max_iters=20, min_pairs=100):
        """refine_poses with the residual taken along the map's surface normals (erasor_hip_refine_poses_plane_clouds / _map): the map's
        normals and curvature from its k nearest neighbours are computed once on the device; a scan point within max_dist of a map point
        with a finite normal and a curvature <= max_curvature is a pair; the 6x6 normal equations are solved on the host over the
        directions whose eigenvalue is above rank_tol times the largest.  A row's rank tells how many of the pose's six directions the
        frame's pairs constrain; lambda_ratio how well the weakest one.  scans, poses, T_lidar2body and map as for refine_poses.
        Returns (T_refined float64 [n, 4, 4], rows, summary) as evalmap.refine_poses_plane does, bit for bit."""
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f = len(offs) - 1
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n_f, 16) if n_f else np.zeros((1, 16), np.float32))
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        prm = RefinePlaneParams(float(max_dist), float(eps_t), float(eps_r), int(max_iters), int(min_pairs), int(k), float(max_curvature),
                                float(rank_tol))
        rows = (RefinePlaneRow * max(n_f, 1))()
        summ = RefinePlaneSummary()
        tail = (q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), Tl, _p(Tb), C.byref(prm), rows, C.byref(summ))
        if map is None:
            self._check(lib().erasor_hip_refine_poses_plane_map(self._h, *tail))
        else:
            m = self._eval_cloud(map, kept)
            self._check(lib().erasor_hip_refine_poses_plane_clouds(self._h, *m, *tail))
        T = np.array([list(rows[f].T) for f in range(n_f)], np.float64).reshape(n_f, 4, 4)
        return T, [rows[f].as_dict() for f in range(n_f)], summ.as_dict()

    # -- the see-through check: every scan's range image votes on every map point (on the host: evalmap.visibility) --
    def visibility(self, scans, T_body2origin, T_lidar2body=None, map=None, grid=None, min_range=0.5, max_range=80.0, margin_abs=0.2, margin_rel=0.01,
                   window=1, k=0, min_cos=0.25, min_through=2, hit_weight=1.0, keep=True, image_budget_bytes=0):
        """Every map point voted on by every scan's range image (erasor_hip_visibility_clouds / _map): a point that scans look straight
        through was not static.  scans, poses and T_lidar2body as for align_frames; `map` a cloud as for evaluate, or None for the
        handle's current map (which stays as it is); `grid` from visibility_grid(), or a dict with a sensor's own width, height, col_tan
        and row_tan.  A map point in view of a frame is a hit, occluded, without return or seen through within margin_abs + margin_rel *
        range over a (2 window + 1)^2 pixel window; with k > 0 a see-through at an incidence below min_cos against the point's normal
        (k neighbours) is not counted.  A point is removed iff through >= min_through and through > hit_weight * hit.  The frames are
        handled in batches whose images fit image_budget_bytes (0: VISIBILITY_IMAGE_BUDGET).  Returns (votes (n, 4) uint16: in_view,
        hit, through, occluded; mask uint8, 1 = kept; the kept rows in the order given, or None unless keep; a row per frame; the
        result) as evalmap.visibility does, byte for byte.  A min_through outside 0 .. 2^32 - 1 is a ValueError, as it is there."""
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f = len(offs) - 1
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n_f, 16) if n_f else np.zeros((1, 16), np.float32))
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        if grid is None:
            raise ValueError("visibility: a grid is needed (visibility_grid)")
        if not 0 <= int(min_through) <= 0xFFFFFFFF:
            raise ValueError("visibility: min_through must fit 32 bits")
        col = np.ascontiguousarray(grid["col_tan"], np.float64).reshape(-1)
        row = np.ascontiguousarray(grid["row_tan"], np.float64).reshape(-1)
        W, H = int(grid["width"]), int(grid["height"])
        if 8 <= W <= 4096 and 1 <= H <= 256 and (len(col) != W // 8 - 1 or len(row) != H + 1):
            raise ValueError("visibility: col_tan has width / 8 - 1 entries and row_tan height + 1")
        prm = Visibility(W & 0xFFFFFFFF, H & 0xFFFFFFFF, col.ctypes.data_as(C.POINTER(C.c_double)), row.ctypes.data_as(C.POINTER(C.c_double)),
                         float(min_range), float(max_range), float(margin_abs), float(margin_rel), int(window) & 0xFFFFFFFF, int(k) & 0xFFFFFFFF,
                         float(min_cos), int(min_through), 0, float(hit_weight), int(image_budget_bytes))
        if map is None:
            head, n = (), self._map_n()
            fn = lib().erasor_hip_visibility_map
        else:
            head = self._eval_cloud(map, kept)
            n = head[1].value
            fn = lib().erasor_hip_visibility_clouds
        votes = np.empty((max(n, 1), 4), np.uint16)
        mask = np.empty(max(n, 1), np.uint8)
        out = np.empty((max(n, 1), 4), np.float32) if keep else None
        rows = (VisibilityRow * max(n_f, 1))()
        r = VisibilityResult()
        self._check(fn(self._h, *head, q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), Tl, _p(Tb), C.byref(prm),
                       _p(votes), _p(mask), _p(out) if keep else None, C.c_size_t(n if keep else 0), rows, C.byref(r)))
        return votes[:n], mask[:n], (out[: r.n_kept] if keep else None), [rows[f].as_dict() for f in range(n_f)], r.as_dict()

    # -- carving free space: every scan's rays walked through the map's voxels (on the host: evalmap.carve) --
    def carve(self, scans, T_body2origin, T_lidar2body=None, map=None, voxel=0.2, min_range=0.5, max_range=80.0, stop_short=0, logodds=None, keep=True):
        """Free space carved out of a map, OctoMap's way (erasor_hip_carve_clouds / _map): the map goes into voxels of `voxel` metres, every
        ray of every scan is walked through them from the lidar's origin to its return; a voxel that rays pass through is free in that
        frame, one that rays end in is hit (hits first), and the frames are integrated in order as clamped float32 log-odds (`logodds`: a
        dict with l_init, l_hit, l_miss, l_min, l_max, l_thr; None: carve_logodds()).  A point is removed iff its voxel's log-odds end
        below l_thr.  The last stop_short voxels before a ray's end give no free evidence.  scans, poses and T_lidar2body as for
        visibility; `map` a cloud as for evaluate, or None for the handle's current map (which stays as it is).  Returns (votes (n, 2)
        uint16: the hits and misses of the point's voxel; logodds (n,) float32; mask uint8, 1 = kept; the kept rows in the order given,
        or None unless keep; a row per frame; the result) as evalmap.carve does, byte for byte."""
        from . import evalmap
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f = len(offs) - 1
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n_f, 16) if n_f else np.zeros((1, 16), np.float32))
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        lg = evalmap.carve_logodds() if logodds is None else logodds
        if not 0 <= int(stop_short) <= 0xFFFFFFFF:
            raise ValueError("carve: stop_short must fit 32 bits")
        prm = Carve(float(voxel), float(min_range), float(max_range), *[float(lg[k]) for k in evalmap.CARVE_LOGODDS_FIELDS], int(stop_short), 0)
        if map is None:
            head, n = (), self._map_n()
            fn = lib().erasor_hip_carve_map
        else:
            head = self._eval_cloud(map, kept)
            n = head[1].value
            fn = lib().erasor_hip_carve_clouds
        votes = np.empty((max(n, 1), 2), np.uint16)
        lo = np.empty(max(n, 1), np.float32)
        mask = np.empty(max(n, 1), np.uint8)
        out = np.empty((max(n, 1), 4), np.float32) if keep else None
        rows = (CarveRow * max(n_f, 1))()
        r = CarveResult()
        self._check(fn(self._h, *head, q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), Tl, _p(Tb), C.byref(prm),
                       _p(votes), _p(lo), _p(mask), _p(out) if keep else None, C.c_size_t(n if keep else 0), rows, C.byref(r)))
        return votes[:n], lo[:n], mask[:n], (out[: r.n_kept] if keep else None), [rows[f].as_dict() for f in range(n_f)], r.as_dict()

    # -- every scan's ground, and the map's ground points by vote (on the host: evalmap.ground_scans / ground_votes) --
    def _ground_params(self, grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, kept, min_votes=1,
                       ratio=0.5, keep=1, work_budget_bytes=0):
        """erasor_ground from the arguments (its tables are appended to `kept`, which must outlive the call)"""
        from . import evalmap
        g = evalmap.ground_grid() if grid is None else grid
        S = int(g["n_sectors"])
        col = np.ascontiguousarray(g["col_tan"], np.float64).reshape(-1)
        edge = np.ascontiguousarray(g["ring_edge"], np.float64).reshape(-1)
        R = len(edge) - 1
        if 8 <= S <= 512 and len(col) != S // 8 - 1:
            raise ValueError("ground: col_tan has n_sectors / 8 - 1 entries")
        for v in (num_lpr, iters, min_points, min_votes):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("ground: num_lpr, iters, min_points and min_votes must fit 32 bits")
        tabs = []
        for t in (elevation, flatness):
            a = None if t is None else np.ascontiguousarray(t, np.float64).reshape(-1)
            if a is not None and len(a) != max(R, 0):
                raise ValueError("ground: elevation and flatness have n_rings entries")
            tabs.append(a)
        kept += [col, edge] + tabs
        dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        return Ground(max(R, 0) & 0xFFFFFFFF, S & 0xFFFFFFFF, dp(edge), dp(col), dp(tabs[0]), dp(tabs[1]), int(num_lpr), int(iters), int(min_points),
                      int(min_votes), float(th_seeds), float(th_dist), float(min_z), float(uprightness), float(ratio), 1 if keep else 0, 0,
                      int(work_budget_bytes)), max(R, 1), S

    def ground_scans(self, scans, grid=None, num_lpr=10, th_seeds=0.5, th_dist=0.15, iters=3, min_points=10, min_z=-3.03, uprightness=0.707,
                     elevation=None, flatness=None, patches=False):
        """Every scan's ground (erasor_hip_ground_scans): R-GPF (erasor.cpp:183-294) on every polar patch of every scan, all frames in one
        call.  scans: a list of XYZI arrays in the lidar frame, or (device_ptr, offsets); grid: ground_grid() or a dict with n_sectors,
        col_tan and ring_edge (None: ground_grid()); elevation, flatness: tables of n_rings entries (None: both gates off).  A point's code:
        1 ground, 0 judged and not ground, 2 not judged (out of range, a sparse or degenerate patch), 255 non-finite.  Returns (codes uint8,
        all frames one after another; a row per frame; their sums; with `patches` the table [n_frames, n_rings, n_sectors] of
        evalmap.GROUND_PATCH_DTYPE, else None) as evalmap.ground_scans does, byte for byte."""
        from . import evalmap
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f, n = len(offs) - 1, q[1].value
        prm, R, S = self._ground_params(grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, kept)
        codes = np.empty(max(n, 1), np.uint8)
        rows = (GroundRow * max(n_f, 1))()
        tab = np.zeros((n_f, R, S), evalmap.GROUND_PATCH_DTYPE) if patches else None
        r = GroundResult()
        self._check(lib().erasor_hip_ground_scans(self._h, q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), C.byref(prm), _p(codes), rows,
                                                  tab.ctypes.data_as(C.c_void_p) if patches and tab.size else None, C.byref(r)))
        res = {k: v for k, v in r.as_dict().items() if not k.startswith("n_map_") and k != "n_kept"}
        return codes[:n], [rows[f].as_dict() for f in range(n_f)], res, tab

    def ground_votes(self, T_body2origin, T_lidar2body=None, map=None, grid=None, num_lpr=10, th_seeds=0.5, th_dist=0.15, iters=3, min_points=10,
                     min_z=-3.03, uprightness=0.707, elevation=None, flatness=None, min_votes=1, ratio=0.5, keep=1, work_budget_bytes=0):
        """The map's ground points by vote (erasor_hip_ground_votes_clouds / _map): what every frame sees of the map is segmented exactly
        as a scan (ground_scans), and a map point is ground iff ground >= min_votes and ground > ratio * seen over the frames that judged
        it.  Poses and T_lidar2body as for visibility; `map` a cloud as for evaluate, or None for the handle's current map (which stays as
        it is).  The frames go in batches of work_budget_bytes / (n_map * 16) frames (0: GROUND_WORK_BUDGET); the result does not depend on
        it.  Returns (votes (n, 2) uint16: seen, ground; mask uint8, 1 = ground; the ground rows (keep = 1) or the rest (keep = 0) in map
        order; a row per frame; the result) as evalmap.ground_votes does, byte for byte."""
        kept = []
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(-1, 16))
        n_f = len(Tb)
        if not n_f:
            Tb = np.zeros((1, 16), np.float32)
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        prm, _, _ = self._ground_params(grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, kept, min_votes,
                                        ratio, keep, work_budget_bytes)
        if map is None:
            head, n = (), self._map_n()
            fn = lib().erasor_hip_ground_votes_map
        else:
            head = self._eval_cloud(map, kept)
            n = head[1].value
            fn = lib().erasor_hip_ground_votes_clouds
        votes = np.empty((max(n, 1), 2), np.uint16)
        mask = np.empty(max(n, 1), np.uint8)
        out = np.empty((max(n, 1), 4), np.float32)
        rows = (GroundRow * max(n_f, 1))()
        r = GroundResult()
        self._check(fn(self._h, *head, Tl, _p(Tb), C.c_size_t(n_f), C.byref(prm), _p(votes), _p(mask), _p(out), C.c_size_t(n), rows, C.byref(r)))
        res = {"n_points": int(r.n_map_points), "n_ground": int(r.n_map_ground), "n_ground_dynamic": int(r.n_map_ground_dynamic),
               "n_ground_static": int(r.n_map_ground_static), "n_unseen": int(r.n_map_unseen), "n_kept": int(r.n_kept),
               "n_gathered": int(r.n_points), "n_judged": int(r.n_judged)}
        return votes[:n], mask[:n], out[: r.n_kept], [rows[f].as_dict(gathered=True) for f in range(n_f)], res

    # -- every scan's points labelled static or moving from a cleaned map (on the host: evalmap.label_scans) --
    def label_scans(self, scans, T_body2origin, T_lidar2body=None, static_map=None, raw_map=None, tau=None, voxelsize=0.2, split=None):
        """Every point of every scan classified against the cleaned map `static_map` (a cloud as for evaluate; None: the handle's current
        map) and, optionally, the raw map `raw_map`, all frames in one call (erasor_hip_label_scans_clouds / _map): 0 static (a static-map
        point within tau), 1 dynamic, 2 unknown (a raw map was given and has no point within tau either), 255 dropped.  scans and poses as
        for align_frames; tau: voxelsize * np.sqrt(3) / 2 when None.  Returns (codes, rows, summary) as evalmap.label_scans does; with
        split = 0, 1 or 2 also the rows of that code, as given, one (k, 4) array per frame."""
        from . import evalmap
        kept = []
        if isinstance(scans, tuple):
            ptr, offsets = scans
            offs = np.ascontiguousarray(offsets, np.uint64)
            q = (C.c_void_p(ptr), C.c_size_t(int(offs[-1]) if len(offs) else 0), 1)
        else:
            a = [_f32(s).reshape(-1, 4) for s in scans]
            offs = np.zeros(len(a) + 1, np.uint64)
            offs[1:] = np.cumsum([len(s) for s in a], dtype=np.uint64)
            cat = _f32(np.concatenate(a) if a else np.zeros((0, 4), np.float32))
            kept.append(cat)
            q = (_p(cat), C.c_size_t(len(cat)), 0)
        n_f, n_pts = len(offs) - 1, int(q[1].value)
        Tb = _f32(np.asarray(T_body2origin, np.float32).reshape(n_f, 16) if n_f else np.zeros((1, 16), np.float32))
        if T_lidar2body is not None:
            kept.append(_f32(T_lidar2body).reshape(16))
        Tl = None if T_lidar2body is None else _p(kept[-1])
        tau = evalmap.label_tau(voxelsize) if tau is None else float(tau)
        raw = (None, C.c_size_t(0), 0) if raw_map is None else self._eval_cloud(raw_map, kept)
        codes = np.zeros(max(n_pts, 1), np.uint8)
        out = np.empty((max(n_pts, 1), 4), np.float32) if split is not None else None
        out_offs = np.zeros(n_f + 1, np.uint64)
        rows = (ScanLabelRow * max(n_f, 1))()
        summ = ScanLabelRow()
        tail = (*raw, C.c_int(int(raw_map is not None)), q[0], q[1], _p(offs), C.c_size_t(n_f), C.c_int(q[2]), Tl, _p(Tb), C.c_double(tau), _p(codes),
                C.c_int(0 if split is None else int(split)), None if split is None else _p(out), C.c_size_t(0 if split is None else len(out)),
                None if split is None else _p(out_offs), rows, C.byref(summ))
        if static_map is None:
            self._check(lib().erasor_hip_label_scans_map(self._h, *tail))
        else:
            m = self._eval_cloud(static_map, kept)
            self._check(lib().erasor_hip_label_scans_clouds(self._h, *m, *tail))
        o = offs.astype(np.int64)
        res = ([codes[o[f]:o[f + 1]].copy() for f in range(n_f)], [rows[f].as_dict() for f in range(n_f)], summ.as_dict())
        if split is None:
            return res
        oo = out_offs.astype(np.int64)
        return res + ([out[oo[f]:oo[f + 1]].copy() for f in range(n_f)],)

    # -- a cloud as connected objects: Euclidean clustering (on the host: evalmap.cluster) --
    def _cluster(self, fn, head, n, tol, min_size, max_size, ids, keep):
        r = ClusterResult()
        tail = (C.c_double(tol), C.c_size_t(int(min_size)), C.c_size_t(int(max_size)))
        id_buf = np.empty(max(n, 1), np.uint32) if ids else None
        rows = np.zeros(max(min(n, 1 << 16), 1), CLUSTER_ROW_DTYPE)
        kept = np.empty((max(n, 1), 4), np.float32) if keep else None
        for attempt in range(2):  # (a second call only when the rows did not fit: then with their exact count; the ids came with the first)
            rc = fn(self._h, *head, *tail, _p(id_buf) if ids and not attempt else None, _p(rows), C.c_size_t(len(rows)), _p(kept) if keep else None,
                    C.c_size_t(len(kept) if keep else 0), C.byref(r))
            if rc != E_CAPACITY or attempt:
                break
            rows = np.zeros(max(int(r.n_listed), 1), CLUSTER_ROW_DTYPE)
        self._check(rc)
        return (rows[: r.n_listed], id_buf[:n] if ids else None, kept[: r.n_points_listed] if keep else None, r.as_dict())

    def cluster(self, cloud, tol, min_size=1, max_size=0, ids=True, keep=False):
        """Euclidean clustering of `cloud` (as for evaluate) on the device (erasor_hip_cluster_clouds): the connected components of
        "within tol" (float64 distances), a cluster listed when min_size <= n_points and (max_size == 0 or n_points <= max_size).
        Returns (rows, ids, kept, result) as evalmap.cluster does: CLUSTER_ROW_DTYPE records in increasing `first`; per point the index
        of its cluster among the rows or CLUSTER_NONE (None unless ids); the rows of the points of listed clusters in the order given
        (None unless keep: the residue filter); and the result's counts as a dict."""
        kept = []
        c = self._eval_cloud(cloud, kept)
        return self._cluster(lib().erasor_hip_cluster_clouds, c, c[1].value, tol, min_size, max_size, ids, keep)

    def cluster_map(self, tol, min_size=1, max_size=0, ids=True, keep=False):
        """cluster of the handle's current map (the get_map view, never copied to the host; erasor_hip_cluster_map)"""
        n = C.c_size_t(0)
        if lib().erasor_hip_map_size(self._h, C.byref(n)) != 0:  # (no map, a step in flight: the call itself says so)
            n = C.c_size_t(0)
        return self._cluster(lib().erasor_hip_cluster_map, (), n.value, tol, min_size, max_size, ids, keep)

    # -- the decision per object: a method's per-point votes spread over clusters, fragments reverted (on the host: evalmap.object_vote) --
    def _object_vote(self, fn, head, tail_n, n, votes, ground, prm, ids, keep):
        v = np.ascontiguousarray(np.asarray(votes, np.uint8).reshape(-1))
        g = None if ground is None else np.ascontiguousarray(np.asarray(ground, np.uint8).reshape(-1))
        if len(v) != n or (g is not None and len(g) != n):
            raise ErasorError(-1, "object_vote: votes and ground must have one entry per point")
        if not (0 <= prm["vote_thr"] < 1 << 32 and prm["min_size"] >= 0 and prm["max_size"] >= 0 and prm["min_voted"] >= 0):
            raise ErasorError(-1, "object_vote: vote_thr must be within 1 .. 255 and the size limits not negative")
        P = ObjectVoteParams(tol=prm["tol"], max_extent=prm["max_extent"], remove_ratio=prm["remove_ratio"], revert_ratio=prm["revert_ratio"],
                             min_size=min(int(prm["min_size"]), 2 ** 64 - 1), max_size=min(int(prm["max_size"]), 2 ** 64 - 1),
                             min_voted=min(int(prm["min_voted"]), 2 ** 64 - 1), vote_thr=int(prm["vote_thr"]), ground_keep=int(bool(prm["ground_keep"])))
        r = ObjectVoteResult()
        v = v if n else np.zeros(1, np.uint8)
        mask = np.empty(max(n, 1), np.uint8)
        id_buf = np.empty(max(n, 1), np.uint32) if ids else None
        rows = np.zeros(max(min(n, 1 << 16), 1), OBJECT_ROW_DTYPE)
        kept = np.empty((max(n, 1), 4), np.float32) if keep else None
        for attempt in range(2):  # (a second call only when the rows did not fit: then with their exact count; mask and ids came with the first)
            rc = fn(self._h, *head, _p(v), None if g is None else _p(g), *tail_n, C.byref(P), None if attempt else _p(mask),
                    _p(id_buf) if ids and not attempt else None, _p(rows), C.c_size_t(len(rows)), _p(kept) if keep else None,
                    C.c_size_t(len(kept) if keep else 0), C.byref(r))
            if rc != E_CAPACITY or attempt:
                break
            rows = np.zeros(max(int(r.n_touched), 1), OBJECT_ROW_DTYPE)
        self._check(rc)
        return (mask[:n], rows[: r.n_touched], id_buf[:n] if ids else None, kept[: r.n_points - r.n_removed] if keep else None, r.as_dict())

    def object_vote(self, cloud, votes, ground=None, tol=0.5, vote_thr=1, min_size=1, max_size=0, max_extent=0.0, remove_ratio=0.5,
                    revert_ratio=0.0, min_voted=1, ground_keep=True, ids=True, keep=True):
        """A removal method's per-point votes decided per object, on the device (erasor_hip_object_vote_clouds).  `cloud` as for
        evaluate; `votes`: uint8 per point, voted iff >= vote_thr (votes_from_masks turns the 1 = kept masks of visibility, carve and a
        step into them; their sum with vote_thr=2 of three is the majority); `ground`: uint8 per point (ground_votes' mask, 1 = ground)
        or None.  Ground points are cut out of the graph -- the ground connects everything -- and kept if ground_keep.  Every cluster
        of the other points at `tol` is removed whole when at least min_voted and the share remove_ratio of its points are voted, kept
        whole when at most the share revert_ratio is, and left to its per-point votes otherwise, or when it is no object: fewer than
        min_size or more than max_size points, a box side above max_extent.  revert_ratio is 0 by default, so nothing is reverted:
        with an incomplete ground mask one huge cluster holds every object and its tiny vote share would wipe the votes out -- set
        max_size or max_extent before using revert_ratio.  Returns (mask, rows, ids, kept, result) as evalmap.object_vote does: uint8
        per point, 1 = kept; OBJECT_ROW_DTYPE records of the touched clusters in increasing `first`; per point its row or OBJECT_NONE
        (None unless ids); the rows with mask 1 in the order given (None unless keep: pass it to set_map); the counts as a dict."""
        hold = []
        c = self._eval_cloud(cloud, hold)
        prm = dict(tol=tol, vote_thr=vote_thr, min_size=min_size, max_size=max_size, max_extent=max_extent, remove_ratio=remove_ratio,
                   revert_ratio=revert_ratio, min_voted=min_voted, ground_keep=ground_keep)
        return self._object_vote(lib().erasor_hip_object_vote_clouds, c, (), c[1].value, votes, ground, prm, ids, keep)

    def object_vote_map(self, votes, ground=None, tol=0.5, vote_thr=1, min_size=1, max_size=0, max_extent=0.0, remove_ratio=0.5,
                        revert_ratio=0.0, min_voted=1, ground_keep=True, ids=True, keep=True):
        """object_vote over the handle's current map (the get_map view, never copied to the host; erasor_hip_object_vote_map): votes and
        ground index that view, as the masks of visibility, carve and ground_votes with map=None do"""
        n = len(np.asarray(votes).reshape(-1))
        prm = dict(tol=tol, vote_thr=vote_thr, min_size=min_size, max_size=max_size, max_extent=max_extent, remove_ratio=remove_ratio,
                   revert_ratio=revert_ratio, min_voted=min_voted, ground_keep=ground_keep)
        return self._object_vote(lib().erasor_hip_object_vote_map, (), (C.c_size_t(n),), n, votes, ground, prm, ids, keep)

    def residue(self, gt, est, tol=0.5, voxelsize=0.2, voxel_leaf=0.0, min_size=1):
        """The ghost objects a method left: the dynamic points of the labelled ground truth `gt` that evaluate(gt, est, voxelsize) found
        kept (EVAL_KEPT_DYNAMIC), clustered at `tol` -- boxes and sizes, no instance labels needed.  Host clouds; voxel_leaf > 0: both
        voxelised at that leaf first.  Returns (rows, ids, points, result): cluster's rows, ids and result over `points`, the kept
        dynamic ground-truth rows in ground-truth order."""
        g = _f32(gt).reshape(-1, 4)
        e = _f32(est).reshape(-1, 4)
        if voxel_leaf > 0:
            g = self.voxelize_preserving_labels(g, voxel_leaf)
            e = self.voxelize_preserving_labels(e, voxel_leaf)
        codes = self.evaluate(g, e, voxelsize, 0.0, per_point=True)["per_point"]
        pts = np.ascontiguousarray(g[codes == EVAL_KEPT_DYNAMIC])
        rows, ids, _, res = self.cluster(pts, tol, min_size)
        return rows, ids, pts, res

    # -- how dense the cloud is around each point: k nearest neighbours, radius counts, the outlier filters (on the host: evalmap.knn /
    # radius_count / density_filter) --
    def _map_n(self):
        n = C.c_size_t(0)
        if lib().erasor_hip_map_size(self._h, C.byref(n)) != 0:  # (no map, a step in flight: the call itself says so)
            return 0
        return n.value

    def _knn(self, fn, head, n, k, neighbours):
        k = int(k)
        kk = k if 1 <= k <= 32 else 1  # (a refused k needs no buffers)
        r = KnnResult()
        kth = np.empty(max(n, 1), np.float64)
        mean = np.empty(max(n, 1), np.float64)
        ni = np.empty((max(n, 1), kk), np.uint32) if neighbours else None
        nd = np.empty((max(n, 1), kk), np.float64) if neighbours else None
        self._check(fn(self._h, *head, C.c_uint32(k & 0xFFFFFFFF), _p(ni) if neighbours else None, _p(nd) if neighbours else None, _p(kth), _p(mean),
                       C.byref(r)))
        out = {"n_points": int(r.n_points), "n_short": int(r.n_short), "k": k, "kth": kth[:n], "mean": mean[:n], "kth_stats": r.kth.as_dict(),
               "mean_stats": r.mean.as_dict()}
        if neighbours:
            out["nbr_idx"] = ni[:n]
            out["nbr_dist"] = nd[:n]
        return out

    def knn(self, cloud, k, neighbours=False):
        """Every point's k nearest other points inside `cloud` (as for evaluate), 1 <= k <= 32, on the device (erasor_hip_knn_clouds):
        float64 distances, neighbours ordered by (d2, index), self excluded by index.  Returns evalmap.knn's dict: n_points, n_short, k,
        kth and mean (float64 per point; +inf where a point has fewer than k other points), kth_stats / mean_stats, and with
        neighbours=True nbr_idx (n, k) uint32 / nbr_dist (n, k) float64, padded with KNN_NONE / +inf."""
        kept = []
        c = self._eval_cloud(cloud, kept)
        return self._knn(lib().erasor_hip_knn_clouds, c, c[1].value, k, neighbours)

    def knn_map(self, k, neighbours=False):
        """knn of the handle's current map (the get_map view, never copied to the host; erasor_hip_knn_map)"""
        return self._knn(lib().erasor_hip_knn_map, (), self._map_n(), k, neighbours)

    def _radius_count(self, fn, head, n, r):
        st = ScoreStats()
        cnt = np.empty(max(n, 1), np.uint32)
        self._check(fn(self._h, *head, C.c_double(r), _p(cnt), C.byref(st)))
        return cnt[:n], st.as_dict()

    def radius_count(self, cloud, r):
        """(count, stats) as evalmap.radius_count: per point the number of other points of `cloud` within r (float64 d2 <= r*r), uint32,
        and the counts' statistics (erasor_hip_radius_count_clouds)"""
        kept = []
        c = self._eval_cloud(cloud, kept)
        return self._radius_count(lib().erasor_hip_radius_count_clouds, c, c[1].value, r)

    def radius_count_map(self, r):
        """radius_count of the handle's current map (erasor_hip_radius_count_map)"""
        return self._radius_count(lib().erasor_hip_radius_count_map, (), self._map_n(), r)

    def _density_filter(self, fn, head, n, score, k, radius, rule, thr, mul, min_neighbors, keep):
        f = DensityFilter(DENSITY_SCORES.get(score, -1) if isinstance(score, str) else int(score),
                          DENSITY_RULES.get(rule, -1) if isinstance(rule, str) else int(rule), int(k) & 0xFFFFFFFF, min(max(int(min_neighbors), 0), 0xFFFFFFFF),
                          float(radius), float(thr), float(mul))
        r = DensityResult()
        mask = np.empty(max(n, 1), np.uint8)
        kept = np.empty((max(n, 1), 4), np.float32) if keep else None
        self._check(fn(self._h, *head, C.byref(f), _p(mask), _p(kept) if keep else None, C.c_size_t(n if keep else 0), C.byref(r)))
        return mask[:n], (kept[: r.n_kept] if keep else None), r.as_dict()

    def density_filter(self, cloud, score="mean", k=16, radius=0.5, rule="mad", thr=0.5, mul=2.0, min_neighbors=2, keep=True):
        """`cloud` (as for evaluate) filtered by its density on the device (erasor_hip_density_filter_clouds).  score "kth" / "mean" (the
        k-th neighbour's distance / the mean distance of the k nearest) with rule "abs" (keep iff score <= thr) or "mad" (thr = m + mul
        * (1.4826 * mad) from the median and the median absolute deviation of the finite scores); score "count": keep iff at least
        min_neighbors other points lie within radius.  score "mean" with "mad" is pcl::StatisticalOutlierRemoval's selection up to its
        sigma rule, "count" is pcl::RadiusOutlierRemoval's.  Returns (mask, kept, result) as evalmap.density_filter does: uint8 per
        point, the kept rows in the order given (None unless keep) and the result's dict."""
        held = []
        c = self._eval_cloud(cloud, held)
        return self._density_filter(lib().erasor_hip_density_filter_clouds, c, c[1].value, score, k, radius, rule, thr, mul, min_neighbors, keep)

    def density_filter_map(self, score="mean", k=16, radius=0.5, rule="mad", thr=0.5, mul=2.0, min_neighbors=2, keep=True):
        """density_filter of the handle's current map, which stays as it is (erasor_hip_density_filter_map)"""
        return self._density_filter(lib().erasor_hip_density_filter_map, (), self._map_n(), score, k, radius, rule, thr, mul, min_neighbors, keep)

    # -- the surface a point lies on: normals, curvature, covariance eigenvalues (on the host: evalmap.normals) --
    def _normals(self, fn, head, n, k, viewpoint, eigenvalues):
        r = NormalsResult()
        v = None if viewpoint is None else (C.c_double * 3)(*[float(x) for x in np.asarray(viewpoint, np.float64).reshape(3)])
        nrm = np.empty((max(n, 1), 3), np.float32)
        curv = np.empty(max(n, 1), np.float64)
        eig = np.empty((max(n, 1), 3), np.float64) if eigenvalues else None
        self._check(fn(self._h, *head, C.c_uint32(int(k) & 0xFFFFFFFF), v, _p(nrm), _p(curv), _p(eig) if eigenvalues else None, C.byref(r)))
        res = {**{f: int(getattr(r, f)) for f in ("n_points", "n_short", "n_degenerate", "n_ambiguous", "n_flipped")}, "k": int(k),
               "curvature_stats": r.curvature.as_dict()}
        return nrm[:n], curv[:n], (eig[:n] if eigenvalues else None), res

    def normals(self, cloud, k=16, viewpoint=None, eigenvalues=False):
        """Every point's surface normal and curvature from itself and its k nearest other points inside `cloud` (as for evaluate),
        2 <= k <= 32, on the device (erasor_hip_normals_clouds): the covariance's smallest eigenvector by a Jacobi solve in float64,
        turned towards `viewpoint` (three numbers) or upwards (None); pcl::NormalEstimation's job.  Returns (normals (n, 3) float32,
        curvature (n,) float64, eigenvalues (n, 3) float64 ascending or None, result) as evalmap.normals does; points with fewer
        than k other points and neighbourhoods without extent are NaN and counted in the result."""
        kept = []
        c = self._eval_cloud(cloud, kept)
        return self._normals(lib().erasor_hip_normals_clouds, c, c[1].value, k, viewpoint, eigenvalues)

    def normals_map(self, k=16, viewpoint=None, eigenvalues=False):
        """normals of the handle's current map (the get_map view, never copied to the host; erasor_hip_normals_map)"""
        return self._normals(lib().erasor_hip_normals_map, (), self._map_n(), k, viewpoint, eigenvalues)

    # -- maps without labels (fill_removert_intensity.cpp:24-59, compare_complement.cpp:43-75; on the host: evalmap.label_from /
    # evalmap.static_complement) --
    def label_map(self, src, medium, leaf=0.2):
        """label_map on the device (erasor_hip_label_map): `src` voxelised by VoxelGrid at `leaf`, each centroid labelled with the
        intensity of its nearest `medium` point (float32 d^2 as KdTreeFLANN, the lowest index on ties).  Clouds as for evaluate.
        Returns (rows, {"n_src", "n_out", "n_tied", "passthrough"})."""
        kept = []
        s = self._eval_cloud(src, kept)
        m = self._eval_cloud(medium, kept)
        out = np.empty((max(s[1].value, 1), 4), np.float32)
        r = LabelResult()
        self._check(lib().erasor_hip_label_map(self._h, *s, *m, C.c_double(leaf), _p(out), C.c_size_t(len(out)), C.byref(r)))
        return out[: r.n_out].copy(), r.as_dict()

    def static_complement(self, est, gt):
        """calc_complement on the device (erasor_hip_static_complement): the static points of the labelled ground truth `gt` whose
        nearest point of the estimate `est` has a float32 d^2 > 0.03, in ground-truth order.  Clouds as for evaluate.
        Returns (rows, {"n_gt", "n_gt_static", "n_lost", "n_label_out_of_range"})."""
        kept = []
        e = self._eval_cloud(est, kept)
        g = self._eval_cloud(gt, kept)
        out = np.empty((max(g[1].value, 1), 4), np.float32)
        r = ComplementResult()
        self._check(lib().erasor_hip_static_complement(self._h, *e, *g, _p(out), C.c_size_t(len(out)), C.byref(r)))
        return out[: r.n_lost].copy(), r.as_dict()

    # -- mapgen (src/mapgen/mapgen.hpp) --
    def mapgen_begin(self, leafsize, is_large_scale=False):
        self._check(lib().erasor_hip_mapgen_begin(self._h, C.c_double(leafsize), C.c_int(int(is_large_scale))))

    def mapgen_accum(self, scan, T_pose, T_lidar2origin=None):
        scan = _f32(scan).reshape(-1, 4)
        tp = _f32(T_pose).reshape(16)
        tl = _f32(T_lidar2origin).reshape(16) if T_lidar2origin is not None else None
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_mapgen_accum(self._h, _p(scan), C.c_size_t(len(scan)), _p(tp), _p(tl) if tl is not None else None,
                                                  C.byref(n)))
        return n.value

    def mapgen_get(self, which):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_mapgen_get(self._h, C.c_int(which), None, C.c_size_t(0), C.byref(n)))
        out = np.empty((max(n.value, 1), 4), np.float32)
        self._check(lib().erasor_hip_mapgen_get(self._h, C.c_int(which), _p(out), C.c_size_t(len(out)), C.byref(n)))
        return out[: n.value].copy()

    def mapgen_save(self):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_mapgen_get(self._h, C.c_int(2), None, C.c_size_t(0), C.byref(n)))
        out = np.empty((max(n.value, 1), 4), np.float32)
        self._check(lib().erasor_hip_mapgen_save(self._h, _p(out), C.c_size_t(len(out)), C.byref(n)))
        return out[: n.value].copy()

    def count_static_dynamic(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().erasor_hip_count_static_dynamic(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- measurement --
    def profiling(self, on):
        self._check(lib().erasor_hip_profiling(self._h, C.c_int(int(on))))

    def profile_reset(self):
        self._check(lib().erasor_hip_profile_reset(self._h))

    def profile_get(self):
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_profile_get(self._h, None, None, None, C.c_size_t(0), C.byref(n)))
        k = n.value
        names = (C.c_char_p * max(k, 1))()
        ms = (C.c_double * max(k, 1))()
        cnt = (C.c_uint64 * max(k, 1))()
        self._check(lib().erasor_hip_profile_get(self._h, names, ms, cnt, C.c_size_t(k), C.byref(n)))
        return {names[i].decode(): (ms[i], int(cnt[i])) for i in range(k)}

    def voi_split_bytes(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().erasor_hip_voi_split_bytes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def ahead_split_counts(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().erasor_hip_ahead_split_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def overlap_counts(self):
        """(steps whose front was launched beside the previous step's per-bin launch, steps that took it)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().erasor_hip_overlap_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def overlap_auto(self):
        """(mode the next step will use: 1 overlapped / 0 plain, period measured plain, period measured overlapped [us; 0: not yet])"""
        m, a, b = C.c_int(0), C.c_double(0), C.c_double(0)
        self._check(lib().erasor_hip_overlap_auto(self._h, C.byref(m), C.byref(a), C.byref(b)))
        return m.value, a.value, b.value

    def stream_pipes(self):
        """where the handle's streams landed (erasor_hip_stream_pipes): {"pipes": [main, q0, q1, early] as me * 4 + pipe, -1 unknown or
        not created, "n_pads": idle pad streams kept, "distinct_seen": different pipes the rehearsal saw}"""
        p = (C.c_int * 4)()
        a, b = C.c_int(0), C.c_int(0)
        self._check(lib().erasor_hip_stream_pipes(self._h, p, C.byref(a), C.byref(b)))
        return {"pipes": [int(v) for v in p], "n_pads": a.value, "distinct_seen": b.value}

    def step_log(self):
        """the last collected steps (up to 256), oldest first, as dicts: step, period_us (0: not consecutive), n_alloc / n_free / n_create
        (allocations, frees, stream or event creations inside the step's calls and the announcements before it), reserved, use_ov, deep,
        sampled, grown (1: map scratch enlarged, 2: outskirts rebuilt), and the overlap decision's mode / block / skip before the step's sample (erasor_hip_step_log)"""
        buf = (StepLogEntry * 256)()
        n = C.c_size_t(0)
        self._check(lib().erasor_hip_step_log(self._h, buf, C.c_size_t(256), C.byref(n)))
        return [{f: getattr(buf[k], f) for f, _ in StepLogEntry._fields_} for k in range(n.value)]

    def chain_batch(self, n_scans, lead=3):
        """the query chains of `n_scans` announced nodes share one set of launches (erasor_hip_chain_batch); 1: every chain on its own"""
        self._check(lib().erasor_hip_chain_batch(self._h, C.c_int(n_scans), C.c_int(lead)))

    def chain_batch_counts(self):
        """(sets of shared launches made so far, chains that went into them)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(lib().erasor_hip_chain_batch_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def chain_timing(self, reset=False):
        """(average span of the main stream's chain per step, average time between a step's end and the next chunk scan, steps, average
        period chunk scan -> chunk scan) -- on the device's own clock (erasor_hip_chain_timing)."""
        a, b, p, n = C.c_double(0), C.c_double(0), C.c_double(0), C.c_uint64(0)
        self._check(lib().erasor_hip_chain_timing(self._h, C.byref(a), C.byref(b), C.byref(p), C.byref(n), C.c_int(1 if reset else 0)))
        return a.value, b.value, n.value, p.value

    def stream(self):
        return lib().erasor_hip_stream(self._h)

    def device_array(self, a):
        """a host array copied into a device buffer of the handle's device (erasor_hip_device_alloc / _upload); returns the
        device pointer.  Freed with device_free (or with the process)."""
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self._check(lib().erasor_hip_device_alloc(self._h, C.c_size_t(a.nbytes), C.byref(p)))
        self._check(lib().erasor_hip_device_upload(self._h, p, _p(a), C.c_size_t(a.nbytes)))
        return p.value

    def device_free(self, ptr):
        self._check(lib().erasor_hip_device_free(self._h, C.c_void_p(ptr)))
