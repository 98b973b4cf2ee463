/*
 * erasor_hip.h — C ABI of the MI355X-native ERASOR hot path (liberasor_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, POD
 * structs, no C++/torch types, never throws.  Every entry point names the
 * reference interface it replaces (paths relative to the reference checkout):
 *
 *   erasor.h   = include/erasor/erasor.h
 *   erasor.cpp = src/offline_map_updater/src/erasor.cpp
 *   OMU.cpp    = src/offline_map_updater/src/OfflineMapUpdater.cpp
 *   utils.cpp  = src/offline_map_updater/src/erasor_utils.cpp
 *
 * Point layout everywhere: rows of 4 floats {x, y, z, intensity}; intensity carries
 * the SemanticKITTI label as a *numeric* float (utils.cpp:64).  4x4 transforms are
 * 16 floats, row-major.
 *
 * Threading: one handle = one GPU + one HIP stream; a handle is not thread-safe,
 * distinct handles are independent (reference: single-threaded ros::spin()).
 */
#ifndef ERASOR_HIP_H
#define ERASOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define ERASOR_OK               0
#define ERASOR_E_INVALID       -1  /* bad argument (reference: std::invalid_argument, OMU.cpp:125,274,312) */
#define ERASOR_E_NO_DEVICE     -2  /* no usable HIP device / HIP runtime error */
#define ERASOR_E_CAPACITY      -3  /* caller buffer too small */
#define ERASOR_E_STATE         -4  /* call order (e.g. step before set_map) */
#define ERASOR_E_UNSUPPORTED   -5  /* e.g. version not in {2,3} (OMU.cpp:273-275) */
#define ERASOR_E_INTERNAL      -6

/* ---- bin status codes (erasor.h:12-18), reported as the reference's doubles */
#define ERASOR_ST_LITTLE_NUM      0.0   /* == NOT_ASSIGNED */
#define ERASOR_ST_MERGE_BINS      0.25
#define ERASOR_ST_MAP_IS_HIGHER   0.5
#define ERASOR_ST_BLOCKED         0.8
#define ERASOR_ST_CURR_IS_HIGHER  1.0

/* ---- parameters: the rosparam names of erasor.h:47-61 and OMU.cpp:66-83 --- */
typedef struct erasor_params {
    /* /erasor/... (erasor.h:47-61) */
    double  max_range;             /* max_r            default 10.0 (erasor.h:47) */
    int32_t num_rings;             /*                  default 20   */
    int32_t num_sectors;           /*                  default 60   */
    double  max_h;                 /*                  default 3.0  */
    double  min_h;                 /*                  default 0.0  */
    double  th_bin_max_h;          /* v2 only          default 0.39 */
    double  scan_ratio_threshold;  /*                  default 0.22 */
    int32_t num_lowest_pts;        /*                  default 5    */
    int32_t minimum_num_pts;       /*                  default 4    */
    double  rejection_ratio;       /* unused upstream  default 0.33 */
    double  gf_dist_thr;           /* th_dist_         default 0.05 */
    int32_t gf_iter;               /*                  default 3    */
    int32_t gf_num_lpr;            /*                  default 10   */
    double  gf_th_seeds_height;    /*                  default 0.5  */
    double  map_voxel_size;        /* /erasor/map_voxel_size, v3 per-bin voxelise, default 0.2 */
    int32_t version;               /* /erasor/version  2 or 3, default 3 (OMU.cpp:81) */
    /* /MapUpdater/... (OMU.cpp:66-73) */
    double  query_voxel_size;      /* default 0.05 */
    int32_t removal_interval;      /* default 2; gating is done by the caller-side shim (OMU.cpp:206-209) */
    /* VoI radius used by fetch_VoI: /erasor/max_range read a second time with a
     * different default (60.0, OMU.cpp:78).  <=0 means "same as max_range". */
    double  voi_max_range;
    /* /large_scale/... (OMU.cpp:75-76): map_arranged_ becomes a submap |dx|,|dy| < submap_size around the pose,
     * re-centred when the pose moves more than submap_size/2 (OMU.cpp:332-379); save = submap + complement */
    int32_t is_large_scale;        /* default false */
    int32_t reserved0_;
    double  submap_size;           /* default 200.0 */
    int32_t reserved_[3];
} erasor_params;

/* Per-step result: the sizes the reference prints (OMU.cpp:431-433,452-464) plus
 * the parity/edge counters this implementation defines. */
typedef struct erasor_step_result {
    uint64_t n_map_in;          /* |map_arranged_| before the step */
    uint64_t n_voi;             /* |map_voi_|                       (OMU.cpp:431) */
    uint64_t n_outskirts;       /* |map_outskirts_|                 */
    uint64_t n_query;           /* |query_voi_| after voxelise       (OMU.cpp:238-241) */
    uint64_t n_static_estimate; /* |map_static_estimate_|  incl. duplicated ground (erasor.cpp:616) */
    uint64_t n_complement;      /* |map_egocentric_complement_| */
    uint64_t n_map_rejected;    /* |map_rejected_| = the dynamic-point mask */
    uint64_t n_curr_rejected;   /* |query_rejected_| (v2 only)      */
    uint64_t n_ground;          /* |ground_viz|                      */
    uint64_t n_map_out;         /* |map_arranged_| after the step    */
    uint64_t n_static;          /* parse_dynamic_obj static count    (utils.cpp:57-78) */
    uint64_t n_dynamic;         /* parse_dynamic_obj dynamic count   */
    uint32_t n_reverted_bins;   /* bins where R-GPF ran (erasor.cpp:511-533 / 383-394) */
    uint32_t n_neg_sector;      /* y==-0.0f,x<0 hazard: reference throws (erasor.cpp:112), here clamped to sector 0 */
    uint32_t n_ambiguous;       /* points whose theta/sector_size is within 1e-11 of an integer (device atan2 vs libm) */
    uint32_t n_degenerate_plane;/* estimate_plane_ on an empty ground set (uninitialised in reference, erasor.cpp:184-186) */
    uint32_t n_voxel_overflow;  /* VoxelGrid dx*dy*dz > INT_MAX passthroughs */
    uint32_t n_sort_fallback;   /* introsort depth-limit (heapsort) fallbacks taken */
    uint32_t reserved_[6];
} erasor_step_result;

/* cloud selectors for erasor_hip_get_cloud */
#define ERASOR_CLOUD_QUERY_VOI        0  /* query_voi_ (body frame)            OMU.cpp:241      */
#define ERASOR_CLOUD_MAP_VOI          1  /* map_voi_ (egocentric)              OMU.cpp:435-437  */
#define ERASOR_CLOUD_STATIC_ESTIMATE  2  /* map_static_estimate_ (egocentric)  erasor.cpp:612-616 */
#define ERASOR_CLOUD_COMPLEMENT       3  /* map_egocentric_complement_         erasor.cpp:622   */
#define ERASOR_CLOUD_MAP_REJECTED     4  /* map_rejected_ in map frame         OMU.cpp:284,287  */
#define ERASOR_CLOUD_CURR_REJECTED    5  /* query_rejected_ in map frame       OMU.cpp:284,288  */
#define ERASOR_CLOUD_GROUND_VIZ       6  /* ERASOR::ground_viz (egocentric)    erasor.h:127     */
#define ERASOR_CLOUD_MAP              7  /* map_arranged_ (same as get_map)    OMU.cpp:290      */

typedef struct erasor_hip_handle erasor_hip_handle;

/* library identity; safe without a GPU */
const char *erasor_hip_version(void);

/* fills the reference's compiled-in defaults (erasor.h:47-61, OMU.cpp:66-83) */
int erasor_hip_params_default(erasor_params *p);

/* replaces: OfflineMapUpdater ctor + `new ERASOR(&nh)` (OMU.cpp:5-32, erasor.h:46-103) */
int  erasor_hip_create(const erasor_params *p, int device, erasor_hip_handle **out);
void erasor_hip_destroy(erasor_hip_handle *h);
const char *erasor_hip_last_error(const erasor_hip_handle *h);

/* replaces: load_global_map's `*map_arranged_ = *map_init_` (OMU.cpp:107-167).
 * The map becomes device-resident.  _device: xyzi is a device pointer (same GPU). */
int erasor_hip_set_map(erasor_hip_handle *h, const float *xyzi, size_t n);
int erasor_hip_set_map_device(erasor_hip_handle *h, const void *d_xyzi, size_t n);

/* Look-ahead for offline sequences (the reference receives all nodes of a bag anyway, OMU.cpp:203): announce the scan
 * of the NEXT callback_node.  Its voxelisation (OMU.cpp:238-241: voxelize_preserving_labels, lidar->body) and R-POD
 * binning (erasor.cpp:100-115) do not depend on the map, so they run on their own stream beside the map-side stages
 * of the step in flight.  Results are unchanged; only the throughput of a scan sequence rises.
 *   erasor_hip_prefetch_scan(h, scan[0]);  erasor_hip_prefetch_scan(h, scan[1]);
 *   for k: erasor_hip_prefetch_scan(h, scan[k+2]);  erasor_hip_step*(h, scan[k], ...);      (or one ahead: k+1)
 * The following step must pass the same pointer, size and T_lidar2body (otherwise every announcement is dropped;
 * their chains have run out when that step returns).  A host
 * scan is copied at once (the buffer is the caller's again when the announcement returns).  The step that follows recognises its
 * scan by pointer, size, T_lidar2body AND a hash of EVERY record of the buffer it is handed against the hash of the copy that was
 * staged (round 4; rounds 2-3 sampled ~258 records, so a buffer refilled in place could be mistaken for the announced scan): a buffer
 * that has changed in any record is a different scan -- the announcements are dropped and the step runs on what it was given.  That
 * second pass over the caller's buffer costs ~0.1 ms of host time per 2 MB scan; a caller that knows which announcement its step
 * belongs to should say so instead -- erasor_hip_prefetch_node_rows returns a TICKET, erasor_hip_step_ticket takes it, nothing is
 * compared and the buffer is not read again.  A device scan (src_is_device != 0) is read in place and must stay valid until the step that
 * consumes it has returned.  Up to four scans can be outstanding between two steps (four query sides: a step can have its own scan
 * and three more announced ahead of it); the chains of consecutive scans alternate between two streams.  When every side is taken, a new announcement re-uses the side of the last
 * finished step: its query-derived outputs (erasor_hip_get_cloud / _get_bins) are gone from then on. */
int erasor_hip_prefetch_scan(erasor_hip_handle *h, const void *scan_xyzi, size_t n, int src_is_device,
                             const float T_lidar2body[16]);
/* The same for a whole node (msg/node.msg:1-7 carries the scan AND its pose): with T_body2origin known ahead, the step in
 * flight also launches the next callback's VoI membership pass (fetch_VoI, OMU.cpp:246-254, 391-395) behind its own last
 * kernel, so that the pass runs while the host collects the results.  The step that follows must pass the same pose; any
 * other pose (or a map store touched in between) simply runs its own pass.  Results are unchanged. */
int erasor_hip_prefetch_node(erasor_hip_handle *h, const void *scan_xyzi, size_t n, int src_is_device,
                             const float T_lidar2body[16], const float T_body2origin[16]);

/* replaces: the body of callback_node between OMU.cpp:237 and OMU.cpp:294:
 *   voxelize_preserving_labels(query) + transformPointCloud(tf_lidar2body_)   (OMU.cpp:238-241)
 *   fetch_VoI                                                                  (OMU.cpp:254, 381-438)
 *   ERASOR::set_inputs                                                         (OMU.cpp:266, erasor.cpp:57-85)
 *   compare_vois_and_revert_ground[_w_block]                                   (OMU.cpp:268/271)
 *   get_static_estimate / get_outliers / body2origin / map re-assembly         (OMU.cpp:272-290)
 *   parse_dynamic_obj counters                                                 (OMU.cpp:294)
 * T_origin2body is tf_body2origin_.inverse() (OMU.cpp:436), computed once by the
 * caller so host and device use the same 16 floats. */
int erasor_hip_step(erasor_hip_handle *h, const float *scan_xyzi, size_t n_scan,
                    const float T_lidar2body[16], const float T_body2origin[16],
                    const float T_origin2body[16], erasor_step_result *res);
int erasor_hip_step_device(erasor_hip_handle *h, const void *d_scan_xyzi, size_t n_scan,
                           const float T_lidar2body[16], const float T_body2origin[16],
                           const float T_origin2body[16], erasor_step_result *res);

/* The same step in two halves (threading row).  erasor_hip_step_async enqueues everything a step enqueues -- this
 * scan's query chain unless it was announced, the map chain, Scan Ratio Test .. write-back, the next announced scan's chain --
 * and returns without waiting; erasor_hip_step_wait blocks until the results are on the host, commits them and fills *res
 * exactly like erasor_hip_step.  erasor_hip_step_done polls (1: the wait would not block).  One host thread can so keep several
 * handles busy: independent sequences are independent updaters (one callback per node per updater, OMU.cpp:203), and one step
 * leaves most of the chip idle.  Between the two calls the handle accepts NO other call (ERASOR_E_STATE): announce the scans
 * ahead BEFORE erasor_hip_step_async.  A host scan buffer must stay valid until erasor_hip_step_wait has returned (a VoxelGrid
 * pass-through flip re-runs the step there). */
int erasor_hip_step_async(erasor_hip_handle *h, const void *scan_xyzi, size_t n_scan, int src_is_device,
                          const float T_lidar2body[16], const float T_body2origin[16], const float T_origin2body[16]);
int erasor_hip_step_wait(erasor_hip_handle *h, erasor_step_result *res);
int erasor_hip_step_done(erasor_hip_handle *h);

/* replaces: the node loop of the offline driver (main_in_your_env.cpp:92-123): nodes [first, first + count) of a sequence of n_total,
 * every node announced `lookahead` (0..7) nodes ahead with its pose, stepped one after the other -- the very calls a host loop would
 * make (erasor_hip_prefetch_node, erasor_hip_step[_device]), minus the caller's own time between two steps.  *announced (in / out):
 * nodes [0, *announced) are announced already, so a sequence can be split over several calls.  T_body2origin / T_origin2body: n_total
 * row-major 4x4 matrices each; res: `count` result blocks (may be NULL). */
int erasor_hip_run_nodes(erasor_hip_handle *h, const void *const *scans, const size_t *n_pts, size_t n_total, int src_is_device,
                         const float T_lidar2body[16], const float *T_body2origin, const float *T_origin2body, size_t first, size_t count,
                         int lookahead, size_t *announced, erasor_step_result *res);

/* Device buffers for callers that keep scans (erasor_hip_step_device, erasor_hip_prefetch_* with src_is_device) or the map
 * (erasor_hip_set_map_device) resident in HBM but have no HIP of their own: hipMalloc / blocking hipMemcpy / hipFree on the
 * handle's device.  (A ROS node hands over host clouds, OMU.cpp:237; these are for offline drivers and benchmarks.) */
int erasor_hip_device_alloc(erasor_hip_handle *h, size_t bytes, void **d_ptr);
int erasor_hip_device_upload(erasor_hip_handle *h, void *d_dst, const void *src, size_t bytes);
int erasor_hip_device_free(erasor_hip_handle *h, void *d_ptr);

/* replaces: the ERASOR class used on its own (erasor.h:109-141): set_inputs(map_voi, query_voi) +
 * compare_vois_and_revert_ground[_w_block] on caller-provided EGOCENTRIC clouds (query already voxelised and
 * in the body frame).  Results: erasor_hip_get_cloud(STATIC_ESTIMATE / COMPLEMENT / MAP_REJECTED /
 * CURR_REJECTED / GROUND_VIZ), erasor_hip_get_status, erasor_hip_get_bins.  Replaces the handle's map. */
int erasor_hip_erasor_run(erasor_hip_handle *h, const float *map_voi_xyzi, size_t n_map,
                          const float *query_voi_xyzi, size_t n_query, erasor_step_result *res);

/* map_arranged_ read-back (OMU.cpp:183: what save_static_map starts from) */
int erasor_hip_map_size(erasor_hip_handle *h, size_t *n);
int erasor_hip_get_map(erasor_hip_handle *h, float *dst_xyzi, size_t cap_points, size_t *n);

/* replaces: ERASOR::get_static_estimate / get_outliers outputs and the public
 * members of erasor.h:127,139-141 — clouds of the *last* step. */
int erasor_hip_get_cloud(erasor_hip_handle *h, int which, float *dst_xyzi, size_t cap_points, size_t *n);

/* index of every map_rejected_ point in the map *before* the step (the dynamic-point mask
 * of BASELINE.json:north_star, as indices into the pre-step map_arranged_ order) */
int erasor_hip_get_rejected_indices(erasor_hip_handle *h, uint64_t *dst, size_t cap, size_t *n);

/* replaces: r_pod_map / r_pod_curr descriptors (erasor.h:143-144; Bin erasor.h:24-33).
 * which: 0 = map, 1 = curr.  Arrays of num_rings*num_sectors, index = ring*num_sectors + sector.
 * Empty bins report count 0, min_h = +1e13, max_h = -1e13 (erasor.h:3, erasor.cpp:45-46). */
int erasor_hip_get_bins(erasor_hip_handle *h, int which, uint32_t *count, double *min_h, double *max_h);

/* r_pod_selected[r][theta].status after the step (erasor.cpp:503-560), index = ring*num_sectors + sector */
int erasor_hip_get_status(erasor_hip_handle *h, double *status);

/* replaces: the public R-PODs themselves, `R_POD r_pod_map, r_pod_curr, r_pod_selected` (erasor.h:143-145): the
 * point list of every bin (Bin::points, erasor.h:32), egocentric.  which: 0 = map, 1 = curr, 2 = selected.
 * The points come theta-major (the order ERASOR::r_pod2pc walks the bins, erasor.cpp:309-320), each bin's points in
 * the reference's order; begin[i] / count[i] locate bin i = ring*num_sectors + sector inside xyzi. */
int erasor_hip_get_rpod(erasor_hip_handle *h, int which, float *xyzi, size_t cap_points, size_t *n,
                        uint32_t *begin, uint32_t *count);

/* R-GPF plane per reverted bin, in the (theta, ring) order the reference visits them
 * (erasor.cpp:493-494): for reverted bin k and iteration it < gf_iter:
 *   normal[(k*gf_iter+it)*3 .. +3], d[k*gf_iter+it]  (erasor.cpp:183-198);
 * bin_index[k] = ring*num_sectors + sector. */
int erasor_hip_get_planes(erasor_hip_handle *h, uint32_t *bin_index, float *normal, double *d,
                          size_t cap_bins, size_t *n_bins);

/* replaces: erasor_utils::voxelize_preserving_labels (utils.cpp:80-114), standalone */
int erasor_hip_voxelize_preserving_labels(erasor_hip_handle *h, const float *src_xyzi, size_t n,
                                          double leaf_size, float *dst_xyzi, size_t cap_points,
                                          size_t *n_out);

/* ---- PR / RR of a cleaned map: the step AFTER the hot path (scripts/analysis_runner.py) ---------------------------------------
 * replaces: analysis_runner.py:74-105 (evaluate), restated on the host in erasor_amd/evalmap.py.  For every ground-truth point the
 * nearest estimated point (1-NN); the point is kept if that distance is < voxelsize*sqrt(3)/2.  Labels: uint32(intensity) & 0xFFFF,
 * dynamic classes 252..259.  PR = preserved_static / gt_static, RR = 1 - preserved_dynamic / gt_dynamic (both in percent), F1 of
 * PR/100 and RR/100 -- evalmap.evaluate's formulas; gt_static == 0 gives PR 0 and gt_dynamic == 0 gives RR 0. */
typedef struct erasor_eval_result {
    uint64_t gt_static, gt_dynamic, est_static, est_dynamic, preserved_static, preserved_dynamic;
    uint64_t n_tied;               /* kept ground-truth points whose nearest distance is shared by estimated points of both classes: which
                                    * one cKDTree returns is not defined (here: the smallest estimated index) */
    uint64_t n_label_out_of_range; /* intensities (both clouds) that are not finite or outside [0, 2^32): counted as static */
    double PR, RR, F1;             /* percent, percent, fraction */
} erasor_eval_result;

/* per-ground-truth-point codes of erasor_hip_evaluate_clouds */
#define ERASOR_EVAL_OUT            0  /* no estimated point within the threshold */
#define ERASOR_EVAL_KEPT_STATIC    1
#define ERASOR_EVAL_KEPT_DYNAMIC   2
#define ERASOR_EVAL_CLASS_DIFFERS  3  /* within the threshold, but the nearest point's class is the other one */

/* replaces: analysis_runner.py:74-105 on two caller clouds (XYZI rows), each on the host or on the handle's device (_is_device).
 * voxel_leaf > 0: both are first voxelised with voxelize_preserving_labels at that leaf on the device (the save_static_map protocol,
 * OMU.cpp:174-196); that borrows the query side of the last step like erasor_hip_voxelize_preserving_labels does: nodes announced
 * ahead are dropped (their steps run their own chains, results unchanged; a dropped ticket is ERASOR_E_STATE) and erasor_hip_get_cloud
 * answers ERASOR_E_STATE until the next step.  voxel_leaf == 0: evaluated as given, in scratch of the evaluator's own -- announcements and
 * the last step's clouds stay as they are.  per_gt (optional, n_gt bytes, ERASOR_EVAL_*) only with voxel_leaf == 0.
 * ERASOR_E_INVALID: a non-finite coordinate, voxelsize <= 0, per_gt with voxel_leaf > 0.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_evaluate_clouds(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                               const void *est_xyzi, size_t n_est, int est_is_device,
                               double voxel_leaf, double voxelsize, uint8_t *per_gt, erasor_eval_result *res);
/* the same with the handle's current map as the estimate -- the erasor_hip_get_map view (large-scale mode: the submap followed by its
 * complement), compacted on the device, never copied to the host.  ERASOR_E_STATE: no map, or a step in flight. */
int erasor_hip_evaluate_map(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                            double voxel_leaf, double voxelsize, erasor_eval_result *res);

/* K estimates against ONE ground truth (compare_map.cpp's use: raw / OctoMap / Peopleremover / Removert / ERASOR maps against one GT):
 * rows[j] is what erasor_hip_evaluate_clouds(h, gt, est[j], voxel_leaf, voxelsize) returns, field for field (the same decision per
 * GT point: its nearest point of estimate j by (float64 d^2, index within estimate j), kept if sqrt(d^2) < voxelsize*sqrt(3)/2), from one
 * index of all estimates and one query launch.  est_xyzi / n_est / est_is_device: k entries (est_is_device may be NULL: all on the host).
 * voxel_leaf > 0: the GT is voxelised once and every estimate once, with what that borrows (see erasor_hip_evaluate_clouds); 0 works in
 * the evaluator's own scratch.  Device memory: below 56 B per estimated point + 8 KiB per estimate, plus a host GT's copy.
 * ERASOR_E_INVALID: those of erasor_hip_evaluate_clouds (a non-finite point in estimate j names j in erasor_hip_last_error), more than
 * 2^31 estimated points in all.  k == 0: ERASOR_OK, no rows.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_evaluate_many(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                             const void *const *est_xyzi, const size_t *n_est, const int *est_is_device, size_t k,
                             double voxel_leaf, double voxelsize, erasor_eval_result *rows);

/* ---- a parameter sweep: ERASOR configurations over one sequence, each scored by PR / RR ----------------------------------------
 * Per configuration, what OfflineMapUpdater + save_static_map + the saved map's evaluation do (the offline driver's --config <yaml> n
 * <gt>): node j (0-based) is stepped iff (j + 1) % removal_interval == 0 (OMU.cpp:206-209), the map after the last node is voxelised by
 * voxelize_preserving_labels at save_leaf (main_in_your_env.cpp:123; 0: not voxelised) and evaluated against gt as given (no
 * voxelisation of the GT).  The map, the scans and the GT are uploaded to h's device once (device inputs are read in place).  The
 * configurations run in waves of `concurrency` (1..4) worker handles on h's device, one host thread each, every worker with ONE query
 * stream; the saved maps are then scored by erasor_hip_evaluate_many's kernels in groups of eval_batch (0: all at once).  Free device
 * memory is checked before each wave.  A configuration that fails -- its parameters (version 4: ERASOR_E_UNSUPPORTED), memory, a step --
 * carries that status in its row; the call still returns ERASOR_OK.  Only h's evaluator scratch is used: h's map, announcements and later
 * steps stay as they were.  Scans / offsets / poses as erasor_hip_align_frames_clouds and erasor_hip_run_nodes take them: the scans back
 * to back, offsets (n_nodes + 1, host), T_body2origin / T_origin2body n_nodes row-major 4x4 matrices each.
 * ERASOR_E_INVALID: more than 256 configurations, bad offsets, non-finite poses / map / GT points, voxelsize <= 0, save_leaf < 0,
 * concurrency outside 1..4.  ERASOR_E_STATE: a step of h in flight. */
typedef struct erasor_sweep_row {
    erasor_params params;      /* the configuration as run */
    int32_t status;            /* ERASOR_OK, or this configuration's own error */
    uint32_t n_steps;          /* nodes stepped after the removal_interval gate */
    uint64_t n_map_final;      /* erasor_hip_map_size after the last node */
    uint64_t n_saved;          /* points of the saved map */
    erasor_eval_result eval;   /* the saved map against gt */
    double run_ms;             /* host wall time of this configuration's node loop */
    uint32_t reserved_[8];
} erasor_sweep_row;

int erasor_hip_sweep(erasor_hip_handle *h, const erasor_params *configs, size_t n_configs,
                     const void *map_xyzi, size_t n_map, int map_is_device,
                     const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_nodes, int scans_are_device,
                     const float T_lidar2body[16], const float *T_body2origin, const float *T_origin2body,
                     const void *gt_xyzi, size_t n_gt, int gt_is_device,
                     double save_leaf, double voxelsize, int concurrency, int eval_batch, erasor_sweep_row *rows);

/* ---- PR / RR broken down by semantic class and by dynamic instance --------------------------------------------------------------
 * The decision of erasor_hip_evaluate_* for every ground-truth point (its nearest estimated point, the threshold, the smallest
 * estimated index on a tie), counted per class key and per dynamic instance.  Class key: uint32(intensity) & 0xFFFF, or
 * ERASOR_EVAL_KEY_LABEL_OUT_OF_RANGE for an intensity that is not finite or outside [0, 2^32) (static, as in erasor_eval_result).
 * Class rows: every key present in either cloud, in ascending order.  Instance rows: every whole label L = uint32(intensity) with a
 * dynamic class (252..259) present in either cloud, in ascending order (n_gt may be 0: an estimate-only label).
 * Summing the class rows gives gt_static / gt_dynamic, est_static / est_dynamic, preserved_static (static keys), preserved_dynamic
 * (dynamic keys) and n_tied of erasor_eval_result; summing the instance rows of one dynamic class gives that class's row. */
#define ERASOR_EVAL_KEY_LABEL_OUT_OF_RANGE 0x10000u
typedef struct erasor_eval_class_row {
    uint32_t key;         /* class: sem or ERASOR_EVAL_KEY_LABEL_OUT_OF_RANGE; instance: the whole uint32 label */
    uint32_t is_dynamic;
    uint64_t n_gt;        /* ground-truth points with this key */
    uint64_t n_within;    /* ... whose nearest estimated point is within the threshold */
    uint64_t n_preserved; /* ... counted in preserved_static / preserved_dynamic */
    uint64_t n_tied;      /* ... counted in n_tied */
    uint64_t n_est;       /* estimated points with this key */
} erasor_eval_class_row;

/* erasor_hip_evaluate_clouds / _map (arguments, errors, voxel_leaf and the map view as there; no per-point codes) with the rows.  res is
 * what erasor_hip_evaluate_* returns on the same inputs.  *n_classes / *n_instances (required) and res are always written; the rows
 * only when both fit their capacity, else ERASOR_E_CAPACITY: size the arrays and call again.  A NULL array with capacity 0 is allowed
 * (a class array of 65537 rows always fits). */
int erasor_hip_evaluate_clouds_by_class(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                                        const void *est_xyzi, size_t n_est, int est_is_device, double voxel_leaf, double voxelsize,
                                        erasor_eval_class_row *classes, size_t cap_classes, size_t *n_classes,
                                        erasor_eval_class_row *instances, size_t cap_instances, size_t *n_instances,
                                        erasor_eval_result *res);
int erasor_hip_evaluate_map_by_class(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                                     double voxel_leaf, double voxelsize,
                                     erasor_eval_class_row *classes, size_t cap_classes, size_t *n_classes,
                                     erasor_eval_class_row *instances, size_t cap_instances, size_t *n_instances,
                                     erasor_eval_result *res);

/* ---- bird's-eye images: looking at a map and at PR / RR's per-point decisions (kernels: render.hip.h) ---------------------------
 * replaces: what the reference shows in RViz -- src/utils/viz_kitti_map.cpp:27-82,118-125 (one map as static / dynamic / one chosen
 * class or instance) and src/utils/compare_map.cpp:65-96 (ground truth and several methods' maps, static and dynamic, side by side) --
 * as an image file, plus the error map: the ground truth coloured by erasor_hip_evaluate_clouds' decision per point.
 * A top-down orthographic raster of XYZI rows.  Pixel of a point, in float64 from its float32 coordinates, every operation on its own:
 * cx = floor((x - x0) / res), cy = floor((y - y0) / res); drawn iff 0 <= cx < width and 0 <= cy < height (compared as doubles);
 * column cx, image row height - 1 - cy (north up).  A point with a non-finite x, y or z is dropped and counted (n_nonfinite), a finite
 * one off the image is counted (n_outside); neither is an error.  The winner of a pixel is the point with the largest (priority of its
 * category, z), z compared in float32's total order (-0.0 < +0.0); the colour is a function of (category, z): the category's palette
 * entry shaded by s = z_hi > z_lo ? clamp((z - z_lo) / (z_hi - z_lo), 0, 1) : 1, channel = (uint8)floor(base * (0.35 + 0.65 * s) + 0.5)
 * in float64.  So the image depends on the point set, not on its order, and equals erasor_amd/evalmap.py's render byte for byte.
 * Pixels no point hit take `background`.  Output: height x width x 3 bytes, RGB, row-major. */
#define ERASOR_RENDER_LABEL   0  /* static / dynamic / target by label (parse_dynamic_obj, utils.cpp:57-78; viz_kitti_map.cpp:51-82) */
#define ERASOR_RENDER_HEIGHT  1  /* one category: maps with intensity = 0 */
#define ERASOR_RENDER_EVAL    2  /* erasor_hip_render_eval_* only: the evaluator's decision per ground-truth point */
#define ERASOR_RENDER_NCAT    8
#define ERASOR_RENDER_CAT_STATIC           0  /* LABEL, priority 1 */
#define ERASOR_RENDER_CAT_DYNAMIC          1  /* LABEL, priority 2: class 252..259 */
#define ERASOR_RENDER_CAT_TARGET           2  /* LABEL, priority 3: a dynamic point of target_class (and target_instance) */
#define ERASOR_RENDER_CAT_HEIGHT           3  /* HEIGHT, priority 1 */
#define ERASOR_RENDER_CAT_STATIC_KEPT      4  /* EVAL, priority 1: ERASOR_EVAL_KEPT_STATIC */
#define ERASOR_RENDER_CAT_DYNAMIC_REMOVED  5  /* EVAL, priority 2: GT dynamic and not ERASOR_EVAL_KEPT_DYNAMIC */
#define ERASOR_RENDER_CAT_STATIC_LOST      6  /* EVAL, priority 3: GT static and not ERASOR_EVAL_KEPT_STATIC */
#define ERASOR_RENDER_CAT_DYNAMIC_LEFT     7  /* EVAL, priority 4: ERASOR_EVAL_KEPT_DYNAMIC -- errors on top, whatever their height */
/* base colour 0xRRGGBB and priority per category */
static const uint32_t ERASOR_RENDER_PALETTE[ERASOR_RENDER_NCAT] = {0xC8C8C8u, 0xFF5050u, 0xFFE000u, 0x80D0FFu,
                                                                   0xB4B4B4u, 0x30C040u, 0x3060FFu, 0xFF2020u};
static const uint8_t ERASOR_RENDER_PRIORITY[ERASOR_RENDER_NCAT] = {1, 2, 3, 1, 1, 2, 3, 4};

typedef struct erasor_render_view {
    double x0, y0, res;      /* world coordinates of the lower left corner, metres per pixel (finite, res > 0) */
    uint32_t width, height;  /* 1 .. 16384 each, width * height <= 2^26 */
    double z_lo, z_hi;       /* the shading's height range (finite) */
    uint32_t background;     /* 0xRRGGBB */
    uint32_t reserved_;
} erasor_render_view;

typedef struct erasor_render_stats {
    uint64_t n_points, n_drawn, n_outside, n_nonfinite, n_pixels_hit;
    uint64_t cat_points[ERASOR_RENDER_NCAT];  /* points drawn per category */
    uint64_t cat_pixels[ERASOR_RENDER_NCAT];  /* pixels won per category */
} erasor_render_stats;

/* A view that contains every finite point of a cloud (host or device), or of the handle's map (erasor_hip_render_fit_map), over the
 * finite points, in float64: x0 = floor(min_x / res) * res - margin * res, width = (uint32)floor((max_x - x0) / res) + 1 + margin (the
 * same in y); margin_px in 1 .. 1024 pixels, at least 1 so that a last-bit rounding of floor(min_x / res) * res cannot put the lowest point off the image.
 * z_lo / z_hi are order statistics, not interpolated: the values at ranks floor(0.02 * (n - 1)) and floor(0.98 * (n - 1)) of the
 * ascending finite z (an exact radix select on the device), so one outlier does not flatten the shading.
 * ERASOR_E_INVALID: res not finite or <= 0, margin_px outside 1 .. 1024, no finite point, or a size beyond the limits (erasor_hip_last_error then
 * names a res that fits).  ERASOR_E_STATE: a step in flight; _map: no map. */
int erasor_hip_render_fit(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, double res, uint32_t margin_px,
                          uint32_t background, erasor_render_view *view);
int erasor_hip_render_fit_map(erasor_hip_handle *h, double res, uint32_t margin_px, uint32_t background, erasor_render_view *view);

/* One cloud (host or device) as an image, mode ERASOR_RENDER_LABEL or _HEIGHT.  target_class < 0: no target; target_instance < 0: every
 * instance of target_class (fetch_specific_class / fetch_specific_object, viz_kitti_map.cpp:51-82: among the dynamic points).  rgb:
 * height * width * 3 bytes on the host, or on the handle's device (rgb_is_device); may be NULL (statistics only).  Works in scratch of
 * the renderer's own: announcements and the last step's clouds stay as they are.  An empty cloud gives the background.
 * ERASOR_E_INVALID: a view outside the limits above, a mode other than those two, more than 2^30 points.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_render_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, int mode, int32_t target_class,
                             int32_t target_instance, const erasor_render_view *view, void *rgb, int rgb_is_device,
                             erasor_render_stats *stats);
/* the same of the handle's current map: the erasor_hip_get_map view (large-scale mode: the submap followed by its complement),
 * compacted on the device, never copied to the host.  ERASOR_E_STATE also: no map. */
int erasor_hip_render_map(erasor_hip_handle *h, int mode, int32_t target_class, int32_t target_instance, const erasor_render_view *view,
                          void *rgb, int rgb_is_device, erasor_render_stats *stats);

/* The error map: erasor_hip_evaluate_clouds / _map (arguments, errors and voxel_leaf as there; res as there) and the ground truth drawn
 * in mode ERASOR_RENDER_EVAL, each point by what the evaluation decided for it; the per-point codes stay on the device in between.
 * voxel_leaf > 0: the voxelised ground truth is what is drawn.  When the view contains every ground-truth point, cat_points of the
 * four EVAL categories equal preserved_static, gt_dynamic - preserved_dynamic, gt_static - preserved_static and preserved_dynamic. */
int erasor_hip_render_eval_clouds(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, const void *est_xyzi, size_t n_est,
                                  int est_is_device, double voxel_leaf, double voxelsize, const erasor_render_view *view, void *rgb,
                                  int rgb_is_device, erasor_render_stats *stats, erasor_eval_result *res);
int erasor_hip_render_eval_map(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device, double voxel_leaf, double voxelsize,
                               const erasor_render_view *view, void *rgb, int rgb_is_device, erasor_render_stats *stats,
                               erasor_eval_result *res);

/* ---- the estimate-to-ground-truth overlap report: the alignment check before PR / RR (scripts/analysis_runner.py) -------------
 * replaces: analysis_runner.py:53-71 (overlap_report).  For every estimated point the distance d to its nearest ground-truth point
 * (exact and unbounded: float64 d^2 as cKDTree / NearestNeighbors compute it, the correctly rounded sqrt), then np.median, np.percentile
 * (90, 99; method "linear") and the max of those distances, and np.mean(d < x) * 100 for x = 0.5 * voxelsize, voxelsize, 2 * voxelsize --
 * each formed with numpy's operations, so the values are the reference's bit for bit.  n_est == 0: counts 0, statistics NaN. */
typedef struct erasor_overlap_result {
    uint64_t n_est;                                   /* distances measured (after voxel_leaf) */
    uint64_t n_below_half, n_below_one, n_below_two;  /* d < 0.5*v, < v, < 2*v */
    double median, p90, p99, max;                     /* metres */
    double frac_half, frac_one, frac_two;             /* percent, np.mean(d < x) * 100 */
} erasor_overlap_result;

/* replaces: analysis_runner.py:53-71 on two caller clouds (XYZI rows; the intensity is not read), each on the host or on the handle's
 * device (_is_device).  voxel_leaf as for erasor_hip_evaluate_clouds: > 0 voxelises both clouds first and drops nodes announced ahead;
 * 0 works in the evaluator's own scratch and leaves announcements and the last step's clouds as they are.  per_est_dist / per_est_nearest
 * (optional, host, n_est entries each): d of every estimated point, and the index of its nearest ground-truth point (the smallest index
 * among points at the same d^2); only with voxel_leaf == 0.
 * ERASOR_E_INVALID: a non-finite coordinate, voxelsize <= 0, a per-point output with voxel_leaf > 0, more than 2^30 points, or an empty
 * ground truth with a non-empty estimate.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_overlap_clouds(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                              const void *est_xyzi, size_t n_est, int est_is_device, double voxel_leaf, double voxelsize,
                              double *per_est_dist, uint32_t *per_est_nearest, erasor_overlap_result *res);
/* the same with the handle's current map as the estimate (the erasor_hip_get_map view, compacted on the device, never copied to the
 * host).  ERASOR_E_STATE: no map, or a step in flight. */
int erasor_hip_overlap_map(erasor_hip_handle *h, const void *gt_xyzi, size_t n_gt, int gt_is_device,
                           double voxel_leaf, double voxelsize, erasor_overlap_result *res);

/* ---- every frame's pose against the map, before a run (the reference README's pitfalls 1, 3 and 5) ----------------------------
 * replaces: transforming each scan on the host and running overlap_report (analysis_runner.py:53-71) on it, frame by frame.  Frame f is
 * the scans' points [offsets[f], offsets[f + 1]) as given (no voxelisation, no range filter), put into the map frame as the reference
 * puts its RViz query (OfflineMapUpdater.cpp:238-242): T_lidar2body, then T_body2origin[f], each in float32 with pcl::transformPointCloud's
 * association ((a*x + b*y) + c*z) + d.  Points with a non-finite coordinate after the two transforms are dropped and counted; the row
 * is the overlap report of the others against the map, bit for bit.  An empty frame, or one whose points were all dropped: n_est = 0,
 * statistics NaN.  summary (optional): the overlap report of every frame's kept points together. */
typedef struct erasor_align_row {
    uint64_t n_points;        /* points of the frame as given */
    uint64_t n_non_finite;    /* excluded: a non-finite coordinate after the two transforms */
    erasor_overlap_result r;  /* overlap_report of the remaining points against the map (r.n_est = n_points - n_non_finite) */
} erasor_align_row;

/* The map (XYZI rows; the intensity is not read) and the concatenated scans, each on the host or on the handle's device (_is_device);
 * offsets: host, n_frames + 1 entries, offsets[0] = 0 and offsets[n_frames] = n_scan_points; T_lidar2body: NULL for the identity (still
 * applied as a transform); T_body2origin: host, n_frames row-major 4x4 matrices (the step's layout); rows: n_frames entries.  Works in
 * the evaluator's own scratch: announced nodes, tickets and the last step's clouds stay as they are.
 * ERASOR_E_INVALID: a non-finite pose entry or map point; offsets[0] != 0, decreasing offsets or a last offset other than n_scan_points;
 * voxelsize <= 0; more than 2^30 scan or map points; more than 65536 frames; an empty map with a non-empty frame.
 * ERASOR_E_STATE: a step in flight. */
int erasor_hip_align_frames_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device,
                                   const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                   int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, double voxelsize,
                                   erasor_align_row *rows, erasor_overlap_result *summary);
/* the same against the handle's current map (the erasor_hip_get_map view, compacted on the device as erasor_hip_overlap_map does, never
 * copied to the host).  ERASOR_E_STATE also: no map. */
int erasor_hip_align_frames_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, double voxelsize,
                                erasor_align_row *rows, erasor_overlap_result *summary);

/* ---- every frame's pose refined against the map: point-to-point ICP, all frames side by side -----------------------------------
 * replaces: "fix the poses in your SLAM and come back" -- the reference README's first pitfall (pose_i · pcds/00000<i>.pcd must
 * overlay on dense_global_map.pcd) names the fault, erasor_hip_align_frames_* finds the frames, and this moves them.  Frame f is the
 * scans' points [offsets[f], offsets[f + 1]) put into the map frame as the reference puts a scan there (OfflineMapUpdater.cpp:238-242,
 * 441-449): p = T_lidar2body · row in float32 (NULL: the identity, still applied), then q = R·p + t with the frame's pose in float64,
 * which starts as the float32 T_body2origin[f] widened.  Per iteration: every q's exact nearest map point (ties to the lowest index),
 * the pairs with d^2 <= max_dist * max_dist, Horn's closed-form rigid update from their sums, until the update's translation is
 * <= eps_t and its rotation angle (2 |q_xyz| of the unit quaternion) <= eps_r, or max_iters updates.  Every sum is taken in one
 * defined order, so the result is the host restatement's (evalmap.refine_poses) bit for bit.  No re-orthonormalisation:
 * max_iters <= 64 keeps R's drift at rounding level. */
typedef struct erasor_refine_params {
    double max_dist;     /* the correspondence gate, > 0 */
    double eps_t;        /* stop: |translation update| <= eps_t ... */
    double eps_r;        /* ... and rotation update <= eps_r (radians) */
    uint32_t max_iters;  /* 1 .. 64 */
    uint32_t min_pairs;  /* a frame with fewer pairs keeps the pose it has and ends (0 counts as 1) */
} erasor_refine_params;

#define ERASOR_REFINE_CONVERGED  0  /* the last update was below eps_t and eps_r */
#define ERASOR_REFINE_MAX_ITERS  1  /* max_iters updates made */
#define ERASOR_REFINE_FEW_PAIRS  2  /* fewer than min_pairs pairs: the pose of the iteration before (first iteration: the input, bit for bit) */
#define ERASOR_REFINE_NO_POINTS  3  /* no point with finite coordinates under the input pose (an empty frame too) */

typedef struct erasor_refine_row {
    double T[16];            /* the refined T_body2origin, row-major: R, t, and 0 0 0 1 */
    uint32_t status;         /* ERASOR_REFINE_* */
    uint32_t iters;          /* updates applied */
    uint64_t n_points;       /* points of the frame as given */
    uint64_t n_non_finite;   /* without a query under the input pose: a non-finite coordinate after T_lidar2body or after the pose */
    uint64_t n_pairs_first;  /* pairs within the gate under the input pose ... */
    uint64_t n_pairs_last;   /* ... and under T */
    double rms_first;        /* sqrt(sum of the pairs' d^2 / pairs) under the input pose; NaN without a pair ... */
    double rms_last;         /* ... and under T */
    double moved_t;          /* |t - t_input| */
    double moved_r;          /* the angle of R · R_inputᵀ from its trace: acos of (trace - 1) / 2 clamped to [-1, 1] */
} erasor_refine_row;

typedef struct erasor_refine_summary {
    uint64_t n_frames;
    uint64_t n_status[4];    /* frames by ERASOR_REFINE_* */
    uint64_t n_pairs_first;  /* the rows' totals, added in frame order */
    uint64_t n_pairs_last;
    double sum_d2_first;
    double sum_d2_last;
} erasor_refine_summary;

/* Map, scans, offsets, T_lidar2body and T_body2origin as erasor_hip_align_frames_clouds takes them, except that a non-finite entry of
 * T_body2origin is not refused: that frame's points have no query and it ends with ERASOR_REFINE_NO_POINTS.  rows: n_frames entries or
 * NULL; summary: optional.  Works in the evaluator's own scratch, like erasor_hip_align_frames_clouds; the map's tree is built once.
 * ERASOR_E_INVALID: params NULL, max_iters outside 1 .. 64, max_dist / eps_t / eps_r not a finite number > 0, the offsets' and sizes'
 * errors of erasor_hip_align_frames_clouds, a non-finite map point or T_lidar2body entry, an empty map with a non-empty frame.
 * ERASOR_E_STATE: a step in flight. */
int erasor_hip_refine_poses_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device,
                                   const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                   int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                                   const erasor_refine_params *params, erasor_refine_row *rows, erasor_refine_summary *summary);
/* the same against the handle's current map (compacted on the device as erasor_hip_align_frames_map does, never copied to the host).
 * ERASOR_E_STATE also: no map. */
int erasor_hip_refine_poses_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                                const erasor_refine_params *params, erasor_refine_row *rows, erasor_refine_summary *summary);

/* ---- every frame's pose refined point-to-plane against the map's own normals, all frames side by side --------------------------
 * erasor_hip_refine_poses_* with the residual taken along the map's surface normal: a scan never samples the map's own points, so
 * point-to-point stops a fraction of the sampling step off and creeps along surfaces; point-to-plane lets a frame slide along a
 * surface and converges in a few iterations.  Once per call the map's normals and curvature are computed on the device as
 * erasor_hip_normals_* computes them (k = normals_k, no viewpoint; the orientation cannot matter, every summed product holds two
 * factors of the normal) and stay there.  Per iteration, frames and points as for erasor_hip_refine_poses_*: q' = R·p, q = q' + t,
 * q's exact nearest map point j (ties to the lowest index); a CANDIDATE has d^2 <= max_dist * max_dist; a PAIR is a candidate whose
 * normal n_j is finite and whose curvature is <= max_curvature; any other candidate is counted as unusable.  A pair's residual is
 * r = n·(q - m_j) and its row J = (q' x n, n); the frame's 29 sums (J[a]J[b] for a <= b, J[a]r, r^2, d^2) are taken in the defined
 * order of erasor_hip_refine_poses_*.  The host then solves the 6x6 normal equations (A = sum J^T J, b = -sum J^T r) by cyclic Jacobi
 * (the rotation of the 4x4 solve, pivots row-major, 32 sweeps at most) and applies the pseudo-inverse over the eigen-directions with
 * lambda_i > rank_tol * lambda_max: x = sum over the kept i of v_i (v_i·b) / lambda_i; the rotation is the unit quaternion of the half
 * vector h = x[0..2] / 2, w = 1 / sqrt(1 + |h|^2), (x, y, z) = h w; R <- D·R, t <- t + x[3..5].  rank is the number of kept
 * directions: a frame that sees one plane has rank 3, two perpendicular planes 5, and only a rank of 6 constrains the whole pose --
 * the directions left out are not moved.  The eigenvalues mix radians and metres, so rank_tol is a parameter and lambda_ratio
 * (lambda_min / lambda_max) is reported; a null direction held only by noise in the normals passes rank_tol and shows in
 * lambda_ratio alone.  Stopping, min_pairs (applied to the pairs), frozen frames and the final evaluation are
 * erasor_hip_refine_poses_*'s.  The result is the host restatement's (evalmap.refine_poses_plane) bit for bit. */
typedef struct erasor_refine_plane_params {
    double max_dist;       /* the correspondence gate, > 0 */
    double eps_t;          /* stop: |translation update| <= eps_t ... */
    double eps_r;          /* ... and rotation update <= eps_r (radians) */
    uint32_t max_iters;    /* 1 .. 64 */
    uint32_t min_pairs;    /* a frame with fewer pairs keeps the pose it has and ends (0 counts as 1) */
    uint32_t normals_k;    /* the neighbourhood of the map's normals, 2 .. 32 */
    double max_curvature;  /* a map point with a larger curvature gives no pair; finite, > 0 (curvature is <= 1/3: 1.0 gates nothing) */
    double rank_tol;       /* a direction counts when lambda_i > rank_tol * lambda_max; finite, within [0, 1) */
} erasor_refine_plane_params;

#define ERASOR_REFINE_DEGENERATE 4  /* a solve with no direction above rank_tol (lambda_max is not > 0): the pose is kept */

typedef struct erasor_refine_plane_row {
    double T[16];            /* as erasor_refine_row, field for field, down to moved_r */
    uint32_t status;         /* ERASOR_REFINE_*, ERASOR_REFINE_DEGENERATE included */
    uint32_t iters;
    uint64_t n_points;
    uint64_t n_non_finite;
    uint64_t n_pairs_first;
    uint64_t n_pairs_last;
    double rms_first;        /* the pairs' point distances, as in erasor_refine_row */
    double rms_last;
    double moved_t;
    double moved_r;
    uint32_t rank;             /* directions kept by the last solve made; 0 when none was made */
    double lambda_ratio;       /* lambda_min / lambda_max of that solve; NaN when lambda_max is not > 0 or no solve was made */
    uint64_t n_unusable_first; /* candidates without a usable normal under the input pose ... */
    uint64_t n_unusable_last;  /* ... and under T */
    double rms_plane_first;    /* sqrt(sum of the pairs' r^2 / pairs) under the input pose; NaN without a pair ... */
    double rms_plane_last;     /* ... and under T */
} erasor_refine_plane_row;

typedef struct erasor_refine_plane_summary {
    uint64_t n_frames;
    uint64_t n_status[5];    /* frames by ERASOR_REFINE_* */
    uint64_t n_pairs_first;  /* the rows' totals, added in frame order */
    uint64_t n_pairs_last;
    double sum_d2_first;
    double sum_d2_last;
    double sum_r2_first;
    double sum_r2_last;
    uint64_t n_map_no_normal;  /* map points whose normal is NaN: fewer than normals_k other points, or a neighbourhood of identical points */
} erasor_refine_plane_summary;

/* Arguments and errors as erasor_hip_refine_poses_clouds.  ERASOR_E_INVALID also: normals_k outside 2 .. 32, max_curvature not a
 * finite number > 0, rank_tol not a finite number within [0, 1); each message names the parameter. */
int erasor_hip_refine_poses_plane_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device,
                                         const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                         int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                                         const erasor_refine_plane_params *params, erasor_refine_plane_row *rows,
                                         erasor_refine_plane_summary *summary);
/* the same against the handle's current map, as erasor_hip_refine_poses_map */
int erasor_hip_refine_poses_plane_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets,
                                      size_t n_frames, int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                                      const erasor_refine_plane_params *params, erasor_refine_plane_row *rows,
                                      erasor_refine_plane_summary *summary);

/* ---- the see-through check: map points voted out by every scan's range image ----------------------------------------------------
 * stands in for: nothing the reference runs.  ERASOR rejects by its bin-wise height test alone; the reference only COMPARES its result
 * against the visibility-based methods' maps (README.md:214, roslaunch erasor compare_results.launch, and the OctoMap / PeopleRemover /
 * Removert panels of img/<seq>/README.md), and erasor_hip_label_map exists so that such maps can be scored here.  This call produces
 * that second opinion: a map point that later scans look straight through was not static.
 * The contract; the normative text is erasor_amd/evalmap.py (visibility / visibility_brute), which the device equals byte for byte.
 * Float64 on the float32 coordinates, every operation a separate IEEE operation in the order written, nothing but + - * /, sqrt and
 * comparisons -- the pixel grid is data, two tables of tangents, so that no pixel needs atan2:
 *   - the pixel of (x, y, z) in a lidar frame, W columns (M = W / 8 per octant) and H rows: a = |x|, b = |y|; a == b == 0 is ON THE
 *     AXIS.  t = min(a, b) / max(a, b), j = the number of col_tan entries <= t.  The quadrant q is 0 (x >= 0, y >= 0), 1 (x < 0,
 *     y >= 0), 2 (x < 0, y < 0), 3 (x >= 0, y < 0), a zero of either sign being >= 0; the octant o = 2 q + odd, odd = (a < b) in
 *     quadrants 0 and 2 and !(a < b) in 1 and 3 (octants counted counter-clockwise from +x).  The column is o M + j in an even octant
 *     and o M + (M - 1) - j, mirrored, in an odd one.  s = z / sqrt(x*x + y*y), row = (the number of row_tan entries <= s) - 1; a row
 *     outside 0 .. H - 1 is OUT OF VIEW.  rho = sqrt((x*x + y*y) + z*z);
 *   - the gates, in this order: a non-finite coordinate, on the axis, rho outside [min_range, max_range], out of view;
 *   - range images: per frame H x W uint32.  A scan point, as given in the lidar frame with no transform, that passes the gates puts the
 *     bits of (float)rho into its pixel by an integer minimum; an empty pixel is 0xFFFFFFFF.  The others are counted per frame and gate;
 *   - every frame's map-to-lidar transform is the rigid inverse of T_body2origin[f] . T_lidar2body (upper three rows, widened), in
 *     float64 on the host: M[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j], + A[i][3] in column 3; the inverse's
 *     rotation is M's transposed, its translation -((M[0][i] M[0][3] + M[1][i] M[1][3]) + M[2][i] M[2][3]); the lidar's origin in the
 *     map frame is M's column 3.  A map point p goes into frame f as q = ((r0 x + r1 y) + r2 z) + t per row; it is IN VIEW of f when it
 *     passes the gates;
 *   - the verdict of a point in view, with m = margin_abs + margin_rel * rho, over the non-empty pixels r (as float64) of the
 *     (2 window + 1)^2 pixels around its own, columns wrapping mod W and rows clipped, in this priority: HIT (some rho - m <= r <=
 *     rho + m), OCCLUDED (some r < rho - m), NO RETURN (every pixel empty: no evidence), THROUGH (every r > rho + m);
 *   - with k > 0 a THROUGH is demoted to GRAZING (no evidence) when |n . v| < min_cos * sqrt(v . v), v = p - the frame's origin and n
 *     the point's float32 normal of erasor_hip_normals_* with k neighbours ("up"), computed once a call on the device and never copied
 *     out; a NaN normal gates nothing (isolated fragments are what should stay removable);
 *   - a point is removed iff through >= min_through and (double)through > hit_weight * (double)hit. */
typedef struct erasor_visibility {
    uint32_t width;               /* W: columns, a multiple of 8 within 8 .. 4096 */
    uint32_t height;              /* H: rows, 1 .. 256 */
    const double *col_tan;        /* [W / 8 - 1] strictly increasing, within (0, 1): the inner column edges of an octant (host) */
    const double *row_tan;        /* [H + 1] strictly increasing, finite: the row edges from the bottom (host) */
    double min_range, max_range;  /* finite, 0 <= min_range < max_range */
    double margin_abs, margin_rel;/* finite, >= 0 */
    uint32_t window;              /* w: 0, 1 or 2 */
    uint32_t k;                   /* 0: no incidence gate; 2 .. 32: the normals' neighbourhood */
    double min_cos;               /* finite */
    uint32_t min_through;
    uint32_t reserved;            /* 0 */
    double hit_weight;            /* finite, >= 0 */
    uint64_t image_budget_bytes;  /* the frames are cut into batches whose images fit this; 0: ERASOR_VISIBILITY_IMAGE_BUDGET; at least one image */
} erasor_visibility;
#define ERASOR_VISIBILITY_IMAGE_BUDGET (256ull << 20)
#define ERASOR_VISIBILITY_MAX_FRAMES 65535

typedef struct erasor_visibility_row {  /* one frame */
    uint64_t n_points;        /* scan points given */
    uint64_t n_non_finite;    /* ... dropped: a non-finite coordinate */
    uint64_t n_on_axis;       /* ... x == y == 0 */
    uint64_t n_out_of_range;  /* ... rho outside [min_range, max_range] */
    uint64_t n_out_of_view;   /* ... a row outside 0 .. H - 1 */
    uint64_t n_pixels;        /* pixels filled */
    uint64_t n_map_in_view;   /* map points in view, and their verdicts: */
    uint64_t n_hit, n_occluded, n_no_return, n_through, n_grazing;
} erasor_visibility_row;

typedef struct erasor_visibility_result {
    uint64_t n_points;           /* map points */
    uint64_t n_never_in_view;    /* ... in view of no frame */
    uint64_t n_kept, n_removed;
    uint64_t n_removed_dynamic;  /* removed points by label, as erasor_density_result counts them */
    uint64_t n_removed_static;
    uint64_t n_map_no_normal;    /* k > 0: map points whose normal is NaN (not gated) */
    uint64_t n_in_view, n_hit, n_occluded, n_no_return, n_through, n_grazing;  /* over all frames */
} erasor_visibility_result;

/* Map, scans, offsets, T_lidar2body and T_body2origin as erasor_hip_align_frames_clouds takes them.  Every output is a host buffer and
 * may be NULL: votes (n_map x 4 uint16: in_view, hit, through, occluded), keep_mask (n_map uint8, 1 = kept), kept_xyzi (the kept rows in
 * the order given, erasor_hip_density_filter_*'s stable compaction; cap_points rows, ERASOR_E_CAPACITY after res is filled if they do
 * not fit), rows (n_frames), res.  Works in the evaluator's own scratch.  ERASOR_E_INVALID: params NULL, a bad width or height, tables
 * that are NULL or not increasing, min_range >= max_range or a negative or non-finite range or margin, window above 2, k = 1 or above
 * 32, a non-finite min_cos or hit_weight, more than 65535 frames, offsets that are not monotone, a non-finite pose entry or frame
 * transform, more than 2^30 points, and with k > 0 a non-finite map coordinate (the normals' refusal).  ERASOR_E_STATE: a step in
 * flight. */
int erasor_hip_visibility_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi,
                                 size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device,
                                 const float T_lidar2body[16] /* NULL: identity */, const float *T_body2origin,
                                 const erasor_visibility *params, uint16_t *votes, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points,
                                 erasor_visibility_row *rows, erasor_visibility_result *res);
/* the same for the handle's current map (compacted on the device as erasor_hip_normals_map does, never copied to the host and not
 * modified).  ERASOR_E_STATE also: no map. */
int erasor_hip_visibility_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                              int scans_are_device, const float T_lidar2body[16], const float *T_body2origin,
                              const erasor_visibility *params, uint16_t *votes, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points,
                              erasor_visibility_row *rows, erasor_visibility_result *res);

/* ---- carving free space: every scan's rays cast through the map's voxels ------------------------------------------------------------
 * stands in for: nothing the reference runs.  The reference only COMPARES ERASOR's map with those of OctoMap and Peopleremover
 * (roslaunch erasor compare_results.launch, src/utils/compare_map.cpp, the panels of img/<seq>/README.md,
 * scripts/semantickitti2bag/analysis_octomap.py), the two methods that put the map into a voxel grid and walk every ray of every scan
 * through it.  These calls produce OctoMap's side of that comparison: a voxel that rays pass through is free, a voxel that rays end in
 * is occupied, and the two are integrated as clamped log-odds.  Unlike the range-image vote of erasor_hip_visibility_* this separates
 * an occluder from what stands behind it in the same pixel, and depends on a voxel size, not on the sensor's beam layout.
 * The contract; the normative text is erasor_amd/evalmap.py (carve / carve_brute), which the device equals byte for byte.
 * Coordinates are float64 on the float32 inputs.  Every operation is a separate IEEE operation in the order written.  Only + - * /,
 * sqrt, floor and comparisons are used.  The log-odds are float32.
 * Voxels.
 *   - A finite point lies in cell c = floor(x / voxel) per axis.
 *   - A map point with a non-finite coordinate lies in no voxel.  It is kept, gets zero votes and log-odds l_init, and is counted as
 *     n_map_non_finite.
 *   - The map voxels are the cells that hold at least one finite map point.  Only they carry state.
 * Rays.
 *   - The forward matrix of frame f is the M of visibility_transforms: T_body2origin[f] . T_lidar2body, upper three rows, float32
 *     entries widened.
 *   - The ray's origin o is M's column 3.
 *   - A scan point (x, y, z) in the lidar frame has rho = sqrt((x x + y y) + z z).
 *   - The gates, in this order: a non-finite coordinate, then rho outside [min_range, max_range].  Both are dropped and counted per
 *     frame.
 *   - The end point is e_i = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3].
 *   - Under a rigid M the end lies within max_range of the origin, so at most 4097 cells away per axis.  A ray whose end cell is not
 *     within 4098 cells of the origin's cell on every axis (a matrix that stretches, or an end that is not finite) is dropped and
 *     counted as out of range: this keeps every walk below 3 * 4098 steps whatever the matrix.
 * Traversal.
 *   - c0 = cell(o), c1 = cell(e), n_a = |c1_a - c0_a|, step_a = +-1, N = n_x + n_y + n_z.
 *   - For an axis with n_a > 0: d_a = e_a - o_a; tMax_a = ((c0_a + (step_a > 0 ? 1 : 0)) * voxel - o_a) / d_a; tDelta_a = voxel / |d_a|.
 *   - An axis with no steps left never moves.
 *   - Each of the N steps moves the axis with the smallest tMax among the axes that still have steps left.  Ties go to x before y
 *     before z.
 *   - After the move, c_a += step_a, the steps left on that axis drop by one, and tMax_a += tDelta_a.
 *   - So the walk visits V_0 = c0 ... V_N = c1, and always ends in c1 whatever the rounding.
 *   - Free evidence: V_i for 0 <= i <= N - 1 - stop_short.
 *   - Hit evidence: V_N.
 *   - n_steps of a ray is max(0, N - stop_short).
 * One update per voxel and scan, hits first (OctoMap's insertPointCloud rule).
 *   - In frame f a map voxel is hit if any ray of f ends in it.
 *   - Otherwise it is free if any ray of f has it as free evidence.
 *   - Otherwise it is untouched.
 * Integration, per map voxel, frames in index order.
 *   - L starts at l_init.
 *   - A hit frame: L = min(L + l_hit, l_max), and hits += 1.
 *   - A free frame: L = max(L + l_miss, l_min), and misses += 1.
 *   - Everything is float32.
 *   - The log-odds are parameters.  No kernel calls log.
 * Decision.  A map point is removed iff its voxel's L < l_thr.  Every point of a voxel shares its voxel's fate. */
typedef struct erasor_carve {
    double voxel;                 /* finite, > 0 */
    double min_range, max_range;  /* finite, 0 <= min_range < max_range, max_range / voxel <= 4096 */
    float l_init, l_hit, l_miss;  /* finite; l_hit >= 0, l_miss <= 0 (erasor_amd.carve_logodds forms OctoMap's defaults) */
    float l_min, l_max, l_thr;    /* finite; l_min <= l_init <= l_max */
    uint32_t stop_short;          /* 0 .. 64: the last stop_short voxels before a ray's end give no free evidence */
    uint32_t reserved;            /* 0 */
} erasor_carve;
#define ERASOR_CARVE_MAX_FRAMES 65535
#define ERASOR_CARVE_MAX_CELLS 4096
#define ERASOR_CARVE_MAX_STOP_SHORT 64

typedef struct erasor_carve_row {  /* one frame */
    uint64_t n_points;        /* scan points given */
    uint64_t n_non_finite;    /* ... dropped: a non-finite coordinate */
    uint64_t n_out_of_range;  /* ... rho outside [min_range, max_range] (or an end out of reach) */
    uint64_t n_rays;          /* rays walked */
    uint64_t n_steps;         /* the sum of their max(0, N - stop_short) */
    uint64_t n_end_in_map;    /* rays whose end voxel is a map voxel */
    uint64_t n_voxels_hit;    /* distinct map voxels hit by this frame */
    uint64_t n_voxels_free;   /* distinct map voxels free in this frame (and not hit) */
} erasor_carve_row;

typedef struct erasor_carve_result {
    uint64_t n_points;           /* map points */
    uint64_t n_map_non_finite;   /* ... with a non-finite coordinate: in no voxel, kept */
    uint64_t n_voxels;           /* map voxels */
    uint64_t n_blocks;           /* 4 x 4 x 4 blocks that hold one */
    uint64_t n_voxels_touched;   /* map voxels with at least one hit or miss */
    uint64_t n_kept, n_removed;
    uint64_t n_removed_dynamic;  /* removed points by label, as erasor_density_result counts them */
    uint64_t n_removed_static;
    uint64_t n_scan_points, n_non_finite, n_out_of_range, n_rays, n_steps, n_end_in_map, n_voxels_hit, n_voxels_free;  /* the rows' sums */
} erasor_carve_result;

/* Map, scans, offsets, T_lidar2body and T_body2origin as erasor_hip_visibility_clouds takes them.  Every output is a host buffer and
 * may be NULL: votes (n_map x 2 uint16: the hits and misses of the point's voxel), logodds (n_map float32), keep_mask (n_map uint8,
 * 1 = kept), kept_xyzi (the kept rows in the order given, the stable compaction; cap_points rows, ERASOR_E_CAPACITY after res is
 * filled if they do not fit), rows (n_frames), res.  Works in the evaluator's own scratch.
 * ERASOR_E_INVALID: params NULL; voxel not finite or not > 0; 0 <= min_range < max_range does not hold; max_range / voxel > 4096; a
 * non-finite log-odds parameter, l_hit < 0, l_miss > 0, or not l_min <= l_init <= l_max; stop_short > 64; more than 65535 frames (the
 * uint16 votes cannot wrap); offsets that are not monotone; a non-finite pose entry or frame matrix; more than 2^30 points; a finite map
 * point or a frame origin whose cell coordinate reaches +-2^28.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_carve_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device, const void *scans_xyzi,
                            size_t n_scan_points, const uint64_t *offsets, size_t n_frames, int scans_are_device,
                            const float T_lidar2body[16] /* NULL: identity */, const float *T_body2origin, const erasor_carve *params,
                            uint16_t *votes, float *logodds, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_carve_row *rows,
                            erasor_carve_result *res);
/* the same for the handle's current map (compacted on the device as erasor_hip_visibility_map does, never copied to the host and not
 * modified).  ERASOR_E_STATE also: no map. */
int erasor_hip_carve_map(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                         int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, const erasor_carve *params,
                         uint16_t *votes, float *logodds, uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_carve_row *rows,
                         erasor_carve_result *res);

/* ---- every scan's ground, patch by patch; the map's ground points by vote -------------------------------------------------------
 * restates: R-GPF, erasor.cpp:183-294 (extract_initial_seeds_, estimate_plane_, the loop of extract_ground), which the reference runs
 * per bin, inside a step, for the bins the Scan Ratio Test reverts.  Here it runs on every polar patch of every scan, as the author's
 * follow-up (Patchwork) runs it, so that "which of these points are ground?" has an answer outside a step.
 * Where the contract departs from the reference:
 *   - the orders are defined: a patch's points in scan order, the seeds' candidates by (z, index), the moments by the summing rule of
 *     erasor_hip_refine_poses_* (chunks of 256, a halving tree, chunks in sequence); the reference leaves them to std::sort and PCL;
 *   - float64 on the float32 coordinates with a cyclic Jacobi solve (erasor_hip_normals_*'s); the reference fits in float32 with
 *     Eigen's JacobiSVD; the covariance is taken from raw moments over n, where PCL centres first and divides by n - 1 -- the
 *     eigenvectors are the same in exact arithmetic;
 *   - the gates: uprightness (erasor.cpp:286 carries it commented out), and elevation / flatness per ring (Patchwork's); min_z is
 *     the reference's min_h in the lidar frame.
 * The contract; the normative text is erasor_amd/evalmap.py (ground_scans / ground_votes and their *_brute twins), which the device
 * equals byte for byte.  Every operation is a separate IEEE operation in the order written.
 * Patch.
 *   - The sector of (x, y) is erasor_visibility's column over col_tan with n_sectors for the width.
 *   - r = sqrt(x x + y y); ring = (the number of ring_edge entries <= r) - 1.
 *   - The gates, in this order: a non-finite coordinate (code 255); on the axis or a ring outside 0 .. n_rings - 1 (out of range).
 *   - A patch is (frame, ring, sector).  Its points are kept in scan order.
 * Fit, per patch.
 *   - Fewer than min_points points: SPARSE.
 *   - The candidates are the points with z >= min_z, ascending by (z, index), -0.0 equal to +0.0.
 *   - lpr = (((0.0 + z_0) + z_1) + ...) / k over the first k = min(num_lpr, candidates).  No candidate: DEGENERATE.
 *   - The seeds: z >= min_z and z < lpr + th_seeds.
 *   - iters times: n members and the nine raw moments x y z xx xy xz yy yz zz over all the patch's points (a non-member holds +0.0);
 *     n < 3: DEGENERATE; mean = S / n; cov_ab = S_ab / n - mean_a mean_b; tr = (cxx + cyy) + czz; not tr > 0: DEGENERATE; the
 *     eigenvalues ascending by (value, column); the normal is the first one's column, negated iff nz < 0;
 *     d = -((nx mx + ny my) + nz mz); the new members: ((nx x + ny y) + nz z) + d < th_dist (one-sided, as the reference).
 *   - Then nz < uprightness: REJECTED_UPRIGHT; else mean_z > elevation[ring] and not (l0 / tr <= flatness[ring]): REJECTED_ELEVATION.
 * Codes, one uint8 per point: 1 a member of an OK patch; 0 judged and not a member, or any point of a REJECTED patch; 2 not judged
 * (out of range, SPARSE, DEGENERATE); 255 non-finite. */
typedef struct erasor_ground {
    uint32_t n_rings;          /* 1 .. 64 */
    uint32_t n_sectors;        /* a multiple of 8 within 8 .. 512 */
    const double *ring_edge;   /* n_rings + 1 finite, strictly increasing radii, the first >= 0 */
    const double *col_tan;     /* n_sectors / 8 - 1 tangents, strictly increasing within (0, 1) (erasor_visibility's) */
    const double *elevation;   /* n_rings entries, none NaN; NULL: +inf, the gate is off */
    const double *flatness;    /* n_rings entries, none NaN; NULL: 0 */
    uint32_t num_lpr;          /* 1 .. 64 */
    uint32_t iters;            /* 1 .. 16 */
    uint32_t min_points;       /* >= 3 */
    uint32_t min_votes;        /* the map form: a ground point has at least this many ground votes ... */
    double th_seeds, th_dist, min_z, uprightness;  /* finite */
    double ratio;              /* ... and (double)ground > ratio * (double)seen; finite */
    uint32_t keep;             /* the map form's kept_xyzi: 1 the ground rows, 0 the rest */
    uint32_t reserved;         /* 0 */
    uint64_t work_budget_bytes;  /* the map form: frames go in batches of n_map * 16 bytes each within this; 0: ERASOR_GROUND_WORK_BUDGET */
} erasor_ground;
#define ERASOR_GROUND_MAX_FRAMES 65535
#define ERASOR_GROUND_MAX_RINGS 64
#define ERASOR_GROUND_MAX_SECTORS 512
#define ERASOR_GROUND_MAX_LPR 64
#define ERASOR_GROUND_MAX_ITERS 16
#define ERASOR_GROUND_WORK_BUDGET (256ull << 20)
/* the fit's size classes: a patch of at most WAVE_POINTS points is fitted by one wavefront, a larger one by a workgroup whose LDS holds
 * SMALL_POINTS or LDS_POINTS coordinates; a patch beyond LDS_POINTS streams from memory in every pass (the same bytes) */
#define ERASOR_GROUND_WAVE_POINTS 64u
#define ERASOR_GROUND_SMALL_POINTS 1024u
#define ERASOR_GROUND_LDS_POINTS 4096u
enum { ERASOR_GROUND_EMPTY = 0, ERASOR_GROUND_OK = 1, ERASOR_GROUND_SPARSE = 2, ERASOR_GROUND_DEGENERATE = 3,
       ERASOR_GROUND_REJECTED_UPRIGHT = 4, ERASOR_GROUND_REJECTED_ELEVATION = 5 };
enum { ERASOR_GROUND_CODE_NOT = 0, ERASOR_GROUND_CODE_GROUND = 1, ERASOR_GROUND_CODE_NOT_JUDGED = 2, ERASOR_GROUND_CODE_NON_FINITE = 255 };

typedef struct erasor_ground_row {  /* one frame */
    uint64_t n_points;              /* points given (the map form: gathered) */
    uint64_t n_non_finite;          /* ... with a non-finite coordinate */
    uint64_t n_out_of_range;        /* ... on the axis or in no ring */
    uint64_t n_judged;              /* ... of OK and REJECTED patches: code 0 or 1 */
    uint64_t n_ground;              /* ... code 1 */
    uint64_t n_ground_dynamic;      /* ... of those labelled 252 .. 259 */
    uint64_t n_patches;             /* non-empty patches */
    uint64_t n_sparse, n_degenerate, n_rejected_upright, n_rejected_elevation;  /* ... by status */
    uint64_t n_gathered;            /* the map form: map points gathered into this frame; erasor_hip_ground_scans: 0 */
} erasor_ground_row;

typedef struct erasor_ground_patch {  /* one (frame, ring, sector) */
    uint32_t status;     /* ERASOR_GROUND_EMPTY .. REJECTED_ELEVATION */
    uint32_t n_points;
    uint32_t n_ground;   /* OK: the members */
    uint32_t reserved;
    double normal[3], d, mean_z, eig[3];  /* OK and REJECTED: the last iteration's plane, its members' mean z, the eigenvalues ascending; else 0 */
} erasor_ground_patch;

typedef struct erasor_ground_result {
    uint64_t n_frames;
    uint64_t n_points, n_non_finite, n_out_of_range, n_judged, n_ground, n_ground_dynamic, n_patches, n_sparse, n_degenerate,
        n_rejected_upright, n_rejected_elevation;  /* the rows' sums */
    /* the map form; erasor_hip_ground_scans: 0 */
    uint64_t n_map_points;
    uint64_t n_map_ground;          /* map points decided ground */
    uint64_t n_map_ground_dynamic;  /* ... by label, as erasor_density_result counts them */
    uint64_t n_map_ground_static;
    uint64_t n_map_unseen;          /* map points no frame judged */
    uint64_t n_kept;                /* rows of kept_xyzi: n_map_ground (keep = 1) or the rest (keep = 0) */
} erasor_ground_result;

/* Every scan's ground (R-GPF, erasor.cpp:183-294, per polar patch; the departures -- defined orders, float64, the gates -- above).
 * Scans and offsets as erasor_hip_carve_clouds takes them, taken as given in the lidar frame.  Every output is a host buffer and may be
 * NULL: codes (n_scan_points uint8), rows (n_frames), patches (n_frames x n_rings x n_sectors, empty patches EMPTY and zeros), res.
 * n_frames == 0 and n_scan_points == 0 are fine.  Works in the evaluator's own scratch.
 * ERASOR_E_INVALID, the message naming the argument: params NULL; n_rings outside 1 .. 64; n_sectors not a multiple of 8 within
 * 8 .. 512; ring_edge or col_tan NULL, not finite, not strictly increasing, ring_edge[0] < 0, col_tan outside (0, 1); a NaN in elevation
 * or flatness; num_lpr outside 1 .. 64; iters outside 1 .. 16; min_points < 3; th_seeds, th_dist, min_z, uprightness or ratio not finite;
 * more than 65535 frames; offsets NULL or not monotone; NULL scans; more than 2^30 points.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_ground_scans(erasor_hip_handle *h, const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                            int scans_are_device, const erasor_ground *params, uint8_t *codes, erasor_ground_row *rows,
                            erasor_ground_patch *patches, erasor_ground_result *res);
/* The map's ground points by vote (the same R-GPF restatement of erasor.cpp:183-294 and the same departures).  For every frame, every
 * finite map point goes into the frame's lidar frame by erasor_hip_visibility_clouds' transform, q = ((r0 x + r1 y) + r2 z) + t in
 * float64 rounded to float32; the points whose rounded coordinates are finite and have a patch are kept in map order (a stable
 * compaction) and that cloud is segmented exactly as a scan.  A map point gets seen += 1 where it was judged and ground += 1 where its
 * code was 1; it is ground iff ground >= min_votes and (double)ground > ratio * (double)seen.  Frames go in index order, in batches of
 * work_budget_bytes / (n_map * 16) frames, at least one: the result does not depend on the budget.
 * Outputs, host buffers that may be NULL: votes (n_map x 2 uint16: seen, ground), ground_mask (n_map uint8, 1 = ground), kept_xyzi (the
 * ground rows or the rest by params->keep, in map order; cap_points rows, ERASOR_E_CAPACITY after res is filled if they do not fit),
 * rows (n_frames), res.  ERASOR_E_INVALID as erasor_hip_ground_scans, and: T_body2origin NULL with frames, a non-finite pose entry or
 * frame transform (the message names the frame), a NULL map with points. */
int erasor_hip_ground_votes_clouds(erasor_hip_handle *h, const void *map_xyzi, size_t n_map, int map_is_device,
                                   const float T_lidar2body[16] /* NULL: identity */, const float *T_body2origin, size_t n_frames,
                                   const erasor_ground *params, uint16_t *votes, uint8_t *ground_mask, float *kept_xyzi, size_t cap_points,
                                   erasor_ground_row *rows, erasor_ground_result *res);
/* the same for the handle's current map (compacted on the device as erasor_hip_carve_map does, never copied to the host and not
 * modified).  ERASOR_E_STATE also: no map. */
int erasor_hip_ground_votes_map(erasor_hip_handle *h, const float T_lidar2body[16], const float *T_body2origin, size_t n_frames,
                                const erasor_ground *params, uint16_t *votes, uint8_t *ground_mask, float *kept_xyzi, size_t cap_points,
                                erasor_ground_row *rows, erasor_ground_result *res);

/* ---- every scan's points labelled static or moving from a cleaned map ---------------------------------------------------------
 * replaces: what users of a cleaned map do on the host afterwards -- a KD-tree over the cleaned map, a radius test per scan point, the
 * scan's moving points dropped (automatic moving-object-segmentation labels, cleaned scans for re-mapping); the reference itself stops
 * at the map.  Frame f is the scans' points [offsets[f], offsets[f + 1]) as given, put into the map frame exactly as
 * erasor_hip_align_frames_clouds puts them (T_lidar2body, NULL for the identity and still applied, then T_body2origin[f], in float32).
 * With d_s / d_r the float64 distances from a point to its nearest static-map / raw-map point (as cKDTree returns them) its code is
 *   0   static:  d_s < tau
 *   1   dynamic: not static, and no raw map was given or d_r < tau
 *   2   unknown: a raw map was given, not static, and d_r >= tau (structure neither map holds)
 *   255 dropped: a non-finite coordinate after the two transforms.
 * An empty static map: nothing is static.  An empty raw map that is given (have_raw != 0, n_raw == 0): everything else is unknown.  The
 * answer is exact: the search is bounded by tau and stops at the first map point within it, and decides as the distances would.
 * The scan's own label: moving when uint32(intensity) & 0xFFFF is in 252..259; an intensity that is not finite or outside [0, 2^32)
 * counts as static and is counted. */
typedef struct erasor_scan_label_row {
    uint64_t n_points;              /* points of the frame as given */
    uint64_t n_non_finite;          /* dropped (code 255) */
    uint64_t n_label_out_of_range;  /* kept points whose intensity is not finite or outside [0, 2^32): decoded as static */
    uint64_t n[2][3];               /* [the scan's own label: 0 static, 1 moving][code 0, 1, 2] */
} erasor_scan_label_row;

/* The static map, the optional raw map (have_raw) and the concatenated scans, each on the host or on the handle's device (_is_device);
 * offsets / T_lidar2body / T_body2origin as erasor_hip_align_frames_clouds takes them; rows: n_frames entries; summary (optional): the
 * sum of the rows.  codes (optional, host): one byte per scan point.  The split (optional): the rows of the points with code split_code,
 * as given (sensor frame, all four floats copied as bits), frame by frame in scan order, into split_xyzi (host, split_cap rows), and
 * split_offsets (host, n_frames + 1 entries: frame f's rows are [split_offsets[f], split_offsets[f + 1])); either may be NULL, both
 * NULL: no split.  n_scan_points rows always suffice; a smaller buffer that does not hold the result gives ERASOR_E_CAPACITY (rows,
 * summary, codes and split_offsets are filled first).  Works in the evaluator's own scratch: announced nodes, tickets and the last
 * step's clouds stay as they are.
 * ERASOR_E_INVALID: as erasor_hip_align_frames_clouds (poses, offsets, 2^30 points, 65536 frames, a non-finite map point); tau not a
 * finite number > 0; a split with split_code outside 0..2, or 2 without a raw map.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_label_scans_clouds(erasor_hip_handle *h, const void *static_xyzi, size_t n_static, int static_is_device,
                                  const void *raw_xyzi, size_t n_raw, int raw_is_device, int have_raw,
                                  const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                                  int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, double tau,
                                  uint8_t *codes, int split_code, float *split_xyzi, size_t split_cap, uint64_t *split_offsets,
                                  erasor_scan_label_row *rows, erasor_scan_label_row *summary);
/* the same with the handle's current map as the static map (the erasor_hip_get_map view, compacted on the device as
 * erasor_hip_overlap_map does, never copied to the host).  ERASOR_E_STATE also: no map. */
int erasor_hip_label_scans_map(erasor_hip_handle *h, const void *raw_xyzi, size_t n_raw, int raw_is_device, int have_raw,
                               const void *scans_xyzi, size_t n_scan_points, const uint64_t *offsets, size_t n_frames,
                               int scans_are_device, const float T_lidar2body[16], const float *T_body2origin, double tau,
                               uint8_t *codes, int split_code, float *split_xyzi, size_t split_cap, uint64_t *split_offsets,
                               erasor_scan_label_row *rows, erasor_scan_label_row *summary);

/* ---- a cloud as connected objects: Euclidean clustering, listed and filtered by size --------------------------------------------
 * replaces: what users of a cleaned map do on the host afterwards -- pcl::EuclideanClusterExtraction (a KD-tree and a region-growing
 * loop) over the removed points, the left-over dynamic points or the whole map, then "drop every cluster smaller than n points"; the
 * reference itself stops at the map.  The contract, restated on the host by erasor_amd/evalmap.py (cluster, cluster_brute), which the
 * device equals byte for byte:
 *   - points i and j are adjacent iff ((dx*dx + dy*dy) + dz*dz) <= tol*tol, dx = (double)x_i - (double)x_j and likewise dy, dz, all
 *     in float64, left to right, no fused multiply-add (symmetric bit for bit);
 *   - a cluster is a connected component of that graph; its name is `first`, the lowest point index it contains;
 *   - a cluster is listed when min_size <= n_points and (max_size == 0 or n_points <= max_size) -- the size limits of
 *     pcl::EuclideanClusterExtraction; min_size 0 is taken as 1;
 *   - one row per listed cluster, in increasing `first`.
 * There is no centroid: a float sum depends on the order of its terms, a box and a count do not, and nothing in the result depends
 * on how the device scheduled its work.  Up to the metric at the very edge d == tol this is the partition PCL's region growing
 * produces; PCL measures in float32, is not a dependency of this project, and the contract is not pinned against it. */
typedef struct erasor_cluster_row {
    uint32_t first;                 /* the lowest point index of the cluster */
    uint32_t n_points;
    uint32_t n_dynamic;             /* points whose uint32(intensity) & 0xFFFF is in 252..259 */
    uint32_t n_label_out_of_range;  /* points whose intensity is not finite or outside [0, 2^32): decoded as static */
    float min_xyz[3], max_xyz[3];   /* the box, per coordinate in float32's total order (-0.0 below +0.0), copied as bits */
} erasor_cluster_row;

typedef struct erasor_cluster_result {
    uint64_t n_points;         /* points given */
    uint64_t n_clusters;       /* all clusters, listed or not */
    uint64_t n_listed;         /* rows */
    uint64_t n_points_listed;  /* points of listed clusters: the kept cloud's rows */
    uint64_t n_singletons;     /* clusters of one point */
    uint64_t largest;          /* the largest n_points of any cluster */
} erasor_cluster_result;

/* The cloud (XYZI rows, on the host or on the handle's device: is_device) clustered at the tolerance tol.  All outputs are host
 * buffers and optional.  ids (n entries): the index of point i's cluster among the rows, or 0xFFFFFFFF when its cluster is not listed.
 * rows (cap_rows entries) and kept_xyzi (cap_points rows): the listed clusters, and the rows of all points of listed clusters in the
 * order given, all four floats copied as bits (the residue filter); NULL asks for the counts only.  n rows always suffice for either;
 * a buffer that does not hold the result gives ERASOR_E_CAPACITY, with res, and ids if asked for, filled first.  n == 0: zero clusters,
 * ERASOR_OK.  Works in the evaluator's own scratch: announced nodes, tickets and the last step's clouds stay as they are.
 * ERASOR_E_INVALID: a non-finite coordinate, tol not a finite number > 0, more than 2^30 points, res NULL.  ERASOR_E_STATE: a step in
 * flight. */
int erasor_hip_cluster_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, double tol, size_t min_size,
                              size_t max_size, uint32_t *ids, erasor_cluster_row *rows, size_t cap_rows, float *kept_xyzi,
                              size_t cap_points, erasor_cluster_result *res);
/* the same over the handle's current map (the erasor_hip_get_map view, compacted on the device as erasor_hip_overlap_map does, never
 * copied to the host).  ERASOR_E_STATE also: no map. */
int erasor_hip_cluster_map(erasor_hip_handle *h, double tol, size_t min_size, size_t max_size, uint32_t *ids,
                           erasor_cluster_row *rows, size_t cap_rows, float *kept_xyzi, size_t cap_points,
                           erasor_cluster_result *res);

/* ---- the decision per object: a removal method's votes spread over clusters, fragments reverted ------------------------------------
 * replaces: nothing in the reference, which decides bin by bin and stops there; ERASOR2 decides per instance and Removert has a
 * "revert" stage for the two failures this repairs -- half of a moving object left standing because no vote reached its lower part,
 * and static structure chewed by stray votes.  Every removal method here decides one point at a time (a step by bin, the see-through
 * check by pixel vote, the carving by voxel log-odds); this call takes such per-point votes, finds the objects they fall on and
 * decides per object.  The contract, restated on the host by erasor_amd/evalmap.py (object_vote, object_vote_brute), which the device
 * equals byte for byte; every definition is free of order:
 *   - point i is VOTED iff votes[i] >= vote_thr (1 <= vote_thr <= 255; votes may be a sum over several methods: vote_thr 2 of three
 *     is their majority) and GROUND iff ground[i] != 0 (ground NULL: no point is);
 *   - ground points are outside the graph: adjacent to nothing, members of no cluster.  A ground point comes out kept if ground_keep,
 *     otherwise removed iff voted.  The ground is what connects everything (a voxelised map is a handful of clusters at tol 0.5):
 *     the mask is what cuts the objects loose;
 *   - over the other points adjacency is erasor_hip_cluster_*'s: ((dx*dx + dy*dy) + dz*dz) <= tol*tol in float64 on the float32
 *     coordinates, left to right, no fused multiply-add.  A cluster is a connected component; its `first` is the lowest index it
 *     contains in the GIVEN cloud's indexing;
 *   - a cluster's decision, tested in this order:
 *       ERASOR_OBJECT_NOT_OBJECT (3)  n_points < max(min_size, 1), or max_size != 0 and n_points > max_size, or max_extent > 0 and
 *                                     (double)max - (double)min > max_extent on some axis: per-point votes stand;
 *       ERASOR_OBJECT_REMOVED (1)     n_voted >= min_voted and (double)n_voted >= remove_ratio * (double)n_points (one float64
 *                                     multiply): every point of the cluster is removed;
 *       ERASOR_OBJECT_REVERTED (2)    n_voted > 0 and (double)n_voted <= revert_ratio * (double)n_points: every point is kept;
 *       ERASOR_OBJECT_UNCHANGED (0)   per-point votes stand;
 *   - one row per TOUCHED cluster (n_voted > 0), in increasing `first`; untouched clusters are counted, not listed.
 * With revert_ratio 0 (the default of every wrapper) nothing is ever reverted, on purpose: where the ground mask is incomplete one
 * huge cluster holds every car through the ground, and its tiny vote share must not wipe the votes out.  Set max_size or max_extent
 * before using revert_ratio.  As for the clusters there is no centroid and no float sum: counts, boxes and one float64 product per
 * cluster, none of which depends on how the device scheduled its work. */
enum { ERASOR_OBJECT_UNCHANGED = 0, ERASOR_OBJECT_REMOVED = 1, ERASOR_OBJECT_REVERTED = 2, ERASOR_OBJECT_NOT_OBJECT = 3 };

typedef struct erasor_object_vote_params {
    double tol;           /* finite, > 0 */
    double max_extent;    /* 0: no limit; otherwise finite, > 0: the longest box side of an object */
    double remove_ratio;  /* within (0, 1] */
    double revert_ratio;  /* within [0, 1) and below remove_ratio; 0: nothing is reverted */
    uint64_t min_size;    /* 0 is taken as 1 */
    uint64_t max_size;    /* 0: no limit */
    uint64_t min_voted;
    uint32_t vote_thr;    /* 1 .. 255 */
    uint32_t ground_keep; /* != 0: every ground point is kept; 0: a ground point is removed iff voted */
} erasor_object_vote_params;

typedef struct erasor_object_row {
    uint32_t first;                 /* the lowest index of the cluster, in the given cloud's indexing */
    uint32_t n_points;
    uint32_t n_voted;
    uint32_t n_dynamic;             /* points whose uint32(intensity) & 0xFFFF is in 252..259, decoded as erasor_hip_cluster_* does */
    uint32_t n_voted_dynamic;
    uint32_t n_label_out_of_range;
    float min_xyz[3], max_xyz[3];   /* the box, per coordinate in float32's total order, copied as bits */
    uint32_t decision;              /* ERASOR_OBJECT_* */
} erasor_object_row;

typedef struct erasor_object_vote_result {
    uint64_t n_points;             /* points given */
    uint64_t n_ground;
    uint64_t n_clusters;           /* all clusters of the non-ground points, touched or not */
    uint64_t n_touched;            /* rows */
    uint64_t n_removed_clusters;
    uint64_t n_reverted_clusters;
    uint64_t n_not_object;         /* touched clusters with ERASOR_OBJECT_NOT_OBJECT */
    uint64_t n_voted;              /* voted points, ground points included */
    uint64_t n_removed;            /* points with mask 0: n_points - n_removed is the kept cloud's rows */
    uint64_t n_grown;              /* unvoted points that come out removed ... */
    uint64_t n_grown_dynamic;      /* ... and how many of them carry a dynamic label: whether the growth eats structure */
    uint64_t n_reverted;           /* voted non-ground points that come out kept */
    uint64_t n_reverted_dynamic;
    uint64_t n_ground_reverted;    /* voted ground points that come out kept */
    uint64_t n_ground_reverted_dynamic;
    uint64_t largest;              /* the largest n_points of any cluster */
} erasor_object_vote_result;

/* The cloud (XYZI rows, on the host or on the handle's device: is_device) with one vote byte and, unless ground is NULL, one ground
 * byte per point (host arrays of n bytes).  All outputs are host buffers and optional: mask (n bytes, 1 = kept, as the see-through
 * check and the carving return it), ids (n entries: the point's row index, or 0xFFFFFFFF for ground points and points of untouched
 * clusters), rows (cap_rows entries), kept_xyzi (cap_points rows: the rows with mask 1 in the order given, all four floats copied as
 * bits).  n rows always suffice for either; a buffer that does not hold the result gives ERASOR_E_CAPACITY, with res, and mask and
 * ids if asked for, filled first.  n == 0: ERASOR_OK and a zero result.  Works in the evaluator's own scratch: announced nodes,
 * tickets and the last step's clouds stay as they are.  ERASOR_E_INVALID: a non-finite coordinate (of any point, ground or not), tol
 * not a finite number > 0, remove_ratio outside (0, 1], revert_ratio outside [0, 1) or not below remove_ratio, vote_thr outside
 * 1 .. 255, max_extent negative or not finite, more than 2^30 points, params, votes or res NULL.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_object_vote_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, const uint8_t *votes,
                                  const uint8_t *ground, const erasor_object_vote_params *params, uint8_t *mask, uint32_t *ids,
                                  erasor_object_row *rows, size_t cap_rows, float *kept_xyzi, size_t cap_points,
                                  erasor_object_vote_result *res);
/* the same over the handle's current map (the erasor_hip_get_map view, compacted on the device as erasor_hip_cluster_map does, never
 * copied to the host); votes and ground index that view.  ERASOR_E_INVALID also: n is not erasor_hip_map_size.  ERASOR_E_STATE
 * also: no map. */
int erasor_hip_object_vote_map(erasor_hip_handle *h, const uint8_t *votes, const uint8_t *ground, size_t n,
                               const erasor_object_vote_params *params, uint8_t *mask, uint32_t *ids, erasor_object_row *rows,
                               size_t cap_rows, float *kept_xyzi, size_t cap_points, erasor_object_vote_result *res);

/* ---- how dense the cloud is around each point: k nearest neighbours, radius counts, and the outlier filters on them ---------------
 * replaces: what users of a cleaned map run on the host next -- pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval, a
 * KD-tree over the whole map -- to drop the single returns in the air, the thin shells dynamic removal leaves behind and the stray
 * centroids at the rim of a reverted bin.  erasor_hip_cluster_* only drops disconnected fragments: it does not find a lone point one
 * tolerance from a wall, and has no notion of "sparser than the rest of this map".  The contract, restated on the host by
 * erasor_amd/evalmap.py (knn / knn_brute, radius_count / radius_count_brute, density_filter), which the device equals byte for byte:
 *   - distance: ex = (double)x_i - (double)x_j and likewise ey, ez; d2 = (ex*ex + ey*ey) + ez*ez in float64, left to right, no fused
 *     multiply-add; d = sqrt(d2), correctly rounded;
 *   - the neighbour order of point i: every j != i by (d2, j) ascending, a total order under any number of ties and duplicates.  Self
 *     is excluded by index, not by distance: an identical point at another index is a neighbour at distance 0;
 *   - knn, 1 <= k <= 32: the first k entries of that order as nbr_idx[i*k + e] / nbr_dist[i*k + e]; kth[i] = nbr_dist[i*k + k-1];
 *     mean[i] = (((0.0 + d_0) + d_1) + ... + d_{k-1}) / (double)k.  A point with fewer than k other points (n - 1 < k): the missing
 *     entries are index 0xFFFFFFFF and distance +inf, kth and mean are +inf, and it is counted in n_short;
 *   - radius count: count[i] = the number of j != i with d2 <= r*r, r*r formed once in float64;
 *   - the statistics of a score are taken over the points whose score is finite (n_scored): min, median, p90, p99, max exactly as
 *     erasor_hip_overlap_* takes its median and percentiles (the same ranks, the same interpolation, exact order statistics); NaN
 *     when n_scored == 0.
 * Not offered: PCL's mean + mul * sigma.  Sigma is a float sum and its value depends on the order of its terms; a median and a median
 * absolute deviation do not.  Up to that rule and PCL's float32 metric, MEAN / MAD is StatisticalOutlierRemoval's selection and COUNT
 * is RadiusOutlierRemoval's; PCL is not a dependency of this project and nothing is pinned against it. */
typedef struct erasor_score_stats {
    uint64_t n_scored;                  /* points whose score is finite */
    double min, median, p90, p99, max;  /* over those; NaN when there are none */
} erasor_score_stats;

typedef struct erasor_knn_result {
    uint64_t n_points;  /* points given */
    uint64_t n_short;   /* points with fewer than k other points: padded lists, kth = mean = +inf */
    erasor_score_stats kth, mean;
} erasor_knn_result;

enum { ERASOR_DENSITY_KTH = 0, ERASOR_DENSITY_MEAN = 1, ERASOR_DENSITY_COUNT = 2 };  /* erasor_density_filter.score */
enum { ERASOR_DENSITY_ABS = 0, ERASOR_DENSITY_MAD = 1 };                             /* erasor_density_filter.rule */

/* One filter.  score KTH / MEAN (the k-th neighbour's distance, the mean distance of the k nearest; both need k) with rule
 *   ABS: keep iff score <= thr, thr given, finite and >= 0;
 *   MAD: m = the median of the finite scores, dev_i = |score_i - m| in float64 over them, mad = the median of dev taken the same way,
 *        thr = m + mul * (1.4826 * mad) evaluated on the host in that order, mul finite and >= 0; keep iff score <= thr.
 * An infinite score is never kept and a NaN thr keeps nothing.  score COUNT (needs radius, finite and > 0): keep iff count >=
 * min_neighbors; the rule must be a known one and is not used.  Fields a filter does not need are not read. */
typedef struct erasor_density_filter {
    int32_t score, rule;
    uint32_t k, min_neighbors;
    double radius, thr, mul;
} erasor_density_filter;

typedef struct erasor_density_result {
    uint64_t n_points, n_kept, n_removed;
    uint64_t n_removed_dynamic;  /* removed points whose uint32(intensity) & 0xFFFF is in 252..259 (decoded as erasor_hip_cluster_* does) */
    uint64_t n_removed_static;   /* the other removed points: a labelled map shows at once whether the filter eats structure */
    uint64_t n_short;            /* KTH / MEAN: points with fewer than k other points (their score is +inf); COUNT: 0 */
    uint64_t n_scored;           /* points with a finite score */
    double m, mad;               /* MAD: the median and the median absolute deviation; otherwise NaN */
    double thr;                  /* the threshold applied: given (ABS), computed (MAD), (double)min_neighbors (COUNT) */
    double min, median, p90, p99, max;  /* the score's statistics over the scored points; NaN when there are none */
} erasor_density_result;

/* The k nearest neighbours of every point of the cloud (XYZI rows, on the host or on the handle's device: is_device) inside that
 * cloud.  All outputs are host buffers and optional: nbr_idx / nbr_dist (n * k entries each, row i = point i's list), kth / mean (n
 * entries); NULL asks for the rest only.  n == 0: ERASOR_OK, counts zero and statistics NaN.  Works in the evaluator's own scratch:
 * announced nodes, tickets and the last step's clouds stay as they are.  ERASOR_E_INVALID: a non-finite coordinate, k outside 1 .. 32,
 * more than 2^30 points, res NULL, neighbour lists asked for with n * k > 2^30.  ERASOR_E_STATE: a step in flight.
 * Identical points are searched exhaustively among themselves (every tie is visited): thousands of copies of one point are quadratic. */
int erasor_hip_knn_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, uint32_t k, uint32_t *nbr_idx,
                          double *nbr_dist, double *kth, double *mean, erasor_knn_result *res);
/* the same over the handle's current map (the erasor_hip_get_map view, compacted on the device as erasor_hip_cluster_map does, never
 * copied to the host).  ERASOR_E_STATE also: no map. */
int erasor_hip_knn_map(erasor_hip_handle *h, uint32_t k, uint32_t *nbr_idx, double *nbr_dist, double *kth, double *mean,
                       erasor_knn_result *res);

/* count[i] (n entries, a host buffer, optional) = the number of other points within the radius of point i, and the counts' statistics
 * (n_scored = n).  What pcl::RadiusOutlierRemoval counts on the host.  ERASOR_E_INVALID: a non-finite coordinate, radius not a finite
 * number > 0, more than 2^30 points, res NULL.  ERASOR_E_STATE: a step in flight.  Voxelise a dense cloud first: the pass is quadratic
 * in the points per radius-cell. */
int erasor_hip_radius_count_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, double radius, uint32_t *count,
                                   erasor_score_stats *res);
/* the same over the handle's current map.  ERASOR_E_STATE also: no map. */
int erasor_hip_radius_count_map(erasor_hip_handle *h, double radius, uint32_t *count, erasor_score_stats *res);

/* The cloud filtered by `filter`: keep_mask (n bytes, 1 = kept) and kept_xyzi (cap_points rows: the kept rows in the order given, all
 * four floats copied as bits), host buffers, optional; NULL asks for the counts only.  n rows always suffice; a kept buffer that
 * does not hold the result gives ERASOR_E_CAPACITY, with res, and keep_mask if asked for, filled first.  What
 * pcl::StatisticalOutlierRemoval (MEAN / MAD, up to its sigma rule) and pcl::RadiusOutlierRemoval (COUNT) do on the host.
 * ERASOR_E_INVALID: a non-finite coordinate, an unknown score or rule, k outside 1 .. 32, radius not a finite number > 0, thr or mul
 * not a finite number >= 0, more than 2^30 points, filter or res NULL.  ERASOR_E_STATE: a step in flight. */
int erasor_hip_density_filter_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, const erasor_density_filter *filter,
                                     uint8_t *keep_mask, float *kept_xyzi, size_t cap_points, erasor_density_result *res);
/* the same over the handle's current map; the map itself stays as it is.  ERASOR_E_STATE also: no map. */
int erasor_hip_density_filter_map(erasor_hip_handle *h, const erasor_density_filter *filter, uint8_t *keep_mask, float *kept_xyzi,
                                  size_t cap_points, erasor_density_result *res);

/* ---- the surface a point lies on: every point's normal, curvature and covariance eigenvalues from its k nearest neighbours ---------
 * replaces: what users of a cleaned map compute on the host next -- pcl::NormalEstimation over a KD-tree of the whole map -- and what
 * a point-to-plane registration, a shaded rendering and telling a wall from scatter start from.  The contract, restated on the host by
 * erasor_amd/evalmap.py (normals / normals_brute), which the device equals byte for byte.  Everything is float64 on the float32
 * coordinates, every operation a separate IEEE operation in the order written:
 *   - the neighbourhood of point i: the point itself first, then its k nearest other points in erasor_hip_knn_*'s order, (d2, j)
 *     ascending, self excluded by index: m = k + 1 points, 2 <= k <= 32.  A point with fewer than k other points is short: its normal,
 *     curvature and eigenvalues are NaN, and it is counted in n_short;
 *   - centroid, per axis: s = ((0.0 + p_self) + p_n0) + ... in list order, c = s / (double)m;
 *   - covariance: for each neighbourhood point in the same order e = p - c and cxx = cxx + ex*ex (likewise cxy, cxz, cyy, cyz, czz),
 *     each from 0.0; after the loop each entry divided by (double)m, PCL's scale; tr = (cxx + cyy) + czz, taken before the solve;
 *   - a point is degenerate if !(tr > 0) -- all m points identical: NaN outputs, counted in n_degenerate;
 *   - the eigen-solve: cyclic Jacobi on the symmetric 3x3, pivots (0,1), (0,2), (1,2), the rotation of erasor_hip_refine_poses' 4x4
 *     solve, a pivot that is exactly 0 skipped; it stops when all three off-diagonals are exactly 0 before a sweep, or after 32 sweeps.
 *     The eigenvalues are the diagonal, ascending by (value, column index); the normal is the column of V of the first, not
 *     renormalised.  n_ambiguous counts the points whose two smallest eigenvalues are exactly equal (an exactly collinear
 *     neighbourhood: a direction that is defined by these rules, but arbitrary) -- counted, not hidden;
 *   - curvature = fabs(l0) / tr, PCL's definition;
 *   - orientation: with a viewpoint v, s = ((vx-px)*nx + (vy-py)*ny) + (vz-pz)*nz and all three components are negated iff s < 0;
 *     without one ("up") iff nz < 0, or nz == 0 and ny < 0, or nz == 0 and ny == 0 and nx < 0.  n_flipped counts the negations;
 *   - the curvature's statistics are taken over the finite curvatures, as erasor_score_stats says.
 * Not offered: a radius neighbourhood, whose point count is unbounded (the list has no fixed size on the device and the sums no
 * bounded order), and MLS smoothing -- the reason erasor_hip_knn_* gives for sigma: sums whose value depends on the order of their
 * terms.  PCL is not a dependency of this project and nothing is pinned against it. */
typedef struct erasor_normals_result {
    uint64_t n_points;      /* points given */
    uint64_t n_short;       /* points with fewer than k other points: NaN outputs */
    uint64_t n_degenerate;  /* points whose neighbourhood has no extent (!(tr > 0)): NaN outputs */
    uint64_t n_ambiguous;   /* points whose two smallest eigenvalues are exactly equal */
    uint64_t n_flipped;     /* normals negated by the orientation rule */
    erasor_score_stats curvature;  /* over the finite curvatures (n_points - n_short - n_degenerate of them) */
} erasor_normals_result;

/* The normals of every point of the cloud (XYZI rows, on the host or on the handle's device: is_device) from its neighbourhood inside
 * that cloud -- pcl::NormalEstimation with setKSearch(k) and setViewPoint on the host.  viewpoint: three float64, or NULL for "up".
 * All outputs are host buffers and optional: normals (n * 3 float32), curvature (n float64), eigenvalues (n * 3 float64, ascending);
 * NULL asks for the rest only.  n == 0: ERASOR_OK, counts zero and statistics NaN.  Works in the evaluator's own scratch: announced
 * nodes, tickets and the last step's clouds stay as they are.  ERASOR_E_INVALID: a non-finite coordinate, k outside 2 .. 32, a
 * non-finite viewpoint, more than 2^30 points, res NULL.  ERASOR_E_STATE: a step in flight.  The search is erasor_hip_knn_*'s:
 * thousands of copies of one point are quadratic. */
int erasor_hip_normals_clouds(erasor_hip_handle *h, const void *xyzi, size_t n, int is_device, uint32_t k,
                              const double *viewpoint /* NULL: up */, float *normals, double *curvature, double *eigenvalues,
                              erasor_normals_result *res);
/* the same over the handle's current map (the erasor_hip_get_map view, compacted on the device as erasor_hip_knn_map does, never
 * copied to the host) -- pcl::NormalEstimation over the map.  ERASOR_E_STATE also: no map. */
int erasor_hip_normals_map(erasor_hip_handle *h, uint32_t k, const double *viewpoint /* NULL: up */, float *normals, double *curvature,
                           double *eigenvalues, erasor_normals_result *res);

/* ---- maps without labels: label a third-party map from a dense labelled one, and the static points a method lost ----------------
 * Both search the overlap report's tree in FLANN's metric, as pcl::KdTreeFLANN (K = 1) does: float32 d^2 = ((0 + dx*dx) + dy*dy) + dz*dz
 * with dx = q.x - p.x in float, exact, the lowest index on ties.  Outputs are XYZI rows in caller HOST buffers; dst == NULL asks for
 * the counts only.  n_out <= n_src and n_lost <= n_gt, so a buffer of that many rows always suffices; a smaller one that does not hold
 * the result gives ERASOR_E_CAPACITY (res is filled first).  ERASOR_E_INVALID: a non-finite coordinate, more than 2^30 points.
 * ERASOR_E_STATE: a step in flight. */
typedef struct erasor_label_result {
    uint64_t n_src;        /* points given */
    uint64_t n_out;        /* rows written: the VoxelGrid centroids (n_src when passthrough) */
    uint64_t n_tied;       /* rows whose nearest distance is shared by medium points of different intensity bits (the tie rule decided) */
    uint32_t passthrough;  /* 1: VoxelGrid's voxel index overflowed and the input was labelled as it is, as PCL returns it */
} erasor_label_result;

/* replaces: label_map (src/utils/fill_removert_intensity.cpp:24-59; the same at src/utils/compare_map.cpp:77-110).  src is voxelised by
 * pcl::VoxelGrid at `leaf` (voxelize_preserving_labels' grid and centroids); each centroid's row is its x, y, z and the intensity of its
 * nearest `medium` point, copied as bits.  Like erasor_hip_evaluate_clouds with voxel_leaf > 0 it drops nodes announced ahead, and
 * erasor_hip_get_cloud answers ERASOR_E_STATE until the next step.  Where the reference is undefined: an empty src gives an empty
 * output; an empty medium with a non-empty src is ERASOR_E_INVALID; leaf must be finite and > 0. */
int erasor_hip_label_map(erasor_hip_handle *h, const void *src_xyzi, size_t n_src, int src_is_device,
                         const void *medium_xyzi, size_t n_medium, int medium_is_device,
                         double leaf, float *dst_xyzi, size_t cap_points, erasor_label_result *res);

typedef struct erasor_complement_result {
    uint64_t n_gt;                  /* ground-truth points given */
    uint64_t n_gt_static;           /* of them static: uint32(intensity) & 0xFFFF not in 252..259 */
    uint64_t n_lost;                /* static points whose nearest estimated point has (double)d2 > 0.03 (rows written) */
    uint64_t n_label_out_of_range;  /* intensities not finite or outside [0, 2^32): decoded as static */
} erasor_complement_result;

/* replaces: calc_complement (src/utils/compare_complement.cpp:43-75): the static ground-truth points whose nearest estimated point has a
 * float squared distance greater than 0.03 (compared as double, as the reference's literal is), in ground-truth order -- what the
 * method wrongly removed.  The intensity's instance bits (>> 16) are ignored.  An empty estimate (the reference would push nothing)
 * gives every static point: the distance is +inf.  Works in the evaluator's own scratch: announcements and the last step's clouds stay
 * as they are. */
int erasor_hip_static_complement(erasor_hip_handle *h, const void *est_xyzi, size_t n_est, int est_is_device,
                                 const void *gt_xyzi, size_t n_gt, int gt_is_device,
                                 float *dst_xyzi, size_t cap_points, erasor_complement_result *res);

/* ---- mapgen: the step BEFORE the hot path (src/mapgen/mapgen.hpp), device-resident accumulation ----
 * replaces: mapgen::setValue + constructor (mapgen.hpp:182-196): leafsize = /map/voxelsize, is_large_scale */
int erasor_hip_mapgen_begin(erasor_hip_handle *h, double leafsize, int is_large_scale);
/* replaces: mapgen::accumPointCloud (mapgen.hpp:198-257) for one erasor::node: self-filter of points closer than
 * CAR_BODY_SIZE (2.7 m, :219-228), lidar->origin-of-body then pose (two pcl::transformPointCloud, :231-237; pass
 * T_lidar2origin = NULL for the reference's constant, z + 1.73), voxelize_preserving_labels at 0.2 m -> cloud_curr
 * (:239), cloud_map += cloud_curr, and in large-scale mode the re-voxelisation of the accumulated submap on the
 * first and every 500th accumulated scan (:247-255).  T_pose = geoPose2eigen(node.odom), row-major. */
int erasor_hip_mapgen_accum(erasor_hip_handle *h, const float *scan_xyzi, size_t n, const float T_pose[16],
                            const float T_lidar2origin[16], size_t *n_curr);
/* replaces: mapgen::getPointClouds (:258-262) and saveNaiveMap's un-voxelised cloud_src (:267-279).
 * which: 0 cloud_curr, 1 cloud_map, 2 all finished submaps followed by cloud_map.  dst may be NULL (size query). */
int erasor_hip_mapgen_get(erasor_hip_handle *h, int which, float *dst_xyzi, size_t cap_points, size_t *n_out);
/* replaces: saveNaiveMap's voxelize_preserving_labels(cloud_src, leafsize) (:281-299): the map that is saved as
 * <seq>_<from>_to_<to>_w_interval<k>_voxel_<leaf>.pcd and later loaded by OfflineMapUpdater::load_global_map */
int erasor_hip_mapgen_save(erasor_hip_handle *h, float *dst_xyzi, size_t cap_points, size_t *n_out);

/* replaces: erasor_utils::parse_dynamic_obj as counters (utils.cpp:57-78) over the current map */
int erasor_hip_count_static_dynamic(erasor_hip_handle *h, uint64_t *n_static, uint64_t *n_dynamic);

/* ---- host records in the caller's layout, and announcements by ticket (round 4) ------------------------------------------
 * replaces: pcl::fromROSMsg(msg->lidar, *ptr_query) (OMU.cpp:237) handing a pcl::PointCloud<pcl::PointXYZI> to the per-scan path.
 * `rows`: n records of `stride_bytes` bytes, float x, y, z at byte 0, float intensity at byte `intensity_offset_bytes`
 * (XYZI rows: 16 / 12; pcl::PointXYZI: 32 / 16).  The pass that stages a host scan in pinned memory repacks it, so the caller does
 * not rewrite the cloud into XYZI rows first.  Host memory only. */
int erasor_hip_step_rows(erasor_hip_handle *h, const void *rows, size_t n, size_t stride_bytes, size_t intensity_offset_bytes,
                         const float T_lidar2body[16], const float T_body2origin[16], const float T_origin2body[16],
                         erasor_step_result *res);
/* Announce the NEXT node (like erasor_hip_prefetch_node; T_body2origin may be NULL = erasor_hip_prefetch_scan) and get its ticket
 * (never 0).  The buffer is the caller's again when this returns. */
int erasor_hip_prefetch_node_rows(erasor_hip_handle *h, const void *rows, size_t n, size_t stride_bytes, size_t intensity_offset_bytes,
                                  const float T_lidar2body[16], const float *T_body2origin, uint64_t *ticket);
/* The step of the announced node that holds `ticket` (tickets are consumed in the order of the announcements; anything else is
 * ERASOR_E_STATE).  T_lidar2body is the announcement's.  _async: first half only, collect with erasor_hip_step_wait. */
int erasor_hip_step_ticket(erasor_hip_handle *h, uint64_t ticket, const float T_body2origin[16], const float T_origin2body[16],
                           erasor_step_result *res);
int erasor_hip_step_ticket_async(erasor_hip_handle *h, uint64_t ticket, const float T_body2origin[16], const float T_origin2body[16]);

/* ---- one host process, several devices (round 4) --------------------------------------------------------------------------
 * replaces: one OfflineMapUpdater per process, each loading the global map itself (main_kitti.cpp:4-11, main_in_your_env.cpp:92-123,
 * OfflineMapUpdater::load_global_map OMU.cpp:107-135) when ONE process drives several GPUs: the map of handles[root] is sent to every
 * other handle (one per device, erasor_hip_create(.., device, ..)) -- single-process RCCL (ncclCommInitAll + ncclBroadcast of the
 * XYZI rows over xGMI; librccl is loaded on first use), hipMemcpyPeerAsync where RCCL is not available or two handles share a device.
 * The receivers end up as after erasor_hip_set_map.  *transport (may be NULL): 1 RCCL, 2 peer copies, 0 empty map.
 * Replicas then run independently (scans are a sequential fold over ONE map): no per-scan communication. */
int erasor_hip_replicate_map(erasor_hip_handle *const *handles, int n, int root, int *transport);

/* ---- measurement hooks (no reference counterpart) ------------------------ */
/* When enabled, every kernel launch of a step is bracketed by HIP events on the
 * handle's stream; totals are accumulated per kernel name. */
/* enable: 0 off, 1 every kernel, 2 only the HBM-roofline kernel (voi_split), timed by start / stop events attached
 * to its launch (hipExtLaunchKernelGGL): the kernel's own execution window, without perturbing the step */
int erasor_hip_profiling(erasor_hip_handle *h, int enable);
int erasor_hip_profile_reset(erasor_hip_handle *h);
/* returns number of distinct kernels; fills up to cap entries */
int erasor_hip_profile_get(erasor_hip_handle *h, const char **names, double *total_ms,
                           uint64_t *launches, size_t cap, size_t *n);
/* HBM bytes the voi_split kernel must read per launch for the current map: 16 * physical entries */
int erasor_hip_voi_split_bytes(erasor_hip_handle *h, uint64_t *algorithmic_bytes, uint64_t *physical_entries);
/* VoI splits launched ahead of their step (erasor_hip_prefetch_node) and how many of them the following step could use */
int erasor_hip_ahead_split_counts(erasor_hip_handle *h, uint64_t *launched, uint64_t *used);
/* Round 5 -- OVERLAPPED steps.  The scans of one sequence are a sequential fold over the map (OfflineMapUpdater.cpp:290 -> :393), but only
 * the points of the bins the Scan Ratio Test reverts (erasor.cpp:510-528) have to wait for R-GPF: a step writes everything else back
 * at once, reserving the reverted bins' places at full size, and -- when the NEXT node was announced with its pose
 * (erasor_hip_prefetch_node*) AND its inverse transform (this call, right after the announcement; the step must then pass the very same
 * 16 floats, tf_body2origin_.inverse() of OfflineMapUpdater.cpp:436) -- that node's fetch_VoI pass, transform and R-POD keys run beside
 * this step's per-bin launch on a second stream; the reserved places are filled in (or left as holes) when the per-bin launch is
 * through.  Results are bit-identical to the plain sequence.  ERASOR_HIP_OVERLAP=0 / =1: never / always (unset: the handle decides). */
int erasor_hip_announce_origin2body(erasor_hip_handle *h, const float T_origin2body[16]);
/* steps whose early passes were launched ahead like that / steps that took them */
int erasor_hip_overlap_counts(erasor_hip_handle *h, uint64_t *launched, uint64_t *used);
/* ERASOR_HIP_OVERLAP unset: the handle decides by measurement whether consecutive steps overlap: the period of a step on the device's
 * clock, four samples plain, then four overlapped.  If the two means (each without its largest sample) differ by more than a margin the
 * decision is taken there, after a fresh handle's 16th step; otherwise a second overlapped and a second
 * plain block follow and the shorter mean wins (plain has to lose by 2 %; after the 27th step).  Measured again every 600 steps.  *mode: 1 overlapped,
 * 0 plain -- what the next step will use; the two periods the last decision compared, in microseconds (0: not measured yet). */
int erasor_hip_overlap_auto(erasor_hip_handle *h, int *mode, double *plain_period_us, double *overlapped_period_us);
/* What a handle's steps cost beside their kernels: one record per COLLECTED step, the last 256 are kept. */
typedef struct erasor_step_log_entry {
    uint64_t step;        /* the step's number (1: the handle's first) */
    double period_us;     /* end of the previous step to the end of this one on the device's clock -- the value the overlap decision
                             samples --, 0 when the two were not consecutive */
    uint32_t n_alloc;     /* device (and pinned host) allocations, frees, stream / event creations made inside this step's calls and */
    uint32_t n_free;      /* in the announcements since the previous step was collected */
    uint32_t n_create;
    uint8_t reserved;     /* the step wrote the reserved layout (an overlapped step) */
    uint8_t use_ov;       /* it took the passes launched ahead of it beside the previous step's per-bin launch */
    uint8_t deep;         /* the caller had announced deep enough for the overlap decision to sample it */
    uint8_t sampled;      /* the period was counted by the overlap decision (not skipped, not between two measurements) */
    uint8_t ova_mode;     /* the overlap decision's state BEFORE this step's sample: the mode in force, */
    uint8_t ova_block;    /* the block being sampled (0..3: plain, overlapped, overlapped, plain; 4: decided) */
    uint8_t ova_skip;     /* and the samples still to be ignored */
    uint8_t grown;        /* growth the map's own growth forced inside the step: 1 the map-sized scratch was enlarged, 2 the outskirts were
                             rebuilt (a pass over the store), 3 both */
} erasor_step_log_entry;
/* the last records, oldest first: up to `cap` of them into out[], *n = how many were written */
int erasor_hip_step_log(erasor_hip_handle *h, erasor_step_log_entry *out, size_t cap, size_t *n);
/* Where the handle's streams landed.  A handle with two query streams sees, when it is created, which compute pipe its main stream and
 * its two query streams run on, and steers the early stream of overlapped steps -- created at the first deep step -- onto a pipe none
 * of them has: candidate streams are created one at a time (four at most); one that shares a pipe stays alive as an idle pad, the first
 * one on a free pipe holds the place and is destroyed right in front of the early stream's creation, which lands where it was.  pipes[]: main, q0, q1, early, each me * 4 + pipe of the
 * hardware's HW_ID, -1 for unknown or not created; *n_pads: pads kept; *distinct_seen: different pipes seen in all (the three streams'
 * and every candidate's).  Handles with one or three query streams, ERASOR_HIP_OVERLAP=0 and ERASOR_HIP_NO_PLACEMENT=1: nothing is
 * probed, every pipe is -1.  Results never depend on any of it. */
int erasor_hip_stream_pipes(erasor_hip_handle *h, int pipes[4], int *n_pads, int *distinct_seen);
/* Round 6 -- the query chains of SEVERAL announced nodes as one set of launches.  A node's query chain (voxelize_preserving_labels of
 * its scan, OfflineMapUpdater.cpp:237-241; lidar->body, R-POD keys, per-bin statistics, erasor.cpp:100-115) does not depend on the map,
 * and every launch of it is bound by latency, not by work: a launch that serves the same stage of n_scans scans costs what it costs for
 * one.  With n_scans >= 2 the chain of an announced node is held back until n_scans of them can share their launches -- unless fewer
 * than `lead` chains are in their queues in front of it (or its own step is fewer than `lead` steps away): then it goes off at once, alone.
 * An offline driver that knows its nodes ahead (main_in_your_env.cpp:92-123; erasor_hip_run_nodes with lookahead >= lead + n_scans) gets
 * the shared launches; a callback that can announce one node ahead (OfflineMapUpdater.cpp:203) never holds anything back.
 * n_scans: 1 .. 4 (1: every chain on its own; the default is 2), lead: 1 .. 6 (default 3).  Results do not depend on either. */
int erasor_hip_chain_batch(erasor_hip_handle *h, int n_scans, int lead);
/* Forget every node that is announced and not yet stepped (their chains run out, passes launched ahead of them are discarded): what a
 * step does by itself when it meets a scan that is not the oldest announced one (erasor_hip_prefetch_scan), as a call of its own -- for a
 * caller that lost track of its announcements (the shim's OfflineMapUpdater: a callback without a ticket while several nodes are
 * announced by ticket, OfflineMapUpdater.cpp:203 has no notion of either). */
int erasor_hip_drop_announced(erasor_hip_handle *h);
/* How many nodes are announced and not yet stepped or dropped.  A step WITHOUT a ticket may consume the oldest announcement (its scan,
 * recognised by pointer, size and content), keep the one announcement that has not started (another scan: the next one) or drop them all:
 * a caller that keeps books of its tickets asks here which of the three it was.  Reads host state only; any time, also with a step in
 * flight. */
int erasor_hip_announced_count(const erasor_hip_handle *h, int *n);
/* sets of shared launches made so far / chains that went into them */
int erasor_hip_chain_batch_counts(erasor_hip_handle *h, uint64_t *sets, uint64_t *chains);
/* The main stream's dependency chain on the device's own clock (no events, no extra launches: the chunk scan and the step's end stamp
 * the 100 MHz counter): average span of a step from its chunk scan to its end (when the scan is launched ahead, behind the next VoI
 * split, that span contains the stream's wait for the host), average time between a step's end and the next step's chunk scan (the
 * VoI split launched ahead runs in there), and the PERIOD: chunk scan to chunk scan of consecutive steps -- the steady-state time per
 * scan of a sequence.  reset != 0 clears the sums. */
int erasor_hip_chain_timing(erasor_hip_handle *h, double *main_chain_us, double *between_steps_us, double *period_us, uint64_t *steps, int reset);
/* the hipStream_t the handle launches on (as void*) */
void *erasor_hip_stream(erasor_hip_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* ERASOR_HIP_H */
