"""Preservation Rate / Rejection Rate of a static map against a labelled ground-truth map.

Same protocol as the reference's evaluator (scripts/analysis_runner.py:74-105; README.md:196): for every GT point the
nearest estimated point (1-NN, Euclidean); a GT point is "preserved" if that distance is < voxelsize*sqrt(3)/2;
PR = preserved static / GT static, RR = 1 - preserved dynamic / GT dynamic (both in %), F1 of PR/100 and RR/100.
Labels: numeric cast of intensity, & 0xFFFF, dynamic classes 252..259 (analysis_runner.py:14,44-47).
Pinned against the reference implementation by tests/golden/eval_golden.npz (tests/golden/make_eval_golden.py).

overlap / overlap_lines: the estimate-to-GT distance report printed before the PR / RR row (analysis_runner.py:53-71,
overlap_report), pinned by tests/golden/overlap_golden.npz (tests/golden/make_overlap_golden.py).

nearest_f32 / label_from / static_complement: the 1-NN of pcl::KdTreeFLANN (float32 d^2, lowest index on ties) behind the
reference's label_map (src/utils/fill_removert_intensity.cpp:24-59) and calc_complement (src/utils/compare_complement.cpp:43-75).

align_frames: overlap() of every frame's scan, put into the map frame by its pose, against the map (Erasor.align_frames).

refine_poses: every frame's pose refined against the map by point-to-point ICP, every sum in one defined order (Erasor.refine_poses).

label_scans / moving_iou: every scan's points labelled static / dynamic / unknown from a cleaned map, against the scan's own labels
(Erasor.label_scans).

evaluate_by_class: the same decision per GT point, counted per semantic class and per dynamic instance (Erasor.evaluate_by_class).

cluster / cluster_brute: Euclidean clustering of a cloud, the host restatement of Erasor.cluster (include/erasor_hip.h,
erasor_cluster_row): connected components of "within tol", listed and filtered by size, with counts and boxes.

knn / radius_count / density_filter (and knn_brute, radius_count_brute): every point's k nearest neighbours inside its own cloud, the
points within a radius of it, and the outlier filters on both -- the host restatement of Erasor.knn / radius_count / density_filter.

normals / normals_brute: every point's surface normal, curvature and covariance eigenvalues from its k nearest neighbours -- the host
restatement of Erasor.normals.

visibility / visibility_brute (and visibility_grid, visibility_column, visibility_transforms, visibility_decide): the see-through check,
map points voted out by every scan's range image -- the normative text of Erasor.visibility.

carve / carve_brute (and carve_walk, carve_logodds): free space carved out of a map, every scan's rays walked through the map's voxels and
the voxels' clamped log-odds integrated, OctoMap's way -- the normative text of Erasor.carve.
"""
import numpy as np
from scipy.spatial import cKDTree

DYNAMIC_CLASSES = np.arange(252, 260)


def labels(intensity):
    return np.asarray(intensity).astype(np.uint32) & 0xFFFF


def evaluate(gt_xyz, gt_sem, est_xyz, est_sem, voxelsize=0.2):
    gt_xyz = np.asarray(gt_xyz, np.float32)
    est_xyz = np.asarray(est_xyz, np.float32)
    gt_dyn_all = np.isin(gt_sem, DYNAMIC_CLASSES)
    ns_gt, nd_gt = int((~gt_dyn_all).sum()), int(gt_dyn_all.sum())
    est_dyn_all = np.isin(est_sem, DYNAMIC_CLASSES)
    # (workers=-1: the query runs on every host core -- the result does not depend on it; a 10 M-point map takes seconds instead of a minute)
    dists, idx = cKDTree(est_xyz.astype(np.float64)).query(gt_xyz.astype(np.float64), k=1, workers=-1)
    is_in = dists < voxelsize * np.sqrt(3) / 2
    gt_is_dyn = gt_dyn_all[is_in]
    est_is_dyn = est_dyn_all[idx[is_in]]
    kept_s = int(np.sum((~gt_is_dyn) & (~est_is_dyn)))
    kept_d = int(np.sum(gt_is_dyn & est_is_dyn))
    pr = kept_s / ns_gt * 100.0
    rr = (nd_gt - kept_d) / nd_gt * 100.0 if nd_gt > 0 else 0.0
    f1 = 2 * (pr / 100) * (rr / 100) / ((pr / 100) + (rr / 100)) if (pr + rr) > 0 else 0.0
    return {"gt_static": ns_gt, "gt_dynamic": nd_gt, "est_static": int((~est_dyn_all).sum()), "est_dynamic": int(est_dyn_all.sum()),
            "preserved_static": kept_s, "preserved_dynamic": kept_d, "PR": pr, "RR": rr, "F1": f1}


def evaluate_clouds(gt_xyzi, est_xyzi, voxelsize=0.2):
    gt = np.asarray(gt_xyzi, np.float32).reshape(-1, 4)
    est = np.asarray(est_xyzi, np.float32).reshape(-1, 4)
    return evaluate(gt[:, :3], labels(gt[:, 3]), est[:, :3], labels(est[:, 3]), voxelsize)


def overlap(gt_xyz, est_xyz, voxelsize=0.2):
    """overlap_report's numbers: the distance of every estimated point to its nearest GT point (the reference fits
    NearestNeighbors(kd_tree) on the GT; cKDTree gives the same float64 distances), then numpy's median / percentiles / max
    and the percentages below 0.5*v, v and 2*v, with the thresholds formed as the reference forms them"""
    gt_xyz = np.asarray(gt_xyz, np.float32).reshape(-1, 3)
    est_xyz = np.asarray(est_xyz, np.float32).reshape(-1, 3)
    half = 0.5 * voxelsize
    one = voxelsize
    if len(est_xyz) == 0:
        nan = float("nan")
        return {"n_est": 0, "n_below_half": 0, "n_below_one": 0, "n_below_two": 0, "median": nan, "p90": nan, "p99": nan, "max": nan,
                "frac_half": nan, "frac_one": nan, "frac_two": nan}
    d, _ = cKDTree(gt_xyz.astype(np.float64)).query(est_xyz.astype(np.float64), k=1, workers=-1)
    d = d.reshape(-1)
    return {"n_est": int(len(d)), "n_below_half": int(np.sum(d < half)), "n_below_one": int(np.sum(d < one)),
            "n_below_two": int(np.sum(d < 2 * one)), "median": float(np.median(d)), "p90": float(np.percentile(d, 90)),
            "p99": float(np.percentile(d, 99)), "max": float(d.max()), "frac_half": float(np.mean(d < half) * 100),
            "frac_one": float(np.mean(d < one) * 100), "frac_two": float(np.mean(d < 2 * one) * 100)}


def overlap_lines(r, voxelsize=0.2):
    """the two lines overlap_report prints, from overlap()'s (or Erasor.overlap's) dict"""
    half = 0.5 * voxelsize
    one = voxelsize
    return [f"est->GT dist: median={r['median']:.4f}m  p90={r['p90']:.4f}m  p99={r['p99']:.4f}m  max={r['max']:.4f}m",
            f"  fraction <0.5*v ({half:.2f}m): {r['frac_half']:.2f}%  <1*v ({one:.2f}m): {r['frac_one']:.2f}%  "
            f"<2*v ({2*one:.2f}m): {r['frac_two']:.2f}%"]


def _xform(T, xyz):
    """pcl::transformPointCloud in float32, operation by operation: ((a*x + b*y) + c*z) + d per output coordinate"""
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def align_frames(map_xyz, scans, T_body2origin, T_lidar2body=None, voxelsize=0.2):
    """Every frame's pose checked against the map (the reference README's pitfalls 1, 3 and 5): scan f as given, put into the map frame
    as the reference puts its RViz query, body2origin(tf_lidar2body · scan) -- T_lidar2body (the identity when None, still applied),
    then T_body2origin[f], in float32 --, points with a non-finite coordinate afterwards dropped and counted, and overlap() of the rest
    against the map.  Returns (rows, summary): a row per frame with overlap()'s keys plus n_points / n_non_finite, and overlap() of all
    frames' kept points together."""
    map_xyz = np.asarray(map_xyz, np.float32).reshape(-1, 3)
    Tl = np.eye(4, dtype=np.float32) if T_lidar2body is None else T_lidar2body
    rows, kept = [], []
    for f, scan in enumerate(scans):
        xyz = np.asarray(scan, np.float32).reshape(len(scan), 4)[:, :3]
        with np.errstate(over="ignore", invalid="ignore"):
            q = _xform(T_body2origin[f], _xform(Tl, xyz))
        ok = np.isfinite(q).all(1)
        kept.append(q[ok])
        r = overlap(map_xyz, q[ok], voxelsize)
        r.update(n_points=int(len(xyz)), n_non_finite=int((~ok).sum()))
        rows.append(r)
    allk = np.concatenate(kept) if kept else np.zeros((0, 3), np.float32)
    return rows, overlap(map_xyz, allk, voxelsize)


LABEL_STATIC, LABEL_DYNAMIC, LABEL_UNKNOWN, LABEL_DROPPED = 0, 1, 2, 255


def label_tau(voxelsize=0.2):
    """label_scans' default threshold: evaluate's, voxelsize * np.sqrt(3) / 2, formed as evaluate forms it"""
    return float(voxelsize * np.sqrt(3) / 2)


def label_bound(tau):
    """the largest float64 whose sqrt is < tau: d < tau <=> d^2 <= label_bound(tau) for d = sqrt(d^2) (what the device tests)"""
    tau = np.float64(tau)
    with np.errstate(over="ignore", under="ignore"):
        x = tau * tau
    while x > 0 and not np.sqrt(x) < tau:
        x = np.nextafter(x, 0.0)
    while True:
        y = np.nextafter(x, np.inf)
        if not y < np.inf or not np.sqrt(y) < tau:
            return float(x)
        x = y


def _nearest_dist(map_xyz, q):
    """the float64 distance of every row of q to its nearest map point, as cKDTree returns it (+inf against an empty map)"""
    if len(map_xyz) == 0 or len(q) == 0:
        return np.full(len(q), np.inf)
    d, _ = cKDTree(map_xyz.astype(np.float64)).query(q.astype(np.float64), k=1, workers=-1)
    return d.reshape(-1)


def label_scans(static_xyz, scans, T_body2origin, T_lidar2body=None, raw_xyz=None, tau=None, voxelsize=0.2, split=None):
    """Every point of every scan classified against a cleaned (static) map and, optionally, the raw map.  Scan f is put into the map
    frame as align_frames puts it.  Per point: 255 dropped (a non-finite coordinate after the transforms); else 0 static when its distance
    to the nearest static-map point is < tau; else 1 dynamic when no raw map was given or its distance to the nearest raw-map point is
    < tau; else 2 unknown.  tau: voxelsize * np.sqrt(3) / 2 when None.  The scan's own label: moving when labels(intensity) is in
    DYNAMIC_CLASSES; intensities outside [0, 2^32) (or not finite) count as static and are counted, over the kept points.
    Returns (codes, rows, summary): a uint8 array per frame; per frame {"n_points", "n_non_finite", "n_label_out_of_range", "n"} with
    n[gt moving][code] a 2 x 3 list; and the sum of the rows.  split (0, 1 or 2): also the rows of that code, as given, per frame."""
    static_xyz = np.asarray(static_xyz, np.float32).reshape(-1, 3)
    raw = None if raw_xyz is None else np.asarray(raw_xyz, np.float32).reshape(-1, 3)
    tau = label_tau(voxelsize) if tau is None else float(tau)
    if not (tau > 0 and np.isfinite(tau)):
        raise ValueError("tau must be a finite number > 0")
    if split is not None and (split not in (0, 1, 2) or (split == 2 and raw is None)):
        raise ValueError("split must be 0, 1 or 2 (2 only with a raw map)")
    Tl = np.eye(4, dtype=np.float32) if T_lidar2body is None else T_lidar2body
    codes, rows, clouds = [], [], []
    total = {"n_points": 0, "n_non_finite": 0, "n_label_out_of_range": 0, "n": [[0, 0, 0], [0, 0, 0]]}
    for f, scan in enumerate(scans):
        s = np.ascontiguousarray(scan, np.float32).reshape(len(scan), 4)
        with np.errstate(over="ignore", invalid="ignore"):
            q = _xform(T_body2origin[f], _xform(Tl, s[:, :3]))
        ok = np.isfinite(q).all(1)
        code = np.full(len(s), LABEL_DROPPED, np.uint8)
        c = np.full(int(ok.sum()), LABEL_DYNAMIC, np.uint8)
        not_static = ~(_nearest_dist(static_xyz, q[ok]) < tau)
        c[~not_static] = LABEL_STATIC
        if raw is not None:
            far = ~(_nearest_dist(raw, q[ok][not_static]) < tau)
            c[np.flatnonzero(not_static)[far]] = LABEL_UNKNOWN
        code[ok] = c
        w = s[ok, 3]
        in_range = (w >= 0) & (w < 4294967296.0)  # (NaN fails both)
        moving = np.zeros(len(w), bool)
        moving[in_range] = np.isin(labels(w[in_range]), DYNAMIC_CLASSES)
        r = {"n_points": int(len(s)), "n_non_finite": int((~ok).sum()), "n_label_out_of_range": int((~in_range).sum()),
             "n": [[int(np.sum((moving == bool(g)) & (c == k))) for k in range(3)] for g in range(2)]}
        for k in ("n_points", "n_non_finite", "n_label_out_of_range"):
            total[k] += r[k]
        for g in range(2):
            for k in range(3):
                total["n"][g][k] += r["n"][g][k]
        codes.append(code)
        rows.append(r)
        if split is not None:
            clouds.append(s[code == split].copy())
    return (codes, rows, total) if split is None else (codes, rows, total, clouds)


def moving_iou(summary):
    """moving-object segmentation scores of a label_scans summary (or row), in float64: TP = n[1][1], FP = n[0][1], FN = n[1][0] + n[1][2];
    IoU = TP / (TP + FP + FN), precision = TP / (TP + FP), recall = TP / (TP + FN); NaN where a denominator is 0"""
    n = summary["n"]
    tp, fp, fn = int(n[1][1]), int(n[0][1]), int(n[1][0]) + int(n[1][2])

    def ratio(a, b):
        return float(a) / float(b) if b else float("nan")

    return {"TP": tp, "FP": fp, "FN": fn, "IoU": ratio(tp, tp + fp + fn), "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn)}


# ---- refine_poses: every frame's pose refined against the map by point-to-point ICP (Erasor.refine_poses, refine.hip.h) ----
REFINE_CONVERGED, REFINE_MAX_ITERS, REFINE_FEW_PAIRS, REFINE_NO_POINTS = 0, 1, 2, 3  # ERASOR_REFINE_*
REFINE_CHUNK = 256   # RF_CHUNK: the sums' chunks, counted from each frame's own first point
REFINE_NSUM = 16     # RF_NSUM: sum q' (3), sum m' (3), sum q' m't row-major (9), sum d2
REFINE_ROW_FIELDS = ("status", "iters", "n_points", "n_non_finite", "n_pairs_first", "n_pairs_last", "rms_first", "rms_last", "moved_t", "moved_r")
REFINE_SUMMARY_FIELDS = ("n_frames", "n_status", "n_pairs_first", "n_pairs_last", "sum_d2_first", "sum_d2_last")


def _ieee_div(a, b):
    """a / b on Python floats as IEEE 754 defines it where Python raises (b == 0)"""
    import math
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def nearest_f64(map64, tree, q):
    """the exact float64 1-NN of every row of q (finite) in map64 (its cKDTree: `tree`): (d2, j) with d2 by pair_d2 and the lowest index
    among the points at the minimum.  The tree only proposes candidates; a row whose last candidate is not strictly beyond its best is
    redone over every map point."""
    n, nm = len(q), len(map64)
    if n == 0:
        return np.zeros(0), np.zeros(0, np.int64)
    kk = min(10, nm)
    dist, cand = tree.query(q, k=kk, workers=-1)
    dist, cand = dist.reshape(n, kk), cand.reshape(n, kk).astype(np.int64)
    d2 = pair_d2(q[:, None, :], map64[cand])
    by_j = np.argsort(cand, axis=1, kind="stable")
    cand, d2 = np.take_along_axis(cand, by_j, 1), np.take_along_axis(d2, by_j, 1)
    by_d = np.argsort(d2, axis=1, kind="stable")
    best_j, best = np.take_along_axis(cand, by_d, 1)[:, 0].copy(), np.take_along_axis(d2, by_d, 1)[:, 0].copy()
    if kk < nm:  # (the tree's own distances are a few ulps off the predicate's: 1e-9 relative is far above that)
        redo = np.flatnonzero(~(best < dist[:, -1] * dist[:, -1] * (1 - 1e-9)))
        for lo in range(0, len(redo), 256):
            r = redo[lo:lo + 256]
            full = pair_d2(q[r, None, :], map64[None, :, :])
            j = np.argmin(full, axis=1)  # (the first of equal minima: the lowest index)
            best_j[r], best[r] = j, full[np.arange(len(r)), j]
    return best, best_j


def refine_tree_sum(v):
    """the defined sum of one frame's per-point rows v (n, k), in scan order: chunks of 256 from the frame's first point, padded with +0.0;
    inside a chunk the halving tree v[i] += v[i + s] for s = 128 .. 1; the chunks' partials one after another from 0.0.  Returns (k,)"""
    n, k = v.shape
    nc = -(-n // REFINE_CHUNK)
    pad = np.zeros((nc * REFINE_CHUNK, k))
    pad[:n] = v
    c = pad.reshape(nc, REFINE_CHUNK, k)
    s = REFINE_CHUNK // 2
    while s >= 1:
        c = c[:, :s] + c[:, s:2 * s]
        s //= 2
    total = np.zeros(k)
    for b in range(nc):
        total = total + c[b, 0]
    return total


def _jacobi4(A):
    """cyclic Jacobi on the symmetric 4x4 A (lists of Python floats, changed in place): pivots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
    until every element above the diagonal is exactly zero before a sweep, or 32 sweeps.  Returns V (columns: eigenvectors)"""
    from math import sqrt
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(32):
        if A[0][1] == 0.0 and A[0][2] == 0.0 and A[0][3] == 0.0 and A[1][2] == 0.0 and A[1][3] == 0.0 and A[2][3] == 0.0:
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = _ieee_div(A[q][q] - A[p][p], 2.0 * apq)
                at = -theta if theta < 0.0 else theta
                t = _ieee_div(1.0, at + sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = _ieee_div(1.0, sqrt(t * t + 1.0))
                s = t * c
                for k in range(4):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(4):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                A[p][q] = 0.0
                for i in range(4):
                    for j in range(i + 1, 4):
                        A[j][i] = A[i][j]
                for k in range(4):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return V


def refine_solve(S, n, R, t):
    """one frame's update from its sums S (16 Python floats) over n >= 1 pairs: Horn's quaternion from the centred cross-covariance by
    _jacobi4, R <- dR R, t <- t + delta.  R: 9 floats row-major, t: 3.  Returns (R, t, |delta|, 2 |q_xyz|)"""
    from math import sqrt
    nn = float(n)
    mq = [S[a] / nn for a in range(3)]
    mm = [S[3 + a] / nn for a in range(3)]
    H = [[S[6 + 3 * a + b] - (S[a] * S[3 + b]) / nn for b in range(3)] for a in range(3)]
    N = [[0.0] * 4 for _ in range(4)]
    N[0][0] = (H[0][0] + H[1][1]) + H[2][2]
    N[0][1] = H[1][2] - H[2][1]
    N[0][2] = H[2][0] - H[0][2]
    N[0][3] = H[0][1] - H[1][0]
    N[1][1] = (H[0][0] - H[1][1]) - H[2][2]
    N[1][2] = H[0][1] + H[1][0]
    N[1][3] = H[2][0] + H[0][2]
    N[2][2] = (H[1][1] - H[0][0]) - H[2][2]
    N[2][3] = H[1][2] + H[2][1]
    N[3][3] = (H[2][2] - H[0][0]) - H[1][1]
    for i in range(4):
        for j in range(i + 1, 4):
            N[j][i] = N[i][j]
    V = _jacobi4(N)
    k = 0
    for i in range(1, 4):
        if N[i][i] > N[k][k]:
            k = i
    w, x, y, z = V[0][k], V[1][k], V[2][k], V[3][k]
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    nrm = sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = _ieee_div(w, nrm), _ieee_div(x, nrm), _ieee_div(y, nrm), _ieee_div(z, nrm)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    D = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    d = [mm[a] - ((D[a][0] * mq[0] + D[a][1] * mq[1]) + D[a][2] * mq[2]) for a in range(3)]
    Rn = [(D[a][0] * R[b] + D[a][1] * R[3 + b]) + D[a][2] * R[6 + b] for a in range(3) for b in range(3)]
    tn = [t[a] + d[a] for a in range(3)]
    return Rn, tn, sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), 2.0 * sqrt((xx + yy) + zz)


def refine_frame_sums(map64, tree, p32, R, t, gate2, nearest=nearest_f64):
    """one frame's sums under the pose (R, t): p32 the body points (float32, T_lidar2body applied).  Returns (S (16,), pairs, points
    without a query).  q' = R p and q = q' + t in float64, rows as ((a*x + b*y) + c*z); the pairs: d2 <= gate2; m' = map[j] - t"""
    n = len(p32)
    p = p32.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.stack([(R[3 * a] * p[:, 0] + R[3 * a + 1] * p[:, 1]) + R[3 * a + 2] * p[:, 2] for a in range(3)], 1)
        q = r + np.asarray(t, np.float64)[None, :]
    ok = np.isfinite(p32).all(1) & np.isfinite(q).all(1)
    v = np.zeros((n, REFINE_NSUM))
    pairs = 0
    if ok.any():
        d2, j = nearest(map64, tree, q[ok])
        inl = d2 <= gate2
        rows = np.flatnonzero(ok)[inl]
        rr = r[rows]
        m = map64[j[inl]] - np.asarray(t, np.float64)[None, :]
        v[rows, 0:3] = rr
        v[rows, 3:6] = m
        for a in range(3):
            for b in range(3):
                v[rows, 6 + 3 * a + b] = rr[:, a] * m[:, b]
        v[rows, 15] = d2[inl]
        pairs = int(inl.sum())
    return refine_tree_sum(v), pairs, int((~ok).sum())


def refine_poses(map_xyz, scans, T_body2origin, T_lidar2body=None, max_dist=1.0, eps_t=1e-4, eps_r=1e-5, max_iters=20, min_pairs=100,
                 nearest=nearest_f64):
    """Every frame's T_body2origin refined against the map by point-to-point ICP with a fixed gate: the host restatement of
    Erasor.refine_poses (include/erasor_hip.h, erasor_refine_row), operation for operation.  Per frame: p = T_lidar2body · scan row in
    float32 (the identity when None, still applied); the pose (R, t) in float64 from the float32 T_body2origin[f]; per iteration
    refine_frame_sums and refine_solve, until the update is <= eps_t and <= eps_r (status 0) or max_iters updates (1); a frame with fewer
    than max(min_pairs, 1) pairs keeps its pose (2; 3 when no point has finite coordinates under the input pose).  Returns
    (T float64 [n, 4, 4], rows, summary): REFINE_ROW_FIELDS per frame, REFINE_SUMMARY_FIELDS."""
    import math
    if not (1 <= int(max_iters) <= 64):
        raise ValueError("refine_poses: max_iters must be 1 .. 64")
    for name, val in (("max_dist", max_dist), ("eps_t", eps_t), ("eps_r", eps_r)):
        if not (np.isfinite(val) and val > 0):
            raise ValueError("refine_poses: %s must be a finite number > 0" % name)
    map32 = np.asarray(map_xyz, np.float32).reshape(-1, 3)
    map64 = map32.astype(np.float64)
    tree = cKDTree(map64) if len(map64) else None
    if tree is None and any(len(s) for s in scans):
        raise ValueError("refine_poses: empty map with a non-empty frame (no nearest point to match)")
    Tl = np.eye(4, dtype=np.float32) if T_lidar2body is None else T_lidar2body
    gate2 = float(max_dist) * float(max_dist)
    need = max(int(min_pairs), 1)
    nan = float("nan")
    n_f = len(scans)
    T_out = np.zeros((n_f, 4, 4))
    rows = []
    summary = {"n_frames": n_f, "n_status": [0, 0, 0, 0], "n_pairs_first": 0, "n_pairs_last": 0, "sum_d2_first": 0.0, "sum_d2_last": 0.0}
    for f, scan in enumerate(scans):  # (the frames do not interact: one after the other here, side by side on the device)
        xyz = np.asarray(scan, np.float32).reshape(len(scan), 4)[:, :3]
        with np.errstate(over="ignore", invalid="ignore"):
            p32 = _xform(Tl, xyz)
        T0 = np.asarray(T_body2origin[f], np.float32).reshape(4, 4)
        R0 = [float(T0[a, b]) for a in range(3) for b in range(3)]
        t0 = [float(T0[a, 3]) for a in range(3)]
        R, t = list(R0), list(t0)
        status, iters = REFINE_MAX_ITERS, 0
        pairs_first, d2_first, bad_first = 0, 0.0, 0
        for it in range(1, int(max_iters) + 1):
            S, pairs, bad = refine_frame_sums(map64, tree, p32, R, t, gate2, nearest)
            if it == 1:
                pairs_first, d2_first, bad_first = pairs, float(S[15]), bad
            if pairs < need:
                status = REFINE_NO_POINTS if bad_first == len(xyz) else REFINE_FEW_PAIRS
                break
            R, t, st, sr = refine_solve([float(s) for s in S], pairs, R, t)
            iters = it
            if st <= eps_t and sr <= eps_r:
                status = REFINE_CONVERGED
                break
        S, pairs_last, _ = refine_frame_sums(map64, tree, p32, R, t, gate2, nearest)
        d2_last = float(S[15])
        for a in range(3):
            T_out[f, a, :3] = R[3 * a:3 * a + 3]
            T_out[f, a, 3] = t[a]
        T_out[f, 3, 3] = 1.0
        dx, dy, dz = t[0] - t0[0], t[1] - t0[1], t[2] - t0[2]
        tr = 0.0
        for a in range(3):
            tr = tr + ((R[3 * a] * R0[3 * a] + R[3 * a + 1] * R0[3 * a + 1]) + R[3 * a + 2] * R0[3 * a + 2])
        cs = (tr - 1.0) / 2.0
        if cs > 1.0:
            cs = 1.0
        if cs < -1.0:
            cs = -1.0
        rows.append({"status": status, "iters": iters, "n_points": int(len(xyz)), "n_non_finite": bad_first, "n_pairs_first": pairs_first,
                     "n_pairs_last": pairs_last, "rms_first": math.sqrt(d2_first / float(pairs_first)) if pairs_first else nan,
                     "rms_last": math.sqrt(d2_last / float(pairs_last)) if pairs_last else nan,
                     "moved_t": math.sqrt((dx * dx + dy * dy) + dz * dz), "moved_r": math.acos(cs)})
        summary["n_status"][status] += 1
        summary["n_pairs_first"] += pairs_first
        summary["n_pairs_last"] += pairs_last
        summary["sum_d2_first"] = summary["sum_d2_first"] + d2_first
        summary["sum_d2_last"] = summary["sum_d2_last"] + d2_last
    return T_out, rows, summary


# ---- refine_poses_plane: every frame's pose refined point-to-plane against the map's normals (Erasor.refine_poses_plane,
# refine_plane.hip.h).  The map's normals and curvature are normals(map, k) with no viewpoint; a scan point within the gate of a map point
# with a finite normal and a curvature <= max_curvature is a pair with the residual r = n . (q - m) and the row J = (q' x n, n); the 29
# sums are refine_tree_sum's; the 6x6 normal equations are solved by _jacobi6 and a pseudo-inverse over the directions above rank_tol.
REFINE_DEGENERATE = 4  # ERASOR_REFINE_DEGENERATE: no direction of the normal equations above rank_tol (the pose is kept)
REFINE_PLANE_NSUM = 29  # RFP_NSUM: J[a]*J[b] for a <= b row-major (0..20), J[a]*r (21..26), r*r (27), d2 (28)
REFINE_PLANE_ROW_FIELDS = REFINE_ROW_FIELDS + ("rank", "lambda_ratio", "n_unusable_first", "n_unusable_last", "rms_plane_first", "rms_plane_last")
REFINE_PLANE_SUMMARY_FIELDS = REFINE_SUMMARY_FIELDS + ("sum_r2_first", "sum_r2_last", "n_map_no_normal")


def _jacobi6(A):
    """_jacobi4 on a symmetric 6x6 (lists of Python floats, changed in place): the pivots (p, q), p < q, row-major, the same rotation, a
    pivot that is exactly zero skipped, until every element above the diagonal is exactly zero before a sweep, or 32 sweeps.  Returns V
    (columns: eigenvectors); the eigenvalues are A's diagonal"""
    from math import sqrt
    V = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    for _ in range(32):
        if all(A[i][j] == 0.0 for i in range(5) for j in range(i + 1, 6)):
            break
        for p in range(5):
            for q in range(p + 1, 6):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = _ieee_div(A[q][q] - A[p][p], 2.0 * apq)
                at = -theta if theta < 0.0 else theta
                t = _ieee_div(1.0, at + sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = _ieee_div(1.0, sqrt(t * t + 1.0))
                s = t * c
                for k in range(6):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(6):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                A[p][q] = 0.0
                for i in range(6):
                    for j in range(i + 1, 6):
                        A[j][i] = A[i][j]
                for k in range(6):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return V


def refine_plane_solve(S, R, t, rank_tol):
    """one frame's update from its sums S (29 Python floats): A from S[0..20], b = -S[21..26], _jacobi6, the pseudo-inverse over the
    directions i with lambda_i > rank_tol * lambda_max (lambda_max > 0) in index order, the rotation from the half vector without
    trigonometry, R <- D R, t <- t + x[3..5].  rank 0: (R, t) as given and steps of 0.0.  Returns (R, t, |x[3..5]|, 2 |q_xyz|, rank,
    lambda_ratio)"""
    from math import sqrt
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = S[k]
            k += 1
    bb = [-S[21 + a] for a in range(6)]
    V = _jacobi6(A)
    lam = [A[i][i] for i in range(6)]
    lmax = lmin = lam[0]
    for i in range(1, 6):
        if lam[i] > lmax:
            lmax = lam[i]
        if lam[i] < lmin:
            lmin = lam[i]
    ratio = lmin / lmax if lmax > 0 else float("nan")
    x = [0.0] * 6
    rank = 0
    for i in range(6):
        if not (lmax > 0 and lam[i] > rank_tol * lmax):
            continue
        rank += 1
        g = (((((V[0][i] * bb[0] + V[1][i] * bb[1]) + V[2][i] * bb[2]) + V[3][i] * bb[3]) + V[4][i] * bb[4]) + V[5][i] * bb[5]) / lam[i]
        for a in range(6):
            x[a] = x[a] + V[a][i] * g
    if rank == 0:
        return list(R), list(t), 0.0, 0.0, 0, ratio
    hx, hy, hz = 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]
    w = 1.0 / sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    qx, qy, qz = hx * w, hy * w, hz * w
    xx, yy, zz, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, w * qx, w * qy, w * qz
    D = [[1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]]
    Rn = [(D[a][0] * R[b] + D[a][1] * R[3 + b]) + D[a][2] * R[6 + b] for a in range(3) for b in range(3)]
    tn = [t[a] + x[3 + a] for a in range(3)]
    return Rn, tn, sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]), 2.0 * sqrt((xx + yy) + zz), rank, ratio


def refine_plane_frame_sums(map64, tree, nrm32, curv, p32, R, t, gate2, max_curvature, nearest=nearest_f64):
    """one frame's sums under the pose (R, t): p32 the body points (float32, T_lidar2body applied), nrm32 / curv the map's normals and
    curvature.  Returns (S (29,), pairs, points without a query, unusable candidates).  A candidate: d2 <= gate2; a pair: a candidate
    whose map point has three finite normal components and a curvature <= max_curvature"""
    n = len(p32)
    p = p32.astype(np.float64)
    tt = np.asarray(t, np.float64)[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        qr = np.stack([(R[3 * a] * p[:, 0] + R[3 * a + 1] * p[:, 1]) + R[3 * a + 2] * p[:, 2] for a in range(3)], 1)
        q = qr + tt
    ok = np.isfinite(p32).all(1) & np.isfinite(q).all(1)
    v = np.zeros((n, REFINE_PLANE_NSUM))
    pairs = unusable = 0
    if ok.any():
        d2, j = nearest(map64, tree, q[ok])
        cand = d2 <= gate2
        with np.errstate(invalid="ignore"):
            use = cand & np.isfinite(nrm32[j]).all(1) & (curv[j] <= max_curvature)
        rows = np.flatnonzero(ok)[use]
        ju = j[use]
        nn = nrm32[ju].astype(np.float64)
        e = q[rows] - map64[ju]
        qq = qr[rows]
        r = (e[:, 0] * nn[:, 0] + e[:, 1] * nn[:, 1]) + e[:, 2] * nn[:, 2]
        J = [qq[:, 1] * nn[:, 2] - qq[:, 2] * nn[:, 1], qq[:, 2] * nn[:, 0] - qq[:, 0] * nn[:, 2], qq[:, 0] * nn[:, 1] - qq[:, 1] * nn[:, 0],
             nn[:, 0], nn[:, 1], nn[:, 2]]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                v[rows, k] = J[a] * J[b]
                k += 1
        for a in range(6):
            v[rows, 21 + a] = J[a] * r
        v[rows, 27] = r * r
        v[rows, 28] = d2[use]
        pairs = int(use.sum())
        unusable = int(cand.sum()) - pairs
    return refine_tree_sum(v), pairs, int((~ok).sum()), unusable


def refine_poses_plane(map_xyz, scans, T_body2origin, T_lidar2body=None, k=16, max_dist=1.0, max_curvature=1.0, rank_tol=1e-9, eps_t=1e-4,
                       eps_r=1e-5, max_iters=20, min_pairs=100, nearest=nearest_f64, normals_hook=None):
    """Every frame's T_body2origin refined point-to-plane against the map's normals: the host restatement of Erasor.refine_poses_plane
    (include/erasor_hip.h, erasor_refine_plane_row), operation for operation.  The map's normals and curvature: normals(map, k), "up";
    normals_hook(nrm32, curv) -> nrm32, if given, replaces the normals (the orientation test's way in).  Per frame as refine_poses, with
    refine_plane_frame_sums and refine_plane_solve; min_pairs applies to the pairs; a solve of rank 0 keeps the pose and ends the frame
    with status 4.  Returns (T float64 [n, 4, 4], rows, summary): REFINE_PLANE_ROW_FIELDS per frame, REFINE_PLANE_SUMMARY_FIELDS."""
    import math
    who = "refine_poses_plane"
    if not (1 <= int(max_iters) <= 64):
        raise ValueError(who + ": max_iters must be 1 .. 64")
    for name, val in (("max_dist", max_dist), ("eps_t", eps_t), ("eps_r", eps_r), ("max_curvature", max_curvature)):
        if not (np.isfinite(val) and val > 0):
            raise ValueError(who + ": %s must be a finite number > 0" % name)
    if not (np.isfinite(rank_tol) and 0 <= rank_tol < 1):
        raise ValueError(who + ": rank_tol must be within [0, 1)")
    if not (isinstance(k, (int, np.integer)) and NORMALS_MIN_K <= k <= KNN_MAX_K):
        raise ValueError(who + ": normals_k must be within 2 .. 32")
    map32 = np.asarray(map_xyz, np.float32).reshape(-1, 3)
    map64 = map32.astype(np.float64)
    tree = cKDTree(map64) if len(map64) else None
    if tree is None and any(len(s) for s in scans):
        raise ValueError(who + ": empty map with a non-empty frame (no nearest point to match)")
    if len(map32):
        nrm32, curv, _, _ = normals(np.concatenate([map32, np.zeros((len(map32), 1), np.float32)], 1), int(k))
    else:
        nrm32, curv = np.zeros((0, 3), np.float32), np.zeros(0)
    if normals_hook is not None:
        nrm32 = np.asarray(normals_hook(nrm32, curv), np.float32).reshape(len(map32), 3)
    Tl = np.eye(4, dtype=np.float32) if T_lidar2body is None else T_lidar2body
    gate2 = float(max_dist) * float(max_dist)
    need = max(int(min_pairs), 1)
    max_curvature, rank_tol = float(max_curvature), float(rank_tol)
    nan = float("nan")
    n_f = len(scans)
    T_out = np.zeros((n_f, 4, 4))
    rows = []
    summary = {"n_frames": n_f, "n_status": [0, 0, 0, 0, 0], "n_pairs_first": 0, "n_pairs_last": 0, "sum_d2_first": 0.0, "sum_d2_last": 0.0,
               "sum_r2_first": 0.0, "sum_r2_last": 0.0, "n_map_no_normal": int(np.isnan(nrm32).any(1).sum())}
    for f, scan in enumerate(scans):
        xyz = np.asarray(scan, np.float32).reshape(len(scan), 4)[:, :3]
        with np.errstate(over="ignore", invalid="ignore"):
            p32 = _xform(Tl, xyz)
        T0 = np.asarray(T_body2origin[f], np.float32).reshape(4, 4)
        R0 = [float(T0[a, b]) for a in range(3) for b in range(3)]
        t0 = [float(T0[a, 3]) for a in range(3)]
        R, t = list(R0), list(t0)
        status, iters, rank, ratio = REFINE_MAX_ITERS, 0, 0, nan
        first = None
        for it in range(1, int(max_iters) + 1):
            S, pairs, bad, unusable = refine_plane_frame_sums(map64, tree, nrm32, curv, p32, R, t, gate2, max_curvature, nearest)
            if it == 1:
                first = (pairs, float(S[28]), float(S[27]), bad, unusable)
            if pairs < need:
                status = REFINE_NO_POINTS if first[3] == len(xyz) else REFINE_FEW_PAIRS
                break
            R, t, st, sr, rank, ratio = refine_plane_solve([float(s) for s in S], R, t, rank_tol)
            if rank == 0:
                status = REFINE_DEGENERATE
                break
            iters = it
            if st <= eps_t and sr <= eps_r:
                status = REFINE_CONVERGED
                break
        pairs_first, d2_first, r2_first, bad_first, unusable_first = first
        S, pairs_last, _, unusable_last = refine_plane_frame_sums(map64, tree, nrm32, curv, p32, R, t, gate2, max_curvature, nearest)
        d2_last, r2_last = float(S[28]), float(S[27])
        for a in range(3):
            T_out[f, a, :3] = R[3 * a:3 * a + 3]
            T_out[f, a, 3] = t[a]
        T_out[f, 3, 3] = 1.0
        dx, dy, dz = t[0] - t0[0], t[1] - t0[1], t[2] - t0[2]
        tr = 0.0
        for a in range(3):
            tr = tr + ((R[3 * a] * R0[3 * a] + R[3 * a + 1] * R0[3 * a + 1]) + R[3 * a + 2] * R0[3 * a + 2])
        cs = (tr - 1.0) / 2.0
        if cs > 1.0:
            cs = 1.0
        if cs < -1.0:
            cs = -1.0
        rows.append({"status": status, "iters": iters, "n_points": int(len(xyz)), "n_non_finite": bad_first, "n_pairs_first": pairs_first,
                     "n_pairs_last": pairs_last, "rms_first": math.sqrt(d2_first / float(pairs_first)) if pairs_first else nan,
                     "rms_last": math.sqrt(d2_last / float(pairs_last)) if pairs_last else nan,
                     "moved_t": math.sqrt((dx * dx + dy * dy) + dz * dz), "moved_r": math.acos(cs), "rank": rank, "lambda_ratio": ratio,
                     "n_unusable_first": unusable_first, "n_unusable_last": unusable_last,
                     "rms_plane_first": math.sqrt(r2_first / float(pairs_first)) if pairs_first else nan,
                     "rms_plane_last": math.sqrt(r2_last / float(pairs_last)) if pairs_last else nan})
        summary["n_status"][status] += 1
        summary["n_pairs_first"] += pairs_first
        summary["n_pairs_last"] += pairs_last
        summary["sum_d2_first"] = summary["sum_d2_first"] + d2_first
        summary["sum_d2_last"] = summary["sum_d2_last"] + d2_last
        summary["sum_r2_first"] = summary["sum_r2_first"] + r2_first
        summary["sum_r2_last"] = summary["sum_r2_last"] + r2_last
    return T_out, rows, summary


def _l2_simple(q, p):
    """FLANN's L2_Simple in float32, operation by operation: r = 0; r += dx*dx; r += dy*dy; r += dz*dz with dx = q.x - p.x"""
    r = np.zeros(len(q), np.float32)
    with np.errstate(over="ignore"):  # (a difference above 1.8e19 squares to +inf, as it does in FLANN)
        for a in range(3):
            d = q[:, a] - p[:, a]
            r += d * d
    return r


def nearest_f32(tree_xyz, query_xyz, tree_key=None):
    """Exact 1-NN in FLANN's float32 metric: (index, float32 d^2, tied) per query point.  The answer is the smallest tree index
    among the points at the minimum float32 d^2; `tied` says that those points carry more than one value of tree_key (default:
    the index itself, i.e. more than one point at the minimum).

    cKDTree is exact only in float64, whose minimum can be a different point: two float64 distances a few ulps apart can round
    to the same float32, or swap.  So cKDTree gives the float64 minimum d2_64 first, and query_ball_point then collects every
    point with d^2 <= d2_64 * (1 + 1e-5) + 1e-30, a superset of the float32 minimum's points: float32 rounding moves a d^2 by
    a relative 5 * 2^-24 (about 3e-7) at most, which the relative margin covers, except where products underflow to
    subnormals or zero, where the error is absolute (below 2^-149 per operation), which the absolute margin covers.  Among those
    candidates the float32 d^2 is computed as FLANN does and the minimum, then the lowest index, wins.  Queries with a single
    candidate (nearly all) need no second look: that candidate is cKDTree's answer.

    The margin argument needs finite values.  Where the float32 d^2 of cKDTree's answer overflows to +inf (a coordinate
    difference above about 1.8e19), a relative margin around the float64 minimum says nothing about which points share that
    +inf: those queries take ALL tree points as candidates, and the float32 minimum and its lowest index are computed outright."""
    t = np.ascontiguousarray(np.asarray(tree_xyz, np.float32).reshape(-1, 3))
    q = np.ascontiguousarray(np.asarray(query_xyz, np.float32).reshape(-1, 3))
    if len(t) == 0:
        raise ValueError("nearest_f32: empty tree")
    if len(q) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, bool)
    q64 = q.astype(np.float64)
    tree = cKDTree(t.astype(np.float64))
    d64, idx = tree.query(q64, k=1, workers=-1)
    idx = np.asarray(idx, np.int64)
    r = np.sqrt(d64 * d64 * (1 + 1e-5) + 1e-30)
    cnt = tree.query_ball_point(q64, r, workers=-1, return_length=True)
    d2 = _l2_simple(q, t[idx])
    tied = np.zeros(len(q), bool)
    overflowed = ~np.isfinite(d2)
    multi = np.nonzero((cnt > 1) | (overflowed & (len(t) > 1)))[0]
    if len(multi):
        lists = tree.query_ball_point(q64[multi], r[multi], workers=-1)
        everything = np.arange(len(t), dtype=np.int64)
        lists = [everything if o else c for c, o in zip(lists, overflowed[multi])]
        lens = np.array([len(c) for c in lists], np.int64)
        cand = np.concatenate([np.asarray(c, np.int64) for c in lists])
        owner = np.repeat(np.arange(len(multi)), lens)
        dd = _l2_simple(q[multi][owner], t[cand])
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        m = np.minimum.reduceat(dd, starts)
        at = dd == m[owner]
        # the lowest index at the minimum: sort the (owner, index) pairs at the minimum and take each owner's first
        o_at, c_at = owner[at], cand[at]
        order = np.lexsort((c_at, o_at))
        o_at, c_at = o_at[order], c_at[order]
        first = np.concatenate([[True], o_at[1:] != o_at[:-1]])
        idx[multi] = c_at[first]
        d2[multi] = m
        key = c_at if tree_key is None else np.asarray(tree_key)[c_at]
        k_first = np.repeat(key[first], np.diff(np.concatenate([np.nonzero(first)[0], [len(o_at)]])))
        differs = np.zeros(len(multi), bool)
        np.logical_or.at(differs, o_at, key != k_first)
        tied[multi] = differs
    return idx, d2, tied


def label_from(centroids, medium):
    """label_map's second half: each row of `centroids` (XYZI; its intensity is not read) takes the intensity of its nearest
    `medium` point, copied as bits.  Returns (rows, {"n_tied": rows whose minimum is shared by medium points of different
    intensity bits})."""
    c = np.asarray(centroids, np.float32).reshape(-1, 4)
    m = np.asarray(medium, np.float32).reshape(-1, 4)
    out = c.copy()
    if len(c) == 0:
        return out, {"n_tied": 0}
    wbits = np.ascontiguousarray(m[:, 3]).view(np.uint32)
    idx, _, tied = nearest_f32(m[:, :3], c[:, :3], wbits)
    out.view(np.uint32)[:, 3] = wbits[idx]
    return out, {"n_tied": int(tied.sum())}


def static_complement(est, gt):
    """calc_complement: the static points of the labelled ground truth `gt` (XYZI) whose nearest point of `est` has a float32
    d^2 that, widened to double, is > 0.03 (the reference compares the float with a double literal), in ground-truth order.
    Labels as `labels`; intensities the cast is not defined for (not finite, outside [0, 2^32)) are static and counted.  An
    empty estimate loses every static point.  Returns (rows, {"n_gt", "n_gt_static", "n_lost", "n_label_out_of_range"})."""
    e = np.asarray(est, np.float32).reshape(-1, 4)
    g = np.asarray(gt, np.float32).reshape(-1, 4)
    w = g[:, 3]
    oor = ~((w >= 0) & (w < 4294967296.0))
    sem = np.where(oor, 0, w).astype(np.uint32) & 0xFFFF
    static = oor | ~np.isin(sem, DYNAMIC_CLASSES)
    d2 = np.full(len(g), np.inf, np.float32)
    if len(e) and static.any():
        _, d2[static], _ = nearest_f32(e[:, :3], g[static, :3])
    lost = static & (d2.astype(np.float64) > 0.03)
    return g[lost].copy(), {"n_gt": int(len(g)), "n_gt_static": int(static.sum()), "n_lost": int(lost.sum()),
                            "n_label_out_of_range": int(oor.sum())}


# the public SemanticKITTI label names (semantic-kitti.yaml), for printing
SEMANTIC_KITTI_NAMES = {
    0: "unlabeled", 1: "outlier", 10: "car", 11: "bicycle", 13: "bus", 15: "motorcycle", 16: "on-rails", 18: "truck",
    20: "other-vehicle", 30: "person", 31: "bicyclist", 32: "motorcyclist", 40: "road", 44: "parking", 48: "sidewalk",
    49: "other-ground", 50: "building", 51: "fence", 52: "other-structure", 60: "lane-marking", 70: "vegetation", 71: "trunk",
    72: "terrain", 80: "pole", 81: "traffic-sign", 99: "other-object", 252: "moving-car", 253: "moving-bicyclist",
    254: "moving-person", 255: "moving-motorcyclist", 256: "moving-on-rails", 257: "moving-bus", 258: "moving-truck",
    259: "moving-other-vehicle",
}
KEY_LABEL_OUT_OF_RANGE = 0x10000
ROW_FIELDS = ("key", "is_dynamic", "n_gt", "n_within", "n_preserved", "n_tied", "n_est", "PR", "RR")


def _decode(w):
    """(class key, whole label, is_dynamic) per intensity: uint32(w) & 0xFFFF, or KEY_LABEL_OUT_OF_RANGE (static) where the cast is not
    defined (not finite, outside [0, 2^32))"""
    w = np.asarray(w, np.float32)
    inr = (w >= 0) & (w < np.float32(4294967296.0))
    lab = np.where(inr, w, np.float32(0)).astype(np.uint32)
    sem = lab & 0xFFFF
    key = np.where(inr, sem, KEY_LABEL_OUT_OF_RANGE).astype(np.int64)
    return key, lab, inr & (sem >= 252) & (sem <= 259)


def _rows(keys, is_dyn, cnt):
    """records of the rows: cnt[name] are arrays aligned with keys; PR / RR as evaluate forms them, per row"""
    dt = np.dtype([("key", np.uint32), ("is_dynamic", np.uint32)] + [(k, np.uint64) for k in ROW_FIELDS[2:7]] +
                  [("PR", np.float64), ("RR", np.float64)])
    out = np.zeros(len(keys), dt)
    out["key"] = keys
    out["is_dynamic"] = is_dyn
    for k in ROW_FIELDS[2:7]:
        out[k] = cnt[k]
    n, kept = out["n_gt"].astype(np.float64), out["n_preserved"].astype(np.float64)
    has = n > 0
    pr, rr = np.zeros(len(out)), np.zeros(len(out))
    pr[has] = kept[has] / n[has] * 100.0
    rr[has] = (n[has] - kept[has]) / n[has] * 100.0
    dyn = out["is_dynamic"] != 0
    out["PR"] = np.where(dyn, np.nan, pr)
    out["RR"] = np.where(dyn, rr, np.nan)
    return out


def evaluate_by_class(gt_xyzi, est_xyzi, voxelsize=0.2):
    """PR / RR broken down by class key and by dynamic instance (include/erasor_hip.h, erasor_eval_class_row), on the host.  The decision
    per GT point is evaluate's: the nearest estimated point (cKDTree), within voxelsize*sqrt(3)/2, kept when both are static or both
    dynamic; among estimated points at exactly the same float64 d^2 the smallest index answers, and a GT point whose minimum is shared
    by points of both classes is counted as tied.  Returns evaluate's counts, n_tied, and "classes" / "instances" (records with
    ROW_FIELDS)."""
    gt = np.asarray(gt_xyzi, np.float32).reshape(-1, 4)
    est = np.asarray(est_xyzi, np.float32).reshape(-1, 4)
    g_key, g_lab, g_dyn = _decode(gt[:, 3])
    e_key, e_lab, e_dyn = _decode(est[:, 3])
    thr = voxelsize * np.sqrt(3) / 2
    within = np.zeros(len(gt), bool)
    kept = np.zeros(len(gt), bool)
    tied = np.zeros(len(gt), bool)
    if len(gt) and len(est):
        e64 = est[:, :3].astype(np.float64)
        g64 = gt[:, :3].astype(np.float64)
        tree = cKDTree(e64)
        k = 2 if len(est) > 1 else 1
        d, idx = tree.query(g64, k=k, workers=-1)
        d, idx = d.reshape(len(gt), k), idx.reshape(len(gt), k)
        within = d[:, 0] < thr
        best = idx[:, 0].copy()
        # a second point as near (to 1e-9): every candidate at the exact minimum of ((dx*dx + dy*dy) + dz*dz)
        maybe = np.nonzero(within & (d[:, -1] <= d[:, 0] * (1 + 1e-9)))[0] if k == 2 else np.zeros(0, np.int64)
        for i in maybe:
            cand = np.asarray(sorted(tree.query_ball_point(g64[i], d[i, 0] * (1 + 1e-9) + 1e-300)), np.int64)
            dd = g64[i] - e64[cand]
            d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
            at = cand[d2 == d2.min()]
            best[i] = at[0]
            tied[i] = e_dyn[at].any() and (~e_dyn[at]).any()
        kept = within & (g_dyn == e_dyn[best])
    res = {"gt_static": int((~g_dyn).sum()), "gt_dynamic": int(g_dyn.sum()), "est_static": int((~e_dyn).sum()),
           "est_dynamic": int(e_dyn.sum()), "preserved_static": int((kept & ~g_dyn).sum()), "preserved_dynamic": int((kept & g_dyn).sum()),
           "n_tied": int(tied.sum())}

    def table(gk, ek, n):
        c = {"n_gt": np.bincount(gk, minlength=n), "n_within": np.bincount(gk, within, minlength=n).astype(np.int64),
             "n_preserved": np.bincount(gk, kept, minlength=n).astype(np.int64),
             "n_tied": np.bincount(gk, tied, minlength=n).astype(np.int64), "n_est": np.bincount(ek, minlength=n)}
        return {k: v[:n] for k, v in c.items()}

    keys = np.union1d(g_key, e_key).astype(np.int64)
    c = table(np.searchsorted(keys, g_key), np.searchsorted(keys, e_key), len(keys))
    sem = keys & 0xFFFF
    res["classes"] = _rows(keys, (keys < KEY_LABEL_OUT_OF_RANGE) & (sem >= 252) & (sem <= 259), c)
    labs = np.union1d(g_lab[g_dyn], e_lab[e_dyn]).astype(np.int64)
    gi = np.searchsorted(labs, g_lab.astype(np.int64))
    ei = np.searchsorted(labs, e_lab.astype(np.int64))
    ci = {k: np.bincount(gi[g_dyn], v[g_dyn] if v is not None else None, minlength=len(labs)).astype(np.int64)
          for k, v in (("n_gt", None), ("n_within", within), ("n_preserved", kept), ("n_tied", tied))}
    ci["n_est"] = np.bincount(ei[e_dyn], minlength=len(labs))
    res["instances"] = _rows(labs, np.ones(len(labs), np.uint32), ci)
    return res


# ---- bird's-eye images (include/erasor_hip.h: erasor_hip_render_*; kernels: erasor_amd/csrc/render.hip.h), on the host -------------
# The arithmetic of the device rasteriser spelled out in numpy, byte for byte: the pixel of a point in float64 from its float32
# coordinates, the winner of a pixel by (priority, z in float32's total order), the colour from (category, z).
RENDER_LABEL, RENDER_HEIGHT, RENDER_EVAL = 0, 1, 2
RENDER_MODES = {"label": RENDER_LABEL, "height": RENDER_HEIGHT, "eval": RENDER_EVAL}
RENDER_CATEGORIES = ("static", "dynamic", "target", "height", "static_kept", "dynamic_removed", "static_lost", "dynamic_left")
RENDER_PALETTE = (0xC8C8C8, 0xFF5050, 0xFFE000, 0x80D0FF, 0xB4B4B4, 0x30C040, 0x3060FF, 0xFF2020)  # ERASOR_RENDER_PALETTE
RENDER_PRIORITY = (1, 2, 3, 1, 1, 2, 3, 4)                                                          # ERASOR_RENDER_PRIORITY
RENDER_CAT_BASE = {RENDER_LABEL: 0, RENDER_HEIGHT: 3, RENDER_EVAL: 4}  # category = base + priority - 1
RENDER_MAX_EDGE, RENDER_MAX_PIXELS = 16384, 1 << 26
VIEW_FIELDS = ("x0", "y0", "res", "width", "height", "z_lo", "z_hi", "background")


def render_view(x0, y0, res, width, height, z_lo=0.0, z_hi=0.0, background=0):
    return {"x0": float(x0), "y0": float(y0), "res": float(res), "width": int(width), "height": int(height), "z_lo": float(z_lo),
            "z_hi": float(z_hi), "background": int(background) & 0xFFFFFF}


def check_view(v):
    ok = (np.isfinite([v["x0"], v["y0"], v["res"], v["z_lo"], v["z_hi"]]).all() and v["res"] > 0 and 1 <= v["width"] <= RENDER_MAX_EDGE and
          1 <= v["height"] <= RENDER_MAX_EDGE and v["width"] * v["height"] <= RENDER_MAX_PIXELS)
    if not ok:
        raise ValueError("render: view outside the limits (finite, res > 0, 1 <= width, height <= 16384, width * height <= 2^26)")


def z_order(z):
    """float32's total order as uint32 keys: -0.0 below +0.0"""
    b = np.ascontiguousarray(z, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def z_from_order(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def shade(base, z, z_lo, z_hi):
    """one channel: (uint8)floor(base * (0.35 + 0.65 * s) + 0.5), s = z_hi > z_lo ? clamp((z - z_lo) / (z_hi - z_lo), 0, 1) : 1"""
    z = np.asarray(z, np.float32).astype(np.float64)
    if z_hi > z_lo:
        s = np.minimum(np.maximum((z - z_lo) / (z_hi - z_lo), 0.0), 1.0)
    else:
        s = np.ones_like(z)
    return np.floor(np.asarray(base, np.float64) * (0.35 + 0.65 * s) + 0.5).astype(np.uint8)


def render_fit(cloud, res=0.2, margin=2, background=0):
    """erasor_hip_render_fit: the view that contains every finite point, z_lo / z_hi at ranks floor(0.02 (n - 1)) / floor(0.98 (n - 1))"""
    c = np.asarray(cloud, np.float32).reshape(-1, 4)
    if not (np.isfinite(res) and res > 0 and 1 <= margin <= 1024):
        raise ValueError("render_fit: res must be finite and > 0, margin in 1 .. 1024")
    c = c[np.isfinite(c[:, :3]).all(1)]
    if len(c) == 0:
        raise ValueError("render_fit: the cloud has no finite point")
    out = {}
    for name, size, a in (("x0", "width", 0), ("y0", "height", 1)):
        mn, mx = float(c[:, a].min()), float(c[:, a].max())
        o = np.floor(mn / res) * res - margin * res
        out[name] = float(o)
        out[size] = float(np.floor((mx - o) / res) + 1 + margin)
    if not (out["width"] <= RENDER_MAX_EDGE and out["height"] <= RENDER_MAX_EDGE and out["width"] * out["height"] <= RENDER_MAX_PIXELS):
        raise ValueError("render_fit: %.0f x %.0f pixels at res %g is beyond the limits" % (out["width"], out["height"], res))
    n = len(c)
    zs = z_from_order(np.sort(z_order(c[:, 2])))  # (ascending in the total order)
    z_lo, z_hi = float(zs[int(np.floor(0.02 * (n - 1)))]), float(zs[int(np.floor(0.98 * (n - 1)))])
    return render_view(out["x0"], out["y0"], res, int(out["width"]), int(out["height"]), z_lo, z_hi, background)


def _raster(c, prio, mode, view):
    """the image and the statistics of the points c (float32 XYZI rows) with per-point priorities (1..4) within `mode`"""
    check_view(view)
    W, H = view["width"], view["height"]
    fin = np.isfinite(c[:, :3]).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        cx = np.floor((c[:, 0].astype(np.float64) - view["x0"]) / view["res"])
        cy = np.floor((c[:, 1].astype(np.float64) - view["y0"]) / view["res"])
        inside = fin & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    key = (prio[inside].astype(np.uint64) << np.uint64(32)) | z_order(c[inside, 2]).astype(np.uint64)
    pix = (H - 1 - cy[inside].astype(np.int64)) * W + cx[inside].astype(np.int64)
    kimg = np.zeros(H * W, np.uint64)
    np.maximum.at(kimg, pix, key)
    hit = kimg != 0
    p_img = (kimg >> np.uint64(32)).astype(np.int64)
    z_img = np.where(hit, z_from_order((kimg & np.uint64(0xFFFFFFFF)).astype(np.uint32)), np.float32(0))  # (key 0 decodes to NaN)
    base0 = RENDER_CAT_BASE[mode]
    pal = np.asarray(RENDER_PALETTE, np.int64)[np.where(hit, base0 + p_img - 1, 0)]
    img = np.empty((H * W, 3), np.uint8)
    for ch, sh in enumerate((16, 8, 0)):
        img[:, ch] = np.where(hit, shade((pal >> sh) & 0xFF, z_img, view["z_lo"], view["z_hi"]), (view["background"] >> sh) & 0xFF)
    cat_points, cat_pixels = [0] * 8, [0] * 8
    for k in range(1, 5):
        if base0 + k - 1 < 8:
            cat_points[base0 + k - 1] = int((prio[inside] == k).sum())
            cat_pixels[base0 + k - 1] = int((hit & (p_img == k)).sum())
    stats = {"n_points": int(len(c)), "n_drawn": int(inside.sum()), "n_outside": int((fin & ~inside).sum()), "n_nonfinite": int((~fin).sum()),
             "n_pixels_hit": int(hit.sum()), "cat_points": cat_points, "cat_pixels": cat_pixels}
    return img.reshape(H, W, 3), stats


def render(cloud, view, mode="label", target_class=None, target_instance=None):
    """erasor_hip_render_clouds on the host: (uint8 image H x W x 3, stats).  mode "label": static 1, dynamic 2, target 3 (a dynamic
    point of target_class, and of target_instance when given); "height": one category."""
    c = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 4))
    m = RENDER_MODES[mode] if isinstance(mode, str) else mode
    prio = np.ones(len(c), np.int64)
    if m == RENDER_LABEL:
        _, lab, dyn = _decode(c[:, 3])
        prio[dyn] = 2
        if target_class is not None and target_class >= 0:
            t = dyn & ((lab & 0xFFFF) == target_class)
            if target_instance is not None and target_instance >= 0:
                t &= (lab >> 16) == target_instance
            prio[t] = 3
    elif m != RENDER_HEIGHT:
        raise ValueError("render: mode must be 'label' or 'height' (the error map: render_eval)")
    return _raster(c, prio, m, view)


def eval_codes(gt_xyzi, est_xyzi, voxelsize=0.2):
    """evaluate's decision per ground-truth point as ERASOR_EVAL_* codes (0 out, 1 kept static, 2 kept dynamic, 3 class differs), and
    the ground truth's dynamic flags"""
    gt = np.asarray(gt_xyzi, np.float32).reshape(-1, 4)
    est = np.asarray(est_xyzi, np.float32).reshape(-1, 4)
    g_dyn, e_dyn = _decode(gt[:, 3])[2], _decode(est[:, 3])[2]
    code = np.zeros(len(gt), np.uint8)
    if len(gt) and len(est):
        dists, idx = cKDTree(est[:, :3].astype(np.float64)).query(gt[:, :3].astype(np.float64), k=1, workers=-1)
        is_in = dists < voxelsize * np.sqrt(3) / 2
        same = g_dyn == e_dyn[idx]
        code[is_in & same & ~g_dyn] = 1
        code[is_in & same & g_dyn] = 2
        code[is_in & ~same] = 3
    return code, g_dyn


def render_eval(gt_xyzi, est_xyzi, view, voxelsize=0.2):
    """erasor_hip_render_eval_clouds (voxel_leaf 0) on the host: the ground truth drawn by evaluate's decision per point -- static kept 1,
    dynamic removed 2, static lost 3, dynamic left 4.  Returns (image, stats, evaluate_clouds' dict)."""
    gt = np.ascontiguousarray(np.asarray(gt_xyzi, np.float32).reshape(-1, 4))
    code, g_dyn = eval_codes(gt, est_xyzi, voxelsize)
    prio = np.where(code == 1, 1, np.where(code == 2, 4, np.where(g_dyn, 2, 3))).astype(np.int64)
    img, stats = _raster(gt, prio, RENDER_EVAL, view)
    return img, stats, evaluate_clouds(gt, est_xyzi, voxelsize)


# ---- Euclidean clustering (include/erasor_hip.h: erasor_hip_cluster_*; kernels: erasor_amd/csrc/cluster.hip.h), on the host ---------
# The host restatement of the device's contract: points i and j are adjacent iff ((dx*dx + dy*dy) + dz*dz) <= tol*tol in float64 (dx =
# float64(x_i) - float64(x_j)), a cluster is a connected component named by its lowest point index, a cluster is listed when min_size <=
# n_points and (max_size == 0 or n_points <= max_size), rows in increasing `first`, the box in z_order's total order.
CLUSTER_ROW_DTYPE = np.dtype([("first", np.uint32), ("n_points", np.uint32), ("n_dynamic", np.uint32), ("n_label_out_of_range", np.uint32),
                              ("min_xyz", np.float32, 3), ("max_xyz", np.float32, 3)])
CLUSTER_NONE = 0xFFFFFFFF
CLUSTER_RESULT_FIELDS = ("n_points", "n_clusters", "n_listed", "n_points_listed", "n_singletons", "largest")


def cluster_adjacent(a, b, tol):
    """the predicate, row by row: a, b float32 (k, 3) arrays"""
    d = np.asarray(a, np.float32).astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= np.float64(tol) * np.float64(tol)


def _cluster_args(cloud, tol, min_size, max_size):
    c = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 4))
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("cluster: tol must be a finite number > 0")
    if len(c) > 1 << 30:
        raise ValueError("cluster: more than 2^30 points")
    if not np.isfinite(c[:, :3]).all():
        raise ValueError("cluster: non-finite coordinate")
    if min_size < 0 or max_size < 0:
        raise ValueError("cluster: negative size limit")
    return c, float(tol), max(int(min_size), 1), int(max_size)


def _cluster_finish(c, comp_any, min_size, max_size):
    """rows, ids, kept cloud and result from any labelling of the components (comp_any[i]: an integer per component)"""
    n = len(c)
    if n == 0:
        return (np.zeros(0, CLUSTER_ROW_DTYPE), np.zeros(0, np.uint32), c.copy(),
                dict.fromkeys(CLUSTER_RESULT_FIELDS, 0))
    # canonical form: the clusters numbered in the order of their lowest point index
    _, first, inv, counts = np.unique(comp_any, return_index=True, return_inverse=True, return_counts=True)
    by_first = np.argsort(first)
    number = np.empty(len(first), np.int64)
    number[by_first] = np.arange(len(first))
    comp = number[inv.reshape(-1)]
    first, counts = first[by_first], counts[by_first]
    k = len(first)
    key, _, dyn = _decode(c[:, 3])
    order = np.argsort(comp, kind="stable")
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    rows_all = np.zeros(k, CLUSTER_ROW_DTYPE)
    rows_all["first"] = first
    rows_all["n_points"] = counts
    rows_all["n_dynamic"] = np.bincount(comp, dyn, minlength=k).astype(np.uint32)
    rows_all["n_label_out_of_range"] = np.bincount(comp, key == KEY_LABEL_OUT_OF_RANGE, minlength=k).astype(np.uint32)
    for a in range(3):
        keys = z_order(c[:, a])[order]
        rows_all["min_xyz"][:, a] = z_from_order(np.minimum.reduceat(keys, starts))
        rows_all["max_xyz"][:, a] = z_from_order(np.maximum.reduceat(keys, starts))
    listed = (counts >= min_size) & ((max_size == 0) | (counts <= max_size))
    lrank = np.full(k, CLUSTER_NONE, np.uint32)
    lrank[listed] = np.arange(int(listed.sum()), dtype=np.uint32)
    ids = lrank[comp]
    res = {"n_points": int(n), "n_clusters": int(k), "n_listed": int(listed.sum()), "n_points_listed": int(counts[listed].sum()),
           "n_singletons": int((counts == 1).sum()), "largest": int(counts.max())}
    return rows_all[listed].copy(), ids, c[ids != CLUSTER_NONE].copy(), res


def _components(n, i, j):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = coo_matrix((np.ones(len(i), np.uint8), (i, j)), shape=(n, n))
    return connected_components(g, directed=False)[1]


def cluster(cloud, tol, min_size=1, max_size=0):
    """Euclidean clustering of `cloud` (XYZI rows) at the tolerance tol.  cKDTree.query_pairs with a radius a hair above tol only
    proposes the pairs; the float64 predicate decides.  Returns (rows, ids, kept, result): CLUSTER_ROW_DTYPE records of the listed
    clusters in increasing `first`; per point the index of its cluster among the rows, or CLUSTER_NONE; the rows of the points of listed
    clusters in the order given; and a dict with CLUSTER_RESULT_FIELDS."""
    c, tol, min_size, max_size = _cluster_args(cloud, tol, min_size, max_size)
    n = len(c)
    if n == 0:
        return _cluster_finish(c, None, min_size, max_size)
    c64 = c[:, :3].astype(np.float64)
    # (the tree's own float64 distances are a few ulps off the predicate's: 1e-9 relative is far above that, far below a float32 step)
    pairs = cKDTree(c64).query_pairs(tol * (1 + 1e-9), output_type="ndarray")
    ok = cluster_adjacent(c[pairs[:, 0], :3], c[pairs[:, 1], :3], tol)
    return _cluster_finish(c, _components(n, pairs[ok, 0], pairs[ok, 1]), min_size, max_size)


def cluster_brute(cloud, tol, min_size=1, max_size=0):
    """cluster() with every pair tested by the predicate in numpy (no tree): for a few thousand points"""
    c, tol, min_size, max_size = _cluster_args(cloud, tol, min_size, max_size)
    n = len(c)
    if n == 0:
        return _cluster_finish(c, None, min_size, max_size)
    c64 = c[:, :3].astype(np.float64)
    t2 = np.float64(tol) * np.float64(tol)
    ii, jj = [], []
    for lo in range(0, n, 512):  # (row blocks: 512 x n distances at a time)
        d = c64[lo:lo + 512, None, :] - c64[None, :, :]
        adj = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2] <= t2
        a, b = np.nonzero(adj)
        ii.append(a + lo)
        jj.append(b)
    return _cluster_finish(c, _components(n, np.concatenate(ii), np.concatenate(jj)), min_size, max_size)


# ---- the decision per object (include/erasor_hip.h: erasor_hip_object_vote_*; kernels: erasor_amd/csrc/objects.hip.h), on the host -----
# The host restatement of the device's contract.  Point i is voted iff votes[i] >= vote_thr and ground iff ground[i] != 0.  Ground points
# are outside the graph: adjacent to nothing, in no cluster; over the others adjacency is cluster's, a cluster is a connected component
# and its `first` the lowest index it contains in the GIVEN cloud's indexing.  Per cluster, in this order: OBJECT_NOT_OBJECT when n_points <
# max(min_size, 1), or max_size != 0 and n_points > max_size, or max_extent > 0 and float64(max) - float64(min) > max_extent on some axis
# (per-point votes stand); OBJECT_REMOVED when n_voted >= min_voted and float64(n_voted) >= remove_ratio * float64(n_points) (every
# point goes); OBJECT_REVERTED when n_voted > 0 and float64(n_voted) <= revert_ratio * float64(n_points) (every point stays);
# OBJECT_UNCHANGED otherwise (per-point votes stand).  A ground point is kept if ground_keep, otherwise removed iff voted.  One row per
# touched cluster (n_voted > 0) in increasing `first`.  Counts, boxes and one float64 product per cluster: no float sum anywhere.
OBJECT_UNCHANGED, OBJECT_REMOVED, OBJECT_REVERTED, OBJECT_NOT_OBJECT = 0, 1, 2, 3
OBJECT_NONE = 0xFFFFFFFF
OBJECT_ROW_DTYPE = np.dtype([(k, np.uint32) for k in ("first", "n_points", "n_voted", "n_dynamic", "n_voted_dynamic", "n_label_out_of_range")] +
                            [("min_xyz", np.float32, 3), ("max_xyz", np.float32, 3), ("decision", np.uint32)])
OBJECT_RESULT_FIELDS = ("n_points", "n_ground", "n_clusters", "n_touched", "n_removed_clusters", "n_reverted_clusters", "n_not_object", "n_voted",
                        "n_removed", "n_grown", "n_grown_dynamic", "n_reverted", "n_reverted_dynamic", "n_ground_reverted",
                        "n_ground_reverted_dynamic", "largest")


def _object_args(cloud, votes, ground, tol, vote_thr, min_size, max_size, max_extent, remove_ratio, revert_ratio, min_voted):
    c = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 4))
    v = np.ascontiguousarray(np.asarray(votes, np.uint8).reshape(-1))
    g = np.zeros(len(c), np.uint8) if ground is None else np.ascontiguousarray(np.asarray(ground, np.uint8).reshape(-1))
    if len(v) != len(c) or len(g) != len(c):
        raise ValueError("object_vote: votes and ground must have one entry per point")
    if len(c) > 1 << 30:
        raise ValueError("object_vote: more than 2^30 points")
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("object_vote: tol must be a finite number > 0")
    if not 1 <= int(vote_thr) <= 255:
        raise ValueError("object_vote: vote_thr must be within 1 .. 255")
    if not (np.isfinite(max_extent) and max_extent >= 0):
        raise ValueError("object_vote: max_extent must be 0 or a finite number > 0")
    if not (0 < remove_ratio <= 1):
        raise ValueError("object_vote: remove_ratio must be within (0, 1]")
    if not (0 <= revert_ratio < 1) or revert_ratio >= remove_ratio:
        raise ValueError("object_vote: revert_ratio must be within [0, 1) and below remove_ratio")
    if min_size < 0 or max_size < 0 or min_voted < 0:
        raise ValueError("object_vote: negative size limit")
    if not np.isfinite(c[:, :3]).all():
        raise ValueError("object_vote: non-finite coordinate")
    return c, v, g != 0


def object_decide(n_points, n_voted, min_xyz, max_xyz, min_size=1, max_size=0, max_extent=0.0, remove_ratio=0.5, revert_ratio=0.0, min_voted=1):
    """the decision code of every cluster (arrays, one entry per cluster; the boxes float32 (k, 3)), tested in the contract's order"""
    n = np.asarray(n_points, np.int64)
    nv = np.asarray(n_voted, np.int64)
    ext = np.asarray(max_xyz, np.float32).astype(np.float64) - np.asarray(min_xyz, np.float32).astype(np.float64)
    gate = (n < max(int(min_size), 1)) | ((int(max_size) != 0) & (n > int(max_size)))
    if max_extent > 0:
        gate = gate | (ext > np.float64(max_extent)).any(axis=1)
    nd, vd = n.astype(np.float64), nv.astype(np.float64)
    removed = (nv >= int(min_voted)) & (vd >= np.float64(remove_ratio) * nd)
    reverted = (nv > 0) & (vd <= np.float64(revert_ratio) * nd)
    return np.where(gate, OBJECT_NOT_OBJECT, np.where(removed, OBJECT_REMOVED, np.where(reverted, OBJECT_REVERTED, OBJECT_UNCHANGED))).astype(np.uint32)


def _object_finish(c, voted, is_ground, comp_any, min_size, max_size, max_extent, remove_ratio, revert_ratio, min_voted, ground_keep):
    """mask, rows, ids, kept cloud and result from any labelling of the non-ground points' components (comp_any: an integer per non-ground
    point, in the order of their indices)"""
    n = len(c)
    res = dict.fromkeys(OBJECT_RESULT_FIELDS, 0)
    res["n_points"] = int(n)
    ids = np.full(n, OBJECT_NONE, np.uint32)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(0, OBJECT_ROW_DTYPE), ids, c.copy(), res
    _, _, dyn = _decode(c[:, 3])
    src = np.flatnonzero(~is_ground)  # (ascending: a cluster's lowest compacted index is its lowest given index)
    removed = voted & ~(is_ground & bool(ground_keep))  # (the per-point votes; the clusters' decisions change them below)
    rows = np.zeros(0, OBJECT_ROW_DTYPE)
    if len(src):
        rows_cl, comp, _, r_cl = _cluster_finish(np.ascontiguousarray(c[src]), comp_any, 1, 0)
        k = len(rows_cl)
        comp = comp.astype(np.int64)
        n_voted = np.bincount(comp, voted[src], minlength=k).astype(np.int64)
        code = object_decide(rows_cl["n_points"], n_voted, rows_cl["min_xyz"], rows_cl["max_xyz"], min_size, max_size, max_extent, remove_ratio,
                             revert_ratio, min_voted)
        touched = n_voted > 0
        rows = np.zeros(int(touched.sum()), OBJECT_ROW_DTYPE)
        rows["first"] = src[rows_cl["first"][touched]]
        for f in ("n_points", "n_dynamic", "n_label_out_of_range", "min_xyz", "max_xyz"):
            rows[f] = rows_cl[f][touched]
        rows["n_voted"] = n_voted[touched]
        rows["n_voted_dynamic"] = np.bincount(comp, voted[src] & dyn[src], minlength=k)[touched]
        rows["decision"] = code[touched]
        rank = np.full(k, OBJECT_NONE, np.uint32)
        rank[touched] = np.arange(len(rows), dtype=np.uint32)
        ids[src] = rank[comp]
        pc = code[comp]
        removed[src] = np.where(pc == OBJECT_REMOVED, True, np.where(pc == OBJECT_REVERTED, False, voted[src]))
        res.update(n_clusters=int(k), n_touched=len(rows), n_removed_clusters=int((code[touched] == OBJECT_REMOVED).sum()),
                   n_reverted_clusters=int((code[touched] == OBJECT_REVERTED).sum()), n_not_object=int((code[touched] == OBJECT_NOT_OBJECT).sum()),
                   largest=r_cl["largest"])
    grown, rev, grev = ~voted & removed, voted & ~is_ground & ~removed, voted & is_ground & ~removed
    res.update(n_ground=int(is_ground.sum()), n_voted=int(voted.sum()), n_removed=int(removed.sum()), n_grown=int(grown.sum()),
               n_grown_dynamic=int((grown & dyn).sum()), n_reverted=int(rev.sum()), n_reverted_dynamic=int((rev & dyn).sum()),
               n_ground_reverted=int(grev.sum()), n_ground_reverted_dynamic=int((grev & dyn).sum()))
    mask = (~removed).astype(np.uint8)
    return mask, rows, ids, c[mask != 0].copy(), res


def object_vote(cloud, votes, ground=None, tol=0.5, vote_thr=1, min_size=1, max_size=0, max_extent=0.0, remove_ratio=0.5, revert_ratio=0.0,
                min_voted=1, ground_keep=True):
    """A removal method's per-point votes decided per object.  `cloud`: XYZI rows; `votes`: uint8 per point (voted iff >= vote_thr: a sum
    of several methods' votes with vote_thr=2 of three is their majority); `ground`: uint8 per point or None -- ground points are cut out
    of the graph, which is what lets the objects standing on them fall apart into clusters.  Every cluster of the other points (cluster's
    adjacency at `tol`) is removed whole when at least min_voted and the share remove_ratio of its points are voted, kept whole when at
    most the share revert_ratio is, and left to its per-point votes otherwise or when it is no object (fewer than min_size or more than
    max_size points, a box side above max_extent).  revert_ratio is 0 by default and nothing is reverted: where the ground mask is
    incomplete one huge cluster holds every object through the ground, and its tiny vote share must not wipe the votes out -- set
    max_size or max_extent before using revert_ratio.  Returns (mask, rows, ids, kept, result): uint8 per point, 1 = kept;
    OBJECT_ROW_DTYPE records of the touched clusters (n_voted > 0) in increasing `first`; per point its row index or OBJECT_NONE (ground
    points, points of untouched clusters); the rows with mask 1 in the order given; a dict with OBJECT_RESULT_FIELDS.  cKDTree only
    proposes the pairs, as in cluster."""
    c, v, g = _object_args(cloud, votes, ground, tol, vote_thr, min_size, max_size, max_extent, remove_ratio, revert_ratio, min_voted)
    voted = v >= int(vote_thr)
    src = np.flatnonzero(~g)
    comp = None
    if len(src):
        c64 = c[src, :3].astype(np.float64)
        pairs = cKDTree(c64).query_pairs(float(tol) * (1 + 1e-9), output_type="ndarray")
        ok = cluster_adjacent(c[src[pairs[:, 0]], :3], c[src[pairs[:, 1]], :3], tol)
        comp = _components(len(src), pairs[ok, 0], pairs[ok, 1])
    return _object_finish(c, voted, g, comp, min_size, max_size, max_extent, remove_ratio, revert_ratio, min_voted, ground_keep)


def object_vote_brute(cloud, votes, ground=None, tol=0.5, vote_thr=1, min_size=1, max_size=0, max_extent=0.0, remove_ratio=0.5, revert_ratio=0.0,
                      min_voted=1, ground_keep=True):
    """object_vote() with no tree: a plain flood fill from every non-ground point not yet reached, each step testing the predicate against
    all non-ground points -- for a few thousand points"""
    c, v, g = _object_args(cloud, votes, ground, tol, vote_thr, min_size, max_size, max_extent, remove_ratio, revert_ratio, min_voted)
    voted = v >= int(vote_thr)
    src = np.flatnonzero(~g)
    c64 = c[src, :3].astype(np.float64)
    t2 = np.float64(tol) * np.float64(tol)
    comp = np.full(len(src), -1, np.int64)
    for seed in range(len(src)):
        if comp[seed] >= 0:
            continue
        comp[seed] = seed
        stack = [seed]
        while stack:
            d = c64[stack.pop()][None, :] - c64
            near = np.flatnonzero(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= t2) & (comp < 0))
            comp[near] = seed
            stack.extend(near.tolist())
    return _object_finish(c, voted, g, comp if len(src) else None, min_size, max_size, max_extent, remove_ratio, revert_ratio, min_voted, ground_keep)


# ---- k nearest neighbours, radius counts and the density filters (include/erasor_hip.h: erasor_hip_knn_* / _radius_count_* /
# _density_filter_*; kernels: erasor_amd/csrc/knn.hip.h), on the host ---------------------------------------------------------------
# The host restatement of the device's contract.  Distance: d2 = (ex*ex + ey*ey) + ez*ez in float64 with ex = float64(x_i) - float64(x_j),
# d = sqrt(d2).  The neighbour order of point i: every j != i by (d2, j) ascending; self is excluded by index, so an identical point at
# another index is a neighbour at distance 0.  A point with fewer than k other points gets KNN_NONE / +inf padding and infinite scores.
KNN_NONE = 0xFFFFFFFF
KNN_MAX_K = 32
SCORE_STATS_FIELDS = ("n_scored", "min", "median", "p90", "p99", "max")
DENSITY_SCORES = {"kth": 0, "mean": 1, "count": 2}  # ERASOR_DENSITY_KTH / _MEAN / _COUNT
DENSITY_RULES = {"abs": 0, "mad": 1}                # ERASOR_DENSITY_ABS / _MAD
DENSITY_RESULT_FIELDS = ("n_points", "n_kept", "n_removed", "n_removed_dynamic", "n_removed_static", "n_short", "n_scored", "m", "mad", "thr",
                         "min", "median", "p90", "p99", "max")


def _knn_cloud(cloud, who):
    c = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 4))
    if len(c) > 1 << 30:
        raise ValueError(who + ": more than 2^30 points")
    if not np.isfinite(c[:, :3]).all():
        raise ValueError(who + ": non-finite coordinate")
    return c


def _check_k(k, who):
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= KNN_MAX_K):
        raise ValueError(who + ": k must be within 1 .. 32")
    return int(k)


def _check_radius(r, who):
    if not (np.isfinite(r) and r > 0):
        raise ValueError(who + ": radius must be a finite number > 0")
    return float(r)


def pair_d2(a64, b64):
    """the squared distance, operation by operation: float64 (..., 3) arrays that broadcast"""
    e = a64 - b64
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def score_stats(score):
    """min / median / p90 / p99 / max over the finite scores, as overlap() takes them; NaN when there are none"""
    s = np.asarray(score, np.float64).reshape(-1)
    f = s[np.isfinite(s)]
    if len(f) == 0:
        nan = float("nan")
        return {"n_scored": 0, "min": nan, "median": nan, "p90": nan, "p99": nan, "max": nan}
    return {"n_scored": int(len(f)), "min": float(f.min()), "median": float(np.median(f)), "p90": float(np.percentile(f, 90)),
            "p99": float(np.percentile(f, 99)), "max": float(f.max())}


def _knn_rows_brute(c64, rows, k):
    """(idx, d2) of the first k neighbours of every point in `rows`, every pair by the predicate: (len(rows), k), padded"""
    n = len(c64)
    idx = np.full((len(rows), k), KNN_NONE, np.uint32)
    d2o = np.full((len(rows), k), np.inf)
    m = min(k, n - 1)
    for lo in range(0, len(rows), 256):  # (row blocks: 256 x n distances at a time)
        r = rows[lo:lo + 256]
        d2 = pair_d2(c64[r, None, :], c64[None, :, :])
        d2[np.arange(len(r)), r] = np.inf  # (self, by index: no real d2 is infinite, so it sorts last)
        order = np.argsort(d2, axis=1, kind="stable")[:, :m]  # (stable: equal d2 in index order)
        idx[lo:lo + len(r), :m] = order
        d2o[lo:lo + len(r), :m] = np.take_along_axis(d2, order, 1)
    return idx, d2o


def _knn_finish(c, k, idx, d2, neighbours):
    n = len(c)
    d = np.sqrt(d2)
    total = np.zeros(n)
    for e in range(k):  # (((0.0 + d_0) + d_1) + ...): in list order
        total = total + d[:, e]
    short = n - 1 < k
    kth = d[:, k - 1].copy() if n else np.zeros(0)
    mean = total / np.float64(k)
    out = {"n_points": int(n), "n_short": int(n if short else 0), "k": int(k), "kth": kth, "mean": mean, "kth_stats": score_stats(kth),
           "mean_stats": score_stats(mean)}
    if neighbours:
        out["nbr_idx"] = idx
        out["nbr_dist"] = d
    return out


def knn_brute(cloud, k, neighbours=False):
    """knn() with every pair tested by the predicate in numpy (no tree): for a few thousand points"""
    c = _knn_cloud(cloud, "knn")
    k = _check_k(k, "knn")
    idx, d2 = _knn_rows_brute(c[:, :3].astype(np.float64), np.arange(len(c)), k)
    return _knn_finish(c, k, idx, d2, neighbours)


def knn(cloud, k, neighbours=False):
    """Every point's k nearest other points inside `cloud` (XYZI rows), 1 <= k <= 32.  cKDTree.query(k + 10) only proposes candidates;
    they are re-ranked by (d2, j) with the float64 predicate, and a row whose last candidate is not strictly beyond its k-th neighbour
    (ties, duplicates) is redone over every pair.  Returns a dict: n_points, n_short, k, kth and mean (float64 per point), kth_stats and
    mean_stats (SCORE_STATS_FIELDS), and with neighbours=True nbr_idx (n, k) uint32 / nbr_dist (n, k) float64, padded with KNN_NONE /
    +inf where a point has fewer than k other points."""
    c = _knn_cloud(cloud, "knn")
    k = _check_k(k, "knn")
    n = len(c)
    c64 = c[:, :3].astype(np.float64)
    kk = min(k + 10, n)
    if n - 1 <= k or kk == n:  # (every other point is a candidate anyway)
        idx, d2 = _knn_rows_brute(c64, np.arange(n), k)
        return _knn_finish(c, k, idx, d2, neighbours)
    dist, cand = cKDTree(c64).query(c64, k=kk, workers=-1)
    me = np.arange(n)[:, None]
    d2 = pair_d2(c64[:, None, :], c64[cand])
    d2[cand == me] = np.inf
    cand = np.where(cand == me, KNN_NONE, cand).astype(np.int64)
    by_j = np.argsort(cand, axis=1, kind="stable")
    cand, d2 = np.take_along_axis(cand, by_j, 1), np.take_along_axis(d2, by_j, 1)
    by_d = np.argsort(d2, axis=1, kind="stable")
    cand, d2 = np.take_along_axis(cand, by_d, 1)[:, :k], np.take_along_axis(d2, by_d, 1)[:, :k]
    # every point outside the candidates is at least as far as the tree's last one; its own float64 distances are a few ulps off the
    # predicate's, 1e-9 relative is far above that
    far = dist[:, -1] * dist[:, -1] * (1 - 1e-9)
    redo = np.flatnonzero(~(d2[:, k - 1] < far))
    idx = cand.astype(np.uint32)
    if len(redo):
        idx[redo], d2[redo] = _knn_rows_brute(c64, redo, k)
    return _knn_finish(c, k, idx, d2, neighbours)


def radius_count_brute(cloud, r):
    """radius_count() with every pair tested by the predicate in numpy (no tree)"""
    c = _knn_cloud(cloud, "radius_count")
    r = _check_radius(r, "radius_count")
    c64 = c[:, :3].astype(np.float64)
    r2 = np.float64(r) * np.float64(r)
    cnt = np.zeros(len(c), np.uint32)
    for lo in range(0, len(c), 256):
        within = pair_d2(c64[lo:lo + 256, None, :], c64[None, :, :]) <= r2
        cnt[lo:lo + 256] = within.sum(1) - 1  # (self, by index: its d2 is 0)
    return cnt, score_stats(cnt)


def radius_count(cloud, r):
    """(count, stats): per point the number of other points with d2 <= r*r (uint32), and the counts' SCORE_STATS_FIELDS.
    cKDTree.query_pairs with a radius a hair above r only proposes the pairs; the float64 predicate decides."""
    c = _knn_cloud(cloud, "radius_count")
    r = _check_radius(r, "radius_count")
    n = len(c)
    if n == 0:
        return np.zeros(0, np.uint32), score_stats([])
    c64 = c[:, :3].astype(np.float64)
    pairs = cKDTree(c64).query_pairs(r * (1 + 1e-9), output_type="ndarray")
    ok = pair_d2(c64[pairs[:, 0]], c64[pairs[:, 1]]) <= np.float64(r) * np.float64(r)
    cnt = (np.bincount(pairs[ok, 0], minlength=n) + np.bincount(pairs[ok, 1], minlength=n)).astype(np.uint32)
    return cnt, score_stats(cnt)


def density_threshold(score, rule, thr=None, mul=None):
    """(keep, m, mad, thr) of the KTH / MEAN filters over `score` (float64, +inf where a point has no score).  "abs": keep iff score <=
    thr.  "mad": m = the median of the finite scores, mad = the median of |score - m| over them, thr = m + mul * (1.4826 * mad).  An
    infinite score is never kept and a NaN thr keeps nothing."""
    s = np.asarray(score, np.float64).reshape(-1)
    nan = np.float64("nan")
    m = mad = nan
    if rule == "abs":
        if not (np.isfinite(thr) and thr >= 0):
            raise ValueError("density_filter: thr must be a finite number >= 0")
        t = np.float64(thr)
    elif rule == "mad":
        if not (np.isfinite(mul) and mul >= 0):
            raise ValueError("density_filter: mul must be a finite number >= 0")
        f = s[np.isfinite(s)]
        t = nan
        if len(f):
            m = np.median(f)
            mad = np.median(np.abs(f - m))
            with np.errstate(over="ignore"):
                t = m + np.float64(mul) * (np.float64(1.4826) * mad)
    else:
        raise ValueError("density_filter: unknown rule")
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(s) & (s <= t)
    return keep, float(m), float(mad), float(t)


def density_filter(cloud, score="mean", k=16, radius=0.5, rule="mad", thr=0.5, mul=2.0, min_neighbors=2, keep=True):
    """The cloud filtered by its density.  score "kth" / "mean" (of knn(cloud, k)) with rule "abs" (thr) or "mad" (mul), see
    density_threshold; score "count" (of radius_count(cloud, radius)): keep iff count >= min_neighbors.  Returns (mask, kept, result):
    uint8 per point, the kept rows in the order given (None unless keep), and a dict with DENSITY_RESULT_FIELDS."""
    c = _knn_cloud(cloud, "density_filter")
    if score not in DENSITY_SCORES:
        raise ValueError("density_filter: unknown score")
    if rule not in DENSITY_RULES:
        raise ValueError("density_filter: unknown rule")
    n = len(c)
    nan = float("nan")
    if score == "count":
        r = _check_radius(radius, "density_filter")
        cnt, st = radius_count(c, r)
        ok = cnt >= np.uint64(min_neighbors)
        m = mad = nan
        t = float(min_neighbors)
        n_short = 0
    else:
        k = _check_k(k, "density_filter")
        if rule == "abs" and not (np.isfinite(thr) and thr >= 0):
            raise ValueError("density_filter: thr must be a finite number >= 0")
        if rule == "mad" and not (np.isfinite(mul) and mul >= 0):
            raise ValueError("density_filter: mul must be a finite number >= 0")
        q = knn(c, k)
        st = q[score + "_stats"]
        n_short = q["n_short"]
        ok, m, mad, t = density_threshold(q[score], rule, thr, mul)
    dyn = _decode(c[:, 3])[2]
    res = {"n_points": int(n), "n_kept": int(ok.sum()), "n_removed": int(n - ok.sum()), "n_removed_dynamic": int((~ok & dyn).sum()),
           "n_removed_static": int((~ok & ~dyn).sum()), "n_short": int(n_short), "n_scored": st["n_scored"], "m": m, "mad": mad, "thr": t,
           "min": st["min"], "median": st["median"], "p90": st["p90"], "p99": st["p99"], "max": st["max"]}
    return ok.astype(np.uint8), (c[ok].copy() if keep else None), res


# ---- surface normals, curvature and eigenvalues (include/erasor_hip.h: erasor_hip_normals_*; kernel: erasor_amd/csrc/normals.hip.h),
# on the host ----------------------------------------------------------------------------------------------------------------------
# The host restatement of the device's contract; include/erasor_hip.h states it in full.  Float64 on the float32 coordinates, one IEEE
# operation at a time: the neighbourhood is the point itself and then its k nearest others in knn's order; the centroid and the six
# covariance entries are summed in that order and divided by m = k + 1; _jacobi3 solves; the eigenvalues ascend by (value, column).
NORMALS_MIN_K = 2
NORMALS_RESULT_FIELDS = ("n_points", "n_short", "n_degenerate", "n_ambiguous", "n_flipped")


def _check_normals_args(k, viewpoint, who):
    if not (isinstance(k, (int, np.integer)) and NORMALS_MIN_K <= k <= KNN_MAX_K):
        raise ValueError(who + ": k must be within 2 .. 32")
    if viewpoint is None:
        return int(k), None
    v = np.asarray(viewpoint, np.float64).reshape(-1)
    if len(v) != 3 or not np.isfinite(v).all():
        raise ValueError(who + ": viewpoint must be three finite numbers")
    return int(k), (float(v[0]), float(v[1]), float(v[2]))


def _jacobi3(A):
    """cyclic Jacobi on the symmetric 3x3 A (lists of Python floats, changed in place): pivots (0,1) (0,2) (1,2) with _jacobi4's rotation,
    a pivot that is exactly zero skipped, until every element above the diagonal is exactly zero before a sweep, or 32 sweeps.  Returns
    V (columns: eigenvectors); the eigenvalues are A's diagonal"""
    from math import sqrt
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(32):
        if A[0][1] == 0.0 and A[0][2] == 0.0 and A[1][2] == 0.0:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                theta = _ieee_div(A[q][q] - A[p][p], 2.0 * apq)
                at = -theta if theta < 0.0 else theta
                t = _ieee_div(1.0, at + sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = _ieee_div(1.0, sqrt(t * t + 1.0))
                s = t * c
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                A[p][q] = 0.0
                for i in range(3):
                    for j in range(i + 1, 3):
                        A[j][i] = A[i][j]
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return V


def _normals_result(n, k, n_short, n_degenerate, n_ambiguous, n_flipped, curvature):
    return {"n_points": int(n), "n_short": int(n_short), "n_degenerate": int(n_degenerate), "n_ambiguous": int(n_ambiguous),
            "n_flipped": int(n_flipped), "k": int(k), "curvature_stats": score_stats(curvature)}


def normals_brute(cloud, k, viewpoint=None):
    """normals() in pure Python floats, one point at a time, over all-pairs neighbour lists: for a few hundred points"""
    c = _knn_cloud(cloud, "normals")
    k, view = _check_normals_args(k, viewpoint, "normals")
    n, m = len(c), float(k + 1)
    nan = float("nan")
    nrm, curv, eig = np.full((n, 3), nan), np.full(n, nan), np.full((n, 3), nan)
    c64 = c[:, :3].astype(np.float64)
    n_deg = n_amb = n_flip = 0
    if n - 1 < k:
        return nrm.astype(np.float32), curv, eig, _normals_result(n, k, n, 0, 0, 0, curv)
    idx, _ = _knn_rows_brute(c64, np.arange(n), k)
    P = c64.tolist()
    for i in range(n):
        hood = [P[i]] + [P[j] for j in idx[i].tolist()]
        sx = sy = sz = 0.0
        for p in hood:
            sx, sy, sz = sx + p[0], sy + p[1], sz + p[2]
        cx, cy, cz = sx / m, sy / m, sz / m
        xx = xy = xz = yy = yz = zz = 0.0
        for p in hood:
            ex, ey, ez = p[0] - cx, p[1] - cy, p[2] - cz
            xx, xy, xz, yy, yz, zz = xx + ex * ex, xy + ex * ey, xz + ex * ez, yy + ey * ey, yz + ey * ez, zz + ez * ez
        xx, xy, xz, yy, yz, zz = xx / m, xy / m, xz / m, yy / m, yz / m, zz / m
        tr = (xx + yy) + zz
        if not tr > 0:
            n_deg += 1
            continue
        A = [[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]
        V = _jacobi3(A)
        col = sorted(range(3), key=lambda j: (A[j][j], j))
        l0, l1, l2 = (A[j][j] for j in col)
        nx, ny, nz = V[0][col[0]], V[1][col[0]], V[2][col[0]]
        n_amb += l0 == l1
        if view is None:
            flip = nz < 0 or (nz == 0 and (ny < 0 or (ny == 0 and nx < 0)))
        else:
            flip = ((view[0] - P[i][0]) * nx + (view[1] - P[i][1]) * ny) + (view[2] - P[i][2]) * nz < 0
        if flip:
            nx, ny, nz = -nx, -ny, -nz
            n_flip += 1
        nrm[i], curv[i], eig[i] = (nx, ny, nz), abs(l0) / tr, (l0, l1, l2)
    return nrm.astype(np.float32), curv, eig, _normals_result(n, k, 0, n_deg, n_amb, n_flip, curv)


def _jacobi3_rows(a, live):
    """_jacobi3 on every row at once: a = [a00, a01, a02, a11, a12, a22] (float64 arrays, changed in place), only where `live`.  The same
    operations element by element; a row whose pivot is exactly zero, or whose off-diagonals all were before the sweep, keeps its
    values.  Returns the nine entries of V, row-major"""
    n = len(a[0])
    v = [np.ones(n) if j in (0, 4, 8) else np.zeros(n) for j in range(9)]
    # per pivot: (app, aqq, apq, apr, aqr) in a, and the columns p and q of V
    pivots = (((0, 3, 1, 2, 4), (0, 1)), ((0, 5, 2, 1, 4), (0, 2)), ((3, 5, 4, 1, 2), (1, 2)))
    with np.errstate(all="ignore"):
        for _ in range(32):
            active = live & ~((a[1] == 0.0) & (a[2] == 0.0) & (a[4] == 0.0))
            if not active.any():
                break
            for (pp, qq, pq, pr, qr), (p, q) in pivots:
                app, aqq, apq, apr, aqr = a[pp], a[qq], a[pq], a[pr], a[qr]
                do = active & (apq != 0.0)
                theta = (aqq - app) / (2.0 * apq)
                at = np.where(theta < 0.0, -theta, theta)
                t = 1.0 / (at + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                bpp, bpq = c * app - s * apq, s * app + c * apq  # A <- A J
                bqp, bqq = c * apq - s * aqq, s * apq + c * aqq
                a[pp] = np.where(do, c * bpp - s * bqp, app)     # A <- Jt A
                a[qq] = np.where(do, s * bpq + c * bqq, aqq)
                a[pq] = np.where(do, 0.0, apq)
                a[pr] = np.where(do, c * apr - s * aqr, apr)
                a[qr] = np.where(do, s * apr + c * aqr, aqr)
                for row in range(3):                             # V <- V J
                    vp, vq = v[3 * row + p], v[3 * row + q]
                    v[3 * row + p] = np.where(do, c * vp - s * vq, vp)
                    v[3 * row + q] = np.where(do, s * vp + c * vq, vq)
    return v


def normals(cloud, k, viewpoint=None):
    """Every point's surface normal, curvature and covariance eigenvalues from itself and its k nearest other points inside `cloud` (XYZI
    rows), 2 <= k <= 32; viewpoint: three finite numbers the normals are turned towards, or None for "up".  knn() gives the neighbour
    lists; the arithmetic is element-wise numpy float64 over all points at once, sequential over the neighbour index.  Returns (normals
    (n, 3) float32, curvature (n,) float64, eigenvalues (n, 3) float64 ascending, result): result has NORMALS_RESULT_FIELDS, k and
    curvature_stats (SCORE_STATS_FIELDS over the finite curvatures).  Short and degenerate points are NaN."""
    c = _knn_cloud(cloud, "normals")
    k, view = _check_normals_args(k, viewpoint, "normals")
    n, m = len(c), np.float64(k + 1)
    if n - 1 < k:
        curv = np.full(n, np.nan)
        return np.full((n, 3), np.nan, np.float32), curv, np.full((n, 3), np.nan), _normals_result(n, k, n, 0, 0, 0, curv)
    nb = knn(c, k, True)["nbr_idx"].astype(np.int64)
    c64 = c[:, :3].astype(np.float64)
    hood = [c64] + [c64[nb[:, e]] for e in range(k)]  # the point itself, then the list in its order
    s = np.zeros((n, 3))
    for p in hood:
        s = s + p
    cen = s / m
    a = [np.zeros(n) for _ in range(6)]  # xx, xy, xz, yy, yz, zz
    for p in hood:
        e = p - cen
        ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
        for j, term in enumerate((ex * ex, ex * ey, ex * ez, ey * ey, ey * ez, ez * ez)):
            a[j] = a[j] + term
    a = [x / m for x in a]
    tr = (a[0] + a[3]) + a[5]
    ok = tr > 0
    v = _jacobi3_rows(a, ok)
    d0, d1, d2 = a[0], a[3], a[5]
    r0 = (d1 < d0).astype(np.int64) + (d2 < d0)
    r1 = (d0 <= d1).astype(np.int64) + (d2 < d1)
    pick = lambda r, x0, x1, x2: np.where(r0 == r, x0, np.where(r1 == r, x1, x2))
    l0, l1, l2 = pick(0, d0, d1, d2), pick(1, d0, d1, d2), pick(2, d0, d1, d2)
    nx, ny, nz = pick(0, v[0], v[1], v[2]), pick(0, v[3], v[4], v[5]), pick(0, v[6], v[7], v[8])
    with np.errstate(all="ignore"):
        curv = np.where(ok, np.abs(l0) / tr, np.nan)
    if view is None:
        flip = (nz < 0) | ((nz == 0) & ((ny < 0) | ((ny == 0) & (nx < 0))))
    else:
        flip = ((view[0] - c64[:, 0]) * nx + (view[1] - c64[:, 1]) * ny) + (view[2] - c64[:, 2]) * nz < 0
    flip = flip & ok
    nrm = np.stack([np.where(flip, -x, x) for x in (nx, ny, nz)], 1)
    nrm[~ok] = np.nan
    eig = np.stack([l0, l1, l2], 1)
    eig[~ok] = np.nan
    return nrm.astype(np.float32), curv, eig, _normals_result(n, k, 0, (~ok).sum(), (ok & (l0 == l1)).sum(), flip.sum(), curv)


# ---- the see-through check: map points voted out by every scan's range image (include/erasor_hip.h: erasor_hip_visibility_*; kernels:
# erasor_amd/csrc/visibility.hip.h), on the host ----------------------------------------------------------------------------------
# The normative text of the contract; the device equals it byte for byte.  Float64 on the float32 coordinates, one IEEE operation at a
# time, and nothing but + - * /, sqrt and comparisons: the pixel grid is DATA, two tables of tangents made once by the caller
# (visibility_grid, or a sensor's own beam edges), so no pixel needs atan2 and its last-bit trouble at sector boundaries.
#
# The pixel of a point (x, y, z) in the lidar frame, W columns (M = W / 8 per octant) and H rows:
#   a = |x|, b = |y|; a == b == 0: ON THE AXIS, no pixel.  t = min(a, b) / max(a, b) in [0, 1]; j = the number of col_tan entries <= t
#   (col_tan: M - 1 strictly increasing tangents in (0, 1), the inner column edges of an octant; 0 <= j <= M - 1).
#   quadrant q: 0 (x >= 0, y >= 0), 1 (x < 0, y >= 0), 2 (x < 0, y < 0), 3 (x >= 0, y < 0) -- a zero of either sign is >= 0;
#   octant o = 2 q + odd with odd = (a < b) in quadrants 0 and 2, and odd = !(a < b) in quadrants 1 and 3: the octants 0 .. 7 counted
#   counter-clockwise from +x.  An even octant runs outward from an axis, t grows with the angle: column o M + j.  An odd octant runs
#   towards an axis, t falls with the angle, it is mirrored: column o M + (M - 1) - j.  So the columns 0 .. W - 1 follow each other
#   once round the circle, and a direction on an edge belongs to exactly one of them.
#   s = z / sqrt(x*x + y*y); row = (the number of row_tan entries <= s) - 1 (row_tan: H + 1 strictly increasing finite tangents, the row
#   edges from the bottom); a row outside 0 .. H - 1 is OUT OF VIEW.
#   range rho = sqrt((x*x + y*y) + z*z).
# The gates, in this order: non-finite coordinate, on the axis, rho outside [min_range, max_range], out of view.
VISIBILITY_EMPTY = 0xFFFFFFFF
VISIBILITY_MAX_FRAMES = 65535
VISIBILITY_ROW_FIELDS = ("n_points", "n_non_finite", "n_on_axis", "n_out_of_range", "n_out_of_view", "n_pixels", "n_map_in_view", "n_hit",
                         "n_occluded", "n_no_return", "n_through", "n_grazing")
VISIBILITY_RESULT_FIELDS = ("n_points", "n_never_in_view", "n_kept", "n_removed", "n_removed_dynamic", "n_removed_static", "n_map_no_normal",
                            "n_in_view", "n_hit", "n_occluded", "n_no_return", "n_through", "n_grazing")
VISIBILITY_DEFAULTS = {"min_range": 0.5, "max_range": 80.0, "margin_abs": 0.2, "margin_rel": 0.01, "window": 1, "k": 0, "min_cos": 0.25,
                       "min_through": 2, "hit_weight": 1.0}
VIS_HIT, VIS_OCCLUDED, VIS_NO_RETURN, VIS_THROUGH, VIS_GRAZING, VIS_NOT_IN_VIEW = 0, 1, 2, 3, 4, 5
_VIS_OK, _VIS_NON_FINITE, _VIS_AXIS, _VIS_RANGE, _VIS_VIEW = 0, 1, 2, 3, 4


def visibility_grid(width, height, el_bottom_deg, el_top_deg):
    """The two edge tables of a uniform grid: `width` columns of equal azimuth (a multiple of 8), `height` rows of equal elevation between
    el_bottom_deg and el_top_deg.  col_tan[k - 1] = tan(((pi / 4) * k) / M) for k = 1 .. M - 1, M = width / 8; row_tan[i] =
    tan((((top - bottom) * i) / H + bottom) * (pi / 180)) for i = 0 .. H -- the driver forms them by the same expressions with C's tan."""
    import math
    W, H = int(width), int(height)
    if W % 8 or not 8 <= W <= 4096 or not 1 <= H <= 256:
        raise ValueError("visibility_grid: width must be a multiple of 8 within 8 .. 4096, height within 1 .. 256")
    M = W // 8
    col = np.array([math.tan(((math.pi / 4.0) * k) / M) for k in range(1, M)], np.float64)
    row = np.array([math.tan((((float(el_top_deg) - float(el_bottom_deg)) * i) / H + float(el_bottom_deg)) * (math.pi / 180.0)) for i in range(H + 1)],
                   np.float64)
    return check_visibility_grid({"width": W, "height": H, "col_tan": col, "row_tan": row})


def check_visibility_grid(grid):
    W, H = int(grid["width"]), int(grid["height"])
    col = np.ascontiguousarray(grid["col_tan"], np.float64).reshape(-1)
    row = np.ascontiguousarray(grid["row_tan"], np.float64).reshape(-1)
    if W % 8 or not 8 <= W <= 4096:
        raise ValueError("visibility: width must be a multiple of 8 within 8 .. 4096")
    if not 1 <= H <= 256:
        raise ValueError("visibility: height must be within 1 .. 256")
    if len(col) != W // 8 - 1 or len(row) != H + 1:
        raise ValueError("visibility: col_tan has width / 8 - 1 entries and row_tan height + 1")
    if not ((col > 0) & (col < 1)).all() or not (np.diff(col) > 0).all():
        raise ValueError("visibility: col_tan must be strictly increasing within (0, 1)")
    if not np.isfinite(row).all() or not (np.diff(row) > 0).all():
        raise ValueError("visibility: row_tan must be finite and strictly increasing")
    return {"width": W, "height": H, "col_tan": col, "row_tan": row}


def visibility_column(x, y, col_tan, width):
    """the column of the direction (x, y), or -1 on the axis: THE pixel mapping, written down once (float64 arrays)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    M = int(width) // 8
    a, b = np.abs(x), np.abs(y)
    swap = a < b
    lo, hi = np.where(swap, a, b), np.where(swap, b, a)
    axis = hi == 0
    with np.errstate(all="ignore"):
        t = lo / np.where(axis, 1.0, hi)
    j = np.searchsorted(col_tan, t, side="right").astype(np.int64)  # the number of entries <= t
    sx, sy = x < 0, y < 0
    q = np.where(sx, np.where(sy, 2, 1), np.where(sy, 3, 0))
    odd = np.where((q & 1) == 1, ~swap, swap).astype(np.int64)
    o = 2 * q + odd
    return np.where(axis, -1, np.where(odd == 1, o * M + (M - 1) - j, o * M + j))


def _vis_pixels(x, y, z, finite, grid, min_range, max_range):
    """(gate, rho, column, row) of points in a lidar frame (float64 arrays): gate is _VIS_OK or the first gate that rejects"""
    W, H = grid["width"], grid["height"]
    with np.errstate(all="ignore"):
        x, y, z = (np.where(finite, v, 1.0) for v in (x, y, z))
        col = visibility_column(x, y, grid["col_tan"], W)
        xy = x * x + y * y
        rho = np.sqrt(xy + z * z)
        s = z / np.sqrt(np.where(col < 0, 1.0, xy))
    row = np.searchsorted(grid["row_tan"], s, side="right").astype(np.int64) - 1
    gate = np.full(len(x), _VIS_OK, np.int64)
    gate[(row < 0) | (row >= H)] = _VIS_VIEW
    gate[~((rho >= min_range) & (rho <= max_range))] = _VIS_RANGE
    gate[col < 0] = _VIS_AXIS
    gate[~finite] = _VIS_NON_FINITE
    return gate, rho, col, row


def visibility_transforms(T_body2origin, T_lidar2body=None):
    """Every frame's map-to-lidar transform in float64, the rigid inverse of T_body2origin[f] . T_lidar2body (their upper three rows, the
    float32 entries widened), every sum in index order: M[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j], and + A[i][3] in
    column 3; the inverse's rotation is M's transposed and its translation -((M[0][i] M[0][3] + M[1][i] M[1][3]) + M[2][i] M[2][3]).
    Returns (m [n, 12]: per row r0, r1, r2, t; origin [n, 3]: the lidar's origin in the map frame).  ValueError on a non-finite entry."""
    A = np.asarray(T_body2origin, np.float32).reshape(-1, 4, 4).astype(np.float64)
    B = (np.eye(4, dtype=np.float32) if T_lidar2body is None else np.asarray(T_lidar2body, np.float32).reshape(4, 4)).astype(np.float64)
    n = len(A)
    M = np.zeros((n, 3, 4))
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(4):
                v = (A[:, i, 0] * B[0, j] + A[:, i, 1] * B[1, j]) + A[:, i, 2] * B[2, j]
                M[:, i, j] = v + A[:, i, 3] if j == 3 else v
        m = np.zeros((n, 12))
        for i in range(3):
            for j in range(3):
                m[:, 4 * i + j] = M[:, j, i]
            m[:, 4 * i + 3] = -((M[:, 0, i] * M[:, 0, 3] + M[:, 1, i] * M[:, 1, 3]) + M[:, 2, i] * M[:, 2, 3])
    if not (np.isfinite(m).all() and np.isfinite(M).all()):
        raise ValueError("visibility: non-finite frame transform")
    return m, M[:, :, 3].copy()


def visibility_decide(votes, min_through, hit_weight):
    """the points removed (bool): through >= min_through and (double)through > hit_weight * (double)hit"""
    v = np.asarray(votes).reshape(-1, 4)
    th, hit = v[:, 2].astype(np.float64), v[:, 1].astype(np.float64)
    return (v[:, 2].astype(np.int64) >= int(min_through)) & (th > np.float64(hit_weight) * hit)


def _vis_args(map_xyzi, scans, grid, min_range, max_range, margin_abs, margin_rel, window, k, min_cos, min_through, hit_weight):
    if grid is None:
        raise ValueError("visibility: a grid is needed (visibility_grid)")
    g = check_visibility_grid(grid)
    if not (np.isfinite(min_range) and np.isfinite(max_range) and 0 <= min_range < max_range):
        raise ValueError("visibility: 0 <= min_range < max_range, both finite")
    if not (np.isfinite(margin_abs) and np.isfinite(margin_rel) and margin_abs >= 0 and margin_rel >= 0):
        raise ValueError("visibility: the margins must be finite numbers >= 0")
    if window not in (0, 1, 2):
        raise ValueError("visibility: window must be 0, 1 or 2")
    if not (k == 0 or NORMALS_MIN_K <= k <= KNN_MAX_K):
        raise ValueError("visibility: k must be 0 or within 2 .. 32")
    if not (np.isfinite(min_cos) and np.isfinite(hit_weight) and hit_weight >= 0):
        raise ValueError("visibility: min_cos must be finite and hit_weight a finite number >= 0")
    if not 0 <= int(min_through) <= 0xFFFFFFFF:
        raise ValueError("visibility: min_through must fit 32 bits")
    if len(scans) > VISIBILITY_MAX_FRAMES:
        raise ValueError("visibility: more than 65535 frames")
    c = np.ascontiguousarray(np.asarray(map_xyzi, np.float32).reshape(-1, 4))
    if k and not np.isfinite(c[:, :3]).all():
        raise ValueError("visibility: non-finite coordinate in the map (the normals need a finite cloud)")
    return g, c


def _vis_finish(c, votes, rows, n_no_normal, min_through, hit_weight, keep):
    rem = visibility_decide(votes, min_through, hit_weight)
    dyn = _decode(c[:, 3])[2]
    res = {"n_points": int(len(c)), "n_never_in_view": int((votes[:, 0] == 0).sum()), "n_kept": int((~rem).sum()), "n_removed": int(rem.sum()),
           "n_removed_dynamic": int((rem & dyn).sum()), "n_removed_static": int((rem & ~dyn).sum()), "n_map_no_normal": int(n_no_normal)}
    for key, src in (("n_in_view", "n_map_in_view"), ("n_hit", "n_hit"), ("n_occluded", "n_occluded"), ("n_no_return", "n_no_return"),
                     ("n_through", "n_through"), ("n_grazing", "n_grazing")):
        res[key] = int(sum(r[src] for r in rows))
    return votes, (~rem).astype(np.uint8), (c[~rem].copy() if keep else None), rows, res


def visibility_verdicts(map_xyzi, scans, T_body2origin, T_lidar2body=None, grid=None, min_range=0.5, max_range=80.0, margin_abs=0.2, margin_rel=0.01,
                        window=1, k=0, min_cos=0.25, min_through=2, hit_weight=1.0):
    """the verdict of every (frame, map point) pair, VIS_* codes as uint8 [n_frames, n_map], and every frame's range image [n_frames, H, W]
    uint32: what visibility() counts, for the tests and for looking at one frame"""
    g, c = _vis_args(map_xyzi, scans, grid, min_range, max_range, margin_abs, margin_rel, window, k, min_cos, min_through, hit_weight)
    W, H, w = g["width"], g["height"], int(window)
    m, org = visibility_transforms(np.zeros((0, 4, 4), np.float32) if len(scans) == 0 else T_body2origin, T_lidar2body)
    if len(m) != len(scans):
        raise ValueError("visibility: one T_body2origin per frame")
    nrm = normals(c, int(k))[0].astype(np.float64) if k else None
    p = c[:, :3].astype(np.float64)
    pfin = np.isfinite(c[:, :3]).all(1)
    verd = np.full((len(scans), len(c)), VIS_NOT_IN_VIEW, np.uint8)
    imgs = np.full((len(scans), H, W), VISIBILITY_EMPTY, np.uint32)
    drops = np.zeros((len(scans), 5), np.int64)
    for f, scan in enumerate(scans):
        s = np.asarray(scan, np.float32).reshape(-1, 4)[:, :3]
        s64 = s.astype(np.float64)
        gate, rho, col, row = _vis_pixels(s64[:, 0], s64[:, 1], s64[:, 2], np.isfinite(s).all(1), g, min_range, max_range)
        ok = gate == _VIS_OK
        drops[f] = [len(s)] + [int((gate == code).sum()) for code in (_VIS_NON_FINITE, _VIS_AXIS, _VIS_RANGE, _VIS_VIEW)]
        with np.errstate(over="ignore"):
            bits = rho[ok].astype(np.float32).view(np.uint32)
        np.minimum.at(imgs[f].reshape(-1), row[ok] * W + col[ok], bits)  # (non-negative floats order as their bits)
        # the map in this frame
        with np.errstate(all="ignore"):
            px, py, pz = (np.where(pfin, p[:, a], 0.0) for a in range(3))
            q = [((m[f, 4 * r] * px + m[f, 4 * r + 1] * py) + m[f, 4 * r + 2] * pz) + m[f, 4 * r + 3] for r in range(3)]
        gate, rho, col, row = _vis_pixels(q[0], q[1], q[2], pfin, g, min_range, max_range)
        iv = np.flatnonzero(gate == _VIS_OK)
        rho, col, row = rho[iv], col[iv], row[iv]
        mg = margin_abs + margin_rel * rho
        lo, hi = rho - mg, rho + mg
        hit = np.zeros(len(iv), bool)
        occ = np.zeros(len(iv), bool)
        some = np.zeros(len(iv), bool)
        for dr in range(-w, w + 1):
            rr = row + dr
            inr = (rr >= 0) & (rr < H)
            for dc in range(-w, w + 1):
                cc = (col + dc) % W
                b = imgs[f][np.where(inr, rr, 0), cc]
                full = inr & (b != VISIBILITY_EMPTY)
                r = b.view(np.float32).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    hit |= full & (lo <= r) & (r <= hi)
                    occ |= full & (r < lo)
                some |= full
        v = np.where(hit, VIS_HIT, np.where(occ, VIS_OCCLUDED, np.where(~some, VIS_NO_RETURN, VIS_THROUGH))).astype(np.uint8)
        if k:
            d = p[iv] - org[f]
            n = nrm[iv]
            with np.errstate(invalid="ignore"):
                dot = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
                vv = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                graze = (v == VIS_THROUGH) & ~np.isnan(n[:, 0]) & (np.abs(dot) < min_cos * np.sqrt(vv))
            v[graze] = VIS_GRAZING
        verd[f, iv] = v
    return verd, imgs, drops, (int(np.isnan(nrm[:, 0]).sum()) if k else 0), c


def _vis_rows(verd, imgs, drops):
    return [dict(zip(VISIBILITY_ROW_FIELDS, [int(x) for x in drops[f]] + [int((imgs[f] != VISIBILITY_EMPTY).sum()), int((verd[f] != VIS_NOT_IN_VIEW).sum())] +
                     [int((verd[f] == code).sum()) for code in (VIS_HIT, VIS_OCCLUDED, VIS_NO_RETURN, VIS_THROUGH, VIS_GRAZING)])) for f in range(len(verd))]


def visibility(map_xyzi, scans, T_body2origin, T_lidar2body=None, grid=None, min_range=0.5, max_range=80.0, margin_abs=0.2, margin_rel=0.01,
               window=1, k=0, min_cos=0.25, min_through=2, hit_weight=1.0, keep=True):
    """The see-through check (Erasor.visibility): a map point that later scans look straight through was not static.  Every scan (XYZI
    rows in the lidar frame, taken as given) becomes an H x W range image: per pixel the smallest float32 range of the points that pass
    the gates.  Every map point is put into every frame by visibility_transforms; where it passes the gates it is IN VIEW, and with m =
    margin_abs + margin_rel * rho the non-empty pixels r (as float64) of the (2 window + 1)^2 pixels around its own -- columns wrap, rows
    clip -- give its verdict, in this priority: HIT (some rho - m <= r <= rho + m), OCCLUDED (some r < rho - m), NO RETURN (all empty:
    no evidence), THROUGH (every r > rho + m).  With k > 0 a THROUGH is demoted to GRAZING (no evidence) when |n . v| < min_cos *
    sqrt(v . v), v = p - the lidar's origin in the map frame and n the point's float32 normal from normals(map, k); a NaN normal gates
    nothing.  A point is removed iff through >= min_through and through > hit_weight * hit.
    Returns (votes [n, 4] uint16: in_view, hit, through, occluded; mask uint8, 1 = kept; the kept rows in the order given or None;
    a row per frame with VISIBILITY_ROW_FIELDS; a dict with VISIBILITY_RESULT_FIELDS)."""
    verd, imgs, drops, n_no_normal, c = visibility_verdicts(map_xyzi, scans, T_body2origin, T_lidar2body, grid, min_range, max_range, margin_abs,
                                                            margin_rel, window, k, min_cos, min_through, hit_weight)
    votes = np.stack([(verd != VIS_NOT_IN_VIEW).sum(0), (verd == VIS_HIT).sum(0), (verd == VIS_THROUGH).sum(0), (verd == VIS_OCCLUDED).sum(0)],
                     1).astype(np.uint16).reshape(-1, 4)
    return _vis_finish(c, votes, _vis_rows(verd, imgs, drops), n_no_normal, min_through, hit_weight, keep)


def visibility_brute(map_xyzi, scans, T_body2origin, T_lidar2body=None, grid=None, min_range=0.5, max_range=80.0, margin_abs=0.2, margin_rel=0.01,
                     window=1, k=0, min_cos=0.25, min_through=2, hit_weight=1.0, keep=True):
    """visibility() point by point in plain Python floats (math.sqrt, bisect), for small inputs: the check of the vectorised text"""
    import bisect
    import math
    g, c = _vis_args(map_xyzi, scans, grid, min_range, max_range, margin_abs, margin_rel, window, k, min_cos, min_through, hit_weight)
    W, H, w, M = g["width"], g["height"], int(window), g["width"] // 8
    ct, rt = [float(v) for v in g["col_tan"]], [float(v) for v in g["row_tan"]]
    m, org = visibility_transforms(np.zeros((0, 4, 4), np.float32) if len(scans) == 0 else T_body2origin, T_lidar2body)
    nrm = normals_brute(c, int(k))[0] if k else None

    def pixel(x, y, z):
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            return _VIS_NON_FINITE, 0.0, 0, 0
        a, b = abs(x), abs(y)
        if a == 0 and b == 0:
            return _VIS_AXIS, 0.0, 0, 0
        xy = x * x + y * y
        rho = math.sqrt(xy + z * z)
        if not (min_range <= rho <= max_range):
            return _VIS_RANGE, rho, 0, 0
        swap = a < b
        t = (a / b) if swap else (b / a)
        j = bisect.bisect_right(ct, t)
        q = (2 if y < 0 else 1) if x < 0 else (3 if y < 0 else 0)
        odd = (not swap) if q & 1 else swap
        o = 2 * q + (1 if odd else 0)
        col = o * M + (M - 1) - j if odd else o * M + j
        row = bisect.bisect_right(rt, z / math.sqrt(xy)) - 1
        if row < 0 or row >= H:
            return _VIS_VIEW, rho, col, row
        return _VIS_OK, rho, col, row

    votes = np.zeros((len(c), 4), np.uint16)
    rows = []
    for f, scan in enumerate(scans):
        s = np.asarray(scan, np.float32).reshape(-1, 4)
        img = [VISIBILITY_EMPTY] * (H * W)
        cnt = [0] * 5
        for x, y, z, _ in s.astype(np.float64).tolist():
            gate, rho, col, row = pixel(x, y, z)
            cnt[gate] += 1
            if gate == _VIS_OK:
                with np.errstate(over="ignore"):
                    bits = int(np.float32(rho).view(np.uint32))
                img[row * W + col] = min(img[row * W + col], bits)
        tally = [0] * 6
        mf, of = [float(v) for v in m[f]], [float(v) for v in org[f]]
        for i, (x32, y32, z32, _) in enumerate(c.astype(np.float64).tolist()):
            if not (math.isfinite(x32) and math.isfinite(y32) and math.isfinite(z32)):
                continue
            q = [((mf[4 * r] * x32 + mf[4 * r + 1] * y32) + mf[4 * r + 2] * z32) + mf[4 * r + 3] for r in range(3)]
            gate, rho, col, row = pixel(q[0], q[1], q[2])
            if gate != _VIS_OK:
                continue
            mg = margin_abs + margin_rel * rho
            lo, hi = rho - mg, rho + mg
            hit = occ = some = False
            for dr in range(-w, w + 1):
                if not 0 <= row + dr < H:
                    continue
                for dc in range(-w, w + 1):
                    b = img[(row + dr) * W + (col + dc) % W]
                    if b == VISIBILITY_EMPTY:
                        continue
                    r = float(np.uint32(b).view(np.float32))
                    some = True
                    hit = hit or lo <= r <= hi
                    occ = occ or r < lo
            v = VIS_HIT if hit else VIS_OCCLUDED if occ else VIS_NO_RETURN if not some else VIS_THROUGH
            if v == VIS_THROUGH and k:
                n = [float(t) for t in nrm[i]]
                if not math.isnan(n[0]):
                    d = [x32 - of[0], y32 - of[1], z32 - of[2]]
                    dot = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
                    if abs(dot) < min_cos * math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]):
                        v = VIS_GRAZING
            tally[5] += 1
            tally[v] += 1
            votes[i, 0] += 1
            if v == VIS_HIT:
                votes[i, 1] += 1
            elif v == VIS_THROUGH:
                votes[i, 2] += 1
            elif v == VIS_OCCLUDED:
                votes[i, 3] += 1
        rows.append(dict(zip(VISIBILITY_ROW_FIELDS, [len(s), cnt[_VIS_NON_FINITE], cnt[_VIS_AXIS], cnt[_VIS_RANGE], cnt[_VIS_VIEW],
                                                     sum(1 for b in img if b != VISIBILITY_EMPTY), tally[5], tally[VIS_HIT], tally[VIS_OCCLUDED],
                                                     tally[VIS_NO_RETURN], tally[VIS_THROUGH], tally[VIS_GRAZING]])))
    n_no_normal = int(np.isnan(nrm[:, 0]).sum()) if k else 0
    return _vis_finish(c, votes, rows, n_no_normal, min_through, hit_weight, keep)


# ---- carving free space: every scan's rays walked through the map's voxels, the voxels' log-odds integrated (include/erasor_hip.h:
# erasor_hip_carve_*; kernels: erasor_amd/csrc/carve.hip.h), on the host ----------------------------------------------------------
# The normative text of the contract; the device equals it byte for byte.  OctoMap's and Peopleremover's argument (the reference's
# compare_results.launch, compare_map.cpp, analysis_octomap.py): the map goes into a voxel grid, every ray of every scan is walked
# through it, a voxel that rays pass through is free, one that rays end in is occupied, and the two are integrated as clamped log-odds.
#
# Coordinates are float64 on the float32 inputs.  Every operation is a separate IEEE operation in the order written.  Only + - * /,
# sqrt, floor and comparisons are used.  The log-odds are float32.
#
# Voxels.
#   - A finite point lies in cell c = floor(x / voxel) per axis.
#   - A map point with a non-finite coordinate lies in no voxel.  It is kept, gets zero votes and log-odds l_init, and is counted as
#     n_map_non_finite.
#   - The map voxels are the cells that hold at least one finite map point.  Only they carry state.
# Rays.
#   - The forward matrix of frame f is the M of visibility_transforms: T_body2origin[f] . T_lidar2body, upper three rows, float32
#     entries widened.
#   - The ray's origin o is M's column 3.
#   - A scan point (x, y, z) in the lidar frame has rho = sqrt((x x + y y) + z z).
#   - The gates, in this order: a non-finite coordinate, then rho outside [min_range, max_range].  Both are dropped and counted per
#     frame.
#   - The end point is e_i = ((M[i][0] x + M[i][1] y) + M[i][2] z) + M[i][3].
#   - Under a rigid M the end lies within max_range of the origin, so at most 4097 cells away per axis.  A ray whose end cell is not
#     within 4098 cells of the origin's cell on every axis (a matrix that stretches, or an end that is not finite) is dropped and
#     counted as out of range: this keeps every walk below 3 * 4098 steps whatever the matrix.
# Traversal.
#   - c0 = cell(o), c1 = cell(e), n_a = |c1_a - c0_a|, step_a = +-1, N = n_x + n_y + n_z.
#   - For an axis with n_a > 0: d_a = e_a - o_a; tMax_a = ((c0_a + (step_a > 0 ? 1 : 0)) * voxel - o_a) / d_a; tDelta_a = voxel / |d_a|.
#   - An axis with no steps left never moves.
#   - Each of the N steps moves the axis with the smallest tMax among the axes that still have steps left.  Ties go to x before y
#     before z.
#   - After the move, c_a += step_a, the steps left on that axis drop by one, and tMax_a += tDelta_a.
#   - So the walk visits V_0 = c0 ... V_N = c1, and always ends in c1 whatever the rounding.
#   - Free evidence: V_i for 0 <= i <= N - 1 - stop_short.
#   - Hit evidence: V_N.
#   - n_steps of a ray is max(0, N - stop_short).
# One update per voxel and scan, hits first (OctoMap's insertPointCloud rule).
#   - In frame f a map voxel is hit if any ray of f ends in it.
#   - Otherwise it is free if any ray of f has it as free evidence.
#   - Otherwise it is untouched.
# Integration, per map voxel, frames in index order.
#   - L starts at l_init.
#   - A hit frame: L = min(L + l_hit, l_max), and hits += 1.
#   - A free frame: L = max(L + l_miss, l_min), and misses += 1.
#   - Everything is float32.
#   - The log-odds are parameters.  No kernel calls log.
# Decision.  A map point is removed iff its voxel's L < l_thr.  Every point of a voxel shares its voxel's fate.
CARVE_MAX_FRAMES = 65535
CARVE_MAX_CELLS = 4096      # max_range / voxel
CARVE_MAX_REACH = 4098      # cells between a ray's origin and its end, per axis
CARVE_MAX_STOP_SHORT = 64
CARVE_CELL_LIMIT = 1 << 28  # a finite map point's or a frame origin's cell coordinate stays inside +- this
CARVE_ROW_FIELDS = ("n_points", "n_non_finite", "n_out_of_range", "n_rays", "n_steps", "n_end_in_map", "n_voxels_hit", "n_voxels_free")
CARVE_RESULT_FIELDS = ("n_points", "n_map_non_finite", "n_voxels", "n_blocks", "n_voxels_touched", "n_kept", "n_removed", "n_removed_dynamic",
                       "n_removed_static", "n_scan_points", "n_non_finite", "n_out_of_range", "n_rays", "n_steps", "n_end_in_map", "n_voxels_hit",
                       "n_voxels_free")
CARVE_LOGODDS_FIELDS = ("l_init", "l_hit", "l_miss", "l_min", "l_max", "l_thr")


def carve_logodds(p_hit=0.7, p_miss=0.4, p_min=0.12, p_max=0.97, p_thr=0.5):
    """OctoMap's log-odds from its probabilities, float32(log(p / (1 - p))) each, and l_init = 0 (its prior of one half): the defaults
    are OctoMap's own.  The driver forms them by the same expression with C's log."""
    import math
    lo = lambda p: float(np.float32(math.log(float(p) / (1.0 - float(p)))))
    return {"l_init": 0.0, "l_hit": lo(p_hit), "l_miss": lo(p_miss), "l_min": lo(p_min), "l_max": lo(p_max), "l_thr": lo(p_thr)}


def _carve_args(map_xyzi, scans, voxel, min_range, max_range, stop_short, logodds):
    lg = carve_logodds() if logodds is None else {k: float(np.float32(logodds[k])) for k in CARVE_LOGODDS_FIELDS}
    voxel, min_range, max_range = float(voxel), float(min_range), float(max_range)
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("carve: voxel must be a finite number > 0")
    if not (np.isfinite(min_range) and np.isfinite(max_range) and 0 <= min_range < max_range):
        raise ValueError("carve: 0 <= min_range < max_range, both finite")
    if max_range / voxel > CARVE_MAX_CELLS:
        raise ValueError("carve: max_range / voxel must not exceed 4096")
    if not (all(np.isfinite(lg[k]) for k in CARVE_LOGODDS_FIELDS) and lg["l_hit"] >= 0 and lg["l_miss"] <= 0 and lg["l_min"] <= lg["l_init"] <= lg["l_max"]):
        raise ValueError("carve: the log-odds must be finite, l_hit >= 0, l_miss <= 0 and l_min <= l_init <= l_max")
    if not 0 <= int(stop_short) <= CARVE_MAX_STOP_SHORT:
        raise ValueError("carve: stop_short must be within 0 .. 64")
    if len(scans) > CARVE_MAX_FRAMES:
        raise ValueError("carve: more than 65535 frames")
    c = np.ascontiguousarray(np.asarray(map_xyzi, np.float32).reshape(-1, 4))
    return c, voxel, min_range, max_range, int(stop_short), {k: np.float32(v) for k, v in lg.items()}


def _carve_frames(scans, T_body2origin, T_lidar2body, voxel):
    """every frame's forward matrix M [n, 3, 4] in float64 (visibility_transforms' M) and its origin's cell"""
    n = len(scans)
    A = (np.zeros((0, 4, 4), np.float32) if n == 0 else np.asarray(T_body2origin, np.float32).reshape(-1, 4, 4)).astype(np.float64)
    if len(A) != n:
        raise ValueError("carve: one T_body2origin per frame")
    visibility_transforms(A.astype(np.float32), T_lidar2body)  # (the refusal of a non-finite frame matrix)
    B = (np.eye(4, dtype=np.float32) if T_lidar2body is None else np.asarray(T_lidar2body, np.float32).reshape(4, 4)).astype(np.float64)
    M = np.zeros((n, 3, 4))
    for i in range(3):
        for j in range(4):
            v = (A[:, i, 0] * B[0, j] + A[:, i, 1] * B[1, j]) + A[:, i, 2] * B[2, j]
            M[:, i, j] = v + A[:, i, 3] if j == 3 else v
    c0 = np.floor(M[:, :, 3] / voxel)
    if not (np.abs(c0) < CARVE_CELL_LIMIT).all():
        raise ValueError("carve: a frame origin's cell coordinate reaches 2^28")
    return M, c0.astype(np.int64)


def _carve_map_cells(c, voxel):
    """(finite [n] bool, cells [n, 3] int64 with zeros where not finite)"""
    fin = np.isfinite(c[:, :3]).all(1)
    cells = np.zeros((len(c), 3), np.int64)
    f = np.floor(c[fin, :3].astype(np.float64) / voxel)
    if not (np.abs(f) < CARVE_CELL_LIMIT).all():
        raise ValueError("carve: a map point's cell coordinate reaches 2^28")
    cells[fin] = f.astype(np.int64)
    return fin, cells


def _carve_rays(scan, M, voxel, min_range, max_range, c0):
    """the rays of one frame that pass the gates: (n_points, n_non_finite, n_out_of_range, o [3], e [k, 3], c1 [k, 3] int64)"""
    s = np.asarray(scan, np.float32).reshape(-1, 4)[:, :3]
    fin = np.isfinite(s).all(1)
    p = s[fin].astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rho = np.sqrt((x * x + y * y) + z * z)
    ok = (rho >= min_range) & (rho <= max_range)
    with np.errstate(all="ignore"):
        e = np.stack([((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)], 1)
        fe = np.floor(e / voxel)
        ok &= (np.abs(fe - c0.astype(np.float64)) <= CARVE_MAX_REACH).all(1)  # (False for NaN)
    return len(s), int((~fin).sum()), int((~ok).sum()), M[:, 3].copy(), e[ok], fe[ok].astype(np.int64)


class _CarveGrid:
    """the map voxels: the distinct cells in lexicographic order, looked up through compressed coordinates (no key overflows)"""

    def __init__(self, cells):
        self.U = np.unique(cells.reshape(-1, 3), axis=0) if len(cells) else np.zeros((0, 3), np.int64)
        self.n = len(self.U)
        if self.n:
            self.ax = [np.unique(self.U[:, a]) for a in range(3)]
            i = [np.searchsorted(self.ax[a], self.U[:, a]) for a in range(3)]
            kxy = i[0] * len(self.ax[1]) + i[1]
            self.uxy = np.unique(kxy)
            self.keys = np.searchsorted(self.uxy, kxy) * len(self.ax[2]) + i[2]  # (increasing: U is in lexicographic order)

    def find(self, q):
        """the voxel index of every cell of q [k, 3], or -1"""
        q = np.asarray(q, np.int64).reshape(-1, 3)
        if not self.n or not len(q):
            return np.full(len(q), -1, np.int64)
        ok = np.ones(len(q), bool)
        i = []
        for a in range(3):
            j = np.minimum(np.searchsorted(self.ax[a], q[:, a]), len(self.ax[a]) - 1)
            ok &= self.ax[a][j] == q[:, a]
            i.append(j)
        kxy = i[0] * len(self.ax[1]) + i[1]
        j = np.minimum(np.searchsorted(self.uxy, kxy), len(self.uxy) - 1)
        ok &= self.uxy[j] == kxy
        key = j * len(self.ax[2]) + i[2]
        v = np.minimum(np.searchsorted(self.keys, key), self.n - 1)
        ok &= self.keys[v] == key
        return np.where(ok, v, -1)


def _carve_walk_setup(o, e, c0, c1, voxel):
    """(step, left, tmax, tdelta) of rays [k]: o [3] or [k, 3], e [k, 3], c0 [3] or [k, 3], c1 [k, 3]"""
    o = np.broadcast_to(np.asarray(o, np.float64), e.shape)
    c0 = np.broadcast_to(np.asarray(c0, np.int64), c1.shape)
    left = np.abs(c1 - c0)
    step = np.where(c1 > c0, 1, -1).astype(np.int64)
    with np.errstate(all="ignore"):
        d = e - o
        tmax = ((c0 + (step > 0)).astype(np.float64) * voxel - o) / d
        tdelta = voxel / np.abs(d)
    return step, left, tmax, tdelta


def carve_walk(origin, end, voxel):
    """One ray's voxel list [N + 1, 3] int64, V_0 = cell(origin) ... V_N = cell(end), by the traversal of the contract (float64 origin
    and end, as given): for the tests and for looking at one ray."""
    import math
    voxel = float(voxel)
    o, e = [float(v) for v in origin], [float(v) for v in end]
    c = [int(math.floor(o[a] / voxel)) for a in range(3)]
    c1 = [int(math.floor(e[a] / voxel)) for a in range(3)]
    left = [abs(c1[a] - c[a]) for a in range(3)]
    step = [1 if c1[a] > c[a] else -1 for a in range(3)]
    tmax, tdelta = [0.0] * 3, [0.0] * 3
    for a in range(3):
        if left[a]:
            d = e[a] - o[a]
            tmax[a] = (float(c[a] + (1 if step[a] > 0 else 0)) * voxel - o[a]) / d
            tdelta[a] = voxel / abs(d)
    out = [tuple(c)]
    for _ in range(sum(left)):
        a = -1
        for b in range(3):
            if left[b] and (a < 0 or tmax[b] < tmax[a]):
                a = b
        c[a] += step[a]
        left[a] -= 1
        tmax[a] += tdelta[a]
        out.append(tuple(c))
    assert list(out[-1]) == c1
    return np.array(out, np.int64).reshape(-1, 3)


def _carve_finish(c, fin, vox_of, L, hits, misses, n_blocks, rows, lg, keep):
    n = len(c)
    votes = np.zeros((n, 2), np.uint16)
    lo = np.full(n, lg["l_init"], np.float32)
    votes[fin, 0], votes[fin, 1], lo[fin] = hits[vox_of[fin]], misses[vox_of[fin]], L[vox_of[fin]]
    rem = fin & (lo < lg["l_thr"])
    dyn = _decode(c[:, 3])[2]
    res = {"n_points": n, "n_map_non_finite": int((~fin).sum()), "n_voxels": int(len(L)), "n_blocks": int(n_blocks),
           "n_voxels_touched": int(((hits.astype(np.int64) + misses) > 0).sum()), "n_kept": int((~rem).sum()), "n_removed": int(rem.sum()),
           "n_removed_dynamic": int((rem & dyn).sum()), "n_removed_static": int((rem & ~dyn).sum())}
    for key, src in (("n_scan_points", "n_points"),) + tuple((k, k) for k in CARVE_ROW_FIELDS[1:]):
        res[key] = int(sum(r[src] for r in rows))
    return votes, lo, (~rem).astype(np.uint8), (c[~rem].copy() if keep else None), rows, res


def carve(map_xyzi, scans, T_body2origin, T_lidar2body=None, voxel=0.2, min_range=0.5, max_range=80.0, stop_short=0, logodds=None, keep=True):
    """Free space carved out of a map (Erasor.carve): the contract above.  scans: XYZI rows per frame in the lidar frame; logodds: a dict
    with CARVE_LOGODDS_FIELDS (None: carve_logodds()).  Returns (votes [n, 2] uint16: hits, misses of the point's voxel; logodds [n]
    float32; mask uint8, 1 = kept; the kept rows in the order given or None; a row per frame with CARVE_ROW_FIELDS; a dict with
    CARVE_RESULT_FIELDS)."""
    c, voxel, min_range, max_range, ss, lg = _carve_args(map_xyzi, scans, voxel, min_range, max_range, stop_short, logodds)
    M, c0s = _carve_frames(scans, T_body2origin, T_lidar2body, voxel)
    fin, cells = _carve_map_cells(c, voxel)
    G = _CarveGrid(cells[fin])
    vox_of = np.zeros(len(c), np.int64)
    vox_of[fin] = G.find(cells[fin])
    n_blocks = len(np.unique(G.U >> 2, axis=0)) if G.n else 0
    L = np.full(G.n, lg["l_init"], np.float32)
    hits, misses = np.zeros(G.n, np.uint16), np.zeros(G.n, np.uint16)
    rows = []
    for f, scan in enumerate(scans):
        n_pts, n_nf, n_oor, o, e, c1 = _carve_rays(scan, M[f], voxel, min_range, max_range, c0s[f])
        step, left, tmax, tdelta = _carve_walk_setup(o, e, c0s[f], c1, voxel)
        N = left.sum(1)
        vh = G.find(c1)
        hit = np.zeros(G.n, bool)
        hit[vh[vh >= 0]] = True
        free = np.zeros(G.n, bool)
        last = N - 1 - ss  # the index of a ray's last free voxel
        cur = np.broadcast_to(c0s[f], c1.shape).copy()
        live = np.flatnonzero(last >= 0)
        left, tmax = left.copy(), tmax.copy()
        i = 0
        while len(live):
            v = G.find(cur[live])
            free[v[v >= 0]] = True
            live = live[last[live] > i]  # (those still have a step before their next free voxel)
            tm = np.where(left[live] > 0, tmax[live], np.inf)
            a = np.argmin(tm, 1)  # (the first of equal minima: x before y before z)
            cur[live, a] += step[live, a]
            left[live, a] -= 1
            tmax[live, a] += tdelta[live, a]
            i += 1
        free &= ~hit
        L[hit] = np.minimum(L[hit] + lg["l_hit"], lg["l_max"])
        L[free] = np.maximum(L[free] + lg["l_miss"], lg["l_min"])
        hits[hit] += 1
        misses[free] += 1
        rows.append(dict(zip(CARVE_ROW_FIELDS, [n_pts, n_nf, n_oor, len(e), int(np.maximum(N - ss, 0).sum()), int((vh >= 0).sum()), int(hit.sum()),
                                                int(free.sum())])))
    return _carve_finish(c, fin, vox_of, L, hits, misses, n_blocks, rows, lg, keep)


def carve_brute(map_xyzi, scans, T_body2origin, T_lidar2body=None, voxel=0.2, min_range=0.5, max_range=80.0, stop_short=0, logodds=None, keep=True):
    """carve() ray by ray in plain Python floats (math.sqrt, math.floor) with dicts for the voxels, for small inputs: the check of the
    vectorised text"""
    import math
    c, voxel, min_range, max_range, ss, lg = _carve_args(map_xyzi, scans, voxel, min_range, max_range, stop_short, logodds)
    M, c0s = _carve_frames(scans, T_body2origin, T_lidar2body, voxel)
    fin, cells = _carve_map_cells(c, voxel)
    vox = {}  # cell -> [L, hits, misses]
    for i, row in enumerate(c.astype(np.float64).tolist()):
        if all(math.isfinite(v) for v in row[:3]):
            vox.setdefault(tuple(int(math.floor(v / voxel)) for v in row[:3]), [lg["l_init"], 0, 0])
    rows = []
    for f, scan in enumerate(scans):
        s = np.asarray(scan, np.float32).reshape(-1, 4)
        m = [[float(v) for v in r] for r in M[f]]
        o = [m[i][3] for i in range(3)]
        c0 = tuple(int(v) for v in c0s[f])
        n_nf = n_oor = n_rays = n_steps = n_end = 0
        hit, free = set(), set()
        for x, y, z, _ in s.astype(np.float64).tolist():
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                n_nf += 1
                continue
            rho = math.sqrt((x * x + y * y) + z * z)
            if not (min_range <= rho <= max_range):
                n_oor += 1
                continue
            e = [((m[i][0] * x + m[i][1] * y) + m[i][2] * z) + m[i][3] for i in range(3)]
            if not all(math.isfinite(v) and abs(math.floor(v / voxel) - c0[a]) <= CARVE_MAX_REACH for a, v in enumerate(e)):
                n_oor += 1
                continue
            walk = [tuple(int(v) for v in w) for w in carve_walk(o, e, voxel)]
            N = len(walk) - 1
            n_rays += 1
            n_steps += max(0, N - ss)
            for w in walk[: max(0, N - ss)]:
                if w in vox:
                    free.add(w)
            if walk[N] in vox:
                hit.add(walk[N])
                n_end += 1
        free -= hit
        for w in hit:
            st = vox[w]
            st[0], st[1] = min(np.float32(st[0] + lg["l_hit"]), lg["l_max"]), st[1] + 1
        for w in free:
            st = vox[w]
            st[0], st[2] = max(np.float32(st[0] + lg["l_miss"]), lg["l_min"]), st[2] + 1
        rows.append(dict(zip(CARVE_ROW_FIELDS, [len(s), n_nf, n_oor, n_rays, n_steps, n_end, len(hit), len(free)])))
    order = sorted(vox)
    index = {w: j for j, w in enumerate(order)}
    vox_of = np.array([index[tuple(int(v) for v in cells[i])] if fin[i] else 0 for i in range(len(c))], np.int64).reshape(-1)
    L = np.array([vox[w][0] for w in order], np.float32).reshape(-1)
    hits = np.array([vox[w][1] for w in order], np.uint16).reshape(-1)
    misses = np.array([vox[w][2] for w in order], np.uint16).reshape(-1)
    return _carve_finish(c, fin, vox_of, L, hits, misses, len({tuple(v >> 2 for v in w) for w in order}), rows, lg, keep)


# ---- the ground of every scan, and the map's ground points by vote (Erasor.ground_scans / ground_votes; kernels: ground.hip.h) ----
# R-GPF (erasor.cpp:183-294: extract_initial_seeds_, estimate_plane_, the loop of extract_ground) run on every polar patch of every scan,
# as the author's follow-up (Patchwork) runs it, with every order fixed.  The reference fits in float32 with Eigen's JacobiSVD over an
# unordered cloud and sorts the seeds' candidates with std::sort; here everything is float64 on the float32 coordinates, every operation a
# separate IEEE operation in the order written, and only + - * /, sqrt and comparisons:
#   * the patch grid is data: n_sectors (a multiple of 8) columns of visibility_column over col_tan, and n_rings rings between the
#     ring_edge radii; r = sqrt(x*x + y*y), ring = (the number of ring_edge entries <= r) - 1.  The gates, in this order: a non-finite
#     coordinate (code 255); on the axis, or a ring outside 0 .. n_rings - 1 (OUT OF RANGE, code 2).  A patch is (frame, ring, sector);
#     its points are kept in scan order, j = 0 .. m - 1;
#   * a patch of fewer than min_points points is SPARSE (its points: code 2);
#   * seeds: the candidates are the points with z >= min_z ordered by (z, j) (-0.0 equals +0.0); lpr = (((0.0 + z_0) + z_1) + ...) / k over
#     the first k = min(num_lpr, candidates); no candidate: DEGENERATE.  The seeds: z >= min_z and z < lpr + th_seeds;
#   * `iters` times over the current member set: the count n and the nine raw moments x y z xx xy xz yy yz zz summed over ALL the patch's
#     points in patch order by refine_tree_sum's rule (a non-member holds +0.0); n < 3: DEGENERATE; mean = S / n; cov_ab = S_ab / n -
#     mean_a * mean_b; tr = (cxx + cyy) + czz, taken before the solve; not tr > 0: DEGENERATE (zero, or below it by rounding);
#     _jacobi3; the eigenvalues ascend by (value, column); the normal is the first one's column, negated iff its z < 0; d = -((nx mx +
#     ny my) + nz mz); the new members are the patch's points with ((nx x + ny y) + nz z) + d < th_dist (one-sided, as the reference);
#   * after the last iteration: nz < uprightness: REJECTED_UPRIGHT; else mean_z > elevation[ring] and not (l0 / tr <= flatness[ring]):
#     REJECTED_ELEVATION (mean_z, l0, tr: the last iteration's); else OK;
#   * codes: 1 a member of an OK patch; 0 judged and not a member, or any point of a REJECTED patch; 2 not judged (out of range, SPARSE,
#     DEGENERATE); 255 non-finite.  The patch table's rows of SPARSE and DEGENERATE patches carry zeros behind n_points.
GROUND_EMPTY, GROUND_OK, GROUND_SPARSE, GROUND_DEGENERATE, GROUND_REJECTED_UPRIGHT, GROUND_REJECTED_ELEVATION = 0, 1, 2, 3, 4, 5
GROUND_CODE_NOT, GROUND_CODE_GROUND, GROUND_CODE_NOT_JUDGED, GROUND_CODE_NON_FINITE = 0, 1, 2, 255
GROUND_MAX_FRAMES = 65535
GROUND_MAX_RINGS, GROUND_MAX_SECTORS, GROUND_MAX_LPR, GROUND_MAX_ITERS = 64, 512, 64, 16
GROUND_WAVE_POINTS = 64     # ERASOR_GROUND_WAVE_POINTS: a patch of at most this many points is fitted by one wavefront
GROUND_SMALL_POINTS = 1024  # ERASOR_GROUND_SMALL_POINTS: ... by a workgroup with the small LDS allotment; beyond, the large one
GROUND_LDS_POINTS = 4096    # ERASOR_GROUND_LDS_POINTS: a patch beyond this streams from memory in every iteration
GROUND_WORK_BUDGET = 256 << 20
GROUND_ROW_FIELDS = ("n_points", "n_non_finite", "n_out_of_range", "n_judged", "n_ground", "n_ground_dynamic", "n_patches", "n_sparse",
                     "n_degenerate", "n_rejected_upright", "n_rejected_elevation")
GROUND_VOTES_ROW_FIELDS = GROUND_ROW_FIELDS + ("n_gathered",)
GROUND_VOTES_RESULT_FIELDS = ("n_points", "n_ground", "n_ground_dynamic", "n_ground_static", "n_unseen", "n_kept", "n_gathered", "n_judged")
GROUND_DEFAULTS = {"num_lpr": 10, "th_seeds": 0.5, "th_dist": 0.15, "iters": 3, "min_points": 10, "min_z": -3.03, "uprightness": 0.707}
GROUND_PATCH_DTYPE = np.dtype([("status", np.uint32), ("n_points", np.uint32), ("n_ground", np.uint32), ("reserved", np.uint32),
                               ("normal", np.float64, 3), ("d", np.float64), ("mean_z", np.float64), ("eig", np.float64, 3)])  # erasor_ground_patch


def ground_grid(n_rings=20, n_sectors=64, min_range=0.5, max_range=80.0):
    """A uniform patch grid: n_sectors columns of equal azimuth (visibility_grid's column table for that width) and n_rings rings of equal
    width, ring_edge[i] = min_range + ((max_range - min_range) * i) / n_rings -- the driver forms both by the same expressions"""
    import math
    R, S = int(n_rings), int(n_sectors)
    if S % 8 or not 8 <= S <= GROUND_MAX_SECTORS or not 1 <= R <= GROUND_MAX_RINGS:
        raise ValueError("ground_grid: n_sectors must be a multiple of 8 within 8 .. 512, n_rings within 1 .. 64")
    M = S // 8
    col = np.array([math.tan(((math.pi / 4.0) * k) / M) for k in range(1, M)], np.float64)
    edge = np.array([float(min_range) + ((float(max_range) - float(min_range)) * i) / R for i in range(R + 1)], np.float64)
    return check_ground_grid({"n_sectors": S, "col_tan": col, "ring_edge": edge})


def check_ground_grid(grid):
    S = int(grid["n_sectors"])
    col = np.ascontiguousarray(grid["col_tan"], np.float64).reshape(-1)
    edge = np.ascontiguousarray(grid["ring_edge"], np.float64).reshape(-1)
    if S % 8 or not 8 <= S <= GROUND_MAX_SECTORS:
        raise ValueError("ground: n_sectors must be a multiple of 8 within 8 .. 512")
    if not 2 <= len(edge) <= GROUND_MAX_RINGS + 1:
        raise ValueError("ground: ring_edge has n_rings + 1 entries, n_rings within 1 .. 64")
    if len(col) != S // 8 - 1:
        raise ValueError("ground: col_tan has n_sectors / 8 - 1 entries")
    if not ((col > 0) & (col < 1)).all() or not (np.diff(col) > 0).all():
        raise ValueError("ground: col_tan must be strictly increasing within (0, 1)")
    if not np.isfinite(edge).all() or not (np.diff(edge) > 0).all() or not edge[0] >= 0:
        raise ValueError("ground: ring_edge must be finite, strictly increasing and start at >= 0")
    return {"n_sectors": S, "col_tan": col, "ring_edge": edge}


def _ground_args(grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, n_frames):
    g = check_ground_grid(ground_grid() if grid is None else grid)
    R = len(g["ring_edge"]) - 1
    if not (isinstance(num_lpr, (int, np.integer)) and 1 <= num_lpr <= GROUND_MAX_LPR):
        raise ValueError("ground: num_lpr must be within 1 .. 64")
    if not (isinstance(iters, (int, np.integer)) and 1 <= iters <= GROUND_MAX_ITERS):
        raise ValueError("ground: iters must be within 1 .. 16")
    if not (isinstance(min_points, (int, np.integer)) and 3 <= min_points <= 0xFFFFFFFF):
        raise ValueError("ground: min_points must be at least 3")
    if not all(np.isfinite(v) for v in (th_seeds, th_dist, min_z, uprightness)):
        raise ValueError("ground: th_seeds, th_dist, min_z and uprightness must be finite")
    el = np.full(R, np.inf) if elevation is None else np.ascontiguousarray(elevation, np.float64).reshape(-1)
    fl = np.zeros(R) if flatness is None else np.ascontiguousarray(flatness, np.float64).reshape(-1)
    if len(el) != R or len(fl) != R or np.isnan(el).any() or np.isnan(fl).any():
        raise ValueError("ground: elevation and flatness have n_rings entries, none of them NaN")
    if n_frames > GROUND_MAX_FRAMES:
        raise ValueError("ground: more than 65535 frames")
    prm = {"num_lpr": int(num_lpr), "th_seeds": float(th_seeds), "th_dist": float(th_dist), "iters": int(iters), "min_points": int(min_points),
           "min_z": float(min_z), "uprightness": float(uprightness), "elevation": el, "flatness": fl}
    return g, R, prm


def ground_patch_of(x, y, grid):
    """(ring, sector) of points in a lidar frame (float64 arrays of finite values), ring = -1 where the point is out of range: THE patch
    mapping, written down once"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    edge = grid["ring_edge"]
    sec = visibility_column(x, y, grid["col_tan"], grid["n_sectors"])
    r = np.sqrt(x * x + y * y)
    ring = np.searchsorted(edge, r, side="right").astype(np.int64) - 1
    ring[(sec < 0) | (ring < 0) | (ring >= len(edge) - 1)] = -1
    return ring, sec


def _ground_plane(S, n):
    """mean, covariance, trace and (when the trace is positive) the sorted eigen-solve of nine raw moments S over n members, in Python floats"""
    nn = float(n)
    mx, my, mz = float(S[0]) / nn, float(S[1]) / nn, float(S[2]) / nn
    cxx, cxy, cxz = float(S[3]) / nn - mx * mx, float(S[4]) / nn - mx * my, float(S[5]) / nn - mx * mz
    cyy, cyz, czz = float(S[6]) / nn - my * my, float(S[7]) / nn - my * mz, float(S[8]) / nn - mz * mz
    tr = (cxx + cyy) + czz
    if not tr > 0:
        return None
    A = [[cxx, cxy, cxz], [cxy, cyy, cyz], [cxz, cyz, czz]]
    V = _jacobi3(A)
    col = sorted(range(3), key=lambda j: (A[j][j], j))
    l = [A[j][j] for j in col]
    nx, ny, nz = V[0][col[0]], V[1][col[0]], V[2][col[0]]
    if nz < 0:
        nx, ny, nz = -nx, -ny, -nz
    d = -((nx * mx + ny * my) + nz * mz)
    return (nx, ny, nz), d, mz, l, tr


def _ground_gates(nz, mean_z, l0, tr, ring, prm):
    if nz < prm["uprightness"]:
        return GROUND_REJECTED_UPRIGHT
    if mean_z > prm["elevation"][ring] and not (l0 / tr <= prm["flatness"][ring]):
        return GROUND_REJECTED_ELEVATION
    return GROUND_OK


def ground_fit(p64, ring, prm):
    """R-GPF on one patch: p64 its points (m, 3) float64 in patch order, m >= min_points.  Returns (status, members (bool), plane or None),
    plane = ((nx, ny, nz), d, mean_z, [l0, l1, l2], trace) of the last iteration"""
    x, y, z = p64[:, 0], p64[:, 1], p64[:, 2]
    m = len(z)
    none = np.zeros(m, bool)
    cand = np.flatnonzero(z >= prm["min_z"])
    if len(cand) == 0:
        return GROUND_DEGENERATE, none, None
    lowest = cand[np.argsort(z[cand], kind="stable")][: prm["num_lpr"]]  # (a stable sort of z: ascending by (z, j))
    s = 0.0
    for v in z[lowest].tolist():
        s = s + v
    lpr = s / float(len(lowest))
    mem = (z >= prm["min_z"]) & (z < lpr + prm["th_seeds"])
    rows = np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], 1)
    plane = None
    for _ in range(prm["iters"]):
        n = int(mem.sum())
        if n < 3:
            return GROUND_DEGENERATE, none, None
        plane = _ground_plane(refine_tree_sum(np.where(mem[:, None], rows, 0.0)), n)
        if plane is None:
            return GROUND_DEGENERATE, none, None
        (nx, ny, nz), d = plane[0], plane[1]
        with np.errstate(all="ignore"):
            mem = ((nx * x + ny * y) + nz * z) + d < prm["th_dist"]
    return _ground_gates(plane[0][2], plane[2], plane[3][0], plane[4], ring, prm), mem, plane


def _tree_sum_brute(vals):
    """refine_tree_sum of one column, in Python floats"""
    total = 0.0
    for b in range(0, len(vals), REFINE_CHUNK):
        c = vals[b:b + REFINE_CHUNK] + [0.0] * (REFINE_CHUNK - len(vals[b:b + REFINE_CHUNK]))
        s = REFINE_CHUNK // 2
        while s >= 1:
            c = [c[i] + c[i + s] for i in range(s)]
            s //= 2
        total = total + c[0]
    return total


def ground_fit_brute(p64, ring, prm):
    """ground_fit point by point in Python floats"""
    P = [[float(v) for v in r] for r in np.asarray(p64, np.float64).reshape(-1, 3).tolist()]
    m = len(P)
    none = np.zeros(m, bool)
    cand = sorted((P[j][2] + 0.0, j) for j in range(m) if P[j][2] >= prm["min_z"])  # (-0.0 + 0.0 = +0.0: tuples compare z, then j)
    if not cand:
        return GROUND_DEGENERATE, none, None
    k = min(prm["num_lpr"], len(cand))
    s = 0.0
    for zj, _ in cand[:k]:
        s = s + zj
    lpr = s / float(k)
    mem = [p[2] >= prm["min_z"] and p[2] < lpr + prm["th_seeds"] for p in P]
    plane = None
    for _ in range(prm["iters"]):
        n = sum(mem)
        if n < 3:
            return GROUND_DEGENERATE, none, None
        cols = []
        for a, b in ((0, None), (1, None), (2, None), (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
            cols.append(_tree_sum_brute([(p[a] if b is None else p[a] * p[b]) if g else 0.0 for p, g in zip(P, mem)]))
        plane = _ground_plane(cols, n)
        if plane is None:
            return GROUND_DEGENERATE, none, None
        (nx, ny, nz), d = plane[0], plane[1]
        mem = [((nx * p[0] + ny * p[1]) + nz * p[2]) + d < prm["th_dist"] for p in P]
    return _ground_gates(plane[0][2], plane[2], plane[3][0], plane[4], ring, prm), np.array(mem, bool).reshape(-1), plane


def _ground_scans(scans, grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, patches, fit):
    g, R, prm = _ground_args(grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, len(scans))
    S = g["n_sectors"]
    table = np.zeros((len(scans), R, S), GROUND_PATCH_DTYPE)
    codes, rows = [], []
    for f, scan in enumerate(scans):
        s = np.ascontiguousarray(np.asarray(scan, np.float32).reshape(-1, 4))
        fin = np.isfinite(s[:, :3]).all(1)
        p64 = np.where(fin[:, None], s[:, :3], np.float32(1)).astype(np.float64)
        ring, sec = ground_patch_of(p64[:, 0], p64[:, 1], g)
        ring[~fin] = -1
        code = np.full(len(s), GROUND_CODE_NOT_JUDGED, np.uint8)
        code[~fin] = GROUND_CODE_NON_FINITE
        inr = np.flatnonzero(ring >= 0)
        key = ring[inr] * S + sec[inr]
        order = inr[np.argsort(key, kind="stable")]  # (patch by patch, each in scan order)
        cnt = {st: 0 for st in (GROUND_SPARSE, GROUND_DEGENERATE, GROUND_REJECTED_UPRIGHT, GROUND_REJECTED_ELEVATION)}
        n_judged = 0
        pos = 0
        for k, m in zip(*np.unique(key, return_counts=True)):
            idx = order[pos:pos + m]
            pos += m
            rg, sc = int(k) // S, int(k) % S
            row = table[f, rg, sc]
            row["n_points"] = m
            if int(m) < prm["min_points"]:
                row["status"] = GROUND_SPARSE
                cnt[GROUND_SPARSE] += 1
                continue
            status, mem, plane = fit(p64[idx], rg, prm)
            row["status"] = status
            if status == GROUND_DEGENERATE:
                cnt[status] += 1
                continue
            n_judged += int(m)
            row["normal"], row["d"], row["mean_z"], row["eig"] = plane[0], plane[1], plane[2], plane[3]
            code[idx] = GROUND_CODE_NOT
            if status == GROUND_OK:
                code[idx[mem]] = GROUND_CODE_GROUND
                row["n_ground"] = int(mem.sum())
            else:
                cnt[status] += 1
        gr = code == GROUND_CODE_GROUND
        rows.append(dict(zip(GROUND_ROW_FIELDS, [len(s), int((~fin).sum()), int((fin & (ring < 0)).sum()), n_judged, int(gr.sum()),
                                                 int((gr & _decode(s[:, 3])[2]).sum()), len(np.unique(key)), cnt[GROUND_SPARSE],
                                                 cnt[GROUND_DEGENERATE], cnt[GROUND_REJECTED_UPRIGHT], cnt[GROUND_REJECTED_ELEVATION]])))
        codes.append(code)
    res = {"n_frames": len(scans)}
    for k in GROUND_ROW_FIELDS:
        res[k] = int(sum(r[k] for r in rows))
    return (np.concatenate(codes) if codes else np.zeros(0, np.uint8)), rows, res, (table if patches else None)


def ground_scans(scans, grid=None, num_lpr=10, th_seeds=0.5, th_dist=0.15, iters=3, min_points=10, min_z=-3.03, uprightness=0.707,
                 elevation=None, flatness=None, patches=False):
    """Every scan's ground (Erasor.ground_scans): the contract above.  scans: XYZI rows per frame in the lidar frame; grid: ground_grid()
    or a dict with n_sectors, col_tan and ring_edge (None: ground_grid()); elevation, flatness: float64 tables of n_rings entries (None:
    +inf and 0, both gates off).  Returns (codes uint8, all frames one after another; a row per frame with GROUND_ROW_FIELDS, where
    n_ground_dynamic counts the ground points labelled 252 .. 259; their sums with n_frames; with `patches` the table [n_frames, n_rings,
    n_sectors] of GROUND_PATCH_DTYPE, else None)."""
    return _ground_scans(scans, grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, patches, ground_fit)


def ground_scans_brute(scans, grid=None, num_lpr=10, th_seeds=0.5, th_dist=0.15, iters=3, min_points=10, min_z=-3.03, uprightness=0.707,
                       elevation=None, flatness=None, patches=False):
    """ground_scans() with every patch fitted point by point in plain Python floats, for small inputs: the check of the vectorised text"""
    return _ground_scans(scans, grid, num_lpr, th_seeds, th_dist, iters, min_points, min_z, uprightness, elevation, flatness, patches,
                         ground_fit_brute)


def ground_gather(map_xyzi, T_body2origin, T_lidar2body=None, grid=None):
    """What every frame sees of the map, as ground_votes segments it: every finite map point put into the frame's lidar frame by
    visibility_transforms' row in float64, q = ((r0 x + r1 y) + r2 z) + t, and rounded to float32; the points whose rounded coordinates
    are finite and whose ring is in range are kept in map order with the map point's intensity.  Returns (clouds, indices): per frame the
    (k, 4) float32 cloud and the map indices of its rows."""
    g = check_ground_grid(ground_grid() if grid is None else grid)
    c = np.ascontiguousarray(np.asarray(map_xyzi, np.float32).reshape(-1, 4))
    n_f = len(np.asarray(T_body2origin, np.float32).reshape(-1, 16))
    m, _ = visibility_transforms(np.zeros((0, 4, 4), np.float32) if n_f == 0 else T_body2origin, T_lidar2body)
    pfin = np.isfinite(c[:, :3]).all(1)
    p = np.where(pfin[:, None], c[:, :3], np.float32(0)).astype(np.float64)
    clouds, indices = [], []
    for f in range(n_f):
        with np.errstate(all="ignore"):
            q = np.stack([((m[f, 4 * r] * p[:, 0] + m[f, 4 * r + 1] * p[:, 1]) + m[f, 4 * r + 2] * p[:, 2]) + m[f, 4 * r + 3] for r in range(3)],
                         1).astype(np.float32)
        ok = pfin & np.isfinite(q).all(1)
        q64 = np.where(ok[:, None], q, np.float32(1)).astype(np.float64)
        ring, _ = ground_patch_of(q64[:, 0], q64[:, 1], g)
        idx = np.flatnonzero(ok & (ring >= 0))
        clouds.append(np.concatenate([q[idx], c[idx, 3:4]], 1).astype(np.float32).reshape(-1, 4))
        indices.append(idx)
    return clouds, indices


def ground_decide(votes, min_votes, ratio):
    """the map's ground points (bool): ground >= min_votes and (double)ground > ratio * (double)seen"""
    v = np.asarray(votes).reshape(-1, 2)
    return (v[:, 1].astype(np.int64) >= int(min_votes)) & (v[:, 1].astype(np.float64) > np.float64(ratio) * v[:, 0].astype(np.float64))


def _ground_votes(scans_fn, map_xyzi, T_body2origin, T_lidar2body, grid, kw, min_votes, ratio, keep):
    if not 0 <= int(min_votes) <= 0xFFFFFFFF or not np.isfinite(ratio):
        raise ValueError("ground: min_votes must fit 32 bits and ratio be finite")
    c = np.ascontiguousarray(np.asarray(map_xyzi, np.float32).reshape(-1, 4))
    clouds, indices = ground_gather(c, T_body2origin, T_lidar2body, grid)
    codes, rows, res, _ = scans_fn(clouds, grid, **kw)
    votes = np.zeros((len(c), 2), np.uint16)
    pos = 0
    for f, idx in enumerate(indices):
        cf = codes[pos:pos + len(idx)]
        pos += len(idx)
        votes[idx[cf <= GROUND_CODE_GROUND], 0] += 1
        votes[idx[cf == GROUND_CODE_GROUND], 1] += 1
        rows[f]["n_gathered"] = len(idx)
    gr = ground_decide(votes, min_votes, ratio)
    dyn = _decode(c[:, 3])[2]
    kept = gr if keep else ~gr
    out = {"n_points": len(c), "n_ground": int(gr.sum()), "n_ground_dynamic": int((gr & dyn).sum()), "n_ground_static": int((gr & ~dyn).sum()),
           "n_unseen": int((votes[:, 0] == 0).sum()), "n_kept": int(kept.sum()), "n_gathered": res["n_points"], "n_judged": res["n_judged"]}
    return votes, gr.astype(np.uint8), c[kept].copy(), rows, out


def ground_votes(map_xyzi, T_body2origin, T_lidar2body=None, grid=None, num_lpr=10, th_seeds=0.5, th_dist=0.15, iters=3, min_points=10,
                 min_z=-3.03, uprightness=0.707, elevation=None, flatness=None, min_votes=1, ratio=0.5, keep=1, work_budget_bytes=0):
    """The map's ground points by vote (Erasor.ground_votes): ground_gather's cloud of every frame is segmented exactly as a scan
    (ground_scans); a map point gets seen += 1 where it was judged (code 0 or 1) and ground += 1 where its code was 1; it is ground iff
    ground >= min_votes and (double)ground > ratio * (double)seen.  work_budget_bytes only sizes the device's batches: the result does not
    depend on it.  Returns (votes [n, 2] uint16: seen, ground; mask uint8, 1 = ground; the ground rows (keep = 1) or the rest (keep = 0)
    in map order; a row per frame with GROUND_VOTES_ROW_FIELDS; a dict with GROUND_VOTES_RESULT_FIELDS)."""
    kw = dict(num_lpr=num_lpr, th_seeds=th_seeds, th_dist=th_dist, iters=iters, min_points=min_points, min_z=min_z, uprightness=uprightness,
              elevation=elevation, flatness=flatness)
    return _ground_votes(ground_scans, map_xyzi, T_body2origin, T_lidar2body, grid, kw, min_votes, ratio, keep)


def ground_votes_brute(map_xyzi, T_body2origin, T_lidar2body=None, grid=None, num_lpr=10, th_seeds=0.5, th_dist=0.15, iters=3, min_points=10,
                       min_z=-3.03, uprightness=0.707, elevation=None, flatness=None, min_votes=1, ratio=0.5, keep=1, work_budget_bytes=0):
    """ground_votes() over ground_scans_brute, for small inputs"""
    kw = dict(num_lpr=num_lpr, th_seeds=th_seeds, th_dist=th_dist, iters=iters, min_points=min_points, min_z=min_z, uprightness=uprightness,
              elevation=elevation, flatness=flatness)
    return _ground_votes(ground_scans_brute, map_xyzi, T_body2origin, T_lidar2body, grid, kw, min_votes, ratio, keep)
