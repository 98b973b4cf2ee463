// erasor_offline_demo — ROS-free driver shaped like src/offline_map_updater/main_in_your_env.cpp:61-127:
//   <dir>/map.pcd, <dir>/pcds/%06d.pcd, <dir>/poses.csv (header line; idx,?,x,y,z,qx,qy,qz,qw per line, cols 2..8)
// processes every node through erasor::OfflineMapUpdater and writes <dir>/<data_name>_result.pcd and map_final.pcd.
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <deque>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <thread>

#include "erasor_shim.h"

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static bool read_bin(const std::string &path, pcl::PointCloud<pcl::PointXYZI> &c) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const size_t n = (size_t)f.tellg() / 16;
    f.seekg(0);
    std::vector<float> v(n * 4);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * 16));
    c.points.resize(n);
    for (size_t i = 0; i < n; ++i) { c.points[i].x = v[4 * i]; c.points[i].y = v[4 * i + 1]; c.points[i].z = v[4 * i + 2]; c.points[i].intensity = v[4 * i + 3]; }
    return true;
}
static void write_bin(const std::string &path, const pcl::PointCloud<pcl::PointXYZI> &c) {
    std::ofstream f(path, std::ios::binary);
    for (const auto &p : c.points) {
        const float v[4] = {p.x, p.y, p.z, p.intensity};
        f.write(reinterpret_cast<const char *>(v), 16);
    }
}

// --erasor-class <map_voi.bin> <query_voi.bin> <out_prefix> <version>: the ERASOR class used the way
// OfflineMapUpdater.cpp:266-284 uses it (set_inputs -> compare_* -> get_static_estimate -> get_outliers)
static int erasor_class_mode(int argc, char **argv) {
    if (argc < 6) return 2;
    erasor_params p;
    erasor_hip_params_default(&p);
    p.max_range = 60.0; p.num_rings = 15; p.num_sectors = 60; p.min_h = -1.3; p.max_h = 3.2; p.th_bin_max_h = 0.05;
    p.scan_ratio_threshold = 0.3; p.minimum_num_pts = 10; p.gf_dist_thr = 0.15; p.gf_iter = 3; p.gf_num_lpr = 10; p.gf_th_seeds_height = 0.5;
    pcl::PointCloud<pcl::PointXYZI> map_voi, query_voi, arranged, complement, map_rejected, curr_rejected;
    if (!read_bin(argv[2], map_voi) || !read_bin(argv[3], query_voi)) return 3;
    const std::string out = argv[4];
    const int version = atoi(argv[5]);
    ERASOR erasor(p);
    erasor.set_inputs(map_voi, query_voi);
    if (version == 2) erasor.compare_vois_and_revert_ground(0);
    else if (version == 3) erasor.compare_vois_and_revert_ground_w_block(0);
    else throw std::invalid_argument("Other version is not implemented!");
    erasor.get_static_estimate(arranged, complement);
    erasor.get_outliers(map_rejected, curr_rejected);
    write_bin(out + "_arranged.bin", arranged);
    write_bin(out + "_complement.bin", complement);
    write_bin(out + "_map_rejected.bin", map_rejected);
    write_bin(out + "_ground_viz.bin", erasor.ground_viz);
    {   // the public R-PODs (erasor.h:143-145): per bin count / min_h / max_h / status, theta-major point dumps, and
        // is_dynamic_obj_close for every bin (erasor.cpp:573-595)
        std::ofstream f(out + "_rpod.txt");
        pcl::PointCloud<pcl::PointXYZI> flat[3];
        R_POD *pods[3] = {&erasor.r_pod_map, &erasor.r_pod_curr, &erasor.r_pod_selected};
        for (int t = 0; t < p.num_sectors; ++t)
            for (int r = 0; r < p.num_rings; ++r) {
                for (int w = 0; w < 3; ++w)
                    if ((*pods[w])[r][t].is_occupied) flat[w] += (*pods[w])[r][t].points;  // r_pod2pc, erasor.cpp:309-320
                const Bin &m = erasor.r_pod_map[r][t], &c = erasor.r_pod_curr[r][t], &s = erasor.r_pod_selected[r][t];
                char line[256];
                snprintf(line, sizeof(line), "%d %d %zu %.17g %.17g %zu %.17g %.17g %zu %.17g %d\n", r, t, m.points.size(), m.min_h, m.max_h,
                         c.points.size(), c.min_h, c.max_h, s.points.size(), s.status,
                         erasor.is_dynamic_obj_close(erasor.r_pod_selected, r, t, 1, 1) ? 1 : 0);
                f << line;
            }
        write_bin(out + "_rpod_map.bin", flat[0]);
        write_bin(out + "_rpod_curr.bin", flat[1]);
        write_bin(out + "_rpod_selected.bin", flat[2]);
    }
    printf("ERASOR class: arranged %zu complement %zu rejected %zu max_range %.1f\n", arranged.size(), complement.size(), map_rejected.size(),
           erasor.get_max_range());
    return 0;
}

// ---- PR / RR (scripts/analysis_runner.py:74-105 on the device: erasor_hip_evaluate_clouds) ----
// a cloud from a PCD (any encoding erasor_utils::load_pcd reads) or a .bin of XYZI float rows, as XYZI rows
static bool load_cloud_xyzi(const std::string &path, std::vector<float> &xyzi) {
    pcl::PointCloud<pcl::PointXYZI> c;
    const bool is_bin = path.size() >= 4 && path.compare(path.size() - 4, 4, ".bin") == 0;
    if (is_bin ? !read_bin(path, c) : erasor_utils::load_pcd(path, c) == -1) return false;
    xyzi.resize(c.size() * 4);
    for (size_t i = 0; i < c.size(); ++i) {
        xyzi[4 * i] = c.points[i].x;
        xyzi[4 * i + 1] = c.points[i].y;
        xyzi[4 * i + 2] = c.points[i].z;
        xyzi[4 * i + 3] = c.points[i].intensity;
    }
    return true;
}
// the row analysis_runner.py prints (tabulate, orgtbl)
static void print_eval_row(const erasor_eval_result &r) {
    printf("|   gt_S |   gt_D |   est_S |   est_D |   kept_S |   kept_D |     PR%% |     RR%% |     F1 |\n");
    printf("|--------+--------+---------+---------+----------+----------+---------+---------+--------|\n");
    printf("| %6llu | %6llu | %7llu | %7llu | %8llu | %8llu | %7.3f | %7.3f | %6.4f |\n", (unsigned long long)r.gt_static,
           (unsigned long long)r.gt_dynamic, (unsigned long long)r.est_static, (unsigned long long)r.est_dynamic,
           (unsigned long long)r.preserved_static, (unsigned long long)r.preserved_dynamic, r.PR, r.RR, r.F1);
    if (r.n_tied || r.n_label_out_of_range)
        printf("(%llu ground-truth point(s) with an equidistant nearest point of the other class, %llu label(s) out of range)\n",
               (unsigned long long)r.n_tied, (unsigned long long)r.n_label_out_of_range);
}
static int evaluate_host(erasor_hip_handle *h, const std::vector<float> &gt, const std::vector<float> &est, double voxel_leaf, double voxelsize) {
    erasor_eval_result r;
    const int rc = erasor_hip_evaluate_clouds(h, gt.data(), gt.size() / 4, 0, est.data(), est.size() / 4, 0, voxel_leaf, voxelsize, nullptr, &r);
    if (rc) {
        fprintf(stderr, "evaluate: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        return 1;
    }
    print_eval_row(r);
    return 0;
}
// --eval <gt> <est> [voxelsize = 0.2] [voxel_leaf = 0]: analysis_runner.py's evaluation of two map files, on the device
static int eval_mode(int argc, char **argv) {
    if (argc < 4) return 2;
    const double voxelsize = argc > 4 ? atof(argv[4]) : 0.2, voxel_leaf = argc > 5 ? atof(argv[5]) : 0.0;
    std::vector<float> gt, est;
    if (!load_cloud_xyzi(argv[2], gt) || !load_cloud_xyzi(argv[3], est)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    printf("GT : %s\nEst: %s\n", argv[2], argv[3]);
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    const int rc = evaluate_host(h, gt, est, voxel_leaf, voxelsize);
    erasor_hip_destroy(h);
    return rc;
}
// ---- bird's-eye images (viz_kitti_map.cpp / compare_map.cpp as PPM files: erasor_hip_render_*) ----
extern "C" int erasor_shim_write_ppm(const char *path, const uint8_t *rgb, uint32_t width, uint32_t height);
static const char *const RENDER_CAT_NAMES[ERASOR_RENDER_NCAT] = {"static", "dynamic", "target", "height", "static kept", "dynamic removed",
                                                                 "static lost", "dynamic left"};
static void print_view_and_stats(const erasor_render_view &v, const erasor_render_stats &s) {
    printf("view: x0 %.3f y0 %.3f res %g, %u x %u pixels, z %.3f .. %.3f\n", v.x0, v.y0, v.res, v.width, v.height, v.z_lo, v.z_hi);
    printf("points %llu drawn %llu outside %llu non-finite %llu, pixels hit %llu\n", (unsigned long long)s.n_points, (unsigned long long)s.n_drawn,
           (unsigned long long)s.n_outside, (unsigned long long)s.n_nonfinite, (unsigned long long)s.n_pixels_hit);
    for (int c = 0; c < ERASOR_RENDER_NCAT; ++c)
        if (s.cat_points[c])
            printf("  %-16s %10llu points %10llu pixels\n", RENDER_CAT_NAMES[c], (unsigned long long)s.cat_points[c], (unsigned long long)s.cat_pixels[c]);
}
static int render_fail(erasor_hip_handle *h, const char *what, int rc) {
    fprintf(stderr, "%s: %s (rc %d)\n", what, erasor_hip_last_error(h), rc);
    erasor_hip_destroy(h);
    return 1;
}
static erasor_hip_handle *render_handle() {
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return nullptr;
    }
    return h;
}
// --render <out.ppm> <map> [res = 0.2] [class_num] [instance]: viz_kitti_map's picture of one map -- static / dynamic / the chosen class
// (and instance) among the dynamic points
static int render_mode(int argc, char **argv) {
    if (argc < 4) return 2;
    const double res = argc > 4 ? atof(argv[4]) : 0.2;
    const int32_t cls = argc > 5 ? atoi(argv[5]) : -1, inst = argc > 6 ? atoi(argv[6]) : -1;
    std::vector<float> m;
    if (!load_cloud_xyzi(argv[3], m)) {
        fprintf(stderr, "cannot read %s\n", argv[3]);
        return 3;
    }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    erasor_render_view v;
    erasor_render_stats st;
    int rc = erasor_hip_render_fit(h, m.data(), m.size() / 4, 0, res, 2, 0x000000, &v);
    if (rc) return render_fail(h, "render_fit", rc);
    std::vector<uint8_t> rgb((size_t)v.width * v.height * 3);
    if ((rc = erasor_hip_render_clouds(h, m.data(), m.size() / 4, 0, ERASOR_RENDER_LABEL, cls, inst, &v, rgb.data(), 0, &st)))
        return render_fail(h, "render", rc);
    erasor_hip_destroy(h);
    print_view_and_stats(v, st);
    if (erasor_shim_write_ppm(argv[2], rgb.data(), v.width, v.height) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 3;
    }
    return 0;
}
// --render-compare <out.ppm> <res> <gt> <est1> [<est2> ...]: compare_map.cpp's side-by-side picture -- one panel per file, left to right,
// all in the view fitted to the first, 4 background pixels between neighbours
static int render_compare_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    const double res = atof(argv[3]);
    const int k = argc - 4;
    const uint32_t gap = 4;
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    erasor_render_view v;
    std::vector<uint8_t> out, rgb;
    uint32_t W = 0;
    for (int j = 0; j < k; ++j) {
        std::vector<float> m;
        if (!load_cloud_xyzi(argv[4 + j], m)) {
            fprintf(stderr, "cannot read %s\n", argv[4 + j]);
            erasor_hip_destroy(h);
            return 3;
        }
        int rc;
        if (j == 0) {
            if ((rc = erasor_hip_render_fit(h, m.data(), m.size() / 4, 0, res, 2, 0x000000, &v))) return render_fail(h, "render_fit", rc);
            W = v.width * k + gap * (k - 1);
            out.assign((size_t)W * v.height * 3, 0);
            rgb.resize((size_t)v.width * v.height * 3);
        }
        erasor_render_stats st;
        if ((rc = erasor_hip_render_clouds(h, m.data(), m.size() / 4, 0, ERASOR_RENDER_LABEL, -1, -1, &v, rgb.data(), 0, &st)))
            return render_fail(h, "render", rc);
        printf("panel %d: %s\n", j, argv[4 + j]);
        print_view_and_stats(v, st);
        for (uint32_t r = 0; r < v.height; ++r)
            memcpy(&out[((size_t)r * W + (size_t)j * (v.width + gap)) * 3], &rgb[(size_t)r * v.width * 3], (size_t)v.width * 3);
    }
    erasor_hip_destroy(h);
    printf("%d panel(s), %u x %u pixels\n", k, W, v.height);
    if (erasor_shim_write_ppm(argv[2], out.data(), W, v.height) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 3;
    }
    return 0;
}
// --render-eval <out.ppm> <gt> <est> [voxelsize = 0.2] [voxel_leaf = 0] [res = 0.2]: --eval's table, and the error map -- the ground truth
// coloured by the evaluation's decision per point
static int render_eval_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    const double voxelsize = argc > 5 ? atof(argv[5]) : 0.2, voxel_leaf = argc > 6 ? atof(argv[6]) : 0.0, res = argc > 7 ? atof(argv[7]) : 0.2;
    std::vector<float> gt, est;
    if (!load_cloud_xyzi(argv[3], gt) || !load_cloud_xyzi(argv[4], est)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[3], argv[4]);
        return 3;
    }
    printf("GT : %s\nEst: %s\n", argv[3], argv[4]);
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    erasor_render_view v;
    erasor_render_stats st;
    erasor_eval_result r;
    int rc = erasor_hip_render_fit(h, gt.data(), gt.size() / 4, 0, res, 2, 0x000000, &v);
    if (rc) return render_fail(h, "render_fit", rc);
    std::vector<uint8_t> rgb((size_t)v.width * v.height * 3);
    if ((rc = erasor_hip_render_eval_clouds(h, gt.data(), gt.size() / 4, 0, est.data(), est.size() / 4, 0, voxel_leaf, voxelsize, &v, rgb.data(), 0, &st,
                                            &r)))
        return render_fail(h, "render_eval", rc);
    erasor_hip_destroy(h);
    print_eval_row(r);
    print_view_and_stats(v, st);
    if (erasor_shim_write_ppm(argv[2], rgb.data(), v.width, v.height) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 3;
    }
    return 0;
}
// the public SemanticKITTI label names (semantic-kitti.yaml) of a class key
static const char *semantic_kitti_name(uint32_t key) {
    switch (key) {
        case 0: return "unlabeled";        case 1: return "outlier";            case 10: return "car";
        case 11: return "bicycle";         case 13: return "bus";               case 15: return "motorcycle";
        case 16: return "on-rails";        case 18: return "truck";             case 20: return "other-vehicle";
        case 30: return "person";          case 31: return "bicyclist";         case 32: return "motorcyclist";
        case 40: return "road";            case 44: return "parking";           case 48: return "sidewalk";
        case 49: return "other-ground";    case 50: return "building";          case 51: return "fence";
        case 52: return "other-structure"; case 60: return "lane-marking";      case 70: return "vegetation";
        case 71: return "trunk";           case 72: return "terrain";           case 80: return "pole";
        case 81: return "traffic-sign";    case 99: return "other-object";      case 252: return "moving-car";
        case 253: return "moving-bicyclist"; case 254: return "moving-person";  case 255: return "moving-motorcyclist";
        case 256: return "moving-on-rails";  case 257: return "moving-bus";     case 258: return "moving-truck";
        case 259: return "moving-other-vehicle";
        case ERASOR_EVAL_KEY_LABEL_OUT_OF_RANGE: return "(label out of range)";
        default: return "-";
    }
}
// --eval-classes <gt> <est> [voxelsize = 0.2] [voxel_leaf = 0]: --eval's output, then PR / RR per class and a summary of the dynamic
// instances of the ground truth (erasor_hip_evaluate_clouds_by_class)
static int eval_classes_mode(int argc, char **argv) {
    if (argc < 4) return 2;
    const double voxelsize = argc > 4 ? atof(argv[4]) : 0.2, voxel_leaf = argc > 5 ? atof(argv[5]) : 0.0;
    std::vector<float> gt, est;
    if (!load_cloud_xyzi(argv[2], gt) || !load_cloud_xyzi(argv[3], est)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    printf("GT : %s\nEst: %s\n", argv[2], argv[3]);
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    std::vector<erasor_eval_class_row> cls(ERASOR_EVAL_KEY_LABEL_OUT_OF_RANGE + 1), inst(4096);
    size_t nc = 0, ni = 0;
    erasor_eval_result r;
    int rc = ERASOR_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {  // (again with the instances' exact count when they did not fit)
        rc = erasor_hip_evaluate_clouds_by_class(h, gt.data(), gt.size() / 4, 0, est.data(), est.size() / 4, 0, voxel_leaf, voxelsize, cls.data(),
                                                 cls.size(), &nc, inst.data(), inst.size(), &ni, &r);
        if (rc != ERASOR_E_CAPACITY) break;
        inst.resize(std::max<size_t>(ni, 1));
    }
    if (rc) {
        fprintf(stderr, "evaluate: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    print_eval_row(r);
    printf("\nper class:\n");
    printf("|    key | name                 |       gt |     kept |   PR%%/RR%% |      est |\n");
    printf("|--------+----------------------+----------+----------+-----------+----------|\n");
    for (size_t k = 0; k < nc; ++k) {
        const erasor_eval_class_row &c = cls[k];
        const double n = (double)c.n_gt, kept = (double)c.n_preserved;
        const double rate = c.n_gt ? (c.is_dynamic ? (n - kept) / n * 100.0 : kept / n * 100.0) : 0.0;
        printf("| %6u | %-20s | %8llu | %8llu | %s %7.3f | %8llu |\n", c.key, semantic_kitti_name(c.key), (unsigned long long)c.n_gt,
               (unsigned long long)c.n_preserved, c.is_dynamic ? "RR" : "PR", rate, (unsigned long long)c.n_est);
    }
    size_t in_gt = 0, all = 0, ge90 = 0, ge50 = 0, none = 0;
    for (size_t k = 0; k < ni; ++k) {
        const erasor_eval_class_row &c = inst[k];
        if (!c.n_gt) continue;
        ++in_gt;
        const uint64_t removed = c.n_gt - c.n_preserved;
        all += removed == c.n_gt;
        ge90 += removed * 10 >= c.n_gt * 9;
        ge50 += removed * 2 >= c.n_gt;
        none += removed == 0;
    }
    printf("\ndynamic instances in the ground truth: %zu; fully removed %zu, >= 90%% removed %zu, >= 50%% removed %zu, not removed %zu\n", in_gt, all,
           ge90, ge50, none);
    erasor_hip_destroy(h);
    return 0;
}
// --analyze <gt> <est> [voxelsize = 0.2] [voxel_leaf = 0]: analysis_runner.py's main() on the device -- the two files, the overlap
// report (analysis_runner.py:53-71, erasor_hip_overlap_clouds; printf's %.4f / %.2f round the binary value exactly, as Python's format
// does) and the PR / RR row
static int analyze_mode(int argc, char **argv) {
    if (argc < 4) return 2;
    const double voxelsize = argc > 4 ? atof(argv[4]) : 0.2, voxel_leaf = argc > 5 ? atof(argv[5]) : 0.0;
    std::vector<float> gt, est;
    if (!load_cloud_xyzi(argv[2], gt) || !load_cloud_xyzi(argv[3], est)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    printf("GT : %s\nEst: %s\n", argv[2], argv[3]);
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    erasor_overlap_result o;
    int rc = erasor_hip_overlap_clouds(h, gt.data(), gt.size() / 4, 0, est.data(), est.size() / 4, 0, voxel_leaf, voxelsize, nullptr, nullptr, &o);
    if (rc) {
        fprintf(stderr, "overlap: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    const double half = 0.5 * voxelsize, one = voxelsize;
    printf("est->GT dist: median=%.4fm  p90=%.4fm  p99=%.4fm  max=%.4fm\n", o.median, o.p90, o.p99, o.max);
    printf("  fraction <0.5*v (%.2fm): %.2f%%  <1*v (%.2fm): %.2f%%  <2*v (%.2fm): %.2f%%\n", half, o.frac_half, one, o.frac_one, 2 * one,
           o.frac_two);
    rc = evaluate_host(h, gt, est, voxel_leaf, voxelsize);
    erasor_hip_destroy(h);
    return rc;
}
static void rows_to_cloud(const std::vector<float> &rows, size_t n, pcl::PointCloud<pcl::PointXYZI> &c) {
    c.points.resize(n);
    for (size_t i = 0; i < n; ++i) {
        c.points[i].x = rows[4 * i];
        c.points[i].y = rows[4 * i + 1];
        c.points[i].z = rows[4 * i + 2];
        c.points[i].intensity = rows[4 * i + 3];
    }
    c.width = (unsigned)n;
    c.height = 1;
}
// --label <map> <dense_labelled> [leaf = 0.2]: fill_removert_intensity.cpp's main() (:61-111) on the device -- label_map
// (erasor_hip_label_map) of a map without labels (another method's output, or one cleaned with intensity = 0) from the dense labelled
// map, saved as <map minus its 4-character extension>_w_label.pcd in ASCII; prints "n_src - > n_out" as label_map does (:38)
static int label_mode(int argc, char **argv) {
    if (argc < 4) return 2;
    const double leaf = argc > 4 ? atof(argv[4]) : 0.2;
    std::vector<float> src, medium;
    if (!load_cloud_xyzi(argv[2], src) || !load_cloud_xyzi(argv[3], medium)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    const size_t n_src = src.size() / 4;
    std::vector<float> rows(std::max<size_t>(n_src, 1) * 4);
    erasor_label_result r;
    const int rc = erasor_hip_label_map(h, src.data(), n_src, 0, medium.data(), medium.size() / 4, 0, leaf, rows.data(), n_src, &r);
    if (rc) {
        fprintf(stderr, "label_map: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    erasor_hip_destroy(h);
    printf("%llu - > %llu\n", (unsigned long long)r.n_src, (unsigned long long)r.n_out);
    if (r.n_tied || r.passthrough)
        printf("(%llu point(s) with equidistant medium points of different labels%s)\n", (unsigned long long)r.n_tied,
               r.passthrough ? "; voxel index overflow: the map was labelled as it is" : "");
    pcl::PointCloud<pcl::PointXYZI> out;
    rows_to_cloud(rows, r.n_out, out);
    std::string name = argv[2];
    name.erase(name.size() >= 4 ? name.size() - 4 : 0);  // (the reference drops the last four characters: ".pcd")
    const std::string save_name = name + "_w_label.pcd";
    if (erasor_utils::save_pcd_ascii(save_name, out) != 0) {
        fprintf(stderr, "cannot write %s\n", save_name.c_str());
        return 1;
    }
    printf("saved %s\n", save_name.c_str());
    return 0;
}
// --complement <est> <gt> <out.pcd>: calc_complement (compare_complement.cpp:43-75) on the device -- the static ground-truth points
// the estimate lost (erasor_hip_static_complement), saved as <out.pcd> in ASCII
static int complement_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    std::vector<float> est, gt;
    if (!load_cloud_xyzi(argv[2], est) || !load_cloud_xyzi(argv[3], gt)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    const size_t n_gt = gt.size() / 4;
    std::vector<float> rows(std::max<size_t>(n_gt, 1) * 4);
    erasor_complement_result r;
    const int rc = erasor_hip_static_complement(h, est.data(), est.size() / 4, 0, gt.data(), n_gt, 0, rows.data(), n_gt, &r);
    if (rc) {
        fprintf(stderr, "static_complement: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    erasor_hip_destroy(h);
    printf("%llu of %llu static ground-truth point(s) lost\n", (unsigned long long)r.n_lost, (unsigned long long)r.n_gt_static);
    pcl::PointCloud<pcl::PointXYZI> out;
    rows_to_cloud(rows, r.n_lost, out);
    if (erasor_utils::save_pcd_ascii(argv[4], out) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[4]);
        return 1;
    }
    printf("saved %s\n", argv[4]);
    return 0;
}
// ---- a cloud as connected objects (erasor_hip_cluster_clouds) ----
// a number argument read whole: false on anything else
static bool parse_number(const char *a, double *v) {
    char *end = nullptr;
    *v = strtod(a, &end);
    return end != a && *end == '\0' && std::isfinite(*v);
}
static bool parse_count(const char *a, size_t *v) {
    double d = 0;
    if (!parse_number(a, &d) || d < 0 || d != floor(d) || d > 4294967295.0) return false;
    *v = (size_t)d;
    return true;
}
// the result line and the twenty largest listed clusters (ties: the lower `first`): size, dynamic share, box
static void print_clusters(const erasor_cluster_result &r, std::vector<erasor_cluster_row> rows) {
    printf("clusters: n=%llu  clusters=%llu  listed=%llu  points listed=%llu  singletons=%llu  largest=%llu\n", (unsigned long long)r.n_points,
           (unsigned long long)r.n_clusters, (unsigned long long)r.n_listed, (unsigned long long)r.n_points_listed, (unsigned long long)r.n_singletons,
           (unsigned long long)r.largest);
    std::stable_sort(rows.begin(), rows.end(), [](const erasor_cluster_row &a, const erasor_cluster_row &b) { return a.n_points > b.n_points; });
    for (size_t k = 0; k < rows.size() && k < 20; ++k) {
        const erasor_cluster_row &c = rows[k];
        printf("  first=%u  n=%u  dynamic=%u (%.1f%%)  box=[%.3f %.3f %.3f]..[%.3f %.3f %.3f]\n", c.first, c.n_points, c.n_dynamic,
               100.0 * (double)c.n_dynamic / (double)c.n_points, c.min_xyz[0], c.min_xyz[1], c.min_xyz[2], c.max_xyz[0], c.max_xyz[1], c.max_xyz[2]);
    }
}
// the clustering of a host cloud: the rows (all of them), optionally the kept cloud; 0, or 1 after printing the error
static int cluster_host(erasor_hip_handle *h, const std::vector<float> &cloud, double tol, size_t min_size, size_t max_size, erasor_cluster_result *r,
                        std::vector<erasor_cluster_row> *rows, std::vector<float> *kept) {
    const size_t n = cloud.size() / 4;
    rows->assign(std::max<size_t>(n, 1), erasor_cluster_row());
    if (kept) kept->assign(std::max<size_t>(n, 1) * 4, 0.f);
    const int rc = erasor_hip_cluster_clouds(h, cloud.data(), n, 0, tol, min_size, max_size, nullptr, rows->data(), rows->size(), kept ? kept->data() : nullptr,
                                             kept ? n : 0, r);
    if (rc) {
        fprintf(stderr, "cluster: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        return 1;
    }
    rows->resize(r->n_listed);
    if (kept) kept->resize(r->n_points_listed * 4);
    return 0;
}
// --clusters <cloud.pcd> <tol> [min_size = 1] [max_size = 0] [kept_out.pcd]: Euclidean clustering of one cloud -- the result line, the
// twenty largest clusters, and optionally the points of the listed clusters saved as a binary PCD (the residue filter)
static int clusters_mode(int argc, char **argv) {
    if (argc < 4 || argc > 7) return 2;
    double tol = 0;
    size_t min_size = 1, max_size = 0;
    if (!parse_number(argv[3], &tol) || !(tol > 0)) return 2;
    if ((argc > 4 && !parse_count(argv[4], &min_size)) || (argc > 5 && !parse_count(argv[5], &max_size))) return 2;
    std::vector<float> cloud;
    if (!load_cloud_xyzi(argv[2], cloud)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    erasor_cluster_result r;
    std::vector<erasor_cluster_row> rows;
    std::vector<float> kept;
    const int rc = cluster_host(h, cloud, tol, min_size, max_size, &r, &rows, argc > 6 ? &kept : nullptr);
    erasor_hip_destroy(h);
    if (rc) return rc;
    print_clusters(r, rows);
    if (argc > 6) {
        pcl::PointCloud<pcl::PointXYZI> out;
        rows_to_cloud(kept, r.n_points_listed, out);
        if (erasor_utils::save_pcd_binary(argv[6], out) != 0) {
            fprintf(stderr, "cannot write %s\n", argv[6]);
            return 1;
        }
        printf("saved %s\n", argv[6]);
    }
    return 0;
}
// --residue <gt> <est> [tol = 0.5] [voxelsize = 0.2] [voxel_leaf = 0]: the ghost objects a method left -- the ground truth's dynamic points
// that --eval counts as kept, clustered (no instance labels needed)
static int residue_mode(int argc, char **argv) {
    if (argc < 4 || argc > 7) return 2;
    double tol = 0.5, voxelsize = 0.2, voxel_leaf = 0.0;
    if ((argc > 4 && (!parse_number(argv[4], &tol) || !(tol > 0))) || (argc > 5 && (!parse_number(argv[5], &voxelsize) || !(voxelsize > 0))) ||
        (argc > 6 && (!parse_number(argv[6], &voxel_leaf) || voxel_leaf < 0)))
        return 2;
    std::vector<float> gt, est;
    if (!load_cloud_xyzi(argv[2], gt) || !load_cloud_xyzi(argv[3], est)) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    if (voxel_leaf > 0)
        for (std::vector<float> *c : {&gt, &est}) {
            std::vector<float> out(std::max<size_t>(c->size(), 4));
            size_t n_out = 0;
            const int rc = erasor_hip_voxelize_preserving_labels(h, c->data(), c->size() / 4, voxel_leaf, out.data(), out.size() / 4, &n_out);
            if (rc) return render_fail(h, "voxelize", rc);
            out.resize(n_out * 4);
            c->swap(out);
        }
    const size_t n_gt = gt.size() / 4;
    std::vector<uint8_t> code(std::max<size_t>(n_gt, 1));
    erasor_eval_result e;
    int rc = erasor_hip_evaluate_clouds(h, gt.data(), n_gt, 0, est.data(), est.size() / 4, 0, 0.0, voxelsize, code.data(), &e);
    if (rc) return render_fail(h, "evaluate", rc);
    std::vector<float> left;
    for (size_t i = 0; i < n_gt; ++i)
        if (code[i] == ERASOR_EVAL_KEPT_DYNAMIC) left.insert(left.end(), gt.begin() + 4 * i, gt.begin() + 4 * i + 4);
    erasor_cluster_result r;
    std::vector<erasor_cluster_row> rows;
    rc = cluster_host(h, left, tol, 1, 0, &r, &rows, nullptr);
    erasor_hip_destroy(h);
    if (rc) return rc;
    printf("residue: %llu of %llu dynamic ground-truth point(s) left\n", (unsigned long long)e.preserved_dynamic, (unsigned long long)e.gt_dynamic);
    print_clusters(r, rows);
    return 0;
}
// ---- the decision per object (erasor_hip_object_vote_clouds) ----
// near[i] = the cloud `ref` has a point within tau of raw point i: erasor_hip_label_scans_clouds with `ref` as the static map and the raw
// map as one frame under identity poses -- code 0 (static) is "within tau", code 1 (dynamic) is not.  An empty `ref` (a method that
// removed everything) is near nothing: every raw point is voted by it.  On failure the error is printed and the handle destroyed
// (render_fail): the caller returns at once.
static int near_cloud(erasor_hip_handle *h, const std::vector<float> &ref, const std::vector<float> &raw, double tau, std::vector<uint8_t> *near) {
    const size_t n = raw.size() / 4;
    const uint64_t offsets[2] = {0, (uint64_t)n};
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    erasor_scan_label_row row;
    std::vector<uint8_t> codes(std::max<size_t>(n, 1));
    const int rc = erasor_hip_label_scans_clouds(h, ref.data(), ref.size() / 4, 0, nullptr, 0, 0, 0, raw.data(), n, offsets, 1, 0, nullptr, I, tau, codes.data(), 0,
                                                 nullptr, 0, nullptr, &row, nullptr);
    if (rc) return render_fail(h, "label_scans", rc);
    near->resize(n);
    for (size_t i = 0; i < n; ++i) (*near)[i] = codes[i] == 0 ? 1 : 0;
    return 0;
}
// --objects <raw.pcd> <ground.pcd|-> <out.pcd> <tol> <vote_thr> <remove_ratio> <revert_ratio> <max_size> <kept1.pcd> [<kept2.pcd> ...]
// [--tau t]: the votes of one or more removal methods decided per object.  A raw point is voted by kept_j iff kept_j has no point within
// tau of it (default 0.2 * sqrt(3) / 2, the evaluator's threshold), so kept clouds that are subsets of the raw map (--visibility, --carve)
// and a voxelised ERASOR map both work; it is ground iff <ground.pcd> (what --ground-map writes; "-": no ground mask) has a point within
// tau.  Prints the result, the twenty largest touched clusters and one line per decision, and saves the kept cloud as a binary PCD.
static int objects_mode(int argc, char **argv) {
    double tau = 0.2 * sqrt(3.0) / 2.0;
    if (argc >= 4 && std::string(argv[argc - 2]) == "--tau") {
        if (!parse_number(argv[argc - 1], &tau) || !(tau > 0)) return 2;
        argc -= 2;
    }
    if (argc < 11) return 2;
    erasor_object_vote_params P;
    memset(&P, 0, sizeof(P));
    size_t thr = 0, max_size = 0;
    if (!parse_number(argv[5], &P.tol) || !(P.tol > 0) || !parse_count(argv[6], &thr) || thr < 1 || thr > 255 || !parse_number(argv[7], &P.remove_ratio) ||
        !(P.remove_ratio > 0 && P.remove_ratio <= 1) || !parse_number(argv[8], &P.revert_ratio) ||
        !(P.revert_ratio >= 0 && P.revert_ratio < 1 && P.revert_ratio < P.remove_ratio) || !parse_count(argv[9], &max_size))
        return 2;
    P.vote_thr = (uint32_t)thr, P.max_size = max_size, P.min_size = 1, P.min_voted = 1, P.ground_keep = 1;
    const bool have_ground = std::string(argv[3]) != "-";
    std::vector<float> raw, gnd;
    std::vector<std::vector<float>> kept_in(argc - 10);
    if (!load_cloud_xyzi(argv[2], raw)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    if (have_ground && !load_cloud_xyzi(argv[3], gnd)) {
        fprintf(stderr, "cannot read %s\n", argv[3]);
        return 3;
    }
    for (int k = 10; k < argc; ++k)
        if (!load_cloud_xyzi(argv[k], kept_in[k - 10])) {
            fprintf(stderr, "cannot read %s\n", argv[k]);
            return 3;
        }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n = raw.size() / 4;
    std::vector<uint8_t> votes(std::max<size_t>(n, 1), 0), ground, near;
    for (const std::vector<float> &k : kept_in) {
        if (near_cloud(h, k, raw, tau, &near)) return 1;
        for (size_t i = 0; i < n; ++i)
            if (!near[i] && votes[i] < 255) ++votes[i];
    }
    if (have_ground && near_cloud(h, gnd, raw, tau, &ground)) return 1;
    if (have_ground && !n) ground.assign(1, 0);
    std::vector<uint8_t> mask(std::max<size_t>(n, 1));
    std::vector<erasor_object_row> rows(std::max<size_t>(n, 1));
    std::vector<float> kept(std::max<size_t>(n, 1) * 4);
    erasor_object_vote_result r;
    const int rc = erasor_hip_object_vote_clouds(h, raw.data(), n, 0, votes.data(), have_ground ? ground.data() : nullptr, &P, mask.data(), nullptr, rows.data(),
                                                 rows.size(), kept.data(), n, &r);
    if (rc) return render_fail(h, "object_vote", rc);
    erasor_hip_destroy(h);  // (the handle's last use: nothing below needs it, a failed write included)
    rows.resize(r.n_touched);
    typedef unsigned long long ull;
    printf("objects: n=%llu  ground=%llu  clusters=%llu  touched=%llu  removed=%llu  reverted=%llu  not objects=%llu  largest=%llu\n", (ull)r.n_points,
           (ull)r.n_ground, (ull)r.n_clusters, (ull)r.n_touched, (ull)r.n_removed_clusters, (ull)r.n_reverted_clusters, (ull)r.n_not_object, (ull)r.largest);
    printf("points: voted=%llu  removed=%llu  grown=%llu (dynamic %llu)  reverted=%llu (dynamic %llu)  ground reverted=%llu (dynamic %llu)\n", (ull)r.n_voted,
           (ull)r.n_removed, (ull)r.n_grown, (ull)r.n_grown_dynamic, (ull)r.n_reverted, (ull)r.n_reverted_dynamic, (ull)r.n_ground_reverted,
           (ull)r.n_ground_reverted_dynamic);
    static const char *const NAMES[4] = {"unchanged", "removed", "reverted", "not an object"};
    ull n_cl[4] = {0, 0, 0, 0}, n_pt[4] = {0, 0, 0, 0}, n_dyn[4] = {0, 0, 0, 0};
    for (const erasor_object_row &c : rows) {
        const uint32_t d = c.decision & 3u;
        ++n_cl[d], n_pt[d] += c.n_points, n_dyn[d] += c.n_dynamic;
    }
    std::stable_sort(rows.begin(), rows.end(), [](const erasor_object_row &a, const erasor_object_row &b) { return a.n_points > b.n_points; });
    for (size_t k = 0; k < rows.size() && k < 20; ++k) {
        const erasor_object_row &c = rows[k];
        printf("  first=%u  n=%u  voted=%u  dynamic=%u (%.1f%%)  %s  box=[%.3f %.3f %.3f]..[%.3f %.3f %.3f]\n", c.first, c.n_points, c.n_voted, c.n_dynamic,
               100.0 * (double)c.n_dynamic / (double)c.n_points, NAMES[c.decision & 3u], c.min_xyz[0], c.min_xyz[1], c.min_xyz[2], c.max_xyz[0], c.max_xyz[1],
               c.max_xyz[2]);
    }
    for (int d = 0; d < 4; ++d)
        printf("%s: clusters=%llu  points=%llu  dynamic=%llu (%.1f%%)\n", NAMES[d], n_cl[d], n_pt[d], n_dyn[d], n_pt[d] ? 100.0 * (double)n_dyn[d] / (double)n_pt[d] : 0.0);
    pcl::PointCloud<pcl::PointXYZI> out;
    rows_to_cloud(kept, r.n_points - r.n_removed, out);
    if (erasor_utils::save_pcd_binary(argv[4], out) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[4]);
        return 1;
    }
    printf("saved %s\n", argv[4]);
    return 0;
}
// ---- how dense a cloud is around each point, and the outlier filters on that (erasor_hip_knn_clouds, erasor_hip_density_filter_clouds) ----
static void print_stats(const char *name, double mn, double median, double p90, double p99, double mx) {
    printf("  %s: min=%.9g  median=%.9g  p90=%.9g  p99=%.9g  max=%.9g\n", name, mn, median, p90, p99, mx);
}
// --denoise <in.pcd> <out.pcd> sor <k> <mul> | ror <radius> <min_neighbors> | kth <k> <thr>: the cloud without its stragglers, saved as a
// binary PCD.  sor: the mean distance to the k nearest neighbours against median + mul * 1.4826 * MAD (pcl::StatisticalOutlierRemoval's
// selection, with a median and a MAD where PCL has a mean and a sigma); ror: at least min_neighbors other points within radius
// (pcl::RadiusOutlierRemoval); kth: the k-th neighbour no farther than thr.
static int denoise_mode(int argc, char **argv) {
    if (argc != 7) return 2;
    const std::string how = argv[4];
    erasor_density_filter f;
    memset(&f, 0, sizeof(f));
    double a = 0, b = 0;
    size_t cnt = 0;
    if (how == "sor" || how == "kth") {
        if (!parse_count(argv[5], &cnt) || cnt < 1 || cnt > 32 || !parse_number(argv[6], &b) || b < 0) return 2;
        f.k = (uint32_t)cnt;
        f.score = how == "sor" ? ERASOR_DENSITY_MEAN : ERASOR_DENSITY_KTH;
        f.rule = how == "sor" ? ERASOR_DENSITY_MAD : ERASOR_DENSITY_ABS;
        (how == "sor" ? f.mul : f.thr) = b;
    } else if (how == "ror") {
        if (!parse_number(argv[5], &a) || !(a > 0) || !parse_count(argv[6], &cnt)) return 2;
        f.score = ERASOR_DENSITY_COUNT;
        f.rule = ERASOR_DENSITY_ABS;
        f.radius = a;
        f.min_neighbors = (uint32_t)cnt;
    } else {
        return 2;
    }
    std::vector<float> cloud;
    if (!load_cloud_xyzi(argv[2], cloud)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n = cloud.size() / 4;
    std::vector<float> kept(std::max<size_t>(n, 1) * 4, 0.f);
    erasor_density_result r;
    const int rc = erasor_hip_density_filter_clouds(h, cloud.data(), n, 0, &f, nullptr, kept.data(), n, &r);
    if (rc) return render_fail(h, "density_filter", rc);
    erasor_hip_destroy(h);
    printf("denoise: n=%llu  kept=%llu  removed=%llu (dynamic %llu, static %llu)  short=%llu  scored=%llu\n", (unsigned long long)r.n_points,
           (unsigned long long)r.n_kept, (unsigned long long)r.n_removed, (unsigned long long)r.n_removed_dynamic, (unsigned long long)r.n_removed_static,
           (unsigned long long)r.n_short, (unsigned long long)r.n_scored);
    print_stats(how == "sor" ? "mean" : (how == "ror" ? "count" : "kth"), r.min, r.median, r.p90, r.p99, r.max);
    printf("  m=%.9g  mad=%.9g  thr=%.9g\n", r.m, r.mad, r.thr);
    pcl::PointCloud<pcl::PointXYZI> out;
    rows_to_cloud(kept, r.n_kept, out);
    if (erasor_utils::save_pcd_binary(argv[3], out) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 1;
    }
    printf("saved %s\n", argv[3]);
    return 0;
}
// --density <cloud.pcd> <k>: the statistics of the k-th neighbour's distance and of the mean distance to the k nearest, nothing written
static int density_mode(int argc, char **argv) {
    if (argc != 4) return 2;
    size_t k = 0;
    if (!parse_count(argv[3], &k) || k < 1 || k > 32) return 2;
    std::vector<float> cloud;
    if (!load_cloud_xyzi(argv[2], cloud)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    erasor_knn_result r;
    const int rc = erasor_hip_knn_clouds(h, cloud.data(), cloud.size() / 4, 0, (uint32_t)k, nullptr, nullptr, nullptr, nullptr, &r);
    if (rc) return render_fail(h, "knn", rc);
    erasor_hip_destroy(h);
    printf("density: n=%llu  k=%u  short=%llu  scored=%llu\n", (unsigned long long)r.n_points, (unsigned)k, (unsigned long long)r.n_short,
           (unsigned long long)r.kth.n_scored);
    print_stats("kth", r.kth.min, r.kth.median, r.kth.p90, r.kth.p99, r.kth.max);
    print_stats("mean", r.mean.min, r.mean.median, r.mean.p90, r.mean.p99, r.mean.max);
    return 0;
}
// --normals <in.pcd> <out.pcd> <k> [vx vy vz]: every point's surface normal and curvature from its k nearest neighbours
// (erasor_hip_normals_clouds; pcl::NormalEstimation's job), turned towards the viewpoint or, without one, upwards; the counts, the
// curvature's statistics, and the cloud saved as a binary PCD with the fields x y z intensity normal_x normal_y normal_z curvature
static int normals_mode(int argc, char **argv) {
    if (argc != 5 && argc != 8) return 2;
    size_t k = 0;
    if (!parse_count(argv[4], &k) || k < 2 || k > 32) return 2;
    double view[3] = {0, 0, 0};
    if (argc == 8)
        for (int a = 0; a < 3; ++a)
            if (!parse_number(argv[5 + a], &view[a]) || !std::isfinite(view[a])) return 2;
    std::vector<float> cloud;
    if (!load_cloud_xyzi(argv[2], cloud)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n = cloud.size() / 4;
    std::vector<float> nrm(std::max<size_t>(n, 1) * 3, 0.f);
    std::vector<double> curv(std::max<size_t>(n, 1), 0.0);
    erasor_normals_result r;
    const int rc = erasor_hip_normals_clouds(h, cloud.data(), n, 0, (uint32_t)k, argc == 8 ? view : nullptr, nrm.data(), curv.data(), nullptr, &r);
    if (rc) return render_fail(h, "normals", rc);
    erasor_hip_destroy(h);
    printf("normals: n=%llu  k=%u  short=%llu  degenerate=%llu  ambiguous=%llu  flipped=%llu  scored=%llu\n", (unsigned long long)r.n_points, (unsigned)k,
           (unsigned long long)r.n_short, (unsigned long long)r.n_degenerate, (unsigned long long)r.n_ambiguous, (unsigned long long)r.n_flipped,
           (unsigned long long)r.curvature.n_scored);
    print_stats("curvature", r.curvature.min, r.curvature.median, r.curvature.p90, r.curvature.p99, r.curvature.max);
    std::vector<float> curv32(curv.begin(), curv.end());
    if (erasor_utils::save_pcd_normals_binary(argv[3], cloud.data(), nrm.data(), curv32.data(), n) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 1;
    }
    printf("saved %s\n", argv[3]);
    return 0;
}
// --eval-many <voxelsize> <voxel_leaf> <gt> <est1> [<est2> ...]: --eval's row for every estimate against one ground truth, from ONE
// erasor_hip_evaluate_many call (compare_map.cpp's use: several methods' maps against one GT)
static int eval_many_mode(int argc, char **argv) {
    if (argc < 6) return 2;
    const double voxelsize = atof(argv[2]), voxel_leaf = atof(argv[3]);
    std::vector<float> gt;
    if (!load_cloud_xyzi(argv[4], gt)) {
        fprintf(stderr, "cannot read %s\n", argv[4]);
        return 3;
    }
    const int k = argc - 5;
    std::vector<std::vector<float>> est(k);
    std::vector<const void *> ptr(k);
    std::vector<size_t> n(k);
    for (int j = 0; j < k; ++j) {
        if (!load_cloud_xyzi(argv[5 + j], est[j])) {
            fprintf(stderr, "cannot read %s\n", argv[5 + j]);
            return 3;
        }
        ptr[j] = est[j].data();
        n[j] = est[j].size() / 4;
    }
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    std::vector<erasor_eval_result> rows(k);
    const int rc = erasor_hip_evaluate_many(h, gt.data(), gt.size() / 4, 0, ptr.data(), n.data(), nullptr, k, voxel_leaf, voxelsize, rows.data());
    if (rc) {
        fprintf(stderr, "evaluate_many: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    printf("GT : %s\n", argv[4]);
    for (int j = 0; j < k; ++j) {
        printf("Est: %s\n", argv[5 + j]);
        print_eval_row(rows[j]);
    }
    erasor_hip_destroy(h);
    return 0;
}

// PR / RR of the map save_static_map(0.2) writes (voxelize_preserving_labels of map_arranged_) against a ground-truth file
static int evaluate_saved_map(erasor::OfflineMapUpdater &updater, const std::string &gt_path) {
    std::vector<float> gt;
    if (!load_cloud_xyzi(gt_path, gt)) {
        fprintf(stderr, "cannot read %s\n", gt_path.c_str());
        return 3;
    }
    pcl::PointCloud<pcl::PointXYZI> m;
    updater.get_map(m);
    std::vector<float> src(m.size() * 4), saved(m.size() * 4 + 4);
    for (size_t i = 0; i < m.size(); ++i) {
        src[4 * i] = m.points[i].x;
        src[4 * i + 1] = m.points[i].y;
        src[4 * i + 2] = m.points[i].z;
        src[4 * i + 3] = m.points[i].intensity;
    }
    size_t n = 0;
    erasor_hip_handle *h = updater.handle();
    if (erasor_hip_voxelize_preserving_labels(h, src.data(), m.size(), 0.2, saved.data(), m.size() + 1, &n) != ERASOR_OK) {
        fprintf(stderr, "voxelize_preserving_labels: %s\n", erasor_hip_last_error(h));
        return 1;
    }
    saved.resize(n * 4);
    printf("PR / RR of the saved static map against %s:\n", gt_path.c_str());
    return evaluate_host(h, gt, saved, 0.0, 0.2);
}

// --config <rosparam.yaml> [n_frames] [gt]: the reference's own driver, main_in_your_env.cpp:61-127, without ROS:
//   <data_dir>/poses_lidar2body.csv, <data_dir>/pcds/%06d.pcd from init_idx on, every node through
//   OfflineMapUpdater::callback_node (pose -> eigen2geoPose -> node.odom), then save_static_map(0.2).
// The initial map is /MapUpdater/initial_map_path, or <data_dir>/dense_global_map.pcd when that key is absent.
// With a ground-truth map file `gt` (PCD or .bin), the PR / RR of the saved map are printed (analysis_runner.py's row).
static int run_config(const std::string &yaml, int max_frames, int device, bool verbose, int *nodes_done = nullptr, const std::string &gt = "") {
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    cfg.params.query_voxel_size = 0.05;  // OMU.cpp:66
    cfg.params.removal_interval = 2;     // OMU.cpp:69
    cfg.verbose = verbose;               // OMU.cpp:83
    cfg.device = device;
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(yaml, cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", yaml.c_str());
        return 3;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    if (cfg.save_path == "/" || cfg.save_path == ".") cfg.save_path = drv.data_dir;
    erasor::OfflineMapUpdater updater(cfg);
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    printf("Total %zu poses are loaded\n", poses.size() + 1);  // main_in_your_env.cpp:58 counts the header line too
    int done = 0;
    auto load = [&](int i, pcl::PointCloud<pcl::PointXYZI> &c) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        return erasor_utils::load_pcd(drv.data_dir + name, c) != -1;
    };
    // offline: the driver knows its nodes ahead (main_in_your_env.cpp:92-123 reads them from disk one by one).  Round 6: up to `lookahead`
    // nodes (ERASOR_DEMO_LOOKAHEAD, default 6) are read and ANNOUNCED before the node in front of them is processed -- their query chains
    // then share their launches and consecutive steps overlap (erasor_shim.h: set_lookahead); every node is stepped by the ticket of its
    // announcement.  Results do not depend on it.
    const int lookahead = std::max(1, std::min(getenv("ERASOR_DEMO_LOOKAHEAD") ? atoi(getenv("ERASOR_DEMO_LOOKAHEAD")) : 6, 7));
    updater.set_lookahead(lookahead);
    struct Ahead {
        pcl::PointCloud<pcl::PointXYZI> cloud;
        uint64_t ticket = 0;
        bool announced = false;  // (false: refused for now -- gate or capacity --, tried again before the next callback unless it is the upcoming node)
    };
    std::deque<Ahead> q;  // q[0] = the upcoming node i, q[j] = node i + j
    const int last = std::min((int)poses.size(), drv.init_idx + max_frames);  // one past the last node to process
    auto fill = [&](int i) {
        while ((int)q.size() < lookahead + 1 && i + (int)q.size() < last) {
            q.emplace_back();
            if (!load(i + (int)q.size() - 1, q.back().cloud)) {
                q.pop_back();
                return false;
            }
        }
        return true;
    };
    bool have = drv.init_idx < last && fill(drv.init_idx) && !q.empty();
    for (int i = drv.init_idx; have && i < last; ++i, ++done) {
        (void)fill(i);
        if (i == drv.init_idx && lookahead > 1) q[0].ticket = updater.announce_upcoming(q[0].cloud, erasor_utils::eigen2geoPose(poses[i]));
        // announce, in node order, every node behind the upcoming one that is not announced yet (a node the updater refuses -- gated out, or
        // as many outstanding as it takes -- stops the round: announcements are made in order)
        for (size_t j = 1; j < q.size(); ++j) {
            if (q[j].announced) continue;
            if (i > drv.init_idx && j + 1 == q.size() && updater.outstanding() < updater.lookahead()) {
                // the pipeline is full: the one new node of this round is staged INSIDE the upcoming callback, while its step runs on the
                // GPU (announce_next_deferred; its own callback finds the ticket by the sequence number)
                updater.announce_next_deferred(i + (int)j, q[j].cloud, erasor_utils::eigen2geoPose(poses[i + (int)j]));
                q[j].announced = true;
                break;
            }
            q[j].ticket = updater.announce_next(q[j].cloud, erasor_utils::eigen2geoPose(poses[i + (int)j]));
            q[j].announced = true;  // (ticket 0: gated out by removal_interval, or full: either way this node is stepped without a ticket)
            if (!q[j].ticket && updater.outstanding() >= updater.lookahead()) {
                q[j].announced = false;  // full: again before the next callback
                break;
            }
        }
        updater.callback_node(i, erasor_utils::eigen2geoPose(poses[i]), q[0].cloud, q[0].ticket);
        q.pop_front();
        have = !q.empty() || (i + 1 < last && fill(i + 1) && !q.empty());
    }
    if (nodes_done) *nodes_done = done;
    if (done == 0 && !have) return 3;
    updater.save_static_map(0.2f);  // main_in_your_env.cpp:123
    if (verbose) printf("Static map building complete!\n");
    return gt.empty() ? 0 : evaluate_saved_map(updater, gt);
}
static int config_mode(int argc, char **argv) {
    if (argc < 3) return 2;
    return run_config(argv[2], argc > 3 ? atoi(argv[3]) : 1 << 30, 0, true, nullptr, argc > 4 ? argv[4] : "");
}

// --sweep <rosparam.yaml> <grid.yaml> <gt> [n_frames] [voxelsize = 0.2] [concurrency = 2]: every configuration of the grid (the base
// file with the grid's scalars and one value of every axis, erasor::expand_sweep_grid) over the sequence --config reads, each one's saved
// map (save_static_map(0.2), main_in_your_env.cpp:123) scored against gt, from ONE erasor_hip_sweep call.  The map, the scans and the
// poses are read as --config reads them, and the poses take callback_node's way (eigen2geoPose -> node.odom -> geoPose2eigen, and its
// inverse), so every configuration steps with the matrices the shim steps with.  One row per configuration, the swept values in front,
// sorted by F1 (highest first, ties in grid order), then the best configuration as rosparam lines.
static int sweep_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    const int max_frames = argc > 5 ? atoi(argv[5]) : 1 << 30;
    const double voxelsize = argc > 6 ? atof(argv[6]) : 0.2;
    const int concurrency = argc > 7 ? atoi(argv[7]) : 2;
    erasor::SweepGrid grid;
    erasor::DriverConfig drv;
    std::string bad;
    const int grc = erasor::expand_sweep_grid(argv[2], argv[3], 256, grid, &drv, &bad);
    if (grc == -2) {
        fprintf(stderr, "%s: key %s cannot be swept (allowed: the /erasor/* parameters, /MapUpdater/query_voxel_size, "
                        "/MapUpdater/removal_interval, /large_scale/*)\n", argv[3], bad.c_str());
        return 2;
    }
    if (grc == -3) {
        fprintf(stderr, "%s: more than 256 configurations\n", argv[3]);
        return 2;
    }
    if (grc) {
        fprintf(stderr, "cannot read %s or %s\n", argv[2], argv[3]);
        return 3;
    }
    erasor::OfflineMapUpdater::Config &cfg = grid.base;
    if (cfg.environment != "outdoor") {  // (OfflineMapUpdater: OMU.cpp:149, 312)
        fprintf(stderr, "env %s: only outdoor is supported\n", cfg.environment.c_str());
        return 1;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    std::vector<float> map, gt, scans, Tb, To;
    if (!load_cloud_xyzi(cfg.initial_map_path, map) || !load_cloud_xyzi(argv[4], gt)) {
        fprintf(stderr, "cannot read %s or %s\n", cfg.initial_map_path.c_str(), argv[4]);
        return 3;
    }
    std::vector<uint64_t> offsets{0};
    const int last = std::min((int)poses.size(), drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {  // (run_config stops at the first scan it cannot read)
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        std::vector<float> scan;
        if (!load_cloud_xyzi(drv.data_dir + name, scan)) break;
        scans.insert(scans.end(), scan.begin(), scan.end());
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node, OMU.cpp:219)
        const Eigen::Matrix4f Ti = erasor_utils::inverse(T);                                            // (OMU.cpp:436)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                Tb.push_back(T(r, c));
                To.push_back(Ti(r, c));
            }
    }
    const size_t n_nodes = offsets.size() - 1;
    if (!n_nodes) {
        fprintf(stderr, "no scan under %s/pcds\n", drv.data_dir.c_str());
        return 3;
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    float Tl[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
    const size_t k = grid.configs.size();
    std::vector<erasor_params> params(k);
    for (size_t i = 0; i < k; ++i) {  // (what OfflineMapUpdater's constructor makes of the configuration)
        params[i] = grid.configs[i].params;
        params[i].is_large_scale = grid.configs[i].is_large_scale ? 1 : 0;
        if (grid.configs[i].is_large_scale) params[i].submap_size = grid.configs[i].submap_size;
    }
    erasor_params p0;
    erasor_hip_params_default(&p0);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p0, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    std::vector<erasor_sweep_row> rows(std::max<size_t>(k, 1));
    const double t0 = now_ms();
    const int rc = erasor_hip_sweep(h, params.data(), k, map.data(), map.size() / 4, 0, scans.data(), scans.size() / 4, offsets.data(), n_nodes, 0, Tl,
                                    Tb.data(), To.data(), gt.data(), gt.size() / 4, 0, 0.2, voxelsize, concurrency, 0, rows.data());
    const double t1 = now_ms();
    if (rc) {
        fprintf(stderr, "sweep: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    erasor_hip_destroy(h);
    printf("%zu configurations over %zu nodes of %s, saved maps (leaf 0.2) against %s, %.1f ms in all:\n", k, n_nodes, drv.data_dir.c_str(), argv[4],
           t1 - t0);
    std::vector<size_t> order(k);
    for (size_t i = 0; i < k; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        const bool oa = rows[a].status == ERASOR_OK, ob = rows[b].status == ERASOR_OK;
        if (oa != ob) return oa;
        return oa && rows[a].eval.F1 > rows[b].eval.F1;
    });
    std::string head = "|";
    for (const auto &a : grid.axes) head += " " + a.substr(a.rfind('/') + 1) + " |";
    printf("%s   gt_S |   gt_D |   est_S |   est_D |   kept_S |   kept_D |     PR%% |     RR%% |     F1 |\n", head.c_str());
    for (size_t i : order) {
        std::string pre = "|";
        for (size_t a = 0; a < grid.axes.size(); ++a) pre += " " + grid.values[i][a] + " |";
        const erasor_eval_result &r = rows[i].eval;
        if (rows[i].status != ERASOR_OK) {
            printf("%s failed: rc %d\n", pre.c_str(), rows[i].status);
            continue;
        }
        printf("%s %6llu | %6llu | %7llu | %7llu | %8llu | %8llu | %7.3f | %7.3f | %6.4f |\n", pre.c_str(), (unsigned long long)r.gt_static,
               (unsigned long long)r.gt_dynamic, (unsigned long long)r.est_static, (unsigned long long)r.est_dynamic,
               (unsigned long long)r.preserved_static, (unsigned long long)r.preserved_dynamic, r.PR, r.RR, r.F1);
    }
    if (k && rows[order[0]].status == ERASOR_OK) {
        const size_t b = order[0];
        printf("best configuration (F1 %.4f), as rosparam lines:\n", rows[b].eval.F1);
        std::vector<std::pair<std::string, std::string>> kv = grid.scalars;
        for (size_t a = 0; a < grid.axes.size(); ++a) kv.emplace_back(grid.axes[a], grid.values[b][a]);
        std::vector<std::string> sections;
        for (const auto &e : kv) {
            const std::string sec = e.first.substr(1, e.first.find('/', 1) - 1);
            if (std::find(sections.begin(), sections.end(), sec) == sections.end()) sections.push_back(sec);
        }
        for (const auto &sec : sections) {
            printf("%s:\n", sec.c_str());
            for (const auto &e : kv)
                if (e.first.compare(1, sec.size() + 1, sec + "/") == 0) printf("  %s: %s\n", e.first.substr(sec.size() + 2).c_str(), e.second.c_str());
        }
    }
    return 0;
}

// --align <rosparam.yaml> [n_frames] [voxelsize = 0.2]: the check the reference README asks for before anything else ("ERASOR in the
// Wild", pitfalls 1, 3 and 5): does pose_i · pcds/%06d.pcd overlay the initial map?  The same files as --config (data_dir, init_idx,
// poses_lidar2body.csv, the initial map, tf/lidar2body), and every frame's T_body2origin is the matrix run_config hands the step: the
// CSV pose after the eigen2geoPose / geoPose2eigen round trip.  One line per frame (erasor_hip_align_frames_clouds), a frame flagged
// when 50 % or less of its points lie within 0.5 * v ("most points should sit within 0.5 × voxel_size"), then the summary in
// overlap_report's two lines.  When tf/lidar2body is not the identity, a second pass with the identity, and which of the README's two
// conventions puts more of the points within v of the map: (A) poses T_map_from_lidar with an identity tf, (B) poses T_map_from_body
// with the extrinsic in tf/lidar2body.
static int align_mode(int argc, char **argv) {
    if (argc < 3) return 2;
    const int max_frames = argc > 3 ? atoi(argv[3]) : 1 << 30;
    const double voxelsize = argc > 4 ? atof(argv[4]) : 0.2;
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(argv[2], cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    std::vector<float> map, scans, Tb;
    if (!load_cloud_xyzi(cfg.initial_map_path, map)) {
        fprintf(stderr, "cannot read %s\n", cfg.initial_map_path.c_str());
        return 3;
    }
    std::vector<uint64_t> offsets{0};
    const int last = std::min((int)poses.size(), drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        std::vector<float> scan;
        if (!load_cloud_xyzi(drv.data_dir + name, scan)) {
            fprintf(stderr, "cannot read %s%s\n", drv.data_dir.c_str(), name);
            return 3;
        }
        scans.insert(scans.end(), scan.begin(), scan.end());
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node's round trip)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tb.push_back(T(r, c));
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    float Tl[16];
    bool identity = true;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            Tl[4 * r + c] = TL(r, c);
            identity = identity && TL(r, c) == (r == c ? 1.0f : 0.0f);
        }
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    const size_t n_frames = offsets.size() - 1;
    std::vector<erasor_align_row> rows(std::max<size_t>(n_frames, 1));
    const double half = 0.5 * voxelsize, one = voxelsize;
    double within_one[2] = {0, 0};
    for (int pass = 0; pass < (identity ? 1 : 2); ++pass) {
        erasor_overlap_result sum;
        const int rc = erasor_hip_align_frames_clouds(h, map.data(), map.size() / 4, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0,
                                                      pass ? nullptr : Tl, Tb.data(), voxelsize, rows.data(), &sum);
        if (rc) {
            fprintf(stderr, "align: %s (rc %d)\n", erasor_hip_last_error(h), rc);
            erasor_hip_destroy(h);
            return 1;
        }
        if (pass == 0)
            printf("%zu frames against %s (%zu points), tf/lidar2body as configured%s:\n", n_frames, cfg.initial_map_path.c_str(), map.size() / 4,
                   identity ? " (the identity)" : ", convention (B)");
        else
            printf("the same with tf/lidar2body = identity, convention (A):\n");
        for (size_t f = 0; f < n_frames; ++f) {
            const erasor_overlap_result &r = rows[f].r;
            printf("%6d  n=%llu  median=%.4fm  p90=%.4fm  <0.5*v %.2f%%  <1*v %.2f%%  <2*v %.2f%%%s\n", drv.init_idx + (int)f,
                   (unsigned long long)rows[f].n_points, r.median, r.p90, r.frac_half, r.frac_one, r.frac_two,
                   r.frac_half > 50.0 ? "" : "  <- check this pose");
        }
        printf("est->GT dist: median=%.4fm  p90=%.4fm  p99=%.4fm  max=%.4fm\n", sum.median, sum.p90, sum.p99, sum.max);
        printf("  fraction <0.5*v (%.2fm): %.2f%%  <1*v (%.2fm): %.2f%%  <2*v (%.2fm): %.2f%%\n", half, sum.frac_half, one, sum.frac_one, 2 * one,
               sum.frac_two);
        within_one[pass] = sum.n_est ? (double)sum.n_below_one / (double)sum.n_est * 100.0 : 0.0;
    }
    if (!identity)
        printf("convention: (B) T_map_from_body with tf/lidar2body as configured puts %.2f%% of the points within v of the map, (A) "
               "T_map_from_lidar with an identity tf/lidar2body %.2f%%: %s\n",
               within_one[0], within_one[1], within_one[0] >= within_one[1] ? "(B) fits better" : "(A) fits better");
    erasor_hip_destroy(h);
    return 0;
}

// --visibility <rosparam.yaml> <map.pcd|-> <out.pcd> [n_frames] [W H el_bottom el_top] [window] [k]: the see-through check
// (erasor_hip_visibility_clouds): every scan becomes a W x H range image between the two elevations (degrees; 1024 x 64 between -24.8 and
// 2.0, an HDL-64E's, by default), every map point is voted on by every image, and the points that scans look straight through leave.
// The same files and poses as --align (data_dir, init_idx, poses_lidar2body.csv after callback_node's round trip, tf/lidar2body); the
// map is <map.pcd>, or with "-" the configured initial map.  The two edge tables are evalmap.visibility_grid's expressions with C's tan.
// window (1) and k (0: no incidence gate) as erasor_visibility says; the other parameters are the documented defaults (0.5 .. 80 m,
// margins 0.2 m + 1 %, min_cos 0.25, min_through 2, hit_weight 1).  One line per frame, the result, and the kept cloud as a binary PCD --
// which --eval scores against a ground truth like any other map.
static int visibility_mode(int argc, char **argv) {
    if (argc < 5 || (argc > 6 && argc < 10)) return 2;
    const int max_frames = argc > 5 ? atoi(argv[5]) : 1 << 30;
    size_t W = 1024, H = 64, window = 1, k = 0;
    double el0 = -24.8, el1 = 2.0;
    if (argc > 9 && (!parse_count(argv[6], &W) || !parse_count(argv[7], &H) || !parse_number(argv[8], &el0) || !parse_number(argv[9], &el1))) return 2;
    if ((argc > 10 && !parse_count(argv[10], &window)) || (argc > 11 && !parse_count(argv[11], &k)) || argc > 12) return 2;
    if (W % 8 || W < 8 || W > 4096 || H < 1 || H > 256 || !(el0 < el1) || !(el0 > -90.0) || !(el1 < 90.0) || window > 2 || k == 1 || k > 32) return 2;
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(argv[2], cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    const std::string map_path = std::string(argv[3]) == "-" ? cfg.initial_map_path : std::string(argv[3]);
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    std::vector<float> map, scans, Tb;
    if (!load_cloud_xyzi(map_path, map)) {
        fprintf(stderr, "cannot read %s\n", map_path.c_str());
        return 3;
    }
    std::vector<uint64_t> offsets{0};
    const int last = std::min((int)poses.size(), drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        std::vector<float> scan;
        if (!load_cloud_xyzi(drv.data_dir + name, scan)) {
            fprintf(stderr, "cannot read %s%s\n", drv.data_dir.c_str(), name);
            return 3;
        }
        scans.insert(scans.end(), scan.begin(), scan.end());
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node's round trip)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tb.push_back(T(r, c));
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    float Tl[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
    // the edge tables: evalmap.visibility_grid's expressions
    const size_t M = W / 8;
    const double pi = 3.141592653589793;
    std::vector<double> col_tan, row_tan;
    for (size_t j = 1; j < M; ++j) col_tan.push_back(tan(((pi / 4.0) * (double)j) / (double)M));
    for (size_t i = 0; i <= H; ++i) row_tan.push_back(tan((((el1 - el0) * (double)i) / (double)H + el0) * (pi / 180.0)));
    erasor_visibility prm;
    memset(&prm, 0, sizeof(prm));
    prm.width = (uint32_t)W, prm.height = (uint32_t)H, prm.col_tan = col_tan.data(), prm.row_tan = row_tan.data();
    prm.min_range = 0.5, prm.max_range = 80.0, prm.margin_abs = 0.2, prm.margin_rel = 0.01;
    prm.window = (uint32_t)window, prm.k = (uint32_t)k, prm.min_cos = 0.25, prm.min_through = 2, prm.hit_weight = 1.0;
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n = map.size() / 4, n_frames = offsets.size() - 1;
    std::vector<float> kept(std::max<size_t>(n, 1) * 4, 0.f);
    std::vector<erasor_visibility_row> rows(std::max<size_t>(n_frames, 1));
    erasor_visibility_result r;
    const int rc = erasor_hip_visibility_clouds(h, map.data(), n, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0, Tl, Tb.data(), &prm, nullptr,
                                                nullptr, kept.data(), n, rows.data(), &r);
    if (rc) return render_fail(h, "visibility", rc);
    erasor_hip_destroy(h);
    typedef unsigned long long ull;
    printf("%zu frames against %s (%zu points), %zu x %zu pixels between %.9g and %.9g degrees, window %zu, k %zu:\n", n_frames, map_path.c_str(), n, W, H,
           el0, el1, window, k);
    for (size_t f = 0; f < n_frames; ++f) {
        const erasor_visibility_row &w = rows[f];
        printf("%6d  n=%llu  dropped %llu non-finite, %llu on the axis, %llu out of range, %llu out of view  pixels %llu  map in view %llu: hit %llu, "
               "occluded %llu, no return %llu, through %llu, grazing %llu\n",
               drv.init_idx + (int)f, (ull)w.n_points, (ull)w.n_non_finite, (ull)w.n_on_axis, (ull)w.n_out_of_range, (ull)w.n_out_of_view, (ull)w.n_pixels,
               (ull)w.n_map_in_view, (ull)w.n_hit, (ull)w.n_occluded, (ull)w.n_no_return, (ull)w.n_through, (ull)w.n_grazing);
    }
    printf("visibility: n=%llu  never in view=%llu  kept=%llu  removed=%llu (dynamic %llu, static %llu)  without a normal=%llu\n", (ull)r.n_points,
           (ull)r.n_never_in_view, (ull)r.n_kept, (ull)r.n_removed, (ull)r.n_removed_dynamic, (ull)r.n_removed_static, (ull)r.n_map_no_normal);
    printf("  verdicts: in view %llu  hit %llu  occluded %llu  no return %llu  through %llu  grazing %llu\n", (ull)r.n_in_view, (ull)r.n_hit, (ull)r.n_occluded,
           (ull)r.n_no_return, (ull)r.n_through, (ull)r.n_grazing);
    pcl::PointCloud<pcl::PointXYZI> out;
    rows_to_cloud(kept, r.n_kept, out);
    if (erasor_utils::save_pcd_binary(argv[4], out) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[4]);
        return 1;
    }
    printf("saved %s\n", argv[4]);
    return 0;
}

// --carve <rosparam.yaml> <map.pcd|-> <out.pcd> [n_frames] [voxel] [max_range] [stop_short]: free space carved out of a map, OctoMap's
// way (erasor_hip_carve_clouds): the map goes into voxels of `voxel` metres (0.2), every ray of every scan is walked through them up to
// max_range (80 m; from 0.5 m), a voxel that rays pass through is free and one that rays end in is occupied, the frames are integrated as
// clamped log-odds, and the points of the voxels that end below the threshold leave.  The same files and poses as --visibility.  The
// log-odds are OctoMap's defaults, evalmap.carve_logodds' expression with C's log: (float)log(p / (1 - p)) of 0.7 (hit), 0.4 (miss),
// 0.12 and 0.97 (the clamps) and 0.5 (the threshold), from 0.  One line per frame, the result, and the kept cloud as a binary PCD -- which
// --eval scores against a ground truth like any other map.
static int carve_mode(int argc, char **argv) {
    if (argc < 5 || argc > 9) return 2;
    size_t max_frames = (size_t)1 << 30, stop_short = 0;
    double voxel = 0.2, max_range = 80.0;
    const double min_range = 0.5;
    if ((argc > 5 && !parse_count(argv[5], &max_frames)) || (argc > 6 && !parse_number(argv[6], &voxel)) || (argc > 7 && !parse_number(argv[7], &max_range)) ||
        (argc > 8 && !parse_count(argv[8], &stop_short)))
        return 2;
    if (!(voxel > 0) || !std::isfinite(voxel) || !(max_range > min_range) || !std::isfinite(max_range) || max_range / voxel > (double)ERASOR_CARVE_MAX_CELLS ||
        stop_short > ERASOR_CARVE_MAX_STOP_SHORT)
        return 2;
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(argv[2], cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    const std::string map_path = std::string(argv[3]) == "-" ? cfg.initial_map_path : std::string(argv[3]);
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    std::vector<float> map, scans, Tb;
    if (!load_cloud_xyzi(map_path, map)) {
        fprintf(stderr, "cannot read %s\n", map_path.c_str());
        return 3;
    }
    std::vector<uint64_t> offsets{0};
    const int last = (int)std::min<size_t>(poses.size(), (size_t)drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        std::vector<float> scan;
        if (!load_cloud_xyzi(drv.data_dir + name, scan)) {
            fprintf(stderr, "cannot read %s%s\n", drv.data_dir.c_str(), name);
            return 3;
        }
        scans.insert(scans.end(), scan.begin(), scan.end());
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node's round trip)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tb.push_back(T(r, c));
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    float Tl[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
    auto logodds = [](double p) { return (float)log(p / (1.0 - p)); };  // evalmap.carve_logodds' expression
    erasor_carve prm;
    memset(&prm, 0, sizeof(prm));
    prm.voxel = voxel, prm.min_range = min_range, prm.max_range = max_range, prm.stop_short = (uint32_t)stop_short;
    prm.l_init = 0.f, prm.l_hit = logodds(0.7), prm.l_miss = logodds(0.4), prm.l_min = logodds(0.12), prm.l_max = logodds(0.97), prm.l_thr = logodds(0.5);
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n = map.size() / 4, n_frames = offsets.size() - 1;
    std::vector<float> kept(std::max<size_t>(n, 1) * 4, 0.f);
    std::vector<erasor_carve_row> rows(std::max<size_t>(n_frames, 1));
    erasor_carve_result r;
    const int rc = erasor_hip_carve_clouds(h, map.data(), n, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0, Tl, Tb.data(), &prm, nullptr, nullptr,
                                           nullptr, kept.data(), n, rows.data(), &r);
    if (rc) return render_fail(h, "carve", rc);
    erasor_hip_destroy(h);
    typedef unsigned long long ull;
    printf("%zu frames against %s (%zu points), voxel %.9g, range %.9g .. %.9g, stop_short %zu:\n", n_frames, map_path.c_str(), n, voxel, min_range, max_range,
           stop_short);
    for (size_t f = 0; f < n_frames; ++f) {
        const erasor_carve_row &w = rows[f];
        printf("%6d  n=%llu  dropped %llu non-finite, %llu out of range  rays %llu  steps %llu  ends in the map %llu  voxels hit %llu, free %llu\n",
               drv.init_idx + (int)f, (ull)w.n_points, (ull)w.n_non_finite, (ull)w.n_out_of_range, (ull)w.n_rays, (ull)w.n_steps, (ull)w.n_end_in_map,
               (ull)w.n_voxels_hit, (ull)w.n_voxels_free);
    }
    printf("carve: n=%llu  non-finite=%llu  voxels=%llu in %llu blocks, touched %llu  kept=%llu  removed=%llu (dynamic %llu, static %llu)\n", (ull)r.n_points,
           (ull)r.n_map_non_finite, (ull)r.n_voxels, (ull)r.n_blocks, (ull)r.n_voxels_touched, (ull)r.n_kept, (ull)r.n_removed, (ull)r.n_removed_dynamic,
           (ull)r.n_removed_static);
    printf("  rays: %llu of %llu points (dropped %llu non-finite, %llu out of range)  steps %llu  ends in the map %llu  voxel hits %llu, misses %llu\n",
           (ull)r.n_rays, (ull)r.n_scan_points, (ull)r.n_non_finite, (ull)r.n_out_of_range, (ull)r.n_steps, (ull)r.n_end_in_map, (ull)r.n_voxels_hit,
           (ull)r.n_voxels_free);
    pcl::PointCloud<pcl::PointXYZI> out;
    rows_to_cloud(kept, r.n_kept, out);
    if (erasor_utils::save_pcd_binary(argv[4], out) != 0) {
        fprintf(stderr, "cannot write %s\n", argv[4]);
        return 1;
    }
    printf("saved %s\n", argv[4]);
    return 0;
}

// --refine <rosparam.yaml> <poses_out> [n_frames] [max_dist = 1.0] [max_iters = 20]: what to do about the frames --align flags.  The same
// files and poses as --align (data_dir, init_idx, poses_lidar2body.csv after callback_node's round trip, the initial map, tf/lidar2body);
// every frame's T_body2origin is refined against the initial map by point-to-point ICP (erasor_hip_refine_poses_clouds).  One line per
// frame: --align's "<0.5*v" percentage before and after (erasor_hip_align_frames_clouds, twice, voxelsize 0.2) and the frame's row; a frame
// is flagged when it did not converge or moved more than max_dist.  Writes <poses_out> in poses_lidar2body.csv's own format -- the
// file's lines as they are, x y z qx qy qz qw of the refined frames replaced (17 digits; a frame without enough pairs keeps its line) --
// so that it can take the pose file's place in the run.
// --refine-plane <rosparam.yaml> <poses_out> [n_frames] [max_dist = 1.0] [max_iters = 20] [k = 16]: the same mode with the residual taken
// along the map's surface normals (erasor_hip_refine_poses_plane_clouds; k: the normals' neighbourhood).  Each row also prints the rank of
// the frame's normal equations, lambda_ratio and the plane rms; a frame whose pairs constrain fewer than the pose's six directions is
// flagged -- the directions left out were not moved.
static void rot_to_quat(const double *T, double q[4]) {  // (x y z w) of T's rotation (row-major 4x4): the largest of the four pivots
    const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
    const double tr = r00 + r11 + r22;
    if (tr > 0) {
        const double s = std::sqrt(tr + 1.0) * 2;
        q[3] = 0.25 * s, q[0] = (r21 - r12) / s, q[1] = (r02 - r20) / s, q[2] = (r10 - r01) / s;
    } else if (r00 > r11 && r00 > r22) {
        const double s = std::sqrt(1.0 + r00 - r11 - r22) * 2;
        q[3] = (r21 - r12) / s, q[0] = 0.25 * s, q[1] = (r01 + r10) / s, q[2] = (r02 + r20) / s;
    } else if (r11 > r22) {
        const double s = std::sqrt(1.0 + r11 - r00 - r22) * 2;
        q[3] = (r02 - r20) / s, q[0] = (r01 + r10) / s, q[1] = 0.25 * s, q[2] = (r12 + r21) / s;
    } else {
        const double s = std::sqrt(1.0 + r22 - r00 - r11) * 2;
        q[3] = (r10 - r01) / s, q[0] = (r02 + r20) / s, q[1] = (r12 + r21) / s, q[2] = 0.25 * s;
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) q[k] /= n;
}
static int refine_mode(int argc, char **argv, bool plane) {
    if (argc < 4) return 2;
    const std::string out_path = argv[3];
    const int max_frames = argc > 4 ? atoi(argv[4]) : 1 << 30;
    erasor_refine_params prm = {argc > 5 ? atof(argv[5]) : 1.0, 1e-4, 1e-5, (uint32_t)(argc > 6 ? atoi(argv[6]) : 20), 100};
    const double voxelsize = 0.2;
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(argv[2], cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    const std::string pose_path = drv.data_dir + "/poses_lidar2body.csv";
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(pose_path, poses)) {
        fprintf(stderr, "cannot read %s\n", pose_path.c_str());
        return 3;
    }
    std::vector<float> map, scans, Tb;
    if (!load_cloud_xyzi(cfg.initial_map_path, map)) {
        fprintf(stderr, "cannot read %s\n", cfg.initial_map_path.c_str());
        return 3;
    }
    std::vector<uint64_t> offsets{0};
    const int last = std::min((int)poses.size(), drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        std::vector<float> scan;
        if (!load_cloud_xyzi(drv.data_dir + name, scan)) {
            fprintf(stderr, "cannot read %s%s\n", drv.data_dir.c_str(), name);
            return 3;
        }
        scans.insert(scans.end(), scan.begin(), scan.end());
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node's round trip)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tb.push_back(T(r, c));
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    float Tl[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    const size_t n_frames = offsets.size() - 1;
    std::vector<erasor_align_row> before(std::max<size_t>(n_frames, 1)), after(std::max<size_t>(n_frames, 1));
    std::vector<erasor_refine_plane_row> rows(std::max<size_t>(n_frames, 1));  // (--refine fills the fields the two rows share)
    erasor_refine_plane_summary sum;
    memset(&sum, 0, sizeof(sum));
    const erasor_refine_plane_params pprm = {prm.max_dist, prm.eps_t, prm.eps_r, prm.max_iters, prm.min_pairs, (uint32_t)(argc > 7 ? atoi(argv[7]) : 16), 1.0, 1e-9};
    std::vector<float> Tr(Tb.size());
    int rc = erasor_hip_align_frames_clouds(h, map.data(), map.size() / 4, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0, Tl, Tb.data(),
                                            voxelsize, before.data(), nullptr);
    if (!rc && plane)
        rc = erasor_hip_refine_poses_plane_clouds(h, map.data(), map.size() / 4, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0, Tl,
                                                  Tb.data(), &pprm, rows.data(), &sum);
    if (!rc && !plane) {
        std::vector<erasor_refine_row> r0(rows.size());
        erasor_refine_summary s0;
        rc = erasor_hip_refine_poses_clouds(h, map.data(), map.size() / 4, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0, Tl, Tb.data(),
                                            &prm, r0.data(), &s0);
        for (size_t f = 0; f < n_frames && !rc; ++f) {
            erasor_refine_plane_row &r = rows[f];
            memcpy(r.T, r0[f].T, sizeof(r.T));
            r.status = r0[f].status, r.iters = r0[f].iters, r.n_points = r0[f].n_points, r.n_non_finite = r0[f].n_non_finite;
            r.n_pairs_first = r0[f].n_pairs_first, r.n_pairs_last = r0[f].n_pairs_last, r.rms_first = r0[f].rms_first, r.rms_last = r0[f].rms_last;
            r.moved_t = r0[f].moved_t, r.moved_r = r0[f].moved_r;
        }
        for (int k = 0; k < 4; ++k) sum.n_status[k] = s0.n_status[k];
        sum.n_pairs_first = s0.n_pairs_first, sum.n_pairs_last = s0.n_pairs_last, sum.sum_d2_first = s0.sum_d2_first, sum.sum_d2_last = s0.sum_d2_last;
    }
    if (!rc) {
        for (size_t f = 0; f < n_frames; ++f)
            for (int k = 0; k < 16; ++k) Tr[16 * f + k] = (float)rows[f].T[k];
        rc = erasor_hip_align_frames_clouds(h, map.data(), map.size() / 4, 0, scans.data(), scans.size() / 4, offsets.data(), n_frames, 0, Tl, Tr.data(),
                                            voxelsize, after.data(), nullptr);
    }
    if (rc) {
        fprintf(stderr, "%s: %s (rc %d)\n", plane ? "refine-plane" : "refine", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    erasor_hip_destroy(h);
    static const char *const STATUS[5] = {"converged", "iteration limit", "too few pairs", "no finite points", "degenerate"};
    printf("%zu frames against %s (%zu points), max_dist %.3f m, at most %u iterations", n_frames, cfg.initial_map_path.c_str(), map.size() / 4,
           prm.max_dist, prm.max_iters);
    if (plane) printf(", point-to-plane with normals from %u neighbours (%llu map points without one)", pprm.normals_k, (unsigned long long)sum.n_map_no_normal);
    printf(":\n");
    for (size_t f = 0; f < n_frames; ++f) {
        const erasor_refine_plane_row &r = rows[f];
        const bool flag = r.status != ERASOR_REFINE_CONVERGED || r.moved_t > prm.max_dist;
        printf("%6d  n=%llu  <0.5*v %.2f%% -> %.2f%%  %s after %u  pairs %llu -> %llu  rms %.4fm -> %.4fm  moved %.4fm %.5frad",
               drv.init_idx + (int)f, (unsigned long long)r.n_points, before[f].r.frac_half, after[f].r.frac_half, STATUS[r.status < 5 ? r.status : 4],
               r.iters, (unsigned long long)r.n_pairs_first, (unsigned long long)r.n_pairs_last, r.rms_first, r.rms_last, r.moved_t, r.moved_r);
        if (plane) printf("  rank %u  lambda_ratio %.3g  plane rms %.4fm -> %.4fm", r.rank, r.lambda_ratio, r.rms_plane_first, r.rms_plane_last);
        printf("%s", flag ? (r.status != ERASOR_REFINE_CONVERGED ? "  <- not converged: check this pose" : "  <- moved more than max_dist: check this pose") : "");
        if (plane && r.status <= ERASOR_REFINE_MAX_ITERS && r.rank < 6) printf("  <- only %u of 6 directions constrained", r.rank);
        printf("\n");
    }
    printf("summary: %llu converged, %llu at the iteration limit, %llu with too few pairs, %llu without finite points", (unsigned long long)sum.n_status[0],
           (unsigned long long)sum.n_status[1], (unsigned long long)sum.n_status[2], (unsigned long long)sum.n_status[3]);
    if (plane) printf(", %llu degenerate", (unsigned long long)sum.n_status[4]);
    printf("; pairs %llu -> %llu, rms %.4fm -> %.4fm", (unsigned long long)sum.n_pairs_first, (unsigned long long)sum.n_pairs_last,
           sum.n_pairs_first ? std::sqrt(sum.sum_d2_first / (double)sum.n_pairs_first) : 0.0,
           sum.n_pairs_last ? std::sqrt(sum.sum_d2_last / (double)sum.n_pairs_last) : 0.0);
    if (plane)
        printf(", plane rms %.4fm -> %.4fm", sum.n_pairs_first ? std::sqrt(sum.sum_r2_first / (double)sum.n_pairs_first) : 0.0,
               sum.n_pairs_last ? std::sqrt(sum.sum_r2_last / (double)sum.n_pairs_last) : 0.0);
    printf("\n");
    // the pose file again, line by line: the header and every pose outside the refined range as they are
    std::ifstream in(pose_path);
    std::ofstream out(out_path);
    if (!in || !out) {
        fprintf(stderr, "cannot write %s\n", out_path.c_str());
        return 1;
    }
    std::string line;
    int row = -1;  // the line's pose index (the header: -1), counted as load_all_poses counts
    bool header = true;
    while (std::getline(in, line)) {
        if (header) {
            header = false;
            out << line << "\n";
            continue;
        }
        size_t c1 = line.find(','), c2 = c1 == std::string::npos ? c1 : line.find(',', c1 + 1);
        if (c2 == std::string::npos) {  // (a blank line: load_all_poses skips it too)
            out << line << "\n";
            continue;
        }
        ++row;
        const int f = row - drv.init_idx;
        if (f < 0 || f >= (int)n_frames || rows[f].status >= ERASOR_REFINE_FEW_PAIRS) {
            out << line << "\n";
            continue;
        }
        double q[4];
        rot_to_quat(rows[f].T, q);
        char buf[256];
        snprintf(buf, sizeof(buf), "%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g", rows[f].T[3], rows[f].T[7], rows[f].T[11], q[0], q[1], q[2], q[3]);
        out << line.substr(0, c2 + 1) << buf << "\n";
    }
    out.close();
    if (!out) {
        fprintf(stderr, "cannot write %s\n", out_path.c_str());
        return 1;
    }
    printf("wrote %s\n", out_path.c_str());
    return 0;
}

// --label-scans <rosparam.yaml> <static.pcd> <raw.pcd|-> <out_dir> [n_frames] [tau]: a cleaned map carried back to the scans
// (erasor_hip_label_scans_clouds).  The same files and poses as --align (data_dir, init_idx, poses_lidar2body.csv after callback_node's
// round trip, tf/lidar2body); every scan point is static (a point of <static.pcd> within tau), dynamic, or -- with a raw map -- unknown
// (neither map has a point within tau).  tau: 0.2 * sqrt(3) / 2, --eval's threshold at its default voxel size.  One line per frame
// and the summary with the moving-object IoU / precision / recall against the scans' own labels (classes 252..259 moving).  Writes
// <out_dir>/%06d.label, one little-endian uint32 per point in scan order: static 9, moving 251, unknown and dropped 0 -- the ids
// SemanticKITTI's moving-object-segmentation benchmark uses for "static", "moving" and "unlabeled", quoted from memory: check them
// against the benchmark's semantic-kitti-mos.yaml before training on these files --, and <out_dir>/%06d.pcd (binary: every float
// keeps its bits) with the frame's static points, as given.
static double ratio_or_nan(uint64_t a, uint64_t b) { return b ? (double)a / (double)b : std::numeric_limits<double>::quiet_NaN(); }
static int label_scans_mode(int argc, char **argv) {
    if (argc < 6) return 2;
    const std::string static_path = argv[3], raw_path = argv[4], out_dir = argv[5];
    const int max_frames = argc > 6 ? atoi(argv[6]) : 1 << 30;
    const double tau = argc > 7 ? atof(argv[7]) : (0.2 * std::sqrt(3.0)) / 2.0;
    const bool have_raw = raw_path != "-";
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(argv[2], cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 3;
    }
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    std::vector<float> smap, rmap, scans, Tb;
    if (!load_cloud_xyzi(static_path, smap) || (have_raw && !load_cloud_xyzi(raw_path, rmap))) {
        fprintf(stderr, "cannot read %s or %s\n", static_path.c_str(), raw_path.c_str());
        return 3;
    }
    std::vector<uint64_t> offsets{0};
    const int last = std::min((int)poses.size(), drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        std::vector<float> scan;
        if (!load_cloud_xyzi(drv.data_dir + name, scan)) {
            fprintf(stderr, "cannot read %s%s\n", drv.data_dir.c_str(), name);
            return 3;
        }
        scans.insert(scans.end(), scan.begin(), scan.end());
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node's round trip)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tb.push_back(T(r, c));
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    float Tl[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
    erasor_params p;
    erasor_hip_params_default(&p);
    erasor_hip_handle *h = nullptr;
    if (erasor_hip_create(&p, 0, &h) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_create failed\n");
        return 1;
    }
    const size_t n_frames = offsets.size() - 1, n_pts = scans.size() / 4;
    std::vector<erasor_scan_label_row> rows(std::max<size_t>(n_frames, 1));
    std::vector<uint8_t> codes(std::max<size_t>(n_pts, 1));
    std::vector<float> kept(std::max<size_t>(n_pts, 1) * 4);
    std::vector<uint64_t> kept_off(n_frames + 1);
    erasor_scan_label_row sum;
    const int rc = erasor_hip_label_scans_clouds(h, smap.data(), smap.size() / 4, 0, have_raw ? rmap.data() : nullptr, rmap.size() / 4, 0, have_raw ? 1 : 0,
                                                 scans.data(), n_pts, offsets.data(), n_frames, 0, Tl, Tb.data(), tau, codes.data(), 0, kept.data(), n_pts,
                                                 kept_off.data(), rows.data(), &sum);
    if (rc) {
        fprintf(stderr, "label_scans: %s (rc %d)\n", erasor_hip_last_error(h), rc);
        erasor_hip_destroy(h);
        return 1;
    }
    erasor_hip_destroy(h);
    printf("%zu frames against %s (%zu points)%s%s, tau %.6f m:\n", n_frames, static_path.c_str(), smap.size() / 4, have_raw ? " and " : "",
           have_raw ? raw_path.c_str() : "", tau);
    for (size_t f = 0; f < n_frames; ++f) {
        const erasor_scan_label_row &r = rows[f];
        printf("%6d  n=%llu  static=%llu  dynamic=%llu  unknown=%llu  dropped=%llu  moving IoU=%.4f\n", drv.init_idx + (int)f,
               (unsigned long long)r.n_points, (unsigned long long)(r.n[0][0] + r.n[1][0]), (unsigned long long)(r.n[0][1] + r.n[1][1]),
               (unsigned long long)(r.n[0][2] + r.n[1][2]), (unsigned long long)r.n_non_finite,
               ratio_or_nan(r.n[1][1], r.n[1][1] + r.n[0][1] + r.n[1][0] + r.n[1][2]));
        char name[64];
        snprintf(name, sizeof(name), "/%06d.label", drv.init_idx + (int)f);
        FILE *fp = fopen((out_dir + name).c_str(), "wb");
        if (!fp) {
            fprintf(stderr, "cannot write %s%s\n", out_dir.c_str(), name);
            return 1;
        }
        for (uint64_t i = offsets[f]; i < offsets[f + 1]; ++i) {
            const uint32_t id = codes[i] == 0 ? 9u : codes[i] == 1 ? 251u : 0u;
            const unsigned char le[4] = {(unsigned char)(id & 0xFF), (unsigned char)((id >> 8) & 0xFF), (unsigned char)((id >> 16) & 0xFF),
                                         (unsigned char)(id >> 24)};
            fwrite(le, 1, 4, fp);
        }
        if (fclose(fp) != 0) return 1;
        pcl::PointCloud<pcl::PointXYZI> out;
        const std::vector<float> frame_rows(kept.begin() + 4 * kept_off[f], kept.begin() + 4 * kept_off[f + 1]);
        rows_to_cloud(frame_rows, kept_off[f + 1] - kept_off[f], out);
        snprintf(name, sizeof(name), "/%06d.pcd", drv.init_idx + (int)f);
        if (erasor_utils::save_pcd_binary(out_dir + name, out) != 0) {
            fprintf(stderr, "cannot write %s%s\n", out_dir.c_str(), name);
            return 1;
        }
    }
    const uint64_t TP = sum.n[1][1], FP = sum.n[0][1], FN = sum.n[1][0] + sum.n[1][2];
    printf("summary: n=%llu  dropped=%llu  labels out of range=%llu\n", (unsigned long long)sum.n_points, (unsigned long long)sum.n_non_finite,
           (unsigned long long)sum.n_label_out_of_range);
    printf("  own label static: static=%llu dynamic=%llu unknown=%llu\n", (unsigned long long)sum.n[0][0], (unsigned long long)sum.n[0][1],
           (unsigned long long)sum.n[0][2]);
    printf("  own label moving: static=%llu dynamic=%llu unknown=%llu\n", (unsigned long long)sum.n[1][0], (unsigned long long)sum.n[1][1],
           (unsigned long long)sum.n[1][2]);
    printf("  moving: TP=%llu FP=%llu FN=%llu  IoU=%.6f  precision=%.6f  recall=%.6f\n", (unsigned long long)TP, (unsigned long long)FP,
           (unsigned long long)FN, ratio_or_nan(TP, TP + FP + FN), ratio_or_nan(TP, TP + FP), ratio_or_nan(TP, TP + FN));
    return 0;
}

// What --ground and --ground-map read: the rosparam file, the poses (after callback_node's round trip), tf/lidar2body and the first
// max_frames scans from init_idx on.  0, or the status to leave with (3: a file cannot be read).
static int ground_load(const char *yaml, size_t max_frames, bool want_scans, erasor::OfflineMapUpdater::Config &cfg, erasor::DriverConfig &drv,
                       std::vector<float> &scans, std::vector<uint64_t> &offsets, std::vector<float> &Tb, float Tl[16]) {
    erasor_hip_params_default(&cfg.params);
    if (!erasor::load_config_yaml(yaml, cfg, &drv)) {
        fprintf(stderr, "cannot read %s\n", yaml);
        return 3;
    }
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) {
        fprintf(stderr, "cannot read %s/poses_lidar2body.csv\n", drv.data_dir.c_str());
        return 3;
    }
    offsets.assign(1, 0);
    const int last = (int)std::min<size_t>(poses.size(), (size_t)drv.init_idx + max_frames);
    for (int i = drv.init_idx; i < last; ++i) {
        if (want_scans) {
            char name[64];
            snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
            std::vector<float> scan;
            if (!load_cloud_xyzi(drv.data_dir + name, scan)) {
                fprintf(stderr, "cannot read %s%s\n", drv.data_dir.c_str(), name);
                return 3;
            }
            scans.insert(scans.end(), scan.begin(), scan.end());
        }
        offsets.push_back(scans.size() / 4);
        const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(erasor_utils::eigen2geoPose(poses[i]));  // (callback_node's round trip)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tb.push_back(T(r, c));
    }
    geometry_msgs::Pose l2b;
    l2b.position.x = cfg.lidar2body[0];
    l2b.position.y = cfg.lidar2body[1];
    l2b.position.z = cfg.lidar2body[2];
    l2b.orientation.x = cfg.lidar2body[3];
    l2b.orientation.y = cfg.lidar2body[4];
    l2b.orientation.z = cfg.lidar2body[5];
    l2b.orientation.w = cfg.lidar2body[6];
    const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2b);  // (OMU.cpp:100)
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
    return 0;
}

// erasor_ground with the reference's parameters (config/seq_05.yaml; min_z: its min_h in the lidar frame) over a uniform grid:
// evalmap.ground_grid's expressions with C's tan
static void ground_params(size_t R, size_t S, double min_range, double max_range, std::vector<double> &ring_edge, std::vector<double> &col_tan,
                          erasor_ground *prm) {
    const size_t M = S / 8;
    const double pi = 3.141592653589793;
    for (size_t j = 1; j < M; ++j) col_tan.push_back(tan(((pi / 4.0) * (double)j) / (double)M));
    for (size_t i = 0; i <= R; ++i) ring_edge.push_back(min_range + ((max_range - min_range) * (double)i) / (double)R);
    memset(prm, 0, sizeof(*prm));
    prm->n_rings = (uint32_t)R, prm->n_sectors = (uint32_t)S, prm->ring_edge = ring_edge.data(), prm->col_tan = col_tan.data();
    prm->num_lpr = 10, prm->iters = 3, prm->min_points = 10, prm->min_votes = 1;
    prm->th_seeds = 0.5, prm->th_dist = 0.15, prm->min_z = -3.03, prm->uprightness = 0.707, prm->ratio = 0.5, prm->keep = 1;
}

static void ground_print_row(int frame, const erasor_ground_row &w, bool map_form) {
    typedef unsigned long long ull;
    printf("%6d  n=%llu  dropped %llu non-finite, %llu out of range  judged %llu  ground %llu (dynamic %llu)  patches %llu: sparse %llu, degenerate %llu, "
           "not upright %llu, elevated %llu",
           frame, (ull)w.n_points, (ull)w.n_non_finite, (ull)w.n_out_of_range, (ull)w.n_judged, (ull)w.n_ground, (ull)w.n_ground_dynamic, (ull)w.n_patches,
           (ull)w.n_sparse, (ull)w.n_degenerate, (ull)w.n_rejected_upright, (ull)w.n_rejected_elevation);
    if (map_form) printf("  gathered %llu", (ull)w.n_gathered);
    printf("\n");
}

// --ground <rosparam.yaml> <out_dir> [n_frames] [n_rings n_sectors max_range]: every scan's ground (erasor_hip_ground_scans): R-GPF with
// the reference's parameters on every patch of a uniform polar grid (20 rings x 64 sectors between 0.5 and 80 m by default), the scans
// taken as given in the lidar frame.  One line per frame and the sums.  Writes <out_dir>/%06d.ground, one byte per point in scan order
// (1 ground, 0 not ground, 2 not judged, 255 non-finite), and <out_dir>/%06d.pcd (binary) with the frame's points that are not ground.
static int ground_mode(int argc, char **argv) {
    if (argc != 4 && argc != 5 && argc != 8) return 2;
    size_t max_frames = (size_t)1 << 30, R = 20, S = 64;
    double max_range = 80.0;
    const double min_range = 0.5;
    if (argc > 4 && !parse_count(argv[4], &max_frames)) return 2;
    if (argc > 7 && (!parse_count(argv[5], &R) || !parse_count(argv[6], &S) || !parse_number(argv[7], &max_range))) return 2;
    if (R < 1 || R > ERASOR_GROUND_MAX_RINGS || S % 8 || S < 8 || S > ERASOR_GROUND_MAX_SECTORS || !(max_range > min_range) || !std::isfinite(max_range)) return 2;
    const std::string out_dir = argv[3];
    erasor::OfflineMapUpdater::Config cfg;
    erasor::DriverConfig drv;
    std::vector<float> scans, Tb;
    std::vector<uint64_t> offsets;
    float Tl[16];
    const int st = ground_load(argv[2], max_frames, true, cfg, drv, scans, offsets, Tb, Tl);
    if (st) return st;
    std::vector<double> ring_edge, col_tan;
    erasor_ground prm;
    ground_params(R, S, min_range, max_range, ring_edge, col_tan, &prm);
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n_frames = offsets.size() - 1, n_pts = scans.size() / 4;
    std::vector<uint8_t> codes(std::max<size_t>(n_pts, 1));
    std::vector<erasor_ground_row> rows(std::max<size_t>(n_frames, 1));
    erasor_ground_result r;
    const int rc = erasor_hip_ground_scans(h, scans.data(), n_pts, offsets.data(), n_frames, 0, &prm, codes.data(), rows.data(), nullptr, &r);
    if (rc) return render_fail(h, "ground", rc);
    erasor_hip_destroy(h);
    typedef unsigned long long ull;
    printf("%zu frames, %zu rings x %zu sectors between %.9g and %.9g m:\n", n_frames, R, S, min_range, max_range);
    for (size_t f = 0; f < n_frames; ++f) {
        ground_print_row(drv.init_idx + (int)f, rows[f], false);
        char name[64];
        snprintf(name, sizeof(name), "/%06d.ground", drv.init_idx + (int)f);
        FILE *fp = fopen((out_dir + name).c_str(), "wb");
        if (!fp) {
            fprintf(stderr, "cannot write %s%s\n", out_dir.c_str(), name);
            return 1;
        }
        const size_t m = (size_t)(offsets[f + 1] - offsets[f]);
        if (fwrite(codes.data() + offsets[f], 1, m, fp) != m || fclose(fp) != 0) return 1;
        std::vector<float> rest;
        for (uint64_t i = offsets[f]; i < offsets[f + 1]; ++i)
            if (codes[i] != ERASOR_GROUND_CODE_GROUND) rest.insert(rest.end(), scans.begin() + 4 * i, scans.begin() + 4 * i + 4);
        pcl::PointCloud<pcl::PointXYZI> out;
        rows_to_cloud(rest, rest.size() / 4, out);
        snprintf(name, sizeof(name), "/%06d.pcd", drv.init_idx + (int)f);
        if (erasor_utils::save_pcd_binary(out_dir + name, out) != 0) {
            fprintf(stderr, "cannot write %s%s\n", out_dir.c_str(), name);
            return 1;
        }
    }
    printf("ground: frames=%llu  n=%llu  non-finite=%llu  out of range=%llu  judged=%llu  ground=%llu (dynamic %llu)  patches=%llu: sparse %llu, degenerate %llu, "
           "not upright %llu, elevated %llu\n",
           (ull)r.n_frames, (ull)r.n_points, (ull)r.n_non_finite, (ull)r.n_out_of_range, (ull)r.n_judged, (ull)r.n_ground, (ull)r.n_ground_dynamic, (ull)r.n_patches,
           (ull)r.n_sparse, (ull)r.n_degenerate, (ull)r.n_rejected_upright, (ull)r.n_rejected_elevation);
    return 0;
}

// --ground-map <rosparam.yaml> <map.pcd|-> <ground_out.pcd> <rest_out.pcd> [n_frames] [min_votes] [ratio]: the map's ground points by
// vote (erasor_hip_ground_votes_clouds): what every frame sees of the map is segmented as a scan over the default grid, and a map point is
// ground iff it has at least min_votes (1) ground votes and more than ratio (0.5) times the frames that judged it.  The same files and
// poses as --carve; the map is <map.pcd>, or with "-" the configured initial map.  One line per frame, the result, and two binary PCDs:
// the ground points and the rest, both in map order.
static int ground_map_mode(int argc, char **argv) {
    if (argc < 6 || argc > 9) return 2;
    size_t max_frames = (size_t)1 << 30, min_votes = 1;
    double ratio = 0.5;
    if ((argc > 6 && !parse_count(argv[6], &max_frames)) || (argc > 7 && !parse_count(argv[7], &min_votes)) || (argc > 8 && !parse_number(argv[8], &ratio)))
        return 2;
    if (!std::isfinite(ratio) || min_votes > 0xFFFFFFFFull) return 2;
    erasor::OfflineMapUpdater::Config cfg;
    erasor::DriverConfig drv;
    std::vector<float> scans, Tb, map;
    std::vector<uint64_t> offsets;
    float Tl[16];
    const int st = ground_load(argv[2], max_frames, false, cfg, drv, scans, offsets, Tb, Tl);
    if (st) return st;
    const std::string map_path = std::string(argv[3]) == "-" ? cfg.initial_map_path : std::string(argv[3]);
    if (!load_cloud_xyzi(map_path, map)) {
        fprintf(stderr, "cannot read %s\n", map_path.c_str());
        return 3;
    }
    std::vector<double> ring_edge, col_tan;
    erasor_ground prm;
    ground_params(20, 64, 0.5, 80.0, ring_edge, col_tan, &prm);
    prm.min_votes = (uint32_t)min_votes, prm.ratio = ratio;
    erasor_hip_handle *h = render_handle();
    if (!h) return 1;
    const size_t n = map.size() / 4, n_frames = offsets.size() - 1;
    std::vector<uint8_t> mask(std::max<size_t>(n, 1));
    std::vector<erasor_ground_row> rows(std::max<size_t>(n_frames, 1));
    erasor_ground_result r;
    const int rc = erasor_hip_ground_votes_clouds(h, map.data(), n, 0, Tl, Tb.data(), n_frames, &prm, nullptr, mask.data(), nullptr, 0, rows.data(), &r);
    if (rc) return render_fail(h, "ground-map", rc);
    erasor_hip_destroy(h);
    typedef unsigned long long ull;
    printf("%zu frames against %s (%zu points), min_votes %zu, ratio %.9g:\n", n_frames, map_path.c_str(), n, min_votes, ratio);
    for (size_t f = 0; f < n_frames; ++f) ground_print_row(drv.init_idx + (int)f, rows[f], true);
    printf("ground-map: n=%llu  ground=%llu (dynamic %llu, static %llu)  unseen=%llu  gathered=%llu  judged=%llu\n", (ull)r.n_map_points, (ull)r.n_map_ground,
           (ull)r.n_map_ground_dynamic, (ull)r.n_map_ground_static, (ull)r.n_map_unseen, (ull)r.n_points, (ull)r.n_judged);
    std::vector<float> part[2];
    for (size_t i = 0; i < n; ++i) part[mask[i] ? 0 : 1].insert(part[mask[i] ? 0 : 1].end(), map.begin() + 4 * i, map.begin() + 4 * i + 4);
    for (int k = 0; k < 2; ++k) {
        pcl::PointCloud<pcl::PointXYZI> out;
        rows_to_cloud(part[k], part[k].size() / 4, out);
        if (erasor_utils::save_pcd_binary(argv[4 + k], out) != 0) {
            fprintf(stderr, "cannot write %s\n", argv[4 + k]);
            return 1;
        }
        printf("saved %s\n", argv[4 + k]);
    }
    return 0;
}

// --queue <n_workers> <max_frames> <a.yaml> <b.yaml> ...: independent sequences (one rosparam file each) over n_workers devices
// (worker w drives device w mod the visible devices): every worker is a thread with its own updater per job, and takes the NEXT sequence
// of the list whenever it is idle (erasor::WorkQueue) -- BASELINE config 3 on a node with fewer GPUs than sequences.
static int queue_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    const int n_workers = std::max(1, atoi(argv[2])), max_frames = atoi(argv[3]);
    std::vector<std::string> jobs(argv + 4, argv + argc);
    int ndev = 1;
    {   // (the C ABI answers with ERASOR_E_NO_DEVICE for a device that does not exist: probe upwards)
        erasor_params p;
        erasor_hip_params_default(&p);
        for (ndev = 0; ndev < 64; ++ndev) {
            erasor_hip_handle *h = nullptr;
            if (erasor_hip_create(&p, ndev, &h) != ERASOR_OK) break;
            erasor_hip_destroy(h);
        }
        if (ndev == 0) return 4;
    }
    erasor::WorkQueue q(jobs.size());
    std::vector<int> rc(jobs.size(), -1), nodes(jobs.size(), 0);
    std::vector<double> t_begin(jobs.size(), 0), t_end(jobs.size(), 0);
    const double t0 = now_ms();
    std::vector<std::thread> th;
    for (int w = 0; w < n_workers; ++w)
        th.emplace_back([&, w] {
            for (long j; (j = q.next(w)) >= 0;) {
                t_begin[j] = now_ms() - t0;
                try {
                    rc[j] = run_config(jobs[j], max_frames, w % ndev, false, &nodes[j]);
                } catch (const std::exception &e) {
                    fprintf(stderr, "job %ld (%s): %s\n", j, jobs[j].c_str(), e.what());
                    rc[j] = 1;
                }
                t_end[j] = now_ms() - t0;
            }
        });
    for (auto &t : th) t.join();
    int bad = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        printf("job %zu %s: worker %d (device %d), %d nodes, %.1f .. %.1f ms, rc %d\n", j, jobs[j].c_str(), q.taken_by(j), q.taken_by(j) % ndev, nodes[j],
               t_begin[j], t_end[j], rc[j]);
        bad += rc[j] != 0;
    }
    printf("{\"mode\": \"queue\", \"workers\": %d, \"devices\": %d, \"jobs\": %zu, \"failed\": %d, \"wall_ms\": %.1f}\n", n_workers, ndev, jobs.size(), bad,
           now_ms() - t0);
    return bad ? 5 : 0;
}

// --replicas <n> <rosparam.yaml> [n_frames]: ONE process, n updaters (device r mod the visible devices), the global map loaded ONCE and
// replicated with erasor_hip_replicate_map (RCCL broadcast over xGMI / peer copies), then replica r works through nodes r, r + n, ... of the
// sequence on its own thread -- scan-parallel replicas (every replica folds ITS scans into ITS copy; a deviation from
// the reference's single sequential fold, which is why nothing is saved here: it reports what each replica removed).
static int replicas_mode(int argc, char **argv) {
    if (argc < 4) return 2;
    const int n = std::max(1, atoi(argv[2]));
    const int max_frames = argc > 4 ? atoi(argv[4]) : 1 << 30;
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    cfg.params.query_voxel_size = 0.05;
    cfg.params.removal_interval = 2;
    erasor::DriverConfig drv;
    if (!erasor::load_config_yaml(argv[3], cfg, &drv)) return 3;
    if (cfg.initial_map_path.empty() || cfg.initial_map_path == "/") cfg.initial_map_path = drv.data_dir + "/dense_global_map.pcd";
    const std::string map_path = cfg.initial_map_path;
    cfg.params.removal_interval = 1;  // (the interval is what spreads the nodes over the replicas here)
    int ndev = 0;
    for (; ndev < 64; ++ndev) {
        erasor_hip_handle *h = nullptr;
        if (erasor_hip_create(&cfg.params, ndev, &h) != ERASOR_OK) break;
        erasor_hip_destroy(h);
    }
    if (ndev == 0) return 4;
    std::vector<std::unique_ptr<erasor::OfflineMapUpdater>> up;
    for (int r = 0; r < n; ++r) {
        erasor::OfflineMapUpdater::Config c = cfg;
        c.device = r % ndev;
        c.initial_map_path = r == 0 ? map_path : std::string();  // only the root reads the file
        up.emplace_back(new erasor::OfflineMapUpdater(c));
    }
    std::vector<erasor_hip_handle *> hs;
    for (auto &u : up) hs.push_back(u->handle());
    int transport = 0;
    const double tb = now_ms();
    if (erasor_hip_replicate_map(hs.data(), n, 0, &transport) != ERASOR_OK) {
        fprintf(stderr, "erasor_hip_replicate_map: %s\n", erasor_hip_last_error(hs[0]));
        return 4;
    }
    const double ms_bcast = now_ms() - tb;
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(drv.data_dir + "/poses_lidar2body.csv", poses)) return 3;
    const int last = std::min<int>((int)poses.size(), drv.init_idx + max_frames);
    std::vector<unsigned long long> rejected(n, 0), map_out(n, 0);
    std::vector<int> done(n, 0);
    std::vector<std::thread> th;
    for (int r = 0; r < n; ++r)
        th.emplace_back([&, r] {
            for (int i = drv.init_idx + r; i < last; i += n) {
                char name[64];
                snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
                pcl::PointCloud<pcl::PointXYZI> scan;
                if (erasor_utils::load_pcd(drv.data_dir + name, scan) == -1) break;
                up[r]->callback_node(i, erasor_utils::eigen2geoPose(poses[i]), scan);
                rejected[r] += up[r]->last.n_map_rejected;
                map_out[r] = up[r]->last.n_map_out;
                ++done[r];
            }
        });
    for (auto &t : th) t.join();
    for (int r = 0; r < n; ++r)
        printf("replica %d (device %d): %d nodes, %llu map points rejected, map %llu\n", r, r % ndev, done[r], rejected[r], map_out[r]);
    printf("{\"mode\": \"replicas\", \"replicas\": %d, \"devices\": %d, \"transport\": \"%s\", \"replicate_ms\": %.2f}\n", n, ndev,
           transport == 1 ? "rccl" : (transport == 2 ? "peer copies" : "none"), ms_bcast);
    return 0;
}

// --mapgen <data_dir> <n_frames> <voxelsize> <is_large_scale>: src/mapgen/main.cpp:41-64 without ROS — every node of
// <data_dir>/poses_lidar2body.csv + pcds/%06d.pcd through mapgen::accumPointCloud, then saveNaiveMap
static int mapgen_mode(int argc, char **argv) {
    if (argc < 6) return 2;
    const std::string dir = argv[2];
    const int n = atoi(argv[3]);
    mapgen gen;
    gen.setValue(dir, (float)atof(argv[4]), "05", "0", std::to_string(n - 1), 1, atoi(argv[5]) != 0);
    std::vector<Eigen::Matrix4f> poses;
    if (!erasor::load_all_poses(dir + "/poses_lidar2body.csv", poses)) return 3;
    for (int i = 0; i < n && i < (int)poses.size(); ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
        pcl::PointCloud<pcl::PointXYZI> scan;
        if (erasor_utils::load_pcd(dir + name, scan) == -1) return 3;
        gen.accumPointCloud(erasor_utils::eigen2geoPose(poses[i]), scan);
    }
    pcl::PointCloud<pcl::PointXYZI> m, c;
    gen.getPointClouds(m, c);
    write_bin(dir + "/mapgen_cloud_map.bin", m);
    write_bin(dir + "/mapgen_cloud_curr.bin", c);
    gen.saveNaiveMap(dir + "/05_original.pcd", gen.map_file_name());
    printf("[MAPGEN] map saved to %s\n", gen.map_file_name().c_str());
    return 0;
}

// --voxelize <in.bin> <leaf> <out.bin>: the free function erasor_utils::voxelize_preserving_labels(Ptr, Cloud&, double)
// (utils.hpp:103), as OMU.cpp:186,238 / erasor.cpp:528 / mapgen.hpp:239 call it
static int voxelize_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    pcl::PointCloud<pcl::PointXYZI>::Ptr src(new pcl::PointCloud<pcl::PointXYZI>());
    pcl::PointCloud<pcl::PointXYZI> dst;
    if (!read_bin(argv[2], *src)) return 3;
    erasor_utils::voxelize_preserving_labels(src, dst, atof(argv[3]));
    write_bin(argv[4], dst);
    printf("voxelize_preserving_labels: %zu -> %zu\n", src->size(), dst.size());
    return 0;
}

// --bench <dir> <n_timed> <n_warmup>: what a caller of the drop-in surface gets, timed in C++ (no Python in the loop) on the workload
// tools/export_cpp_bench.py wrote (bench.py's config 2).  Three passes over the same nodes, each on a fresh map:
//   1. erasor::OfflineMapUpdater::callback_node, host cloud in (OMU.cpp:237 fromROSMsg has just produced it), map_rejected /
//      query_rejected clouds out on the host (what OMU.cpp:316-320 publishes) -- nothing announced;
//   2. the same with the next node announced (announce_next: what an offline driver or a node holding one message back can do);
//   3. the C ABI itself with the scans resident in HBM and nodes announced two ahead (bench.py's loop, minus Python).
// Prints ONE JSON line.
static int bench_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    const std::string dir = argv[2];
    const int K = atoi(argv[3]), W = atoi(argv[4]);
    erasor::OfflineMapUpdater::Config cfg;
    {
        std::ifstream f(dir + "/params.bin", std::ios::binary);
        if (!f.read(reinterpret_cast<char *>(&cfg.params), sizeof(cfg.params))) return 3;
    }
    std::vector<double> poses, l2b(7);
    {
        std::ifstream f(dir + "/poses.bin", std::ios::binary | std::ios::ate);
        if (!f) return 3;
        poses.resize((size_t)f.tellg() / 8);
        f.seekg(0);
        f.read(reinterpret_cast<char *>(poses.data()), (std::streamsize)(poses.size() * 8));
        std::ifstream g(dir + "/l2b.bin", std::ios::binary);
        if (!g.read(reinterpret_cast<char *>(l2b.data()), 56)) return 3;
    }
    const int n_nodes = (int)(poses.size() / 7);
    if (n_nodes < K + W + 2) {
        fprintf(stderr, "need %d nodes, %d exported\n", K + W + 2, n_nodes);
        return 3;
    }
    for (int k = 0; k < 7; ++k) cfg.lidar2body[k] = l2b[k];
    cfg.params.removal_interval = 1;
    cfg.verbose = false;
    pcl::PointCloud<pcl::PointXYZI> map0;
    if (!read_bin(dir + "/map.bin", map0)) return 3;
    const int NS = std::min(n_nodes, K + W + 8);  // (the deep pass announces up to six nodes ahead: as many more as were exported)
    std::vector<pcl::PointCloud<pcl::PointXYZI>> scans(NS);
    std::vector<geometry_msgs::Pose> odom(NS);
    for (int i = 0; i < NS; ++i) {
        char name[64];
        snprintf(name, sizeof(name), "/scan_%06d.bin", i);
        if (!read_bin(dir + name, scans[i])) return 3;
        const double *v = &poses[(size_t)i * 7];
        odom[i].position.x = v[0]; odom[i].position.y = v[1]; odom[i].position.z = v[2];
        odom[i].orientation.x = v[3]; odom[i].orientation.y = v[4]; odom[i].orientation.z = v[5]; odom[i].orientation.w = v[6];
    }
    double ms_cb[4] = {0, 0, 0, 0}, ms_announce = 0;
    unsigned long long rejected[4] = {0, 0, 0, 0}, map_out[4] = {0, 0, 0, 0};
    const int deep_la = std::max(1, std::min(6, NS - (K + W)));
    for (int pass = 0; pass < 4; ++pass) {
        erasor::OfflineMapUpdater updater(cfg);
        updater.set_global_map(map0);
        double t0 = 0;
        uint64_t ticket = 0, next_ticket = 0;
        std::vector<uint64_t> tk(NS, 0);
        int announced_upto = 0;  // (pass 3: nodes [1, announced_upto] are announced)
        if (pass == 3) {
            updater.set_lookahead(deep_la);
            tk[0] = updater.announce_upcoming(scans[0], odom[0]);  // (a first callback without a ticket would drop the nodes announced behind it)
        }
        for (int i = 0; i < W + K; ++i) {
            if (i == W) t0 = now_ms();
            if (pass == 3) {  // round 6: as many nodes ahead as the updater takes, in node order, each stepped by its ticket
                while (announced_upto < std::min(i + deep_la, NS - 1) && updater.outstanding() < updater.lookahead()) {
                    ++announced_upto;
                    if (i > 0 && announced_upto == i + deep_la) {  // the pipeline is full: the round's one new node is staged beside this callback's step
                        updater.announce_next_deferred(announced_upto, scans[announced_upto], odom[announced_upto]);
                        break;
                    }
                    tk[announced_upto] = updater.announce_next(scans[announced_upto], odom[announced_upto]);
                }
                updater.callback_node(i, odom[i], scans[i], tk[i]);
                if (i >= W) rejected[pass] += updater.map_rejected.size();
                continue;
            }
            if (pass == 1) {
                const double ta = now_ms();
                next_ticket = updater.announce_next(scans[i + 1], odom[i + 1]);
                if (i >= W) ms_announce += now_ms() - ta;
            } else if (pass == 2)
                updater.announce_next_deferred(i + 1, scans[i + 1], odom[i + 1]);  // (staged inside callback_node(i), beside its step)
            updater.callback_node(i, odom[i], scans[i], pass == 1 ? ticket : 0);
            ticket = next_ticket;
            if (i >= W) rejected[pass] += updater.map_rejected.size();  // (the host copies of what the node publishes)
        }
        ms_cb[pass] = (now_ms() - t0) / K;
        map_out[pass] = updater.last.n_map_out;
    }
    // pass 3: the C ABI, device-resident scans, nodes announced two ahead
    double ms_dev = 0;
    unsigned long long rejected_dev = 0, map_out_dev = 0;
    {
        erasor_hip_handle *h = nullptr;
        if (erasor_hip_create(&cfg.params, 0, &h) != ERASOR_OK) return 4;
        std::vector<float> buf(map0.size() * 4);
        for (size_t i = 0; i < map0.size(); ++i) { buf[4 * i] = map0.points[i].x; buf[4 * i + 1] = map0.points[i].y; buf[4 * i + 2] = map0.points[i].z; buf[4 * i + 3] = map0.points[i].intensity; }
        if (erasor_hip_set_map(h, buf.data(), map0.size()) != ERASOR_OK) return 4;
        std::vector<void *> d_scan(K + W + 2, nullptr);
        std::vector<size_t> n_scan(K + W + 2);
        std::vector<std::array<float, 16>> Tb(K + W + 2), To(K + W + 2);
        float Tl[16];
        geometry_msgs::Pose l2bp;
        l2bp.position.x = l2b[0]; l2bp.position.y = l2b[1]; l2bp.position.z = l2b[2];
        l2bp.orientation.x = l2b[3]; l2bp.orientation.y = l2b[4]; l2bp.orientation.z = l2b[5]; l2bp.orientation.w = l2b[6];
        const Eigen::Matrix4f TL = erasor_utils::geoPose2eigen(l2bp);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tl[4 * r + c] = TL(r, c);
        for (int i = 0; i < K + W + 2; ++i) {
            n_scan[i] = scans[i].size();
            buf.resize(n_scan[i] * 4);
            for (size_t j = 0; j < n_scan[i]; ++j) { buf[4 * j] = scans[i].points[j].x; buf[4 * j + 1] = scans[i].points[j].y; buf[4 * j + 2] = scans[i].points[j].z; buf[4 * j + 3] = scans[i].points[j].intensity; }
            if (erasor_hip_device_alloc(h, n_scan[i] * 16, &d_scan[i]) != ERASOR_OK || erasor_hip_device_upload(h, d_scan[i], buf.data(), n_scan[i] * 16) != ERASOR_OK) return 4;
            const Eigen::Matrix4f T = erasor_utils::geoPose2eigen(odom[i]), Ti = erasor_utils::inverse(T);
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { Tb[i][4 * r + c] = T(r, c); To[i][4 * r + c] = Ti(r, c); }
        }
        for (int j = 0; j < 2; ++j) {
            erasor_hip_prefetch_node(h, d_scan[j], n_scan[j], 1, Tl, Tb[j].data());
            erasor_hip_announce_origin2body(h, To[j].data());
        }
        double t0 = 0;
        erasor_step_result res;
        for (int i = 0; i < W + K; ++i) {
            if (i == W) t0 = now_ms();
            if (i + 2 < W + K + 2) {
                erasor_hip_prefetch_node(h, d_scan[i + 2], n_scan[i + 2], 1, Tl, Tb[i + 2].data());
                erasor_hip_announce_origin2body(h, To[i + 2].data());
            }
            if (erasor_hip_step_device(h, d_scan[i], n_scan[i], Tl, Tb[i].data(), To[i].data(), &res) != ERASOR_OK) {
                fprintf(stderr, "step %d: %s\n", i, erasor_hip_last_error(h));
                return 4;
            }
            if (i >= W) rejected_dev += res.n_map_rejected;
        }
        ms_dev = (now_ms() - t0) / K;
        map_out_dev = res.n_map_out;
        for (void *p : d_scan) erasor_hip_device_free(h, p);
        erasor_hip_destroy(h);
    }
    const bool same = rejected[0] == rejected[1] && rejected[0] == rejected[2] && rejected[0] == rejected[3] && rejected[0] == rejected_dev &&
                      map_out[0] == map_out[1] && map_out[0] == map_out[2] && map_out[0] == map_out[3] && map_out[0] == map_out_dev;
    printf("{\"bench\": \"erasor_offline_demo --bench (C++, no Python in the loop)\", \"nodes_timed\": %d, \"warmup\": %d, \"map_points\": %zu, "
           "\"scan_points\": %zu, \"ms_per_callback\": %.4f, \"ms_per_callback_next_node_announced\": %.4f, "
           "\"of_which_announce_next\": %.4f, \"ms_per_callback_next_node_announced_deferred\": %.4f, \"ms_per_callback_nodes_announced_deep\": %.4f, \"deep_lookahead\": %d, \"ms_per_step_device_resident_two_ahead\": %.4f, \"callback_note\": \"OfflineMapUpdater::callback_node: host PointXYZI cloud in "
           "(32-byte records staged as they lie; an announced node is stepped by its ticket), map_rejected / query_rejected clouds copied back to the host\", "
           "\"map_rejected_points\": %llu, \"final_map_points\": %llu, \"passes_agree\": %s}\n",
           K, W, map0.size(), scans[W].size(), ms_cb[0], ms_cb[1], ms_announce / K, ms_cb[2], ms_cb[3], deep_la, ms_dev, rejected[0], map_out[0], same ? "true" : "false");
    return same ? 0 : 5;
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "--bench") {
        try {
            return bench_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--queue" || std::string(argv[1]) == "--replicas")) {
        try {
            return std::string(argv[1]) == "--queue" ? queue_mode(argc, argv) : replicas_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--voxelize") {
        try {
            return voxelize_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--eval") {
        try {
            return eval_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--render" || std::string(argv[1]) == "--render-compare" || std::string(argv[1]) == "--render-eval")) {
        try {
            const std::string mode = argv[1];
            return mode == "--render" ? render_mode(argc, argv) : mode == "--render-compare" ? render_compare_mode(argc, argv) : render_eval_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--eval-classes") {
        try {
            return eval_classes_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--sweep" || std::string(argv[1]) == "--eval-many")) {
        try {
            return std::string(argv[1]) == "--sweep" ? sweep_mode(argc, argv) : eval_many_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--align") {
        try {
            return align_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--refine" || std::string(argv[1]) == "--refine-plane")) {
        try {
            return refine_mode(argc, argv, std::string(argv[1]) == "--refine-plane");
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--visibility") {
        try {
            return visibility_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--carve") {
        try {
            return carve_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--ground" || std::string(argv[1]) == "--ground-map")) {
        try {
            const int st = std::string(argv[1]) == "--ground" ? ground_mode(argc, argv) : ground_map_mode(argc, argv);
            if (st == 2)
                fprintf(stderr, "usage: %s --ground <rosparam.yaml> <out_dir> [n_frames] [n_rings n_sectors max_range]\n"
                                "       %s --ground-map <rosparam.yaml> <map.pcd|-> <ground_out.pcd> <rest_out.pcd> [n_frames] [min_votes] [ratio]\n",
                        argv[0], argv[0]);
            return st;
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--label-scans") {
        try {
            return label_scans_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--clusters" || std::string(argv[1]) == "--residue")) {
        try {
            return std::string(argv[1]) == "--clusters" ? clusters_mode(argc, argv) : residue_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--objects") {
        try {
            const int st = objects_mode(argc, argv);
            if (st == 2)
                fprintf(stderr, "usage: %s --objects <raw.pcd> <ground.pcd|-> <out.pcd> <tol> <vote_thr> <remove_ratio> <revert_ratio> <max_size> <kept1.pcd> "
                                "[<kept2.pcd> ...] [--tau t]\n", argv[0]);
            return st;
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--denoise" || std::string(argv[1]) == "--density")) {
        try {
            return std::string(argv[1]) == "--denoise" ? denoise_mode(argc, argv) : density_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--normals") {
        try {
            return normals_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--analyze") {
        try {
            return analyze_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--label" || std::string(argv[1]) == "--complement")) {
        try {
            return std::string(argv[1]) == "--label" ? label_mode(argc, argv) : complement_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && std::string(argv[1]) == "--mapgen") {
        try {
            return mapgen_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc >= 2 && (std::string(argv[1]) == "--erasor-class" || std::string(argv[1]) == "--config")) {
        try {
            return std::string(argv[1]) == "--config" ? config_mode(argc, argv) : erasor_class_mode(argc, argv);
        } catch (const std::exception &e) {
            fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    if (argc < 3) {
        fprintf(stderr,
                "usage: %s <data_dir> <n_frames> [version] [removal_interval] [gt]\n       %s --config <rosparam.yaml> [n_frames] [gt]\n"
                "       %s --eval <gt> <est> [voxelsize] [voxel_leaf]\n       %s --eval-classes <gt> <est> [voxelsize] [voxel_leaf]\n"
                "       %s --analyze <gt> <est> [voxelsize] [voxel_leaf]\n       %s --align <rosparam.yaml> [n_frames] [voxelsize]\n"
                "       %s --label <map> <dense_labelled> [leaf]\n       %s --complement <est> <gt> <out.pcd>\n"
                "       %s --sweep <rosparam.yaml> <grid.yaml> <gt> [n_frames] [voxelsize] [concurrency]\n"
                "       %s --eval-many <voxelsize> <voxel_leaf> <gt> <est1> [<est2> ...]\n"
                "       %s --label-scans <rosparam.yaml> <static.pcd> <raw.pcd|-> <out_dir> [n_frames] [tau]\n"
                "       %s --refine <rosparam.yaml> <poses_out> [n_frames] [max_dist] [max_iters]\n"
                "       %s --refine-plane <rosparam.yaml> <poses_out> [n_frames] [max_dist] [max_iters] [k]\n"
                "       %s --clusters <cloud.pcd> <tol> [min_size] [max_size] [kept_out.pcd]\n"
                "       %s --residue <gt> <est> [tol] [voxelsize] [voxel_leaf]\n"
                "       %s --denoise <in.pcd> <out.pcd> sor <k> <mul> | ror <radius> <min_neighbors> | kth <k> <thr>\n"
                "       %s --density <cloud.pcd> <k>\n"
                "       %s --normals <in.pcd> <out.pcd> <k> [vx vy vz]\n"
                "       %s --visibility <rosparam.yaml> <map.pcd|-> <out.pcd> [n_frames] [W H el_bottom el_top] [window] [k]\n"
                "       %s --carve <rosparam.yaml> <map.pcd|-> <out.pcd> [n_frames] [voxel] [max_range] [stop_short]\n"
                "       %s --ground <rosparam.yaml> <out_dir> [n_frames] [n_rings n_sectors max_range]\n"
                "       %s --ground-map <rosparam.yaml> <map.pcd|-> <ground_out.pcd> <rest_out.pcd> [n_frames] [min_votes] [ratio]\n"
                "       %s --objects <raw.pcd> <ground.pcd|-> <out.pcd> <tol> <vote_thr> <remove_ratio> <revert_ratio> <max_size> <kept1.pcd> [<kept2.pcd> ...] [--tau t]\n",
                argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0],
                argv[0], argv[0], argv[0], argv[0], argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int n = atoi(argv[2]);
    erasor::OfflineMapUpdater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    // config/seq_05.yaml
    cfg.params.max_range = 60.0; cfg.params.num_rings = 15; cfg.params.num_sectors = 60; cfg.params.min_h = -1.3; cfg.params.max_h = 3.2;
    cfg.params.th_bin_max_h = 0.05; cfg.params.scan_ratio_threshold = 0.3; cfg.params.minimum_num_pts = 10; cfg.params.gf_dist_thr = 0.15;
    cfg.params.gf_iter = 3; cfg.params.gf_num_lpr = 10; cfg.params.gf_th_seeds_height = 0.5; cfg.params.query_voxel_size = 0.2;
    cfg.params.version = argc > 3 ? atoi(argv[3]) : 3;
    cfg.params.removal_interval = argc > 4 ? atoi(argv[4]) : 1;
    cfg.lidar2body[2] = 1.73;
    cfg.initial_map_path = dir + "/map.pcd";
    cfg.save_path = dir;
    cfg.data_name = "05";
    try {
        erasor::OfflineMapUpdater updater(cfg);
        std::ifstream in(dir + "/poses.csv");
        std::string line;
        std::getline(in, line);  // header
        for (int i = 0; i < n; ++i) {
            if (!std::getline(in, line)) break;
            std::vector<double> v;
            std::stringstream ss(line);
            std::string t;
            while (std::getline(ss, t, ',')) v.push_back(atof(t.c_str()));
            geometry_msgs::Pose odom;
            odom.position.x = v[2]; odom.position.y = v[3]; odom.position.z = v[4];
            odom.orientation.x = v[5]; odom.orientation.y = v[6]; odom.orientation.z = v[7]; odom.orientation.w = v[8];
            char name[64];
            snprintf(name, sizeof(name), "/pcds/%06d.pcd", i);
            pcl::PointCloud<pcl::PointXYZI> scan;
            if (erasor_utils::load_pcd(dir + name, scan) == -1) return 3;
            updater.callback_node(i, odom, scan);
            printf("frame %d: voi %llu rejected %llu reverted bins %u map %llu\n", i, (unsigned long long)updater.last.n_voi,
                   (unsigned long long)updater.last.n_map_rejected, updater.last.n_reverted_bins, (unsigned long long)updater.last.n_map_out);
        }
        pcl::PointCloud<pcl::PointXYZI> m;
        updater.get_map(m);
        erasor_utils::save_pcd_ascii(dir + "/map_final.pcd", m);
        write_bin(dir + "/map_final.bin", m);
        updater.save_static_map(0.2f);
        if (argc > 5) return evaluate_saved_map(updater, argv[5]);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
