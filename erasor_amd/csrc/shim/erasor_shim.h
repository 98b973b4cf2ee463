// erasor_shim.h — the reference's C++ surface for the hot path, backed by liberasor_hip.so.
//
// Same class / function names, argument meaning and error behaviour as
//   include/erasor/erasor.h:43-147            (class ERASOR)
//   include/erasor/OfflineMapUpdater.h:9-151   (class erasor::OfflineMapUpdater)
//   include/tools/erasor_utils.hpp:50-108      (namespace erasor_utils)
// minus ROS: parameters arrive in an erasor_params struct instead of the rosparam server, the per-node
// message is passed as (seq, odom pose, lidar cloud), debug topics become public clouds.
#ifndef ERASOR_SHIM_H
#define ERASOR_SHIM_H

#include "erasor_shim_queue.h"
#include <memory>
#include <stdexcept>
#include <deque>
#include <string>
#include <vector>

#include "../../../include/erasor_hip.h"
#include "erasor_shim_types.h"
#ifdef ERASOR_SHIM_WITH_ROS
#include <ros/ros.h>
#endif

namespace erasor_utils {
typedef pcl::PointCloud<pcl::PointXYZI> Cloud;
// utils.cpp:35-55 (tf::Matrix3x3(tf::Quaternion) in double, narrowed to float)
Eigen::Matrix4f geoPose2eigen(const geometry_msgs::Pose &geoPose);
// tf_body2origin_.inverse() (OMU.cpp:436): double-precision cofactor inverse, narrowed
Eigen::Matrix4f inverse(const Eigen::Matrix4f &T);
// utils.cpp:57-78
void parse_dynamic_obj(const Cloud &cloudIn, Cloud &dynamicOut, Cloud &staticOut);
// utils.cpp:116-138
void count_stat_dyn(const Cloud &cloudIn, int &num_static, int &num_dynamic);
// utils.cpp:6-33 (tf::Matrix3x3::getRotation in double)
geometry_msgs::Pose eigen2geoPose(const Eigen::Matrix4f &pose);
// utils.hpp:75-93 — .pcd with fields x y z [intensity] (ASCII, binary with any SIZE/TYPE/COUNT layout,
// binary_compressed); returns -1 on failure like the reference
int load_pcd(const std::string &pcd_name, Cloud &dst);
// pcl::io::savePCDFileASCII as used at OMU.cpp:193 (PCL's default: 8 significant digits), and the lossless binary form
int save_pcd_ascii(const std::string &pcd_name, const Cloud &src);
int save_pcd_binary(const std::string &pcd_name, const Cloud &src);
// a cloud with its normals (erasor_hip_normals_*): binary, fields x y z intensity normal_x normal_y normal_z curvature, all float32 -- the
// layout of pcl::PointXYZINormal's fields.  xyzi: n rows of 4, normals: n rows of 3, curvature: n
int save_pcd_normals_binary(const std::string &pcd_name, const float *xyzi, const float *normals, const float *curvature, size_t n);
// utils.cpp:80-114, same signature as utils.hpp:103 (called at OMU.cpp:186,238, erasor.cpp:528, mapgen.hpp:239,252,295):
// PCL VoxelGrid + exact 1-NN label, on the GPU (erasor_hip_voxelize_preserving_labels).  The free function has no
// object to hang a device handle on: it uses one process-wide handle on device `voxelize_device()` (default 0).
void voxelize_preserving_labels(Cloud::Ptr src, Cloud &dst, double leaf_size);
int &voxelize_device();
}  // namespace erasor_utils

// struct Bin / R_POD / Ring of the reference (erasor.h:24-41), same member names
struct Bin {
    double max_h;
    double min_h;
    double x;
    double y;
    double status;
    bool is_occupied;
    pcl::PointCloud<pcl::PointXYZI> points;
};
typedef std::vector<std::vector<Bin>> R_POD;
typedef std::vector<Bin> Ring;

// class ERASOR (erasor.h:43-228).  Inputs of set_inputs are egocentric clouds, as in the reference.
class ERASOR {
public:
    explicit ERASOR(const erasor_params &p, int device = 0);
#ifdef ERASOR_SHIM_WITH_ROS
    // the reference's constructor (erasor.h:46-61): parameters from the rosparam server under their reference names
    explicit ERASOR(ros::NodeHandle *nodehandler);
#endif
    ~ERASOR();
    void set_inputs(const pcl::PointCloud<pcl::PointXYZI> &map_voi, const pcl::PointCloud<pcl::PointXYZI> &query_voi);  // erasor.cpp:57-85
    void compare_vois_and_revert_ground(int frame);           // v2, erasor.cpp:332-434
    void compare_vois_and_revert_ground_w_block(int frame);   // v3, erasor.cpp:438-571
    void get_static_estimate(pcl::PointCloud<pcl::PointXYZI> &arranged, pcl::PointCloud<pcl::PointXYZI> &complement);  // :612-626
    void get_outliers(pcl::PointCloud<pcl::PointXYZI> &map_rejected, pcl::PointCloud<pcl::PointXYZI> &curr_rejected);   // :322-327
    double get_max_range();  // :628
    // erasor.cpp:573-595: is a CURR_IS_HIGHER bin within (r_range, theta_range) of the target?  Works on the R-POD it is
    // given (the reference passes r_pod_selected) and keeps the reference's theta wrap by num_rings.
    bool is_dynamic_obj_close(R_POD &r_pod_selected, int r_target, int theta_target, int r_range, int theta_range);
    // erasor.h:143-145, filled by compare_*: r_pod[ring][sector]; Bin::points are the device's bin lists (egocentric),
    // max_h / min_h / is_occupied / status as the reference leaves them (x, y: the bin's highest point, erasor.cpp:91-94)
    R_POD r_pod_map, r_pod_curr, r_pod_selected;
    // Rebuilding the three R-PODs costs six read-backs (each with a stream synchronisation) and a per-point host loop after
    // EVERY compare_* call.  A caller that only wants get_static_estimate / get_outliers sets this to false; fetch_rpods()
    // fills them on demand for the last compare_* call.
    bool keep_rpods = true;
    void fetch_rpods();
    // guard counters of the last compare_* call (erasor_step_result): a non-zero n_ambiguous means a point sat within 1e-11 of a
    // sector boundary, where the device's atan2 may round differently from glibc's -- bin membership of that point is then not
    // provably the reference's
    unsigned n_ambiguous = 0, n_neg_sector = 0, n_degenerate_plane = 0;
    // public members of the reference (erasor.h:127,139-141)
    pcl::PointCloud<pcl::PointXYZI> ground_viz, debug_curr_rejected, debug_map_rejected, map_complement;
    // r_pod_selected[r][theta].status after compare_* (erasor.h:145), index = ring*num_sectors + sector
    std::vector<double> status;

private:
    void run(int version);
    erasor_params P_;
    int device_;
    erasor_hip_handle *h_[2] = {nullptr, nullptr};  // one handle per algorithm version
    int last_run_ = -1;                             // which of the two the last compare_* call used
    pcl::PointCloud<pcl::PointXYZI> map_voi_, query_voi_, arranged_;
};

// class mapgen (src/mapgen/mapgen.hpp:27-305): builds the naive accumulated map that OfflineMapUpdater later loads.
// Same public methods; the erasor::node message is passed as (odom pose, lidar cloud), nav_msgs::Path is dropped.
class mapgen {
public:
    explicit mapgen(int device = 0);
    ~mapgen();
    void setValue(std::string pcd_save_path, float voxelsize, std::string sequence, std::string init_time_stamp, std::string final_time_stamp,
                  int frame_interval, bool is_map_large_scale);                                                   // mapgen.hpp:182-196
    void accumPointCloud(const geometry_msgs::Pose &odom, const pcl::PointCloud<pcl::PointXYZI> &lidar);         // :198-257
    void getPointClouds(pcl::PointCloud<pcl::PointXYZI> &map_out, pcl::PointCloud<pcl::PointXYZI> &curr_out);   // :258-262
    void saveNaiveMap(const std::string &original_dir, const std::string &map_dir);                              // :264-303
    // main.cpp:34-38: <save_path>/<seq>_<from>_to_<to>_w_interval<k>_voxel_<leaf>.pcd
    std::string map_file_name() const;

private:
    erasor_hip_handle *h_ = nullptr;
    float leafsize_ = 0.05f;
    std::string seq_, init_stamp_, final_stamp_, save_path_;
    int interval_ = 1;
    bool is_large_scale_ = false;
};

namespace erasor {
// erasor::OfflineMapUpdater (OfflineMapUpdater.h:9-151): owns the (device-resident) map, one callback per node.
class OfflineMapUpdater {
public:
    struct Config {
        erasor_params params;                                  // /erasor/*, /MapUpdater/* (set_params, OMU.cpp:63-105)
        double lidar2body[7] = {0, 0, 0, 0, 0, 0, 1};          // /tf/lidar2body: x y z qx qy qz qw (OMU.cpp:89-104)
        std::string environment = "outdoor";                   // /MapUpdater/env
        std::string initial_map_path, save_path = ".", data_name = "00";
        bool is_large_scale = false;                           // /large_scale/is_large_scale (OMU.cpp:75)
        double submap_size = 200.0;                            // /large_scale/submap_size   (OMU.cpp:76)
        bool verbose = false;
        int device = 0;
    };
    explicit OfflineMapUpdater(const Config &cfg);            // OMU.cpp:5-32 (+ load_global_map when a path is given)
    ~OfflineMapUpdater();
    void set_global_map(const pcl::PointCloud<pcl::PointXYZI> &map_init);  // load_global_map's copy, OMU.cpp:133
    // one erasor::node message: header.seq, odom, lidar (msg/node.msg:1-4) — OMU.cpp:203-330
    void callback_node(int seq, const geometry_msgs::Pose &odom, const pcl::PointCloud<pcl::PointXYZI> &lidar);
    // Offline look-ahead (no counterpart in the reference, which learns about a node when its message arrives): called BEFORE
    // callback_node(k) with the cloud of node k + 1 -- tell the updater which cloud the callback after the upcoming one brings.  Its
    // voxelisation / binning then overlap the current node's map-side stages; results are unchanged.  Ignored (returns 0) for nodes
    // the removal_interval gate skips.  The cloud is copied at once: it is the caller's again when the call returns.
    // Round 4: the call returns a TICKET.  Hand it to the callback of that node (callback_node(seq, odom, lidar, ticket)) and nothing
    // has to be recognised: the step runs on the announced copy, the cloud is not read again.  Without a ticket the callback's cloud
    // is compared with the announced copy record by record (a hash of every point, ~0.1 ms): a cloud that differs anywhere is
    // processed as the new cloud it is -- rounds 2-3 sampled 257 points and could run on a stale copy.
    uint64_t announce_next(const pcl::PointCloud<pcl::PointXYZI> &lidar);
    // ... and its odometry, when the whole next node is known (erasor_hip_prefetch_node: the VoI pass of the next callback is
    // launched ahead as well)
    uint64_t announce_next(const pcl::PointCloud<pcl::PointXYZI> &lidar, const geometry_msgs::Pose &odom);
    // Round 6 -- DEEP look-ahead for drivers that know their nodes ahead (main_in_your_env.cpp:92-123 reads them from disk): after
    // set_lookahead(n), n = 1 .. 7, announce_next may be called for up to n nodes beyond the upcoming callback, IN NODE ORDER (each call is
    // about the node behind the last one announced or gated; with nothing announced beyond it: the node behind the upcoming callback's).
    // With three or more nodes ahead the library lets consecutive steps overlap and the announced nodes' query chains share their launches
    // (erasor_hip_chain_batch): the offline rate of the C ABI through the reference's own class.
    //
    // THE CONTRACT OF AN ANNOUNCEMENT (announce_next, announce_upcoming, announce_next_deferred) -- last_announce() says which it was:
    //   ANNOUNCED  the node is staged; announce_next / announce_upcoming returned its ticket (never 0).
    //   FULL       nothing was taken and NOTHING MOVED: n nodes are announced beyond the upcoming callback, or 7 in all (the library's
    //              query sides).  The call is still about the same node: make it again before a later callback, while the node is still
    //              beyond the upcoming callback (a node whose own callback is the upcoming one is past announcing; it simply comes
    //              without a ticket).  The capacity test comes FIRST: a node the removal_interval gate will skip is answered FULL as well
    //              while outstanding() >= lookahead(), and GATED once there is room -- so `returned 0 && outstanding() >= lookahead()`
    //              is the same test as last_announce() == FULL, and a caller that retries on either never retries a node the updater
    //              has moved past.
    //   GATED      the removal_interval gate skips that node (OMU.cpp:206-209): nothing to announce, the updater has moved past it; the
    //              next call is about the node behind it.
    //   NOT_FIRST  announce_upcoming while something is announced already: nothing moved.
    //   PENDING    announce_next_deferred has been called and the upcoming callback has not run yet; after that callback it is one of
    //              ANNOUNCED / GATED / FULL like any other (FULL: the cloud was NOT taken -- hand the node over again).
    // A callback takes its node's announcement by the TICKET it is handed, or by itself when the node came through
    // announce_next_deferred.  A callback without a ticket hands its cloud to the library, which compares it with the oldest announced
    // copy (pointer, size, every record): the same cloud consumes that announcement and the nodes behind it stay announced; any other
    // cloud is the fresh scan it is, and every announcement in front of which it arrived is dropped (their nodes then come as fresh scans
    // too: a ticket the updater no longer holds -- dropped, consumed, or never given out -- counts as no ticket; announcing goes on with
    // the node behind the last one handed over).  Only an announcement that has not started yet (the latest, with no step since) survives
    // a foreign cloud: announce_next(k + 1) in front of an unannounced callback_node(k), the first node of a sequence.
    // save_static_map drops what is announced (its voxelisation borrows the query sides).
    enum AnnounceStatus { ANNOUNCED = 0, GATED = 1, FULL = 2, NOT_FIRST = 3, PENDING = 4 };
    void set_lookahead(int n);
    // ... and the node the UPCOMING callback itself brings, while nothing is announced yet (the first node of a sequence); 0 if something
    // is announced already (NOT_FIRST) or the gate skips the node (GATED)
    uint64_t announce_upcoming(const pcl::PointCloud<pcl::PointXYZI> &lidar, const geometry_msgs::Pose &odom);
    int lookahead() const { return max_ahead_; }
    int outstanding() const { return (int)ahead_.size(); }  // nodes announced and not yet stepped or dropped, the upcoming callback's own included
    AnnounceStatus last_announce() const { return announce_status_; }
    // the callback of an announced node, by ticket (0, or a ticket the updater does not hold for this node: like the three-argument form)
    void callback_node(int seq, const geometry_msgs::Pose &odom, const pcl::PointCloud<pcl::PointXYZI> &lidar, uint64_t ticket);
    // The same announcement WITHOUT the copy on the caller's time: the cloud is staged by the UPCOMING callback_node while that node's
    // own step runs on the GPU (0.1 ms of host work per 125 k-point cloud that no longer precedes the step) -- AFTER that callback has
    // taken its own announcement, so the hand-over finds room where announce_next in front of the callback would not.  `lidar` must stay
    // alive and unchanged until that callback has returned (the updater does not look at it afterwards, taken or not); the callback of
    // that node then finds its ticket by itself.  `seq` is what staged() answers to; WHICH node it is follows from the order of the calls.
    void announce_next_deferred(int seq, const pcl::PointCloud<pcl::PointXYZI> &lidar, const geometry_msgs::Pose &odom);
    // is node `seq` staged (its callback will not look at the cloud it is handed)?
    bool staged(int seq) const {
        for (const auto &a : ahead_)
            if (a.by_seq && a.seq == seq) return true;
        return false;
    }
    // read-only counters for tests and drivers: callbacks stepped by a ticket (handed in or found), and announcements the updater or the
    // library dropped unstepped (a foreign cloud without a ticket in front of them, save_static_map)
    size_t stepped_by_ticket() const { return n_ticket_steps_; }
    size_t announcements_dropped() const { return n_dropped_; }
    void save_static_map(float voxel_size);                    // OMU.cpp:174-196
    void get_map(pcl::PointCloud<pcl::PointXYZI> &dst);        // *map_arranged_
    erasor_hip_handle *handle() { return h_; }                 // for adapters that read more of the last step (ros1_adapter.cpp)
    // last step's products (the clouds the reference publishes, OMU.cpp:316-320)
    pcl::PointCloud<pcl::PointXYZI> map_rejected, query_rejected;
    erasor_step_result last;
    size_t num_processed = 0;

private:
    Config cfg_;
    erasor_hip_handle *h_ = nullptr;
    Eigen::Matrix4f tf_lidar2body_, tf_body2origin_;
    int stack_count_ = 0;
    // nodes announced and not yet stepped, oldest first (node order): the callback number each one belongs to (stack_count_ counts
    // callbacks, gated ones too), its ticket, and for announce_next_deferred the caller's sequence number (that callback takes the ticket by
    // itself).  Up to max_ahead_ beyond the upcoming callback (set_lookahead).  ahead_upto_: callback number of the last node an
    // announcement was made -- or skipped by the gate -- for; a refusal for capacity leaves it alone
    struct Ahead {
        int cb_no;
        uint64_t ticket;
        int seq;
        bool by_seq;
    };
    std::deque<Ahead> ahead_;
    int max_ahead_ = 1, ahead_upto_ = 0;
    AnnounceStatus announce_status_ = ANNOUNCED;
    size_t n_ticket_steps_ = 0, n_dropped_ = 0;
    const pcl::PointCloud<pcl::PointXYZI> *def_cloud_ = nullptr;  // announce_next_deferred: staged by the upcoming callback
    geometry_msgs::Pose def_odom_;
    int def_seq_ = 0;
    bool full(int upcoming_cb, bool gated) const;  // the capacity test of an announcement (upcoming_cb: the callback in front of it)
    void forget_announced();                       // the library has dropped what was announced: the books follow
    void stage_deferred();
    uint64_t announce(const pcl::PointCloud<pcl::PointXYZI> &lidar, const geometry_msgs::Pose *odom, bool upcoming = false);
};
// main_in_your_env.cpp:66-70: the driver's own rosparams
struct DriverConfig {
    std::string data_dir = "/";
    double voxel_size = 0.075;
    int init_idx = 0, interval = 2;
};
// Reads a rosparam YAML file in the reference's layout (config/*.yaml).  Keys that are absent keep the values already
// in cfg (fill it with the reference's defaults first: erasor_hip_params_default + OMU.cpp:66-83).
bool load_config_yaml(const std::string &path, OfflineMapUpdater::Config &cfg, DriverConfig *drv = nullptr);
// a sweep grid (erasor_offline_demo --sweep): a file in the rosparam layout whose flow-list values `[a, b, ...]` are axes and whose
// scalars override the base file; only the keys that set the step's parameters (/erasor/*, /MapUpdater/query_voxel_size,
// /MapUpdater/removal_interval, /large_scale/*).  configs: the base file with the scalars and one value of every axis, as
// load_config_yaml reads it, for the Cartesian product of the axes in file order (the last axis varying fastest).
struct SweepGrid {
    std::vector<std::string> axes;                                   // the swept keys, in file order
    std::vector<std::pair<std::string, std::string>> scalars;        // the grid's scalar overrides, in file order
    std::vector<std::vector<std::string>> values;                    // per configuration: the value of every axis, as written
    std::vector<OfflineMapUpdater::Config> configs;
    OfflineMapUpdater::Config base;                                  // the base file with the scalars applied
};
// 0, or -1 (a file unreadable, an empty list), -2 (a key a grid may not set: *bad), -3 (more than cap configurations)
int expand_sweep_grid(const std::string &base_yaml, const std::string &grid_yaml, size_t cap, SweepGrid &out, DriverConfig *drv, std::string *bad);
// main_in_your_env.cpp:33-59: poses_lidar2body.csv -> 4x4 float transforms (one per line after the header)
bool load_all_poses(const std::string &txt, std::vector<Eigen::Matrix4f> &poses);
}  // namespace erasor
#endif
