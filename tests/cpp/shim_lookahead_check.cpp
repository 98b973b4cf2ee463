// shim_lookahead_check.cpp — scripted callers of erasor::OfflineMapUpdater's look-ahead (announce_upcoming, announce_next,
// announce_next_deferred, callback_node with and without a ticket) under the removal_interval gate.  TEST INFRASTRUCTURE.
//   shim_lookahead_check <dir> <out_prefix> <n_scans> <removal_interval> <lookaheads: 1,2,7> <policy> <seeds: first:count>
// <dir>/map.pcd, <dir>/scan%d.bin (XYZI float32), <dir>/poses.txt (7 doubles per line), n_scans of each; node k brings scan and pose
// k % n_scans.  For every seed and every lookahead one SCRIPT: a fresh updater, N = 3 * interval + lookahead + 3 nodes, driven by the
// policy; an exception ends the script (it is reported, the program goes on).  Written:
//   <out_prefix>log.txt   one line per shim call: operation, node, whether a ticket came back / was handed in, outstanding() and the
//                         library's own count of announced nodes after the call, the announcement's status, whether the call threw
//   <out_prefix>res.bin   chunks {int32 kind, a, b, payload bytes} + payload: 1 script (a lookahead, b seed), 8 the scans' T_body2origin
//                         and T_origin2body as the shim computes them (n_scans x 32 floats), 2 processed callback (a node), 3 map_rejected,
//                         4 query_rejected, 5 the `last` result block, 6 the final map, 7 end of script (a threw, b calls after which
//                         outstanding() differed from the library's count)
// Policies (all but `ticketless` keep to erasor_shim.h):
//   window           the offline driver's loop: announce_upcoming for the first node, announce_next up to node i + lookahead in front of
//                    callback i, the round's one new node (i + lookahead) through announce_next_deferred
//   greedy           no window: in front of every callback, announce_next node after node until the updater answers 0; a node refused
//                    while outstanding() >= lookahead() is tried again in front of the next callback, any other 0 is the gate's
//   greedy_deferred  greedy, but the node refused for capacity is handed over with announce_next_deferred at once
//   ticketless       window's announcements, every callback through the three-argument callback_node
//   stop_and_go      window, but nothing is announced in front of callbacks N/3 .. 2N/3 - 1
//   random           seeded: in front of every callback some announce_next calls, an announce_next_deferred, or nothing; a callback
//                    hands in the ticket it holds, or (one time in four) none -- and then, every other time, its cloud in another buffer
//                    than the announced one (the library does not recognise it: a fresh scan); refusals are read from last_announce()
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../erasor_amd/csrc/shim/erasor_shim.h"

typedef pcl::PointCloud<pcl::PointXYZI> Cloud;
typedef erasor::OfflineMapUpdater Updater;

static FILE *g_log = nullptr, *g_res = nullptr;

static void chunk(int kind, int a, int b, const void *payload, size_t bytes) {
    const int head[4] = {kind, a, b, (int)bytes};
    fwrite(head, sizeof(head), 1, g_res);
    if (bytes) fwrite(payload, 1, bytes, g_res);
}
static void chunk_cloud(int kind, const Cloud &c) {
    std::vector<float> v(c.size() * 4);
    for (size_t i = 0; i < c.size(); ++i) {
        v[4 * i] = c.points[i].x; v[4 * i + 1] = c.points[i].y; v[4 * i + 2] = c.points[i].z; v[4 * i + 3] = c.points[i].intensity;
    }
    chunk(kind, (int)c.size(), 0, v.data(), v.size() * sizeof(float));
}
static const char *status_name(Updater::AnnounceStatus s) {
    switch (s) {
        case Updater::ANNOUNCED: return "announced";
        case Updater::GATED: return "gated";
        case Updater::FULL: return "full";
        case Updater::NOT_FIRST: return "not_first";
        default: return "pending";
    }
}

struct Script {
    Updater &up;
    const std::vector<Cloud> &scans;
    const std::vector<geometry_msgs::Pose> &odom;
    int N, L, interval;
    std::string policy;
    std::mt19937 rng;
    std::vector<uint64_t> ticket;
    int p = 0;                        // the next node to announce
    int deferred = -1;                // the node handed over with announce_next_deferred in front of the upcoming callback
    std::unique_ptr<Cloud> def_copy;  // its cloud: alive until that callback has returned, not a moment longer
    int mismatches = 0;
    const char *op = "";              // the call being made (for the log line of a call that throws)
    int op_node = -1;
    Script(Updater &u, const std::vector<Cloud> &s, const std::vector<geometry_msgs::Pose> &o, int n, int l, int iv, const std::string &pol, unsigned seed)
        : up(u), scans(s), odom(o), N(n), L(l), interval(iv), policy(pol), rng(seed), ticket((size_t)n, 0) {}

    const Cloud &cloud(int k) const { return scans[(size_t)k % scans.size()]; }
    const geometry_msgs::Pose &pose(int k) const { return odom[(size_t)k % odom.size()]; }
    void logline(const char *op, int node, bool tk, const char *extra) {
        int lib = -1;
        (void)erasor_hip_announced_count(up.handle(), &lib);
        if (lib != up.outstanding()) ++mismatches;
        fprintf(g_log, "%s node=%d ticket=%d out=%d lib=%d status=%s%s threw=0\n", op, node, tk ? 1 : 0, up.outstanding(), lib, status_name(up.last_announce()), extra);
    }
    uint64_t upcoming(int k) {
        op = "announce_upcoming", op_node = k;
        const uint64_t t = up.announce_upcoming(cloud(k), pose(k));
        ticket[(size_t)k] = t;
        logline("announce_upcoming", k, t != 0, "");
        return t;
    }
    uint64_t next(int k) {
        op = "announce_next", op_node = k;
        const uint64_t t = up.announce_next(cloud(k), pose(k));
        ticket[(size_t)k] = t;
        logline("announce_next", k, t != 0, "");
        return t;
    }
    void defer(int k) {
        op = "announce_next_deferred", op_node = k;
        def_copy.reset(new Cloud(cloud(k)));
        up.announce_next_deferred(k, *def_copy, pose(k));
        deferred = k;
        logline("announce_next_deferred", k, false, "");
    }
    // another_buffer: the cloud arrives in a buffer of its own (a message's), not in the one that was announced
    void callback(int k, bool hand_ticket, bool three_arguments, bool another_buffer = false) {
        op = "callback_node", op_node = k;
        const size_t by_ticket0 = up.stepped_by_ticket(), processed0 = up.num_processed;
        const uint64_t t = hand_ticket ? ticket[(size_t)k] : 0;
        std::unique_ptr<Cloud> copy(another_buffer ? new Cloud(cloud(k)) : nullptr);
        const Cloud &c = copy ? *copy : cloud(k);
        if (three_arguments) up.callback_node(k, pose(k), c);
        else up.callback_node(k, pose(k), c, t);
        copy.reset();
        const bool processed = up.num_processed != processed0;
        char extra[64];
        snprintf(extra, sizeof(extra), " byticket=%d processed=%d", (int)(up.stepped_by_ticket() - by_ticket0), processed ? 1 : 0);
        logline("callback_node", k, t != 0, extra);
        if (processed) {
            chunk(2, k, 0, nullptr, 0);
            chunk_cloud(3, up.map_rejected);
            chunk_cloud(4, up.query_rejected);
            chunk(5, 0, 0, &up.last, sizeof(up.last));
        }
        if (deferred >= 0) {  // what became of the hand-over: its cloud goes out of scope NOW (the updater must not look at it again)
            def_copy.reset();
            logline("deferred_result", deferred, up.last_announce() == Updater::ANNOUNCED, "");
            if (up.last_announce() != Updater::FULL) p = deferred + 1;  // (FULL: not taken, nothing moved: the node is handed over again)
            deferred = -1;
        }
    }
    // node i itself is next and still unannounced: announce_upcoming is the one call for it, and only with nothing announced
    void at_the_upcoming_node(int i) {
        if (p != i) return;
        if (up.outstanding() == 0) (void)upcoming(i);
        p = i + 1;
    }
    void window_round(int i) {
        if (p < i) p = i;
        at_the_upcoming_node(i);
        const int limit = std::min(i + L, N - 1);
        while (p <= limit) {
            if (p == limit) {
                defer(p);
                break;
            }
            if (!next(p) && up.last_announce() == Updater::FULL) break;
            ++p;
        }
    }
    void greedy_round(int i, bool hand_over) {
        if (p < i) p = i;
        at_the_upcoming_node(i);
        while (p < N) {
            if (!next(p) && up.outstanding() >= up.lookahead()) {  // erasor_shim.h: "call again before a later callback"
                if (hand_over) defer(p);
                break;
            }
            ++p;
        }
    }
    void random_round(int i) {
        if (p < i) p = i;
        for (int tries = 0; tries < 8 && p < N; ++tries) {
            const unsigned a = rng() % 3u;
            if (a == 2) break;
            if (p == i) {
                at_the_upcoming_node(i);
                continue;
            }
            if (a == 1) {
                defer(p);
                break;
            }
            if (!next(p) && up.last_announce() == Updater::FULL) break;
            ++p;
        }
    }
    void run() {
        for (int i = 0; i < N; ++i) {
            bool hand_ticket = true, three = false, another_buffer = false;
            if (policy == "window") window_round(i);
            else if (policy == "greedy") greedy_round(i, false);
            else if (policy == "greedy_deferred") greedy_round(i, true);
            else if (policy == "ticketless") { window_round(i); three = true; hand_ticket = false; }
            else if (policy == "stop_and_go") { if (i < N / 3 || i >= 2 * N / 3) window_round(i); }
            else {
                random_round(i);
                hand_ticket = rng() % 4u != 0;
                another_buffer = !hand_ticket && rng() % 2u != 0;
            }
            callback(i, hand_ticket, three, another_buffer);
        }
    }
};

static bool read_scan(const std::string &path, Cloud &c) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const size_t n = (size_t)f.tellg() / 16;
    f.seekg(0);
    std::vector<float> v(n * 4);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * 4));
    c.points.resize(n);
    for (size_t i = 0; i < n; ++i) {
        c.points[i].x = v[4 * i]; c.points[i].y = v[4 * i + 1]; c.points[i].z = v[4 * i + 2]; c.points[i].intensity = v[4 * i + 3];
    }
    c.width = (unsigned)n;
    return true;
}

int main(int argc, char **argv) {
    if (argc < 8) return 2;
    const std::string dir = argv[1], out = argv[2], policy = argv[6];
    const int n_scans = atoi(argv[3]), interval = atoi(argv[4]);
    std::vector<int> lookaheads;
    for (const char *s = argv[5]; *s;) {
        lookaheads.push_back(atoi(s));
        while (*s && *s != ',') ++s;
        if (*s) ++s;
    }
    unsigned seed0 = 0;
    int n_seeds = 1;
    if (sscanf(argv[7], "%u:%d", &seed0, &n_seeds) < 1) return 2;
    std::vector<Cloud> scans((size_t)n_scans);
    std::vector<geometry_msgs::Pose> odom((size_t)n_scans);
    std::ifstream poses(dir + "/poses.txt");
    for (int k = 0; k < n_scans; ++k) {
        if (!read_scan(dir + "/scan" + std::to_string(k) + ".bin", scans[(size_t)k])) return 3;
        double v[7];
        for (double &x : v)
            if (!(poses >> x)) return 3;
        odom[(size_t)k].position.x = v[0]; odom[(size_t)k].position.y = v[1]; odom[(size_t)k].position.z = v[2];
        odom[(size_t)k].orientation.x = v[3]; odom[(size_t)k].orientation.y = v[4]; odom[(size_t)k].orientation.z = v[5]; odom[(size_t)k].orientation.w = v[6];
    }
    g_log = fopen((out + "log.txt").c_str(), "w");
    g_res = fopen((out + "res.bin").c_str(), "wb");
    if (!g_log || !g_res) return 3;
    Updater::Config cfg;
    erasor_hip_params_default(&cfg.params);
    // config/seq_05.yaml, as erasor_offline_demo's plain mode sets it
    cfg.params.max_range = 60.0; cfg.params.num_rings = 15; cfg.params.num_sectors = 60; cfg.params.min_h = -1.3; cfg.params.max_h = 3.2;
    cfg.params.th_bin_max_h = 0.05; cfg.params.scan_ratio_threshold = 0.3; cfg.params.minimum_num_pts = 10; cfg.params.gf_dist_thr = 0.15;
    cfg.params.gf_iter = 3; cfg.params.gf_num_lpr = 10; cfg.params.gf_th_seeds_height = 0.5; cfg.params.query_voxel_size = 0.2;
    cfg.params.version = 3;
    cfg.params.removal_interval = interval;
    cfg.lidar2body[2] = 1.73;
    cfg.initial_map_path = dir + "/map.pcd";
    int failed = 0;
    for (int s = 0; s < n_seeds; ++s)
        for (int L : lookaheads) {
            const unsigned seed = seed0 + (unsigned)s;
            const int N = 3 * interval + L + 3;
            fprintf(g_log, "script lookahead=%d seed=%u nodes=%d\n", L, seed, N);
            chunk(1, L, (int)seed, nullptr, 0);
            std::vector<float> T((size_t)n_scans * 32);
            for (int k = 0; k < n_scans; ++k) {
                const Eigen::Matrix4f Tb = erasor_utils::geoPose2eigen(odom[(size_t)k]), To = erasor_utils::inverse(Tb);
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) {
                        T[(size_t)k * 32 + (size_t)(r * 4 + c)] = Tb(r, c);
                        T[(size_t)k * 32 + 16 + (size_t)(r * 4 + c)] = To(r, c);
                    }
            }
            chunk(8, n_scans, 0, T.data(), T.size() * sizeof(float));
            int threw = 0, mismatches = 0;
            try {
                Updater up(cfg);
                up.set_lookahead(L);
                Script sc(up, scans, odom, N, L, interval, policy, seed * 7919u + (unsigned)L);
                try {
                    sc.run();
                    Cloud m;
                    up.get_map(m);
                    chunk_cloud(6, m);
                } catch (const std::exception &e) {
                    threw = 1;
                    fprintf(stderr, "lookahead %d seed %u: %s\n", L, seed, e.what());
                    fprintf(g_log, "%s node=%d threw=1\n", sc.op, sc.op_node);
                }
                mismatches = sc.mismatches;
                fprintf(g_log, "end stepped_by_ticket=%zu dropped=%zu processed=%zu threw=%d\n", up.stepped_by_ticket(), up.announcements_dropped(),
                        up.num_processed, threw);
            } catch (const std::exception &e) {
                threw = 1;
                fprintf(stderr, "lookahead %d seed %u: %s\n", L, seed, e.what());
                fprintf(g_log, "end threw=1\n");
            }
            chunk(7, threw, mismatches, nullptr, 0);
            failed += threw;
        }
    fclose(g_log);
    fclose(g_res);
    printf("scripts failed: %d\n", failed);
    return 0;
}
