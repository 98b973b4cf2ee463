// fake_erasor_hip.cpp — a recording stand-in for the part of liberasor_hip.so's C ABI that erasor::OfflineMapUpdater drives.
// TEST INFRASTRUCTURE: built into a liberasor_hip.so in a test's temporary directory (or linked into the driver), never installed.
//
// No GPU, no ERASOR: what it implements is the ANNOUNCEMENT CONTRACT of erasor_hip.hip (prefetch_common, flush_announced, step_admit,
// q_drain, erasor_hip_announce_origin2body), restated from that file:
//   * the newest announcement waits in `ann` until the next announcement or the next step moves it behind the older ones in `pend`
//     (at most 7 there); an announcement made while a step is in flight goes to `pend` at once, and is refused when all 7 are taken;
//   * a step by ticket takes the OLDEST announcement and nothing else (ERASOR_E_STATE otherwise); a still unstarted `ann` with that
//     ticket is started first;
//   * a step without a ticket compares its cloud (pointer, size, T_lidar2body, record layout, then every record) with the oldest
//     announcement: the same cloud consumes it; any other cloud drops everything -- except that with nothing in `pend` an unstarted `ann`
//     that is another cloud stays (it is the NEXT scan).  An unstarted `ann` that IS the cloud is started and then -- step_admit takes the
//     fingerprint of `pend` only when `pend` was not empty before -- dropped like a foreign one: the step runs on the caller's buffer;
//   * every step ends with `ann` moved to `pend`; erasor_hip_drop_announced and erasor_hip_voxelize_preserving_labels drop everything;
//   * one step in flight at most: erasor_hip_step_ticket_async .. erasor_hip_step_wait.
// tests/test_gpu_shim_lookahead.py pins this to the real library: every scripted caller must leave the same call log on both.
//
// A "step" here records WHICH staged cloud ran with WHICH two transforms: map_rejected is the cloud's first 8 records, query_rejected
// the 16 + 16 floats of T_body2origin and T_origin2body as 8 records, and the map grows by one record per step (the cloud's first).
// Entry points outside the updater's path return ERASOR_E_UNSUPPORTED.
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/erasor_hip.h"

namespace {
constexpr int kMaxAhead = 7;  // erasor_hip.hip: MAX_AHEAD = NSIDE - 1
struct Announced {
    uint64_t ticket = 0;
    const void *src = nullptr;
    size_t n = 0, stride = 0, ioff = 0;
    float Tl[16] = {0};
    std::vector<float> rows;  // the staged copy, XYZI
    bool pose_valid = false, to_valid = false;
};
std::vector<float> repack(const void *rows, size_t n, size_t stride, size_t ioff) {
    std::vector<float> v(n * 4);
    const char *p = static_cast<const char *>(rows);
    for (size_t i = 0; i < n; ++i) {
        memcpy(&v[4 * i], p + i * stride, 12);
        memcpy(&v[4 * i + 3], p + i * stride + ioff, 4);
    }
    return v;
}
bool bad_fmt(size_t stride, size_t ioff) { return stride < 16 || ioff < 12 || ioff + 4 > stride || stride > 0xFFFFFFFFull || ioff > 0xFFFFFFFFull; }
}  // namespace

struct erasor_hip_handle {
    erasor_params P;
    std::string err;
    std::vector<float> map;
    bool have_map = false, fly = false;
    Announced ann;
    bool ann_valid = false;
    std::deque<Announced> pend;
    uint64_t next_ticket = 1, last_ticket = 0;
    erasor_step_result res;
    std::vector<float> map_rejected, curr_rejected;

    void flush() {
        if (!ann_valid) return;
        ann_valid = false;
        pend.push_back(ann);
    }
    void drain() {
        pend.clear();
        ann_valid = false;
    }
    bool same_scan(const Announced &a, const void *src, size_t n, const float *Tl, size_t stride, size_t ioff) const {
        return a.src == src && a.n == n && memcmp(a.Tl, Tl, sizeof(a.Tl)) == 0 && a.stride == stride && a.ioff == ioff;
    }
    void run(const std::vector<float> &rows, const float Tb[16], const float To[16]) {
        const size_t n = rows.size() / 4, k = n < 8 ? n : 8;
        memset(&res, 0, sizeof(res));
        res.n_map_in = map.size() / 4;
        res.n_voi = res.n_query = n;
        map_rejected.assign(rows.begin(), rows.begin() + (long)(4 * k));
        curr_rejected.assign(Tb, Tb + 16);
        curr_rejected.insert(curr_rejected.end(), To, To + 16);
        if (n) map.insert(map.end(), rows.begin(), rows.begin() + 4);
        res.n_map_rejected = k;
        res.n_curr_rejected = 8;
        res.n_map_out = map.size() / 4;
        flush();  // (step_end_and_ahead: the next scan's chain goes into its queue behind this step)
    }
};

extern "C" {
int erasor_hip_params_default(erasor_params *p) {
    if (!p) return ERASOR_E_INVALID;
    memset(p, 0, sizeof(*p));
    p->version = 3;
    p->removal_interval = 1;
    return ERASOR_OK;
}
int erasor_hip_create(const erasor_params *p, int, erasor_hip_handle **out) {
    if (!p || !out) return ERASOR_E_INVALID;
    *out = new erasor_hip_handle();
    (*out)->P = *p;
    memset(&(*out)->res, 0, sizeof((*out)->res));
    return ERASOR_OK;
}
void erasor_hip_destroy(erasor_hip_handle *h) { delete h; }
const char *erasor_hip_last_error(const erasor_hip_handle *h) { return h ? h->err.c_str() : ""; }
int erasor_hip_set_map(erasor_hip_handle *h, const float *xyzi, size_t n) {
    if (!h || (!xyzi && n)) return ERASOR_E_INVALID;
    if (h->fly) return ERASOR_E_STATE;
    h->map.assign(xyzi, xyzi + 4 * n);
    h->have_map = true;
    h->drain();
    return ERASOR_OK;
}
int erasor_hip_map_size(erasor_hip_handle *h, size_t *n) {
    if (!h || !n) return ERASOR_E_INVALID;
    *n = h->map.size() / 4;
    return ERASOR_OK;
}
int erasor_hip_get_map(erasor_hip_handle *h, float *dst, size_t cap, size_t *n) {
    if (!h || !n) return ERASOR_E_INVALID;
    *n = h->map.size() / 4;
    if (dst && cap >= *n && *n) memcpy(dst, h->map.data(), h->map.size() * sizeof(float));
    return ERASOR_OK;
}
int erasor_hip_get_cloud(erasor_hip_handle *h, int which, float *dst, size_t cap, size_t *n) {
    if (!h || !n) return ERASOR_E_INVALID;
    const std::vector<float> *c = which == ERASOR_CLOUD_MAP_REJECTED ? &h->map_rejected : which == ERASOR_CLOUD_CURR_REJECTED ? &h->curr_rejected : nullptr;
    if (!c) return ERASOR_E_UNSUPPORTED;
    *n = c->size() / 4;
    if (dst && cap >= *n && *n) memcpy(dst, c->data(), c->size() * sizeof(float));
    return ERASOR_OK;
}

int erasor_hip_prefetch_node_rows(erasor_hip_handle *h, const void *rows, size_t n, size_t stride, size_t ioff, const float Tl[16], const float *Tb,
                                  uint64_t *ticket) {
    if (!h || !Tl || (!rows && n) || n > 0x3FFFFFFFull || bad_fmt(stride, ioff)) return ERASOR_E_INVALID;
    if (h->ann_valid && (int)h->pend.size() >= kMaxAhead) {
        h->err = "as many scans as there are query sides to hold them are already announced";
        return ERASOR_E_STATE;
    }
    h->flush();
    if (h->fly && (int)h->pend.size() >= kMaxAhead) {  // (pick_side: the one side left is the side of the step in flight)
        h->err = "all query sides are taken while a step is in flight";
        return ERASOR_E_STATE;
    }
    h->ann = Announced();
    h->ann.ticket = h->next_ticket++;
    h->ann.src = rows;
    h->ann.n = n;
    h->ann.stride = stride;
    h->ann.ioff = ioff;
    memcpy(h->ann.Tl, Tl, sizeof(h->ann.Tl));
    h->ann.rows = repack(rows, n, stride, ioff);  // (a host scan is taken over at once)
    h->ann.pose_valid = Tb != nullptr;
    h->ann_valid = true;
    h->last_ticket = h->ann.ticket;
    if (ticket) *ticket = h->ann.ticket;
    if (h->fly) h->flush();  // (announced beside a step in flight: its chain starts now)
    return ERASOR_OK;
}
int erasor_hip_announce_origin2body(erasor_hip_handle *h, const float To[16]) {
    if (!h || !To) return ERASOR_E_INVALID;
    if (h->ann_valid && h->ann.pose_valid) {
        h->ann.to_valid = true;
        return ERASOR_OK;
    }
    for (auto &a : h->pend)
        if (a.ticket == h->last_ticket && a.pose_valid) {
            a.to_valid = true;
            return ERASOR_OK;
        }
    h->err = "no node announced with its pose to attach the transform to";
    return ERASOR_E_STATE;
}
static int admit(erasor_hip_handle *h, const float *Tb, const float *To) {
    if (!h) return ERASOR_E_INVALID;
    if (h->fly) {
        h->err = "the previous step has not been collected";
        return ERASOR_E_STATE;
    }
    if (!h->have_map) {
        h->err = "step before erasor_hip_set_map";
        return ERASOR_E_STATE;
    }
    return (!Tb || !To) ? ERASOR_E_INVALID : ERASOR_OK;
}
int erasor_hip_step_ticket_async(erasor_hip_handle *h, uint64_t ticket, const float Tb[16], const float To[16]) {
    if (!ticket) return ERASOR_E_INVALID;
    const int rc = admit(h, Tb, To);
    if (rc) return rc;
    if (h->pend.empty() && h->ann_valid && h->ann.ticket == ticket) h->flush();
    if (h->pend.empty() || h->pend.front().ticket != ticket) {
        h->err = "not the ticket of the oldest announced scan (announcements are consumed in order)";
        return ERASOR_E_STATE;
    }
    const Announced a = h->pend.front();
    h->pend.pop_front();
    h->run(a.rows, Tb, To);
    h->fly = true;
    return ERASOR_OK;
}
int erasor_hip_step_wait(erasor_hip_handle *h, erasor_step_result *res) {
    if (!h) return ERASOR_E_INVALID;
    if (!h->fly) {
        h->err = "erasor_hip_step_wait without a step in flight";
        return ERASOR_E_STATE;
    }
    h->fly = false;
    if (res) *res = h->res;
    return ERASOR_OK;
}
int erasor_hip_step_rows(erasor_hip_handle *h, const void *rows, size_t n, size_t stride, size_t ioff, const float Tl[16], const float Tb[16],
                         const float To[16], erasor_step_result *res) {
    if (!h) return ERASOR_E_INVALID;
    if (h->fly || !h->have_map) return admit(h, Tb, To);
    if (!Tl || (!rows && n) || n > 0x3FFFFFFFull || !Tb || !To || bad_fmt(stride, ioff)) return ERASOR_E_INVALID;
    const std::vector<float> mine = repack(rows, n, stride, ioff);
    const bool ann_cand = h->pend.empty() && h->ann_valid && h->same_scan(h->ann, rows, n, Tl, stride, ioff);
    const bool pend_cand = !h->pend.empty() && h->same_scan(h->pend.front(), rows, n, Tl, stride, ioff);
    if (ann_cand && h->ann.rows == mine) h->flush();
    bool took = false;
    if (!h->pend.empty()) {
        if (pend_cand && h->pend.front().rows == mine) {
            h->pend.pop_front();
            took = true;
        } else {
            h->drain();
        }
    }
    (void)took;  // (the staged copy holds the same records: the step computes the same either way)
    h->run(mine, Tb, To);
    if (res) *res = h->res;
    return ERASOR_OK;
}
int erasor_hip_drop_announced(erasor_hip_handle *h) {
    if (!h) return ERASOR_E_INVALID;
    if (h->fly) return ERASOR_E_STATE;
    h->drain();
    return ERASOR_OK;
}
int erasor_hip_announced_count(const erasor_hip_handle *h, int *n) {
    if (!h || !n) return ERASOR_E_INVALID;
    *n = (int)h->pend.size() + (h->ann_valid ? 1 : 0);
    return ERASOR_OK;
}

// ---- outside the updater's path
int erasor_hip_voxelize_preserving_labels(erasor_hip_handle *, const float *, size_t, double, float *, size_t, size_t *) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_erasor_run(erasor_hip_handle *, const float *, size_t, const float *, size_t, erasor_step_result *) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_get_status(erasor_hip_handle *, double *) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_get_rpod(erasor_hip_handle *, int, float *, size_t, size_t *, uint32_t *, uint32_t *) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_mapgen_begin(erasor_hip_handle *, double, int) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_mapgen_accum(erasor_hip_handle *, const float *, size_t, const float *, const float *, size_t *) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_mapgen_get(erasor_hip_handle *, int, float *, size_t, size_t *) { return ERASOR_E_UNSUPPORTED; }
int erasor_hip_mapgen_save(erasor_hip_handle *, float *, size_t, size_t *) { return ERASOR_E_UNSUPPORTED; }
}
