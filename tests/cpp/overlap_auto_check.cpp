// The overlap decision (erasor_amd/csrc/overlap_auto.h) fed with synthetic step periods: a stand-alone program, no device, no handle.
// Every scenario steps the way a handle does: the period of a step depends on the mode the decision had in force for it.
#include "../../erasor_amd/csrc/overlap_auto.h"

#include <cstdio>
#include <functional>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);           \
            ++g_fail;                                                     \
        }                                                                 \
    } while (0)

struct Run {
    OvAuto a;
    std::string modes;       // the mode every fed sample ran in
    int decided_at = -1;     // samples fed when block first reached 4
    int first_plain_after_decision = -1;
    // period(mode, k): the k-th sample's period in `mode`
    void feed(int n, const std::function<double(int, int)> &period) {
        for (int k = 0; k < n; ++k) {
            const int m = a.mode;
            modes.push_back(m ? 'O' : 'P');
            const bool was_decided = a.block >= 4;
            overlap_auto_sample(a, period(m, (int)modes.size() - 1));
            if (!was_decided && a.block >= 4 && decided_at < 0) decided_at = (int)modes.size();
            if (decided_at >= 0 && (int)modes.size() > decided_at && m == 0 && first_plain_after_decision < 0)
                first_plain_after_decision = (int)modes.size() - 1;
        }
    }
};

// samples a fresh handle needs up to the end of the first overlapped block / of the whole schedule
static const int N_EARLY = OVA_START_SKIP + OVA_W + OVA_SKIP + OVA_W;
static const int N_FULL = N_EARLY + OVA_W + OVA_SKIP + OVA_W;

int main() {
    // "clearly apart" below: plain 192 us against overlapped 64 or 320 us -- outside the margin, whatever it is set to
    CHECK(64.0 < 192.0 * (1.0 - OVA_MARGIN) && 320.0 > 192.0 * (1.0 + OVA_MARGIN) && OVA_MARGIN > 0.04);
    {   // overlapped clearly faster: decided right after the first overlapped block, overlapped from then on, both estimates there
        Run r;
        r.feed(60, [](int m, int) { return m ? 64.0 : 192.0; });
        CHECK(r.decided_at == N_EARLY);
        CHECK(r.a.mode == 1 && r.a.early);
        CHECK(r.first_plain_after_decision < 0);
        CHECK(r.a.est[0] == 192.0 && r.a.est[1] == 64.0);
        CHECK(r.modes.substr(0, N_EARLY) == std::string(OVA_START_SKIP + OVA_W, 'P') + std::string(OVA_SKIP + OVA_W, 'O'));
        CHECK(r.modes.find('P', N_EARLY) == std::string::npos);
    }
    {   // plain clearly faster: decided plain at the same point, plain from then on
        Run r;
        r.feed(60, [](int m, int) { return m ? 320.0 : 192.0; });
        CHECK(r.decided_at == N_EARLY);
        CHECK(r.a.mode == 0 && r.a.early);
        CHECK(r.a.est[0] == 192.0 && r.a.est[1] == 320.0);
        CHECK(r.modes.find('O', N_EARLY) == std::string::npos);
    }
    {   // a difference inside the margin: the full four blocks, then the 2 % rule -- either way
        const double inside = 1.0 - 0.5 * OVA_MARGIN;  // overlapped faster by half the margin: more than 2 %
        Run r;
        r.feed(60, [&](int m, int) { return m ? 200.0 * inside : 200.0; });
        CHECK(r.decided_at == N_FULL);
        CHECK(r.a.mode == 1 && !r.a.early);
        CHECK(r.a.cnt[0] == 2 * OVA_W && r.a.cnt[1] == 2 * OVA_W);
        CHECK(r.modes.substr(0, N_FULL) == std::string(OVA_START_SKIP + OVA_W, 'P') + std::string(OVA_SKIP + 2 * OVA_W, 'O') + std::string(OVA_SKIP + OVA_W, 'P'));
        Run q;  // overlapped faster by 1 %: not enough, plain runs on
        q.feed(60, [](int m, int) { return m ? 198.0 : 200.0; });
        CHECK(q.decided_at == N_FULL && q.a.mode == 0 && !q.a.early);
        CHECK(q.a.est[0] == 200.0 && q.a.est[1] == 198.0);
    }
    {   // equal modes under a linear drift that puts half the margin between neighbouring blocks (the margin is twice the largest drift
        // measured): no early exit, the order plain, overlapped, overlapped, plain cancels the drift, plain is kept
        const double per_sample = 200.0 * (0.5 * OVA_MARGIN) / (OVA_W + OVA_SKIP);  // blocks start OVA_W + OVA_SKIP samples apart
        Run r;
        r.feed(60, [&](int, int k) { return 200.0 - per_sample * std::min(k, N_FULL); });
        CHECK(r.decided_at == N_FULL);
        CHECK(!r.a.early && r.a.mode == 0);
        CHECK(r.a.est[1] * OVA_PLAIN_LOSES >= r.a.est[0]);
        Run u;  // ... and the same drift upwards
        u.feed(60, [&](int, int k) { return 200.0 + per_sample * std::min(k, N_FULL); });
        CHECK(u.decided_at == N_FULL && !u.a.early && u.a.mode == 0);
    }
    {   // one sample ten times the others, in any position up to the end of the first overlapped block: the decision is what it is without it
        for (int bad = OVA_START_SKIP; bad < N_EARLY; ++bad) {
            Run r;
            r.feed(60, [&](int m, int k) { return (k == bad ? 10.0 : 1.0) * (m ? 64.0 : 192.0); });
            CHECK(r.decided_at == N_EARLY && r.a.mode == 1 && r.first_plain_after_decision < 0);
            Run q;
            q.feed(60, [&](int m, int k) { return (k == bad ? 10.0 : 1.0) * (m ? 320.0 : 192.0); });
            CHECK(q.decided_at == N_EARLY && q.a.mode == 0);
            Run e;  // (inside the margin: the full schedule with or without the hiccup)
            e.feed(60, [&](int m, int k) { return (k == bad ? 10.0 : 1.0) * (m ? 198.0 : 200.0); });
            CHECK(e.decided_at == N_FULL && e.a.mode == 0);
        }
    }
    {   // OVA_AGAIN samples later: measuring starts again, by the same rules, and can reverse the choice
        Run r;
        r.feed(N_EARLY, [](int m, int) { return m ? 64.0 : 192.0; });
        CHECK(r.a.block == 4 && r.a.mode == 1);
        r.feed((int)OVA_AGAIN - 1, [](int m, int) { return m ? 64.0 : 192.0; });
        CHECK(r.a.block == 4 && r.a.mode == 1 && r.modes.find('P', N_EARLY) == std::string::npos);
        r.decided_at = -1;
        const int before = (int)r.modes.size();
        r.feed(1, [](int, int) { return 64.0; });  // the OVA_AGAIN-th sample: back to the first block, plain, with its skip
        CHECK(r.a.block == 0 && r.a.mode == 0 && r.a.skip == OVA_SKIP && r.a.cnt[0] == 0 && r.a.cnt[1] == 0);
        r.feed(60, [](int m, int) { return m ? 320.0 : 192.0; });  // the workload has changed: plain is faster now
        CHECK(r.decided_at == before + 1 + OVA_SKIP + OVA_W + OVA_SKIP + OVA_W);
        CHECK(r.a.mode == 0 && r.a.early && r.a.est[0] == 192.0 && r.a.est[1] == 320.0);
    }
    {   // samples while skip > 0 are not counted: absurd periods there change nothing
        Run r;
        r.feed(60, [](int m, int k) {
            const bool skipped = k < OVA_START_SKIP || (k >= OVA_START_SKIP + OVA_W && k < OVA_START_SKIP + OVA_W + OVA_SKIP);
            return skipped ? 1.0e6 : (m ? 64.0 : 192.0);
        });
        CHECK(r.decided_at == N_EARLY && r.a.mode == 1);
        CHECK(r.a.est[0] == 192.0 && r.a.est[1] == 64.0);
        OvAuto a;
        for (int k = 0; k < OVA_START_SKIP; ++k) {
            overlap_auto_sample(a, 123.0);
            CHECK(a.cnt[0] == 0 && a.cnt[1] == 0 && a.sum[0] == 0 && a.n == 0 && a.block == 0);
        }
        overlap_auto_sample(a, 123.0);
        CHECK(a.cnt[0] == 1 && a.sum[0] == 123.0);
    }
    printf(g_fail ? "%d CHECKS FAILED\n" : "OVERLAP-AUTO OK\n", g_fail);
    return g_fail ? 1 : 0;
}
