// ERASOR_HIP_OVERLAP unset: does overlapping consecutive steps pay on this handle's workload?  The decision, as plain C++: no handle, no
// device call -- the handle feeds it one period per consecutive deep step (erasor_hip.hip, step_collect) and reads `mode` back; the
// stand-alone check (tests/cpp/overlap_auto_check.cpp) feeds it synthetic periods.
//
// The period of a step -- end to end on the device's own clock -- is sampled in blocks of OVA_W samples: plain, overlapped, overlapped,
// plain.  A sequence drifts (its first steps revert more bins), and this order cancels a linear drift.  The first OVA_SKIP samples after
// a change of mode are not counted (OVA_START_SKIP at a handle's start).  (The per-step record shows ONE slow step after a change on
// three workloads, but on large_scale_05 the first five overlapped steps run at 515-550 us and the next at 305-390: with a skip of one
// and two the handle chose against the forced A/B on two of four workloads, MEASUREMENTS.md "cold start"; left at 3 and 4.)  A mode's mean leaves
// out its ONE largest sample: a page fault in one of a few steps is not the mode's doing.  (One per mode, not one per block: every
// second to fourth overlapped step is late by 100-350 us, EXPERIMENTS cs-3, and that IS the mode's doing -- a rule that dropped one
// sample of every block of four never saw those steps and chose the overlap where the forced A/B says plain.)
//
// EARLY EXIT: a handle's first 25 steps used to lie wholly inside the four blocks (the reference's own schedule is ~20 steps per
// sequence).  When the first overlapped block is through and the two means differ by more than OVA_MARGIN, the decision is taken there:
// overlapped stays on without a further change of mode, or plain comes back for good.  OVA_MARGIN has to exceed what the drift alone
// puts between two neighbouring blocks of the SAME mode (MEASUREMENTS.md, "cold start": twice the largest such difference measured).
// Inside the margin the four blocks run as before and the mode with the shorter mean runs on (plain has to lose by 2 %).
// Measured again, by the same rules, every OVA_AGAIN steps.  Results never depend on the mode.
#pragma once
#include <algorithm>

static constexpr int OVA_W = 4, OVA_SKIP = 3, OVA_START_SKIP = 4;
static constexpr unsigned long long OVA_AGAIN = 600;
static constexpr double OVA_MARGIN = 0.50;      // relative difference of the two means beyond which the first two blocks decide
static constexpr double OVA_PLAIN_LOSES = 1.02;  // the full schedule: plain has to lose by 2 %

struct OvAuto {
    int mode = 0;            // 1: overlapped, 0: plain -- what the next step uses
    int block = 0;           // 0..3: the block being sampled (modes 0 1 1 0); 4: decided
    int skip = OVA_START_SKIP;  // samples still to be ignored (start-up, a change of mode)
    int n = 0;               // samples of the current block
    double sum[2] = {0, 0};
    double mx[2] = {0, 0};   // the largest sample of each mode: left out of its mean (one hiccup in eight samples must not decide 600 steps)
    int cnt[2] = {0, 0};
    double est[2] = {0, 0};  // the last decision's mean periods (0: not measured)
    unsigned long long since_decision = 0;
    bool early = false;      // the last decision was taken after the first overlapped block
};

static inline int ova_block_mode(int block) { return block == 1 || block == 2 ? 1 : 0; }

static inline double ova_mean(const OvAuto &a, int m) {
    return a.cnt[m] > 1 ? (a.sum[m] - a.mx[m]) / (a.cnt[m] - 1) : (a.cnt[m] ? a.sum[m] / a.cnt[m] : 0.0);
}

static inline void ova_decide(OvAuto &a, int m, bool early) {
    a.est[0] = ova_mean(a, 0);
    a.est[1] = ova_mean(a, 1);
    if (m != a.mode) a.skip = OVA_SKIP;
    a.mode = m;
    a.block = 4;
    a.n = 0;
    a.since_decision = 0;
    a.early = early;
}

// one period (microseconds) of a consecutive deep step that ran in a.mode
static inline void overlap_auto_sample(OvAuto &a, double period_us) {
    if (a.block >= 4) {  // decided: measure again after a while
        if (++a.since_decision >= OVA_AGAIN) {
            a.block = 0;
            a.n = 0;
            a.sum[0] = a.sum[1] = 0;
            a.mx[0] = a.mx[1] = 0;
            a.cnt[0] = a.cnt[1] = 0;
            if (a.mode != ova_block_mode(0)) {
                a.mode = ova_block_mode(0);
                a.skip = OVA_SKIP;
            }
        }
        return;
    }
    if (a.skip > 0) {
        --a.skip;
        return;
    }
    a.sum[a.mode] += period_us;
    a.mx[a.mode] = std::max(a.mx[a.mode], period_us);
    ++a.cnt[a.mode];
    if (++a.n < OVA_W) return;
    a.n = 0;
    ++a.block;
    if (a.block == 2) {  // one block of either mode: decide now if they are clearly apart
        const double p = ova_mean(a, 0), o = ova_mean(a, 1);
        if (o < p * (1.0 - OVA_MARGIN)) return ova_decide(a, 1, true);
        if (o > p * (1.0 + OVA_MARGIN)) return ova_decide(a, 0, true);
    }
    if (a.block < 4) {
        if (ova_block_mode(a.block) != a.mode) {
            a.mode = ova_block_mode(a.block);
            a.skip = OVA_SKIP;
        }
        return;
    }
    ova_decide(a, ova_mean(a, 1) * OVA_PLAIN_LOSES < ova_mean(a, 0) ? 1 : 0, false);
}
