// Where does the early stream of overlapped steps land?  The decision, as plain C++: no handle, no device call -- the handle feeds it
// the compute pipe every stream was seen on (erasor_hip.hip: place_rehearsal, k_stream_pipe) and does what it answers; the stand-alone
// check (tests/cpp/stream_place_check.cpp) feeds it pipe sequences.
//
// A process with few hardware queues (GPU_MAX_HW_QUEUES = 4: main, two query streams, and the framework's own) gets its FOURTH stream on
// a queue another stream already has, and the runtime picks the least-used one.  Where that is a query stream's queue, a set of ~40 chain
// launches sits in front of the next step's early passes every fourth step (MEASUREMENTS, "Stream placement").  The rehearsal at handle
// creation creates candidate streams one at a time: a candidate on a pipe main / q0 / q1 already have stays alive as an idle PAD -- it
// keeps that queue's use count up --; the first candidate on a free pipe holds the place and is destroyed right in front of the early
// stream's creation, which lands where it was.  SP_TRIES candidates at most; if none is free, every pad goes and the handle is what it
// was without a rehearsal.
//
// A pipe is me * 4 + pipe (0 .. 15), -1: unknown (no such register: the CPU stand-in; a failed probe).  Unknown never counts as free.
#pragma once

static constexpr int SP_TRIES = 4;      // candidates at most
static constexpr int SP_FIXED = 3;      // main, q0, q1

enum SpAction {
    SP_PAD = 0,      // the candidate shares a pipe with main / q0 / q1 (or its pipe is unknown): keep it alive, idle; try another
    SP_FREE = 1,     // a free pipe: this candidate holds the place; destroyed, the next stream created lands there.  Done.
    SP_GIVE_UP = 2,  // SP_TRIES candidates and none free: destroy all of them, pads included.  Done.
};

struct StreamPlace {
    int fixed[SP_FIXED] = {-1, -1, -1};  // main, q0, q1
    int early = -1;                      // the early stream, once it exists and was probed
    int tries = 0;                       // candidates seen
    int n_pads = 0;                      // pads alive
    int free_at = -1;                    // the candidate (0-based) that found a free pipe, -1: none
    int cand[SP_TRIES] = {-1, -1, -1, -1};  // where each candidate was seen (ERASOR_HIP_PLACEMENT_LOG prints them)
    bool done = false;
    unsigned seen_mask = 0;              // pipes seen in all: main, q0, q1 and every candidate
};

static inline int sp_pipe(unsigned me, unsigned pipe) { return (int)((me & 3u) * 4u + (pipe & 3u)); }
// HW_ID -> me * 4 + pipe (fields as in tools/queue_probe.hip: pipe [7:6], me [31:30])
static inline int sp_pipe_of_hw_id(unsigned id) { return id == 0xFFFFFFFFu ? -1 : sp_pipe(id >> 30, (id >> 6) & 3u); }

static inline bool sp_taken(const StreamPlace &s, int pipe) {
    for (int k = 0; k < SP_FIXED; ++k)
        if (s.fixed[k] == pipe) return true;
    return false;
}
static inline int sp_distinct_seen(const StreamPlace &s) {
    int n = 0;
    for (unsigned m = s.seen_mask; m; m &= m - 1) ++n;
    return n;
}
// the three streams every step uses; false: one of them is unknown -- no rehearsal, nothing is steered
static inline bool sp_begin(StreamPlace &s, int main_pipe, int q0_pipe, int q1_pipe) {
    s = StreamPlace();
    s.fixed[0] = main_pipe;
    s.fixed[1] = q0_pipe;
    s.fixed[2] = q1_pipe;
    for (int k = 0; k < SP_FIXED; ++k) {
        if (s.fixed[k] < 0 || s.fixed[k] > 15) {
            s.done = true;
            return false;
        }
        s.seen_mask |= 1u << s.fixed[k];
    }
    return true;
}
// one more candidate stream was created and seen on `pipe`: what to do with it
static inline SpAction sp_candidate(StreamPlace &s, int pipe) {
    if (s.done) return SP_GIVE_UP;
    const int idx = s.tries++;
    if (idx < SP_TRIES) s.cand[idx] = pipe;
    if (pipe >= 0 && pipe <= 15) {
        s.seen_mask |= 1u << pipe;
        if (!sp_taken(s, pipe)) {
            s.free_at = idx;
            s.done = true;
            return SP_FREE;
        }
    }
    if (s.tries >= SP_TRIES) {
        s.n_pads = 0;
        s.done = true;
        return SP_GIVE_UP;
    }
    ++s.n_pads;
    return SP_PAD;
}
// the early stream exists and was seen on `pipe`: does it share a pipe with main / q0 / q1?  (unknown: not known to)
static inline bool sp_early(StreamPlace &s, int pipe) {
    s.early = pipe >= 0 && pipe <= 15 ? pipe : -1;
    return s.early >= 0 && sp_taken(s, s.early);
}
