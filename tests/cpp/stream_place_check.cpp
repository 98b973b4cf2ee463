// stream_place.h (the placement rule of the early stream: plain C++, no device) against pipe sequences.  Stand-alone: own main.
#include <cstdio>
#include <vector>

#include "../../erasor_amd/csrc/stream_place.h"

static int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
            ++g_fail;                                                   \
        }                                                               \
    } while (0)

struct Outcome {
    std::vector<SpAction> acts;
    StreamPlace s;
};
// what the handle does: candidates one at a time until the rule says anything but "pad"
static Outcome rehearse(int pm, int p0, int p1, const std::vector<int> &cands) {
    Outcome o;
    if (!sp_begin(o.s, pm, p0, p1)) return o;
    for (int p : cands) {
        o.acts.push_back(sp_candidate(o.s, p));
        if (o.acts.back() != SP_PAD) break;
    }
    return o;
}
static int P(int pipe) { return sp_pipe(1, (unsigned)pipe); }  // (compute queues: me 1)

int main() {
    // HW_ID fields: me [31:30], pipe [7:6]
    CHECK(sp_pipe_of_hw_id((1u << 30) | (2u << 6) | (2u << 24) | 5u) == 6);
    CHECK(sp_pipe_of_hw_id((2u << 30) | (3u << 6)) == 11);
    CHECK(sp_pipe_of_hw_id(0xFFFFFFFFu) == -1);
    CHECK(sp_pipe(1, 0) == 4 && sp_pipe(0, 3) == 3);

    {  // the order of a bare process with four queues (the committed probe): 2, 1, 0, then 0, 1, 2, 3
        Outcome o = rehearse(P(2), P(1), P(0), {P(0), P(1), P(2), P(3)});
        CHECK(o.acts.size() == 4);
        CHECK(o.acts[0] == SP_PAD && o.acts[1] == SP_PAD && o.acts[2] == SP_PAD && o.acts[3] == SP_FREE);
        CHECK(o.s.n_pads == 3 && o.s.free_at == 3 && o.s.done && o.s.tries == 4);
        CHECK(sp_distinct_seen(o.s) == 4);
        CHECK(!sp_early(o.s, P(3)) && o.s.early == P(3));  // the early stream landed where the candidate was
        CHECK(sp_early(o.s, P(0)) && o.s.early == P(0));   // ... or beside q1 after all: reported, not retried
        CHECK(sp_candidate(o.s, P(3)) == SP_GIVE_UP && o.s.tries == 4 && o.s.n_pads == 3);  // (done: nothing more is taken)
    }
    {  // a free pipe on the first try: no pad
        Outcome o = rehearse(P(2), P(1), P(0), {P(3), P(0)});
        CHECK(o.acts.size() == 1 && o.acts[0] == SP_FREE);
        CHECK(o.s.n_pads == 0 && o.s.free_at == 0 && sp_distinct_seen(o.s) == 4);
    }
    {  // a free pipe on the third try: two pads
        Outcome o = rehearse(P(2), P(1), P(0), {P(0), P(2), P(3), P(3)});
        CHECK(o.acts.size() == 3 && o.acts[2] == SP_FREE && o.s.n_pads == 2 && o.s.free_at == 2);
    }
    {  // none in four tries: every candidate goes, the handle is what it was
        Outcome o = rehearse(P(2), P(1), P(0), {P(0), P(1), P(2), P(0), P(3)});
        CHECK(o.acts.size() == 4);
        CHECK(o.acts[0] == SP_PAD && o.acts[1] == SP_PAD && o.acts[2] == SP_PAD && o.acts[3] == SP_GIVE_UP);
        CHECK(o.s.n_pads == 0 && o.s.free_at == -1 && o.s.done && sp_distinct_seen(o.s) == 3);
    }
    {  // unknown pipes among the candidates never count as free
        Outcome o = rehearse(P(2), P(1), P(0), {-1, -1, P(3)});
        CHECK(o.acts.size() == 3 && o.acts[0] == SP_PAD && o.acts[1] == SP_PAD && o.acts[2] == SP_FREE && o.s.n_pads == 2);
        Outcome u = rehearse(P(2), P(1), P(0), {-1, -1, -1, -1});
        CHECK(u.acts.size() == 4 && u.acts[3] == SP_GIVE_UP && u.s.n_pads == 0 && sp_distinct_seen(u.s) == 3);
        Outcome w = rehearse(P(2), P(1), P(0), {99, P(3)});  // (out of range: unknown)
        CHECK(w.acts.size() == 2 && w.acts[0] == SP_PAD && w.acts[1] == SP_FREE);
    }
    {  // one of the three streams unknown (the CPU stand-in): no rehearsal, nothing steered, nothing shared
        Outcome o = rehearse(-1, -1, -1, {P(3)});
        CHECK(o.acts.empty() && o.s.done && o.s.n_pads == 0 && o.s.tries == 0);
        CHECK(sp_candidate(o.s, P(3)) == SP_GIVE_UP && o.s.tries == 0);
        CHECK(!sp_early(o.s, -1) && o.s.early == -1);
        Outcome q = rehearse(P(2), -1, P(0), {P(3)});
        CHECK(q.acts.empty() && q.s.done);
    }
    {  // two of the three share a pipe (several handles): a free pipe is still one none of them has
        Outcome o = rehearse(P(2), P(1), P(1), {P(1), P(0)});
        CHECK(o.acts.size() == 2 && o.acts[0] == SP_PAD && o.acts[1] == SP_FREE && o.s.n_pads == 1 && sp_distinct_seen(o.s) == 3);
    }
    {  // never more than SP_TRIES - 1 pads, whatever comes
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b)
                for (int c = 0; c < 4; ++c)
                    for (int d = 0; d < 4; ++d) {
                        Outcome o = rehearse(P(2), P(1), P(0), {P(a), P(b), P(c), P(d)});
                        CHECK(o.s.n_pads <= SP_TRIES - 1 && o.s.done);
                        const bool any_free = a == 3 || b == 3 || c == 3 || d == 3;
                        CHECK((o.s.free_at >= 0) == any_free);
                        if (!any_free) CHECK(o.s.n_pads == 0);
                        if (any_free) CHECK(o.s.n_pads == o.s.free_at);
                    }
    }
    if (g_fail) {
        printf("STREAM-PLACE FAILED: %d\n", g_fail);
        return 1;
    }
    printf("STREAM-PLACE OK\n");
    return 0;
}
