// Host-only check of the bookkeeping behind hc_get_morison_member_node_increments / hc_get_morison_member_point_increments
// (hydrochrono_amd/csrc/hc_member_increments.hpp): which of the two host copies an evaluation writes, when the copies change hands,
// and what the getters may answer with.  Built with -fsanitize=address,undefined by tests/test_morison_members2_ref_cpu.py; the
// copies here are plain vectors sized by the layout, so a wrong size or a stale layout shows as an out-of-bounds access.
#include <cstdio>
#include <vector>

#include "../../hydrochrono_amd/csrc/hc_member_increments.hpp"

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #c);            \
            ++failures;                                            \
        }                                                          \
    } while (0)

int main() {
    using namespace hc;
    MemberIncrementCopies c;
    std::vector<double> host[2];
    CHECK(!c.done && !c.flight && c.last().doubles() == 0);
    // an end without increments in flight leaves everything as it is
    CHECK(!c.retire() && !c.done);

    // evaluation 1: two bodies, 5 + 3 nodes, 8 + 4 points, long-crested
    const std::vector<int> node_off{0, 5, 8}, point_off{0, 8, 12};
    int slot = c.stage(kMemPointIncDoubles, node_off, point_off);
    CHECK(slot == 1 && c.flight && !c.done);
    CHECK(c.layout[slot].nodes() == 8 && c.layout[slot].points() == 12);
    CHECK(c.layout[slot].point_base() == 32 && c.layout[slot].doubles() == 32 + 8 * 12);
    host[slot].assign(c.layout[slot].doubles(), 1.0);
    CHECK(c.retire() && !c.flight && !c.done);  // before the wait: nothing to answer with
    c.complete();
    CHECK(c.done && c.cur == 1 && c.last().width == kMemPointIncDoubles);
    // the getter's walk over body 1 stays inside the copy
    {
        const MemberIncrementLayout& l = c.last();
        double sum = 0.0;
        for (int j = l.node_off[1]; j < l.node_off[2]; ++j) sum += host[c.cur][static_cast<size_t>(kMemNodeIncDoubles) * j + 3];
        for (int e = l.point_off[1]; e < l.point_off[2]; ++e) sum += host[c.cur][l.point_base() + static_cast<size_t>(l.width) * e + l.width - 1];
        CHECK(sum == 3.0 + 4.0);
    }

    // evaluation 2, directional and larger: written into the other copy while the first still answers
    const std::vector<int> node_off2{0, 9, 20}, point_off2{0, 16, 38};
    slot = c.stage(kMemPointDirIncDoubles, node_off2, point_off2);
    CHECK(slot == 0 && c.done && c.last().width == kMemPointIncDoubles && c.last().nodes() == 8);
    host[slot].assign(c.layout[slot].doubles(), 2.0);
    CHECK(c.layout[slot].doubles() == 4 * 20 + 10 * 38);
    CHECK(c.retire());
    c.complete();
    CHECK(c.done && c.cur == 0 && c.last().width == kMemPointDirIncDoubles && c.last().points() == 38);
    CHECK(host[c.cur][c.last().doubles() - 1] == 2.0);

    // an evaluation without a second-order member part: the one before still answers
    c.reset();
    CHECK(!c.retire() && c.done && c.cur == 0);
    // a begin that failed after staging: reset by the next begin, nothing changes hands
    c.stage(kMemPointIncDoubles, node_off, point_off);
    c.reset();
    CHECK(!c.flight && !c.retire() && c.done && c.cur == 0 && c.last().points() == 38);
    // a wait that fails: retired, never completed
    c.stage(kMemPointIncDoubles, node_off, point_off);
    CHECK(c.retire() && !c.done);
    CHECK(c.cur == 0);
    // a list change or the switch going off forgets
    c.stage(kMemPointIncDoubles, node_off, point_off);
    CHECK(c.retire());
    c.complete();
    CHECK(c.done && c.cur == 1);
    c.forget();
    CHECK(!c.done);
    // empty lists
    MemberIncrementLayout none;
    CHECK(none.nodes() == 0 && none.points() == 0 && none.doubles() == 0);
    std::printf("%d failures\n", failures);
    return failures != 0;
}
