// hc_member_increments.hpp -- the bookkeeping of the two host copies of the strip members' second-order increments
// (hc_morison_members.hip, DESIGN.md 3.7c''): which copy the evaluation in flight writes, which one holds the last completed
// evaluation, and the layout either was written in.  The copies change hands around the wait of hc_morison_end, as the elements'
// do (hc_side.hpp: Order2Part::stage / retire / complete).  No HIP dependency: tests/cpp/member_increments_host_check.cpp exercises it
// in a plain host build.
#pragma once
#include <cstddef>
#include <vector>

namespace hc {

constexpr int kMemNodeIncDoubles     = 4;   // P, eta2 of a node
constexpr int kMemPointIncDoubles    = 8;   // p, eta2, u2x, u2z, a2x, a2z of a Gauss point
constexpr int kMemPointDirIncDoubles = 10;  // p, eta2, u2[3], a2[3] of a Gauss point in the short-crested sea

// One copy: [nodes][kMemNodeIncDoubles], then [points][width]
struct MemberIncrementLayout {
    int width = 0;                         // doubles per Gauss point
    std::vector<int> node_off, point_off;  // [nloc + 1] first node / Gauss point of an owned body
    int nodes() const { return node_off.empty() ? 0 : node_off.back(); }
    int points() const { return point_off.empty() ? 0 : point_off.back(); }
    size_t point_base() const { return static_cast<size_t>(kMemNodeIncDoubles) * nodes(); }
    size_t doubles() const { return point_base() + static_cast<size_t>(width) * points(); }
};

struct MemberIncrementCopies {
    MemberIncrementLayout layout[2];
    int cur     = 0;      // which of the two holds the last completed evaluation
    bool flight = false;  // the evaluation in flight writes the other one
    bool done   = false;  // layout[cur] is a completed evaluation of the lists as they are

    // the copy the evaluation in flight writes, with the layout it is written in
    int stage(int width, const std::vector<int>& node_off, const std::vector<int>& point_off) {
        MemberIncrementLayout& l = layout[cur ^ 1];
        l.width     = width;
        l.node_off  = node_off;
        l.point_off = point_off;
        flight      = true;
        return cur ^ 1;
    }
    // a begin starts from nothing in flight (a failed one leaves nothing pending)
    void reset() { flight = false; }
    // before the wait of the lane's end: whether the evaluation carries increments.  The getters answer nothing until it has
    // completed (and stay so when the wait fails).
    bool retire() {
        const bool with_inc = flight;
        flight = false;
        if (with_inc) done = false;
        return with_inc;
    }
    // after the wait: the evaluation that has completed is the one the getters answer with
    void complete() {
        cur ^= 1;
        done = true;
    }
    // a member list has changed or the switch went off: the last evaluation no longer describes the lists
    void forget() { done = false; }
    const MemberIncrementLayout& last() const { return layout[cur]; }
};

}  // namespace hc
