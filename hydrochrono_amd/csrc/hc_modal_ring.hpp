// hc_modal_ring.hpp -- bookkeeping of the snapshot ring of the modal radiation term (hc_radiation_modes.hip; host only, no HIP
// dependency, unit-tested on CPU: tests/cpp/modal_ring_test.cpp).  The snapshots themselves -- the modal state z and the velocities
// v of an accepted time -- live in `depth` slots in HBM; this is the index: which times are kept, newest first, which slot holds
// the newest one, and what a step BACK in time does to both.  As hc_history.hpp is for the convolution's velocity ring, with one
// difference: the recursion needs one earlier snapshot, not a window, so nothing is pruned by age and nothing is re-admitted.
#pragma once
#include <deque>

namespace hc {

constexpr int kModalDepthMin = 2, kModalDepthMax = 64, kModalDepthDefault = 4;

// What a call at time t does: which slot it reads and which it writes.  Made by plan(), which changes nothing; commit() applies it
// once the launch is on its way, so a refused call leaves the ring as it was.
struct ModalAdvance {
    enum Status { kOk = 0, kDuplicateTime = 1, kNoSnapshot = 2 };
    Status status = kOk;
    bool first    = false;  // no snapshot to start from: z = 0 goes to slot `dst`, the result is zero
    int src = -1, dst = 0;  // slot of the snapshot the step starts from (-1: first), slot of the new one
    double t_src  = 0.0;    // time of the source snapshot (h = t - t_src)
    int dropped   = 0;      // snapshots of an abandoned attempt (times >= t) a step back in time removes
};

struct ModalRing {
    int depth = kModalDepthDefault;
    int head  = -1;             // slot of the newest snapshot, -1: none
    std::deque<double> times;   // accepted times, newest first; at most `depth`

    void reset() {
        times.clear();
        head = -1;
    }
    // true: the depth was taken (the ring is emptied: the slots are laid out anew)
    bool set_depth(int d) {
        if (d < kModalDepthMin || d > kModalDepthMax) return false;
        depth = d;
        reset();
        return true;
    }
    // t above the newest time: the next slot from the newest snapshot.  t equal to it: the convolution's duplicate-time error.
    // t below it (a rejected step): the snapshots at times >= t belong to the abandoned attempt and go; the step starts from the
    // newest one that survives, and if none does the call is refused.
    ModalAdvance plan(double t) const {
        ModalAdvance a;
        if (times.empty()) {
            a.first = true;
            a.dst   = 0;
            return a;
        }
        if (t == times.front()) {
            a.status = ModalAdvance::kDuplicateTime;
            return a;
        }
        int k = 0;
        while (k < static_cast<int>(times.size()) && times[static_cast<size_t>(k)] >= t) ++k;
        if (k == static_cast<int>(times.size())) {
            a.status = ModalAdvance::kNoSnapshot;
            return a;
        }
        a.dropped = k;
        a.src     = ((head - k) % depth + depth) % depth;
        a.dst     = (a.src + 1) % depth;
        a.t_src   = times[static_cast<size_t>(k)];
        return a;
    }
    void commit(const ModalAdvance& a, double t) {
        for (int k = 0; k < a.dropped; ++k) times.pop_front();
        times.push_front(t);
        while (static_cast<int>(times.size()) > depth) times.pop_back();  // the oldest snapshot's slot is the one just written
        head = a.dst;
    }
};

}  // namespace hc
