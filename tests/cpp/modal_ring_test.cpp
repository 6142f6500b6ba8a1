// CPU unit test of the snapshot-ring bookkeeping of the modal radiation term (hydrochrono_amd/csrc/hc_modal_ring.hpp, host only):
// first call, advance, duplicate time, a step back in time (which snapshots go, which slot is read and written), a step back past
// everything the ring keeps (refused, state unchanged), depth changes and reset -- against a model that keeps every snapshot in a
// plain list.  Built with plain g++ by tests/test_radiation_modes_ref_cpu.py.
#include <cstdio>
#include <vector>

#include "../../hydrochrono_amd/csrc/hc_modal_ring.hpp"

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            ++failures;                                                   \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
        }                                                                 \
    } while (0)

// what the slots hold, by the time written into them (the test's stand-in for z and v)
struct Model {
    hc::ModalRing ring;
    std::vector<double> slot;
    explicit Model(int depth) : slot(static_cast<size_t>(depth), -1.0) { ring.set_depth(depth); }
    // returns the status; on success *from is the time of the snapshot the step started from (-1: first)
    hc::ModalAdvance::Status step(double t, double* from) {
        const hc::ModalAdvance a = ring.plan(t);
        if (a.status != hc::ModalAdvance::kOk) return a.status;
        CHECK(a.dst >= 0 && a.dst < ring.depth);
        if (a.first) {
            *from = -1.0;
        } else {
            CHECK(a.src >= 0 && a.src < ring.depth && a.src != a.dst);
            *from = slot[static_cast<size_t>(a.src)];
            CHECK(*from == a.t_src);
        }
        slot[static_cast<size_t>(a.dst)] = t;
        ring.commit(a, t);
        CHECK(ring.head == a.dst && ring.times.front() == t);
        CHECK(static_cast<int>(ring.times.size()) <= ring.depth);
        // every kept time sits in the slot the index says: newest at head, older ones behind it
        for (size_t k = 0; k < ring.times.size(); ++k) {
            const int s = ((ring.head - static_cast<int>(k)) % ring.depth + ring.depth) % ring.depth;
            CHECK(slot[static_cast<size_t>(s)] == ring.times[k]);
        }
        return a.status;
    }
};

int main() {
    double from = 0.0;
    {  // first call, advance, duplicate
        Model m(4);
        CHECK(m.step(0.0, &from) == hc::ModalAdvance::kOk && from == -1.0);
        CHECK(m.step(0.1, &from) == hc::ModalAdvance::kOk && from == 0.0);
        CHECK(m.step(0.25, &from) == hc::ModalAdvance::kOk && from == 0.1);
        const hc::ModalRing before = m.ring;
        CHECK(m.step(0.25, &from) == hc::ModalAdvance::kDuplicateTime);
        CHECK(m.ring.times == before.times && m.ring.head == before.head);
        CHECK(m.step(0.3, &from) == hc::ModalAdvance::kOk && from == 0.25);
    }
    {  // a rejected step: t1 t2 t3, back to t2' -- t2 and t3 go, the step starts from t1; then on from t2'
        Model m(4);
        m.step(1.0, &from);
        m.step(2.0, &from);
        m.step(3.0, &from);
        CHECK(m.step(1.5, &from) == hc::ModalAdvance::kOk && from == 1.0);
        CHECK(m.ring.times.size() == 2 && m.ring.times[0] == 1.5 && m.ring.times[1] == 1.0);
        CHECK(m.step(2.5, &from) == hc::ModalAdvance::kOk && from == 1.5);
        // back to exactly an accepted time: that snapshot goes as well (times >= t)
        CHECK(m.step(1.5, &from) == hc::ModalAdvance::kOk && from == 1.0);
        CHECK(m.ring.times.size() == 2);
    }
    {  // past the depth: the ring of 3 keeps 3 times; a step back below the oldest is refused and changes nothing
        Model m(3);
        for (int k = 0; k < 7; ++k) CHECK(m.step(1.0 + k, &from) == hc::ModalAdvance::kOk);
        CHECK(m.ring.times.size() == 3 && m.ring.times.back() == 5.0);
        const hc::ModalRing before = m.ring;
        const std::vector<double> slots = m.slot;
        CHECK(m.step(4.5, &from) == hc::ModalAdvance::kNoSnapshot);
        CHECK(m.step(5.0, &from) == hc::ModalAdvance::kNoSnapshot);  // the oldest itself would have to go
        CHECK(m.ring.times == before.times && m.ring.head == before.head && m.slot == slots);
        CHECK(m.step(5.5, &from) == hc::ModalAdvance::kOk && from == 5.0);  // the deepest rewind that is possible
        CHECK(m.ring.times.size() == 2);
        CHECK(m.step(8.0, &from) == hc::ModalAdvance::kOk && from == 5.5);
    }
    {  // before the very first time
        Model m(2);
        m.step(1.0, &from);
        CHECK(m.step(0.5, &from) == hc::ModalAdvance::kNoSnapshot);
        CHECK(m.step(1.5, &from) == hc::ModalAdvance::kOk && from == 1.0);
        CHECK(m.step(2.5, &from) == hc::ModalAdvance::kOk && from == 1.5);
        CHECK(m.ring.times.size() == 2);
        CHECK(m.step(1.2, &from) == hc::ModalAdvance::kNoSnapshot);  // depth 2: 1.0 is gone
        CHECK(m.step(2.0, &from) == hc::ModalAdvance::kOk && from == 1.5);
    }
    {  // reset and depth
        Model m(4);
        m.step(1.0, &from);
        m.step(2.0, &from);
        m.ring.reset();
        CHECK(m.ring.times.empty() && m.ring.head == -1);
        CHECK(m.step(2.0, &from) == hc::ModalAdvance::kOk && from == -1.0);  // a first call again: no duplicate
        CHECK(!m.ring.set_depth(1) && !m.ring.set_depth(65) && m.ring.depth == 4 && m.ring.times.size() == 1);
        CHECK(m.ring.set_depth(64) && m.ring.depth == 64 && m.ring.times.empty());
        hc::ModalRing fresh;
        CHECK(fresh.depth == hc::kModalDepthDefault && fresh.depth == 4);
    }
    {  // a long irregular walk with rewinds, against the plain list
        Model m(5);
        std::vector<double> accepted;
        unsigned long long s = 12345;
        double t = 0.0;
        for (int n = 0; n < 2000; ++n) {
            s = s * 6364136223846793005ULL + 1442695040888963407ULL;
            const double u = static_cast<double>(s >> 11) / 9007199254740992.0;
            const bool back = !accepted.empty() && u < 0.2;
            const double tn = back ? t - 3.0 * u * 5.0 : t + 0.01 + u;
            std::vector<double> keep;
            for (double a : accepted)
                if (a < tn) keep.push_back(a);
            while (accepted.size() > 5) accepted.erase(accepted.begin());
            const hc::ModalAdvance::Status st = m.step(tn, &from);
            if (accepted.empty()) {
                CHECK(st == hc::ModalAdvance::kOk && from == -1.0);
            } else if (tn == accepted.back()) {
                CHECK(st == hc::ModalAdvance::kDuplicateTime);
                continue;
            } else if (keep.empty()) {
                CHECK(st == hc::ModalAdvance::kNoSnapshot);
                continue;
            } else {
                CHECK(st == hc::ModalAdvance::kOk && from == keep.back());
            }
            accepted = keep;
            accepted.push_back(tn);
            while (accepted.size() > 5) accepted.erase(accepted.begin());
            t = tn;
        }
    }
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
