// hc_side.hpp -- what the terms that run beside the step share on the host (hc_morison.hip, hc_nonlinear.hip, hc_qtf.hip, and the
// component table of hc_wave_kin.hip): a path's own copy of the wave-component table, the lane with its begin / end protocol, and
// the second-order sea of a path.  DESIGN.md 3.7m states the invariants once.  Part of hc_context.hpp, which includes it behind the
// buffer types it is made of.
#pragma once
#include <functional>

#include "hc_wave_kin2.hpp"

struct hc_ctx;

namespace hc {

struct Wk2Sea;  // hc_wave_kin2_sum.hpp

// A path's own copy of the wave-component table (hc_wave_kin.hpp), [kKinCols][nf] with the two direction columns behind it when
// directions are set: another path may rebuild its table for another regular phase while a launch of this one is in flight.
struct KinTableCopy {
    unsigned long long serial = ~0ULL;  // wave_serial it was built at; ~0: nothing cached
    double phase = 0.0;                 // ... and the regular phase
    int nf = 0;
    bool dir = false;  // it carries the direction columns: the launch goes to the directional instantiation
    DeviceBuffer<double> tab;
    // what a path makes of the host table before the upload: the table [kKinCols][nf] and the direction columns [kDirCols][nf]
    // (empty: none set), which go behind whatever `tab` holds afterwards
    using Shape = std::function<void(std::vector<double>& tab, std::vector<double>& dir, int nf)>;
    bool current(const hc_ctx* c, double regular_phase) const;
    // The table of the wave model in force on the device, complete when the call returns.  Rebuilt on `st` when a hc_set_wave_* call
    // has come in since or the regular wave's phase differs; a failure on the way leaves nothing that counts as current.
    void refresh(hc_ctx* c, double regular_phase, hipStream_t st, const Shape& shape = nullptr);  // hc_wave_kin.hip
};

struct Order2Part;

// The lane of a side term: a stream, a component table and options of its own -- nothing of it is shared with a step or with
// another lane -- and the begin / end protocol: a setter never races a launch, a failed begin leaves nothing pending.
struct SideLane {
    hipStream_t stream = nullptr;  // created by the path's first setter
    bool dirty = false;            // the path's lists or tables have changed since the device copy was made
    int pending = 0;               // a begin without its end: 1 zeros (nothing launched), 2 a launch is in flight
    KinTableCopy kin;
    hc_wave_kinematics_opts opts{0.0, 0.0, 1};
    void open() {
        if (!stream) HC_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    void close() {
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
    void require_idle(const char* msg) const {
        if (pending) throw Error(HC_ERR_INVALID, msg);
    }
    // the options call of a path (`need_mwl`: the path reads mwl)
    void set_options(const hc_wave_kinematics_opts* o, bool need_mwl, const char* msg_bad, const char* msg_in_flight) {
        hc_wave_kinematics_opts v;
        hc_wave_kinematics_opts_default(&v);
        if (o) v = *o;
        if (!((!need_mwl || std::isfinite(v.mwl)) && std::isfinite(v.regular_phase))) throw Error(HC_ERR_INVALID, msg_bad);
        require_idle(msg_in_flight);
        opts = v;
    }
    template <class Enqueue>
    void begin(bool launch, Enqueue&& enqueue) {
        if (launch) {
            try {
                enqueue();
            } catch (...) {
                (void)hipStreamSynchronize(stream);  // nothing stays pending
                throw;
            }
        }
        pending = launch ? 2 : 1;
    }
    // clears `pending`, waits for the launch if there was one, and returns which it was; `o2`: the path's second-order sea, whose
    // increments change hands around the wait
    inline int end(const char* msg_no_begin, Order2Part* o2 = nullptr);
};

// The second-order sea of a path (hc_set_morison_second_order, hc_set_nonlinear_second_order): tables of its own, built on the
// lane's stream (a hc_wave_kinematics2 call with other cut-offs may rebuild its `wk2[]` set while a launch of the path is in flight), and the
// increments at the path's points with their two host copies: of the evaluation in flight and of the last completed one.
struct Order2Part {
    bool on = false;
    // hc_set_morison_second_order_directional, hc_set_nonlinear_second_order_directional: under directions the path runs the
    // directional pair sum
    bool dir_on = false;
    double cut[4] = {0.0, HUGE_VAL, 0.0, HUGE_VAL};
    int ramp = 1;
    Wk2TableSet tabs;       // long-crested or directional (Wk2TableSet::dir), as the evaluation that built them: never both at once
    DeviceBuffer<double> d_inc;
    PinnedBuffer<double> h_inc[2];
    int h_width[2] = {0, 0};  // doubles per point in each host copy (the directional Morison path stores more)
    int cur = 0;            // which of the two holds the last completed one
    bool flight = false;    // the evaluation in flight writes the other one
    std::vector<int> off;   // [nloc + 1] first point of an owned body in the device copy of the lists
    std::vector<int> done;  // ... in the last completed evaluation; empty: none has completed
    // `on` false: the second copy of the tables and the increments go (nothing of the path is in flight)
    void set(const SideLane& lane, const char* msg_in_flight, int on_, double diff_lo, double diff_hi, double sum_lo, double sum_hi,
             int apply_ramp) {
        hc_wave_kinematics2_opts o;
        hc_wave_kinematics2_opts_default(&o);
        o.diff_lo = diff_lo, o.diff_hi = diff_hi, o.sum_lo = sum_lo, o.sum_hi = sum_hi;
        if (const char* bad = wk2_check_opts(o)) throw Error(HC_ERR_INVALID, bad);
        lane.require_idle(msg_in_flight);
        on     = on_ != 0;
        cut[0] = diff_lo, cut[1] = diff_hi, cut[2] = sum_lo, cut[3] = sum_hi;
        ramp   = apply_ramp != 0;
        if (!on) release();
    }
    void get(int* on_, double* diff_lo, double* diff_hi, double* sum_lo, double* sum_hi, int* apply_ramp) const {
        if (on_) *on_ = on ? 1 : 0;
        if (diff_lo) *diff_lo = cut[0];
        if (diff_hi) *diff_hi = cut[1];
        if (sum_lo) *sum_lo = cut[2];
        if (sum_hi) *sum_hi = cut[3];
        if (apply_ramp) *apply_ramp = ramp;
    }
    void release() {
        tabs.release();
        d_inc.release();
        done.clear();
    }
    // The tables for the lane's regular phase (wk2_tables; `dir`: in the layout of the short-crested sea), built on its stream;
    // whether order 2 applies to this evaluation.  No components (NoWave, no model, an imported eta record) or no pair inside either
    // band: order 1, no further launch.
    bool prepare(hc_ctx* c, const SideLane& lane, bool dir);  // hc_wave_kin2.hip
    Wk2Sea sea(const hc_ctx* c, double mwl) const;  // hc_wave_kin2.hip
    int ramped(const hc_ctx* c) const;              // hc_wave_kin2.hip: the switch only (wk2_ramp2)
    // the host copy the evaluation in flight writes, for n doubles, `width` per point (the device increments grow with it)
    double* stage(size_t n, int width = 0) {
        PinnedBuffer<double>& h = h_inc[cur ^ 1];
        if (d_inc.n < n) d_inc.alloc(n);
        if (h.n < n) h.alloc(n);
        h_width[cur ^ 1] = width;
        flight = true;
        return h.p;
    }
    const double* last() const { return h_inc[cur].p; }
    int last_width() const { return h_width[cur]; }
    bool retire() {  // before the wait of the path's end
        const bool with_inc = flight;
        flight = false;
        done.clear();  // (stays so when the wait fails)
        return with_inc;
    }
    void complete() {  // the evaluation that has completed is the one the increments getter answers with
        cur ^= 1;
        done = off;
    }
};

inline int SideLane::end(const char* msg_no_begin, Order2Part* o2) {
    if (!pending) throw Error(HC_ERR_INVALID, msg_no_begin);
    const int what = pending;
    pending        = 0;
    const bool with_inc = o2 && o2->retire();
    if (what == 2) HC_HIP(hipStreamSynchronize(stream));
    if (with_inc) o2->complete();
    return what;
}

}  // namespace hc
