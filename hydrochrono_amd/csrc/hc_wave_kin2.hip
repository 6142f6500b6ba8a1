// hc_wave_kin2.hip -- second-order irregular waves (Sharma and Dean 1981): the second-order increments to the elevation, velocity
// and acceleration of hc_wave_kinematics, batched over P points x T times, in the long-crested sea and -- `dir` on the host, DIR
// in the kernels -- in a short-crested one whose components travel in directions of their own (include/hydrochrono_amd.h:
// hc_wave_kinematics2, hc_wave_kinematics2_pair_tables, hc_wave_kinematics2_dir, hc_wave_kinematics2_dir_pair_tables).  Not in the
// reference.  Off the step path: each of the two calls has its own stream, component table, pair tables and buffers
// (hc_ctx::wk2[dir]); they read and write nothing a step uses, so they are not ordered against the direct queue (as hc_qtf.hip).
// DESIGN.md 3.7f has the definition, the checks behind it, the kernels and their invariants; 3.7n the short-crested sea.
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"
#include "hc_wave_kin2.hpp"
#include "hc_wave_kin2_dir.hpp"
#include "hc_wave_kin2_sum.hpp"

#include <algorithm>
#include <cstring>

using namespace hc::detail;

// No implicit fusing of a multiplication into an addition below (the pair sums of hc_wave_kin2_sum.hpp and hc_wave_kin2_dir.hpp
// switch it off for themselves, wherever they are compiled): the sums are written with explicit fma() where one is wanted, so that
// an item's bits are the same in every instantiation of the sum kernel (whatever outputs were asked for).
#pragma clang fp contract(off)

namespace hc {
namespace {

struct Wk2PairArgs {
    const double* tab;  // [kKinCols][nf] (hc_wave_kin.hpp); DIR: [kKinCols + kDirCols][nf], cos and sin of the directions behind it
    int nf;
    int finite_depth;
    double g, depth;
    double cut[4];      // diff_lo, diff_hi, sum_lo, sum_hi
    double* pair;       // [kWk2Tables][nf][nf]
};

// One work item per pair (i, j) of the full matrix; an entry outside its cut-off band is stored as 0.
// DIR: the same evaluation form with the angle between the two components in it: gamma = cos(beta_i - beta_j) = tau - sigma,
//     k_i . k_j - R_i R_j = gamma (k_i delta_j + R_j delta_i) - 2 sigma R_i R_j
//     k_i . k_j + R_i R_j = gamma (k_i delta_j + R_j delta_i) + 2 tau R_i R_j
// and from them K+- = (D+- - gamma (k_i delta_j + R_j delta_i)) / (r_i r_j) + 2 sigma r_i r_j + {R_i + R_j, (r_i - r_j)^2}.
// Two arithmetic forms, one skeleton: the long-crested one is not the directional one at sigma = 0 (not the same bits).
template <bool DIR>
__global__ void __launch_bounds__(kWk2Threads) wk2_pair_kernel(Wk2PairArgs a) {
    const long long n2 = static_cast<long long>(a.nf) * a.nf;
    const long long e  = static_cast<long long>(blockIdx.x) * kWk2Threads + threadIdx.x;
    if (e >= n2) return;
    const int i = static_cast<int>(e / a.nf), j = static_cast<int>(e - static_cast<long long>(i) * a.nf);
    const double Ai = a.tab[kKinAmp * a.nf + i], wi = a.tab[kKinOmega * a.nf + i], ki = a.tab[kKinK * a.nf + i];
    const double Aj = a.tab[kKinAmp * a.nf + j], wj = a.tab[kKinOmega * a.nf + j], kj = a.tab[kKinK * a.nf + j];
    double sig = 0.0, tau = 1.0;  // (DIR only)
    if constexpr (DIR)
        wk2_dir_angle(a.tab[kKinCols * a.nf + i], a.tab[(kKinCols + 1) * a.nf + i], a.tab[kKinCols * a.nf + j], a.tab[(kKinCols + 1) * a.nf + j],
                      sig, tau);
    const double gam = tau - sig;
    const double Ri = wi * wi / a.g, Rj = wj * wj / a.g;
    const double ri = sqrt(Ri), rj = sqrt(Rj);
    const double bb = 0.25 * (Ai * a.g / wi) * (Aj * a.g / wj);
    // With delta = k - R (exact: the two are close, equal in deep water) k^2 - R^2 and k_i k_j - R_i R_j keep their relative
    // accuracy where the textbook differences would cancel to rounding noise
    const double di = ki - Ri, dj = kj - Rj;
    // k_i . k_j -+ R_i R_j, what K+- subtract from D+-, and r_i r_j, each form's statements in the order the compiler's schedule of
    // that form was measured with
    double kmR, kpR, gq, rr;
    if constexpr (DIR) {
        gq = gam * (ki * dj + Rj * di);
        const double RR = Ri * Rj;
        rr = ri * rj;
        kmR = gq - 2.0 * sig * RR, kpR = gq + 2.0 * tau * RR;
    } else {
        kmR = ki * dj + Rj * di, kpR = ki * kj + Ri * Rj;
        rr = ri * rj;
        gq = kmR;
    }
    const double ni = di * (ki + Ri), nj = dj * (kj + Rj);  // k^2 - R^2
    double Kp = 0.0, Km = 0.0, Bp = 0.0, Bm = 0.0;
    if (wk2_in_band(wi, wj, 1, a.cut[2], a.cut[3])) {
        const double rs = ri + rj;
        double ak;
        if constexpr (DIR) ak = sqrt(wk2_dir_kappa2(ki, kj, sig, tau)); else ak = fabs(ki + kj);
        const double T   = ak * (a.finite_depth ? tanh(ak * a.depth) : 1.0);
        const double den = rs * rs - T;
        const double D   = (rs * (ri * nj + rj * ni) + 2.0 * (rs * rs) * kmR) / den;
        if constexpr (DIR) Kp = (D - gq) / rr + 2.0 * sig * rr + (Ri + Rj); else Kp = (D - kmR) / rr + (Ri + Rj);
        Bp = bb * D / (wi + wj);
    }
    if (wk2_in_band(wi, wj, 0, a.cut[0], a.cut[1])) {
        const double rd = ri - rj;
        double D = 0.0;
        if (wi != wj) {
            double ak;
            if constexpr (DIR) ak = sqrt(wk2_dir_kappa2(ki, -kj, sig, tau)); else ak = fabs(ki - kj);
            const double T   = ak * (a.finite_depth ? tanh(ak * a.depth) : 1.0);
            const double den = rd * rd - T;
            D  = (rd * (rj * ni - ri * nj) + 2.0 * (rd * rd) * kpR) / den;
            Bm = bb * D / (wi - wj);
        }
        // long-crested: (D - (k_i k_j + R_i R_j)) / (r_i r_j) + R_i + R_j with R = r^2
        if constexpr (DIR) Km = (D - gq) / rr + 2.0 * sig * rr + rd * rd; else Km = (D - kmR) / rr + rd * rd;
    }
    a.pair[kWk2Kp * n2 + e] = Kp;
    a.pair[kWk2Km * n2 + e] = Km;
    a.pair[kWk2Bp * n2 + e] = Bp;
    a.pair[kWk2Bm * n2 + e] = Bm;
}

struct Wk2SumArgs {
    const double* tab;   // [kKinCols][nf]; DIR: [kKinCols + kDirCols][nf]
    int nf;
    int P, T;
    const double* pair;  // [kWk2Tables][nf][nf]
    const int* band;     // [2][nf][2]: sign 0 difference, 1 sum; first and last column j >= i of row i inside the band
    const double* xyz;   // [P][3]
    const double* t;     // [T]
    double depth, mwl;
    int finite_depth;    // 0: water depth +inf, the profiles are e^{|kappa| z}
    int sign_on[2];      // some pair lies inside the difference / the sum band
    int ramped;          // the ramp applies (synthesised irregular model, ramp_duration > 0, apply_ramp)
    double ramp_duration;
    double* eta;         // [T][P]    } NULL: not wanted
    double* vel;         // [T][P][3] }
    double* acc;         // [T][P][3] }
};

// One workgroup per (point, time) item o = j * P + p: the pair sum of the sea (wk2_sea_sum: wk2_item_sum, DIR wk2_dir_item_sum) at
// the item's point and time, then the ramp.  An item's bits depend on the item, the tables and the options only.
template <bool DIR, bool ETA, bool KIN>
__global__ void __launch_bounds__(kWk2Threads) wk2_sum_kernel(Wk2SumArgs a) {
    constexpr int kH = DIR ? 3 : 2;  // velocity components the sum returns: the long-crested sea has no y
    const long long o = blockIdx.x;
    const int p = static_cast<int>(o % a.P), jt = static_cast<int>(o / a.P);
    const double t = a.t[jt];
    const Wk2Sea sea{a.tab, a.nf, a.pair, a.band, a.depth, a.mwl, a.finite_depth, {a.sign_on[0], a.sign_on[1]}};
    const double* q = a.xyz + 3 * static_cast<size_t>(p);
    double sum[wk2_sums(DIR)];
    wk2_sea_sum<DIR, ETA, KIN>(sea, q[0], DIR ? q[1] : 0.0, q[2], t, sum);
    if (threadIdx.x == 0) {
        const double ramp2 = wk2_ramp2(a.ramped != 0, a.ramp_duration, t);  // second order in the amplitude
        if constexpr (ETA) a.eta[o] = 0.25 * sum[0] * ramp2;
        if (KIN && a.vel) {
            a.vel[3 * o]     = sum[1] * ramp2;
            a.vel[3 * o + 1] = DIR ? sum[2] * ramp2 : 0.0;
            a.vel[3 * o + 2] = sum[kH] * ramp2;
        }
        if (KIN && a.acc) {
            a.acc[3 * o]     = sum[kH + 1] * ramp2;
            a.acc[3 * o + 1] = DIR ? sum[kH + 2] * ramp2 : 0.0;
            a.acc[3 * o + 2] = sum[2 * kH] * ramp2;
        }
    }
}

using Wk2SumKernel = void (*)(Wk2SumArgs);
// [dir][eta wanted][velocity or acceleration wanted]
const Wk2SumKernel kWk2Sum[2][2][2] = {
    {{nullptr, wk2_sum_kernel<false, false, true>}, {wk2_sum_kernel<false, true, false>, wk2_sum_kernel<false, true, true>}},
    {{nullptr, wk2_sum_kernel<true, false, true>}, {wk2_sum_kernel<true, true, false>, wk2_sum_kernel<true, true, true>}}};

}  // namespace

int wk2_component_count(const hc_ctx* c) { return c->wave_kind == kWaveRegular ? 1 : static_cast<int>(c->spec_f.size()); }

void wk2_tables(hc_ctx* c, Wk2TableSet& s, hipStream_t st, double regular_phase, const double cut[4], bool keep_empty, bool dir) {
    if (s.dir == dir && kin_table_current(c, s.serial, s.phase, regular_phase) && std::memcmp(s.cut, cut, sizeof(s.cut)) == 0) return;
    s.serial = ~0ULL;  // nothing is cached until all of it is in place
    s.dir    = dir;    // (a set of the other layout is never current)
    std::vector<double> tab = kin_table_host(c, regular_phase);
    const int nf = static_cast<int>(tab.size() / kKinCols);
    if (dir) {
        std::vector<double> cs = kin_dir_columns_host(c);
        if (cs.empty()) {  // no directions set: all along x
            cs.assign(static_cast<size_t>(kDirCols) * nf, 0.0);
            std::fill(cs.begin(), cs.begin() + nf, 1.0);
        }
        require(cs.size() == static_cast<size_t>(kDirCols) * nf, HC_ERR_RUNTIME, "the wave directions do not match the component table");
        tab.insert(tab.end(), cs.begin(), cs.end());
    }
    std::vector<int> band(4 * static_cast<size_t>(nf));
    const double* omega = tab.data() + static_cast<size_t>(kKinOmega) * nf;
    s.any[0] = wk2_bands(omega, nf, 0, cut[0], cut[1], band.data());
    s.any[1] = wk2_bands(omega, nf, 1, cut[2], cut[3], band.data() + 2 * static_cast<size_t>(nf));
    s.d_tab.upload(tab, st);
    s.d_band.upload(band, st);
    const size_t n2 = static_cast<size_t>(nf) * nf;
    if (!(s.any[0] || s.any[1]) && !keep_empty) {
        s.d_pair.release();
    } else {
        if (s.d_pair.n != kWk2Tables * n2) s.d_pair.alloc(kWk2Tables * n2);
        Wk2PairArgs a{};
        a.tab          = s.d_tab.p;
        a.nf           = nf;
        a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
        a.g            = std::fabs(c->g);
        a.depth        = c->depth;
        std::copy(cut, cut + 4, a.cut);
        a.pair = s.d_pair.p;
        hipLaunchKernelGGL(dir ? wk2_pair_kernel<true> : wk2_pair_kernel<false>, dim3(static_cast<unsigned>((n2 + kWk2Threads - 1) / kWk2Threads)),
                           dim3(kWk2Threads), 0, st, a);
        HC_HIP(hipGetLastError());
        HC_HIP(hipStreamSynchronize(st));
    }
    s.nf = nf;
    s.phase = regular_phase;
    std::copy(cut, cut + 4, s.cut);
    s.serial = c->wave_serial;
}

bool Order2Part::prepare(hc_ctx* c, const SideLane& lane, bool dir) {
    if (!on || !kin_has_components(c)) return false;
    wk2_tables(c, tabs, lane.stream, lane.opts.regular_phase, cut, false, dir);
    return tabs.any[0] || tabs.any[1];
}

Wk2Sea Order2Part::sea(const hc_ctx* c, double mwl) const {
    return Wk2Sea{tabs.d_tab.p, tabs.nf, tabs.d_pair.p, tabs.d_band.p, c->depth, mwl, std::isfinite(c->depth) ? 1 : 0,
                  {tabs.any[0] ? 1 : 0, tabs.any[1] ? 1 : 0}};
}

int Order2Part::ramped(const hc_ctx* c) const { return (ramp && kin_synthesised(c) && c->irr.ramp_duration > 0.0) ? 1 : 0; }

namespace {

hc_wave_kinematics2_opts wk2_opts(const hc_wave_kinematics2_opts* opts) {
    hc_wave_kinematics2_opts o;
    hc_wave_kinematics2_opts_default(&o);
    if (opts) o = *opts;
    const char* bad = wk2_check_opts(o);
    require(bad == nullptr, HC_ERR_INVALID, bad ? bad : "");
    return o;
}

// the tables the two calls of a sea read: the call's own set, on its own stream (created by the first call)
Wk2Call& wk2_own_tables(hc_ctx* c, bool dir, const hc_wave_kinematics2_opts& o) {
    Wk2Call& w = c->wk2[dir];
    if (!w.stream) HC_HIP(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    const double cut[4] = {o.diff_lo, o.diff_hi, o.sum_lo, o.sum_hi};
    wk2_tables(c, w.tabs, w.stream, o.regular_phase, cut, true, dir);
    return w;
}

// hc_wave_kinematics2 (which refuses while directions are set) and hc_wave_kinematics2_dir (which reads y)
void wk2_kinematics(hc_ctx* c, bool dir, const hc_wave_kinematics2_opts* opts, int n_points, const double* xyz, int n_times, const double* t,
                    double* eta, double* vel, double* acc) {
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    const hc_wave_kinematics2_opts o = wk2_opts(opts);
    const char* bad = wk2_check_batch(n_points, xyz, n_times, t);
    require(bad == nullptr, HC_ERR_INVALID, bad ? bad : "");
    if (dir)
        for (int p = 0; p < n_points; ++p) require(std::isfinite(xyz[3 * static_cast<size_t>(p) + 1]), HC_ERR_INVALID, "non-finite y of a point");
    const bool waves = kin_has_components(c);
    require(dir || c->wave_dir.empty(), HC_ERR_UNSUPPORTED,
            "the second-order sea is long-crested: not available while wave directions are set (hc_set_wave_directions)");
    require(!waves || wk2_component_count(c) <= kWk2MaxFreq, HC_ERR_UNSUPPORTED, "more than 4096 wave components");
    const size_t n = static_cast<size_t>(n_points) * n_times;
    if (n == 0 || !(eta || vel || acc)) return;
    Wk2Call& w = waves ? wk2_own_tables(c, dir, o) : c->wk2[dir];
    // NoWave, no model, an imported eta record (no components), or no pair inside either band: zeros, no launch
    if (!waves || !(w.tabs.any[0] || w.tabs.any[1])) {
        if (eta) std::fill(eta, eta + n, 0.0);
        if (vel) std::fill(vel, vel + 3 * n, 0.0);
        if (acc) std::fill(acc, acc + 3 * n, 0.0);
        return;
    }
    hipStream_t st = w.stream;
    // one buffer: points, times, then the requested outputs
    const size_t n_in = 3 * static_cast<size_t>(n_points) + n_times;
    const size_t n_out = (eta ? n : 0) + (vel ? 3 * n : 0) + (acc ? 3 * n : 0);
    if (w.io.n < n_in + n_out) w.io.alloc(n_in + n_out);
    double* d_xyz = w.io.p;
    double* d_t   = d_xyz + 3 * static_cast<size_t>(n_points);
    double* d_out = d_t + n_times;
    Wk2SumArgs a{};
    a.tab          = w.tabs.d_tab.p;
    a.nf           = w.tabs.nf;
    a.P            = n_points;
    a.T            = n_times;
    a.pair         = w.tabs.d_pair.p;
    a.band         = w.tabs.d_band.p;
    a.xyz          = d_xyz;
    a.t            = d_t;
    a.depth        = c->depth;
    a.mwl          = o.mwl;
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    a.sign_on[0]   = w.tabs.any[0] ? 1 : 0;
    a.sign_on[1]   = w.tabs.any[1] ? 1 : 0;
    a.ramped        = (o.apply_ramp && kin_synthesised(c) && c->irr.ramp_duration > 0.0) ? 1 : 0;  // the switch only (wk2_ramp2)
    a.ramp_duration = c->irr.ramp_duration;
    if (eta) {
        a.eta = d_out;
        d_out += n;
    }
    if (vel) {
        a.vel = d_out;
        d_out += 3 * n;
    }
    if (acc) a.acc = d_out;
    HC_HIP(hipMemcpyAsync(d_xyz, xyz, 3 * static_cast<size_t>(n_points) * sizeof(double), hipMemcpyHostToDevice, st));
    HC_HIP(hipMemcpyAsync(d_t, t, static_cast<size_t>(n_times) * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kWk2Sum[dir][eta != nullptr][vel || acc], dim3(static_cast<unsigned>(n)), dim3(kWk2Threads), 0, st, a);
    HC_HIP(hipGetLastError());
    if (eta) HC_HIP(hipMemcpyAsync(eta, a.eta, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (vel) HC_HIP(hipMemcpyAsync(vel, a.vel, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (acc) HC_HIP(hipMemcpyAsync(acc, a.acc, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
}

void wk2_pair_tables(hc_ctx* c, bool dir, const hc_wave_kinematics2_opts* opts, double* Kp, double* Km, double* Bp, double* Bm) {
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    const hc_wave_kinematics2_opts o = wk2_opts(opts);
    if (!kin_has_components(c)) return;
    require(wk2_component_count(c) <= kWk2MaxFreq, HC_ERR_UNSUPPORTED, "more than 4096 wave components");
    const Wk2Call& w = wk2_own_tables(c, dir, o);
    const size_t n2 = static_cast<size_t>(w.tabs.nf) * w.tabs.nf;
    double* out[kWk2Tables] = {Kp, Km, Bp, Bm};
    for (int k = 0; k < kWk2Tables; ++k)
        if (out[k]) HC_HIP(hipMemcpyAsync(out[k], w.tabs.d_pair.p + k * n2, n2 * sizeof(double), hipMemcpyDeviceToHost, w.stream));
    HC_HIP(hipStreamSynchronize(w.stream));
}

}  // namespace
}  // namespace hc

extern "C" {

void hc_wave_kinematics2_opts_default(hc_wave_kinematics2_opts* o) {
    if (!o) return;
    o->mwl           = 0.0;
    o->regular_phase = 0.0;
    o->diff_lo       = 0.0;
    o->diff_hi       = HUGE_VAL;
    o->sum_lo        = 0.0;
    o->sum_hi        = HUGE_VAL;
    o->apply_ramp    = 1;
}

// The four calls touch no step state, so they are not ordered against the direct queue (HC_API_BEGIN_HOT): a call between steps
// leaves a pass that is running alone.
int hc_wave_kinematics2(hc_ctx* c, const hc_wave_kinematics2_opts* opts, int n_points, const double* xyz, int n_times, const double* t,
                        double* eta, double* vel, double* acc) {
    HC_API_BEGIN_HOT(c)
    hc::wk2_kinematics(c, false, opts, n_points, xyz, n_times, t, eta, vel, acc);
    HC_API_END(c)
}

int hc_wave_kinematics2_dir(hc_ctx* c, const hc_wave_kinematics2_opts* opts, int n_points, const double* xyz, int n_times, const double* t,
                            double* eta, double* vel, double* acc) {
    HC_API_BEGIN_HOT(c)
    hc::wk2_kinematics(c, true, opts, n_points, xyz, n_times, t, eta, vel, acc);
    HC_API_END(c)
}

int hc_wave_kinematics2_pair_tables(hc_ctx* c, const hc_wave_kinematics2_opts* opts, double* Kp, double* Km, double* Bp, double* Bm) {
    HC_API_BEGIN_HOT(c)
    hc::wk2_pair_tables(c, false, opts, Kp, Km, Bp, Bm);
    HC_API_END(c)
}

int hc_wave_kinematics2_dir_pair_tables(hc_ctx* c, const hc_wave_kinematics2_opts* opts, double* Kp, double* Km, double* Bp, double* Bm) {
    HC_API_BEGIN_HOT(c)
    hc::wk2_pair_tables(c, true, opts, Kp, Km, Bp, Bm);
    HC_API_END(c)
}

}  // extern "C"
