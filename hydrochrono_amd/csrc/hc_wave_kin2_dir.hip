// hc_wave_kin2_dir.hip -- second-order irregular waves in a short-crested sea: the increments of hc_wave_kin2.hip for components
// that travel in directions of their own (hc_set_wave_directions), batched over P points x T times (include/hydrochrono_amd.h:
// hc_wave_kinematics2_dir, hc_wave_kinematics2_dir_pair_tables).  Not in the reference.  A call beside hc_wave_kinematics2, which
// keeps its refusal, its kernels and its bits: own stream, component table with the direction columns, pair tables and buffers.
// DESIGN.md 3.7n has the definition, the evaluation form, the kernels and their invariants.
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"
#include "hc_wave_kin2.hpp"
#include "hc_wave_kin2_dir.hpp"

#include <algorithm>
#include <cstring>

using namespace hc::detail;

// No implicit fusing of a multiplication into an addition (as hc_wave_kin2.hip): an item's bits are the same in every instantiation
#pragma clang fp contract(off)

namespace hc {
namespace {

struct Wk2DirPairArgs {
    const double* tab;  // [kKinCols + kDirCols][nf]: the table of hc_wave_kin.hpp, then cos and sin of the directions
    int nf;
    int finite_depth;
    double g, depth;
    double cut[4];      // diff_lo, diff_hi, sum_lo, sum_hi
    double* pair;       // [kWk2Tables][nf][nf]
};

// One work item per pair (i, j) of the full matrix; an entry outside its cut-off band is stored as 0.  The evaluation form of
// wk2_pair_kernel with the angle between the two components in it: gamma = cos(beta_i - beta_j) = tau - sigma,
//     k_i . k_j - R_i R_j = gamma (k_i delta_j + R_j delta_i) - 2 sigma R_i R_j
//     k_i . k_j + R_i R_j = gamma (k_i delta_j + R_j delta_i) + 2 tau R_i R_j
// and from them K+- = (D+- - gamma (k_i delta_j + R_j delta_i)) / (r_i r_j) + 2 sigma r_i r_j + {R_i + R_j, (r_i - r_j)^2}.
__global__ void __launch_bounds__(kWk2Threads) wk2_dir_pair_kernel(Wk2DirPairArgs a) {
    const long long n2 = static_cast<long long>(a.nf) * a.nf;
    const long long e  = static_cast<long long>(blockIdx.x) * kWk2Threads + threadIdx.x;
    if (e >= n2) return;
    const int i = static_cast<int>(e / a.nf), j = static_cast<int>(e - static_cast<long long>(i) * a.nf);
    const double Ai = a.tab[kKinAmp * a.nf + i], wi = a.tab[kKinOmega * a.nf + i], ki = a.tab[kKinK * a.nf + i];
    const double Aj = a.tab[kKinAmp * a.nf + j], wj = a.tab[kKinOmega * a.nf + j], kj = a.tab[kKinK * a.nf + j];
    double sig, tau;
    wk2_dir_angle(a.tab[kKinCols * a.nf + i], a.tab[(kKinCols + 1) * a.nf + i], a.tab[kKinCols * a.nf + j], a.tab[(kKinCols + 1) * a.nf + j],
                  sig, tau);
    const double gam = tau - sig;
    const double Ri = wi * wi / a.g, Rj = wj * wj / a.g;
    const double ri = sqrt(Ri), rj = sqrt(Rj);
    const double bb = 0.25 * (Ai * a.g / wi) * (Aj * a.g / wj);
    const double di = ki - Ri, dj = kj - Rj;
    const double gq = gam * (ki * dj + Rj * di), RR = Ri * Rj, rr = ri * rj;
    const double kmR = gq - 2.0 * sig * RR, kpR = gq + 2.0 * tau * RR;  // k_i . k_j -+ R_i R_j
    const double ni = di * (ki + Ri), nj = dj * (kj + Rj);              // k^2 - R^2
    double Kp = 0.0, Km = 0.0, Bp = 0.0, Bm = 0.0;
    if (wk2_in_band(wi, wj, 1, a.cut[2], a.cut[3])) {
        const double rs = ri + rj, ak = sqrt(wk2_dir_kappa2(ki, kj, sig, tau));
        const double T   = ak * (a.finite_depth ? tanh(ak * a.depth) : 1.0);
        const double den = rs * rs - T;
        const double D   = (rs * (ri * nj + rj * ni) + 2.0 * (rs * rs) * kmR) / den;
        Kp = (D - gq) / rr + 2.0 * sig * rr + (Ri + Rj);
        Bp = bb * D / (wi + wj);
    }
    if (wk2_in_band(wi, wj, 0, a.cut[0], a.cut[1])) {
        const double rd = ri - rj;
        double D = 0.0;
        if (wi != wj) {
            const double ak  = sqrt(wk2_dir_kappa2(ki, -kj, sig, tau));
            const double T   = ak * (a.finite_depth ? tanh(ak * a.depth) : 1.0);
            const double den = rd * rd - T;
            D  = (rd * (rj * ni - ri * nj) + 2.0 * (rd * rd) * kpR) / den;
            Bm = bb * D / (wi - wj);
        }
        Km = (D - gq) / rr + 2.0 * sig * rr + rd * rd;
    }
    a.pair[kWk2Kp * n2 + e] = Kp;
    a.pair[kWk2Km * n2 + e] = Km;
    a.pair[kWk2Bp * n2 + e] = Bp;
    a.pair[kWk2Bm * n2 + e] = Bm;
}

struct Wk2DirSumArgs {
    const double* tab;   // [kKinCols + kDirCols][nf]
    int nf;
    int P, T;
    const double* pair;  // [kWk2Tables][nf][nf]
    const int* band;     // [2][nf][2] (wk2_bands)
    const double* xyz;   // [P][3]
    const double* t;     // [T]
    double depth, mwl;
    int finite_depth;
    int sign_on[2];
    int ramped;
    double ramp_duration;
    double* eta;         // [T][P]    } NULL: not wanted
    double* vel;         // [T][P][3] }
    double* acc;         // [T][P][3] }
};

// One workgroup per (point, time) item o = j * P + p: the pair sum (hc_wave_kin2_dir.hpp: wk2_dir_item_sum) at the item's point and
// time, then the ramp.  An item's bits depend on the item, the tables and the options only.
template <bool ETA, bool KIN>
__global__ void __launch_bounds__(kWk2Threads) wk2_dir_sum_kernel(Wk2DirSumArgs a) {
    const long long o = blockIdx.x;
    const int p = static_cast<int>(o % a.P), jt = static_cast<int>(o / a.P);
    const double t = a.t[jt];
    const Wk2Sea sea{a.tab, a.nf, a.pair, a.band, a.depth, a.mwl, a.finite_depth, {a.sign_on[0], a.sign_on[1]}};
    const double* q = a.xyz + 3 * static_cast<size_t>(p);
    double sum[kWk2DirSums];
    wk2_dir_item_sum<ETA, KIN>(sea, q[0], q[1], q[2], t, sum);
    if (threadIdx.x == 0) {
        const double ramp2 = wk2_ramp2(a.ramped != 0, a.ramp_duration, t);  // second order in the amplitude
        if constexpr (ETA) a.eta[o] = 0.25 * sum[0] * ramp2;
        if (KIN && a.vel) {
            a.vel[3 * o]     = sum[1] * ramp2;
            a.vel[3 * o + 1] = sum[2] * ramp2;
            a.vel[3 * o + 2] = sum[3] * ramp2;
        }
        if (KIN && a.acc) {
            a.acc[3 * o]     = sum[4] * ramp2;
            a.acc[3 * o + 1] = sum[5] * ramp2;
            a.acc[3 * o + 2] = sum[6] * ramp2;
        }
    }
}

}  // namespace

// (declared in hc_wave_kin2_dir.hpp)  The rules of wk2_tables: current or absent -- the mark goes first and the stamp last; a
// direction change counts in wave_serial; a set wk2_tables filled is not current here, whatever its stamp says.
void wk2_dir_tables(hc_ctx* c, Wk2TableSet& s, hipStream_t st, const hc_wave_kinematics2_opts& o, bool keep_empty) {
    const double cut[4] = {o.diff_lo, o.diff_hi, o.sum_lo, o.sum_hi};
    if (s.dir && kin_table_current(c, s.serial, s.phase, o.regular_phase) && std::memcmp(s.cut, cut, sizeof(s.cut)) == 0) return;
    s.serial = ~0ULL;  // nothing is cached until all of it is in place
    s.dir    = true;
    std::vector<double> tab = kin_table_host(c, o.regular_phase);
    const int nf = static_cast<int>(tab.size() / kKinCols);
    std::vector<double> dir = kin_dir_columns_host(c);
    if (dir.empty()) {
        dir.assign(static_cast<size_t>(kDirCols) * nf, 0.0);
        std::fill(dir.begin(), dir.begin() + nf, 1.0);
    }
    require(dir.size() == static_cast<size_t>(kDirCols) * nf, HC_ERR_RUNTIME, "the wave directions do not match the component table");
    std::vector<int> band(4 * static_cast<size_t>(nf));
    const double* omega = tab.data() + static_cast<size_t>(kKinOmega) * nf;
    s.any[0] = wk2_bands(omega, nf, 0, cut[0], cut[1], band.data());
    s.any[1] = wk2_bands(omega, nf, 1, cut[2], cut[3], band.data() + 2 * static_cast<size_t>(nf));
    tab.insert(tab.end(), dir.begin(), dir.end());
    s.d_tab.upload(tab, st);
    s.d_band.upload(band, st);
    const size_t n2 = static_cast<size_t>(nf) * nf;
    if (!(s.any[0] || s.any[1]) && !keep_empty) {
        s.d_pair.release();
    } else {
        if (s.d_pair.n != kWk2Tables * n2) s.d_pair.alloc(kWk2Tables * n2);
        Wk2DirPairArgs a{};
        a.tab          = s.d_tab.p;
        a.nf           = nf;
        a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
        a.g            = std::fabs(c->g);
        a.depth        = c->depth;
        std::copy(cut, cut + 4, a.cut);
        a.pair = s.d_pair.p;
        hipLaunchKernelGGL(wk2_dir_pair_kernel, dim3(static_cast<unsigned>((n2 + kWk2Threads - 1) / kWk2Threads)), dim3(kWk2Threads), 0, st, a);
        HC_HIP(hipGetLastError());
        HC_HIP(hipStreamSynchronize(st));
    }
    s.nf    = nf;
    s.phase = o.regular_phase;
    std::copy(cut, cut + 4, s.cut);
    s.serial = c->wave_serial;
}

bool Order2Part::prepare_dir(hc_ctx* c, const SideLane& lane) {
    if (!on || !kin_has_components(c)) return false;
    hc_wave_kinematics2_opts o;
    hc_wave_kinematics2_opts_default(&o);
    o.regular_phase = lane.opts.regular_phase;
    o.diff_lo = cut[0], o.diff_hi = cut[1], o.sum_lo = cut[2], o.sum_hi = cut[3];
    wk2_dir_tables(c, tabs, lane.stream, o, false);
    return tabs.any[0] || tabs.any[1];
}

namespace {

hc_wave_kinematics2_opts wk2_dir_opts(const hc_wave_kinematics2_opts* opts) {
    hc_wave_kinematics2_opts o;
    hc_wave_kinematics2_opts_default(&o);
    if (opts) o = *opts;
    const char* bad = wk2_check_opts(o);
    require(bad == nullptr, HC_ERR_INVALID, bad ? bad : "");
    return o;
}

}  // namespace
}  // namespace hc

extern "C" {

// Touches no step state, so it is not ordered against the direct queue (HC_API_BEGIN_HOT), as hc_wave_kinematics2
int hc_wave_kinematics2_dir(hc_ctx* c, const hc_wave_kinematics2_opts* opts, int n_points, const double* xyz, int n_times, const double* t,
                            double* eta, double* vel, double* acc) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    const hc_wave_kinematics2_opts o = hc::wk2_dir_opts(opts);
    const char* bad = hc::wk2_check_batch(n_points, xyz, n_times, t);
    require(bad == nullptr, HC_ERR_INVALID, bad ? bad : "");
    for (int p = 0; p < n_points; ++p) require(std::isfinite(xyz[3 * static_cast<size_t>(p) + 1]), HC_ERR_INVALID, "non-finite y of a point");
    const bool waves = hc::kin_has_components(c);
    require(!waves || hc::wk2_component_count(c) <= hc::kWk2MaxFreq, HC_ERR_UNSUPPORTED, "more than 4096 wave components");
    const size_t n = static_cast<size_t>(n_points) * n_times;
    if (n == 0 || !(eta || vel || acc)) return HC_OK;
    if (waves) {
        if (!c->stream_wk2d) HC_HIP(hipStreamCreateWithFlags(&c->stream_wk2d, hipStreamNonBlocking));
        hc::wk2_dir_tables(c, c->wk2d, c->stream_wk2d, o, true);
    }
    // NoWave, no model, an imported eta record (no components), or no pair inside either band: zeros, no launch
    if (!waves || !(c->wk2d.any[0] || c->wk2d.any[1])) {
        if (eta) std::fill(eta, eta + n, 0.0);
        if (vel) std::fill(vel, vel + 3 * n, 0.0);
        if (acc) std::fill(acc, acc + 3 * n, 0.0);
        return HC_OK;
    }
    hipStream_t st = c->stream_wk2d;
    // one buffer: points, times, then the requested outputs
    const size_t n_in = 3 * static_cast<size_t>(n_points) + n_times;
    const size_t n_out = (eta ? n : 0) + (vel ? 3 * n : 0) + (acc ? 3 * n : 0);
    if (c->d_wk2d_io.n < n_in + n_out) c->d_wk2d_io.alloc(n_in + n_out);
    double* d_xyz = c->d_wk2d_io.p;
    double* d_t   = d_xyz + 3 * static_cast<size_t>(n_points);
    double* d_out = d_t + n_times;
    hc::Wk2DirSumArgs a{};
    a.tab          = c->wk2d.d_tab.p;
    a.nf           = c->wk2d.nf;
    a.P            = n_points;
    a.T            = n_times;
    a.pair         = c->wk2d.d_pair.p;
    a.band         = c->wk2d.d_band.p;
    a.xyz          = d_xyz;
    a.t            = d_t;
    a.depth        = c->depth;
    a.mwl          = o.mwl;
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    a.sign_on[0]   = c->wk2d.any[0] ? 1 : 0;
    a.sign_on[1]   = c->wk2d.any[1] ? 1 : 0;
    a.ramped        = (o.apply_ramp && hc::kin_synthesised(c) && c->irr.ramp_duration > 0.0) ? 1 : 0;  // the switch only (wk2_ramp2)
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
    const dim3 grid(static_cast<unsigned>(n)), block(hc::kWk2Threads);
    if (!(vel || acc))
        hipLaunchKernelGGL((hc::wk2_dir_sum_kernel<true, false>), grid, block, 0, st, a);
    else if (!eta)
        hipLaunchKernelGGL((hc::wk2_dir_sum_kernel<false, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((hc::wk2_dir_sum_kernel<true, true>), grid, block, 0, st, a);
    HC_HIP(hipGetLastError());
    if (eta) HC_HIP(hipMemcpyAsync(eta, a.eta, n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (vel) HC_HIP(hipMemcpyAsync(vel, a.vel, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (acc) HC_HIP(hipMemcpyAsync(acc, a.acc, 3 * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HC_HIP(hipStreamSynchronize(st));
    HC_API_END(c)
}

int hc_wave_kinematics2_dir_pair_tables(hc_ctx* c, const hc_wave_kinematics2_opts* opts, double* Kp, double* Km, double* Bp, double* Bm) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    const hc_wave_kinematics2_opts o = hc::wk2_dir_opts(opts);
    if (!hc::kin_has_components(c)) return HC_OK;
    require(hc::wk2_component_count(c) <= hc::kWk2MaxFreq, HC_ERR_UNSUPPORTED, "more than 4096 wave components");
    if (!c->stream_wk2d) HC_HIP(hipStreamCreateWithFlags(&c->stream_wk2d, hipStreamNonBlocking));
    hc::wk2_dir_tables(c, c->wk2d, c->stream_wk2d, o, true);
    const size_t n2 = static_cast<size_t>(c->wk2d.nf) * c->wk2d.nf;
    double* out[hc::kWk2Tables] = {Kp, Km, Bp, Bm};
    for (int k = 0; k < hc::kWk2Tables; ++k)
        if (out[k]) HC_HIP(hipMemcpyAsync(out[k], c->wk2d.d_pair.p + k * n2, n2 * sizeof(double), hipMemcpyDeviceToHost, c->stream_wk2d));
    HC_HIP(hipStreamSynchronize(c->stream_wk2d));
    HC_API_END(c)
}

}  // extern "C"
