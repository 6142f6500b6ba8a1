// hc_wave_kin2.hpp -- the host side of the second-order wave kinematics (hc_wave_kin2.hip): argument validation, the band test the
// pair kernel shares, and the band limits of the pair matrix.  No HIP dependency: tests/cpp/wave_kin2_host_check.cpp exercises it
// in a plain host build.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/hydrochrono_amd.h"
#include "hc_limits.hpp"

namespace hc {

constexpr int kWk2MaxFreq = 4096;  // components: the four pair tables take 4 nf^2 doubles (537 MB at 4096)
// (point, time) pairs per call: one workgroup each, and the limit of hc_wave_kinematics
constexpr long long kWk2MaxItems = (1LL << 31) - 256;

// NULL when the call's arguments are valid, else what is wrong with them (HC_ERR_INVALID)
inline const char* wk2_check_opts(const hc_wave_kinematics2_opts& o) {
    if (!std::isfinite(o.mwl) || !std::isfinite(o.regular_phase)) return "non-finite mwl or regular_phase";
    // (a NaN fails every comparison)
    if (!(o.diff_lo >= 0.0) || !(o.diff_hi >= 0.0) || !(o.sum_lo >= 0.0) || !(o.sum_hi >= 0.0)) return "negative or NaN cut-off frequency";
    if (o.diff_lo > o.diff_hi || o.sum_lo > o.sum_hi) return "cut-off band with lo > hi";
    return nullptr;
}

inline const char* wk2_check_batch(int n_points, const double* xyz, int n_times, const double* t) {
    if (n_points < 0 || n_times < 0) return "negative point or time count";
    if ((n_points > 0 && !xyz) || (n_times > 0 && !t)) return "null points or times";
    for (int p = 0; p < n_points; ++p)
        if (!std::isfinite(xyz[3 * static_cast<size_t>(p)]) || !std::isfinite(xyz[3 * static_cast<size_t>(p) + 2])) return "non-finite x or z of a point";
    for (int j = 0; j < n_times; ++j)
        if (!std::isfinite(t[j])) return "non-finite time";
    if (static_cast<long long>(n_points) * n_times > kWk2MaxItems) return "too many (point, time) pairs for one call";
    return nullptr;
}

// The frequency a cut-off band is compared with: |w_i - w_j| (sign 0) or w_i + w_j (sign 1).  One expression for the pair kernel
// and the band limits below, symmetric in (i, j) bit for bit.
HC_HOST_DEVICE inline double wk2_pair_omega(double wi, double wj, int sign) { return sign ? wi + wj : std::fabs(wi - wj); }
HC_HOST_DEVICE inline bool wk2_in_band(double wi, double wj, int sign, double lo, double hi) {
    const double v = wk2_pair_omega(wi, wj, sign);
    return v >= lo && v <= hi;
}

// band[i][0..1]: first and last column j >= i of row i inside [lo, hi] (first > last: none), for frequencies in ascending order
// -- both pair frequencies then grow with j, so the band of a row is one run of columns.  Frequencies in any other order: every
// row gets [i, nf - 1] (the pair tables hold zeros outside the band, so the sums stay right and only the saving is lost).
// Returns whether any pair is inside.
inline bool wk2_bands(const double* omega, int nf, int sign, double lo, double hi, int* band) {
    bool sorted = true;
    for (int i = 1; i < nf; ++i) sorted = sorted && omega[i] >= omega[i - 1];
    bool any = false;
    for (int i = 0; i < nf; ++i) {
        int first = i, last = nf - 1;
        if (sorted) {
            int a = i, b = nf;  // first j in [i, nf) with pair frequency >= lo
            while (a < b) {
                const int m = a + (b - a) / 2;
                if (wk2_pair_omega(omega[i], omega[m], sign) >= lo) b = m; else a = m + 1;
            }
            first = a;
            a = i, b = nf;  // first j in [i, nf) with pair frequency > hi
            while (a < b) {
                const int m = a + (b - a) / 2;
                if (wk2_pair_omega(omega[i], omega[m], sign) > hi) b = m; else a = m + 1;
            }
            last = a - 1;
            any = any || first <= last;
        } else {
            for (int j = i; j < nf; ++j) any = any || wk2_in_band(omega[i], omega[j], sign, lo, hi);
        }
        band[2 * i]     = first;
        band[2 * i + 1] = last;
    }
    return any;
}

// ramp * ramp's switch: that of kin_ramp (hc_wave_kin.hpp: kin_synthesised, ramp_duration > 0); the factor itself is taken per
// time: 0 for t <= 0, (t / ramp_duration)^2 for t < ramp_duration, else 1
HC_HOST_DEVICE inline double wk2_ramp2(bool ramped, double ramp_duration, double t) {
    if (!ramped || !(t < ramp_duration)) return 1.0;
    const double r = t <= 0.0 ? 0.0 : t / ramp_duration;
    return r * r;
}

}  // namespace hc
