// hc_eta_components.hpp -- the host parts of the component analysis of an imported eta record (hc_set_eta_record_components,
// hc_eta_components.hip).  Host only, no HIP: tests/cpp/eta_components_driver.cpp compiles it with plain g++.
//
//   eta_grid_uniform       |t[j] - (t[0] + j h)| <= 1e-9 h for every j, h = (t[n-1] - t[0]) / (n-1) the mean spacing.
//   eta_resample_uniform   the record's piecewise-linear interpolant (the one the excitation path reads, hc_kernels.hip: eta_interp)
//                          at t[0] + j h, j = 0 .. n-1.
//   eta_band_bins          the bins 1 <= m <= n/2 with f_min <= m / T_w <= f_max, T_w = n h: one run [m_lo, m_hi], empty: m_lo > m_hi.
//   eta_phase_start / _next  (m j) mod n for j = s, s + stride, ... in 64-bit integers: the angle 2 pi ((m j) mod n) / n is exact
//                          before sincos whatever n and m are.  Shared with the kernel.
//   eta_rotate_origin      c exp(i w_m t0): the coefficient taken against sample 0 turned to the absolute time origin; the product
//                          w_m t0 is formed and reduced in long double (in cycles: m t0 / T_w minus its integer part).
//   eta_select_components  the max_components candidates of largest amplitude (ties: the lower bin), in ascending bin order.
#pragma once

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#define HC_ETA_HD __host__ __device__
#else
#define HC_ETA_HD
#endif

namespace hc {

constexpr double kEtaUniformTol = 1e-9;  // of the mean spacing

inline double eta_mean_spacing(const double* t, long long n) { return (t[n - 1] - t[0]) / static_cast<double>(n - 1); }

inline bool eta_grid_uniform(const double* t, long long n, double h) {
    for (long long j = 0; j < n; ++j)
        if (!(std::fabs(t[j] - (t[0] + static_cast<double>(j) * h)) <= kEtaUniformTol * h)) return false;
    return true;
}

// (t, eta) must have passed validate_eta_record (hc_eta_record.hpp)
inline std::vector<double> eta_resample_uniform(const double* t, const double* eta, long long n, double h) {
    std::vector<double> out(static_cast<size_t>(n));
    long long idx = 0;
    for (long long j = 0; j < n; ++j) {
        const double q = std::min(t[0] + static_cast<double>(j) * h, t[n - 1]);  // (the last point may round past the record's end)
        while (idx < n - 2 && t[idx + 1] <= q) ++idx;
        const double t1 = t[idx], t2 = t[idx + 1], e1 = eta[idx], e2 = eta[idx + 1];
        if (q == t1) {
            out[static_cast<size_t>(j)] = e1;
        } else if (q == t2) {
            out[static_cast<size_t>(j)] = e2;
        } else {
            const double w1 = (t2 - q) / (t2 - t1);
            const double w2 = 1.0 - w1;
            out[static_cast<size_t>(j)] = w1 * e1 + w2 * e2;
        }
    }
    return out;
}

// the frequency of bin m as every layer states it
inline double eta_bin_frequency(long long m, double T_w) { return static_cast<double>(m) / T_w; }

inline void eta_band_bins(long long n, double T_w, double f_min, double f_max, long long* m_lo, long long* m_hi) {
    const long long top = n / 2;
    const auto in_lo   = [&](long long m) { return f_min <= eta_bin_frequency(m, T_w); };
    const auto in_hi   = [&](long long m) { return eta_bin_frequency(m, T_w) <= f_max; };
    // both tests are monotone in m: a guess from the product, then steps to the exact boundary of the comparison itself
    const auto guess = [&](double f) { return static_cast<long long>(std::min(std::max(f * T_w, 0.0), static_cast<double>(top) + 1.0)); };
    long long lo = std::max(1LL, guess(f_min));
    while (lo > 1 && in_lo(lo - 1)) --lo;
    while (lo <= top && !in_lo(lo)) ++lo;
    long long hi = std::min(top, guess(f_max));
    while (hi < top && in_hi(hi + 1)) ++hi;
    while (hi >= 1 && !in_hi(hi)) --hi;
    *m_lo = lo;
    *m_hi = hi;
}

// (m j) mod n along j = s, s + stride, ...: m <= n / 2 and s, stride < 2^31 keep every product below 2^63
HC_ETA_HD inline unsigned long long eta_phase_start(unsigned long long m, unsigned long long s, unsigned long long n) { return (m * s) % n; }
HC_ETA_HD inline unsigned long long eta_phase_next(unsigned long long r, unsigned long long step, unsigned long long n) {
    r += step;  // step = (m stride) mod n < n
    return r >= n ? r - n : r;
}

inline void eta_rotate_origin(double re, double im, long long m, double T_w, double t0, double* out_re, double* out_im) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    long double cycles       = static_cast<long double>(m) * static_cast<long double>(t0) / static_cast<long double>(T_w);
    cycles -= std::floor(cycles);
    const long double ang = two_pi * cycles, cs = std::cos(ang), sn = std::sin(ang);
    const long double r = re, i = im;
    *out_re = static_cast<double>(r * cs - i * sn);
    *out_im = static_cast<double>(r * sn + i * cs);
}

// positions (into the candidate list) of the kept components, ascending
inline std::vector<long long> eta_select_components(const double* amp, long long n_cand, long long max_components) {
    std::vector<long long> idx(static_cast<size_t>(n_cand));
    std::iota(idx.begin(), idx.end(), 0LL);
    if (max_components <= 0 || max_components >= n_cand) return idx;
    std::stable_sort(idx.begin(), idx.end(), [&](long long a, long long b) { return amp[a] > amp[b]; });  // stable: ties keep the lower bin first
    idx.resize(static_cast<size_t>(max_components));
    std::sort(idx.begin(), idx.end());
    return idx;
}

}  // namespace hc
