// Stand-alone check of the host side of the second-order wave kinematics (hydrochrono_amd/csrc/hc_wave_kin2.hpp): the argument
// validation and the band limits of the pair matrix against a brute-force scan.  Built with -fsanitize=address,undefined and run
// by tests/test_wave_kin2_host.py; needs no GPU and no library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../hydrochrono_amd/csrc/hc_wave_kin2.hpp"

namespace {
int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

hc_wave_kinematics2_opts defaults() {
    hc_wave_kinematics2_opts o;
    o.mwl = o.regular_phase = 0.0;
    o.diff_lo = o.sum_lo = 0.0;
    o.diff_hi = o.sum_hi = HUGE_VAL;
    o.apply_ramp         = 1;
    return o;
}

void check_bands(const std::vector<double>& w, int sign, double lo, double hi) {
    const int nf = static_cast<int>(w.size());
    std::vector<int> band(2 * w.size() + 2, -7);  // two guard words behind the rows
    const bool any = hc::wk2_bands(w.data(), nf, sign, lo, hi, band.data());
    CHECK(band[2 * w.size()] == -7 && band[2 * w.size() + 1] == -7);
    bool sorted = true;
    for (int i = 1; i < nf; ++i) sorted = sorted && w[i] >= w[i - 1];
    bool brute_any = false;
    for (int i = 0; i < nf; ++i) {
        const int first = band[2 * i], last = band[2 * i + 1];
        CHECK(first >= i && first <= nf && last >= i - 1 && last < nf);
        for (int j = i; j < nf; ++j) {
            const bool in = hc::wk2_in_band(w[i], w[j], sign, lo, hi);
            brute_any = brute_any || in;
            if (sorted)
                CHECK(in == (j >= first && j <= last));  // the band is exactly the run of columns inside
            else
                CHECK(!in || (j >= first && j <= last));  // unsorted: every column inside is covered
            CHECK(in == hc::wk2_in_band(w[j], w[i], sign, lo, hi));
        }
    }
    CHECK(any == brute_any);
}
}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- options ----
    CHECK(hc::wk2_check_opts(defaults()) == nullptr);
    for (int field = 0; field < 6; ++field)
        for (double bad : {nan, -1.0, -inf}) {
            hc_wave_kinematics2_opts o = defaults();
            double* f[6] = {&o.mwl, &o.regular_phase, &o.diff_lo, &o.diff_hi, &o.sum_lo, &o.sum_hi};
            if (field < 2 && bad == -1.0) continue;  // a negative mwl or phase is fine
            *f[field] = bad;
            CHECK(hc::wk2_check_opts(o) != nullptr);
        }
    {
        hc_wave_kinematics2_opts o = defaults();
        o.diff_lo = 0.5, o.diff_hi = 0.25;
        CHECK(hc::wk2_check_opts(o) != nullptr);
        o.diff_hi = 0.5;  // lo == hi is a band
        CHECK(hc::wk2_check_opts(o) == nullptr);
        o.sum_lo = inf;  // [inf, inf]: valid and empty
        CHECK(hc::wk2_check_opts(o) == nullptr);
        o.mwl = inf;
        CHECK(hc::wk2_check_opts(o) != nullptr);
    }
    // ---- batches ----
    const double xyz[6] = {0.0, nan, -1.0, 2.0, 0.0, 0.0}, t[2] = {0.0, 1.0};  // (y does not enter)
    CHECK(hc::wk2_check_batch(2, xyz, 2, t) == nullptr);
    CHECK(hc::wk2_check_batch(0, nullptr, 0, nullptr) == nullptr);
    CHECK(hc::wk2_check_batch(0, nullptr, 2, t) == nullptr);
    CHECK(hc::wk2_check_batch(-1, xyz, 2, t) != nullptr);
    CHECK(hc::wk2_check_batch(2, xyz, -1, t) != nullptr);
    CHECK(hc::wk2_check_batch(2, nullptr, 2, t) != nullptr);
    CHECK(hc::wk2_check_batch(2, xyz, 2, nullptr) != nullptr);
    const double bad_x[3] = {inf, 0.0, 0.0}, bad_z[3] = {0.0, 0.0, nan}, bad_t[1] = {nan};
    CHECK(hc::wk2_check_batch(1, bad_x, 1, t) != nullptr);
    CHECK(hc::wk2_check_batch(1, bad_z, 1, t) != nullptr);
    CHECK(hc::wk2_check_batch(1, xyz, 1, bad_t) != nullptr);
    CHECK(hc::wk2_check_batch(0, nullptr, 2147483647, nullptr) != nullptr);  // null times
    // ---- bands ----
    std::vector<double> w;
    for (int i = 0; i < 67; ++i) w.push_back(0.2 + 0.09 * i + 0.001 * (i % 3));
    std::vector<double> dup = w;
    dup[10] = dup[9];  // a repeated frequency
    dup[11] = dup[9];
    std::vector<double> unsorted = w;
    unsorted[20] = 0.1;
    const double cuts[][2] = {{0.0, inf}, {0.0, 0.0}, {0.05, 0.9}, {0.09, 0.09}, {1.5, 6.0}, {100.0, 200.0}, {0.0, 0.3}, {inf, inf}, {12.0, inf}};
    for (const auto& c : cuts)
        for (int sign = 0; sign < 2; ++sign) {
            check_bands(w, sign, c[0], c[1]);
            check_bands(dup, sign, c[0], c[1]);
            check_bands(unsorted, sign, c[0], c[1]);
            check_bands({0.7}, sign, c[0], c[1]);
            check_bands({}, sign, c[0], c[1]);
        }
    // ---- ramp ----
    CHECK(hc::wk2_ramp2(false, 20.0, 5.0) == 1.0);
    CHECK(hc::wk2_ramp2(true, 20.0, -1.0) == 0.0 && hc::wk2_ramp2(true, 20.0, 0.0) == 0.0);
    CHECK(hc::wk2_ramp2(true, 20.0, 5.0) == 0.0625 && hc::wk2_ramp2(true, 20.0, 20.0) == 1.0 && hc::wk2_ramp2(true, 20.0, 50.0) == 1.0);
    std::printf("wave_kin2 host check: %d failures\n", failures);
    return failures ? 1 : 0;
}
