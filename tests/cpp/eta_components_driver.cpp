// The host half of the component analysis of an imported eta record (hydrochrono_amd/csrc/hc_eta_components.hpp) without a GPU: the
// uniformity test, the resampling, the band, the modular phase, the origin rotation and the selection.  Built with plain g++ by
// tests/test_eta_components_cpu.py, once more with -fsanitize=address,undefined.
//   usage: eta_components_driver grid   <file>                         "h <h>", "uniform <0|1>", then the n values on the uniform grid
//          eta_components_driver bins   <n> <T_w> <f_min> <f_max>      "<m_lo> <m_hi>"  (empty band: m_lo > m_hi)
//          eta_components_driver phase  <n> <m> <s> <stride> <count>   (m j) mod n for j = s, s + stride, ... (count values)
//          eta_components_driver rotate <re> <im> <m> <T_w> <t0>       "<re> <im>" of c exp(i 2 pi m t0 / T_w)
//          eta_components_driver select <max_components> <A_0> <A_1> ..  the kept positions, ascending
// Numbers are printed with %.17g.  Exit 0 on success, 1 on an error line, 2 on bad usage.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hydrochrono_amd/csrc/hc_eta_components.hpp"
#include "../../hydrochrono_amd/csrc/hc_eta_record.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "grid" && argc >= 3) {
        std::vector<double> t, eta;
        std::string err = hc::read_eta_file(argv[2], t, eta);
        if (err.empty()) err = hc::validate_eta_record(t.data(), eta.data(), static_cast<long long>(t.size()));
        if (!err.empty()) {
            std::printf("error %s\n", err.c_str());
            return 1;
        }
        const long long n = static_cast<long long>(t.size());
        const double h    = hc::eta_mean_spacing(t.data(), n);
        const bool uni    = hc::eta_grid_uniform(t.data(), n, h);
        std::printf("h %.17g\nuniform %d\n", h, uni ? 1 : 0);
        const std::vector<double> v = uni ? eta : hc::eta_resample_uniform(t.data(), eta.data(), n, h);
        for (double x : v) std::printf("%.17g\n", x);
        return 0;
    }
    if (mode == "bins" && argc >= 6) {
        long long lo = 0, hi = 0;
        hc::eta_band_bins(std::atoll(argv[2]), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5]), &lo, &hi);
        std::printf("%lld %lld\n", lo, hi);
        return 0;
    }
    if (mode == "phase" && argc >= 7) {
        const unsigned long long n = std::strtoull(argv[2], nullptr, 10), m = std::strtoull(argv[3], nullptr, 10);
        const unsigned long long s = std::strtoull(argv[4], nullptr, 10), stride = std::strtoull(argv[5], nullptr, 10);
        const long long count      = std::atoll(argv[6]);
        const unsigned long long inc = hc::eta_phase_start(m, stride, n);
        unsigned long long r         = hc::eta_phase_start(m, s, n);
        for (long long i = 0; i < count; ++i) {
            std::printf("%llu\n", r);
            r = hc::eta_phase_next(r, inc, n);
        }
        return 0;
    }
    if (mode == "rotate" && argc >= 7) {
        double re = 0.0, im = 0.0;
        hc::eta_rotate_origin(std::atof(argv[2]), std::atof(argv[3]), std::atoll(argv[4]), std::atof(argv[5]), std::atof(argv[6]), &re, &im);
        std::printf("%.17g %.17g\n", re, im);
        return 0;
    }
    if (mode == "select" && argc >= 3) {
        std::vector<double> amp;
        for (int i = 3; i < argc; ++i) amp.push_back(std::atof(argv[i]));
        for (long long k : hc::eta_select_components(amp.data(), static_cast<long long>(amp.size()), std::atoll(argv[2]))) std::printf("%lld\n", k);
        return 0;
    }
    return 2;
}
