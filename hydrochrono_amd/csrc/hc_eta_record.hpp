// hc_eta_record.hpp -- imported free-surface elevation records (hc_read_eta_file, hc_set_wave_irregular_eta).  Host only, no HIP:
// tests/cpp/eta_record_driver.cpp compiles it with plain g++.
//
//   parse_eta_lines      IrregularWaves::ReadEtaFromFile (src/wave_types.cpp:480-500): per line `ss >> time >> delimiter >> eta`, the
//                        delimiter must be ':', anything after the value is ignored; the reference's messages.
//   validate_eta_record  n >= 2, times finite and strictly increasing, values finite.
//   extend_eta_record    the table the kernels interpolate in: the record with eta = 0 samples on both sides, spaced by the record's
//                        mean spacing h = (t[n-1] - t[0]) / (n-1), ceil(max(tau_max, 0) / h) + 1 of them before the record and
//                        ceil(max(-tau_min, 0) / h) + 1 after it -- enough for every step time in [t[0], t[n-1]] against an excitation
//                        IRF on [tau_min, tau_max].
#pragma once

#include <algorithm>
#include <cmath>
#include <fstream>
#include <istream>
#include <sstream>
#include <string>
#include <vector>

namespace hc {

// Reads "time : eta" lines from `in` until its end.  Returns "" on success, else the reference's message for the first bad line.
inline std::string parse_eta_lines(std::istream& in, std::vector<double>& t, std::vector<double>& eta) {
    std::string line;
    double time = 0.0, value = 0.0;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        char delimiter = 0;
        if (!(ss >> time >> delimiter >> value) || delimiter != ':') return "Could not parse line: " + line + ".";
        t.push_back(time);
        eta.push_back(value);
    }
    return "";
}

inline std::string read_eta_file(const std::string& path, std::vector<double>& t, std::vector<double>& eta) {
    std::ifstream file(path);
    if (!file) return "Unable to open file at: " + path + ".";
    return parse_eta_lines(file, t, eta);
}

// "" when (t, eta) is a usable record, else what is wrong with it
inline std::string validate_eta_record(const double* t, const double* eta, long long n) {
    if (n < 2) return "an eta record needs at least two samples";
    if (!t || !eta) return "null eta record";
    for (long long i = 0; i < n; ++i) {
        if (!std::isfinite(t[i]) || !std::isfinite(eta[i])) return "eta record sample " + std::to_string(i) + " is not finite";
        if (i > 0 && !(t[i] > t[i - 1])) return "eta record times must be strictly increasing (sample " + std::to_string(i) + ")";
    }
    if (!std::isfinite(t[n - 1] - t[0])) return "eta record spans more than the double range";
    return "";
}

struct EtaExtended {
    std::vector<double> t, eta;  // n_front zeros | the record | n_back zeros
    double h = 0.0;              // mean spacing of the record (the kernels' search hint)
    long long n_front = 0, n_back = 0;
};

// (t, eta) must have passed validate_eta_record
inline EtaExtended extend_eta_record(const double* t, const double* eta, long long n, double tau_min, double tau_max) {
    EtaExtended x;
    x.h       = (t[n - 1] - t[0]) / static_cast<double>(n - 1);
    x.n_front = static_cast<long long>(std::ceil(std::max(tau_max, 0.0) / x.h)) + 1;
    x.n_back  = static_cast<long long>(std::ceil(std::max(-tau_min, 0.0) / x.h)) + 1;
    const size_t total = static_cast<size_t>(x.n_front + n + x.n_back);
    x.t.reserve(total);
    x.eta.assign(total, 0.0);
    for (long long k = x.n_front; k >= 1; --k) x.t.push_back(t[0] - static_cast<double>(k) * x.h);
    x.t.insert(x.t.end(), t, t + n);
    for (long long k = 1; k <= x.n_back; ++k) x.t.push_back(t[n - 1] + static_cast<double>(k) * x.h);
    for (long long i = 0; i < n; ++i) x.eta[static_cast<size_t>(x.n_front + i)] = eta[i];
    return x;
}

}  // namespace hc
