// Stand-alone caller of hc::spreading_directions (hc_host_math.cpp): prints nf directions, one per line with 17 digits.
//   spreading_driver nf heading s n_bins seed
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>
#include "hc_host_math.hpp"
int main(int argc, char** argv) {
    if (argc != 6) return 2;
    try {
        const std::vector<double> th = hc::spreading_directions(std::atoi(argv[1]), std::atof(argv[2]), std::atof(argv[3]), std::atoi(argv[4]),
                                                                std::strtoull(argv[5], nullptr, 10));
        for (double v : th) std::printf("%.17g\n", v);
    } catch (const std::invalid_argument& e) {
        std::printf("invalid: %s\n", e.what());
        return 3;
    }
    return 0;
}
