// Prints the index arithmetic of the spectral radiation tail (hydrochrono_amd/csrc/hc_tail.hpp) for one (S, depth), so that
// tests/test_spectral_tail_cpu.py can run an overlap-save convolution with it in NumPy.
//   tail_index_dump S L D   the partitions, far chunks, windows, K-hat columns and X-hat shifts
//   tail_index_dump grid    reads "n_times n_tau times... tau... dt t_first" from stdin, prints tail_grid_ok's verdict (1 / 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "../../hydrochrono_amd/csrc/hc_tail.hpp"

static int grid_mode() {
    int nt = 0, ns = 0;
    if (std::scanf("%d %d", &nt, &ns) != 2 || nt < 0 || ns < 0) return 2;
    std::deque<double> times(static_cast<size_t>(nt));
    std::vector<double> tau(static_cast<size_t>(ns));
    for (auto& x : times)
        if (std::scanf("%lf", &x) != 1) return 2;
    for (auto& x : tau)
        if (std::scanf("%lf", &x) != 1) return 2;
    double dt = 0.0, t_first = 0.0;
    if (std::scanf("%lf %lf", &dt, &t_first) != 2) return 2;
    std::printf("%d\n", hc::tail_grid_ok(times, tau, dt, t_first) ? 1 : 0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "grid") == 0) return grid_mode();
    if (argc < 4) return 2;
    const int S = std::atoi(argv[1]), L = std::atoi(argv[2]), D = std::atoi(argv[3]);
    const int NP = hc::tail_partitions(S), Q = hc::tail_blocks_per_superblock(L);
    std::printf("P %d N %d bins %d NP %d Q %d\n", hc::kTailP, hc::kTailN, hc::kTailBins, NP, Q);
    for (int k = 0; k < hc::tail_far_chunks(Q); ++k) {
        int lo, hi;
        hc::tail_chunk_bins(k, hc::tail_far_chunks(Q), &lo, &hi);
        std::printf("chunk %d %d %d\n", k, lo, hi);
    }
    for (int a = 1; a <= NP; ++a)
        for (int k = 0; k < hc::kTailN; ++k) std::printf("win %d %d %d %d\n", a, k, hc::tail_window_back(a, k), hc::tail_window_live(S, a, k) ? 1 : 0);
    for (int p = 1; p <= NP; ++p)
        for (int c = 0; c < D; ++c) std::printf("col %d %d %d\n", p, c, hc::tail_col(p, c, D));
    std::printf("shift %d %d\n", hc::tail_x_shift(false, D), hc::tail_x_shift(true, D));
    return 0;
}
