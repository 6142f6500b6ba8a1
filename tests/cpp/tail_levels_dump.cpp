// Prints the level arithmetic of the spectral radiation tail (hydrochrono_amd/csrc/hc_tail.hpp: tail_levels and the tail_level_*
// functions) for one (S, depth, form), so that tests/test_spectral_tail_levels_cpu.py can check the level set and run the levelled
// overlap-save convolution with it in NumPy.
//   tail_levels_dump S L form     form: 1 levelled, 2 uniform
#include <cstdio>
#include <cstdlib>

#include "../../hydrochrono_amd/csrc/hc_tail.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int S = std::atoi(argv[1]), L = std::atoi(argv[2]), form = std::atoi(argv[3]);
    hc::TailLevel lv[hc::kTailLevelsMax];
    const int n = hc::tail_levels(S, form, lv);
    std::printf("levels %d head %d\n", n, hc::tail_head_lags(lv, n));
    for (int i = 0; i < n; ++i) {
        const hc::TailLevel& v = lv[i];
        std::printf("level %d P %d N %d bins %d lag_lo %d lag_hi %d NP %d period %d blocks %d far_ahead %d\n", i, v.P, v.N, v.bins, v.lag_lo, v.lag_hi, v.NP, v.period,
                    hc::tail_level_blocks(v, L), hc::tail_level_far_ahead(v) ? 1 : 0);
        for (int j = 0; j < lv[0].period; j += L)
            if (hc::tail_level_starts(v, j)) std::printf("start %d %d\n", i, j);
        const int Q = hc::tail_level_blocks(lv[0], L), nch = hc::tail_far_chunks(Q);
        if (hc::tail_level_far_ahead(v))
            for (int k = 0; k < nch; ++k) {
                int lo, hi;
                hc::tail_level_chunk_bins(v, k, nch, &lo, &hi);
                std::printf("chunk %d %d %d %d\n", i, k, lo, hi);
            }
        for (int a = 1; a <= v.NP; ++a)
            for (int k = 0; k < v.N; ++k) std::printf("win %d %d %d %d %d\n", i, a, k, hc::tail_level_window_back(v, a, k), hc::tail_level_window_live(v, S, a, k) ? 1 : 0);
        for (int p = 1; p <= v.NP; ++p)
            for (int r = 0; r < v.N; ++r) std::printf("tap %d %d %d %d %d\n", i, p, r, hc::tail_level_lag(v, p, r), hc::tail_level_tap_live(v, S, p, r) ? 1 : 0);
    }
    return 0;
}
