// hc_tail.hpp -- index arithmetic of the spectral radiation tail (host only; no HIP dependency, so that a CPU test can check it:
// tests/test_spectral_tail_cpu.py).
//
// On the common grid (step = IRF spacing) the lags s >= P of the radiation sum of step m,  sum_s G_s v_{m-s}  with G_s = w_s K_s,
// are an ordinary linear convolution with the velocity sequence.  They are evaluated by uniformly partitioned overlap-save: the P
// steps of a SUPERBLOCK (steps m0 .. m0 + P - 1, m0 = the first step of an at-start look-ahead block) take partition p = 1 .. NP,
// the lags [pP, (p+1)P), as one circular convolution of size N = 2P:
//     y_p[n] = sum_r h_p[r] x_p[(n - r) mod N],   h_p[r] = G_{pP + r} (zero where pP + r >= S or r >= P),
//     x_p[k] = v_{m0 - (p+1)P + k},               k = 0 .. N - 1,
// whose outputs n = P + j (j = 0 .. P - 1) are partition p's share of step m0 + j (no wrap-around reaches them).  In the frequency
// domain that is Y[bin] = sum_p Khat_p[bin] Xhat_p[bin] over the P + 1 bins of a real transform; its inverse gives the whole tail.
// Every x_p[k] is a sample older than m0, i.e. known when the superblock starts.
#pragma once
#include <algorithm>
#include <cmath>
#include <deque>
#include <limits>
#include <vector>

namespace hc {

constexpr int kTailP    = 256;          // lags per partition = steps per superblock
constexpr int kTailN    = 2 * kTailP;   // transform size
constexpr int kTailBins = kTailP + 1;   // bins of a real transform of size kTailN
constexpr int kTailMaxCols = 4096;      // K-hat columns a row may have (NP * D): X-hat of one bin is staged in LDS (64 KB)

// Tail partitions p = 1 .. NP (lags P .. S - 1); 0: no tail (S < 2P keeps the full pass).
inline int tail_partitions(int S) { return S >= 2 * kTailP ? (S + kTailP - 1) / kTailP - 1 : 0; }

// Look-ahead blocks per superblock.
inline int tail_blocks_per_superblock(int lookahead) { return lookahead > 0 ? kTailP / lookahead : 0; }

// Far chunks: bins [lo, hi) of sum_{p >= 2} Khat_p Xhat_p for the NEXT superblock, one per block of a superblock but its first (which
// already carries the near partition and the transforms): chunk k = 0 .. Q - 2 goes with block k + 1.
inline int tail_far_chunks(int Q) { return Q > 1 ? Q - 1 : 1; }
inline void tail_chunk_bins(int k, int nchunks, int* lo, int* hi) {
    *lo = static_cast<int>(static_cast<long long>(k) * kTailBins / nchunks);
    *hi = static_cast<int>(static_cast<long long>(k + 1) * kTailBins / nchunks);
}

// Input windows, computed at every superblock start from the history ring: window a = 1 .. NP holds
//     x[k] = v_{m0 - (a+1)P + k},  i.e. the sample tail_window_back(a, k) behind the newest one (0 = the sample of step m0 - 1).
// Window a is x_1 of this superblock for a = 1, and x_p of the NEXT superblock for p = a + 1 (far chunks); a fallback that has to
// complete this superblock's far part takes x_p = window p.  Samples no output needs are zero: x[0] (it only reaches the outputs
// n < P) and everything older than the oldest sample of the IRF window (it only meets zero-padded lags).
inline int tail_window_back(int a, int k) { return (a + 1) * kTailP - 1 - k; }
inline bool tail_window_live(int S, int a, int k) { return k >= 1 && tail_window_back(a, k) <= S - 2; }

// K-hat column of (partition p >= 1, DoF col): rows are [bin][row][(p - 1) * D + col]; X-hat is [bin][(a - 1) * D + col].
inline int tail_col(int p, int col, int D) { return (p - 1) * D + col; }
// shift from a K-hat column to the X-hat column it meets: 0 for this superblock (x_p = window p), -D for the next one (x_p = window p - 1)
inline int tail_x_shift(bool next_superblock, int D) { return next_superblock ? -D : 0; }

// May the blocks of a superblock that starts at the block just planned take their lags s >= P from the tail?  The history is the
// uniform grid of the step (times[k] = times[0] - k dt, k < S: the samples the windows read), the IRF grid is that grid too (tau_s = s dt), and the history
// reaches past the oldest query of the block (every IRF sample has an older history sample, as far_pass_allowed asks).
// t_first: the first predicted step of the block.  The tolerance is the planner's (plan_step).
inline bool tail_grid_ok(const std::deque<double>& times, const std::vector<double>& tau, double dt, double t_first) {
    const int S = static_cast<int>(tau.size());
    if (tail_partitions(S) < 1 || !(dt > 0.0) || static_cast<int>(times.size()) < S) return false;
    const double tol_t = std::max(1e-9 * dt, 64.0 * std::numeric_limits<double>::epsilon() * std::fabs(t_first));
    if (std::fabs(t_first - (times[0] + dt)) > tol_t) return false;
    for (int k = 1; k < S; ++k)
        if (std::fabs(times[static_cast<size_t>(k)] - (times[0] - k * dt)) > tol_t) return false;
    const double tol_s = std::max(1e-9 * dt, 64.0 * std::numeric_limits<double>::epsilon() * std::fabs(tau.back()));
    for (int s = 0; s < S; ++s)
        if (std::fabs(tau[static_cast<size_t>(s)] - s * dt) > tol_s) return false;
    const double margin = 8.0 * tol_t;
    return t_first - times.back() > tau.back() + margin;
}

}  // namespace hc
