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

// ---- levels (Gardner's non-uniform partitioning, cut off at 128 lags) -------------------------------------------------------------
// A uniform scheme streams every partition's K-hat once per P steps: 2 P / P = 2 "units" of K per step and partition, whatever P is,
// so lags are cheapest in the LARGEST partition whose input is known in time.  A level is the uniform scheme above with its own
// partition length P: transform size N = 2P, bins = P + 1, a period of P steps, NP partitions p = 1 .. NP over the lags
// [pP, (p+1)P), i.e. the lags [lag_lo, lag_hi) = [P, min(S, (NP + 1) P)).  A level whose lags stop at 2P (NP = 1) leaves the lags
// from 2P on to the level above it.  The levelled form of a window of S lags:
//     S >= 1024:        P = 512 with NP = ceil(S / 512) - 1 (lags 512 .. S - 1),  P = 256 (lags 256 .. 511),  P = 128 (lags 128 .. 255)
//     512 <= S < 1024:  P = 256 with NP = tail_partitions(S) (lags 256 .. S - 1, the uniform scheme as it is),  P = 128 (lags 128 .. 255)
// and the head pass keeps the lags below 128 (below that a direct pass streams no more than a transform: P / lookahead <= 2 units at
// P = 64).  The uniform form is the single level P = 256 with all its partitions, head pass below 256.
// All periods start together at the start of the largest one: at step offset j of the top period the level P starts a period iff
// j % P == 0.  Windows, the zero rule, K-hat / X-hat columns and far chunks are those above with the level's P for kTailP.
struct TailLevel {
    int P, N, bins;  // lags per partition, transform size 2P, bins P + 1 of a real transform
    int lag_lo;      // first lag of the level (= P)
    int NP;          // partitions
    int period;      // steps between two period starts (= P)
    int lag_hi;      // one past the last lag: min(S, (NP + 1) P)
};
constexpr int kTailLevelsMax = 3;
constexpr int kTailFormLevelled = 1, kTailFormUniform = 2;  // hc_set_radiation_tail

inline TailLevel tail_make_level(int P, int NP, int S) { return TailLevel{P, 2 * P, P + 1, P, NP, P, std::min(S, (NP + 1) * P)}; }

// The levels of a form, largest P first; returns their number (0: no tail, the full pass).
inline int tail_levels(int S, int form, TailLevel* lv) {
    if (tail_partitions(S) < 1) return 0;
    if (form == kTailFormUniform) {
        lv[0] = tail_make_level(kTailP, tail_partitions(S), S);
        return 1;
    }
    if (S >= 4 * kTailP) {
        lv[0] = tail_make_level(2 * kTailP, (S + 2 * kTailP - 1) / (2 * kTailP) - 1, S);
        lv[1] = tail_make_level(kTailP, 1, S);
        lv[2] = tail_make_level(kTailP / 2, 1, S);
        return 3;
    }
    lv[0] = tail_make_level(kTailP, tail_partitions(S), S);
    lv[1] = tail_make_level(kTailP / 2, 1, S);
    return 2;
}
// lags the head pass keeps: those below the smallest level
inline int tail_head_lags(const TailLevel* lv, int n) { return n > 0 ? lv[n - 1].lag_lo : 0; }

// Are the far partitions (p >= 2) of a level made during the period BEFORE the one they serve, a chunk of bins beside each of its
// blocks (tail_far_chunks)?  Only at P = kTailP.  Far chunks keep the samples of the previous period's windows for two periods, so a
// sample that has left the IRF window can still meet (zero-padded) taps up to 2P steps later -- rounding noise where the sum is
// exactly zero; at P = 512 that is past the S - 1 + 2 kTailP + 2 L steps after which the radiation of a body at rest is held to be
// exactly zero.  The far partitions of the P = 512 level are therefore made at its period start, from that period's own windows:
// the same bytes per step, in front of one step in 512 instead of spread over the blocks.
inline bool tail_level_far_ahead(const TailLevel& lv) { return lv.NP > 1 && lv.P <= kTailP; }

inline int tail_level_blocks(const TailLevel& lv, int lookahead) { return lookahead > 0 ? lv.P / lookahead : 0; }
inline bool tail_level_starts(const TailLevel& lv, int j) { return j % lv.period == 0; }  // j: step offset in the top period
inline void tail_level_chunk_bins(const TailLevel& lv, int k, int nchunks, int* lo, int* hi) {
    *lo = static_cast<int>(static_cast<long long>(k) * lv.bins / nchunks);
    *hi = static_cast<int>(static_cast<long long>(k + 1) * lv.bins / nchunks);
}
inline int tail_level_window_back(const TailLevel& lv, int a, int k) { return (a + 1) * lv.P - 1 - k; }
inline bool tail_level_window_live(const TailLevel& lv, int S, int a, int k) { return k >= 1 && tail_level_window_back(lv, a, k) <= S - 2; }
// lag of tap r of partition p, and whether K-hat holds it (the others are zero padding)
inline int tail_level_lag(const TailLevel& lv, int p, int r) { return p * lv.P + r; }
inline bool tail_level_tap_live(const TailLevel& lv, int S, int p, int r) { return r < lv.P && p >= 1 && p <= lv.NP && tail_level_lag(lv, p, r) < S; }

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
