// hc_qtf.hpp -- what the kernels of the two QTF terms share: those of tables on a frequency grid (hc_qtf.hip: drift_qtf_kernel,
// sum_qtf_kernel) and those of tables on a heading x frequency grid (hc_qtf_dir.hip).  The argument block, a slot's descriptor, the two
// sign patterns of the pair product and the reduction tree.  DESIGN.md 3.7e, 3.7i, 3.7l.
#pragma once
#include <hip/hip_runtime.h>

#include "hc_limits.hpp"
#include "hc_wave_kin.hpp"

namespace hc {

constexpr int kQtfThreads = 256;  // work items per workgroup: one per grid bin in phase 1 (kDriftMaxFreq bins at the most)
static_assert(kDriftMaxFreq <= kQtfThreads, "one lane per bin of the frequency grid");
static_assert(kKinTile == kQtfThreads, "one lane per component of a staged tile");

// per (owned body with a table): [kDescWords] 64-bit words.  A table on a heading grid: kDescNq holds its node count J = nh nq
enum QtfDesc { kDescBody = 0, kDescNq, kDescRowPtr, kDescP, kDescQ, kDescE, kDescWords };

enum QtfKind { kQtfDrift, kQtfSum };

struct QtfArgs {
    const double* tab;      // [kKinCols][nf] (hc_wave_kin.hpp), then [kDirCols][nf]: cos and sin of the component directions
    int nf;
    int mode;               // drift: 1 mean drift, 2 Newman, 3 full QTF (the sum kernel does not read it)
    const long long* desc;  // [slots][kDescWords]: body, nq, first row pointer, offsets of P, Q (-1: none) and E (drift)
    const int* rowptr;      // per slot nq + 1 entries: bin m owns the entries [rowptr[m], rowptr[m + 1])
    const int* ent_idx;     // component index of an entry, ascending within a bin
    const double* ent_w;    // its interpolation weight
    const double* pq;       // the tables, [6][nq][nq] each
    const double* em;       // drift: E_m = sum_i W[i][m] A_i^2 per slot and bin
    const double* pos;      // [3 N]
    double t, ramp2;
    double* out;            // [slots][6]
};

// One entry of the bilinear form over bin (node) pairs: the signs of theta_i - theta_j (drift) and of theta_i + theta_j (sum)
template <QtfKind KIND>
__device__ __forceinline__ double qtf_pair_pq(double P, double Q, double Um, double Vm, double Un, double Vn) {
    if constexpr (KIND == kQtfDrift)
        return P * (Um * Un + Vm * Vn) - Q * (Vm * Un - Um * Vn);
    else
        return P * (Um * Un - Vm * Vn) - Q * (Vm * Un + Um * Vn);
}
template <QtfKind KIND>
__device__ __forceinline__ double qtf_pair_p(double P, double Um, double Vm, double Un, double Vn) {
    if constexpr (KIND == kQtfDrift)
        return P * (Um * Un + Vm * Vn);
    else
        return P * (Um * Un - Vm * Vn);
}

// Fixed-shape tree over the 256 lanes of R columns: lane l adds lane l + h for h = 128, 64, ..., 1 (nl_panels_kernel); the sums end
// in red[k][0], for lane 0 to read
template <int R>
__device__ __forceinline__ void qtf_tree(double (*red)[kQtfThreads]) {
    const int tid = threadIdx.x;
    for (int h = kQtfThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < R; ++k) red[k][tid] += red[k][tid + h];
        }
    }
}

// ---- tables on a heading x frequency grid (hc_qtf_dir.hip) ----
constexpr int kQtfDirRows   = 32;                              // node rows of a table row one workgroup of the pair kernel sums
constexpr int kQtfDirChunks = kQtfMaxNodes / kQtfDirRows;      // partials a (slot, row) may have
constexpr int kQtfDirOwned  = kQtfMaxNodes / kQtfThreads;      // nodes a lane projects onto: l, l + 256, ...
static_assert(kQtfMaxNodes % kQtfDirRows == 0 && kQtfMaxNodes % kQtfThreads == 0, "whole chunks, whole lanes");

struct QtfDirArgs {
    QtfArgs a;     // desc, out: those of the slots with a heading grid; pq: [6][J][J] each, node p = a nq + m
    double* part;  // [slots][6][kQtfDirChunks]
};

// The pair kernel (grid: chunks x 6 slots) and the finish kernel behind it on `st`; chunks: the most any slot needs in this mode
void qtf_dir_launch(const QtfDirArgs& g, QtfKind kind, int slots, int chunks, hipStream_t st);

}  // namespace hc
