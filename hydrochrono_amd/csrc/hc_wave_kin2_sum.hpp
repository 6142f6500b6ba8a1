// hc_wave_kin2_sum.hpp -- the pair sum of the second-order wave kinematics as a device function, shared by the kernels that run it
// (hc_wave_kin2.hip: wk2_sum_kernel; hc_morison.hip: morison2_incr_kernel; hc_nonlinear.hip: nl2_incr_kernel -- their <false>
// instantiations; the short-crested sea's sum is hc_wave_kin2_dir.hpp), and the host calls that build the tables of either sea.
// HIP only.  DESIGN.md 3.7f has the definition and the invariants, 3.7g and 3.7h the other users.
#pragma once
#include <hip/hip_runtime.h>

#include "hc_context.hpp"
#include "hc_wave_kin.hpp"
#include "hc_wave_kin2.hpp"

namespace hc {

constexpr int kWk2Threads = 256;  // work items per workgroup: four waves, each takes every fourth row of a tile
constexpr int kWk2Waves   = kWk2Threads / 64;
static_assert(kKinTile == kWk2Threads, "one lane per component of a staged tile");

enum Wk2Table { kWk2Kp = 0, kWk2Km, kWk2Bp, kWk2Bm, kWk2Tables };

// What a pair sum reads besides its own (x, z, t): the tables of a Wk2TableSet and the options that are uniform over a launch
struct Wk2Sea {
    const double* tab;   // [kKinCols][nf] (hc_wave_kin.hpp)
    int nf;
    const double* pair;  // [kWk2Tables][nf][nf]
    const int* band;     // [2][nf][2]: sign 0 difference, 1 sum; first and last column j >= i of row i inside the band
    double depth, mwl;
    int finite_depth;    // 0: water depth +inf, the profiles are e^{|kappa| z}
    int sign_on[2];      // some pair lies inside the difference / the sum band
};

// The sum of one (point, time) item by the whole workgroup of kWk2Threads: every work item of the group calls it with the same
// arguments.  The upper triangle j >= i of the pair matrix is visited (the terms are symmetric in (i, j): an off-diagonal pair
// counts twice), tile of rows by tile of columns.  Per tile pair the workgroup stages cos theta, sin theta, A and -- for the
// kinematics -- k, w, e^{k z2} and the two finite-depth factors of both tiles in LDS, one component per lane, one sincos per
// component.  Wave v then takes the rows v, v + 4, ... of the row tile and its lanes stride over the row's band of columns: the
// table is read along j, the column values from consecutive LDS words, the row values by broadcast.  Every lane adds its terms in
// that fixed order into its own partial sums, and the 256 partials go through a tree whose shape depends on the lane index alone:
// an item's bits depend on the item, the tables and the options only -- not on the kernel that asks.
// out (work item 0 only; zeros elsewhere): 4 eta2, u2x, u2z, a2x, a2z before the ramp, and with Q2 a sixth value
// q2 = -d phi2 / dt = sum B Omega C cos Theta [m^2/s^2], the second-order potential's part of the pressure over rho:
// one more accumulator over the same pairs with C as the kinematics form it, one more row of the tree.  Q2 without KIN computes
// no velocity or acceleration; eta2 has the same bits in every instantiation.
// No implicit fusing of a multiplication into an addition: the sums are written with explicit fma() where one is wanted, so that an
// item's bits are the same in every instantiation and in every translation unit, whatever that unit's default is.
template <bool ETA, bool KIN, bool Q2 = false>
__device__ inline void wk2_item_sum(const Wk2Sea& a, double x, double z, double t, double (&out)[Q2 ? 6 : 5]) {
#pragma clang fp contract(off)
    constexpr bool PROF = KIN || Q2;  // the depth profiles are wanted
    constexpr int kT = kKinTile, kTK = PROF ? kKinTile : 1, kR = Q2 ? 6 : 5;
    __shared__ double sc[2][kT], ss[2][kT], sA[2][kT];  // [0]: the tile of rows, [1]: the tile of columns
    __shared__ double sk[2][kTK], sw[2][kTK], sE[2][kTK], sG[2][kTK], sF[2][kTK];
    __shared__ double red[kR][kWk2Threads];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nf = a.nf;
    const long long n2 = static_cast<long long>(nf) * nf;
    // the second-order fields are held at their mean-level value above it, and at the bed's below it
    double z2 = fmin(z - a.mwl, 0.0);
    if (a.finite_depth && z2 < -a.depth) z2 = -a.depth;
    const double zh = a.finite_depth ? z2 + a.depth : 0.0;
    double eta = 0.0, ux = 0.0, uz = 0.0, ax = 0.0, az = 0.0, q2 = 0.0;

    for (int j0 = 0; j0 < nf; j0 += kT) {
        const int mj = min(kT, nf - j0), j1 = j0 + mj - 1;
        for (int i0 = 0; i0 <= j0; i0 += kT) {
            const int mi = min(kT, nf - i0);
            // does any row of the tile reach into the tile of columns?  (also the barrier that frees the LDS tiles)
            int reach = 0;
            if (tid < mi) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (!a.sign_on[s]) continue;
                    const int* b = a.band + 2 * (static_cast<size_t>(s) * nf + i0 + tid);
                    reach |= max(b[0], j0) <= min(b[1], j1);
                }
            }
            if (!__syncthreads_or(reach)) continue;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int base = h ? j0 : i0, m = h ? mj : mi;
                if (tid < m) {
                    const int i = base + tid;
                    const double k = a.tab[kKinK * nf + i], w = a.tab[kKinOmega * nf + i];
                    double sn, cs;
                    sincos(k * x - w * t + a.tab[kKinPhase * nf + i], &sn, &cs);
                    sc[h][tid] = cs;
                    ss[h][tid] = sn;
                    sA[h][tid] = a.tab[kKinAmp * nf + i];
                    if constexpr (PROF) {
                        sk[h][tid] = k;
                        sw[h][tid] = w;
                        sE[h][tid] = exp(k * z2);
                        sG[h][tid] = a.finite_depth ? exp(-2.0 * k * zh) : 0.0;
                        sF[h][tid] = a.finite_depth ? exp(-2.0 * k * a.depth) : 0.0;
                    }
                }
            }
            __syncthreads();
            for (int r = wave; r < mi; r += kWk2Waves) {
                const int i = i0 + r;
                const double ci = sc[0][r], si = ss[0][r], Ai = sA[0][r];
                const double* row = a.pair + static_cast<size_t>(i) * nf;
                // ---- difference terms: Theta = theta_i - theta_j, kappa = k_i - k_j, Omega = w_i - w_j ----
                if (a.sign_on[0]) {
                    const int* b    = a.band + 2 * static_cast<size_t>(i);
                    const int first = max(b[0], j0), last = min(b[1], j1);
                    for (int j = first + lane; j <= last; j += 64) {
                        const int c     = j - j0;
                        const double cj = sc[1][c], sj = ss[1][c];
                        const double cm = fma(ci, cj, si * sj), sm = fma(si, cj, -(ci * sj));
                        const double wgt = j == i ? 1.0 : 2.0;
                        if constexpr (ETA) eta = fma(wgt * (Ai * sA[1][c]) * row[kWk2Km * n2 + j], cm, eta);
                        if constexpr (PROF) {
                            const double B   = wgt * row[kWk2Bm * n2 + j];
                            const double kap = sk[0][r] - sk[1][c], ak = fabs(kap), Om = sw[0][r] - sw[1][c];
                            const double e   = exp(ak * z2);  // (not E_i / E_j: either may have underflowed)
                            double C = e, S = e;
                            if (a.finite_depth) {  // (uniform over the launch)
                                const double q = exp(-2.0 * ak * zh), d = 1.0 / (1.0 + exp(-2.0 * ak * a.depth));
                                C = e * (1.0 + q) * d;
                                S = e * (1.0 - q) * d;
                            }
                            if constexpr (KIN) {
                                const double bkC = B * kap * C, bkS = B * ak * S;
                                ux = fma(bkC, cm, ux);
                                uz = fma(bkS, sm, uz);
                                ax = fma(bkC * Om, sm, ax);
                                az = fma(-(bkS * Om), cm, az);
                            }
                            if constexpr (Q2) q2 = fma(B * C * Om, cm, q2);
                        }
                    }
                }
                // ---- sum terms: Theta = theta_i + theta_j, kappa = k_i + k_j, Omega = w_i + w_j ----
                if (a.sign_on[1]) {
                    const int* b    = a.band + 2 * (static_cast<size_t>(nf) + i);
                    const int first = max(b[0], j0), last = min(b[1], j1);
                    for (int j = first + lane; j <= last; j += 64) {
                        const int c     = j - j0;
                        const double cj = sc[1][c], sj = ss[1][c];
                        const double cp = fma(ci, cj, -(si * sj)), sp = fma(si, cj, ci * sj);
                        const double wgt = j == i ? 1.0 : 2.0;
                        if constexpr (ETA) eta = fma(wgt * (Ai * sA[1][c]) * row[kWk2Kp * n2 + j], cp, eta);
                        if constexpr (PROF) {
                            const double B   = wgt * row[kWk2Bp * n2 + j];
                            const double kap = sk[0][r] + sk[1][c], ak = fabs(kap), Om = sw[0][r] + sw[1][c];
                            const double e   = sE[0][r] * sE[1][c];  // e^{(k_i + k_j) z2}: 0, never NaN, where a factor has underflowed
                            double C = e, S = e;
                            if (a.finite_depth) {
                                const double q = sG[0][r] * sG[1][c], d = 1.0 / (1.0 + sF[0][r] * sF[1][c]);
                                C = e * (1.0 + q) * d;
                                S = e * (1.0 - q) * d;
                            }
                            if constexpr (KIN) {
                                const double bkC = B * kap * C, bkS = B * ak * S;
                                ux = fma(bkC, cp, ux);
                                uz = fma(bkS, sp, uz);
                                ax = fma(bkC * Om, sp, ax);
                                az = fma(-(bkS * Om), cp, az);
                            }
                            if constexpr (Q2) q2 = fma(B * C * Om, cp, q2);
                        }
                    }
                }
            }
        }
    }
    red[0][tid] = eta;
    red[1][tid] = ux;
    red[2][tid] = uz;
    red[3][tid] = ax;
    red[4][tid] = az;
    if constexpr (Q2) red[5][tid] = q2;
    // ---- fixed-shape tree over the 256 lanes: lane l adds lane l + h for h = 128, 64, ..., 1 (drift_qtf_kernel) ----
    for (int h = kWk2Threads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < kR; ++k) red[k][tid] += red[k][tid + h];
        }
    }
#pragma unroll
    for (int k = 0; k < kR; ++k) out[k] = tid == 0 ? red[k][0] : 0.0;
}

// ---- hc_wave_kin2.hip: the host side all users share (the four calls; hc_morison.hip and hc_nonlinear.hip through Order2Part) ----
int wk2_component_count(const hc_ctx* c);
// The component table, the pair tables and the band limits of the context's wave model in `s`, built on `st` (wk2_pair_kernel<dir>)
// and complete when the call returns.  `dir`: the layout of the short-crested sea -- the direction columns behind the component
// table ((1, 0) with no directions set) and the angles in the pair tables.  Rebuilt when a hc_set_wave_* call has come in since
// (wave_serial; a direction change counts), the regular wave's phase or a cut-off differs from the cached one, or `s` holds the
// other layout (Wk2TableSet::dir).  The mark goes first and the stamp last: a failure on the way leaves nothing that counts as
// current.  With no pair inside either band the pair tables hold zeros, or -- keep_empty false: nobody reads them -- are released
// and no kernel is launched.
void wk2_tables(hc_ctx* c, Wk2TableSet& s, hipStream_t st, double regular_phase, const double cut[4], bool keep_empty, bool dir);

}  // namespace hc
