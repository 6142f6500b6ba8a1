// hc_wave_kin2_dir.hpp -- the pair sum of the second-order wave kinematics in a short-crested sea as a device function, and the
// angle and wave-number forms the pair kernel shares (hc_wave_kin2.hip: wk2_pair_kernel<true>, wk2_sum_kernel<true, ...>).  HIP only.
// DESIGN.md 3.7n has the definition and the invariants; the long-crested sum is hc_wave_kin2_sum.hpp, which this leaves alone.
#pragma once
#include <hip/hip_runtime.h>

#include "hc_wave_kin.hpp"
#include "hc_wave_kin2_sum.hpp"

namespace hc {

// sigma = sin^2((beta_i - beta_j) / 2) and tau = cos^2((beta_i - beta_j) / 2) from the unit vectors (c, s) of the two directions:
// a quarter of the squared length of their difference and of their sum, so each keeps its relative accuracy where it is small
// (directions that nearly agree, directions that nearly oppose).  cos(beta_i - beta_j) = tau - sigma = 1 - 2 sigma = 2 tau - 1.
__host__ __device__ __forceinline__ void wk2_dir_angle(double ci, double si, double cj, double sj, double& sig, double& tau) {
#pragma clang fp contract(off)
    const double dc = ci - cj, ds = si - sj, pc = ci + cj, ps = si + sj;
    sig = 0.25 * (dc * dc + ds * ds);
    tau = 0.25 * (pc * pc + ps * ps);
}

// |kappa|^2 of kappa = k_i e_i + kjs e_j with kjs = +-k_j: (k_i + kjs)^2 - 4 k_i kjs sigma = (k_i - kjs)^2 + 4 k_i kjs tau; the
// form is taken whose second part is at most half the first, so neither sign cancels for any angle.
__host__ __device__ __forceinline__ double wk2_dir_kappa2(double ki, double kjs, double sig, double tau) {
#pragma clang fp contract(off)
    const double p = ki + kjs, m = ki - kjs, kk = 4.0 * ki * kjs;
    return sig <= 0.5 ? p * p - kk * sig : m * m + kk * tau;
}

constexpr int kWk2DirSums = 7;  // 4 eta2, u2x, u2y, u2z, a2x, a2y, a2z

// The sum of one (point, time) item by the whole workgroup of kWk2Threads, structured as wk2_item_sum (hc_wave_kin2_sum.hpp): the
// upper triangle of the pair matrix tile of rows by tile of columns, one sincos per component and tile pair staged in LDS, a tile
// pair no band reaches into skipped, wave v on the rows v, v + 4, ..., its lanes along the row's band, every lane's terms in a
// fixed order into its own partial sums, and the fixed tree over the 256 lanes.  `a.tab` is [kKinCols + kDirCols][nf].
// New against the long-crested sum: the phase is k (x c + y s) - w t + phi (kin_kx<true>); c and s of both tiles are staged, and
// per pair and sign sigma, tau, |kappa|, kappa_x, kappa_y, e^{|kappa| z2} and the finite-depth factors are computed -- |kappa+| is
// not k_i + k_j here, so no product of staged factors stands in for its profile.  e^{|kappa| z2} is an exp of a finite,
// non-positive argument: 0, never NaN, once it underflows.  The two signs share one loop body (sg = -1, +1).
// out (work item 0 only; zeros elsewhere): 4 eta2, u2x, u2y, u2z, a2x, a2y, a2z before the ramp, and with Q2 an eighth value
// q2 = -d phi2 / dt = sum B Omega C cos Theta [m^2/s^2] (wk2_item_sum's Q2 in this sea): one more accumulator over
// the same pairs with B C as u2x forms it, one more row of the tree.  Q2 without KIN stages k, w and the directions and computes
// |kappa|, e^{|kappa| z2} and the finite-depth C, but no velocity or acceleration; eta2 has the same bits in every instantiation.
template <bool ETA, bool KIN, bool Q2 = false>
__device__ inline void wk2_dir_item_sum(const Wk2Sea& a, double x, double y, double z, double t,
                                        double (&out)[Q2 ? kWk2DirSums + 1 : kWk2DirSums]) {
#pragma clang fp contract(off)
    constexpr bool PROF = KIN || Q2;  // the pair's wave number and depth profile are wanted
    constexpr int kT = kKinTile, kTK = PROF ? kKinTile : 1, kDc = kKinCols, kDs = kKinCols + 1;
    constexpr int kR = Q2 ? kWk2DirSums + 1 : kWk2DirSums;
    __shared__ double sc[2][kT], ss[2][kT], sA[2][kT];  // [0]: the tile of rows, [1]: the tile of columns
    __shared__ double sk[2][kTK], sw[2][kTK], sdc[2][kTK], sds[2][kTK];
    __shared__ double red[kR][kWk2Threads];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nf = a.nf;
    const long long n2 = static_cast<long long>(nf) * nf;
    double z2 = fmin(z - a.mwl, 0.0);
    if (a.finite_depth && z2 < -a.depth) z2 = -a.depth;
    const double zh = a.finite_depth ? z2 + a.depth : 0.0;
    double eta = 0.0, ux = 0.0, uy = 0.0, uz = 0.0, ax = 0.0, ay = 0.0, az = 0.0, q2 = 0.0;

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
                    const double dc = a.tab[kDc * nf + i], ds = a.tab[kDs * nf + i];
                    double sn, cs;
                    sincos(kin_kx<true>(k, x, y, dc, ds) - w * t + a.tab[kKinPhase * nf + i], &sn, &cs);
                    sc[h][tid] = cs;
                    ss[h][tid] = sn;
                    sA[h][tid] = a.tab[kKinAmp * nf + i];
                    if constexpr (PROF) {
                        sk[h][tid]  = k;
                        sw[h][tid]  = w;
                        sdc[h][tid] = dc;
                        sds[h][tid] = ds;
                    }
                }
            }
            __syncthreads();
            for (int r = wave; r < mi; r += kWk2Waves) {
                const int i = i0 + r;
                const double ci = sc[0][r], si = ss[0][r], Ai = sA[0][r];
                double ki = 0.0, wi = 0.0, dci = 0.0, dsi = 0.0, kci = 0.0, ksi = 0.0;
                if constexpr (PROF) {
                    ki  = sk[0][r];
                    wi  = sw[0][r];
                    dci = sdc[0][r];
                    dsi = sds[0][r];
                }
                if constexpr (KIN) {
                    kci = ki * dci;
                    ksi = ki * dsi;
                }
                const double* row = a.pair + static_cast<size_t>(i) * nf;
                // sign 0: Theta = theta_i - theta_j, kappa = k_i e_i - k_j e_j, Omega = w_i - w_j; sign 1: the sums
#pragma unroll 1
                for (int s = 0; s < 2; ++s) {
                    if (!(s ? a.sign_on[1] : a.sign_on[0])) continue;
                    const double sg  = s ? 1.0 : -1.0;
                    const double* Kt = row + (s ? kWk2Kp : kWk2Km) * n2;
                    const double* Bt = row + (s ? kWk2Bp : kWk2Bm) * n2;
                    const int* b     = a.band + 2 * (static_cast<size_t>(s) * nf + i);
                    const int first = max(b[0], j0), last = min(b[1], j1);
                    for (int j = first + lane; j <= last; j += 64) {
                        const int c     = j - j0;
                        const double cj = sc[1][c], sjs = sg * ss[1][c];
                        const double cT = fma(ci, cj, -(si * sjs)), sT = fma(si, cj, ci * sjs);
                        const double wgt = j == i ? 1.0 : 2.0;
                        if constexpr (ETA) eta = fma(wgt * (Ai * sA[1][c]) * Kt[j], cT, eta);
                        if constexpr (PROF) {
                            const double B   = wgt * Bt[j];
                            const double kjs = sg * sk[1][c], Om = wi + sg * sw[1][c];
                            const double dcj = sdc[1][c], dsj = sds[1][c];
                            double sig, tau;
                            wk2_dir_angle(dci, dsi, dcj, dsj, sig, tau);
                            const double ak = sqrt(wk2_dir_kappa2(ki, kjs, sig, tau));
                            double kx = 0.0, ky = 0.0;  // (KIN only)
                            if constexpr (KIN) kx = kci + kjs * dcj, ky = ksi + kjs * dsj;
                            const double e  = exp(ak * z2);
                            double C = e, S = e;
                            if (a.finite_depth) {  // (uniform over the launch)
                                const double q = exp(-2.0 * ak * zh), d = 1.0 / (1.0 + exp(-2.0 * ak * a.depth));
                                C = e * (1.0 + q) * d;
                                S = e * (1.0 - q) * d;
                            }
                            const double bC = B * C;
                            if constexpr (KIN) {
                                const double bS = B * ak * S;
                                const double bx = bC * kx, by = bC * ky;
                                ux = fma(bx, cT, ux);
                                uy = fma(by, cT, uy);
                                uz = fma(bS, sT, uz);
                                ax = fma(bx * Om, sT, ax);
                                ay = fma(by * Om, sT, ay);
                                az = fma(-(bS * Om), cT, az);
                            }
                            if constexpr (Q2) q2 = fma(bC * Om, cT, q2);
                        }
                    }
                }
            }
        }
    }
    red[0][tid] = eta;
    red[1][tid] = ux;
    red[2][tid] = uy;
    red[3][tid] = uz;
    red[4][tid] = ax;
    red[5][tid] = ay;
    red[6][tid] = az;
    if constexpr (Q2) red[7][tid] = q2;
    // ---- fixed-shape tree over the 256 lanes: lane l adds lane l + h for h = 128, 64, ..., 1 (wk2_item_sum) ----
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

// A value every lane of the wave holds, moved to scalar registers (its bits unchanged): the point of morison2_incr_kernel<true> and
// of the strip members' increment kernels (hc_morison_members.hip) then costs the pair sum no vector register, as the point
// wk2_sum_kernel loads with scalar loads costs it none
__device__ __forceinline__ double wave_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// The pair sum of either sea behind one name, for the kernels that exist once per sea (wk2_sum_kernel, morison2_incr_kernel,
// nl2_incr_kernel): wk2_item_sum, which has no y, or wk2_dir_item_sum.  The two stay two functions -- their arithmetic differs on
// purpose -- and each keeps its own bits.  out: wk2_sums(DIR) values, and q2 behind them with Q2.
constexpr int wk2_sums(bool dir) { return dir ? kWk2DirSums : 5; }

template <bool DIR, bool ETA, bool KIN, bool Q2 = false>
__device__ __forceinline__ void wk2_sea_sum(const Wk2Sea& a, double x, double y, double z, double t,
                                            double (&out)[wk2_sums(DIR) + (Q2 ? 1 : 0)]) {
    if constexpr (DIR) wk2_dir_item_sum<ETA, KIN, Q2>(a, x, y, z, t, out);
    else wk2_item_sum<ETA, KIN, Q2>(a, x, z, t, out);
}

}  // namespace hc
