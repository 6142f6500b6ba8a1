// hc_wave_kin.hip -- wave kinematics: WaveBase::GetElevation / GetVelocity / GetAcceleration of the reference
// (include/hydroc/wave_types.h:69-73; src/wave_types.cpp:14-158 for the sums, :301-313 RegularWave, :515-550 IrregularWaves with
// Wheeler stretching) for the context's wave model, batched over P points x T times.  Off the force path: the kernel reads its own
// component table and writes its own buffers, nothing a step uses.  DESIGN.md 3.7a describes the kernel and the reference
// behaviour reproduced here, INTEGRATION.md 2 the one deviation (infinite depth under stretching).
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"

using namespace hc::detail;

namespace hc {

std::vector<double> kin_table_host(const hc_ctx* c, double regular_phase) {
    if (c->wave_kind == kWaveNone || (c->wave_kind == kWaveIrregular && c->eta_record && !c->record_components())) return {};
    std::vector<double> amp, omega, k, phase;
    if (c->wave_kind == kWaveRegular) {
        amp   = {c->reg_amp};
        omega = {c->reg_omega};
        k     = {c->reg_wavenumber};
        phase = {regular_phase};
    } else {
        const size_t nf = c->spec_f.size();
        const bool rec  = c->record_components();  // the amplitudes of the analysis as they are, not through S and back
        amp.resize(nf);
        omega.resize(nf);
        for (size_t i = 0; i < nf; ++i) {
            amp[i]   = rec ? c->rec_amp[i] : std::sqrt(2 * c->spec_S[i] * c->spec_df[i]);
            omega[i] = 2 * M_PI * c->spec_f[i];
        }
        k     = c->spec_k;
        phase = c->spec_phase;
    }
    const int nf = static_cast<int>(amp.size());
    const double d = c->depth;
    std::vector<double> tab(static_cast<size_t>(kKinCols) * nf);
    auto at = [&](int col, int i) -> double& { return tab[static_cast<size_t>(col) * nf + i]; };
    for (int i = 0; i < nf; ++i) {
        const bool deep     = 2 * M_PI / k[i] > d || k[i] * d > 500.0;  // src/wave_types.cpp:74,108
        at(kKinAmp, i)      = amp[i];
        at(kKinOmega, i)    = omega[i];
        at(kKinK, i)        = k[i];
        at(kKinPhase, i)    = phase[i];
        at(kKinWA, i)       = omega[i] * amp[i];
        at(kKinW2A, i)      = omega[i] * omega[i] * amp[i];
        at(kKinInvSinh, i)  = deep ? 0.0 : 1.0 / std::sinh(k[i] * d);
        at(kKinDeep, i)     = deep ? 1.0 : 0.0;
    }
    return tab;
}

bool kin_has_components(const hc_ctx* c) {
    return c->wave_kind == kWaveRegular || c->wave_kind == kWaveSpectral || (c->wave_kind == kWaveIrregular && !c->eta_record) ||
           c->record_components();
}

bool kin_synthesised(const hc_ctx* c) { return (c->wave_kind == kWaveIrregular && !c->eta_record) || c->wave_kind == kWaveSpectral; }

double kin_ramp(const hc_ctx* c, double t) {
    const double rd = c->irr.ramp_duration;
    return (kin_synthesised(c) && rd > 0.0 && t < rd) ? (t <= 0.0 ? 0.0 : t / rd) : 1.0;
}

bool kin_table_current(const hc_ctx* c, unsigned long long serial, double cached_phase, double phase) {
    return serial == c->wave_serial && (c->wave_kind != kWaveRegular || std::memcmp(&cached_phase, &phase, sizeof(double)) == 0);
}

std::vector<double> kin_dir_columns_host(const hc_ctx* c) {
    const size_t nf = c->wave_dir.size();
    std::vector<double> col(kDirCols * nf);
    for (size_t i = 0; i < nf; ++i) {
        col[i]      = std::cos(c->wave_dir[i]);
        col[nf + i] = std::sin(c->wave_dir[i]);
    }
    return col;
}

bool KinTableCopy::current(const hc_ctx* c, double regular_phase) const { return kin_table_current(c, serial, phase, regular_phase); }

void KinTableCopy::refresh(hc_ctx* c, double regular_phase, hipStream_t st, const Shape& shape) {
    if (current(c, regular_phase)) return;
    serial = ~0ULL;  // a failure below leaves nothing that counts as current
    std::vector<double> host = kin_table_host(c, regular_phase);
    nf = static_cast<int>(host.size() / kKinCols);
    std::vector<double> cols = kin_dir_columns_host(c);
    if (shape) shape(host, cols, nf);
    host.insert(host.end(), cols.begin(), cols.end());
    tab.upload(host, st);
    dir    = !cols.empty();
    serial = c->wave_serial;
    phase  = regular_phase;
}

namespace {

constexpr int kKinThreads = 256;  // work items per workgroup, one per (point, time)
// (point, time) pairs per call: the grid's work-item count stays below 2^31
constexpr long long kKinMaxItems = (1LL << 31) - kKinThreads;

struct KinArgs {
    const double* tab;  // [kKinCols][nf]; the directional instantiation: [kKinCols + kDirCols][nf]
    int nf;
    int P, T;
    const double* xyz;  // [P][3]
    const double* t;    // [T]
    double depth, mwl;
    int stretch;       // Wheeler stretching (IrregularWaveParams::wave_stretching_)
    int finite_depth;  // 0: water depth +inf, the stretched z is the limit z' - eta
    double* eta;       // [T][P]    } NULL: not wanted
    double* vel;       // [T][P][3] }
    double* acc;       // [T][P][3] }
};

// One work item per (point, time), item o = j * P + p.  Every item sums the components in index order from the same LDS tiles, so
// its bits do not depend on P, T or where in the grid it sits.  With stretching, eta is summed first (the reference's
// GetEtaIrregular) and the kinematics are evaluated at the stretched z in a second pass.
// DIR: every component has a direction; its cos and sin are staged behind the other columns, the phase is taken
// at k (x cos + y sin) and the horizontal velocity and acceleration are laid along (cos, sin).  Everything else is the code of the
// long-crested instantiation, whose arithmetic is unchanged.
template <bool DIR>
__global__ void __launch_bounds__(kKinThreads) wave_kinematics_kernel(KinArgs a) {
    constexpr int kDc = kKinCols, kDs = kKinCols + 1;  // rows of the direction columns (DIR only)
    __shared__ double s[DIR ? kKinCols + kDirCols : kKinCols][kKinTile];
    const long long n  = static_cast<long long>(a.P) * a.T;
    const long long o  = static_cast<long long>(blockIdx.x) * kKinThreads + threadIdx.x;
    const bool active  = o < n;
    const long long oc = active ? o : 0;  // items past the end evaluate item 0 and store nothing (all take part in the staging)
    const int p = static_cast<int>(oc % a.P), j = static_cast<int>(oc / a.P);
    const double x = a.xyz[3 * p], y = DIR ? a.xyz[3 * p + 1] : 0.0, z = a.xyz[3 * p + 2], t = a.t[j];
    const bool want_kin = a.vel || a.acc;

    // ---- eta = sum_i A_i cos(k_i x - w_i t + phi_i)  (src/wave_types.cpp:14-44; the expression of eta_kernel at x = 0) ----
    double eta = 0.0;
    if (a.eta || (a.stretch && want_kin)) {
        for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
            const int m = min(kKinTile, a.nf - i0);
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += kKinThreads) {
                s[kKinAmp][i]   = a.tab[kKinAmp * a.nf + i0 + i];
                s[kKinOmega][i] = a.tab[kKinOmega * a.nf + i0 + i];
                s[kKinK][i]     = a.tab[kKinK * a.nf + i0 + i];
                s[kKinPhase][i] = a.tab[kKinPhase * a.nf + i0 + i];
                if constexpr (DIR) {
                    s[kDc][i] = a.tab[kDc * a.nf + i0 + i];
                    s[kDs][i] = a.tab[kDs * a.nf + i0 + i];
                }
            }
            __syncthreads();
            for (int i = 0; i < m; ++i)
                eta += s[kKinAmp][i] *
                       cos(kin_kx<DIR>(s[kKinK][i], x, y, DIR ? s[kDc][i] : 0.0, DIR ? s[kDs][i] : 0.0) - s[kKinOmega][i] * t + s[kKinPhase][i]);
        }
    }
    if (!want_kin) {  // (uniform over the launch)
        if (active) a.eta[o] = eta;
        return;
    }

    // ---- z at which the profiles are evaluated (:515-544; GetWaterVelocity subtracts mwl from what it is given, :69-71) ----
    double zs = z;
    if (a.stretch) {
        const double zr = z - a.mwl;
        zs = a.finite_depth ? a.depth * (zr - eta) / (a.depth + eta) : zr - eta;
    }
    const double ze = zs - a.mwl;  // under stretching mwl is subtracted a second time, as in the reference

    // ---- velocity and acceleration (:61-158) ----
    double ux = 0.0, uy = 0.0, uz = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int m = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += kKinThreads) {
#pragma unroll
            for (int col = kKinOmega; col < (DIR ? kKinCols + kDirCols : kKinCols); ++col) s[col][i] = a.tab[col * a.nf + i0 + i];
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const double k = s[kKinK][i];
            const double dc = DIR ? s[kDc][i] : 0.0, ds = DIR ? s[kDs][i] : 0.0;
            double sn, cs;
            sincos(kin_kx<DIR>(k, x, y, dc, ds) - s[kKinOmega][i] * t + s[kKinPhase][i], &sn, &cs);
            double px, pz;
            if (s[kKinDeep][i] != 0.0) {  // (the same branch for every item: no divergence)
                px = pz = exp(k * ze);
            } else {
                const double q = k * (ze + a.depth);
                px = cosh(q) * s[kKinInvSinh][i];
                pz = sinh(q) * s[kKinInvSinh][i];
            }
            const double wa = s[kKinWA][i], w2a = s[kKinW2A][i];
            if constexpr (DIR) {
                const double uh = wa * px * cs, ah = w2a * px * sn;
                ux += uh * dc;
                uy += uh * ds;
                ax += ah * dc;
                ay += ah * ds;
            } else {
                ux += wa * px * cs;
                ax += w2a * px * sn;
            }
            uz += wa * pz * sn;
            az -= w2a * pz * cs;
        }
    }
    if (!active) return;
    if (a.eta) a.eta[o] = eta;
    if (a.vel) {
        a.vel[3 * o]     = ux;
        a.vel[3 * o + 1] = uy;
        a.vel[3 * o + 2] = uz;
    }
    if (a.acc) {
        a.acc[3 * o]     = ax;
        a.acc[3 * o + 1] = ay;
        a.acc[3 * o + 2] = az;
    }
}

void grow(hc::DeviceBuffer<double>& b, size_t n) {
    if (b.n < n) b.alloc(n);
}

}  // namespace
}  // namespace hc

extern "C" {

void hc_wave_kinematics_opts_default(hc_wave_kinematics_opts* o) {
    if (!o) return;
    o->mwl             = 0.0;
    o->regular_phase   = 0.0;
    o->wave_stretching = 1;
}

// Touches no step state, so it is not ordered against the direct queue (HC_API_BEGIN_HOT): a call between steps leaves a pass that
// is running alone.
int hc_wave_kinematics(hc_ctx* c, const hc_wave_kinematics_opts* opts, int n_points, const double* xyz, int n_times, const double* t,
                       double* eta, double* vel, double* acc) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    hc_wave_kinematics_opts o;
    hc_wave_kinematics_opts_default(&o);
    if (opts) o = *opts;
    require(std::isfinite(o.mwl) && std::isfinite(o.regular_phase), HC_ERR_INVALID, "non-finite mwl or regular_phase");
    require(n_points >= 0 && n_times >= 0, HC_ERR_INVALID, "negative point or time count");
    require((n_points == 0 || xyz) && (n_times == 0 || t), HC_ERR_INVALID, "null points or times");
    const bool dir = !c->wave_dir.empty();  // y enters the phase
    for (int p = 0; p < n_points; ++p)
        require(std::isfinite(xyz[3 * p]) && std::isfinite(xyz[3 * p + 2]) && (!dir || std::isfinite(xyz[3 * p + 1])), HC_ERR_INVALID,
                dir ? "non-finite coordinate of a point" : "non-finite x or z of a point");
    for (int j = 0; j < n_times; ++j) require(std::isfinite(t[j]), HC_ERR_INVALID, "non-finite time");
    const long long n = static_cast<long long>(n_points) * n_times;
    require(n <= hc::kKinMaxItems, HC_ERR_INVALID, "too many (point, time) pairs for one call");
    if (n == 0 || !(eta || vel || acc)) return HC_OK;
    // NoWave (wave_types.h:103-109), and an imported eta record without components (no spectrum: GetEtaIrregular & co. over no
    // component): zeros, no launch
    if (!hc::kin_has_components(c)) {
        if (eta) std::fill(eta, eta + n, 0.0);
        if (vel) std::fill(vel, vel + 3 * n, 0.0);
        if (acc) std::fill(acc, acc + 3 * n, 0.0);
        return HC_OK;
    }
    c->kin.refresh(c, o.regular_phase, c->stream);
    // one buffer: points, times, then the requested outputs
    const size_t n_in = 3 * static_cast<size_t>(n_points) + n_times;
    const size_t n_out = (eta ? n : 0) + (vel ? 3 * n : 0) + (acc ? 3 * n : 0);
    hc::grow(c->d_kin_io, n_in + n_out);
    double* d_xyz = c->d_kin_io.p;
    double* d_t   = d_xyz + 3 * static_cast<size_t>(n_points);
    double* d_out = d_t + n_times;
    hc::KinArgs a{};
    a.tab          = c->kin.tab.p;
    a.nf           = c->kin.nf;
    a.P            = n_points;
    a.T            = n_times;
    a.xyz          = d_xyz;
    a.t            = d_t;
    a.depth        = c->depth;
    a.mwl          = o.mwl;
    a.stretch      = (c->wave_kind != hc::kWaveRegular && o.wave_stretching) ? 1 : 0;  // RegularWave has none (:301-313)
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    if (eta) {
        a.eta = d_out;
        d_out += n;
    }
    if (vel) {
        a.vel = d_out;
        d_out += 3 * n;
    }
    if (acc) a.acc = d_out;
    HC_HIP(hipMemcpyAsync(d_xyz, xyz, 3 * static_cast<size_t>(n_points) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HC_HIP(hipMemcpyAsync(d_t, t, static_cast<size_t>(n_times) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const unsigned blocks = static_cast<unsigned>((n + hc::kKinThreads - 1) / hc::kKinThreads);
    if (c->kin.dir)
        hipLaunchKernelGGL(hc::wave_kinematics_kernel<true>, dim3(blocks), dim3(hc::kKinThreads), 0, c->stream, a);
    else
        hipLaunchKernelGGL(hc::wave_kinematics_kernel<false>, dim3(blocks), dim3(hc::kKinThreads), 0, c->stream, a);
    HC_HIP(hipGetLastError());
    if (eta) HC_HIP(hipMemcpyAsync(eta, a.eta, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (vel) HC_HIP(hipMemcpyAsync(vel, a.vel, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (acc) HC_HIP(hipMemcpyAsync(acc, a.acc, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    HC_API_END(c)
}

}  // extern "C"
