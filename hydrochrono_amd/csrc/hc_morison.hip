// hc_morison.hip -- Morison drag and inertia elements on the wave kinematics (include/hydrochrono_amd.h: hc_set_morison_elements,
// hc_morison_begin / hc_morison_end).  Not in the reference.  Off the step path: its own stream, component table, buffers and pinned
// staging; it reads and writes nothing a step uses, so it is not ordered against the direct queue (as hc_wave_kinematics).
// DESIGN.md 3.7c has the definition, the kernels and their invariants.
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kMorThreads = 256;  // work items per workgroup, one per element
constexpr int kMorElemDoubles = 9;  // r, cd_area, cm_vol

struct MorArgs {
    const double* tab;  // [kKinCols][nf] (hc_wave_kin.hpp); nf = 0: still water
    int nf;
    int n_items;
    const double* elem;   // [n_items][9], owned bodies one after the other
    const int* body;      // [n_items] body (of the system) an element belongs to
    const double* state;  // [12 N] pos | rpy | linvel | angvel, [3N] each
    int N;
    double t, depth, mwl, rho;
    double ramp;       // factor on u_f and a_f
    int stretch;       // Wheeler stretching
    int finite_depth;  // 0: water depth +inf
    double* item;      // [n_items][6] (F, M) of every element
};

// One work item per element.  Every item derives its body's frame from the 12 state values, sums the wave components in index
// order from the same LDS tiles (the loop of wave_kinematics_kernel) and writes its own 6-vector: its bits depend on its body's
// state, its own data, the table, t and the options, not on where in the grid it sits.  Without stretching eta comes out of the
// kinematics pass (the same sincos); with stretching it is summed first.
__global__ void __launch_bounds__(kMorThreads) morison_items_kernel(MorArgs a) {
    __shared__ double s[kKinCols][kKinTile];
    const int o       = blockIdx.x * kMorThreads + threadIdx.x;
    const bool active = o < a.n_items;
    const int e       = active ? o : 0;  // items past the end evaluate item 0 and store nothing (all take part in the staging)
    const int b       = a.body[e];
    const double* el  = a.elem + static_cast<size_t>(kMorElemDoubles) * e;
    const double* pos = a.state + 3 * b;
    const double* rpy = pos + 3 * a.N;
    const double* lin = rpy + 3 * a.N;
    const double* ang = lin + 3 * a.N;

    // ---- R = Rx(rpy0) Ry(rpy1) Rz(rpy2), d = R r, p = pos + d ----
    double sa, ca, sb, cb, sc, cc;
    sincos(rpy[0], &sa, &ca);
    sincos(rpy[1], &sb, &cb);
    sincos(rpy[2], &sc, &cc);
    const double r00 = cb * cc, r01 = -cb * sc, r02 = sb;
    const double r10 = ca * sc + sa * sb * cc, r11 = ca * cc - sa * sb * sc, r12 = -sa * cb;
    const double r20 = sa * sc - ca * sb * cc, r21 = sa * cc + ca * sb * sc, r22 = ca * cb;
    const double d0 = r00 * el[0] + r01 * el[1] + r02 * el[2];
    const double d1 = r10 * el[0] + r11 * el[1] + r12 * el[2];
    const double d2 = r20 * el[0] + r21 * el[1] + r22 * el[2];
    const double x = pos[0] + d0, z = pos[2] + d2, t = a.t;

    // ---- eta first under stretching (wave_kinematics_kernel) ----
    double eta = 0.0;
    if (a.stretch) {
        for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
            const int m = min(kKinTile, a.nf - i0);
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += kMorThreads) {
                s[kKinAmp][i]   = a.tab[kKinAmp * a.nf + i0 + i];
                s[kKinOmega][i] = a.tab[kKinOmega * a.nf + i0 + i];
                s[kKinK][i]     = a.tab[kKinK * a.nf + i0 + i];
                s[kKinPhase][i] = a.tab[kKinPhase * a.nf + i0 + i];
            }
            __syncthreads();
            for (int i = 0; i < m; ++i) eta += s[kKinAmp][i] * cos(s[kKinK][i] * x - s[kKinOmega][i] * t + s[kKinPhase][i]);
        }
    }
    double zs = z;
    if (a.stretch) {
        const double zr = z - a.mwl;
        zs = a.finite_depth ? a.depth * (zr - eta) / (a.depth + eta) : zr - eta;
    }
    const double ze = zs - a.mwl;  // under stretching mwl is subtracted a second time, as in the reference

    // ---- velocity and acceleration (and eta without stretching) ----
    double ux = 0.0, uz = 0.0, ax = 0.0, az = 0.0, eta1 = 0.0;
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int m = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += kMorThreads) {
#pragma unroll
            for (int col = 0; col < kKinCols; ++col) s[col][i] = a.tab[col * a.nf + i0 + i];
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const double k = s[kKinK][i];
            double sn, cs;
            sincos(k * x - s[kKinOmega][i] * t + s[kKinPhase][i], &sn, &cs);
            double px, pz;
            if (s[kKinDeep][i] != 0.0) {  // (the same branch for every item: no divergence)
                px = pz = exp(k * ze);
            } else {
                const double q = k * (ze + a.depth);
                px = cosh(q) * s[kKinInvSinh][i];
                pz = sinh(q) * s[kKinInvSinh][i];
            }
            const double wa = s[kKinWA][i], w2a = s[kKinW2A][i];
            eta1 += s[kKinAmp][i] * cs;
            ux += wa * px * cs;
            uz += wa * pz * sn;
            ax += w2a * px * sn;
            az -= w2a * pz * cs;
        }
    }
    if (!active) return;
    if (!a.stretch) eta = eta1;

    double* out = a.item + 6 * static_cast<size_t>(o);
    if (!(z - a.mwl <= eta)) {  // dry
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = 0.0;
        return;
    }
    // ---- relative flow in the body frame, force per body axis, back to the world frame ----
    const double w0 = ang[0], w1 = ang[1], w2 = ang[2];
    const double q0 = a.ramp * ux - (lin[0] + (w1 * d2 - w2 * d1));
    const double q1 = -(lin[1] + (w2 * d0 - w0 * d2));
    const double q2 = a.ramp * uz - (lin[2] + (w0 * d1 - w1 * d0));
    const double afx = a.ramp * ax, afz = a.ramp * az;
    const double u0 = r00 * q0 + r10 * q1 + r20 * q2, a0 = r00 * afx + r20 * afz;
    const double u1 = r01 * q0 + r11 * q1 + r21 * q2, a1 = r01 * afx + r21 * afz;
    const double u2 = r02 * q0 + r12 * q1 + r22 * q2, a2 = r02 * afx + r22 * afz;
    const double f0 = 0.5 * a.rho * el[3] * fabs(u0) * u0 + a.rho * el[6] * a0;
    const double f1 = 0.5 * a.rho * el[4] * fabs(u1) * u1 + a.rho * el[7] * a1;
    const double f2 = 0.5 * a.rho * el[5] * fabs(u2) * u2 + a.rho * el[8] * a2;
    const double F0 = r00 * f0 + r01 * f1 + r02 * f2;
    const double F1 = r10 * f0 + r11 * f1 + r12 * f2;
    const double F2 = r20 * f0 + r21 * f1 + r22 * f2;
    out[0] = F0;
    out[1] = F1;
    out[2] = F2;
    out[3] = d1 * F2 - d2 * F1;
    out[4] = d2 * F0 - d0 * F2;
    out[5] = d0 * F1 - d1 * F0;
}

// One work item per (owned body, component): the serial sum over the body's elements in index order.
__global__ void __launch_bounds__(kMorThreads) morison_sum_kernel(const double* item, const int* off, int rows, double* out) {
    const int row = blockIdx.x * kMorThreads + threadIdx.x;
    if (row >= rows) return;
    const int b = row / 6, k = row - 6 * b;
    double acc = 0.0;
    for (int e = off[b]; e < off[b + 1]; ++e) acc += item[6 * static_cast<size_t>(e) + k];
    out[row] = acc;
}

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// the device copy of the owned bodies' lists, body-major
void upload_elements(hc_ctx* c) {
    std::vector<double> elem;
    std::vector<int> body, off(c->nloc + 1, 0);
    for (int b = c->b0; b < c->b1; ++b) {
        for (const hc_morison_element& m : c->mor_elems[b]) {
            elem.insert(elem.end(), m.r, m.r + 3);
            elem.insert(elem.end(), m.cd_area, m.cd_area + 3);
            elem.insert(elem.end(), m.cm_vol, m.cm_vol + 3);
            body.push_back(b);
        }
        off[b - c->b0 + 1] = static_cast<int>(body.size());
    }
    c->d_mor_elem.upload(elem, c->stream_mor);
    c->d_mor_body.upload(body, c->stream_mor);
    c->d_mor_off.upload(off, c->stream_mor);
    c->mor_items = static_cast<int>(body.size());
    if (c->d_mor_item.n < 6 * body.size()) c->d_mor_item.alloc(6 * body.size());
    c->mor_dirty = false;
}

// The component table of the wave model in force, a copy of this path's own (hc_wave_kinematics may rebuild its table for another
// regular phase while a launch of this one is in flight).
void morison_table(hc_ctx* c) {
    const double phase = c->mor_opts.regular_phase;
    const bool regular = c->wave_kind == kWaveRegular;
    if (c->mor_serial == c->wave_serial && (!regular || std::memcmp(&c->mor_phase, &phase, sizeof(double)) == 0)) return;
    const std::vector<double> tab = kin_table_host(c, phase);
    c->d_mor_tab.upload(tab, c->stream_mor);
    c->mor_nf     = static_cast<int>(tab.size() / kKinCols);
    c->mor_serial = c->wave_serial;
    c->mor_phase  = phase;
}

void morison_enqueue(hc_ctx* c, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel) {
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    if (c->mor_dirty) upload_elements(c);
    morison_table(c);
    if (c->h_mor_state.n < 4 * n3) c->h_mor_state.alloc(4 * n3);
    if (c->d_mor_state.n < 4 * n3) c->d_mor_state.alloc(4 * n3);
    if (c->h_mor_out.n < static_cast<size_t>(c->Dloc)) c->h_mor_out.alloc(c->Dloc);
    if (c->d_mor_out.n < static_cast<size_t>(c->Dloc)) c->d_mor_out.alloc(c->Dloc);
    std::copy(pos, pos + n3, c->h_mor_state.p);
    std::copy(rpy, rpy + n3, c->h_mor_state.p + n3);
    std::copy(linvel, linvel + n3, c->h_mor_state.p + 2 * n3);
    std::copy(angvel, angvel + n3, c->h_mor_state.p + 3 * n3);
    const bool synthesised = (c->wave_kind == kWaveIrregular && !c->eta_record) || c->wave_kind == kWaveSpectral;
    const double rd = c->irr.ramp_duration;
    MorArgs a{};
    a.tab          = c->d_mor_tab.p;
    a.nf           = c->mor_nf;
    a.n_items      = c->mor_items;
    a.elem         = c->d_mor_elem.p;
    a.body         = c->d_mor_body.p;
    a.state        = c->d_mor_state.p;
    a.N            = c->N;
    a.t            = t;
    a.depth        = c->depth;
    a.mwl          = c->mor_opts.mwl;
    a.rho          = c->rho;
    a.ramp         = (synthesised && rd > 0.0 && t < rd) ? (t <= 0.0 ? 0.0 : t / rd) : 1.0;  // the rule of the spectral excitation (hc_kernels.hip)
    a.stretch      = (synthesised && c->mor_opts.wave_stretching) ? 1 : 0;  // RegularWave has none
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    a.item         = c->d_mor_item.p;
    hipStream_t st = c->stream_mor;
    HC_HIP(hipMemcpyAsync(c->d_mor_state.p, c->h_mor_state.p, 4 * n3 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(morison_items_kernel, dim3((a.n_items + kMorThreads - 1) / kMorThreads), dim3(kMorThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    hipLaunchKernelGGL(morison_sum_kernel, dim3((c->Dloc + kMorThreads - 1) / kMorThreads), dim3(kMorThreads), 0, st, c->d_mor_item.p,
                       c->d_mor_off.p, c->Dloc, c->d_mor_out.p);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(c->h_mor_out.p, c->d_mor_out.p, static_cast<size_t>(c->Dloc) * sizeof(double), hipMemcpyDeviceToHost, st));
}

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_morison_elements(hc_ctx* c, int body, const hc_morison_element* elems, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n >= 0 && n <= hc::kMorisonMaxElements, HC_ERR_INVALID, "element count negative or above the limit per body");
    require(n == 0 || elems, HC_ERR_INVALID, "null element list");
    require(!c->mor_pending, HC_ERR_INVALID, "a Morison evaluation is in flight (hc_morison_end has not been called)");
    for (int e = 0; e < n; ++e) {
        const hc_morison_element& m = elems[e];
        require(hc::all_finite(m.r, 3) && hc::all_finite(m.cd_area, 3) && hc::all_finite(m.cm_vol, 3), HC_ERR_INVALID,
                "non-finite value in a Morison element");
        for (int k = 0; k < 3; ++k) require(m.cd_area[k] >= 0.0 && m.cm_vol[k] >= 0.0, HC_ERR_INVALID, "negative Morison coefficient");
    }
    if (!c->stream_mor) HC_HIP(hipStreamCreateWithFlags(&c->stream_mor, hipStreamNonBlocking));
    if (c->mor_elems.empty()) c->mor_elems.resize(c->N);
    c->mor_elems[body].assign(elems, elems + n);
    c->mor_dirty = true;
    HC_API_END(c)
}

int hc_get_morison_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = c->mor_elems.empty() ? 0 : static_cast<int>(c->mor_elems[body].size());
    HC_API_END(c)
}

int hc_set_morison_options(hc_ctx* c, const hc_wave_kinematics_opts* o) {
    HC_API_BEGIN_HOT(c)
    hc_wave_kinematics_opts v;
    hc_wave_kinematics_opts_default(&v);
    if (o) v = *o;
    require(std::isfinite(v.mwl) && std::isfinite(v.regular_phase), HC_ERR_INVALID, "non-finite mwl or regular_phase");
    require(!c->mor_pending, HC_ERR_INVALID, "a Morison evaluation is in flight (hc_morison_end has not been called)");
    c->mor_opts = v;
    HC_API_END(c)
}

int hc_morison_begin(hc_ctx* c, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    require(!c->mor_pending, HC_ERR_INVALID, "hc_morison_begin twice without hc_morison_end");
    require(pos && rpy && linvel && angvel, HC_ERR_INVALID, "null state");
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    require(std::isfinite(t) && hc::all_finite(pos, n3) && hc::all_finite(rpy, n3) && hc::all_finite(linvel, n3) && hc::all_finite(angvel, n3),
            HC_ERR_INVALID, "non-finite time or state");
    int items = 0;
    if (!c->mor_elems.empty())
        for (int b = c->b0; b < c->b1; ++b) items += static_cast<int>(c->mor_elems[b].size());
    if (items == 0) {
        c->mor_pending = 1;
        return HC_OK;
    }
    try {
        hc::morison_enqueue(c, t, pos, rpy, linvel, angvel);
    } catch (...) {
        (void)hipStreamSynchronize(c->stream_mor);  // nothing stays pending
        throw;
    }
    c->mor_pending = 2;
    HC_API_END(c)
}

int hc_morison_end(hc_ctx* c, double* out) {
    HC_API_BEGIN_HOT(c)
    require(c->mor_pending != 0, HC_ERR_INVALID, "hc_morison_end without hc_morison_begin");
    const int what = c->mor_pending;
    c->mor_pending = 0;
    if (what == 2) HC_HIP(hipStreamSynchronize(c->stream_mor));
    require(out != nullptr, HC_ERR_INVALID, "null output");
    if (what == 2) std::copy(c->h_mor_out.p, c->h_mor_out.p + c->Dloc, out);
    else std::fill(out, out + c->Dloc, 0.0);
    HC_API_END(c)
}

int hc_compute_morison(hc_ctx* c, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel, double* out) {
    const int rc = hc_morison_begin(c, t, pos, rpy, linvel, angvel);
    return rc != HC_OK ? rc : hc_morison_end(c, out);
}

}  // extern "C"
