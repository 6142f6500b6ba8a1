// hc_drift.hip -- second-order wave drift forces from difference-frequency QTF tables (include/hydrochrono_amd.h: hc_set_drift_qtf,
// hc_drift_begin / hc_drift_end).  Not in the reference.  Off the step path: its own stream, component table, table copies and pinned
// staging; it reads and writes nothing a step uses, so it is not ordered against the direct queue (as hc_morison.hip).
// DESIGN.md 3.7e has the definition, the projected evaluation form, the kernel and its invariants.
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"

#include <algorithm>

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kDriftThreads = 256;  // work items per workgroup: one per grid bin in phase 1 (kDriftMaxFreq bins at the most)
static_assert(kDriftMaxFreq <= kDriftThreads, "one lane per bin of the frequency grid");
static_assert(kKinTile == kDriftThreads, "one lane per component of a staged tile");

// per (owned body with a table): [kDescWords] 64-bit words
enum DriftDesc { kDescBody = 0, kDescNq, kDescRowPtr, kDescP, kDescQ, kDescE, kDescWords };

struct DriftArgs {
    const double* tab;      // [kKinCols][nf] (hc_wave_kin.hpp)
    int nf;
    int mode;               // 1 mean drift, 2 Newman, 3 full QTF
    const long long* desc;  // [slots][kDescWords]: body, nq, first row pointer, offsets of P, Q (-1: none) and E
    const int* rowptr;      // per slot nq + 1 entries: bin m owns the entries [rowptr[m], rowptr[m + 1])
    const int* ent_idx;     // component index of an entry, ascending within a bin
    const double* ent_w;    // its interpolation weight
    const double* pq;       // the tables, [6][nq][nq] each
    const double* em;       // E_m = sum_i W[i][m] A_i^2 per slot and bin
    const double* pos;      // [3 N]
    double t, ramp2;
    double* out;            // [slots][6]
};

// One workgroup per (slot, row d).  Phase 1: u_i = A_i cos theta_i, w_i = A_i sin theta_i tile by tile through LDS; lane m < nq adds
// its bin's entries in component order into one accumulator pair (U_m, V_m), whatever the tiling.  Phase 2: the lanes stride over
// the nq^2 table entries in ascending e, and the 256 partials go through a tree whose shape depends on the lane index alone.  A
// row's bits depend on its body's table, pos[b].x, t, the component table and the mode only.
__global__ void __launch_bounds__(kDriftThreads) drift_qtf_kernel(DriftArgs a) {
    __shared__ double su[kKinTile], sw[kKinTile];
    __shared__ double sU[kDriftThreads], sV[kDriftThreads];
    __shared__ double red[4][kDriftThreads];
    const int tid          = threadIdx.x;
    const int slot         = blockIdx.x / 6, d = blockIdx.x - 6 * slot;
    const long long* desc  = a.desc + static_cast<size_t>(kDescWords) * slot;
    const int nq           = static_cast<int>(desc[kDescNq]);
    const int nq2          = nq * nq;
    const double* P        = a.pq + desc[kDescP] + static_cast<size_t>(d) * nq2;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;

    if (a.mode == 1) {
        if (tid < nq) p0 = P[tid * nq + tid] * a.em[desc[kDescE] + tid];
    } else {
        const double x = a.pos[3 * desc[kDescBody]], t = a.t;
        const int* rp  = a.rowptr + desc[kDescRowPtr];
        int p          = tid < nq ? rp[tid] : 0;
        const int pend = tid < nq ? rp[tid + 1] : 0;
        double U = 0.0, V = 0.0;
        for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
            const int m = min(kKinTile, a.nf - i0);
            __syncthreads();
            if (tid < m) {
                const int i = i0 + tid;
                double sn, cs;
                sincos(a.tab[kKinK * a.nf + i] * x - a.tab[kKinOmega * a.nf + i] * t + a.tab[kKinPhase * a.nf + i], &sn, &cs);
                const double A = a.tab[kKinAmp * a.nf + i];
                su[tid]        = A * cs;
                sw[tid]        = A * sn;
            }
            __syncthreads();
            while (p < pend) {
                const int i = a.ent_idx[p];
                if (i >= i0 + m) break;
                const double w = a.ent_w[p];
                U += w * su[i - i0];
                V += w * sw[i - i0];
                ++p;
            }
        }
        sU[tid] = U;  // zero for the lanes past the grid
        sV[tid] = V;
        __syncthreads();
        if (a.mode == 2) {
            if (tid < nq) {
                const double D = P[tid * nq + tid];
                p0 = D * U;
                p1 = U;
                p2 = D * V;
                p3 = V;
            }
        } else if (desc[kDescQ] >= 0) {
            const double* Q = a.pq + desc[kDescQ] + static_cast<size_t>(d) * nq2;
            for (int e = tid; e < nq2; e += kDriftThreads) {
                const int m = e / nq, n = e - m * nq;
                const double Um = sU[m], Vm = sV[m], Un = sU[n], Vn = sV[n];
                p0 += P[e] * (Um * Un + Vm * Vn) - Q[e] * (Vm * Un - Um * Vn);
            }
        } else {
            for (int e = tid; e < nq2; e += kDriftThreads) {
                const int m = e / nq, n = e - m * nq;
                p0 += P[e] * (sU[m] * sU[n] + sV[m] * sV[n]);
            }
        }
    }
    red[0][tid] = p0;
    red[1][tid] = p1;
    red[2][tid] = p2;
    red[3][tid] = p3;
    // ---- fixed-shape tree over the 256 lanes: lane l adds lane l + h for h = 128, 64, ..., 1 (nl_panels_kernel) ----
    for (int h = kDriftThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + h];
        }
    }
    if (tid == 0) {
        const double F = a.mode == 2 ? red[0][0] * red[1][0] + red[2][0] * red[3][0] : red[0][0];
        a.out[6 * static_cast<size_t>(slot) + d] = F * a.ramp2;
    }
}

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// The device copy of the owned bodies' tables (when a table has changed) and, per owned body with a table, the map from grid bin
// to (component, weight) and E_m for the component table in force (when a table or the wave model has changed).
void drift_layout(hc_ctx* c) {
    const double phase = c->drift_phase_opt;
    const bool regular = c->wave_kind == kWaveRegular;
    const bool same_waves = c->drift_serial == c->wave_serial && (!regular || std::memcmp(&c->drift_phase, &phase, sizeof(double)) == 0);
    if (same_waves && !c->drift_dirty) return;
    hipStream_t st = c->stream_drift;
    std::vector<double> tab;
    if (!same_waves) {
        tab = kin_table_host(c, phase);
        c->d_drift_tab.upload(tab, st);
        c->drift_nf     = static_cast<int>(tab.size() / kKinCols);
        c->drift_serial = c->wave_serial;
        c->drift_phase  = phase;
        c->drift_amp.assign(tab.begin() + static_cast<size_t>(kKinAmp) * c->drift_nf, tab.begin() + static_cast<size_t>(kKinAmp + 1) * c->drift_nf);
        c->drift_omega.assign(tab.begin() + static_cast<size_t>(kKinOmega) * c->drift_nf, tab.begin() + static_cast<size_t>(kKinOmega + 1) * c->drift_nf);
    }
    const int nf = c->drift_nf;
    std::vector<long long> desc;
    std::vector<int> rowptr, idx, slot_body;
    std::vector<double> wgt, em, pq;
    size_t pq_n = 0;  // doubles of the tables before this body's
    for (int b = c->b0; b < c->b1; ++b) {
        const DriftTable& T = c->drift_tabs[b];
        if (T.nq == 0) continue;
        const int nq = T.nq;
        const size_t n6 = 6 * static_cast<size_t>(nq) * nq;
        // cell and weight of every component inside [Omega_0, Omega_{nq-1}] (both ends inside)
        std::vector<std::vector<std::pair<int, double>>> bins(nq);
        std::vector<double> E(nq, 0.0);
        for (int i = 0; i < nf; ++i) {
            const double w = c->drift_omega[i], A = c->drift_amp[i];
            if (!(w >= T.omega.front() && w <= T.omega.back())) continue;
            int m = static_cast<int>(std::upper_bound(T.omega.begin(), T.omega.end(), w) - T.omega.begin()) - 1;  // largest m with Omega_m <= w
            m     = std::min(m, nq - 2);
            const double lam = (w - T.omega[m]) / (T.omega[m + 1] - T.omega[m]);
            const double w0 = 1.0 - lam, w1 = lam;
            if (w0 != 0.0) {
                bins[m].emplace_back(i, w0);
                E[m] += w0 * (A * A);
            }
            if (w1 != 0.0) {
                bins[m + 1].emplace_back(i, w1);
                E[m + 1] += w1 * (A * A);
            }
        }
        desc.push_back(b);
        desc.push_back(nq);
        desc.push_back(static_cast<long long>(rowptr.size()));
        desc.push_back(static_cast<long long>(pq_n));
        desc.push_back(T.has_q ? static_cast<long long>(pq_n + n6) : -1LL);
        desc.push_back(static_cast<long long>(em.size()));
        for (int m = 0; m < nq; ++m) {
            rowptr.push_back(static_cast<int>(idx.size()));
            for (const auto& e : bins[m]) {
                idx.push_back(e.first);
                wgt.push_back(e.second);
            }
        }
        rowptr.push_back(static_cast<int>(idx.size()));
        em.insert(em.end(), E.begin(), E.end());
        pq_n += n6 * (T.has_q ? 2 : 1);
        if (c->drift_dirty) {  // otherwise the device copy is in place
            pq.insert(pq.end(), T.P.begin(), T.P.end());
            if (T.has_q) pq.insert(pq.end(), T.Q.begin(), T.Q.end());
        }
        slot_body.push_back(b - c->b0);
    }
    if (idx.empty()) {  // keep the pointers valid where no component falls inside a grid
        idx.push_back(0);
        wgt.push_back(0.0);
    }
    c->d_drift_desc.upload(desc, st);
    c->d_drift_rowptr.upload(rowptr, st);
    c->d_drift_idx.upload(idx, st);
    c->d_drift_w.upload(wgt, st);
    c->d_drift_em.upload(em, st);
    if (c->drift_dirty) c->d_drift_pq.upload(pq, st);
    c->drift_slot_body = slot_body;
    c->drift_dirty     = false;
}

void drift_enqueue(hc_ctx* c, double t, const double* pos) {
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    drift_layout(c);
    const size_t nout = 6 * c->drift_slot_body.size();
    if (c->h_drift_pos.n < n3) c->h_drift_pos.alloc(n3);
    if (c->d_drift_pos.n < n3) c->d_drift_pos.alloc(n3);
    if (c->h_drift_out.n < nout) c->h_drift_out.alloc(nout);
    if (c->d_drift_out.n < nout) c->d_drift_out.alloc(nout);
    std::copy(pos, pos + n3, c->h_drift_pos.p);
    const bool synthesised = (c->wave_kind == kWaveIrregular && !c->eta_record) || c->wave_kind == kWaveSpectral;
    const double rd        = c->irr.ramp_duration;
    const double ramp      = (synthesised && rd > 0.0 && t < rd) ? (t <= 0.0 ? 0.0 : t / rd) : 1.0;  // the rule of the Morison term
    DriftArgs a{};
    a.tab     = c->d_drift_tab.p;
    a.nf      = c->drift_nf;
    a.mode    = c->drift_mode;
    a.desc    = c->d_drift_desc.p;
    a.rowptr  = c->d_drift_rowptr.p;
    a.ent_idx = c->d_drift_idx.p;
    a.ent_w   = c->d_drift_w.p;
    a.pq      = c->d_drift_pq.p;
    a.em      = c->d_drift_em.p;
    a.pos     = c->d_drift_pos.p;
    a.t       = t;
    a.ramp2   = ramp * ramp;  // second order in the amplitude
    a.out     = c->d_drift_out.p;
    hipStream_t st = c->stream_drift;
    HC_HIP(hipMemcpyAsync(c->d_drift_pos.p, c->h_drift_pos.p, n3 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(drift_qtf_kernel, dim3(static_cast<unsigned>(nout)), dim3(kDriftThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(c->h_drift_out.p, c->d_drift_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, st));
}

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_drift_qtf(hc_ctx* c, int body, int nq, const double* omega, const double* P, const double* Q) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(nq == 0 || (nq >= 2 && nq <= hc::kDriftMaxFreq), HC_ERR_INVALID, "drift frequency count must be 0 or 2 .. 256");
    require(nq == 0 || (omega && P), HC_ERR_INVALID, "null frequency grid or QTF table");
    require(!c->drift_pending, HC_ERR_INVALID, "a drift evaluation is in flight (hc_drift_end has not been called)");
    const size_t n6 = 6 * static_cast<size_t>(nq) * nq;
    if (nq) {
        require(hc::all_finite(omega, nq) && hc::all_finite(P, n6) && (!Q || hc::all_finite(Q, n6)), HC_ERR_INVALID,
                "non-finite value in a drift table");
        for (int m = 1; m < nq; ++m) require(omega[m] > omega[m - 1], HC_ERR_INVALID, "the drift frequency grid is not strictly increasing");
    }
    if (!c->stream_drift) HC_HIP(hipStreamCreateWithFlags(&c->stream_drift, hipStreamNonBlocking));
    if (c->drift_tabs.empty()) c->drift_tabs.resize(c->N);
    hc::DriftTable& T = c->drift_tabs[body];
    T.nq              = nq;
    T.has_q           = nq != 0 && Q != nullptr;
    T.omega.assign(omega, omega + nq);
    T.P.assign(P, P + n6);
    T.Q.assign(Q, Q + (T.has_q ? n6 : 0));
    c->drift_dirty = true;
    HC_API_END(c)
}

int hc_get_drift_qtf_size(hc_ctx* c, int body, int* nq) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && nq, HC_ERR_INVALID, "body index out of range or null pointer");
    *nq = c->drift_tabs.empty() ? 0 : c->drift_tabs[body].nq;
    HC_API_END(c)
}

int hc_set_drift_mode(hc_ctx* c, int mode) {
    HC_API_BEGIN_HOT(c)
    require(mode >= 0 && mode <= 3, HC_ERR_INVALID, "drift mode must be 0, 1, 2 or 3");
    require(!c->drift_pending, HC_ERR_INVALID, "a drift evaluation is in flight (hc_drift_end has not been called)");
    c->drift_mode = mode;
    HC_API_END(c)
}

int hc_get_drift_mode(hc_ctx* c, int* mode) {
    HC_API_BEGIN_HOT(c)
    require(mode != nullptr, HC_ERR_INVALID, "null pointer");
    *mode = c->drift_mode;
    HC_API_END(c)
}

int hc_set_drift_options(hc_ctx* c, const hc_wave_kinematics_opts* o) {
    HC_API_BEGIN_HOT(c)
    hc_wave_kinematics_opts v;
    hc_wave_kinematics_opts_default(&v);
    if (o) v = *o;
    require(std::isfinite(v.regular_phase), HC_ERR_INVALID, "non-finite regular_phase");
    require(!c->drift_pending, HC_ERR_INVALID, "a drift evaluation is in flight (hc_drift_end has not been called)");
    c->drift_phase_opt = v.regular_phase;
    HC_API_END(c)
}

int hc_drift_begin(hc_ctx* c, double t, const double* pos) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    require(!c->drift_pending, HC_ERR_INVALID, "hc_drift_begin twice without hc_drift_end");
    require(pos != nullptr, HC_ERR_INVALID, "null state");
    require(std::isfinite(t) && hc::all_finite(pos, 3 * static_cast<size_t>(c->N)), HC_ERR_INVALID, "non-finite time or position");
    require(c->drift_mode == 0 || c->wave_dir.empty(), HC_ERR_UNSUPPORTED,
            "the QTF tables hold one heading: wave drift forces are not available while wave directions are set (hc_set_wave_directions)");
    bool any = false;
    if (!c->drift_tabs.empty())
        for (int b = c->b0; b < c->b1; ++b) any = any || c->drift_tabs[b].nq != 0;
    // components: none for NoWave and for an imported eta record (kin_table_host)
    const bool waves = c->wave_kind == hc::kWaveRegular || c->wave_kind == hc::kWaveSpectral || (c->wave_kind == hc::kWaveIrregular && !c->eta_record);
    if (!any || c->drift_mode == 0 || !waves) {
        c->drift_pending = 1;
        return HC_OK;
    }
    try {
        hc::drift_enqueue(c, t, pos);
    } catch (...) {
        (void)hipStreamSynchronize(c->stream_drift);  // nothing stays pending
        throw;
    }
    c->drift_pending = 2;
    HC_API_END(c)
}

int hc_drift_end(hc_ctx* c, double* out) {
    HC_API_BEGIN_HOT(c)
    require(c->drift_pending != 0, HC_ERR_INVALID, "hc_drift_end without hc_drift_begin");
    const int what   = c->drift_pending;
    c->drift_pending = 0;
    if (what == 2) HC_HIP(hipStreamSynchronize(c->stream_drift));
    require(out != nullptr, HC_ERR_INVALID, "null output");
    std::fill(out, out + c->Dloc, 0.0);  // bodies without a table
    if (what == 2)
        for (size_t s = 0; s < c->drift_slot_body.size(); ++s)
            std::copy(c->h_drift_out.p + 6 * s, c->h_drift_out.p + 6 * s + 6, out + 6 * static_cast<size_t>(c->drift_slot_body[s]));
    HC_API_END(c)
}

int hc_compute_drift(hc_ctx* c, double t, const double* pos, double* out) {
    const int rc = hc_drift_begin(c, t, pos);
    return rc != HC_OK ? rc : hc_drift_end(c, out);
}

}  // extern "C"
