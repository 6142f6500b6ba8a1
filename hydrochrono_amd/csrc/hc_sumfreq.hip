// hc_sumfreq.hip -- second-order wave forces from sum-frequency QTF tables (include/hydrochrono_amd.h: hc_set_sum_qtf,
// hc_sum_qtf_begin / hc_sum_qtf_end).  Not in the reference.  The counterpart of hc_drift.hip above the wave band: the same component
// table, bin map and projections U_m, V_m, the signs of cos / sin (theta_i + theta_j).  Off the step path: its own stream, component
// table, table copies and pinned staging; it reads and writes nothing a step uses, so it is not ordered against the direct queue.
// DESIGN.md 3.7i has the definition, the projected evaluation form, the kernel and its invariants.
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"

#include <algorithm>

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kSumThreads = 256;  // work items per workgroup: one per grid bin in phase 1 (kDriftMaxFreq bins at the most)
static_assert(kDriftMaxFreq <= kSumThreads, "one lane per bin of the frequency grid");
static_assert(kKinTile == kSumThreads, "one lane per component of a staged tile");

// per (owned body with a table): [kDescWords] 64-bit words
enum SumDesc { kDescBody = 0, kDescNq, kDescRowPtr, kDescP, kDescQ, kDescWords };

struct SumArgs {
    const double* tab;      // [kKinCols][nf] (hc_wave_kin.hpp)
    int nf;
    const long long* desc;  // [slots][kDescWords]: body, nq, first row pointer, offsets of P and Q (-1: none)
    const int* rowptr;      // per slot nq + 1 entries: bin m owns the entries [rowptr[m], rowptr[m + 1])
    const int* ent_idx;     // component index of an entry, ascending within a bin
    const double* ent_w;    // its interpolation weight
    const double* pq;       // the tables, [6][nq][nq] each
    const double* pos;      // [3 N]
    double t, ramp2;
    double* out;            // [slots][6]
};

// One workgroup per (slot, row d).  Phase 1 is that of drift_qtf_kernel: u_i = A_i cos theta_i, w_i = A_i sin theta_i tile by tile
// through LDS; lane m < nq adds its bin's entries in component order into one accumulator pair (U_m, V_m), whatever the tiling.
// Phase 2: the lanes stride over the nq^2 table entries in ascending e, and the 256 partials go through a tree whose shape depends on
// the lane index alone.  A row's bits depend on its body's table, pos[b].x, t and the component table only.
__global__ void __launch_bounds__(kSumThreads) sum_qtf_kernel(SumArgs a) {
    __shared__ double su[kKinTile], sw[kKinTile];
    __shared__ double sU[kSumThreads], sV[kSumThreads];
    __shared__ double red[kSumThreads];
    const int tid         = threadIdx.x;
    const int slot        = blockIdx.x / 6, d = blockIdx.x - 6 * slot;
    const long long* desc = a.desc + static_cast<size_t>(kDescWords) * slot;
    const int nq          = static_cast<int>(desc[kDescNq]);
    const int nq2         = nq * nq;
    const double* P       = a.pq + desc[kDescP] + static_cast<size_t>(d) * nq2;
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
    double acc = 0.0;
    if (desc[kDescQ] >= 0) {
        const double* Q = a.pq + desc[kDescQ] + static_cast<size_t>(d) * nq2;
        for (int e = tid; e < nq2; e += kSumThreads) {
            const int m = e / nq, n = e - m * nq;
            const double Um = sU[m], Vm = sV[m], Un = sU[n], Vn = sV[n];
            acc += P[e] * (Um * Un - Vm * Vn) - Q[e] * (Vm * Un + Um * Vn);
        }
    } else {
        for (int e = tid; e < nq2; e += kSumThreads) {
            const int m = e / nq, n = e - m * nq;
            acc += P[e] * (sU[m] * sU[n] - sV[m] * sV[n]);
        }
    }
    red[tid] = acc;
    // ---- fixed-shape tree over the 256 lanes: lane l adds lane l + h for h = 128, 64, ..., 1 (drift_qtf_kernel) ----
    for (int h = kSumThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] += red[tid + h];
    }
    if (tid == 0) a.out[6 * static_cast<size_t>(slot) + d] = red[0] * a.ramp2;
}

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// The device copy of the owned bodies' tables (when a table has changed) and, per owned body with a table, the map from grid bin
// to (component, weight) for the component table in force (when a table or the wave model has changed).  The cell and weight rules
// are those of drift_layout (hc_drift.hip), word for word.
void sum_layout(hc_ctx* c) {
    const double phase = c->sum_phase_opt;
    const bool regular = c->wave_kind == kWaveRegular;
    const bool same_waves = c->sum_serial == c->wave_serial && (!regular || std::memcmp(&c->sum_phase, &phase, sizeof(double)) == 0);
    if (same_waves && !c->sum_dirty) return;
    hipStream_t st = c->stream_sum;
    std::vector<double> tab;
    if (!same_waves) {
        tab = kin_table_host(c, phase);
        c->d_sum_tab.upload(tab, st);
        c->sum_nf     = static_cast<int>(tab.size() / kKinCols);
        c->sum_serial = c->wave_serial;
        c->sum_phase  = phase;
        c->sum_omega.assign(tab.begin() + static_cast<size_t>(kKinOmega) * c->sum_nf, tab.begin() + static_cast<size_t>(kKinOmega + 1) * c->sum_nf);
    }
    const int nf = c->sum_nf;
    std::vector<long long> desc;
    std::vector<int> rowptr, idx, slot_body;
    std::vector<double> wgt, pq;
    size_t pq_n = 0;  // doubles of the tables before this body's
    for (int b = c->b0; b < c->b1; ++b) {
        const DriftTable& T = c->sum_tabs[b];
        if (T.nq == 0) continue;
        const int nq = T.nq;
        const size_t n6 = 6 * static_cast<size_t>(nq) * nq;
        // cell and weight of every component inside [Omega_0, Omega_{nq-1}] (both ends inside)
        std::vector<std::vector<std::pair<int, double>>> bins(nq);
        for (int i = 0; i < nf; ++i) {
            const double w = c->sum_omega[i];
            if (!(w >= T.omega.front() && w <= T.omega.back())) continue;
            int m = static_cast<int>(std::upper_bound(T.omega.begin(), T.omega.end(), w) - T.omega.begin()) - 1;  // largest m with Omega_m <= w
            m     = std::min(m, nq - 2);
            const double lam = (w - T.omega[m]) / (T.omega[m + 1] - T.omega[m]);
            const double w0 = 1.0 - lam, w1 = lam;
            if (w0 != 0.0) bins[m].emplace_back(i, w0);
            if (w1 != 0.0) bins[m + 1].emplace_back(i, w1);
        }
        desc.push_back(b);
        desc.push_back(nq);
        desc.push_back(static_cast<long long>(rowptr.size()));
        desc.push_back(static_cast<long long>(pq_n));
        desc.push_back(T.has_q ? static_cast<long long>(pq_n + n6) : -1LL);
        for (int m = 0; m < nq; ++m) {
            rowptr.push_back(static_cast<int>(idx.size()));
            for (const auto& e : bins[m]) {
                idx.push_back(e.first);
                wgt.push_back(e.second);
            }
        }
        rowptr.push_back(static_cast<int>(idx.size()));
        pq_n += n6 * (T.has_q ? 2 : 1);
        if (c->sum_dirty) {  // otherwise the device copy is in place
            pq.insert(pq.end(), T.P.begin(), T.P.end());
            if (T.has_q) pq.insert(pq.end(), T.Q.begin(), T.Q.end());
        }
        slot_body.push_back(b - c->b0);
    }
    if (idx.empty()) {  // keep the pointers valid where no component falls inside a grid
        idx.push_back(0);
        wgt.push_back(0.0);
    }
    c->d_sum_desc.upload(desc, st);
    c->d_sum_rowptr.upload(rowptr, st);
    c->d_sum_idx.upload(idx, st);
    c->d_sum_w.upload(wgt, st);
    if (c->sum_dirty) c->d_sum_pq.upload(pq, st);
    c->sum_slot_body = slot_body;
    c->sum_dirty     = false;
}

void sum_enqueue(hc_ctx* c, double t, const double* pos) {
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    sum_layout(c);
    const size_t nout = 6 * c->sum_slot_body.size();
    if (c->h_sum_pos.n < n3) c->h_sum_pos.alloc(n3);
    if (c->d_sum_pos.n < n3) c->d_sum_pos.alloc(n3);
    if (c->h_sum_out.n < nout) c->h_sum_out.alloc(nout);
    if (c->d_sum_out.n < nout) c->d_sum_out.alloc(nout);
    std::copy(pos, pos + n3, c->h_sum_pos.p);
    const bool synthesised = (c->wave_kind == kWaveIrregular && !c->eta_record) || c->wave_kind == kWaveSpectral;
    const double rd        = c->irr.ramp_duration;
    const double ramp      = (synthesised && rd > 0.0 && t < rd) ? (t <= 0.0 ? 0.0 : t / rd) : 1.0;  // the rule of the drift term
    SumArgs a{};
    a.tab     = c->d_sum_tab.p;
    a.nf      = c->sum_nf;
    a.desc    = c->d_sum_desc.p;
    a.rowptr  = c->d_sum_rowptr.p;
    a.ent_idx = c->d_sum_idx.p;
    a.ent_w   = c->d_sum_w.p;
    a.pq      = c->d_sum_pq.p;
    a.pos     = c->d_sum_pos.p;
    a.t       = t;
    a.ramp2   = ramp * ramp;  // second order in the amplitude
    a.out     = c->d_sum_out.p;
    hipStream_t st = c->stream_sum;
    HC_HIP(hipMemcpyAsync(c->d_sum_pos.p, c->h_sum_pos.p, n3 * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sum_qtf_kernel, dim3(static_cast<unsigned>(nout)), dim3(kSumThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(c->h_sum_out.p, c->d_sum_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, st));
}

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_sum_qtf(hc_ctx* c, int body, int nq, const double* omega, const double* P, const double* Q) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(nq == 0 || (nq >= 2 && nq <= hc::kDriftMaxFreq), HC_ERR_INVALID, "sum-frequency count must be 0 or 2 .. 256");
    require(nq == 0 || (omega && P), HC_ERR_INVALID, "null frequency grid or QTF table");
    require(!c->sum_pending, HC_ERR_INVALID, "a sum-frequency evaluation is in flight (hc_sum_qtf_end has not been called)");
    const size_t n6 = 6 * static_cast<size_t>(nq) * nq;
    if (nq) {
        require(hc::all_finite(omega, nq) && hc::all_finite(P, n6) && (!Q || hc::all_finite(Q, n6)), HC_ERR_INVALID,
                "non-finite value in a sum-frequency table");
        for (int m = 1; m < nq; ++m) require(omega[m] > omega[m - 1], HC_ERR_INVALID, "the sum-frequency grid is not strictly increasing");
    }
    if (!c->stream_sum) HC_HIP(hipStreamCreateWithFlags(&c->stream_sum, hipStreamNonBlocking));
    if (c->sum_tabs.empty()) c->sum_tabs.resize(c->N);
    hc::DriftTable& T = c->sum_tabs[body];
    T.nq              = nq;
    T.has_q           = nq != 0 && Q != nullptr;
    T.omega.assign(omega, omega + nq);
    T.P.assign(P, P + n6);
    T.Q.assign(Q, Q + (T.has_q ? n6 : 0));
    c->sum_dirty = true;
    HC_API_END(c)
}

int hc_get_sum_qtf_size(hc_ctx* c, int body, int* nq) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && nq, HC_ERR_INVALID, "body index out of range or null pointer");
    *nq = c->sum_tabs.empty() ? 0 : c->sum_tabs[body].nq;
    HC_API_END(c)
}

int hc_set_sum_mode(hc_ctx* c, int mode) {
    HC_API_BEGIN_HOT(c)
    require(mode == 0 || mode == 1, HC_ERR_INVALID, "sum-frequency mode must be 0 or 1");
    require(!c->sum_pending, HC_ERR_INVALID, "a sum-frequency evaluation is in flight (hc_sum_qtf_end has not been called)");
    c->sum_mode = mode;
    HC_API_END(c)
}

int hc_get_sum_mode(hc_ctx* c, int* mode) {
    HC_API_BEGIN_HOT(c)
    require(mode != nullptr, HC_ERR_INVALID, "null pointer");
    *mode = c->sum_mode;
    HC_API_END(c)
}

int hc_set_sum_options(hc_ctx* c, const hc_wave_kinematics_opts* o) {
    HC_API_BEGIN_HOT(c)
    hc_wave_kinematics_opts v;
    hc_wave_kinematics_opts_default(&v);
    if (o) v = *o;
    require(std::isfinite(v.regular_phase), HC_ERR_INVALID, "non-finite regular_phase");
    require(!c->sum_pending, HC_ERR_INVALID, "a sum-frequency evaluation is in flight (hc_sum_qtf_end has not been called)");
    c->sum_phase_opt = v.regular_phase;
    HC_API_END(c)
}

int hc_sum_qtf_begin(hc_ctx* c, double t, const double* pos) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    require(!c->sum_pending, HC_ERR_INVALID, "hc_sum_qtf_begin twice without hc_sum_qtf_end");
    require(pos != nullptr, HC_ERR_INVALID, "null state");
    require(std::isfinite(t) && hc::all_finite(pos, 3 * static_cast<size_t>(c->N)), HC_ERR_INVALID, "non-finite time or position");
    require(c->sum_mode == 0 || c->wave_dir.empty(), HC_ERR_UNSUPPORTED,
            "the QTF tables hold one heading: sum-frequency forces are not available while wave directions are set (hc_set_wave_directions)");
    bool any = false;
    if (!c->sum_tabs.empty())
        for (int b = c->b0; b < c->b1; ++b) any = any || c->sum_tabs[b].nq != 0;
    // components: none for NoWave and for an imported eta record (kin_table_host)
    const bool waves = c->wave_kind == hc::kWaveRegular || c->wave_kind == hc::kWaveSpectral || (c->wave_kind == hc::kWaveIrregular && !c->eta_record);
    if (!any || c->sum_mode == 0 || !waves) {
        c->sum_pending = 1;
        return HC_OK;
    }
    try {
        hc::sum_enqueue(c, t, pos);
    } catch (...) {
        (void)hipStreamSynchronize(c->stream_sum);  // nothing stays pending
        throw;
    }
    c->sum_pending = 2;
    HC_API_END(c)
}

int hc_sum_qtf_end(hc_ctx* c, double* out) {
    HC_API_BEGIN_HOT(c)
    require(c->sum_pending != 0, HC_ERR_INVALID, "hc_sum_qtf_end without hc_sum_qtf_begin");
    const int what = c->sum_pending;
    c->sum_pending = 0;
    if (what == 2) HC_HIP(hipStreamSynchronize(c->stream_sum));
    require(out != nullptr, HC_ERR_INVALID, "null output");
    std::fill(out, out + c->Dloc, 0.0);  // bodies without a table
    if (what == 2)
        for (size_t s = 0; s < c->sum_slot_body.size(); ++s)
            std::copy(c->h_sum_out.p + 6 * s, c->h_sum_out.p + 6 * s + 6, out + 6 * static_cast<size_t>(c->sum_slot_body[s]));
    HC_API_END(c)
}

int hc_compute_sum_qtf(hc_ctx* c, double t, const double* pos, double* out) {
    const int rc = hc_sum_qtf_begin(c, t, pos);
    return rc != HC_OK ? rc : hc_sum_qtf_end(c, out);
}

}  // extern "C"
