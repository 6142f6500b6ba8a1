// hc_qtf.hip -- second-order wave forces from QTF tables: the drift term from difference-frequency tables (include/hydrochrono_amd.h:
// hc_set_drift_qtf, hc_drift_begin / hc_drift_end) and its counterpart above the wave band from sum-frequency tables (hc_set_sum_qtf,
// hc_sum_qtf_begin / hc_sum_qtf_end).  Not in the reference.  One implementation, two instances (hc_ctx::drift, hc_ctx::sum): the same
// component table, bin map and projections U_m, V_m; the terms differ in the signs of the pair product (cos / sin of theta_i - theta_j
// against theta_i + theta_j), in the drift term's modes 1 and 2, and in the words of their messages.  Off the step path: each term has
// its own lane (hc_side.hpp), table copies and pinned staging; it reads and writes nothing a step or the other term uses, so it is
// not ordered against the direct queue (as hc_morison.hip).  DESIGN.md 3.7e and 3.7i have the definitions, the projected evaluation
// form, the kernels and their invariants.
#include "hc_heading.hpp"
#include "hc_internal.hpp"
#include "hc_qtf.hpp"
#include "hc_wave_kin.hpp"

#include <algorithm>

using namespace hc::detail;

namespace hc {
namespace {

// Phase 1: u_i = A_i cos theta_i, w_i = A_i sin theta_i tile by tile through LDS; lane m < nq adds its bin's entries in component order
// into one accumulator pair (U_m, V_m), whatever the tiling.  Leaves them in sU, sV (zero for the lanes past the grid), visible to all.
__device__ __forceinline__ void qtf_project(const QtfArgs& a, const long long* desc, int nq, double* su, double* sw, double* sU,
                                            double* sV, double& U, double& V) {
    const int tid  = threadIdx.x;
    const double x = a.pos[3 * desc[kDescBody]], t = a.t;
    const int* rp  = a.rowptr + desc[kDescRowPtr];
    int p          = tid < nq ? rp[tid] : 0;
    const int pend = tid < nq ? rp[tid + 1] : 0;
    U = 0.0, V = 0.0;
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
    sU[tid] = U;
    sV[tid] = V;
    __syncthreads();
}

// Phase 2, the full table: the lanes stride over the nq^2 entries of row d (P: that row of the table) in ascending e; a lane's partial
template <QtfKind KIND>
__device__ __forceinline__ double qtf_pairs(const QtfArgs& a, const long long* desc, int d, int nq, const double* P, const double* sU,
                                            const double* sV) {
    const int tid = threadIdx.x;
    const int nq2 = nq * nq;
    double acc    = 0.0;
    if (desc[kDescQ] >= 0) {
        const double* Q = a.pq + desc[kDescQ] + static_cast<size_t>(d) * nq2;
        for (int e = tid; e < nq2; e += kQtfThreads) {
            const int m = e / nq, n = e - m * nq;
            acc += qtf_pair_pq<KIND>(P[e], Q[e], sU[m], sV[m], sU[n], sV[n]);
        }
    } else {
        for (int e = tid; e < nq2; e += kQtfThreads) {
            const int m = e / nq, n = e - m * nq;
            acc += qtf_pair_p<KIND>(P[e], sU[m], sV[m], sU[n], sV[n]);
        }
    }
    return acc;
}

// One workgroup per (slot, row d): qtf_project, then the mode's sum over the bins (modes 1 and 2: the diagonal alone) and the tree,
// whose shape depends on the lane index alone.  A row's bits depend on its body's table, pos[b].x, t, the component table and the
// mode only.
__global__ void __launch_bounds__(kQtfThreads) drift_qtf_kernel(QtfArgs a) {
    __shared__ double su[kKinTile], sw[kKinTile];
    __shared__ double sU[kQtfThreads], sV[kQtfThreads];
    __shared__ double red[4][kQtfThreads];
    const int tid         = threadIdx.x;
    const int slot        = blockIdx.x / 6, d = blockIdx.x - 6 * slot;
    const long long* desc = a.desc + static_cast<size_t>(kDescWords) * slot;
    const int nq          = static_cast<int>(desc[kDescNq]);
    const int nq2         = nq * nq;
    const double* P       = a.pq + desc[kDescP] + static_cast<size_t>(d) * nq2;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;

    if (a.mode == 1) {
        if (tid < nq) p0 = P[tid * nq + tid] * a.em[desc[kDescE] + tid];
    } else {
        double U, V;
        qtf_project(a, desc, nq, su, sw, sU, sV, U, V);
        if (a.mode == 2) {
            if (tid < nq) {
                const double D = P[tid * nq + tid];
                p0 = D * U;
                p1 = U;
                p2 = D * V;
                p3 = V;
            }
        } else {
            p0 = qtf_pairs<kQtfDrift>(a, desc, d, nq, P, sU, sV);
        }
    }
    red[0][tid] = p0;
    red[1][tid] = p1;
    red[2][tid] = p2;
    red[3][tid] = p3;
    qtf_tree<4>(red);
    if (tid == 0) {
        const double F = a.mode == 2 ? red[0][0] * red[1][0] + red[2][0] * red[3][0] : red[0][0];
        a.out[6 * static_cast<size_t>(slot) + d] = F * a.ramp2;
    }
}

// As drift_qtf_kernel in its mode 3, with the signs of the sum frequencies and one reduction column.  A row's bits depend on its
// body's table, pos[b].x, t and the component table only.
__global__ void __launch_bounds__(kQtfThreads) sum_qtf_kernel(QtfArgs a) {
    __shared__ double su[kKinTile], sw[kKinTile];
    __shared__ double sU[kQtfThreads], sV[kQtfThreads];
    __shared__ double red[1][kQtfThreads];
    const int tid         = threadIdx.x;
    const int slot        = blockIdx.x / 6, d = blockIdx.x - 6 * slot;
    const long long* desc = a.desc + static_cast<size_t>(kDescWords) * slot;
    const int nq          = static_cast<int>(desc[kDescNq]);
    const double* P       = a.pq + desc[kDescP] + static_cast<size_t>(d) * (nq * nq);
    double U, V;
    qtf_project(a, desc, nq, su, sw, sU, sV, U, V);
    red[0][tid] = qtf_pairs<kQtfSum>(a, desc, d, nq, P, sU, sV);
    qtf_tree<1>(red);
    if (tid == 0) a.out[6 * static_cast<size_t>(slot) + d] = red[0][0] * a.ramp2;
}

// What tells the two terms apart on the host
struct QtfSpec {
    hc::QtfTerm hc_ctx::*term;
    void (*kernel)(QtfArgs);
    QtfKind kind;
    bool build_em;  // E_m of the drift term's mode 1
    int mode_max;
    const char *msg_count, *msg_in_flight, *msg_table, *msg_grid, *msg_mode, *msg_twice, *msg_directions, *msg_no_begin;
};

const QtfSpec kDrift = {&hc_ctx::drift,
                        drift_qtf_kernel,
                        kQtfDrift,
                        true,
                        3,
                        "drift frequency count must be 0 or 2 .. 256",
                        "a drift evaluation is in flight (hc_drift_end has not been called)",
                        "non-finite value in a drift table",
                        "the drift frequency grid is not strictly increasing",
                        "drift mode must be 0, 1, 2 or 3",
                        "hc_drift_begin twice without hc_drift_end",
                        "the QTF tables hold one heading: wave drift forces are not available while wave directions are set (hc_set_wave_directions)",
                        "hc_drift_end without hc_drift_begin"};
const QtfSpec kSum   = {&hc_ctx::sum,
                        sum_qtf_kernel,
                        kQtfSum,
                        false,
                        1,
                        "sum-frequency count must be 0 or 2 .. 256",
                        "a sum-frequency evaluation is in flight (hc_sum_qtf_end has not been called)",
                        "non-finite value in a sum-frequency table",
                        "the sum-frequency grid is not strictly increasing",
                        "sum-frequency mode must be 0 or 1",
                        "hc_sum_qtf_begin twice without hc_sum_qtf_end",
                        "the QTF tables hold one heading: sum-frequency forces are not available while wave directions are set (hc_set_wave_directions)",
                        "hc_sum_qtf_end without hc_sum_qtf_begin"};

const char* const kOutsideQtfGrid =
    "a wave direction lies outside the heading grid of a body's QTF table (hc_set_drift_qtf_headings, hc_set_sum_qtf_headings: no "
    "extrapolation, no wrap-around)";

// A table on a heading grid as the kernels of hc_qtf_dir.hip read it: [6][J][J] with node p = a nq + m, from [6][nh][nh][nq][nq]
void qtf_append_nodes(std::vector<double>& pq, const std::vector<double>& T, int nh, int nq) {
    const size_t J = static_cast<size_t>(nh) * nq, at = pq.size();
    pq.resize(at + 6 * J * J);
    for (int d = 0; d < 6; ++d)
        for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nh; ++b)
                for (int m = 0; m < nq; ++m) {
                    const double* src = T.data() + (((static_cast<size_t>(d) * nh + a) * nh + b) * nq + m) * nq;
                    std::copy(src, src + nq, pq.begin() + at + (d * J + a * nq + m) * J + static_cast<size_t>(b) * nq);
                }
}

// The device copy of the owned bodies' tables (when a table has changed) and, per owned body with a table, the map from grid bin
// (node, for a table on a heading grid) to (component, weight) and (drift) E_m for the component table and the directions in force
// (when a table, the wave model or the directions have changed).  The slots of the one-heading tables come first, in every list.
void qtf_layout(hc_ctx* c, const QtfSpec& s) {
    QtfTerm& q         = c->*s.term;
    KinTableCopy& kin  = q.lane.kin;
    const double phase = q.lane.opts.regular_phase;
    if (kin.current(c, phase) && !q.lane.dirty) return;
    hipStream_t st = q.lane.stream;
    kin.refresh(c, phase, st, [&](std::vector<double>& tab, std::vector<double>& dir, int nf) {
        q.amp.assign(tab.begin() + static_cast<size_t>(kKinAmp) * nf, tab.begin() + static_cast<size_t>(kKinAmp + 1) * nf);
        q.omega.assign(tab.begin() + static_cast<size_t>(kKinOmega) * nf, tab.begin() + static_cast<size_t>(kKinOmega + 1) * nf);
        // the direction columns behind the table's own (hc_qtf_dir.hip); none set: theta_i = 0, the phase of the one-heading kernels
        q.theta = c->wave_dir;
        if (dir.empty()) {
            dir.assign(static_cast<size_t>(kDirCols) * nf, 0.0);
            std::fill(dir.begin(), dir.begin() + nf, 1.0);
            q.theta.assign(nf, 0.0);
        }
    });
    kin.serial   = ~0ULL;  // the bin map below belongs to the table: a failure leaves nothing that counts as current
    const int nf = kin.nf;
    std::vector<long long> desc;
    std::vector<int> rowptr, idx, slot_body;
    std::vector<double> wgt, em, pq;
    size_t pq_n = 0;  // doubles of the tables before this body's
    int slots_dir = 0, chunks_dir = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int b = c->b0; b < c->b1; ++b) {
            const QtfTable& T = q.tabs[b];
            if (T.nq == 0 || (T.nh != 0) != (pass == 1)) continue;
            const int nq = T.nq, nh = std::max(T.nh, 1), J = nh * nq;
            const size_t n6 = 6 * static_cast<size_t>(J) * J;
            // cell and weight of every component inside [Omega_0, Omega_{nq-1}] (both ends inside); on a heading grid times the
            // weights of the two headings around its direction
            std::vector<std::vector<std::pair<int, double>>> bins(J);
            std::vector<double> E(s.build_em ? J : 0, 0.0);
            const auto deposit = [&](int node, int i, double w, double A) {
                if (w == 0.0) return;
                bins[node].emplace_back(i, w);
                if (s.build_em) E[node] += w * (A * A);
            };
            for (int i = 0; i < nf; ++i) {
                const double w = q.omega[i], A = q.amp[i];
                if (!(w >= T.omega.front() && w <= T.omega.back())) continue;
                int m = static_cast<int>(std::upper_bound(T.omega.begin(), T.omega.end(), w) - T.omega.begin()) - 1;  // largest m with Omega_m <= w
                m     = std::min(m, nq - 2);
                const double lam = (w - T.omega[m]) / (T.omega[m + 1] - T.omega[m]);
                const double w0 = 1.0 - lam, w1 = lam;
                if (pass == 0) {
                    deposit(m, i, w0, A);
                    deposit(m + 1, i, w1, A);
                } else {
                    const HeadBracket hb = heading_bracket(T.beta, q.theta[i], kOutsideQtfGrid);
                    const double h0 = 1.0 - hb.wt, h1 = hb.wt;
                    deposit(hb.j0 * nq + m, i, h0 * w0, A);
                    deposit(hb.j0 * nq + m + 1, i, h0 * w1, A);
                    deposit(hb.j1 * nq + m, i, h1 * w0, A);  // (j1 == j0 at the last heading: h1 is 0)
                    deposit(hb.j1 * nq + m + 1, i, h1 * w1, A);
                }
            }
            desc.push_back(b);
            desc.push_back(J);
            desc.push_back(static_cast<long long>(rowptr.size()));
            desc.push_back(static_cast<long long>(pq_n));
            desc.push_back(T.has_q ? static_cast<long long>(pq_n + n6) : -1LL);
            desc.push_back(static_cast<long long>(em.size()));
            for (int m = 0; m < J; ++m) {
                rowptr.push_back(static_cast<int>(idx.size()));
                for (const auto& e : bins[m]) {
                    idx.push_back(e.first);
                    wgt.push_back(e.second);
                }
            }
            rowptr.push_back(static_cast<int>(idx.size()));
            em.insert(em.end(), E.begin(), E.end());
            pq_n += n6 * (T.has_q ? 2 : 1);
            if (q.lane.dirty) {  // otherwise the device copy is in place
                if (pass == 0) {
                    pq.insert(pq.end(), T.P.begin(), T.P.end());
                    if (T.has_q) pq.insert(pq.end(), T.Q.begin(), T.Q.end());
                } else {
                    qtf_append_nodes(pq, T.P, nh, nq);
                    if (T.has_q) qtf_append_nodes(pq, T.Q, nh, nq);
                }
            }
            slot_body.push_back(b - c->b0);
            if (pass == 1) {
                ++slots_dir;
                chunks_dir = std::max(chunks_dir, (J + kQtfDirRows - 1) / kQtfDirRows);
            }
        }
    if (idx.empty()) {  // keep the pointers valid where no component falls inside a grid
        idx.push_back(0);
        wgt.push_back(0.0);
    }
    q.desc.upload(desc, st);
    q.rowptr.upload(rowptr, st);
    q.idx.upload(idx, st);
    q.w.upload(wgt, st);
    if (s.build_em) q.em.upload(em, st);
    if (q.lane.dirty) q.pq.upload(pq, st);
    q.slot_body  = slot_body;
    q.slots_dir  = slots_dir;
    q.chunks_dir = chunks_dir;
    q.lane.dirty = false;
    kin.serial   = c->wave_serial;
}

void qtf_enqueue(hc_ctx* c, const QtfSpec& s, double t, const double* pos) {
    QtfTerm& q      = c->*s.term;
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    qtf_layout(c, s);
    const size_t nout = 6 * q.slot_body.size(), nout_dir = 6 * static_cast<size_t>(q.slots_dir), nout_one = nout - nout_dir;
    require(nout_dir <= 65535, HC_ERR_INVALID, "too many bodies with a QTF table on a heading grid for one launch");
    if (q.h_pos.n < n3) q.h_pos.alloc(n3);
    if (q.pos.n < n3) q.pos.alloc(n3);
    if (q.h_out.n < nout) q.h_out.alloc(nout);
    if (q.out.n < nout) q.out.alloc(nout);
    if (q.part.n < nout_dir * kQtfDirChunks) q.part.alloc(nout_dir * kQtfDirChunks);
    std::copy(pos, pos + n3, q.h_pos.p);
    const double ramp = kin_ramp(c, t);
    QtfArgs a{};
    a.tab     = q.lane.kin.tab.p;
    a.nf      = q.lane.kin.nf;
    a.mode    = q.mode;
    a.desc    = q.desc.p;
    a.rowptr  = q.rowptr.p;
    a.ent_idx = q.idx.p;
    a.ent_w   = q.w.p;
    a.pq      = q.pq.p;
    a.em      = q.em.p;
    a.pos     = q.pos.p;
    a.t       = t;
    a.ramp2   = ramp * ramp;  // second order in the amplitude
    a.out     = q.out.p;
    hipStream_t st = q.lane.stream;
    HC_HIP(hipMemcpyAsync(q.pos.p, q.h_pos.p, n3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (nout_one) {
        hipLaunchKernelGGL(s.kernel, dim3(static_cast<unsigned>(nout_one)), dim3(kQtfThreads), 0, st, a);
        HC_HIP(hipGetLastError());
    }
    if (nout_dir) {  // the slots behind those of the one-heading tables
        QtfDirArgs g{};
        g.a      = a;
        g.a.desc = a.desc + kDescWords * (nout_one / 6);
        g.a.out  = a.out + nout_one;
        g.part   = q.part.p;
        const bool diagonal = s.kind == kQtfDrift && q.mode != 3;
        qtf_dir_launch(g, s.kind, q.slots_dir, diagonal ? 1 : q.chunks_dir, st);
        HC_HIP(hipGetLastError());
    }
    HC_HIP(hipMemcpyAsync(q.h_out.p, q.out.p, nout * sizeof(double), hipMemcpyDeviceToHost, st));
}

// ---- the entry points of a term (include/hydrochrono_amd.h): the extern "C" functions below forward to these ----

// nh = 0: a one-heading table (hc_set_drift_qtf, hc_set_sum_qtf); nh > 0: P, Q [6][nh][nh][nq][nq] on the heading grid beta
int qtf_set_table(hc_ctx* c, const QtfSpec& s, int body, int nh, const double* beta, int nq, const double* omega, const double* P,
                  const double* Q, bool headings) {
    HC_API_BEGIN_HOT(c)
    QtfTerm& q = c->*s.term;
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(nq == 0 || (nq >= 2 && nq <= kDriftMaxFreq), HC_ERR_INVALID, s.msg_count);
    if (nq == 0 || !headings) nh = 0;
    if (nq && headings) {
        require(nh >= 1 && nh <= kQtfMaxHeadings, HC_ERR_INVALID, "QTF heading count must be 1 .. 16");
        require(nh * nq <= kQtfMaxNodes, HC_ERR_INVALID, "heading count times frequency count of a QTF table must not exceed 1024 nodes");
    }
    require(nq == 0 || (omega && P && (!headings || beta)), HC_ERR_INVALID, "null frequency grid, heading grid or QTF table");
    q.lane.require_idle(s.msg_in_flight);
    const size_t nn = static_cast<size_t>(std::max(nh, 1)) * nq, n6 = 6 * nn * nn;
    if (nq) {
        require(all_finite(omega, nq) && all_finite(P, n6) && (!Q || all_finite(Q, n6)), HC_ERR_INVALID, s.msg_table);
        for (int m = 1; m < nq; ++m) require(omega[m] > omega[m - 1], HC_ERR_INVALID, s.msg_grid);
        require(nh == 0 || all_finite(beta, nh), HC_ERR_INVALID, "non-finite value in a QTF heading grid");
        for (int j = 1; j < nh; ++j) require(beta[j] > beta[j - 1], HC_ERR_INVALID, "the QTF heading grid is not strictly increasing");
    }
    q.lane.open();
    if (q.tabs.empty()) q.tabs.resize(c->N);
    QtfTable& T = q.tabs[body];
    T.nq        = nq;
    T.nh        = nh;
    T.has_q     = nq != 0 && Q != nullptr;
    T.omega.assign(omega, omega + nq);
    T.beta.assign(beta, beta + nh);
    T.P.assign(P, P + n6);
    T.Q.assign(Q, Q + (T.has_q ? n6 : 0));
    q.lane.dirty = true;
    HC_API_END(c)
}

int qtf_get_size(hc_ctx* c, const QtfSpec& s, int body, int* nq, bool headings) {
    HC_API_BEGIN_HOT(c)
    const QtfTerm& q = c->*s.term;
    require(body >= 0 && body < c->N && nq, HC_ERR_INVALID, "body index out of range or null pointer");
    *nq = q.tabs.empty() ? 0 : (headings ? q.tabs[body].nh : q.tabs[body].nq);
    HC_API_END(c)
}

int qtf_set_mode(hc_ctx* c, const QtfSpec& s, int mode) {
    HC_API_BEGIN_HOT(c)
    QtfTerm& q = c->*s.term;
    require(mode >= 0 && mode <= s.mode_max, HC_ERR_INVALID, s.msg_mode);
    q.lane.require_idle(s.msg_in_flight);
    q.mode = mode;
    HC_API_END(c)
}

int qtf_get_mode(hc_ctx* c, const QtfSpec& s, int* mode) {
    HC_API_BEGIN_HOT(c)
    require(mode != nullptr, HC_ERR_INVALID, "null pointer");
    *mode = (c->*s.term).mode;
    HC_API_END(c)
}

int qtf_set_options(hc_ctx* c, const QtfSpec& s, const hc_wave_kinematics_opts* o) {
    HC_API_BEGIN_HOT(c)
    (c->*s.term).lane.set_options(o, false, "non-finite regular_phase", s.msg_in_flight);
    HC_API_END(c)
}

int qtf_begin(hc_ctx* c, const QtfSpec& s, double t, const double* pos) {
    HC_API_BEGIN_HOT(c)
    QtfTerm& q = c->*s.term;
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    q.lane.require_idle(s.msg_twice);
    require(pos != nullptr, HC_ERR_INVALID, "null state");
    require(std::isfinite(t) && all_finite(pos, 3 * static_cast<size_t>(c->N)), HC_ERR_INVALID, "non-finite time or position");
    bool one_heading = false;  // of any body of the system: every shard context answers alike
    for (const QtfTable& T : q.tabs) one_heading = one_heading || (T.nq != 0 && T.nh == 0);
    require(q.mode == 0 || c->wave_dir.empty() || !one_heading, HC_ERR_UNSUPPORTED, s.msg_directions);
    bool any = false;
    if (!q.tabs.empty())
        for (int b = c->b0; b < c->b1; ++b) any = any || q.tabs[b].nq != 0;
    q.lane.begin(any && q.mode != 0 && kin_has_components(c), [&] { qtf_enqueue(c, s, t, pos); });
    HC_API_END(c)
}

int qtf_end(hc_ctx* c, const QtfSpec& s, double* out) {
    HC_API_BEGIN_HOT(c)
    QtfTerm& q = c->*s.term;
    const int what = q.lane.end(s.msg_no_begin);
    require(out != nullptr, HC_ERR_INVALID, "null output");
    std::fill(out, out + c->Dloc, 0.0);  // bodies without a table
    if (what == 2)
        for (size_t i = 0; i < q.slot_body.size(); ++i)
            std::copy(q.h_out.p + 6 * i, q.h_out.p + 6 * i + 6, out + 6 * static_cast<size_t>(q.slot_body[i]));
    HC_API_END(c)
}

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_drift_qtf(hc_ctx* c, int body, int nq, const double* omega, const double* P, const double* Q) {
    return hc::qtf_set_table(c, hc::kDrift, body, 0, nullptr, nq, omega, P, Q, false);
}
int hc_set_drift_qtf_headings(hc_ctx* c, int body, int nh, const double* beta, int nq, const double* omega, const double* P, const double* Q) {
    return hc::qtf_set_table(c, hc::kDrift, body, nh, beta, nq, omega, P, Q, true);
}
int hc_get_drift_qtf_size(hc_ctx* c, int body, int* nq) { return hc::qtf_get_size(c, hc::kDrift, body, nq, false); }
int hc_get_drift_qtf_headings(hc_ctx* c, int body, int* nh) { return hc::qtf_get_size(c, hc::kDrift, body, nh, true); }
int hc_set_drift_mode(hc_ctx* c, int mode) { return hc::qtf_set_mode(c, hc::kDrift, mode); }
int hc_get_drift_mode(hc_ctx* c, int* mode) { return hc::qtf_get_mode(c, hc::kDrift, mode); }
int hc_set_drift_options(hc_ctx* c, const hc_wave_kinematics_opts* o) { return hc::qtf_set_options(c, hc::kDrift, o); }
int hc_drift_begin(hc_ctx* c, double t, const double* pos) { return hc::qtf_begin(c, hc::kDrift, t, pos); }
int hc_drift_end(hc_ctx* c, double* out) { return hc::qtf_end(c, hc::kDrift, out); }
int hc_compute_drift(hc_ctx* c, double t, const double* pos, double* out) {
    const int rc = hc_drift_begin(c, t, pos);
    return rc != HC_OK ? rc : hc_drift_end(c, out);
}

int hc_set_sum_qtf(hc_ctx* c, int body, int nq, const double* omega, const double* P, const double* Q) {
    return hc::qtf_set_table(c, hc::kSum, body, 0, nullptr, nq, omega, P, Q, false);
}
int hc_set_sum_qtf_headings(hc_ctx* c, int body, int nh, const double* beta, int nq, const double* omega, const double* P, const double* Q) {
    return hc::qtf_set_table(c, hc::kSum, body, nh, beta, nq, omega, P, Q, true);
}
int hc_get_sum_qtf_size(hc_ctx* c, int body, int* nq) { return hc::qtf_get_size(c, hc::kSum, body, nq, false); }
int hc_get_sum_qtf_headings(hc_ctx* c, int body, int* nh) { return hc::qtf_get_size(c, hc::kSum, body, nh, true); }
int hc_set_sum_mode(hc_ctx* c, int mode) { return hc::qtf_set_mode(c, hc::kSum, mode); }
int hc_get_sum_mode(hc_ctx* c, int* mode) { return hc::qtf_get_mode(c, hc::kSum, mode); }
int hc_set_sum_options(hc_ctx* c, const hc_wave_kinematics_opts* o) { return hc::qtf_set_options(c, hc::kSum, o); }
int hc_sum_qtf_begin(hc_ctx* c, double t, const double* pos) { return hc::qtf_begin(c, hc::kSum, t, pos); }
int hc_sum_qtf_end(hc_ctx* c, double* out) { return hc::qtf_end(c, hc::kSum, out); }
int hc_compute_sum_qtf(hc_ctx* c, double t, const double* pos, double* out) {
    const int rc = hc_sum_qtf_begin(c, t, pos);
    return rc != HC_OK ? rc : hc_sum_qtf_end(c, out);
}

}  // extern "C"
