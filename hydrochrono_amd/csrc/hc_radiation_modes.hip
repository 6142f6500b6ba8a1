// hc_radiation_modes.hip -- state-space radiation by modal recursion (include/hydrochrono_amd.h: hc_set_radiation_modes,
// hc_radiation_modes_begin / hc_radiation_modes_end).  Not in the reference.  Off the step path: a lane of its own (hc_side.hpp:
// stream and begin / end protocol), its own buffers and pinned staging; it reads and writes nothing a step uses, so it is not
// ordered against the direct queue (as the Morison term).  DESIGN.md 3.7r has the mathematics, the kernel and its invariants;
// hc_modal_ring.hpp the bookkeeping of the snapshot slots.
#include "hc_internal.hpp"
#include "hc_limits.hpp"

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kRadmThreads = 256;  // work items per workgroup, one workgroup per owned row
constexpr int kRadmWaves   = kRadmThreads / 64;
// |lambda h|^2 below this: phi1 and phi2 from their Taylor series, kRadmSeriesTerms terms behind the leading one (at |x| = 1 the
// first dropped term of phi1 is 1 / 20! = 4e-19, below half an ulp of its leading 1); at or above it the closed forms, whose
// cancellation then costs a few ulp at most
constexpr double kRadmSeriesBelow = 1.0;
constexpr int kRadmSeriesTerms    = 18;

struct RadmArgs {
    const int* off;     // [rows + 1] first mode of an owned row
    const int* col;     // [items] column 0 .. D-1
    const double2* lam; // [items]
    const double2* res; // [items] residue times rho
    const double2* z_src;  // [items] modal state of the source snapshot (unused when first)
    double2* z_dst;        // [items] ... of the new one
    const double* v_src;   // [D] velocities of the source snapshot (unused when first)
    const double* v_dst;   // [D] velocities at the new time
    double h;              // t_new - t_src
    int first;             // z = 0, rad = 0
    double* out;           // [rows]
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// One workgroup per owned row.  Every work item walks the row's modes with stride 256: e^x from one exp and one sincos, phi1 and
// phi2 (series or closed form, chosen per mode: h is the same for all, lambda is not), z from the source slot, the new z to the
// target slot, and Re[res z] added to its own partial in index order.  The row's sum: a shuffle tree inside each wave, the four
// wave sums through LDS, added in wave order -- a fixed shape, so a row's bits depend on the row's modes, the two velocity samples
// and h, not on where the row sits, on other rows or on N.
__global__ void __launch_bounds__(kRadmThreads) radiation_modes_kernel(RadmArgs a) {
    __shared__ double s_wave[kRadmWaves];
    const int row = blockIdx.x;  // the grid is the owned rows
    const int i0 = a.off[row], i1 = a.off[row + 1];
    double acc = 0.0;
    if (!a.first) {
        for (int i = i0 + threadIdx.x; i < i1; i += kRadmThreads) {
            const double2 lam = a.lam[i], res = a.res[i];
            const int c       = a.col[i];
            const double2 x   = make_double2(lam.x * a.h, lam.y * a.h);
            double sn, cs;
            sincos(x.y, &sn, &cs);
            const double er = exp(x.x);  // Re x -> -inf: 0, and phi1 -> -1 / x below
            const double2 e = make_double2(er * cs, er * sn);
            double2 p1, p2;
            const double ax2 = x.x * x.x + x.y * x.y;
            if (ax2 < kRadmSeriesBelow) {
                // Horner, highest term first: phi1 = sum x^k / (k + 1)!, phi2 = sum x^k / (k + 2)!
                p1 = make_double2(0.0, 0.0);
                p2 = make_double2(0.0, 0.0);
#pragma unroll
                for (int k = kRadmSeriesTerms; k >= 1; --k) {
                    // p <- (1 + p) x / (k + 1), applied from the top: p1 ends as phi1 - 1 (the reciprocals are compile-time constants)
                    const double r1 = 1.0 / (k + 1), r2 = 1.0 / (k + 2);
                    const double2 q1 = make_double2((1.0 + p1.x) * r1, p1.y * r1);
                    const double2 q2 = make_double2((1.0 + p2.x) * r2, p2.y * r2);
                    p1 = cmul(q1, x);
                    p2 = cmul(q2, x);
                }
                p1.x += 1.0;                      // phi1 = 1 + x/2 (1 + x/3 (1 + ...))
                p2 = make_double2(0.5 * (1.0 + p2.x), 0.5 * p2.y);  // phi2 = 1/2 (1 + x/3 (1 + x/4 (1 + ...)))
            } else {
                const double inv = 1.0 / ax2;
                const double2 xi = make_double2(x.x * inv, -x.y * inv);  // 1 / x
                p1 = cmul(make_double2(e.x - 1.0, e.y), xi);
                p2 = cmul(make_double2(p1.x - 1.0, p1.y), xi);
            }
            const double vn = a.v_src[c], vm = a.v_dst[c];
            const double2 zs = a.z_src[i];
            const double2 ez = cmul(e, zs);
            // z_new = e^x z + h [(phi1 - phi2) v_n + phi2 v_n+1]
            const double2 zn = make_double2(ez.x + a.h * ((p1.x - p2.x) * vn + p2.x * vm), ez.y + a.h * ((p1.y - p2.y) * vn + p2.y * vm));
            a.z_dst[i] = zn;
            acc += res.x * zn.x - res.y * zn.y;
        }
    } else {
        for (int i = i0 + threadIdx.x; i < i1; i += kRadmThreads) a.z_dst[i] = make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s_wave[0];
#pragma unroll
        for (int w = 1; w < kRadmWaves; ++w) r += s_wave[w];
        a.out[row] = r;  // a row without modes: 0
    }
}

const char* const kRadmInFlight = "a radiation-modes evaluation is in flight (hc_radiation_modes_end has not been called)";

// the device copy of the owned bodies' lists, row-major; within a row by column, within a pair in the order given.  The modal state
// belongs to the lists: the ring is emptied.
void upload_modes(hc_ctx* c) {
    RadiationModesData& d = c->radmodes;
    std::vector<int> col, off(static_cast<size_t>(c->Dloc) + 1, 0);
    std::vector<double> lam, res;
    for (int b = c->b0; b < c->b1; ++b) {
        const std::vector<hc_radiation_mode>& list = d.modes[b];
        for (int r = 0; r < 6; ++r) {
            std::vector<const hc_radiation_mode*> rowm;
            for (const hc_radiation_mode& m : list)
                if (m.row == r) rowm.push_back(&m);
            std::stable_sort(rowm.begin(), rowm.end(), [](const hc_radiation_mode* x, const hc_radiation_mode* y) { return x->col < y->col; });
            for (const hc_radiation_mode* m : rowm) {
                col.push_back(m->col);
                lam.push_back(m->lambda_re);
                lam.push_back(m->lambda_im);
                res.push_back(c->rho * m->rho_re);
                res.push_back(c->rho * m->rho_im);
            }
            off[static_cast<size_t>(6 * (b - c->b0) + r) + 1] = static_cast<int>(col.size());
        }
    }
    hipStream_t st = c->radm.stream;
    d.col.upload(col, st);
    d.lam.upload(lam, st);
    d.res.upload(res, st);
    d.off.upload(off, st);
    d.items = static_cast<int>(col.size());
    d.z.alloc(static_cast<size_t>(2) * d.items * d.ring.depth);
    d.v.alloc(static_cast<size_t>(c->D) * d.ring.depth);
    if (d.out.n < static_cast<size_t>(c->Dloc)) d.out.alloc(c->Dloc);
    if (d.h_out.n < static_cast<size_t>(c->Dloc)) d.h_out.alloc(c->Dloc);
    if (d.h_v.n < static_cast<size_t>(c->D)) d.h_v.alloc(c->D);
    d.ring.reset();
    c->radm.dirty = false;
}

void radm_enqueue(hc_ctx* c, const ModalAdvance& adv, double t, const double* linvel, const double* angvel) {
    RadiationModesData& d = c->radmodes;
    hipStream_t st        = c->radm.stream;
    for (int b = 0; b < c->N; ++b)
        for (int k = 0; k < 3; ++k) {
            d.h_v.p[6 * b + k]     = linvel[3 * b + k];
            d.h_v.p[6 * b + 3 + k] = angvel[3 * b + k];
        }
    const size_t D = static_cast<size_t>(c->D), items2 = static_cast<size_t>(2) * d.items;
    double* v_dst  = d.v.p + D * adv.dst;
    HC_HIP(hipMemcpyAsync(v_dst, d.h_v.p, D * sizeof(double), hipMemcpyHostToDevice, st));
    RadmArgs a{};
    a.off   = d.off.p;
    a.col   = d.col.p;
    a.lam   = reinterpret_cast<const double2*>(d.lam.p);
    a.res   = reinterpret_cast<const double2*>(d.res.p);
    a.z_src = reinterpret_cast<const double2*>(d.z.p + items2 * (adv.first ? adv.dst : adv.src));
    a.z_dst = reinterpret_cast<double2*>(d.z.p + items2 * adv.dst);
    a.v_src = adv.first ? v_dst : d.v.p + D * adv.src;
    a.v_dst = v_dst;
    a.h     = adv.first ? 0.0 : t - adv.t_src;
    a.first = adv.first ? 1 : 0;
    a.out   = d.out.p;
    hipLaunchKernelGGL(radiation_modes_kernel, dim3(c->Dloc), dim3(kRadmThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(d.h_out.p, d.out.p, static_cast<size_t>(c->Dloc) * sizeof(double), hipMemcpyDeviceToHost, st));
}

int owned_items(const hc_ctx* c) {
    int items = 0;
    if (!c->radmodes.modes.empty())
        for (int b = c->b0; b < c->b1; ++b) items += static_cast<int>(c->radmodes.modes[b].size());
    return items;
}

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_radiation_modes(hc_ctx* c, int body, const hc_radiation_mode* modes, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n >= 0 && n <= 6 * c->D * hc::kRadiationModesMaxPerPair, HC_ERR_INVALID, "mode count negative or above the limit per body");
    require(n == 0 || modes, HC_ERR_INVALID, "null mode list");
    require(c->have_sim, HC_ERR_INVALID, "set simulation parameters first (rho scales the residues)");
    c->radm.require_idle(hc::kRadmInFlight);
    std::vector<int> per_pair(static_cast<size_t>(6) * c->D, 0);
    for (int e = 0; e < n; ++e) {
        const hc_radiation_mode& m = modes[e];
        require(m.row >= 0 && m.row < 6 && m.col >= 0 && m.col < c->D, HC_ERR_INVALID, "row or column of a radiation mode out of range");
        require(std::isfinite(m.lambda_re) && std::isfinite(m.lambda_im) && std::isfinite(m.rho_re) && std::isfinite(m.rho_im), HC_ERR_INVALID,
                "non-finite value in a radiation mode");
        require(m.lambda_re < 0.0, HC_ERR_INVALID, "a radiation mode needs Re lambda < 0");
        require(++per_pair[static_cast<size_t>(m.row) * c->D + m.col] <= hc::kRadiationModesMaxPerPair, HC_ERR_INVALID,
                "more than 16 radiation modes on one (row, column) pair");
    }
    c->radm.open();
    if (c->radmodes.modes.empty()) c->radmodes.modes.resize(c->N);
    c->radmodes.modes[body].assign(modes, modes + n);
    c->radm.dirty = true;
    c->radmodes.ring.reset();  // the modal state belonged to the lists before
    HC_API_END(c)
}

int hc_get_radiation_mode_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = c->radmodes.modes.empty() ? 0 : static_cast<int>(c->radmodes.modes[body].size());
    HC_API_END(c)
}

int hc_set_radiation_modes_depth(hc_ctx* c, int depth) {
    HC_API_BEGIN_HOT(c)
    c->radm.require_idle(hc::kRadmInFlight);
    require(depth >= hc::kModalDepthMin && depth <= hc::kModalDepthMax, HC_ERR_INVALID, "depth must be 2 .. 64");
    if (c->radm.stream) HC_HIP(hipStreamSynchronize(c->radm.stream));  // (the slots are re-allocated by the next begin)
    (void)c->radmodes.ring.set_depth(depth);
    c->radm.dirty = true;
    HC_API_END(c)
}

int hc_reset_radiation_modes(hc_ctx* c) {
    HC_API_BEGIN_HOT(c)
    c->radm.require_idle(hc::kRadmInFlight);
    c->radmodes.ring.reset();
    HC_API_END(c)
}

int hc_radiation_modes_begin(hc_ctx* c, double t, const double* linvel, const double* angvel) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    c->radm.require_idle("hc_radiation_modes_begin twice without hc_radiation_modes_end");
    require(linvel && angvel, HC_ERR_INVALID, "null velocity");
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    require(std::isfinite(t) && hc::all_finite(linvel, n3) && hc::all_finite(angvel, n3), HC_ERR_INVALID, "non-finite time or velocity");
    const bool launch = hc::owned_items(c) != 0;
    hc::ModalAdvance adv;
    if (launch) {
        if (c->radm.dirty) hc::upload_modes(c);
        adv = c->radmodes.ring.plan(t);
        require(adv.status != hc::ModalAdvance::kDuplicateTime, HC_ERR_RUNTIME,
                "Tried to compute the radiation force from the modes twice within the same time step!");
        require(adv.status != hc::ModalAdvance::kNoSnapshot, HC_ERR_INVALID,
                "a step back in time past every snapshot the radiation modes keep (hc_set_radiation_modes_depth)");
    }
    try {
        c->radm.begin(launch, [&] { hc::radm_enqueue(c, adv, t, linvel, angvel); });
    } catch (...) {
        c->radmodes.ring.reset();  // the target slot may have been written: nothing of the ring counts any more
        throw;
    }
    if (launch) c->radmodes.ring.commit(adv, t);
    HC_API_END(c)
}

int hc_radiation_modes_end(hc_ctx* c, double* out) {
    HC_API_BEGIN_HOT(c)
    const int what = c->radm.end("hc_radiation_modes_end without hc_radiation_modes_begin");
    require(out != nullptr, HC_ERR_INVALID, "null output");
    if (what == 2) std::copy(c->radmodes.h_out.p, c->radmodes.h_out.p + c->Dloc, out);
    else std::fill(out, out + c->Dloc, 0.0);
    HC_API_END(c)
}

int hc_compute_radiation_modes(hc_ctx* c, double t, const double* linvel, const double* angvel, double* out) {
    const int rc = hc_radiation_modes_begin(c, t, linvel, angvel);
    return rc != HC_OK ? rc : hc_radiation_modes_end(c, out);
}

int hc_get_radiation_modes_irf(hc_ctx* c, int body, int n_tau, const double* tau, double* K) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n_tau >= 0 && (n_tau == 0 || (tau && K)), HC_ERR_INVALID, "null pointer");
    const size_t n = static_cast<size_t>(n_tau);
    std::fill(K, K + 6 * static_cast<size_t>(c->D) * n, 0.0);
    if (c->radmodes.modes.empty()) return HC_OK;
    for (const hc_radiation_mode& m : c->radmodes.modes[body]) {
        double* k = K + (static_cast<size_t>(m.row) * c->D + m.col) * n;
        for (size_t j = 0; j < n; ++j) {
            const double e = std::exp(m.lambda_re * tau[j]);
            k[j] += e * (m.rho_re * std::cos(m.lambda_im * tau[j]) - m.rho_im * std::sin(m.lambda_im * tau[j]));
        }
    }
    HC_API_END(c)
}

}  // extern "C"
