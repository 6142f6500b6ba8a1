// hc_morison.hip -- Morison drag and inertia elements on the wave kinematics (include/hydrochrono_amd.h: hc_set_morison_elements,
// hc_morison_begin / hc_morison_end).  Not in the reference.  Off the step path: a lane of its own (hc_side.hpp: stream, component table, begin / end
// protocol), its own buffers and pinned staging; it reads and writes nothing a step uses, so it is not ordered against the direct queue
// (as hc_wave_kinematics).
// DESIGN.md 3.7c has the definition, the kernels and their invariants; 3.7g the elements on the second-order sea
// (hc_set_morison_second_order): the increments of hc_wave_kinematics2 at every element, added before the wet test and the force;
// 3.7o the same in a short-crested sea (hc_set_morison_second_order_directional): the increments of hc_wave_kinematics2_dir.
#include "hc_internal.hpp"
#include "hc_morison_members.hpp"
#include "hc_wave_kin.hpp"
#include "hc_wave_kin2.hpp"
#include "hc_wave_kin2_dir.hpp"
#include "hc_wave_kin2_sum.hpp"

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kMorThreads = 256;  // work items per workgroup, one per element
constexpr int kMorElemDoubles = 9;  // r, cd_area, cm_vol
constexpr int kMorIncDoubles = 8;   // p, eta2, u2x, u2z, a2x, a2z of an element on the second-order sea
constexpr int kMorDirIncDoubles = 10;  // p, eta2, u2[3], a2[3] of an element on the directional second-order sea

struct MorArgs {
    const double* tab;  // [kKinCols][nf] (hc_wave_kin.hpp), with directions [kKinCols + kDirCols][nf]; nf = 0: still water
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
    const double* inc; // [n_items][kMorIncDoubles] of morison2_incr_kernel, with directions [n_items][kMorDirIncDoubles] of
                       // morison2_incr_kernel<true> (the order-2 instantiations only)
};

// R = Rx(rpy0) Ry(rpy1) Rz(rpy2), d = R r, p = pos + d (x and z: the wave travels along x): one expression for the kernel that
// evaluates the elements and the one that sums their second-order increments, so that both see the same point bit for bit
struct MorFrame {
    double r00, r01, r02, r10, r11, r12, r20, r21, r22;
    double d0, d1, d2;
    double x, y, z;
};

__device__ inline MorFrame morison_frame(const double* el, const double* pos, const double* rpy) {
    double sa, ca, sb, cb, sc, cc;
    sincos(rpy[0], &sa, &ca);
    sincos(rpy[1], &sb, &cb);
    sincos(rpy[2], &sc, &cc);
    MorFrame f;
    f.r00 = cb * cc, f.r01 = -cb * sc, f.r02 = sb;
    f.r10 = ca * sc + sa * sb * cc, f.r11 = ca * cc - sa * sb * sc, f.r12 = -sa * cb;
    f.r20 = sa * sc - ca * sb * cc, f.r21 = sa * cc + ca * sb * sc, f.r22 = ca * cb;
    f.d0 = f.r00 * el[0] + f.r01 * el[1] + f.r02 * el[2];
    f.d1 = f.r10 * el[0] + f.r11 * el[1] + f.r12 * el[2];
    f.d2 = f.r20 * el[0] + f.r21 * el[1] + f.r22 * el[2];
    f.x = pos[0] + f.d0, f.y = pos[1] + f.d1, f.z = pos[2] + f.d2;
    return f;
}

// One work item per element.  Every item derives its body's frame from the 12 state values, sums the wave components in index
// order from the same LDS tiles (the loop of wave_kinematics_kernel) and writes its own 6-vector: its bits depend on its body's
// state, its own data, the table, t and the options, not on where in the grid it sits.  Without stretching eta comes out of the
// kinematics pass (the same sincos); with stretching it is summed first.
// ORDER2: the element's second-order increments (morison2_incr_kernel, earlier on the stream) are read after the first-order sums
// and added before the wet test and the force; the first-order part, stretching by eta1 included, is the code of order 1.
// DIR (morison_dir_items_kernel, morison2_dir_items_kernel): the directional sea of wave_kinematics_kernel<true> -- the phase at k (x cos + y sin), the horizontal flow
// along (cos, sin), so that u_f and a_f have a y component; the long-crested instantiations keep their arithmetic.
// ORDER2 and DIR: the ten doubles of morison2_incr_kernel<true>, u2y and a2y among them, enter the same places.
template <bool ORDER2, bool DIR>
__device__ __forceinline__ void morison_items_body(const MorArgs& a) {
    constexpr int kDc = kKinCols, kDs = kKinCols + 1;  // rows of the direction columns (DIR only)
    __shared__ double s[DIR ? kKinCols + kDirCols : kKinCols][kKinTile];
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
    const MorFrame f = morison_frame(el, pos, rpy);
    const double r00 = f.r00, r01 = f.r01, r02 = f.r02, r10 = f.r10, r11 = f.r11, r12 = f.r12, r20 = f.r20, r21 = f.r21, r22 = f.r22;
    const double d0 = f.d0, d1 = f.d1, d2 = f.d2;
    const double x = f.x, y = DIR ? f.y : 0.0, z = f.z, t = a.t;

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
    double zs = z;
    if (a.stretch) {
        const double zr = z - a.mwl;
        zs = a.finite_depth ? a.depth * (zr - eta) / (a.depth + eta) : zr - eta;
    }
    const double ze = zs - a.mwl;  // under stretching mwl is subtracted a second time, as in the reference

    // ---- velocity and acceleration (and eta without stretching) ----
    double ux = 0.0, uy = 0.0, uz = 0.0, ax = 0.0, ay = 0.0, az = 0.0, eta1 = 0.0;
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int m = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += kMorThreads) {
#pragma unroll
            for (int col = 0; col < (DIR ? kKinCols + kDirCols : kKinCols); ++col) s[col][i] = a.tab[col * a.nf + i0 + i];
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
            eta1 += s[kKinAmp][i] * cs;
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
    if (!a.stretch) eta = eta1;
    double u2x = 0.0, u2y = 0.0, u2z = 0.0, a2x = 0.0, a2y = 0.0, a2z = 0.0;
    if constexpr (ORDER2 && DIR) {
        const double* q = a.inc + static_cast<size_t>(kMorDirIncDoubles) * o;
        eta += q[3];
        u2x = q[4], u2y = q[5], u2z = q[6], a2x = q[7], a2y = q[8], a2z = q[9];
    } else if constexpr (ORDER2) {
        const double* q = a.inc + static_cast<size_t>(kMorIncDoubles) * o;
        eta += q[3];
        u2x = q[4], u2z = q[5], a2x = q[6], a2z = q[7];
    }

    double* out = a.item + 6 * static_cast<size_t>(o);
    if (!(z - a.mwl <= eta)) {  // dry
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = 0.0;
        return;
    }
    // ---- relative flow in the body frame, force per body axis, back to the world frame ----
    const double w0 = ang[0], w1 = ang[1], w2 = ang[2];
    double ufx = a.ramp * ux, ufz = a.ramp * uz, afx = a.ramp * ax, afz = a.ramp * az;
    if constexpr (ORDER2) ufx += u2x, ufz += u2z, afx += a2x, afz += a2z;
    const double q0 = ufx - (lin[0] + (w1 * d2 - w2 * d1));
    double q1, a0, a1, a2;
    if constexpr (DIR) {
        double ufy = a.ramp * uy, afy = a.ramp * ay;
        if constexpr (ORDER2) ufy += u2y, afy += a2y;
        q1 = ufy - (lin[1] + (w2 * d0 - w0 * d2));
        a0 = r00 * afx + r10 * afy + r20 * afz;
        a1 = r01 * afx + r11 * afy + r21 * afz;
        a2 = r02 * afx + r12 * afy + r22 * afz;
    } else {
        q1 = -(lin[1] + (w2 * d0 - w0 * d2));
        a0 = r00 * afx + r20 * afz;
        a1 = r01 * afx + r21 * afz;
        a2 = r02 * afx + r22 * afz;
    }
    const double q2 = ufz - (lin[2] + (w0 * d1 - w1 * d0));
    const double u0 = r00 * q0 + r10 * q1 + r20 * q2;
    const double u1 = r01 * q0 + r11 * q1 + r21 * q2;
    const double u2 = r02 * q0 + r12 * q1 + r22 * q2;
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

template <bool ORDER2>
__global__ void __launch_bounds__(kMorThreads) morison_items_kernel(MorArgs a) {
    morison_items_body<ORDER2, false>(a);
}
__global__ void __launch_bounds__(kMorThreads) morison_dir_items_kernel(MorArgs a) { morison_items_body<false, true>(a); }
__global__ void __launch_bounds__(kMorThreads) morison2_dir_items_kernel(MorArgs a) { morison_items_body<true, true>(a); }
// [order 2][directions set]
void (*const kMorItems[2][2])(MorArgs) = {{morison_items_kernel<false>, morison_dir_items_kernel},
                                          {morison_items_kernel<true>, morison2_dir_items_kernel}};

struct Mor2Args {
    Wk2Sea sea;           // the Morison path's own tables (hc_ctx::mor2), mwl of the Morison options
    const double* elem;   // as MorArgs
    const int* body;
    const double* state;
    int N;
    double t;
    int ramped;           // ramp * ramp applies (apply_ramp, a synthesised irregular model, ramp_duration > 0)
    double ramp_duration;
    double* inc;          // [n_items][kMorIncDoubles]
};

// One workgroup per element of the owned bodies: the point of morison_items_kernel (morison_frame), then the pair sum of
// hc_wave_kinematics2 at that point and time with the epilogue of wk2_sum_kernel: the eight doubles it stores are what that call
// returns for the stored point, bit for bit.
// DIR: the short-crested sea -- the point with its y in scalar registers (of the frame only the point stays live across the pair
// sum), the pair sum of hc_wave_kinematics2_dir, and ten doubles, u2y and a2y among them.
template <bool DIR>
__global__ void __launch_bounds__(kWk2Threads) morison2_incr_kernel(Mor2Args a) {
    const int e       = blockIdx.x;  // the grid is n_items
    const int b       = a.body[e];
    const double* pos = a.state + 3 * b;
    const MorFrame f  = morison_frame(a.elem + static_cast<size_t>(kMorElemDoubles) * e, pos, pos + 3 * a.N);
    double x, y, z;
    if constexpr (DIR) x = wave_uniform(f.x), y = wave_uniform(f.y), z = wave_uniform(f.z);
    else x = f.x, y = pos[1] + f.d1, z = f.z;
    double sum[wk2_sums(DIR)];
    wk2_sea_sum<DIR, true, true>(a.sea, x, y, z, a.t, sum);
    if (threadIdx.x == 0) {
        const double ramp2 = wk2_ramp2(a.ramped != 0, a.ramp_duration, a.t);
        double* out = a.inc + static_cast<size_t>(DIR ? kMorDirIncDoubles : kMorIncDoubles) * e;
        out[0] = x;
        out[1] = y;
        out[2] = z;
        out[3] = 0.25 * sum[0] * ramp2;
        if constexpr (DIR) {
#pragma unroll
            for (int k = 1; k < kWk2DirSums; ++k) out[3 + k] = sum[k] * ramp2;
        } else {
            out[4] = sum[1] * ramp2;
            out[5] = sum[2] * ramp2;
            out[6] = sum[3] * ramp2;
            out[7] = sum[4] * ramp2;
        }
    }
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

// the device copy of the owned bodies' lists, body-major
void upload_elements(hc_ctx* c) {
    MorisonData& d = c->morison;
    std::vector<double> elem;
    std::vector<int> body, off(c->nloc + 1, 0);
    for (int b = c->b0; b < c->b1; ++b) {
        for (const hc_morison_element& m : d.elems[b]) {
            elem.insert(elem.end(), m.r, m.r + 3);
            elem.insert(elem.end(), m.cd_area, m.cd_area + 3);
            elem.insert(elem.end(), m.cm_vol, m.cm_vol + 3);
            body.push_back(b);
        }
        off[b - c->b0 + 1] = static_cast<int>(body.size());
    }
    d.elem.upload(elem, c->mor.stream);
    d.body.upload(body, c->mor.stream);
    d.off.upload(off, c->mor.stream);
    c->mor2.off = off;
    d.items     = static_cast<int>(body.size());
    if (d.item.n < 6 * body.size()) d.item.alloc(6 * body.size());
    c->mor.dirty = false;
}

void morison_enqueue(hc_ctx* c, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel) {
    MorisonData& d  = c->morison;
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    hipStream_t st  = c->mor.stream;
    if (c->mor.dirty) upload_elements(c);
    c->mor.kin.refresh(c, c->mor.opts.regular_phase, st);
    if (d.h_state.n < 4 * n3) d.h_state.alloc(4 * n3);
    if (d.state.n < 4 * n3) d.state.alloc(4 * n3);
    if (d.h_out.n < static_cast<size_t>(c->Dloc)) d.h_out.alloc(c->Dloc);
    if (d.out.n < static_cast<size_t>(c->Dloc)) d.out.alloc(c->Dloc);
    std::copy(pos, pos + n3, d.h_state.p);
    std::copy(rpy, rpy + n3, d.h_state.p + n3);
    std::copy(linvel, linvel + n3, d.h_state.p + 2 * n3);
    std::copy(angvel, angvel + n3, d.h_state.p + 3 * n3);
    MorArgs a{};
    a.tab          = c->mor.kin.tab.p;
    a.nf           = c->mor.kin.nf;
    a.n_items      = d.items;
    a.elem         = d.elem.p;
    a.body         = d.body.p;
    a.state        = d.state.p;
    a.N            = c->N;
    a.t            = t;
    a.depth        = c->depth;
    a.mwl          = c->mor.opts.mwl;
    a.rho          = c->rho;
    a.ramp         = kin_ramp(c, t);
    a.stretch      = (kin_synthesised(c) && c->mor.opts.wave_stretching) ? 1 : 0;  // RegularWave has none
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    a.item         = d.item.p;
    // the second-order sea: tables of this path's own (with directions: those of the directional pair sum), then the increments of
    // every element
    const bool dir     = c->mor.kin.dir;
    const bool order2  = c->mor2.prepare(c, c->mor, dir);
    const int width    = dir ? kMorDirIncDoubles : kMorIncDoubles;
    const size_t n_inc = static_cast<size_t>(width) * a.n_items;
    // (with members and no element on any owned body nothing of the elements' increments is staged: their getter stays as it was)
    double* h_inc      = order2 && a.n_items != 0 ? c->mor2.stage(n_inc, width) : nullptr;
    if (h_inc) a.inc = c->mor2.d_inc.p;
    HC_HIP(hipMemcpyAsync(d.state.p, d.h_state.p, 4 * n3 * sizeof(double), hipMemcpyHostToDevice, st));
    // strip members only (hc_morison_members.hip): no element launch, the element part of the result is zero
    const bool members2 = order2 && c->members.order2;  // hc_set_morison_members_second_order: the lane's tables serve them too
    if (a.n_items == 0) {
        members_enqueue(c, t, d.state.p, members2);
        return;
    }
    const dim3 item_grid((a.n_items + kMorThreads - 1) / kMorThreads);
    if (order2) {
        Mor2Args m{};
        m.sea           = c->mor2.sea(c, a.mwl);
        m.elem          = a.elem;
        m.body          = a.body;
        m.state         = a.state;
        m.N             = a.N;
        m.t             = t;
        m.ramped        = c->mor2.ramped(c);
        m.ramp_duration = c->irr.ramp_duration;
        m.inc           = c->mor2.d_inc.p;
        hipLaunchKernelGGL(dir ? morison2_incr_kernel<true> : morison2_incr_kernel<false>, dim3(a.n_items), dim3(kWk2Threads), 0, st, m);
        HC_HIP(hipGetLastError());
        HC_HIP(hipMemcpyAsync(h_inc, c->mor2.d_inc.p, n_inc * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL(kMorItems[order2][dir], item_grid, dim3(kMorThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    hipLaunchKernelGGL(morison_sum_kernel, dim3((c->Dloc + kMorThreads - 1) / kMorThreads), dim3(kMorThreads), 0, st, d.item.p, d.off.p,
                       c->Dloc, d.out.p);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(d.h_out.p, d.out.p, static_cast<size_t>(c->Dloc) * sizeof(double), hipMemcpyDeviceToHost, st));
    if (members_owned(c) != 0) members_enqueue(c, t, d.state.p, members2);  // behind the element launches
}

const char* const kMorInFlight = "a Morison evaluation is in flight (hc_morison_end has not been called)";

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_morison_elements(hc_ctx* c, int body, const hc_morison_element* elems, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n >= 0 && n <= hc::kMorisonMaxElements, HC_ERR_INVALID, "element count negative or above the limit per body");
    require(n == 0 || elems, HC_ERR_INVALID, "null element list");
    c->mor.require_idle(hc::kMorInFlight);
    for (int e = 0; e < n; ++e) {
        const hc_morison_element& m = elems[e];
        require(hc::all_finite(m.r, 3) && hc::all_finite(m.cd_area, 3) && hc::all_finite(m.cm_vol, 3), HC_ERR_INVALID,
                "non-finite value in a Morison element");
        for (int k = 0; k < 3; ++k) require(m.cd_area[k] >= 0.0 && m.cm_vol[k] >= 0.0, HC_ERR_INVALID, "negative Morison coefficient");
    }
    c->mor.open();
    if (c->morison.elems.empty()) c->morison.elems.resize(c->N);
    c->morison.elems[body].assign(elems, elems + n);
    c->mor.dirty = true;
    c->mor2.done.clear();  // hc_get_morison_increments: the lists of the last evaluation are no longer the lists
    HC_API_END(c)
}

int hc_get_morison_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = c->morison.elems.empty() ? 0 : static_cast<int>(c->morison.elems[body].size());
    HC_API_END(c)
}

int hc_set_morison_options(hc_ctx* c, const hc_wave_kinematics_opts* o) {
    HC_API_BEGIN_HOT(c)
    c->mor.set_options(o, true, "non-finite mwl or regular_phase", hc::kMorInFlight);
    HC_API_END(c)
}

int hc_set_morison_second_order(hc_ctx* c, int on, double diff_lo, double diff_hi, double sum_lo, double sum_hi, int apply_ramp) {
    HC_API_BEGIN_HOT(c)
    c->mor2.set(c->mor, hc::kMorInFlight, on, diff_lo, diff_hi, sum_lo, sum_hi, apply_ramp);
    HC_API_END(c)
}

int hc_set_morison_second_order_directional(hc_ctx* c, int on) {
    HC_API_BEGIN_HOT(c)
    c->mor.require_idle(hc::kMorInFlight);
    c->mor2.dir_on = on != 0;
    HC_API_END(c)
}

int hc_get_morison_second_order_directional(hc_ctx* c, int* on) {
    HC_API_BEGIN_HOT(c)
    if (on) *on = c->mor2.dir_on ? 1 : 0;
    HC_API_END(c)
}

int hc_get_morison_second_order(hc_ctx* c, int* on, double* diff_lo, double* diff_hi, double* sum_lo, double* sum_hi, int* apply_ramp) {
    HC_API_BEGIN_HOT(c)
    c->mor2.get(on, diff_lo, diff_hi, sum_lo, sum_hi, apply_ramp);
    HC_API_END(c)
}

int hc_get_morison_increments(hc_ctx* c, int body, double* p, double* eta2, double* vel2, double* acc2) {
    HC_API_BEGIN_HOT(c)
    require(c->mor2.on, HC_ERR_INVALID, "Morison elements on the second-order sea are switched off (hc_set_morison_second_order)");
    require(body >= c->b0 && body < c->b1, HC_ERR_INVALID, "body not owned by this context");
    require(!c->mor2.done.empty(), HC_ERR_INVALID, "no Morison evaluation with a second-order part has completed");
    const double* q = c->mor2.last();
    const int width = c->mor2.last_width();  // of the evaluation that completed: long-crested or directional
    const int e0 = c->mor2.done[body - c->b0], e1 = c->mor2.done[body - c->b0 + 1];
    for (int e = e0; e < e1; ++e) {
        const double* v = q + static_cast<size_t>(width) * e;
        const size_t i  = static_cast<size_t>(e - e0);
        if (p) std::copy(v, v + 3, p + 3 * i);
        if (eta2) eta2[i] = v[3];
        if (width == hc::kMorDirIncDoubles) {
            if (vel2) std::copy(v + 4, v + 7, vel2 + 3 * i);
            if (acc2) std::copy(v + 7, v + 10, acc2 + 3 * i);
        } else {
            if (vel2) vel2[3 * i] = v[4], vel2[3 * i + 1] = 0.0, vel2[3 * i + 2] = v[5];
            if (acc2) acc2[3 * i] = v[6], acc2[3 * i + 1] = 0.0, acc2[3 * i + 2] = v[7];
        }
    }
    HC_API_END(c)
}

int hc_morison_begin(hc_ctx* c, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    c->mor.require_idle("hc_morison_begin twice without hc_morison_end");
    require(pos && rpy && linvel && angvel, HC_ERR_INVALID, "null state");
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    require(std::isfinite(t) && hc::all_finite(pos, n3) && hc::all_finite(rpy, n3) && hc::all_finite(linvel, n3) && hc::all_finite(angvel, n3),
            HC_ERR_INVALID, "non-finite time or state");
    require(!(c->mor2.on && !c->wave_dir.empty() && !c->mor2.dir_on), HC_ERR_UNSUPPORTED,
            "Morison elements on the second-order sea are not available while wave directions are set (hc_set_wave_directions): switch "
            "the directional second-order sea on (hc_set_morison_second_order_directional), clear the directions or switch the "
            "second-order sea off");
    require(!(c->mor2.on && hc::kin_has_components(c)) || hc::wk2_component_count(c) <= hc::kWk2MaxFreq, HC_ERR_UNSUPPORTED,
            "Morison elements on the second-order sea: more than 4096 wave components");
    const int members = hc::members_owned(c);
    require(!(c->mor2.on && members != 0 && !c->members.order2), HC_ERR_UNSUPPORTED,
            "Morison strip members see the first-order sea only: switch the members on the second-order sea on "
            "(hc_set_morison_members_second_order), switch the second-order sea off (hc_set_morison_second_order) or clear the members "
            "of the owned bodies (hc_set_morison_members)");
    int items = 0;
    if (!c->morison.elems.empty())
        for (int b = c->b0; b < c->b1; ++b) items += static_cast<int>(c->morison.elems[b].size());
    c->mor2.flight    = false;
    c->members.flight = false;
    c->members.mass_flight = false;
    c->members.copies.reset();
    c->mor.begin(items != 0 || members != 0, [&] { hc::morison_enqueue(c, t, pos, rpy, linvel, angvel); });
    HC_API_END(c)
}

int hc_morison_end(hc_ctx* c, double* out) {
    HC_API_BEGIN_HOT(c)
    const bool with_members = c->members.flight;
    c->members.flight       = false;
    const bool with_mass    = c->members.mass_flight;  // the members' added-mass matrices change hands as their forces do
    c->members.mass_flight  = false;
    // the members' increments change hands around the wait, as the elements' do inside the lane's end
    const bool with_member_inc = c->mor.pending != 0 && c->members.copies.retire();
    const int what = c->mor.end("hc_morison_end without hc_morison_begin", &c->mor2);
    if (with_member_inc) c->members.copies.complete();
    if (what == 2 && with_members) c->members.done = true;  // hc_get_morison_member_forces answers with this evaluation
    if (what == 2 && with_mass) c->members.mass_done = true;  // hc_get_morison_added_mass and the per-member getter too
    require(out != nullptr, HC_ERR_INVALID, "null output");
    if (what == 2 && c->morison.items != 0) std::copy(c->morison.h_out.p, c->morison.h_out.p + c->Dloc, out);
    else std::fill(out, out + c->Dloc, 0.0);
    if (what == 2 && with_members) {  // elements + members, one addition per component of a body that carries members
        const hc::MorisonMemberData& m = c->members;
        for (int lb = 0; lb < c->nloc; ++lb)
            if (m.off[lb + 1] != m.off[lb])
                for (int k = 6 * lb; k < 6 * lb + 6; ++k) out[k] = out[k] + m.h_out.p[k];
    }
    HC_API_END(c)
}

int hc_compute_morison(hc_ctx* c, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel, double* out) {
    const int rc = hc_morison_begin(c, t, pos, rpy, linvel, angvel);
    return rc != HC_OK ? rc : hc_morison_end(c, out);
}

}  // extern "C"
