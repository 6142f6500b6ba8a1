// hc_nonlinear.hip -- nonlinear buoyancy and Froude-Krylov forces on body surface panels and on triangles clipped at the free surface
// (include/hydrochrono_amd.h: hc_set_surface_panels, hc_set_surface_triangles, hc_nonlinear_begin / hc_nonlinear_end).  Not in the reference (src/hydro_types.h:33 is a TODO).  Off the
// step path, as hc_morison.hip: a lane of its own (hc_side.hpp), its own buffers and pinned staging; it reads and writes nothing a step
// uses, so it is not ordered against the direct queue.  DESIGN.md 3.7d and 3.7d' have the definitions, the kernels and their invariants;
// 3.7h the surface on the second-order sea (hc_set_nonlinear_second_order): eta2 and q2 = -d phi2 / dt of the pair sum at every surface
// point, added before the wet test and the clipping, and the quadratic term -1/2 rho |grad phi1|^2; 3.7p the same in a
// short-crested sea (hc_set_nonlinear_second_order_directional): eta2 and q2 of the directional pair sum, u1 with its y component.
#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"
#include "hc_wave_kin2.hpp"
#include "hc_wave_kin2_dir.hpp"
#include "hc_wave_kin2_sum.hpp"

#include <array>
#include <cstdint>
#include <map>

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kNlThreads = 256;      // work items per workgroup, one per panel: a chunk of one body's list
constexpr int kNlPanelDoubles = 6;   // c, s
constexpr int kNlOut = 12;           // buoy (F, M), fk (F, M)
constexpr int kNlIncDoubles = 5;     // P, eta2, q2 of a surface point on the second-order sea

// This path's own component table, struct of arrays [kNlCols][nf]: the columns of hc_wave_kin.hpp the pressure needs and
// omega^2 A / k in place of the velocity and acceleration amplitudes.
enum NlCol { kNlAmp = 0, kNlOmega, kNlK, kNlPhase, kNlW2AoK, kNlInvSinh, kNlDeep, kNlCols };

struct NlArgs {
    const double* tab;  // [kNlCols][nf], with directions [kNlCols + kDirCols][nf]; nf = 0: still water
    int nf;
    const double* panel;  // nl_panels_kernel: [items][6] (c, s); nl_tris_kernel: [items][9] (v[3][3]); owned bodies one after the other
    const int* chunk;     // [chunks][3]: body (of the system), first item of its kind, count (1 .. 256); from the launch's first chunk on
    const double* state;  // [6 N] pos | rpy, [3N] each
    int N;
    double t, depth, mwl, rho, g;
    double ramp;       // factor on p_d
    int stretch;       // Wheeler stretching
    int finite_depth;  // 0: water depth +inf
    double* part;      // [chunks][12] per-chunk sums
    // the order-2 kernels only: the increments of nl2_incr_kernel<DIR>, [points][kNlIncDoubles], and the surface point of every panel
    // ([panels]) or triangle vertex ([triangles][3]) in it
    const double* inc;
    const int* pidx;
};

// R = Rx(rpy0) Ry(rpy1) Rz(rpy2) and d = R c: one expression for the kernels that evaluate the items and the one that sums the
// second-order increments of their points, so that all see the same point P = pos + d bit for bit (as morison_frame)
struct NlFrame {
    double r00, r01, r02, r10, r11, r12, r20, r21, r22;
};

__device__ __forceinline__ NlFrame nl_frame(const double* rpy) {
    double sa, ca, sb, cb, sc, cc;
    sincos(rpy[0], &sa, &ca);
    sincos(rpy[1], &sb, &cb);
    sincos(rpy[2], &sc, &cc);
    NlFrame f;
    f.r00 = cb * cc, f.r01 = -cb * sc, f.r02 = sb;
    f.r10 = ca * sc + sa * sb * cc, f.r11 = ca * cc - sa * sb * sc, f.r12 = -sa * cb;
    f.r20 = sa * sc - ca * sb * cc, f.r21 = sa * cc + ca * sb * sc, f.r22 = ca * cb;
    return f;
}

__device__ __forceinline__ void nl_rotate(const NlFrame& f, const double* c, double& d0, double& d1, double& d2) {
    d0 = f.r00 * c[0] + f.r01 * c[1] + f.r02 * c[2];
    d1 = f.r10 * c[0] + f.r11 * c[1] + f.r12 * c[2];
    d2 = f.r20 * c[0] + f.r21 * c[1] + f.r22 * c[2];
}

// One workgroup per chunk of up to 256 panels of ONE body, one work item per panel.  The body's frame is derived once per item
// from the same six state values (workgroup-uniform); every item sums the wave components in index order from the same LDS tiles
// (the loop of wave_kinematics_kernel), so a panel's 12 values depend on its body's state, its own data, the table, t and the
// options only.  Idle items of a partly filled chunk and dry panels contribute exact zeros.  The 12 components are then reduced over
// the 256 lanes by a tree whose shape depends on the lane index alone, and lane 0 stores the chunk's 12-vector.
// ORDER2 (nl2_panels_kernel): the component loop also sums the first-order velocity u1 at the same z_e (a sincos where order 1 has
// a cos), and the centroid's increments eta2, q2 (nl2_incr_kernel, earlier on the stream) are read after the loop: eta2 enters the
// wet test, rho q2 - 1/2 rho ramp^2 |u1|^2 the dynamic pressure.  Everything else is the code of order 1.
// DIR (nl_panels_dir_kernel, nl2_dir_panels_kernel): the directional sea of wave_kinematics_kernel<true> -- cos and sin of every
// component's direction staged behind the other columns, the phase at k (x cos + y sin); the pressure is a scalar, so nothing else
// changes at order 1.  ORDER2 and DIR: the horizontal part of u1 lies along every component's direction, so |u1|^2 gains u1y^2; the
// increments are those of nl2_incr_kernel<true>.
template <bool ORDER2, bool DIR = false>
__device__ __forceinline__ void nl_panels_body(const NlArgs& a) {
    constexpr int kDc = kNlCols, kDs = kNlCols + 1;  // rows of the direction columns (DIR only)
    __shared__ double s[DIR ? kNlCols + kDirCols : kNlCols][kKinTile];
    __shared__ double red[kNlOut][kNlThreads];
    const int tid     = threadIdx.x;
    const int b       = a.chunk[3 * blockIdx.x];
    const int first   = a.chunk[3 * blockIdx.x + 1];
    const int count   = a.chunk[3 * blockIdx.x + 2];
    const bool active = tid < count;
    const int item    = first + (active ? tid : 0);  // idle items read the chunk's first panel
    const double* pn  = a.panel + static_cast<size_t>(kNlPanelDoubles) * item;
    const double* pos = a.state + 3 * b;
    const double* rpy = pos + 3 * a.N;

    // ---- R = Rx(rpy0) Ry(rpy1) Rz(rpy2), d = R c, p = pos + d, n = R s (the expressions of morison_items_kernel) ----
    const NlFrame f = nl_frame(rpy);
    double d0, d1, d2, n0, n1, n2;
    nl_rotate(f, pn, d0, d1, d2);
    nl_rotate(f, pn + 3, n0, n1, n2);
    const double x = pos[0] + d0, y = DIR ? pos[1] + d1 : 0.0, z = pos[2] + d2, t = a.t;

    // ---- eta first under stretching (wave_kinematics_kernel) ----
    double eta = 0.0;
    if (a.stretch) {
        for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
            const int m = min(kKinTile, a.nf - i0);
            __syncthreads();
            for (int i = tid; i < m; i += kNlThreads) {
                s[kNlAmp][i]   = a.tab[kNlAmp * a.nf + i0 + i];
                s[kNlOmega][i] = a.tab[kNlOmega * a.nf + i0 + i];
                s[kNlK][i]     = a.tab[kNlK * a.nf + i0 + i];
                s[kNlPhase][i] = a.tab[kNlPhase * a.nf + i0 + i];
                if constexpr (DIR) {
                    s[kDc][i] = a.tab[kDc * a.nf + i0 + i];
                    s[kDs][i] = a.tab[kDs * a.nf + i0 + i];
                }
            }
            __syncthreads();
            for (int i = 0; i < m; ++i)
                eta += s[kNlAmp][i] *
                       cos(kin_kx<DIR>(s[kNlK][i], x, y, DIR ? s[kDc][i] : 0.0, DIR ? s[kDs][i] : 0.0) - s[kNlOmega][i] * t + s[kNlPhase][i]);
        }
    }
    double zs = z;
    if (a.stretch) {
        const double zr = z - a.mwl;
        zs = a.finite_depth ? a.depth * (zr - eta) / (a.depth + eta) : zr - eta;
    }
    const double ze = zs - a.mwl;  // under stretching mwl is subtracted a second time, as in the reference

    // ---- dynamic pressure sum (and eta without stretching) ----
    double pd = 0.0, eta1 = 0.0, ux = 0.0, uy = 0.0, uz = 0.0;
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int m = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = tid; i < m; i += kNlThreads) {
#pragma unroll
            for (int col = 0; col < (DIR ? kNlCols + kDirCols : kNlCols); ++col) s[col][i] = a.tab[col * a.nf + i0 + i];
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const double k = s[kNlK][i];
            double sn = 0.0, cs;
            if constexpr (ORDER2 && DIR)
                sincos(kin_kx<true>(k, x, y, s[kDc][i], s[kDs][i]) - s[kNlOmega][i] * t + s[kNlPhase][i], &sn, &cs);
            else if constexpr (ORDER2)
                sincos(k * x - s[kNlOmega][i] * t + s[kNlPhase][i], &sn, &cs);
            else
                cs = cos(kin_kx<DIR>(k, x, y, DIR ? s[kDc][i] : 0.0, DIR ? s[kDs][i] : 0.0) - s[kNlOmega][i] * t + s[kNlPhase][i]);
            double px, pz;
            if (s[kNlDeep][i] != 0.0) {  // (the same branch for every item: no divergence)
                px = pz = exp(k * ze);
            } else {
                px = cosh(k * (ze + a.depth)) * s[kNlInvSinh][i];
                pz = ORDER2 ? sinh(k * (ze + a.depth)) * s[kNlInvSinh][i] : 0.0;
            }
            eta1 += s[kNlAmp][i] * cs;
            pd += s[kNlW2AoK][i] * px * cs;
            if constexpr (ORDER2) {  // u1 of the kinematics (omega A is the table's column there), unramped
                const double wa = s[kNlOmega][i] * s[kNlAmp][i];
                if constexpr (DIR) {  // the horizontal flow along (cos, sin) of the component's direction
                    ux += wa * px * cs * s[kDc][i];
                    uy += wa * px * cs * s[kDs][i];
                } else {
                    ux += wa * px * cs;
                }
                uz += wa * pz * sn;
            }
        }
    }
    if (!a.stretch) eta = eta1;
    double q2 = 0.0;
    if constexpr (ORDER2) {
        const double* q = a.inc + static_cast<size_t>(kNlIncDoubles) * a.pidx[item];
        eta += q[3];
        q2 = q[4];
    }

    // ---- pressures, the panel's two 6-vectors at the body reference ----
    const bool wet  = active && (z - a.mwl <= eta);
    const double ps = -(a.rho * a.g) * (z - a.mwl);
    double pw       = a.rho * pd * a.ramp;
    if constexpr (ORDER2 && DIR)
        pw = pw + a.rho * q2 - 0.5 * a.rho * (a.ramp * a.ramp) * (ux * ux + uy * uy + uz * uz);
    else if constexpr (ORDER2)
        pw = pw + a.rho * q2 - 0.5 * a.rho * (a.ramp * a.ramp) * (ux * ux + uz * uz);
    double v[kNlOut];
    v[0]  = -ps * n0;
    v[1]  = -ps * n1;
    v[2]  = -ps * n2;
    v[3]  = d1 * v[2] - d2 * v[1];
    v[4]  = d2 * v[0] - d0 * v[2];
    v[5]  = d0 * v[1] - d1 * v[0];
    v[6]  = -pw * n0;
    v[7]  = -pw * n1;
    v[8]  = -pw * n2;
    v[9]  = d1 * v[8] - d2 * v[7];
    v[10] = d2 * v[6] - d0 * v[8];
    v[11] = d0 * v[7] - d1 * v[6];
#pragma unroll
    for (int k = 0; k < kNlOut; ++k) red[k][tid] = wet ? v[k] : 0.0;

    // ---- fixed-shape tree over the 256 lanes: lane l adds lane l + h for h = 128, 64, ..., 1 ----
    for (int h = kNlThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < kNlOut; ++k) red[k][tid] += red[k][tid + h];
        }
    }
    if (tid == 0) {
        double* out = a.part + static_cast<size_t>(kNlOut) * blockIdx.x;
#pragma unroll
        for (int k = 0; k < kNlOut; ++k) out[k] = red[k][0];
    }
}

__global__ void __launch_bounds__(kNlThreads) nl_panels_kernel(NlArgs a) { nl_panels_body<false>(a); }
__global__ void __launch_bounds__(kNlThreads) nl2_panels_kernel(NlArgs a) { nl_panels_body<true>(a); }
__global__ void __launch_bounds__(kNlThreads) nl_panels_dir_kernel(NlArgs a) { nl_panels_body<false, true>(a); }
__global__ void __launch_bounds__(kNlThreads) nl2_dir_panels_kernel(NlArgs a) { nl_panels_body<true, true>(a); }

// One work item per (owned body, component): the serial sum over the body's chunk partials in chunk order.
__global__ void __launch_bounds__(kNlThreads) nl_sum_kernel(const double* part, const int* off, int rows, double* out) {
    const int row = blockIdx.x * kNlThreads + threadIdx.x;
    if (row >= rows) return;
    const int b = row / kNlOut, k = row - kNlOut * b;
    double acc = 0.0;
    for (int c = off[b]; c < off[b + 1]; ++c) acc += part[static_cast<size_t>(kNlOut) * c + k];
    out[row] = acc;
}

// ---- triangles clipped at the instantaneous free surface (hc_set_surface_triangles; DESIGN.md 3.7d') ----
constexpr int kNlTriDoubles = 9;  // v[3][3]

// a vertex of a triangle or of its wet part: lever from the body reference (world axes) and the two pressures there
struct NlVertex {
    double d0, d1, d2, ps, pd;
};

// the point of edge x -> y where h = 0, h taken as linear along it; x is the wet end: h_x <= 0 < h_y, so the denominator is positive
__device__ __forceinline__ NlVertex nl_cut(const NlVertex& x, const NlVertex& y, double hx, double hy) {
    const double s = hx / (hx - hy);
    return NlVertex{x.d0 + s * (y.d0 - x.d0), x.d1 + s * (y.d1 - x.d1), x.d2 + s * (y.d2 - x.d2), x.ps + s * (y.ps - x.ps), x.pd + s * (y.pd - x.pd)};
}

// one edge midpoint of a sub-triangle: -p_m S / 3 and its moment, for p_s into v[0..6) and for p_d into v[6..12)
__device__ __forceinline__ void nl_midpoint(const NlVertex& a, const NlVertex& b, double t0, double t1, double t2, double (&v)[kNlOut]) {
    const double m0 = 0.5 * (a.d0 + b.d0), m1 = 0.5 * (a.d1 + b.d1), m2 = 0.5 * (a.d2 + b.d2);
    const double ps = 0.5 * (a.ps + b.ps), pd = 0.5 * (a.pd + b.pd);
    const double f0 = -ps * t0, f1 = -ps * t1, f2 = -ps * t2;
    const double w0 = -pd * t0, w1 = -pd * t1, w2 = -pd * t2;
    v[0] += f0;
    v[1] += f1;
    v[2] += f2;
    v[3] += m1 * f2 - m2 * f1;
    v[4] += m2 * f0 - m0 * f2;
    v[5] += m0 * f1 - m1 * f0;
    v[6] += w0;
    v[7] += w1;
    v[8] += w2;
    v[9] += m1 * w2 - m2 * w1;
    v[10] += m2 * w0 - m0 * w2;
    v[11] += m0 * w1 - m1 * w0;
}

// sub-triangle (q0, q1, q2): S = 1/2 (q1 - q0) x (q2 - q0), the three edge midpoints with the mean of the two end pressures -- exact for
// a pressure linear in space, the moment included
__device__ __forceinline__ void nl_sub_triangle(const NlVertex& q0, const NlVertex& q1, const NlVertex& q2, double (&v)[kNlOut]) {
    const double a0 = q1.d0 - q0.d0, a1 = q1.d1 - q0.d1, a2 = q1.d2 - q0.d2;
    const double b0 = q2.d0 - q0.d0, b1 = q2.d1 - q0.d1, b2 = q2.d2 - q0.d2;
    const double t0 = 0.5 * (a1 * b2 - a2 * b1) / 3.0, t1 = 0.5 * (a2 * b0 - a0 * b2) / 3.0, t2 = 0.5 * (a0 * b1 - a1 * b0) / 3.0;
    nl_midpoint(q0, q1, t0, t1, t2, v);
    nl_midpoint(q1, q2, t0, t1, t2, v);
    nl_midpoint(q2, q0, t0, t1, t2, v);
}

// nl_panels_kernel's shape for triangles: one workgroup per chunk of up to 256 triangles of ONE body, one work item per triangle
// (a.panel is the triangle list, [items][9]).  Each item evaluates eta, p_s and p_d at its three vertices -- three independent
// accumulator sets over the same staged components, each vertex in the expressions and the component order of nl_panels_kernel, so a
// vertex's eta is what hc_wave_kinematics returns there -- takes h = z - mwl - eta and the pressures as linear over the triangle, cuts
// the triangle at h = 0 and integrates over the wet part.  Idle items of a partly filled chunk evaluate the chunk's first triangle and
// contribute exact zeros, as dry triangles do.  Then the fixed tree; lane 0 stores the chunk's 12-vector.
// ORDER2 (nl2_tris_kernel): as in the panel kernel -- u1 of every vertex in the component loop, the vertices' increments after it,
// eta2 into h and rho q2 - 1/2 rho ramp^2 |u1|^2 into p_d before the case table, which is the one of order 1.
// DIR (nl_tris_dir_kernel, nl2_dir_tris_kernel): as in the panel kernel -- every vertex's phase at k (x cos + y sin), eta at the
// vertices where the triangle is clipped included; with ORDER2 u1y of every vertex and the increments of nl2_incr_kernel<true>.
template <bool ORDER2, bool DIR = false>
__device__ __forceinline__ void nl_tris_body(const NlArgs& a) {
    constexpr int kDc = kNlCols, kDs = kNlCols + 1;  // rows of the direction columns (DIR only)
    __shared__ double s[DIR ? kNlCols + kDirCols : kNlCols][kKinTile];
    __shared__ double red[kNlOut][kNlThreads];
    const int tid     = threadIdx.x;
    const int b       = a.chunk[3 * blockIdx.x];
    const int first   = a.chunk[3 * blockIdx.x + 1];
    const int count   = a.chunk[3 * blockIdx.x + 2];
    const bool active = tid < count;
    const int item    = first + (active ? tid : 0);
    const double* tv  = a.panel + static_cast<size_t>(kNlTriDoubles) * item;
    const double* pos = a.state + 3 * b;
    const double* rpy = pos + 3 * a.N;

    // ---- R = Rx(rpy0) Ry(rpy1) Rz(rpy2), d_j = R v_j, P_j = pos + d_j (the expressions of nl_panels_kernel) ----
    const NlFrame f = nl_frame(rpy);
    NlVertex q0, q1, q2;
    nl_rotate(f, tv, q0.d0, q0.d1, q0.d2);
    nl_rotate(f, tv + 3, q1.d0, q1.d1, q1.d2);
    nl_rotate(f, tv + 6, q2.d0, q2.d1, q2.d2);
    const double x0 = pos[0] + q0.d0, x1 = pos[0] + q1.d0, x2 = pos[0] + q2.d0;
    const double y0 = DIR ? pos[1] + q0.d1 : 0.0, y1 = DIR ? pos[1] + q1.d1 : 0.0, y2 = DIR ? pos[1] + q2.d1 : 0.0;
    const double z0 = pos[2] + q0.d2, z1 = pos[2] + q1.d2, z2 = pos[2] + q2.d2;
    const double t = a.t;

    // ---- eta first under stretching ----
    double eta0 = 0.0, eta1 = 0.0, eta2 = 0.0;
    if (a.stretch) {
        for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
            const int m = min(kKinTile, a.nf - i0);
            __syncthreads();
            for (int i = tid; i < m; i += kNlThreads) {
                s[kNlAmp][i]   = a.tab[kNlAmp * a.nf + i0 + i];
                s[kNlOmega][i] = a.tab[kNlOmega * a.nf + i0 + i];
                s[kNlK][i]     = a.tab[kNlK * a.nf + i0 + i];
                s[kNlPhase][i] = a.tab[kNlPhase * a.nf + i0 + i];
                if constexpr (DIR) {
                    s[kDc][i] = a.tab[kDc * a.nf + i0 + i];
                    s[kDs][i] = a.tab[kDs * a.nf + i0 + i];
                }
            }
            __syncthreads();
            for (int i = 0; i < m; ++i) {
                const double dc = DIR ? s[kDc][i] : 0.0, ds = DIR ? s[kDs][i] : 0.0;
                eta0 += s[kNlAmp][i] * cos(kin_kx<DIR>(s[kNlK][i], x0, y0, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i]);
                eta1 += s[kNlAmp][i] * cos(kin_kx<DIR>(s[kNlK][i], x1, y1, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i]);
                eta2 += s[kNlAmp][i] * cos(kin_kx<DIR>(s[kNlK][i], x2, y2, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i]);
            }
        }
    }
    double zs0 = z0, zs1 = z1, zs2 = z2;
    if (a.stretch) {
        const double zr0 = z0 - a.mwl, zr1 = z1 - a.mwl, zr2 = z2 - a.mwl;
        zs0 = a.finite_depth ? a.depth * (zr0 - eta0) / (a.depth + eta0) : zr0 - eta0;
        zs1 = a.finite_depth ? a.depth * (zr1 - eta1) / (a.depth + eta1) : zr1 - eta1;
        zs2 = a.finite_depth ? a.depth * (zr2 - eta2) / (a.depth + eta2) : zr2 - eta2;
    }
    const double ze0 = zs0 - a.mwl, ze1 = zs1 - a.mwl, ze2 = zs2 - a.mwl;  // the second mwl subtraction under stretching

    // ---- dynamic pressure sums (and eta without stretching): three independent chains per component ----
    double pd0 = 0.0, pd1 = 0.0, pd2 = 0.0, e0 = 0.0, e1 = 0.0, e2 = 0.0;
    double ux0 = 0.0, ux1 = 0.0, ux2 = 0.0, uz0 = 0.0, uz1 = 0.0, uz2 = 0.0;
    double uy0 = 0.0, uy1 = 0.0, uy2 = 0.0;  // (ORDER2 and DIR only)
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int m = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = tid; i < m; i += kNlThreads) {
#pragma unroll
            for (int col = 0; col < (DIR ? kNlCols + kDirCols : kNlCols); ++col) s[col][i] = a.tab[col * a.nf + i0 + i];
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const double k = s[kNlK][i];
            const double dc = DIR ? s[kDc][i] : 0.0, ds = DIR ? s[kDs][i] : 0.0;
            double sn0 = 0.0, sn1 = 0.0, sn2 = 0.0, cs0, cs1, cs2;
            if constexpr (ORDER2 && DIR) {
                sincos(kin_kx<true>(k, x0, y0, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i], &sn0, &cs0);
                sincos(kin_kx<true>(k, x1, y1, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i], &sn1, &cs1);
                sincos(kin_kx<true>(k, x2, y2, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i], &sn2, &cs2);
            } else if constexpr (ORDER2) {
                sincos(k * x0 - s[kNlOmega][i] * t + s[kNlPhase][i], &sn0, &cs0);
                sincos(k * x1 - s[kNlOmega][i] * t + s[kNlPhase][i], &sn1, &cs1);
                sincos(k * x2 - s[kNlOmega][i] * t + s[kNlPhase][i], &sn2, &cs2);
            } else {
                cs0 = cos(kin_kx<DIR>(k, x0, y0, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i]);
                cs1 = cos(kin_kx<DIR>(k, x1, y1, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i]);
                cs2 = cos(kin_kx<DIR>(k, x2, y2, dc, ds) - s[kNlOmega][i] * t + s[kNlPhase][i]);
            }
            double px0, px1, px2, pz0 = 0.0, pz1 = 0.0, pz2 = 0.0;
            if (s[kNlDeep][i] != 0.0) {  // (the same branch for every item: no divergence)
                px0 = pz0 = exp(k * ze0);
                px1 = pz1 = exp(k * ze1);
                px2 = pz2 = exp(k * ze2);
            } else {
                px0 = cosh(k * (ze0 + a.depth)) * s[kNlInvSinh][i];
                px1 = cosh(k * (ze1 + a.depth)) * s[kNlInvSinh][i];
                px2 = cosh(k * (ze2 + a.depth)) * s[kNlInvSinh][i];
                if constexpr (ORDER2) {
                    pz0 = sinh(k * (ze0 + a.depth)) * s[kNlInvSinh][i];
                    pz1 = sinh(k * (ze1 + a.depth)) * s[kNlInvSinh][i];
                    pz2 = sinh(k * (ze2 + a.depth)) * s[kNlInvSinh][i];
                }
            }
            e0 += s[kNlAmp][i] * cs0;
            e1 += s[kNlAmp][i] * cs1;
            e2 += s[kNlAmp][i] * cs2;
            pd0 += s[kNlW2AoK][i] * px0 * cs0;
            pd1 += s[kNlW2AoK][i] * px1 * cs1;
            pd2 += s[kNlW2AoK][i] * px2 * cs2;
            if constexpr (ORDER2) {  // u1 of the kinematics at every vertex, unramped
                const double wa = s[kNlOmega][i] * s[kNlAmp][i];
                if constexpr (DIR) {  // the horizontal flow along (cos, sin) of the component's direction
                    ux0 += wa * px0 * cs0 * dc;
                    ux1 += wa * px1 * cs1 * dc;
                    ux2 += wa * px2 * cs2 * dc;
                    uy0 += wa * px0 * cs0 * ds;
                    uy1 += wa * px1 * cs1 * ds;
                    uy2 += wa * px2 * cs2 * ds;
                } else {
                    ux0 += wa * px0 * cs0;
                    ux1 += wa * px1 * cs1;
                    ux2 += wa * px2 * cs2;
                }
                uz0 += wa * pz0 * sn0;
                uz1 += wa * pz1 * sn1;
                uz2 += wa * pz2 * sn2;
            }
        }
    }
    if (!a.stretch) {
        eta0 = e0;
        eta1 = e1;
        eta2 = e2;
    }
    double qa = 0.0, qb = 0.0, qc = 0.0;  // q2 of the three vertices
    if constexpr (ORDER2) {
        const int* ix    = a.pidx + 3 * static_cast<size_t>(item);
        const double* ia = a.inc + static_cast<size_t>(kNlIncDoubles) * ix[0];
        const double* ib = a.inc + static_cast<size_t>(kNlIncDoubles) * ix[1];
        const double* ic = a.inc + static_cast<size_t>(kNlIncDoubles) * ix[2];
        eta0 += ia[3], eta1 += ib[3], eta2 += ic[3];
        qa = ia[4], qb = ib[4], qc = ic[4];
    }

    // ---- h and the pressures at the vertices; a vertex is wet iff h <= 0 ----
    const double h0 = z0 - a.mwl - eta0, h1 = z1 - a.mwl - eta1, h2 = z2 - a.mwl - eta2;
    q0.ps = -(a.rho * a.g) * (z0 - a.mwl);
    q1.ps = -(a.rho * a.g) * (z1 - a.mwl);
    q2.ps = -(a.rho * a.g) * (z2 - a.mwl);
    q0.pd = a.rho * pd0 * a.ramp;
    q1.pd = a.rho * pd1 * a.ramp;
    q2.pd = a.rho * pd2 * a.ramp;
    if constexpr (ORDER2 && DIR) {
        const double hr2 = 0.5 * a.rho * (a.ramp * a.ramp);
        q0.pd = q0.pd + a.rho * qa - hr2 * (ux0 * ux0 + uy0 * uy0 + uz0 * uz0);
        q1.pd = q1.pd + a.rho * qb - hr2 * (ux1 * ux1 + uy1 * uy1 + uz1 * uz1);
        q2.pd = q2.pd + a.rho * qc - hr2 * (ux2 * ux2 + uy2 * uy2 + uz2 * uz2);
    } else if constexpr (ORDER2) {
        const double hr2 = 0.5 * a.rho * (a.ramp * a.ramp);
        q0.pd = q0.pd + a.rho * qa - hr2 * (ux0 * ux0 + uz0 * uz0);
        q1.pd = q1.pd + a.rho * qb - hr2 * (ux1 * ux1 + uz1 * uz1);
        q2.pd = q2.pd + a.rho * qc - hr2 * (ux2 * ux2 + uz2 * uz2);
    }
    const bool w0 = h0 <= 0.0, w1 = h1 <= 0.0, w2 = h2 <= 0.0;
    const int nw = active ? static_cast<int>(w0) + static_cast<int>(w1) + static_cast<int>(w2) : 0;

    // ---- the case table: (A, B, C) is the triangle turned so that A is the one wet vertex, or C the one dry vertex ----
    int r = 0;
    if (nw == 1) r = w0 ? 0 : (w1 ? 1 : 2);
    if (nw == 2) r = !w0 ? 1 : (!w1 ? 2 : 0);
    const NlVertex A = r == 0 ? q0 : (r == 1 ? q1 : q2);
    const NlVertex B = r == 0 ? q1 : (r == 1 ? q2 : q0);
    const NlVertex C = r == 0 ? q2 : (r == 1 ? q0 : q1);
    const double hA = r == 0 ? h0 : (r == 1 ? h1 : h2);
    const double hB = r == 0 ? h1 : (r == 1 ? h2 : h0);
    const double hC = r == 0 ? h2 : (r == 1 ? h0 : h1);
    double v[kNlOut];
#pragma unroll
    for (int k = 0; k < kNlOut; ++k) v[k] = 0.0;
    if (nw == 3) {
        nl_sub_triangle(A, B, C, v);
    } else if (nw == 2) {  // (a, b, bc) and (a, bc, ca)
        const NlVertex bc = nl_cut(B, C, hB, hC), ca = nl_cut(A, C, hA, hC);
        nl_sub_triangle(A, B, bc, v);
        nl_sub_triangle(A, bc, ca, v);
    } else if (nw == 1) {  // (a, ab, ac)
        const NlVertex ab = nl_cut(A, B, hA, hB), ac = nl_cut(A, C, hA, hC);
        nl_sub_triangle(A, ab, ac, v);
    }
#pragma unroll
    for (int k = 0; k < kNlOut; ++k) red[k][tid] = v[k];

    // ---- fixed-shape tree over the 256 lanes: lane l adds lane l + h for h = 128, 64, ..., 1 (nl_panels_kernel) ----
    for (int h = kNlThreads / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < kNlOut; ++k) red[k][tid] += red[k][tid + h];
        }
    }
    if (tid == 0) {
        double* out = a.part + static_cast<size_t>(kNlOut) * blockIdx.x;
#pragma unroll
        for (int k = 0; k < kNlOut; ++k) out[k] = red[k][0];
    }
}

__global__ void __launch_bounds__(kNlThreads) nl_tris_kernel(NlArgs a) { nl_tris_body<false>(a); }
__global__ void __launch_bounds__(kNlThreads) nl2_tris_kernel(NlArgs a) { nl_tris_body<true>(a); }
__global__ void __launch_bounds__(kNlThreads) nl_tris_dir_kernel(NlArgs a) { nl_tris_body<false, true>(a); }
__global__ void __launch_bounds__(kNlThreads) nl2_dir_tris_kernel(NlArgs a) { nl_tris_body<true, true>(a); }
// [order 2][directions set][triangles]
void (*const kNlItems[2][2][2])(NlArgs) = {{{nl_panels_kernel, nl_tris_kernel}, {nl_panels_dir_kernel, nl_tris_dir_kernel}},
                                           {{nl2_panels_kernel, nl2_tris_kernel}, {nl2_dir_panels_kernel, nl2_dir_tris_kernel}}};

struct Nl2Args {
    Wk2Sea sea;           // the nonlinear path's own tables (hc_ctx::nl2), mwl of the nonlinear options
    const double* point;  // [points][3]: the distinct body-frame points of the owned bodies' lists, body-major
    const int* body;      // [points] body (of the system) a point belongs to
    const double* state;  // as NlArgs
    int N;
    double t;
    int ramped;           // ramp * ramp applies (apply_ramp, a synthesised irregular model, ramp_duration > 0)
    double ramp_duration;
    double* inc;          // [points][kNlIncDoubles]
};

// One workgroup per distinct surface point of the owned bodies: the point of the item kernels (nl_frame, nl_rotate), then the pair
// sum of hc_wave_kinematics2 -- DIR: of hc_wave_kinematics2_dir, which reads the point's y -- at that point and time with the
// epilogue of wk2_sum_kernel (1/4 on eta2, ramp^2): eta2 is what that call returns for the stored point, bit for bit, and
// q2 = -d phi2 / dt comes from the same pairs, behind the sea's other sums.  No velocity or acceleration is computed.
template <bool DIR>
__global__ void __launch_bounds__(kWk2Threads) nl2_incr_kernel(Nl2Args a) {
    const int e       = blockIdx.x;  // the grid is the number of points
    const double* pos = a.state + 3 * a.body[e];
    const NlFrame f   = nl_frame(pos + 3 * a.N);
    double d0, d1, d2;
    nl_rotate(f, a.point + 3 * static_cast<size_t>(e), d0, d1, d2);
    const double x = pos[0] + d0, y = pos[1] + d1, z = pos[2] + d2;
    double sum[wk2_sums(DIR) + 1];
    wk2_sea_sum<DIR, true, false, true>(a.sea, x, y, z, a.t, sum);
    if (threadIdx.x == 0) {
        const double ramp2 = wk2_ramp2(a.ramped != 0, a.ramp_duration, a.t);
        double* out = a.inc + static_cast<size_t>(kNlIncDoubles) * e;
        out[0] = x;
        out[1] = y;
        out[2] = z;
        out[3] = 0.25 * sum[0] * ramp2;
        out[4] = sum[wk2_sums(DIR)] * ramp2;
    }
}

// the device copy of the owned bodies' lists, body-major, and the chunk map: every body's list (panels or triangles, a body has one kind)
// cut into chunks of 256 in index order.  Both kinds share the map and the partial buffer; consecutive chunks of one kind are a run,
// one launch of that kind's kernel (a system with one kind: one run, one launch)
void upload_panels(hc_ctx* c) {
    std::vector<double> panel, tri;
    std::vector<int> chunk, off(c->nloc + 1, 0);
    c->surface.runs.clear();
    int items = 0, tris = 0;
    for (int b = c->b0; b < c->b1; ++b) {
        const int n  = c->surface.panels.empty() ? 0 : static_cast<int>(c->surface.panels[b].size());
        const int nt = (n || c->surface.tris.empty()) ? 0 : static_cast<int>(c->surface.tris[b].size() / kNlTriDoubles);  // (the setters keep one kind)
        if (n) {
            for (const hc_surface_panel& p : c->surface.panels[b]) {
                panel.insert(panel.end(), p.c, p.c + 3);
                panel.insert(panel.end(), p.s, p.s + 3);
            }
        } else if (nt) {
            tri.insert(tri.end(), c->surface.tris[b].begin(), c->surface.tris[b].end());
        }
        const int kind = n ? 0 : 1, len = n ? n : nt, at = n ? items : tris;
        const int chunk0 = static_cast<int>(chunk.size() / 3);
        for (int e = 0; e < len; e += kNlThreads) {
            chunk.push_back(b);
            chunk.push_back(at + e);
            chunk.push_back(std::min(kNlThreads, len - e));
        }
        const int chunk1 = static_cast<int>(chunk.size() / 3);
        if (chunk1 > chunk0) {
            if (!c->surface.runs.empty() && c->surface.runs[c->surface.runs.size() - 3] == kind)
                c->surface.runs.back() += chunk1 - chunk0;
            else
                c->surface.runs.insert(c->surface.runs.end(), {kind, chunk0, chunk1 - chunk0});
        }
        items += n;
        tris += nt;
        off[b - c->b0 + 1] = chunk1;
    }
    c->surface.panel.upload(panel, c->nl.stream);
    c->surface.tri.upload(tri, c->nl.stream);
    c->surface.chunk.upload(chunk, c->nl.stream);
    c->surface.off.upload(off, c->nl.stream);
    c->surface.items  = items + tris;
    c->surface.chunks = static_cast<int>(chunk.size() / 3);
    if (c->surface.part.n < static_cast<size_t>(kNlOut) * c->surface.chunks) c->surface.part.alloc(static_cast<size_t>(kNlOut) * c->surface.chunks);
    c->nl.dirty          = false;
    c->surface.pts_dirty = true;  // upload_points, once an evaluation on the second-order sea needs them
}

// The distinct body-frame points of one body's list in the order of their first use -- a panel's centroid, a triangle's vertices;
// two points are the same when all three doubles have equal bits -- appended to `pts`, and for every panel, or triangle and vertex,
// the index of its point counted from `base`, appended to `idx`.  Returns the number of points added.
int unique_points(const hc_ctx* c, int b, int base, std::vector<double>* pts, std::vector<int>* idx) {
    std::map<std::array<std::uint64_t, 3>, int> seen;
    const auto add = [&](const double* v) {
        std::array<std::uint64_t, 3> key;
        std::memcpy(key.data(), v, sizeof(key));
        const auto at = seen.emplace(key, static_cast<int>(seen.size()));
        if (at.second && pts) pts->insert(pts->end(), v, v + 3);
        if (idx) idx->push_back(base + at.first->second);
    };
    if (!c->surface.panels.empty() && !c->surface.panels[b].empty()) {
        for (const hc_surface_panel& p : c->surface.panels[b]) add(p.c);
    } else if (!c->surface.tris.empty()) {
        for (size_t e = 0; e + 3 <= c->surface.tris[b].size(); e += 3) add(c->surface.tris[b].data() + e);
    }
    return static_cast<int>(seen.size());
}

// the surface points of the owned bodies, body-major, and the point of every panel and of every triangle vertex: the two index lists
// follow `panel` and `tri` item by item
void upload_points(hc_ctx* c) {
    std::vector<double> pts;
    std::vector<int> body, pidx, tidx, off(c->nloc + 1, 0);
    for (int b = c->b0; b < c->b1; ++b) {
        const bool panels = !c->surface.panels.empty() && !c->surface.panels[b].empty();
        const int n = unique_points(c, b, off[b - c->b0], &pts, panels ? &pidx : &tidx);
        body.insert(body.end(), n, b);
        off[b - c->b0 + 1] = off[b - c->b0] + n;
    }
    c->surface.pt.upload(pts, c->nl.stream);
    c->surface.pbody.upload(body, c->nl.stream);
    c->surface.pidx.upload(pidx, c->nl.stream);
    c->surface.tidx.upload(tidx, c->nl.stream);
    c->nl2.off    = off;
    c->surface.pts_dirty = false;
}

// The path's copy of the component table holds the columns its kernels read (kNlCols of them), one of them divided by k
void nonlinear_shape(std::vector<double>& tab, std::vector<double>&, int nf) {
    const std::vector<double> kin = tab;
    const int from[kNlCols] = {kKinAmp, kKinOmega, kKinK, kKinPhase, kKinW2A, kKinInvSinh, kKinDeep};
    tab.resize(static_cast<size_t>(kNlCols) * nf);
    for (int col = 0; col < kNlCols; ++col)
        for (int i = 0; i < nf; ++i) tab[static_cast<size_t>(col) * nf + i] = kin[static_cast<size_t>(from[col]) * nf + i];
    for (int i = 0; i < nf; ++i) tab[static_cast<size_t>(kNlW2AoK) * nf + i] /= kin[static_cast<size_t>(kKinK) * nf + i];
}

// (the state is in h_state already: hc_nonlinear_begin)
void nonlinear_enqueue(hc_ctx* c, double t) {
    SurfaceData& d = c->surface;
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    const size_t n_out = static_cast<size_t>(kNlOut) * c->nloc;
    hipStream_t st = c->nl.stream;
    if (c->nl.dirty) upload_panels(c);
    c->nl.kin.refresh(c, c->nl.opts.regular_phase, st, nonlinear_shape);
    if (d.state.n < 2 * n3) d.state.alloc(2 * n3);
    if (d.h_out.n < n_out) d.h_out.alloc(n_out);
    if (d.out.n < n_out) d.out.alloc(n_out);
    NlArgs a{};
    a.tab          = c->nl.kin.tab.p;
    a.nf           = c->nl.kin.nf;
    a.panel        = d.panel.p;
    a.chunk        = d.chunk.p;
    a.state        = d.state.p;
    a.N            = c->N;
    a.t            = t;
    a.depth        = c->depth;
    a.mwl          = c->nl.opts.mwl;
    a.rho          = c->rho;
    a.g            = -c->gsys[2];  // gravity is (0, 0, -g): checked by hc_nonlinear_begin
    a.ramp         = kin_ramp(c, t);
    a.stretch      = (kin_synthesised(c) && c->nl.opts.wave_stretching) ? 1 : 0;  // RegularWave has none
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    a.part         = d.part.p;
    const int rows = static_cast<int>(n_out);
    // the second-order sea: tables of this path's own (with directions: those of the directional pair sum), then the increments of
    // every surface point
    const bool dir    = c->nl.kin.dir;
    const bool order2 = c->nl2.prepare(c, c->nl, dir);
    HC_HIP(hipMemcpyAsync(d.state.p, d.h_state.p, 2 * n3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (order2) {
        if (d.pts_dirty) upload_points(c);
        const int points   = c->nl2.off.back();
        const size_t n_inc = static_cast<size_t>(kNlIncDoubles) * points;
        double* h_inc      = c->nl2.stage(n_inc);
        Nl2Args m{};
        m.sea           = c->nl2.sea(c, a.mwl);
        m.point         = d.pt.p;
        m.body          = d.pbody.p;
        m.state         = a.state;
        m.N             = a.N;
        m.t             = t;
        m.ramped        = c->nl2.ramped(c);
        m.ramp_duration = c->irr.ramp_duration;
        m.inc           = c->nl2.d_inc.p;
        hipLaunchKernelGGL(dir ? nl2_incr_kernel<true> : nl2_incr_kernel<false>, dim3(points), dim3(kWk2Threads), 0, st, m);
        HC_HIP(hipGetLastError());
        HC_HIP(hipMemcpyAsync(h_inc, c->nl2.d_inc.p, n_inc * sizeof(double), hipMemcpyDeviceToHost, st));
        a.inc = c->nl2.d_inc.p;
    }
    for (size_t r = 0; r < d.runs.size(); r += 3) {  // a run's chunk map and partials start at its first chunk: blockIdx.x counts from there
        const int kind = d.runs[r], chunk0 = d.runs[r + 1], chunks = d.runs[r + 2];
        NlArgs ar = a;
        ar.panel  = kind ? d.tri.p : d.panel.p;
        ar.chunk  = d.chunk.p + 3 * static_cast<size_t>(chunk0);
        ar.part   = d.part.p + static_cast<size_t>(kNlOut) * chunk0;
        ar.pidx   = kind ? d.tidx.p : d.pidx.p;  // (indexed by the item, as the list)
        hipLaunchKernelGGL(kNlItems[order2][dir][kind != 0], dim3(chunks), dim3(kNlThreads), 0, st, ar);
        HC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(nl_sum_kernel, dim3((rows + kNlThreads - 1) / kNlThreads), dim3(kNlThreads), 0, st, d.part.p, d.off.p, rows, d.out.p);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(d.h_out.p, d.out.p, n_out * sizeof(double), hipMemcpyDeviceToHost, st));
}

// The linear hydrostatic term of the owned bodies for pos, rpy (ComputeForceHydrostatics, src/hydro_forces.cpp:263-322), from the
// context's host copies, in the expression order of the step kernels.
void hs_linear_host(const hc_ctx* c, const double* pos, const double* rpy, double* out) {
    const double gx = c->gsys[0], gy = c->gsys[1], gz = c->gsys[2];
    const double glen = std::sqrt(gx * gx + gy * gy + gz * gz);
    for (int b = c->b0; b < c->b1; ++b) {
        const hc::BodyHost& bd = c->bodies[b];
        double dq[6], r[3];
        for (int j = 0; j < 3; ++j) {
            dq[j]     = pos[3 * b + j] - bd.cg[j];
            dq[3 + j] = rpy[3 * b + j] - 0.0;
            r[j]      = bd.cb[j] - bd.cg[j];
        }
        const double V = bd.disp_vol;
        const double fbx = c->rho * (-gx) * V, fby = c->rho * (-gy) * V, fbz = c->rho * (-gz) * V;
        const double add[6] = {fbx, fby, fbz, r[1] * fbz - r[2] * fby, r[2] * fbx - r[0] * fbz, r[0] * fby - r[1] * fbx};
        for (int i = 0; i < 6; ++i) {
            double s = 0.0;
            for (int j = 0; j < 6; ++j) s += bd.lin[6 * i + j] * dq[j];
            double hs = -(c->rho * glen) * s;
            hs += add[i];
            out[6 * (b - c->b0) + i] = hs;
        }
    }
}

const char* const kNlInFlight = "a nonlinear evaluation is in flight (hc_nonlinear_end has not been called)";

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_surface_panels(hc_ctx* c, int body, const hc_surface_panel* panels, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n >= 0 && n <= hc::kSurfaceMaxPanels, HC_ERR_INVALID, "surface panel count negative or above the limit per body");
    require(n == 0 || panels, HC_ERR_INVALID, "null surface panel list");
    c->nl.require_idle(hc::kNlInFlight);
    for (int e = 0; e < n; ++e)
        require(hc::all_finite(panels[e].c, 3) && hc::all_finite(panels[e].s, 3), HC_ERR_INVALID, "non-finite value in a surface panel");
    c->nl.open();
    if (c->surface.panels.empty()) c->surface.panels.resize(c->N);
    c->surface.panels[body].assign(panels, panels + n);
    if (!c->surface.tris.empty()) c->surface.tris[body].clear();  // a body carries panels or triangles
    c->nl.dirty = true;
    c->nl2.done.clear();  // hc_get_nonlinear_increments: the lists of the last evaluation are no longer the lists
    HC_API_END(c)
}

int hc_get_surface_panel_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = c->surface.panels.empty() ? 0 : static_cast<int>(c->surface.panels[body].size());
    HC_API_END(c)
}

int hc_set_surface_triangles(hc_ctx* c, int body, const double* tri, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n >= 0 && n <= hc::kSurfaceMaxPanels, HC_ERR_INVALID, "surface triangle count negative or above the limit per body");
    require(n == 0 || tri, HC_ERR_INVALID, "null surface triangle list");
    c->nl.require_idle(hc::kNlInFlight);
    const size_t len = static_cast<size_t>(hc::kNlTriDoubles) * static_cast<size_t>(n);
    require(hc::all_finite(tri, len), HC_ERR_INVALID, "non-finite value in a surface triangle");
    c->nl.open();
    if (c->surface.tris.empty()) c->surface.tris.resize(c->N);
    c->surface.tris[body].assign(tri, tri + len);
    if (!c->surface.panels.empty()) c->surface.panels[body].clear();  // a body carries panels or triangles
    c->nl.dirty = true;
    c->nl2.done.clear();
    HC_API_END(c)
}

int hc_get_surface_triangle_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = c->surface.tris.empty() ? 0 : static_cast<int>(c->surface.tris[body].size() / hc::kNlTriDoubles);
    HC_API_END(c)
}

int hc_set_nonlinear_options(hc_ctx* c, const hc_wave_kinematics_opts* o) {
    HC_API_BEGIN_HOT(c)
    c->nl.set_options(o, true, "non-finite mwl or regular_phase", hc::kNlInFlight);
    HC_API_END(c)
}

int hc_set_nonlinear_second_order(hc_ctx* c, int on, double diff_lo, double diff_hi, double sum_lo, double sum_hi, int apply_ramp) {
    HC_API_BEGIN_HOT(c)
    c->nl2.set(c->nl, hc::kNlInFlight, on, diff_lo, diff_hi, sum_lo, sum_hi, apply_ramp);
    if (!c->nl2.on) {  // the points go with the tables and the increments
        c->surface.pt.release();
        c->surface.pbody.release();
        c->surface.pidx.release();
        c->surface.tidx.release();
        c->surface.pts_dirty = true;
    }
    HC_API_END(c)
}

int hc_set_nonlinear_second_order_directional(hc_ctx* c, int on) {
    HC_API_BEGIN_HOT(c)
    c->nl.require_idle(hc::kNlInFlight);
    c->nl2.dir_on = on != 0;
    HC_API_END(c)
}

int hc_get_nonlinear_second_order_directional(hc_ctx* c, int* on) {
    HC_API_BEGIN_HOT(c)
    if (on) *on = c->nl2.dir_on ? 1 : 0;
    HC_API_END(c)
}

int hc_get_nonlinear_second_order(hc_ctx* c, int* on, double* diff_lo, double* diff_hi, double* sum_lo, double* sum_hi, int* apply_ramp) {
    HC_API_BEGIN_HOT(c)
    c->nl2.get(on, diff_lo, diff_hi, sum_lo, sum_hi, apply_ramp);
    HC_API_END(c)
}

int hc_get_nonlinear_point_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = hc::unique_points(c, body, 0, nullptr, nullptr);
    HC_API_END(c)
}

int hc_get_nonlinear_increments(hc_ctx* c, int body, int n, double* p, double* eta2, double* q2) {
    HC_API_BEGIN_HOT(c)
    require(c->nl2.on, HC_ERR_INVALID, "the surface on the second-order sea is switched off (hc_set_nonlinear_second_order)");
    require(body >= c->b0 && body < c->b1, HC_ERR_INVALID, "body not owned by this context");
    require(!c->nl2.done.empty(), HC_ERR_INVALID, "no nonlinear evaluation with a second-order part has completed");
    const int e0 = c->nl2.done[body - c->b0], e1 = c->nl2.done[body - c->b0 + 1];
    require(n == e1 - e0, HC_ERR_INVALID, "n is not the body's surface point count (hc_get_nonlinear_point_count)");
    const double* q = c->nl2.last();
    for (int e = e0; e < e1; ++e) {
        const double* v = q + static_cast<size_t>(hc::kNlIncDoubles) * e;
        const size_t i  = static_cast<size_t>(e - e0);
        if (p) std::copy(v, v + 3, p + 3 * i);
        if (eta2) eta2[i] = v[3];
        if (q2) q2[i] = v[4];
    }
    HC_API_END(c)
}

int hc_nonlinear_begin(hc_ctx* c, double t, const double* pos, const double* rpy) {
    HC_API_BEGIN_HOT(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    c->nl.require_idle("hc_nonlinear_begin twice without hc_nonlinear_end");
    require(pos && rpy, HC_ERR_INVALID, "null state");
    const size_t n3 = 3 * static_cast<size_t>(c->N);
    require(std::isfinite(t) && hc::all_finite(pos, n3) && hc::all_finite(rpy, n3), HC_ERR_INVALID, "non-finite time or state");
    require(c->gsys[0] == 0.0 && c->gsys[1] == 0.0 && c->gsys[2] < 0.0, HC_ERR_INVALID,
            "the nonlinear surface forces need gravity (0, 0, -g): z up");
    require(!(c->nl2.on && !c->wave_dir.empty() && !c->nl2.dir_on), HC_ERR_UNSUPPORTED,
            "the surface on the second-order sea is not available while wave directions are set (hc_set_wave_directions): switch the "
            "directional second-order sea on (hc_set_nonlinear_second_order_directional), clear the directions or switch the "
            "second-order sea off");
    require(!(c->nl2.on && hc::kin_has_components(c)) || hc::wk2_component_count(c) <= hc::kWk2MaxFreq, HC_ERR_UNSUPPORTED,
            "the surface on the second-order sea: more than 4096 wave components");
    // the host copy of the state: the kernel's source, and what hc_nonlinear_end computes hs_lin from (the caller's arrays are
    // borrowed for this call only)
    if (c->surface.h_state.n < 2 * n3) c->surface.h_state.alloc(2 * n3);
    std::copy(pos, pos + n3, c->surface.h_state.p);
    std::copy(rpy, rpy + n3, c->surface.h_state.p + n3);
    int items = 0;
    if (!c->surface.panels.empty())
        for (int b = c->b0; b < c->b1; ++b) items += static_cast<int>(c->surface.panels[b].size());
    if (!c->surface.tris.empty())
        for (int b = c->b0; b < c->b1; ++b) items += static_cast<int>(c->surface.tris[b].size() / hc::kNlTriDoubles);
    c->nl2.flight = false;
    c->nl.begin(items != 0, [&] { hc::nonlinear_enqueue(c, t); });
    HC_API_END(c)
}

int hc_nonlinear_end(hc_ctx* c, double* buoy, double* fk, double* hs_lin) {
    HC_API_BEGIN_HOT(c)
    const int what = c->nl.end("hc_nonlinear_end without hc_nonlinear_begin", &c->nl2);
    for (int bl = 0; bl < c->nloc; ++bl)
        for (int k = 0; k < 6; ++k) {
            if (buoy) buoy[6 * bl + k] = what == 2 ? c->surface.h_out.p[hc::kNlOut * bl + k] : 0.0;
            if (fk) fk[6 * bl + k] = what == 2 ? c->surface.h_out.p[hc::kNlOut * bl + 6 + k] : 0.0;
        }
    if (hs_lin) hc::hs_linear_host(c, c->surface.h_state.p, c->surface.h_state.p + 3 * static_cast<size_t>(c->N), hs_lin);
    HC_API_END(c)
}

int hc_compute_nonlinear(hc_ctx* c, double t, const double* pos, const double* rpy, double* buoy, double* fk, double* hs_lin) {
    const int rc = hc_nonlinear_begin(c, t, pos, rpy);
    return rc != HC_OK ? rc : hc_nonlinear_end(c, buoy, fk, hs_lin);
}

}  // extern "C"
