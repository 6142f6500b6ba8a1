// hc_morison_members.hip -- Morison strip members: slender cylinders given by two end points, integrated along their wet length and
// cut at the instantaneous free surface (include/hydrochrono_amd.h: hc_set_morison_members).  Not in the reference.  On the lane of
// the Morison elements (hc_morison.hip: hc_morison_begin / hc_morison_end; hc_side.hpp), behind their launches: the lane's stream,
// component table and options, buffers and pinned staging of its own.  DESIGN.md 3.7c' has the definition, the kernels and their
// invariants.  The kernels carry their own component loop, built from the pieces of hc_wave_kin.hpp.
// 3.7c'' the members on the second-order sea (hc_set_morison_members_second_order): eta2 of hc_wave_kinematics2 at every node, taken
// off h before the cut, then u2 and a2 at the Gauss points the cut yields, added before the drag product; in a short-crested sea
// the increments of hc_wave_kinematics2_dir.
// 3.7c''' the added-mass matrix on the same wet cut (hc_set_morison_member_added_mass): one more item kernel and the two sum levels
// over 21 entries, behind the force's launches, and only while some owned member has ca > 0.
#include "hc_morison_members.hpp"

#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"
#include "hc_wave_kin2.hpp"
#include "hc_wave_kin2_dir.hpp"
#include "hc_wave_kin2_sum.hpp"

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kMemThreads = 256;    // work items per workgroup
constexpr int kMemDoubles = 11;     // r0, r1 - r0, |r1 - r0|, d0, d1, cd, cm
constexpr int kMemInts = 4;         // body, n_seg, first node, first Gauss point
constexpr double kGaussLo = 0.21132486540518711775;  // 1/2 - 1/(2 sqrt 3)
constexpr double kGaussHi = 0.78867513459481288225;  // 1/2 + 1/(2 sqrt 3)
constexpr double kQuarterPi = 0.78539816339744830962;
constexpr int kMassEntries = 21;     // the upper triangle of a 6 x 6 matrix, row by row

struct MemArgs {
    const double* tab;  // the lane's table: [kKinCols][nf], with directions [kKinCols + kDirCols][nf]; nf = 0: still water
    int nf;
    int n_nodes, n_points;
    const double* mem;        // [members][kMemDoubles], owned bodies one after the other
    const int* desc;          // [members][kMemInts]
    const int* node_member;   // [n_nodes] member a node belongs to
    const int* point_member;  // [n_points] member a Gauss point belongs to
    const double* state;      // [12 N] pos | rpy | linvel | angvel, [3N] each
    int N;
    double t, depth, mwl, rho;
    double ramp;       // factor on u_f and a_f
    int stretch;       // Wheeler stretching
    int finite_depth;  // 0: water depth +inf
    double* h;         // [n_nodes] P_j.z - mwl - eta_j
    double* item;      // [n_points][6] (dF, dM) of every Gauss point
    const double* inc; // [n_points][kMemPointIncDoubles] of morison_member2_points_kernel, with directions
                       // [n_points][kMemPointDirIncDoubles] (the order-2 instantiations only)
};

// R = Rx(rpy0) Ry(rpy1) Rz(rpy2) as the elements form it (hc_morison.hip: morison_frame)
struct MemRot {
    double r00, r01, r02, r10, r11, r12, r20, r21, r22;
};

__device__ __forceinline__ MemRot member_rotation(const double* rpy) {
    double sa, ca, sb, cb, sc, cc;
    sincos(rpy[0], &sa, &ca);
    sincos(rpy[1], &sb, &cb);
    sincos(rpy[2], &sc, &cc);
    MemRot f;
    f.r00 = cb * cc, f.r01 = -cb * sc, f.r02 = sb;
    f.r10 = ca * sc + sa * sb * cc, f.r11 = ca * cc - sa * sb * sc, f.r12 = -sa * cb;
    f.r20 = sa * sc - ca * sb * cc, f.r21 = sa * cc + ca * sb * sc, f.r22 = ca * cb;
    return f;
}

// P_j = pos + R (r0 + (j / n_seg)(r1 - r0)): one expression for the kernel that sums eta1 at the node and the one that sums eta2
// there (morison_member2_nodes_kernel): the same expression in both (compiled with the default contraction, which the order-1
// kernels keep for their bits; the stored point is the one the pair sum was given)
struct MemNode {
    double x, y, z;
};

__device__ __forceinline__ MemNode member_node(const double* mem, const double* pos, const double* rpy, int j, int n_seg) {
    const MemRot f  = member_rotation(rpy);
    const double sj = static_cast<double>(j) / static_cast<double>(n_seg);
    const double rx = mem[0] + sj * mem[3], ry = mem[1] + sj * mem[4], rz = mem[2] + sj * mem[5];
    MemNode p;
    p.x = pos[0] + (f.r00 * rx + f.r01 * ry + f.r02 * rz);
    p.y = pos[1] + (f.r10 * rx + f.r11 * ry + f.r12 * rz);
    p.z = pos[2] + (f.r20 * rx + f.r21 * ry + f.r22 * rz);
    return p;
}

// Gauss point g of segment `seg`: the wet interval [sa, sb] of the segment (local coordinate from node `seg`) from its two h values
// with selects -- the cut's division runs in the cut case only --, the weight, the diameter, R, d = R r_g and p = pos + d.  One
// expression for the kernel that evaluates the force and the one that sums the second-order increments
// (morison_member2_points_kernel), so that the increments are those of the point the force is evaluated at: the same expression
// from the same h in both.
struct MemGauss {
    bool w0, w1;  // node `seg` / node `seg + 1` is wet
    double wg, diam;
    MemRot f;
    double d0, d1, d2;
    double x, y, z;
};

__device__ __forceinline__ MemGauss member_gauss(const double* mem, const double* pos, const double* rpy, double hx, double hy, int seg, int g,
                                                 int n_seg) {
    MemGauss p;
    p.w0 = hx <= 0.0, p.w1 = hy <= 0.0;
    double sa = 0.0, sb = (p.w0 && p.w1) ? 1.0 : 0.0;
    if (p.w0 != p.w1) {  // one cut, measured from the wet end: h_wet <= 0 < h_dry, the denominator is negative
        const double hw = p.w0 ? hx : hy, hd = p.w0 ? hy : hx;
        const double cut = hw / (hw - hd);
        sa = p.w0 ? 0.0 : 1.0 - cut;
        sb = p.w0 ? cut : 1.0;
    }
    const double width = sb - sa;
    const double sg    = sa + width * (g ? kGaussHi : kGaussLo);
    const double along = (static_cast<double>(seg) + sg) / static_cast<double>(n_seg);
    p.wg   = 0.5 * width * mem[6] / static_cast<double>(n_seg);
    p.diam = mem[7] + along * (mem[8] - mem[7]);
    p.f    = member_rotation(rpy);
    const double rx = mem[0] + along * mem[3], ry = mem[1] + along * mem[4], rz = mem[2] + along * mem[5];
    p.d0 = p.f.r00 * rx + p.f.r01 * ry + p.f.r02 * rz;
    p.d1 = p.f.r10 * rx + p.f.r11 * ry + p.f.r12 * rz;
    p.d2 = p.f.r20 * rx + p.f.r21 * ry + p.f.r22 * rz;
    p.x = pos[0] + p.d0, p.y = pos[1] + p.d1, p.z = pos[2] + p.d2;
    return p;
}

// One work item per node of the owned bodies' members, body-major.  The frame comes from the body's state, eta from the loop over
// the LDS-staged component tiles in index order (the cosine only); h_j = P_j.z - mwl - eta_j is stored.  A node's bits depend on
// its body's state, its member, the table, t and mwl, not on where in the grid it sits.
template <bool DIR>
__global__ void __launch_bounds__(kMemThreads) morison_member_nodes_kernel(MemArgs a) {
    constexpr int kRows = DIR ? 6 : 4;  // A, omega, k, phi (and cos theta, sin theta)
    __shared__ double s[kRows][kKinTile];
    const int o       = blockIdx.x * kMemThreads + threadIdx.x;
    const bool active = o < a.n_nodes;
    const int e       = active ? o : 0;  // items past the end evaluate item 0 and store nothing (all take part in the staging)
    const int m       = a.node_member[e];
    const int* ds     = a.desc + kMemInts * m;
    const int b = ds[0], n_seg = ds[1], j = e - ds[2];
    const double* mem = a.mem + static_cast<size_t>(kMemDoubles) * m;
    const double* pos = a.state + 3 * b;
    const MemNode p   = member_node(mem, pos, pos + 3 * a.N, j, n_seg);
    const double x = p.x, y = DIR ? p.y : 0.0, z = p.z;
    double eta = 0.0;
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int n = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kMemThreads) {
            s[0][i] = a.tab[kKinAmp * a.nf + i0 + i];
            s[1][i] = a.tab[kKinOmega * a.nf + i0 + i];
            s[2][i] = a.tab[kKinK * a.nf + i0 + i];
            s[3][i] = a.tab[kKinPhase * a.nf + i0 + i];
            if constexpr (DIR) {
                s[4][i] = a.tab[kKinCols * a.nf + i0 + i];
                s[5][i] = a.tab[(kKinCols + 1) * a.nf + i0 + i];
            }
        }
        __syncthreads();
        for (int i = 0; i < n; ++i)
            eta += s[0][i] * cos(kin_kx<DIR>(s[2][i], x, y, DIR ? s[4][i] : 0.0, DIR ? s[5][i] : 0.0) - s[1][i] * a.t + s[3][i]);
    }
    if (active) a.h[o] = (z - a.mwl) - eta;
}

// One work item per Gauss point (two per segment), body-major.  The wet interval of the segment comes from its two h values with
// selects; the cut's division runs in the cut case only.  Then the kinematics loop of the element kernel at the point (one pass, two
// under stretching), the transverse force per length times the weight, and the moment about the body reference.  A point of a dry
// segment writes exact zeros.
// ORDER2 (morison_member2_items_kernel): the point's second-order increments (morison_member2_points_kernel, earlier on the stream,
// summed at the same point: member_gauss) are read after the first-order loops and added to ramp u1 and ramp a1 before q and a_n;
// the first-order part, stretching by the point's own eta1 included, is the code of order 1, and the two order-1 kernels keep
// their arithmetic and their registers.
template <bool DIR, bool ORDER2>
__device__ __forceinline__ void morison_member_items_body(const MemArgs& a) {
    constexpr int kDc = kKinCols, kDs = kKinCols + 1;  // rows of the direction columns (DIR only)
    __shared__ double s[DIR ? kKinCols + kDirCols : kKinCols][kKinTile];
    const int o       = blockIdx.x * kMemThreads + threadIdx.x;
    const bool active = o < a.n_points;
    const int e       = active ? o : 0;  // items past the end evaluate item 0 and store nothing
    const int m       = a.point_member[e];
    const int* dsc    = a.desc + kMemInts * m;
    const int b = dsc[0], n_seg = dsc[1], local = e - dsc[3];
    const int seg = local >> 1, g = local & 1;
    const double* mem = a.mem + static_cast<size_t>(kMemDoubles) * m;
    const double* pos = a.state + 3 * b;
    const double* rpy = pos + 3 * a.N;
    const double* lin = rpy + 3 * a.N;
    const double* ang = lin + 3 * a.N;

    // ---- the wet interval of the segment, the weight and the diameter; R, d = R r_g, p = pos + d ----
    const MemGauss gp = member_gauss(mem, pos, rpy, a.h[dsc[2] + seg], a.h[dsc[2] + seg + 1], seg, g, n_seg);
    const bool w0 = gp.w0, w1 = gp.w1;
    const double len = mem[6], wg = gp.wg, diam = gp.diam;
    const MemRot f  = gp.f;
    const double d0 = gp.d0, d1 = gp.d1, d2 = gp.d2;
    const double x = gp.x, y = DIR ? gp.y : 0.0, z = gp.z, t = a.t;

    // ---- eta first under stretching ----
    double eta = 0.0;
    if (a.stretch) {
        for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
            const int n = min(kKinTile, a.nf - i0);
            __syncthreads();
            for (int i = threadIdx.x; i < n; i += kMemThreads) {
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
            for (int i = 0; i < n; ++i)
                eta += s[kKinAmp][i] *
                       cos(kin_kx<DIR>(s[kKinK][i], x, y, DIR ? s[kDc][i] : 0.0, DIR ? s[kDs][i] : 0.0) - s[kKinOmega][i] * t + s[kKinPhase][i]);
        }
    }
    double zs = z;
    if (a.stretch) {
        const double zr = z - a.mwl;
        zs = a.finite_depth ? a.depth * (zr - eta) / (a.depth + eta) : zr - eta;
    }
    const double ze = zs - a.mwl;  // under stretching mwl is subtracted a second time, as for the elements

    // ---- velocity and acceleration ----
    double ux = 0.0, uy = 0.0, uz = 0.0, ax = 0.0, ay = 0.0, az = 0.0;
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int n = min(kKinTile, a.nf - i0);
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kMemThreads) {
#pragma unroll
            for (int col = 0; col < (DIR ? kKinCols + kDirCols : kKinCols); ++col) s[col][i] = a.tab[col * a.nf + i0 + i];
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const double k  = s[kKinK][i];
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
    double* out = a.item + 6 * static_cast<size_t>(o);
    if (!(w0 || w1)) {  // a dry segment
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = 0.0;
        return;
    }
    // ---- the flow relative to the point, its part normal to the axis, force and moment in the world frame ----
    const double ex = mem[3] / len, ey = mem[4] / len, ez = mem[5] / len;
    const double t0 = f.r00 * ex + f.r01 * ey + f.r02 * ez;
    const double t1 = f.r10 * ex + f.r11 * ey + f.r12 * ez;
    const double t2 = f.r20 * ex + f.r21 * ey + f.r22 * ez;
    const double w0a = ang[0], w1a = ang[1], w2a_ = ang[2];
    double u2x = 0.0, u2y = 0.0, u2z = 0.0, a2x = 0.0, a2y = 0.0, a2z = 0.0;
    if constexpr (ORDER2 && DIR) {
        const double* v = a.inc + static_cast<size_t>(kMemPointDirIncDoubles) * o;
        u2x = v[4], u2y = v[5], u2z = v[6], a2x = v[7], a2y = v[8], a2z = v[9];
    } else if constexpr (ORDER2) {
        const double* v = a.inc + static_cast<size_t>(kMemPointIncDoubles) * o;
        u2x = v[4], u2z = v[5], a2x = v[6], a2z = v[7];
    }
    const double afx = ORDER2 ? a.ramp * ax + a2x : a.ramp * ax;
    const double afy = ORDER2 ? a.ramp * ay + a2y : a.ramp * ay;
    const double afz = ORDER2 ? a.ramp * az + a2z : a.ramp * az;
    const double vx = lin[0] + (w1a * d2 - w2a_ * d1), vy = lin[1] + (w2a_ * d0 - w0a * d2), vz = lin[2] + (w0a * d1 - w1a * d0);
    const double q0 = ORDER2 ? (a.ramp * ux + u2x) - vx : a.ramp * ux - vx;
    const double q1 = ORDER2 ? (a.ramp * uy + u2y) - vy : a.ramp * uy - vy;
    const double q2 = ORDER2 ? (a.ramp * uz + u2z) - vz : a.ramp * uz - vz;
    const double qa = q0 * t0 + q1 * t1 + q2 * t2;
    const double n0 = q0 - qa * t0, n1 = q1 - qa * t1, n2 = q2 - qa * t2;
    const double aa = afx * t0 + afy * t1 + afz * t2;
    const double a0 = afx - aa * t0, a1 = afy - aa * t1, a2 = afz - aa * t2;
    const double speed = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double c1 = 0.5 * a.rho * mem[9] * diam * speed;
    const double c2 = a.rho * mem[10] * kQuarterPi * diam * diam;
    const double F0 = wg * (c1 * n0 + c2 * a0);
    const double F1 = wg * (c1 * n1 + c2 * a1);
    const double F2 = wg * (c1 * n2 + c2 * a2);
    out[0] = F0;
    out[1] = F1;
    out[2] = F2;
    out[3] = d1 * F2 - d2 * F1;
    out[4] = d2 * F0 - d0 * F2;
    out[5] = d0 * F1 - d1 * F0;
}

template <bool DIR>
__global__ void __launch_bounds__(kMemThreads) morison_member_items_kernel(MemArgs a) {
    morison_member_items_body<DIR, false>(a);
}
template <bool DIR>
__global__ void __launch_bounds__(kMemThreads) morison_member2_items_kernel(MemArgs a) {
    morison_member_items_body<DIR, true>(a);
}

struct Mem2Args {
    Wk2Sea sea;               // the Morison lane's tables (hc_ctx::mor2, shared with the elements), mwl of the Morison options
    const double* mem;        // as MemArgs
    const int* desc;
    const int* node_member;
    const int* point_member;
    const double* state;
    int N;
    double t;
    int ramped;               // ramp * ramp applies (apply_ramp, a synthesised irregular model, ramp_duration > 0)
    double ramp_duration;
    double* h;                // [n_nodes]: h_j of the nodes kernel in, h_j - eta2_j out
    double* nodes;            // [n_nodes][kMemNodeIncDoubles]
    double* points;           // [n_points][kMemPointIncDoubles], with directions [n_points][kMemPointDirIncDoubles]
};

// One workgroup per node, behind morison_member_nodes_kernel: the node's point (member_node) in scalar registers, the pair sum of
// hc_wave_kinematics2 for eta2 alone -- no depth profile is touched --, and work item 0 stores P_j, eta2_j and h_j - eta2_j: the
// value it stores is what that call returns for the stored point, bit for bit.
template <bool DIR>
__global__ void __launch_bounds__(kWk2Threads) morison_member2_nodes_kernel(Mem2Args a) {
    const int e       = blockIdx.x;  // the grid is n_nodes
    const int m       = a.node_member[e];
    const int* ds     = a.desc + kMemInts * m;
    const double* pos = a.state + 3 * ds[0];
    const MemNode p   = member_node(a.mem + static_cast<size_t>(kMemDoubles) * m, pos, pos + 3 * a.N, e - ds[2], ds[1]);
    const double x = wave_uniform(p.x), y = wave_uniform(p.y), z = wave_uniform(p.z);
    double sum[wk2_sums(DIR)];
    wk2_sea_sum<DIR, true, false>(a.sea, x, y, z, a.t, sum);
    if (threadIdx.x == 0) {
        const double eta2 = 0.25 * sum[0] * wk2_ramp2(a.ramped != 0, a.ramp_duration, a.t);
        double* out = a.nodes + static_cast<size_t>(kMemNodeIncDoubles) * e;
        out[0] = x;
        out[1] = y;
        out[2] = z;
        out[3] = eta2;
        a.h[e] = a.h[e] - eta2;
    }
}

// One workgroup per Gauss point, behind the kernel above: the point the items kernel evaluates (member_gauss, from the same h) in
// scalar registers, then the pair sum of hc_wave_kinematics2 at that point and time with the epilogue of morison2_incr_kernel.  A
// point of a dry segment stores its point and exact zeros and runs no pair sum: both h values are the same in every work item, so
// the whole workgroup leaves before the sum's first barrier.
template <bool DIR>
__global__ void __launch_bounds__(kWk2Threads) morison_member2_points_kernel(Mem2Args a) {
    constexpr int kWidth = DIR ? kMemPointDirIncDoubles : kMemPointIncDoubles;
    const int e       = blockIdx.x;  // the grid is n_points
    const int m       = a.point_member[e];
    const int* ds     = a.desc + kMemInts * m;
    const int local   = e - ds[3], seg = local >> 1;
    const double* pos = a.state + 3 * ds[0];
    const MemGauss gp = member_gauss(a.mem + static_cast<size_t>(kMemDoubles) * m, pos, pos + 3 * a.N, a.h[ds[2] + seg], a.h[ds[2] + seg + 1],
                                     seg, local & 1, ds[1]);
    const double x = wave_uniform(gp.x), y = wave_uniform(gp.y), z = wave_uniform(gp.z);
    double* out = a.points + static_cast<size_t>(kWidth) * e;
    if (!(gp.w0 || gp.w1)) {  // a dry segment
        if (threadIdx.x == 0) {
            out[0] = x;
            out[1] = y;
            out[2] = z;
#pragma unroll
            for (int k = 3; k < kWidth; ++k) out[k] = 0.0;
        }
        return;
    }
    double sum[wk2_sums(DIR)];
    wk2_sea_sum<DIR, true, true>(a.sea, x, y, z, a.t, sum);
    if (threadIdx.x == 0) {
        const double ramp2 = wk2_ramp2(a.ramped != 0, a.ramp_duration, a.t);
        out[0] = x;
        out[1] = y;
        out[2] = z;
        out[3] = 0.25 * sum[0] * ramp2;
#pragma unroll
        for (int k = 1; k < wk2_sums(DIR); ++k) out[3 + k] = sum[k] * ramp2;
    }
}

// The two sum levels, one launch each.  One work item per (group, component): the serial sum, in index order, of the rows
// [scale off[g], scale off[g + 1]) of `in`.  Level one: a member's Gauss points (off: the members' first segments, scale 2).
// Level two: a body's members (off: the owned bodies' first members, scale 1).  Plain vector stores, no atomics.  W components per
// row: 6 for the force, kMassEntries for the added-mass matrix (morison_member_mass_sum_kernel).
template <int W>
__device__ __forceinline__ void morison_member_sum_body(const double* in, const int* off, int scale, int rows, double* out) {
    const int row = blockIdx.x * kMemThreads + threadIdx.x;
    if (row >= rows) return;
    const int g = row / W, k = row - W * g;
    double acc = 0.0;
    for (int e = scale * off[g]; e < scale * off[g + 1]; ++e) acc += in[W * static_cast<size_t>(e) + k];
    out[row] = acc;
}
__global__ void __launch_bounds__(kMemThreads) morison_member_sum_kernel(const double* in, const int* off, int scale, int rows, double* out) {
    morison_member_sum_body<6>(in, off, scale, rows, out);
}
__global__ void __launch_bounds__(kMemThreads) morison_member_mass_sum_kernel(const double* in, const int* off, int scale, int rows,
                                                                              double* out) {
    morison_member_sum_body<kMassEntries>(in, off, scale, rows, out);
}

// 3.7c''' the added-mass matrix on the instantaneous wet length (hc_set_morison_member_added_mass).  One work item per Gauss point,
// indexed as in morison_member_items_kernel, behind it on the stream: whichever node kernels ran have left h (eta1, and eta2 on the
// second-order sea) in place, and member_gauss makes of it the wet interval, w_g, D_g, R and d of the force item, bit for bit.  No
// component loop, no LDS.  With a^ = R (r1 - r0) / L, P = I - a^ a^T, S = [d]x, c = d x a^ and m_g = w_g rho ca (pi / 4) D_g^2 the
// item is
//     m_g [ P, -P S ; S P, -S P S ],   -P S = -(S + a^ c^T),   -S P S = |d|^2 I - d d^T - c c^T
// of which the 21 upper entries are stored row by row (the getters mirror them).  A point of a dry segment and a point of a member
// with ca = 0 store exact zeros.
struct MemMassArgs {
    int n_points;
    int N;
    const double* mem;         // as MemArgs
    const int* desc;
    const int* point_member;
    const double* ca;          // [members]
    const double* state;
    const double* h;           // [n_nodes], as the force items read it
    double rho;
    double* item;              // [n_points][kMassEntries]
};

__global__ void __launch_bounds__(kMemThreads) morison_member_mass_kernel(MemMassArgs a) {
    const int o       = blockIdx.x * kMemThreads + threadIdx.x;
    const bool active = o < a.n_points;
    const int e       = active ? o : 0;  // items past the end evaluate item 0 and store nothing
    const int m       = a.point_member[e];
    const int* dsc    = a.desc + kMemInts * m;
    const int n_seg = dsc[1], local = e - dsc[3];
    const int seg = local >> 1, g = local & 1;
    const double* mem = a.mem + static_cast<size_t>(kMemDoubles) * m;
    const double* pos = a.state + 3 * dsc[0];
    const MemGauss gp = member_gauss(mem, pos, pos + 3 * a.N, a.h[dsc[2] + seg], a.h[dsc[2] + seg + 1], seg, g, n_seg);
    if (!active) return;
    double* out     = a.item + static_cast<size_t>(kMassEntries) * o;
    const double ca = a.ca[m];
    if (!(gp.w0 || gp.w1) || ca == 0.0) {
#pragma unroll
        for (int k = 0; k < kMassEntries; ++k) out[k] = 0.0;
        return;
    }
    const MemRot f   = gp.f;
    const double len = mem[6];
    const double ex = mem[3] / len, ey = mem[4] / len, ez = mem[5] / len;
    const double t0 = f.r00 * ex + f.r01 * ey + f.r02 * ez;
    const double t1 = f.r10 * ex + f.r11 * ey + f.r12 * ez;
    const double t2 = f.r20 * ex + f.r21 * ey + f.r22 * ez;
    const double d0 = gp.d0, d1 = gp.d1, d2 = gp.d2;
    const double c0 = d1 * t2 - d2 * t1, c1 = d2 * t0 - d0 * t2, c2 = d0 * t1 - d1 * t0;
    const double mg = gp.wg * (a.rho * ca * kQuarterPi * gp.diam * gp.diam);
    // row 0: P00 P01 P02 | -(P S)00 -(P S)01 -(P S)02
    out[0] = mg * (1.0 - t0 * t0);
    out[1] = mg * (-(t0 * t1));
    out[2] = mg * (-(t0 * t2));
    out[3] = mg * (-(t0 * c0));
    out[4] = mg * (d2 - t0 * c1);
    out[5] = mg * (-d1 - t0 * c2);
    // row 1: P11 P12 | -(P S)10 -(P S)11 -(P S)12
    out[6]  = mg * (1.0 - t1 * t1);
    out[7]  = mg * (-(t1 * t2));
    out[8]  = mg * (-d2 - t1 * c0);
    out[9]  = mg * (-(t1 * c1));
    out[10] = mg * (d0 - t1 * c2);
    // row 2: P22 | -(P S)20 -(P S)21 -(P S)22
    out[11] = mg * (1.0 - t2 * t2);
    out[12] = mg * (d1 - t2 * c0);
    out[13] = mg * (-d0 - t2 * c1);
    out[14] = mg * (-(t2 * c2));
    // rows 3 to 5: the upper entries of -S P S
    out[15] = mg * ((d1 * d1 + d2 * d2) - c0 * c0);
    out[16] = mg * (-(d0 * d1) - c0 * c1);
    out[17] = mg * (-(d0 * d2) - c0 * c2);
    out[18] = mg * ((d0 * d0 + d2 * d2) - c1 * c1);
    out[19] = mg * (-(d1 * d2) - c1 * c2);
    out[20] = mg * ((d0 * d0 + d1 * d1) - c2 * c2);
}

// the device copy of the owned bodies' lists, body-major
void upload_members(hc_ctx* c) {
    MorisonMemberData& d = c->members;
    std::vector<double> tab;
    std::vector<int> desc, node_member, point_member, seg_off(1, 0);
    d.off.assign(c->nloc + 1, 0);
    d.node_off.assign(c->nloc + 1, 0);
    d.point_off.assign(c->nloc + 1, 0);
    int segs = 0;
    for (int b = c->b0; b < c->b1; ++b) {
        for (const hc_morison_member& m : d.lists[b]) {
            const int idx = static_cast<int>(desc.size()) / kMemInts;
            const double e[3] = {m.r1[0] - m.r0[0], m.r1[1] - m.r0[1], m.r1[2] - m.r0[2]};
            tab.insert(tab.end(), m.r0, m.r0 + 3);
            tab.insert(tab.end(), e, e + 3);
            tab.push_back(std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
            tab.push_back(m.d0);
            tab.push_back(m.d1);
            tab.push_back(m.cd);
            tab.push_back(m.cm);
            desc.push_back(b);
            desc.push_back(m.n_seg);
            desc.push_back(static_cast<int>(node_member.size()));
            desc.push_back(static_cast<int>(point_member.size()));
            node_member.insert(node_member.end(), m.n_seg + 1, idx);
            point_member.insert(point_member.end(), 2 * m.n_seg, idx);
            segs += m.n_seg;
            seg_off.push_back(segs);
        }
        d.off[b - c->b0 + 1] = static_cast<int>(desc.size()) / kMemInts;
        d.node_off[b - c->b0 + 1]  = static_cast<int>(node_member.size());
        d.point_off[b - c->b0 + 1] = static_cast<int>(point_member.size());
    }
    // the first-segment list of level one and the first-member list of level two, one behind the other
    std::vector<int> offs(seg_off);
    offs.insert(offs.end(), d.off.begin(), d.off.end());
    hipStream_t st = c->mor.stream;
    d.tab.upload(tab, st);
    d.desc.upload(desc, st);
    d.node_member.upload(node_member, st);
    d.point_member.upload(point_member, st);
    d.d_off.upload(offs, st);
    d.members = static_cast<int>(desc.size()) / kMemInts;
    d.nodes   = static_cast<int>(node_member.size());
    d.points  = static_cast<int>(point_member.size());
    if (d.h.n < static_cast<size_t>(d.nodes)) d.h.alloc(d.nodes);
    if (d.item.n < 6 * static_cast<size_t>(d.points)) d.item.alloc(6 * static_cast<size_t>(d.points));
    if (d.mout.n < 6 * static_cast<size_t>(d.members)) d.mout.alloc(6 * static_cast<size_t>(d.members));
    if (d.h_mout.n < 6 * static_cast<size_t>(d.members)) d.h_mout.alloc(6 * static_cast<size_t>(d.members));
    if (d.out.n < static_cast<size_t>(c->Dloc)) d.out.alloc(c->Dloc);
    if (d.h_out.n < static_cast<size_t>(c->Dloc)) d.h_out.alloc(c->Dloc);
    d.dirty    = false;
    d.ca_dirty = true;  // the members have other places
}

// The device copy of ca, in the order of the member table (upload_members has run).  With no ca > 0 on any owned member the mass
// part has no buffer at all.
void upload_added_mass(hc_ctx* c) {
    MorisonMemberData& d = c->members;
    std::vector<double> ca;
    bool any = false;
    for (int b = c->b0; b < c->b1; ++b) {
        const size_t n = d.lists[b].size();
        if (d.ca.empty() || d.ca[b].empty()) ca.insert(ca.end(), n, 0.0);
        else ca.insert(ca.end(), d.ca[b].begin(), d.ca[b].end());
    }
    for (double v : ca) any = any || v > 0.0;
    d.mass     = any;
    d.ca_dirty = false;
    if (!any) {
        d.d_ca.release();
        d.mass_item.release();
        d.mass_mout.release();
        d.mass_out.release();
        d.h_mass_mout.alloc(0);
        d.h_mass_out.alloc(0);
        return;
    }
    const size_t W = kMassEntries;
    d.d_ca.upload(ca, c->mor.stream);
    if (d.mass_item.n < W * d.points) d.mass_item.alloc(W * d.points);
    if (d.mass_mout.n < W * d.members) d.mass_mout.alloc(W * d.members);
    if (d.h_mass_mout.n < W * d.members) d.h_mass_mout.alloc(W * d.members);
    if (d.mass_out.n < W * c->nloc) d.mass_out.alloc(W * c->nloc);
    if (d.h_mass_out.n < W * c->nloc) d.h_mass_out.alloc(W * c->nloc);
}

// The mass launches of one evaluation, behind the member force's on the lane's stream: the items from the h the force items read,
// then the two sum levels of the force over kMassEntries components, and the copies to the pinned staging.
void mass_enqueue(hc_ctx* c, const double* d_state) {
    MorisonMemberData& d = c->members;
    hipStream_t st       = c->mor.stream;
    MemMassArgs a{};
    a.n_points     = d.points;
    a.N            = c->N;
    a.mem          = d.tab.p;
    a.desc         = d.desc.p;
    a.point_member = d.point_member.p;
    a.ca           = d.d_ca.p;
    a.state        = d_state;
    a.h            = d.h.p;
    a.rho          = c->rho;
    a.item         = d.mass_item.p;
    d.mass_flight  = true;
    hipLaunchKernelGGL(morison_member_mass_kernel, dim3((a.n_points + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    const int rows1 = kMassEntries * d.members, rows2 = kMassEntries * c->nloc;
    hipLaunchKernelGGL(morison_member_mass_sum_kernel, dim3((rows1 + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st,
                       d.mass_item.p, d.d_off.p, 2, rows1, d.mass_mout.p);
    HC_HIP(hipGetLastError());
    hipLaunchKernelGGL(morison_member_mass_sum_kernel, dim3((rows2 + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st,
                       d.mass_mout.p, d.d_off.p + (d.members + 1), 1, rows2, d.mass_out.p);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(d.h_mass_mout.p, d.mass_mout.p, static_cast<size_t>(rows1) * sizeof(double), hipMemcpyDeviceToHost, st));
    HC_HIP(hipMemcpyAsync(d.h_mass_out.p, d.mass_out.p, static_cast<size_t>(rows2) * sizeof(double), hipMemcpyDeviceToHost, st));
}

// the 36 entries of a matrix from its 21 upper ones: M == M^T bitwise
void mass_unpack(const double* up, double* M) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) M[6 * i + j] = M[6 * j + i] = up[k];
}

// what the two matrix getters answer from, or HC_ERR_INVALID
void require_mass_answer(const hc_ctx* c, int body, const double* out) {
    require(body >= c->b0 && body < c->b1, HC_ERR_INVALID, "body not owned by this context");
    require(out != nullptr, HC_ERR_INVALID, "null output");
    require(c->members.mass_done, HC_ERR_INVALID,
            "no Morison evaluation with an added-mass part has completed since a member list or ca was last set "
            "(hc_set_morison_member_added_mass)");
}

}  // namespace

int members_owned(const hc_ctx* c) {
    int n = 0;
    if (!c->members.lists.empty())
        for (int b = c->b0; b < c->b1; ++b) n += static_cast<int>(c->members.lists[b].size());
    return n;
}

void members_enqueue(hc_ctx* c, double t, const double* d_state, bool order2) {
    MorisonMemberData& d = c->members;
    hipStream_t st       = c->mor.stream;
    d.done               = false;
    if (d.dirty) upload_members(c);
    MemArgs a{};
    a.tab          = c->mor.kin.tab.p;
    a.nf           = c->mor.kin.nf;
    a.n_nodes      = d.nodes;
    a.n_points     = d.points;
    a.mem          = d.tab.p;
    a.desc         = d.desc.p;
    a.node_member  = d.node_member.p;
    a.point_member = d.point_member.p;
    a.state        = d_state;
    a.N            = c->N;
    a.t            = t;
    a.depth        = c->depth;
    a.mwl          = c->mor.opts.mwl;
    a.rho          = c->rho;
    a.ramp         = kin_ramp(c, t);
    a.stretch      = (kin_synthesised(c) && c->mor.opts.wave_stretching) ? 1 : 0;  // as for the elements
    a.finite_depth = std::isfinite(c->depth) ? 1 : 0;
    a.h            = d.h.p;
    a.item         = d.item.p;
    const bool dir = c->mor.kin.dir;
    d.flight       = true;
    hipLaunchKernelGGL(dir ? morison_member_nodes_kernel<true> : morison_member_nodes_kernel<false>,
                       dim3((a.n_nodes + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    // the second-order sea: eta2 at the nodes, off h before the cut; then the increments at the Gauss points the cut yields
    if (order2) {
        const int width = dir ? kMemPointDirIncDoubles : kMemPointIncDoubles;
        const int slot  = d.copies.stage(width, d.node_off, d.point_off);
        const size_t n  = d.copies.layout[slot].doubles();
        if (d.inc.n < n) d.inc.alloc(n);
        if (d.h_inc[slot].n < n) d.h_inc[slot].alloc(n);
        Mem2Args m{};
        m.sea           = c->mor2.sea(c, a.mwl);
        m.mem           = a.mem;
        m.desc          = a.desc;
        m.node_member   = a.node_member;
        m.point_member  = a.point_member;
        m.state         = a.state;
        m.N             = a.N;
        m.t             = t;
        m.ramped        = c->mor2.ramped(c);
        m.ramp_duration = c->irr.ramp_duration;
        m.h             = d.h.p;
        m.nodes         = d.inc.p;
        m.points        = d.inc.p + d.copies.layout[slot].point_base();
        a.inc           = m.points;
        hipLaunchKernelGGL(dir ? morison_member2_nodes_kernel<true> : morison_member2_nodes_kernel<false>, dim3(a.n_nodes), dim3(kWk2Threads), 0,
                           st, m);
        HC_HIP(hipGetLastError());
        hipLaunchKernelGGL(dir ? morison_member2_points_kernel<true> : morison_member2_points_kernel<false>, dim3(a.n_points), dim3(kWk2Threads),
                           0, st, m);
        HC_HIP(hipGetLastError());
        HC_HIP(hipMemcpyAsync(d.h_inc[slot].p, d.inc.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL(order2 ? (dir ? morison_member2_items_kernel<true> : morison_member2_items_kernel<false>)
                              : (dir ? morison_member_items_kernel<true> : morison_member_items_kernel<false>),
                       dim3((a.n_points + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st, a);
    HC_HIP(hipGetLastError());
    const int rows1 = 6 * d.members;
    hipLaunchKernelGGL(morison_member_sum_kernel, dim3((rows1 + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st, d.item.p, d.d_off.p, 2,
                       rows1, d.mout.p);
    HC_HIP(hipGetLastError());
    hipLaunchKernelGGL(morison_member_sum_kernel, dim3((c->Dloc + kMemThreads - 1) / kMemThreads), dim3(kMemThreads), 0, st, d.mout.p,
                       d.d_off.p + (d.members + 1), 1, c->Dloc, d.out.p);
    HC_HIP(hipGetLastError());
    HC_HIP(hipMemcpyAsync(d.h_mout.p, d.mout.p, static_cast<size_t>(rows1) * sizeof(double), hipMemcpyDeviceToHost, st));
    HC_HIP(hipMemcpyAsync(d.h_out.p, d.out.p, static_cast<size_t>(c->Dloc) * sizeof(double), hipMemcpyDeviceToHost, st));
    // the added-mass matrix on the same wet cut; with no ca > 0 on an owned member nothing more is launched
    d.mass_done = false;
    if (d.ca_dirty) upload_added_mass(c);
    if (d.mass) mass_enqueue(c, d_state);
}

// what the two increment getters answer with, or HC_ERR_INVALID (the rules of hc_get_morison_increments)
const MemberIncrementLayout& member_increments_answer(const hc_ctx* c, int body) {
    require(c->members.order2, HC_ERR_INVALID,
            "Morison strip members on the second-order sea are switched off (hc_set_morison_members_second_order)");
    require(body >= c->b0 && body < c->b1, HC_ERR_INVALID, "body not owned by this context");
    require(c->members.copies.done, HC_ERR_INVALID,
            "no Morison evaluation with a second-order member part has completed since a member list was last set");
    return c->members.copies.last();
}

}  // namespace hc

extern "C" {

int hc_set_morison_members(hc_ctx* c, int body, const hc_morison_member* members, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    require(n >= 0 && n <= hc::kMorisonMaxMembers, HC_ERR_INVALID, "member count negative or above the limit per body");
    require(n == 0 || members, HC_ERR_INVALID, "null member list");
    c->mor.require_idle("a Morison evaluation is in flight (hc_morison_end has not been called)");
    for (int e = 0; e < n; ++e) {
        const hc_morison_member& m = members[e];
        const double v[4]          = {m.d0, m.d1, m.cd, m.cm};
        require(hc::all_finite(m.r0, 3) && hc::all_finite(m.r1, 3) && hc::all_finite(v, 4), HC_ERR_INVALID, "non-finite value in a Morison member");
        require(m.d0 >= 0.0 && m.d1 >= 0.0, HC_ERR_INVALID, "negative diameter of a Morison member");
        require(m.cd >= 0.0 && m.cm >= 0.0, HC_ERR_INVALID, "negative coefficient of a Morison member");
        require(m.r0[0] != m.r1[0] || m.r0[1] != m.r1[1] || m.r0[2] != m.r1[2], HC_ERR_INVALID, "a Morison member of zero length (r0 == r1)");
        require(m.n_seg >= 1 && m.n_seg <= hc::kMorisonMaxSegments, HC_ERR_INVALID, "n_seg of a Morison member outside 1..64");
    }
    c->mor.open();
    if (c->members.lists.empty()) c->members.lists.resize(c->N);
    c->members.lists[body].assign(members, members + n);
    c->members.dirty = true;
    c->members.done  = false;  // hc_get_morison_member_forces: the lists of the last evaluation are no longer the lists
    c->members.copies.forget();  // ... nor for the two increment getters
    if (!c->members.ca.empty()) c->members.ca[body].clear();  // the new list starts with ca = 0
    c->members.mass_done = false;
    HC_API_END(c)
}

int hc_set_morison_member_added_mass(hc_ctx* c, int body, const double* ca, int n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    c->mor.require_idle("a Morison evaluation is in flight (hc_morison_end has not been called)");
    const int members = c->members.lists.empty() ? 0 : static_cast<int>(c->members.lists[body].size());
    const bool clear  = ca == nullptr || n == 0;
    require(clear || n == members, HC_ERR_INVALID, "n is not the member count of the body (hc_get_morison_member_count)");
    if (!clear) {
        require(hc::all_finite(ca, static_cast<size_t>(n)), HC_ERR_INVALID, "non-finite added-mass coefficient of a Morison member");
        for (int e = 0; e < n; ++e) require(ca[e] >= 0.0, HC_ERR_INVALID, "negative added-mass coefficient of a Morison member");
    }
    if (c->members.ca.empty()) c->members.ca.resize(c->N);
    if (clear) c->members.ca[body].clear();
    else c->members.ca[body].assign(ca, ca + n);
    c->members.ca_dirty  = true;
    c->members.mass_done = false;  // the matrices of the last evaluation are no longer those of the coefficients
    HC_API_END(c)
}

int hc_get_morison_member_added_mass_coefficients(hc_ctx* c, int body, double* ca) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    const size_t n = c->members.lists.empty() ? 0 : c->members.lists[body].size();
    require(n == 0 || ca, HC_ERR_INVALID, "null output");
    if (c->members.ca.empty() || c->members.ca[body].empty()) std::fill(ca, ca + n, 0.0);
    else std::copy(c->members.ca[body].begin(), c->members.ca[body].end(), ca);
    HC_API_END(c)
}

int hc_get_morison_added_mass(hc_ctx* c, int body, double* M) {
    HC_API_BEGIN_HOT(c)
    hc::require_mass_answer(c, body, M);
    hc::mass_unpack(c->members.h_mass_out.p + static_cast<size_t>(hc::kMassEntries) * (body - c->b0), M);
    HC_API_END(c)
}

int hc_get_morison_member_added_mass(hc_ctx* c, int body, double* out) {
    HC_API_BEGIN_HOT(c)
    hc::require_mass_answer(c, body, out);
    const int m0 = c->members.off[body - c->b0], m1 = c->members.off[body - c->b0 + 1];
    for (int m = m0; m < m1; ++m)
        hc::mass_unpack(c->members.h_mass_mout.p + static_cast<size_t>(hc::kMassEntries) * m, out + 36 * static_cast<size_t>(m - m0));
    HC_API_END(c)
}

int hc_set_morison_members_second_order(hc_ctx* c, int on) {
    HC_API_BEGIN_HOT(c)
    c->mor.require_idle("a Morison evaluation is in flight (hc_morison_end has not been called)");
    c->members.order2 = on != 0;
    if (!on) {  // the increments and their two host copies go (nothing of the lane is in flight)
        c->members.copies.forget();
        c->members.inc.release();
        c->members.h_inc[0].alloc(0);
        c->members.h_inc[1].alloc(0);
    }
    HC_API_END(c)
}

int hc_get_morison_member_increment_counts(hc_ctx* c, int body, int* nodes, int* points) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N, HC_ERR_INVALID, "body index out of range");
    int segs = 0, members = 0;
    if (!c->members.lists.empty())
        for (const hc_morison_member& m : c->members.lists[body]) segs += m.n_seg, ++members;
    if (nodes) *nodes = segs + members;
    if (points) *points = 2 * segs;
    HC_API_END(c)
}

int hc_get_morison_members_second_order(hc_ctx* c, int* on) {
    HC_API_BEGIN_HOT(c)
    if (on) *on = c->members.order2 ? 1 : 0;
    HC_API_END(c)
}

int hc_get_morison_member_node_increments(hc_ctx* c, int body, double* p, double* eta2) {
    HC_API_BEGIN_HOT(c)
    const hc::MemberIncrementLayout& l = hc::member_increments_answer(c, body);
    const double* q = c->members.h_inc[c->members.copies.cur].p;
    const int j0 = l.node_off[body - c->b0], j1 = l.node_off[body - c->b0 + 1];
    for (int j = j0; j < j1; ++j) {
        const double* v = q + static_cast<size_t>(hc::kMemNodeIncDoubles) * j;
        const size_t i  = static_cast<size_t>(j - j0);
        if (p) std::copy(v, v + 3, p + 3 * i);
        if (eta2) eta2[i] = v[3];
    }
    HC_API_END(c)
}

int hc_get_morison_member_point_increments(hc_ctx* c, int body, double* p, double* eta2, double* vel2, double* acc2) {
    HC_API_BEGIN_HOT(c)
    const hc::MemberIncrementLayout& l = hc::member_increments_answer(c, body);
    const double* q = c->members.h_inc[c->members.copies.cur].p + l.point_base();
    const int e0 = l.point_off[body - c->b0], e1 = l.point_off[body - c->b0 + 1];
    for (int e = e0; e < e1; ++e) {
        const double* v = q + static_cast<size_t>(l.width) * e;
        const size_t i  = static_cast<size_t>(e - e0);
        if (p) std::copy(v, v + 3, p + 3 * i);
        if (eta2) eta2[i] = v[3];
        if (l.width == hc::kMemPointDirIncDoubles) {
            if (vel2) std::copy(v + 4, v + 7, vel2 + 3 * i);
            if (acc2) std::copy(v + 7, v + 10, acc2 + 3 * i);
        } else {
            if (vel2) vel2[3 * i] = v[4], vel2[3 * i + 1] = 0.0, vel2[3 * i + 2] = v[5];
            if (acc2) acc2[3 * i] = v[6], acc2[3 * i + 1] = 0.0, acc2[3 * i + 2] = v[7];
        }
    }
    HC_API_END(c)
}

int hc_get_morison_member_count(hc_ctx* c, int body, int* n) {
    HC_API_BEGIN_HOT(c)
    require(body >= 0 && body < c->N && n, HC_ERR_INVALID, "body index out of range or null pointer");
    *n = c->members.lists.empty() ? 0 : static_cast<int>(c->members.lists[body].size());
    HC_API_END(c)
}

int hc_get_morison_member_forces(hc_ctx* c, int body, double* out) {
    HC_API_BEGIN_HOT(c)
    require(body >= c->b0 && body < c->b1, HC_ERR_INVALID, "body not owned by this context");
    require(out != nullptr, HC_ERR_INVALID, "null output");
    require(c->members.done, HC_ERR_INVALID, "no Morison evaluation with members has completed since a member list was last set");
    const int m0 = c->members.off[body - c->b0], m1 = c->members.off[body - c->b0 + 1];
    std::copy(c->members.h_mout.p + 6 * static_cast<size_t>(m0), c->members.h_mout.p + 6 * static_cast<size_t>(m1), out);
    HC_API_END(c)
}

}  // extern "C"
