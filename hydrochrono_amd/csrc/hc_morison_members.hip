// hc_morison_members.hip -- Morison strip members: slender cylinders given by two end points, integrated along their wet length and
// cut at the instantaneous free surface (include/hydrochrono_amd.h: hc_set_morison_members).  Not in the reference.  On the lane of
// the Morison elements (hc_morison.hip: hc_morison_begin / hc_morison_end; hc_side.hpp), behind their launches: the lane's stream,
// component table and options, buffers and pinned staging of its own.  DESIGN.md 3.7c' has the definition, the kernels and their
// invariants.  The kernels carry their own component loop, built from the pieces of hc_wave_kin.hpp.
#include "hc_morison_members.hpp"

#include "hc_internal.hpp"
#include "hc_wave_kin.hpp"

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kMemThreads = 256;    // work items per workgroup
constexpr int kMemDoubles = 11;     // r0, r1 - r0, |r1 - r0|, d0, d1, cd, cm
constexpr int kMemInts = 4;         // body, n_seg, first node, first Gauss point
constexpr double kGaussLo = 0.21132486540518711775;  // 1/2 - 1/(2 sqrt 3)
constexpr double kGaussHi = 0.78867513459481288225;  // 1/2 + 1/(2 sqrt 3)
constexpr double kQuarterPi = 0.78539816339744830962;

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
    const MemRot f    = member_rotation(pos + 3 * a.N);
    const double sj   = static_cast<double>(j) / static_cast<double>(n_seg);
    const double rx = mem[0] + sj * mem[3], ry = mem[1] + sj * mem[4], rz = mem[2] + sj * mem[5];
    const double x = pos[0] + (f.r00 * rx + f.r01 * ry + f.r02 * rz);
    const double y = DIR ? pos[1] + (f.r10 * rx + f.r11 * ry + f.r12 * rz) : 0.0;
    const double z = pos[2] + (f.r20 * rx + f.r21 * ry + f.r22 * rz);
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
template <bool DIR>
__global__ void __launch_bounds__(kMemThreads) morison_member_items_kernel(MemArgs a) {
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

    // ---- the wet interval [sa, sb] of the segment, local coordinate from node `seg` ----
    const double hx = a.h[dsc[2] + seg], hy = a.h[dsc[2] + seg + 1];
    const bool w0 = hx <= 0.0, w1 = hy <= 0.0;
    double sa = 0.0, sb = (w0 && w1) ? 1.0 : 0.0;
    if (w0 != w1) {  // one cut, measured from the wet end: h_wet <= 0 < h_dry, the denominator is negative
        const double hw = w0 ? hx : hy, hd = w0 ? hy : hx;
        const double cut = hw / (hw - hd);
        sa = w0 ? 0.0 : 1.0 - cut;
        sb = w0 ? cut : 1.0;
    }
    const double width = sb - sa;
    const double sg    = sa + width * (g ? kGaussHi : kGaussLo);
    const double along = (static_cast<double>(seg) + sg) / static_cast<double>(n_seg);
    const double len   = mem[6];
    const double wg    = 0.5 * width * len / static_cast<double>(n_seg);
    const double diam  = mem[7] + along * (mem[8] - mem[7]);

    // ---- R, d = R r_g, p = pos + d, the unit axis ----
    const MemRot f  = member_rotation(rpy);
    const double rx = mem[0] + along * mem[3], ry = mem[1] + along * mem[4], rz = mem[2] + along * mem[5];
    const double d0 = f.r00 * rx + f.r01 * ry + f.r02 * rz;
    const double d1 = f.r10 * rx + f.r11 * ry + f.r12 * rz;
    const double d2 = f.r20 * rx + f.r21 * ry + f.r22 * rz;
    const double x = pos[0] + d0, y = DIR ? pos[1] + d1 : 0.0, z = pos[2] + d2, t = a.t;

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
    const double afx = a.ramp * ax, afy = a.ramp * ay, afz = a.ramp * az;
    const double q0 = a.ramp * ux - (lin[0] + (w1a * d2 - w2a_ * d1));
    const double q1 = a.ramp * uy - (lin[1] + (w2a_ * d0 - w0a * d2));
    const double q2 = a.ramp * uz - (lin[2] + (w0a * d1 - w1a * d0));
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

// The two sum levels, one launch each.  One work item per (group, component): the serial sum, in index order, of the rows
// [scale off[g], scale off[g + 1]) of `in`.  Level one: a member's Gauss points (off: the members' first segments, scale 2).
// Level two: a body's members (off: the owned bodies' first members, scale 1).  Plain vector stores, no atomics.
__global__ void __launch_bounds__(kMemThreads) morison_member_sum_kernel(const double* in, const int* off, int scale, int rows, double* out) {
    const int row = blockIdx.x * kMemThreads + threadIdx.x;
    if (row >= rows) return;
    const int g = row / 6, k = row - 6 * g;
    double acc = 0.0;
    for (int e = scale * off[g]; e < scale * off[g + 1]; ++e) acc += in[6 * static_cast<size_t>(e) + k];
    out[row] = acc;
}

// the device copy of the owned bodies' lists, body-major
void upload_members(hc_ctx* c) {
    MorisonMemberData& d = c->members;
    std::vector<double> tab;
    std::vector<int> desc, node_member, point_member, seg_off(1, 0);
    d.off.assign(c->nloc + 1, 0);
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
    d.dirty = false;
}

}  // namespace

int members_owned(const hc_ctx* c) {
    int n = 0;
    if (!c->members.lists.empty())
        for (int b = c->b0; b < c->b1; ++b) n += static_cast<int>(c->members.lists[b].size());
    return n;
}

void members_enqueue(hc_ctx* c, double t, const double* d_state) {
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
    hipLaunchKernelGGL(dir ? morison_member_items_kernel<true> : morison_member_items_kernel<false>,
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
