// hc_qtf_dir.hip -- the kernels of the two QTF terms for tables on a heading x frequency grid (include/hydrochrono_amd.h:
// hc_set_drift_qtf_headings, hc_set_sum_qtf_headings).  Not in the reference.  A grid node is a (heading, frequency) pair
// p = a nq + m, J = nh nq <= 1024 of them; the evaluation form is that of hc_qtf.hip with nodes for bins and the phase of the
// directional kinematics.  A row's table has up to J^2 = 1 M entries, too many for one workgroup: the pair kernel sums chunks of 32
// node rows, the finish kernel adds a row's partials in ascending chunk order.  The host side (tables, node map, launches' arguments)
// is that of hc_qtf.hip.  DESIGN.md 3.7l.
#include "hc_qtf.hpp"

namespace hc {
namespace {

// the chunks of a slot: drift modes 1 and 2 read the diagonal alone, in the workgroup of chunk 0
template <QtfKind KIND>
__device__ __forceinline__ int qtf_dir_chunks(int mode, int J) {
    return (KIND == kQtfDrift && mode != 3) ? 1 : (J + kQtfDirRows - 1) / kQtfDirRows;
}

// Phase 1: u_i = A_i cos psi_i, w_i = A_i sin psi_i tile by tile through LDS, psi_i = k_i (x c_i + y s_i) - w_i t + phi_i; lane l
// owns the nodes l, l + 256, ... and adds each node's entries in component order into an accumulator pair of its own, whatever the
// tiling.  Leaves U_p, V_p in sU, sV (zero past the grid), visible to all.
__device__ __forceinline__ void qtf_dir_project(const QtfArgs& a, const long long* desc, int J, double* su, double* sw, double* sU,
                                                double* sV) {
    const int tid  = threadIdx.x;
    const size_t b = static_cast<size_t>(desc[kDescBody]);
    const double x = a.pos[3 * b], y = a.pos[3 * b + 1], t = a.t;
    const int* rp  = a.rowptr + desc[kDescRowPtr];
    int p[kQtfDirOwned], pend[kQtfDirOwned];
    double U[kQtfDirOwned], V[kQtfDirOwned];
#pragma unroll
    for (int r = 0; r < kQtfDirOwned; ++r) {
        const int node = tid + r * kQtfThreads;
        p[r]    = node < J ? rp[node] : 0;
        pend[r] = node < J ? rp[node + 1] : 0;
        U[r] = 0.0, V[r] = 0.0;
    }
    for (int i0 = 0; i0 < a.nf; i0 += kKinTile) {
        const int m = min(kKinTile, a.nf - i0);
        __syncthreads();
        if (tid < m) {
            const int i = i0 + tid;
            double sn, cs;
            sincos(kin_kx<true>(a.tab[kKinK * a.nf + i], x, y, a.tab[kKinCols * a.nf + i], a.tab[(kKinCols + 1) * a.nf + i]) -
                       a.tab[kKinOmega * a.nf + i] * t + a.tab[kKinPhase * a.nf + i],
                   &sn, &cs);
            const double A = a.tab[kKinAmp * a.nf + i];
            su[tid]        = A * cs;
            sw[tid]        = A * sn;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kQtfDirOwned; ++r) {
            while (p[r] < pend[r]) {
                const int i = a.ent_idx[p[r]];
                if (i >= i0 + m) break;
                const double w = a.ent_w[p[r]];
                U[r] += w * su[i - i0];
                V[r] += w * sw[i - i0];
                ++p[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kQtfDirOwned; ++r) {
        sU[tid + r * kQtfThreads] = U[r];
        sV[tid + r * kQtfThreads] = V[r];
    }
    __syncthreads();
}

// One workgroup per (chunk, slot, row d); a workgroup past its slot's chunk count leaves before any barrier.  qtf_dir_project, then
// the lanes stride over the chunk's entries of row d in ascending e (modes 1 and 2 of the drift term: over the diagonal), then the
// tree, whose shape depends on the lane index alone.  Lane 0 stores the chunk's partial.  A partial's bits depend on its body's table,
// pos[b].x, pos[b].y, t, the component table and the mode only.
template <QtfKind KIND>
__global__ void __launch_bounds__(kQtfThreads) qtf_dir_pair_kernel(QtfDirArgs g) {
    constexpr int R = KIND == kQtfDrift ? 4 : 1;
    __shared__ double su[kKinTile], sw[kKinTile];
    __shared__ double sU[kQtfMaxNodes], sV[kQtfMaxNodes];
    __shared__ double red[R][kQtfThreads];
    const QtfArgs& a      = g.a;
    const int tid         = threadIdx.x;
    const int chunk       = blockIdx.x;
    const int slot        = blockIdx.y / 6, d = blockIdx.y - 6 * slot;
    const long long* desc = a.desc + static_cast<size_t>(kDescWords) * slot;
    const int J           = static_cast<int>(desc[kDescNq]);
    if (chunk >= qtf_dir_chunks<KIND>(a.mode, J)) return;
    const double* P = a.pq + desc[kDescP] + static_cast<size_t>(d) * J * J;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;

    if (KIND == kQtfDrift && a.mode == 1) {
        const double* E = a.em + desc[kDescE];
        for (int p = tid; p < J; p += kQtfThreads) p0 += P[static_cast<size_t>(p) * J + p] * E[p];
    } else {
        qtf_dir_project(a, desc, J, su, sw, sU, sV);
        if (KIND == kQtfDrift && a.mode == 2) {
            for (int p = tid; p < J; p += kQtfThreads) {
                const double D = P[static_cast<size_t>(p) * J + p], U = sU[p], V = sV[p];
                p0 += D * U;
                p1 += U;
                p2 += D * V;
                p3 += V;
            }
        } else {
            const int e1 = min((chunk + 1) * kQtfDirRows, J) * J;
            if (desc[kDescQ] >= 0) {
                const double* Q = a.pq + desc[kDescQ] + static_cast<size_t>(d) * J * J;
                for (int e = chunk * kQtfDirRows * J + tid; e < e1; e += kQtfThreads) {
                    const int p = e / J, q = e - p * J;
                    p0 += qtf_pair_pq<KIND>(P[e], Q[e], sU[p], sV[p], sU[q], sV[q]);
                }
            } else {
                for (int e = chunk * kQtfDirRows * J + tid; e < e1; e += kQtfThreads) {
                    const int p = e / J, q = e - p * J;
                    p0 += qtf_pair_p<KIND>(P[e], sU[p], sV[p], sU[q], sV[q]);
                }
            }
        }
    }
    red[0][tid] = p0;
    if constexpr (R == 4) {
        red[1][tid] = p1;
        red[2][tid] = p2;
        red[3][tid] = p3;
    }
    qtf_tree<R>(red);
    if (tid == 0) {
        double F = red[0][0];
        if constexpr (R == 4)
            if (a.mode == 2) F = red[0][0] * red[1][0] + red[2][0] * red[3][0];
        g.part[static_cast<size_t>(blockIdx.y) * kQtfDirChunks + chunk] = F;
    }
}

// One work item per (slot, row d): the row's partials in ascending chunk order, times ramp^2
template <QtfKind KIND>
__global__ void __launch_bounds__(kQtfThreads) qtf_dir_finish_kernel(QtfDirArgs g, int rows) {
    const int r = blockIdx.x * kQtfThreads + threadIdx.x;
    if (r >= rows) return;
    const QtfArgs& a = g.a;
    const int J      = static_cast<int>(a.desc[static_cast<size_t>(kDescWords) * (r / 6) + kDescNq]);
    const int chunks = qtf_dir_chunks<KIND>(a.mode, J);
    const double* pt = g.part + static_cast<size_t>(r) * kQtfDirChunks;
    double F         = pt[0];
    for (int c = 1; c < chunks; ++c) F += pt[c];
    a.out[r] = F * a.ramp2;
}

template <QtfKind KIND>
void launch(const QtfDirArgs& g, int slots, int chunks, hipStream_t st) {
    const int rows = 6 * slots;
    hipLaunchKernelGGL(qtf_dir_pair_kernel<KIND>, dim3(static_cast<unsigned>(chunks), static_cast<unsigned>(rows)), dim3(kQtfThreads), 0, st, g);
    hipLaunchKernelGGL(qtf_dir_finish_kernel<KIND>, dim3(static_cast<unsigned>((rows + kQtfThreads - 1) / kQtfThreads)), dim3(kQtfThreads), 0,
                       st, g, rows);
}

}  // namespace

void qtf_dir_launch(const QtfDirArgs& g, QtfKind kind, int slots, int chunks, hipStream_t st) {
    if (kind == kQtfDrift)
        launch<kQtfDrift>(g, slots, chunks, st);
    else
        launch<kQtfSum>(g, slots, chunks, st);
}

}  // namespace hc
