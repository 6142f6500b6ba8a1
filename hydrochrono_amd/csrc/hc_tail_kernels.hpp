// hc_tail_kernels.hpp -- the kernels of the spectral radiation tail (hc_tail.hpp), included into hc_kernels.hip so that the
// stand-alone code object of the direct dispatch carries them.  All FP64; one transform of size N per workgroup (N = 2P of the level,
// hc_tail.hpp: TailLevel; instantiated for 256, 512 and 1024), radix-2 in LDS with a twiddle table made on the host per N; every sum
// in a fixed order that depends on neither the row range nor the launch geometry, so that row shards stay bitwise equal to the
// unsharded context.
//   tail_khat_kernel   (init) Khat[bin][row][(p-1)D + col] = FFT_N(w_s K[row, s, col], s in partition p, zero-padded)
//   tail_fft_fwd       (superblock start) Xw[bin][(a-1)D + col] = FFT_N(window a of DoF col, from ring_vT)
//   tail_gemv          Y[bin][row] = Yin[bin][row] + sum_c Khat[bin][row][c] Xw[bin][c + x_shift]  over a range of bins and columns
//   tail_fft_inv       tail[j][row] = Re(IFFT_N(Y[.][row]))[P + j] / N, the Hermitian half of Y extended to the full spectrum
#pragma once

namespace hc {

// N / 2 work items per transform: one butterfly per work item and stage.
// In-place radix-2 transform of the N points (re, im) in LDS, input in bit-reversed order.  tw[k] = exp(-2 pi i k / N) as
// (cos, sin) pairs; inverse: the conjugate twiddles.  Ends with a barrier.
template <int N>
__device__ __forceinline__ void tail_fft_lds(double* __restrict__ re, double* __restrict__ im, const double* __restrict__ tw, bool inverse) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll 1
    for (int len = 2; len <= N; len <<= 1) {
        const int half = len >> 1;
        const int pos  = t & (half - 1);
        const int i    = (t - pos) * 2 + pos;
        const int j    = i + half;
        const int k    = pos * (N / len);
        const double wr = tw[2 * k], wi = inverse ? -tw[2 * k + 1] : tw[2 * k + 1];
        const double br = re[j], bi = im[j];
        const double pr = wr * br - wi * bi, pi = wr * bi + wi * br;
        const double ar = re[i], ai = im[i];
        re[i] = ar + pr;
        im[i] = ai + pi;
        re[j] = ar - pr;
        im[j] = ai - pi;
        __syncthreads();
    }
}

constexpr int tail_log2(int n) { return n <= 1 ? 0 : 1 + tail_log2(n >> 1); }
template <int N>
__device__ __forceinline__ int tail_bitrev(int k) {
    static_assert(N >= 4 && (N & (N - 1)) == 0, "a transform of 2^b points");
    return static_cast<int>(__brev(static_cast<unsigned>(k)) >> (32 - tail_log2(N)));
}


template <int N>
__global__ void __launch_bounds__(N / 2) tail_khat_kernel(TailKhatArgs a) {
    constexpr int P = N / 2, kBins = P + 1, kThreads = N / 2;
    __shared__ double re[N], im[N];
    const int t   = threadIdx.x;
    const int col = blockIdx.x % a.D;
    const int rp  = blockIdx.x / a.D;
    const int p   = rp % a.NP + 1;
    const int row = rp / a.NP;
    for (int k = t; k < N; k += kThreads) {
        const int s = p * P + k;
        double g = 0.0;
        if (k < P && s < a.S) g = a.width[s] * a.K.base[panel_offset(a.K.ngp, row, s * a.D + col)];
        const int kr = tail_bitrev<N>(k);
        re[kr] = g;
        im[kr] = 0.0;
    }
    tail_fft_lds<N>(re, im, a.tw, false);
    const size_t ncols = static_cast<size_t>(a.NP) * a.D;
    const size_t c     = static_cast<size_t>(p - 1) * a.D + col;
    for (int b = t; b < kBins; b += kThreads) {
        double* dst = a.Khat + 2 * ((static_cast<size_t>(b) * a.Dloc + row) * ncols + c);
        dst[0] = re[b];
        dst[1] = im[b];
    }
}


template <int N>
__global__ void __launch_bounds__(N / 2) tail_fft_fwd(TailFwdArgs a) {
    constexpr int P = N / 2, kBins = P + 1, kThreads = N / 2;
    __shared__ double re[N], im[N];
    const int t   = threadIdx.x;
    const int col = blockIdx.x % a.D;
    const int w   = blockIdx.x / a.D + 1;  // window 1 .. NP
    const double* __restrict__ series = a.ring_vT + static_cast<size_t>(col) * a.HcapT;
    for (int k = t; k < N; k += kThreads) {
        const int back = (w + 1) * P - 1 - k;  // hc_tail.hpp: tail_window_back / tail_window_live
        double x = 0.0;
        if (k >= 1 && back <= a.S - 2) {
            int slot = (a.head - back) % a.Hcap;
            if (slot < 0) slot += a.Hcap;
            x = series[slot];
        }
        const int kr = tail_bitrev<N>(k);
        re[kr] = x;
        im[kr] = 0.0;
    }
    tail_fft_lds<N>(re, im, a.tw, false);
    const size_t ncols = static_cast<size_t>(a.NP) * a.D;
    const size_t c     = static_cast<size_t>(w - 1) * a.D + col;
    for (int b = t; b < kBins; b += kThreads) {
        double* dst = a.Xw + 2 * (static_cast<size_t>(b) * ncols + c);
        dst[0] = re[b];
        dst[1] = im[b];
    }
}

static constexpr int kTailGemvUnroll = 6;  // 16-byte loads per lane and row in flight
static constexpr int kTailGemvBatch  = 4;  // rows a wave streams at once

// One workgroup per (bin, rows_per_wg rows): the bin's X-hat columns go to LDS once, every wave then streams kTailGemvBatch whole rows
// of Khat at a time (16 bytes per lane, coalesced; 4 x 6 loads per lane in flight).  Lane l adds the columns col_lo + l + 64 i in order,
// the 64 lane sums are combined by a fixed butterfly: the same order for a row whatever the launch covers.
__global__ void __launch_bounds__(256) tail_gemv(TailGemvArgs a) {
    extern __shared__ double xs[];  // [col_hi - col_lo][2]
    const int nbin_rows = (a.Dloc + a.rows_per_wg - 1) / a.rows_per_wg;
    const int bin       = a.bin_lo + blockIdx.x / nbin_rows;
    const int row0      = (blockIdx.x % nbin_rows) * a.rows_per_wg;
    const int n         = a.col_hi - a.col_lo;
    const double* __restrict__ xsrc = a.Xw + 2 * (static_cast<size_t>(bin) * a.ncols + a.col_lo + a.x_shift);
    for (int i = threadIdx.x; i < 2 * n; i += 256) xs[i] = xsrc[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_end = min(a.Dloc, row0 + a.rows_per_wg);
    const dvec2* __restrict__ kbin = reinterpret_cast<const dvec2*>(a.Khat + 2 * (static_cast<size_t>(bin) * a.Dloc * a.ncols + a.col_lo));
    for (int rb = row0 + wave * kTailGemvBatch; rb < row_end; rb += 4 * kTailGemvBatch) {
        double sr[kTailGemvBatch], si[kTailGemvBatch];
#pragma unroll
        for (int q = 0; q < kTailGemvBatch; ++q) sr[q] = si[q] = 0.0;
        for (int c0 = 0; c0 < n; c0 += 64 * kTailGemvUnroll) {
            dvec2 kv[kTailGemvBatch][kTailGemvUnroll];
#pragma unroll
            for (int q = 0; q < kTailGemvBatch; ++q) {
                const int row = min(rb + q, row_end - 1);  // (rows past the end re-read the last one; their sums are not stored)
#pragma unroll
                for (int u = 0; u < kTailGemvUnroll; ++u) {
                    const int c = c0 + 64 * u + lane;
                    kv[q][u] = c < n ? __builtin_nontemporal_load(kbin + static_cast<size_t>(row) * a.ncols + c) : dvec2{0.0, 0.0};
                }
            }
#pragma unroll
            for (int u = 0; u < kTailGemvUnroll; ++u) {
                const int c = c0 + 64 * u + lane;
                const double xr = c < n ? xs[2 * c] : 0.0, xi = c < n ? xs[2 * c + 1] : 0.0;
#pragma unroll
                for (int q = 0; q < kTailGemvBatch; ++q) {
                    sr[q] = fma(kv[q][u].x, xr, sr[q]);
                    sr[q] = fma(-kv[q][u].y, xi, sr[q]);
                    si[q] = fma(kv[q][u].x, xi, si[q]);
                    si[q] = fma(kv[q][u].y, xr, si[q]);
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int q = 0; q < kTailGemvBatch; ++q) {
                sr[q] += __shfl_xor(sr[q], off, 64);
                si[q] += __shfl_xor(si[q], off, 64);
            }
        }
        if (lane < kTailGemvBatch && rb + lane < row_end) {
            double yr = sr[0], yi = si[0];
#pragma unroll
            for (int q = 1; q < kTailGemvBatch; ++q)
                if (lane == q) {
                    yr = sr[q];
                    yi = si[q];
                }
            const size_t o = 2 * (static_cast<size_t>(bin) * a.Dloc + rb + lane);
            if (a.Yin) {
                yr = a.Yin[o] + yr;
                yi = a.Yin[o + 1] + yi;
            }
            a.Yout[o]     = yr;
            a.Yout[o + 1] = yi;
        }
    }
}

template <int N>
__global__ void __launch_bounds__(N / 2) tail_fft_inv(TailInvArgs a) {
    constexpr int P = N / 2, kThreads = N / 2;
    __shared__ double re[N], im[N];
    const int t   = threadIdx.x;
    const int row = blockIdx.x;
    for (int k = t; k < N; k += kThreads) {
        // the Hermitian extension of bins 0 .. P; bins 0 and P of a real signal's transform are real
        const int b = k <= P ? k : N - k;
        const double* y = a.Y + 2 * (static_cast<size_t>(b) * a.Dloc + row);
        const double yr = y[0];
        double yi       = (b == 0 || b == P) ? 0.0 : y[1];
        if (k > P) yi = -yi;
        const int kr = tail_bitrev<N>(k);
        re[kr] = yr;
        im[kr] = yi;
    }
    tail_fft_lds<N>(re, im, a.tw, true);
    for (int j = t; j < P; j += kThreads) a.tail[static_cast<size_t>(j) * a.Dpad + row] = re[P + j] * (1.0 / N);
}

int tail_gemv_lds_bytes(const TailGemvArgs& g) { return 16 * (g.col_hi - g.col_lo); }
int tail_gemv_grid(const TailGemvArgs& g) { return (g.bin_hi - g.bin_lo) * ((g.Dloc + g.rows_per_wg - 1) / g.rows_per_wg); }

// The transform sizes of the levels (hc_tail.hpp: tail_levels); the direct dispatch finds these instantiations by name.
template __global__ void tail_khat_kernel<256>(TailKhatArgs);
template __global__ void tail_khat_kernel<512>(TailKhatArgs);
template __global__ void tail_khat_kernel<1024>(TailKhatArgs);
template __global__ void tail_fft_fwd<256>(TailFwdArgs);
template __global__ void tail_fft_fwd<512>(TailFwdArgs);
template __global__ void tail_fft_fwd<1024>(TailFwdArgs);
template __global__ void tail_fft_inv<256>(TailInvArgs);
template __global__ void tail_fft_inv<512>(TailInvArgs);
template __global__ void tail_fft_inv<1024>(TailInvArgs);

// (an N no level has: hipErrorInvalidValue, which the callers' HC_HIP turns into the library's error)
#define HC_TAIL_BY_N(n, call)                                 \
    switch (n) {                                              \
        case 256: { constexpr int kN = 256; call; break; }    \
        case 512: { constexpr int kN = 512; call; break; }    \
        case 1024: { constexpr int kN = 1024; call; break; }  \
        default: return hipErrorInvalidValue;                 \
    }                                                         \
    return hipSuccess;

hipError_t launch_tail_khat(const TailKhatArgs& a, int N, hipStream_t s) {
    HC_TAIL_BY_N(N, hipLaunchKernelGGL(tail_khat_kernel<kN>, dim3(static_cast<unsigned>(a.Dloc) * a.NP * a.D), dim3(kN / 2), 0, s, a))
}
hipError_t launch_tail_fwd(const TailFwdArgs& a, int N, hipStream_t s) {
    HC_TAIL_BY_N(N, hipLaunchKernelGGL(tail_fft_fwd<kN>, dim3(static_cast<unsigned>(a.NP) * a.D), dim3(kN / 2), 0, s, a))
}
void launch_tail_gemv(const TailGemvArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tail_gemv, dim3(static_cast<unsigned>(tail_gemv_grid(a))), dim3(256), static_cast<unsigned>(tail_gemv_lds_bytes(a)), s, a);
}
hipError_t launch_tail_inv(const TailInvArgs& a, int N, hipStream_t s) {
    HC_TAIL_BY_N(N, hipLaunchKernelGGL(tail_fft_inv<kN>, dim3(static_cast<unsigned>(a.Dloc)), dim3(kN / 2), 0, s, a))
}
#undef HC_TAIL_BY_N

}  // namespace hc
