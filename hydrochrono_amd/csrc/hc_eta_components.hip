// hc_eta_components.hip -- wave components of an imported eta record (include/hydrochrono_amd.h: hc_set_eta_record_components).
// Not in the reference, whose record branch has no spectrum.  The record's discrete Fourier coefficients on its own grid become the
// component table (A, w, k, phi) that hc_wave_kinematics and every side term read (hc_wave_kin.hip: kin_table_host), so all of them
// run under a record through the kernels they have.  The excitation path is not touched: the record still drives the convolution
// with its zero extension.  DESIGN.md 3.7q; the host parts are hc_eta_components.hpp.
#include "hc_eta_components.hpp"

#include <climits>

#include "hc_internal.hpp"

using namespace hc::detail;

namespace hc {
namespace {

constexpr int kDftThreads = 256;

struct EtaDftArgs {
    const double* eta;  // [n] the samples on the uniform grid
    int n;
    int m0, nb;   // the candidate bins m0 .. m0 + nb - 1, one workgroup each
    double* out;  // [2][nb]: real parts, then imaginary parts, of c_m = (2 / n) sum_j eta_j exp(+i 2 pi ((m j) mod n) / n)
};

// One workgroup per bin.  Work item s sums j = s, s + 256, ... in ascending order; the 256 partial sums are combined by an LDS tree
// in a fixed order, so a bin's bits depend on the record and on m only -- not on the band, the number of bins or the shard.  The
// angle is 2 pi r / n with r = (m j) mod n kept exactly in 64-bit integers; sincospi takes 2 r / n, one rounding, and needs no
// argument reduction beyond its own exact one.
__global__ void __launch_bounds__(kDftThreads) eta_dft_kernel(EtaDftArgs a) {
    __shared__ double sre[kDftThreads], sim[kDftThreads];
    const int s                  = threadIdx.x;
    const unsigned long long n   = static_cast<unsigned long long>(a.n);
    const unsigned long long m   = static_cast<unsigned long long>(a.m0) + blockIdx.x;
    const unsigned long long inc = eta_phase_start(m, kDftThreads, n);  // (m * 256) mod n
    unsigned long long r         = eta_phase_start(m, static_cast<unsigned long long>(s), n);
    double re = 0.0, im = 0.0;
    for (long long j = s; j < a.n; j += kDftThreads) {
        double sn, cs;
        sincospi(2.0 * static_cast<double>(r) / static_cast<double>(a.n), &sn, &cs);
        const double e = a.eta[j];
        re += e * cs;
        im += e * sn;
        r = eta_phase_next(r, inc, n);
    }
    sre[s] = re;
    sim[s] = im;
    __syncthreads();
    for (int w = kDftThreads / 2; w > 0; w >>= 1) {
        if (s < w) {
            sre[s] += sre[s + w];
            sim[s] += sim[s + w];
        }
        __syncthreads();
    }
    if (s == 0) {
        const double scale   = (2 * m == n ? 1.0 : 2.0) / static_cast<double>(a.n);  // the Nyquist bin of an even n is halved
        a.out[blockIdx.x]        = sre[0] * scale;
        a.out[a.nb + blockIdx.x] = sim[0] * scale;
    }
}

struct EtaResidualArgs {
    const double* eta;  // [n]
    int n;
    double mean;
    const int* m;     // [K] bins of the kept components
    const double* c;  // [2][K] their coefficients against sample 0 (before the turn to the absolute origin)
    int K;
    double* out;  // [n] eta_j - mean - sum_m (re_m cos th + im_m sin th), th = 2 pi ((m j) mod n) / n
};

// One work item per sample; the kept components are staged in LDS tiles and summed in index order
__global__ void __launch_bounds__(kDftThreads) eta_residual_kernel(EtaResidualArgs a) {
    __shared__ double sre[kDftThreads], sim[kDftThreads];
    __shared__ int sm[kDftThreads];
    const long long j  = static_cast<long long>(blockIdx.x) * kDftThreads + threadIdx.x;
    const bool active  = j < a.n;
    const unsigned long long jc = active ? static_cast<unsigned long long>(j) : 0ULL;
    const unsigned long long n  = static_cast<unsigned long long>(a.n);
    double sum = 0.0;
    for (int i0 = 0; i0 < a.K; i0 += kDftThreads) {
        const int cnt = min(kDftThreads, a.K - i0);
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < cnt) {
            sm[threadIdx.x]  = a.m[i0 + threadIdx.x];
            sre[threadIdx.x] = a.c[i0 + threadIdx.x];
            sim[threadIdx.x] = a.c[a.K + i0 + threadIdx.x];
        }
        __syncthreads();
        for (int i = 0; i < cnt; ++i) {
            const unsigned long long r = eta_phase_start(static_cast<unsigned long long>(sm[i]), jc, n);
            double sn, cs;
            sincospi(2.0 * static_cast<double>(r) / static_cast<double>(a.n), &sn, &cs);
            sum += sre[i] * cs + sim[i] * sn;
        }
    }
    if (active) a.out[j] = a.eta[j] - a.mean - sum;
}

}  // namespace
}  // namespace hc

extern "C" {

int hc_set_eta_record_components(hc_ctx* c, double f_min_hz, double f_max_hz, int max_components) {
    HC_API_BEGIN(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    require(c->wave_kind == hc::kWaveIrregular && c->eta_record, HC_ERR_INVALID,
            "the wave model in force is not an imported eta record (hc_set_wave_irregular_eta)");
    require(std::isfinite(f_min_hz) && std::isfinite(f_max_hz), HC_ERR_INVALID, "non-finite band edge");
    const long long n = static_cast<long long>(c->rec_t.size());
    require(n >= 4, HC_ERR_INVALID, "the component analysis needs a record of at least four samples");
    require(n <= INT_MAX, HC_ERR_INVALID, "record too long");
    const double* t  = c->rec_t.data();
    const double h   = hc::eta_mean_spacing(t, n);
    const double T_w = static_cast<double>(n) * h;
    long long m_lo = 0, m_hi = -1;
    hc::eta_band_bins(n, T_w, f_min_hz, f_max_hz, &m_lo, &m_hi);
    require(m_lo <= m_hi, HC_ERR_INVALID, "no bin of the record's Fourier grid (m / T_w, 1 <= m <= n / 2) lies inside [f_min, f_max]");
    const int nb = static_cast<int>(m_hi - m_lo + 1);

    // ---- the samples on the uniform grid, their mean and variance ----
    std::vector<double> resampled;
    if (!hc::eta_grid_uniform(t, n, h)) resampled = hc::eta_resample_uniform(t, c->rec_eta.data(), n, h);
    const std::vector<double>& eta = resampled.empty() ? c->rec_eta : resampled;
    long double acc = 0.0L;
    for (double v : eta) acc += v;
    const double mean = static_cast<double>(acc / static_cast<long double>(n));
    acc = 0.0L;
    for (double v : eta) acc += (static_cast<long double>(v) - mean) * (static_cast<long double>(v) - mean);
    const double var = static_cast<double>(acc / static_cast<long double>(n));

    // ---- the coefficients of every candidate bin: one upload, one launch, one copy back ----
    hc::DeviceBuffer<double> d_eta, d_out;
    d_eta.upload(eta, c->stream);
    d_out.alloc(2 * static_cast<size_t>(nb));
    hc::EtaDftArgs a{};
    a.eta = d_eta.p;
    a.n   = static_cast<int>(n);
    a.m0  = static_cast<int>(m_lo);
    a.nb  = nb;
    a.out = d_out.p;
    hipLaunchKernelGGL(hc::eta_dft_kernel, dim3(static_cast<unsigned>(nb)), dim3(hc::kDftThreads), 0, c->stream, a);
    HC_HIP(hipGetLastError());
    std::vector<double> raw(2 * static_cast<size_t>(nb));
    HC_HIP(hipMemcpyAsync(raw.data(), d_out.p, raw.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));

    // ---- to the absolute time origin, amplitude and phase (eta(0, t) = sum A cos(phi - w t), as kin_table_host and eta_kernel) ----
    std::vector<double> amp(nb), phase(nb);
    for (int b = 0; b < nb; ++b) {
        double re, im;
        hc::eta_rotate_origin(raw[b], raw[static_cast<size_t>(nb) + b], m_lo + b, T_w, t[0], &re, &im);
        amp[b]   = std::hypot(re, im);
        phase[b] = std::atan2(im, re);
    }
    const std::vector<long long> keep = hc::eta_select_components(amp.data(), nb, max_components);
    const int K = static_cast<int>(keep.size());
    std::vector<int> rm(K);
    std::vector<double> rf(K), rS(K), rdf(K, 1.0 / T_w), rA(K), rph(K), rk(K), coef(2 * static_cast<size_t>(K));
    double energy = 0.0;
    for (int i = 0; i < K; ++i) {
        const long long b = keep[i];
        rm[i]  = static_cast<int>(m_lo + b);
        rf[i]  = hc::eta_bin_frequency(m_lo + b, T_w);
        rA[i]  = amp[b];
        rph[i] = phase[b];
        rS[i]  = rA[i] * rA[i] / (2.0 * rdf[i]);  // the one-sided periodogram (hc_get_spectrum); the table takes rec_amp itself
        rk[i]  = hc::wave_number(2 * M_PI * rf[i], c->depth, c->g);
        coef[i]                         = raw[b];
        coef[static_cast<size_t>(K) + i] = raw[static_cast<size_t>(nb) + b];
        energy += 0.5 * rA[i] * rA[i];
    }

    // ---- what the kept components leave of the record, at the sample times ----
    hc::DeviceBuffer<int> d_m;
    hc::DeviceBuffer<double> d_c, d_res;
    d_m.upload(rm, c->stream);
    d_c.upload(coef, c->stream);
    d_res.alloc(static_cast<size_t>(n));
    hc::EtaResidualArgs ra{};
    ra.eta  = d_eta.p;
    ra.n    = static_cast<int>(n);
    ra.mean = mean;
    ra.m    = d_m.p;
    ra.c    = d_c.p;
    ra.K    = K;
    ra.out  = d_res.p;
    const unsigned blocks = static_cast<unsigned>((n + hc::kDftThreads - 1) / hc::kDftThreads);
    hipLaunchKernelGGL(hc::eta_residual_kernel, dim3(blocks), dim3(hc::kDftThreads), 0, c->stream, ra);
    HC_HIP(hipGetLastError());
    std::vector<double> res(static_cast<size_t>(n));
    HC_HIP(hipMemcpyAsync(res.data(), d_res.p, res.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HC_HIP(hipStreamSynchronize(c->stream));
    acc = 0.0L;
    for (double v : res) acc += static_cast<long double>(v) * v;
    const double rms = std::sqrt(static_cast<double>(acc / static_cast<long double>(n)));

    // ---- into the context: a wave-model change for every cached component table; no step state is touched ----
    HC_HIP(hipDeviceSynchronize());  // a side lane may still read the table this replaces
    c->wave_dir.clear();             // as every hc_set_wave_* call: the component count is another
    c->spec_f.swap(rf);
    c->spec_S.swap(rS);
    c->spec_df.swap(rdf);
    c->spec_phase.swap(rph);
    c->spec_k.swap(rk);
    c->rec_m.swap(rm);
    c->rec_amp.swap(rA);
    c->rec_mean  = mean;
    c->rec_share = var > 0.0 ? energy / var : 0.0;
    c->rec_rms   = rms;
    ++c->wave_serial;
    HC_API_END(c)
}

int hc_clear_eta_record_components(hc_ctx* c) {
    HC_API_BEGIN(c)
    require(c->wave_kind == hc::kWaveIrregular && c->eta_record, HC_ERR_INVALID,
            "the wave model in force is not an imported eta record (hc_set_wave_irregular_eta)");
    if (!c->record_components()) return HC_OK;  // nothing set, nothing to clear: no table is touched
    HC_HIP(hipDeviceSynchronize());
    c->wave_dir.clear();
    for (auto* v : {&c->spec_f, &c->spec_S, &c->spec_df, &c->spec_phase, &c->spec_k}) v->clear();
    c->drop_record_components();
    ++c->wave_serial;
    HC_API_END(c)
}

int hc_get_eta_record_components(hc_ctx* c, int* n, int* m, double* f, double* amplitude, double* phase, double* k, double* mean,
                                 double* variance_share, double* rms_residual) {
    HC_API_BEGIN_HOT(c)
    require(c->wave_kind == hc::kWaveIrregular && c->eta_record, HC_ERR_INVALID,
            "the wave model in force is not an imported eta record (hc_set_wave_irregular_eta)");
    const bool on = c->record_components();
    if (n) *n = on ? static_cast<int>(c->rec_amp.size()) : 0;
    if (mean) *mean = c->rec_mean;
    if (variance_share) *variance_share = c->rec_share;
    if (rms_residual) *rms_residual = c->rec_rms;
    if (!on) return HC_OK;
    if (m) std::copy(c->rec_m.begin(), c->rec_m.end(), m);
    if (f) std::copy(c->spec_f.begin(), c->spec_f.end(), f);
    if (amplitude) std::copy(c->rec_amp.begin(), c->rec_amp.end(), amplitude);
    if (phase) std::copy(c->spec_phase.begin(), c->spec_phase.end(), phase);
    if (k) std::copy(c->spec_k.begin(), c->spec_k.end(), k);
    HC_API_END(c)
}

}  // extern "C"
