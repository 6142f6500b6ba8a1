// hc_directions.cpp -- directions of the wave components (include/hydrochrono_amd.h: hc_set_wave_directions) and the first-order
// excitation under a heading (hc_set_excitation_rao_headings).  Not in the reference, which parses waves.direction and ignores it
// (src/wave_types.cpp:20,34).  Host code only: the directions are state that the component tables of the side terms pick up
// (hc_wave_kin.hip: kin_dir_columns_host), and the excitation follows by rebuilding the per-row x per-component (magnitude, phase)
// tables the step kernels already read -- no kernel of the step path changes.  DESIGN.md 3.7k.
#include "hc_heading.hpp"
#include "hc_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

using namespace hc::detail;

namespace hc {
namespace detail {
namespace {

bool uniform(const std::vector<double>& theta) {
    for (double v : theta)
        if (std::memcmp(&v, &theta[0], sizeof(double)) != 0) return false;
    return true;
}

const char* const kOutsideExcitationGrid =
    "a wave direction lies outside the heading grid of a body's excitation tables (no extrapolation, no wrap-around)";

// (magnitude, phase) of row r of a body at (omega bracket, heading bracket): the omega interpolation at the two headings, then
// linear in the heading on the values as given
void heading_value(const BodyHost& bd, int r, const RaoBracket& br, const HeadBracket& hb, double* mag, double* phase) {
    const size_t nw = bd.hd_w.size(), nd = bd.hd_dir.size();
    const auto at   = [&](const std::vector<double>& v, int j) {
        const double* row = v.data() + (static_cast<size_t>(r) * nd + j) * nw;
        const double v0 = row[br.k0], v1 = row[br.k1];
        return (br.fr * (v1 - v0)) + v0;
    };
    const double m0 = at(bd.hd_mag, hb.j0), m1 = at(bd.hd_mag, hb.j1);
    const double p0 = at(bd.hd_phase, hb.j0), p1 = at(bd.hd_phase, hb.j1);
    *mag   = (hb.wt * (m1 - m0)) + m0;
    *phase = (hb.wt * (p1 - p0)) + p0;
}

}  // namespace

void apply_wave_directions(hc_ctx* c, const std::vector<double>& theta, bool commit, bool force) {
    const bool set = !theta.empty(), uni = uniform(theta);
    if (c->wave_kind == kWaveSpectral) {
        bool any = false;
        for (int b = c->b0; b < c->b1; ++b) any = any || !c->bodies[b].hd_dir.empty();
        if (set && !uni)
            for (int b = c->b0; b < c->b1; ++b)
                require(!c->bodies[b].hd_dir.empty(), HC_ERR_INVALID,
                        "non-uniform wave directions need excitation tables on a heading grid for every local body "
                        "(hc_set_excitation_rao_headings)");
        if (!any && !force) return;  // every local body keeps its {6,1,nw} table: what the device holds
        const int nf = static_cast<int>(c->spec_f.size());
        const double two_pi = 2 * M_PI;
        std::vector<double> mag(static_cast<size_t>(c->Dloc) * nf), ph(static_cast<size_t>(c->Dloc) * nf);
        for (int bl = 0; bl < c->nloc; ++bl) {
            const BodyHost& bd = c->bodies[c->b0 + bl];
            const bool heads   = set && !bd.hd_dir.empty();
            const int nw       = static_cast<int>(heads ? bd.hd_w.size() : bd.rao_w.size());
            for (int i = 0; i < nf; ++i) {
                const RaoBracket br = rao_bracket_clamped(two_pi * c->spec_f[i], heads ? bd.hd_w.back() : bd.rao_w.back(), nw);
                for (int r = 0; r < 6; ++r) {
                    double m, p;
                    if (heads) {
                        heading_value(bd, r, br, heading_bracket(bd.hd_dir, theta[i], kOutsideExcitationGrid), &m, &p);
                    } else {  // the expression of hc_set_wave_irregular_spectral
                        const double m0 = bd.rao_mag[static_cast<size_t>(r) * nw + br.k0], m1 = bd.rao_mag[static_cast<size_t>(r) * nw + br.k1];
                        const double p0 = bd.rao_phase[static_cast<size_t>(r) * nw + br.k0], p1 = bd.rao_phase[static_cast<size_t>(r) * nw + br.k1];
                        m = (br.fr * (m1 - m0)) + m0;
                        p = (br.fr * (p1 - p0)) + p0;
                    }
                    mag[static_cast<size_t>(6 * bl + r) * nf + i] = m;
                    ph[static_cast<size_t>(6 * bl + r) * nf + i]  = p;
                }
            }
        }
        if (!commit) return;
        // as hc_set_wave_irregular_spectral before it replaces its tables: rows a look-ahead pass has precomputed belong to the old
        // tables, and steps on a caller's stream may still read them
        drop_lookahead_excitation(c);
        HC_HIP(hipDeviceSynchronize());
        c->d_spec_mag.upload(mag, c->stream);
        c->d_spec_phase.upload(ph, c->stream);
        HC_HIP(hipStreamSynchronize(c->stream));
    } else if (c->wave_kind == kWaveRegular) {
        bool any = false;
        for (int b = 0; b < c->wave_nb_arg; ++b) any = any || !c->bodies[b].hd_dir.empty();
        if (!any && !force) return;
        std::vector<double> mag = c->reg_mag, ph = c->reg_phase;
        for (int b = 0; b < c->wave_nb_arg; ++b) {
            const BodyHost& bd = c->bodies[b];
            const bool heads   = set && !bd.hd_dir.empty();
            const int nw       = static_cast<int>(heads ? bd.hd_w.size() : bd.rao_w.size());
            // a body's heading tables on their own frequency list; without them body 0's list serves, as in hc_set_wave_regular
            const auto& w0      = c->bodies[0].rao_w;
            const RaoBracket br = heads ? rao_bracket_regular(c->reg_omega, bd.hd_w.back(), nw)
                                        : rao_bracket_regular(c->reg_omega, w0.back(), static_cast<int>(w0.size()));
            rao_bracket_check(br, nw);
            for (int r = 0; r < 6; ++r) {
                double m, p;
                if (heads) {
                    heading_value(bd, r, br, heading_bracket(bd.hd_dir, theta[0], kOutsideExcitationGrid), &m, &p);
                } else {  // the expression of hc_set_wave_regular
                    const double m0 = bd.rao_mag[static_cast<size_t>(r) * nw + br.k0], m1 = bd.rao_mag[static_cast<size_t>(r) * nw + br.k1];
                    const double p0 = bd.rao_phase[static_cast<size_t>(r) * nw + br.k0], p1 = bd.rao_phase[static_cast<size_t>(r) * nw + br.k1];
                    m = (br.fr * (m1 - m0)) + m0;
                    p = (br.fr * (p1 - p0)) + p0;
                }
                mag[6 * b + r] = m;
                ph[6 * b + r]  = p;
            }
        }
        if (!commit) return;
        drop_lookahead_excitation(c);
        HC_HIP(hipDeviceSynchronize());
        c->reg_mag   = mag;
        c->reg_phase = ph;
        std::vector<double> local(mag.begin() + 6 * c->b0, mag.begin() + 6 * c->b1);
        c->d_reg_mag.upload(local, c->stream);
        HC_HIP(hipStreamSynchronize(c->stream));
    }
    // the IRF model: one convolution of eta(0, t) with the caller's IRF, which is understood to be the one of the (uniform) heading
}

}  // namespace detail
}  // namespace hc

extern "C" {

int hc_set_wave_directions(hc_ctx* c, int n, const double* theta) {
    HC_API_BEGIN(c)
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    require(n >= 0, HC_ERR_INVALID, "negative direction count");
    std::vector<double> th;
    if (n > 0 && theta) th.assign(theta, theta + n);
    if (!th.empty()) {
        const bool components = c->wave_kind == hc::kWaveRegular || c->wave_kind == hc::kWaveSpectral ||
                                (c->wave_kind == hc::kWaveIrregular && !c->eta_record) || c->record_components();
        require(components, HC_ERR_INVALID,
                "the wave model in force has no components to give directions to (NoWave, no model or an imported eta record without "
                "components: hc_set_eta_record_components)");
        const int nf = c->wave_kind == hc::kWaveRegular ? 1 : static_cast<int>(c->spec_f.size());
        require(n == nf, HC_ERR_INVALID, "the direction count is not the component count of the wave model (1 for a regular wave, else nf)");
        for (double v : th) require(std::isfinite(v), HC_ERR_INVALID, "non-finite wave direction");
        require(c->wave_kind != hc::kWaveIrregular || uniform(th), HC_ERR_UNSUPPORTED,
                "non-uniform wave directions on the IRF model of hc_set_wave_irregular: its excitation is one convolution of eta(0, t), "
                "which a spread sea does not have -- use hc_set_wave_irregular_spectral");
    } else if (c->wave_dir.empty()) {
        return HC_OK;  // nothing set, nothing to clear: no table is touched
    }
    apply_wave_directions(c, th, false, false);  // every error before any state changes
    apply_wave_directions(c, th, true, false);
    c->wave_dir.swap(th);
    ++c->wave_serial;  // the component tables of the side terms are rebuilt with (or without) the direction columns
    HC_API_END(c)
}

int hc_get_wave_directions(hc_ctx* c, int* n, double* theta) {
    HC_API_BEGIN_HOT(c)
    if (n) *n = static_cast<int>(c->wave_dir.size());
    if (theta) std::copy(c->wave_dir.begin(), c->wave_dir.end(), theta);
    HC_API_END(c)
}

int hc_set_excitation_rao_headings(hc_ctx* c, int body, int n_dir, const double* dir, const double* w, int nw, const double* mag,
                                   const double* phase) {
    HC_API_BEGIN(c)
    check_body(c, body);
    require(n_dir >= 0, HC_ERR_INVALID, "negative heading count");
    require(c->have_sim, HC_ERR_INVALID, "set simulation parameters first (rho*g scales the excitation magnitude)");
    hc::BodyHost& b = c->bodies[body];
    hc::BodyHost keep;
    keep.hd_dir.swap(b.hd_dir), keep.hd_w.swap(b.hd_w), keep.hd_mag.swap(b.hd_mag), keep.hd_phase.swap(b.hd_phase);
    const auto restore = [&] { keep.hd_dir.swap(b.hd_dir), keep.hd_w.swap(b.hd_w), keep.hd_mag.swap(b.hd_mag), keep.hd_phase.swap(b.hd_phase); };
    try {
        if (n_dir > 0) {
            require(dir && w && mag && phase && nw > 0, HC_ERR_INVALID, "null pointer or empty heading tables");
            const size_t len = static_cast<size_t>(6) * n_dir * nw;
            for (int j = 0; j < n_dir; ++j) require(std::isfinite(dir[j]), HC_ERR_INVALID, "non-finite heading");
            for (int j = 1; j < n_dir; ++j) require(dir[j] > dir[j - 1], HC_ERR_INVALID, "the heading grid must be strictly increasing");
            for (int k = 0; k < nw; ++k) require(std::isfinite(w[k]), HC_ERR_INVALID, "non-finite frequency");
            for (size_t i = 0; i < len; ++i) require(std::isfinite(mag[i]) && std::isfinite(phase[i]), HC_ERR_INVALID, "non-finite excitation coefficient");
            b.hd_dir.assign(dir, dir + n_dir);
            b.hd_w.assign(w, w + nw);
            b.hd_mag.assign(mag, mag + len);
            const double rg = c->rho * c->g;
            for (auto& x : b.hd_mag) x = x * rg;  // as hc_set_excitation_rao
            b.hd_phase.assign(phase, phase + len);
        }
        if (c->finalized && !c->wave_dir.empty()) {  // directions in force: the tables follow at once
            apply_wave_directions(c, c->wave_dir, false, true);  // (a body that has just lost its tables goes back to {6,1,nw})
            apply_wave_directions(c, c->wave_dir, true, true);
        }
    } catch (...) {
        restore();
        throw;
    }
    HC_API_END(c)
}

int hc_get_excitation_rao_headings_size(hc_ctx* c, int body, int* n_dir, int* nw) {
    HC_API_BEGIN_HOT(c)
    check_body(c, body);
    if (n_dir) *n_dir = static_cast<int>(c->bodies[body].hd_dir.size());
    if (nw) *nw = static_cast<int>(c->bodies[body].hd_w.size());
    HC_API_END(c)
}

// needs no context: pure host math (hc_host_math.cpp)
int hc_wave_spreading_directions(int nf, double heading_rad, double s, int n_bins, unsigned long long seed, double* theta_out) {
    if (nf < 0 || (nf > 0 && !theta_out)) return HC_ERR_INVALID;
    try {
        const std::vector<double> th = hc::spreading_directions(nf, heading_rad, s, n_bins, seed);
        std::copy(th.begin(), th.end(), theta_out);
    } catch (const std::invalid_argument&) {
        return HC_ERR_INVALID;
    } catch (...) {
        return HC_ERR_RUNTIME;
    }
    return HC_OK;
}

}  // extern "C"
