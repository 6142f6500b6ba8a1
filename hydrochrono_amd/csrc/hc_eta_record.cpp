// hc_eta_record.cpp -- irregular waves from an imported free-surface elevation record: the reference's eta file reader
// (IrregularWaves::ReadEtaFromFile, src/wave_types.cpp:480-500) and the wave model built on a record.  The reference reads the
// record into time_data_ but convolves against free_surface_time_sampled_, which stays empty on that branch; here the
// record is the free-surface table, extended by zeros (hc_eta_record.hpp), and the per-step path is the one of hc_set_wave_irregular.
#include "hc_eta_record.hpp"

#include <climits>

#include "hc_internal.hpp"

using namespace hc::detail;

namespace {
double seconds_since(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

extern "C" {

int hc_read_eta_file(const char* path, double* t, double* eta, int capacity, int* n) {
    try {
        require(path && n, HC_ERR_INVALID, "null path or count");
        std::vector<double> tv, ev;
        const std::string msg = hc::read_eta_file(path, tv, ev);
        if (!msg.empty()) throw Error(HC_ERR_RUNTIME, msg);  // the reference throws std::runtime_error
        require(tv.size() <= static_cast<size_t>(INT_MAX), HC_ERR_INVALID, "eta file has more lines than an int counts");
        const int count = static_cast<int>(tv.size());
        *n              = count;
        if (!t && !eta) return HC_OK;  // size query
        require(t && eta, HC_ERR_INVALID, "null time or elevation array");
        if (capacity < count)
            throw Error(HC_ERR_OUT_OF_RANGE, "eta file holds " + std::to_string(count) + " samples, capacity is " + std::to_string(capacity));
        std::copy(tv.begin(), tv.end(), t);
        std::copy(ev.begin(), ev.end(), eta);
        return HC_OK;
    } catch (const Error& e) {
        g_create_error = e.what();
        return e.status;
    } catch (const std::exception& e) {
        g_create_error = e.what();
        return HC_ERR_RUNTIME;
    }
}

int hc_set_wave_irregular_eta(hc_ctx* c, const hc_irregular_wave_params* pp, const double* t, const double* eta, int n) {
    HC_API_BEGIN(c)
    drop_lookahead_excitation(c);
    ++c->wave_serial;
    HC_HIP(hipDeviceSynchronize());  // the tables replaced below may be in use by steps on a caller's stream
    require(c->finalized, HC_ERR_INVALID, "hc_finalize has not been called");
    require(pp, HC_ERR_INVALID, "null parameters");
    const hc_irregular_wave_params p = *pp;
    require(p.num_bodies == c->N, HC_ERR_INVALID, "IrregularWaveParams.num_bodies_ must equal the number of hydro bodies");
    require(p.simulation_dt > 0.0, HC_ERR_INVALID, "simulation_dt must be positive");
    const std::string bad = hc::validate_eta_record(t, eta, n);
    require(bad.empty(), HC_ERR_INVALID, bad.c_str());
    const auto t_call = std::chrono::steady_clock::now();
    // the excitation IRF on the simulation_dt grid, as for a synthesised table (InitializeIRFVectors, src/wave_types.cpp:447-449)
    ExcitationGrid ex = resample_excitation(c, p.simulation_dt);
    hc::EtaExtended x = hc::extend_eta_record(t, eta, n, ex.tau_min, ex.tau_max);
    require(x.t.size() <= static_cast<size_t>(INT_MAX / 2), HC_ERR_INVALID, "eta record too long once extended over the excitation IRF");
    for (size_t i = 1; i < x.t.size(); ++i)
        require(x.t[i] > x.t[i - 1], HC_ERR_INVALID, "eta record spacing too fine for its time values (zero extension not increasing)");
    const int nt = static_cast<int>(x.t.size());
    const auto t_up = std::chrono::steady_clock::now();
    c->d_eta_t.upload(x.t, c->stream);
    c->d_eta.upload(x.eta, c->stream);
    upload_excitation(c, ex);
    c->init.wave_upload_seconds += seconds_since(t_up);
    c->init.wave_upload_bytes += 8.0 * (2.0 * nt + 2.0 * static_cast<double>(c->Dloc) * ex.L + 2.0 * ex.L);
    c->wave_dir.clear();  // the new model is in force from here: its component count is another (hc_set_wave_directions)
    c->irr = p;
    c->nf  = 0;
    c->nt  = nt;
    for (auto* v : {&c->spec_f, &c->spec_S, &c->spec_df, &c->spec_phase, &c->spec_k}) v->clear();
    c->eta_t.swap(x.t);
    c->eta.swap(x.eta);
    c->rec_t.assign(t, t + n);
    c->rec_eta.assign(eta, eta + n);
    c->eta_h      = x.h;
    c->eta_record = true;
    c->drop_record_components();  // a new record has none until hc_set_eta_record_components is called for it
    commit_excitation(c, ex);
    c->wave_nb_arg = p.num_bodies;
    HC_HIP(hipStreamSynchronize(c->stream));
    c->init.wave_total_seconds += seconds_since(t_call);
    HC_API_END(c)
}

}  // extern "C"
