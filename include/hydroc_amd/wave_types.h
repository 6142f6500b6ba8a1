// hydroc_amd/wave_types.h -- the reference's wave classes (include/hydroc/wave_types.h:40-467) as configuration holders over the
// C ABI: same class names, constructors, public members and getters; the arithmetic (AddH5Data + Initialize, GetForceAtTime) runs
// behind hc_set_wave_* / hc_compute_waves on the GPU.  Header-only; link with libhydrochrono_amd.so.
//
// A reference program changes `#include <hydroc/wave_types.h>` to `#include <hydroc_amd/wave_types.h>` and adds
// `using namespace hydroc_amd;` -- the wave set-up lines stay as they are (demos/sphere/demo_sphere_reg_waves.cpp:126-128,
// tests/regression/sphere/irreg_waves/sphere_irreg_waves_test.cpp:113-122).
//
// Wave kinematics (GetElevation / GetVelocity / GetAcceleration, include/hydroc/wave_types.h:69-73) run on the GPU through
// hc_wave_kinematics for all three classes.  Differences: positions are std::array<double, 3> or any type with
// .x() .y() .z() (Eigen::Vector3d, ChVector3d); GetVelocity / GetAcceleration return std::array<double, 3>; GetKinematics evaluates
// a grid of points x a series of times in one call; a model that is not attached throws std::runtime_error.  Attach copies g_ and
// water_depth_ from the hydro data as the reference's AddH5Data does; the kinematics use the context's values, so writing these
// members afterwards has no effect.  eta_file_path_ reads the record with hc_read_eta_file and attaches it with
// hc_set_wave_irregular_eta, whose defined behaviour replaces the reference's undefined one (src/wave_types.cpp:480-500 vs :784-785;
// DESIGN.md section 3): the record is zero-extended, there is no spectrum (GetSpectrum throws the reference's message), and the
// kinematics are zeros -- unless components are set (IrregularWaves::SetRecordComponents).  The mesh helper the irregular demos call (SetUpWaveMesh / GetMeshFile / GetWaveMeshVelocity) is there so that they
// compile.  GetSecondOrderElevation / GetSecondOrderVelocity / GetSecondOrderAcceleration and the batched GetSecondOrderKinematics
// (hc_wave_kinematics2) give the second-order increments of an irregular sea; they have no counterpart in the reference.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../hydrochrono_amd.h"
#include "../hydrochrono_amd_host.h"

namespace hydroc_amd {

// C status codes become the exception types the reference throws (std::runtime_error / std::out_of_range).
inline void check(hc_ctx* ctx, int rc) {
    if (rc == HC_OK) return;
    const std::string msg = hc_last_error(ctx);
    if (rc == HC_ERR_OUT_OF_RANGE) throw std::out_of_range(msg);
    throw std::runtime_error(msg);
}

enum class WaveMode { noWaveCIC = 0, regular = 1, irregular = 2 };  // include/hydroc/wave_types.h:40-47

// The two spectrum helpers the reference's header exports (include/hydroc/wave_types.h:14-20, src/wave_types.cpp:679-715), on the host
// routine the library itself uses for IrregularWaves (Eigen::VectorXd becomes std::vector<double>): spectral density in m^2/Hz at the
// frequencies f (Hz), which are sorted in place first, as the reference does (:681).
inline std::vector<double> JONSWAPSpectrumHz(std::vector<double>& f, double Hs, double Tp, double gamma = 3.3, bool is_normalized = false) {
    std::sort(f.begin(), f.end());
    std::vector<double> S(f.size());
    hc_host_jonswap_spectrum_hz(f.data(), static_cast<int>(f.size()), Hs, Tp, gamma, is_normalized ? 1 : 0, S.data());
    return S;
}
inline std::vector<double> PiersonMoskowitzSpectrumHz(std::vector<double>& f, double Hs, double Tp) { return JONSWAPSpectrumHz(f, Hs, Tp, 1.0, false); }

class WaveBase {  // :52-79
  public:
    virtual ~WaveBase()            = default;
    virtual void Initialize() {}   // the library initialises the model when it is attached
    virtual WaveMode GetWaveMode() = 0;
    // AddH5Data + Initialize of the reference, executed by the library for one (shard) context; TestHydro::AddWaves calls it
    virtual void Attach(hc_ctx* ctx) = 0;
    // 6 * num_bodies forces of the model at time t (GetForceAtTime of the reference returns an Eigen::VectorXd)
    std::vector<double> GetForceAtTime(double t) {
        if (!ctx_) throw std::runtime_error("wave model is not attached to a TestHydro");
        int N = 0, n_local = 0;
        check(ctx_, hc_get_sizes(ctx_, &N, &n_local, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        if (n_local != N) throw std::runtime_error("GetForceAtTime: ask the TestHydro of a sharded system (ComputeForceWaves)");
        std::vector<double> f(static_cast<size_t>(6) * N);
        check(ctx_, hc_compute_waves(ctx_, t, f.data()));
        return f;
    }
    // Wave kinematics of the attached model (src/wave_types.cpp:14-158,301-313,515-550; NoWave: zeros).  Non-virtual: a subclass
    // supplies its options through KinematicsOptions(), so the overloads for Eigen / Chrono vectors below stay visible.
    double GetElevation(const std::array<double, 3>& position, double time) {
        double eta = 0.0;
        kinematics(1, position.data(), 1, &time, &eta, nullptr, nullptr);
        return eta;
    }
    std::array<double, 3> GetVelocity(const std::array<double, 3>& position, double time) {
        std::array<double, 3> v{};
        kinematics(1, position.data(), 1, &time, nullptr, v.data(), nullptr);
        return v;
    }
    std::array<double, 3> GetAcceleration(const std::array<double, 3>& position, double time) {
        std::array<double, 3> a{};
        kinematics(1, position.data(), 1, &time, nullptr, nullptr, a.data());
        return a;
    }
    // the same for any vector type with .x() .y() .z() (Eigen::Vector3d, chrono::ChVector3d)
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    double GetElevation(const V& position, double time) {
        return GetElevation(as_array(position), time);
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    std::array<double, 3> GetVelocity(const V& position, double time) {
        return GetVelocity(as_array(position), time);
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    std::array<double, 3> GetAcceleration(const V& position, double time) {
        return GetAcceleration(as_array(position), time);
    }
    // Batched: every point at every time in one GPU call.  eta [T][P], vel / acc [T][P][3] (row-major, T = times.size(),
    // P = points.size()); a null output is not computed.  Each value has the bits of the single-point call.
    void GetKinematics(const std::vector<std::array<double, 3>>& points, const std::vector<double>& times, std::vector<double>* eta,
                       std::vector<double>* vel = nullptr, std::vector<double>* acc = nullptr) {
        const size_t n = points.size() * times.size();
        if (eta) eta->assign(n, 0.0);
        if (vel) vel->assign(3 * n, 0.0);
        if (acc) acc->assign(3 * n, 0.0);
        kinematics(static_cast<int>(points.size()), points.empty() ? nullptr : points[0].data(), static_cast<int>(times.size()),
                   times.data(), eta ? eta->data() : nullptr, vel ? vel->data() : nullptr, acc ? acc->data() : nullptr);
    }
    // Second-order increments of the long-crested sea of Sharma and Dean (hc_wave_kinematics2; not in the reference): what a caller
    // adds to GetElevation / GetVelocity / GetAcceleration.  mwl_ and a regular wave's phase are those of the first-order calls,
    // the cut-offs and the ramp switch are second_order_; NoWave (and an imported eta record, unless components are set) give zeros.
    struct SecondOrderOptions {
        double diff_lo = 0.0, diff_hi = HUGE_VAL, sum_lo = 0.0, sum_hi = HUGE_VAL;  // rad/s
        bool apply_ramp = true;
    } second_order_;
    double GetSecondOrderElevation(const std::array<double, 3>& position, double time) {
        double eta = 0.0;
        kinematics2(1, position.data(), 1, &time, &eta, nullptr, nullptr);
        return eta;
    }
    std::array<double, 3> GetSecondOrderVelocity(const std::array<double, 3>& position, double time) {
        std::array<double, 3> v{};
        kinematics2(1, position.data(), 1, &time, nullptr, v.data(), nullptr);
        return v;
    }
    std::array<double, 3> GetSecondOrderAcceleration(const std::array<double, 3>& position, double time) {
        std::array<double, 3> a{};
        kinematics2(1, position.data(), 1, &time, nullptr, nullptr, a.data());
        return a;
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    double GetSecondOrderElevation(const V& position, double time) {
        return GetSecondOrderElevation(as_array(position), time);
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    std::array<double, 3> GetSecondOrderVelocity(const V& position, double time) {
        return GetSecondOrderVelocity(as_array(position), time);
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    std::array<double, 3> GetSecondOrderAcceleration(const V& position, double time) {
        return GetSecondOrderAcceleration(as_array(position), time);
    }
    // Batched, as GetKinematics: eta2 [T][P], vel2 / acc2 [T][P][3]; each value has the bits of the single-point call.
    void GetSecondOrderKinematics(const std::vector<std::array<double, 3>>& points, const std::vector<double>& times,
                                  std::vector<double>* eta2, std::vector<double>* vel2 = nullptr, std::vector<double>* acc2 = nullptr) {
        const size_t n = points.size() * times.size();
        if (eta2) eta2->assign(n, 0.0);
        if (vel2) vel2->assign(3 * n, 0.0);
        if (acc2) acc2->assign(3 * n, 0.0);
        kinematics2(static_cast<int>(points.size()), points.empty() ? nullptr : points[0].data(), static_cast<int>(times.size()),
                    times.data(), eta2 ? eta2->data() : nullptr, vel2 ? vel2->data() : nullptr, acc2 ? acc2->data() : nullptr);
    }
    // The same increments in the short-crested sea of SetDirections (hc_wave_kinematics2_dir; not in the reference): every pair of
    // components interacts at the angle between its two directions, and the velocities gain a y component.  With no directions
    // set it is the long-crested sea along +x, equal to the getters above to rounding.  Options: second_order_, mwl_, the phase.
    double GetDirectionalSecondOrderElevation(const std::array<double, 3>& position, double time) {
        double eta = 0.0;
        kinematics2(1, position.data(), 1, &time, &eta, nullptr, nullptr, true);
        return eta;
    }
    std::array<double, 3> GetDirectionalSecondOrderVelocity(const std::array<double, 3>& position, double time) {
        std::array<double, 3> v{};
        kinematics2(1, position.data(), 1, &time, nullptr, v.data(), nullptr, true);
        return v;
    }
    std::array<double, 3> GetDirectionalSecondOrderAcceleration(const std::array<double, 3>& position, double time) {
        std::array<double, 3> a{};
        kinematics2(1, position.data(), 1, &time, nullptr, nullptr, a.data(), true);
        return a;
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    double GetDirectionalSecondOrderElevation(const V& position, double time) {
        return GetDirectionalSecondOrderElevation(as_array(position), time);
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    std::array<double, 3> GetDirectionalSecondOrderVelocity(const V& position, double time) {
        return GetDirectionalSecondOrderVelocity(as_array(position), time);
    }
    template <class V, class = decltype(std::declval<const V&>().x() + std::declval<const V&>().z())>
    std::array<double, 3> GetDirectionalSecondOrderAcceleration(const V& position, double time) {
        return GetDirectionalSecondOrderAcceleration(as_array(position), time);
    }
    // Batched, as GetSecondOrderKinematics; each value has the bits of the single-point call.
    void GetDirectionalSecondOrderKinematics(const std::vector<std::array<double, 3>>& points, const std::vector<double>& times,
                                             std::vector<double>* eta2, std::vector<double>* vel2 = nullptr,
                                             std::vector<double>* acc2 = nullptr) {
        const size_t n = points.size() * times.size();
        if (eta2) eta2->assign(n, 0.0);
        if (vel2) vel2->assign(3 * n, 0.0);
        if (acc2) acc2->assign(3 * n, 0.0);
        kinematics2(static_cast<int>(points.size()), points.empty() ? nullptr : points[0].data(), static_cast<int>(times.size()),
                    times.data(), eta2 ? eta2->data() : nullptr, vel2 ? vel2->data() : nullptr, acc2 ? acc2->data() : nullptr, true);
    }
    // Wave heading and short-crested seas (hc_set_wave_directions; not in the reference, which ignores waves.direction): one
    // direction [rad, 0 along +x, positive towards +y] per component of the model -- 1 for a RegularWave, the number of spectrum
    // components for IrregularWaves (whose IRF model takes a uniform heading only).  The member is applied at the end of every Attach
    // (the library drops the directions with every new wave model); SetDirections also applies it to the context of the getters --
    // a sharded system sets them through TestHydro::SetWaveDirections, which reaches every shard.  GetElevation / GetVelocity / GetAcceleration, the Morison elements and the nonlinear surface forces then
    // sample the directional sea; the GetSecondOrder* getters throw while directions are set (GetDirectionalSecondOrder* answer).  Empty: the long-crested sea along +x.
    std::vector<double> wave_directions_;
    void SetDirections(const std::vector<double>& theta_rad) {
        if (ctx_)  // (an error leaves the member as it was)
            check(ctx_, hc_set_wave_directions(ctx_, static_cast<int>(theta_rad.size()), theta_rad.empty() ? nullptr : theta_rad.data()));
        wave_directions_ = theta_rad;
    }
    // the directions in force on the context of the getters (empty: none); not attached: the member
    std::vector<double> GetDirections() const {
        if (!ctx_) return wave_directions_;
        int n = 0;
        check(ctx_, hc_get_wave_directions(ctx_, &n, nullptr));
        std::vector<double> th(static_cast<size_t>(n));
        if (n) check(ctx_, hc_get_wave_directions(ctx_, &n, th.data()));
        return th;
    }
    // equal-energy directions of the cos-2s spreading about `heading_rad` for the attached model (hc_wave_spreading_directions),
    // for SetDirections / TestHydro::SetWaveDirections; s <= 0: the uniform heading.
    std::vector<double> SpreadingDirections(double heading_rad, double s = 0.0, int n_bins = 15, unsigned long long seed = 1) {
        if (!ctx_) throw std::runtime_error("wave model is not attached to a TestHydro");
        std::vector<double> th(static_cast<size_t>(ComponentCount()));
        if (hc_wave_spreading_directions(static_cast<int>(th.size()), heading_rad, s, n_bins, seed, th.data()) != HC_OK)
            throw std::runtime_error("SpreadingDirections: no bin, or a non-finite heading or exponent");
        return th;
    }
    double mwl_ = 0.0, g_ = 9.81, water_depth_ = 0.0;  // public members of the reference's base class (:74-78); unused by the force path

  protected:
    hc_ctx* ctx_ = nullptr;  // the first context the model was attached to (getters, kinematics)
    // what the model adds to the call's options (RegularWave: its phase, IrregularWaves: stretching); the base gives mwl_
    virtual hc_wave_kinematics_opts KinematicsOptions() const {
        hc_wave_kinematics_opts o;
        hc_wave_kinematics_opts_default(&o);
        o.mwl = mwl_;
        return o;
    }
    // end of every Attach: the context the getters use, and g_ / water_depth_ as the reference's AddH5Data sets them (:280-281,509-510)
    void attached(hc_ctx* ctx) {
        ctx_ = ctx;
        check(ctx, hc_get_simulation_parameters(ctx, nullptr, &g_, &water_depth_));
        if (!wave_directions_.empty()) check(ctx, hc_set_wave_directions(ctx, static_cast<int>(wave_directions_.size()), wave_directions_.data()));
    }
    // components of the attached model as the kinematics see them: the spectrum's; RegularWave 1, NoWave 0
    virtual int ComponentCount() const {
        int nf = 0;
        check(ctx_, hc_get_sizes(ctx_, nullptr, nullptr, nullptr, nullptr, &nf, nullptr, nullptr, nullptr));
        return nf;
    }

  private:
    template <class V>
    static std::array<double, 3> as_array(const V& p) {
        return {static_cast<double>(p.x()), static_cast<double>(p.y()), static_cast<double>(p.z())};
    }
    void kinematics(int n_points, const double* xyz, int n_times, const double* t, double* eta, double* vel, double* acc) {
        if (!ctx_) throw std::runtime_error("wave model is not attached to a TestHydro");
        const hc_wave_kinematics_opts o = KinematicsOptions();
        check(ctx_, hc_wave_kinematics(ctx_, &o, n_points, xyz, n_times, t, eta, vel, acc));
    }
    void kinematics2(int n_points, const double* xyz, int n_times, const double* t, double* eta, double* vel, double* acc,
                     bool directional = false) {
        if (!ctx_) throw std::runtime_error("wave model is not attached to a TestHydro");
        const hc_wave_kinematics_opts first = KinematicsOptions();
        hc_wave_kinematics2_opts o;
        hc_wave_kinematics2_opts_default(&o);
        o.mwl           = first.mwl;
        o.regular_phase = first.regular_phase;
        o.diff_lo       = second_order_.diff_lo;
        o.diff_hi       = second_order_.diff_hi;
        o.sum_lo        = second_order_.sum_lo;
        o.sum_hi        = second_order_.sum_hi;
        o.apply_ramp    = second_order_.apply_ramp ? 1 : 0;
        check(ctx_, directional ? hc_wave_kinematics2_dir(ctx_, &o, n_points, xyz, n_times, t, eta, vel, acc)
                                : hc_wave_kinematics2(ctx_, &o, n_points, xyz, n_times, t, eta, vel, acc));
    }
};

class NoWave : public WaveBase {  // :84-104
  public:
    NoWave() : num_bodies_(1) {}
    NoWave(unsigned int num_b) : num_bodies_(num_b) {}
    WaveMode GetWaveMode() override { return WaveMode::noWaveCIC; }
    void Attach(hc_ctx* ctx) override {
        check(ctx, hc_set_wave_none(ctx, static_cast<int>(num_bodies_)));
        attached(ctx);
    }

  protected:
    int ComponentCount() const override { return 0; }

  private:
    unsigned int num_bodies_;
};

class RegularWave : public WaveBase {  // :109-158
  public:
    RegularWave() : num_bodies_(1) {}
    RegularWave(unsigned int num_b) : num_bodies_(num_b) {}
    WaveMode GetWaveMode() override { return WaveMode::regular; }
    void Attach(hc_ctx* ctx) override {
        check(ctx, hc_set_wave_regular(ctx, static_cast<int>(num_bodies_), regular_wave_amplitude_, regular_wave_omega_));
        attached(ctx);
    }
    // user input variables
    double regular_wave_amplitude_ = 0.0;
    double regular_wave_omega_     = 0.0;
    double regular_wave_phase_     = 0.0;  // unused by the force, as in the reference (src/wave_types.cpp:315-327); the kinematics' phase

  protected:
    hc_wave_kinematics_opts KinematicsOptions() const override {
        hc_wave_kinematics_opts o = WaveBase::KinematicsOptions();
        o.regular_phase           = regular_wave_phase_;
        return o;
    }
    int ComponentCount() const override { return 1; }

  private:
    unsigned int num_bodies_;
};

struct IrregularWaveParams {  // :277-292
    unsigned int num_bodies_        = 1;
    double simulation_dt_           = 0.0;
    double simulation_duration_     = 0.0;
    double ramp_duration_           = 0.0;
    std::string eta_file_path_;     // a "time : eta" record (ReadEtaFromFile, src/wave_types.cpp:480-500); replaces the spectrum
    double wave_height_             = 0.0;
    double wave_period_             = 0.0;
    double frequency_min_           = 0.001;
    double frequency_max_           = 1.0;
    double nfrequencies_            = 0;
    double peak_enhancement_factor_ = 1.0;
    bool is_normalized_             = false;
    int seed_                       = 1;
    bool wave_stretching_           = true;  // Wheeler stretching of the kinematics (src/wave_types.cpp:515-544); not on the force path
};

class IrregularWaves : public WaveBase {  // :294-380
  public:
    IrregularWaves(const IrregularWaveParams& params) : params_(params) {}
    WaveMode GetWaveMode() override { return WaveMode::irregular; }
    void Attach(hc_ctx* ctx) override {
        hc_irregular_wave_params p;
        hc_irregular_wave_params_default(&p);
        p.num_bodies              = static_cast<int>(params_.num_bodies_);
        p.simulation_dt           = params_.simulation_dt_;
        p.simulation_duration     = params_.simulation_duration_;
        p.ramp_duration           = params_.ramp_duration_;
        p.wave_height             = params_.wave_height_;
        p.wave_period             = params_.wave_period_;
        p.frequency_min           = params_.frequency_min_;
        p.frequency_max           = params_.frequency_max_;
        p.nfrequencies            = params_.nfrequencies_;
        p.peak_enhancement_factor = params_.peak_enhancement_factor_;
        p.is_normalized           = params_.is_normalized_ ? 1 : 0;
        p.seed                    = params_.seed_;
        if (!params_.eta_file_path_.empty()) {  // InitializeIRFVectors (src/wave_types.cpp:451-453): the record instead of a spectrum
            int n = 0;
            if (hc_read_eta_file(params_.eta_file_path_.c_str(), nullptr, nullptr, 0, &n) != HC_OK) throw std::runtime_error(hc_last_error(nullptr));
            std::vector<double> t(n), eta(n);
            if (hc_read_eta_file(params_.eta_file_path_.c_str(), t.data(), eta.data(), n, &n) != HC_OK)
                throw std::runtime_error(hc_last_error(nullptr));
            check(ctx, hc_set_wave_irregular_eta(ctx, &p, t.data(), eta.data(), n));
        } else {
            check(ctx, hc_set_wave_irregular(ctx, &p));
        }
        attached(ctx);
    }
    // Exporter inputs (src/wave_types.cpp:461-478, read by the runner at run_hydrochrono_from_yaml.cpp:668-679).  GetSpectrum returns
    // the spectral densities S(f) its comment promises; the reference returns a member it never fills ("do not reproduce").
    // After SetRecordComponents an imported record answers with the one-sided periodogram A^2 / (2 df) of its kept components.
    std::vector<double> GetSpectrum() {
        if (!params_.eta_file_path_.empty() && !record_has_components())  // spectrumCreated_ == false (src/wave_types.cpp:461-467)
            throw std::runtime_error("Spectrum has not been created. Initialize with wave height and period to create spectrum.");
        return spectrum(1);
    }
    std::vector<double> GetFreeSurfaceElevation() { return table(false); }
    std::vector<double> GetFreeSurfaceTime() const { return table(true); }
    std::vector<double> GetFrequenciesHz() const { return spectrum(0); }
    // Wave components of an imported record (not in the reference; hc_set_eta_record_components in hydrochrono_amd.h): the record's
    // discrete Fourier coefficients inside [f_min_hz, f_max_hz], the max_components largest (0: all).  GetElevation / GetVelocity /
    // GetAcceleration and the side terms of the TestHydro this model is attached to then see that sea, the periodic continuation of
    // the record; the excitation convolution keeps its bits.  A sharded system calls it on the model of every shard.
    struct RecordComponents {
        std::vector<int> m;                     // bins of the record's Fourier grid
        std::vector<double> f, A, phase, k;     // Hz, m, rad, rad/m
        double mean = 0.0, variance_share = 0.0, rms_residual = 0.0;
    };
    void SetRecordComponents(double f_min_hz, double f_max_hz, int max_components = 0) {
        need_ctx();
        check(ctx_, hc_set_eta_record_components(ctx_, f_min_hz, f_max_hz, max_components));
    }
    void ClearRecordComponents() {
        need_ctx();
        check(ctx_, hc_clear_eta_record_components(ctx_));
    }
    RecordComponents GetRecordComponents() const {
        need_ctx();
        RecordComponents r;
        int n = 0;
        check(ctx_, hc_get_eta_record_components(ctx_, &n, nullptr, nullptr, nullptr, nullptr, nullptr, &r.mean, &r.variance_share, &r.rms_residual));
        r.m.resize(n), r.f.resize(n), r.A.resize(n), r.phase.resize(n), r.k.resize(n);
        check(ctx_, hc_get_eta_record_components(ctx_, nullptr, r.m.data(), r.f.data(), r.A.data(), r.phase.data(), r.k.data(), nullptr, nullptr, nullptr));
        return r;
    }
    // Visualisation helper the reference's irregular-wave demos call (demos/sphere/demo_sphere_irreg_waves.cpp:144-153,
    // src/wave_types.cpp:846-864): the free-surface elevation over the simulated time as a Wavefront OBJ ribbon (x = -t, y = -10 / +10,
    // z = eta(t)) that the demo drags past the body with GetWaveMeshVelocity().  Off the force path; written from the eta(t) table the
    // force path uses, against the table's own time stamps (t >= 0).
    void SetUpWaveMesh(std::string filename = "fse_mesh.obj") {
        mesh_file_name_ = std::move(filename);
        const std::vector<double> t = table(true), eta = table(false);
        std::FILE* out = std::fopen(mesh_file_name_.c_str(), "w");
        if (!out) throw std::runtime_error("SetUpWaveMesh: cannot write " + mesh_file_name_);
        std::fprintf(out, "# free-surface elevation ribbon (hydroc_amd)\n");
        size_t n = 0;
        for (size_t i = 0; i < t.size(); ++i) {
            if (t[i] < 0.0 || t[i] > params_.simulation_duration_) continue;
            std::fprintf(out, "v %.6f %.6f %.6f\nv %.6f %.6f %.6f\n", -t[i], -10.0, eta[i], -t[i], 10.0, eta[i]);
            ++n;
        }
        for (size_t i = 0; i + 1 < n; ++i)  // two triangles per step of the ribbon (OBJ indices are 1-based)
            std::fprintf(out, "f %zu %zu %zu\nf %zu %zu %zu\n", 2 * i + 1, 2 * i + 2, 2 * i + 4, 2 * i + 1, 2 * i + 4, 2 * i + 3);
        std::fclose(out);
    }
    std::string GetMeshFile() { return mesh_file_name_; }
    std::array<double, 3> GetWaveMeshVelocity() { return {1.0, 0.0, 0.0}; }  // (an Eigen::Vector3d in the reference; ChVector3d(v[0], v[1], v[2]))

  protected:
    hc_wave_kinematics_opts KinematicsOptions() const override {
        hc_wave_kinematics_opts o = WaveBase::KinematicsOptions();
        o.wave_stretching         = params_.wave_stretching_ ? 1 : 0;
        return o;
    }

  private:
    std::vector<double> spectrum(int which) const {
        need_ctx();
        int nf = 0;
        check(ctx_, hc_get_sizes(ctx_, nullptr, nullptr, nullptr, nullptr, &nf, nullptr, nullptr, nullptr));
        std::vector<double> v(nf);
        check(ctx_, which == 0 ? hc_get_spectrum(ctx_, v.data(), nullptr, nullptr, nullptr, nullptr)
                               : hc_get_spectrum(ctx_, nullptr, v.data(), nullptr, nullptr, nullptr));
        return v;
    }
    std::vector<double> table(bool time) const {
        need_ctx();
        int nt = 0;
        check(ctx_, hc_get_sizes(ctx_, nullptr, nullptr, nullptr, nullptr, nullptr, &nt, nullptr, nullptr));
        std::vector<double> v(nt);
        check(ctx_, time ? hc_get_eta_table(ctx_, v.data(), nullptr) : hc_get_eta_table(ctx_, nullptr, v.data()));
        return v;
    }
    void need_ctx() const {
        if (!ctx_) throw std::runtime_error("IrregularWaves is not attached to a TestHydro");
    }
    bool record_has_components() const {
        int n = 0;
        return ctx_ && hc_get_eta_record_components(ctx_, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == HC_OK && n > 0;
    }
    IrregularWaveParams params_;
    std::string mesh_file_name_;
};

}  // namespace hydroc_amd
