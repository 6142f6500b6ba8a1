// hydroc_amd/hydro_forces.h -- the reference's plugin surface for the hydro-force path (include/hydroc/hydro_forces.h:45-285) over the
// C ABI (include/hydrochrono_amd.h).  Header-only; link with libhydrochrono_amd.so.
//
// Source compatibility is the point of this file.  A program written against the reference
//
//     #include <hydroc/hydro_forces.h>                               ->   #include <hydroc_amd/hydro_forces.h>
//                                                                         using namespace hydroc_amd;
//     std::vector<std::shared_ptr<ChBody>> bodies;
//     bodies.push_back(sphereBody);
//     TestHydro hydro_forces(bodies, h5fname);                            (unchanged; demos/sphere/demo_sphere_reg_waves.cpp:130-133)
//     hydro_forces.AddWaves(my_hydro_inputs);                             (unchanged)
//
// keeps its hydro lines: with Project Chrono on the include path the constructor does what the reference's does
// (src/hydro_forces.cpp:170-242) -- BEMIO-HDF5 ingest, one ForceFunc6d per body (two WORLD_DIR ChForce objects "hydroforce" /
// "hydrotorque" fed by six ComponentFunc, added to the body, :96-168), ChLoadAddedMass in a ChLoadContainer added to the bodies'
// ChSystem (:223-234), AddWaves -- and every Chrono update then reaches the GPU as ONE hc_step (or hc_step_multi) per distinct
// time (CoordinateFuncForBody, :727-767).  Same names, argument meaning and error behaviour:
//   TestHydro(bodies, h5_file, waves = NoWave), AddWaves, GetWave, ComputeForceHydrostatics / RadiationDampingConv / Waves,
//   GetRIRFval, SetRadiationConvolutionMode, SetTaperedDirectOptions, SetDiagnosticsOutputDirectory, CoordinateFuncForBody,
//   GetProfileStats; ComponentFunc(ForceFunc6d*, i), ForceFunc6d(body, TestHydro*)::CoordinateFunc(i); HydroProfileStats.
// Additions (not in the reference): an optional trailing `device_ids` argument -- one body-row shard per listed GPU inside this one
// process -- and SetPassSchedule.
//
// Without Chrono (drivers, tests, the examples/) bodies are seen through the small `BodyView` interface -- exactly the ChBody
// getters the reference calls (src/hydro_forces.cpp:106-107,279-280,550,567-568); `MockBody` implements it with plain fields.
// Deliberate deviations from the reference are listed in DESIGN.md 1 (default NoWave() with more than one body is an error
// instead of an out-of-bounds read; a step back in time is handled).
#pragma once

#include <algorithm>
#include <array>
#include <complex>
#include <cstdlib>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../hydrochrono_amd.h"
#include "wave_types.h"

#if !defined(HYDROCHRONO_AMD_WITH_CHRONO) && defined(__has_include)
#if __has_include(<chrono/physics/ChBody.h>)
#define HYDROCHRONO_AMD_WITH_CHRONO 1
#endif
#endif

#ifdef HYDROCHRONO_AMD_WITH_CHRONO
#include <chrono/functions/ChFunction.h>
#include <chrono/physics/ChBody.h>
#include <chrono/physics/ChForce.h>
#include <chrono/physics/ChLoad.h>
#include <chrono/physics/ChLoadContainer.h>
#include <chrono/physics/ChSystem.h>
#endif

namespace hydroc_amd {

// ---------------------------------------------------------------------------------------------------------------
// Body view: what the force path reads from a body
// ---------------------------------------------------------------------------------------------------------------
struct BodyView {
    virtual ~BodyView()                                      = default;
    virtual std::string GetName() const                      = 0;  // "body<k>", 1-based (src/hydro_forces.cpp:106-107)
    virtual double GetChTime() const                         = 0;
    virtual std::array<double, 3> GetPos() const             = 0;
    virtual std::array<double, 3> GetCardanAnglesXYZ() const = 0;  // GetRot().GetCardanAnglesXYZ()
    virtual std::array<double, 3> GetPosDt() const           = 0;
    virtual std::array<double, 3> GetAngVelParent() const    = 0;
};

struct MockBody : BodyView {
    std::string name;
    double time = 0.0;
    std::array<double, 3> pos{0, 0, 0}, rpy{0, 0, 0}, linvel{0, 0, 0}, angvel{0, 0, 0};
    explicit MockBody(std::string n) : name(std::move(n)) {}
    std::string GetName() const override { return name; }
    double GetChTime() const override { return time; }
    std::array<double, 3> GetPos() const override { return pos; }
    std::array<double, 3> GetCardanAnglesXYZ() const override { return rpy; }
    std::array<double, 3> GetPosDt() const override { return linvel; }
    std::array<double, 3> GetAngVelParent() const override { return angvel; }
};

#ifdef HYDROCHRONO_AMD_WITH_CHRONO
struct ChronoBody : BodyView {
    std::shared_ptr<chrono::ChBody> body;
    explicit ChronoBody(std::shared_ptr<chrono::ChBody> b) : body(std::move(b)) {}
    std::string GetName() const override { return body->GetName(); }
    double GetChTime() const override { return body->GetChTime(); }
    std::array<double, 3> GetPos() const override { auto v = body->GetPos(); return {v.x(), v.y(), v.z()}; }
    std::array<double, 3> GetCardanAnglesXYZ() const override { auto v = body->GetRot().GetCardanAnglesXYZ(); return {v.x(), v.y(), v.z()}; }
    std::array<double, 3> GetPosDt() const override { auto v = body->GetPosDt(); return {v.x(), v.y(), v.z()}; }
    std::array<double, 3> GetAngVelParent() const override { auto v = body->GetAngVelParent(); return {v.x(), v.y(), v.z()}; }
};

class TestHydro;
class ForceFunc6d;
class ChLoadAddedMass;

// ComponentFunc (include/hydroc/hydro_forces.h:45-86): one degree of freedom of a body's hydro force as a ChFunction.  GetVal's
// argument is ignored -- the time comes from the first body (src/hydro_forces.cpp:79-85,739).
class ComponentFunc : public chrono::ChFunction {
  public:
    ComponentFunc() : base_(nullptr), index_(6) {}
    ComponentFunc(ForceFunc6d* b, int i) : base_(b), index_(i) {}
    ComponentFunc(const ComponentFunc& old) : chrono::ChFunction(old), base_(old.base_), index_(old.index_) {}
    ComponentFunc* Clone() const override { return new ComponentFunc(*this); }
    double GetVal(double x) const override;

  private:
    ForceFunc6d* base_;
    int index_;
};

// ForceFunc6d (include/hydroc/hydro_forces.h:91-148): the six components of one body, wired as two ChForce objects.  Owned by
// TestHydro behind a stable address (the reference re-points its ComponentFunc array after vector growth, :117-134; here the
// objects never move, so the class is not copyable).
class ForceFunc6d {
  public:
    ForceFunc6d(std::shared_ptr<chrono::ChBody> object, TestHydro* all_hydro_forces_user);
    ForceFunc6d(const ForceFunc6d&)            = delete;
    ForceFunc6d& operator=(const ForceFunc6d&) = delete;
    double CoordinateFunc(int i);
    int body_number() const { return b_num_; }

  private:
    std::shared_ptr<chrono::ChBody> body_;
    int b_num_;  // 1-based, from the body name "body<k>"
    std::shared_ptr<ComponentFunc> force_ptrs_[6];
    std::shared_ptr<chrono::ChForce> chrono_force_, chrono_torque_;
    TestHydro* all_hydro_forces_;
};
#endif  // HYDROCHRONO_AMD_WITH_CHRONO

struct HydroProfileStats {  // include/hydroc/hydro_forces.h:153-160
    double hydrostatics_seconds = 0.0, radiation_seconds = 0.0, waves_seconds = 0.0;
    int hydrostatics_calls = 0, radiation_calls = 0, waves_calls = 0;
};

// A Morison drag / inertia element of a body (not in the reference; hc_morison_element): position in the body frame, Cd_i A_i [m^2]
// and Cm_i V [m^3] per body axis.
struct MorisonElement {
    std::array<double, 3> r{0, 0, 0}, cd_area{0, 0, 0}, cm_vol{0, 0, 0};
};

// A Morison strip member of a body (not in the reference; hc_morison_member): a slender cylinder from r0 to r1 in the body frame,
// diameter d0 at r0 and d1 at r1, transverse Cd and Cm, integrated along its wet length in n_seg segments (1..64).
struct MorisonMember {
    std::array<double, 3> r0{0, 0, 0}, r1{0, 0, 0};
    double d0 = 0.0, d1 = 0.0, cd = 0.0, cm = 0.0;
    int n_seg = 1;
};

// What the Morison elements of a body saw of the second-order sea (TestHydro::GetMorisonIncrements): per element the world point
// and the increments of WaveBase::GetSecondOrderElevation / Velocity / Acceleration there.
struct MorisonIncrements {
    std::vector<std::array<double, 3>> p, vel2, acc2;
    std::vector<double> eta2;
};

// What the strip members of a body saw of the second-order sea (TestHydro::GetMorisonMemberIncrements), over the body's members in
// index order: per node (n_seg + 1 of each member) the world position and the elevation increment that moved the cut; per Gauss
// point (2 n_seg of each member) the world position and the increments, exact zeros behind the point of a dry segment.
struct MorisonMemberIncrements {
    std::vector<std::array<double, 3>> node_p;
    std::vector<double> node_eta2;
    std::vector<std::array<double, 3>> p, vel2, acc2;
    std::vector<double> eta2;
};

// What the surface points of a body saw of the second-order sea (TestHydro::GetNonlinearIncrements): per distinct point -- a panel's
// centroid, a triangle's vertex -- the world position, the elevation increment and q2 = -d phi2 / dt [m^2/s^2].
struct NonlinearIncrements {
    std::vector<std::array<double, 3>> p;
    std::vector<double> eta2, q2;
};

// A radiation mode of a body (not in the reference; hc_radiation_mode): row 0..5 of the body, column 0..6N-1, complex pole
// (Re < 0) and residue, K_rc(tau) = sum Re[rho exp(lambda tau)] in the units of the file's K.
struct RadiationMode {
    int row = 0, col = 0;
    std::complex<double> lambda{-1.0, 0.0}, rho{0.0, 0.0};
};

// A surface panel of a body (not in the reference; hc_surface_panel): centroid [m] and area vector [m^2] (area times the outward
// normal, body into water) in the body frame.
struct SurfacePanel {
    std::array<double, 3> c{0, 0, 0}, s{0, 0, 0};
};

// ---------------------------------------------------------------------------------------------------------------
// TestHydro
// ---------------------------------------------------------------------------------------------------------------
class TestHydro {
  public:
    TestHydro()                            = delete;
    TestHydro(const TestHydro&)            = delete;
    TestHydro& operator=(const TestHydro&) = delete;

#ifdef HYDROCHRONO_AMD_WITH_CHRONO
    // The reference's constructor (include/hydroc/hydro_forces.h:178-180, src/hydro_forces.cpp:170-242): reads the h5 file, wires the
    // forces and the added-mass load into the bodies' ChSystem, attaches the waves.
    TestHydro(std::vector<std::shared_ptr<chrono::ChBody>> user_bodies, std::string h5_file_name,
              std::shared_ptr<WaveBase> waves = std::make_shared<NoWave>())
        : TestHydro(std::move(user_bodies), std::move(h5_file_name), std::move(waves), std::vector<int>{0}) {}
    // ... on several GPUs: one body-row shard per entry of `device_ids` (a device may be listed more than once)
    TestHydro(std::vector<std::shared_ptr<chrono::ChBody>> user_bodies, std::string h5_file_name, std::shared_ptr<WaveBase> waves,
              const std::vector<int>& device_ids);
#endif

    TestHydro(std::vector<std::shared_ptr<BodyView>> user_bodies, const std::string& h5_file_name,
              std::shared_ptr<WaveBase> waves = std::make_shared<NoWave>(), int device_id = 0)
        : TestHydro(std::move(user_bodies), h5_file_name, std::move(waves), std::vector<int>{device_id}) {}
    // Multi-GPU inside the one Chrono process (drop-in variant): contiguous balanced split of the bodies over the
    // shards; every call below fans out to the shard contexts, the per-step evaluation goes through hc_step_multi (all GPUs
    // started before any is waited for, host-side gather).  One entry = the single-GPU object.
    TestHydro(std::vector<std::shared_ptr<BodyView>> user_bodies, const std::string& h5_file_name, std::shared_ptr<WaveBase> waves,
              const std::vector<int>& device_ids)
        : bodies_(std::move(user_bodies)), num_bodies_(static_cast<int>(bodies_.size())) {
        create_contexts(h5_file_name, std::move(waves), device_ids);
    }
    // Adopts contexts that are already configured (hc_create_from_hydro_yaml[_sharded], or a C caller's own set-up): together they
    // own bodies [0, N).  Their configuration -- pass schedule included -- is left as it is.  The contexts belong to the object
    // from the call on, also when it throws.
    TestHydro(std::vector<std::shared_ptr<BodyView>> user_bodies, hc_ctx* configured_ctx)
        : TestHydro(std::move(user_bodies), std::vector<hc_ctx*>{configured_ctx}) {}
    TestHydro(std::vector<std::shared_ptr<BodyView>> user_bodies, std::vector<hc_ctx*> configured_ctxs)
        : bodies_(std::move(user_bodies)), num_bodies_(static_cast<int>(bodies_.size())), ctxs_(std::move(configured_ctxs)) {
        try {
            if (ctxs_.empty() || bodies_.empty()) throw std::runtime_error("TestHydro: no context / no body");
            ctx_ = ctxs_[0];
            read_body_numbers();
            total_force_.assign(6 * static_cast<size_t>(num_bodies_), 0.0);
        } catch (...) {
            destroy_contexts();
            throw;
        }
    }
    ~TestHydro() { destroy_contexts(); }

    void AddWaves(std::shared_ptr<WaveBase> waves) {  // src/hydro_forces.cpp:244-261
        user_waves_ = std::move(waves);
        for (auto it = ctxs_.rbegin(); it != ctxs_.rend(); ++it) user_waves_->Attach(*it);  // (the wave object keeps the first context for its getters)
    }
    std::shared_ptr<WaveBase> GetWave() const { return user_waves_; }
    // ChSystem::GetGravitationalAcceleration(), which the reference reads in every hydrostatics evaluation (:267-269).  The
    // ChBody constructors follow the system's value by themselves; Chrono-free drivers set it here (default (0, 0, -9.81)).
    void SetGravitationalAcceleration(double gx, double gy, double gz) {
        const double g[3] = {gx, gy, gz};
        for (hc_ctx* c : ctxs_) check(c, hc_set_gravity(c, g));
        gravity_ = {gx, gy, gz};
    }

    enum class RadiationConvolutionMode { Baseline, TaperedDirect };
    void SetRadiationConvolutionMode(RadiationConvolutionMode mode) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_convolution_mode(c, mode == RadiationConvolutionMode::TaperedDirect ? 1 : 0));
    }
    struct TaperedDirectOptions {  // include/hydroc/hydro_forces.h:246-259
        std::string smoothing        = "sg";  // "sg" (Savitzky-Golay) or "moving_average"
        int window_length            = 5;
        double rirf_end_time         = -1.0;
        double taper_start_percent   = 0.8;
        double taper_end_percent     = 1.0;
        double taper_final_amplitude = 0.0;
        bool export_plot_csv         = false;  // rirf_body<b>_summary.csv in the diagnostics directory (src/hydro_forces.cpp:509-531)
    };
    void SetTaperedDirectOptions(const TaperedDirectOptions& o) {
        hc_tapered_direct_options c;
        hc_tapered_direct_options_default(&c);
        c.smoothing             = (o.smoothing == "moving_average") ? 1 : 0;
        c.window_length         = o.window_length;
        c.rirf_end_time         = o.rirf_end_time;
        c.taper_start_percent   = o.taper_start_percent;
        c.taper_end_percent     = o.taper_end_percent;
        c.taper_final_amplitude = o.taper_final_amplitude;
        c.export_plot_csv       = o.export_plot_csv ? 1 : 0;
        for (hc_ctx* x : ctxs_) check(x, hc_set_tapered_direct_options(x, &c));
    }
    void SetDiagnosticsOutputDirectory(const std::string& dir) {  // include/hydroc/hydro_forces.h:269
        for (hc_ctx* x : ctxs_) check(x, hc_set_diagnostics_output_directory(x, dir.c_str()));
    }

    // Not in the reference (it has no such notion): when the look-ahead pass of a block runs, see hc_set_pass_schedule.  The contexts
    // come with the library's ADAPTIVE schedule (one_block_ahead < 0): a Chrono loop, which does its own work between two force
    // evaluations, gets the pass of every block one block ahead, beside the steps (64 bodies, 30 / 100 us of host work between calls:
    // 12.8 / 12.7 us per step instead of 17.4 / 15.6, and no step waits for a whole pass); a driver that steps back to back gets it at
    // block start.  0 / 1 pin a schedule.
    void SetPassSchedule(int one_block_ahead, int slices = 0) {
        for (hc_ctx* x : ctxs_) check(x, hc_set_pass_schedule(x, one_block_ahead < 0 ? -1 : (one_block_ahead ? 1 : 0), slices));
    }

    std::vector<double> ComputeForceHydrostatics() {
        gather_state();
        std::vector<double> out(6 * static_cast<size_t>(num_bodies_));
        for (hc_ctx* c : ctxs_) check(c, hc_compute_hydrostatics(c, pos_.data(), rpy_.data(), out.data() + row0(c)));
        return out;
    }
    std::vector<double> ComputeForceRadiationDampingConv() {
        gather_state();
        std::vector<double> out(6 * static_cast<size_t>(num_bodies_));
        for (hc_ctx* c : ctxs_) check(c, hc_compute_radiation(c, bodies_[0]->GetChTime(), lin_.data(), ang_.data(), out.data() + row0(c)));
        return out;
    }
    std::vector<double> ComputeForceWaves() {  // (an Eigen::VectorXd in the reference)
        std::vector<double> out(6 * static_cast<size_t>(num_bodies_));
        for (hc_ctx* c : ctxs_) check(c, hc_compute_waves(c, bodies_[0]->GetChTime(), out.data() + row0(c)));
        return out;
    }
    // Morison elements (not in the reference; include/hydrochrono_amd.h: hc_set_morison_elements).  Once a body carries elements,
    // CoordinateFuncForBody returns total + Morison term: hc_morison_begin on every shard, the step, hc_morison_end on every shard,
    // one elementwise add.  The body index is 1-based, as everywhere in this class; an empty vector clears the list.
    void SetMorisonElements(int body_index_1_based, const std::vector<MorisonElement>& elements) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetMorisonElements: body index out of range");
        std::vector<hc_morison_element> raw(elements.size());
        for (size_t e = 0; e < elements.size(); ++e)
            for (int k = 0; k < 3; ++k) {
                raw[e].r[k]       = elements[e].r[k];
                raw[e].cd_area[k] = elements[e].cd_area[k];
                raw[e].cm_vol[k]  = elements[e].cm_vol[k];
            }
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_elements(c, body_index_1_based - 1, raw.data(), static_cast<int>(raw.size())));
        morison_count_.resize(static_cast<size_t>(num_bodies_), 0);
        morison_count_[static_cast<size_t>(body_index_1_based - 1)] = raw.size();
        update_have_morison();
        have_time_    = false;  // the cached total belongs to the lists before
    }
    // Morison strip members (hc_set_morison_members): cylinders between two end points, cut at the free surface.  A body with
    // members counts as one that carries elements: the Morison term CoordinateFuncForBody adds is elements + members.  An empty
    // vector clears the list.
    void SetMorisonMembers(int body_index_1_based, const std::vector<MorisonMember>& members) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetMorisonMembers: body index out of range");
        std::vector<hc_morison_member> raw(members.size());
        for (size_t e = 0; e < members.size(); ++e) {
            for (int k = 0; k < 3; ++k) {
                raw[e].r0[k] = members[e].r0[k];
                raw[e].r1[k] = members[e].r1[k];
            }
            raw[e].d0    = members[e].d0;
            raw[e].d1    = members[e].d1;
            raw[e].cd    = members[e].cd;
            raw[e].cm    = members[e].cm;
            raw[e].n_seg = members[e].n_seg;
        }
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_members(c, body_index_1_based - 1, raw.data(), static_cast<int>(raw.size())));
        morison_member_count_.resize(static_cast<size_t>(num_bodies_), 0);
        morison_member_count_[static_cast<size_t>(body_index_1_based - 1)] = raw.size();
        if (static_cast<size_t>(body_index_1_based - 1) < morison_member_ca_.size()) morison_member_ca_[static_cast<size_t>(body_index_1_based - 1)] = false;
        update_have_morison();
        have_time_ = false;
    }
    // The members on the second-order sea (hc_set_morison_members_second_order): with SetMorisonSecondOrder on -- and
    // SetMorisonSecondOrderDirectional under wave directions -- eta2 at every node moves the cut and u2, a2 at the Gauss points enter
    // the force, where CoordinateFuncForBody otherwise throws for a body with members.  A switch of its own.  Applied to every shard
    // context.
    void SetMorisonMembersSecondOrder(bool on) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_members_second_order(c, on ? 1 : 0));
        have_time_ = false;
    }
    // What the members of a body saw in the last evaluation on the second-order sea (hc_get_morison_member_node_increments,
    // hc_get_morison_member_point_increments), answered by the shard that owns the body.
    MorisonMemberIncrements GetMorisonMemberIncrements(int body_index_1_based) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("GetMorisonMemberIncrements: body index out of range");
        const int b = body_index_1_based - 1;
        for (hc_ctx* c : ctxs_) {
            int b0 = 0, b1 = 0;
            check(c, hc_get_shard(c, &b0, &b1));
            if (b < b0 || b >= b1) continue;
            int n_nodes = 0, n_points = 0;
            check(c, hc_get_morison_member_increment_counts(c, b, &n_nodes, &n_points));
            const size_t nn = static_cast<size_t>(n_nodes), np = static_cast<size_t>(n_points);
            std::vector<double> P(3 * nn + 1), p(3 * np + 1), vel(3 * np + 1), acc(3 * np + 1);
            MorisonMemberIncrements out;
            out.node_eta2.resize(nn);
            out.eta2.resize(np);
            check(c, hc_get_morison_member_node_increments(c, b, P.data(), out.node_eta2.data()));
            check(c, hc_get_morison_member_point_increments(c, b, p.data(), out.eta2.data(), vel.data(), acc.data()));
            for (size_t j = 0; j < nn; ++j) out.node_p.push_back({P[3 * j], P[3 * j + 1], P[3 * j + 2]});
            for (size_t e = 0; e < np; ++e) {
                out.p.push_back({p[3 * e], p[3 * e + 1], p[3 * e + 2]});
                out.vel2.push_back({vel[3 * e], vel[3 * e + 1], vel[3 * e + 2]});
                out.acc2.push_back({acc[3 * e], acc[3 * e + 1], acc[3 * e + 2]});
            }
            return out;
        }
        throw std::out_of_range("GetMorisonMemberIncrements: no context owns the body");
    }
    // The 6-vectors of a body's members in the last evaluation (hc_get_morison_member_forces), from the context that owns the body
    std::vector<std::array<double, 6>> GetMorisonMemberForces(int body_index_1_based) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("GetMorisonMemberForces: body index out of range");
        const int b = body_index_1_based - 1;
        for (hc_ctx* c : ctxs_) {
            int b0 = 0, b1 = 0, n = 0;
            check(c, hc_get_shard(c, &b0, &b1));
            if (b < b0 || b >= b1) continue;
            check(c, hc_get_morison_member_count(c, b, &n));
            std::vector<std::array<double, 6>> out(static_cast<size_t>(n));
            std::vector<double> flat(6 * static_cast<size_t>(n) + 1);
            check(c, hc_get_morison_member_forces(c, b, flat.data()));
            for (size_t e = 0; e < out.size(); ++e)
                for (size_t k = 0; k < 6; ++k) out[e][k] = flat[6 * e + k];
            return out;
        }
        throw std::out_of_range("GetMorisonMemberForces: no context owns the body");
    }
    // The added-mass coefficients ca >= 0 of a body's members (hc_set_morison_member_added_mass), one per member of the list as it
    // stands; an empty vector clears them and SetMorisonMembers resets them to 0.  The forces do not change; from the next
    // evaluation on GetMorisonAddedMass returns the body's 6 x 6 matrix on the instantaneous wet length, which
    // ChLoadAddedMass::SetIncludeMorisonAddedMass hands to Chrono.  Applied to every shard context.
    void SetMorisonMemberAddedMass(int body_index_1_based, const std::vector<double>& ca) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetMorisonMemberAddedMass: body index out of range");
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_member_added_mass(c, body_index_1_based - 1, ca.data(), static_cast<int>(ca.size())));
        bool any = false;
        for (double v : ca) any = any || v > 0.0;
        morison_member_ca_.resize(static_cast<size_t>(num_bodies_), false);
        morison_member_ca_[static_cast<size_t>(body_index_1_based - 1)] = any;
        have_time_ = false;  // the next read evaluates again: the matrices belong to an evaluation with these coefficients
    }
    // The body's added-mass matrix [6][6] (row-major; world axes, at the body's reference point) in the last evaluation
    // (hc_get_morison_added_mass), from the context that owns the body; zeros for a body no member of which has ca > 0
    std::array<double, 36> GetMorisonAddedMass(int body_index_1_based) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("GetMorisonAddedMass: body index out of range");
        const int b = body_index_1_based - 1;
        std::array<double, 36> out{};
        if (static_cast<size_t>(b) >= morison_member_ca_.size() || !morison_member_ca_[static_cast<size_t>(b)]) return out;
        hc_ctx* c = owner_of(b, "GetMorisonAddedMass");
        check(c, hc_get_morison_added_mass(c, b, out.data()));
        return out;
    }
    // ... and those of its members (hc_get_morison_member_added_mass): their serial sum in member order is the body's, bit for bit;
    // zeros as well for a body no member of which has ca > 0
    std::vector<std::array<double, 36>> GetMorisonMemberAddedMass(int body_index_1_based) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("GetMorisonMemberAddedMass: body index out of range");
        const int b = body_index_1_based - 1;
        hc_ctx* c   = owner_of(b, "GetMorisonMemberAddedMass");
        int n       = 0;
        check(c, hc_get_morison_member_count(c, b, &n));
        std::vector<std::array<double, 36>> out(static_cast<size_t>(n));  // (zeros)
        if (static_cast<size_t>(b) >= morison_member_ca_.size() || !morison_member_ca_[static_cast<size_t>(b)]) return out;
        std::vector<double> flat(36 * static_cast<size_t>(n) + 1);
        check(c, hc_get_morison_member_added_mass(c, b, flat.data()));
        for (size_t e = 0; e < out.size(); ++e)
            for (size_t k = 0; k < 36; ++k) out[e][k] = flat[36 * e + k];
        return out;
    }
    // mwl, regular phase and stretching of the kinematics the elements see (those of WaveBase::GetVelocity & co.)
    void SetMorisonOptions(double mwl = 0.0, double regular_phase = 0.0, bool wave_stretching = true) {
        hc_wave_kinematics_opts o;
        hc_wave_kinematics_opts_default(&o);
        o.mwl             = mwl;
        o.regular_phase   = regular_phase;
        o.wave_stretching = wave_stretching ? 1 : 0;
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_options(c, &o));
        have_time_ = false;
    }
    // Wave heading and short-crested seas (not in the reference; include/hydrochrono_amd.h: hc_set_wave_directions): one direction
    // [rad] per component of the wave model in force, on every shard context; the wave object keeps them (wave_directions_) across a
    // later AddWaves of the same object; an empty vector clears them.  The kinematics, the Morison elements, the
    // nonlinear surface forces and -- with SetExcitationRAOHeadings -- the first-order excitation then follow the heading; the
    // second-order terms and both QTF terms throw from CoordinateFuncForBody while directions are set.
    void SetWaveDirections(const std::vector<double>& theta_rad) {
        if (!user_waves_) throw std::runtime_error("SetWaveDirections: no wave model (AddWaves)");
        for (hc_ctx* c : ctxs_)
            check(c, hc_set_wave_directions(c, static_cast<int>(theta_rad.size()), theta_rad.empty() ? nullptr : theta_rad.data()));
        user_waves_->wave_directions_ = theta_rad;
        have_time_ = false;  // the cached total belongs to the sea before
    }
    std::vector<double> GetWaveDirections() const {
        if (!user_waves_) return {};
        return user_waves_->GetDirections();
    }
    std::vector<double> SetWaveSpreading(double heading_rad, double s = 0.0, int n_bins = 15, unsigned long long seed = 1) {
        if (!user_waves_) throw std::runtime_error("SetWaveSpreading: no wave model (AddWaves)");
        const std::vector<double> th = user_waves_->SpreadingDirections(heading_rad, s, n_bins, seed);
        SetWaveDirections(th);
        return th;
    }
    // Excitation coefficients of a body on a grid of headings (hc_set_excitation_rao_headings): dirs [n_dir] strictly increasing,
    // mag / phase [6][n_dir][nw] as in a BEMIO file; empty dirs remove them.  The body index is 1-based.
    void SetExcitationRAOHeadings(int body_index_1_based, const std::vector<double>& dirs_rad, const std::vector<double>& w,
                                  const std::vector<double>& mag, const std::vector<double>& phase) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetExcitationRAOHeadings: body index out of range");
        const size_t len = 6 * dirs_rad.size() * w.size();
        if (mag.size() != len || phase.size() != len) throw std::invalid_argument("SetExcitationRAOHeadings: mag and phase must hold 6 * n_dir * nw values");
        for (hc_ctx* c : ctxs_)
            check(c, hc_set_excitation_rao_headings(c, body_index_1_based - 1, static_cast<int>(dirs_rad.size()), dirs_rad.data(), w.data(),
                                                    static_cast<int>(w.size()), mag.data(), phase.data()));
        have_time_ = false;
    }
    // The elements on the second-order sea (hc_set_morison_second_order): the increments of WaveBase::GetSecondOrder* at every
    // element, added before the wet test and the force; the cut-offs [rad/s] are as in WaveBase::second_order_, mwl and the
    // regular phase those of SetMorisonOptions.  Applied to every shard context; on = false frees the tables.
    void SetMorisonSecondOrder(bool on, double diff_lo = 0.0, double diff_hi = std::numeric_limits<double>::infinity(), double sum_lo = 0.0,
                               double sum_hi = std::numeric_limits<double>::infinity(), bool apply_ramp = true) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_second_order(c, on ? 1 : 0, diff_lo, diff_hi, sum_lo, sum_hi, apply_ramp ? 1 : 0));
        have_time_ = false;
    }
    // Under wave directions the elements see the increments of WaveBase::GetDirectionalSecondOrder* instead of a refusal
    // (hc_set_morison_second_order_directional): a switch of its own beside SetMorisonSecondOrder.  Applied to every shard context.
    void SetMorisonSecondOrderDirectional(bool on) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_morison_second_order_directional(c, on ? 1 : 0));
        have_time_ = false;
    }
    // What the elements of a body saw in the last evaluation on the second-order sea (hc_get_morison_increments): one entry per
    // element, answered by the shard that owns the body.
    MorisonIncrements GetMorisonIncrements(int body_index_1_based) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("GetMorisonIncrements: body index out of range");
        const int b = body_index_1_based - 1;
        for (hc_ctx* c : ctxs_) {
            int b0 = 0, b1 = 0, n = 0;
            check(c, hc_get_shard(c, &b0, &b1));
            if (b < b0 || b >= b1) continue;
            check(c, hc_get_morison_count(c, b, &n));
            std::vector<double> p(3 * static_cast<size_t>(n)), vel(p.size()), acc(p.size());
            MorisonIncrements out;
            out.eta2.resize(static_cast<size_t>(n));
            check(c, hc_get_morison_increments(c, b, p.data(), out.eta2.data(), vel.data(), acc.data()));
            for (int e = 0; e < n; ++e) {
                out.p.push_back({p[3 * e], p[3 * e + 1], p[3 * e + 2]});
                out.vel2.push_back({vel[3 * e], vel[3 * e + 1], vel[3 * e + 2]});
                out.acc2.push_back({acc[3 * e], acc[3 * e + 1], acc[3 * e + 2]});
            }
            return out;
        }
        throw std::out_of_range("GetMorisonIncrements: no context owns the body");
    }
    std::vector<double> ComputeForceMorison() {
        return compute_alone(kMorison);
    }

    // Nonlinear buoyancy and Froude-Krylov forces on surface panels (not in the reference; include/hydrochrono_amd.h:
    // hc_set_surface_panels).  With a mode > 0, CoordinateFuncForBody returns, for a body that carries panels,
    // total - hs_lin + buoy (mode 1) or total - hs_lin + buoy + fk (mode 2: the excitation data should then be the scattering part
    // only, nothing is subtracted from the wave term); the rows of other bodies are untouched.  The body index is 1-based; an
    // empty vector clears the list.
    void SetSurfacePanels(int body_index_1_based, const std::vector<SurfacePanel>& panels) {
        const int body = surface_body(body_index_1_based, "SetSurfacePanels");
        std::vector<hc_surface_panel> raw(panels.size());
        for (size_t e = 0; e < panels.size(); ++e)
            for (int k = 0; k < 3; ++k) {
                raw[e].c[k] = panels[e].c[k];
                raw[e].s[k] = panels[e].s[k];
            }
        for (hc_ctx* c : ctxs_) check(c, hc_set_surface_panels(c, body, raw.data(), static_cast<int>(raw.size())));
        surface_list_set(body, raw.size());
    }
    // triangles (three vertices each, in the body frame, counter-clockwise seen from the water):
    // c = (v0 + v1 + v2) / 3, s = 1/2 (v1 - v0) x (v2 - v0)
    // clip = true keeps the vertices instead (hc_set_surface_triangles): every triangle is cut at the instantaneous free surface.  A
    // body carries panels or triangles: either call replaces what the body carried.
    void SetSurfaceMesh(int body_index_1_based, const std::vector<std::array<std::array<double, 3>, 3>>& triangles, bool clip = false) {
        if (clip) {
            const int body = surface_body(body_index_1_based, "SetSurfaceMesh");
            std::vector<double> raw;
            raw.reserve(9 * triangles.size());
            for (const auto& v : triangles)
                for (int j = 0; j < 3; ++j) raw.insert(raw.end(), v[j].begin(), v[j].end());
            for (hc_ctx* c : ctxs_) check(c, hc_set_surface_triangles(c, body, raw.data(), static_cast<int>(triangles.size())));
            surface_list_set(body, triangles.size());
            return;
        }
        std::vector<SurfacePanel> panels(triangles.size());
        for (size_t e = 0; e < triangles.size(); ++e) {
            const auto& v = triangles[e];
            double a[3], b[3];
            for (int k = 0; k < 3; ++k) {
                panels[e].c[k] = (v[0][k] + v[1][k] + v[2][k]) / 3.0;
                a[k]           = v[1][k] - v[0][k];
                b[k]           = v[2][k] - v[0][k];
            }
            panels[e].s = {0.5 * (a[1] * b[2] - a[2] * b[1]), 0.5 * (a[2] * b[0] - a[0] * b[2]), 0.5 * (a[0] * b[1] - a[1] * b[0])};
        }
        SetSurfacePanels(body_index_1_based, panels);
    }
    // 0: off, 1: nonlinear buoyancy, 2: nonlinear buoyancy + Froude-Krylov
    void SetNonlinearHydroMode(int mode) {
        if (mode < 0 || mode > 2) throw std::invalid_argument("SetNonlinearHydroMode: mode must be 0, 1 or 2");
        nonlinear_mode_ = mode;
        have_time_      = false;
    }
    // mwl, regular phase and stretching of the kinematics the panels see (those of WaveBase::GetVelocity & co.)
    void SetNonlinearHydroOptions(double mwl = 0.0, double regular_phase = 0.0, bool wave_stretching = true) {
        hc_wave_kinematics_opts o;
        hc_wave_kinematics_opts_default(&o);
        o.mwl             = mwl;
        o.regular_phase   = regular_phase;
        o.wave_stretching = wave_stretching ? 1 : 0;
        for (hc_ctx* c : ctxs_) check(c, hc_set_nonlinear_options(c, &o));
        have_time_ = false;
    }
    // The panels and clipped triangles on the second-order sea (hc_set_nonlinear_second_order): eta1 + eta2 in the wet test and the
    // clipping height, rho q2 - 1/2 rho ramp^2 |u1|^2 added to the dynamic pressure; the cut-offs [rad/s] are as in
    // WaveBase::second_order_, mwl and the regular phase those of SetNonlinearHydroOptions.  Applied to every shard context;
    // on = false frees the tables.  CoordinateFuncForBody composes as before, with no further call.
    void SetNonlinearSecondOrder(bool on, double diff_lo = 0.0, double diff_hi = std::numeric_limits<double>::infinity(), double sum_lo = 0.0,
                                 double sum_hi = std::numeric_limits<double>::infinity(), bool apply_ramp = true) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_nonlinear_second_order(c, on ? 1 : 0, diff_lo, diff_hi, sum_lo, sum_hi, apply_ramp ? 1 : 0));
        have_time_ = false;
    }
    // Under wave directions the surface points see eta2 and q2 of the directional pair sum (WaveBase::GetDirectionalSecondOrder*) and
    // |u1|^2 with its y component instead of a refusal (hc_set_nonlinear_second_order_directional): a switch of its own beside
    // SetNonlinearSecondOrder.  Applied to every shard context.
    void SetNonlinearSecondOrderDirectional(bool on) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_nonlinear_second_order_directional(c, on ? 1 : 0));
        have_time_ = false;
    }
    // What the surface points of a body saw in the last evaluation on the second-order sea (hc_get_nonlinear_increments): one entry
    // per distinct point, answered by the shard that owns the body.
    NonlinearIncrements GetNonlinearIncrements(int body_index_1_based) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("GetNonlinearIncrements: body index out of range");
        const int b = body_index_1_based - 1;
        for (hc_ctx* c : ctxs_) {
            int b0 = 0, b1 = 0, n = 0;
            check(c, hc_get_shard(c, &b0, &b1));
            if (b < b0 || b >= b1) continue;
            check(c, hc_get_nonlinear_point_count(c, b, &n));
            std::vector<double> p(3 * static_cast<size_t>(n));
            NonlinearIncrements out;
            out.eta2.resize(static_cast<size_t>(n));
            out.q2.resize(static_cast<size_t>(n));
            check(c, hc_get_nonlinear_increments(c, b, n, p.data(), out.eta2.data(), out.q2.data()));
            for (int e = 0; e < n; ++e) out.p.push_back({p[3 * e], p[3 * e + 1], p[3 * e + 2]});
            return out;
        }
        throw std::out_of_range("GetNonlinearIncrements: no context owns the body");
    }
    // buoy | fk | hs_lin of all bodies for the bodies' present state, 6 N values each
    std::vector<double> ComputeForceNonlinear() {
        return compute_alone(kNonlinear);
    }

    // Second-order wave drift forces from difference-frequency QTF tables (not in the reference; include/hydrochrono_amd.h:
    // hc_set_drift_qtf).  omega [nq] rad/s strictly increasing, P and Q [6][nq][nq] row-major (Q may be empty: zeros), force per
    // squared amplitude, dimensional.  With a mode > 0 and at least one table CoordinateFuncForBody returns total + drift term, added
    // after the nonlinear composition and the Morison term.  The body index is 1-based; an empty omega clears the table.
    void SetDriftQTF(int body_index_1_based, const std::vector<double>& omega, const std::vector<double>& P, const std::vector<double>& Q = {}) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetDriftQTF: body index out of range");
        const size_t nq = omega.size(), n6 = 6 * nq * nq;
        if (P.size() != n6 || (!Q.empty() && Q.size() != n6)) throw std::invalid_argument("SetDriftQTF: P and Q must hold 6 * nq * nq values");
        for (hc_ctx* c : ctxs_)
            check(c, hc_set_drift_qtf(c, body_index_1_based - 1, static_cast<int>(nq), nq ? omega.data() : nullptr, nq ? P.data() : nullptr,
                                      Q.empty() ? nullptr : Q.data()));
        drift_size_.resize(static_cast<size_t>(num_bodies_), 0);
        drift_size_[static_cast<size_t>(body_index_1_based - 1)] = nq;
        have_time_ = false;  // the cached total belongs to the tables before
    }
    // The same on a heading grid (hc_set_drift_qtf_headings): beta [nh] rad, world frame, strictly increasing; P and Q
    // [6][nh][nh][nq][nq] row-major, element (d, a, b, m, n) = T(beta_a, beta_b, Omega_m, Omega_n).  The one kind of table that is
    // evaluated while wave directions are set (SetWaveDirections); it replaces a table set with SetDriftQTF, and the other way round.
    void SetDriftQTFHeadings(int body_index_1_based, const std::vector<double>& beta, const std::vector<double>& omega,
                             const std::vector<double>& P, const std::vector<double>& Q = {}) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetDriftQTFHeadings: body index out of range");
        const size_t nq = omega.size(), nh = beta.size(), n6 = 6 * nh * nh * nq * nq;
        if (P.size() != n6 || (!Q.empty() && Q.size() != n6))
            throw std::invalid_argument("SetDriftQTFHeadings: P and Q must hold 6 * nh * nh * nq * nq values");
        for (hc_ctx* c : ctxs_)
            check(c, hc_set_drift_qtf_headings(c, body_index_1_based - 1, static_cast<int>(nh), beta.data(), static_cast<int>(nq),
                                               nq ? omega.data() : nullptr, nq ? P.data() : nullptr, Q.empty() ? nullptr : Q.data()));
        drift_size_.resize(static_cast<size_t>(num_bodies_), 0);
        drift_size_[static_cast<size_t>(body_index_1_based - 1)] = nq;
        have_time_ = false;  // the cached total belongs to the tables before
    }
    // mean-drift coefficients D [6][nq]: a table with D on the diagonal and zeros elsewhere, for modes 1 and 2 (mode 3 needs a full
    // table: it would take the zeros off the diagonal as data)
    void SetMeanDriftCoefficients(int body_index_1_based, const std::vector<double>& omega, const std::vector<double>& D) {
        const size_t nq = omega.size();
        if (D.size() != 6 * nq) throw std::invalid_argument("SetMeanDriftCoefficients: D must hold 6 * nq values");
        std::vector<double> P(6 * nq * nq, 0.0);
        for (size_t d = 0; d < 6; ++d)
            for (size_t m = 0; m < nq; ++m) P[(d * nq + m) * nq + m] = D[d * nq + m];
        SetDriftQTF(body_index_1_based, omega, P);
    }
    // 0: off, 1: mean drift, 2: Newman's approximation, 3: full QTF
    void SetDriftMode(int mode) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_drift_mode(c, mode));
        drift_mode_ = mode;
        have_time_  = false;
    }
    // the phase of a regular wave as the drift term sees it (that of WaveBase::GetElevation & co.)
    void SetDriftOptions(double regular_phase = 0.0) {
        hc_wave_kinematics_opts o;
        hc_wave_kinematics_opts_default(&o);
        o.regular_phase = regular_phase;
        for (hc_ctx* c : ctxs_) check(c, hc_set_drift_options(c, &o));
        have_time_ = false;
    }
    // the drift term of all bodies for the bodies' present positions, 6 N values
    std::vector<double> ComputeForceDrift() {
        return compute_alone(kDrift);
    }

    // Second-order wave forces from sum-frequency QTF tables (not in the reference; include/hydrochrono_amd.h: hc_set_sum_qtf).
    // omega [nq] rad/s, a grid of its own, strictly increasing, P and Q [6][nq][nq] row-major (Q may be empty: zeros), force per
    // squared amplitude, dimensional; only the symmetric part of a table can contribute.  With SetSumMode(1) and at least one table
    // CoordinateFuncForBody returns total + sum-frequency term, added after the drift term.  The body index is 1-based; an empty
    // omega clears the table.
    void SetSumQTF(int body_index_1_based, const std::vector<double>& omega, const std::vector<double>& P, const std::vector<double>& Q = {}) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetSumQTF: body index out of range");
        const size_t nq = omega.size(), n6 = 6 * nq * nq;
        if (P.size() != n6 || (!Q.empty() && Q.size() != n6)) throw std::invalid_argument("SetSumQTF: P and Q must hold 6 * nq * nq values");
        for (hc_ctx* c : ctxs_)
            check(c, hc_set_sum_qtf(c, body_index_1_based - 1, static_cast<int>(nq), nq ? omega.data() : nullptr, nq ? P.data() : nullptr,
                                    Q.empty() ? nullptr : Q.data()));
        sum_size_.resize(static_cast<size_t>(num_bodies_), 0);
        sum_size_[static_cast<size_t>(body_index_1_based - 1)] = nq;
        have_time_ = false;  // the cached total belongs to the tables before
    }
    // The same on a heading grid (hc_set_sum_qtf_headings), as SetDriftQTFHeadings
    void SetSumQTFHeadings(int body_index_1_based, const std::vector<double>& beta, const std::vector<double>& omega,
                           const std::vector<double>& P, const std::vector<double>& Q = {}) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetSumQTFHeadings: body index out of range");
        const size_t nq = omega.size(), nh = beta.size(), n6 = 6 * nh * nh * nq * nq;
        if (P.size() != n6 || (!Q.empty() && Q.size() != n6))
            throw std::invalid_argument("SetSumQTFHeadings: P and Q must hold 6 * nh * nh * nq * nq values");
        for (hc_ctx* c : ctxs_)
            check(c, hc_set_sum_qtf_headings(c, body_index_1_based - 1, static_cast<int>(nh), beta.data(), static_cast<int>(nq),
                                             nq ? omega.data() : nullptr, nq ? P.data() : nullptr, Q.empty() ? nullptr : Q.data()));
        sum_size_.resize(static_cast<size_t>(num_bodies_), 0);
        sum_size_[static_cast<size_t>(body_index_1_based - 1)] = nq;
        have_time_ = false;  // the cached total belongs to the tables before
    }
    // 0: off, 1: on
    void SetSumMode(int mode) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_sum_mode(c, mode));
        sum_mode_  = mode;
        have_time_ = false;
    }
    // the phase of a regular wave as the sum-frequency term sees it (that of WaveBase::GetElevation & co.)
    void SetSumOptions(double regular_phase = 0.0) {
        hc_wave_kinematics_opts o;
        hc_wave_kinematics_opts_default(&o);
        o.regular_phase = regular_phase;
        for (hc_ctx* c : ctxs_) check(c, hc_set_sum_options(c, &o));
        have_time_ = false;
    }
    // the sum-frequency term of all bodies for the bodies' present positions, 6 N values
    std::vector<double> ComputeForceSumQTF() {
        return compute_alone(kSum);
    }

    // State-space radiation by modal recursion (not in the reference; include/hydrochrono_amd.h: hc_set_radiation_modes).  Once a body
    // carries modes, CoordinateFuncForBody returns total - modal radiation term: hc_radiation_modes_begin on every shard, the step,
    // hc_radiation_modes_end on every shard, one elementwise subtraction.  The term is independent of the convolution: what the file's
    // K gives is still in the total.  The body index is 1-based; an empty vector clears the list.
    void SetRadiationModes(int body_index_1_based, const std::vector<RadiationMode>& modes) {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range("SetRadiationModes: body index out of range");
        std::vector<hc_radiation_mode> raw(modes.size());
        for (size_t e = 0; e < modes.size(); ++e)
            raw[e] = hc_radiation_mode{modes[e].row, modes[e].col, modes[e].lambda.real(), modes[e].lambda.imag(), modes[e].rho.real(),
                                       modes[e].rho.imag()};
        for (hc_ctx* c : ctxs_) check(c, hc_set_radiation_modes(c, body_index_1_based - 1, raw.data(), static_cast<int>(raw.size())));
        radm_count_.resize(static_cast<size_t>(num_bodies_), 0);
        radm_count_[static_cast<size_t>(body_index_1_based - 1)] = raw.size();
        have_radm_ = std::any_of(radm_count_.begin(), radm_count_.end(), [](size_t n) { return n != 0; });
        have_time_ = false;  // the cached total belongs to the lists before
    }
    // snapshots kept for steps back in time (hc_set_radiation_modes_depth), and a fresh start of the modal state
    void SetRadiationModesDepth(int depth) {
        for (hc_ctx* c : ctxs_) check(c, hc_set_radiation_modes_depth(c, depth));
    }
    void ResetRadiationModes() {
        for (hc_ctx* c : ctxs_) check(c, hc_reset_radiation_modes(c));
        have_time_ = false;
    }
    // advances the modal state to the bodies' present time with their present velocities: the modal radiation term, 6 N values
    std::vector<double> ComputeForceRadiationModes() {
        return compute_alone(kRadm);
    }

    // the modal radiation term of the last CoordinateFuncForBody evaluation (zeros before the first one)
    std::vector<double> GetForceRadiationModes() const {
        std::vector<double> out(6 * static_cast<size_t>(num_bodies_), 0.0);
        if (have_radm_ && radm_force_.size() == out.size()) out = radm_force_;
        return out;
    }

    // src/hydro_forces.cpp:693-711: the radiation IRF value the convolution uses (rho-scaled; the processed kernel in
    // TaperedDirect mode).  Reads one value back from the GPU -- a debugging accessor, as in the reference.
    double GetRIRFval(int row, int col, int st) {
        double v = 0.0;
        const int b = row / 6;
        if (row < 0 || b >= num_bodies_) throw std::out_of_range("GetRIRFval: row index out of range");
        for (hc_ctx* c : ctxs_) {
            int b0 = 0, b1 = 0;
            check(c, hc_get_shard(c, &b0, &b1));
            if (b >= b0 && b < b1) check(c, hc_get_rirf_value(c, row - 6 * b0, col, st, &v));
        }
        return v;
    }

    // src/hydro_forces.cpp:727-767.  b is 1-based.  All 6N callbacks of one Chrono update share one evaluation.
    double CoordinateFuncForBody(int b, int dof_index) {
        if (dof_index < 0 || dof_index >= 6 || b < 1 || b > num_bodies_) throw std::out_of_range("Invalid index in CoordinateFuncForBody");
        const double t = bodies_[0]->GetChTime();
        if (!(have_time_ && t == prev_time_)) {
            have_time_ = false;  // an evaluation that throws leaves no total behind: the next call at this time evaluates again
            gather_state();
            // the side terms beside the step, in the order of side_terms(): begin all, step, end all, compose
            const auto terms = side_terms();
            for (size_t k = 0; k < terms.size(); ++k) {
                if (!terms[k].on) continue;
                try {
                    begin_all(terms[k], t);
                } catch (...) {  // nothing stays pending
                    for (size_t j = 0; j < k; ++j)
                        if (terms[j].on) drop(terms[j], ctxs_.size());
                    throw;
                }
            }
            const int rc = ctxs_.size() == 1 ? hc_step(ctx_, t, pos_.data(), rpy_.data(), lin_.data(), ang_.data(), total_force_.data())
                                             : hc_step_multi(ctxs_.data(), static_cast<int>(ctxs_.size()), t, pos_.data(), rpy_.data(), lin_.data(),
                                                             ang_.data(), total_force_.data());
            Failure failed;  // every term is ended whatever the step answered; the step's error goes first, then the first end's
            for (const SideTerm& s : terms) {
                if (!s.on) continue;
                std::vector<double>& x = this->*s.result;
                x.resize(s.nout * total_force_.size());
                const Failure f = end_all(s, x.data());
                if (!failed.ctx) failed = f;
            }
            check(ctx_, rc);
            if (failed.ctx) check(failed.ctx, failed.rc);
            for (const SideTerm& s : terms)
                if (s.on) compose(s);
            prev_time_ = t;
            have_time_ = true;
        }
        return total_force_[6 * static_cast<size_t>(b - 1) + dof_index];
    }

    // GPU seconds per term; the shards of a multi-GPU object run side by side, so the largest shard figure is reported
    HydroProfileStats GetProfileStats() const {
        HydroProfileStats s;
        for (hc_ctx* c : ctxs_) {
            hc_profile_stats p;
            check(c, hc_get_profile(c, &p));
            s.hydrostatics_seconds = std::max(s.hydrostatics_seconds, p.hydrostatics_seconds);
            s.radiation_seconds    = std::max(s.radiation_seconds, p.radiation_seconds);
            s.waves_seconds        = std::max(s.waves_seconds, p.waves_seconds);
            s.hydrostatics_calls   = p.hydrostatics_calls;
            s.radiation_calls      = p.radiation_calls;
            s.waves_calls          = p.waves_calls;
        }
        return s;
    }

    // ChLoadAddedMass data (src/chloadaddedmass.cpp)
    std::vector<double> GetAddedMassMatrix() const {
        const size_t D = static_cast<size_t>(6) * num_bodies_;
        std::vector<double> M(D * D);
        for (hc_ctx* c : ctxs_) check(c, hc_added_mass_matrix(c, M.data() + static_cast<size_t>(row0(c)) * D));  // each shard: its rows
        return M;
    }
    void AddedMassMv(double* R, const double* w, double c, int n_sys) const {
        if (ctxs_.size() == 1) check(ctx_, hc_added_mass_mv(ctx_, w, c, R, n_sys));
        else check(ctx_, hc_added_mass_mv_multi(ctxs_.data(), static_cast<int>(ctxs_.size()), w, c, R, n_sys));
    }

#ifdef HYDROCHRONO_AMD_WITH_CHRONO
    // the added-mass load the ChBody constructor put into the system (for ChLoadAddedMass::SetIncludeMorisonAddedMass)
    std::shared_ptr<ChLoadAddedMass> GetAddedMassLoad() const { return my_loadbodyinertia; }
#endif

    hc_ctx* context() const { return ctx_; }
    const std::vector<hc_ctx*>& contexts() const { return ctxs_; }
    int num_shards() const { return static_cast<int>(ctxs_.size()); }
    int body_number(int i) const { return body_numbers_[i]; }
    int num_bodies() const { return num_bodies_; }

  private:
    // file -> shard contexts -> waves; on failure nothing is left behind
    void create_contexts(const std::string& h5_file_name, std::shared_ptr<WaveBase> waves, const std::vector<int>& device_ids) {
        if (bodies_.empty()) throw std::runtime_error("TestHydro needs at least one body");
        if (device_ids.empty() || static_cast<int>(device_ids.size()) > num_bodies_)
            throw std::runtime_error("TestHydro: between one shard and one shard per body");
        const int G = static_cast<int>(device_ids.size()), base = num_bodies_ / G, extra = num_bodies_ % G;
        try {
            read_body_numbers();
            for (int g = 0; g < G; ++g) {
                const int b0 = g * base + (g < extra ? g : extra), b1 = b0 + base + (g < extra ? 1 : 0);
                hc_ctx* c = nullptr;
                if (hc_create_sharded(num_bodies_, b0, b1, device_ids[g], &c) != HC_OK) throw std::runtime_error(hc_last_error(nullptr));
                ctxs_.push_back(c);
                check(c, hc_load_bemio_h5(c, h5_file_name.c_str()));
                check(c, hc_finalize(c));
            }
            ctx_ = ctxs_[0];
            if (!waves) waves = std::make_shared<NoWave>(static_cast<unsigned>(num_bodies_));
            AddWaves(std::move(waves));
        } catch (...) {
            destroy_contexts();
            throw;
        }
        total_force_.assign(6 * static_cast<size_t>(num_bodies_), 0.0);
    }
    void destroy_contexts() {
        for (hc_ctx* c : ctxs_)
            if (c) hc_destroy(c);
        ctxs_.clear();
        ctx_ = nullptr;
    }
    // body numbers come from the names "body<k>", 1-based (ForceFunc6d ctor, src/hydro_forces.cpp:104-108)
    void read_body_numbers() {
        for (auto& b : bodies_) {
            std::string temp = b->GetName();
            body_numbers_.push_back(std::stoi(temp.erase(0, 4)));
        }
    }
    void gather_state() {
#ifdef HYDROCHRONO_AMD_WITH_CHRONO
        follow_system_gravity();
#endif
        const size_t n = static_cast<size_t>(3) * num_bodies_;
        pos_.resize(n); rpy_.resize(n); lin_.resize(n); ang_.resize(n);
        for (int b = 0; b < num_bodies_; ++b) {
            const auto p = bodies_[b]->GetPos(), r = bodies_[b]->GetCardanAnglesXYZ(), v = bodies_[b]->GetPosDt(),
                       w = bodies_[b]->GetAngVelParent();
            for (int k = 0; k < 3; ++k) {
                pos_[3 * b + k] = p[k]; rpy_[3 * b + k] = r[k]; lin_[3 * b + k] = v[k]; ang_[3 * b + k] = w[k];
            }
        }
    }
    // the 0-based index of a body a surface list is set on
    int surface_body(int body_index_1_based, const char* who) const {
        if (body_index_1_based < 1 || body_index_1_based > num_bodies_) throw std::out_of_range(std::string(who) + ": body index out of range");
        return body_index_1_based - 1;
    }
    // after either setter of a body's surface list (panels or clipped triangles: the body carries the one set last)
    void surface_list_set(int body, size_t n) {
        panel_count_.resize(static_cast<size_t>(num_bodies_), 0);
        panel_count_[static_cast<size_t>(body)] = n;
        have_time_ = false;  // the cached total belongs to the lists before
    }
    bool nonlinear_on() const {
        return nonlinear_mode_ != 0 && std::any_of(panel_count_.begin(), panel_count_.end(), [](size_t n) { return n != 0; });
    }
    bool drift_on() const {
        return drift_mode_ != 0 && std::any_of(drift_size_.begin(), drift_size_.end(), [](size_t n) { return n != 0; });
    }
    bool sum_on() const {
        return sum_mode_ != 0 && std::any_of(sum_size_.begin(), sum_size_.end(), [](size_t n) { return n != 0; });
    }
    // A term that runs on a lane of its own beside the step.  side_terms() lists them in the order of their begins, their ends and
    // their composition; a new term is one more row, its result vector and its "on" flag.
    struct SideTerm {
        bool on;      // takes part in CoordinateFuncForBody
        size_t nout;  // vectors of 6 N values the end fills, one behind the other in *result
        int (*begin)(const TestHydro&, hc_ctx*, double t);
        int (*end)(hc_ctx*, double* out, size_t D);  // out: the shard's first row of the first vector; the others follow D apart
        std::vector<double> TestHydro::*result;      // the term of the last evaluation
        int sign;                                    // +1: added to the total, -1: subtracted, 0: the per-body nonlinear composition
    };
    enum { kNonlinear, kMorison, kDrift, kSum, kRadm, kSideTerms };
    std::array<SideTerm, kSideTerms> side_terms() const {
        return {{{nonlinear_on(), 3, [](const TestHydro& h, hc_ctx* c, double t) { return hc_nonlinear_begin(c, t, h.pos_.data(), h.rpy_.data()); },
                  [](hc_ctx* c, double* o, size_t D) { return hc_nonlinear_end(c, o, o + D, o + 2 * D); }, &TestHydro::nonlinear_force_, 0},
                 {have_morison_, 1,
                  [](const TestHydro& h, hc_ctx* c, double t) {
                      return hc_morison_begin(c, t, h.pos_.data(), h.rpy_.data(), h.lin_.data(), h.ang_.data());
                  },
                  [](hc_ctx* c, double* o, size_t) { return hc_morison_end(c, o); }, &TestHydro::morison_force_, +1},
                 {drift_on(), 1, [](const TestHydro& h, hc_ctx* c, double t) { return hc_drift_begin(c, t, h.pos_.data()); },
                  [](hc_ctx* c, double* o, size_t) { return hc_drift_end(c, o); }, &TestHydro::drift_force_, +1},
                 {sum_on(), 1, [](const TestHydro& h, hc_ctx* c, double t) { return hc_sum_qtf_begin(c, t, h.pos_.data()); },
                  [](hc_ctx* c, double* o, size_t) { return hc_sum_qtf_end(c, o); }, &TestHydro::sum_force_, +1},
                 {have_radm_, 1,
                  [](const TestHydro& h, hc_ctx* c, double t) { return hc_radiation_modes_begin(c, t, h.lin_.data(), h.ang_.data()); },
                  [](hc_ctx* c, double* o, size_t) { return hc_radiation_modes_end(c, o); }, &TestHydro::radm_force_, -1}}};
    }
    struct Failure {
        hc_ctx* ctx = nullptr;
        int rc      = HC_OK;
    };
    // ends the term on the first n shards into a scratch buffer, whatever they answer: nothing stays pending
    void drop(const SideTerm& s, size_t n) {
        const size_t D = total_force_.size();
        std::vector<double> scratch(s.nout * D);
        for (size_t g = 0; g < n; ++g) (void)s.end(ctxs_[g], scratch.data() + row0(ctxs_[g]), D);
    }
    // begins the term on every shard; a refusal ends it on the shards before, and is thrown
    void begin_all(const SideTerm& s, double t) {
        for (size_t g = 0; g < ctxs_.size(); ++g) {
            const int rc = s.begin(*this, ctxs_[g], t);
            if (rc != HC_OK) {
                drop(s, g);
                check(ctxs_[g], rc);
            }
        }
    }
    // ends the term on every shard, each into its rows of out [nout][6 N]; the first failure is returned, not thrown
    Failure end_all(const SideTerm& s, double* out) {
        Failure first;
        for (hc_ctx* c : ctxs_) {
            const int rc = s.end(c, out + row0(c), total_force_.size());
            if (rc != HC_OK && !first.ctx) first = Failure{c, rc};
        }
        return first;
    }
    // a term for the bodies' present state, outside CoordinateFuncForBody: nout vectors of 6 N values
    std::vector<double> compute_alone(size_t k) {
        gather_state();
        const SideTerm s = side_terms()[k];
        std::vector<double> out(s.nout * total_force_.size());
        begin_all(s, bodies_[0]->GetChTime());
        const Failure f = end_all(s, out.data());
        if (f.ctx) check(f.ctx, f.rc);
        return out;
    }
    void compose(const SideTerm& s) {
        const std::vector<double>& x = this->*s.result;
        const size_t D = total_force_.size();
        if (s.sign > 0) {
            for (size_t i = 0; i < D; ++i) total_force_[i] += x[i];
        } else if (s.sign < 0) {
            for (size_t i = 0; i < D; ++i) total_force_[i] -= x[i];
        } else {  // total - hs_lin + buoy (+ fk in mode 2) on the rows of every body that carries a surface list
            const double *buoy = x.data(), *fk = buoy + D, *hs = fk + D;
            for (size_t body = 0; body < panel_count_.size(); ++body) {
                if (panel_count_[body] == 0) continue;
                for (size_t i = 6 * body; i < 6 * body + 6; ++i) {
                    total_force_[i] = total_force_[i] - hs[i] + buoy[i];
                    if (nonlinear_mode_ == 2) total_force_[i] = total_force_[i] + fk[i];
                }
            }
        }
    }
    static int row0(hc_ctx* c) {  // first output row of a shard context
        int b0 = 0;
        check(c, hc_get_shard(c, &b0, nullptr));
        return 6 * b0;
    }
    std::vector<std::shared_ptr<BodyView>> bodies_;
    int num_bodies_;
    std::vector<int> body_numbers_;
    std::vector<hc_ctx*> ctxs_;  // one per body-row shard (one = the single-GPU object)
    hc_ctx* ctx_ = nullptr;      // ctxs_[0]
    std::shared_ptr<WaveBase> user_waves_;
    std::vector<double> total_force_, pos_, rpy_, lin_, ang_;
    std::vector<double> morison_force_;  // the Morison term of the last evaluation
    std::vector<size_t> morison_count_;  // elements per body
    std::vector<size_t> morison_member_count_;  // strip members per body
    std::vector<bool> morison_member_ca_;       // per body: some member has an added-mass coefficient ca > 0
    hc_ctx* owner_of(int body_0_based, const char* who) {  // the shard context that owns a body
        for (hc_ctx* c : ctxs_) {
            int b0 = 0, b1 = 0;
            check(c, hc_get_shard(c, &b0, &b1));
            if (body_0_based >= b0 && body_0_based < b1) return c;
        }
        throw std::out_of_range(std::string(who) + ": no context owns the body");
    }
    bool have_morison_ = false;  // some body carries elements or members
    void update_have_morison() {
        const auto any = [](const std::vector<size_t>& v) { return std::any_of(v.begin(), v.end(), [](size_t n) { return n != 0; }); };
        have_morison_ = any(morison_count_) || any(morison_member_count_);
    }
    std::vector<double> nonlinear_force_;  // buoy | fk | hs_lin of the last evaluation
    std::vector<size_t> panel_count_;      // surface panels or triangles per body (a body carries one kind)
    int nonlinear_mode_ = 0;               // 0 off, 1 buoyancy, 2 buoyancy + Froude-Krylov
    std::vector<double> drift_force_;      // the drift term of the last evaluation
    std::vector<size_t> drift_size_;       // grid size of every body's drift table
    int drift_mode_ = 0;                   // 0 off, 1 mean drift, 2 Newman, 3 full QTF
    std::vector<double> sum_force_;        // the sum-frequency term of the last evaluation
    std::vector<size_t> sum_size_;         // grid size of every body's sum-frequency table
    int sum_mode_ = 0;                     // 0 off, 1 on
    std::vector<double> radm_force_;       // the modal radiation term of the last evaluation
    std::vector<size_t> radm_count_;       // radiation modes per body
    bool have_radm_ = false;
    std::array<double, 3> gravity_{0.0, 0.0, -9.81};
    bool have_time_   = false;
    double prev_time_ = -1.0;

#ifdef HYDROCHRONO_AMD_WITH_CHRONO
    static std::vector<std::shared_ptr<BodyView>> views_of(const std::vector<std::shared_ptr<chrono::ChBody>>& chbodies) {
        std::vector<std::shared_ptr<BodyView>> views;
        for (auto& b : chbodies) views.push_back(std::make_shared<ChronoBody>(b));
        return views;
    }
    // the reference asks the system for g at every evaluation (src/hydro_forces.cpp:267-269); a changed value reaches the contexts
    // before the next one (hc_set_gravity waits for the queue, so it is not called while nothing changes)
    void follow_system_gravity() {
        if (!system_) return;
        const auto g = system_->GetGravitationalAcceleration();
        if (g.x() != gravity_[0] || g.y() != gravity_[1] || g.z() != gravity_[2]) SetGravitationalAcceleration(g.x(), g.y(), g.z());
    }
    void wire_into_chrono();
    std::vector<std::shared_ptr<chrono::ChBody>> chbodies_;
    chrono::ChSystem* system_ = nullptr;
    std::vector<std::unique_ptr<ForceFunc6d>> force_per_body_;
    std::shared_ptr<chrono::ChLoadContainer> my_loadcontainer;
    std::shared_ptr<ChLoadAddedMass> my_loadbodyinertia;
#endif
};

}  // namespace hydroc_amd

#ifdef HYDROCHRONO_AMD_WITH_CHRONO
namespace hydroc_amd {

inline double ComponentFunc::GetVal(double) const { return base_ ? base_->CoordinateFunc(index_) : 0.0; }

inline ForceFunc6d::ForceFunc6d(std::shared_ptr<chrono::ChBody> object, TestHydro* all_hydro_forces_user)
    : body_(std::move(object)), all_hydro_forces_(all_hydro_forces_user) {
    std::string temp = body_->GetName();  // "body<k>" -> k
    b_num_           = std::stoi(temp.erase(0, 4));
    for (int i = 0; i < 6; ++i) force_ptrs_[i] = chrono_types::make_shared<ComponentFunc>(this, i);
    chrono_force_  = chrono_types::make_shared<chrono::ChForce>();
    chrono_torque_ = chrono_types::make_shared<chrono::ChForce>();
    chrono_force_->SetAlign(chrono::ChForce::AlignmentFrame::WORLD_DIR);
    chrono_torque_->SetAlign(chrono::ChForce::AlignmentFrame::WORLD_DIR);
    chrono_force_->SetName("hydroforce");
    chrono_torque_->SetName("hydrotorque");
    chrono_force_->SetF_x(force_ptrs_[0]);
    chrono_force_->SetF_y(force_ptrs_[1]);
    chrono_force_->SetF_z(force_ptrs_[2]);
    chrono_torque_->SetF_x(force_ptrs_[3]);
    chrono_torque_->SetF_y(force_ptrs_[4]);
    chrono_torque_->SetF_z(force_ptrs_[5]);
    chrono_torque_->SetMode(chrono::ChForce::ForceType::TORQUE);
    body_->AddForce(chrono_force_);
    body_->AddForce(chrono_torque_);
}

inline double ForceFunc6d::CoordinateFunc(int i) {
    if (i < 0 || i >= 6) return 0.0;  // the reference prints a message and returns 0 (src/hydro_forces.cpp:136-144)
    return all_hydro_forces_->CoordinateFuncForBody(b_num_, i);
}

// Round-3 name of "a TestHydro wired into a ChSystem", kept for callers written against it.
class ChronoHydroSystem {
  public:
    ChronoHydroSystem(std::vector<std::shared_ptr<chrono::ChBody>> bodies, const std::string& h5, std::shared_ptr<WaveBase> waves,
                      const std::vector<int>& device_ids = {0})
        : hydro_(std::move(bodies), h5, std::move(waves), device_ids) {}
    TestHydro& hydro() { return hydro_; }

  private:
    TestHydro hydro_;
};

}  // namespace hydroc_amd

#include "chloadaddedmass.h"  // ChLoadAddedMass and the part of TestHydro that creates it
#endif  // HYDROCHRONO_AMD_WITH_CHRONO
