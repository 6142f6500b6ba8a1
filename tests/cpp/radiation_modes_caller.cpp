// A reference-style caller with radiation modes through the C++ mirror: TestHydro over one MockBody in a regular wave, modes set with
// SetRadiationModes, the force read through CoordinateFuncForBody as Chrono's callbacks do -- on a step that is NOT uniform.
//   usage: radiation_modes_caller <sphere.h5>
// Prints one line per step: t linvel[3] angvel[3] pos[3] rpy[3] total[6] modal[6] (%.17g), total = CoordinateFuncForBody (hydro - modal
// term), modal = GetForceRadiationModes of that evaluation.  After the steps: one step back in time, one line more, and a line
// "standalone" from ComputeForceRadiationModes on a reset state.  Exit 3: a second read at the same time gave other bits; exit 4:
// clearing the modes did not bring the plain total back; exit 5: a duplicate time through ComputeForceRadiationModes did not throw.
// Built with plain g++ by tests/test_radiation_modes_ref_cpu.py, run on the GPU by tests/test_gpu_radiation_modes.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;

static void set_state(MockBody& body, double t, int n) {
    body.time   = t;
    body.pos    = {0.05 * t, 0.0, -2.0 + 0.1 * t};
    body.rpy    = {0.01 * t, -0.02 * t, 0.005 * t};
    body.linvel = {0.1 + 0.3 * t, -0.05 * n, 0.3 - 0.2 * t};
    body.angvel = {0.02, -0.03 + 0.01 * t, 0.01 * n};
}

static void print_line(double t, const MockBody& body, const double* total, const std::vector<double>& modal) {
    std::printf("%.17g", t);
    for (const auto* v : {&body.linvel, &body.angvel, &body.pos, &body.rpy})
        for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
    for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
    for (int k = 0; k < 6; ++k) std::printf(" %.17g", modal[k]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <sphere.h5>\n", argv[0]);
        return 2;
    }
    try {
        auto w                     = std::make_shared<RegularWave>(1);
        w->regular_wave_amplitude_ = 0.177;
        w->regular_wave_omega_     = 2.094395102;
        auto body                  = std::make_shared<MockBody>("body1");
        std::vector<std::shared_ptr<BodyView>> bodies{body};
        TestHydro hydro_forces(bodies, argv[1]);
        hydro_forces.AddWaves(w);
        std::vector<RadiationMode> modes(4);
        modes[0] = RadiationMode{2, 2, {-0.9, 0.0}, {30.0, 0.0}};
        modes[1] = RadiationMode{2, 2, {-0.3, 2.1}, {12.0, -4.0}};
        modes[2] = RadiationMode{0, 4, {-1.2, 0.7}, {-3.0, 1.5}};
        modes[3] = RadiationMode{4, 0, {-1.2, 0.7}, {-3.0, 1.5}};
        hydro_forces.SetRadiationModes(1, modes);
        double t = 0.0;
        double total[6];
        for (int n = 0; n < 30; ++n) {
            t += (n % 3 == 0) ? 0.004 : (n % 3 == 1 ? 0.031 : 0.0125);
            set_state(*body, t, n);
            for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
            for (int k = 0; k < 6; ++k) {
                const double again = hydro_forces.CoordinateFuncForBody(1, k);
                if (std::memcmp(&again, &total[k], sizeof(double)) != 0) return 3;
            }
            print_line(t, *body, total, hydro_forces.GetForceRadiationModes());
        }
        // a rejected step: back by less than the last step
        t -= 0.007;
        set_state(*body, t, 30);
        for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
        print_line(t, *body, total, hydro_forces.GetForceRadiationModes());
        // the term on its own, from a fresh state: zeros at the first time, then one step
        hydro_forces.ResetRadiationModes();
        set_state(*body, 1.0, 0);
        for (double v : hydro_forces.ComputeForceRadiationModes())
            if (v != 0.0) return 4;
        bool threw = false;
        try {
            (void)hydro_forces.ComputeForceRadiationModes();
        } catch (const std::exception&) {
            threw = true;
        }
        if (!threw) return 5;
        set_state(*body, 1.25, 1);
        const std::vector<double> alone = hydro_forces.ComputeForceRadiationModes();
        std::printf("standalone");
        for (double v : alone) std::printf(" %.17g", v);
        std::printf("\n");
        // cleared: the modal term is zero
        hydro_forces.SetRadiationModes(1, {});
        for (double v : hydro_forces.ComputeForceRadiationModes())
            if (v != 0.0) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "radiation_modes_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
