// A reference-style caller with a drift QTF table through the C++ mirror: TestHydro over one MockBody in a regular wave, the table set
// with SetDriftQTF, the force read through CoordinateFuncForBody as Chrono's callbacks do.
//   usage: drift_caller <sphere.h5>
// Prints one line per step: t pos[3] rpy[3] linvel[3] angvel[3] total[6] drift[6] (%.17g), total = CoordinateFuncForBody (hydro +
// drift), drift = ComputeForceDrift at the same state.  The first 20 steps run mode 3 on the full table, the last 20 mode 2 on
// mean-drift coefficients.  Exit 3: a second read at the same time gave other bits; exit 4: mode 0 or a cleared table did not bring
// zeros back.
// Built with plain g++ by tests/test_drift_ref_cpu.py, run on the GPU by tests/test_gpu_drift.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;

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
        // the table of tests/test_gpu_drift.py: cpp_table()
        const int nq = 3;
        const std::vector<double> omega{1.5, 2.25, 3.0};
        std::vector<double> P(6 * nq * nq), Q(6 * nq * nq), D(6 * nq);
        for (int d = 0; d < 6; ++d)
            for (int m = 0; m < nq; ++m) {
                D[d * nq + m] = 2000.0 * (d + 1) + 125.0 * m;
                for (int n = 0; n < nq; ++n) {
                    P[(d * nq + m) * nq + n] = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n;
                    Q[(d * nq + m) * nq + n] = 500.0 * (m - n) + 62.5 * d;
                }
            }
        hydro_forces.SetDriftQTF(1, omega, P, Q);
        hydro_forces.SetDriftOptions(0.3);
        hydro_forces.SetDriftMode(3);
        const int steps = 40;
        for (int n = 0; n < steps; ++n) {
            if (n == 20) {
                hydro_forces.SetMeanDriftCoefficients(1, omega, D);
                hydro_forces.SetDriftMode(2);
            }
            const double t = 0.015 * n;
            body->time   = t;
            body->pos    = {0.1 * n * 0.015, 0.0, -2.0 + 0.004 * n};
            body->rpy    = {0.002 * n, -0.003 * n, 0.001 * n};
            body->linvel = {0.1, 0.0, 0.3 - 0.01 * n};
            body->angvel = {0.02, -0.03 + 0.001 * n, 0.01};
            double total[6];
            for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
            for (int k = 0; k < 6; ++k) {
                const double again = hydro_forces.CoordinateFuncForBody(1, k);
                if (std::memcmp(&again, &total[k], sizeof(double)) != 0) return 3;
            }
            const std::vector<double> drift = hydro_forces.ComputeForceDrift();
            std::printf("%.17g", t);
            for (const auto* v : {&body->pos, &body->rpy, &body->linvel, &body->angvel})
                for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", drift[k]);
            std::printf("\n");
        }
        // mode 0, then a cleared table: the drift term is zero
        hydro_forces.SetDriftMode(0);
        for (double v : hydro_forces.ComputeForceDrift())
            if (v != 0.0) return 4;
        hydro_forces.SetDriftMode(1);
        hydro_forces.SetDriftQTF(1, {}, {});
        for (double v : hydro_forces.ComputeForceDrift())
            if (v != 0.0) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "drift_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
