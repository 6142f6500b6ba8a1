// A reference-style caller with QTF tables on a heading grid through the C++ mirror: TestHydro over one MockBody in a regular wave
// with a heading of 0.4 rad, the tables set with SetDriftQTFHeadings and SetSumQTFHeadings, the force read through
// CoordinateFuncForBody as Chrono's callbacks do.
//   usage: qtf_dir_caller <sphere.h5>
// Prints one line per step: t pos[3] rpy[3] linvel[3] angvel[3] total[6] drift[6] sum[6] (%.17g), total = CoordinateFuncForBody
// (hydro + drift + sum-frequency term), drift = ComputeForceDrift and sum = ComputeForceSumQTF at the same state.  Exit 3: a second
// read at the same time gave other bits; exit 4: a one-heading table in place of the drift table did not bring the refusal back;
// exit 5: cleared tables did not bring zeros back.
// Built with plain g++ by tests/test_qtf_dir_ref_cpu.py, run on the GPU by tests/test_gpu_qtf_dir.py.
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
        hydro_forces.SetWaveDirections({0.4});
        // the tables of tests/test_gpu_qtf_dir.py: cpp_tables()
        const int nh = 2, nq = 3;
        const std::vector<double> beta{0.0, 1.0}, omega{1.5, 2.25, 3.0};
        std::vector<double> P(6 * nh * nh * nq * nq), Q(P.size()), S(P.size());
        size_t e = 0;
        for (int d = 0; d < 6; ++d)
            for (int a = 0; a < nh; ++a)
                for (int b = 0; b < nh; ++b)
                    for (int m = 0; m < nq; ++m)
                        for (int n = 0; n < nq; ++n, ++e) {
                            P[e] = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n + 500.0 * a - 375.0 * b;
                            Q[e] = 500.0 * (m - n) + 62.5 * d + 31.25 * (a - b);
                            S[e] = 800.0 * (d + 1) - 100.0 * m - 50.0 * n + 25.0 * a * b;
                        }
        hydro_forces.SetDriftQTFHeadings(1, beta, omega, P, Q);
        hydro_forces.SetSumQTFHeadings(1, beta, omega, S);
        hydro_forces.SetDriftOptions(0.3);
        hydro_forces.SetSumOptions(0.3);
        hydro_forces.SetDriftMode(3);
        hydro_forces.SetSumMode(1);
        const int steps = 20;
        for (int n = 0; n < steps; ++n) {
            const double t = 0.015 * n;
            body->time   = t;
            body->pos    = {0.1 * n * 0.015, 0.5 - 0.02 * n, -2.0 + 0.004 * n};
            body->rpy    = {0.002 * n, -0.003 * n, 0.001 * n};
            body->linvel = {0.1, 0.0, 0.3 - 0.01 * n};
            body->angvel = {0.02, -0.03 + 0.001 * n, 0.01};
            double total[6];
            for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
            for (int k = 0; k < 6; ++k) {
                const double again = hydro_forces.CoordinateFuncForBody(1, k);
                if (std::memcmp(&again, &total[k], sizeof(double)) != 0) return 3;
            }
            const std::vector<double> drift = hydro_forces.ComputeForceDrift(), sum = hydro_forces.ComputeForceSumQTF();
            std::printf("%.17g", t);
            for (const auto* v : {&body->pos, &body->rpy, &body->linvel, &body->angvel})
                for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", drift[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", sum[k]);
            std::printf("\n");
        }
        // a one-heading table replaces the heading table: refused again while the heading is set
        hydro_forces.SetDriftQTF(1, omega, std::vector<double>(6 * nq * nq, 1.0));
        bool refused = false;
        try {
            (void)hydro_forces.ComputeForceDrift();
        } catch (const std::exception&) {
            refused = true;
        }
        if (!refused) return 4;
        hydro_forces.SetDriftQTFHeadings(1, {}, {}, {});
        hydro_forces.SetSumQTFHeadings(1, {}, {}, {});
        for (double v : hydro_forces.ComputeForceDrift())
            if (v != 0.0) return 5;
        for (double v : hydro_forces.ComputeForceSumQTF())
            if (v != 0.0) return 5;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "qtf_dir_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
