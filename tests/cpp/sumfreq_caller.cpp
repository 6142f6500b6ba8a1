// A reference-style caller with a sum-frequency QTF table through the C++ mirror: TestHydro over three MockBodies in a regular wave,
// the tables set with SetSumQTF (and a drift table beside them), the force read through CoordinateFuncForBody as Chrono's callbacks do.
//   usage: sumfreq_caller <three_body.h5> <shards>
// Prints one line per step: t, then pos[3] rpy[3] linvel[3] angvel[3] per body, total[18], sum[18] (%.17g), total =
// CoordinateFuncForBody (hydro + drift + sum-frequency term), sum = ComputeForceSumQTF at the same state.  Exit 3: a second read at the
// same time gave other bits; exit 4: mode 0 or a cleared table did not bring zeros back.
// Built with plain g++ by tests/test_sumfreq_ref_cpu.py, run on the GPU by tests/test_gpu_sumfreq.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <file.h5> <shards>\n", argv[0]);
        return 2;
    }
    try {
        const int N = 3, shards = std::atoi(argv[2]);
        auto w                     = std::make_shared<RegularWave>(N);
        w->regular_wave_amplitude_ = 0.177;
        w->regular_wave_omega_     = 0.6;
        std::vector<std::shared_ptr<MockBody>> mocks;
        std::vector<std::shared_ptr<BodyView>> bodies;
        for (int b = 0; b < N; ++b) {
            mocks.push_back(std::make_shared<MockBody>("body" + std::to_string(b + 1)));
            bodies.push_back(mocks.back());
        }
        TestHydro hydro_forces(bodies, argv[1], w, std::vector<int>(static_cast<size_t>(shards), 0));
        // the tables of tests/test_gpu_sumfreq.py: cpp_table()
        const int nq = 3;
        const std::vector<double> omega{0.4, 0.55, 0.9};
        std::vector<double> P(6 * nq * nq), Q(6 * nq * nq), P3(6 * nq * nq);
        for (int d = 0; d < 6; ++d)
            for (int m = 0; m < nq; ++m)
                for (int n = 0; n < nq; ++n) {
                    P[(d * nq + m) * nq + n]  = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n;
                    Q[(d * nq + m) * nq + n]  = 500.0 * (m + n) + 62.5 * d;
                    P3[(d * nq + m) * nq + n] = -750.0 * (d + 1) + 50.0 * m * n;
                }
        hydro_forces.SetSumQTF(1, omega, P, Q);
        hydro_forces.SetSumQTF(3, omega, P3);  // body 2 has no table
        hydro_forces.SetSumOptions(0.3);
        hydro_forces.SetSumMode(1);
        hydro_forces.SetDriftQTF(2, omega, P);  // the drift term beside it
        hydro_forces.SetDriftOptions(0.3);
        hydro_forces.SetDriftMode(3);
        const int steps = 24;
        for (int n = 0; n < steps; ++n) {
            const double t = 0.015 * n;
            for (int b = 0; b < N; ++b) {
                MockBody& body = *mocks[b];
                body.time      = t;
                body.pos       = {15.0 * b + 0.1 * n * 0.015, 0.0, -2.0 + 0.004 * n};
                body.rpy       = {0.002 * n, -0.003 * n, 0.001 * (n + b)};
                body.linvel    = {0.1, 0.0, 0.3 - 0.01 * n};
                body.angvel    = {0.02, -0.03 + 0.001 * n, 0.01};
            }
            double total[18];
            for (int b = 0; b < N; ++b)
                for (int k = 0; k < 6; ++k) total[6 * b + k] = hydro_forces.CoordinateFuncForBody(b + 1, k);
            for (int b = 0; b < N; ++b)
                for (int k = 0; k < 6; ++k) {
                    const double again = hydro_forces.CoordinateFuncForBody(b + 1, k);
                    if (std::memcmp(&again, &total[6 * b + k], sizeof(double)) != 0) return 3;
                }
            const std::vector<double> sum = hydro_forces.ComputeForceSumQTF();
            std::printf("%.17g", t);
            for (int b = 0; b < N; ++b)
                for (const auto* v : {&mocks[b]->pos, &mocks[b]->rpy, &mocks[b]->linvel, &mocks[b]->angvel})
                    for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 18; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 18; ++k) std::printf(" %.17g", sum[k]);
            std::printf("\n");
        }
        // mode 0, then cleared tables: the term is zero
        hydro_forces.SetSumMode(0);
        for (double v : hydro_forces.ComputeForceSumQTF())
            if (v != 0.0) return 4;
        hydro_forces.SetSumMode(1);
        hydro_forces.SetSumQTF(1, {}, {});
        hydro_forces.SetSumQTF(3, {}, {});
        for (double v : hydro_forces.ComputeForceSumQTF())
            if (v != 0.0) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sumfreq_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
