// All three side terms at once through the C++ mirror, on several bodies and several shards: TestHydro over four MockBody on
// four_body.h5 in irregular waves, surface panels on bodies 1 and 3, Morison elements on bodies 2 and 3, QTF tables on bodies 1 and 4,
// nonlinear mode 2, drift mode 3 (Newman, mode 2, from step 20 on), the force read through CoordinateFuncForBody as Chrono's callbacks do.
//   usage: side_terms_caller <four_body.h5> [device list, e.g. 0,0,0,0  (default: 0)]
// Prints one line per step (%.17g): t, pos rpy linvel angvel of the four bodies (48), the 24 totals of CoordinateFuncForBody,
// ComputeForceMorison (24), ComputeForceNonlinear (buoy | fk | hs_lin, 72), ComputeForceDrift (24).  The output does not depend on
// the device list.  The lists, tables and states are those of tests/side_terms_inputs.py (cpp_*: dyadic values, the same bits there).
// Exit 3: a second read at the same time gave other bits; exit 4: with every list and table cleared the total is not the plain
// total of a TestHydro that never carried one; exit 5: with a drift evaluation begun by hand on the last shard context
// CoordinateFuncForBody did not throw, or left an evaluation pending on some context, or ended the one begun by hand.
// Built with plain g++ by tests/test_side_terms_cpu.py, run on the GPU by tests/test_gpu_side_terms.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;

static std::vector<SurfacePanel> panels(int body, int n) {
    std::vector<SurfacePanel> v(n);
    for (int k = 0; k < n; ++k) {
        v[k].c = {-3.0 + 0.25 * ((k * 3 + body) % 25), -2.0 + 0.5 * ((k * 7) % 9), -4.0 + 0.125 * ((k * 11 + 5 * body) % 64)};
        v[k].s = {0.25 - 0.0625 * (k % 9), -0.5 + 0.125 * ((k * 5) % 8), 0.375 - 0.03125 * ((k * 3) % 23)};
    }
    return v;
}

static std::vector<MorisonElement> elements(int body, int n) {
    std::vector<MorisonElement> v(n);
    for (int k = 0; k < n; ++k) {
        v[k].r       = {-4.0 + 0.5 * ((k * 5 + body) % 17), -3.0 + 0.25 * ((k * 3) % 25), -6.0 + 0.125 * ((k * 13 + 7 * body) % 96)};
        v[k].cd_area = {0.5 + 0.125 * (k % 7), 0.25 * ((k * 3) % 5), 1.0 + 0.0625 * (k % 11)};
        v[k].cm_vol  = {0.5 * (k % 3), 1.5 + 0.25 * (k % 4), 0.125 * ((k * 7) % 13)};
    }
    return v;
}

static void set_table(TestHydro& hydro, int body, int nq, bool with_q) {
    std::vector<double> omega(nq), P(6 * nq * nq), Q(6 * nq * nq);
    for (int m = 0; m < nq; ++m) omega[m] = 0.75 + 0.3125 * m;
    for (int d = 0; d < 6; ++d)
        for (int m = 0; m < nq; ++m)
            for (int n = 0; n < nq; ++n) {
                P[(d * nq + m) * nq + n] = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n + 31.25 * body;
                Q[(d * nq + m) * nq + n] = 500.0 * (m - n) + 62.5 * d;
            }
    if (with_q) hydro.SetDriftQTF(body + 1, omega, P, Q);
    else hydro.SetDriftQTF(body + 1, omega, P);
}

static void set_state(std::vector<std::shared_ptr<MockBody>>& mock, int n) {
    for (int b = 0; b < 4; ++b) {
        mock[b]->time   = 2.0 + 0.015625 * n;
        mock[b]->pos    = {15.0 * b + 0.03125 * n, 0.5 * b, -1.0 - 0.25 * b + 0.0078125 * n};
        mock[b]->rpy    = {0.001953125 * n, -0.00390625 * n + 0.015625 * b, 0.0009765625 * n};
        mock[b]->linvel = {0.125, 0.03125 * b, 0.25 - 0.0078125 * n};
        mock[b]->angvel = {0.015625, -0.03125 + 0.0009765625 * n, 0.0078125 * (b + 1)};
    }
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <four_body.h5> [devices, e.g. 0,0,0,0]\n", argv[0]);
        return 2;
    }
    std::vector<int> devices;
    {
        std::stringstream ss(argc > 2 ? argv[2] : "0");
        for (std::string tok; std::getline(ss, tok, ',');) devices.push_back(std::atoi(tok.c_str()));
    }
    try {
        IrregularWaveParams p;  // THREE_IRREG of the Python tests
        p.num_bodies_          = 4;
        p.simulation_dt_       = 0.01;
        p.simulation_duration_ = 40.0;
        p.ramp_duration_       = 5.0;
        p.wave_height_         = 2.0;
        p.wave_period_         = 7.0;
        p.frequency_min_       = 0.05;
        p.frequency_max_       = 0.8;
        p.nfrequencies_        = 200;
        p.seed_                = 3;
        std::vector<std::shared_ptr<MockBody>> mock;
        std::vector<std::shared_ptr<BodyView>> bodies;
        for (int b = 0; b < 4; ++b) {
            mock.push_back(std::make_shared<MockBody>("body" + std::to_string(b + 1)));
            bodies.push_back(mock.back());
        }
        TestHydro hydro(bodies, argv[1], std::make_shared<IrregularWaves>(p), devices);
        TestHydro plain(bodies, argv[1], std::make_shared<IrregularWaves>(p), devices);  // never carries a list or a table
        hydro.SetSurfacePanels(1, panels(0, 70));
        hydro.SetSurfacePanels(3, panels(2, 12));
        hydro.SetMorisonElements(2, elements(1, 9));
        hydro.SetMorisonElements(3, elements(2, 40));
        set_table(hydro, 0, 9, true);
        set_table(hydro, 3, 5, false);
        hydro.SetNonlinearHydroOptions(0.125, 0.0, true);
        hydro.SetMorisonOptions(0.0625, 0.0, true);
        hydro.SetNonlinearHydroMode(2);
        hydro.SetDriftMode(3);
        const int steps = 40;
        std::vector<double> drop(24);
        for (int n = 0; n < steps; ++n) {
            if (n == 20) hydro.SetDriftMode(2);
            set_state(mock, n);
            if (n == 10) {
                // a drift evaluation begun by hand on the last shard: the next begin there is refused, the evaluation throws, and
                // every evaluation it had begun on any context has been ended
                hc_ctx* last = hydro.contexts().back();
                const std::vector<double> pos(12, 0.0);
                if (hc_drift_begin(last, mock[0]->time, pos.data()) != HC_OK) return 5;
                bool thrown = false;
                try {
                    (void)hydro.CoordinateFuncForBody(1, 0);
                } catch (const std::exception&) {
                    thrown = true;
                }
                if (!thrown) return 5;
                for (hc_ctx* c : hydro.contexts()) {
                    if (hc_nonlinear_end(c, nullptr, nullptr, nullptr) != HC_ERR_INVALID) return 5;
                    if (hc_morison_end(c, drop.data()) != HC_ERR_INVALID) return 5;
                    if (hc_drift_end(c, drop.data()) != (c == last ? HC_OK : HC_ERR_INVALID)) return 5;
                }
                // ... and the evaluation below, at the same time, is a whole one (its row is compared like every other)
            }
            double total[24];
            for (int b = 0; b < 4; ++b)
                for (int k = 0; k < 6; ++k) total[6 * b + k] = hydro.CoordinateFuncForBody(b + 1, k);
            for (int b = 0; b < 4; ++b)
                for (int k = 0; k < 6; ++k)
                    if (!same_bits(hydro.CoordinateFuncForBody(b + 1, k), total[6 * b + k])) return 3;
            (void)plain.CoordinateFuncForBody(1, 0);  // in step with hydro: the same history
            const std::vector<double> mor = hydro.ComputeForceMorison(), nl = hydro.ComputeForceNonlinear(), dft = hydro.ComputeForceDrift();
            std::printf("%.17g", mock[0]->time);
            for (int b = 0; b < 4; ++b)
                for (const auto* v : {&mock[b]->pos, &mock[b]->rpy, &mock[b]->linvel, &mock[b]->angvel})
                    for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (double v : total) std::printf(" %.17g", v);
            for (const auto* vec : {&mor, &nl, &dft})
                for (double v : *vec) std::printf(" %.17g", v);
            std::printf("\n");
        }
        // everything cleared: the plain total again, bit for bit
        for (int b = 1; b <= 4; ++b) {
            hydro.SetSurfacePanels(b, {});
            hydro.SetMorisonElements(b, {});
            hydro.SetDriftQTF(b, {}, {});
        }
        set_state(mock, steps);
        for (int b = 0; b < 4; ++b)
            for (int k = 0; k < 6; ++k)
                if (!same_bits(hydro.CoordinateFuncForBody(b + 1, k), plain.CoordinateFuncForBody(b + 1, k))) return 4;
        for (const auto& vec : {hydro.ComputeForceMorison(), hydro.ComputeForceDrift()})
            for (double v : vec)
                if (v != 0.0) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "side_terms_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
