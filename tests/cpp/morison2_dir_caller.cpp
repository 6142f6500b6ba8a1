// A reference-style caller with Morison elements on the second-order sea under a wave heading through the C++ mirror: TestHydro over
// one MockBody in an irregular sea whose 65 components all travel at -0.4 rad (WaveBase::wave_directions_, applied by AddWaves),
// elements set with SetMorisonElements, second order switched on with SetMorisonSecondOrder and its directional form with
// SetMorisonSecondOrderDirectional, the force read through CoordinateFuncForBody as Chrono's callbacks do.
//   usage: morison2_dir_caller <sphere.h5>
// Prints one line per step: t pos[3] rpy[3] linvel[3] angvel[3] total[6] morison[6] eta2[3] vel2y[3] (%.17g), total =
// CoordinateFuncForBody (hydro + Morison), morison = ComputeForceMorison at the same state, eta2 and vel2y = GetMorisonIncrements of
// the three elements.  Exit 3: a second read at the same time gave other bits; exit 4: switching second order off did not change
// the term; exit 5: the increments are not those of the wave object's GetDirectionalSecondOrder* at the reported points; exit 6:
// the evaluation did not refuse while the directional switch was off; exit 7: the switch did not survive second order off and on.
// Built with plain g++ and run on the GPU by tests/test_gpu_morison2_dir.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;

namespace {
bool same(double u, double v) { return std::memcmp(&u, &v, sizeof(double)) == 0; }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <sphere.h5>\n", argv[0]);
        return 2;
    }
    try {
        IrregularWaveParams p;
        p.num_bodies_          = 1;
        p.simulation_dt_       = 0.015;
        p.simulation_duration_ = 60.0;
        p.ramp_duration_       = 20.0;
        p.wave_height_         = 2.0;
        p.wave_period_         = 12.0;
        p.frequency_min_       = 0.02;
        p.frequency_max_       = 1.0;
        p.nfrequencies_        = 65;
        p.seed_                = 2;
        auto waves             = std::make_shared<IrregularWaves>(p);
        waves->mwl_            = 0.25;
        waves->second_order_.diff_lo = 0.05;
        waves->second_order_.diff_hi = 0.9;
        waves->second_order_.sum_lo  = 1.5;
        waves->second_order_.sum_hi  = 6.0;
        waves->wave_directions_.assign(65, -0.4);
        auto body = std::make_shared<MockBody>("body1");
        std::vector<std::shared_ptr<BodyView>> bodies{body};
        TestHydro hydro_forces(bodies, argv[1]);
        hydro_forces.AddWaves(waves);
        std::vector<MorisonElement> elems(3);
        elems[0].r = {0.0, 0.0, -6.0};
        elems[0].cd_area = {3.0, 3.0, 12.0};
        elems[1].r = {2.5, 0.5, -3.0};
        elems[1].cd_area = {1.0, 1.5, 0.5};
        elems[1].cm_vol = {2.0, 2.0, 1.0};
        elems[2].r = {0.0, 0.0, 9.0};  // dry
        elems[2].cd_area = {5.0, 5.0, 5.0};
        hydro_forces.SetMorisonElements(1, elems);
        hydro_forces.SetMorisonOptions(0.25, 0.0, true);
        hydro_forces.SetMorisonSecondOrder(true, 0.05, 0.9, 1.5, 6.0, true);
        body->time = 12.0;
        body->pos  = {0.0, 0.0, -2.0};
        try {  // the directional switch is off: the evaluation refuses
            hydro_forces.ComputeForceMorison();
            return 6;
        } catch (const std::runtime_error&) {
        }
        hydro_forces.SetMorisonSecondOrderDirectional(true);
        const int steps = 40;
        for (int n = 0; n < steps; ++n) {
            const double t = 0.015 * n + 12.0;  // inside the ramp of 20 s
            body->time   = t;
            body->pos    = {0.1 * n * 0.015, 0.3, -2.0 + 0.004 * n};
            body->rpy    = {0.002 * n, -0.003 * n, 0.001 * n};
            body->linvel = {0.1, -0.05, 0.3 - 0.01 * n};
            body->angvel = {0.02, -0.03 + 0.001 * n, 0.01};
            double total[6];
            for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
            for (int k = 0; k < 6; ++k)
                if (!same(hydro_forces.CoordinateFuncForBody(1, k), total[k])) return 3;
            const std::vector<double> mor = hydro_forces.ComputeForceMorison();
            const MorisonIncrements inc   = hydro_forces.GetMorisonIncrements(1);
            if (inc.p.size() != 3 || inc.eta2.size() != 3) return 5;
            for (size_t e = 0; e < 3; ++e) {
                const std::array<double, 3> v = waves->GetDirectionalSecondOrderVelocity(inc.p[e], t);
                const std::array<double, 3> a = waves->GetDirectionalSecondOrderAcceleration(inc.p[e], t);
                bool ok = same(inc.eta2[e], waves->GetDirectionalSecondOrderElevation(inc.p[e], t));
                for (int k = 0; k < 3; ++k) ok = ok && same(inc.vel2[e][k], v[k]) && same(inc.acc2[e][k], a[k]);
                if (!ok) return 5;
            }
            std::printf("%.17g", t);
            for (const auto* v : {&body->pos, &body->rpy, &body->linvel, &body->angvel})
                for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", mor[k]);
            for (int e = 0; e < 3; ++e) std::printf(" %.17g", inc.eta2[e]);
            for (int e = 0; e < 3; ++e) std::printf(" %.17g", inc.vel2[e][1]);
            std::printf("\n");
        }
        // second order off: the directional term of order 1 again; on again: the directional switch has kept its value
        const std::vector<double> on = hydro_forces.ComputeForceMorison();
        hydro_forces.SetMorisonSecondOrder(false);
        const std::vector<double> off = hydro_forces.ComputeForceMorison();
        if (same(on[0], off[0]) && same(on[1], off[1])) return 4;
        hydro_forces.SetMorisonSecondOrder(true, 0.05, 0.9, 1.5, 6.0, true);
        const std::vector<double> again = hydro_forces.ComputeForceMorison();
        for (int k = 0; k < 6; ++k)
            if (!same(again[k], on[k])) return 7;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "morison2_dir_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
