// A reference-style caller with Morison strip members through the C++ mirror: TestHydro over one MockBody in a regular wave, two
// elements set with SetMorisonElements and three members with SetMorisonMembers, the force read through CoordinateFuncForBody.
//   usage: morison_members_caller <sphere.h5>
// Prints one line per step: t pos[3] rpy[3] linvel[3] angvel[3] total[6] morison[6] members[3][6] (%.17g), total =
// CoordinateFuncForBody (hydro + elements + members), morison = ComputeForceMorison at the same state, members =
// GetMorisonMemberForces after it.  Exit 3: a second read at the same time gave other bits; exit 4: clearing both lists did not
// bring a zero Morison term back.
// Built and run on the GPU by tests/test_gpu_morison_members.py.
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
        std::vector<MorisonElement> elems(2);
        elems[0].r = {0.0, 0.0, -6.0};
        elems[0].cd_area = {3.0, 3.0, 12.0};
        elems[1].r = {2.5, 0.5, -3.0};
        elems[1].cd_area = {1.0, 1.5, 0.5};
        elems[1].cm_vol = {2.0, 2.0, 1.0};
        hydro_forces.SetMorisonElements(1, elems);
        std::vector<MorisonMember> members(3);
        members[0].r0 = {0.0, 0.0, -5.0};  // a surface-piercing column
        members[0].r1 = {0.0, 0.0, 6.0};
        members[0].d0 = members[0].d1 = 1.2;
        members[0].cd = 1.0, members[0].cm = 2.0, members[0].n_seg = 8;
        members[1].r0 = {-3.0, -3.0, -4.0};  // a tapered cross brace
        members[1].r1 = {3.0, 3.0, 1.5};
        members[1].d0 = 0.8, members[1].d1 = 0.4;
        members[1].cd = 0.9, members[1].cm = 1.6, members[1].n_seg = 5;
        members[2].r0 = {1.0, 0.0, 8.0};  // dry
        members[2].r1 = {4.0, 0.0, 9.0};
        members[2].d0 = members[2].d1 = 0.5;
        members[2].cd = 1.0, members[2].cm = 2.0, members[2].n_seg = 1;
        hydro_forces.SetMorisonMembers(1, members);
        hydro_forces.SetMorisonOptions(0.25, 0.3, true);
        const int steps = 40;
        for (int n = 0; n < steps; ++n) {
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
            const std::vector<double> mor = hydro_forces.ComputeForceMorison();
            const auto per_member         = hydro_forces.GetMorisonMemberForces(1);
            std::printf("%.17g", t);
            for (const auto* v : {&body->pos, &body->rpy, &body->linvel, &body->angvel})
                for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", mor[k]);
            for (const auto& m : per_member)
                for (int k = 0; k < 6; ++k) std::printf(" %.17g", m[k]);
            std::printf("\n");
        }
        // both lists cleared: the Morison term is zero again
        hydro_forces.SetMorisonElements(1, {});
        hydro_forces.SetMorisonMembers(1, {});
        for (double v : hydro_forces.ComputeForceMorison())
            if (v != 0.0) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "morison_members_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
