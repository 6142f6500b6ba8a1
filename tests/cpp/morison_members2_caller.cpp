// A reference-style caller with Morison strip members on the second-order sea through the C++ mirror: TestHydro over one MockBody in
// an irregular sea of 65 components, one element and three members, SetMorisonSecondOrder with SetMorisonMembersSecondOrder, the
// force read through CoordinateFuncForBody as Chrono's callbacks do.
//   usage: morison_members2_caller <sphere.h5>
// Prints one line per step: t pos[3] rpy[3] linvel[3] angvel[3] total[6] morison[6] members[3][6] node_eta2[16] (%.17g), total =
// CoordinateFuncForBody (hydro + elements + members), morison = ComputeForceMorison at the same state, members =
// GetMorisonMemberForces and node_eta2 = GetMorisonMemberIncrements after it.  Exit 3: a second read at the same time gave other
// bits; exit 5: an increment is not what WaveBase::GetSecondOrder* returns for the stored point, or a dry segment's point carries an
// increment (which segments are dry is worked out here from GetElevation and the stored eta2 at the nodes); exit 7: the column's foot
// is not wet or its top not dry; exit 6: without SetMorisonMembersSecondOrder the evaluation did not throw; exit 4: with second order off the members did
// not return to order 1.
// Built and run on the GPU by tests/test_gpu_morison_members2.py.
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
        auto body = std::make_shared<MockBody>("body1");
        std::vector<std::shared_ptr<BodyView>> bodies{body};
        TestHydro hydro_forces(bodies, argv[1]);
        hydro_forces.AddWaves(waves);
        std::vector<MorisonElement> elems(1);
        elems[0].r = {2.5, 0.5, -3.0};
        elems[0].cd_area = {1.0, 1.5, 0.5};
        elems[0].cm_vol = {2.0, 2.0, 1.0};
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
        hydro_forces.SetMorisonOptions(0.25, 0.0, true);
        hydro_forces.SetMorisonSecondOrder(true, 0.05, 0.9, 1.5, 6.0, true);
        body->time = 12.0;
        body->pos  = {0.0, 0.0, -2.0};
        bool refused = false;
        try {
            hydro_forces.ComputeForceMorison();
        } catch (const std::exception&) {
            refused = true;
        }
        if (!refused) return 6;
        hydro_forces.SetMorisonMembersSecondOrder(true);
        const size_t nodes = 9 + 6 + 2, points = 2 * (8 + 5 + 1);
        const int steps = 40;
        for (int n = 0; n < steps; ++n) {
            const double t = 0.015 * n + 12.0;  // inside the ramp of 20 s
            body->time   = t;
            body->pos    = {0.1 * n * 0.015, 0.0, -2.0 + 0.004 * n};
            body->rpy    = {0.002 * n, -0.003 * n, 0.001 * n};
            body->linvel = {0.1, 0.0, 0.3 - 0.01 * n};
            body->angvel = {0.02, -0.03 + 0.001 * n, 0.01};
            double total[6];
            for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
            for (int k = 0; k < 6; ++k)
                if (!same(hydro_forces.CoordinateFuncForBody(1, k), total[k])) return 3;
            const std::vector<double> mor     = hydro_forces.ComputeForceMorison();
            const auto per_member             = hydro_forces.GetMorisonMemberForces(1);
            const MorisonMemberIncrements inc = hydro_forces.GetMorisonMemberIncrements(1);
            if (inc.node_p.size() != nodes || inc.node_eta2.size() != nodes || inc.p.size() != points || inc.eta2.size() != points) return 5;
            std::vector<bool> node_wet(nodes);
            for (size_t j = 0; j < nodes; ++j) {
                if (!same(inc.node_eta2[j], waves->GetSecondOrderElevation(inc.node_p[j], t))) return 5;
                node_wet[j] = ((inc.node_p[j][2] - 0.25) - waves->GetElevation(inc.node_p[j], t)) - inc.node_eta2[j] <= 0.0;
            }
            // a segment is dry when both its nodes are: segment s of a member whose first node is n0 lies between nodes n0 + s, n0 + s + 1
            std::vector<bool> point_dry;
            size_t n0 = 0;
            for (int n_seg : {8, 5, 1}) {
                for (int s = 0; s < n_seg; ++s) {
                    const bool dry = !node_wet[n0 + s] && !node_wet[n0 + s + 1];
                    point_dry.push_back(dry);
                    point_dry.push_back(dry);
                }
                n0 += static_cast<size_t>(n_seg) + 1;
            }
            // the column's foot is wet, its top segment and the third member are dry: the inputs are what this file says they are
            if (point_dry[0] || !point_dry[2 * 7 + 1] || !point_dry[points - 1]) return 7;
            for (size_t e = 0; e < points; ++e) {
                const bool dry = point_dry[e];
                const std::array<double, 3> v = waves->GetSecondOrderVelocity(inc.p[e], t), a = waves->GetSecondOrderAcceleration(inc.p[e], t);
                bool ok = dry ? inc.eta2[e] == 0.0 : same(inc.eta2[e], waves->GetSecondOrderElevation(inc.p[e], t));
                for (int k = 0; k < 3; ++k)
                    ok = ok && (dry ? inc.vel2[e][k] == 0.0 && inc.acc2[e][k] == 0.0 : same(inc.vel2[e][k], v[k]) && same(inc.acc2[e][k], a[k]));
                if (!ok) return 5;
            }
            std::printf("%.17g", t);
            for (const auto* v : {&body->pos, &body->rpy, &body->linvel, &body->angvel})
                for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", mor[k]);
            for (const auto& m : per_member)
                for (int k = 0; k < 6; ++k) std::printf(" %.17g", m[k]);
            for (size_t j = 0; j < 16; ++j) std::printf(" %.17g", inc.node_eta2[j]);
            std::printf("\n");
        }
        // second order off: the term of order 1 again, whatever the members' switch says
        const std::vector<double> on = hydro_forces.ComputeForceMorison();
        hydro_forces.SetMorisonSecondOrder(false);
        const std::vector<double> off = hydro_forces.ComputeForceMorison();
        hydro_forces.SetMorisonMembersSecondOrder(false);
        const std::vector<double> off2 = hydro_forces.ComputeForceMorison();
        bool differs = false;
        for (size_t k = 0; k < 6; ++k) {
            differs = differs || !same(on[k], off[k]);
            if (!same(off[k], off2[k])) return 4;
        }
        if (!differs) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "morison_members2_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
