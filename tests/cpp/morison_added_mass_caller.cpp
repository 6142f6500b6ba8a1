// The strip members' added-mass matrix through the C++ mirror and ChLoadAddedMass, against the stand-in Chrono headers under
// tests/cpp/chrono_stub/ (test infrastructure): TestHydro over three ChBody on three_body.h5 in still water plus one body without
// hydrodynamics, members on bodies 1 and 3, SetMorisonMemberAddedMass on both (body 3: one member with ca = 0).
//   usage: morison_added_mass_caller <three_body.h5> [device list, e.g. 0,0,0  (default: 0)]
// Prints (hex doubles, %a) "BODY b" + 36 entries of GetMorisonAddedMass for b = 1..3, "MEMBER b m" + 36 entries of
// GetMorisonMemberAddedMass, and the states, so that the Python side repeats the evaluation through the C calls.
// Exit 3: with SetIncludeMorisonAddedMass(false) the Jacobian's M or R += c M w is not bitwise what it was before the members were
// set; exit 4: with it on, M is not the BEM matrix plus the blocks, entry by entry with one addition; exit 5: R += c M w with it on
// is not the product without the blocks plus c * (block times w), or differs between the host and the GPU product path by more than
// rounding; exit 6: the serial sum of the members' matrices is not the body's; exit 7: a getter answered before an evaluation with
// the coefficients, or SetMorisonMembers did not reset ca.
// Built by tests/test_morison_added_mass_ref_cpu.py, run on the GPU by tests/test_gpu_morison_added_mass.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#define HYDROCHRONO_AMD_WITH_CHRONO 1
#include "../../include/hydroc_amd/setup_hydro_from_yaml.h"

using namespace hydroc_amd;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static std::vector<MorisonMember> members(int body) {
    std::vector<MorisonMember> v(body == 0 ? 2 : 3);
    v[0].r0 = {0.5, 0.0, -6.0}, v[0].r1 = {0.5, 0.0, 2.0}, v[0].d0 = 1.25, v[0].d1 = 1.25, v[0].n_seg = 5;
    v[1].r0 = {-4.0, -3.0, -5.0}, v[1].r1 = {4.0, 3.0, 5.5}, v[1].d0 = 0.875, v[1].d1 = 0.375, v[1].n_seg = 3;
    if (body != 0) v[2].r0 = {1.0, 1.0, -7.0}, v[2].r1 = {1.5, 1.0, -2.0}, v[2].d0 = 0.75, v[2].d1 = 0.75, v[2].n_seg = 2;
    for (auto& m : v) m.cd = 1.0, m.cm = 2.0;
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<int> devices;
    {
        std::stringstream ss(argc > 2 ? argv[2] : "0");
        for (std::string tok; std::getline(ss, tok, ',');) devices.push_back(std::atoi(tok.c_str()));
    }
    using namespace chrono;
    try {
        ChSystem system;
        system.SetGravitationalAcceleration(ChVector3d(0, 0, -9.81));
        std::vector<std::shared_ptr<ChBody>> bodies;
        for (int b = 0; b < 3; ++b) {
            bodies.push_back(chrono_types::make_shared<ChBody>());
            bodies.back()->SetName("body" + std::to_string(b + 1));
            bodies.back()->pos = ChVector3d(15.0 * b + 0.25, 0.5 * b, -1.0 - 0.25 * b);
            system.AddBody(bodies.back());
        }
        auto ground = chrono_types::make_shared<ChBody>();
        ground->SetName("ground");
        system.AddBody(ground);
        TestHydro hydro(bodies, argv[1], std::make_shared<NoWave>(3), devices);
        auto load        = hydro.GetAddedMassLoad();
        const long n_sys = system.GetNumCoordsVelLevel();
        const int D      = 18;
        if (n_sys != 24) return 2;
        ChVectorDynamic<> w(n_sys), R0(n_sys);
        for (int i = 0; i < n_sys; ++i) w(i) = 0.25 * ((i * 7) % 11) - 1.0, R0(i) = 1.0 - 0.0625 * i;
        const auto product = [&](int limit) {
            ChVectorDynamic<> R = R0;
            load->SetHostProductLimit(limit);
            load->LoadIntLoadResidual_Mv(R, w, -0.5);
            load->SetHostProductLimit(ChLoadAddedMass::kHostProductMaxDofs);
            return R;
        };
        // ---- before any member: the BEM matrix and both product paths ----
        load->StubUpdate(n_sys);
        const ChMatrixDynamic<double> bem = load->m_jacobians->M;
        const ChVectorDynamic<> host0 = product(ChLoadAddedMass::kHostProductMaxDofs), gpu0 = product(0);

        hydro.SetMorisonMembers(1, members(0));
        hydro.SetMorisonMembers(3, members(2));
        hydro.SetMorisonMemberAddedMass(1, {1.0, 0.5});
        hydro.SetMorisonMemberAddedMass(3, {0.75, 0.0, 1.0});
        bool thrown = false;
        try {
            (void)hydro.GetMorisonAddedMass(1);  // no evaluation with these coefficients yet
        } catch (const std::exception&) {
            thrown = true;
        }
        if (!thrown) return 7;
        system.time = 0.5;
        (void)bodies[0]->forces[0]->Evaluate(system.time);  // the evaluation Chrono's force update makes

        // ---- off (the default): bitwise what it was ----
        load->StubUpdate(n_sys);
        for (int i = 0; i < n_sys; ++i)
            for (int j = 0; j < n_sys; ++j)
                if (!same_bits(load->m_jacobians->M(i, j), bem(i, j))) return 3;
        {
            const ChVectorDynamic<> a = product(ChLoadAddedMass::kHostProductMaxDofs), b = product(0);
            for (int i = 0; i < n_sys; ++i)
                if (!same_bits(a(i), host0(i)) || !same_bits(b(i), gpu0(i))) return 3;
        }
        // ---- on ----
        load->SetIncludeMorisonAddedMass(true);
        load->StubUpdate(n_sys);
        std::array<double, 36> blocks[3];
        for (int b = 0; b < 3; ++b) {
            blocks[b] = hydro.GetMorisonAddedMass(b + 1);
            std::printf("BODY %d", b + 1);
            for (double v : blocks[b]) std::printf(" %a", v);
            std::printf("\n");
            const auto rows = hydro.GetMorisonMemberAddedMass(b + 1);
            std::array<double, 36> acc{};
            for (size_t m = 0; m < rows.size(); ++m) {
                std::printf("MEMBER %d %zu", b + 1, m);
                for (size_t k = 0; k < 36; ++k) {
                    acc[k] = acc[k] + rows[m][k];
                    std::printf(" %a", rows[m][k]);
                }
                std::printf("\n");
            }
            for (size_t k = 0; k < 36; ++k)
                if (!same_bits(acc[k], blocks[b][k])) return 6;
        }
        for (double v : blocks[1])
            if (v != 0.0) return 4;  // body 2 carries no member
        for (int i = 0; i < n_sys; ++i)
            for (int j = 0; j < n_sys; ++j) {
                double want = bem(i, j);
                if (i < D && j < D && i / 6 == j / 6) want = want + blocks[i / 6][static_cast<size_t>(6 * (i % 6) + j % 6)];
                if (!same_bits(load->m_jacobians->M(i, j), want)) return 4;
            }
        if (!(blocks[0][0] > 1000.0) || !(blocks[2][0] > 100.0)) return 4;
        {
            const ChVectorDynamic<> a = product(ChLoadAddedMass::kHostProductMaxDofs), b = product(0);
            for (int i = 0; i < n_sys; ++i) {
                double s = 0.0, mag = 0.0;
                if (i < D)
                    for (int j = 0; j < 6; ++j) {
                        const double term = blocks[i / 6][static_cast<size_t>(6 * (i % 6) + j)] * w(6 * (i / 6) + j);
                        s += term, mag += std::fabs(term);
                    }
                // the blocks go in first, then the product path: R0 + c s + c (M w)_i against host0 = R0 + c (M w)_i
                const double tol = 8 * 2.220446049250313e-16 * (std::fabs(host0(i)) + std::fabs(R0(i)) + 0.5 * mag + 1.0);
                if (std::fabs(a(i) - (host0(i) + -0.5 * s)) > tol || std::fabs(b(i) - (gpu0(i) + -0.5 * s)) > tol) return 5;
                if (i < 6 && !(std::fabs(0.5 * s) > 1.0)) return 5;
                if (i >= D && (!same_bits(a(i), R0(i)) || !same_bits(b(i), R0(i)))) return 5;
            }
        }
        // ---- a new list starts with ca = 0: the body's block is zero without a further evaluation's help ----
        hydro.SetMorisonMembers(3, members(2));
        for (double v : hydro.GetMorisonAddedMass(3))
            if (v != 0.0) return 7;
        load->SetIncludeMorisonAddedMass(false);
        std::printf("STATE %a", system.time);
        for (int b = 0; b < 3; ++b) std::printf(" %a %a %a", bodies[b]->pos.x(), bodies[b]->pos.y(), bodies[b]->pos.z());
        std::printf("\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "morison_added_mass_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
