// All four side terms at once through the C++ mirror under a wave heading, on several bodies and several shards: TestHydro over four
// MockBody on four_body.h5, excitation tables on a heading grid on every body (SetExcitationRAOHeadings), a clipped box on body 1 and
// surface panels on body 3, Morison elements on bodies 2 and 3, drift tables on heading grids on bodies 1 and 4
// (SetDriftQTFHeadings), sum-frequency tables on heading grids on bodies 2 and 3 (SetSumQTFHeadings), nonlinear mode 2, drift mode 3,
// sum mode 1.  Steps 0 .. 11 run in irregular waves (IrregularWaves is the IRF model: a uniform heading), steps 12 .. 23 in a regular
// wave, whose excitation coefficients follow the heading tables; the heading is 0.25 rad and changes to -0.5 rad at steps 6 and 18
// (SetWaveDirections).  The force is read through CoordinateFuncForBody as Chrono's callbacks do.
//   usage: side_terms_dir_caller <four_body.h5> [device list, e.g. 0,0,0,0  (default: 0)]
// Prints one line per step (hex doubles, %a): t, pos rpy linvel angvel of the four bodies (48), the 24 totals of
// CoordinateFuncForBody, ComputeForceMorison (24), ComputeForceNonlinear (buoy | fk | hs_lin, 72), ComputeForceDrift (24),
// ComputeForceSumQTF (24).  The output does not depend on the device list.  The lists, tables and states are those of
// tests/side_terms_dir_inputs.py (cpp_*: dyadic values, the same bits there).
// Exit 3: a second read at the same time gave other bits; exit 4: GetWaveDirections does not return what was set.
// Built with plain g++ by tests/test_side_terms_dir_cpu.py, run on the GPU by tests/test_gpu_side_terms_dir.py.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;
using Tri = std::array<std::array<double, 3>, 3>;

static std::vector<SurfacePanel> panels(int body, int n) {
    std::vector<SurfacePanel> v(n);
    for (int k = 0; k < n; ++k) {
        v[k].c = {-3.0 + 0.25 * ((k * 3 + body) % 25), -2.0 + 0.5 * ((k * 7) % 9), -4.0 + 0.125 * ((k * 11 + 5 * body) % 64)};
        v[k].s = {0.25 - 0.0625 * (k % 9), -0.5 + 0.125 * ((k * 5) % 8), 0.375 - 0.03125 * ((k * 3) % 23)};
    }
    return v;
}

// the twelve triangles of the box [-a, a] x [-b, b] x [z0, z1], normals outward (tests/cpp/side_terms2_caller.cpp)
static std::vector<Tri> box(double a, double b, double z0, double z1) {
    const double x[2] = {-a, a}, y[2] = {-b, b}, z[2] = {z0, z1};
    auto v = [&](int i, int j, int k) { return std::array<double, 3>{x[i], y[j], z[k]}; };
    std::vector<Tri> t;
    auto quad = [&](std::array<double, 3> p0, std::array<double, 3> p1, std::array<double, 3> p2, std::array<double, 3> p3) {
        t.push_back({p0, p1, p2});
        t.push_back({p0, p2, p3});
    };
    quad(v(0, 0, 0), v(0, 1, 0), v(1, 1, 0), v(1, 0, 0));  // bottom, -z
    quad(v(0, 0, 1), v(1, 0, 1), v(1, 1, 1), v(0, 1, 1));  // top, +z
    quad(v(0, 0, 0), v(1, 0, 0), v(1, 0, 1), v(0, 0, 1));  // -y
    quad(v(0, 1, 0), v(0, 1, 1), v(1, 1, 1), v(1, 1, 0));  // +y
    quad(v(0, 0, 0), v(0, 0, 1), v(0, 1, 1), v(0, 1, 0));  // -x
    quad(v(1, 0, 0), v(1, 1, 0), v(1, 1, 1), v(1, 0, 1));  // +x
    return t;
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

// cpp_heading_table: three headings -0.75, 0, 0.5; the drift tables on 0.75 + 0.3125 m rad/s, the sum tables (sum = true) on
// 0.625 + 0.28125 m
static void set_table(TestHydro& hydro, int body, int nq, bool with_q, bool sum) {
    const int nh = 3;
    const std::vector<double> beta{-0.75, 0.0, 0.5};
    std::vector<double> omega(nq), P(static_cast<size_t>(6) * nh * nh * nq * nq), Q(P.size());
    for (int m = 0; m < nq; ++m) omega[m] = sum ? 0.625 + 0.28125 * m : 0.75 + 0.3125 * m;
    size_t e = 0;
    for (int d = 0; d < 6; ++d)
        for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nh; ++b)
                for (int m = 0; m < nq; ++m)
                    for (int n = 0; n < nq; ++n, ++e) {
                        P[e] = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n + 31.25 * body + 500.0 * a - 375.0 * b;
                        Q[e] = 500.0 * (m - n) + 62.5 * d + 93.75 * (a - b);
                    }
    if (!with_q) Q.clear();
    if (sum) hydro.SetSumQTFHeadings(body + 1, beta, omega, P, Q);
    else hydro.SetDriftQTFHeadings(body + 1, beta, omega, P, Q);
}

// cpp_excitation_headings: {6, 3, 16} tables on w = 0.25 (j + 1), another table at every heading
static void set_excitation(TestHydro& hydro, int body) {
    const int nd = 3, nw = 16;
    const std::vector<double> dirs{-1.0, 0.0, 1.0};
    std::vector<double> w(nw), mag(6 * nd * nw), ph(6 * nd * nw);
    for (int j = 0; j < nw; ++j) w[j] = 0.25 * (j + 1);
    for (int r = 0; r < 6; ++r)
        for (int d = 0; d < nd; ++d)
            for (int j = 0; j < nw; ++j) {
                mag[(r * nd + d) * nw + j] = 0.5 + 0.125 * r + 0.25 * d + 0.0625 * j + 0.03125 * body;
                ph[(r * nd + d) * nw + j]  = 0.25 * r - 0.5 * d + 0.125 * j;
            }
    hydro.SetExcitationRAOHeadings(body + 1, dirs, w, mag, ph);
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

static IrregularWaveParams wave_params() {  // CPP_WAVES of the Python tests
    IrregularWaveParams p;
    p.num_bodies_          = 4;
    p.simulation_dt_       = 0.01;
    p.simulation_duration_ = 40.0;
    p.ramp_duration_       = 5.0;
    p.wave_height_         = 2.0;
    p.wave_period_         = 7.0;
    p.frequency_min_       = 0.05;
    p.frequency_max_       = 0.8;
    p.nfrequencies_        = 24;
    p.seed_                = 3;
    return p;
}

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
        std::vector<std::shared_ptr<MockBody>> mock;
        std::vector<std::shared_ptr<BodyView>> bodies;
        for (int b = 0; b < 4; ++b) {
            mock.push_back(std::make_shared<MockBody>("body" + std::to_string(b + 1)));
            bodies.push_back(mock.back());
        }
        TestHydro hydro(bodies, argv[1], std::make_shared<IrregularWaves>(wave_params()), devices);
        for (int b = 0; b < 4; ++b) set_excitation(hydro, b);
        hydro.SetSurfaceMesh(1, box(2.0, 1.5, -3.0, 4.0), true);
        hydro.SetSurfacePanels(3, panels(2, 12));
        hydro.SetMorisonElements(2, elements(1, 9));
        hydro.SetMorisonElements(3, elements(2, 40));
        set_table(hydro, 0, 9, true, false);
        set_table(hydro, 3, 5, false, false);
        set_table(hydro, 1, 7, false, true);
        set_table(hydro, 2, 9, true, true);
        hydro.SetNonlinearHydroOptions(0.125, 0.0, true);
        hydro.SetMorisonOptions(0.0625, 0.0, true);
        hydro.SetNonlinearHydroMode(2);
        hydro.SetDriftMode(3);
        hydro.SetSumMode(1);
        // CPP_STEPS, CPP_SWITCH, CPP_REGULAR, CPP_REG and CPP_HEADINGS of tests/side_terms_dir_inputs.py
        const int steps = 24, switch_at = 6, regular_at = 12;
        const double before = 0.25, after = -0.5;
        int nf = 24;
        hydro.SetWaveDirections(std::vector<double>(nf, before));
        for (int n = 0; n < steps; ++n) {
            if (n == regular_at) {
                auto w                     = std::make_shared<RegularWave>(4);
                w->regular_wave_amplitude_ = 0.25;
                w->regular_wave_omega_     = 0.75;
                hydro.AddWaves(w);
                nf = 1;
                hydro.SetWaveDirections(std::vector<double>(nf, before));
            }
            if (n == switch_at || n == regular_at + switch_at) {
                hydro.SetWaveDirections(std::vector<double>(nf, after));
                const std::vector<double> th = hydro.GetWaveDirections();
                if (th.size() != static_cast<size_t>(nf) || !same_bits(th[0], after)) return 4;
            }
            set_state(mock, n);
            double total[24];
            for (int b = 0; b < 4; ++b)
                for (int k = 0; k < 6; ++k) total[6 * b + k] = hydro.CoordinateFuncForBody(b + 1, k);
            for (int b = 0; b < 4; ++b)
                for (int k = 0; k < 6; ++k)
                    if (!same_bits(hydro.CoordinateFuncForBody(b + 1, k), total[6 * b + k])) return 3;
            const std::vector<double> mor = hydro.ComputeForceMorison(), nl = hydro.ComputeForceNonlinear(), dft = hydro.ComputeForceDrift(),
                                      smf = hydro.ComputeForceSumQTF();
            std::printf("%a", mock[0]->time);
            for (int b = 0; b < 4; ++b)
                for (const auto* v : {&mock[b]->pos, &mock[b]->rpy, &mock[b]->linvel, &mock[b]->angvel})
                    for (int k = 0; k < 3; ++k) std::printf(" %a", (*v)[k]);
            for (double v : total) std::printf(" %a", v);
            for (const auto* vec : {&mor, &nl, &dft, &smf})
                for (double v : *vec) std::printf(" %a", v);
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "side_terms_dir_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
