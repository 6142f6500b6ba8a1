// A reference-style caller with a surface mesh CLIPPED at the free surface through the C++ mirror: TestHydro over one MockBody in a
// regular wave, a triangulated box set with SetSurfaceMesh(body, triangles, true), nonlinear mode 2, the force read through
// CoordinateFuncForBody as Chrono's callbacks do.
//   usage: surface_clip_caller <sphere.h5>
// Prints one line per step: t pos[3] rpy[3] linvel[3] angvel[3] total[6] buoy[6] fk[6] hs_lin[6] (%.17g), total =
// CoordinateFuncForBody (hydro - hs_lin + buoy + fk), the three terms = ComputeForceNonlinear at the same state.  Exit 3: a second
// read at the same time gave other bits; exit 4: mode 0, or clearing the list, did not bring the plain total back; exit 5: the same
// mesh without clip (centroid panels) gave the clipped bits, or setting it clipped again did not bring them back.
// Built with plain g++ by tests/test_surface_clip_ref_cpu.py, run on the GPU by tests/test_gpu_surface_clip_cpp.py.
#include <array>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/hydroc_amd/hydro_forces.h"

using namespace hydroc_amd;
using Tri = std::array<std::array<double, 3>, 3>;

// the twelve triangles of the box [-a, a] x [-b, b] x [z0, z1], normals outward
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
        const std::vector<Tri> mesh = box(2.0, 1.5, -3.0, 4.0);
        hydro_forces.SetSurfaceMesh(1, mesh, true);
        hydro_forces.SetNonlinearHydroOptions(0.25, 0.3, true);
        hydro_forces.SetNonlinearHydroMode(2);
        const int steps = 12;
        std::vector<double> last;
        for (int n = 0; n < steps; ++n) {
            const double t = 0.05 * n;
            body->time   = t;
            body->pos    = {0.1 * n * 0.05, 0.0, -0.6 + 0.013 * n};
            body->rpy    = {0.2 + 0.006 * n, -0.15 - 0.009 * n, 0.003 * n};
            body->linvel = {0.1, 0.0, 0.3 - 0.01 * n};
            body->angvel = {0.02, -0.03 + 0.001 * n, 0.01};
            double total[6];
            for (int k = 0; k < 6; ++k) total[k] = hydro_forces.CoordinateFuncForBody(1, k);
            for (int k = 0; k < 6; ++k) {
                const double again = hydro_forces.CoordinateFuncForBody(1, k);
                if (std::memcmp(&again, &total[k], sizeof(double)) != 0) return 3;
            }
            last = hydro_forces.ComputeForceNonlinear();
            std::printf("%.17g", t);
            for (const auto* v : {&body->pos, &body->rpy, &body->linvel, &body->angvel})
                for (int k = 0; k < 3; ++k) std::printf(" %.17g", (*v)[k]);
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", total[k]);
            for (int k = 0; k < 18; ++k) std::printf(" %.17g", last[k]);
            std::printf("\n");
        }
        // the same mesh as centroid panels is another list (and replaces the triangles); clipped again: the bits before
        hydro_forces.SetSurfaceMesh(1, mesh);
        const std::vector<double> centroid = hydro_forces.ComputeForceNonlinear();
        if (std::memcmp(centroid.data(), last.data(), 12 * sizeof(double)) == 0) return 5;
        hydro_forces.SetSurfaceMesh(1, mesh, true);
        const std::vector<double> same = hydro_forces.ComputeForceNonlinear();
        if (std::memcmp(same.data(), last.data(), 18 * sizeof(double)) != 0) return 5;
        // mode 0, and an empty clipped mesh under mode 2: the callbacks return the plain total again
        const double composed = hydro_forces.CoordinateFuncForBody(1, 2);
        hydro_forces.SetNonlinearHydroMode(0);
        const double plain = hydro_forces.CoordinateFuncForBody(1, 2);
        hydro_forces.SetSurfaceMesh(1, {}, true);
        hydro_forces.SetNonlinearHydroMode(2);
        const double cleared = hydro_forces.CoordinateFuncForBody(1, 2);
        if (plain == composed || std::memcmp(&plain, &cleared, sizeof(double)) != 0) return 4;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "surface_clip_caller: %s\n", e.what());
        return 1;
    }
    return 0;
}
