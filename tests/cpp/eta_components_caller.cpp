// Wave components of an imported eta record through the C++ mirror (include/hydroc_amd/wave_types.h: IrregularWaves::
// SetRecordComponents / GetRecordComponents; GetSpectrum and GetFrequenciesHz answer afterwards), on the call sequence of the
// eta-import demo (tests/cpp/eta_import_demo.cpp) against the stand-in Chrono headers of tests/cpp/chrono_stub.
//   usage: eta_components_caller <sphere.h5> <eta file> <f_min> <f_max> <max_components> <x> <y> <z> <t>
// Prints "before <what GetSpectrum threw>", "count <n>", "frequencies <n> <first> <last>", "spectrum <sum of GetSpectrum in index
// order>", "stats <mean> <variance share> <rms residual>", "velocity <vx> <vy> <vz>" of GetVelocity at (x, y, z), t, "elevation <eta>",
// and after ClearRecordComponents "cleared <count> <eta>" (%.17g).
// Built by tests/test_eta_components_cpu.py, run on the GPU by tests/test_gpu_eta_components.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#define HYDROCHRONO_AMD_WITH_CHRONO 1
#include <hydroc_amd/hydro_forces.h>
#include <hydroc_amd/wave_types.h>

using namespace chrono;
using namespace hydroc_amd;

int main(int argc, char** argv) {
    if (argc < 10) return 2;
    const std::string h5fname = argv[1], eta_file = argv[2];
    const double f_min = std::atof(argv[3]), f_max = std::atof(argv[4]);
    const int max_components = std::atoi(argv[5]);
    const std::array<double, 3> p{std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8])};
    const double t = std::atof(argv[9]);
    try {
        ChSystem system;
        system.SetGravitationalAcceleration(ChVector3d(0.0, 0.0, -9.81));
        std::shared_ptr<ChBody> sphereBody = chrono_types::make_shared<ChBody>();
        system.Add(sphereBody);
        sphereBody->SetName("body1");
        sphereBody->SetPos(ChVector3d(0, 0, -2));
        sphereBody->SetMass(261.8e3);
        std::vector<std::shared_ptr<ChBody>> bodies;
        bodies.push_back(sphereBody);

        IrregularWaveParams params;
        params.num_bodies_    = bodies.size();
        params.simulation_dt_ = 0.015;
        params.eta_file_path_ = eta_file;
        std::shared_ptr<IrregularWaves> waves = std::make_shared<IrregularWaves>(params);
        TestHydro hydro_forces(bodies, h5fname);
        hydro_forces.AddWaves(waves);

        try {
            waves->GetSpectrum();
            std::printf("before none\n");
        } catch (const std::runtime_error& e) {
            std::printf("before %s\n", e.what());
        }
        waves->SetRecordComponents(f_min, f_max, max_components);
        const IrregularWaves::RecordComponents rc = waves->GetRecordComponents();
        std::printf("count %zu\n", rc.A.size());
        const std::vector<double> f = waves->GetFrequenciesHz(), S = waves->GetSpectrum();
        if (f.empty() || f.size() != S.size() || f.size() != rc.f.size()) return 3;
        std::printf("frequencies %zu %.17g %.17g\n", f.size(), f.front(), f.back());
        double sum = 0.0;
        for (double v : S) sum += v;
        std::printf("spectrum %.17g\n", sum);
        std::printf("stats %.17g %.17g %.17g\n", rc.mean, rc.variance_share, rc.rms_residual);
        const std::array<double, 3> v = waves->GetVelocity(p, t);
        std::printf("velocity %.17g %.17g %.17g\n", v[0], v[1], v[2]);
        std::printf("elevation %.17g\n", waves->GetElevation(p, t));
        waves->ClearRecordComponents();
        std::printf("cleared %zu %.17g\n", waves->GetRecordComponents().A.size(), waves->GetElevation(p, t));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
