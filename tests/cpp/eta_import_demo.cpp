// The hydro call sequence of the reference's eta-import demo (demos/sphere/demo_sphere_irreg_waves_eta_import.cpp:99-185: body1 at
// (0, 0, -2), IrregularWaveParams with eta_file_path_, IrregularWaves, TestHydro, AddWaves, SetUpWaveMesh / GetMeshFile, stepping)
// against the stand-in Chrono headers of tests/cpp/chrono_stub, with only the include and the namespace changed.
//   usage: eta_import_demo <sphere.h5> <eta file> <nsteps>
// Prints "spectrum <what GetSpectrum threw>", "frequencies <count>", "table <n> <first t> <last t>", "mesh <file>", then
// "w <t> <6 components>" of TestHydro::ComputeForceWaves at t = 0.6 k s, k = 0 .. 199 (before any step, so that every one is a plain
// evaluation), then "s <t> <z>" per step (%.17g).
// Built by tests/test_eta_record_cpu.py, run on the GPU by tests/test_gpu_eta_record.py.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#define HYDROCHRONO_AMD_WITH_CHRONO 1
#include <hydroc_amd/hydro_forces.h>  // reference: <hydroc/hydro_forces.h>
#include <hydroc_amd/wave_types.h>    // reference: <hydroc/wave_types.h>

using namespace chrono;
using namespace hydroc_amd;

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string h5fname = argv[1], eta_file = argv[2];
    const int nsteps          = std::atoi(argv[3]);
    try {
        ChSystem system;
        system.SetGravitationalAcceleration(ChVector3d(0.0, 0.0, -9.81));
        double timestep                    = 0.015;
        double simulationDuration          = 120.0;
        std::shared_ptr<ChBody> sphereBody = chrono_types::make_shared<ChBody>();
        auto ground                        = chrono_types::make_shared<ChBody>();
        ground->SetName("ground");
        system.Add(sphereBody);
        sphereBody->SetName("body1");  // must set body name correctly! (must match .h5 file)
        sphereBody->SetPos(ChVector3d(0, 0, -2));
        sphereBody->SetMass(261.8e3);
        system.Add(ground);

        std::vector<std::shared_ptr<ChBody>> bodies;
        bodies.push_back(sphereBody);

        IrregularWaveParams params;
        params.num_bodies_          = bodies.size();
        params.simulation_dt_       = timestep;
        params.simulation_duration_ = simulationDuration;
        params.ramp_duration_       = 0.0;
        params.eta_file_path_       = eta_file;
        params.frequency_min_       = 0.001;
        params.frequency_max_       = 1.0;
        params.nfrequencies_        = 1000;
        std::shared_ptr<IrregularWaves> my_hydro_inputs = std::make_shared<IrregularWaves>(params);

        TestHydro hydro_forces(bodies, h5fname);
        hydro_forces.AddWaves(my_hydro_inputs);

        try {
            my_hydro_inputs->GetSpectrum();
            std::printf("spectrum none\n");
        } catch (const std::runtime_error& e) {
            std::printf("spectrum %s\n", e.what());
        }
        std::printf("frequencies %zu\n", my_hydro_inputs->GetFrequenciesHz().size());
        const std::vector<double> t = my_hydro_inputs->GetFreeSurfaceTime(), eta = my_hydro_inputs->GetFreeSurfaceElevation();
        if (t.empty() || t.size() != eta.size()) return 3;
        std::printf("table %zu %.17g %.17g\n", t.size(), t.front(), t.back());
        my_hydro_inputs->SetUpWaveMesh();
        std::printf("mesh %s\n", my_hydro_inputs->GetMeshFile().c_str());

        for (int k = 0; k < 200; ++k) {
            system.time = 0.6 * k;  // (stub-only state) the time ComputeForceWaves reads, bodies_[0]->GetChTime()
            const std::vector<double> f = hydro_forces.ComputeForceWaves();
            std::printf("w %.17g", 0.6 * k);
            for (double v : f) std::printf(" %.17g", v);
            std::printf("\n");
        }
        system.time = 0.0;
        for (int n = 0; n < nsteps; ++n) {
            system.DoStepDynamics(timestep);
            std::printf("s %.17g %.17g\n", system.GetChTime(), sphereBody->GetPos().z());
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
