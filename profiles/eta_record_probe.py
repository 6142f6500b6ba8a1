"""Per-step cost of the sphere case with irregular waves from the imported record (tests/golden/sphere_eta_record.txt,
hc_set_wave_irregular_eta) beside the same case with the synthesised table (Hs 2 m, Tp 12 s, 1000 components, ramp 60 s): hc_step_many
over the same prescribed motion, t = 10 .. 100 s at 0.015 s (6000 steps, the first 500 not counted), default configuration.  Reports
the host wall time per hc_step (mean, median, p99) and the GPU time per step of the profiled launches (every 17th step).

  python profiles/eta_record_probe.py [out.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cases import GOLDEN_DIR, SPHERE_DT, sphere_case  # noqa: E402

SPHERE_IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0, wave_period=12.0,
                    frequency_min=0.001, frequency_max=1.0, nfrequencies=1000)


def main():
    import torch  # noqa: F401
    from hydrochrono_amd.hydro import HydroForces, read_eta_file
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    times = 10.0 + SPHERE_DT * np.arange(6000)
    motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
    states = np.array([motion.packed(t) for t in times])
    out = {}
    for name in ("synthesised", "record", "synthesised_again", "record_again"):
        h = HydroForces.from_case(case)
        if name.startswith("record"):
            h.add_waves_irregular_eta(*read_eta_file(os.path.join(GOLDEN_DIR, "sphere_eta_record.txt")), SPHERE_DT)
        else:
            h.add_waves_irregular(**SPHERE_IRREG)
        h.enable_profiling(17)
        _, sec = h.step_many(times, states)
        p = h.profile()
        s = sec[500:] * 1e6
        gpu = p["hydrostatics_seconds"] + p["radiation_seconds"] + p["waves_seconds"]
        out[name] = dict(steps=int(s.size), host_us_mean=float(s.mean()), host_us_median=float(np.median(s)),
                         host_us_p99=float(np.percentile(s, 99)), gpu_us_per_profiled_step=1e6 * gpu / max(1, p["step_kernel_launches"]),
                         profiled_step_launches=int(p["step_kernel_launches"]), direct=h.direct_dispatch()[0], sizes=h.sizes())
        h.close()
        print(name, json.dumps(out[name]))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
