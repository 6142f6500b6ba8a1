"""Times hc_wave_kinematics2_dir beside hc_wave_kinematics2 on the sphere case with a 512-component spectrum: 64 points x 4 times
(256 items), both bands full, all outputs.  Three calls: the directional call on a spread sea, the directional call with no
directions set, and the long-crested call on the same inputs; the last two alternate in one loop.  Host clock around each call
(copies and launches included; the call ends in a stream synchronise), warmed up, `reps` calls each.
Writes profiles/wave_kin2_dir/timing.json.  Usage: python profiles/wave_kin2_dir_timing.py [out.json] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(samples):
    s = np.sort(np.asarray(samples))
    return {"median_s": float(np.median(s)), "min_s": float(s[0]), "p10_s": float(s[len(s) // 10]), "p90_s": float(s[(9 * len(s)) // 10]),
            "calls": int(s.size)}


def main():
    import torch  # noqa: F401
    from cases import SPHERE_DT, sphere_case
    from hydrochrono_amd.hydro import HydroForces
    case = sphere_case()
    h = HydroForces.from_case(case)
    for b, bd in enumerate(case["bodies"]):  # heading tables: what non-uniform directions need
        mag, ph = (np.stack([np.asarray(bd[k]).reshape(6, -1)] * 2, axis=1) for k in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-4.0, 4.0], bd["w"], mag, ph)
    nf = 512
    h.add_waves_irregular(spectral=True, simulation_dt=SPHERE_DT, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0,
                          wave_period=12.0, frequency_min=0.02, frequency_max=1.0, nfrequencies=nf)
    pts = np.stack([np.linspace(-150.0, 150.0, 64), np.linspace(-60.0, 80.0, 64), np.linspace(-40.0, 0.0, 64)], axis=1)
    times = np.array([100.0, 100.5, 101.0, 101.5])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    out = {"nf": nf, "points": 64, "times": 4, "items": 256, "bands": "full", "outputs": "eta2, vel2, acc2",
           "pair_terms_per_item": 2 * nf * nf}

    def timed(**kw):
        t0 = time.perf_counter()
        h.wave_kinematics2(pts, times, **kw)
        return time.perf_counter() - t0

    h.set_wave_directions(1.2 * np.sin(2.3 * np.arange(nf) + 0.4))
    out["dir_spread_first_call_s"] = timed(directional=True)  # the pair tables are built
    for _ in range(5):
        timed(directional=True)
    out["dir_spread"] = stats([timed(directional=True) for _ in range(reps)])
    h.set_wave_directions(None)
    for _ in range(5):
        timed(directional=True)
        timed()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(directional=True))
        b.append(timed())
    out["dir_no_directions"] = stats(a)
    out["long_crested"] = stats(b)
    out["ratio_of_medians_dir_over_long_crested"] = out["dir_no_directions"]["median_s"] / out["long_crested"]["median_s"]
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "wave_kin2_dir", "timing.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
