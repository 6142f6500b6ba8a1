"""What the directional instantiations cost: hc_wave_kinematics at 4096 points x 512 components, one Morison call (256 elements)
and one nonlinear call (a box of 3072 clipped triangles), each with and without wave directions on the same context.  Wall time of
the whole synchronous call (copies included), 10 warm-up calls, median and spread of 50; prints one JSON line per row.
    python profiles/directional_cost.py
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, warm=10, reps=50):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    out = np.array(out) * 1e6
    return dict(median_us=round(float(np.median(out)), 1), p10_us=round(float(np.percentile(out, 10)), 1), p90_us=round(float(np.percentile(out, 90)), 1))


def main():
    import torch  # noqa: F401
    import nonlinear_ref
    from cases import SPHERE_DT, sphere_case
    from hydrochrono_amd.hydro import HydroForces
    case = sphere_case()
    bd = case["bodies"][0]
    h = HydroForces.from_case(case)
    mag, ph = (np.stack([np.asarray(bd[k]).reshape(6, -1)] * 2, axis=1) for k in ("ex_mag", "ex_phase"))
    h.set_body_excitation_rao_headings(0, [-2.0, 2.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, simulation_dt=SPHERE_DT, simulation_duration=60.0, ramp_duration=0.0, wave_height=2.0, wave_period=9.0,
                          frequency_min=0.03, frequency_max=0.9, nfrequencies=512, seed=3)
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(-100, 100, 4096), rng.uniform(-100, 100, 4096), rng.uniform(-30, 0, 4096)], axis=1)
    r = np.stack([rng.uniform(-5, 5, 256), rng.uniform(-5, 5, 256), rng.uniform(-8, -1, 256)], axis=1)
    h.set_morison_elements(0, r, np.full((256, 3), 0.5), np.full((256, 3), 0.3))
    h.set_surface_mesh(0, nonlinear_ref.box_triangles([-2.0, -1.0, -3.0], [2.0, 1.0, 1.0], m=16), clip=True)
    z3 = np.zeros(3)
    rows = {"wave_kinematics 4096 x 512": lambda: h.wave_kinematics(pts, [3.0]),
            "morison 256 elements x 512": lambda: h.compute_morison(3.0, z3, z3, z3, z3),
            "nonlinear clipped triangles x 512": lambda: h.compute_nonlinear(3.0, z3, z3)}
    theta = rng.uniform(-1.0, 1.0, 512)
    for name, fn in rows.items():
        h.set_wave_directions(None)
        off = timed(fn)
        h.set_wave_directions(theta)
        on = timed(fn)
        print(json.dumps(dict(what=name, long_crested=off, directional=on, ratio=round(on["median_us"] / off["median_us"], 3))))


if __name__ == "__main__":
    main()
