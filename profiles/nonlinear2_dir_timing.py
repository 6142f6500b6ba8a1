"""Times the nonlinear surface pressure on the directional second-order sea (MEASURED.md): one hc_compute_nonlinear on
the closed 1000-triangle mesh of profiles/nonlinear2_timing.py (502 distinct vertices), clipped triangles, 512 wave components, both
bands full.  Four calls alternate in one loop, each on a context of its own so that no switch frees a table between them:
directional order 1, directional order 2 (hc_set_nonlinear_second_order_directional), long-crested order 2 on the same mesh and
component count, and hc_wave_kinematics2_dir (eta2, vel2, acc2) at the 502 points of the directional evaluation.  Host clock around
each whole call (copies and launches included; every call ends in a stream synchronise), warmed up, `reps` calls each.  Two figures
are derived: the time per point of nl2_dir_incr_kernel with its copy, (order 2 - order 1) / points, and the time per item of
wk2_dir_sum_kernel<true, true> with its copies, hc_wave_kinematics2_dir / points -- the increment kernel computes a subset of that
kernel's work.  Writes profiles/nonlinear2_dir/timing.json.  Usage: python profiles/nonlinear2_dir_timing.py [out.json] [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
WAVES = dict(simulation_dt=0.05, simulation_duration=100.0, ramp_duration=20.0, wave_height=2.0, wave_period=8.0,
             frequency_min=0.03, frequency_max=0.6, nfrequencies=512, peak_enhancement_factor=2.0, seed=4)


def stats(samples):
    s = np.sort(np.asarray(samples))
    return {"median_s": float(np.median(s)), "min_s": float(s[0]), "p10_s": float(s[len(s) // 10]), "p90_s": float(s[(9 * len(s)) // 10]),
            "calls": int(s.size)}


def main():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.synthetic import many_body_case
    from nonlinear2_timing import uv_sphere
    nf = WAVES["nfrequencies"]
    case = many_body_case(1, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7, water_depth=60.0)
    mesh = uv_sphere()
    pos, rpy, t = np.array([[0.3, -0.1, -0.4]]), np.array([[0.1, -0.05, 0.2]]), 33.0

    def context(directions, order2):
        h = HydroForces.from_case(case)
        if directions:
            bd = case["bodies"][0]  # heading tables: what non-uniform directions need
            mag, ph = (np.stack([np.asarray(bd[k]).reshape(6, -1)] * 2, axis=1) for k in ("ex_mag", "ex_phase"))
            h.set_body_excitation_rao_headings(0, [-4.0, 4.0], bd["w"], mag, ph)
        h.add_waves_irregular(spectral=directions, **WAVES)
        if directions:
            h.set_wave_directions(1.2 * np.sin(2.3 * np.arange(nf) + 0.4))
        h.set_surface_mesh(0, mesh, clip=True)
        h.set_nonlinear_second_order(order2)
        h.set_nonlinear_second_order_directional(True)
        return h

    ctx = {"order1_dir": context(True, False), "order2_dir": context(True, True), "order2_long_crested": context(False, True)}
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    out = {"triangles": len(mesh), "nf": nf, "bands": "full", "pair_terms_per_point": 2 * nf * nf}

    def surface(name):
        t0 = time.perf_counter()
        ctx[name].compute_nonlinear(t, pos, rpy)
        return time.perf_counter() - t0

    out["first_call_s"] = {name: surface(name) for name in ctx}  # tables and point lists are built
    pts = ctx["order2_dir"].nonlinear_increments(0)["p"]
    out["points"] = len(pts)

    def kin2():
        t0 = time.perf_counter()
        ctx["order2_dir"].wave_kinematics2(pts, [t], directional=True)
        return time.perf_counter() - t0

    for _ in range(3):
        for name in ctx:
            surface(name)
        kin2()
    rows = {name: [] for name in ctx}
    rows["wave_kinematics2_dir_same_points"] = []
    for _ in range(reps):
        for name in ctx:
            rows[name].append(surface(name))
        rows["wave_kinematics2_dir_same_points"].append(kin2())
    for name, samples in rows.items():
        out[name] = stats(samples)
    out["per_point_incr_kernel_s"] = (out["order2_dir"]["median_s"] - out["order1_dir"]["median_s"]) / len(pts)
    out["per_item_sum_kernel_s"] = out["wave_kinematics2_dir_same_points"]["median_s"] / len(pts)
    for h in ctx.values():
        h.close()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nonlinear2_dir", "timing.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
