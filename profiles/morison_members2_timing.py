"""Times the Morison strip members on the second-order sea (DESIGN 3.7c'', MEASURED.md): one body, 8 members x 16 segments (136
nodes, 256 Gauss points) through the surface in a long-crested sea of 512 components, both bands full.  hc_compute_morison with the
members at order 1 and at order 2 (hc_set_morison_members_second_order), and hc_wave_kinematics2 at the same nodes and Gauss points
and time -- the same device function, one workgroup per item.  Host clock around each call (copies and launches included; every
call ends in a stream synchronise), warmed up, `reps` calls each.  With `once` as the third argument it makes one warmed-up order-2
evaluation and returns: the run to put under `rocprofv3 --kernel-trace --stats` for the kernel times.
Writes profiles/morison_members2/timing.json.  Usage: python profiles/morison_members2_timing.py [out.json] [reps] [once]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WAVES = dict(simulation_dt=0.05, simulation_duration=200.0, ramp_duration=20.0, wave_height=4.0, wave_period=9.0,
             frequency_min=0.02, frequency_max=0.6, nfrequencies=512, peak_enhancement_factor=2.0, seed=4)


def stats(samples):
    s = np.sort(np.asarray(samples))
    return {"median_s": float(np.median(s)), "min_s": float(s[0]), "p10_s": float(s[len(s) // 10]), "p90_s": float(s[(9 * len(s)) // 10]),
            "calls": int(s.size)}


def main():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import many_body_case
    M, S, nf = 8, 16, WAVES["nfrequencies"]
    h = HydroForces.from_case(many_body_case(1, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7))
    h.add_waves_irregular(**WAVES)
    rng = np.random.default_rng(1)
    r0 = np.stack([rng.uniform(-8, 8, M), rng.uniform(-8, 8, M), rng.uniform(-14.0, -8.0, M)], axis=1)
    r1 = r0 + np.stack([rng.uniform(-3, 3, M), rng.uniform(-3, 3, M), rng.uniform(16.0, 22.0, M)], axis=1)
    h.set_morison_members(0, r0, r1, rng.uniform(0.5, 1.5, (M, 2)), 1.0, 2.0, S)
    t = 55.5
    st = PrescribedMotion(1, np.array([[0.0, 0.0, -1.0]]), seed=8, amplitude=0.5).state(t)
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    h.set_morison_members_second_order(True)

    def morison(order2):
        h.set_morison_second_order(order2)  # (a host switch; the tables stay cached while it is on)
        t0 = time.perf_counter()
        h.compute_morison(t, *st)
        return time.perf_counter() - t0

    if len(sys.argv) > 3 and sys.argv[3] == "once":
        for _ in range(3):
            morison(True)
        return
    # switching second order off frees the tables, so order 1 is timed in a loop of its own, before
    for _ in range(3):
        morison(False)
    first = [morison(False) for _ in range(reps)]
    out = {"members": M, "segments_per_member": S, "nodes": M * (S + 1), "gauss_points": 2 * M * S, "nf": nf, "bands": "full",
           "order1": stats(first)}
    out["order2_first_call_s"] = morison(True)  # the pair tables are built
    inc = h.morison_member_increments(0)
    wet = int(np.count_nonzero(inc["eta2"]))
    pts = np.concatenate([inc["node_p"], inc["p"][inc["eta2"] != 0.0]])
    out["wet_gauss_points"] = wet

    def kin2():
        t0 = time.perf_counter()
        h.wave_kinematics2(pts, [t])
        return time.perf_counter() - t0

    for _ in range(3):
        morison(True)
        kin2()
    a, b = [], []
    for _ in range(reps):
        a.append(morison(True))
        b.append(kin2())
    out["order2"] = stats(a)
    out["wave_kinematics2_same_points"] = stats(b)
    out["items"] = int(len(pts))
    out["per_item_increment_kernels_s"] = (out["order2"]["median_s"] - out["order1"]["median_s"]) / len(pts)
    out["per_item_sum_kernel_s"] = out["wave_kinematics2_same_points"]["median_s"] / len(pts)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "morison_members2", "timing.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
