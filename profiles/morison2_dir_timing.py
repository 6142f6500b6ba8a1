"""Times the Morison elements on the directional second-order sea (MEASURED.md): 64 bodies x 64 elements on a
512-component spread sea, both bands full.  Three calls alternate in one loop: hc_compute_morison of order 1 under directions,
hc_compute_morison with the directional second-order sea on, and hc_wave_kinematics2_dir (eta2, vel2, acc2) at the same 4096 points
and time.  Host clock around each call (copies and launches included; every call ends in a stream synchronise), warmed up, `reps`
calls each.  Two figures are derived: the time per element of morison2_dir_incr_kernel with its copy, (order 2 - order 1) / 4096, and
the time per item of wk2_dir_sum_kernel<true, true> with its copies, hc_wave_kinematics2_dir / 4096 -- the same device function.
Writes profiles/morison2_dir/timing.json.  Usage: python profiles/morison2_dir_timing.py [out.json] [reps]"""
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
    N, E, nf = 64, 64, WAVES["nfrequencies"]
    case = many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)
    h = HydroForces.from_case(case)
    for b, bd in enumerate(case["bodies"]):  # heading tables: what non-uniform directions need
        mag, ph = (np.stack([np.asarray(bd[k]).reshape(6, -1)] * 2, axis=1) for k in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-4.0, 4.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, **WAVES)
    h.set_wave_directions(1.2 * np.sin(2.3 * np.arange(nf) + 0.4))
    rng = np.random.default_rng(1)
    for b in range(N):
        h.set_morison_elements(b, rng.uniform(-10, 10, (E, 3)), rng.uniform(0, 3, (E, 3)), rng.uniform(0, 4, (E, 3)))
    rest = np.zeros((N, 3))
    rest[:, 0] = 15.0 * np.arange(N)
    rest[:, 2] = -1.0
    t = 55.5
    st = PrescribedMotion(N, rest, seed=8, amplitude=0.5).state(t)
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    h.set_morison_second_order_directional(True)

    def morison(order2):
        h.set_morison_second_order(order2)  # (a host switch; the tables stay cached while it is on)
        t0 = time.perf_counter()
        h.compute_morison(t, *st)
        return time.perf_counter() - t0

    # switching second order off frees the tables, so order 1 is timed in a loop of its own, before
    for _ in range(3):
        morison(False)
    first = [morison(False) for _ in range(reps)]
    out = {"bodies": N, "elements_per_body": E, "nf": nf, "bands": "full", "pair_terms_per_item": 2 * nf * nf, "order1_dir": stats(first)}
    out["order2_dir_first_call_s"] = morison(True)  # the pair tables are built
    pts = np.concatenate([h.morison_increments(b)["p"] for b in range(N)])
    assert pts.shape == (N * E, 3)

    def kin2():
        t0 = time.perf_counter()
        h.wave_kinematics2(pts, [t], directional=True)
        return time.perf_counter() - t0

    for _ in range(3):
        morison(True)
        kin2()
    a, b = [], []
    for _ in range(reps):
        a.append(morison(True))
        b.append(kin2())
    out["order2_dir"] = stats(a)
    out["wave_kinematics2_dir_same_points"] = stats(b)
    n = N * E
    out["per_element_incr_kernel_s"] = (out["order2_dir"]["median_s"] - out["order1_dir"]["median_s"]) / n
    out["per_item_sum_kernel_s"] = out["wave_kinematics2_dir_same_points"]["median_s"] / n
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "morison2_dir", "timing.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
