"""Timing of one hc_compute_morison on the second-order sea (MEASURED.md): 64 bodies x 64 elements on the C3 spectrum
(512 components), host clock, copies included -- order 1, order 2 with a difference band of 0-0.5 rad/s and the sum band excluded,
order 2 with full bands -- and beside each order-2 figure hc_wave_kinematics2 on the same 4096 points and bands in the same run.
    python profiles/morison2_timing.py [--reps 30]
Prints the median, the minimum and the maximum of each setting in milliseconds."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INF = float("inf")
C3_WAVES = dict(simulation_dt=0.05, simulation_duration=200.0, ramp_duration=20.0, wave_height=4.0, wave_period=9.0,
                frequency_min=0.02, frequency_max=0.6, nfrequencies=512, peak_enhancement_factor=2.0, seed=4)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return np.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import many_body_case
    N, E = 64, 64
    h = HydroForces.from_case(many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7))
    h.add_waves_irregular(spectral=True, **C3_WAVES)
    rng = np.random.default_rng(1)
    for b in range(N):
        h.set_morison_elements(b, rng.uniform(-10, 10, (E, 3)), rng.uniform(0, 3, (E, 3)), rng.uniform(0, 4, (E, 3)))
    rest = np.zeros((N, 3))
    rest[:, 0] = 15.0 * np.arange(N)
    rest[:, 2] = -1.0
    t = 55.5
    st = PrescribedMotion(N, rest, seed=8, amplitude=0.5).state(t)
    print(f"{N} bodies x {E} elements, {h.wave_component_count()} components, {args.reps} repetitions: median / min / max [ms]")
    print("order 1:                          %8.3f %8.3f %8.3f" % timed(lambda: h.compute_morison(t, *st), args.reps))
    for label, diff_band, sum_band in (("diff 0-0.5 rad/s, no sum", (0.0, 0.5), (100.0, 200.0)), ("full bands", (0.0, INF), (0.0, INF))):
        h.set_morison_second_order(True, diff_band=diff_band, sum_band=sum_band)
        h.compute_morison(t, *st)  # builds the tables
        print("order 2, %-24s %8.3f %8.3f %8.3f" % (label + ":", *timed(lambda: h.compute_morison(t, *st), args.reps)))
        pts = np.concatenate([h.morison_increments(b)["p"] for b in range(N)])
        assert pts.shape == (N * E, 3)
        print("  hc_wave_kinematics2, same points: %6.3f %8.3f %8.3f" % timed(
            lambda: h.wave_kinematics2(pts, [t], diff_band=diff_band, sum_band=sum_band), args.reps))
    h.set_morison_second_order(False)
    print("order 1 again:                    %8.3f %8.3f %8.3f" % timed(lambda: h.compute_morison(t, *st), args.reps))


if __name__ == "__main__":
    main()
