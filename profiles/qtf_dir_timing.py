"""QTF tables on a heading grid (hc_set_drift_qtf_headings, csrc/hc_qtf_dir.hip): what a call of hc_compute_drift costs in mode 3 at
64 bodies x 512 components (the C3 system of bench.py), beside the one-heading call on the same frequency grid.

    python profiles/qtf_dir_timing.py --kind one|dir|dir1024 [--reps N]

  one      one-heading tables, nq = 32 (drift_qtf_kernel): the yardstick, runs on the commit before this feature as well
  dir      heading tables nh = 8, nq = 32 (J = 256) under a uniform heading of 0.3 rad between two nodes
  dir1024  heading tables nh = 16, nq = 64 (J = 1024, the cap; P only: 50 MB per body and table would not fit twice in a quick run)

Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python profiles/qtf_dir_timing.py ...` the kernels' durations."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C3_WAVES = dict(simulation_dt=0.01, simulation_duration=120.0, ramp_duration=0.0, wave_height=2.0, wave_period=8.0,
                frequency_min=0.02, frequency_max=0.5, nfrequencies=512, peak_enhancement_factor=3.3, seed=1)
N_BODIES, S_RIRF, N_EXC, DT = 64, 1024, 1024, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="dir", choices=("one", "dir", "dir1024"))
    ap.add_argument("--reps", type=int, default=300)
    a = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces as HF
    h = HF(N_BODIES)
    h.synth_fill(20251031, S_RIRF, DT, N_EXC, DT)
    h.finalize()
    h.add_waves_irregular(**dict(C3_WAVES, num_bodies=N_BODIES))
    nh, nq = {"one": (0, 32), "dir": (8, 32), "dir1024": (16, 64)}[a.kind]
    rng = np.random.default_rng(11)
    omega = np.linspace(0.2, 3.0, nq)
    if nh:
        h.set_wave_directions(np.full(512, 0.3))
        beta = np.linspace(-1.0, 1.0, nh)
        P = rng.normal(0, 1e4, (6, nh, nh, nq, nq))
        Q = None if a.kind == "dir1024" else rng.normal(0, 1e4, P.shape)
        for b in range(N_BODIES):
            h.set_drift_qtf(b, omega, P, Q, headings=beta)
    else:
        for b in range(N_BODIES):
            h.set_drift_qtf(b, omega, rng.normal(0, 1e4, (6, nq, nq)), rng.normal(0, 1e4, (6, nq, nq)))
    h.set_drift_mode(3)
    pos = np.zeros((N_BODIES, 3))
    pos[:, 0], pos[:, 1] = 30.0 * np.arange(N_BODIES), 7.0
    t0 = time.perf_counter()
    h.compute_drift(12.5, pos)
    first = time.perf_counter() - t0
    for _ in range(20):
        h.compute_drift(12.5, pos)
    s = np.empty(a.reps)
    for i in range(a.reps):
        t0 = time.perf_counter()
        h.compute_drift(12.5, pos)
        s[i] = time.perf_counter() - t0
    J = max(nh, 1) * nq
    nbytes = 8.0 * 6 * J * J * N_BODIES * (1 if a.kind == "dir1024" else 2)
    print(json.dumps(dict(kind=a.kind, nh=nh, nq=nq, J=J, bodies=N_BODIES, nf=512, mode=3, reps=a.reps, first_call_us=1e6 * first,
                          mean_us=1e6 * float(s.mean()), median_us=1e6 * float(np.median(s)), min_us=1e6 * float(s.min()),
                          table_bytes=nbytes, implied_GBps_at_median=nbytes / float(np.median(s)) / 1e9)))
    h.close()


if __name__ == "__main__":
    main()
