"""Wave drift forces on the GPU (hc_compute_drift, csrc/hc_qtf.hip): what a call costs and what it does to the step beside it.

  (a) hc_compute_drift per call at 64 bodies x 512 components x nq = 64 (the C3 system of bench.py), modes 1, 2 and 3, first call
      (tables uploaded, bin map built) and steady state;
  (b) the same at 1 body x 2048 components x nq = 64 (the C5 spectrum);
  (c) HydroForces.step at C3 with no table set (the calls of the commit before this feature) and with 64 tables under mode 3
      (hc_drift_begin -> hc_step -> hc_drift_end), mean and median over consecutive windows in the same process.

    python profiles/drift_timing.py [--parts abc] [--out DIR] [--quick]

Writes DIR/timing_<parts>.json (default profiles/drift) and prints it.  Mode 3 reads 2 tables x 6 rows x nq^2 doubles per body:
96 nq^2 bytes, 25 MB at 64 bodies and nq = 64; the implied rate is printed beside the time."""
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
C5_IRREG = dict(simulation_dt=0.08, simulation_duration=1000.0, ramp_duration=20.0, wave_height=6.0, wave_period=10.0,
                frequency_min=0.01, frequency_max=0.6, nfrequencies=2048, peak_enhancement_factor=2.0, seed=4)
N_BODIES, S_RIRF, N_EXC, DT, NQ = 64, 1024, 1024, 0.01, 64


def stats_us(samples):
    a = 1e6 * np.asarray(samples)
    return dict(mean_us=float(a.mean()), median_us=float(np.median(a)), p99_us=float(np.percentile(a, 99)), min_us=float(a.min()), n=int(a.size))


def timed(fn, reps):
    out = np.empty(reps)
    for i in range(reps):
        t0 = time.perf_counter()
        fn()
        out[i] = time.perf_counter() - t0
    return out


def c3(HF):
    h = HF(N_BODIES)
    h.synth_fill(20251031, S_RIRF, DT, N_EXC, DT)
    h.finalize()
    h.add_waves_irregular(**dict(C3_WAVES, num_bodies=N_BODIES))
    return h


def c5(HF):
    from hydrochrono_amd.synthetic import many_body_case
    h = HF.from_case(many_body_case(1, S=401, dt_rirf=0.05, n_exc=401, dt_exc=0.25, seed=5))
    h.add_waves_irregular(**C5_IRREG)
    return h


def set_tables(h, N, lo, hi):
    rng = np.random.default_rng(11)
    omega = np.linspace(lo, hi, NQ)
    for b in range(N):
        h.set_drift_qtf(b, omega, rng.normal(0, 1e4, (6, NQ, NQ)), rng.normal(0, 1e4, (6, NQ, NQ)))


def call_times(h, N, reps):
    pos = np.zeros((N, 3))
    pos[:, 0] = 30.0 * np.arange(N)
    out = {}
    for mode in (3, 2, 1):
        h.set_drift_mode(mode)
        first = timed(lambda: h.compute_drift(12.5, pos), 1)
        timed(lambda: h.compute_drift(12.5, pos), 20)
        steady = timed(lambda: h.compute_drift(12.5, pos), reps)
        out[f"mode{mode}"] = dict(first_call_us=float(1e6 * first[0]), **stats_us(steady))
    bytes3 = 96.0 * NQ * NQ * N
    out["mode3"]["table_bytes"] = bytes3
    out["mode3"]["implied_GBps_at_median"] = bytes3 / (out["mode3"]["median_us"] * 1e-6) / 1e9
    return out


def step_times(HF, reps, windows):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    h = c3(HF)
    rest = np.zeros((N_BODIES, 3))
    rest[:, 0] = 30.0 * np.arange(N_BODIES)
    motion = PrescribedMotion(N_BODIES, rest, seed=3, amplitude=0.5)
    n = [0]

    def one():
        t = DT * n[0]
        n[0] += 1
        h.step(t, *motion.state(t))

    timed(one, 200)
    res = {"no_table": [], "tables_mode3": []}
    for w in range(windows):
        res["no_table"].append(stats_us(timed(one, reps)))
    set_tables(h, N_BODIES, 0.2, 3.0)
    h.set_drift_mode(3)
    timed(one, 50)
    for w in range(windows):
        res["tables_mode3"].append(stats_us(timed(one, reps)))
    res["note"] = "the times include PrescribedMotion.state() on the host, the same in both loops"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces as HF
    reps = 50 if a.quick else 300
    res = {}
    if "a" in a.parts:
        h = c3(HF)
        set_tables(h, N_BODIES, 0.2, 3.0)
        res["a_c3_64x512x64"] = call_times(h, N_BODIES, reps)
        h.close()
    if "b" in a.parts:
        h = c5(HF)
        set_tables(h, 1, 0.2, 3.5)
        res["b_c5_1x2048x64"] = call_times(h, 1, reps)
        h.close()
    if "c" in a.parts:
        res["c_step_c3"] = step_times(HF, reps, 3 if a.quick else 5)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, f"timing_{a.parts}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
