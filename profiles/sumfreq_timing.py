"""Sum-frequency wave forces on the GPU (hc_compute_sum_qtf, csrc/hc_qtf.hip): what a call costs beside the drift term's, and
what the two terms do to the step beside them.

  (a) hc_compute_sum_qtf and hc_compute_drift (mode 3) per call at 64 bodies x 512 components x nq = 64 (the C3 system of bench.py),
      first call (tables uploaded, bin map built) and steady state;
  (c) HydroForces.step at C3 with 64 drift tables under mode 3 alone, then with 64 sum-frequency tables beside them
      (hc_drift_begin, hc_sum_qtf_begin -> hc_step -> hc_drift_end, hc_sum_qtf_end), mean and median over consecutive windows in the same
      process.  On a checkout without the sum-frequency term (the parent commit) the first half alone is taken.

    python profiles/sumfreq_timing.py [--parts ac] [--out DIR] [--tag NAME] [--quick]

Writes DIR/timing_<tag>.json (default profiles/sumfreq, tag = the parts) and prints it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from drift_timing import N_BODIES, NQ, DT, c3, stats_us, timed  # noqa: E402  (the C3 system and the clocks of the drift figures)


def set_tables(h, N, lo, hi, which):
    rng = np.random.default_rng(11 if which == "drift" else 12)
    omega = np.linspace(lo, hi, NQ)
    setter = h.set_drift_qtf if which == "drift" else h.set_sum_qtf
    for b in range(N):
        setter(b, omega, rng.normal(0, 1e4, (6, NQ, NQ)), rng.normal(0, 1e4, (6, NQ, NQ)))


def call_times(h, N, reps):
    pos = np.zeros((N, 3))
    pos[:, 0] = 30.0 * np.arange(N)
    out = {}
    h.set_drift_mode(3)
    h.set_sum_mode(1)
    for name, fn in (("sum_qtf", lambda: h.compute_sum_qtf(12.5, pos)), ("drift_mode3", lambda: h.compute_drift(12.5, pos))):
        first = timed(fn, 1)
        timed(fn, 20)
        out[name] = dict(first_call_us=float(1e6 * first[0]), **stats_us(timed(fn, reps)))
    # interleaved once more, so that neither owes its figure to its place in the run
    for name, fn in (("drift_mode3_again", lambda: h.compute_drift(12.5, pos)), ("sum_qtf_again", lambda: h.compute_sum_qtf(12.5, pos))):
        timed(fn, 20)
        out[name] = stats_us(timed(fn, reps))
    out["table_bytes_each"] = 96.0 * NQ * NQ * N
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
    res = {"no_table": [], "drift_mode3": []}
    for w in range(windows):
        res["no_table"].append(stats_us(timed(one, reps)))
    set_tables(h, N_BODIES, 0.2, 3.0, "drift")
    h.set_drift_mode(3)
    timed(one, 50)
    for w in range(windows):
        res["drift_mode3"].append(stats_us(timed(one, reps)))
    if hasattr(h, "set_sum_qtf"):
        res["drift_mode3_and_sum"] = []
        set_tables(h, N_BODIES, 0.2, 3.0, "sum")
        h.set_sum_mode(1)
        timed(one, 50)
        for w in range(windows):
            res["drift_mode3_and_sum"].append(stats_us(timed(one, reps)))
        res["drift_mode3_after"] = []  # the sum-frequency term off again: the drift figure at the end of the run
        h.set_sum_mode(0)
        timed(one, 50)
        for w in range(windows):
            res["drift_mode3_after"].append(stats_us(timed(one, reps)))
    res["note"] = "the times include PrescribedMotion.state() on the host, the same in every loop"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ac")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sumfreq"))
    ap.add_argument("--tag", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces as HF
    reps = 50 if a.quick else 300
    res = {}
    if "a" in a.parts:
        h = c3(HF)
        set_tables(h, N_BODIES, 0.2, 3.0, "drift")
        set_tables(h, N_BODIES, 0.2, 3.0, "sum")
        res["a_c3_64x512x64"] = call_times(h, N_BODIES, reps)
        h.close()
    if "c" in a.parts:
        res["c_step_c3"] = step_times(HF, reps, 3 if a.quick else 5)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, f"timing_{a.tag or a.parts}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
