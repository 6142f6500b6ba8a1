"""Records for MEASURED.md: the modal radiation term at the C3 shape (64 bodies, 384 rows, 4 modes on every pair = 589 824 modes)
beside the plain-mode convolution step of the same system.
  python profiles/radiation_modes_timing.py [out.json]
Prints and writes: the begin -> end round trip of hc_radiation_modes (host clock, irregular step), the plain-mode hc_step rate and
its conv_step_kernel time (the library's own event timing).  The kernel's own time comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python profiles/radiation_modes_timing.py): the row radiation_modes_kernel."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402
import torch  # noqa: E402,F401
from hydrochrono_amd.hydro import HydroForces  # noqa: E402
from hydrochrono_amd.mock_chrono import PrescribedMotion  # noqa: E402

N, PER_PAIR, REPS = B.N_BODIES, 4, 200
D = 6 * N
rng = np.random.default_rng(1)
out = {"shape": {"bodies": N, "rows": D, "modes_per_pair": PER_PAIR, "modes": D * D * PER_PAIR}}

# ---- the modal term: a context with the smallest IRF (the term reads none of it) ----
h = HydroForces(N)
h.synth_fill(20251031, 2, 0.05, 0, 0.05)
h.finalize()
t_set = time.perf_counter()
for b in range(N):
    lam = -rng.uniform(0.05, 3.0, size=(6, D, PER_PAIR)) + 1j * rng.uniform(0.0, 4.0, size=(6, D, PER_PAIR))
    rho = rng.normal(size=(6, D, PER_PAIR)) + 1j * rng.normal(size=(6, D, PER_PAIR))
    h.set_radiation_modes(b, [(r, c, lam[r, c, m], rho[r, c, m]) for r in range(6) for c in range(D) for m in range(PER_PAIR)])
out["set_seconds"] = time.perf_counter() - t_set
motion = PrescribedMotion(N, np.zeros((N, 3)), seed=1)
t = 0.0
lv, av = (np.ascontiguousarray(x).reshape(-1) for x in motion.state(t)[2:])
h.compute_radiation_modes(t, lv, av)  # first call: upload, z = 0
trips = []
for n in range(REPS + 20):
    t += 0.004 + 0.02 * rng.uniform()  # no two steps alike
    lv, av = (np.ascontiguousarray(x).reshape(-1) for x in motion.state(t)[2:])
    t0 = time.perf_counter()
    h.radiation_modes_begin(t, lv, av)
    rad = h.radiation_modes_end()
    trips.append(time.perf_counter() - t0)
trips = np.array(trips[20:]) * 1e6
assert np.all(np.isfinite(rad)) and np.abs(rad).max() > 0.0
out["modal_round_trip_us"] = {"median": float(np.median(trips)), "p10": float(np.percentile(trips, 10)), "p90": float(np.percentile(trips, 90)),
                              "evals_per_second": float(1e6 / np.median(trips))}
out["modal_bytes_per_step"] = D * D * PER_PAIR * 68
h.close()

# ---- the plain-mode convolution step of C3 (look-ahead off: what a caller whose step is not uniform gets today) ----
sdt = 0.01
nhist = 1030
t_hist = B.T0 - sdt * np.arange(1, nhist + 1)
v_hist = np.stack([motion.velocity6(tt) for tt in t_hist])
g = B.make_shard(N, 0, N, 0, sdt, B.T0 + 400 * sdt, 0, t_hist, v_hist)
g.enable_profiling(1)
for k in range(20):
    g.step(B.T0 + k * sdt, *motion.state(B.T0 + k * sdt))
g.reset_profile()
secs = []
for k in range(20, 20 + REPS):
    st = motion.state(B.T0 + k * sdt)
    t0 = time.perf_counter()
    g.step(B.T0 + k * sdt, *st)
    secs.append(time.perf_counter() - t0)
p = g.profile()
secs = np.array(secs) * 1e6
out["plain_hc_step_us"] = {"median": float(np.median(secs)), "evals_per_second": float(1e6 / np.median(secs))}
out["conv_step_kernel_us"] = float(p["conv_kernel_seconds"] / max(1, p["conv_kernel_launches"]) * 1e6)
print(json.dumps(out, indent=1))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
