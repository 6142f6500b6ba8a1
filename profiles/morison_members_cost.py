"""What the Morison strip members cost beside the elements: one evaluation on 64 bodies x 30 members x 16 segments x 512
components (61440 Gauss points, 32640 nodes), and the element kernel -- the code path as it was before the members -- at the same
number of kinematic evaluations (960 elements on each of 64 bodies).  Wall time of the whole synchronous hc_compute_morison
(copies included), stretching on, 10 warm-up calls, median and spread of 50.  Each of the two timed steps runs in a child process of
its own under its own time limit; prints one JSON line per row and one with the ratio.
    python profiles/morison_members_cost.py
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
BODIES, MEMBERS, SEGMENTS, COMPONENTS = 64, 30, 16, 512
STEP_LIMIT_S = 240


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


def one(what):
    import torch  # noqa: F401
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.synthetic import many_body_case
    h = HydroForces.from_case(many_body_case(BODIES, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7))
    h.add_waves_irregular(spectral=True, simulation_dt=0.05, simulation_duration=200.0, ramp_duration=0.0, wave_height=4.0, wave_period=9.0,
                          frequency_min=0.02, frequency_max=0.6, nfrequencies=COMPONENTS, peak_enhancement_factor=2.0, seed=4)
    rng = np.random.default_rng(1)
    points = 2 * MEMBERS * SEGMENTS
    for b in range(BODIES):
        if what == "members":
            r0 = np.stack([rng.uniform(-20, 20, MEMBERS), rng.uniform(-20, 20, MEMBERS), rng.uniform(-20, -10, MEMBERS)], axis=1)
            r1 = r0 + np.stack([rng.uniform(-5, 5, MEMBERS), rng.uniform(-5, 5, MEMBERS), rng.uniform(12, 25, MEMBERS)], axis=1)
            h.set_morison_members(b, r0, r1, 1.0, 1.0, 2.0, SEGMENTS)
        else:
            r = np.stack([rng.uniform(-20, 20, points), rng.uniform(-20, 20, points), rng.uniform(-20, 5, points)], axis=1)
            h.set_morison_elements(b, r, np.full((points, 3), 0.5), np.full((points, 3), 0.3))
    pos = np.zeros((BODIES, 3))
    pos[:, 0] = 50.0 * np.arange(BODIES)
    z = np.zeros((BODIES, 3))
    row = timed(lambda: h.compute_morison(3.0, pos, z, z, z))
    print(json.dumps(dict(what=what, kinematic_evaluations=BODIES * points, nodes=BODIES * MEMBERS * (SEGMENTS + 1) if what == "members" else 0,
                          components=COMPONENTS, **row)), flush=True)


def main():
    rows = {}
    for what in ("elements", "members"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), what], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(r.returncode or 1)
        print(r.stdout.strip(), flush=True)
        rows[what] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(dict(what="members / elements", ratio=round(rows["members"]["median_us"] / rows["elements"]["median_us"], 3))))


if __name__ == "__main__":
    one(sys.argv[1]) if len(sys.argv) > 1 else main()
