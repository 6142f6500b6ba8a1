"""What the strip members' added-mass matrix costs: one hc_compute_morison at the shape of profiles/morison_members_cost.py (64
bodies x 30 members x 16 segments x 512 components: 61440 Gauss points) without any ca and with ca = 1 on every member.  Wall time
of the whole synchronous call (copies included), stretching on, 10 warm-up calls, median and spread of 50.  Each timed step runs in
a child process of its own under its own time limit; prints one JSON line per row and one with the difference.
    python profiles/morison_added_mass_cost.py
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]
import morison_members_cost as base  # noqa: E402


def one(what):
    import torch  # noqa: F401
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.synthetic import many_body_case
    h = HydroForces.from_case(many_body_case(base.BODIES, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7))
    h.add_waves_irregular(spectral=True, simulation_dt=0.05, simulation_duration=200.0, ramp_duration=0.0, wave_height=4.0, wave_period=9.0,
                          frequency_min=0.02, frequency_max=0.6, nfrequencies=base.COMPONENTS, peak_enhancement_factor=2.0, seed=4)
    rng = np.random.default_rng(1)
    n = base.MEMBERS
    for b in range(base.BODIES):
        r0 = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-20, -10, n)], axis=1)
        r1 = r0 + np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(12, 25, n)], axis=1)
        h.set_morison_members(b, r0, r1, 1.0, 1.0, 2.0, base.SEGMENTS)
        if what == "with_ca":
            h.set_morison_member_added_mass(b, 1.0)
    pos = np.zeros((base.BODIES, 3))
    pos[:, 0] = 50.0 * np.arange(base.BODIES)
    z = np.zeros((base.BODIES, 3))
    row = base.timed(lambda: h.compute_morison(3.0, pos, z, z, z))
    if what == "with_ca":
        assert h.morison_added_mass().any(axis=(1, 2)).all()
    print(json.dumps(dict(what=what, gauss_points=2 * base.BODIES * n * base.SEGMENTS, components=base.COMPONENTS, **row)), flush=True)


def main():
    rows = {}
    for what in ("without_ca", "with_ca"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), what], capture_output=True, text=True, timeout=base.STEP_LIMIT_S)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            sys.exit(r.returncode or 1)
        print(r.stdout.strip(), flush=True)
        rows[what] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(dict(what="with_ca - without_ca", median_us=round(rows["with_ca"]["median_us"] - rows["without_ca"]["median_us"], 1))))


if __name__ == "__main__":
    one(sys.argv[1]) if len(sys.argv) > 1 else main()
