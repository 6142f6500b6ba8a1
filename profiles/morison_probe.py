"""Morison elements on the GPU (hc_compute_morison, csrc/hc_morison.hip): what a call costs, what it sustains, and what it does to
the step beside it.

  (a) hc_compute_morison per call at 64 bodies x 64 elements x 512 components (the C3 system of bench.py) and at 1 body x 32 elements
      x 2048 components (the C5 spectrum), as time and as element x component evaluations per second (stretching on: an eta pass and
      a kinematics pass), next to hc_wave_kinematics at a comparable item count in the same run;
  (b) hc_step at C3 with no element set: mean and median over consecutive windows (run from a tree built at the parent commit and
      from this one; the windows give the run-to-run spread);
  (c) the composed step at C3 with 64 x 64 elements: hc_morison_begin -> hc_step -> hc_morison_end against hc_step followed by a
      synchronous hc_compute_morison, and hc_step alone in the same loop.

    python profiles/morison_probe.py [--parts abc] [--out DIR] [--tag TAG] [--quick]

Writes DIR/probe_<parts><tag>.json (default profiles/morison) and prints it.  Part b uses nothing the parent commit lacks.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

C3_WAVES = dict(simulation_dt=0.01, simulation_duration=120.0, ramp_duration=0.0, wave_height=2.0, wave_period=8.0,
                frequency_min=0.02, frequency_max=0.5, nfrequencies=512, peak_enhancement_factor=3.3, seed=1)
C5_IRREG = dict(simulation_dt=0.08, simulation_duration=1000.0, ramp_duration=20.0, wave_height=6.0, wave_period=10.0,
                frequency_min=0.01, frequency_max=0.6, nfrequencies=2048, peak_enhancement_factor=2.0, seed=4)
N_BODIES, S_RIRF, N_EXC, DT = 64, 1024, 1024, 0.01


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


def elements(n, seed):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-10.0, 10.0, size=(n, 3))
    r[:, 2] = rng.uniform(-20.0, -3.0, size=n)  # all wet
    return r, rng.uniform(0.5, 2.0, size=(n, 3)), rng.uniform(0.0, 2.0, size=(n, 3))


def states(N, times):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((N, 3))
    rest[:, 0] = 30.0 * np.arange(N)
    m = PrescribedMotion(N, rest, seed=3)
    return [[np.ascontiguousarray(x).reshape(-1) for x in m.state(t)] for t in times]


def part_a(HF, res, reps):
    from hydrochrono_amd.synthetic import many_body_case
    for name, nb, ne in (("c3_64x64x512", N_BODIES, 64), ("c5_1x32x2048", 1, 32)):
        if nb == 1:
            h = HF.from_case(many_body_case(1, S=401, dt_rirf=0.05, n_exc=401, dt_exc=0.25, seed=5))
            h.add_waves_irregular(**C5_IRREG)
        else:
            h = c3(HF)
        nf = h.sizes()["nf"]
        for b in range(nb):
            h.set_morison_elements(b, *elements(ne, 50 + b))
        st = states(nb, [37.1])[0]
        for _ in range(20):
            h.compute_morison(37.1, *st)
        tm = timed(lambda: h.compute_morison(37.1, *st), reps)
        evals = 2 * nb * ne * nf
        row = dict(stats_us(tm), items=nb * ne, nf=nf, term_evaluations=evals, terms_per_s_call=evals / float(np.median(tm)))
        # hc_wave_kinematics at the same item count, same spectrum, stretching on (two passes as well)
        pts = np.zeros((nb * ne, 3))
        pts[:, 0] = np.linspace(-200.0, 200.0, pts.shape[0])
        pts[:, 2] = -2.0
        for _ in range(20):
            h.wave_kinematics(pts, [37.1])
        tk = timed(lambda: h.wave_kinematics(pts, [37.1]), reps)
        row["wave_kinematics_same_items"] = dict(stats_us(tk), terms_per_s_call=evals / float(np.median(tk)))
        res["a_" + name] = row
        h.close()


def step_windows(sts, times, windows, per_window, fn):
    out = []
    k = 0
    for _ in range(windows):
        samples = np.empty(per_window)
        for i in range(per_window):
            t0 = time.perf_counter()
            fn(times[k], sts[k])
            samples[i] = time.perf_counter() - t0
            k += 1
        out.append(stats_us(samples))
    return out


def part_b(HF, res, quick):
    from hydrochrono_amd import capi
    h = c3(HF)
    step = capi.step_raw(h.lib)
    warm, windows, per = (200, 2, 256) if quick else (1200, 5, 1024)
    times = DT * np.arange(warm + windows * per)
    sts = states(N_BODIES, times)
    out = np.empty(h.D_local)

    def plain(t, s):
        step(h.ctx, t, s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data, s[3].ctypes.data, out.ctypes.data)

    for k in range(warm):
        plain(times[k], sts[k])
    res["b_hc_step_c3_no_elements"] = dict(windows=step_windows(sts[warm:], times[warm:], windows, per, plain))
    h.close()


def part_c(HF, res, quick):
    from hydrochrono_amd import capi
    dp = (lambda a: a.ctypes.data_as(capi.c_double_p))
    warm, windows, per = (200, 2, 256) if quick else (1200, 3, 1024)
    times = DT * np.arange(warm + windows * per)
    sts = states(N_BODIES, times)
    for variant in ("step_alone", "begin_step_end", "step_then_compute"):
        h = c3(HF)
        lib, step = h.lib, capi.step_raw(h.lib)
        for b in range(N_BODIES):
            h.set_morison_elements(b, *elements(64, 50 + b))
        out, mor = np.empty(h.D_local), np.empty(h.D_local)

        def plain(t, s):
            step(h.ctx, t, s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data, s[3].ctypes.data, out.ctypes.data)

        def overlapped(t, s):
            lib.hc_morison_begin(h.ctx, t, dp(s[0]), dp(s[1]), dp(s[2]), dp(s[3]))
            plain(t, s)
            lib.hc_morison_end(h.ctx, dp(mor))

        def serial(t, s):
            plain(t, s)
            lib.hc_compute_morison(h.ctx, t, dp(s[0]), dp(s[1]), dp(s[2]), dp(s[3]), dp(mor))

        fn = dict(step_alone=plain, begin_step_end=overlapped, step_then_compute=serial)[variant]
        for k in range(warm):
            fn(times[k], sts[k])
        res["c_" + variant] = dict(windows=step_windows(sts[warm:], times[warm:], windows, per, fn))
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morison"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces as HF
    res = {}
    if "a" in args.parts:
        part_a(HF, res, 30 if args.quick else 300)
    if "b" in args.parts:
        part_b(HF, res, args.quick)
    if "c" in args.parts:
        part_c(HF, res, args.quick)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"probe_{args.parts}{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
