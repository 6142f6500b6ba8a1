"""Nonlinear surface forces on the GPU (hc_compute_nonlinear, csrc/hc_nonlinear.hip): what a call costs, what the kernel sustains,
and what it does to the step beside it.

  (a) hc_compute_nonlinear per call at 64 bodies x 2048 panels x 512 components (the C3 system of bench.py) and at 1 body x 8192
      panels x 2048 components (the C5 spectrum), stretching on (an eta pass and a pressure pass) and off (one pass), as time and as
      panel x component evaluations per second;
  (k) the same launches and nothing else, for a run of its own under the kernel trace:
          rocprofv3 --kernel-trace --stats -d DIR -- python profiles/nonlinear_probe.py --parts k --config c3 --stretching 1
      (nl_panels_kernel's mean duration in the trace is the kernel time; 20 warm-up + 50 measured calls);
  (b) hc_step at C3 with no panel set: mean and median over consecutive windows (run from a tree built at the parent commit and from
      this one, alternating; the windows give the run-to-run spread; uses nothing the parent commit lacks);
  (c) the step at C3 with 64 x 2048 panels: hc_nonlinear_begin -> hc_step -> hc_nonlinear_end against hc_step alone in the same loop.

    python profiles/nonlinear_probe.py [--parts abc] [--out DIR] [--tag TAG] [--quick]

Writes DIR/probe_<parts><tag>.json (default profiles/nonlinear) and prints it.

Operation count per panel x component evaluation, for the fraction of the FP64 vector rate: one cos and one exp (or cosh) and
5 FMA-class operations in the pressure pass; one cos and 3 FMA-class operations in the eta pass.  The OCML cos is ~45 FP64 operations
on the reduced-argument path, exp ~25: ~75 per pressure evaluation, ~48 per eta evaluation.
"""
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
N_BODIES, S_RIRF, N_EXC, DT = 64, 1024, 1024, 0.01
FLOPS_PRESSURE, FLOPS_ETA = 75.0, 48.0
FP64_VECTOR_PEAK = 78.6e12  # MI355X FP64 vector rate (FLOP/s, an FMA counted as two)


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


def panels(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-10.0, 10.0, size=(n, 3))
    c[:, 2] = rng.uniform(-20.0, -3.0, size=n)  # all wet
    return c, rng.normal(size=(n, 3)) * 0.1


def states(N, times):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((N, 3))
    rest[:, 0] = 30.0 * np.arange(N)
    m = PrescribedMotion(N, rest, seed=3)
    return [[np.ascontiguousarray(x).reshape(-1) for x in m.state(t)] for t in times]


def configured(HF, config, stretching):
    h, nb, npan = (c3(HF), N_BODIES, 2048) if config == "c3" else (c5(HF), 1, 8192)
    for b in range(nb):
        h.set_surface_panels(b, *panels(npan, 50 + b))
    h.set_nonlinear_options(wave_stretching=bool(stretching))
    return h, nb, npan


def part_a(HF, res, reps):
    for config in ("c3", "c5"):
        for stretching in (1, 0):
            h, nb, npan = configured(HF, config, stretching)
            nf = h.sizes()["nf"]
            st = states(nb, [37.1])[0]
            for _ in range(20):
                h.compute_nonlinear(37.1, st[0], st[1])
            tm = timed(lambda: h.compute_nonlinear(37.1, st[0], st[1]), reps)
            evals = nb * npan * nf
            flop = evals * (FLOPS_PRESSURE + (FLOPS_ETA if stretching else 0.0))
            res[f"a_{config}_{nb}x{npan}x{nf}_stretching{stretching}"] = dict(
                stats_us(tm), panels=nb * npan, nf=nf, panel_component_evaluations=evals, evaluations_per_s_call=evals / float(np.median(tm)),
                counted_flop=flop, fp64_vector_fraction_of_call=flop / float(np.median(tm)) / FP64_VECTOR_PEAK)
            h.close()


def part_k(HF, config, stretching):
    h, nb, _ = configured(HF, config, stretching)
    st = states(nb, [37.1])[0]
    for _ in range(70):
        h.compute_nonlinear(37.1, st[0], st[1])
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
    res["b_hc_step_c3_no_panels"] = dict(windows=step_windows(sts[warm:], times[warm:], windows, per, plain))
    h.close()


def part_c(HF, res, quick):
    from hydrochrono_amd import capi
    dp = (lambda a: a.ctypes.data_as(capi.c_double_p))
    warm, windows, per = (200, 2, 256) if quick else (600, 3, 512)
    times = DT * np.arange(warm + windows * per)
    sts = states(N_BODIES, times)
    for variant in ("step_alone", "begin_step_end"):
        h = c3(HF)
        lib, step = h.lib, capi.step_raw(h.lib)
        for b in range(N_BODIES):
            h.set_surface_panels(b, *panels(2048, 50 + b))
        out = np.empty(h.D_local)
        nl = [np.empty(h.D_local) for _ in range(3)]

        def plain(t, s):
            step(h.ctx, t, s[0].ctypes.data, s[1].ctypes.data, s[2].ctypes.data, s[3].ctypes.data, out.ctypes.data)

        def beside(t, s):
            lib.hc_nonlinear_begin(h.ctx, t, dp(s[0]), dp(s[1]))
            plain(t, s)
            lib.hc_nonlinear_end(h.ctx, dp(nl[0]), dp(nl[1]), dp(nl[2]))

        fn = dict(step_alone=plain, begin_step_end=beside)[variant]
        for k in range(warm):
            fn(times[k], sts[k])
        res["c_" + variant] = dict(windows=step_windows(sts[warm:], times[warm:], windows, per, fn))
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonlinear"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--config", default="c3", choices=("c3", "c5"))
    ap.add_argument("--stretching", type=int, default=1)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces as HF
    if "k" in args.parts:
        part_k(HF, args.config, args.stretching)
        return
    res = {}
    if "a" in args.parts:
        part_a(HF, res, 20 if args.quick else 100)
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
