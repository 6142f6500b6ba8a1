"""Wave kinematics on the GPU (hc_wave_kinematics, csrc/hc_wave_kin.hip): what a call costs and what the kernel sustains.

  (a) single-point call latency (median / p99 of 1000 calls): regular wave (sphere) and the C5 spectrum (2048 components), on an idle
      context and between the steps of a running sphere simulation (irregular waves);
  (b) a 512 x 512 horizontal grid x 1 time on the C5 spectrum, stretching on;
  (c) 1 point x the C5 time grid (the eta table's times, ~12.5 k);
  whether eta at (0, 0, 0) reproduces the eta(t) table bit for bit (sphere, C5);
  the FP64 vector issue rate of this GPU (profiles/fp64_valu_probe.hip, compiled and run here).
Term evaluations: one per point x time x component and pass (stretching: an eta pass, then the kinematics pass).

    python profiles/wave_kinematics_probe.py [--out DIR] [--quick]
--quick: (b) and (c) only, a few calls each -- the run to put under rocprofv3 --kernel-trace --stats.
Writes DIR/probe.json (default profiles/wave_kinematics) and prints it.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

C5_IRREG = dict(simulation_dt=0.08, simulation_duration=1000.0, ramp_duration=20.0, wave_height=6.0, wave_period=10.0,
                frequency_min=0.01, frequency_max=0.6, nfrequencies=2048, peak_enhancement_factor=2.0, seed=4)
SPHERE_IRREG = dict(simulation_dt=0.015, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0, wave_period=12.0,
                    frequency_min=0.001, frequency_max=1.0, nfrequencies=1000)


def stats_us(samples):
    a = 1e6 * np.asarray(samples)
    return dict(median_us=float(np.median(a)), p99_us=float(np.percentile(a, 99)), min_us=float(a.min()), n=int(a.size))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def c5(HF):
    from hydrochrono_amd.synthetic import many_body_case
    h = HF.from_case(many_body_case(1, S=401, dt_rirf=0.05, n_exc=401, dt_exc=0.25, seed=5))
    h.add_waves_irregular(**C5_IRREG)
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wave_kinematics"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from cases import sphere_case
    from hydrochrono_amd.hydro import HydroForces as HF
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    res = {}
    h5 = c5(HF)
    nf = h5.sizes()["nf"]
    p0 = np.zeros((1, 3))

    # (b) 512 x 512 grid x 1 time, stretching on
    xs = np.linspace(-250.0, 250.0, 512)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    grid = np.stack([X.ravel(), Y.ravel(), np.full(X.size, -2.0)], axis=1)
    h5.wave_kinematics(grid, [37.1])  # warm-up (buffers, table)
    reps = 3 if args.quick else 20
    tb = timed(lambda: h5.wave_kinematics(grid, [37.1]), reps)
    terms_b = 2 * grid.shape[0] * nf
    res["b_grid_512x512_c5_stretch"] = dict(stats_us(tb), points=grid.shape[0], times=1, nf=nf, term_evaluations=terms_b,
                                            terms_per_s_call=terms_b / float(np.median(tb)))
    # (c) 1 point x the C5 time grid
    t_c5, table_c5 = h5.irreg_eta()
    h5.wave_kinematics(p0, t_c5)
    tc = timed(lambda: h5.wave_kinematics(p0, t_c5), reps)
    terms_c = 2 * t_c5.size * nf
    res["c_point_x_c5_times"] = dict(stats_us(tc), points=1, times=int(t_c5.size), nf=nf, term_evaluations=terms_c,
                                     terms_per_s_call=terms_c / float(np.median(tc)))
    if not args.quick:
        # eta at the origin against the eta(t) table (t >= ramp: no ramp factor)
        sel = t_c5 >= C5_IRREG["ramp_duration"]
        e = h5.wave_kinematics(p0, t_c5[sel])[0][:, 0]
        res["eta_vs_table_c5"] = dict(bitwise=bool(np.array_equal(e, table_c5[sel])), max_abs_diff=float(np.max(np.abs(e - table_c5[sel]))),
                                      samples=int(sel.sum()))
        hs = HF.from_case(sphere_case())
        hs.add_waves_irregular(**SPHERE_IRREG)
        ts, tabs = hs.irreg_eta()
        sel = ts >= SPHERE_IRREG["ramp_duration"]
        e = hs.wave_kinematics(p0, ts[sel])[0][:, 0]
        res["eta_vs_table_sphere"] = dict(bitwise=bool(np.array_equal(e, tabs[sel])), max_abs_diff=float(np.max(np.abs(e - tabs[sel]))),
                                          samples=int(sel.sum()))
        hs.close()

        # (a) single-point latency, idle
        pt = np.array([[3.0, 0.0, -2.0]])
        hr = HF.from_case(sphere_case())
        hr.add_waves_regular(0.177, 2.094395102)
        for name, h in (("regular_sphere", hr), ("c5_spectrum", h5)):
            for _ in range(50):
                h.wave_kinematics(pt, [1.0])
            res[f"a_single_point_idle_{name}"] = stats_us(timed(lambda: h.wave_kinematics(pt, [1.0]), 1000))
        hr.close()
        # (a) between the steps of a running sphere simulation (irregular waves): only the kinematics call is timed
        case = sphere_case()
        sim = HF.from_case(case)
        sim.add_waves_irregular(**SPHERE_IRREG)
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        lat, step_s = [], []
        for n in range(1100):
            t = 0.015 * n
            st = motion.state(t)
            t0 = time.perf_counter()
            sim.step(t, *st)
            t1 = time.perf_counter()
            sim.wave_kinematics(pt, [t])
            t2 = time.perf_counter()
            if n >= 100:
                step_s.append(t1 - t0)
                lat.append(t2 - t1)
        res["a_single_point_between_steps_sphere_irregular"] = dict(stats_us(lat), step=stats_us(step_s))
        sim.close()

        # FP64 vector issue rate of this GPU, same visit
        os.makedirs(args.out, exist_ok=True)
        exe = os.path.join(args.out, "fp64_valu_probe")
        from hydrochrono_amd.build import _hipcc
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", os.path.join(ROOT, "profiles", "fp64_valu_probe.hip"), "-o", exe], check=True)
        r = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
        os.remove(exe)
        res["fp64_valu"] = json.loads(r.stdout.strip().splitlines()[-1])
        fma = res["fp64_valu"]["fma_per_s"]
        for key in ("b_grid_512x512_c5_stretch", "c_point_x_c5_times"):
            res[key]["call_terms_per_s_over_fp64_fma_per_s"] = res[key]["terms_per_s_call"] / fma
    h5.close()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "probe_quick.json" if args.quick else "probe.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
