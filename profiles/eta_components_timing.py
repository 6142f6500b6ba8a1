"""Timing of the component analysis of an imported eta record (hc_set_eta_record_components; DESIGN 3.7q, MEASURED.md), host clock,
copies, host parts and the residual evaluation included:
  * the sphere fixture (tests/golden/sphere_eta_record.txt, 8001 samples), full band (4000 bins) and the band 0.03-0.4 Hz (45 bins);
  * a record of 2^20 samples with 4096 bins;
  * beside each, NumPy on the host for the same inputs: np.fft.rfft of the samples (every bin at once), and the direct sum per bin
    that the kernel evaluates (timed on 8 bins and scaled to the bin count);
  * one hc_compute_morison (64 bodies x 64 elements) under a record with 512 components next to the same call under a synthesised
    sea of 512 components: the kernels are the same, so the two should agree.
    python profiles/eta_components_timing.py [--reps 20]
Writes profiles/eta_components/timing.json (milliseconds: median, minimum, maximum) and prints it.  No threshold is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "eta_components", "timing.json")
SYNTH_512 = dict(simulation_dt=0.05, simulation_duration=200.0, ramp_duration=0.0, wave_height=4.0, wave_period=9.0,
                 frequency_min=0.02, frequency_max=0.6, nfrequencies=512, peak_enhancement_factor=2.0, seed=4)


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def numpy_direct(eta, bins, reps):
    n = eta.size
    j = np.arange(n, dtype=np.int64)

    def run():
        for m in bins:
            ang = 2 * np.pi * ((m * j) % n) / n
            (eta * np.cos(ang)).sum(), (eta * np.sin(ang)).sum()
    return timed(run, reps, warmup=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd import read_eta_file
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import many_body_case
    res = {}

    one = many_body_case(1, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)
    t, eta = read_eta_file(os.path.join(ROOT, "tests", "golden", "sphere_eta_record.txt"))
    h = HydroForces.from_case(one)
    h.add_waves_irregular_eta(t, eta, 0.015)
    res["fixture_full_band_4000_bins"] = timed(lambda: h.set_eta_record_components(0.0, 1e9), args.reps)
    res["fixture_band_0.03_0.4_hz_45_bins"] = timed(lambda: h.set_eta_record_components(0.03, 0.4), args.reps)
    res["fixture_numpy_rfft"] = timed(lambda: np.fft.rfft(eta), args.reps)
    d = numpy_direct(eta, range(100, 108), max(3, args.reps // 4))
    res["fixture_numpy_direct_sum_4000_bins_scaled_from_8"] = {k: (v * 500.0 if k.endswith("_ms") else v) for k, v in d.items()}
    h.close()

    n = 1 << 20
    rng = np.random.default_rng(3)
    tl = 0.01 * np.arange(n)
    el = np.zeros(n)
    for m in rng.integers(1000, 5096, 40):
        el += rng.uniform(0.01, 0.1) * np.cos(rng.uniform(0, 6.28) - 2 * np.pi * int(m) * np.arange(n) / n)
    h = HydroForces.from_case(one)
    h.add_waves_irregular_eta(tl, el, 0.01)
    T_w = n * (tl[-1] - tl[0]) / (n - 1)
    band = (999.5 / T_w, 5095.5 / T_w)
    h.set_eta_record_components(*band)
    assert h.eta_record_components()["m"].size == 4096
    res["n_2^20_4096_bins"] = timed(lambda: h.set_eta_record_components(*band), max(3, args.reps // 4), warmup=1)
    res["n_2^20_numpy_rfft"] = timed(lambda: np.fft.rfft(el), max(3, args.reps // 4), warmup=1)
    d = numpy_direct(el, range(1000, 1008), 2)
    res["n_2^20_numpy_direct_sum_4096_bins_scaled_from_8"] = {k: (v * 512.0 if k.endswith("_ms") else v) for k, v in d.items()}
    h.close()

    N, E = 64, 64
    case = many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)
    rest = np.zeros((N, 3))
    rest[:, 0] = 15.0 * np.arange(N)
    rest[:, 2] = -1.0
    tq = 55.5
    st = PrescribedMotion(N, rest, seed=8, amplitude=0.5).state(tq)
    nr = 4096
    tr = 0.05 * np.arange(nr)
    er_ = np.zeros(nr)
    for m in range(5, 5 + 600):
        er_ += rng.uniform(0.001, 0.02) * np.cos(rng.uniform(0, 6.28) - 2 * np.pi * m * np.arange(nr) / nr)
    for label in ("record_512_components", "synthesised_512_components"):
        h = HydroForces.from_case(case)
        if label.startswith("record"):
            h.add_waves_irregular_eta(tr, er_, 0.05)
            h.set_eta_record_components(0.0, 1e9, 512)
            assert h.sizes()["nf"] == 512
        else:
            h.add_waves_irregular(**SYNTH_512)
        h.set_morison_options(wave_stretching=False)
        erng = np.random.default_rng(1)
        for b in range(N):
            h.set_morison_elements(b, erng.uniform(-10, 10, (E, 3)), erng.uniform(0, 3, (E, 3)), erng.uniform(0, 4, (E, 3)))
        res[f"morison_64x64_{label}"] = timed(lambda: h.compute_morison(tq, *st), args.reps, warmup=3)
        h.close()

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
