"""Irregular waves from an imported free-surface record on the GPU (hc_set_wave_irregular_eta, HydroForces.add_waves_irregular_eta,
IrregularWaves with eta_file_path_).  The per-step path is the excitation convolution of synthesised irregular waves; what is new is
the table it interpolates in -- the record, zero-extended over the excitation IRF -- and the search hint of that table.

  * a synthesised table imported as a record gives the synthesised forces bit for bit (same grid, same cells);
  * the reference's record and non-uniform records against a NumPy restatement  f[row](t) = sum_l Kex[row, l] eta_ext(t - tau_l) w_l;
  * the hint: a coarse record costs no more per step than the same record on the step grid;
  * the excitation window, the queries, switching back, row shards, and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN_DIR, "sphere_eta_record.txt")
SPHERE_IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0, wave_period=12.0,
                    frequency_min=0.001, frequency_max=1.0, nfrequencies=1000)
WINDOW_MSG = "Excitation convolution: trying to find free surface elevation at a time out of bounds"


@pytest.fixture(scope="module")
def hydro():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd import hydro
    return hydro


def motion_for(case, seed):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    return PrescribedMotion(case["N"], [b["cg"] for b in case["bodies"]], seed=seed)


def drive(h, times, motion):
    """totals and wave components of every step"""
    tot, wav = [], []
    for t in times:
        tot.append(h.step(t, *motion.state(t)))
        wav.append(h.components()[2])
    return np.array(tot), np.array(wav)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def extended(t, eta, tau):
    """the zero extension of include/hydrochrono_amd.h, restated"""
    h = (t[-1] - t[0]) / (t.size - 1)
    nf = int(np.ceil(max(tau.max(), 0.0) / h)) + 1
    nb = int(np.ceil(max(-tau.min(), 0.0) / h)) + 1
    te = np.concatenate([t[0] - np.arange(nf, 0, -1) * h, t, t[-1] + np.arange(1, nb + 1) * h])
    ee = np.concatenate([np.zeros(nf), eta, np.zeros(nb)])
    return te, ee


def numpy_waves(h, t_rec, eta_rec, times):
    """per-step wave force of every local body: sum_l Kex[row, l] * eta_ext(t - tau_l) * w_l"""
    out = []
    for b in range(h.b0, h.b1):
        tau, w, K = h.irreg_irf(b)
        te, ee = extended(t_rec, eta_rec, tau)
        rows = []
        for chunk in np.array_split(np.asarray(times), max(1, len(times) // 256)):
            q = chunk[:, None] - tau[None, :]
            e = np.interp(q.ravel(), te, ee).reshape(q.shape) * w[None, :]
            rows.append(e @ K.T)
        out.append(np.concatenate(rows))
    return np.concatenate(out, axis=1)


def assert_close(got, ref, what):
    scale = np.abs(ref).max()
    assert scale > 0, what
    err = np.abs(got - ref).max()
    assert err <= 1e-12 * scale, f"{what}: max |gpu - numpy| = {err:.3e} = {err / scale:.3e} of max|f|"


def sphere(hydro, lookahead=32):
    h = hydro.HydroForces.from_case(sphere_case())
    h.set_pass_schedule(0)
    h.set_lookahead(lookahead)
    return h


# ------------------------------------------------------------------------------------------------
# 1: a synthesised table imported as a record gives the synthesised forces bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [1, 0])
@pytest.mark.parametrize("lookahead", [0, 16, 32])
def test_round_trip_of_a_synthesised_table_is_bitwise(hydro, lookahead, direct, monkeypatch):
    monkeypatch.setenv("HC_DIRECT", str(direct))
    a, b = sphere(hydro, lookahead), sphere(hydro, lookahead)
    assert a.direct_dispatch()[0] == bool(direct), a.direct_dispatch()[1]
    a.add_waves_irregular(**SPHERE_IRREG)
    t_tab, eta_tab = a.irreg_eta()
    b.add_waves_irregular_eta(t_tab, eta_tab, SPHERE_DT)
    times = 90.0 + SPHERE_DT * np.arange(300)
    ra, rb = drive(a, times, motion_for(sphere_case(), 7)), drive(b, times, motion_for(sphere_case(), 7))
    assert np.abs(ra[1]).max() > 1e3
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


@pytest.mark.parametrize("lookahead", [0, 32])
def test_round_trip_between_table_samples_is_bitwise(hydro, lookahead):
    """steps of 0.007 s on a 0.015 s table: every query interpolates inside a cell, and both contexts must pick the same cell"""
    a, b = sphere(hydro, lookahead), sphere(hydro, lookahead)
    a.add_waves_irregular(**SPHERE_IRREG)
    b.add_waves_irregular_eta(*a.irreg_eta(), SPHERE_DT)
    times = 100.0 + 0.007 * np.arange(400)
    ra, rb = drive(a, times, motion_for(sphere_case(), 8)), drive(b, times, motion_for(sphere_case(), 8))
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


# ------------------------------------------------------------------------------------------------
# 2-3: records against the NumPy restatement
# ------------------------------------------------------------------------------------------------
def test_reference_record_against_numpy(hydro):
    t_rec, eta_rec = hydro.read_eta_file(FIXTURE)
    h = sphere(hydro)
    h.add_waves_irregular_eta(t_rec, eta_rec, SPHERE_DT)
    times = t_rec[::4]  # 0 .. 120 s (t = 0: half of the IRF reaches into the zero extension before the record)
    assert times[0] == 0.0 and times[-1] == 120.0
    _, wav = drive(h, times, motion_for(sphere_case(), 9))
    assert_close(wav, numpy_waves(h, t_rec, eta_rec, times), "sphere record")
    assert np.abs(wav[0]).max() > 0.0


def test_non_uniform_record_against_numpy(hydro):
    rng = np.random.default_rng(11)
    t_rec = np.concatenate([[0.0], np.cumsum(0.01 * (1.0 + rng.uniform(-0.3, 0.3, 2999)))])
    eta_rec = 0.8 * np.sin(2 * np.pi * t_rec / 9.0) + 0.3 * np.cos(2 * np.pi * t_rec / 3.7 + 1.0)
    h = sphere(hydro)
    h.add_waves_irregular_eta(t_rec, eta_rec, 0.01)
    times = 5.0 + 0.01 * np.arange(300)
    _, wav = drive(h, times, motion_for(sphere_case(), 10))
    assert_close(wav, numpy_waves(h, t_rec, eta_rec, times), "jittered record")


def test_coarse_record_uses_its_own_spacing_as_search_hint(hydro):
    """a record at 0.05 s driven at 0.01 s: right against NumPy, and per step no dearer than the same record resampled to 0.01 s
    (a hint of 0.01 s would send every query of the coarse record on a walk over thousands of entries)"""
    t_coarse = 0.05 * np.arange(40001)  # 0 .. 2000 s
    eta_fn = lambda t: np.sin(2 * np.pi * t / 11.0) + 0.4 * np.sin(2 * np.pi * t / 5.3 + 0.5)  # noqa: E731
    t_fine = 0.01 * np.arange(200001)
    times = 1500.0 + 0.01 * np.arange(200)
    per_step = []
    for t_rec in (t_coarse, t_fine):
        h = sphere(hydro, lookahead=0)
        h.add_waves_irregular_eta(t_rec, eta_fn(t_rec), 0.01)
        h.enable_profiling(1)
        _, wav = drive(h, times, motion_for(sphere_case(), 12))
        p = h.profile()
        per_step.append((p["hydrostatics_seconds"] + p["radiation_seconds"] + p["waves_seconds"]) / len(times))
        assert_close(wav, numpy_waves(h, t_rec, eta_fn(t_rec), times), f"record at {t_rec[1]:g} s")
        h.close()
    assert per_step[1] > 0.0
    assert per_step[0] < 3.0 * per_step[1], f"coarse record {per_step[0] * 1e6:.1f} us per step, fine {per_step[1] * 1e6:.1f} us"


# ------------------------------------------------------------------------------------------------
# 4-5: window, queries, switching back
# ------------------------------------------------------------------------------------------------
def test_window_ends_with_the_record(hydro):
    t_rec, eta_rec = hydro.read_eta_file(FIXTURE)
    h = sphere(hydro)
    h.add_waves_irregular_eta(t_rec, eta_rec, SPHERE_DT)
    motion = motion_for(sphere_case(), 13)
    times = t_rec[-60:]
    for t in times:
        h.step(t, *motion.state(t))
    hstep = (t_rec[-1] - t_rec[0]) / (t_rec.size - 1)
    bad = t_rec[-1] + 2 * hstep
    with pytest.raises(hydro.HydroError, match=WINDOW_MSG) as e:
        h.step(bad, *motion.state(bad))
    assert e.value.status == 1
    # the context stays usable: a fresh history inside the record
    h.reset_history()
    _, wav = drive(h, t_rec[:50], motion)
    assert_close(wav, numpy_waves(h, t_rec, eta_rec, t_rec[:50]), "after the window error")


def test_queries_on_a_record(hydro, tmp_path):
    from hydrochrono_amd import capi
    t_rec, eta_rec = hydro.read_eta_file(FIXTURE)
    h = sphere(hydro)
    h.add_waves_irregular_eta(t_rec, eta_rec, SPHERE_DT)
    t, eta = h.irreg_eta()
    assert np.array_equal(t, t_rec) and np.array_equal(eta, eta_rec)
    s = h.sizes()
    assert s["nf"] == 0 and s["nt"] == t_rec.size and s["L"] > 0
    assert all(v.size == 0 for v in h.irreg_spectrum().values())
    pts = np.array([[0.0, 0.0, 0.0], [10.0, 1.0, -3.0]])
    e, v, a = h.wave_kinematics(pts, [0.0, 33.3])
    assert not e.any() and not v.any() and not a.any()
    with pytest.raises(hydro.HydroError) as err:
        h.export_irregular_inputs_h5(str(tmp_path / "out.h5"))
    assert err.value.status == capi.HC_ERR_INVALID and "eta record" in str(err.value)
    # bad records are refused and leave the model in force
    for bad_t in (t_rec[:1], np.array([0.0, 1.0, 1.0]), np.array([0.0, np.nan, 2.0])):
        with pytest.raises(hydro.HydroError) as err:
            h.add_waves_irregular_eta(bad_t, np.zeros(bad_t.size), SPHERE_DT)
        assert err.value.status == capi.HC_ERR_INVALID
    with pytest.raises(hydro.HydroError):
        h.add_waves_irregular_eta(t_rec, eta_rec, 0.0)


def test_switching_back_to_synthesised_waves(hydro):
    times = 90.0 + SPHERE_DT * np.arange(200)
    fresh = sphere(hydro)
    fresh.add_waves_irregular(**SPHERE_IRREG)
    ref = drive(fresh, times, motion_for(sphere_case(), 14))
    h = sphere(hydro)
    t_rec, eta_rec = hydro.read_eta_file(FIXTURE)
    h.add_waves_irregular_eta(t_rec, eta_rec, SPHERE_DT)
    drive(h, t_rec[1000:1100], motion_for(sphere_case(), 15))
    h.add_waves_irregular(**SPHERE_IRREG)
    h.reset_history()
    got = drive(h, times, motion_for(sphere_case(), 14))
    assert same_bits(ref[0], got[0]) and same_bits(ref[1], got[1])
    assert same_bits(np.concatenate(fresh.irreg_eta()), np.concatenate(h.irreg_eta()))
    assert h.sizes()["nf"] == 1000


# ------------------------------------------------------------------------------------------------
# 6: row shards
# ------------------------------------------------------------------------------------------------
def test_shards_gather_the_unsharded_bits(hydro):
    case = three_body_case()
    t_rec = 0.01 * np.arange(2001)
    eta_rec = 1.2 * np.sin(2 * np.pi * t_rec / 6.0) * np.cos(2 * np.pi * t_rec / 17.0)
    whole = hydro.HydroForces.from_case(case)
    whole.set_pass_schedule(0)
    whole.add_waves_irregular_eta(t_rec, eta_rec, 0.01)
    group = hydro.HydroGroup.from_case(case, 2)
    group.set_pass_schedule(0)
    group.add_waves_irregular_eta(t_rec, eta_rec, 0.01)
    times = 2.0 + 0.01 * np.arange(300)
    rw, rg = drive(whole, times, motion_for(case, 16)), drive(group, times, motion_for(case, 16))
    assert np.abs(rw[1]).max() > 0.0
    assert same_bits(rw[0], rg[0]) and same_bits(rw[1], rg[1])
    assert_close(rw[1], numpy_waves(whole, t_rec, eta_rec, times), "three bodies")


# ------------------------------------------------------------------------------------------------
# 7: the C++ mirror (the eta-import demo's call sequence) gives the bits of the Python path
# ------------------------------------------------------------------------------------------------
def test_cpp_demo_matches_the_python_path(hydro, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    exe = str(tmp_path / "eta_import_demo")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "chrono_stub"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "eta_import_demo.cpp"), "-o", exe,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5, FIXTURE, "300"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "spectrum Spectrum has not been created. Initialize with wave height and period to create spectrum."
    assert lines[1] == "frequencies 0"
    assert lines[2].split()[:2] == ["table", "8001"] and [float(v) for v in lines[2].split()[2:]] == [0.0, 120.0]
    assert lines[3] == "mesh fse_mesh.obj" and (tmp_path / "fse_mesh.obj").stat().st_size > 0
    rows = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[4:] if ln.startswith("w ")])
    steps = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[4:] if ln.startswith("s ")])
    assert rows.shape == (200, 7) and steps.shape == (300, 2)
    assert np.all(np.isfinite(steps)) and np.ptp(steps[:, 1]) > 0.0  # the sphere moves under the record's waves
    h = hydro.HydroForces(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular_eta(*hydro.read_eta_file(FIXTURE), SPHERE_DT)
    py = np.array([h.compute_waves(t) for t in rows[:, 0]])
    assert np.abs(py).max() > 0.0
    assert np.array_equal(rows[:, 1:], py)
