"""Wave kinematics on the GPU (hc_wave_kinematics: WaveBase::GetElevation / GetVelocity / GetAcceleration, include/hydroc/wave_types.h:69-73)
against the tests' NumPy restatement of the reference's formulas (tests/wave_kinematics_ref.py), fed the context's own spectrum /
regular-wave coefficients.

Tolerance per element: |gpu - ref| <= 1e-11 * sum_i |term_i|, where a term's magnitude is taken over its phase (A_i for eta, w_i A_i
|profile_i| for a velocity component, ...): the phase k x - w t + phi carries an absolute rounding error of a few ulp of its own size
in either computation, which a term near its zero crossing cannot scale down."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11
SPHERE_IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0, wave_period=12.0,
                    frequency_min=0.001, frequency_max=1.0, nfrequencies=1000)
C5_IRREG = dict(simulation_dt=0.08, simulation_duration=1000.0, ramp_duration=20.0, wave_height=6.0, wave_period=10.0,
                frequency_min=0.01, frequency_max=0.6, nfrequencies=2048, peak_enhancement_factor=2.0, seed=4)
REG_AMP, REG_OMEGA = 0.177, 2.094395102


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def c5_case():
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(1, S=401, dt_rirf=0.05, n_exc=401, dt_exc=0.25, seed=5)


def grid(xs, zs, y=0.0):
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    return np.stack([X.ravel(), np.full(X.size, y), Z.ravel()], axis=1)


def assert_matches(got, ref, what):
    """got = (eta, vel, acc) of the GPU; ref = ((eta, vel, acc), scales) of the restatement"""
    values, scales = ref
    for g, r, s, name in zip(got, values, scales, ("eta", "velocity", "acceleration")):
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        assert np.all(np.isfinite(g)), (what, name)
        bad = np.abs(g - r) > TOL * s
        assert not bad.any(), f"{what} {name}: {bad.sum()} elements, worst {np.max(np.abs(g - r) / np.maximum(s, 1e-300)):.3e} of sum|term|"


def irregular_comp(h):
    return wk.irregular_components(h.irreg_spectrum())


def regular_comp(h, phase):
    return wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], phase)


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------
# 1-3: the formulas on the three depth situations
# ------------------------------------------------------------------------------------------------
def test_regular_wave_sphere(HF):
    case = sphere_case()
    h = HF.from_case(case)
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    pts = grid(np.linspace(-150, 150, 31), np.linspace(-200, 0, 21), y=2.5)
    times = np.array([0.0, 3.7, 41.3, 200.0])
    for mwl in (0.0, 1.5):
        got = h.wave_kinematics(pts, times, mwl=mwl, regular_phase=0.7)
        ref = wk.kinematics(regular_comp(h, 0.7), case["water_depth"], pts, times, mwl=mwl)
        assert_matches(got, ref, f"regular mwl={mwl}")
        assert np.max(np.abs(got[1])) > 0.1 and np.all(got[1][..., 1] == 0.0) and np.all(got[2][..., 1] == 0.0)
    # the regular wave has no stretching: the option changes nothing
    assert same_bits(h.wave_kinematics(pts, times, regular_phase=0.7, wave_stretching=False), h.wave_kinematics(pts, times, regular_phase=0.7))


def test_irregular_sphere_all_regimes_stretching_on_and_off(HF):
    case = sphere_case()
    h = HF.from_case(case)
    h.add_waves_irregular(**SPHERE_IRREG)
    comp = irregular_comp(h)
    n_long, n_finite, n_kd = wk.regimes(comp, case["water_depth"])
    assert n_long > 0 and n_finite > 0 and n_kd > 0, (n_long, n_finite, n_kd)
    pts = grid(np.linspace(-150, 150, 9), np.array([-200.0, -150.0, -60.0, -12.0, -2.0, 0.0, 0.9]))
    times = np.array([0.0, 77.7, 431.25])
    for stretching in (True, False):
        got = h.wave_kinematics(pts, times, mwl=0.8, wave_stretching=stretching)
        ref = wk.kinematics(comp, case["water_depth"], pts, times, mwl=0.8, stretching=stretching)
        assert_matches(got, ref, f"irregular stretching={stretching}")
    on, off = h.wave_kinematics(pts, times, mwl=0.8), h.wave_kinematics(pts, times, mwl=0.8, wave_stretching=False)
    assert np.array_equal(on[0], off[0]) and not np.array_equal(on[1], off[1])


def test_three_body_infinite_depth(HF):
    """water_depth = +inf: the reference's stretching gives inf / inf = NaN; here the limit z_s = z' - eta."""
    case = three_body_case()
    h = HF.from_case(case)
    h.add_waves_irregular(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
                          frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)
    comp = irregular_comp(h)
    pts = grid(np.linspace(-60, 60, 7), np.array([-80.0, -20.0, -3.0, 0.0]))
    times = np.array([1.0, 12.5, 33.3])
    got = h.wave_kinematics(pts, times, mwl=0.25)
    assert all(np.all(np.isfinite(a)) for a in got)
    assert_matches(got, wk.kinematics(comp, np.inf, pts, times, mwl=0.25, stretching=True), "infinite depth, stretching (limit)")
    got = h.wave_kinematics(pts, times, mwl=0.25, wave_stretching=False)
    assert_matches(got, wk.kinematics(comp, np.inf, pts, times, mwl=0.25, stretching=False), "infinite depth, plain deep formula")


# ------------------------------------------------------------------------------------------------
# 4-5: agreement with the eta(t) table and between the two irregular modes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "c5"])
def test_eta_at_origin_matches_the_eta_table(HF, which):
    case, kw = (sphere_case(), SPHERE_IRREG) if which == "sphere" else (c5_case(), C5_IRREG)
    h = HF.from_case(case)
    h.add_waves_irregular(**kw)
    t, table = h.irreg_eta()
    sel = t >= kw["ramp_duration"]
    eta = h.wave_kinematics(np.zeros((1, 3)), t[sel])[0][:, 0]
    amp_sum = np.sum(irregular_comp(h)[0])
    assert np.max(np.abs(eta - table[sel])) <= 1e-13 * amp_sum


def test_spectral_and_irf_modes_give_the_same_bits(HF):
    case = sphere_case()
    a, b = HF.from_case(case), HF.from_case(case)
    a.add_waves_irregular(**SPHERE_IRREG)
    b.add_waves_irregular(spectral=True, **SPHERE_IRREG)
    pts = grid(np.linspace(-100, 100, 5), np.array([-50.0, -5.0, 0.0]))
    times = np.array([0.0, 10.0, 123.0])
    for st in (True, False):
        assert same_bits(a.wave_kinematics(pts, times, mwl=0.3, wave_stretching=st), b.wave_kinematics(pts, times, mwl=0.3, wave_stretching=st))


# ------------------------------------------------------------------------------------------------
# 6: batch invariance (512 x 512 horizontal grid of the C5 spectrum)
# ------------------------------------------------------------------------------------------------
def test_batch_invariance_c5_grid(HF):
    h = HF.from_case(c5_case())
    h.add_waves_irregular(**C5_IRREG)
    xs = np.linspace(-250.0, 250.0, 512)
    X, Y = np.meshgrid(xs, xs, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), np.full(X.size, -2.0)], axis=1)
    t0 = 37.1
    big = h.wave_kinematics(pts, [t0])
    rng = np.random.default_rng(11)
    pick = rng.choice(pts.shape[0], 200, replace=False)
    for p in pick[:40]:
        one = h.wave_kinematics(pts[p:p + 1], [t0])
        assert same_bits(one, tuple(a[:, p:p + 1] for a in big)), p
    assert_matches(tuple(a[:, pick] for a in big), wk.kinematics(irregular_comp(h), np.inf, pts[pick], [t0], stretching=True), "C5 grid subset")
    # a P x T batch: every (point, time) equals its single call
    times = np.array([0.0, 5.5, 250.25, 999.0])
    sub = pts[pick[:50]]
    pt = h.wave_kinematics(sub, times, mwl=0.1)
    for j in (0, 3):
        for i in (0, 17, 49):
            one = h.wave_kinematics(sub[i:i + 1], times[j:j + 1], mwl=0.1)
            assert same_bits(one, tuple(a[j:j + 1, i:i + 1] for a in pt)), (i, j)


# ------------------------------------------------------------------------------------------------
# 7: NoWave, NULL outputs, empty batches, bad arguments, cache invalidation
# ------------------------------------------------------------------------------------------------
def raw_call(h, P, xyz, T, t, eta=None, vel=None, acc=None, mwl=0.0, phase=0.0, stretching=1):
    from hydrochrono_amd import capi
    o = capi.WaveKinematicsOpts()
    h.lib.hc_wave_kinematics_opts_default(C.byref(o))
    assert (o.mwl, o.regular_phase, o.wave_stretching) == (0.0, 0.0, 1)
    o.mwl, o.regular_phase, o.wave_stretching = mwl, phase, stretching
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    return h.lib.hc_wave_kinematics(h.ctx, C.byref(o), P, dp(xyz), T, dp(t), dp(eta), dp(vel), dp(acc))


def test_nowave_null_outputs_empty_batches_bad_arguments_and_cache(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    case = sphere_case()
    pts = grid(np.linspace(-30, 30, 4), np.array([-10.0, 0.0]))
    times = np.array([0.0, 2.0, 9.0])
    # not finalized
    raw = HF(1)
    assert raw_call(raw, 1, np.zeros(3), 1, np.zeros(1), eta=np.empty(1)) == capi.HC_ERR_INVALID
    raw.close()
    h = HF.from_case(case)
    # no model set (the NoWave of hc_finalize) and NoWave: zeros
    for _ in range(2):
        e, v, a = h.wave_kinematics(pts, times)
        assert not e.any() and not v.any() and not a.any() and e.shape == (3, 8) and v.shape == (3, 8, 3)
        h.add_waves_none()
    h.add_waves_irregular(**SPHERE_IRREG)
    full = h.wave_kinematics(pts, times, mwl=0.2)
    xyz, n = np.ascontiguousarray(pts.reshape(-1)), pts.size // 3 * times.size
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 0, 0)):
        outs = [np.full(k * n, 7.0) if m else None for m, k in zip(mask, (1, 3, 3))]
        assert raw_call(h, 8, xyz, 3, times, *outs, mwl=0.2) == capi.HC_OK
        for o, f in zip(outs, full):
            if o is not None:
                assert np.array_equal(o, f.reshape(-1))
    # empty batches
    for P, T in ((0, 3), (8, 0), (0, 0)):
        e, v, a = h.wave_kinematics(pts[:P], times[:T])
        assert e.shape == (T, P) and v.shape == (T, P, 3)
    assert raw_call(h, 0, None, 3, times, np.empty(1)) == capi.HC_OK
    assert raw_call(h, 8, xyz, 0, None, np.empty(1)) == capi.HC_OK
    # bad arguments
    one = np.empty(3)
    assert raw_call(h, -1, xyz, 3, times, one) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, xyz, -2, times, one) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, None, 3, times, one) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, xyz, 3, None, one) == capi.HC_ERR_INVALID
    for col, bad in ((0, np.nan), (2, np.inf), (0, -np.inf)):
        b = xyz.copy()
        b[3 + col] = bad
        assert raw_call(h, 8, b, 3, times, one) == capi.HC_ERR_INVALID
    for bad in (np.nan, np.inf):
        assert raw_call(h, 8, xyz, 3, np.array([0.0, bad, 1.0]), one) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, xyz, 3, times, one, mwl=np.nan) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, xyz, 3, times, one, phase=np.nan) == capi.HC_ERR_INVALID
    with pytest.raises(HydroError):
        h.wave_kinematics([[0.0, 0.0, np.nan]], [0.0])
    # the y coordinate does not enter
    b = xyz.copy()
    b[1::3] = np.nan
    e = np.empty(n)
    assert raw_call(h, 8, b, 3, times, e, mwl=0.2) == capi.HC_OK and np.array_equal(e, full[0].reshape(-1))
    # a new wave model voids the cached table: regular -> other regular -> irregular with another seed -> the first again
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    r1 = h.wave_kinematics(pts, times, regular_phase=0.4)
    assert_matches(r1, wk.kinematics(regular_comp(h, 0.4), case["water_depth"], pts, times), "regular after irregular")
    r2 = h.wave_kinematics(pts, times, regular_phase=1.1)  # (the phase is part of the cached table)
    assert_matches(r2, wk.kinematics(regular_comp(h, 1.1), case["water_depth"], pts, times), "regular, another phase")
    h.add_waves_regular(0.3, 1.5)
    r3 = h.wave_kinematics(pts, times, regular_phase=1.1)
    assert_matches(r3, wk.kinematics(wk.regular_components(0.3, 1.5, h.regular_coeffs()[2], 1.1), case["water_depth"], pts, times),
                   "second regular wave")
    h.add_waves_irregular(**dict(SPHERE_IRREG, seed=9))
    i9 = h.wave_kinematics(pts, times, mwl=0.2)
    assert not np.array_equal(i9[0], full[0])
    assert_matches(i9, wk.kinematics(irregular_comp(h), case["water_depth"], pts, times, mwl=0.2, stretching=True), "irregular seed 9")
    h.add_waves_irregular(**SPHERE_IRREG)
    assert same_bits(h.wave_kinematics(pts, times, mwl=0.2), full)


# ------------------------------------------------------------------------------------------------
# 8-9: shards, forces
# ------------------------------------------------------------------------------------------------
def test_every_shard_answers_with_the_same_bits(HF):
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    kw = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
              frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)
    whole = HF.from_case(case)
    whole.add_waves_irregular(**kw)
    group = HydroGroup.from_case(case, 3)
    group.add_waves_irregular(**kw)
    pts = grid(np.linspace(-60, 60, 5), np.array([-30.0, -1.0, 0.5]))
    times = np.array([0.0, 3.3, 20.0])
    ref = whole.wave_kinematics(pts, times, mwl=0.1)
    for sh in group.shards:
        assert same_bits(sh.wave_kinematics(pts, times, mwl=0.1), ref), (sh.b0, sh.b1)
    assert same_bits(group.wave_kinematics(pts, times, mwl=0.1), ref)


@pytest.mark.parametrize("ahead", [0, 1])
def test_kinematics_between_steps_change_no_force(HF, ahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_calls in (False, True):
        h = HF.from_case(case)
        h.set_pass_schedule(ahead)
        h.add_waves_irregular(**SPHERE_IRREG)
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        pts = grid(np.linspace(-20, 20, 3), np.array([-5.0, 0.0]))
        forces = []
        for n in range(300):
            t = SPHERE_DT * n
            forces.append(h.step(t, *motion.state(t)))
            if with_calls:
                h.wave_kinematics(pts, [t])
        runs.append(np.array(forces))
        h.close()
    assert np.array_equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# 10: the C++ mirror (shared_ptr<WaveBase>) gives the bits of the Python ABI
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches_the_python_abi(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "wave_kinematics_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "wave_kinematics_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    for mode in ("none", "regular", "irregular", "irregular_nostretch"):
        r = subprocess.run([exe, h5, mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.returncode, r.stderr)
        rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
        assert rows.shape == (12, 11)
        h = HF(1)
        h.load_bemio_h5(h5)
        h.finalize()
        if mode == "regular":
            h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
        elif mode != "none":
            h.add_waves_irregular(**dict(SPHERE_IRREG, simulation_dt=0.015))
        pts, times = rows[:4, 1:4], rows[::4, 0]
        e, v, a = h.wave_kinematics(pts, times, mwl=0.5, regular_phase=0.3, wave_stretching=mode != "irregular_nostretch")
        assert np.array_equal(rows[:, 4], e.reshape(-1)), mode
        assert np.array_equal(rows[:, 5:8], v.reshape(-1, 3)), mode
        assert np.array_equal(rows[:, 8:11], a.reshape(-1, 3)), mode
        if mode == "none":
            assert not rows[:, 4:].any()
        else:
            assert np.abs(rows[:, 4]).max() > 0.01
        h.close()
