"""Wave components of an imported eta record on the GPU (hc_set_eta_record_components; csrc/hc_eta_components.hip: eta_dft_kernel,
eta_residual_kernel) against the long double NumPy restatement (tests/eta_components_ref.py), and the terms that wake up under a
record once it has components: hc_wave_kinematics, the Morison elements, the nonlinear surface pressure, the drift and sum-frequency
QTF forces and the second-order sums, each through the kernel it already had.

Tolerances.  Recovery: A within 1e-12 max A, phi within 1e-11 rad, every other bin below 1e-12 max A -- the yardstick itself recovers
A to 3e-15, phi to 3e-13 rad and leaves 7e-14 in the other bins (tests/test_eta_components_cpu.py); the margin covers the FP64 sincos
and the tree order.  Reconstruction: 8 * 2^-52 * sum A_i (1 + w_i |t|) per time, the rounding of the phase w_i t and of the sum.
Side terms against the regular wave of the same (A, w, phi): 1e-11 of each quantity's maximum -- the amplitude recovery of 1e-12
passes through at most a quadratic term."""
import math
import os
import subprocess

import numpy as np
import pytest

import eta_components_ref as er
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN_DIR, "sphere_eta_record.txt")
H = 0.05
RECOVERY = [(64, 0.0), (257, 3.7), (4096, -5.0)]


@pytest.fixture(scope="module")
def hydro():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd import hydro
    return hydro


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def sphere(hydro):
    h = hydro.HydroForces.from_case(sphere_case())
    h.set_pass_schedule(0)
    return h


def with_record(hydro, t, eta, dt=H):
    h = sphere(hydro)
    h.add_waves_irregular_eta(t, eta, dt)
    return h


_records = {}


def recovery_record(n, t0):
    if (n, t0) not in _records:
        comps = er.five_cosines(n)
        _records[(n, t0)] = (comps,) + er.on_grid_record(n, t0, H, comps)
    return _records[(n, t0)]


def wrap(d):
    return (d + np.pi) % (2 * np.pi) - np.pi


# ------------------------------------------------------------------------------------------------
# 1: recovery of cosines on the record's own grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,t0", RECOVERY)
def test_recovery_of_cosines_on_the_grid(hydro, n, t0):
    comps, t, eta = recovery_record(n, t0)
    h = with_record(hydro, t, eta)
    h.set_eta_record_components(0.0, 1e9)
    c = h.eta_record_components()
    assert list(c["m"]) == list(range(1, n // 2 + 1)) and h.sizes()["nf"] == n // 2
    assert (n // 2 in [m for m, _, _ in comps]) == (n == 64)  # the 64-sample case includes the Nyquist bin
    yard = er.analyse(t, eta, 0.0, np.inf)
    amax = max(a for _, a, _ in comps)
    A = c["A"].copy()
    for m, a, phi in comps:
        dA, dphi = abs(A[m - 1] - a), abs(wrap(c["phase"][m - 1] - phi))
        print(f"n={n} m={m}: |A - A0| = {dA:.3e}, |phi - phi0| = {dphi:.3e}; yardstick {abs(yard['A'][m - 1] - a):.3e}, "
              f"{abs(wrap(yard['phase'][m - 1] - phi)):.3e}")
        assert dA <= 1e-12 * amax and dphi <= 1e-11
        assert abs(A[m - 1] - yard["A"][m - 1]) <= 1e-12 * amax and abs(wrap(c["phase"][m - 1] - yard["phase"][m - 1])) <= 1e-11
        A[m - 1] = 0.0
    print(f"n={n}: largest other bin {A.max():.3e} (yardstick {np.delete(yard['A'], [m - 1 for m, _, _ in comps]).max():.3e})")
    assert A.max() <= 1e-12 * amax
    T_w = n * er.mean_spacing(t)
    assert np.array_equal(c["f"], c["m"] / T_w)
    sp = h.irreg_spectrum()
    assert same_bits(sp["f"], c["f"]) and same_bits(sp["df"], np.full(n // 2, 1.0 / T_w)) and same_bits(sp["S"], c["A"] ** 2 / (2.0 * (1.0 / T_w)))
    assert same_bits(sp["phase"], c["phase"]) and same_bits(sp["k"], c["k"])
    from hydrochrono_amd import capi
    lib = capi.load()
    case = sphere_case()
    k_ref = np.array([lib.hc_host_wave_number(2 * np.pi * f, case["water_depth"], case["g"]) for f in c["f"]])
    assert same_bits(c["k"], k_ref)
    h.close()


# ------------------------------------------------------------------------------------------------
# 2: a bin's bits depend on the record and on m only
# ------------------------------------------------------------------------------------------------
def test_a_bins_bits_do_not_depend_on_the_band_or_the_shard(hydro):
    _, t, eta = recovery_record(257, 3.7)
    h = with_record(hydro, t, eta)
    h.set_eta_record_components(0.0, 1e9)
    full = h.eta_record_components()
    T_w = 257 * er.mean_spacing(t)
    h.set_eta_record_components(50 / T_w, 60 / T_w)
    part = h.eta_record_components()
    assert list(part["m"]) == list(range(50, 61))
    sel = part["m"] - 1
    assert same_bits(part["A"], full["A"][sel]) and same_bits(part["phase"], full["phase"][sel]) and same_bits(part["k"], full["k"][sel])
    h.set_eta_record_components(51 / T_w, 51 / T_w)  # one bin: the one the record has a cosine in
    one = h.eta_record_components()
    assert list(one["m"]) == [51] and same_bits(one["A"], full["A"][50:51]) and same_bits(one["phase"], full["phase"][50:51])
    h.close()
    group = hydro.HydroGroup.from_case(three_body_case(), 2)
    group.add_waves_irregular_eta(t, eta, H)
    group.set_eta_record_components(0.0, 1e9)
    for shard in group.shards:
        c = shard.eta_record_components()
        assert same_bits(c["A"], full["A"]) and same_bits(c["phase"], full["phase"]) and list(c["m"]) == list(full["m"])
    group.close()


# ------------------------------------------------------------------------------------------------
# 3: the fixture: the components give the record back
# ------------------------------------------------------------------------------------------------
def test_reconstruction_of_the_sphere_record(hydro):
    t, eta = hydro.read_eta_file(FIXTURE)
    assert t.size == 8001 and er.is_uniform(t)
    h = with_record(hydro, t, eta, SPHERE_DT)
    h.set_eta_record_components(0.0, 1e9, 0)
    c = h.eta_record_components()
    assert c["m"].size == 4000
    e = h.wave_kinematics(np.zeros((1, 3)), t)[0][:, 0]
    w = 2 * np.pi * c["f"]
    bound = 8 * 2.0 ** -52 * ((c["A"][None, :] * (1.0 + w[None, :] * np.abs(t)[:, None])).sum(axis=1))
    err = np.abs(c["mean"] + e - eta)
    print(f"reconstruction: max |mean + eta_gpu - record| = {err.max():.3e} (max |eta| = {np.abs(eta).max():.3f}), worst err / bound = "
          f"{(err / bound).max():.3e}, bound at t = 120 s: {bound[-1]:.3e}; full-band rms residual {c['rms_residual']:.3e}")
    assert np.all(err <= bound)
    assert abs(np.abs(eta).max() - 1.09) < 0.005
    # the band 0.03 - 0.4 Hz: 45 components, 0.9885 of the variance, an RMS residual of 0.107 standard deviations
    h.set_eta_record_components(0.03, 0.4)
    c = h.eta_record_components()
    ref = er.analyse(t, eta, 0.03, 0.4)
    assert c["m"].size == 45 and list(c["m"]) == list(ref["m"]) and h.sizes()["nf"] == 45
    std = float(np.std(eta))
    print(f"band 0.03-0.4 Hz: share {c['variance_share']:.12f} (numpy {ref['variance_share']:.12f}), rms / std {c['rms_residual'] / std:.12f} "
          f"(numpy {ref['rms_residual'] / ref['std']:.12f}), mean {c['mean']:.6e}")
    assert round(ref["variance_share"], 4) == 0.9885 and round(ref["rms_residual"] / ref["std"], 3) == 0.107
    assert abs(c["variance_share"] - ref["variance_share"]) <= 1e-9
    assert abs(c["rms_residual"] / std - ref["rms_residual"] / ref["std"]) <= 1e-9
    assert abs(c["mean"] - ref["mean"]) <= 1e-15
    h.close()


# ------------------------------------------------------------------------------------------------
# 4: a non-uniform record is analysed through its interpolant at mean spacing
# ------------------------------------------------------------------------------------------------
def test_non_uniform_record(hydro):
    _, t, eta = recovery_record(257, 3.7)
    rng = np.random.default_rng(21)
    tj = t.copy()
    tj[1:-1] += rng.uniform(-0.3, 0.3, t.size - 2) * H
    ej = np.interp(tj, t, eta) + 0.05 * np.sin(7.0 * tj)
    assert not er.is_uniform(tj)
    h = with_record(hydro, tj, ej)
    h.set_eta_record_components(0.0, 1e9)
    c = h.eta_record_components()
    ref = er.analyse(tj, ej, 0.0, np.inf)  # np.interp at mean spacing, then the long double DFT
    amax = ref["A"].max()
    d = np.abs(c["A"] * np.exp(1j * c["phase"]) - ref["A"] * np.exp(1j * ref["phase"]))
    print(f"jittered record: max |c_gpu - c_numpy| = {d.max():.3e} = {d.max() / amax:.3e} of max A")
    assert list(c["m"]) == list(ref["m"]) and d.max() <= 1e-12 * amax
    assert abs(c["mean"] - ref["mean"]) <= 1e-15 and abs(c["variance_share"] - ref["variance_share"]) <= 1e-9
    h.close()


# ------------------------------------------------------------------------------------------------
# 5: the side terms wake up: a single on-grid cosine against the regular wave of the same (A, w, phi)
# ------------------------------------------------------------------------------------------------
N1, M1, A1, PHI1 = 512, 16, 0.4, 0.9
TIMES1 = (3.3, 11.05, 21.7)  # inside the record 0 .. 25.55 s
POINTS = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, -1.0], [-7.5, 2.0, -4.0], [12.0, -3.0, -0.5], [0.4, 0.0, -9.0], [25.0, 1.0, -2.5],
                   [-2.0, 0.0, 0.2], [6.0, 0.0, -15.0]])
EL_R = np.array([[0.0, 0.0, -1.0], [1.5, 0.5, -3.0], [-2.0, 1.0, -0.5], [0.5, -1.0, -6.0]])
EL_CD = np.array([[1.2, 1.2, 0.3], [0.8, 1.0, 0.5], [2.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
EL_CM = np.array([[2.0, 2.0, 0.0], [1.0, 1.5, 0.5], [0.0, 0.0, 0.0], [3.0, 3.0, 1.0]])
QTF_W = np.array([2.0, 3.0, 4.5, 6.0])  # a 4-frequency table around w = 3.927 rad/s


def cone_mesh():
    """20 triangles: an upright cone, apex 3 m below the body reference, rim 1.5 m above it -- the free surface cuts every one"""
    ang = 2 * np.pi * np.arange(21) / 20
    rim = np.stack([2.0 * np.cos(ang), 2.0 * np.sin(ang), np.full(21, 1.5)], axis=1)
    apex = np.array([0.0, 0.0, -3.0])
    return np.array([[apex, rim[i + 1], rim[i]] for i in range(20)])  # counter-clockwise seen from the water (outside)


def qtf_tables():
    d, i, j = np.meshgrid(np.arange(6.0), np.arange(4.0), np.arange(4.0), indexing="ij")
    P = 1000.0 * (d + 1) + 150.0 * (i + j) + 40.0 * i * j
    Q = 60.0 * (i - j) + 5.0 * d
    return P, Q


def state1(t):
    pos = np.array([0.5 + 0.1 * t, 0.2, -2.0 + 0.05 * np.sin(t)])
    rpy = np.array([0.03, -0.02 + 0.001 * t, 0.1])
    lin = np.array([0.1, -0.05, 0.2])
    ang = np.array([0.01, 0.02, -0.015])
    return pos, rpy, lin, ang


def side_terms(h, phase):
    """every quantity of section 5 at TIMES1, with the options both sides use"""
    h.set_morison_elements(0, EL_R, EL_CD, EL_CM)
    h.set_morison_options(regular_phase=phase, wave_stretching=False)
    h.set_surface_mesh(0, cone_mesh(), clip=True)
    h.set_nonlinear_options(regular_phase=phase, wave_stretching=False)
    P, Q = qtf_tables()
    h.set_drift_qtf(0, QTF_W, P, Q)
    h.set_drift_options(regular_phase=phase)
    h.set_sum_qtf(0, QTF_W, P, Q)
    h.set_sum_options(regular_phase=phase)
    h.set_sum_mode(1)
    out = {}
    out["eta"], out["vel"], out["acc"] = h.wave_kinematics(POINTS, TIMES1, regular_phase=phase, wave_stretching=False)
    out["morison"] = np.array([h.compute_morison(t, *state1(t)) for t in TIMES1])
    nl = [h.compute_nonlinear(t, *state1(t)[:2]) for t in TIMES1]
    out["buoy"], out["fk"] = np.array([v[0] for v in nl]), np.array([v[1] for v in nl])
    for mode in (1, 2, 3):
        h.set_drift_mode(mode)
        out[f"drift{mode}"] = np.array([h.compute_drift(t, state1(t)[0]) for t in TIMES1])
    out["sum"] = np.array([h.compute_sum_qtf(t, state1(t)[0]) for t in TIMES1])
    return out


def test_side_terms_wake_up_under_a_record(hydro):
    t, eta = er.on_grid_record(N1, 0.0, H, [(M1, A1, PHI1)])
    h = with_record(hydro, t, eta)
    asleep = side_terms(h, 0.0)
    for name in ("eta", "vel", "acc", "fk", "drift1", "drift2", "drift3", "sum"):  # (Morison: drag in still water, buoy: buoyancy)
        assert not asleep[name].any(), name
    h.set_eta_record_components(0.0, 1e9, 1)  # the one cosine
    c = h.eta_record_components()
    assert list(c["m"]) == [M1] and abs(c["A"][0] - A1) <= 1e-12 * A1 and abs(wrap(c["phase"][0] - PHI1)) <= 1e-11
    got = side_terms(h, 0.0)
    reg = sphere(hydro)
    reg.add_waves_regular(float(c["A"][0]), float(2 * np.pi * c["f"][0]))
    assert same_bits(reg.regular_coeffs()[2], c["k"][0])
    ref = side_terms(reg, float(c["phase"][0]))
    for name in ref:
        scale = np.abs(ref[name]).max()
        err = np.abs(got[name] - ref[name]).max()
        print(f"{name}: max |record - regular| = {err:.3e} = {err / scale if scale else 0.0:.3e} of max {scale:.3e}")
        assert scale > 0.0 and np.abs(got[name]).max() > 0.0, name
        assert err <= 1e-11 * scale, name
    # and against the cosines the record was built from
    regt = sphere(hydro)
    regt.add_waves_regular(A1, 2 * np.pi * M1 / (N1 * er.mean_spacing(t)))
    e0 = regt.wave_kinematics(POINTS, TIMES1, regular_phase=PHI1, wave_stretching=False)[0]
    assert np.abs(got["eta"] - e0).max() <= 1e-11 * np.abs(e0).max()
    for x in (h, reg, regt):
        x.close()


def test_second_order_terms_wake_up_under_a_record(hydro):
    t, eta = er.on_grid_record(N1, 0.0, H, [(M1, A1, PHI1), (23, 0.25, -0.6)])
    h = with_record(hydro, t, eta)
    pts, tt = POINTS[:4], [TIMES1[1]]
    assert not any(v.any() for v in h.wave_kinematics2(pts, tt))
    h.set_eta_record_components(0.0, 1e9, 2)
    assert list(h.eta_record_components()["m"]) == [M1, 23]
    e2, v2, a2 = h.wave_kinematics2(pts, tt)
    assert e2.any() and v2.any() and a2.any()
    h.set_morison_elements(0, EL_R, EL_CD, EL_CM)
    h.set_morison_options(wave_stretching=False)
    first = h.compute_morison(tt[0], *state1(tt[0]))
    h.set_morison_second_order(True)
    second = h.compute_morison(tt[0], *state1(tt[0]))
    assert first.any() and not np.array_equal(first, second)
    inc = h.morison_increments(0)
    e, v, a = h.wave_kinematics2(inc["p"], tt)
    assert inc["eta2"].any() and same_bits(inc["eta2"], e[0]) and same_bits(inc["vel2"], v[0]) and same_bits(inc["acc2"], a[0])
    h.set_surface_mesh(0, cone_mesh(), clip=True)
    h.set_nonlinear_options(wave_stretching=False)
    nl1 = h.compute_nonlinear(tt[0], *state1(tt[0])[:2])
    h.set_nonlinear_second_order(True)
    nl2 = h.compute_nonlinear(tt[0], *state1(tt[0])[:2])
    assert nl1[1].any() and not np.array_equal(nl1[1], nl2[1])
    # the directional sum takes the record's components under a uniform heading
    h.set_wave_directions(np.full(2, 0.3))
    ed = h.wave_kinematics2(pts, tt, directional=True)[0]
    assert ed.any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: state
# ------------------------------------------------------------------------------------------------
def motion_for(case, seed):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    return PrescribedMotion(case["N"], [b["cg"] for b in case["bodies"]], seed=seed)


def drive(h, times, motion):
    """totals and wave components of every step (the drive() of tests/test_gpu_eta_record.py, restated)"""
    tot, wav = [], []
    for t in times:
        tot.append(h.step(t, *motion.state(t)))
        wav.append(h.components()[2])
    return np.array(tot), np.array(wav)


def test_state_and_the_untouched_excitation(hydro):
    from hydrochrono_amd import capi
    comps, t, eta = recovery_record(257, 3.7)
    times = t[40:100]
    fresh = with_record(hydro, t, eta)
    fresh.set_morison_elements(0, EL_R, EL_CD, EL_CM)
    mor_fresh = np.array([fresh.compute_morison(q, *state1(q)) for q in times[:3]])
    fresh.set_morison_elements(0, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    exc_fresh = drive(fresh, times, motion_for(sphere_case(), 5))
    assert np.abs(exc_fresh[1]).max() > 0.0

    h = with_record(hydro, t, eta)
    assert h.eta_record_components()["m"].size == 0 and h.sizes()["nf"] == 0
    assert not any(v.any() for v in h.wave_kinematics(POINTS, times[:3]))
    h.set_eta_record_components(0.0, 1e9, 3)
    c = h.eta_record_components()
    # the three largest of the five cosines, in ascending frequency
    want = sorted(m for m, _, _ in sorted(comps, key=lambda v: -v[1])[:3])
    assert list(c["m"]) == want and np.all(np.diff(c["f"]) > 0) and h.sizes()["nf"] == 3
    assert h.wave_kinematics(POINTS, times[:3])[0].any()
    exc_on = drive(h, times, motion_for(sphere_case(), 5))  # the excitation path does not see the components
    assert same_bits(exc_on[0], exc_fresh[0]) and same_bits(exc_on[1], exc_fresh[1])
    # a uniform heading is accepted and rotates the kinematics as for a synthesised sea; a spread one is refused
    th = 0.7
    e0, v0, _ = h.wave_kinematics(POINTS, times[:2], wave_stretching=False)
    with pytest.raises(hydro.HydroError) as err:
        h.set_wave_directions([0.1, 0.2, 0.3])
    assert err.value.status == capi.HC_ERR_UNSUPPORTED
    with pytest.raises(hydro.HydroError) as err:
        h.set_wave_directions([th, th])
    assert err.value.status == capi.HC_ERR_INVALID
    h.set_wave_directions(np.full(3, th))
    rot = POINTS.copy()
    rot[:, 0], rot[:, 1] = POINTS[:, 0] * np.cos(th) - POINTS[:, 1] * np.sin(th), POINTS[:, 0] * np.sin(th) + POINTS[:, 1] * np.cos(th)
    e1, v1, _ = h.wave_kinematics(rot, times[:2], wave_stretching=False)  # the sea and the points turned together
    assert np.abs(e1 - e0).max() <= 1e-12 * np.abs(e0).max()
    assert np.abs(v1[..., 0] - v0[..., 0] * np.cos(th)).max() <= 1e-12 * np.abs(v0).max()
    assert np.abs(v1[..., 1] - v0[..., 0] * np.sin(th)).max() <= 1e-12 * np.abs(v0).max() and v1[..., 1].any()
    assert np.abs(v1[..., 2] - v0[..., 2]).max() <= 1e-12 * np.abs(v0).max()
    h.set_eta_record_components(0.0, 1e9, 3)  # counts as a wave-model change: the directions are dropped
    assert h.wave_directions().size == 0
    # clear: kinematics are zeros again, the Morison bits are those of a fresh record context
    h.clear_eta_record_components()
    assert h.eta_record_components()["m"].size == 0 and h.sizes()["nf"] == 0 and all(v.size == 0 for v in h.irreg_spectrum().values())
    assert not any(v.any() for v in h.wave_kinematics(POINTS, times[:3]))
    h.set_morison_elements(0, EL_R, EL_CD, EL_CM)
    assert same_bits(np.array([h.compute_morison(q, *state1(q)) for q in times[:3]]), mor_fresh)
    h.set_morison_elements(0, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    h.reset_history()
    exc_off = drive(h, times, motion_for(sphere_case(), 5))
    assert same_bits(exc_off[0], exc_fresh[0]) and same_bits(exc_off[1], exc_fresh[1])
    # an empty band, and a model that is no record
    T_w = 257 * er.mean_spacing(t)
    for band in ((0.2 / T_w, 0.8 / T_w), (1e3, 2e3), (0.5, 0.4), (float("nan"), 1.0)):
        with pytest.raises(hydro.HydroError) as err:
            h.set_eta_record_components(*band)
        assert err.value.status == capi.HC_ERR_INVALID
    assert h.eta_record_components()["m"].size == 0
    h.set_eta_record_components(0.0, 1e9)
    h.add_waves_regular(0.3, 1.1)  # any hc_set_wave_* call drops the components
    for call in (lambda: h.set_eta_record_components(0.0, 1e9), h.clear_eta_record_components, h.eta_record_components):
        with pytest.raises(hydro.HydroError) as err:
            call()
        assert err.value.status == capi.HC_ERR_INVALID
    h.add_waves_irregular_eta(t, eta, H)
    assert h.eta_record_components()["m"].size == 0 and not h.wave_kinematics(POINTS, times[:1])[0].any()
    none = sphere(hydro)
    with pytest.raises(hydro.HydroError) as err:
        none.set_eta_record_components(0.0, 1e9)
    assert err.value.status == capi.HC_ERR_INVALID
    with pytest.raises(hydro.HydroError):
        with_record(hydro, t[:3], eta[:3]).set_eta_record_components(0.0, 1e9)  # n >= 4
    for x in (h, fresh, none):
        x.close()


# ------------------------------------------------------------------------------------------------
# 7: the C++ mirror gives the bits of the Python path
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches_the_python_path(hydro, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    exe = str(tmp_path / "eta_components_caller")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "chrono_stub"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "eta_components_caller.cpp"), "-o", exe,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    p, tq = (3.0, 0.5, -1.5), 33.3
    r = subprocess.run([exe, h5, FIXTURE, "0.03", "0.4", "20", *map(repr, p), repr(tq)], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    assert out["before"] == "Spectrum has not been created. Initialize with wave height and period to create spectrum."
    h = hydro.HydroForces(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular_eta(*hydro.read_eta_file(FIXTURE), SPHERE_DT)
    h.set_eta_record_components(0.03, 0.4, 20)
    c, sp = h.eta_record_components(), h.irreg_spectrum()
    assert out["count"] == "20" and c["m"].size == 20
    fr = out["frequencies"].split()
    assert fr[0] == "20" and [float(v) for v in fr[1:]] == [c["f"][0], c["f"][-1]]
    total = 0.0
    for v in sp["S"]:
        total += float(v)
    assert float(out["spectrum"]) == total and total > 0.0
    assert [float(v) for v in out["stats"].split()] == [c["mean"], c["variance_share"], c["rms_residual"]]
    e, v, _ = h.wave_kinematics([p], [tq])  # the mirror's defaults: mwl 0, Wheeler stretching on
    assert [float(x) for x in out["velocity"].split()] == list(v[0, 0]) and v.any()
    assert float(out["elevation"]) == e[0, 0] and e.any()
    assert out["cleared"].split() == ["0", "0"]
    assert math.isfinite(total)
    h.close()
