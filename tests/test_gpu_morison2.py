"""Morison elements on the second-order sea on the GPU (hc_set_morison_second_order, hc_get_morison_increments; csrc/hc_morison.hip:
morison2_incr_kernel and the order-2 morison_items_kernel) against the tests' NumPy restatement (tests/morison2_ref.py), fed the
context's own spectrum / regular-wave coefficients, on the input sets of tests/morison2_inputs.py.

Tolerance: the bound morison2_ref returns per body and component -- 1e-11 sum|term| for every first-order kinematic quantity plus
1e-11 sum|term| of its second-order increment, propagated to first order through the force expression, plus (n_e + 64) 2^-52
sum_e |contribution_e| for the fixed-order sum and the rotations (the derivation is in morison2_ref's docstring).  The wet test is a
discontinuity: every comparison first asserts, on the reference side, that no element is closer than 1e-6 m to eta1 + eta2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import morison2_inputs as mi
import wave2_inputs as wi
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
THREE8 = wi.three_waves(8)
CUT = dict(diff_band=(0.05, 3.0), sum_band=(1.5, 6.0))


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def set_all(h, elements):
    for b, el in enumerate(elements):
        if el is not None:
            h.set_morison_elements(b, *el)


def raw_step(h, t, state):
    """hc_step itself (HydroForces.step composes the Morison term once elements are set)"""
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def three_with_elements(HF, case=None, seeds=(20, 21, 22), counts=(33, 257, 5)):
    h = HF.from_case(case or three_body_case())
    h.add_waves_irregular(**THREE8)
    for b, (n, s) in enumerate(zip(counts, seeds)):
        h.set_morison_elements(b, *mi.random_elements(n, s))
    h.set_morison_options(mwl=0.1)
    return h


# ------------------------------------------------------------------------------------------------
# 1: parity inside the derived bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mi.SETS))
def test_parity_inside_the_derived_bound(HF, name):
    s = mi.SETS[name]
    case = s["case"]()
    h = HF.from_case(case)
    h.add_waves_irregular(**s["waves"])
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == s["waves"]["nfrequencies"]
    _, g, depth = h.simulation_parameters()
    assert depth == case["water_depth"]
    set_all(h, s["elements"]())
    h.set_morison_second_order(True, diff_band=s["diff_band"], sum_band=s["sum_band"])
    results = {}
    for mwl, stretching in s["options"]:
        h.set_morison_options(mwl=mwl, wave_stretching=stretching)
        for t in s["times"]:
            what = f"{name} mwl={mwl} stretching={stretching} t={t}"
            ref, state = mi.reference(name, comp, abs(g), t, mwl, stretching)
            assert ref["margin"] >= mi.MIN_GAP, f"{what}: an element is {ref['margin']:.3e} m from the free surface (choose other inputs)"
            got = h.compute_morison(t, *state).reshape(-1, 6)
            assert got.shape == ref["F"].shape and np.all(np.isfinite(got)), what
            err = np.abs(got - ref["F"])
            worst = float(np.max(err / np.maximum(ref["bound"], 1e-300)))
            print(f"{what}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(ref['F'])):.3e}")
            assert np.all(err <= ref["bound"]), f"{what}: worst {worst:.3e} of the bound"
            for b, p in enumerate(ref["p"]):  # the points the elements were evaluated at: a few ulp of |pos| + |r| <= 64 m
                if p.size:
                    assert np.allclose(h.morison_increments(b)["p"], p, rtol=0, atol=16 * 64 * 2.0 ** -52)
            results[(mwl, stretching, t)] = got
    if len(s["options"]) > 1:
        t = s["times"][-1]
        (m0, s0), (m1, s1), (m2_, s2) = s["options"]
        assert not np.array_equal(results[(m0, s0, t)], results[(m1, s1, t)]) and not np.array_equal(results[(m0, s0, t)], results[(m2_, s2, t)])
    h.close()


# ------------------------------------------------------------------------------------------------
# 2: a regular wave: first order plus Stokes' second-order velocity and acceleration
# ------------------------------------------------------------------------------------------------
def test_regular_wave_is_first_order_plus_stokes(HF):
    depth, A, w, phi, mwl, t = 30.0, 0.5, 0.8, 0.7, 0.25, 3.7
    case = mi.shallow_case()
    h = HF.from_case(case)
    h.add_waves_regular(A, w)
    k = h.regular_coeffs()[2]
    rho, g, _ = h.simulation_parameters()
    g = abs(g)
    r, cd, cm = np.array([[0.0, 0.0, -6.0]]), np.array([[1.5, 0.7, 2.0]]), np.array([[2.0, 1.0, 0.5]])
    h.set_morison_elements(0, r, cd, cm)
    h.set_morison_options(mwl=mwl, regular_phase=phi)
    pos = np.array([12.0, 1.0, -1.0])
    z3 = np.zeros(3)
    first = h.compute_morison(t, pos, z3, z3, z3)
    h.set_morison_second_order(True)
    got = h.compute_morison(t, pos, z3, z3, z3)
    theta = k * pos[0] - w * t + phi
    z = pos[2] + r[0, 2] - mwl  # well below the trough: z2 = z - mwl
    assert z < -5.0 and z > -depth
    # first order: the profile hc_wave_kinematics takes (exponential where the wave is longer than the depth)
    deep = 2 * np.pi / k > depth or k * depth > 500
    px, pz = (np.exp(k * z),) * 2 if deep else (np.cosh(k * (z + depth)) / np.sinh(k * depth), np.sinh(k * (z + depth)) / np.sinh(k * depth))
    u1 = np.array([w * A * px * np.cos(theta), 0.0, w * A * pz * np.sin(theta)])
    a1 = np.array([w * w * A * px * np.sin(theta), 0.0, -w * w * A * pz * np.cos(theta)])
    # Stokes' second-order potential B cosh(2 k (z + h)) / cosh(2 k h) sin 2 theta.  Its amplitude with R = w^2 / g kept apart from
    # k tanh k h (the reference's k is on the dispersion curve to 1e-6 only, and the library takes R from w):
    # B = (A g / w)^2 / (8 w) * 6 R (k^2 - R^2) / (2 R - k tanh 2 k h); on the curve that is the textbook 3/8 A^2 w / sinh^4 k h
    R = w * w / g
    B = (A * g / w) ** 2 / (8 * w) * 6 * R * (k - R) * (k + R) / (2 * R - k * np.tanh(2 * k * depth))
    textbook = 0.375 * A * A * w * np.cosh(2 * k * depth) / np.sinh(k * depth) ** 4
    assert abs(B - textbook) <= 1e-3 * abs(textbook)
    C2, S2 = np.cosh(2 * k * (z + depth)) / np.cosh(2 * k * depth), np.sinh(2 * k * (z + depth)) / np.cosh(2 * k * depth)
    u2 = np.array([2 * k * B * C2 * np.cos(2 * theta), 0.0, 2 * k * B * S2 * np.sin(2 * theta)])
    a2 = np.array([4 * k * w * B * C2 * np.sin(2 * theta), 0.0, -4 * k * w * B * S2 * np.cos(2 * theta)])
    u, a = u1 + u2, a1 + a2  # a regular wave is not ramped; the body is at rest and upright
    F = 0.5 * rho * cd[0] * np.abs(u) * u + rho * cm[0] * a
    want = np.concatenate([F, np.cross(r[0], F)])
    print("regular: |u2| / |u1| =", np.abs(u2).max() / np.abs(u1).max(), "worst relative", np.max(np.abs(got - want) / np.abs(want).max()))
    assert np.allclose(got, want, rtol=1e-12, atol=0)  # (F_y, M_x and M_z are exact zeros on both sides)
    assert np.abs(u2).max() > 1e-6 * np.abs(u1).max() and not np.allclose(first, want, rtol=1e-9, atol=0)
    inc = h.morison_increments(0)
    assert np.allclose(inc["vel2"][0], u2, rtol=1e-10, atol=0) and np.allclose(inc["acc2"][0], a2, rtol=1e-10, atol=0)
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: the increments are hc_wave_kinematics2's, bit for bit
# ------------------------------------------------------------------------------------------------
def test_increments_are_those_of_wave_kinematics2_bit_for_bit(HF):
    s = mi.SETS["column_30m"]
    h = HF.from_case(s["case"]())
    h.add_waves_irregular(**s["waves"])
    set_all(h, s["elements"]())
    for (mwl, kw) in ((0.3, {}), (0.0, CUT), (0.3, dict(diff_band=(0.0, 0.5), sum_band=wi.NO_PAIR, apply_ramp=False))):
        h.set_morison_options(mwl=mwl)
        h.set_morison_second_order(True, **kw)
        for t in (-1.0, 7.3, 41.7):  # before, inside and after the ramp of 20 s
            h.compute_morison(t, *mi.moving_state(1, -2.0, t))
            inc = h.morison_increments(0)
            e, v, a = h.wave_kinematics2(inc["p"], [t], mwl=mwl, **kw)
            assert same_bits(inc["eta2"], e[0]) and same_bits(inc["vel2"], v[0]) and same_bits(inc["acc2"], a[0]), (mwl, kw, t)
            assert bool(inc["eta2"].any()) == (t > 0.0 or kw.get("apply_ramp") is False)
    # a regular wave carries the regular phase of the Morison options
    h.add_waves_regular(0.5, 0.8)
    h.set_morison_options(mwl=0.2, regular_phase=0.9)
    h.set_morison_second_order(True)
    h.compute_morison(5.0, *mi.moving_state(1, -2.0, 5.0))
    inc = h.morison_increments(0)
    e, v, a = h.wave_kinematics2(inc["p"], [5.0], mwl=0.2, regular_phase=0.9)
    assert same_bits(inc["eta2"], e[0]) and same_bits(inc["vel2"], v[0]) and same_bits(inc["acc2"], a[0]) and inc["vel2"].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 4: the bits depend on the body alone
# ------------------------------------------------------------------------------------------------
def test_shards_other_bodies_and_repeats_leave_the_bits(HF):
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    whole = three_with_elements(HF)
    group = HydroGroup.from_case(case, 3)
    group.add_waves_irregular(**THREE8)
    elements = [mi.random_elements(n, s) for n, s in zip((33, 257, 5), (20, 21, 22))]
    for b, el in enumerate(elements):
        group.set_morison_elements(b, *el)
    group.set_morison_options(mwl=0.1)
    for h in (whole, group):
        h.set_morison_second_order(True, **CUT)
    assert group.morison_second_order() == whole.morison_second_order() == dict(on=True, apply_ramp=True, **CUT)
    st = mi.moving_state(3, -3.0, 12.5)
    ref = whole.compute_morison(12.5, *st)
    assert ref.reshape(3, 6).any(axis=1).all()
    assert same_bits(group.compute_morison(12.5, *st), ref)
    for b in range(3):
        a, c = whole.morison_increments(b), group.morison_increments(b)
        assert all(same_bits(a[k], c[k]) for k in a) and a["eta2"].shape == (elements[b][0].shape[0],)
    for _ in range(3):
        assert same_bits(whole.compute_morison(12.5, *st), ref)
    # another body's list replaced, then cleared: bodies 0 and 2 keep their bits
    whole.set_morison_elements(1, *mi.random_elements(600, 23))
    a = whole.compute_morison(12.5, *st)
    assert same_bits(a[:6], ref[:6]) and same_bits(a[12:], ref[12:]) and not same_bits(a[6:12], ref[6:12])
    whole.set_morison_elements(1, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    a = whole.compute_morison(12.5, *st)
    assert same_bits(a[:6], ref[:6]) and same_bits(a[12:], ref[12:]) and not a[6:12].any()
    whole.set_morison_elements(1, *elements[1])
    assert same_bits(whole.compute_morison(12.5, *st), ref)
    whole.close()
    group.close()


def test_number_of_bodies_leaves_the_bits(HF):
    """The same body data (state, elements, wave model, rho, depth) as the only body of a 1-body context and as body 2 of a 3-body one."""
    from hydrochrono_amd.synthetic import many_body_case
    waves = dict(simulation_dt=0.05, simulation_duration=200.0, ramp_duration=20.0, wave_height=4.0, wave_period=9.0,
                 frequency_min=0.02, frequency_max=0.6, nfrequencies=24, peak_enhancement_factor=2.0, seed=4)
    one, three = (HF.from_case(many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)) for N in (1, 3))
    el = mi.random_elements(130, 30)
    one.set_morison_elements(0, *el)
    three.set_morison_elements(2, *el)
    three.set_morison_elements(0, *mi.random_elements(70, 31))
    for h in (one, three):
        h.add_waves_irregular(**waves)
        h.set_morison_options(mwl=0.2)
        h.set_morison_second_order(True)
    st1 = mi.moving_state(1, -1.0, 33.0, seed=5)
    st3 = [np.concatenate([x, x, x]) for x in st1]
    for x in st3:
        x[:2] += 0.37  # the other bodies move differently
    a, b = one.compute_morison(33.0, *st1), three.compute_morison(33.0, *st3)
    assert a.any() and same_bits(a, b[12:])
    i1, i3 = one.morison_increments(0), three.morison_increments(2)
    assert all(same_bits(i1[k], i3[k]) for k in i1)
    one.close()
    three.close()


# ------------------------------------------------------------------------------------------------
# 5: order 1 untouched, order 2 live
# ------------------------------------------------------------------------------------------------
def test_order_one_keeps_its_bits_and_order_two_differs(HF):
    h = three_with_elements(HF)
    st = mi.moving_state(3, -3.0, 12.5)
    before = h.compute_morison(12.5, *st)
    assert h.morison_second_order() == dict(on=False, diff_band=(0.0, INF), sum_band=(0.0, INF), apply_ramp=True)
    h.set_morison_second_order(True)
    second = h.compute_morison(12.5, *st)
    h.set_morison_second_order(False)
    after = h.compute_morison(12.5, *st)
    h.set_morison_second_order(True, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
    empty = h.compute_morison(12.5, *st)
    assert np.array_equal(before, after) and np.array_equal(before, empty) and before.reshape(3, 6).any(axis=1).all()
    assert not np.array_equal(second, before)
    assert np.all(np.abs(second - before).reshape(3, 6).max(axis=1) > 1e-6 * np.abs(before).reshape(3, 6).max(axis=1))
    # the models without components: equal to order 1 as well
    h.set_morison_second_order(True)
    rec_t = 0.05 * np.arange(400)
    for model in ("nowave", "eta_record"):
        if model == "nowave":
            h.add_waves_none()
        else:
            h.add_waves_irregular_eta(rec_t, 0.5 * np.sin(0.8 * rec_t), 0.05)
        h.set_morison_second_order(True)
        on = h.compute_morison(3.0, *st)
        h.set_morison_second_order(False)
        assert np.array_equal(on, h.compute_morison(3.0, *st)) and on.any(), model
    fresh = HF.from_case(three_body_case())  # no wave model at all
    fresh.set_morison_elements(0, *mi.random_elements(9, 1))
    off = fresh.compute_morison(3.0, *st)
    fresh.set_morison_second_order(True)
    assert np.array_equal(off, fresh.compute_morison(3.0, *st)) and off.any()
    fresh.close()
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: beside the steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 32])
def test_second_order_morison_around_every_step_changes_no_force(HF, lookahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_morison in (False, True):
        h = HF.from_case(case)
        h.set_lookahead(lookahead)
        h.add_waves_irregular(**wi.sphere_waves(65))
        if with_morison:
            h.set_morison_elements(0, *mi.random_elements(64, 2))
            h.set_morison_second_order(True)
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        rows = []
        for n in range(100):  # three look-ahead blocks of 32 steps
            t = SPHERE_DT * n
            st = motion.state(t)
            if with_morison:
                h.morison_begin(t, *st)
            total = raw_step(h, t, st)
            if with_morison:
                assert h.morison_end().any()
            rows.append(np.concatenate([total, *h.components()]))
        if with_morison:
            assert h.morison_increments(0)["eta2"].any()
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# 7: the layers above
# ------------------------------------------------------------------------------------------------
def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    elements = [mi.random_elements(33, 20), None, mi.random_elements(5, 22)]
    a, b, first = HF.from_case(case), HF.from_case(case), HF.from_case(case)
    grp, gplain = HydroGroup.from_case(case, 3), HydroGroup.from_case(case, 3)
    for h in (a, b, first, grp, gplain):
        h.add_waves_irregular(**THREE8)
    for h in (a, b, first, grp):
        set_all(h, elements)
        h.set_morison_options(mwl=0.1)
    for h in (a, b, grp):
        h.set_morison_second_order(True, **CUT)
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)
    for n in range(20):
        t = 0.01 * n + 25.0
        st = motion.state(t)
        fa = a.step(t, *st)
        total, mor = raw_step(b, t, st), b.compute_morison(t, *st)
        assert same_bits(fa, total + mor) and same_bits(a.morison(), mor)
        assert same_bits(grp.step(t, *st), gplain.step(t, *st) + mor) and same_bits(grp.morison(), mor)
        assert same_bits(grp.compute_morison(t, *st), mor)
    assert mor.any() and not np.array_equal(first.compute_morison(t, *st), mor)
    with pytest.raises(Exception):
        grp.morison_increments(1 + 3)
    assert grp.morison_increments(0)["eta2"].size == 33 and grp.morison_increments(2)["eta2"].size == 5
    for h in (a, b, first):
        h.close()
    grp.close()
    gplain.close()


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "morison2_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison2_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (40, 28)
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(**dict(wi.sphere_waves(65), simulation_dt=0.015))
    h.set_morison_elements(0, [[0, 0, -6.0], [2.5, 0.5, -3.0], [0, 0, 9.0]], [[3, 3, 12.0], [1, 1.5, 0.5], [5, 5, 5.0]], [[0, 0, 0], [2, 2, 1.0], [0, 0, 0]])
    h.set_morison_options(mwl=0.25)
    h.set_morison_second_order(True, **dict(CUT, diff_band=(0.05, 0.9)))
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total, mor = raw_step(h, t, st), h.compute_morison(t, *st)
        assert same_bits(row[19:25], mor) and same_bits(row[13:19], total + mor), t
        assert same_bits(row[25:28], h.morison_increments(0)["eta2"]), t
    assert np.abs(rows[:, 19:22]).max() > 1.0 and np.abs(rows[:, 25:28]).max() > 1e-5
    h.close()


# ------------------------------------------------------------------------------------------------
# 8: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    from hydrochrono_amd import capi
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    h = three_with_elements(HF, counts=(4, 3, 0))
    lib = h.lib
    z9, lin, out = np.zeros(9), np.tile([0.5, 0.0, 0.0], 3), np.empty(18)
    pos = np.tile([0.0, 0.0, -3.0], 3)

    def plain_evaluation_works():
        assert lib.hc_morison_end(h.ctx, dp(out)) == INV  # nothing is pending
        assert lib.hc_compute_morison(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(out)) == OK and out[:12].any() and not out[12:].any()

    def set2(on=1, dlo=0.0, dhi=INF, slo=0.0, shi=INF, ramp=1):
        return lib.hc_set_morison_second_order(h.ctx, on, dlo, dhi, slo, shi, ramp)

    eta = np.empty(8)
    # off: no increments to ask for
    assert lib.hc_get_morison_increments(h.ctx, 0, None, dp(eta), None, None) == INV
    plain_evaluation_works()
    # cut-offs: negative, NaN, lo > hi -- and the setting before stays
    assert set2(dlo=0.1, dhi=0.9) == OK
    for bad in (dict(dlo=-0.1), dict(dhi=np.nan), dict(slo=np.nan), dict(shi=-1.0), dict(dlo=0.5, dhi=0.4), dict(slo=2.0, shi=1.0),
                dict(on=0, dlo=-1.0)):
        assert set2(**bad) == INV and (b"cut-off" in lib.hc_last_error(h.ctx)), bad
        assert h.morison_second_order() == dict(on=True, diff_band=(0.1, 0.9), sum_band=(0.0, INF), apply_ramp=True)
        plain_evaluation_works()
    # off and on again: the evaluations before are forgotten, and there is none since
    assert set2(on=0) == OK and set2() == OK
    assert lib.hc_get_morison_increments(h.ctx, 0, None, dp(eta), None, None) == INV
    plain_evaluation_works()
    assert lib.hc_get_morison_increments(h.ctx, 0, None, dp(eta), None, None) == OK
    assert lib.hc_get_morison_increments(h.ctx, 0, None, None, None, None) == OK  # any pointer may be NULL
    for body in (-1, 3, 100):
        assert lib.hc_get_morison_increments(h.ctx, body, None, dp(eta), None, None) == INV
    # a call while a begin is pending
    assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == OK
    assert set2(on=0) == INV and set2(dhi=0.5) == INV
    assert lib.hc_morison_end(h.ctx, dp(out)) == OK
    assert h.morison_second_order()["on"] is True
    plain_evaluation_works()
    # a shard context answers for its own bodies only
    sh = HF.from_case(three_body_case(), body_range=(1, 2))
    sh.add_waves_irregular(**THREE8)
    for b in range(3):
        sh.set_morison_elements(b, *mi.random_elements(3, 40 + b))
    sh.set_morison_second_order(True)
    o6 = np.empty(6)
    assert lib.hc_compute_morison(sh.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(o6)) == OK
    assert lib.hc_get_morison_increments(sh.ctx, 1, None, dp(eta), None, None) == OK
    for body in (0, 2):
        assert lib.hc_get_morison_increments(sh.ctx, body, None, dp(eta), None, None) == INV
    sh.close()
    # more than 4096 components: refused by hc_morison_begin, nothing pending; fine again once second order is off or the sea smaller
    h.add_waves_irregular(**wi.three_waves(4097))
    assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == UNS
    assert lib.hc_compute_morison(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(out)) == UNS
    assert lib.hc_morison_end(h.ctx, dp(out)) == INV
    assert set2(on=0) == OK
    plain_evaluation_works()
    assert set2() == OK
    h.add_waves_irregular(**THREE8)
    plain_evaluation_works()
    with pytest.raises(Exception):
        h.set_morison_second_order(True, diff_band=(1.0, 0.5))
    h.close()
