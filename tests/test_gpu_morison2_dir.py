"""Morison elements on the second-order sea in a short-crested sea on the GPU (hc_set_morison_second_order_directional;
csrc/hc_morison.hip: morison2_incr_kernel<true> and morison2_dir_items_kernel) against the tests' NumPy restatement
(tests/morison2_dir_ref.py), fed the context's own spectrum and directions, on the input sets of tests/morison2_dir_inputs.py.

Tolerance: the bound morison2_dir_ref returns per body and component -- that of tests/test_gpu_morison2.py with the directional
scales: 1e-11 times the first-order scale of every kinematic quantity (tests/directional_ref.py) plus 1e-11 sum|term| of its
second-order increment (tests/wave2_dir_ref.py), propagated to first order through the force expression, plus
(n_e + 64) 2^-52 sum_e |contribution_e| for the fixed-order sum and the rotations.  The wet test is a discontinuity: every comparison
first asserts, on the reference side, that no element is closer than 1e-6 m to eta1 + eta2."""
import os
import subprocess

import numpy as np
import pytest

import morison2_dir_inputs as mdi
import morison2_dir_ref as md
import morison2_inputs as mi
import morison2_ref as m2
import morison_ref as mr
import wave2_inputs as wi
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
CUT = dict(diff_band=(0.05, 3.0), sum_band=(1.5, 6.0))
THREE8 = wi.three_waves(8)


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


def context_of(make, name, second_order=True):
    """A context (HydroForces.from_case or a HydroGroup maker) on the spread sea of a set, its directions and elements in force."""
    s = mdi.SETS[name]
    case = s["case"]()
    h = make(case)
    mdi.spread_sea(h, case, s["waves"])
    h.set_wave_directions(mdi.directions(name))
    set_all(h, s["elements"]())
    if second_order:
        h.set_morison_second_order(True, diff_band=s["diff_band"], sum_band=s["sum_band"])
        h.set_morison_second_order_directional(True)
    return h, case


def three_spread(make, counts=(33, 257, 5), seeds=(20, 21, 22), **second):
    """Three bodies on the 8-component spread sea, second order and its directional form on."""
    case = three_body_case()
    h = make(case)
    mdi.spread_sea(h, case, THREE8)
    h.set_wave_directions(mdi.di.spread(8))
    for b, (n, s) in enumerate(zip(counts, seeds)):
        if n:
            h.set_morison_elements(b, *mi.random_elements(n, s))
    h.set_morison_options(mwl=0.1)
    h.set_morison_second_order(True, **second)
    h.set_morison_second_order_directional(True)
    return h


# ------------------------------------------------------------------------------------------------
# 1: parity inside the derived bound
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mdi.SETS))
def test_parity_inside_the_derived_bound(HF, name):
    s = mdi.SETS[name]
    h, case = context_of(HF.from_case, name)
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == s["waves"]["nfrequencies"] and np.array_equal(h.wave_directions(), mdi.directions(name))
    _, g, depth = h.simulation_parameters()
    assert depth == case["water_depth"]
    for mwl, stretching in s["options"]:
        h.set_morison_options(mwl=mwl, wave_stretching=stretching)
        for t in s["times"]:
            what = f"{name} mwl={mwl} stretching={stretching} t={t}"
            ref, state = mdi.reference(name, comp, abs(g), t, mwl, stretching)
            assert ref["margin"] >= mdi.MIN_GAP, f"{what}: an element is {ref['margin']:.3e} m from the free surface (choose other inputs)"
            got = h.compute_morison(t, *state).reshape(-1, 6)
            assert got.shape == ref["F"].shape and np.all(np.isfinite(got)), what
            err = np.abs(got - ref["F"])
            worst = float(np.max(err / np.maximum(ref["bound"], 1e-300)))
            print(f"{what}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(ref['F'])):.3e}")
            assert np.all(err <= ref["bound"]), f"{what}: worst {worst:.3e} of the bound"
            for b, p in enumerate(ref["p"]):  # the points the elements were evaluated at: a few ulp of |pos| + |r| <= 64 m
                if p.size:
                    inc = h.morison_increments(b)
                    assert np.allclose(inc["p"], p, rtol=0, atol=16 * 64 * 2.0 ** -52)
                    assert inc["vel2"].shape == (p.shape[0], 3)
    # the increments change the result by far more than the bound
    h.set_morison_second_order(False)
    first = h.compute_morison(t, *state).reshape(-1, 6)
    has = [b for b, p in enumerate(ref["p"]) if p.size]
    assert np.all(np.abs(first - got)[has].max(axis=1) > 100 * ref["bound"][has].max(axis=1))
    h.close()


# ------------------------------------------------------------------------------------------------
# 2: the increments are hc_wave_kinematics2_dir's, bit for bit
# ------------------------------------------------------------------------------------------------
def test_increments_are_those_of_wave_kinematics2_dir_bit_for_bit(HF):
    h, _ = context_of(HF.from_case, "column_30m_spread", second_order=False)
    h.set_morison_second_order_directional(True)
    seen_y = False
    for (mwl, kw) in ((0.3, {}), (0.0, CUT), (0.3, dict(diff_band=(0.0, 0.5), sum_band=wi.NO_PAIR, apply_ramp=False))):
        h.set_morison_options(mwl=mwl)
        h.set_morison_second_order(True, **kw)
        for t in (-1.0, 7.3, 41.7):  # before, inside and after the ramp of 20 s
            h.compute_morison(t, *mi.moving_state(1, -2.0, t))
            inc = h.morison_increments(0)
            e, v, a = h.wave_kinematics2(inc["p"], [t], mwl=mwl, directional=True, **kw)
            assert same_bits(inc["eta2"], e[0]) and same_bits(inc["vel2"], v[0]) and same_bits(inc["acc2"], a[0]), (mwl, kw, t)
            assert bool(inc["eta2"].any()) == (t > 0.0 or kw.get("apply_ramp") is False)
            seen_y = seen_y or (inc["vel2"][:, 1].any() and inc["acc2"][:, 1].any())
    assert seen_y  # u2y and a2y are carried
    # a regular wave with a heading carries the regular phase of the Morison options
    h.add_waves_regular(0.5, 0.8)
    h.set_wave_directions([0.7])
    h.set_morison_options(mwl=0.2, regular_phase=0.9)
    h.set_morison_second_order(True)
    h.compute_morison(5.0, *mi.moving_state(1, -2.0, 5.0))
    inc = h.morison_increments(0)
    e, v, a = h.wave_kinematics2(inc["p"], [5.0], mwl=0.2, regular_phase=0.9, directional=True)
    assert same_bits(inc["eta2"], e[0]) and same_bits(inc["vel2"], v[0]) and same_bits(inc["acc2"], a[0])
    assert inc["vel2"][:, 0].any() and inc["vel2"][:, 1].any()
    # the long-crested evaluation after it: the y components are zero again
    h.set_wave_directions(None)
    h.compute_morison(5.0, *mi.moving_state(1, -2.0, 5.0))
    inc = h.morison_increments(0)
    e, v, a = h.wave_kinematics2(inc["p"], [5.0], mwl=0.2, regular_phase=0.9)
    assert same_bits(inc["eta2"], e[0]) and same_bits(inc["vel2"], v[0]) and same_bits(inc["acc2"], a[0])
    assert inc["vel2"][:, 0].any() and not inc["vel2"][:, 1].any() and not inc["acc2"][:, 1].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: a regular wave with a heading: first order plus Stokes' second-order velocity and acceleration along the heading
# ------------------------------------------------------------------------------------------------
def test_regular_wave_with_a_heading_is_first_order_plus_stokes(HF):
    depth, A, w, phi, mwl, t, beta = 30.0, 0.5, 0.8, 0.7, 0.25, 3.7, 0.7
    case = mi.shallow_case()
    h = HF.from_case(case)
    h.add_waves_regular(A, w)
    h.set_wave_directions([beta])
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
    h.set_morison_second_order_directional(True)
    got = h.compute_morison(t, pos, z3, z3, z3)
    cb, sb = np.cos(beta), np.sin(beta)
    e = np.array([cb, sb, 0.0])  # the horizontal vectors lie along the heading
    theta = k * (pos[0] * cb + pos[1] * sb) - w * t + phi
    z = pos[2] + r[0, 2] - mwl  # well below the trough: z2 = z - mwl
    assert z < -5.0 and z > -depth
    deep = 2 * np.pi / k > depth or k * depth > 500
    px, pz = (np.exp(k * z),) * 2 if deep else (np.cosh(k * (z + depth)) / np.sinh(k * depth), np.sinh(k * (z + depth)) / np.sinh(k * depth))
    u1 = w * A * px * np.cos(theta) * e + np.array([0.0, 0.0, w * A * pz * np.sin(theta)])
    a1 = w * w * A * px * np.sin(theta) * e + np.array([0.0, 0.0, -w * w * A * pz * np.cos(theta)])
    # Stokes' second-order potential B cosh(2 k (z + h)) / cosh(2 k h) sin 2 theta, its amplitude with R = w^2 / g kept apart from
    # k tanh k h as in tests/test_gpu_morison2.py
    R = w * w / g
    B = (A * g / w) ** 2 / (8 * w) * 6 * R * (k - R) * (k + R) / (2 * R - k * np.tanh(2 * k * depth))
    textbook = 0.375 * A * A * w * np.cosh(2 * k * depth) / np.sinh(k * depth) ** 4
    assert abs(B - textbook) <= 1e-3 * abs(textbook)
    C2, S2 = np.cosh(2 * k * (z + depth)) / np.cosh(2 * k * depth), np.sinh(2 * k * (z + depth)) / np.cosh(2 * k * depth)
    u2 = 2 * k * B * C2 * np.cos(2 * theta) * e + np.array([0.0, 0.0, 2 * k * B * S2 * np.sin(2 * theta)])
    a2 = 4 * k * w * B * C2 * np.sin(2 * theta) * e + np.array([0.0, 0.0, -4 * k * w * B * S2 * np.cos(2 * theta)])
    u, a = u1 + u2, a1 + a2  # a regular wave is not ramped; the body is at rest and upright
    F = 0.5 * rho * cd[0] * np.abs(u) * u + rho * cm[0] * a
    want = np.concatenate([F, np.cross(r[0], F)])
    print("regular: |u2| / |u1| =", np.abs(u2).max() / np.abs(u1).max(), "worst relative", np.max(np.abs(got - want)[want != 0] / np.abs(want[want != 0])))
    assert np.allclose(got, want, rtol=1e-12, atol=0)  # (M_z is an exact zero on both sides)
    assert np.all(want[:5] != 0) and want[5] == 0
    assert np.abs(u2).max() > 1e-6 * np.abs(u1).max() and not np.allclose(first, want, rtol=1e-9, atol=0)
    inc = h.morison_increments(0)
    assert np.allclose(inc["vel2"][0], u2, rtol=1e-10, atol=0) and np.allclose(inc["acc2"][0], a2, rtol=1e-10, atol=0)
    h.close()


# ------------------------------------------------------------------------------------------------
# 4: every direction 0: the long-crested second-order result
# ------------------------------------------------------------------------------------------------
def test_directions_all_zero_agree_with_the_long_crested_path(HF):
    name = "column_30m_spread"
    s = mdi.SETS[name]
    h, case = context_of(HF.from_case, name)
    nf = s["waves"]["nfrequencies"]
    comp = wk.irregular_components(h.irreg_spectrum())
    _, g, depth = h.simulation_parameters()
    elements = s["elements"]()
    rd = s["waves"]["ramp_duration"]
    for t in s["times"]:
        state = mi.moving_state(1, s["rest_z"], t)
        kw = dict(mwl=0.3, stretching=True, ramp=mr.ramp_factor(t, rd), ramp_duration=rd)
        h.set_morison_options(mwl=0.3, wave_stretching=True)
        h.set_wave_directions(np.zeros(nf))
        dirs = h.compute_morison(t, *state).reshape(-1, 6)
        inc_d = h.morison_increments(0)
        h.set_wave_directions(None)
        lc = h.compute_morison(t, *state).reshape(-1, 6)
        inc_l = h.morison_increments(0)
        rd_ = md.morison2_dir(comp, np.zeros(nf), abs(g), depth, case["rho"], elements, t, *state, **kw)
        rl_ = m2.morison2(comp, abs(g), depth, case["rho"], elements, t, *state, **kw)
        assert min(rd_["margin"], rl_["margin"]) >= mdi.MIN_GAP
        err, bound = np.abs(dirs - lc), rd_["bound"] + rl_["bound"]
        print(f"directions all 0, t={t}: worst {float(np.max(err / bound)):.3e} of the two bounds")
        assert np.all(err <= bound) and np.abs(lc).max() > 1.0
        assert same_bits(inc_d["p"], inc_l["p"]) and not inc_d["vel2"][:, 1].any() and not inc_l["vel2"][:, 1].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 5: the zero cases
# ------------------------------------------------------------------------------------------------
def test_switch_without_directions_and_empty_bands_under_directions(HF):
    h = three_spread(HF.from_case)
    st = mi.moving_state(3, -3.0, 12.5)
    second = h.compute_morison(12.5, *st)
    # directions set, empty bands: the bits of directional order 1, and no evaluation with a second-order part to ask about
    h.set_morison_second_order(True, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
    empty = h.compute_morison(12.5, *st)
    with pytest.raises(Exception):
        h.morison_increments(0)
    h.set_morison_second_order(False)
    first = h.compute_morison(12.5, *st)
    assert same_bits(empty, first) and first.reshape(3, 6).any(axis=1).all() and not np.array_equal(second, first)
    assert np.all(np.abs(second - first).reshape(3, 6).max(axis=1) > 1e-6 * np.abs(first).reshape(3, 6).max(axis=1))
    # no directions: the switch changes nothing, on or off
    h.set_wave_directions(None)
    h.set_morison_second_order(True)
    assert h.morison_second_order_directional() is True
    on = h.compute_morison(12.5, *st)
    inc_on = h.morison_increments(1)
    h.set_morison_second_order_directional(False)
    off = h.compute_morison(12.5, *st)
    inc_off = h.morison_increments(1)
    assert same_bits(on, off) and on.any() and all(same_bits(inc_on[k], inc_off[k]) for k in inc_on)
    assert not np.array_equal(on, second) and inc_on["eta2"].any()
    # the models without components under the switch: order 1
    h.set_morison_second_order_directional(True)
    h.add_waves_none()
    a = h.compute_morison(3.0, *st)
    h.set_morison_second_order(False)
    assert same_bits(a, h.compute_morison(3.0, *st)) and a.any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: the bits depend on the body alone
# ------------------------------------------------------------------------------------------------
def test_shards_other_bodies_and_repeats_leave_the_bits(HF):
    from hydrochrono_amd.hydro import HydroGroup
    whole = three_spread(HF.from_case, **CUT)
    group = three_spread(lambda case: HydroGroup.from_case(case, 2), **CUT)
    assert group.morison_second_order_directional() is True and whole.morison_second_order_directional() is True
    assert group.morison_second_order() == whole.morison_second_order() == dict(on=True, apply_ramp=True, **CUT)
    st = mi.moving_state(3, -3.0, 12.5)
    ref = whole.compute_morison(12.5, *st)
    assert ref.reshape(3, 6).any(axis=1).all()
    assert same_bits(group.compute_morison(12.5, *st), ref)
    for b, n in enumerate((33, 257, 5)):
        a, c = whole.morison_increments(b), group.morison_increments(b)
        assert all(same_bits(a[k], c[k]) for k in a) and a["eta2"].shape == (n,) and a["vel2"][:, 1].any()
    for _ in range(2):
        assert same_bits(whole.compute_morison(12.5, *st), ref)
    # another body's list replaced, then cleared: bodies 0 and 2 keep their bits
    whole.set_morison_elements(1, *mi.random_elements(300, 23))
    a = whole.compute_morison(12.5, *st)
    assert same_bits(a[:6], ref[:6]) and same_bits(a[12:], ref[12:]) and not same_bits(a[6:12], ref[6:12])
    whole.set_morison_elements(1, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    a = whole.compute_morison(12.5, *st)
    assert same_bits(a[:6], ref[:6]) and same_bits(a[12:], ref[12:]) and not a[6:12].any()
    whole.close()
    group.close()


def test_number_of_bodies_leaves_the_bits(HF):
    """The same body data (state, elements, wave model with its directions, rho, depth) as the only body of a 1-body context and as
    body 2 of a 3-body one."""
    from hydrochrono_amd.synthetic import many_body_case
    waves = dict(simulation_dt=0.05, simulation_duration=200.0, ramp_duration=20.0, wave_height=4.0, wave_period=9.0,
                 frequency_min=0.02, frequency_max=0.6, nfrequencies=24, peak_enhancement_factor=2.0, seed=4)
    el = mi.random_elements(130, 30)
    ctxs = []
    for N in (1, 3):
        case = many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)
        h = HF.from_case(case)
        mdi.spread_sea(h, case, waves)
        h.set_wave_directions(mdi.di.spread(24))
        h.set_morison_elements(N - 1, *el)
        h.set_morison_options(mwl=0.2)
        h.set_morison_second_order(True)
        h.set_morison_second_order_directional(True)
        ctxs.append(h)
    one, three = ctxs
    three.set_morison_elements(0, *mi.random_elements(70, 31))
    st1 = mi.moving_state(1, -1.0, 33.0, seed=5)
    st3 = [np.concatenate([x, x, x]) for x in st1]
    for x in st3:
        x[:2] += 0.37  # the other bodies move differently
    a, b = one.compute_morison(33.0, *st1), three.compute_morison(33.0, *st3)
    assert a.any() and same_bits(a, b[12:])
    i1, i3 = one.morison_increments(0), three.morison_increments(2)
    assert all(same_bits(i1[k], i3[k]) for k in i1) and i1["acc2"][:, 1].any()
    one.close()
    three.close()


# ------------------------------------------------------------------------------------------------
# 7: beside the steps, and the layers above
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 32])
def test_directional_second_order_morison_around_every_step_changes_no_force(HF, lookahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_morison in (False, True):
        h = HF.from_case(case)
        h.set_lookahead(lookahead)
        mdi.spread_sea(h, case, wi.sphere_waves(65))
        h.set_wave_directions(mdi.di.spread(65))
        if with_morison:
            h.set_morison_elements(0, *mi.random_elements(64, 2))
            h.set_morison_second_order(True)
            h.set_morison_second_order_directional(True)
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
            inc = h.morison_increments(0)
            assert inc["eta2"].any() and inc["vel2"][:, 1].any()
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    counts = (33, 0, 5)
    a, b = three_spread(HF.from_case, counts, **CUT), three_spread(HF.from_case, counts, **CUT)
    grp = three_spread(lambda c: HydroGroup.from_case(c, 3), counts, **CUT)
    first = three_spread(HF.from_case, counts, **CUT)
    first.set_morison_second_order(False)
    gplain = HydroGroup.from_case(case, 3)
    mdi.spread_sea(gplain, case, THREE8)
    gplain.set_wave_directions(mdi.di.spread(8))
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)
    for n in range(10):
        t = 0.01 * n + 25.0
        st = motion.state(t)
        fa = a.step(t, *st)
        total, mor = raw_step(b, t, st), b.compute_morison(t, *st)
        assert same_bits(fa, total + mor) and same_bits(a.morison(), mor)
        assert same_bits(grp.step(t, *st), gplain.step(t, *st) + mor) and same_bits(grp.morison(), mor)
        assert same_bits(grp.compute_morison(t, *st), mor)
    assert mor.any() and not np.array_equal(first.compute_morison(t, *st), mor)
    assert grp.morison_increments(0)["eta2"].size == 33 and grp.morison_increments(2)["vel2"][:, 1].any()
    for h in (a, b, first, grp, gplain):
        h.close()


# ------------------------------------------------------------------------------------------------
# 8: the C++ mirror
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "morison2_dir_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison2_dir_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (40, 31)
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(**dict(wi.sphere_waves(65), simulation_dt=0.015))
    h.set_wave_directions(np.full(65, -0.4))  # a uniform heading on the IRF model
    h.set_morison_elements(0, [[0, 0, -6.0], [2.5, 0.5, -3.0], [0, 0, 9.0]], [[3, 3, 12.0], [1, 1.5, 0.5], [5, 5, 5.0]], [[0, 0, 0], [2, 2, 1.0], [0, 0, 0]])
    h.set_morison_options(mwl=0.25)
    h.set_morison_second_order(True, **dict(CUT, diff_band=(0.05, 0.9)))
    h.set_morison_second_order_directional(True)
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total, mor = raw_step(h, t, st), h.compute_morison(t, *st)
        assert same_bits(row[19:25], mor) and same_bits(row[13:19], total + mor), t
        inc = h.morison_increments(0)
        assert same_bits(row[25:28], inc["eta2"]) and same_bits(row[28:31], inc["vel2"][:, 1]), t
    assert np.abs(rows[:, 19:21]).max(axis=0).min() > 1.0 and np.abs(rows[:, 25:28]).max() > 1e-5 and np.abs(rows[:, 28:31]).max() > 0
    h.close()


# ------------------------------------------------------------------------------------------------
# 9: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    import ctypes as C
    from hydrochrono_amd import capi
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    h = three_spread(HF.from_case, counts=(4, 3, 0))
    lib = h.lib
    z9, lin, out = np.zeros(9), np.tile([0.5, 0.0, 0.0], 3), np.empty(18)
    pos = np.tile([0.0, 0.0, -3.0], 3)

    def evaluation_works():
        assert lib.hc_morison_end(h.ctx, dp(out)) == INV  # nothing is pending
        assert lib.hc_compute_morison(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(out)) == OK and out[:12].any() and not out[12:].any()

    def getter():
        on = C.c_int(-1)
        assert lib.hc_get_morison_second_order_directional(h.ctx, C.byref(on)) == OK
        return on.value

    evaluation_works()
    assert lib.hc_get_morison_second_order_directional(h.ctx, None) == OK  # the pointer may be NULL
    # the getter round-trips; any non-zero value switches it on
    assert getter() == 1
    assert lib.hc_set_morison_second_order_directional(h.ctx, 0) == OK and getter() == 0 and h.morison_second_order_directional() is False
    # off under directions: the refusal it was, nothing pending, and the switch named beside the word "direction"
    for _ in range(2):
        assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == UNS
        msg = lib.hc_last_error(h.ctx)
        assert b"direction" in msg and b"hc_set_morison_second_order_directional" in msg
        assert lib.hc_compute_morison(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(out)) == UNS
        assert lib.hc_morison_end(h.ctx, dp(out)) == INV
    assert lib.hc_set_morison_second_order_directional(h.ctx, 7) == OK and getter() == 1
    evaluation_works()
    # the switch survives second order off and on; while second order is off it has no effect
    h.set_morison_second_order(False)
    assert getter() == 1
    evaluation_works()
    first = out.copy()
    assert lib.hc_set_morison_second_order_directional(h.ctx, 0) == OK
    evaluation_works()
    assert same_bits(out, first)
    assert lib.hc_set_morison_second_order_directional(h.ctx, 1) == OK
    h.set_morison_second_order(True)
    assert getter() == 1
    evaluation_works()
    assert not np.array_equal(out, first)
    # the setter while a begin is pending
    assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == OK
    assert lib.hc_set_morison_second_order_directional(h.ctx, 0) == INV and lib.hc_set_morison_second_order_directional(h.ctx, 1) == INV
    assert lib.hc_morison_end(h.ctx, dp(out)) == OK and getter() == 1
    evaluation_works()
    # the increments getter keeps its rules: new element lists forget the evaluation
    eta = np.empty(8)
    assert lib.hc_get_morison_increments(h.ctx, 0, None, dp(eta), None, None) == OK
    h.set_morison_elements(1, *mi.random_elements(3, 9))
    assert lib.hc_get_morison_increments(h.ctx, 0, None, dp(eta), None, None) == INV
    evaluation_works()
    # ... and between a later begin and its end it answers with the evaluation before
    before = h.morison_increments(0)
    assert lib.hc_morison_begin(h.ctx, 31.0, dp(pos), dp(z9), dp(lin), dp(z9)) == OK
    during = h.morison_increments(0)
    assert lib.hc_morison_end(h.ctx, dp(out)) == OK
    after = h.morison_increments(0)
    assert all(same_bits(before[k], during[k]) for k in before) and not same_bits(before["eta2"], after["eta2"])
    # the nonlinear surface on the second-order sea still refuses under directions
    import nonlinear_ref
    h.set_surface_mesh(0, nonlinear_ref.box_triangles([-2.0, -1.0, -3.0], [2.0, 1.0, 1.0], m=2))
    h.compute_nonlinear(30.0, pos, z9)  # (first order: fine under directions)
    h.set_nonlinear_second_order(True)
    with pytest.raises(Exception) as ei:
        h.compute_nonlinear(30.0, pos, z9)
    assert "direction" in str(ei.value)
    # more than 4096 components: refused by hc_morison_begin, nothing pending
    h.set_nonlinear_second_order(False)
    h.add_waves_irregular(**wi.three_waves(4097))
    h.set_wave_directions(np.full(4097, 0.3))  # (a uniform heading on the IRF model)
    assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == UNS and b"4096" in lib.hc_last_error(h.ctx)
    assert lib.hc_morison_end(h.ctx, dp(out)) == INV
    h.set_morison_second_order(False)
    evaluation_works()
    h.close()
