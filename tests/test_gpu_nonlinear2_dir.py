"""The nonlinear surface forces on the second-order sea in a short-crested sea on the GPU (hc_set_nonlinear_second_order_directional;
csrc/hc_nonlinear.hip: nl2_incr_kernel<true>, nl2_dir_panels_kernel, nl2_dir_tris_kernel) against the tests' NumPy restatement
(tests/nonlinear2_dir_ref.py), fed the context's own spectrum and directions, on the input sets of tests/nonlinear2_dir_inputs.py.

Tolerance: the bound nonlinear2_dir_ref returns per body and component -- that of tests/test_gpu_nonlinear2.py with the directional
scales (the derivation is in nonlinear2_dir_ref's docstring; nothing new).  q2 itself: 1e-11 of its sum |term|, the figure of the
pair sums (tests/test_gpu_wave_kinematics2_dir.py).  The wet test and the cut are discontinuities: every comparison first asserts the
conditions of tests/nonlinear2_dir_inputs.py."""
import os
import subprocess

import numpy as np
import pytest

import morison2_dir_inputs as mdi
import nonlinear2_dir_inputs as ndi
import nonlinear2_dir_ref as nd
import nonlinear2_ref as n2
import wave2_inputs as wi
import wave2_ref as w2
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case
from morison_ref import KIN_TOL, ramp_factor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
CUT = dict(diff_band=(0.05, 3.0), sum_band=(1.5, 6.0))
EMPTY = dict(diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
ci, di = ndi.ci, ndi.di


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def set_lists(h, lists):
    for b, l in enumerate(lists):
        if l is None:
            continue
        if l[0] == "panels":
            h.set_surface_panels(b, *l[1])
        else:
            h.set_surface_mesh(b, l[1], clip=True)


def raw_step(h, t, state):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def spread(make, N, lists, nf=5, depth=ci.DEPTH, mwl=0.35, directions=True, **second):
    """N bodies of the surface tests on the spread sea of ndi.waves(nf), the lists in force, second order (with `second`) and its
    directional form on.  make: HydroForces.from_case or a HydroGroup maker."""
    case = ci.synth_case(N, depth)
    h = make(case)
    ndi.spread_sea(h, case, nf)
    if directions:
        h.set_wave_directions(di.spread(nf))
    set_lists(h, lists)
    h.set_nonlinear_options(mwl=mwl)
    h.set_nonlinear_second_order(True, **second)
    h.set_nonlinear_second_order_directional(True)
    return h


def group_of(n):
    from hydrochrono_amd.hydro import HydroGroup
    return lambda case: HydroGroup.from_case(case, n)


LISTS3 = [ndi.tri_list(257), ndi.panel_list(12), ndi.tri_list(12)]


# ------------------------------------------------------------------------------------------------
# 1 and 2: parity inside the derived bound; the increments of the same evaluations
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ndi.SETS))
def test_parity_and_increments(HF, name):
    s = ndi.SETS[name]
    case = ci.synth_case(s["N"], s["depth"])
    h = HF.from_case(case)
    ndi.spread_sea(h, case, s["nf"])
    h.set_wave_directions(ndi.directions(name))
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == s["nf"] and h.simulation_parameters()[2] == s["depth"]
    assert np.array_equal(h.wave_directions(), ndi.directions(name))
    lists = s["lists"]()
    set_lists(h, lists)
    h.set_nonlinear_options(mwl=s["mwl"], wave_stretching=s["stretching"])
    bands = dict(diff_band=s["diff_band"], sum_band=s["sum_band"])
    h.set_nonlinear_second_order(True, **bands)
    h.set_nonlinear_second_order_directional(True)
    has = [b for b, l in enumerate(lists) if l is not None]
    for t in s["times"]:
        what = f"{name} t={t}"
        ref, pos, rpy = ndi.reference(name, comp, case["rho"], t)
        # the conditions again, on the context's own spectrum (margin and cut_span are asserted by ndi.reference)
        big = max(np.abs(ref["buoy"]).max(), np.abs(ref["fk"]).max())
        assert max(ref["bound_buoy"].max(), ref["bound_fk"].max()) < 1e-6 * big, what
        if s["tuned"] is not None:
            assert ref["flips"] >= 1, what
        if name.startswith("tris257_deep"):
            assert np.all(ref["cases"].sum(axis=0) > 0), ref["cases"]
        buoy, fk, _ = (x.reshape(-1, 6) for x in h.compute_nonlinear(t, pos, rpy))
        assert np.all(np.isfinite(buoy)) and np.all(np.isfinite(fk)), what
        for got, key in ((buoy, "buoy"), (fk, "fk")):
            err = np.abs(got - ref[key])
            worst = float(np.max(err / np.maximum(ref["bound_" + key], 1e-300)))
            print(f"{what}: {key} worst |gpu - ref| / bound = {worst:.3e}, max |{key}| = {np.max(np.abs(ref[key])):.3e}")
            assert np.all(err <= ref["bound_" + key]), f"{what}: {key} worst {worst:.3e} of the bound"
        for b, l in enumerate(lists):
            if l is None:
                assert h.nonlinear_point_count(b) == 0
                continue
            inc = h.nonlinear_increments(b)
            n_items = len(l[1][0]) if l[0] == "panels" else 3 * len(l[1])
            assert len(inc["p"]) == len(ref["p"][b]) == h.nonlinear_point_count(b) <= n_items  # a shared vertex is stored once
            if l[0] == "tris" and len(l[1]) >= 12:
                assert len(inc["p"]) < n_items
            assert np.allclose(inc["p"], ref["p"][b], rtol=0, atol=16 * 64 * 2.0 ** -52)
            e2, _, _ = h.wave_kinematics2(inc["p"], [t], mwl=s["mwl"], directional=True, **bands)
            assert same_bits(inc["eta2"], e2[0]) and inc["eta2"].any(), what
            qerr = np.abs(inc["q2"] - ref["q2"][b].astype(np.float64)) / ref["q2_scale"][b].astype(np.float64)
            print(f"{what}: body {b}: {len(inc['p'])} points for {n_items} items, q2 worst error / sum|term| = {qerr.max():.3e}")
            assert np.all(qerr <= KIN_TOL) and inc["q2"].any(), what
    # the increments change fk by far more than the bound
    h.set_nonlinear_second_order(False)
    first = h.compute_nonlinear(t, pos, rpy)[1].reshape(-1, 6)
    assert np.all(np.abs(first - fk)[has].max(axis=1) > 100 * ref["bound_fk"][has].max(axis=1))
    h.close()


def test_increments_bit_for_bit_across_the_ramp_and_for_a_regular_wave_with_a_heading(HF):
    h = spread(HF.from_case, 1, [ndi.tri_list(12)])
    pos, rpy = ci.state(1, 0.0)
    for mwl, kw in ((0.35, {}), (0.0, CUT), (0.35, dict(diff_band=(0.0, 0.5), sum_band=wi.NO_PAIR, apply_ramp=False))):
        h.set_nonlinear_options(mwl=mwl)
        h.set_nonlinear_second_order(True, **kw)
        for t in (-1.0, 7.5, 33.3):  # before, inside and after the ramp of 20 s
            h.compute_nonlinear(t, pos, rpy)
            inc = h.nonlinear_increments(0)
            assert inc["p"].shape == (8, 3)
            e2, _, _ = h.wave_kinematics2(inc["p"], [t], mwl=mwl, directional=True, **kw)
            assert same_bits(inc["eta2"], e2[0]), (mwl, kw, t)
            live = t > 0.0 or kw.get("apply_ramp") is False
            assert bool(inc["eta2"].any()) == live and bool(inc["q2"].any()) == live
    # a regular wave with a heading carries the regular phase of the nonlinear options
    h.add_waves_regular(0.5, 0.8)
    h.set_wave_directions([0.7])
    h.set_nonlinear_options(mwl=0.2, regular_phase=0.9)
    h.set_nonlinear_second_order(True)
    h.compute_nonlinear(5.0, pos, rpy)
    inc = h.nonlinear_increments(0)
    e2, _, _ = h.wave_kinematics2(inc["p"], [5.0], mwl=0.2, regular_phase=0.9, directional=True)
    assert same_bits(inc["eta2"], e2[0]) and inc["eta2"].any() and inc["q2"].any()
    # the long-crested evaluation after it: the increments of hc_wave_kinematics2 again
    h.set_wave_directions(None)
    h.compute_nonlinear(5.0, pos, rpy)
    inc = h.nonlinear_increments(0)
    e2, _, _ = h.wave_kinematics2(inc["p"], [5.0], mwl=0.2, regular_phase=0.9)
    assert same_bits(inc["eta2"], e2[0]) and inc["eta2"].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: a regular wave with a heading: first order plus Stokes' second-order elevation and pressure along the heading
# ------------------------------------------------------------------------------------------------
def test_regular_wave_with_a_heading_is_first_order_plus_stokes(HF):
    """One wet panel well below the trough on an upright body: fk = -p_d s with p_d = rho (w^2 A / k) px cos theta + rho q2
    - 1/2 rho |u1|^2, u1 along the heading, q2 = 2 w B C2 cos 2 theta of Stokes' second-order potential (the amplitude B written as
    in tests/test_gpu_morison2_dir.py).  Tolerances: those that file holds the same quantities to -- 1e-12 of every first-order
    term, 1e-10 of the Stokes term -- added up over the three terms of p_d; eta2 and q2 themselves to 1e-10."""
    depth, A, w, phi, mwl, t, beta = 30.0, 0.5, 0.8, 0.7, 0.25, 3.7, 0.7
    h = HF.from_case(ci.synth_case(1, depth))
    h.add_waves_regular(A, w)
    h.set_wave_directions([beta])
    k = h.regular_coeffs()[2]
    rho, g, _ = h.simulation_parameters()
    g = abs(g)
    c0, s0 = np.array([[1.0, -2.0, -6.0]]), np.array([[0.3, -0.2, 1.1]])
    h.set_surface_panels(0, c0, s0)
    h.set_nonlinear_options(mwl=mwl, regular_phase=phi)
    pos, z3 = np.array([12.0, 1.0, -1.0]), np.zeros(3)
    first = h.compute_nonlinear(t, pos, z3)[1]
    h.set_nonlinear_second_order(True)
    h.set_nonlinear_second_order_directional(True)
    got = h.compute_nonlinear(t, pos, z3)[1]
    P = pos + c0[0]
    cb, sb = np.cos(beta), np.sin(beta)
    theta = k * (P[0] * cb + P[1] * sb) - w * t + phi
    z = P[2] - mwl  # well below the trough: z2 = z - mwl, and a regular wave is neither stretched nor ramped
    assert -depth < z < -5.0
    deep = 2 * np.pi / k > depth or k * depth > 500
    px, pz = (np.exp(k * z),) * 2 if deep else (np.cosh(k * (z + depth)) / np.sinh(k * depth), np.sinh(k * (z + depth)) / np.sinh(k * depth))
    uh, uz = w * A * px * np.cos(theta), w * A * pz * np.sin(theta)
    R = w * w / g
    B = (A * g / w) ** 2 / (8 * w) * 6 * R * (k - R) * (k + R) / (2 * R - k * np.tanh(2 * k * depth))
    q2 = 2 * w * B * np.cosh(2 * k * (z + depth)) / np.cosh(2 * k * depth) * np.cos(2 * theta)
    terms = np.array([rho * (w * w * A / k) * px * np.cos(theta), rho * q2, -0.5 * rho * ((uh * cb) ** 2 + (uh * sb) ** 2 + uz * uz)])
    F = -terms.sum() * s0[0]
    want = np.concatenate([F, np.cross(c0[0], F)])
    tol_p = np.abs(terms) @ np.array([1e-12, 1e-10, 2e-12])
    tol = np.concatenate([tol_p * np.abs(s0[0]), np.abs(np.cross(np.abs(c0[0]), tol_p * np.abs(s0[0]))) + 2 * tol_p * np.abs(c0[0]).max() * np.abs(s0[0]).max()])
    print("regular: terms of p_d", terms, "worst error / tolerance", np.max(np.abs(got - want) / tol))
    assert np.all(np.abs(got - want) <= tol) and np.all(want != 0)
    assert abs(terms[1]) > 1e-9 * abs(terms[0]) and abs(terms[2]) > 1e-6 * abs(terms[0])
    assert not np.allclose(first, want, rtol=1e-9, atol=0)
    inc = h.nonlinear_increments(0)
    # eta2 of one component from the definition with R kept apart from k tanh k h, as B above (the context's k is on the dispersion
    # curve to 1e-6 1/m only, which Stokes' closed form -- a function of k alone -- weighs differently: 1e-3 of the term)
    gq = (k - R) * (k + R)
    Kp, Km = (12 * R * gq / (4 * R - 2 * k * np.tanh(2 * k * depth)) - gq) / R + 2 * R, -gq / R  # (K- of a component with itself: the set-down)
    eta2 = 0.25 * A * A * (Kp * np.cos(2 * theta) + Km)
    assert abs(eta2 - w2.stokes_eta2(A, k, depth, theta)) <= 1e-3 * abs(eta2)
    assert np.allclose(inc["eta2"][0], eta2, rtol=1e-10, atol=0)
    assert np.allclose(inc["q2"][0], q2, rtol=1e-10, atol=0)
    h.close()


# ------------------------------------------------------------------------------------------------
# 4: every direction 0: the long-crested second-order result
# ------------------------------------------------------------------------------------------------
def test_directions_all_zero_agree_with_the_long_crested_path(HF):
    lists = [ndi.tri_list(12), ndi.panel_list(12), None]
    h = spread(HF.from_case, 3, lists)
    comp = wk.irregular_components(h.irreg_spectrum())
    rho, g, depth = h.simulation_parameters()
    for t in (7.5, 33.3):
        pos, rpy = ci.state(3, t)
        kw = dict(mwl=0.35, stretching=True, ramp=ramp_factor(t, ndi.RAMP), ramp_duration=ndi.RAMP)
        h.set_wave_directions(np.zeros(5))
        dirs = h.compute_nonlinear(t, pos, rpy)
        inc_d = [h.nonlinear_increments(b) for b in (0, 1)]
        h.set_wave_directions(None)
        lc = h.compute_nonlinear(t, pos, rpy)
        inc_l = [h.nonlinear_increments(b) for b in (0, 1)]
        rd_ = nd.nonlinear2_dir(comp, np.zeros(5), abs(g), depth, rho, lists, t, pos, rpy, **kw)
        rl_ = n2.nonlinear2(comp, abs(g), depth, rho, lists, t, pos, rpy, **kw)
        assert min(rd_["margin"], rl_["margin"]) >= ndi.MIN_GAP and min(rd_["cut_span"], rl_["cut_span"]) >= ndi.MIN_SPAN
        for i, key in enumerate(("buoy", "fk")):
            err, bound = np.abs(dirs[i] - lc[i]).reshape(3, 6), rd_["bound_" + key] + rl_["bound_" + key]
            print(f"directions all 0, t={t}: {key} worst {float(np.max(err[:2] / bound[:2])):.3e} of the two bounds")
            assert np.all(err <= bound) and np.abs(lc[i]).max() > 1.0
        for a, b in zip(inc_d, inc_l):
            assert same_bits(a["p"], b["p"]) and a["eta2"].any() and b["eta2"].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 5: the zero cases
# ------------------------------------------------------------------------------------------------
def test_switch_without_directions_and_empty_bands_under_directions(HF):
    lists = [ndi.tri_list(257), None, ndi.panel_list(12)]
    pos, rpy = ci.state(3, 12.5)
    h = spread(HF.from_case, 3, lists)
    second = h.compute_nonlinear(12.5, pos, rpy)
    # directions set, empty bands: the bits of directional order 1, and no evaluation with a second-order part to ask about
    h.set_nonlinear_second_order(True, **EMPTY)
    empty = h.compute_nonlinear(12.5, pos, rpy)
    with pytest.raises(Exception):
        h.nonlinear_increments(0)
    h.set_nonlinear_second_order(False)
    first = h.compute_nonlinear(12.5, pos, rpy)
    assert all(same_bits(x, y) for x, y in zip(empty, first)) and same_bits(second[2], first[2])
    for b in (0, 2):
        r = slice(6 * b, 6 * b + 6)
        assert first[1][r].any() and np.abs(second[1][r] - first[1][r]).max() > 1e-6 * np.abs(first[1][r]).max(), b
    assert not second[1][6:12].any()
    # no directions: the switch changes nothing, on or off -- the bits of a context that never heard of it
    never = spread(HF.from_case, 3, lists, directions=False)
    never.set_nonlinear_second_order_directional(False)
    want = never.compute_nonlinear(12.5, pos, rpy)
    inc_want = never.nonlinear_increments(0)
    never.close()
    h.set_wave_directions(None)
    h.set_nonlinear_second_order(True)
    assert h.nonlinear_second_order_directional() is True
    on = h.compute_nonlinear(12.5, pos, rpy)
    inc_on = h.nonlinear_increments(0)
    h.set_nonlinear_second_order_directional(False)
    off = h.compute_nonlinear(12.5, pos, rpy)
    inc_off = h.nonlinear_increments(0)
    assert all(same_bits(x, y) and same_bits(x, z) for x, y, z in zip(on, off, want)) and on[1].any()
    assert all(same_bits(inc_on[k], inc_off[k]) and same_bits(inc_on[k], inc_want[k]) for k in inc_on) and inc_on["eta2"].any()
    assert not np.array_equal(on[1], second[1])
    # the models without components under the switch: order 1
    h.set_nonlinear_second_order_directional(True)
    h.add_waves_none()
    a = h.compute_nonlinear(3.0, pos, rpy)
    h.set_nonlinear_second_order(False)
    assert all(same_bits(x, y) for x, y in zip(a, h.compute_nonlinear(3.0, pos, rpy))) and a[0].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: a body's bits depend on the body alone
# ------------------------------------------------------------------------------------------------
def test_shards_other_bodies_grid_place_and_repeats_leave_the_bits(HF):
    pos, rpy = ci.state(3, 12.5)
    whole, group = spread(HF.from_case, 3, LISTS3, **CUT), spread(group_of(2), 3, LISTS3, **CUT)
    assert group.nonlinear_second_order_directional() is True and whole.nonlinear_second_order_directional() is True
    assert group.nonlinear_second_order() == whole.nonlinear_second_order() == dict(on=True, apply_ramp=True, **CUT)
    ref = whole.compute_nonlinear(12.5, pos, rpy)
    assert ref[1].reshape(3, 6).any(axis=1).all()
    got = group.compute_nonlinear(12.5, pos, rpy)
    assert all(same_bits(x, y) for x, y in zip(got, ref))
    for b in range(3):
        a, c = whole.nonlinear_increments(b), group.nonlinear_increments(b)
        assert all(same_bits(a[k], c[k]) for k in a) and a["eta2"].size == whole.nonlinear_point_count(b) == group.nonlinear_point_count(b)
    for _ in range(2):
        assert all(same_bits(x, y) for x, y in zip(whole.compute_nonlinear(12.5, pos, rpy), ref))
    # body 0's list replaced by one of the other kind with three chunks (bodies 1 and 2 move down the grid), then cleared
    keep = slice(6, 18)
    whole.set_surface_panels(0, *ndi.panel_list(768)[1])
    a = whole.compute_nonlinear(12.5, pos, rpy)
    assert same_bits(a[0][keep], ref[0][keep]) and same_bits(a[1][keep], ref[1][keep]) and not same_bits(a[1][:6], ref[1][:6])
    whole.set_surface_mesh(0, np.zeros((0, 3, 3)), clip=True)
    a = whole.compute_nonlinear(12.5, pos, rpy)
    assert same_bits(a[0][keep], ref[0][keep]) and same_bits(a[1][keep], ref[1][keep]) and not a[1][:6].any()
    set_lists(whole, LISTS3[:1])
    assert all(same_bits(x, y) for x, y in zip(whole.compute_nonlinear(12.5, pos, rpy), ref))
    whole.close()
    group.close()


def test_number_of_bodies_leaves_the_bits(HF):
    """The same body data as the only body of a 1-body context and as body 2 of a 3-body one."""
    tri = ndi.tri_list(257)
    one = spread(HF.from_case, 1, [tri], mwl=0.2)
    thr = spread(HF.from_case, 3, [ndi.panel_list(12), None, tri], mwl=0.2)
    p1, r1 = ci.state(1, 33.0)
    p3, r3 = np.tile(p1, (3, 1)), np.tile(r1, (3, 1))
    p3[:2] += 0.37  # the other bodies sit elsewhere
    a, b = one.compute_nonlinear(33.0, p1, r1), thr.compute_nonlinear(33.0, p3, r3)
    assert a[1].any() and all(same_bits(x, y[12:]) for x, y in zip(a[:2], b[:2]))  # (hs_lin is the bodies' own hydrostatic data)
    i1, i3 = one.nonlinear_increments(0), thr.nonlinear_increments(2)
    assert all(same_bits(i1[k], i3[k]) for k in i1) and i1["q2"].any()
    one.close()
    thr.close()


# ------------------------------------------------------------------------------------------------
# 7: beside the steps, the Morison path and hc_wave_kinematics2_dir
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 32])
def test_directional_second_order_surface_around_every_step_changes_no_force(HF, lookahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_surface in (False, True):
        h = HF.from_case(case)
        h.set_lookahead(lookahead)
        mdi.spread_sea(h, case, wi.sphere_waves(65))
        h.set_wave_directions(di.spread(65))
        if with_surface:
            h.set_surface_mesh(0, ci.mesh(12), clip=True)
            h.set_nonlinear_second_order(True)
            h.set_nonlinear_second_order_directional(True)
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        rows = []
        for n in range(100):  # three look-ahead blocks of 32 steps
            t = SPHERE_DT * n
            st = motion.state(t)
            if with_surface:
                h.nonlinear_begin(t, st[0], st[1])
            total = raw_step(h, t, st)
            if with_surface:
                assert h.nonlinear_end()[0].any()
            rows.append(np.concatenate([total, *h.components()]))
        if with_surface:
            inc = h.nonlinear_increments(0)
            assert inc["eta2"].any() and inc["q2"].any()
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


def test_morison2_dir_and_wave_kinematics2_dir_between_begin_and_end_are_undisturbed(HF):
    import morison2_inputs as mi
    h = spread(HF.from_case, 3, LISTS3, **CUT)
    h.set_morison_elements(0, *mi.random_elements(33, 20))
    h.set_morison_second_order(True, diff_band=(0.0, 0.9), sum_band=wi.NO_PAIR)
    h.set_morison_second_order_directional(True)
    pos, rpy = ci.state(3, 12.5)
    z = np.zeros((3, 3))
    pts = np.array([[1.0, 2.0, -2.0], [7.0, -3.0, 0.5]])
    other = dict(diff_band=(0.1, 0.7), sum_band=(2.0, 3.0), directional=True)
    nl = h.compute_nonlinear(12.5, pos, rpy)
    mor = h.compute_morison(12.5, pos, rpy, z, z)
    kin = h.wave_kinematics2(pts, [12.5], mwl=0.1, **other)
    inc = h.nonlinear_increments(0)
    h.nonlinear_begin(12.5, pos, rpy)
    assert all(same_bits(x, y) for x, y in zip(h.wave_kinematics2(pts, [12.5], mwl=0.1, **other), kin)) and kin[1][..., 1].any()
    assert same_bits(h.compute_morison(12.5, pos, rpy, z, z), mor) and mor.any() and h.morison_increments(0)["vel2"][:, 1].any()
    held = h.nonlinear_increments(0)  # the evaluation before still answers
    assert all(same_bits(held[k], inc[k]) for k in inc)
    assert all(same_bits(x, y) for x, y in zip(h.nonlinear_end(), nl)) and nl[1].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 8: the layers above
# ------------------------------------------------------------------------------------------------
def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = ci.synth_case(3)
    lists = [ndi.tri_list(12), None, ndi.panel_list(12)]
    a, b, first = (spread(HF.from_case, 3, lists, **CUT) for _ in range(3))
    first.set_nonlinear_second_order(False)
    grp, gplain = spread(group_of(3), 3, lists, **CUT), spread(group_of(3), 3, [None] * 3)
    for h in (a, first, grp):
        h.set_nonlinear_mode(2)
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4, amplitude=0.3)
    for n in range(10):
        t = 0.01 * n + 25.0
        st = motion.state(t)
        total = raw_step(b, t, st)
        buoy, fk, hs = b.compute_nonlinear(t, st[0], st[1])

        def by_hand(total):
            want = total.copy()
            for body in (0, 2):
                r = slice(6 * body, 6 * body + 6)
                want[r] = total[r] - hs[r] + buoy[r]
                want[r] = want[r] + fk[r]
            return want

        want = by_hand(total)
        assert same_bits(a.step(t, *st), want) and all(same_bits(x, y) for x, y in zip(a.nonlinear(), (buoy, fk, hs)))
        assert same_bits(grp.step(t, *st), by_hand(gplain.step(t, *st)))
        assert all(same_bits(x, y) for x, y in zip(grp.compute_nonlinear(t, st[0], st[1]), (buoy, fk, hs)))
    assert fk.any() and not np.array_equal(first.step(t, *st), want)
    assert grp.nonlinear_increments(0)["eta2"].size == 8 and grp.nonlinear_increments(2)["q2"].size == 12
    for h in (a, b, first, grp, gplain):
        h.close()


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "nonlinear2_dir_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nonlinear2_dir_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (12, 53)
    from test_gpu_surface_clip_cpp import caller_box
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(**dict(wi.sphere_waves(65), simulation_dt=0.015))
    h.set_wave_directions(np.full(65, -0.4))  # a uniform heading on the IRF model
    h.set_surface_mesh(0, caller_box(2.0, 1.5, -3.0, 4.0), clip=True)
    h.set_nonlinear_options(mwl=0.25)
    h.set_nonlinear_second_order(True, diff_band=(0.05, 0.9), sum_band=(1.5, 6.0))
    h.set_nonlinear_second_order_directional(True)
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total = raw_step(h, t, st)
        buoy, fk, hs = row[19:25], row[25:31], row[31:37]
        assert same_bits(row[13:19], total - hs + buoy + fk), t
        assert all(same_bits(x, y) for x, y in zip(h.compute_nonlinear(t, st[0], st[1]), (buoy, fk, hs))), t
        inc = h.nonlinear_increments(0)
        assert same_bits(row[37:45], inc["eta2"]) and same_bits(row[45:53], inc["q2"]), t
    assert np.abs(rows[:, 25:28]).max() > 1.0 and np.abs(rows[:, 37:45]).max() > 1e-5 and np.abs(rows[:, 45:53]).max() > 1e-5
    h.close()


# ------------------------------------------------------------------------------------------------
# 9: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    import ctypes as C

    from hydrochrono_amd import capi
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    h = spread(HF.from_case, 3, [ndi.tri_list(12), ndi.panel_list(12), None])
    lib = h.lib
    pos, rpy = (np.ascontiguousarray(x).reshape(-1) for x in ci.state(3, 30.0))
    o = [np.empty(18) for _ in range(3)]

    def evaluation_works():
        assert lib.hc_nonlinear_end(h.ctx, None, None, None) == INV  # nothing is pending
        assert lib.hc_compute_nonlinear(h.ctx, 30.0, dp(pos), dp(rpy), dp(o[0]), dp(o[1]), dp(o[2])) == OK
        assert o[0][:12].any() and not o[0][12:].any()

    def getter():
        on = C.c_int(-1)
        assert lib.hc_get_nonlinear_second_order_directional(h.ctx, C.byref(on)) == OK
        return on.value

    set_dir = lambda v: lib.hc_set_nonlinear_second_order_directional(h.ctx, v)
    evaluation_works()
    assert lib.hc_get_nonlinear_second_order_directional(h.ctx, None) == OK  # the pointer may be NULL
    # the getter round-trips; any non-zero value switches it on; a new context has it off
    assert getter() == 1
    assert set_dir(0) == OK and getter() == 0 and h.nonlinear_second_order_directional() is False
    fresh = HF.from_case(ci.synth_case(1))
    assert fresh.nonlinear_second_order_directional() is False
    fresh.close()
    # off under directions: the refusal it was, nothing pending, and the switch named beside the word "direction"
    for _ in range(2):
        assert lib.hc_nonlinear_begin(h.ctx, 30.0, dp(pos), dp(rpy)) == UNS
        msg = lib.hc_last_error(h.ctx)
        assert b"direction" in msg and b"hc_set_nonlinear_second_order_directional" in msg
        assert lib.hc_compute_nonlinear(h.ctx, 30.0, dp(pos), dp(rpy), dp(o[0]), dp(o[1]), dp(o[2])) == UNS
        assert lib.hc_nonlinear_end(h.ctx, None, None, None) == INV
    assert set_dir(7) == OK and getter() == 1
    evaluation_works()
    second = [x.copy() for x in o]
    # the switch survives second order off and on; while second order is off it has no effect
    h.set_nonlinear_second_order(False)
    assert getter() == 1
    evaluation_works()
    first = [x.copy() for x in o]
    assert set_dir(0) == OK
    evaluation_works()
    assert all(same_bits(x, y) for x, y in zip(o, first))
    assert set_dir(1) == OK
    h.set_nonlinear_second_order(True)
    assert getter() == 1
    evaluation_works()
    assert all(same_bits(x, y) for x, y in zip(o, second)) and not np.array_equal(o[1], first[1])
    # the setter while a begin is pending; the increments query still answers
    eta = np.empty(16)
    assert lib.hc_nonlinear_begin(h.ctx, 30.0, dp(pos), dp(rpy)) == OK
    assert set_dir(0) == INV and set_dir(1) == INV
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == OK
    assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == OK and getter() == 1
    evaluation_works()
    # the increments getter keeps its layout and its rules
    assert lib.hc_get_nonlinear_increments(h.ctx, 1, 12, None, dp(eta), dp(eta)) == OK
    for body, cnt in ((-1, 8), (3, 8), (0, 7), (1, 8)):
        assert lib.hc_get_nonlinear_increments(h.ctx, body, cnt, None, dp(eta), None) == INV
    h.set_surface_mesh(0, ci.mesh(12), clip=True)
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == INV
    evaluation_works()
    # more than 4096 components: refused by hc_nonlinear_begin, nothing pending; fine again once second order is off
    h.add_waves_irregular(**dict(ndi.waves(4097), frequency_min=0.05, frequency_max=0.8))
    h.set_wave_directions(np.full(4097, 0.3))  # (a uniform heading on the IRF model)
    assert lib.hc_nonlinear_begin(h.ctx, 30.0, dp(pos), dp(rpy)) == UNS and b"4096" in lib.hc_last_error(h.ctx)
    assert lib.hc_compute_nonlinear(h.ctx, 30.0, dp(pos), dp(rpy), dp(o[0]), dp(o[1]), dp(o[2])) == UNS
    assert lib.hc_nonlinear_end(h.ctx, None, None, None) == INV
    h.set_nonlinear_second_order(False)
    evaluation_works()
    h.close()
