"""The nonlinear surface forces on the second-order sea on the GPU (hc_set_nonlinear_second_order, hc_get_nonlinear_increments;
csrc/hc_nonlinear.hip: nl2_incr_kernel, nl2_panels_kernel, nl2_tris_kernel) against the tests' NumPy restatement
(tests/nonlinear2_ref.py), fed the context's own spectrum, on the input sets of tests/nonlinear2_inputs.py.

Tolerance: the bound nonlinear2_ref returns per body and component -- those of nonlinear_ref and surface_clip_ref with 1e-11 sum|term|
of every first-order sum and of every increment propagated through p_d = ramp p_d1 + rho q2 - 1/2 rho ramp^2 |u1|^2 (the derivation is
in nonlinear2_ref's docstring).  q2 itself: 1e-11 of its sum |term|, the figure of the pair sums (tests/test_gpu_wave_kinematics2.py).
The wet test and the cut are discontinuities: every comparison first asserts the conditions of tests/nonlinear2_inputs.py."""
import os
import subprocess

import numpy as np
import pytest

import nonlinear2_inputs as ni
import wave2_inputs as wi
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case
from morison_ref import KIN_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
CUT = dict(diff_band=(0.05, 3.0), sum_band=(1.5, 6.0))
EMPTY = dict(diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
ci = ni.ci


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


def three(HF, lists, waves=None, cls=None, **kw):
    """the three-body system of the surface tests in the sea of ni.waves(5), mwl 0.35"""
    h = (cls or HF).from_case(ci.synth_case(3), *([3] if cls else []), **kw)
    h.add_waves_irregular(**(waves or ni.waves(5)))
    set_lists(h, lists)
    h.set_nonlinear_options(mwl=0.35)
    return h


LISTS3 = [ni.tri_list(257), ni.panel_list(12), ni.tri_list(12)]


# ------------------------------------------------------------------------------------------------
# 1 and 2: parity inside the derived bound; the increments of the same evaluations
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ni.SETS))
def test_parity_and_increments(HF, name):
    s = ni.SETS[name]
    case = ci.synth_case(s["N"], s["depth"])
    h = HF.from_case(case)
    h.add_waves_irregular(**ni.waves(s["nf"]))
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == s["nf"] and h.simulation_parameters()[2] == s["depth"]
    lists = s["lists"]()
    set_lists(h, lists)
    h.set_nonlinear_options(mwl=s["mwl"], wave_stretching=s["stretching"])
    bands = dict(diff_band=s["diff_band"], sum_band=s["sum_band"])
    h.set_nonlinear_second_order(True, **bands)
    for t in s["times"]:
        what = f"{name} t={t}"
        ref, pos, rpy = ni.reference(name, comp, case["rho"], t)
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
            e2, _, _ = h.wave_kinematics2(inc["p"], [t], mwl=s["mwl"], **bands)
            assert same_bits(inc["eta2"], e2[0]) and inc["eta2"].any(), what
            qerr = np.abs(inc["q2"] - ref["q2"][b].astype(np.float64)) / ref["q2_scale"][b].astype(np.float64)
            print(f"{what}: body {b}: {len(inc['p'])} points for {n_items} items, q2 worst error / sum|term| = {qerr.max():.3e}")
            assert np.all(qerr <= KIN_TOL) and inc["q2"].any(), what
    h.close()


def test_increments_bit_for_bit_across_the_ramp_and_for_a_regular_wave(HF):
    h = HF.from_case(ci.synth_case(1))
    h.add_waves_irregular(**ni.waves(5))
    set_lists(h, [ni.tri_list(12)])
    pos, rpy = ci.state(1, 0.0)
    for mwl, kw in ((0.35, {}), (0.0, CUT), (0.35, dict(diff_band=(0.0, 0.5), sum_band=wi.NO_PAIR, apply_ramp=False))):
        h.set_nonlinear_options(mwl=mwl)
        h.set_nonlinear_second_order(True, **kw)
        for t in (-1.0, 7.5, 33.3):  # before, inside and after the ramp of 20 s
            h.compute_nonlinear(t, pos, rpy)
            inc = h.nonlinear_increments(0)
            assert inc["p"].shape == (8, 3)
            e2, _, _ = h.wave_kinematics2(inc["p"], [t], mwl=mwl, **kw)
            assert same_bits(inc["eta2"], e2[0]), (mwl, kw, t)
            live = t > 0.0 or kw.get("apply_ramp") is False
            assert bool(inc["eta2"].any()) == live and bool(inc["q2"].any()) == live
    # a regular wave carries the regular phase of the nonlinear options; in finite depth q2 is Stokes' term
    h.add_waves_regular(0.5, 0.8)
    h.set_nonlinear_options(mwl=0.2, regular_phase=0.9)
    h.set_nonlinear_second_order(True)
    h.compute_nonlinear(5.0, pos, rpy)
    inc = h.nonlinear_increments(0)
    e2, _, _ = h.wave_kinematics2(inc["p"], [5.0], mwl=0.2, regular_phase=0.9)
    assert same_bits(inc["eta2"], e2[0]) and inc["eta2"].any() and inc["q2"].any()
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: order 1 keeps its bits, order 2 differs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["panels", "tris"])
def test_order_one_keeps_its_bits_and_order_two_differs(HF, kind):
    lists = [ni.panel_list(257) if kind == "panels" else ni.tri_list(257), None, ni.panel_list(12) if kind == "panels" else ni.tri_list(12)]
    pos, rpy = ci.state(3, 12.5)
    never = three(HF, lists)  # a context that never heard of the switch
    want = never.compute_nonlinear(12.5, pos, rpy)
    never.close()
    h = three(HF, lists)
    assert h.nonlinear_second_order() == dict(on=False, diff_band=(0.0, INF), sum_band=(0.0, INF), apply_ramp=True)
    h.set_nonlinear_second_order(True)
    second = h.compute_nonlinear(12.5, pos, rpy)
    h.set_nonlinear_second_order(False)
    off = h.compute_nonlinear(12.5, pos, rpy)
    h.set_nonlinear_second_order(True, **EMPTY)
    empty = h.compute_nonlinear(12.5, pos, rpy)
    for k in range(3):
        assert want[k].tobytes() == off[k].tobytes() == empty[k].tobytes(), k
    assert want[1].reshape(3, 6)[[0, 2]].any(axis=1).all() and same_bits(second[2], want[2])
    for b in (0, 2):
        r = slice(6 * b, 6 * b + 6)
        assert np.abs(second[1][r] - want[1][r]).max() > 1e-6 * np.abs(want[1][r]).max(), b
    assert not second[1][6:12].any()
    # the models without components: the bits of order 1 as well
    rec_t = 0.05 * np.arange(400)
    for model in ("nowave", "eta_record"):
        if model == "nowave":
            h.add_waves_none()
        else:
            h.add_waves_irregular_eta(rec_t, 0.5 * np.sin(0.8 * rec_t), 0.05)
        h.set_nonlinear_second_order(True)
        on = h.compute_nonlinear(3.0, pos, rpy)
        h.set_nonlinear_second_order(False)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(on, h.compute_nonlinear(3.0, pos, rpy))) and on[0].any(), model
    h.close()
    fresh = HF.from_case(ci.synth_case(3))  # no wave model at all
    set_lists(fresh, lists)
    a = fresh.compute_nonlinear(3.0, pos, rpy)
    fresh.set_nonlinear_second_order(True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, fresh.compute_nonlinear(3.0, pos, rpy))) and a[0].any()
    fresh.close()


# ------------------------------------------------------------------------------------------------
# 4: a body's bits depend on the body alone
# ------------------------------------------------------------------------------------------------
def test_shards_other_bodies_grid_place_and_repeats_leave_the_bits(HF):
    from hydrochrono_amd.hydro import HydroGroup
    pos, rpy = ci.state(3, 12.5)
    whole, group = three(HF, LISTS3), three(HF, LISTS3, cls=HydroGroup)
    for h in (whole, group):
        h.set_nonlinear_second_order(True, **CUT)
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
    whole.set_surface_panels(0, *ni.panel_list(768)[1])
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
    one, thr = HF.from_case(ci.synth_case(1)), HF.from_case(ci.synth_case(3))
    tri = ni.tri_list(257)[1]
    one.set_surface_mesh(0, tri, clip=True)
    thr.set_surface_mesh(2, tri, clip=True)
    thr.set_surface_panels(0, *ni.panel_list(12)[1])
    for h in (one, thr):
        h.add_waves_irregular(**ni.waves(5))
        h.set_nonlinear_options(mwl=0.2)
        h.set_nonlinear_second_order(True)
    p1, r1 = ci.state(1, 33.0)
    p3, r3 = np.tile(p1, (3, 1)), np.tile(r1, (3, 1))
    p3[:2] += 0.37  # the other bodies sit elsewhere
    a, b = one.compute_nonlinear(33.0, p1, r1), thr.compute_nonlinear(33.0, p3, r3)
    assert a[1].any() and all(same_bits(x, y[12:]) for x, y in zip(a[:2], b[:2]))  # (hs_lin is the bodies' own hydrostatic data)
    i1, i3 = one.nonlinear_increments(0), thr.nonlinear_increments(2)
    assert all(same_bits(i1[k], i3[k]) for k in i1)
    one.close()
    thr.close()


# ------------------------------------------------------------------------------------------------
# 5: beside the steps, the Morison path and hc_wave_kinematics2
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 32])
def test_second_order_surface_around_every_step_changes_no_force(HF, lookahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_surface in (False, True):
        h = HF.from_case(case)
        h.set_lookahead(lookahead)
        h.add_waves_irregular(**wi.sphere_waves(65))
        if with_surface:
            h.set_surface_mesh(0, ci.mesh(12), clip=True)
            h.set_nonlinear_second_order(True)
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
            assert h.nonlinear_increments(0)["eta2"].any()
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


def test_morison2_and_wave_kinematics2_between_begin_and_end_are_undisturbed(HF):
    import morison2_inputs as mi
    h = three(HF, LISTS3)
    h.set_morison_elements(0, *mi.random_elements(33, 20))
    h.set_morison_second_order(True, diff_band=(0.0, 0.9), sum_band=wi.NO_PAIR)
    h.set_nonlinear_second_order(True, **CUT)
    pos, rpy = ci.state(3, 12.5)
    z = np.zeros((3, 3))
    pts = np.array([[1.0, 0.0, -2.0], [7.0, 0.0, 0.5]])
    other = dict(diff_band=(0.1, 0.7), sum_band=(2.0, 3.0))
    nl = h.compute_nonlinear(12.5, pos, rpy)
    mor = h.compute_morison(12.5, pos, rpy, z, z)
    kin = h.wave_kinematics2(pts, [12.5], mwl=0.1, **other)
    inc = h.nonlinear_increments(0)
    h.nonlinear_begin(12.5, pos, rpy)
    assert all(same_bits(x, y) for x, y in zip(h.wave_kinematics2(pts, [12.5], mwl=0.1, **other), kin))
    assert same_bits(h.compute_morison(12.5, pos, rpy, z, z), mor) and mor.any()
    held = h.nonlinear_increments(0)  # the evaluation before still answers
    assert all(same_bits(held[k], inc[k]) for k in inc)
    assert all(same_bits(x, y) for x, y in zip(h.nonlinear_end(), nl))
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: the layers above
# ------------------------------------------------------------------------------------------------
def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = ci.synth_case(3)
    lists = [ni.tri_list(12), None, ni.panel_list(12)]
    a, b, first = three(HF, lists), three(HF, lists), three(HF, lists)
    grp, gplain = three(HF, lists, cls=HydroGroup), three(HF, [None] * 3, cls=HydroGroup)
    for h in (a, b, grp):
        h.set_nonlinear_second_order(True, **CUT)
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
    with pytest.raises(Exception):
        grp.nonlinear_increments(1 + 3)
    assert grp.nonlinear_increments(0)["eta2"].size == 8 and grp.nonlinear_increments(2)["eta2"].size == 12
    for h in (a, b, first, grp, gplain):
        h.close()


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "nonlinear2_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nonlinear2_caller.cpp"),
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
    h.set_surface_mesh(0, caller_box(2.0, 1.5, -3.0, 4.0), clip=True)
    h.set_nonlinear_options(mwl=0.25)
    h.set_nonlinear_second_order(True, diff_band=(0.05, 0.9), sum_band=(1.5, 6.0))
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
# 7: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    import ctypes as C

    from hydrochrono_amd import capi
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    h = three(HF, [ni.tri_list(12), ni.panel_list(12), None])
    lib = h.lib
    pos, rpy = (np.ascontiguousarray(x).reshape(-1) for x in ci.state(3, 30.0))
    o = [np.empty(18) for _ in range(3)]

    def plain_evaluation_works():
        assert lib.hc_nonlinear_end(h.ctx, None, None, None) == INV  # nothing is pending
        assert lib.hc_compute_nonlinear(h.ctx, 30.0, dp(pos), dp(rpy), dp(o[0]), dp(o[1]), dp(o[2])) == OK
        assert o[0][:12].any() and not o[0][12:].any()

    def set2(on=1, dlo=0.0, dhi=INF, slo=0.0, shi=INF, ramp=1):
        return lib.hc_set_nonlinear_second_order(h.ctx, on, dlo, dhi, slo, shi, ramp)

    eta = np.empty(16)
    n = C.c_int()
    assert lib.hc_get_nonlinear_point_count(h.ctx, 0, C.byref(n)) == OK and n.value == 8
    assert lib.hc_get_nonlinear_point_count(h.ctx, 1, C.byref(n)) == OK and n.value == 12
    assert lib.hc_get_nonlinear_point_count(h.ctx, 2, C.byref(n)) == OK and n.value == 0
    for body in (-1, 3):
        assert lib.hc_get_nonlinear_point_count(h.ctx, body, C.byref(n)) == INV
    assert lib.hc_get_nonlinear_point_count(h.ctx, 0, None) == INV
    # off: no increments to ask for
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == INV
    plain_evaluation_works()
    # cut-offs: negative, NaN, lo > hi -- and the setting before stays
    assert set2(dlo=0.1, dhi=0.9) == OK
    for bad in (dict(dlo=-0.1), dict(dhi=np.nan), dict(slo=np.nan), dict(shi=-1.0), dict(dlo=0.5, dhi=0.4), dict(slo=2.0, shi=1.0),
                dict(on=0, dlo=-1.0)):
        assert set2(**bad) == INV and (b"cut-off" in lib.hc_last_error(h.ctx)), bad
        assert h.nonlinear_second_order() == dict(on=True, diff_band=(0.1, 0.9), sum_band=(0.0, INF), apply_ramp=True)
        plain_evaluation_works()
    # off and on again: the evaluations before are forgotten, and there is none since
    assert set2(on=0) == OK and set2() == OK
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == INV
    plain_evaluation_works()
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == OK
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, None, None) == OK  # any pointer may be NULL
    assert lib.hc_get_nonlinear_increments(h.ctx, 1, 12, None, dp(eta), None) == OK
    for body, cnt in ((-1, 8), (3, 8), (100, 8), (0, 7), (0, 9), (1, 8)):
        assert lib.hc_get_nonlinear_increments(h.ctx, body, cnt, None, dp(eta), None) == INV
    # an evaluation without a second-order part forgets the one before; so does a new list
    assert set2(dlo=100.0, dhi=200.0, slo=100.0, shi=200.0) == OK
    plain_evaluation_works()
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == INV
    assert set2() == OK
    plain_evaluation_works()
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == OK
    h.set_surface_mesh(0, ci.mesh(12), clip=True)
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == INV
    plain_evaluation_works()
    # a call while a begin is pending; the query still answers
    assert lib.hc_nonlinear_begin(h.ctx, 30.0, dp(pos), dp(rpy)) == OK
    assert set2(on=0) == INV and set2(dhi=0.5) == INV
    assert lib.hc_get_nonlinear_increments(h.ctx, 0, 8, None, dp(eta), None) == OK
    assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == OK
    assert h.nonlinear_second_order()["on"] is True
    plain_evaluation_works()
    # a shard context answers for its own bodies only
    sh = three(HF, [ni.tri_list(12), ni.panel_list(12), None], body_range=(1, 2))
    sh.set_nonlinear_second_order(True)
    o6 = [np.empty(6) for _ in range(3)]
    assert lib.hc_compute_nonlinear(sh.ctx, 30.0, dp(pos), dp(rpy), dp(o6[0]), dp(o6[1]), dp(o6[2])) == OK
    assert lib.hc_get_nonlinear_increments(sh.ctx, 1, 12, None, dp(eta), None) == OK
    for body, cnt in ((0, 8), (2, 0)):
        assert lib.hc_get_nonlinear_increments(sh.ctx, body, cnt, None, dp(eta), None) == INV
    sh.close()
    # more than 4096 components: refused by hc_nonlinear_begin, nothing pending; fine again once second order is off or the sea smaller
    h.add_waves_irregular(**dict(ni.waves(4097), frequency_min=0.05, frequency_max=0.8))
    assert lib.hc_nonlinear_begin(h.ctx, 30.0, dp(pos), dp(rpy)) == UNS
    assert lib.hc_compute_nonlinear(h.ctx, 30.0, dp(pos), dp(rpy), dp(o[0]), dp(o[1]), dp(o[2])) == UNS
    assert lib.hc_nonlinear_end(h.ctx, None, None, None) == INV
    assert set2(on=0) == OK
    plain_evaluation_works()
    assert set2() == OK
    h.add_waves_irregular(**ni.waves(5))
    plain_evaluation_works()
    with pytest.raises(Exception):
        h.set_nonlinear_second_order(True, diff_band=(1.0, 0.5))
    h.close()
