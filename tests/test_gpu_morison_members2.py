"""Morison strip members on the second-order sea on the GPU (hc_set_morison_members_second_order,
hc_get_morison_member_node_increments, hc_get_morison_member_point_increments; csrc/hc_morison_members.hip:
morison_member2_nodes_kernel, morison_member2_points_kernel and the order-2 item kernels) against the tests' restatement
(tests/morison_members2_ref.py), fed the context's own spectrum, on the inputs of tests/morison_members2_inputs.py.  The short-crested
sea is tests/test_gpu_morison_members2_dir.py.

Tolerance: the bound the restatement returns per body, per member row and per component -- morison_members_ref's derivation with
1e-11 sum|term| of eta2 added to every node's delta h and 1e-11 sum|term| of u2, a2 added to the kinematics part (the derivation is
in morison_members2_ref's docstring).  The cut is a discontinuity in the node's wet state: every comparison first asserts, on the
reference side, that every node is further from the free surface of eta1 + eta2 than the bound of its own error."""
import os
import subprocess

import numpy as np
import pytest

import morison2_inputs as m2i
import morison_members2_inputs as mi
import morison_members2_ref as m2
import morison_members_ref as mm
import wave2_inputs as wi
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_TOL = 16 * 64 * 2.0 ** -52  # the rounding allowance of tests/test_gpu_morison2.py for a stored point
THREE8 = wi.three_waves(8)


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def set_members(h, lists):
    for b, ml in enumerate(lists):
        if ml is not None:
            h.set_morison_members(b, *ml)


def raw_step(h, t, state):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def context(HF, name, members=True, elements=None, second=True, switch=True, bands=None, make=None):
    """a context (or, with make, a group) on a set's case and waves with the Morison options of the set"""
    s = mi.SETS[name]
    h = (make or HF.from_case)(s["case"]())
    h.add_waves_irregular(**s["waves"])
    if members:
        set_members(h, s["lists"]())
    for b, el in enumerate(elements or []):
        if el is not None:
            h.set_morison_elements(b, *el)
    h.set_morison_options(mwl=mi.MWL, wave_stretching=s["stretching"])
    d, sm = bands or (s["diff_band"], s["sum_band"])
    h.set_morison_second_order(second, diff_band=d, sum_band=sm)
    h.set_morison_members_second_order(switch)
    return h


ELEMENTS = [None, m2i.random_elements(33, 21), m2i.random_elements(5, 22)]  # body 1 carries elements alone, body 2 both


# ------------------------------------------------------------------------------------------------
# 1 and 2: parity inside the derived bound; the increments are hc_wave_kinematics2's, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mi.SETS))
def test_parity_inside_the_derived_bound_and_increments_bit_for_bit(HF, name):
    s = mi.SETS[name]
    h = context(HF, name)
    comp = mi.components(h, name, False)
    assert comp[0].size == s["waves"]["nfrequencies"]
    _, g, depth = h.simulation_parameters()
    assert depth == s["case"]()["water_depth"] and h.morison_members_second_order() is True
    ref = mi.reference(name, comp, abs(g))
    mi.check_conditions(ref, name)
    t, st = s["t"], mi.state(name)
    got = h.compute_morison(t, *st).reshape(-1, 6)
    err = np.abs(got - ref["F"])
    worst = float(np.max(err / np.maximum(ref["bound"], 1e-300)))
    print(f"{name}: worst |gpu - ref| / bound = {worst:.3e} per body, max |F| = {np.max(np.abs(ref['F'])):.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= ref["bound"]), f"{name}: worst {worst:.3e} of the bound"
    assert not got[1].any()
    for b in (0, 2):
        rows = h.morison_member_forces(b)
        e = np.abs(rows - ref["members"][b])
        w = float(np.max(e / np.maximum(ref["member_bound"][b], 1e-300)))
        print(f"{name} body {b}: worst member row |gpu - ref| / bound = {w:.3e}")
        assert np.all(e <= ref["member_bound"][b]), (name, b, w)
        # both sum levels, serially in FP64
        acc = np.zeros(6)
        for r in rows:
            acc = acc + r
        assert same_bits(acc, got[b])
        inc = h.morison_member_increments(b)
        wet = ref["wet"][b]
        assert np.allclose(inc["node_p"], ref["node_p"][b], rtol=0, atol=P_TOL) and np.allclose(inc["p"][wet], ref["p"][b][wet], rtol=0, atol=P_TOL)
        # the restatement's increments, inside their own 1e-11 sum|term| (far inside: a sanity check of the layout)
        assert np.allclose(inc["node_eta2"], ref["node_eta2"][b], rtol=1e-9, atol=1e-12)
        assert np.allclose(inc["vel2"][wet], ref["u2"][b][wet], rtol=1e-8, atol=1e-11)
        kw = dict(mwl=mi.MWL, diff_band=s["diff_band"], sum_band=s["sum_band"])
        e2, _, _ = h.wave_kinematics2(inc["node_p"], [t], **kw)
        assert same_bits(inc["node_eta2"], e2[0]) and inc["node_eta2"].all(), (name, b)
        e2, v2, a2 = h.wave_kinematics2(inc["p"], [t], **kw)
        assert same_bits(inc["eta2"][wet], e2[0][wet]) and same_bits(inc["vel2"][wet], v2[0][wet]) and same_bits(inc["acc2"][wet], a2[0][wet])
        assert inc["vel2"][wet][:, 0].all() and not inc["vel2"][:, 1].any() and not inc["acc2"][:, 1].any()
        dry = ~wet
        assert dry.any() and not (inc["eta2"][dry].any() or inc["vel2"][dry].any() or inc["acc2"][dry].any())
    # a repeat leaves the bits
    assert same_bits(h.compute_morison(t, *st).reshape(-1, 6), got)
    h.close()


def test_increments_inside_the_ramp_and_under_a_regular_wave(HF):
    name = "nf3_40m"
    h = context(HF, name)
    st = mi.state(name)
    for t in (-1.0, 7.3):  # before and inside the ramp of 20 s
        h.compute_morison(t, *st)
        inc = h.morison_member_increments(0)
        e2, _, _ = h.wave_kinematics2(inc["node_p"], [t], mwl=mi.MWL)
        assert same_bits(inc["node_eta2"], e2[0]) and bool(inc["node_eta2"].any()) == (t > 0.0)
    h.close()
    # a regular wave carries the regular phase of the Morison options
    h = HF.from_case(m2i.shallow_case())
    h.add_waves_regular(0.5, 0.8)
    h.set_morison_members(0, *mi.body0())
    h.set_morison_options(mwl=0.2, regular_phase=0.9)
    h.set_morison_second_order(True)
    h.set_morison_members_second_order(True)
    h.compute_morison(5.0, *m2i.moving_state(1, -1.0, 5.0))
    inc = h.morison_member_increments(0)
    e2, _, _ = h.wave_kinematics2(inc["node_p"], [5.0], mwl=0.2, regular_phase=0.9)
    assert same_bits(inc["node_eta2"], e2[0]) and inc["node_eta2"].all()
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: the waterline moves
# ------------------------------------------------------------------------------------------------
def test_a_node_between_eta1_and_eta1_plus_eta2_is_wet_with_the_switch_on(HF):
    name = "nf3_40m"
    s = mi.SETS[name]
    case = s["case"]()
    h = HF.from_case(case)
    h.add_waves_irregular(**s["waves"])
    comp = mi.components(h, name, False)
    _, g, depth = h.simulation_parameters()
    rd = s["waves"]["ramp_duration"]
    lists, st, j = mi.flip_inputs(comp, abs(g), depth, rd)
    ref = m2.members2(comp, abs(g), depth, case["rho"], lists, mi.FLIP_T, *st, mwl=mi.MWL, ramp_duration=rd)
    first = mm.members(comp, depth, case["rho"], lists, mi.FLIP_T, *st, mwl=mi.MWL)
    assert ref["node_h1"][0][j] > ref["eta_bound"] and ref["node_h"][0][j] < -ref["eta_bound"]  # dry at order 1, wet at order 2
    mi.check_conditions(ref, "flip", need=("wet",))
    mi.check_conditions(first, "flip at order 1", need=("cut0",))
    set_members(h, lists)
    h.set_morison_options(mwl=mi.MWL, wave_stretching=False)
    one = h.compute_morison(mi.FLIP_T, *st).reshape(3, 6)
    h.set_morison_second_order(True)
    h.set_morison_members_second_order(True)
    two = h.compute_morison(mi.FLIP_T, *st).reshape(3, 6)
    assert np.all(np.abs(one - first["F"]) <= first["bound"]) and np.all(np.abs(two - ref["F"]) <= ref["bound"])
    print("flip: F_x order 1", one[0, 0], "order 2", two[0, 0], "bound", ref["bound"][0, 0])
    assert np.all(np.abs(two[0] - one[0])[[0, 4]] > (ref["bound"][0] + first["bound"][0])[[0, 4]])
    # the top segment is whole at order 2: its upper Gauss point lies above the cut of order 1, and carries increments
    inc = h.morison_member_increments(0)
    assert inc["eta2"].shape == (4,) and inc["eta2"].all() and np.allclose(inc["p"], ref["p"][0], rtol=0, atol=P_TOL)
    assert inc["node_eta2"][j] > 0.0
    h.close()


def test_bichromatic_set_down_changes_the_horizontal_force_on_a_column(HF):
    """Two components 0.02 Hz apart, the difference band alone: eta2 at the column is the set-down of the group.  Its sign, and the
    sign of the change of F_x, are taken from the restatement; the GPU has to show both and a change above the bound."""
    case = mi.finite_case()
    h = HF.from_case(case)
    h.add_waves_irregular(**mi.BICHROMATIC)
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == 2
    _, g, depth = h.simulation_parameters()
    assert depth == case["water_depth"]
    t = mi.BICHROMATIC_T
    lists, st = mi.bichromatic_inputs()
    # the conditions of the inputs (tests/test_morison_members2_ref_cpu.py holds them on the CPU oracle's spectrum), here on the context's
    ref, first, expected = mi.bichromatic_reference(comp, abs(g), case)
    set_members(h, lists)
    h.set_morison_options(mwl=0.0, wave_stretching=False)
    one = h.compute_morison(t, *st)[:6]
    h.set_morison_second_order(True, **mi.BICHROMATIC_BANDS)
    h.set_morison_members_second_order(True)
    two = h.compute_morison(t, *st)[:6]
    inc = h.morison_member_increments(0)
    print("bichromatic: set-down", inc["node_eta2"][0], "F_x", one[0], "->", two[0])
    assert np.all(np.sign(inc["node_eta2"]) == expected)
    want = ref["F"][0, 0] - first["F"][0, 0]
    assert abs((two[0] - one[0]) - want) <= ref["bound"][0, 0] + first["bound"][0, 0] and np.sign(two[0] - one[0]) == np.sign(want)
    h.close()


# ------------------------------------------------------------------------------------------------
# 4: bits that must not move
# ------------------------------------------------------------------------------------------------
def test_switch_off_empty_bands_and_bodies_without_members_keep_their_bits(HF):
    from hydrochrono_amd import capi
    name = "nf3_40m"
    s, st = mi.SETS[name], mi.state(name)
    t = s["t"]
    # the switch at 0: today's refusal (tests/test_gpu_morison_members.py asserts it and its message); the getters refuse
    h = context(HF, name, switch=False)
    assert h.morison_members_second_order() is False
    with pytest.raises(Exception):
        h.compute_morison(t, *st)
    assert b"hc_set_morison_members_second_order" in h.lib.hc_last_error(h.ctx)
    with pytest.raises(Exception):
        h.morison_member_increments(0)
    # second order on with empty bands: the member bits of order 1, and no increments to answer with
    h.set_morison_second_order(False)
    first = h.compute_morison(t, *st)
    rows1 = h.morison_member_forces(0)
    h.set_morison_second_order(True, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
    h.set_morison_members_second_order(True)
    assert same_bits(h.compute_morison(t, *st), first) and same_bits(h.morison_member_forces(0), rows1) and first.any()
    assert h.lib.hc_get_morison_member_node_increments(h.ctx, 0, None, None) == capi.HC_ERR_INVALID
    # the switch has no effect while second order is off
    h.set_morison_second_order(False)
    assert same_bits(h.compute_morison(t, *st), first) and h.morison_members_second_order() is True
    # no components at all: order 1 as well
    h.set_morison_second_order(True)
    h.add_waves_none()
    still = h.compute_morison(t, *st)
    h.set_morison_second_order(False)
    assert same_bits(h.compute_morison(t, *st), still) and still.any()
    h.close()


def test_elements_plus_members_is_the_ieee_sum_and_other_bodies_keep_their_bits(HF):
    name = "nf3_40m"
    s, st = mi.SETS[name], mi.state(name)
    t = s["t"]
    both, el_only, mem_only = context(HF, name, elements=ELEMENTS), context(HF, name, members=False, elements=ELEMENTS), context(HF, name)
    a, e, m = (h.compute_morison(t, *st) for h in (both, el_only, mem_only))
    assert e[6:].any() and m[:6].any() and m[12:].any() and not e[:6].any() and not m[6:12].any()
    assert same_bits(a[:6], m[:6])           # members alone: elements (zeros) + members
    assert same_bits(a[6:12], e[6:12])       # a body without members: the order-2 element bits it had
    assert same_bits(a[12:], e[12:] + m[12:])  # one IEEE addition per component
    for b in (0, 2):
        x, y = both.morison_member_increments(b), mem_only.morison_member_increments(b)
        assert all(same_bits(x[k], y[k]) for k in x)
        assert same_bits(both.morison_member_forces(b), mem_only.morison_member_forces(b))
    assert all(same_bits(both.morison_increments(1)[k], el_only.morison_increments(1)[k]) for k in ("p", "eta2", "vel2", "acc2"))
    # another body's list replaced and cleared: body 2 keeps its bits
    both.set_morison_members(0, *mi.body2(False))
    c = both.compute_morison(t, *st)
    assert same_bits(c[6:], a[6:]) and not same_bits(c[:6], a[:6])
    both.set_morison_members(0, np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 1.0, 1.0, 1)
    c = both.compute_morison(t, *st)
    assert same_bits(c[6:], a[6:]) and not c[:6].any()
    both.set_morison_members(0, *mi.body0())
    assert same_bits(both.compute_morison(t, *st), a)
    for h in (both, el_only, mem_only):
        h.close()


def test_shards_and_the_number_of_bodies_leave_the_bits(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.synthetic import many_body_case
    name = "nf257_deep"
    s, st = mi.SETS[name], mi.state(name)
    t = s["t"]
    whole = context(HF, name, elements=ELEMENTS)
    group = context(HF, name, elements=ELEMENTS, make=lambda case: HydroGroup.from_case(case, 3))
    assert group.morison_members_second_order() is True
    ref = whole.compute_morison(t, *st)
    assert same_bits(group.compute_morison(t, *st), ref) and ref.reshape(3, 6).any(axis=1).all()
    for b in (0, 2):
        x, y = whole.morison_member_increments(b), group.morison_member_increments(b)
        assert all(same_bits(x[k], y[k]) for k in x) and x["eta2"].size
    with pytest.raises(Exception):
        group.morison_member_increments(3)
    whole.close()
    group.close()
    # the same body data as the only body of a 1-body context and as body 2 of a 3-body one
    one, three = (HF.from_case(many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)) for N in (1, 3))
    one.set_morison_members(0, *mi.body0())
    three.set_morison_members(2, *mi.body0())
    three.set_morison_members(0, *mi.body2(False))
    for h in (one, three):
        h.add_waves_irregular(**THREE8)
        h.set_morison_options(mwl=0.2)
        h.set_morison_second_order(True)
        h.set_morison_members_second_order(True)
    st1 = m2i.moving_state(1, -1.0, 33.0, seed=5)
    st3 = [np.concatenate([x, x, x]) for x in st1]
    for x in st3:
        x[:2] += 0.37  # the other bodies move differently
    a, b = one.compute_morison(33.0, *st1), three.compute_morison(33.0, *st3)
    assert a.any() and same_bits(a, b[12:])
    i1, i3 = one.morison_member_increments(0), three.morison_member_increments(2)
    assert all(same_bits(i1[k], i3[k]) for k in i1)
    one.close()
    three.close()


# ------------------------------------------------------------------------------------------------
# 5: protocol and errors
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 32])
def test_members_at_order_two_around_every_step_change_no_force(HF, lookahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_morison in (False, True):
        h = HF.from_case(case)
        h.set_lookahead(lookahead)
        h.add_waves_irregular(**wi.sphere_waves(65))
        if with_morison:
            h.set_morison_members(0, *mi.body0())
            h.set_morison_second_order(True)
            h.set_morison_members_second_order(True)
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        rows = []
        for n in range(100):  # three look-ahead blocks of 32 steps
            t = SPHERE_DT * n
            st = motion.state(t)
            if with_morison:
                h.morison_begin(t, *st)
            total = raw_step(h, t, st)
            if with_morison:
                assert h.morison_end().any() or n == 0
            rows.append(np.concatenate([total, *h.components()]))
        if with_morison:
            assert h.morison_member_increments(0)["node_eta2"].any()
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


def test_errors_and_protocol(HF):
    from hydrochrono_amd import capi
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    name = "nf3_40m"
    h = context(HF, name, switch=False, second=False)
    lib = h.lib
    z9, lin, out = np.zeros(9), np.tile([0.5, 0.0, 0.0], 3), np.empty(18)
    pos = np.tile([0.0, 0.0, -1.0], 3)
    nodes = np.empty(3 * 80)

    def node_inc(body=0, ctx=None):
        return lib.hc_get_morison_member_node_increments(ctx or h.ctx, body, dp(nodes), None)

    def point_inc(body=0):
        return lib.hc_get_morison_member_point_increments(h.ctx, body, None, None, None, None)

    def evaluate():
        assert lib.hc_morison_end(h.ctx, dp(out)) == INV  # nothing is pending
        return lib.hc_compute_morison(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(out))

    # the switch is off: the getters refuse, whatever has been evaluated
    assert evaluate() == OK and node_inc() == INV and point_inc() == INV
    assert lib.hc_set_morison_members_second_order(h.ctx, 1) == OK
    # on, but no evaluation with a second-order member part has completed (second order itself is off)
    assert evaluate() == OK and node_inc() == INV and point_inc() == INV
    h.set_morison_second_order(True)
    assert node_inc() == INV
    assert evaluate() == OK and node_inc() == OK and point_inc() == OK
    # members and no element: the elements' getter has nothing to answer with, as before
    assert lib.hc_get_morison_increments(h.ctx, 0, None, None, None, None) == INV
    n_nodes, n_points = capi.C.c_int(), capi.C.c_int()
    assert lib.hc_get_morison_member_increment_counts(h.ctx, 2, capi.C.byref(n_nodes), capi.C.byref(n_points)) == OK
    assert (n_nodes.value, n_points.value) == (3 + 3 + 2 + 65, 2 * (2 + 2 + 1 + 64))
    assert lib.hc_get_morison_member_increment_counts(h.ctx, 3, None, None) == INV
    for body in (-1, 3, 100):
        assert node_inc(body) == INV and point_inc(body) == INV
    assert node_inc(1) == OK  # an owned body without members: nothing to copy
    # an evaluation without a second-order member part leaves the last one with such a part in place
    h.set_morison_second_order(True, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
    assert evaluate() == OK and node_inc() == OK
    h.set_morison_second_order(True)
    # a member list changes: forgotten, whichever body it was
    h.set_morison_members(2, *mi.body2(False))
    assert node_inc() == INV and point_inc(2) == INV
    assert evaluate() == OK and node_inc() == OK and point_inc(2) == OK
    # the switch off and on again: forgotten
    assert lib.hc_set_morison_members_second_order(h.ctx, 0) == OK and lib.hc_set_morison_members_second_order(h.ctx, 1) == OK
    assert node_inc() == INV
    assert evaluate() == OK and node_inc() == OK
    # the three switches are independent
    h.set_morison_second_order(False)
    h.set_morison_second_order_directional(True)
    assert h.morison_members_second_order() is True
    h.set_morison_members_second_order(False)
    assert h.morison_second_order_directional() is True and h.morison_second_order()["on"] is False
    h.set_morison_second_order(True)
    h.set_morison_second_order_directional(False)
    assert h.morison_members_second_order() is False
    # ... and a refused begin leaves nothing pending, whatever was toggled before it
    assert evaluate() == UNS and b"member" in lib.hc_last_error(h.ctx)
    assert lib.hc_morison_end(h.ctx, dp(out)) == INV
    h.set_morison_members_second_order(True)
    assert evaluate() == OK
    # a setter while a begin is pending
    assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == OK
    assert lib.hc_set_morison_members_second_order(h.ctx, 0) == INV
    assert lib.hc_morison_end(h.ctx, dp(out)) == OK and h.morison_members_second_order() is True
    # a shard context answers for its own bodies only
    sh = context(HF, name, make=lambda case: HF.from_case(case, body_range=(2, 3)))
    o6 = np.empty(6)
    assert lib.hc_compute_morison(sh.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9), dp(o6)) == OK and o6.any()
    assert node_inc(2, sh.ctx) == OK and node_inc(0, sh.ctx) == INV and node_inc(1, sh.ctx) == INV
    sh.close()
    # more than 4096 components: refused by hc_morison_begin, nothing pending; fine again once the sea is smaller
    h.add_waves_irregular(**wi.three_waves(4097))
    assert lib.hc_morison_begin(h.ctx, 30.0, dp(pos), dp(z9), dp(lin), dp(z9)) == UNS and b"4096" in lib.hc_last_error(h.ctx)
    assert lib.hc_morison_end(h.ctx, dp(out)) == INV
    h.add_waves_irregular(**mi.SETS[name]["waves"])
    assert evaluate() == OK and node_inc() == OK
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: the layers above
# ------------------------------------------------------------------------------------------------
def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    name = "nf3_40m"
    case = mi.SETS[name]["case"]()
    a, b = context(HF, name, elements=ELEMENTS), context(HF, name, elements=ELEMENTS)
    first = context(HF, name, elements=ELEMENTS, second=False)
    grp = context(HF, name, elements=ELEMENTS, make=lambda c: HydroGroup.from_case(c, 3))
    gplain = HydroGroup.from_case(case, 3)
    gplain.add_waves_irregular(**mi.SETS[name]["waves"])
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
    x, y = grp.morison_member_increments(2), b.morison_member_increments(2)
    assert all(same_bits(x[k], y[k]) for k in x) and x["node_eta2"].size == 3 + 3 + 2 + 65
    for h in (a, b, first, grp, gplain):
        h.close()


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "morison_members2_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison_members2_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (40, 25 + 18 + 16)
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(**dict(wi.sphere_waves(65), simulation_dt=0.015))
    h.set_morison_elements(0, [[2.5, 0.5, -3.0]], [[1, 1.5, 0.5]], [[2, 2, 1.0]])
    h.set_morison_members(0, [[0, 0, -5.0], [-3, -3, -4.0], [1, 0, 8.0]], [[0, 0, 6.0], [3, 3, 1.5], [4, 0, 9.0]],
                          [[1.2, 1.2], [0.8, 0.4], [0.5, 0.5]], [1.0, 0.9, 1.0], [2.0, 1.6, 2.0], [8, 5, 1])
    h.set_morison_options(mwl=0.25)
    h.set_morison_second_order(True, diff_band=(0.05, 0.9), sum_band=(1.5, 6.0))
    h.set_morison_members_second_order(True)
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total, mor = raw_step(h, t, st), h.compute_morison(t, *st)
        assert same_bits(row[19:25], mor) and same_bits(row[13:19], total + mor), t
        assert same_bits(row[25:43].reshape(3, 6), h.morison_member_forces(0)), t
        assert same_bits(row[43:59], h.morison_member_increments(0)["node_eta2"][:16]), t
    assert np.abs(rows[:, 25:28]).max() > 1.0 and not rows[:, 37:43].any() and np.abs(rows[:, 43:59]).max() > 1e-5
    h.close()
