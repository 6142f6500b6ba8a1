"""Morison strip members on the second-order sea in a short-crested sea on the GPU (hc_set_morison_members_second_order with
hc_set_morison_second_order_directional under hc_set_wave_directions; csrc/hc_morison_members.hip: the <true> instantiations) against
tests/morison_members2_ref.py on five-entry components, on the inputs of tests/morison_members2_inputs.py with the spread directions
of tests/wave2_dir_inputs.py.  Tolerance and conditions as tests/test_gpu_morison_members2.py."""
import numpy as np
import pytest

import morison_members2_inputs as mi
import morison_members2_ref as m2
import morison_members_ref as mm
import wave2_inputs as wi

pytestmark = pytest.mark.gpu
P_TOL = 16 * 64 * 2.0 ** -52  # the rounding allowance of tests/test_gpu_morison2.py for a stored point


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def context(HF, name, lists=None, make=None, bands=None, dir_switch=True, switch=True):
    s = mi.SETS[name]
    case = s["case"]()
    h = (make or HF.from_case)(case)
    mi.spread_sea(h, case, s["waves"])
    h.set_wave_directions(mi.directions(name))
    for b, ml in enumerate(s["lists"]() if lists is None else lists):
        if ml is not None:
            h.set_morison_members(b, *ml)
    h.set_morison_options(mwl=mi.MWL, wave_stretching=s["stretching"])
    d, sm = bands or (s["diff_band"], s["sum_band"])
    h.set_morison_second_order(True, diff_band=d, sum_band=sm)
    h.set_morison_second_order_directional(dir_switch)
    h.set_morison_members_second_order(switch)
    return h


@pytest.mark.parametrize("name", sorted(mi.SETS))
def test_parity_inside_the_derived_bound_and_increments_bit_for_bit(HF, name):
    s = mi.SETS[name]
    h = context(HF, name)
    comp = mi.components(h, name, True)
    assert len(comp) == 5 and comp[0].size == s["waves"]["nfrequencies"]
    _, g, _ = h.simulation_parameters()
    ref = mi.reference(name, comp, abs(g))
    mi.check_conditions(ref, name)
    t, st = s["t"], mi.state(name)
    got = h.compute_morison(t, *st).reshape(-1, 6)
    err = np.abs(got - ref["F"])
    worst = float(np.max(err / np.maximum(ref["bound"], 1e-300)))
    print(f"{name} directional: worst |gpu - ref| / bound = {worst:.3e} per body, max |F| = {np.max(np.abs(ref['F'])):.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= ref["bound"]), f"{name}: worst {worst:.3e} of the bound"
    assert not got[1].any()
    for b in (0, 2):
        rows = h.morison_member_forces(b)
        e = np.abs(rows - ref["members"][b])
        w = float(np.max(e / np.maximum(ref["member_bound"][b], 1e-300)))
        print(f"{name} directional body {b}: worst member row |gpu - ref| / bound = {w:.3e}")
        assert np.all(e <= ref["member_bound"][b]), (name, b, w)
        acc = np.zeros(6)
        for r in rows:
            acc = acc + r
        assert same_bits(acc, got[b])
        inc = h.morison_member_increments(b)
        wet = ref["wet"][b]
        assert np.allclose(inc["node_p"], ref["node_p"][b], rtol=0, atol=P_TOL) and np.allclose(inc["p"][wet], ref["p"][b][wet], rtol=0, atol=P_TOL)
        kw = dict(mwl=mi.MWL, diff_band=s["diff_band"], sum_band=s["sum_band"], directional=True)
        e2, _, _ = h.wave_kinematics2(inc["node_p"], [t], **kw)
        assert same_bits(inc["node_eta2"], e2[0]) and inc["node_eta2"].all(), (name, b)
        e2, v2, a2 = h.wave_kinematics2(inc["p"], [t], **kw)
        assert same_bits(inc["eta2"][wet], e2[0][wet]) and same_bits(inc["vel2"][wet], v2[0][wet]) and same_bits(inc["acc2"][wet], a2[0][wet])
        assert inc["vel2"][wet][:, 1].all() and inc["acc2"][wet][:, 1].all()  # the y components are present
        dry = ~wet
        assert dry.any() and not (inc["eta2"][dry].any() or inc["vel2"][dry].any() or inc["acc2"][dry].any())
    assert same_bits(h.compute_morison(t, *st).reshape(-1, 6), got)
    h.close()


def test_a_node_between_eta1_and_eta1_plus_eta2_is_wet_with_the_switch_on(HF):
    name = "nf3_40m"
    s = mi.SETS[name]
    case = s["case"]()
    probe = context(HF, name)
    comp = mi.components(probe, name, True)
    _, g, depth = probe.simulation_parameters()
    probe.close()
    rd = s["waves"]["ramp_duration"]
    lists, st, j = mi.flip_inputs(comp, abs(g), depth, rd)
    ref = m2.members2(comp, abs(g), depth, case["rho"], lists, mi.FLIP_T, *st, mwl=mi.MWL, ramp_duration=rd)
    first = mm.members(comp, depth, case["rho"], lists, mi.FLIP_T, *st, mwl=mi.MWL)
    assert ref["node_h1"][0][j] > ref["eta_bound"] and ref["node_h"][0][j] < -ref["eta_bound"]  # dry at order 1, wet at order 2
    mi.check_conditions(ref, "flip", need=("wet",))
    mi.check_conditions(first, "flip at order 1", need=("cut0",))
    h = context(HF, name, lists=lists, bands=(mi.FULL, mi.FULL))
    h.set_morison_options(mwl=mi.MWL, wave_stretching=False)
    two = h.compute_morison(mi.FLIP_T, *st).reshape(3, 6)
    h.set_morison_second_order(False)
    one = h.compute_morison(mi.FLIP_T, *st).reshape(3, 6)
    assert np.all(np.abs(one - first["F"]) <= first["bound"]) and np.all(np.abs(two - ref["F"]) <= ref["bound"])
    assert np.all(np.abs(two[0] - one[0])[[0, 4]] > (ref["bound"][0] + first["bound"][0])[[0, 4]])
    h.close()


def test_refusals_empty_bands_and_shards(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroGroup
    name = "nf3_40m"
    s, st = mi.SETS[name], mi.state(name)
    t = s["t"]
    # directions without the directional switch: refused first, whatever the members' switch says
    h = context(HF, name, dir_switch=False)
    with pytest.raises(Exception):
        h.compute_morison(t, *st)
    assert b"hc_set_morison_second_order_directional" in h.lib.hc_last_error(h.ctx)
    assert h.lib.hc_morison_end(h.ctx, None) == capi.HC_ERR_INVALID  # nothing is pending
    # both directional switches, the members' switch off: today's refusal
    h.set_morison_second_order_directional(True)
    h.set_morison_members_second_order(False)
    with pytest.raises(Exception):
        h.compute_morison(t, *st)
    assert b"member" in h.lib.hc_last_error(h.ctx)
    h.set_morison_members_second_order(True)
    full = h.compute_morison(t, *st)
    # empty bands: the directional member bits of order 1
    h.set_morison_second_order(True, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR)
    empty = h.compute_morison(t, *st)
    h.set_morison_second_order(False)
    first = h.compute_morison(t, *st)
    assert same_bits(empty, first) and not same_bits(full, first) and first.any()
    h.close()
    # three shards: the same bits, the owning shard answers the getters
    whole, group = context(HF, name), context(HF, name, make=lambda case: HydroGroup.from_case(case, 3))
    assert same_bits(group.compute_morison(t, *st), whole.compute_morison(t, *st))
    assert same_bits(whole.compute_morison(t, *st), full)
    for b in (0, 2):
        x, y = whole.morison_member_increments(b), group.morison_member_increments(b)
        assert all(same_bits(x[k], y[k]) for k in x) and x["vel2"][:, 1].any()
    whole.close()
    group.close()
