"""Morison strip members on the GPU (hc_set_morison_members, hc_get_morison_member_forces; csrc/hc_morison_members.hip) against the
tests' NumPy restatement of the definition (tests/morison_members_ref.py), fed the context's own spectrum / regular-wave coefficients.

Tolerance: the bound morison_members_ref returns per body and component (derived in its docstring: the 1e-11 sum|term| of the
kinematics through |q_n| q_n and a_n, a cut segment's sensitivity to its cut, (items + 64) 2^-52 of the uncancelled magnitudes).  The
wet test of a node is a discontinuity of the case a segment takes: every comparison first asserts, on the reference side, that every
node's |h_j| exceeds the reference's own bound of its eta error, so GPU and restatement take the same case everywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import directional_ref as dr
import morison_members_ref as mm
import morison_ref as mr
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=60.0, ramp_duration=10.0, wave_height=2.0, wave_period=9.0,
             frequency_min=0.03, frequency_max=0.9, nfrequencies=257, seed=3)
THREE_IRREG = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
                   frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)
REG_AMP, REG_OMEGA = 0.177, 2.094395102


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def frame_members(n_col=64):
    """Every case of a segment on a body whose reference sits about 2 m under the surface: a column cut with r0 wet, a column given
    top down (r1 wet), a tapered brace of one segment, a deep brace wholly wet, a member wholly dry, one of zero diameter"""
    r0 = [[0.0, 0.0, -6.0], [1.0, 1.0, 6.5], [-4.0, -3.0, -5.0], [-5.0, 0.5, -8.0], [-2.0, 2.0, 8.0], [2.0, -1.0, -4.0]]
    r1 = [[0.0, 0.0, 7.0], [1.0, 1.0, -7.0], [4.0, 3.0, 5.5], [5.0, 0.5, -8.5], [2.0, 2.0, 9.0], [2.5, -1.0, 6.0]]
    dia = [[1.2, 1.2], [0.7, 0.7], [0.9, 0.3], [0.5, 0.6], [0.4, 0.4], [0.0, 0.0]]
    return mm.member_lists(r0, r1, dia, [1.0, 0.8, 1.1, 0.0, 1.0, 1.0], [2.0, 1.5, 0.0, 1.8, 2.0, 2.0], [n_col, 2, 1, 3, 2, 4])


def long_members(seed=1):
    """5 members of 64 segments: 325 nodes and 640 Gauss points of one body, both across a workgroup edge"""
    rng = np.random.default_rng(seed)
    r0 = rng.uniform(-5, 5, (5, 3))
    r0[:, 2] = rng.uniform(-9.0, -5.0, 5)
    r1 = r0 + rng.uniform(-4, 4, (5, 3))
    r1[:, 2] = rng.uniform(4.5, 8.0, 5)
    return mm.member_lists(r0, r1, rng.uniform(0.2, 1.5, (5, 2)), rng.uniform(0.5, 1.2, 5), rng.uniform(0.0, 2.0, 5), 64)


def random_elements(n, seed, spread=6.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, (n, 3)), rng.uniform(0.0, 3.0, (n, 3)), rng.uniform(0.0, 4.0, (n, 3))


def moving_state(N, rest_z, t, seed=3):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((N, 3))
    rest[:, 0] = 15.0 * np.arange(N)
    rest[:, 2] = rest_z
    return PrescribedMotion(N, rest, seed=seed, amplitude=0.5).state(t)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def set_all(h, lists):
    for b, ml in enumerate(lists):
        if ml is not None:
            h.set_morison_members(b, *ml)


def serial_sum(rows):
    acc = np.zeros(6)
    for r in rows:
        acc = acc + r
    return acc


def compare(h, case, lists, comp, t, state, what, mwl=0.0, stretching=False, ramp=1.0, need=()):
    """GPU against the restatement, inside the derived bound, the body vectors and every member's row (`member_bound`: the same three
    parts over that member's points alone); asserts the node margin first.  Returns the GPU result and the reference."""
    ref = mm.members(comp, case["water_depth"], case["rho"], lists, t, *state, mwl=mwl, stretching=stretching, ramp=ramp)
    assert ref["clear"] and ref["margin"] > ref["eta_bound"], \
        f"{what}: a node is {ref['margin']:.3e} m from the free surface, the eta bound is {ref['eta_bound']:.3e} m (choose other inputs)"
    got = h.compute_morison(t, *state).reshape(-1, 6)
    assert got.shape == ref["F"].shape and np.all(np.isfinite(got)), what
    err = np.abs(got - ref["F"])
    worst = float(np.max(err / np.maximum(ref["bound"], 1e-300)))
    print(f"{what}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(ref['F'])):.3e}, margin {ref['margin']:.2e} m, "
          f"largest bound / |F| = {np.max(ref['bound'] / np.maximum(np.abs(ref['F']), 1e-300)):.2e}")
    assert np.all(err <= ref["bound"]), f"{what}: worst {worst:.3e} of the bound"
    for b, ml in enumerate(lists):
        if ml is not None and h.b0 <= b < h.b1:
            rows = h.morison_member_forces(b)
            assert rows.shape == ref["members"][b].shape
            merr = np.abs(rows - ref["members"][b])
            mworst = float(np.max(merr / np.maximum(ref["member_bound"][b], 1e-300))) if rows.size else 0.0
            print(f"{what}: body {b}: worst |member row - ref| / member bound = {mworst:.3e}")
            assert np.all(merr <= ref["member_bound"][b]), f"{what}: body {b}'s member rows: worst {mworst:.3e} of the member bound"
            assert same_bits(serial_sum(rows), got[b - h.b0]), f"{what}: the serial sum of body {b}'s member rows is not the body vector"
    for c in need:
        assert any(c in s for s in ref["cases"]), (what, c, ref["cases"])
    return got, ref


def raw_step(h, t, state):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def spread_sea(h, case, **kw):
    """the spectral model with excitation tables on a heading grid for every body: what non-uniform directions need"""
    for b, bd in enumerate(case["bodies"]):
        mag, ph = (np.stack([np.asarray(bd[key]).reshape(6, -1)] * 2, axis=1) for key in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-2.0, 2.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, **dict(IRREG, **kw))


ALL_CASES = ("wet", "dry", "cut0", "cut1")


# ------------------------------------------------------------------------------------------------
# 1: against the restatement
# ------------------------------------------------------------------------------------------------
def test_regular_wave_every_segment_case(HF):
    """one component; n_seg 1, 2 and 64; finite depth; mwl; a regular wave is neither ramped nor stretched"""
    case = sphere_case()
    h = HF.from_case(case)
    h.add_waves_regular(REG_AMP * 4, 0.9)
    lists = [frame_members()]
    set_all(h, lists)
    assert h.morison_member_count(0) == 6
    comp = wk.regular_components(REG_AMP * 4, 0.9, h.regular_coeffs()[2], 0.7)
    for mwl in (0.0, 0.6):
        for stretching in (True, False):
            h.set_morison_options(mwl=mwl, regular_phase=0.7, wave_stretching=stretching)
            for t in (0.0, 3.7):
                got, _ = compare(h, case, lists, comp, t, moving_state(1, -2.0, t), f"regular mwl={mwl} t={t}", mwl=mwl, need=ALL_CASES)
                assert np.max(np.abs(got)) > 100.0
    rows = h.morison_member_forces(0)
    assert not rows[4].any() and not rows[5].any() and rows[:4].any(axis=1).all()  # the dry member and the one of zero diameter


@pytest.mark.parametrize("nf", [255, 256, 257, 300])
def test_spectral_sea_at_the_component_tile_edge(HF, nf):
    """finite depth, stretching on and off, mwl, before, inside and after the ramp; one body of 325 nodes and 640 Gauss points"""
    case = sphere_case()
    h = HF.from_case(case)
    h.add_waves_irregular(spectral=True, **dict(IRREG, nfrequencies=nf))
    comp = wk.irregular_components(h.irreg_spectrum())
    assert len(comp[0]) == nf
    lists = [long_members(nf)]
    set_all(h, lists)
    results = {}
    for mwl, stretching in ((0.0, True), (0.4, False), (0.4, True)):
        h.set_morison_options(mwl=mwl, wave_stretching=stretching)
        for t in (-1.0, 4.0, 33.3):
            got, _ = compare(h, case, lists, comp, t, moving_state(1, -2.0, t), f"spectral nf={nf} mwl={mwl} stretching={stretching} t={t}",
                             mwl=mwl, stretching=stretching, ramp=mr.ramp_factor(t, 10.0), need=("wet", "dry", "cut0"))
            results[(mwl, stretching, t)] = got
    assert not np.array_equal(results[(0.4, True, 33.3)], results[(0.4, False, 33.3)])
    assert not np.array_equal(results[(0.0, True, 33.3)], results[(0.4, True, 33.3)])


def test_three_bodies_infinite_depth_irf_model_and_uniform_heading(HF):
    case = three_body_case()
    assert np.isinf(case["water_depth"])
    h = HF.from_case(case)
    h.add_waves_irregular(**THREE_IRREG)
    comp = wk.irregular_components(h.irreg_spectrum())
    lists = [frame_members(7), None, long_members(5)]
    set_all(h, lists)
    for stretching in (True, False):
        h.set_morison_options(mwl=0.25, wave_stretching=stretching)
        for t in (1.0, 12.5):
            got, _ = compare(h, case, lists, comp, t, moving_state(3, -2.0, t), f"three bodies, IRF model, stretching={stretching} t={t}", mwl=0.25,
                             stretching=stretching, ramp=mr.ramp_factor(t, 5.0), need=ALL_CASES)
            assert got[0].any() and not got[1].any() and got[2].any()
    th = h.set_wave_spreading(0.4, s=0.0)  # a uniform heading on the IRF model
    compare(h, case, lists, dr.with_directions(comp, th), 12.5, moving_state(3, -2.0, 12.5), "three bodies, IRF model, heading 0.4", mwl=0.25,
            stretching=False, need=ALL_CASES)


@pytest.mark.parametrize("N", [1, 3])
def test_spread_sea(HF, N):
    case = sphere_case() if N == 1 else three_body_case()
    h = HF.from_case(case)
    spread_sea(h, case)
    th = h.set_wave_spreading(0.3, s=10, n_bins=15, seed=2)
    assert np.ptp(th) > 0.5
    comp = dr.with_directions(wk.irregular_components(h.irreg_spectrum()), th)
    lists = [frame_members(64)] if N == 1 else [long_members(2), frame_members(3), None]
    set_all(h, lists)
    for stretching in (True, False):
        h.set_morison_options(mwl=-0.2, wave_stretching=stretching)
        t = 21.7
        got, _ = compare(h, case, lists, comp, t, moving_state(N, -2.0, t, seed=6), f"spread sea N={N} stretching={stretching}", mwl=-0.2,
                         stretching=stretching, need=ALL_CASES)
        assert np.abs(got[:, 1]).max() > 1.0  # a transverse force: the sea is short-crested


def test_regular_wave_under_a_heading(HF):
    case = sphere_case()
    h = HF.from_case(case)
    h.add_waves_regular(REG_AMP * 4, 0.9)
    h.set_wave_directions([0.7])
    lists = [frame_members(2)]
    set_all(h, lists)
    h.set_morison_options(regular_phase=0.4)
    comp = dr.with_directions(wk.regular_components(REG_AMP * 4, 0.9, h.regular_coeffs()[2], 0.4), 0.7)
    compare(h, case, lists, comp, 2.2, moving_state(1, -2.0, 2.2), "regular wave, heading 0.7", need=ALL_CASES)


def test_still_water_nowave_and_eta_record(HF):
    case = three_body_case()
    h = HF.from_case(case)
    lists = [None, frame_members(3), None]
    set_all(h, lists)
    pos, z = np.zeros((3, 3)), np.zeros((3, 3))
    pos[:, 2] = -1.0
    lin = np.tile([0.7, 0.0, 0.0], (3, 1))
    rec_t = 0.05 * np.arange(400)
    # the first column alone, upright, surging: draft 7 m of r0 = (0, 0, -6) on a body at z = -1
    f_col = -0.5 * case["rho"] * 1.0 * 1.2 * 0.7 * 0.7 * 7.0
    for model in ("none", "nowave", "eta_record"):
        if model == "nowave":
            h.add_waves_none()
        elif model == "eta_record":
            h.add_waves_irregular_eta(rec_t, 0.5 * np.sin(0.8 * rec_t), 0.05)
        got = h.compute_morison(3.0, pos, z, lin, z).reshape(3, 6)
        assert not got[0].any() and not got[2].any(), model
        assert np.isclose(h.morison_member_forces(1)[0, 0], f_col, rtol=1e-13), model
        compare(h, case, lists, None, 3.0, moving_state(3, -2.0, 3.0), f"still water ({model})", need=ALL_CASES)


# ------------------------------------------------------------------------------------------------
# 2: a heading with the body yawed by it
# ------------------------------------------------------------------------------------------------
def test_heading_and_yaw_rotate_the_force(HF):
    case = sphere_case()
    beta = 0.6
    cb, sb = np.cos(beta), np.sin(beta)
    Rz = np.array([[cb, -sb, 0.0], [sb, cb, 0.0], [0.0, 0.0, 1.0]])
    h = HF.from_case(case)
    h.add_waves_irregular(spectral=True, **dict(IRREG, nfrequencies=64))
    comp = wk.irregular_components(h.irreg_spectrum())
    lists = [frame_members(5)]
    set_all(h, lists)
    t = 14.0
    pos, lin, ang = np.array([1.5, 0.0, -2.1]), np.array([0.4, 0.0, -0.2]), np.array([0.0, 0.0, 0.05])
    f0, ref0 = compare(h, case, lists, comp, t, (pos, np.zeros(3), lin, ang), "long-crested", stretching=True)
    th = h.set_wave_spreading(beta, s=0.0)
    f1, ref1 = compare(h, case, lists, dr.with_directions(comp, th), t, (Rz @ pos, np.array([0.0, 0.0, beta]), Rz @ lin, Rz @ ang),
                       "heading and yaw", stretching=True)
    want = np.concatenate([Rz @ f0[0, :3], Rz @ f0[0, 3:]])
    b0, b1 = ref0["bound"][0], ref1["bound"][0]
    b3 = np.concatenate([np.full(3, np.linalg.norm(b0[:3])), np.full(3, np.linalg.norm(b0[3:]))]) + b1
    assert np.all(np.abs(f1[0] - want) <= b3) and np.linalg.norm(f0[0, :2]) > 100.0


# ------------------------------------------------------------------------------------------------
# 3: invariance, bitwise
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three(HF):
    """a three-body context with members and elements and its result for one state"""
    case = three_body_case()
    h = HF.from_case(case)
    h.add_waves_irregular(**THREE_IRREG)
    lists = [frame_members(9), long_members(3), frame_members(64)]
    elements = [random_elements(33, 20), None, random_elements(5, 22)]
    set_all(h, lists)
    for b, el in enumerate(elements):
        if el is not None:
            h.set_morison_elements(b, *el)
    h.set_morison_options(mwl=0.1)
    st = moving_state(3, -2.0, 12.5)
    return dict(case=case, h=h, lists=lists, elements=elements, st=st, t=12.5, ref=h.compute_morison(12.5, *st))


def test_repeats_leave_the_bits(three):
    assert three["ref"].reshape(3, 6).any(axis=1).all()
    for _ in range(3):
        assert same_bits(three["h"].compute_morison(three["t"], *three["st"]), three["ref"])


def test_compute_is_begin_step_end(three):
    h = three["h"]
    h.morison_begin(three["t"], *three["st"])
    raw_step(h, three["t"], three["st"])
    assert same_bits(h.morison_end(), three["ref"])


def test_shards_leave_the_bits(three):
    from hydrochrono_amd.hydro import HydroGroup
    group = HydroGroup.from_case(three["case"], 3)
    group.add_waves_irregular(**THREE_IRREG)
    for b in range(3):
        group.set_morison_members(b, *three["lists"][b])
        if three["elements"][b] is not None:
            group.set_morison_elements(b, *three["elements"][b])
    group.set_morison_options(mwl=0.1)
    assert same_bits(group.compute_morison(three["t"], *three["st"]), three["ref"])
    for b in range(3):
        assert group.morison_member_count(b) == len(three["lists"][b][0])
        assert same_bits(group.morison_member_forces(b), three["h"].morison_member_forces(b))


def test_other_bodies_lists_of_either_kind_leave_the_bits(three):
    h, ref, t, st = three["h"], three["ref"], three["t"], three["st"]
    h.set_morison_members(1, *frame_members(64))
    a = h.compute_morison(t, *st)
    assert same_bits(a[:6], ref[:6])
    assert same_bits(a[12:], ref[12:])
    assert not same_bits(a[6:12], ref[6:12])
    h.set_morison_members(1, np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 1.0, 1.0, 1)  # cleared
    h.set_morison_elements(1, *random_elements(300, 23))
    a = h.compute_morison(t, *st)
    assert h.morison_member_count(1) == 0
    assert same_bits(a[:6], ref[:6])
    assert same_bits(a[12:], ref[12:])
    h.set_morison_elements(1, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    h.set_morison_members(1, *three["lists"][1])
    assert same_bits(h.compute_morison(t, *st), ref)  # ... and back


def test_number_of_bodies_leaves_the_bits(HF, three):
    """body 2's data as the only body of a one-body context: the same state, lists, wave model, rho and depth"""
    from hydrochrono_amd.synthetic import many_body_case
    kw = dict(S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)
    one, tri = HF.from_case(many_body_case(1, **kw)), HF.from_case(many_body_case(3, **kw))
    ml, el = three["lists"][2], three["elements"][2]
    one.set_morison_members(0, *ml)
    one.set_morison_elements(0, *el)
    tri.set_morison_members(2, *ml)
    tri.set_morison_elements(2, *el)
    tri.set_morison_members(0, *long_members(9))
    for h in (one, tri):
        h.add_waves_irregular(spectral=True, **IRREG)
        h.set_morison_options(mwl=0.2)
    st1 = moving_state(1, -2.0, 33.0, seed=5)
    st3 = [np.concatenate([x, x, x]) for x in st1]
    for x in st3:
        x[:2] += 0.37  # the other bodies move differently
    a, b = one.compute_morison(33.0, *st1), tri.compute_morison(33.0, *st3)
    assert a.any()
    assert same_bits(a, b[12:])
    assert same_bits(one.morison_member_forces(0), tri.morison_member_forces(2))


def test_element_only_body_keeps_its_bits_and_the_sum_is_one_addition(HF, three):
    case, t, st = three["case"], three["t"], three["st"]
    only_el, only_mem = HF.from_case(case), HF.from_case(case)
    for h in (only_el, only_mem):
        h.add_waves_irregular(**THREE_IRREG)
        h.set_morison_options(mwl=0.1)
    for b, el in enumerate(three["elements"]):
        if el is not None:
            only_el.set_morison_elements(b, *el)
    e0 = only_el.compute_morison(t, *st)
    set_all(only_mem, three["lists"])
    m0 = only_mem.compute_morison(t, *st)
    assert e0.any() and m0.any()
    # elements + members is the IEEE sum of the two parts
    assert same_bits(three["ref"], e0 + m0)
    # another body gains members: the element-only bodies return the bits they returned before
    only_el.set_morison_members(1, *three["lists"][1])
    e1 = only_el.compute_morison(t, *st)
    assert same_bits(e1[:6], e0[:6])
    assert same_bits(e1[12:], e0[12:])
    assert same_bits(e1[6:12], m0[6:12])


# ------------------------------------------------------------------------------------------------
# 4: non-interference with the steps
# ------------------------------------------------------------------------------------------------
def test_members_around_every_step_change_no_force(HF):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_members in (False, True):
        h = HF.from_case(case)
        h.add_waves_irregular(**IRREG)
        if with_members:
            h.set_morison_members(0, *frame_members(16))
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        rows = []
        for n in range(100):  # three look-ahead blocks of 32 steps
            t = SPHERE_DT * n
            st = motion.state(t)
            if with_members:
                h.morison_begin(t, *st)
            total = raw_step(h, t, st)
            if with_members:
                assert h.morison_end().any()
            rows.append(np.concatenate([total, *h.components()]))
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# 5: composition one layer up
# ------------------------------------------------------------------------------------------------
def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    lists = [frame_members(4), None, long_members(4)]
    a, b, plain = HF.from_case(case), HF.from_case(case), HF.from_case(case)
    grp, gplain = HydroGroup.from_case(case, 3), HydroGroup.from_case(case, 3)
    for h in (a, b, plain, grp, gplain):
        h.add_waves_irregular(**THREE_IRREG)
    for h in (a, b, grp):
        for k, ml in enumerate(lists):
            if ml is not None:
                h.set_morison_members(k, *ml)
        h.set_morison_elements(0, *random_elements(9, 1))
        h.set_morison_options(mwl=0.1)
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)
    for n in range(12):
        t = 0.01 * n
        st = motion.state(t)
        fa = a.step(t, *st)
        total, mor = raw_step(b, t, st), b.compute_morison(t, *st)
        assert same_bits(fa, total + mor) and same_bits(a.morison(), mor)
        assert same_bits(total, plain.step(t, *st))
        assert same_bits(grp.step(t, *st), gplain.step(t, *st) + mor) and same_bits(grp.morison(), mor)
    assert mor.any()
    # members alone make step() compose; cleared again it is the plain step
    a.set_morison_elements(0, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    b.set_morison_elements(0, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    st = motion.state(0.4)
    assert same_bits(a.step(0.4, *st), raw_step(b, 0.4, st) + b.compute_morison(0.4, *st)) and a.morison().any()
    plain.step(0.4, *st)  # (the same history for the comparison below)
    for k in (0, 2):
        a.set_morison_members(k, np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 1.0, 1.0, 1)
    st = motion.state(0.41)
    assert same_bits(a.step(0.41, *st), plain.step(0.41, *st)) and not a.morison().any()


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "morison_members_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison_members_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (40, 43)
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
    h.set_morison_elements(0, [[0, 0, -6.0], [2.5, 0.5, -3.0]], [[3, 3, 12.0], [1, 1.5, 0.5]], [[0, 0, 0], [2, 2, 1.0]])
    h.set_morison_members(0, [[0, 0, -5.0], [-3, -3, -4.0], [1, 0, 8.0]], [[0, 0, 6.0], [3, 3, 1.5], [4, 0, 9.0]],
                          [[1.2, 1.2], [0.8, 0.4], [0.5, 0.5]], [1.0, 0.9, 1.0], [2.0, 1.6, 2.0], [8, 5, 1])
    h.set_morison_options(mwl=0.25, regular_phase=0.3)
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total, mor = raw_step(h, t, st), h.compute_morison(t, *st)
        assert same_bits(row[19:25], mor) and same_bits(row[13:19], total + mor), t
        assert same_bits(row[25:43].reshape(3, 6), h.morison_member_forces(0)), t
    assert np.abs(rows[:, 25:28]).max() > 1.0 and not rows[:, 37:43].any()


# ------------------------------------------------------------------------------------------------
# 6: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    from hydrochrono_amd import capi
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    z9 = np.zeros(9)
    lin = np.tile([0.5, 0.0, 0.0], 3)
    out = np.full(18, 7.0)

    def mem(r0=(0, 0, -4.0), r1=(0, 0, 3.0), d0=1.0, d1=1.0, cd=1.0, cm=0.0, n_seg=2, n=1):
        arr = (capi.MorisonMember * n)()
        for m in arr:
            m.r0[:], m.r1[:] = r0, r1
            m.d0, m.d1, m.cd, m.cm, m.n_seg = d0, d1, cd, cm, n_seg
        return arr

    h = HF.from_case(case)
    lib = h.lib
    n = C.c_int(-1)
    rows = np.empty(6 * 1024)
    # bad index, count, list
    for body in (-1, 3, 100):
        assert lib.hc_set_morison_members(h.ctx, body, mem(), 1) == INV
        assert lib.hc_get_morison_member_count(h.ctx, body, C.byref(n)) == INV
        assert lib.hc_get_morison_member_forces(h.ctx, body, dp(rows)) == INV
    assert lib.hc_get_morison_member_count(h.ctx, 0, None) == INV
    assert lib.hc_set_morison_members(h.ctx, 0, mem(), -1) == INV
    assert lib.hc_set_morison_members(h.ctx, 0, None, 2) == INV
    assert lib.hc_set_morison_members(h.ctx, 0, mem(n=1025), 1025) == INV
    assert lib.hc_set_morison_members(h.ctx, 0, mem(n=1024), 1024) == OK
    # non-finite values, negative diameters and coefficients, zero length, n_seg
    for bad in (np.nan, np.inf, -np.inf):
        assert lib.hc_set_morison_members(h.ctx, 0, mem(r0=(0, bad, 0)), 1) == INV
        assert lib.hc_set_morison_members(h.ctx, 0, mem(r1=(bad, 0, 0)), 1) == INV
        for key in ("d0", "d1", "cd", "cm"):
            assert lib.hc_set_morison_members(h.ctx, 0, mem(**{key: bad}), 1) == INV
    for key in ("d0", "d1", "cd", "cm"):
        assert lib.hc_set_morison_members(h.ctx, 0, mem(**{key: -1e-300}), 1) == INV
    assert lib.hc_set_morison_members(h.ctx, 0, mem(r0=(1, 2, 3.0), r1=(1, 2, 3.0)), 1) == INV
    for bad in (0, -1, 65):
        assert lib.hc_set_morison_members(h.ctx, 0, mem(n_seg=bad), 1) == INV
    assert lib.hc_set_morison_members(h.ctx, 0, mem(n_seg=64), 1) == OK
    assert lib.hc_get_morison_member_count(h.ctx, 0, C.byref(n)) == OK and n.value == 1
    assert lib.hc_set_morison_members(h.ctx, 0, mem(n_seg=65), 1) == INV
    assert lib.hc_get_morison_member_count(h.ctx, 0, C.byref(n)) == OK and n.value == 1  # a refused list leaves the one before
    assert b"Morison" in lib.hc_last_error(h.ctx)
    assert lib.hc_set_morison_members(h.ctx, 0, mem(), 1) == OK
    # the getter: nothing completed yet; then an evaluation; then a setter forgets it
    assert lib.hc_get_morison_member_forces(h.ctx, 0, dp(rows)) == INV
    assert lib.hc_compute_morison(h.ctx, 0.0, dp(z9), dp(z9), dp(lin), dp(z9), dp(out)) == OK
    assert np.isclose(out[0], -0.5 * case["rho"] * 0.25 * 4.0, rtol=1e-14) and not out[6:].any()  # 4 m of draft
    assert lib.hc_get_morison_member_forces(h.ctx, 0, None) == INV
    assert lib.hc_get_morison_member_forces(h.ctx, 0, dp(rows)) == OK and rows[0] == out[0]
    assert lib.hc_set_morison_members(h.ctx, 1, mem(), 1) == OK
    assert lib.hc_get_morison_member_forces(h.ctx, 0, dp(rows)) == INV
    # between begin and end: the setter is refused, the getter has nothing completed
    assert lib.hc_morison_begin(h.ctx, 0.0, dp(z9), dp(z9), dp(lin), dp(z9)) == OK
    assert lib.hc_set_morison_members(h.ctx, 2, mem(), 1) == INV
    assert lib.hc_get_morison_member_forces(h.ctx, 0, dp(rows)) == INV
    assert lib.hc_morison_end(h.ctx, dp(out)) == OK and out[6] == out[0]
    assert lib.hc_get_morison_member_forces(h.ctx, 1, dp(rows)) == OK and rows[0] == out[6]
    # second order on: unsupported, nothing pending, and the next first-order call succeeds
    h.add_waves_irregular(spectral=True, **dict(IRREG, nfrequencies=32))
    assert lib.hc_set_morison_second_order(h.ctx, 1, 0.0, np.inf, 0.0, np.inf, 1) == OK
    assert lib.hc_morison_begin(h.ctx, 1.0, dp(z9), dp(z9), dp(lin), dp(z9)) == UNS
    assert b"member" in lib.hc_last_error(h.ctx)
    assert lib.hc_morison_end(h.ctx, dp(out)) == INV  # nothing stayed pending
    assert lib.hc_compute_morison(h.ctx, 1.0, dp(z9), dp(z9), dp(lin), dp(z9), dp(out)) == UNS
    assert lib.hc_set_morison_second_order(h.ctx, 0, 0.0, np.inf, 0.0, np.inf, 1) == OK
    assert lib.hc_compute_morison(h.ctx, 1.0, dp(z9), dp(z9), dp(lin), dp(z9), dp(out)) == OK and out[0] != 0.0
    # members on bodies a shard does not own do not stop its second-order elements; the getter refuses a body it does not own
    sh = HF.from_case(case, body_range=(1, 2))
    sh.add_waves_irregular(spectral=True, **dict(IRREG, nfrequencies=32))
    assert lib.hc_set_morison_members(sh.ctx, 0, mem(), 1) == OK
    assert lib.hc_set_morison_second_order(sh.ctx, 1, 0.0, np.inf, 0.0, np.inf, 1) == OK
    o6 = np.empty(6)
    assert lib.hc_compute_morison(sh.ctx, 1.0, dp(z9), dp(z9), dp(lin), dp(z9), dp(o6)) == OK and not o6.any()
    assert lib.hc_set_morison_members(sh.ctx, 1, mem(), 1) == OK
    assert lib.hc_compute_morison(sh.ctx, 1.0, dp(z9), dp(z9), dp(lin), dp(z9), dp(o6)) == UNS
    assert lib.hc_set_morison_second_order(sh.ctx, 0, 0.0, np.inf, 0.0, np.inf, 1) == OK
    assert lib.hc_compute_morison(sh.ctx, 1.0, dp(z9), dp(z9), dp(lin), dp(z9), dp(o6)) == OK and o6[0] != 0.0
    assert lib.hc_get_morison_member_forces(sh.ctx, 0, dp(rows)) == INV
    assert lib.hc_get_morison_member_forces(sh.ctx, 1, dp(rows)) == OK
    with pytest.raises(Exception):
        h.set_morison_members(0, [[0, 0, 0]], [[0, 0, 1]], -1.0, 1.0, 1.0, 1)
