"""The strip members' added-mass matrix on the instantaneous wet length on the GPU (hc_set_morison_member_added_mass,
hc_get_morison_added_mass, hc_get_morison_member_added_mass; csrc/hc_morison_members.hip: morison_member_mass_kernel) against the
closed form of a vertical cylinder and the tests' restatement (tests/morison_added_mass_ref.py), fed the context's own spectrum.

Tolerance: the bound the restatement returns per entry (derived in its docstring: a cut segment's sensitivity to its cut, and
(items + 64) 2^-52 of the uncancelled magnitudes).  Every comparison first asserts, on the reference side, that every node's |h_j|
exceeds the reference's own bound of its eta error, so GPU and restatement take the same case everywhere; the grid-edge test puts a
node on the surface on purpose, in still water on an unrotated body, where h_j = 0 exactly on both sides."""
import os
import subprocess

import numpy as np
import pytest

import directional_ref as dr
import morison_added_mass_ref as am
import morison_members_ref as mm
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case
from test_morison_added_mass_ref_cpu import CYLINDER, cylinder_closed_form

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
WAVES8 = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0, frequency_min=0.05,
              frequency_max=0.8, nfrequencies=8, seed=3)
T = 12.5


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def three_members():
    """one member wholly wet, one wholly dry, one inclined, tapered and cut"""
    r0 = [[-5.0, 0.5, -8.0], [-2.0, 2.0, 8.0], [-4.0, -3.0, -5.0]]
    r1 = [[5.0, 0.5, -8.5], [2.0, 2.0, 9.0], [4.0, 3.0, 5.5]]
    return mm.member_lists(r0, r1, [[0.5, 0.6], [0.4, 0.4], [0.9, 0.3]], [1.0, 1.0, 1.1], [2.0, 2.0, 1.6], [3, 2, 3])


CA = [1.0, 0.7, 0.8]


def two_body_state(other=False):
    """body 1 rotated and displaced; `other`: other velocities, which the matrix does not see"""
    pos = np.array([[0.0, 0.0, -2.0], [15.0, 2.0, -1.5], [30.0, 0.0, 0.0]])
    rpy = np.array([[0.0, 0.0, 0.0], [0.1, -0.15, 0.3], [0.0, 0.0, 0.0]])
    lin = np.array([[0.4, 0.1, 0.0], [-0.2, 0.3, 0.1], [0.0, 0.0, 0.0]]) * (-2.5 if other else 1.0)
    ang = np.array([[0.0, 0.02, 0.01], [0.03, 0.0, -0.02], [0.0, 0.0, 0.0]]) + (0.05 if other else 0.0)
    return pos, rpy, lin, ang


def set_two_bodies(h):
    for b in (0, 1):
        h.set_morison_members(b, *three_members())
        h.set_morison_member_added_mass(b, CA)


def serial_sum(rows):
    acc = np.zeros((6, 6))
    for r in rows:
        acc = acc + r
    return acc


def check_against(h, ref, bodies, what, need_clear=True):
    """the getters of `h` against a result of the restatement, body matrices and member rows, with the bitwise invariants"""
    if need_clear:
        assert ref["clear"] and ref["margin"] > ref["eta_bound"], \
            f"{what}: a node is {ref['margin']:.3e} m from the free surface, the eta bound is {ref['eta_bound']:.3e} m (choose other inputs)"
    worst = 0.0
    for b in bodies:
        M, rows = h.morison_added_mass(b), h.morison_member_added_mass(b)
        assert np.all(np.isfinite(M)) and same_bits(M, M.T) and all(same_bits(r, r.T) for r in rows), (what, b)
        assert same_bits(serial_sum(rows), M), f"{what}: the serial sum of body {b}'s member matrices is not the body's"
        err, merr = np.abs(M - ref["M"][b]), np.abs(rows - ref["members"][b])
        w_b = float(np.max(err / np.maximum(ref["bound"][b], 1e-300)))
        w_m = float(np.max(merr / np.maximum(ref["member_bound"][b], 1e-300))) if rows.size else 0.0
        print(f"{what}: body {b}: worst |gpu - ref| / bound = {w_b:.3e} (members {w_m:.3e}), max |M| = {np.max(np.abs(ref['M'][b])):.3e}, "
              f"largest bound / max |M| = {np.max(ref['bound'][b]) / max(np.max(np.abs(ref['M'][b])), 1e-300):.2e}")
        assert np.all(err <= ref["bound"][b]), f"{what}: body {b}: worst {w_b:.3e} of the bound"
        assert np.all(merr <= ref["member_bound"][b]), f"{what}: body {b}'s member rows: worst {w_m:.3e} of the member bound"
        worst = max(worst, w_b, w_m)
    return worst


# ------------------------------------------------------------------------------------------------
# 1: the closed form
# ------------------------------------------------------------------------------------------------
def test_vertical_cylinder_in_still_water_closed_form(HF):
    case = dict(sphere_case(), rho=1000.0)
    h = HF.from_case(case)
    h.add_waves_none()
    lists = [mm.member_lists([CYLINDER["r0"]], [CYLINDER["r1"]], CYLINDER["dia"], 1.0, 2.0, CYLINDER["n_seg"])]
    h.set_morison_members(0, *lists[0])
    h.set_morison_member_added_mass(0, 1.0)
    z = np.zeros((1, 3))
    h.compute_morison(0.0, z, z, z, z)
    want, mp = cylinder_closed_form()
    ref = am.added_mass(None, case["water_depth"], 1000.0, lists, [[1.0]], 0.0, z, z)
    M = h.morison_added_mass(0)
    scale = mp * np.array([6.0, 18.0 + 0.5 * 6, 72.0 + 0.25 * 6])[am.BLOCK]
    bound = ref["bound"][0] + 4 * EPS * scale  # the restatement's bound around the closed form, and the closed form's own rounding
    print("closed form: worst |gpu - closed form| / bound", np.max(np.abs(M - want) / bound))
    assert np.all(np.abs(M - want) <= bound)
    assert M[0, 0] > 6000.0 and M[2, 2] == 0.0 and same_bits(M, M.T) and same_bits(h.morison_member_added_mass(0)[0], M)
    check_against(h, ref, [0], "closed form")
    h.close()


# ------------------------------------------------------------------------------------------------
# 2: against the restatement, first and second order, long- and short-crested
# ------------------------------------------------------------------------------------------------
def test_two_bodies_against_the_restatement_on_four_seas(HF):
    case = three_body_case()
    h = HF.from_case(case)
    h.add_waves_irregular(**WAVES8)
    comp = wk.irregular_components(h.irreg_spectrum())
    assert len(comp[0]) == 8
    set_two_bodies(h)
    h.set_morison_options(mwl=0.25, wave_stretching=True)
    lists, ca = [three_members(), three_members(), None], [CA, CA, None]
    st = two_body_state()
    kw = dict(mwl=0.25)
    results = {}

    def run(what, components, order2):
        h.compute_morison(T, *st)
        eta2 = [h.morison_member_increments(b)["node_eta2"] for b in (0, 1)] + [None] if order2 else None
        if order2:
            assert all(np.any(e != 0.0) for e in eta2[:2])
        ref = am.added_mass(components, case["water_depth"], case["rho"], lists, ca, T, st[0], st[1], node_eta2=eta2, **kw)
        assert all({"wet", "dry"} <= ref["cases"][b] and ref["cases"][b] & {"cut0", "cut1"} for b in (0, 1)), ref["cases"]
        results[what] = (check_against(h, ref, [0, 1], what), h.morison_added_mass())
        assert not h.morison_added_mass(2).any() and np.max(np.abs(h.morison_added_mass(1))) > 1e3

    run("long-crested", comp, False)
    h.set_morison_second_order(True)
    h.set_morison_members_second_order(True)
    run("long-crested, order 2", comp, True)
    th = h.set_wave_spreading(0.4, s=0.0)
    h.set_morison_second_order_directional(True)
    run("directional, order 2", dr.with_directions(comp, th), True)
    h.set_morison_second_order(False)
    run("directional", dr.with_directions(comp, th), False)
    for a, b in (("long-crested", "long-crested, order 2"), ("directional", "directional, order 2"), ("long-crested", "directional")):
        assert not np.array_equal(results[a][1][:2], results[b][1][:2]), (a, b)
    print("largest ratio over the four seas:", max(r[0] for r in results.values()))
    h.close()


# ------------------------------------------------------------------------------------------------
# 3: bitwise invariants
# ------------------------------------------------------------------------------------------------
def test_matrix_bits_do_not_depend_on_velocities_shards_or_other_bodies(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.synthetic import many_body_case
    case = three_body_case()
    whole, group = HF.from_case(case), HydroGroup.from_case(case, 3)
    for h in (whole, group):
        h.add_waves_irregular(**WAVES8)
        set_two_bodies(h)
    st = two_body_state()
    F = whole.compute_morison(T, *st)
    M, rows = whole.morison_added_mass(), [whole.morison_member_added_mass(b) for b in (0, 1)]
    assert M.shape == (3, 6, 6) and M[:2].any(axis=(1, 2)).all() and not M[2].any()
    whole.compute_morison(T, *two_body_state(other=True))
    assert same_bits(whole.morison_added_mass(), M)
    assert same_bits(group.compute_morison(T, *st), F) and same_bits(group.morison_added_mass(), M)
    for b in (0, 1):
        assert same_bits(group.morison_member_added_mass(b), rows[b]) and same_bits(group.morison_added_mass(b), M[b])
    with pytest.raises(Exception):
        group.morison_added_mass(3)
    # a member with ca = 0: its row is exact zeros, and the forces keep their bits whether ca is set or not
    assert same_bits(whole.compute_morison(T, *st), F)
    frc = [whole.morison_member_forces(b) for b in (0, 1)]
    whole.set_morison_member_added_mass(1, [0.3, 0.0, 0.0])
    assert same_bits(whole.compute_morison(T, *st), F) and all(same_bits(whole.morison_member_forces(b), frc[b]) for b in (0, 1))
    r = whole.morison_member_added_mass(1)
    assert r[0].any() and not r[1].any() and not r[2].any() and not np.signbit(r[1:]).any()
    assert same_bits(whole.morison_added_mass(0), M[0])
    for b in (0, 1):
        whole.set_morison_member_added_mass(b, None)
    assert same_bits(whole.compute_morison(T, *st), F) and all(same_bits(whole.morison_member_forces(b), frc[b]) for b in (0, 1))
    whole.close()
    group.close()
    # the same body data as the only body of a 1-body context and as body 2 of a 3-body one with another list beside it
    one, three = (HF.from_case(many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)) for N in (1, 3))
    one.set_morison_members(0, *three_members())
    one.set_morison_member_added_mass(0, CA)
    three.set_morison_members(2, *three_members())
    three.set_morison_member_added_mass(2, CA)
    three.set_morison_members(0, *mm.member_lists([[0.0, 0.0, -6.0]], [[0.0, 0.0, 7.0]], 1.2, 1.0, 2.0, 4))
    three.set_morison_member_added_mass(0, 0.5)
    for h in (one, three):
        h.add_waves_irregular(**WAVES8)
    st1 = [x[1:2].copy() for x in st]
    st3 = [np.concatenate([x, x, x]) for x in st1]
    for x in st3:
        x[:2] += 0.37  # the other bodies move differently
    one.compute_morison(T, *st1)
    three.compute_morison(T, *st3)
    assert one.morison_added_mass(0).any() and same_bits(one.morison_added_mass(0), three.morison_added_mass(2))
    assert same_bits(one.morison_member_added_mass(0), three.morison_member_added_mass(2))
    one.close()
    three.close()


def test_without_ca_the_getters_refuse_and_the_step_keeps_its_bits(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_members in (False, True):
        h = HF.from_case(case)
        h.add_waves_irregular(**dict(WAVES8, simulation_dt=SPHERE_DT))
        if with_members:
            h.set_morison_members(0, *three_members())
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        rows = []
        for n in range(6):
            t = SPHERE_DT * n
            st = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in motion.state(t)]
            out = np.empty(h.D_local)
            if with_members:
                h.morison_begin(t, *st)
            assert h.lib.hc_step(h.ctx, t, *[x.ctypes.data_as(capi.c_double_p) for x in st], out.ctypes.data_as(capi.c_double_p)) == capi.HC_OK
            if with_members:
                h.morison_end()
                buf = np.empty(36 * 3)
                assert h.lib.hc_get_morison_added_mass(h.ctx, 0, buf.ctypes.data_as(capi.c_double_p)) == capi.HC_ERR_INVALID
                assert h.lib.hc_get_morison_member_added_mass(h.ctx, 0, buf.ctypes.data_as(capi.c_double_p)) == capi.HC_ERR_INVALID
                assert h.morison_member_forces(0).shape == (3, 6) and not h.morison_added_mass(0).any()
            rows.append(out)
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# 4: grid edges
# ------------------------------------------------------------------------------------------------
def test_full_workgroup_plus_a_partly_filled_one_and_a_node_on_the_surface(HF):
    """n_seg = 64, 64, 1: 128 + 128 + 2 Gauss points; the last member's upper node lies on the still-water surface, h = 0"""
    case = sphere_case()
    h = HF.from_case(case)
    h.add_waves_none()
    r0 = [[0.0, 0.0, -6.0], [-4.0, -3.0, 5.5], [1.0, 0.0, -2.0]]
    r1 = [[0.5, 0.25, 7.0], [4.0, 3.0, -5.0], [1.0, 0.0, 0.0]]
    lists = [mm.member_lists(r0, r1, [[1.2, 1.0], [0.9, 0.3], [0.5, 0.5]], 1.0, 2.0, [64, 64, 1])]
    ca = [[1.0, 0.5, 2.0]]
    h.set_morison_members(0, *lists[0])
    h.set_morison_member_added_mass(0, ca[0])
    z = np.zeros((1, 3))
    h.compute_morison(0.0, z, z, z, z)
    ref = am.added_mass(None, case["water_depth"], case["rho"], lists, ca, 0.0, z, z)
    assert ref["h"][0][-1] == 0.0 and ref["h"][0].size == 65 + 65 + 2 and {"wet", "dry", "cut0", "cut1"} <= ref["cases"][0]
    others = np.abs(ref["h"][0][:-1])
    assert np.min(others) > 1e-3  # no other node near the surface: 0 is the one edge, and it is exact on both sides
    check_against(h, ref, [0], "grid edges", need_clear=False)
    rows = h.morison_member_added_mass(0)
    assert rows[2][0, 0] == pytest.approx(case["rho"] * 2.0 * np.pi / 4 * 0.25 * 2.0, rel=1e-14)  # the whole segment is wet
    h.close()


# ------------------------------------------------------------------------------------------------
# 5: protocol
# ------------------------------------------------------------------------------------------------
def test_errors_and_protocol(HF):
    from hydrochrono_amd import capi
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    case = three_body_case()
    h = HF.from_case(case, body_range=(0, 2))
    h.add_waves_irregular(**WAVES8)
    set_two_bodies(h)
    st = two_body_state()
    buf = np.empty(36 * 3)
    dp = buf.ctypes.data_as(capi.c_double_p)
    getters = (h.lib.hc_get_morison_added_mass, h.lib.hc_get_morison_member_added_mass)

    def answers(body=0):
        return [g(h.ctx, body, dp) for g in getters]
    assert answers() == [INV, INV]  # before any evaluation
    h.compute_morison(T, *st)
    assert answers() == [OK, OK] and answers(1) == [OK, OK]
    assert answers(2) == [INV, INV] and answers(-1) == [INV, INV]  # not owned
    assert h.lib.hc_get_morison_added_mass(h.ctx, 0, None) == INV
    h.set_morison_member_added_mass(1, CA)  # a ca change
    assert answers() == [INV, INV]
    h.compute_morison(T, *st)
    assert answers() == [OK, OK]
    h.set_morison_members(2, *three_members())  # a list change, of a body that is not owned even
    assert answers() == [INV, INV]
    h.compute_morison(T, *st)
    assert answers() == [OK, OK]
    ca = np.array(CA)
    cp = ca.ctypes.data_as(capi.c_double_p)
    for bad in ([1.0, -0.5, 0.0], [1.0, np.nan, 0.0], [np.inf, 0.0, 0.0]):
        b = np.array(bad)
        assert h.lib.hc_set_morison_member_added_mass(h.ctx, 0, b.ctypes.data_as(capi.c_double_p), 3) == INV
    assert h.lib.hc_set_morison_member_added_mass(h.ctx, 0, cp, 2) == INV and h.lib.hc_set_morison_member_added_mass(h.ctx, 0, cp, 4) == INV
    assert h.lib.hc_set_morison_member_added_mass(h.ctx, 3, cp, 3) == INV
    assert answers() == [OK, OK]  # a refused call changes nothing
    h.morison_begin(T, *st)
    assert h.lib.hc_set_morison_member_added_mass(h.ctx, 0, cp, 3) == INV  # between begin and end
    h.morison_end()
    assert same_bits(h.morison_member_added_mass_coefficients(0), ca)
    h.set_morison_members(0, *three_members())  # resets ca
    assert not h.morison_member_added_mass_coefficients(0).any() and same_bits(h.morison_member_added_mass_coefficients(1), ca)
    h.compute_morison(T, *st)
    assert answers() == [OK, OK] and not h.morison_member_added_mass(0).any() and h.morison_added_mass(1).any()
    h.set_morison_member_added_mass(1, None)  # no ca > 0 on an owned member: nothing to answer with
    h.compute_morison(T, *st)
    assert answers() == [INV, INV] and answers(1) == [INV, INV]
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: front ends
# ------------------------------------------------------------------------------------------------
def test_python_front_ends_and_the_force_helper(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    whole = HF.from_case(case)
    group = HydroGroup([HF.from_case(case, body_range=r) for r in ((0, 1), (1, 3))])
    for h in (whole, group):
        h.add_waves_irregular(**WAVES8)
        set_two_bodies(h)
    st = two_body_state()
    whole.compute_morison(T, *st)
    group.compute_morison(T, *st)
    raw = np.empty((3, 6, 6))
    for b in (0, 1):
        assert whole.lib.hc_get_morison_added_mass(whole.ctx, b, raw[b].ctypes.data_as(capi.c_double_p)) == capi.HC_OK
        rows = np.empty((3, 6, 6))
        assert whole.lib.hc_get_morison_member_added_mass(whole.ctx, b, rows.ctypes.data_as(capi.c_double_p)) == capi.HC_OK
        assert same_bits(whole.morison_member_added_mass(b), rows) and same_bits(group.morison_member_added_mass(b), rows)
        assert same_bits(whole.morison_added_mass(b), raw[b]) and same_bits(group.morison_added_mass(b), raw[b])
    raw[2] = 0.0
    assert same_bits(whole.morison_added_mass(), raw) and same_bits(group.morison_added_mass(), raw)
    assert same_bits(group.morison_member_added_mass_coefficients(1), np.array(CA))
    rng = np.random.default_rng(5)
    lin, ang = rng.uniform(-1, 1, (3, 3)), rng.uniform(-0.2, 0.2, (3, 3))
    acc = np.concatenate([lin, ang], axis=1)
    want = np.array([-(raw[b] @ acc[b]) for b in range(3)])
    mag = np.array([np.abs(raw[b]) @ np.abs(acc[b]) for b in range(3)])
    for h in (whole, group):
        got = h.morison_added_mass_force(lin, ang)
        assert got.shape == (3, 6) and np.all(np.abs(got - want) <= 8 * EPS * mag) and np.max(np.abs(got[:2])) > 100.0 and not got[2].any()
    whole.close()
    group.close()


def test_cpp_mirror_and_the_added_mass_load(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "morison_added_mass_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "chrono_stub"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "morison_added_mass_caller.cpp"), "-o", exe,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "three_body.h5")
    outputs = []
    for devices in ("0", "0,0,0"):
        r = subprocess.run([exe, h5, devices], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (devices, r.returncode, r.stderr)
        outputs.append(r.stdout)
    assert outputs[0] and outputs[1] == outputs[0]  # identical text whatever the device list
    lines = [ln.split() for ln in outputs[0].strip().splitlines()]
    body = {int(ln[1]): np.array([float.fromhex(v) for v in ln[2:]]).reshape(6, 6) for ln in lines if ln[0] == "BODY"}
    member = {(int(ln[1]), int(ln[2])): np.array([float.fromhex(v) for v in ln[3:]]).reshape(6, 6) for ln in lines if ln[0] == "MEMBER"}
    state = [float.fromhex(v) for v in [ln for ln in lines if ln[0] == "STATE"][0][1:]]
    # the same evaluation through the Python front end: the lists of tests/cpp/morison_added_mass_caller.cpp
    r0 = [[0.5, 0.0, -6.0], [-4.0, -3.0, -5.0], [1.0, 1.0, -7.0]]
    r1 = [[0.5, 0.0, 2.0], [4.0, 3.0, 5.5], [1.5, 1.0, -2.0]]
    dia = [[1.25, 1.25], [0.875, 0.375], [0.75, 0.75]]
    h = HF(3)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_none()
    h.set_morison_members(0, r0[:2], r1[:2], dia[:2], 1.0, 2.0, [5, 3])
    h.set_morison_members(2, r0, r1, dia, 1.0, 2.0, [5, 3, 2])
    h.set_morison_member_added_mass(0, [1.0, 0.5])
    h.set_morison_member_added_mass(2, [0.75, 0.0, 1.0])
    z = np.zeros((3, 3))
    h.compute_morison(state[0], np.array(state[1:]).reshape(3, 3), z, z, z)
    for b in range(3):
        assert same_bits(body[b + 1], h.morison_added_mass(b)), b
    assert sorted(member) == [(1, 0), (1, 1), (3, 0), (3, 1), (3, 2)]
    for (b, m), rows in member.items():
        assert same_bits(rows, h.morison_member_added_mass(b - 1)[m]), (b, m)
    assert body[1][0, 0] > 1000.0 and not body[2].any() and not member[(3, 1)].any()
    h.close()
