"""tests/morison_members_ref.py against closed forms (no GPU): the restatement the GPU tests compare with has to be right by itself.
Also pins what the strip members are for -- the drag of an inclined cylinder, and a force that is continuous in the draft -- and
the layout of the ctypes struct."""
import ctypes as C

import numpy as np

import morison_members_ref as mm
import morison_ref as mr
import wave_kinematics_ref as wk

RHO = 1000.0
Z3 = np.zeros((1, 3))


def one(r0, r1, dia, cd, cm, n_seg):
    return [mm.member_lists([r0], [r1], dia, cd, cm, n_seg)]


def rpy_of(R):
    """Cardan XYZ angles of R = Rx(a) Ry(b) Rz(c): R02 = sin b, R12 = -sin a cos b, R22 = cos a cos b, R01 = -cos b sin c, R00 = cos b cos c"""
    return np.array([np.arctan2(-R[1, 2], R[2, 2]), np.arcsin(R[0, 2]), np.arctan2(-R[0, 1], R[0, 0])])


def about_axis(axis, angle):
    a = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_vertical_cylinder_in_still_water_on_a_surging_body():
    """F_x = -1/2 rho cd D |v| v draft and the moment of a uniform load, to rounding: the rule is exact for any n_seg"""
    D, cd, v, draft = 1.3, 0.9, 0.7, 7.25
    f_len = -0.5 * RHO * cd * D * abs(v) * v
    for n_seg in (1, 3, 64):
        ref = mm.members(None, 50.0, RHO, one([0.3, -0.2, -draft], [0.3, -0.2, 4.0], D, cd, 2.0, n_seg), 0.0, Z3, Z3, [[v, 0, 0]], Z3)
        want = np.array([f_len * draft, 0, 0, 0, f_len * (-draft * draft / 2), -(-0.2) * f_len * draft])
        assert np.allclose(ref["F"][0], want, rtol=1e-14, atol=1e-11), (n_seg, ref["F"][0], want)
        assert np.array_equal(ref["members"][0][0], ref["F"][0])
        assert ("cut0" in ref["cases"][0]) and ref["clear"]
    # the other end wet: the same column given top down
    ref = mm.members(None, 50.0, RHO, one([0.3, -0.2, 4.0], [0.3, -0.2, -draft], D, cd, 2.0, 3), 0.0, Z3, Z3, [[v, 0, 0]], Z3)
    assert np.allclose(ref["F"][0], want, rtol=1e-14, atol=1e-11) and "cut1" in ref["cases"][0]
    # mwl moves the surface
    ref = mm.members(None, 50.0, RHO, one([0, 0, -draft], [0, 0, 4.0], D, cd, 2.0, 5), 0.0, Z3, Z3, [[v, 0, 0]], Z3, mwl=0.5)
    assert np.isclose(ref["F"][0, 0], f_len * (draft + 0.5), rtol=1e-14)


def test_inclined_member_in_uniform_flow_and_a_turn_about_its_own_axis():
    """F = 1/2 rho cd D L |q_n| q_n, and rotating the body about the member's axis changes nothing"""
    D, cd = 0.8, 1.1
    r0, r1 = np.array([-2.0, -1.0, -3.0]) - [0, 0, 20.0], np.array([2.0, 1.0, 3.0]) - [0, 0, 20.0]
    # (the line through r0 and r1 does not pass the body origin: the turn is made about the member's axis through its middle)
    mid, e = 0.5 * (r0 + r1), (r1 - r0)
    L, a = np.linalg.norm(e), (r1 - r0) / np.linalg.norm(r1 - r0)
    v = np.array([0.9, -0.4, 0.2])
    q = -v
    qn = q - (q @ a) * a
    want = 0.5 * RHO * cd * D * L * np.linalg.norm(qn) * qn
    forces = []
    for angle in (0.0, 0.6, 2.1):
        R = about_axis(a, angle)
        pos = mid - R @ mid  # keeps the member's middle, and so the whole member, where it was
        ref = mm.members(None, 200.0, RHO, one(r0, r1, D, cd, 0.0, 4), 0.0, [pos], [rpy_of(R)], [v], Z3)
        assert np.allclose(mr.rotation(rpy_of(R)).astype(float), R, atol=1e-14)
        assert ref["cases"][0] == {"wet"}
        assert np.allclose(ref["F"][0, :3], want, rtol=1e-13, atol=1e-10), (angle, ref["F"][0, :3], want)
        forces.append(ref["F"][0, :3])
    assert np.linalg.norm(want) > 100.0
    # the same member as one three-axis element (projected areas D L |cross section| per body axis) gives another vector: a
    # cylinder at an angle to the body axes is not three flat plates
    elem = [(mid[None, :], (cd * D * L * np.sqrt(1 - a * a))[None, :], np.zeros((1, 3)))]
    el = mr.morison(None, 200.0, RHO, elem, 0.0, Z3, Z3, [v], Z3)["F"][0, :3]
    assert np.linalg.norm(el - want) > 0.1 * np.linalg.norm(want), (el, want)
    cosang = el @ want / (np.linalg.norm(el) * np.linalg.norm(want))
    assert cosang < 0.999


def test_force_is_continuous_in_the_draft_where_an_element_list_jumps():
    D, cd, cm, v, n_seg, top, bottom = 1.0, 1.0, 2.0, 0.8, 4, 5.0, -5.0
    lists = one([0, 0, bottom], [0, 0, top], D, cd, cm, n_seg)
    seg = (top - bottom) / n_seg
    zc = bottom + seg * (np.arange(n_seg) + 0.5)
    elem = [(np.stack([0 * zc, 0 * zc, zc], axis=1), np.tile([cd * D * seg, cd * D * seg, 0.0], (n_seg, 1)),
             np.tile([cm * np.pi / 4 * D * D * seg] * 2 + [0.0], (n_seg, 1)))]
    delta = 0.01
    heave = np.arange(-4.0, 4.0 + delta / 2, delta)  # carries three nodes and three element centres through the surface
    # still water, surging body: dF_x / dz = 1/2 rho cd D v^2 exactly
    lip = 0.5 * RHO * cd * D * v * v
    fx = np.array([mm.members(None, 100.0, RHO, lists, 0.0, [[0, 0, z]], Z3, [[v, 0, 0]], Z3)["F"][0, 0] for z in heave])
    assert np.max(np.abs(np.diff(fx))) <= lip * delta * (1 + 1e-9)
    fe = np.array([mr.morison(None, 100.0, RHO, elem, 0.0, [[0, 0, z]], Z3, [[v, 0, 0]], Z3)["F"][0, 0] for z in heave])
    assert np.max(np.abs(np.diff(fe))) >= lip * seg * (1 - 1e-9)  # one element's whole load at once
    # a deep-water regular wave on top.  Per length the load is at most f_max; a heave of delta moves the wet end by delta (eta is
    # the same at every node of a vertical column) and every point by delta, which changes the kinematics by k delta of their size
    # (2 k for the squared drag); the rule's points move with the cut at no more than unit rate, which the factor 2 covers
    A, om = 0.6, 1.4
    k = om * om / 9.81
    comp = wk.regular_components(A, om, k, 0.3)
    grow = np.exp(k * A)
    f_max = 0.5 * RHO * cd * D * (v + om * A * grow) ** 2 + RHO * cm * np.pi / 4 * D * D * om * om * A * grow
    lip = 2.0 * f_max * (1 + 2 * k * (top - bottom))
    for t in (0.0, 1.7):
        fx = np.array([mm.members(comp, np.inf, RHO, lists, t, [[0, 0, z]], Z3, [[v, 0, 0]], Z3)["F"][0, 0] for z in heave])
        fe = np.array([mr.morison(comp, np.inf, RHO, elem, t, [[0, 0, z]], Z3, [[v, 0, 0]], Z3)["F"][0, 0] for z in heave])
        step_m, step_e = np.max(np.abs(np.diff(fx))), np.max(np.abs(np.diff(fe)))
        print(f"t={t}: largest step of the member {step_m:.3e} N (Lipschitz bound {lip * delta:.3e}), of the element list {step_e:.3e} N")
        assert step_m <= lip * delta
        assert step_e > lip * delta


def test_body_bound_keeps_its_bits_beside_the_per_member_bound():
    """`bound` of two inputs of this file, bit for bit as before `member_bound` was split off the same derivation"""
    ref = mm.members(None, 50.0, RHO, one([0.3, -0.2, -7.25], [0.3, -0.2, 4.0], 1.3, 0.9, 2.0, 3), 0.0, Z3, Z3, [[0.7, 0, 0]], Z3)
    want = [float.fromhex("0x1.2ced300000000p-35")] * 3 + [float.fromhex("0x1.f17aaa5633fbap-33")] * 3
    assert ref["bound"][0].tolist() == want
    A, om, phi, t = 1.0, 1.1, 0.4, 2.0  # the column of convergence_errors() at n_seg = 8
    comp = wk.regular_components(A, om, om * om / 9.81, phi)
    ref = mm.members(comp, np.inf, RHO, one([0, 0, -21.0], [0, 0, 6.0], 2.0, 0.0, 2.0, 8), t, Z3, Z3, Z3, Z3)
    want = [float.fromhex("0x1.09b7046f9497bp-20")] * 3 + [float.fromhex("0x1.5acfaf787ff4cp-17")] * 3
    assert ref["bound"][0].tolist() == want
    # one member: its own bound is the body's with items_m = items
    assert np.array_equal(ref["member_bound"][0][0], ref["bound"][0])


def test_a_gauss_point_credited_to_the_neighbouring_member_breaks_the_member_bound_only():
    """What `member_bound` is for: the last Gauss point of a member summed into the next member's row (a first-segment offset or a
    point-to-member entry wrong by one) moves both rows by a whole point's force, and the body total by summation order alone."""
    A, om = 0.6, 1.4
    comp = wk.regular_components(A, om, om * om / 9.81, 0.3)
    r0 = [[0.0, 0.0, -6.0], [1.0, 1.0, -7.0], [-4.0, -3.0, -5.0]]
    r1 = [[0.0, 0.0, 7.0], [1.5, 1.0, -2.0], [4.0, 3.0, 5.5]]
    lists = [mm.member_lists(r0, r1, [1.2, 0.7, 0.9], 1.0, 2.0, [4, 2, 3])]
    ref = mm.members(comp, np.inf, RHO, lists, 1.7, [[0.0, 0.0, -2.0]], Z3, [[0.4, 0.1, 0.0]], [[0.0, 0.02, 0.01]])
    assert ref["clear"]
    pts = ref["points"][0]
    right = np.array([p.sum(axis=0) for p in pts])
    assert np.all(np.abs(right - ref["members"][0]) <= ref["member_bound"][0]) and np.all(ref["member_bound"][0] > 0.0)
    for m in (0, 1):
        wrong = [p.copy() for p in pts]
        moved, wrong[m] = wrong[m][-1:], wrong[m][:-1]
        wrong[m + 1] = np.concatenate([moved, wrong[m + 1]])
        rows = np.array([p.sum(axis=0) for p in wrong])
        assert np.abs(moved[0, :3]).max() > 1.0
        for k in (m, m + 1):
            assert np.any(np.abs(rows[k] - ref["members"][0][k]) > ref["member_bound"][0][k]), (m, k)
        assert np.all(np.abs(rows.sum(axis=0) - ref["F"][0]) <= ref["bound"][0]), m
        assert np.array_equal(rows[2 - 2 * m], right[2 - 2 * m])  # the third member is not touched


def convergence_errors():
    """|F_x - closed form| of the inertia force on a fixed vertical cylinder in a deep-water regular wave, integrated to the
    instantaneous surface: F_x = rho cm (pi / 4) D^2 w^2 A sin(theta) (e^{k eta} - e^{-k draft}) / k, theta = -w t + phi at x = 0"""
    A, om, phi, t, D, cm, draft, top = 1.0, 1.1, 0.4, 2.0, 2.0, 2.0, 21.0, 6.0
    k = om * om / 9.81
    comp = wk.regular_components(A, om, k, phi)
    th = -om * t + phi
    eta = A * np.cos(th)
    exact = RHO * cm * np.pi / 4 * D * D * om * om * A * np.sin(th) * (np.exp(k * eta) - np.exp(-k * draft)) / k
    errs = []
    for n_seg in (4, 8, 16, 32):
        ref = mm.members(comp, np.inf, RHO, one([0, 0, -draft], [0, 0, top], D, 0.0, cm, n_seg), t, Z3, Z3, Z3, Z3)
        assert "cut0" in ref["cases"][0]
        errs.append(abs(ref["F"][0, 0] - exact) / abs(exact))
    return errs


def test_convergence_against_the_closed_form_inertia_force():
    """Measured with this restatement: relative errors 1.015e-04, 6.446e-06, 4.048e-07, 2.558e-08 at n_seg = 4, 8, 16, 32 -- ratios
    per halving 15.74, 15.92, 15.82 (DESIGN.md 3.7c').  Second order was expected from the linearised surface in the cut segment;
    but this column is vertical, so eta is the same at all its nodes, h is exactly linear along it and the cut is exact: what is
    left is the two-point rule's own error, fourth order in the segment length (ratio 16).  An inclined member in a wave shorter
    than its segments would fall back to second order.  Asserted: half the smallest measured ratio."""
    errs = convergence_errors()
    ratios = [errs[i] / errs[i + 1] for i in range(3)]
    print("relative errors", " ".join(f"{e:.3e}" for e in errs), "ratios", " ".join(f"{r:.2f}" for r in ratios))
    assert errs[0] < 1e-3 and errs[-1] > 1e-12  # above the rounding floor: the ratios mean something
    assert all(r >= MEASURED_RATIO / 2 for r in ratios), ratios


MEASURED_RATIO = 15.74


def test_member_kernels_build_without_scratch_or_spills(tmp_path):
    import os
    import re
    import subprocess

    import pytest
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    root = os.path.dirname(hb.PKG)
    co = str(tmp_path / "hc_morison_members.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(root, "include"), os.path.join(hb.CSRC, "hc_morison_members.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    for kernel, count in (("morison_member_nodes_kernel", 2), ("morison_member_items_kernel", 2), ("morison_member_sum_kernel", 1)):
        assert sum(kernel in n for n in notes) == count, sorted(notes)
    for name, (scratch, vgpr, spills) in notes.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert "hc_morison_members.hip" in hb.SOURCES
    # the mirror's caller builds with plain g++ (tests/test_gpu_morison_members.py runs it)
    libdir = os.path.join(root, "hydrochrono_amd", "lib")
    out = str(tmp_path / "morison_members_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(root, "tests", "cpp", "morison_members_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)


def test_ctypes_struct_is_the_header_struct():
    from hydrochrono_amd import capi
    assert C.sizeof(capi.MorisonMember) == 88
    assert capi.MorisonMember.n_seg.offset == 80 and capi.MorisonMember.d0.offset == 48
