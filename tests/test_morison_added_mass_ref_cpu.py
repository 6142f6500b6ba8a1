"""tests/morison_added_mass_ref.py against closed forms (no GPU): the restatement the GPU tests compare with has to be right by
itself, and its cut and weights have to be those of tests/morison_members_ref.py.  Also here: the new kernels build without
scratch or spills, the library exports the four entry points, and the C++ caller compiles against the stand-in Chrono headers."""
import os
import re
import subprocess

import numpy as np
import pytest

import morison_added_mass_ref as am
import morison_members_ref as mm
import morison_ref as mr
from test_morison_members_ref_cpu import about_axis, rpy_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 1000.0
Z3 = np.zeros((1, 3))
EPS = 2.0 ** -52


def one(r0, r1, dia, n_seg):
    return [mm.member_lists([r0], [r1], np.reshape(dia, (1, -1)) if np.ndim(dia) else dia, 0.0, 0.0, n_seg)]


def cylinder_closed_form():
    """M of the vertical cylinder of the issue in still water: wet from z = -6 to 0 at (0.5, 0), m' = rho (pi / 4) D^2.
    With d = (x0, 0, z), a^ = e_z: P = diag(1, 1, 0); integrals of 1, z, z^2 over the wet length: 6, -18, 72."""
    mp, x0 = RHO * np.pi / 4 * 1.2 ** 2, 0.5
    i0, i1, i2 = 6.0, -18.0, 72.0
    M = np.zeros((6, 6))
    M[0, 0] = M[1, 1] = i0 * mp
    # -P S = [[0, z, -y], [-z, 0, x], [0, 0, 0]] with y = 0
    M[0, 4], M[1, 3], M[1, 5] = i1 * mp, -i1 * mp, x0 * i0 * mp
    # -S P S = [[z^2, 0, 0], [0, z^2, 0], [0, 0, 0]] + x-terms: (d x e_x)(d x e_x)^T + (d x e_y)(d x e_y)^T
    # d x e_x = (0, z, 0), d x e_y = (-z, 0, x): sum = [[z^2, 0, -x z], [0, z^2, 0], [-x z, 0, x^2]]
    M[3, 3] = M[4, 4] = i2 * mp
    M[3, 5] = -x0 * i1 * mp
    M[5, 5] = x0 * x0 * i0 * mp
    return np.triu(M) + np.triu(M, 1).T, mp


CYLINDER = dict(r0=[0.5, 0.0, -6.0], r1=[0.5, 0.0, 2.0], dia=1.2, n_seg=5)


def test_vertical_cylinder_in_still_water():
    """Every integrand is at most quadratic in z: the two-point rule is exact, the error is rounding alone"""
    ref = am.added_mass(None, 50.0, RHO, one(**CYLINDER), [1.0], 0.0, Z3, Z3)
    want, mp = cylinder_closed_form()
    assert ref["cases"][0] == {"wet", "cut0", "dry"} and ref["clear"]
    assert abs(ref["h"][0][3] / (ref["h"][0][3] - ref["h"][0][4]) - 0.75) < 4 * EPS  # the cut inside segment 3 at sigma = 0.75
    M = ref["M"][0]
    assert M[0, 0] == pytest.approx(6 * mp, rel=1e-15) and M[2, 2] == 0.0 and M[0, 4] == pytest.approx(-18 * mp, rel=1e-15)
    assert M[4, 4] == pytest.approx(72 * mp, rel=1e-15)
    scale = mp * np.array([6.0, 18.0 + 0.5 * 6, 72.0 + 0.25 * 6])[am.BLOCK]
    print("worst |M - closed form| / scale", np.max(np.abs(M - want) / scale))
    assert np.all(np.abs(M - want) <= 8 * EPS * scale)
    assert np.all(np.abs(M - want) <= ref["bound"][0] + 4 * EPS * scale)  # (the closed form's own rounding)
    assert np.array_equal(ref["members"][0][0], M)
    # ca scales it, ca = 0 gives exact zeros
    assert np.allclose(am.added_mass(None, 50.0, RHO, one(**CYLINDER), [0.25], 0.0, Z3, Z3)["M"][0], 0.25 * M, rtol=1e-15, atol=0)
    assert not np.any(am.added_mass(None, 50.0, RHO, one(**CYLINDER), [0.0], 0.0, Z3, Z3)["M"])


def test_rotated_body_is_a_congruence():
    """The same member on a turned body whose wet part is the same piece of the member: M = T M0 T^T, T = diag(R, R)"""
    lists = one([0.5, 0.0, -6.0], [0.5, 0.0, -1.0], [1.2, 0.8], 3)  # wholly wet before and after the turn
    M0 = am.added_mass(None, 50.0, RHO, lists, [1.0], 0.0, Z3, Z3)["M"][0]
    R = about_axis([1.0, -2.0, 0.5], 0.4)
    ref = am.added_mass(None, 50.0, RHO, lists, [1.0], 0.0, Z3, [rpy_of(R)])
    assert ref["cases"][0] == {"wet"}
    Rl = mr.rotation(rpy_of(R)).astype(float)
    T = np.block([[Rl, np.zeros((3, 3))], [np.zeros((3, 3)), Rl]])
    want = T @ M0 @ T.T
    assert np.max(np.abs(M0)) > 1e3 and np.max(np.abs(ref["M"][0] - M0)) > 1.0
    assert np.all(np.abs(ref["M"][0] - want) <= 64 * EPS * np.max(np.abs(M0)))
    # a displaced body: d is measured from the body's reference point, so a horizontal shift changes nothing
    moved = am.added_mass(None, 50.0, RHO, lists, [1.0], 0.0, [[7.0, -3.0, 0.0]], [rpy_of(R)])["M"][0]
    assert np.all(np.abs(moved - ref["M"][0]) <= 64 * EPS * np.max(np.abs(M0)))


def inclined_inputs():
    r0 = [[0.0, 0.0, -6.0], [1.0, 1.0, -7.0], [-4.0, -3.0, -5.0]]
    r1 = [[0.0, 0.0, 7.0], [1.5, 1.0, -2.0], [4.0, 3.0, 5.5]]
    return [mm.member_lists(r0, r1, [[1.2, 1.2], [0.7, 0.7], [0.9, 0.4]], 0.0, [1.0, 0.5, 0.8], [4, 2, 3])], [[1.0, 0.5, 0.8]]


def test_symmetric_and_positive_semidefinite():
    lists, ca = inclined_inputs()
    ref = am.added_mass(None, np.inf, RHO, lists, ca, 0.0, [[0.0, 0.0, -2.0]], [[0.1, -0.2, 0.3]])
    assert {"wet", "cut0"} <= ref["cases"][0]
    for M, bound in [(ref["M"][0], ref["bound"][0])] + list(zip(ref["members"][0], ref["member_bound"][0])):
        assert np.array_equal(M, M.T)
        lo = np.linalg.eigvalsh(M)[0]
        # an eigenvalue moves by at most the norm of the perturbation: 6 x the largest entry bound, plus eigvalsh's own rounding
        assert lo >= -(6 * np.max(bound) + 64 * EPS * np.max(np.abs(M))), lo
        assert np.linalg.eigvalsh(M)[-1] > 1e3


def test_identity_with_the_inertia_force_of_the_member_restatement():
    """cm = ca, cd = 0, a uniform fluid acceleration a: the force of morison_members_ref.members() -- its cut, its weights, its
    projection and its cross product -- is M (a, 0)"""
    lists, ca = inclined_inputs()
    st = ([[0.0, 0.0, -2.0]], [[0.1, -0.2, 0.3]])
    ref = am.added_mass(None, np.inf, RHO, lists, ca, 0.0, *st)
    first = mm._kin
    for a in ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.3, -0.7, 1.1]):
        def uniform(comp, depth, pts, t, mwl, stretching, a=a):
            n = len(pts)
            z1, z3 = np.zeros(n), np.zeros((n, 3))
            return z1, z3, np.tile(np.asarray(a), (n, 1)), z1, z3, z3
        mm._kin = uniform
        try:
            got = mm.members(None, np.inf, RHO, lists, 0.0, *st, Z3, Z3)
        finally:
            mm._kin = first
        acc = np.concatenate([a, np.zeros(3)])
        for m in range(3):
            want = ref["members"][0][m] @ acc
            assert np.all(np.abs(got["members"][0][m] - want) <= 32 * EPS * np.max(np.abs(want))), (a, m)
        assert np.max(np.abs(got["F"][0])) > 1e3


def taper_errors():
    """|M_44 - closed form| of a tapered vertical column wholly under water: D = D0 + (D1 - D0) s, d = (0, 0, z0 + L s), so
    M_44 = rho (pi / 4) L int_0^1 D(s)^2 z(s)^2 ds, a quartic integrand"""
    D0, D1, z0, L = 2.0, 0.5, -21.0, 18.0
    s = np.polynomial.Polynomial
    integrand = (s([D0, D1 - D0]) ** 2 * s([z0, L]) ** 2).integ()
    exact = RHO * np.pi / 4 * L * (integrand(1.0) - integrand(0.0))
    errs = []
    for n_seg in (4, 8, 16):
        ref = am.added_mass(None, np.inf, RHO, one([0, 0, z0], [0, 0, z0 + L], [D0, D1], n_seg), [1.0], 0.0, Z3, Z3)
        assert ref["cases"][0] == {"wet"}
        errs.append(abs(ref["M"][0][4, 4] - exact) / exact)
    return errs


MEASURED_TAPER_RATIO = 16.00


def test_taper_converges_at_fourth_order():
    """Measured with this restatement: relative errors 3.609e-05, 2.256e-06, 1.410e-07 at n_seg = 4, 8, 16 -- ratios per halving
    16.00, 16.00 (DESIGN.md 3.7c''': the error of the two-point rule on a quartic is its fourth-derivative term alone, so the
    ratio is 16 to rounding).  Asserted: half the smallest measured ratio."""
    errs = taper_errors()
    ratios = [errs[i] / errs[i + 1] for i in range(2)]
    print("relative errors", " ".join(f"{e:.3e}" for e in errs), "ratios", " ".join(f"{r:.2f}" for r in ratios))
    assert errs[0] < 1e-3 and errs[-1] > 1e-12  # above the rounding floor: the ratios mean something
    assert all(r >= MEASURED_TAPER_RATIO / 2 for r in ratios), ratios


def test_mass_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_morison_members.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_morison_members.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    for kernel in ("morison_member_mass_kernel", "morison_member_mass_sum_kernel"):
        hit = [n for n in notes if kernel in n]
        assert len(hit) == 1, sorted(notes)
        scratch, vgpr, spills = notes[hit[0]]
        print(kernel, "vgpr", vgpr, "scratch", scratch, "spills", spills)
        assert scratch == 0 and spills == 0 and vgpr <= 128  # (128: four waves per SIMD still fit)


def test_library_exports_the_entry_points_and_the_caller_compiles(tmp_path):
    from hydrochrono_amd import build as hb
    from hydrochrono_amd import capi
    hb.build()
    lib = capi.load()
    for name in ("hc_set_morison_member_added_mass", "hc_get_morison_member_added_mass_coefficients", "hc_get_morison_added_mass",
                 "hc_get_morison_member_added_mass"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "morison_added_mass_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "chrono_stub"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "morison_added_mass_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
