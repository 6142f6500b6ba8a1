"""The nonlinear surface forces without a GPU: the tests' NumPy restatement (tests/nonlinear_ref.py) against closed forms, and the
build of the kernels (csrc/hc_nonlinear.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_nonlinear.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import nonlinear_ref as nr
import wave_kinematics_ref as wk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81


def test_submerged_cube_in_still_water_is_archimedes_at_any_attitude():
    """(a) The centroid rule is exact for a pressure linear in z: a closed, fully submerged surface gives (0, 0, rho g V)."""
    L = 2.0
    panels = [nr.triangles_to_panels(nr.box_triangles([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], m=3))]
    for rpy in ([0.0, 0.0, 0.0], [0.3, -0.4, 1.1], [-1.2, 0.7, 2.9]):
        for mwl in (0.0, 0.75):
            out = nr.nonlinear(None, 50.0, RHO, G, panels, 1.0, [3.0, -2.0, -10.0], rpy, mwl=mwl)
            assert out["wet"][0].all() and out["margin"] > 5.0
            want = np.array([0.0, 0.0, RHO * G * L ** 3])
            assert np.all(np.abs(out["buoy"][0, :3] - want) <= out["bound_buoy"][0, :3]), (rpy, out["buoy"][0, :3] - want, out["bound_buoy"][0, :3])
            # a uniform body's buoyancy acts at the centre of volume, here the body reference: no moment
            assert np.all(np.abs(out["buoy"][0, 3:]) <= out["bound_buoy"][0, 3:])
            assert not out["fk"].any()
            assert np.all(out["bound_buoy"][0] < 1e-11 * want[2]) and np.all(out["bound_buoy"][0] > 0)


def test_upright_box_through_the_surface_with_a_panel_row_on_the_waterline():
    """(b) Draft 3 m of a 4 m x 3 m box, sides in rows of 1 m: a row boundary lies exactly on the waterline, every centroid is
    clear of it, and buoy_z = rho g A_wp draft."""
    draft, a, b = 3.0, 4.0, 3.0
    panels = [nr.triangles_to_panels(nr.box_triangles([-a / 2, -b / 2, -draft], [a / 2, b / 2, 2.0], m=4, mz=5))]
    out = nr.nonlinear(None, 50.0, RHO, G, panels, 0.0, [7.0, 1.0, 0.0], [0.0, 0.0, 0.6])
    assert out["margin"] > 0.3
    want = RHO * G * a * b * draft
    assert abs(out["buoy"][0, 2] - want) <= out["bound_buoy"][0, 2]
    assert np.all(np.abs(out["buoy"][0, :2]) <= out["bound_buoy"][0, :2])
    wet = out["wet"][0]
    c = panels[0][0]
    assert np.array_equal(wet, c[:, 2] <= 0.0) and 0 < wet.sum() < wet.size
    # the same box with mwl raised by one row: one more metre of draft
    up = nr.nonlinear(None, 50.0, RHO, G, panels, 0.0, [7.0, 1.0, 0.0], [0.0, 0.0, 0.6], mwl=1.0)
    assert abs(up["buoy"][0, 2] - RHO * G * a * b * (draft + 1.0)) <= up["bound_buoy"][0, 2]


def fk_closed_form(A, omega, k, phi, t, centre, L):
    """-int grad p_d dV over the cube, p_d = rho (omega^2 A / k) e^{k z} cos(k x - omega t + phi) (deep water)."""
    x0, x1 = centre[0] - L / 2, centre[0] + L / 2
    z0, z1 = centre[2] - L / 2, centre[2] + L / 2
    psi = -omega * t + phi
    Ez = (np.exp(k * z1) - np.exp(k * z0)) / k
    Sx = (np.cos(k * x0 + psi) - np.cos(k * x1 + psi)) / k
    Cx = (np.sin(k * x1 + psi) - np.sin(k * x0 + psi)) / k
    amp = RHO * (omega * omega * A / k) * k * L
    return amp * Ez * Sx, -amp * Ez * Cx


KL = 1.0  # k L of case (c): the quadrature error of the centroid rule is then ~1e-2 .. 1e-4 of the force over m = 4 .. 16, far above
          # rounding, and the h^2 term dominates its expansion (the next one is (k h)^2 / 12-ish smaller)


def test_froude_krylov_on_a_submerged_cube_converges_at_second_order():
    """(c) Deep-water regular wave over a submerged cube: fk[0] and fk[2] against the volume integral of -grad p_d; each halving of
    the panel size divides the error by 3 to 5."""
    L, A, omega, phi, t = 2.0, 0.4, None, 0.7, 1.3
    k = KL / L
    omega = np.sqrt(G * k)
    comp = wk.regular_components(A, omega, k, phi)
    centre = np.array([5.0, -1.0, -4.0])
    Fx, Fz = fk_closed_form(A, omega, k, phi, t, centre, L)
    errs = []
    for m in (4, 8, 16):
        panels = [nr.triangles_to_panels(nr.box_triangles([-L / 2] * 3, [L / 2] * 3, m=m))]
        out = nr.nonlinear(comp, np.inf, RHO, G, panels, t, centre, [0.0, 0.0, 0.0])
        assert out["wet"][0].all()
        errs.append((abs(out["fk"][0, 0] - Fx), abs(out["fk"][0, 2] - Fz)))
        assert abs(out["fk"][0, 1]) < 0.02 * abs(Fx)  # the two y faces are split along different diagonals: quadrature error only
        assert errs[-1][0] > 100 * out["bound_fk"][0, 0] and errs[-1][1] > 100 * out["bound_fk"][0, 2]  # quadrature, not rounding
    errs = np.array(errs)
    print("fk errors (x, z) for m = 4, 8, 16:", errs.tolist(), "of", Fx, Fz)
    assert errs[0, 0] < 0.02 * abs(Fx) and errs[0, 1] < 0.02 * abs(Fz)
    for a, b in ((0, 1), (1, 2)):
        for col in (0, 1):
            assert 3.0 <= errs[a, col] / errs[b, col] <= 5.0, (errs[a, col] / errs[b, col])


def test_wet_and_dry_bookkeeping():
    """(d) A panel is wet iff p.z - mwl <= eta (the waterline belongs to the water); a dry one contributes nothing; the ramp scales
    fk and neither buoy nor the wet test."""
    s = np.array([[0.0, 0.0, -2.0]])
    for z, mwl, wet in ((0.5, 0.0, False), (0.5, 1.0, True), (0.0, 0.0, True), (1e-9, 0.0, False)):
        out = nr.nonlinear(None, 50.0, RHO, G, [(np.array([[0.0, 0.0, z]]), s)], 0.0, np.zeros(3), np.zeros(3), mwl=mwl)
        assert bool(out["wet"][0][0]) == wet
        if wet:  # -p_s n_z = rho g (z - mwl) (-2)
            assert np.isclose(out["buoy"][0, 2], 2.0 * RHO * G * (mwl - z), rtol=1e-15, atol=0)
        else:
            assert not out["buoy"].any() and not out["fk"].any()
    A, omega, phi, t = 0.6, 1.1, 0.4, 3.3
    k = omega * omega / G
    comp = wk.regular_components(A, omega, k, phi)
    zs = np.array([-20.0, -8.0, -2.0, -0.5, 0.3, 5.0])
    c = np.stack([np.zeros_like(zs), np.zeros_like(zs), zs], axis=1)
    sv = np.tile([1.5, 0.0, 0.0], (zs.size, 1))
    x0 = 12.0
    th = k * x0 - omega * t + phi
    eta = A * np.cos(th)
    full = nr.nonlinear(comp, np.inf, RHO, G, [(c, sv)], t, [x0, 0.0, 0.0], np.zeros(3))
    half = nr.nonlinear(comp, np.inf, RHO, G, [(c, sv)], t, [x0, 0.0, 0.0], np.zeros(3), ramp=0.5)
    wet = zs <= eta
    assert list(full["wet"][0]) == list(wet) == list(half["wet"][0]) and 0 < wet.sum() < zs.size
    pd = RHO * G * A * np.exp(k * zs) * np.cos(th)
    assert np.isclose(full["fk"][0, 0], -(pd * 1.5)[wet].sum(), rtol=1e-13)
    assert np.isclose(full["fk"][0, 4], -(zs * pd * 1.5)[wet].sum(), rtol=1e-13)  # M_y = d_z F_x
    assert np.isclose(full["buoy"][0, 0], (RHO * G * zs * 1.5)[wet].sum(), rtol=1e-13)
    assert np.allclose(half["fk"], 0.5 * full["fk"], rtol=1e-15, atol=0) and np.array_equal(half["buoy"], full["buoy"])
    assert np.isclose(full["margin"], np.min(np.abs(zs - eta)), rtol=1e-12)
    assert 1e-16 * abs(full["fk"][0, 0]) < full["bound_fk"][0, 0] < 1e-9 * abs(full["fk"][0, 0])


def test_stretched_and_finite_depth_pressure_follow_the_kinematics():
    """p_d uses the kinematics' own profile and z_e: it is the x-velocity sum with w A replaced by w^2 A / k, so with every
    component's w / k set to 1 the two coincide -- stretching, second mwl subtraction and both profile branches included."""
    rng = np.random.default_rng(5)
    nf, depth = 40, 30.0
    k = np.sort(rng.uniform(0.02, 25.0, nf))
    w = k.copy()  # w / k = 1 (not a dispersion relation: an identity check of the restatement)
    comp = (rng.uniform(0.01, 0.05, nf), w, k, rng.uniform(0, 6.28, nf))
    n_long, n_finite, n_kd = wk.regimes(comp, depth)
    assert n_long > 0 and n_finite > 0 and n_kd > 0
    pts = np.column_stack([rng.uniform(-50, 50, 9), np.zeros(9), rng.uniform(-8.0, -0.5, 9)])
    for stretching in (False, True):
        for mwl in (0.0, 0.4):
            eta, pds, pabs = nr.dynamic_pressure_sum(comp, depth, pts, 2.5, mwl=mwl, stretching=stretching)
            (e, v, _), (_, vs, _) = wk.kinematics(comp, depth, pts, [2.5], mwl=mwl, stretching=stretching)
            assert np.array_equal(eta, e[0])
            assert np.allclose(pds, v[0][:, 0], rtol=1e-13, atol=0) and np.allclose(pabs, vs[0][:, 0], rtol=1e-13, atol=0)


def test_hs_linear_against_the_oracle():
    """(d) hs_lin of the restatement against the CPU oracle's hydrostatic component for the same state."""
    from cases import load_into_oracle, three_body_case
    case = three_body_case()
    orc = load_into_oracle(case)
    orc.add_waves_none()
    rng = np.random.default_rng(11)
    pos = np.array([bd["cg"] for bd in case["bodies"]], dtype=float) + rng.uniform(-0.5, 0.5, (3, 3))
    rpy = rng.uniform(-0.2, 0.2, (3, 3))
    orc.step(0.0, pos, rpy, np.zeros((3, 3)), np.zeros((3, 3)))
    want = np.asarray(orc.components()[0]).reshape(3, 6)
    got, scale = nr.hs_linear(case["rho"], [0.0, 0.0, -9.81], case["bodies"], pos, rpy)
    assert np.abs(want).max() > 1.0
    assert np.all(np.abs(got - want) <= 16 * nr.EPS * scale), np.max(np.abs(got - want) / scale)


def test_box_mesh_is_closed_and_outward():
    for m, mz in ((1, None), (3, 5)):
        c, s = nr.triangles_to_panels(nr.box_triangles([-1.0, -2.0, -3.0], [2.0, 1.0, 0.5], m=m, mz=mz))
        assert np.allclose(s.sum(axis=0), 0.0, atol=1e-13)  # closed
        assert np.isclose(np.sum(c * s) / 3.0, 3.0 * 3.0 * 3.5)  # divergence theorem: the volume, positive = outward normals
        assert len(c) == (12 if mz is None else 2 * 2 * (3 * 3 + 2 * 3 * 5))


def test_kernels_build_without_scratch_or_spills(tmp_path):
    """(e) The notes of the code object built from hc_nonlinear.hip, as tests/test_morison_ref_cpu.py reads them."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_nonlinear.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_nonlinear.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    assert any("nl_panels_kernel" in n for n in notes) and any("nl_sum_kernel" in n for n in notes), sorted(notes)
    for name, (scratch, vgpr, spills) in notes.items():
        print(name, "scratch", scratch, "vgpr", vgpr, "spills", spills)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert "hc_nonlinear.hip" in hb.SOURCES


def test_abi_declares_the_nonlinear_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_surface_panels", "hc_get_surface_panel_count", "hc_set_nonlinear_options", "hc_nonlinear_begin", "hc_nonlinear_end",
                 "hc_compute_nonlinear"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    import ctypes as C
    assert C.sizeof(capi.SurfacePanel) == 48
    assert lib.hc_nonlinear_end(None, None, None, None) == capi.HC_ERR_INVALID


def test_python_layer_converts_triangles_as_the_restatement():
    from hydrochrono_amd.hydro import triangles_to_panels
    tri = nr.box_triangles([-1.0, -2.0, -3.0], [2.0, 1.0, 0.5], m=2)
    c, s = triangles_to_panels(tri)
    c_ref, s_ref = nr.triangles_to_panels(tri)
    assert np.array_equal(c, c_ref) and np.array_equal(s, s_ref)


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/nonlinear_caller.cpp (SetSurfaceMesh / SetSurfacePanels / SetNonlinearHydroMode / SetNonlinearHydroOptions of
    include/hydroc_amd/hydro_forces.h) builds with plain g++; tests/test_gpu_nonlinear.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "nonlinear_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nonlinear_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
