"""The Morison term without a GPU: the tests' NumPy restatement (tests/morison_ref.py) against closed forms, and the build of the
kernels (csrc/hc_morison.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_morison.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import morison_ref as mr
import wave_kinematics_ref as wk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 1025.0
Z3 = np.zeros(3)


def one(r, cd, cm):
    return [(np.array([r], dtype=float), np.array([cd], dtype=float), np.array([cm], dtype=float))]


def test_one_element_in_still_water_is_quadratic_drag():
    v = np.array([0.7, -1.3, 0.4])
    cd = np.array([2.0, 0.5, 1.25])
    r = np.array([0.0, 0.0, -3.0])
    out = mr.morison(None, 50.0, RHO, one(r, cd, [1.0, 1.0, 1.0]), 1.0, Z3, Z3, v, Z3)
    F = -0.5 * RHO * cd * np.abs(v) * v
    assert np.allclose(out["F"][0, :3], F, rtol=1e-15, atol=0)
    assert np.allclose(out["F"][0, 3:], np.cross(r, F), rtol=1e-15, atol=0)
    assert out["wet"][0].all() and out["margin"] == 3.0
    assert np.all(out["bound"] > 0) and np.all(out["bound"][0, :3] < 1e-12 * np.abs(F).max())


def test_dry_element_gives_zero_and_the_waterline_belongs_to_the_water():
    v = np.array([1.0, 1.0, 1.0])
    for z, mwl, wet in ((0.5, 0.0, False), (0.5, 1.0, True), (0.0, 0.0, True), (1e-9, 0.0, False)):
        out = mr.morison(None, 50.0, RHO, one([0, 0, z], [1, 1, 1], [0, 0, 0]), 0.0, Z3, Z3, v, Z3, mwl=mwl)
        assert bool(out["wet"][0][0]) == wet
        assert bool(out["F"].any()) == wet


def test_single_axis_rotations_are_the_textbook_matrices():
    a = 0.37
    s, c = np.sin(a), np.cos(a)
    Rx = [[1, 0, 0], [0, c, -s], [0, s, c]]
    Ry = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    Rz = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    for axis, M in enumerate((Rx, Ry, Rz)):
        rpy = np.zeros(3)
        rpy[axis] = a
        assert np.allclose(np.asarray(mr.rotation(rpy), dtype=float), M, rtol=0, atol=1e-16)
    R = np.asarray(mr.rotation([0.3, -0.4, 1.1]), dtype=float)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0)
    assert np.allclose(R, np.asarray(mr.rotation([0.3, 0, 0]) @ mr.rotation([0, -0.4, 0]) @ mr.rotation([0, 0, 1.1]), dtype=float), atol=1e-15)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pure_rotation_about_each_axis(axis):
    """The body spins about one world axis through its reference (attitude tilted about the same axis): v_e = w x d, the drag acts
    per BODY axis against it, M = d x F."""
    w = np.zeros(3)
    w[axis] = 0.8
    rpy = np.zeros(3)
    rpy[axis] = 0.6
    r = np.array([1.5, -2.0, -4.0])
    cd = np.array([1.0, 2.0, 3.0])
    pos = np.array([0.0, 0.0, -10.0])
    out = mr.morison(None, 50.0, RHO, one(r, cd, [0, 0, 0]), 2.0, pos, rpy, Z3, w)
    R = np.asarray(mr.rotation(rpy), dtype=float)
    d = R @ r
    u = R.T @ (-np.cross(w, d))
    F = R @ (0.5 * RHO * cd * np.abs(u) * u)
    assert np.allclose(out["F"][0, :3], F, rtol=1e-13, atol=1e-9)
    assert np.allclose(out["F"][0, 3:], np.cross(d, F), rtol=1e-13, atol=1e-9)
    assert abs(u[axis]) < 1e-12 and abs(out["F"][0, axis]) < 1e-9  # no flow along the spin axis
    assert np.dot(out["F"][0, 3:], w) < 0  # the moment opposes the spin


def test_deep_water_regular_wave_on_a_fixed_vertical_stack():
    g, A, omega, phi, x0, t = 9.81, 0.6, 1.1, 0.4, 12.0, 3.3
    k = omega * omega / g
    comp = wk.regular_components(A, omega, k, phi)
    zs = np.array([-20.0, -8.0, -2.0, -0.5, 5.0])
    n = zs.size
    r = np.stack([np.zeros(n), np.zeros(n), zs], axis=1)
    cd, cm = np.tile([1.2, 1.2, 0.3], (n, 1)), np.tile([2.0, 2.0, 0.0], (n, 1))
    out = mr.morison(comp, np.inf, RHO, [(r, cd, cm)], t, [x0, 0.0, 0.0], Z3, Z3, Z3)
    th = k * x0 - omega * t + phi
    prof = np.exp(k * zs)
    ux, uz = omega * A * prof * np.cos(th), omega * A * prof * np.sin(th)
    ax = omega ** 2 * A * prof * np.sin(th)
    wet = zs <= A * np.cos(th)
    assert list(wet) == [True, True, True, True, False] and list(out["wet"][0]) == list(wet)
    Fx = np.where(wet, 0.5 * RHO * 1.2 * np.abs(ux) * ux + RHO * 2.0 * ax, 0.0)
    Fz = np.where(wet, 0.5 * RHO * 0.3 * np.abs(uz) * uz, 0.0)
    assert np.allclose(out["F"][0, 0], Fx.sum(), rtol=1e-13)
    assert out["F"][0, 1] == 0.0
    assert np.allclose(out["F"][0, 2], Fz.sum(), rtol=1e-13)
    assert np.allclose(out["F"][0, 4], np.sum(zs * Fx), rtol=1e-13)  # M_y = d_z F_x - d_x F_z, d_x = 0
    # the bound follows the kinematics tolerance: far below the force, above its rounding
    assert 1e-16 * abs(Fx.sum()) < out["bound"][0, 0] < 1e-9 * abs(Fx.sum())
    # half the ramp: velocities and accelerations halve, the wet test does not move
    half = mr.morison(comp, np.inf, RHO, [(r, cd, cm)], t, [x0, 0.0, 0.0], Z3, Z3, Z3, ramp=0.5)
    Fxh = np.where(wet, 0.5 * RHO * 1.2 * np.abs(ux) * ux * 0.25 + RHO * 2.0 * ax * 0.5, 0.0)
    assert np.allclose(half["F"][0, 0], Fxh.sum(), rtol=1e-13) and list(half["wet"][0]) == list(wet)


def test_ramp_factor():
    assert mr.ramp_factor(-1.0, 60.0) == 0.0 and mr.ramp_factor(0.0, 60.0) == 0.0
    assert mr.ramp_factor(15.0, 60.0) == 0.25
    assert mr.ramp_factor(60.0, 60.0) == 1.0 and mr.ramp_factor(61.0, 60.0) == 1.0
    assert mr.ramp_factor(-1.0, 0.0) == 1.0 and mr.ramp_factor(5.0, 0.0) == 1.0  # no ramp configured


def test_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_morison.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_morison.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    assert any("morison_items_kernel" in n for n in notes) and any("morison_sum_kernel" in n for n in notes), sorted(notes)
    for name, (scratch, vgpr, spills) in notes.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert "hc_morison.hip" in hb.SOURCES


def test_abi_declares_the_morison_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_morison_elements", "hc_get_morison_count", "hc_set_morison_options", "hc_morison_begin", "hc_morison_end",
                 "hc_compute_morison"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    import ctypes as C
    assert C.sizeof(capi.MorisonElement) == 72
    assert lib.hc_morison_end(None, None) == capi.HC_ERR_INVALID


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/morison_caller.cpp (SetMorisonElements / SetMorisonOptions / ComputeForceMorison of include/hydroc_amd/hydro_forces.h)
    builds with plain g++; tests/test_gpu_morison.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "morison_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
