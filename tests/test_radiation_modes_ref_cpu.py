"""The modal radiation term without a GPU: the tests' longdouble restatement (tests/radiation_modes_ref.py) against closed forms,
the host helpers (hydrochrono_amd/radiation_modes.py: fit and state-space conversion), the ring bookkeeping (csrc/hc_modal_ring.hpp
through tests/cpp/modal_ring_test.cpp), the ABI and the build of the kernel (csrc/hc_radiation_modes.hip: no scratch, no spilled
register).  The GPU side is tests/test_gpu_radiation_modes.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import radiation_modes_ref as rm
from radiation_modes_ref import expm_taylor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def irregular_times(n, seed, h_lo=1e-3, h_hi=0.3):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.0], np.cumsum(np.exp(rng.uniform(np.log(h_lo), np.log(h_hi), size=n)))])


def test_phi_functions_at_both_ends():
    for x in (1e-12, -1e-9, 1e-5j, -0.3 + 0.2j, -0.49, -0.5, -0.51 + 0.0j, -3.0 + 7.0j, -800.0, -800.0 + 5.0j):
        p1, p2 = rm.phi12(x)
        assert np.isfinite(complex(p1)) and np.isfinite(complex(p2))
        x = rm.CLD(x)
        if abs(x) >= 0.5:  # against the series pushed far beyond its threshold where it still converges fast enough
            continue
        e = np.exp(x)
        # (e - 1) / x loses |x|^-1 of the longdouble precision, (e - 1 - x) / x^2 loses |x|^-2: still a check near the threshold
        if abs(x) > 0.1:
            assert abs(p1 - (e - 1) / x) < 1e-17 and abs(p2 - (e - 1 - x) / (x * x)) < 1e-16
    p1, p2 = rm.phi12(1e-12)
    assert abs(complex(p1) - 1.0) < 1e-12 and abs(complex(p2) - 0.5) < 1e-12
    p1, p2 = rm.phi12(-800.0)
    assert abs(complex(p1) - 1.0 / 800.0) < 1e-18 and abs(complex(p2) - (1.0 / 800.0 - 1.0) / -800.0) < 1e-18
    # the two branches meet: just below and just above the threshold
    lo, hi = rm.phi12(-0.5 + 1e-15), rm.phi12(-0.5)
    assert abs(lo[0] - hi[0]) < 1e-15 and abs(lo[1] - hi[1]) < 1e-15


def test_linear_velocity_is_reproduced_whatever_the_steps():
    """v = a + b t from z(0) = 0: z(t) = a t phi1(lambda t) + b t^2 phi2(lambda t) after 200 irregular steps, h = 1e-9 and
    |Re lambda h| = 800 among them.  Tolerance: 200 steps of some 50 longdouble roundings each, 200 * 50 * 1.1e-19 = 1.1e-15 of
    the largest |z| on the way."""
    a, b = 0.7, -0.4
    t = list(irregular_times(196, 3))
    t += [t[-1] + 1e-9, t[-1] + 2e-9, t[-1] + 2e-9 + 0.01]
    lams = [-0.8, -0.3 + 2.0j, -2.5 - 0.7j, -5.0 + 40.0j]
    # one step with |Re lambda h| = 800 for the first mode, then one more ordinary step
    t += [t[-1] + 800.0 / 0.8, t[-1] + 800.0 / 0.8 + 0.05]
    assert len(t) == 202
    ref = rm.ModalRef([[(0, lam, 1.0) for lam in lams]])
    zmax = 0.0
    for tn in t:
        ref.step(tn, [a + b * tn])
        z = ref.snaps[-1][2][0]
        for lam, zn in zip(lams, z):
            want = rm.z_linear(lam, a, b, tn)
            zmax = max(zmax, float(abs(want)))
            assert abs(zn - want) <= 1.1e-15 * max(zmax, 1e-30), (tn, lam, complex(zn), complex(want))
    assert ref.steps == 201 and zmax > 100.0


def test_sine_velocity_stays_within_the_interpolation_bound():
    """v = sin(omega t) on a uniform and on an irregular grid: the row sum against the analytic integral, within
    (omega h)^2 / 8 * v_max * sum |rho| / |Re lambda| (piecewise-linear interpolation of v, the integral of e^{Re lambda s})."""
    omega = 1.3
    modes = [(-0.5, 2.0), (-0.2 + 1.1j, 1.0 - 0.5j), (-1.5 - 3.0j, 0.3 + 0.8j)]
    scale = sum(abs(rho) / abs(complex(lam).real) for lam, rho in modes)
    for times in (0.05 * np.arange(300), irregular_times(300, 7, 1e-3, 0.08)):
        ref = rm.ModalRef([[(0, lam, rho) for lam, rho in modes]])
        hmax = float(np.max(np.diff(times)))
        bound = (omega * hmax) ** 2 / 8.0 * 1.0 * scale
        worst = 0.0
        for tn in times:
            got = ref.step(tn, [np.sin(omega * tn)])[0]
            want = sum((rm.CLD(rho) * rm.z_sine(lam, omega, tn)).real for lam, rho in modes)
            worst = max(worst, float(abs(got - want)))
        assert 0.0 < worst <= bound, (worst, bound)
        assert worst > 1e-3 * bound  # the bound is not vacuous


def test_reference_ring_semantics():
    ref = rm.ModalRef([[(0, -1.0, 1.0)]], depth=3)
    for tn in (0.0, 0.1, 0.2, 0.3, 0.4):
        ref.step(tn, [1.0])
    with pytest.raises(rm.DuplicateTime):
        ref.step(0.4, [1.0])
    with pytest.raises(rm.NoSnapshot):
        ref.step(0.15, [1.0])  # depth 3 keeps 0.2, 0.3, 0.4
    a = ref.step(0.35, [1.0])[0]  # 0.4 goes, from 0.3
    fresh = rm.ModalRef([[(0, -1.0, 1.0)]], depth=3)
    for tn in (0.0, 0.1, 0.2, 0.3):
        fresh.step(tn, [1.0])
    assert a == fresh.step(0.35, [1.0])[0]


def test_fit_recovers_three_known_modes():
    """K sampled from one real pole and two conjugate pairs; fit_radiation_modes recovers K.  The residual against the known K,
    measured here: max |K_fit - K| = 3.4e-14 of max |K| (order 5 = 1 + 2 + 2, three modes found); the test allows ten times that."""
    from hydrochrono_amd.radiation_modes import fit_radiation_modes, modes_irf
    known = [(-0.6, 1.5), (-0.25 + 1.4j, 2.0 - 0.6j), (-0.9 + 3.1j, -0.7 + 0.4j)]
    t = 0.05 * np.arange(400)
    K = modes_irf(known, t)
    modes, r2 = fit_radiation_modes(K, t, max_order=8, r2_min=1.0 - 1e-12)
    resid = float(np.max(np.abs(modes_irf(modes, t) - K)) / np.max(np.abs(K)))
    print(f"fit residual {resid:.3e}, R^2 deficit {1.0 - r2:.3e}, modes {len(modes)}")
    assert len(modes) == 3 and r2 >= 1.0 - 1e-12
    assert resid <= 10 * 3.4e-14  # measured 3.339e-14
    # the poles themselves
    for lam, rho in known:
        near = min(modes, key=lambda m: abs(m[0] - lam))
        assert abs(near[0] - lam) < 1e-8 and abs(near[1] - rho) < 1e-8
    # between the samples as well: the modes are a continuous-time model
    tf = 0.0125 * np.arange(1600)
    assert np.max(np.abs(modes_irf(modes, tf) - modes_irf(known, tf))) < 1e-8


def test_state_space_to_modes_agrees_with_the_matrix_exponential():
    from hydrochrono_amd.radiation_modes import modes_irf, state_space_to_modes
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4, 7):
        A = rng.normal(size=(n, n)) - (1.5 + np.sqrt(n)) * np.eye(n)
        B, C = rng.normal(size=n), rng.normal(size=n)
        modes = state_space_to_modes(A, B, C)
        assert all(lam.real < 0 for lam, _ in modes) and len(modes) <= n
        for tau in (0.0, 0.013, 0.4, 2.5):
            want = float(np.asarray(C, dtype=LD) @ expm_taylor(A, tau) @ np.asarray(B, dtype=LD))
            got = float(modes_irf(modes, [tau])[0])
            assert abs(got - want) <= 1e-12 * max(1.0, np.abs(B).max() * np.abs(C).max() * n), (n, tau, got, want)
    with pytest.raises(ValueError, match="defective"):
        state_space_to_modes([[-1.0, 1.0], [0.0, -1.0]], [0.0, 1.0], [1.0, 0.0])
    with pytest.raises(ValueError, match="unstable"):
        state_space_to_modes([[0.1, 0.0], [0.0, -1.0]], [1.0, 1.0], [1.0, 1.0])
    with pytest.raises(ValueError, match="unstable"):
        state_space_to_modes([[0.0, 1.0], [-1.0, 0.0]], [1.0, 1.0], [1.0, 1.0])  # poles on the imaginary axis


def test_abi_declares_the_radiation_modes_entry_points():
    import ctypes as C

    from hydrochrono_amd import capi
    lib = capi.load()
    names = ("hc_set_radiation_modes", "hc_get_radiation_mode_count", "hc_set_radiation_modes_depth", "hc_radiation_modes_begin",
             "hc_radiation_modes_end", "hc_compute_radiation_modes", "hc_reset_radiation_modes", "hc_get_radiation_modes_irf")
    header = open(os.path.join(ROOT, "include", "hydrochrono_amd.h")).read()
    for name in names:
        assert name in capi.SIGNATURES and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "hc_radiation_mode;" in header and C.sizeof(capi.RadiationMode) == 40
    z = (C.c_double * 3)()
    n = C.c_int()
    mode = capi.RadiationMode(0, 0, -1.0, 0.0, 1.0, 0.0)
    assert lib.hc_set_radiation_modes(None, 0, C.byref(mode), 1) == capi.HC_ERR_INVALID
    assert lib.hc_get_radiation_mode_count(None, 0, C.byref(n)) == capi.HC_ERR_INVALID
    assert lib.hc_set_radiation_modes_depth(None, 4) == capi.HC_ERR_INVALID
    assert lib.hc_radiation_modes_begin(None, 0.0, z, z) == capi.HC_ERR_INVALID
    assert lib.hc_radiation_modes_end(None, z) == capi.HC_ERR_INVALID
    assert lib.hc_compute_radiation_modes(None, 0.0, z, z, z) == capi.HC_ERR_INVALID
    assert lib.hc_reset_radiation_modes(None) == capi.HC_ERR_INVALID
    assert lib.hc_get_radiation_modes_irf(None, 0, 1, z, z) == capi.HC_ERR_INVALID
    limits = open(os.path.join(ROOT, "hydrochrono_amd", "csrc", "hc_limits.hpp")).read()
    assert re.search(r"kRadiationModesMaxPerPair\s*=\s*16\b", limits)


def test_ring_bookkeeping_unit_test(tmp_path):
    exe = str(tmp_path / "modal_ring_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "modal_ring_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    assert r.stdout.splitlines()[-1] == "0 failures"


def test_kernel_builds_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_radiation_modes.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_radiation_modes.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    assert any("radiation_modes_kernel" in n for n in notes), sorted(notes)
    for name, (scratch, vgpr, spills) in notes.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert "hc_radiation_modes.hip" in hb.SOURCES and "hc_modal_ring.hpp" in hb.HEADERS


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/radiation_modes_caller.cpp (SetRadiationModes / ComputeForceRadiationModes of include/hydroc_amd/hydro_forces.h)
    builds with plain g++; tests/test_gpu_radiation_modes.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "radiation_modes_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "radiation_modes_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
