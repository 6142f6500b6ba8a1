"""The NumPy restatement of the second-order waves in a short-crested sea (tests/wave2_dir_ref.py) checked without trusting the
formulas it was written from, before any kernel: the second-order free-surface conditions, Laplace's equation in three dimensions and
the bed condition by difference quotients of its own fields; its reduction to the long-crested restatement (tests/wave2_ref.py) for
equal directions; the sum-frequency potential of an infinite depth, zero unless two components cross; the error a plain FP64
evaluation makes on every input set of the GPU tests; the build of the kernels and the entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_wave2_ref_cpu as lc  # solve_k, d1, d2 and the oracle's components, as the long-crested checks use them
import wave2_dir_inputs as di
import wave2_dir_ref as wd
import wave2_ref as w2

LD = np.longdouble
G = 9.81
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA3 = np.array([-0.6, 0.2, 0.9])


def sea3(depth):
    A = np.array([1.0, 0.7, 0.4])
    w = np.array([0.6, 0.85, 1.3])
    return (A, w, lc.solve_k(w, depth), np.array([0.3, 1.1, -0.7]))


@pytest.mark.parametrize("depth", [8.0, 30.0, np.inf])
def test_free_surface_conditions_laplace_and_bed(depth):
    """The conditions of tests/test_wave2_ref_cpu.py with x and y derivatives, for three components at -0.6, 0.2 and 0.9 rad.
    At z = 0:  phi2_tt + g phi2_z = -d/dt |grad phi1|^2 + (phi1_t / g) d/dz (phi1_tt + g phi1_z)  and
    eta2 = -(phi2_t + 1/2 |grad phi1|^2 + eta1 phi1_zt) / g;  phi2_xx + phi2_yy + phi2_zz = 0 at a submerged point, no flow through
    the bed.  The tolerance is derived there: the quotients' truncation d^4 rho^6 / 30 and rounding eps / d^2, below 1e-8 of the
    sum M of the |terms|."""
    comp = sea3(depth)
    A, w, k, _ = comp
    d = LD(1e-3)
    eps = np.finfo(LD).eps
    rho = float(max(2 * w[-1], 2 * k[-1], 1.0))
    slack = 20 * float(d) ** 4 * rho ** 6 + 200 * float(eps) / float(d) ** 2
    assert slack < 1e-8
    d1, d2 = lc.d1, lc.d2

    def f2(idx):
        return lambda x, y, z, t: wd.fields(comp, BETA3, G, depth, [[x, y, z]], [t], clamp=False)[0][idx][0, 0]

    eta1 = lambda x, y, z, t: wd.first_order(comp, BETA3, G, depth, x, y, z, t)[0]
    phi1 = lambda x, y, z, t: wd.first_order(comp, BETA3, G, depth, x, y, z, t)[1]
    eta2, phi2 = f2(0), f2(3)
    X, Y, Z, T = 0, 1, 2, 3
    grad2 = lambda *a: d1(phi1, X, d)(*a) ** 2 + d1(phi1, Y, d)(*a) ** 2 + d1(phi1, Z, d)(*a) ** 2
    lin = lambda *a: d2(phi1, T, d)(*a) + G * d1(phi1, Z, d)(*a)  # (zero at z = 0; its z derivative is not)
    tabs, _ = wd.pair_tables(comp, BETA3, G, depth)
    geo = wd.pair_geometry(comp, BETA3)
    kap = {s: geo[s][0] for s in "mp"}
    Om = {s: np.abs(geo[s][3]) for s in "mp"}
    M_kin = sum(np.sum(np.abs(tabs["B" + s]) * (Om[s] ** 2 + G * kap[s])) for s in "mp")
    M_eta = np.sum(0.25 * np.outer(A, A) * (np.abs(tabs["Km"]) + np.abs(tabs["Kp"])))
    M_lap = sum(np.sum(np.abs(tabs["B" + s]) * 2 * kap[s] ** 2) for s in "mp")
    M_bed = sum(np.sum(np.abs(tabs["B" + s]) * kap[s]) for s in "mp")
    assert M_kin > 0.01 and M_eta > 0.01
    for x, y, t in ((LD(1.7), LD(-3.1), LD(2.3)), (LD(-40.0), LD(23.0), LD(11.9))):
        a0 = (x, y, LD(0), t)
        lhs = d2(phi2, T, d)(*a0) + G * d1(phi2, Z, d)(*a0)
        rhs = -d1(grad2, T, d)(*a0) + d1(phi1, T, d)(*a0) / G * d1(lin, Z, d)(*a0)
        assert abs(lhs - rhs) <= slack * M_kin, (depth, float(lhs), float(rhs))
        assert abs(lhs) > 1e-3 * M_kin  # (the condition is not met by zeros)
        e2 = -(d1(phi2, T, d)(*a0) + grad2(*a0) / 2 + eta1(*a0) * d1(d1(phi1, Z, d), T, d)(*a0)) / G
        assert abs(e2 - eta2(*a0)) <= slack * M_eta, (depth, float(e2), float(eta2(*a0)))
        a1 = (x, y, LD(-2.5), t)
        lap = d2(phi2, X, d)(*a1) + d2(phi2, Y, d)(*a1) + d2(phi2, Z, d)(*a1)
        assert abs(lap) <= slack * M_lap, (depth, float(lap))
        assert abs(d2(phi2, Y, d)(*a1)) > 1e-4 * M_lap  # (y takes part)
        if np.isfinite(depth):
            assert abs(d1(phi2, Z, d)(x, y, LD(-depth), t)) <= slack * M_bed
    # the fields the library returns are these derivatives of phi2 (at a submerged point, where nothing is held)
    a1 = (LD(1.7), LD(-3.1), LD(-2.5), LD(2.3))
    (_, vel, acc, _), (_, vs, as_, _) = wd.fields(comp, BETA3, G, depth, [a1[:3]], [a1[3]])
    for col, var in ((0, X), (1, Y), (2, Z)):
        assert abs(d1(phi2, var, d)(*a1) - vel[0, 0, col]) <= slack * rho * vs[0, 0, col]
        assert abs(d1(d1(phi2, var, d), T, d)(*a1) - acc[0, 0, col]) <= slack * rho * rho * as_[0, 0, col]
        assert abs(vel[0, 0, col]) > 1e-3 * vs[0, 0, col]


@pytest.mark.parametrize("depth", [8.0, 30.0, np.inf])
def test_equal_directions_are_the_long_crested_sea(depth):
    comp = tuple(np.asarray(v, dtype=np.float64) for v in sea3(depth))  # FP64 component data, as the library holds it
    pts = np.array([[1.7, -3.1, -2.5], [-40.0, 23.0, 0.0], [12.0, 30.0, -7.0], [5.0, 5.0, 1.0]])
    times = [2.3, 11.9]
    cut = dict(diff_band=(0.2, 0.6), sum_band=(1.3, 2.3))
    for kw in ({}, cut, dict(mwl=0.4, ramp_duration=20.0)):
        want, scale = w2.fields(comp, G, depth, pts, times, **kw)
        got, gscale = wd.fields(comp, np.zeros(3), G, depth, pts, times, **kw)
        for a, b, s, sg in zip(got, want, scale, gscale):
            assert np.all(np.abs(a - b) <= 1e-13 * s) and np.all(np.abs(sg - s) <= 1e-13 * s)
        assert np.abs(got[1][..., 0]).max() > 0 and not got[1][..., 1].any() and not got[2][..., 1].any()
        none, _ = wd.fields(comp, None, G, depth, pts, times, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(none, got))
    ta, tm = wd.pair_tables(comp, np.zeros(3), G, depth)
    tb, _ = w2.pair_tables(comp, G, depth)
    for n in ta:
        assert np.all(np.abs(ta[n] - tb[n]) <= 1e-15 * (np.abs(tb[n]) + tm[n])), n
    for beta in (0.7, -2.9):
        c, s = LD(np.cos(beta)), LD(np.sin(beta))  # the FP64 unit vector, as the restatement takes it
        turned = np.stack([pts[:, 0].astype(LD) * c + pts[:, 1].astype(LD) * s, np.zeros(4, dtype=LD), pts[:, 2].astype(LD)], axis=1)
        want, scale = w2.fields(comp, G, depth, turned, times)  # (it rounds the turned x to FP64: 1e-16 |k x| of a phase)
        got, _ = wd.fields(comp, np.full(3, beta), G, depth, pts, times)
        assert np.all(np.abs(got[0] - want[0]) <= 1e-13 * scale[0]) and np.all(np.abs(got[3] - want[3]) <= 1e-13 * scale[3])
        for a, b, sc in zip(got[1:3], want[1:3], scale[1:3]):
            back = np.stack([b[..., 0] * c, b[..., 0] * s, b[..., 2]], axis=-1)  # the horizontal vector turned back by +beta
            hs = np.stack([sc[..., 0], sc[..., 0], sc[..., 2]], axis=-1)
            assert np.all(np.abs(a - back) <= 1e-13 * hs)
        assert np.abs(got[1][..., 1]).max() > 1e-3 * float(scale[1][..., 0].max())


def test_infinite_depth_sum_potential_exists_only_where_components_cross():
    w = np.array([0.6, 0.85, 1.3])
    comp = (np.array([1.0, 0.7, 0.4]), w, w * w / G, np.array([0.3, 1.1, -0.7]))  # k = R bit for bit: delta = 0
    for beta in (np.zeros(3), np.full(3, 0.9), np.full(3, -2.0)):
        tabs, _ = wd.pair_tables(comp, beta, G, np.inf)
        assert np.array_equal(tabs["Bp"], np.zeros((3, 3)))
        (_, vel, _, _), _ = wd.fields(comp, beta, G, np.inf, [[1.0, 2.0, -1.0]], [0.5], diff_band=(100.0, 200.0))
        assert not vel.any()
    beta = np.array([-0.6, 0.2, 0.9])
    tabs, _ = wd.pair_tables(comp, beta, G, np.inf)
    A, wl = comp[0].astype(LD), w.astype(LD)
    R = (w * w / G).astype(LD)
    r = np.sqrt(R)
    sig = np.sin((beta[:, None].astype(LD) - beta[None, :].astype(LD)) / 2) ** 2
    kp = np.sqrt(R[:, None] ** 2 + R[None, :] ** 2 + 2 * R[:, None] * R[None, :] * (1 - 2 * sig))
    rs2 = (r[:, None] + r[None, :]) ** 2
    Dp = -4 * sig * rs2 * R[:, None] * R[None, :] / (rs2 - kp)
    Bp = 0.25 * (A * LD(G) / wl)[:, None] * (A * LD(G) / wl)[None, :] * Dp / (wl[:, None] + wl[None, :])
    off = ~np.eye(3, dtype=bool)
    assert np.all(np.abs(tabs["Bp"][off]) > 1e-3) and np.array_equal(np.diag(tabs["Bp"]), np.zeros(3))
    assert np.all(np.abs(tabs["Bp"] - Bp) <= 1e-14 * np.abs(Bp))  # (the unit vectors are FP64: sigma to 1e-16 / |beta_i - beta_j|)
    (_, vel, _, _), _ = wd.fields(comp, beta, G, np.inf, [[1.0, 2.0, -1.0]], [0.5], diff_band=(100.0, 200.0))
    assert np.all(np.abs(vel) > 1e-4)


def oracle_components(name):
    case = di.case_of(name)
    orc = lc.load_into_oracle(case)
    orc.add_waves_irregular(**di.SETS[name][1])
    from wave_kinematics_ref import irregular_components
    return irregular_components(orc.irreg_spectrum()), case


@pytest.mark.parametrize("name", sorted(di.SETS))
def test_plain_fp64_reaches_the_tolerance(name):
    """The GPU tests allow TOL * sum|term| (fields) and TOL * (|ref| + sum|addends|) (tables).  The same restatement evaluated in
    float64 stays within that on every input set they use, under every choice of bands."""
    comp, case = oracle_components(name)
    beta = di.directions(name)
    assert comp[0].size == di.SETS[name][1]["nfrequencies"] == beta.size and np.all(np.isfinite(comp[0])) and np.all(comp[1] > 0)
    g, depth = case["g"], case["water_depth"]
    for bands in di.BANDS:
        ref, mag = di.reference_tables(name, bands, di.key(comp), g, depth)
        dbl, _ = di.reference_tables(name, bands, di.key(comp), g, depth, np.float64)
        for n in ref:
            assert np.all(np.isfinite(dbl[n])), (bands, n)
            worst = np.max(np.abs(dbl[n] - ref[n]) / np.maximum(np.abs(ref[n]) + mag[n], 1e-300))
            print(f"{name} {bands} table {n}: float64 off by {float(worst):.2e} of |ref| + sum|addends|")
            assert worst <= di.TOL, (bands, n, float(worst))
        vals, scales = di.reference(name, bands, di.key(comp), g, depth)
        dvals, _ = di.reference(name, bands, di.key(comp), g, depth, np.float64)
        for v, dv, s, what in zip(vals[:3], dvals[:3], scales[:3], ("eta2", "vel2", "acc2")):
            assert np.all(np.isfinite(dv)), (bands, what)
            worst = np.max(np.abs(dv - v) / np.maximum(s, 1e-300)) if v.size else 0.0
            print(f"{name} {bands} {what}: float64 off by {float(worst):.2e} of sum|term|")
            assert np.all(np.abs(dv - v) <= di.TOL * s), (bands, what, float(worst))
            if bands == "empty":
                assert not v.any() and not s.any()
        if bands == "full":
            assert np.abs(vals[1][..., 1]).max() > 0 and np.abs(vals[2][..., 1]).max() > 0  # the y components are there


def test_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf not found"
    from hydrochrono_amd import build as hb
    # the directional kernels are the <true, ...> instantiations of csrc/hc_wave_kin2.hip (ILb1E in the symbol)
    co = str(tmp_path / "hc_wave_kin2.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_wave_kin2.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(2): (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(1))) for m in re.finditer(
        r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
        r".*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    notes = {n: v for n, v in notes.items() if "wk2_pair_kernelILb1E" in n or "wk2_sum_kernelILb1E" in n}
    assert sum("wk2_pair_kernel" in n for n in notes) == 1 and sum("wk2_sum_kernel" in n for n in notes) == 3, sorted(notes)
    for name, (scratch, vgpr, spills, lds) in sorted(notes.items()):
        print(f"{name}: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert lds <= 160 * 1024 // 3, (name, lds)  # three workgroups per CU
        assert vgpr <= 512 // 3, (name, vgpr)       # and the registers of a SIMD hold as many of its waves
    assert "hc_wave_kin2.hip" in hb.SOURCES and "hc_wave_kin2_dir.hpp" in hb.HEADERS


def test_abi_declares_the_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "hydrochrono_amd.h")).read()
    for name in ("hc_wave_kinematics2_dir", "hc_wave_kinematics2_dir_pair_tables"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert lib.hc_wave_kinematics2_dir(None, None, 0, None, 0, None, None, None, None) == capi.HC_ERR_INVALID
    assert lib.hc_wave_kinematics2_dir_pair_tables(None, None, None, None, None, None) == capi.HC_ERR_INVALID


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/wave2_dir_caller.cpp (WaveBase::GetDirectionalSecondOrder* of include/hydroc_amd/wave_types.h) builds with plain
    g++; tests/test_gpu_wave_kinematics2_dir.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "wave2_dir_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "wave2_dir_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
