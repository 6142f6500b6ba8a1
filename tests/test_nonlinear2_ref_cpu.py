"""The nonlinear surface forces on the second-order sea without a GPU: the definition itself (the pressure at the second-order free
surface is of third order), the tests' NumPy restatement (tests/nonlinear2_ref.py) against a difference quotient of wave2_ref's
potential and against Stokes' closed form, the input sets of the GPU tests, and the build of the new kernels (csrc/hc_nonlinear.hip:
no scratch, no spilled register).  The GPU side is tests/test_gpu_nonlinear2.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import nonlinear2_inputs as ni
import nonlinear2_ref as n2
import wave2_ref as w2
import wave_kinematics_ref as wk
from cases import load_into_oracle
from morison_ref import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81


def solve_k(w, depth):
    k = w * w / G
    if np.isinf(depth):
        return k
    for _ in range(200):
        k = w * w / (G * np.tanh(k * depth))
    return k


# three components shorter than 30 m (2 pi / k < depth for each: the first-order profile is the finite-depth one, the reference's
# exponential-profile test trips for none) -- checked below
W3 = np.array([1.6, 1.9, 2.3])
A3 = np.array([0.10, 0.075, 0.05])
PHI3 = np.array([0.3, 1.1, -0.7])


@pytest.mark.parametrize("depth", [np.inf, 30.0])
def test_pressure_at_the_second_order_free_surface_is_of_third_order(depth):
    """p_s + p_d at z = mwl + eta1 + eta2 over rho g sum|A| (of the first sea) falls by 6 .. 10 per halving of the amplitudes (third order: 8); without
    the second-order terms -- p_s + ramp p_d1 at z = mwl + eta1 -- it falls by 3 .. 5 (second order: 4).  No stretching."""
    k = solve_k(W3, depth)
    if np.isfinite(depth):
        assert np.all(2 * np.pi / k < depth) and np.all(k * depth < 500.0)
    mwl = 0.25
    for x, t in ((3.0, 1.7), (-11.0, 4.4), (27.5, 9.1), (0.4, 13.3)):
        res2, res1 = [], []
        for halvings in range(4):
            comp = (A3 / 2.0 ** halvings, W3, k, PHI3)
            scale = LD(RHO) * LD(G) * LD(np.sum(np.abs(A3)))  # of the sea before the halvings: a unit, the same for every row
            at0 = n2.point_terms(comp, G, depth, [[x, 0.0, mwl]], t, mwl=mwl)
            for order2, out in ((True, res2), (False, res1)):
                eta = at0["eta"][0] if order2 else LD(at0["eta1"][0])
                z = float(LD(mwl) + eta)
                r = n2.point_terms(comp, G, depth, [[x, 0.0, z]], t, mwl=mwl, second_order=order2)
                ps = -LD(RHO) * LD(G) * (LD(z) - LD(mwl))
                out.append(abs(float((ps + LD(RHO) * r["pds"][0]) / scale)))
        ratios2 = [res2[i] / res2[i + 1] for i in range(3)]
        ratios1 = [res1[i] / res1[i + 1] for i in range(3)]
        print(f"depth {depth} x {x} t {t}: order 2 residues {res2} ratios {ratios2}; order 1 residues {res1} ratios {ratios1}")
        assert all(6.0 <= r <= 10.0 for r in ratios2), ratios2
        assert all(3.0 <= r <= 5.0 for r in ratios1), ratios1


@pytest.mark.parametrize("depth", [np.inf, 30.0])
def test_q2_is_minus_the_time_derivative_of_the_second_order_potential(depth):
    """q2 against a five-point difference quotient of wave2_ref.fields' own phi2 (step 1e-3 s: its truncation (Omega h)^4 / 30 is below
    2e-11 of a term at Omega = 4.6 rad/s), to 1e-8 of the sum of |terms|; above the mean level, below it and at the bed; with bands."""
    k = solve_k(W3, depth)
    comp = (A3, W3, k, PHI3)
    pts = np.array([[3.0, 0.0, 1.2], [-7.0, 0.0, -0.4], [12.0, 0.0, -6.0], [1.0, 0.0, -30.0 + 0.25]])
    t, h = 2.9, 1e-3
    for bands in (dict(), dict(diff_band=(0.2, 0.5), sum_band=(3.6, 4.3))):
        q2, scale = n2.q2_field(comp, G, depth, pts, t, mwl=0.25, **bands)
        phi = {m: w2.fields(comp, G, depth, pts, [t + m * h], mwl=0.25, **bands)[0][3][0] for m in (-2, -1, 1, 2)}
        dphi = (-phi[2] + 8 * phi[1] - 8 * phi[-1] + phi[-2]) / (12 * LD(h))
        err = np.abs(q2 + dphi) / scale
        print("depth", depth, bands, "worst |q2 + d phi2 / dt| / sum|terms|:", float(err.max()))
        assert np.all(scale > 0) and np.all(err <= 1e-8)
    half, _ = n2.q2_field(comp, G, depth, pts, t, mwl=0.25, ramp_duration=2 * t)
    full, _ = n2.q2_field(comp, G, depth, pts, t, mwl=0.25)
    assert np.allclose(np.asarray(half, dtype=float), 0.25 * np.asarray(full, dtype=float), rtol=1e-15, atol=0)


def test_regular_wave_gives_stokes_second_order_terms():
    A, w, depth, phi, t, x = 0.5, 0.9, 25.0, 0.4, 3.3, 7.0
    k = solve_k(w, depth)
    comp = wk.regular_components(A, w, k, phi)
    theta = k * x - w * t + phi
    for z, z2 in ((-4.0, -4.0), (2.0, 0.0)):  # the second point above the mean level: held at z2 = 0
        r = n2.point_terms(comp, G, depth, [[x, 0.0, z]], t)
        assert np.allclose(float(r["eta2"][0]), w2.stokes_eta2(A, k, depth, theta), rtol=1e-9, atol=0)
        # Stokes' second-order potential 3/8 A^2 w cosh(2 k (z + h)) / sinh^4(k h) sin 2 theta: -d/dt of it
        want = 0.75 * A * A * w * w * np.cosh(2 * k * (z2 + depth)) / np.sinh(k * depth) ** 4 * np.cos(2 * theta)
        assert np.allclose(float(r["q2"][0]), want, rtol=1e-9, atol=0)
    deep = n2.point_terms(wk.regular_components(A, w, w * w / G, phi), G, np.inf, [[x, 0.0, -4.0]], t)
    assert abs(float(deep["q2"][0])) <= 1e-12 * A * A * w * w  # no second-order potential in deep water


def test_second_order_off_is_the_first_order_restatement():
    import nonlinear_ref as nr
    import surface_clip_ref as sc
    k = solve_k(W3, 30.0)
    comp = (A3, W3, k, PHI3)
    tri = nr.box_triangles([-1.0, -0.5, -1.0], [1.0, 0.5, 1.0], m=2)
    pos, rpy = [[0.3, -0.1, 0.15], [9.0, 0.0, 0.1]], [[0.31, -0.22, 0.4], [0.1, 0.2, 0.3]]
    lists = [("tris", tri), ("panels", nr.triangles_to_panels(tri))]
    kw = dict(mwl=0.2, stretching=True, ramp=0.5)
    off = n2.nonlinear2(comp, G, 30.0, RHO, lists, 4.0, pos, rpy, second_order=False, **kw)
    a = sc.clipped(comp, 30.0, RHO, G, [tri, None], 4.0, pos, rpy, **kw)
    b = nr.nonlinear(comp, 30.0, RHO, G, [None, lists[1][1]], 4.0, pos, rpy, **kw)
    for key in ("buoy", "fk"):  # (the products are formed in another order: equal inside the bound)
        assert np.all(np.abs(off[key] - (a[key] + b[key])) <= off["bound_" + key]) and off[key].any(axis=1).all()
    on = n2.nonlinear2(comp, G, 30.0, RHO, lists, 4.0, pos, rpy, ramp_duration=8.0, **kw)
    assert np.all(np.abs(on["fk"] - off["fk"]).max(axis=1) > 100 * on["bound_fk"].max(axis=1))  # the increments show
    assert np.all(on["bound_fk"] >= off["bound_fk"])
    assert len(on["p"][0]) == 26 and len(on["p"][1]) == len(tri)  # 48 triangles share 26 vertices; every centroid is its own point


@pytest.mark.parametrize("name", sorted(ni.SETS))
def test_gpu_inputs_keep_the_conditions(name):
    """Every comparison of tests/test_gpu_nonlinear2.py on the CPU oracle's spectrum (CreateSpectrum depends on the parameters alone;
    the GPU test takes the context's own): the conditions tests/nonlinear2_inputs.py lists."""
    s = ni.SETS[name]
    case = ni.ci.synth_case(s["N"], s["depth"])
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**ni.waves(s["nf"]))
    comp = wk.irregular_components(orc.irreg_spectrum())
    orc.close()
    assert comp[0].size == s["nf"]
    for t in s["times"]:
        ref, _, _ = ni.reference(name, comp, case["rho"], t)
        first, _, _ = ni.reference(name, comp, case["rho"], t, second_order=False)
        big = max(np.abs(ref["buoy"]).max(), np.abs(ref["fk"]).max())
        print(f"{name} t={t}: cases {ref['cases'].sum(axis=0).tolist()} flips {ref['flips']} cut_span {ref['cut_span']:.3e} margin {ref['margin']:.3e} "
              f"bound/result {max(ref['bound_buoy'].max(), ref['bound_fk'].max()) / big:.3e} "
              f"|fk2 - fk1| / |fk1| {np.abs(ref['fk'] - first['fk']).max() / np.abs(first['fk']).max():.3e}")
        assert max(ref["bound_buoy"].max(), ref["bound_fk"].max()) < 1e-6 * big
        assert np.abs(ref["fk"] - first["fk"]).max() > 1e-6 * np.abs(first["fk"]).max()
        assert max(np.abs(e).max() for e in ref["eta2"] if e.size) > 0
        if s["tuned"] is not None:
            assert ref["flips"] >= 1
        if name == "one_triangle":
            assert len(ref["p"][0]) == 3
        if name == "tris257_deep_diff":
            assert len(ref["p"][0]) < 3 * 257 and np.all(ref["cases"].sum(axis=0) > 0), ref["cases"]
        if name == "mixed_300":
            assert len(ref["p"][0]) == 12 and len(ref["p"][1]) == 0 and len(ref["p"][2]) == 8


def test_new_kernels_build_without_scratch_or_spills(tmp_path):
    """The notes of the code object built from hc_nonlinear.hip, as tests/test_surface_clip_ref_cpu.py reads them."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_nonlinear.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_nonlinear.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(2): (int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5))) for m in re.finditer(
        r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)",
        txt, re.S)}
    for kernel in ("nl2_incr_kernelILb0E", "nl2_panels_kernel","nl2_tris_kernel", "nl_panels_kernel", "nl_tris_kernel"):
        found = [v for n, v in notes.items() if kernel in n]
        assert len(found) == 1, (kernel, sorted(notes))
        lds, scratch, vgpr, spills = found[0]
        print(kernel, "LDS", lds, "scratch", scratch, "vgpr", vgpr, "spills", spills)
        assert scratch == 0 and spills == 0, kernel
        assert vgpr <= 256 and lds <= 64 * 1024, kernel  # a 256-item workgroup must be able to launch


def test_abi_and_layers_declare_the_entry_points():
    import ctypes as C
    import inspect

    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroForces, HydroGroup
    lib = capi.load()
    for name in ("hc_set_nonlinear_second_order", "hc_get_nonlinear_second_order", "hc_get_nonlinear_point_count", "hc_get_nonlinear_increments"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_set_nonlinear_second_order(None, 1, 0.0, 1.0, 0.0, 1.0, 1) == capi.HC_ERR_INVALID
    assert lib.hc_get_nonlinear_point_count(None, 0, C.byref(C.c_int())) == capi.HC_ERR_INVALID
    assert lib.hc_get_nonlinear_increments(None, 0, 0, None, None, None) == capi.HC_ERR_INVALID
    p = inspect.signature(HydroForces.set_nonlinear_second_order).parameters
    assert p["on"].default is True and p["diff_band"].default == (0.0, float("inf")) and p["apply_ramp"].default is True
    for cls in (HydroForces, HydroGroup):
        assert hasattr(cls, "nonlinear_second_order") and hasattr(cls, "nonlinear_increments") and hasattr(cls, "nonlinear_point_count")
    header = open(os.path.join(ROOT, "include", "hydroc_amd", "hydro_forces.h")).read()
    assert "SetNonlinearSecondOrder" in header and "GetNonlinearIncrements" in header


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/nonlinear2_caller.cpp (SetNonlinearSecondOrder / GetNonlinearIncrements of include/hydroc_amd/hydro_forces.h) builds
    with plain g++; tests/test_gpu_nonlinear2.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "nonlinear2_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nonlinear2_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
