"""The nonlinear surface forces on the second-order sea in a short-crested sea without a GPU: the definition itself (the pressure at
the second-order free surface is of third order, and only with u1y^2 in it), the tests' NumPy restatement
(tests/nonlinear2_dir_ref.py) against a difference quotient of wave2_dir_ref's potential, against the long-crested restatement for
equal directions and against itself in float64, the input sets of the GPU tests, the entry points, and the build of the new kernels
(csrc/hc_nonlinear.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_nonlinear2_dir.py."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import nonlinear2_dir_inputs as ndi
import nonlinear2_dir_ref as nd
import nonlinear2_ref as n2
import nonlinear_ref as nr
import wave2_dir_ref as wd
import wave_kinematics_ref as wk
from cases import load_into_oracle
from morison_ref import LD, rotation
from test_morison2_dir_ref_cpu import cardan_xyz
from test_nonlinear2_ref_cpu import A3, PHI3, W3, solve_k

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81
BETA3 = np.array([0.9, -0.7, 1.4])  # three different directions, none near an axis: u1y is of the size of u1x


@functools.lru_cache(maxsize=None)
def oracle_components(name):
    s = ndi.SETS[name]
    case = ndi.ci.synth_case(s["N"], s["depth"])
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**ndi.waves(s["nf"]))
    comp = wk.irregular_components(orc.irreg_spectrum())
    orc.close()
    assert comp[0].size == s["nf"]
    return comp, case["rho"]


@pytest.mark.parametrize("depth", [np.inf, 30.0])
def test_pressure_at_the_second_order_free_surface_is_of_third_order(depth):
    """tests/test_nonlinear2_ref_cpu.py's test in a sea of three components with three directions, with its margins: p_s + p_d at
    z = mwl + eta1 + eta2 over rho g sum|A| falls by 6 .. 10 per halving of the amplitudes (third order: 8); p_s + ramp p_d1 at
    z = mwl + eta1 by 3 .. 5 (second order: 4).  Without u1y^2 a second-order term is missing from the pressure and the residue no
    longer falls by 6 .. 10 at every halving.  No stretching."""
    k = solve_k(W3, depth)
    mwl = 0.25
    for x, y, t in ((3.0, -2.0, 1.7), (-11.0, 6.5, 4.4), (27.5, 14.0, 9.1), (0.4, -8.0, 13.3)):
        res = {"order2": [], "order1": [], "no_u1y": []}
        for halvings in range(4):
            comp = (A3 / 2.0 ** halvings, W3, k, PHI3)
            scale = LD(RHO) * LD(G) * LD(np.sum(np.abs(A3)))  # of the sea before the halvings: a unit, the same for every row
            at0 = nd.point_terms(comp, BETA3, G, depth, [[x, y, mwl]], t, mwl=mwl)
            for what, kw in (("order2", {}), ("order1", dict(second_order=False)), ("no_u1y", dict(with_u1y=False))):
                eta = LD(at0["eta1"][0]) if what == "order1" else at0["eta"][0]
                z = float(LD(mwl) + eta)
                r = nd.point_terms(comp, BETA3, G, depth, [[x, y, z]], t, mwl=mwl, **kw)
                ps = -LD(RHO) * LD(G) * (LD(z) - LD(mwl))
                res[what].append(abs(float((ps + LD(RHO) * r["pds"][0]) / scale)))
        ratios = {what: [v[i] / v[i + 1] for i in range(3)] for what, v in res.items()}
        print(f"depth {depth} x {x} y {y} t {t}: residues {res} ratios {ratios}")
        assert all(6.0 <= r <= 10.0 for r in ratios["order2"]), ratios
        assert all(3.0 <= r <= 5.0 for r in ratios["order1"]), ratios
        assert not all(6.0 <= r <= 10.0 for r in ratios["no_u1y"]), ratios  # 1/2 rho u1y^2 is a second-order term: left out, it shows


@pytest.mark.parametrize("depth", [np.inf, 30.0])
def test_q2_is_minus_the_time_derivative_of_the_second_order_potential(depth):
    """q2 against a five-point difference quotient of wave2_dir_ref.fields' own phi2 (step 1e-3 s: its truncation (Omega h)^4 / 30 is
    below 2e-11 of a term at Omega = 4.6 rad/s), to 1e-8 of the sum of |terms|; above the mean level, below it and at the bed; with
    bands.  In infinite depth the sum potential of crossing components is there."""
    k = solve_k(W3, depth)
    comp = (A3, W3, k, PHI3)
    pts = np.array([[3.0, 4.0, 1.2], [-7.0, -2.5, -0.4], [12.0, 9.0, -6.0], [1.0, -6.0, -30.0 + 0.25]])
    t, h = 2.9, 1e-3
    for bands in (dict(), dict(diff_band=(0.2, 0.5), sum_band=(3.6, 4.3)), dict(diff_band=(100.0, 200.0))):
        q2, scale = nd.q2_field(comp, BETA3, G, depth, pts, t, mwl=0.25, **bands)
        phi = {m: wd.fields(comp, BETA3, G, depth, pts, [t + m * h], mwl=0.25, **bands)[0][3][0] for m in (-2, -1, 1, 2)}
        dphi = (-phi[2] + 8 * phi[1] - 8 * phi[-1] + phi[-2]) / (12 * LD(h))
        err = np.abs(q2 + dphi) / scale
        print("depth", depth, bands, "worst |q2 + d phi2 / dt| / sum|terms|:", float(err.max()))
        assert np.all(scale > 0) and np.all(err <= 1e-8) and np.all(q2 != 0)
    half, _ = nd.q2_field(comp, BETA3, G, depth, pts, t, mwl=0.25, ramp_duration=2 * t)
    full, _ = nd.q2_field(comp, BETA3, G, depth, pts, t, mwl=0.25)
    assert np.allclose(np.asarray(half, dtype=float), 0.25 * np.asarray(full, dtype=float), rtol=1e-15, atol=0)


@pytest.mark.parametrize("depth", [30.0, np.inf])
@pytest.mark.parametrize("beta", [0.7, -2.9])
def test_equal_directions_are_the_long_crested_term_turned_about_z(depth, beta):
    """Every component at the heading beta: the sea is the long-crested one seen from a frame turned by beta about z
    (tests/test_morison2_dir_ref_cpu.py has the pattern).  The state turned by -beta, evaluated by tests/nonlinear2_ref.py, and the
    6-vectors turned back, within the sum of both bounds (the long-crested one turned with |Rz|)."""
    k = solve_k(W3, depth)
    comp = (A3, W3, k, PHI3)
    tri = nr.box_triangles([-1.0, -0.5, -1.0], [1.0, 0.5, 1.0], m=2)
    lists = [("tris", tri), ("panels", nr.triangles_to_panels(tri))]
    pos, rpy = np.array([[0.3, -0.1, 0.15], [9.0, 2.0, 0.1]]), np.array([[0.31, -0.22, 0.4], [0.1, 0.2, 0.3]])
    c, s = np.cos(LD(beta)), np.sin(LD(beta))
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=LD)  # turns by +beta
    turn = lambda v: (v.astype(LD) @ Rz).astype(np.float64)      # rows: Rz^T v, the turn by -beta
    rpy_t = np.stack([cardan_xyz(Rz.T @ rotation(rpy[b])) for b in range(2)])
    for b in range(2):
        assert np.max(np.abs(rotation(rpy_t[b]) - Rz.T @ rotation(rpy[b]))) < 1e-15
    aRz = np.abs(Rz).astype(np.float64)
    back = lambda v: np.concatenate([(v[:, :3].astype(LD) @ Rz.T), (v[:, 3:].astype(LD) @ Rz.T)], axis=1).astype(np.float64)
    back_abs = lambda v: np.concatenate([v[:, :3] @ aRz.T, v[:, 3:] @ aRz.T], axis=1)
    for stretching in (False, True):
        kw = dict(mwl=0.2, stretching=stretching, ramp=0.5, diff_band=(0.0, 0.9), ramp_duration=8.0)
        got = nd.nonlinear2_dir(comp, np.full(3, beta), G, depth, RHO, lists, 4.0, pos, rpy, **kw)
        lc = n2.nonlinear2(comp, G, depth, RHO, lists, 4.0, turn(pos), rpy_t, **kw)
        for key in ("buoy", "fk"):
            err, bound = np.abs(got[key] - back(lc[key])), got["bound_" + key] + back_abs(lc["bound_" + key])
            print(f"depth {depth} beta {beta} stretching {stretching}: {key} worst {np.max(err / np.maximum(bound, 1e-300)):.3e} of the bounds")
            assert np.all(err <= bound)
        assert np.array_equal(got["cases"], lc["cases"]) and got["flips"] == lc["flips"]
        assert np.abs(got["fk"][:, :2]).min() > 1.0  # F_x and F_y are both there
        for b in range(2):  # eta2 and q2 are scalars
            for key in ("eta2", "q2"):
                a_, b_ = np.asarray(got[key][b], dtype=float), np.asarray(lc[key][b], dtype=float)
                assert np.allclose(a_, b_, rtol=0, atol=1e-12 * np.abs(b_).max()) and b_.any()
        first = nd.nonlinear2_dir(comp, np.full(3, beta), G, depth, RHO, lists, 4.0, pos, rpy, **dict(kw, second_order=False))
        assert np.all(np.abs(first["fk"] - got["fk"]).max(axis=1) > 100 * got["bound_fk"].max(axis=1))  # the increments show


@pytest.mark.parametrize("name", sorted(ndi.SETS))
def test_float64_restatement_stays_within_its_own_bound(name):
    """The pair sums (eta2, q2) in plain float64 against the longdouble restatement: inside the bound the GPU is held to, on every
    set."""
    comp, rho = oracle_components(name)
    t = ndi.SETS[name]["times"][-1]
    ref, _, _ = ndi.reference(name, comp, rho, t)
    dbl, _, _ = ndi.reference(name, comp, rho, t, dtype=np.float64)
    for key in ("buoy", "fk"):
        err = np.abs(dbl[key] - ref[key])
        print(f"{name}: float64 {key} off by {np.max(err / np.maximum(ref['bound_' + key], 1e-300)):.3e} of the bound")
        assert np.all(np.isfinite(dbl[key])) and np.all(err <= ref["bound_" + key])
    assert np.array_equal(dbl["cases"], ref["cases"])


@pytest.mark.parametrize("name", sorted(ndi.SETS))
def test_gpu_inputs_keep_the_conditions(name):
    """Every comparison of tests/test_gpu_nonlinear2_dir.py on the CPU oracle's spectrum (the GPU test takes the context's own): the
    conditions tests/nonlinear2_dir_inputs.py lists."""
    s = ndi.SETS[name]
    comp, rho = oracle_components(name)
    for t in s["times"]:
        ref, _, _ = ndi.reference(name, comp, rho, t)
        first, _, _ = ndi.reference(name, comp, rho, t, second_order=False)
        big = max(np.abs(ref["buoy"]).max(), np.abs(ref["fk"]).max())
        print(f"{name} t={t}: cases {ref['cases'].sum(axis=0).tolist()} flips {ref['flips']} cut_span {ref['cut_span']:.3e} margin {ref['margin']:.3e} "
              f"bound/result {max(ref['bound_buoy'].max(), ref['bound_fk'].max()) / big:.3e} "
              f"|fk2 - fk1| / |fk1| {np.abs(ref['fk'] - first['fk']).max() / np.abs(first['fk']).max():.3e}")
        assert max(ref["bound_buoy"].max(), ref["bound_fk"].max()) < 1e-6 * big
        assert np.abs(ref["fk"] - first["fk"]).max() > 1e-6 * np.abs(first["fk"]).max()
        assert max(np.abs(e).max() for e in ref["eta2"] if e.size) > 0 and max(np.abs(np.asarray(q, dtype=float)).max() for q in ref["q2"] if q.size) > 0
        if s["tuned"] is not None:
            assert ref["flips"] >= 1
        if name == "one_triangle":
            assert len(ref["p"][0]) == 3
        if name.startswith("tris257_deep"):
            assert len(ref["p"][0]) < 3 * 257 and np.all(ref["cases"].sum(axis=0) > 0), ref["cases"]
        if name == "mixed_300":
            assert len(ref["p"][0]) == 12 and len(ref["p"][1]) == 0 and len(ref["p"][2]) == 8


def test_new_kernels_build_without_scratch_or_spills(tmp_path):
    """The notes of the code object built from hc_nonlinear.hip, as tests/test_nonlinear2_ref_cpu.py reads them."""
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
    for kernel in ("nl2_incr_kernelILb1E", "nl2_dir_panels_kernel","nl2_dir_tris_kernel"):
        found = [v for n, v in notes.items() if kernel in n]
        assert len(found) == 1, (kernel, sorted(notes))
        lds, scratch, vgpr, spills = found[0]
        print(kernel, "LDS", lds, "scratch", scratch, "vgpr", vgpr, "spills", spills)
        assert scratch == 0 and spills == 0, kernel
        assert vgpr <= 256 and lds <= 64 * 1024, kernel  # a 256-item workgroup must be able to launch


def test_abi_and_layers_declare_the_entry_points():
    import inspect

    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroForces, HydroGroup
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "hydrochrono_amd.h")).read()
    for name in ("hc_set_nonlinear_second_order_directional", "hc_get_nonlinear_second_order_directional"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert lib.hc_set_nonlinear_second_order_directional(None, 1) == capi.HC_ERR_INVALID
    assert lib.hc_get_nonlinear_second_order_directional(None, None) == capi.HC_ERR_INVALID
    assert inspect.signature(HydroForces.set_nonlinear_second_order_directional).parameters["on"].default is True
    assert hasattr(HydroForces, "nonlinear_second_order_directional") and "nonlinear_second_order_directional" in vars(HydroGroup)
    mirror = open(os.path.join(ROOT, "include", "hydroc_amd", "hydro_forces.h")).read()
    assert "SetNonlinearSecondOrderDirectional" in mirror


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/nonlinear2_dir_caller.cpp (SetNonlinearSecondOrderDirectional of include/hydroc_amd/hydro_forces.h) builds with plain
    g++; tests/test_gpu_nonlinear2_dir.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "nonlinear2_dir_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nonlinear2_dir_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
