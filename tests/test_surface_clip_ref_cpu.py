"""Triangles clipped at the free surface without a GPU: the tests' NumPy restatement (tests/surface_clip_ref.py) against closed forms,
against itself across meshes and against the centroid rule, and the build of nl_tris_kernel (csrc/hc_nonlinear.hip: no scratch, no
spilled register).  The GPU side is tests/test_gpu_surface_clip.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import nonlinear_ref as nr
import surface_clip_ref as sc
import wave_kinematics_ref as wk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81
LO, HI = [-1.0, -0.5, -1.0], [1.0, 0.5, 1.0]  # the box of the tilted and the wave cases
TILT_POS, TILT_RPY = [0.3, -0.1, 0.15], [0.31, -0.22, 0.4]


def inside(got, want, bound):
    return np.all(np.abs(np.asarray(got) - np.asarray(want)) <= bound)


def test_upright_box_in_still_water_is_the_closed_form_at_any_draft_and_mesh():
    """buoy_z = rho g A (mwl - z_bottom) with no mesh row on the waterline: the cut does it."""
    A = 2.0 * 1.0
    for m in (1, 3):
        tri = nr.box_triangles(LO, HI, m=m)
        for z0, mwl in ((-0.37, 0.0), (0.2, 0.0), (0.613, 0.0), (0.1, 0.45)):
            out = sc.clipped(None, 50.0, RHO, G, [tri], 0.0, [0.3, 0.0, z0], [0.0, 0.0, 0.7], mwl=mwl)
            want = RHO * G * A * (mwl - (z0 - 1.0))
            assert out["cases"][0][1] + out["cases"][0][2] > 0 and out["cases"][0][0] > 0 and out["cases"][0][3] > 0
            assert abs(out["buoy"][0, 2] - want) <= out["bound_buoy"][0, 2], (m, z0, out["buoy"][0, 2] - want, out["bound_buoy"][0, 2])
            assert inside(out["buoy"][0, :2], 0.0, out["bound_buoy"][0, :2]) and not out["fk"].any()
            assert np.all(out["bound_buoy"][0] < 1e-9 * want) and np.all(out["bound_buoy"][0] > 0)


def test_moment_of_an_off_centre_box_about_the_body_reference():
    """The box [1, 3] x [-2, -1] x [-1.5, 0.5] of the body frame, upright, draft 1.2: the force rho g V acts at the centre of the
    submerged volume, (2, -1.5, .) from the reference, so M = r x F = (y_c F_z, -x_c F_z, 0)."""
    tri = nr.box_triangles([1.0, -2.0, -1.5], [3.0, -1.0, 0.5], m=2)
    out = sc.clipped(None, np.inf, RHO, G, [tri], 0.0, [5.0, 4.0, 0.3], [0.0, 0.0, 0.0])
    Fz = RHO * G * 2.0 * 1.0 * 1.2
    assert abs(out["buoy"][0, 2] - Fz) <= out["bound_buoy"][0, 2]
    assert inside(out["buoy"][0, 3:], [-1.5 * Fz, -2.0 * Fz, 0.0], out["bound_buoy"][0, 3:]), out["buoy"][0, 3:]
    assert np.all(out["bound_buoy"][0, 3:] < 1e-9 * Fz)


def test_tilted_twelve_triangle_box_equals_the_fine_one():
    """Still water: the result is the hydrostatic load of the polyhedron below the plane, whatever the mesh."""
    coarse = sc.clipped(None, 50.0, RHO, G, [nr.box_triangles(LO, HI, m=1)], 0.0, TILT_POS, TILT_RPY)
    fine = sc.clipped(None, 50.0, RHO, G, [nr.box_triangles(LO, HI, m=8)], 0.0, TILT_POS, TILT_RPY)
    assert coarse["cases"][0][1] + coarse["cases"][0][2] > 0 and fine["cases"][0][1] + fine["cases"][0][2] > 0
    assert coarse["cut_span"] >= 1e-3 and fine["cut_span"] >= 1e-3
    bound = coarse["bound_buoy"][0] + fine["bound_buoy"][0]
    assert inside(coarse["buoy"][0], fine["buoy"][0], bound), (coarse["buoy"][0] - fine["buoy"][0], bound)
    assert np.all(bound < 1e-9 * abs(fine["buoy"][0, 2])) and abs(fine["buoy"][0, 3]) > 1e-3 * abs(fine["buoy"][0, 2])


def test_heave_sweep_is_continuous_where_the_centroid_rule_is_not():
    """The box rolled by a = 0.3 about x, heaved in 1 mm steps while the plane cuts the two long sides only, so the waterplane is the
    constant A_wp = 2 * 1 / cos a; the mesh rows of both sides cross the surface inside the sweep.  Clipped: every step changes F_z by
    rho g A_wp * 1 mm.  The centroid rule on the same mesh takes steps above that."""
    a = 0.3
    tri = nr.box_triangles(LO, HI, m=2)
    panels = [nr.triangles_to_panels(tri)]
    A_wp = 2.0 * 1.0 / np.cos(a)
    zs = np.arange(-200, 201) / 1000.0
    assert -0.2 < -0.5 * np.sin(a) and 0.5 * np.sin(a) < 0.2  # the vertex rows z_body = 0 of the two sides cross inside the sweep
    assert -np.cos(a) + 0.5 * np.sin(a) + 0.2 < 0 < np.cos(a) - 0.5 * np.sin(a) - 0.2  # top and bottom stay clear of the surface
    clip, cent, seen = [], [], set()
    for z in zs:
        out = sc.clipped(None, 50.0, RHO, G, [tri], 0.0, [0.0, 0.0, z], [a, 0.0, 0.0])
        clip.append(out["buoy"][0, 2])
        seen.add(tuple(out["cases"][0]))
        cent.append(nr.nonlinear(None, 50.0, RHO, G, panels, 0.0, [0.0, 0.0, z], [a, 0.0, 0.0])["buoy"][0, 2])
    assert len(seen) > 1  # the case table changed along the way
    limit = RHO * G * A_wp * 1e-3 * (1 + 1e-9)
    dclip, dcent = np.abs(np.diff(clip)), np.abs(np.diff(cent))
    print("largest step: clipped", dclip.max(), "centroid rule", dcent.max(), "limit", limit)
    assert np.all(dclip <= limit), dclip.max() / limit
    assert dcent.max() > limit


def test_froude_krylov_converges_between_first_and_second_order():
    """Regular deep-water wave (A = 0.3 m, w = 2 rad/s) over the tilted box: the error of fk at m = 2, 4, 8 squares per face against
    m = 32 falls by more than 2 sqrt 2 per halving (the geometric mean of a first-order 2 and a second-order 4)."""
    A, w, t = 0.3, 2.0, 0.7
    comp = wk.regular_components(A, w, w * w / G, 0.0)
    res = {m: sc.clipped(comp, np.inf, RHO, G, [nr.box_triangles(LO, HI, m=m)], t, TILT_POS, TILT_RPY) for m in (2, 4, 8, 32)}
    ref = res[32]["fk"][0]
    err = {m: np.max(np.abs(res[m]["fk"][0] - ref)) / np.max(np.abs(ref)) for m in (2, 4, 8)}
    print("fk errors against m = 32:", err, "ratios", err[2] / err[4], err[4] / err[8])
    assert err[8] > 100 * np.max(res[8]["bound_fk"][0]) / np.max(np.abs(ref))  # discretisation, not rounding
    assert err[2] / err[4] > 2 * np.sqrt(2) and err[4] / err[8] > 2 * np.sqrt(2)
    # the clipped buoyancy on the coarsest mesh is already close; the centroid rule on it is not
    buoy_ref = res[32]["buoy"][0]
    cent = nr.nonlinear(comp, np.inf, RHO, G, [nr.triangles_to_panels(nr.box_triangles(LO, HI, m=2))], t, TILT_POS, TILT_RPY)["buoy"][0]
    e_clip = np.max(np.abs(res[2]["buoy"][0] - buoy_ref)) / np.max(np.abs(buoy_ref))
    e_cent = np.max(np.abs(cent - buoy_ref)) / np.max(np.abs(buoy_ref))
    print("buoy at m = 2 against m = 32: clipped", e_clip, "centroid rule", e_cent)
    assert e_clip < 0.1 * e_cent


def test_case_counts_cut_span_and_vertex_values():
    """The bookkeeping the GPU tests rely on: one triangle per case, the span of its cut edges, eta and h at the vertices."""
    tri = np.array([[[0, 0, 1.0], [1, 0, 2.0], [0, 1, 3.0]],      # dry
                    [[0, 0, -1.0], [1, 0, 2.0], [0, 1, 3.0]],     # one wet vertex
                    [[0, 0, -1.0], [1, 0, -2.0], [0, 1, 3.0]],    # two
                    [[0, 0, -1.0], [1, 0, -2.0], [0, 1, -3.0]]])  # three
    out = sc.clipped(None, 50.0, RHO, G, [tri, None], 0.0, np.zeros((2, 3)), np.zeros((2, 3)))
    assert out["cases"].tolist() == [[1, 1, 1, 1], [0, 0, 0, 0]] and out["cut_span"] == 3.0
    assert np.array_equal(out["h"][0], tri[:, :, 2]) and not out["eta"][0].any() and out["points"][1].shape == (0, 3, 3)
    assert not out["buoy"][1].any() and not out["bound_buoy"][1].any()
    # the one-wet triangle alone: the wet part is (a, ab, ac) with s = 1/3 and 1/4; F_z = -(mean p_s) S_z over it
    one = sc.clipped(None, 50.0, RHO, G, [tri[1:2]], 0.0, np.zeros(3), np.zeros(3))
    S_z = 0.5 * (1 / 3) * (1 / 4)
    assert np.isclose(one["buoy"][0, 2], -(RHO * G * 1.0 / 3.0) * S_z, rtol=1e-14)
    # a vertex exactly on the surface counts as wet and its sub-triangle has no area
    on = sc.clipped(None, 50.0, RHO, G, [[[[0, 0, 0.0], [1, 0, 2.0], [0, 1, 3.0]]]], 0.0, np.zeros(3), np.zeros(3))
    assert on["cases"][0].tolist() == [0, 1, 0, 0] and not on["buoy"].any()


def test_vertex_eta_is_the_kinematics_restatement():
    rng = np.random.default_rng(3)
    nf = 30
    k = np.sort(rng.uniform(0.05, 2.0, nf))
    comp = (rng.uniform(0.01, 0.05, nf), np.sqrt(G * k), k, rng.uniform(0, 6.28, nf))
    tri = nr.box_triangles(LO, HI, m=2)
    for stretching in (False, True):
        out = sc.clipped(comp, 40.0, RHO, G, [tri], 1.7, TILT_POS, TILT_RPY, mwl=0.2, stretching=stretching, ramp=0.5)
        eta, _ = wk.elevation(comp, out["points"][0].reshape(-1, 3), [1.7])
        assert np.array_equal(out["eta"][0].reshape(-1), eta[0])
        full = sc.clipped(comp, 40.0, RHO, G, [tri], 1.7, TILT_POS, TILT_RPY, mwl=0.2, stretching=stretching)
        assert np.allclose(out["fk"], 0.5 * full["fk"], rtol=1e-15, atol=0) and np.array_equal(out["buoy"], full["buoy"])
        assert np.array_equal(out["cases"], full["cases"])  # the eta of the wet test is not ramped


def test_tris_kernel_builds_without_scratch_or_spills(tmp_path):
    """The notes of the code object built from hc_nonlinear.hip, as tests/test_nonlinear_ref_cpu.py reads them."""
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
    sgpr_spills = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+).*?\.sgpr_spill_count:\s+(\d+)", txt, re.S)}
    print("scalar registers kept in lanes of a vector register:", {n: c for n, c in sgpr_spills.items() if "nl_tris_kernel" in n})
    tris = [v for n, v in notes.items() if "nl_tris_kernel" in n]
    assert len(tris) == 1, sorted(notes)
    lds, scratch, vgpr, spills = tris[0]
    print("nl_tris_kernel: LDS", lds, "scratch", scratch, "vgpr", vgpr, "spills", spills)
    assert scratch == 0 and spills == 0
    assert vgpr <= 256 and lds <= 64 * 1024  # one wave per SIMD of a 256-item workgroup; a workgroup's LDS limit


def test_abi_and_python_layer_declare_the_triangle_entry_points():
    import ctypes as C

    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroForces, HydroGroup
    lib = capi.load()
    for name in ("hc_set_surface_triangles", "hc_get_surface_triangle_count"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_set_surface_triangles(None, 0, None, 0) == capi.HC_ERR_INVALID
    assert lib.hc_get_surface_triangle_count(None, 0, C.byref(C.c_int())) == capi.HC_ERR_INVALID
    import inspect
    assert inspect.signature(HydroForces.set_surface_mesh).parameters["clip"].default is False
    assert hasattr(HydroForces, "surface_triangle_count") and hasattr(HydroGroup, "surface_triangle_count")


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/surface_clip_caller.cpp (SetSurfaceMesh(body, triangles, true)) builds with plain g++; tests/test_gpu_surface_clip_cpp.py
    runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "surface_clip_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "surface_clip_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)


def test_gpu_inputs_keep_the_conditions():
    """Every comparison of section 1 of tests/test_gpu_surface_clip.py on the CPU oracle's spectrum (CreateSpectrum depends on the
    parameters alone; the GPU test takes the context's own): the conditions tests/surface_clip_inputs.py lists."""
    import surface_clip_inputs as ci
    from cases import load_into_oracle
    for name, N, depth, kind, params in ci.SYSTEMS:
        case = ci.synth_case(N, depth)
        orc = load_into_oracle(case)
        ci.add_waves(orc, kind, params)
        comp = ci.components(orc, kind, params)
        orc.close()
        seen = np.zeros(4, dtype=int)
        for n, mwl, stretching, t, ramp in ci.comparisons(kind, N):
            tris = ci.lists(N, n)
            assert len(tris[0]) == n
            ref, _, _ = ci.reference(case, tris, comp, kind, n, mwl, stretching, t, ramp, f"{name} n={n} mwl={mwl} stretching={stretching} t={t}")
            seen += ref["cases"].sum(axis=0)
            assert np.all(ref["bound_buoy"][0] < 1e-8 * np.abs(ref["buoy"][0]).max())  # far below the result
            if comp is not None and ramp > 0:
                assert np.all(ref["bound_fk"][0] < 1e-6 * np.abs(ref["fk"][0]).max()), (name, n, ref["bound_fk"][0], ref["fk"][0])
        assert np.all(seen > 0), (name, seen.tolist())


def test_kernel_case_table_compiled_for_the_host_is_the_restatement(tmp_path):
    """The text of csrc/hc_nonlinear.hip from NlVertex to nl_sub_triangle, and nl_tris_kernel's lines between the component loop and the
    LDS tree (wet flags, the turn of the triangle, the case table), compiled for the host with g++ and no contraction, fed random
    vertex values d, p_s, p_d, h -- vertices with h = 0 exactly among them -- against the restatement's own clipping of the same values.
    Tolerance: 64 * 2^-52 of a triangle's contribution without cancellation (the largest |p| times the area vector formed from edges
    |d_x| + |d_y|, every product in absolute value; times the largest lever for the moment): some thirty roundings per output, the cut
    fraction's among them.  Dry triangles give exact zeros."""
    from hydrochrono_amd import build as hb
    from morison_ref import EPS, LD
    src = open(os.path.join(hb.CSRC, "hc_nonlinear.hip")).read()
    funcs = src[src.index("struct NlVertex"):src.index("// nl_panels_kernel's shape for triangles")]
    table = src[src.index("    const bool w0 = h0 <= 0.0"):src.index("#pragma unroll\n    for (int k = 0; k < kNlOut; ++k) red[k][tid] = v[k];")]
    assert "nl_sub_triangle(A, bc, ca, v)" in table and "__global__" not in funcs
    prog = """#include <cstdio>
#define __device__
#define __forceinline__ inline
constexpr int kNlOut = 12;
""" + funcs + """
int main() {
    double in[18];
    while (true) {
        for (int i = 0; i < 18; ++i)
            if (std::scanf("%lf", &in[i]) != 1) return 0;
        NlVertex q0{in[0], in[1], in[2], in[3], in[4]}, q1{in[6], in[7], in[8], in[9], in[10]}, q2{in[12], in[13], in[14], in[15], in[16]};
        const double h0 = in[5], h1 = in[11], h2 = in[17];
        const bool active = true;
""" + table + """
        for (int k = 0; k < 12; ++k) std::printf("%.17g ", v[k]);
        std::printf("\\n");
    }
}
"""
    cpp, exe = str(tmp_path / "case_table.cpp"), str(tmp_path / "case_table")
    open(cpp, "w").write(prog)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", cpp, "-o", exe], check=True)
    rng = np.random.default_rng(1)
    n = 4000
    d, ps, pd, h = rng.uniform(-3, 3, (n, 3, 3)), rng.uniform(-1e4, 1e4, (n, 3)), rng.uniform(-1e3, 1e3, (n, 3)), rng.uniform(-1, 1, (n, 3))
    h[:50, 0], h[50:100, 1], h[100:120], h[120:140, :2] = 0.0, 0.0, 0.0, 0.0
    rows = np.concatenate([d, ps[:, :, None], pd[:, :, None], h[:, :, None]], axis=2).reshape(n, 18)
    text = "\n".join(" ".join(repr(float(x)) for x in row) for row in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array([[float(x) for x in line.split()] for line in out.strip().splitlines()])
    assert got.shape == (n, 12) and np.all(np.isfinite(got))
    dL, psL, pdL, hL = (x.astype(LD) for x in (d, ps, pd, h))
    wet = h <= 0
    nw = wet.sum(axis=1)
    r = np.where(nw == 1, np.argmax(wet, axis=1), np.where(nw == 2, (np.argmin(wet, axis=1) + 1) % 3, 0))
    A, B, C = ((sc._take(dL, (r + j) % 3), sc._take(psL, (r + j) % 3), sc._take(pdL, (r + j) % 3)) for j in range(3))
    hA, hB, hC = (sc._take(hL, (r + j) % 3) for j in range(3))
    one, two, three = nw == 1, nw == 2, nw == 3
    ab, ac, bc = sc._cut(A, B, hA, hB, one), sc._cut(A, C, hA, hC, one | two), sc._cut(B, C, hB, hC, two)
    want = np.zeros((n, 12), dtype=LD)
    for mask, sub in ((three, sc._sub_triangle(A, B, C)), (one, sc._sub_triangle(A, ab, ac)), (two, sc._sub_triangle(A, B, bc)),
                      (two, sc._sub_triangle(A, bc, ac))):
        for k in range(4):
            want[:, 3 * k:3 * k + 3] += np.where(mask[:, None], sub[k], 0)
    ad = np.abs(dL)
    e1, e2 = ad[:, 1] + ad[:, 0], ad[:, 2] + ad[:, 0]
    s_tilde = LD(0.5) * np.stack([e1[:, 1] * e2[:, 2] + e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] + e1[:, 0] * e2[:, 2],
                                  e1[:, 0] * e2[:, 1] + e1[:, 1] * e2[:, 0]], axis=1)
    dmax = np.max(np.sqrt(np.sum(dL * dL, axis=2)), axis=1)
    tol = np.zeros((n, 12), dtype=LD)
    for k, p in ((0, psL), (2, pdL)):
        f = np.max(np.abs(p), axis=1)[:, None] * s_tilde
        tol[:, 3 * k:3 * k + 3] = f
        tol[:, 3 * k + 3:3 * k + 6] = (dmax * np.sqrt(np.sum(f * f, axis=1)))[:, None]
    err = np.abs(got - want.astype(np.float64))
    counts = [int((nw == k).sum()) for k in range(4)]
    print("triangles with 0, 1, 2, 3 wet vertices:", counts, "worst error / tolerance:", float(np.max(err / (64 * EPS * tol).astype(np.float64))))
    assert min(counts) > 100 and np.all(err <= (64 * EPS * tol).astype(np.float64))
    assert not got[nw == 0].any()
