"""The C++ mirror with a surface mesh clipped at the free surface (TestHydro::SetSurfaceMesh(body, triangles, true) of
include/hydroc_amd/hydro_forces.h) driven by tests/cpp/surface_clip_caller.cpp: its terms are the C ABI's
(hc_set_surface_triangles + hc_compute_nonlinear) bit for bit and its total is the composition of them."""
import os
import subprocess

import numpy as np
import pytest

import surface_clip_ref as sc
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, sphere_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REG_AMP, REG_OMEGA = 0.177, 2.094395102


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def caller_box(a, b, z0, z1):
    """the twelve triangles of tests/cpp/surface_clip_caller.cpp, in its order"""
    x, y, z = (-a, a), (-b, b), (z0, z1)
    v = (lambda i, j, k: [x[i], y[j], z[k]])
    quads = [(v(0, 0, 0), v(0, 1, 0), v(1, 1, 0), v(1, 0, 0)), (v(0, 0, 1), v(1, 0, 1), v(1, 1, 1), v(0, 1, 1)),
             (v(0, 0, 0), v(1, 0, 0), v(1, 0, 1), v(0, 0, 1)), (v(0, 1, 0), v(0, 1, 1), v(1, 1, 1), v(1, 1, 0)),
             (v(0, 0, 0), v(0, 0, 1), v(0, 1, 1), v(0, 1, 0)), (v(1, 0, 0), v(1, 1, 0), v(1, 1, 1), v(1, 0, 1))]
    return np.array([t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])], dtype=float)


def test_cpp_mirror_clipped_mesh_gives_the_c_abi_values(tmp_path):
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd import build as hb, capi
    from hydrochrono_amd.hydro import HydroForces as HF
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "surface_clip_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "surface_clip_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (12, 37)
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
    mesh = caller_box(2.0, 1.5, -3.0, 4.0)
    assert h.lib.hc_set_surface_triangles(h.ctx, 0, mesh.ctypes.data_as(capi.c_double_p), 12) == capi.HC_OK  # the C ABI itself
    h.set_nonlinear_options(mwl=0.25, regular_phase=0.3)
    comp = wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.3)
    case = sphere_case()
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        a = [np.ascontiguousarray(x) for x in st]
        total = np.empty(6)
        assert h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], total.ctypes.data_as(capi.c_double_p)) == capi.HC_OK
        buoy, fk, hs = row[19:25], row[25:31], row[31:37]
        assert same_bits(row[13:19], total - hs + buoy + fk), t
        assert all(same_bits(x, y) for x, y in zip(h.compute_nonlinear(t, st[0], st[1]), (buoy, fk, hs))), t
    # ... and the last row against the restatement: the box is cut (tilted, the surface between its top and its bottom)
    ref = sc.clipped(comp, case["water_depth"], case["rho"], 9.81, [mesh], t, st[0], st[1], mwl=0.25)
    assert ref["cases"][0][1] + ref["cases"][0][2] > 0 and ref["cut_span"] >= 1e-3
    assert np.all(np.abs(buoy - ref["buoy"][0]) <= ref["bound_buoy"][0]) and np.all(np.abs(fk - ref["fk"][0]) <= ref["bound_fk"][0])
    assert np.abs(rows[:, 19:22]).max() > 1.0 and np.abs(rows[:, 25:28]).max() > 1.0
