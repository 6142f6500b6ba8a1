"""The wave drift term without a GPU: the projected evaluation form in float64 against the direct pair sum of the
definition in longdouble (tests/drift_ref.py), inside the derived bound; closed forms; the grid ends; and the build of the kernel
(csrc/hc_qtf.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_drift.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import drift_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81


def components(nf, seed, lo=0.25, hi=2.4):
    """nf deep-water components, some of them outside [0.4, 2.0]"""
    rng = np.random.default_rng(seed)
    w = np.sort(rng.uniform(lo, hi, size=nf))
    A = rng.uniform(0.01, 0.3, size=nf)
    return A, w, w * w / G, rng.uniform(0.0, 2 * np.pi, size=nf)


@pytest.mark.parametrize("nf,nq", [(1, 2), (7, 2), (257, 33), (512, 64)])
def test_projected_form_equals_the_pair_sum(nf, nq):
    comp = components(nf, 10 + nf) if nf > 1 else (np.array([0.2]), np.array([1.1]), np.array([1.1 ** 2 / G]), np.array([0.4]))
    table = dr.random_table(nq, 20 + nq, 0.4, 2.0)
    inside = dr.cells(table[0], comp[1])[0]
    assert inside.any() and (nf < 7 or not inside.all())
    ref = dr.PairSum(comp, table)
    worst = 0.0
    for t, x in ((0.0, 0.0), (431.0, 850.0), (77.7, -120.5)):  # |theta| <= 850 * 2.4^2 / g + 2.4 * 431 + 2 pi < 1600
        want, bound = ref.force(t, x, ramp=0.5), dr.bounds(comp, table, ramp=0.5)
        for mode in (1, 2, 3):
            got = dr.projected(comp, table, t, x, mode, ramp=0.5)
            err = np.abs(got - want[mode])
            assert np.all(bound[mode] > 0)
            worst = max(worst, float(np.max(err / bound[mode])))
            assert np.all(err <= bound[mode]), (mode, t, x, float(np.max(err / bound[mode])))
    print(f"nf={nf} nq={nq}: worst |projected - pair sum| / bound = {worst:.3e}")
    # Q = None is Q = 0
    g, P, Q = table
    assert np.array_equal(dr.projected(comp, (g, P, None), 3.0, 5.0, 3), dr.projected(comp, (g, P, np.zeros_like(Q)), 3.0, 5.0, 3))
    assert np.array_equal(dr.PairSum(comp, (g, P, None)).force(3.0, 5.0)[3], dr.PairSum(comp, (g, P, np.zeros_like(Q))).force(3.0, 5.0)[3])


def test_newman_closed_form_equals_its_pair_sum():
    """(sum D_i u_i)(sum u_i) + (sum D_i w_i)(sum w_i) with D_i = D(w_i), written per component, against the pair sum."""
    comp = components(40, 3)
    table = dr.random_table(9, 4, 0.4, 2.0)
    A, w, k, phi = comp
    ref = dr.PairSum(comp, table)
    t, x = 12.5, 30.0
    th = (k * x - w * t + phi)[ref.idx]
    u, v, Di = A[ref.idx] * np.cos(th), A[ref.idx] * np.sin(th), np.asarray(ref.Di, dtype=float)
    closed = (Di @ u) * u.sum() + (Di @ v) * v.sum()
    assert np.allclose(closed, ref.force(t, x)[2], rtol=0, atol=dr.bounds(comp, table)[2])
    # one component: modes 1 and 2 agree, and so does mode 3 with the table's own diagonal interpolated bilinearly only on a node
    one = (np.array([0.3]), np.array([table[0][4]]), np.array([0.2]), np.array([1.0]))
    f = dr.PairSum(one, table).force(7.0, 3.0)
    assert np.allclose(f[1], f[2], rtol=1e-15) and np.allclose(f[1], f[3], rtol=1e-15) and np.allclose(f[1], 0.09 * table[1][:, 4, 4], rtol=1e-15)


def test_time_average_of_the_full_qtf_is_the_mean_drift_of_its_diagonal():
    """Hermitian table, components with w_i = n_i w_0 (distinct n_i): over the common period 2 pi / w_0 every pair term i != j
    averages to zero and sum_i A_i^2 P(w_i, w_i) is left.  Equally spaced samples (more than twice the highest difference
    harmonic) average the harmonics exactly."""
    w0 = 0.05
    n = np.array([9, 12, 17, 23, 30, 38])
    w = n * w0
    A = np.array([0.3, 0.25, 0.2, 0.15, 0.1, 0.05])
    comp = (A, w, w * w / G, np.array([0.1, 1.3, 2.9, 4.0, 5.5, 0.7]))
    table = dr.random_table(7, 8, 0.4, 2.0, hermitian=True)
    ref = dr.PairSum(comp, table)
    assert ref.idx.size == 6
    ns = 64  # > 2 * (38 - 9)
    T = 2 * np.pi / w0
    mean = np.mean([np.asarray(ref.force(T * s / ns, 11.0)[3], dtype=float) for s in range(ns)], axis=0)
    want = np.array([np.sum(A ** 2 * np.asarray(np.diagonal(ref.Pij[d]), dtype=float)) for d in range(6)])
    assert np.allclose(mean, want, rtol=0, atol=1e-12 * np.abs(table[1]).max() * A.sum() ** 2)
    # mode 1 on the same table gives the mean of mode 2, not of mode 3, unless the component sits on a node
    assert not np.allclose(ref.force(0.0, 0.0)[1], want, rtol=1e-6)


def test_grid_ends_are_inside_one_ulp_beyond_is_outside():
    g = np.array([0.4, 0.9, 1.7])
    P = np.zeros((6, 3, 3))
    P[:, 0, 0], P[:, 1, 1], P[:, 2, 2] = 10.0, 20.0, 40.0
    for w, want in ((g[0], 10.0), (g[-1], 40.0), (np.nextafter(g[0], 0.0), 0.0), (np.nextafter(g[-1], 9.0), 0.0), (g[1], 20.0),
                    (np.nextafter(g[-1], 0.0), None)):
        comp = (np.array([2.0]), np.array([w]), np.array([0.1]), np.array([0.3]))
        for mode in (1, 2, 3):
            f = dr.PairSum(comp, (g, P, None)).force(1.0, 2.0)[mode]
            p = dr.projected(comp, (g, P, None), 1.0, 2.0, mode)
            if want is None:  # just below the upper end: the last cell, weight almost 1 on the end
                assert np.all(f > 4 * 39.99) and np.all(np.abs(p - f) <= 1e-12)
            else:
                assert np.allclose(f, 4.0 * want, rtol=1e-15, atol=0) and np.allclose(p, 4.0 * want, rtol=1e-15, atol=0), (w, mode)
    inside, m, lam = dr.cells(g, np.array([0.4, 1.7, 0.9]))
    assert inside.all() and list(m) == [0, 1, 1] and list(lam) == [0.0, 1.0, 0.0]


def test_reference_refuses_large_phases():
    comp = (np.array([1.0]), np.array([1.0]), np.array([0.1]), np.array([0.0]))
    table = dr.random_table(2, 1, 0.5, 1.5)
    with pytest.raises(AssertionError):
        dr.PairSum(comp, table).force(1.0e4 + 1.0, 0.0)


def test_kernel_builds_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf not found"
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_qtf.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_qtf.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(2): (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(1))) for m in re.finditer(
        r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
        r".*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    assert any("drift_qtf_kernel" in n for n in notes), sorted(notes)
    for name, (scratch, vgpr, spills, lds) in notes.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert lds == (16384 if "drift_qtf_kernel" in name else 10240), (name, lds)  # four reduction columns against sum_qtf_kernel's one
    assert "hc_qtf.hip" in hb.SOURCES


def test_abi_declares_the_drift_entry_points_and_needs_a_device():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_drift_qtf", "hc_get_drift_qtf_size", "hc_set_drift_mode", "hc_get_drift_mode", "hc_set_drift_options",
                 "hc_drift_begin", "hc_drift_end", "hc_compute_drift"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_drift_end(None, None) == capi.HC_ERR_INVALID
    assert lib.hc_set_drift_mode(None, 1) == capi.HC_ERR_INVALID
    if lib.hc_device_count() == 0:  # no quiet fall-back: without a device there is no context to set a table on
        ctx = C.c_void_p()
        assert lib.hc_create(1, 0, C.byref(ctx)) == capi.HC_ERR_DEVICE and not ctx.value


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/drift_caller.cpp (SetDriftQTF / SetMeanDriftCoefficients / SetDriftMode / SetDriftOptions / ComputeForceDrift of
    include/hydroc_amd/hydro_forces.h) builds with plain g++; tests/test_gpu_drift.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "drift_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "drift_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
