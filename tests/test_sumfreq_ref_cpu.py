"""The sum-frequency term without a GPU: the projected evaluation form in float64 against the direct pair sum of the
definition in longdouble (tests/sumfreq_ref.py), inside the derived bound; the antisymmetric part of a table; the regular-wave closed
form; and the build of the kernel (csrc/hc_qtf.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_sumfreq.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import sumfreq_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81
LO, HI = 0.4, 2.0


def components(nf, seed, grid):
    """nf deep-water components on [0.25, 2.4]; from 7 on: one below and one above the grid, one on either grid end, one on a node"""
    rng = np.random.default_rng(seed)
    w = np.sort(rng.uniform(0.25, 2.4, size=nf))
    if nf >= 7:
        w[0], w[1], w[2], w[3], w[4] = 0.3, grid[0], grid[len(grid) // 2], grid[-1], 2.3
    A = rng.uniform(0.01, 0.3, size=nf)
    return A, w, w * w / G, rng.uniform(0.0, 2 * np.pi, size=nf)


def symmetric(table):
    g, P, Q = table
    return g, 0.5 * (P + P.transpose(0, 2, 1)), 0.5 * (Q + Q.transpose(0, 2, 1))


def antisymmetric(table):
    g, P, Q = table
    return g, P - P.transpose(0, 2, 1), Q - Q.transpose(0, 2, 1)


def one_component(w):
    return np.array([0.2]), np.array([w]), np.array([w * w / G]), np.array([0.4])


STATES = ((0.0, 0.0), (431.0, 850.0), (77.7, -120.5))  # |theta| <= 850 * 2.4^2 / g + 2.4 * 431 + 2 pi < 1600


def check(comp, table, ramp=0.5):
    """worst |projected - pair sum| / bound over STATES (0 where the bound is 0: then both are exactly 0)"""
    ref, bound = sr.PairSum(comp, table), sr.bound(comp, table, ramp=ramp)
    worst = 0.0
    for t, x in STATES:
        err = np.abs(sr.projected(comp, table, t, x, ramp=ramp) - ref.force(t, x, ramp=ramp))
        assert np.all(err <= bound), (t, x, err, bound)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    return worst


@pytest.mark.parametrize("nq", [2, 5, 64])
@pytest.mark.parametrize("nf", [1, 7, 300])
def test_projected_form_equals_the_pair_sum(nf, nq):
    general = sr.random_table(nq, 20 + nq, LO, HI)
    g = general[0]
    if nf == 1:  # on either grid end, on a node, inside a cell, outside
        comps = [one_component(w) for w in (g[0], g[-1], g[nq // 2], 0.5 * (g[0] + g[1]), 0.3, 2.3)]
    else:
        comps = [components(nf, 10 + nf, g)]
        inside, m, lam = sr.cells(g, comps[0][1])
        assert not inside[0] and not inside[4] and inside[1:4].all() and lam[1] == 0.0 and lam[3] == 1.0 and lam[2] in (0.0, 1.0)
    worst = 0.0
    for comp in comps:
        for table in (general, symmetric(general), (g, general[1], None)):
            worst = max(worst, check(comp, table))
    print(f"nf={nf} nq={nq}: worst |projected - pair sum| / bound = {worst:.3e}")
    comp = comps[-1] if nf > 1 else comps[3]
    assert np.abs(sr.PairSum(comp, general).force(3.0, 5.0)).min() > 0.0
    # outside the grid: exactly zero in both forms
    if nf == 1:
        for comp in comps[4:]:
            assert not sr.projected(comp, general, 3.0, 5.0).any() and not sr.PairSum(comp, general).force(3.0, 5.0).any()
    # Q = None is Q = 0
    P, Q = general[1], general[2]
    assert np.array_equal(sr.projected(comp, (g, P, None), 3.0, 5.0), sr.projected(comp, (g, P, np.zeros_like(Q)), 3.0, 5.0))
    assert np.array_equal(sr.PairSum(comp, (g, P, None)).force(3.0, 5.0), sr.PairSum(comp, (g, P, np.zeros_like(Q))).force(3.0, 5.0))


@pytest.mark.parametrize("nf,nq", [(7, 2), (300, 5), (300, 64)])
def test_antisymmetric_table_gives_zero_and_only_the_symmetric_part_counts(nf, nq):
    """cos and sin of theta_i + theta_j are symmetric in (i, j): an antisymmetric table sums to zero, and a general table gives what
    its symmetric part gives -- each within the bound of the table that was summed."""
    general = sr.random_table(nq, 30 + nq, LO, HI)
    comp = components(nf, 40 + nf, general[0])
    anti = antisymmetric(general)
    for t, x in STATES:
        bound = sr.bound(comp, anti)
        assert np.all(bound > 0)
        assert np.all(np.abs(sr.PairSum(comp, anti).force(t, x)) <= bound)
        assert np.all(np.abs(sr.projected(comp, anti, t, x)) <= bound)
        full, sym = sr.PairSum(comp, general).force(t, x), sr.PairSum(comp, symmetric(general)).force(t, x)
        assert np.all(np.abs(full - sym) <= sr.bound(comp, general) + sr.bound(comp, symmetric(general)))
        assert np.abs(full).max() > 1e3 * bound.max()  # not a comparison of zeros


def test_regular_wave_closed_form():
    """One component: A^2 [P_s(w, w) cos 2 theta - Q_s(w, w) sin 2 theta], P_s(w, w) the bilinear interpolation -- not the drift term's
    constant A^2 P(w, w): the force oscillates at 2 w, and Q takes part."""
    table = sr.random_table(5, 3, LO, HI)
    A, w, phi = 0.177, 1.3, 0.7
    comp = (np.array([A]), np.array([w]), np.array([w * w / G]), np.array([phi]))
    Pww, Qww = sr.interp_diag(table, w)
    ref, bound = sr.PairSum(comp, table), sr.bound(comp, table)
    vals = []
    for t, x in ((0.0, 0.0), (3.7, 12.3), (41.3, -7.0)):
        theta = w * w / G * x - w * t + phi
        closed = sr.regular_closed_form(A, theta, Pww, Qww)
        assert np.all(np.abs(ref.force(t, x) - closed) <= bound) and np.all(np.abs(sr.projected(comp, table, t, x) - closed) <= bound)
        vals.append(closed)
    assert not np.allclose(vals[0], vals[1], rtol=1e-3)  # not a constant
    # on a node the table values themselves; Q alone: -A^2 Q sin 2 theta
    node = (np.array([A]), np.array([table[0][2]]), np.array([0.2]), np.array([0.0]))
    f = sr.PairSum(node, (table[0], np.zeros_like(table[1]), table[2])).force(0.0, 1.0)
    assert np.allclose(f, -A * A * table[2][:, 2, 2] * np.sin(0.4), rtol=1e-14, atol=0)


def test_reference_refuses_large_phases():
    comp = (np.array([1.0]), np.array([1.0]), np.array([0.1]), np.array([0.0]))
    with pytest.raises(AssertionError):
        sr.PairSum(comp, sr.random_table(2, 1, 0.5, 1.5)).force(1.0e4 + 1.0, 0.0)


def test_kernel_builds_without_scratch_or_spills_and_the_drift_kernel_is_still_there(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf not found"
    from hydrochrono_amd import build as hb
    assert "hc_qtf.hip" in hb.SOURCES
    co = str(tmp_path / "hc_qtf.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_qtf.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
                         r".*?\.vgpr_spill_count:\s+(\d+)", txt, re.S):
        notes[m.group(2)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(1)))
    assert any("sum_qtf_kernel" in n for n in notes) and any("drift_qtf_kernel" in n for n in notes), (sorted(notes), txt[:2000])
    for name, (scratch, vgpr, spills, lds) in notes.items():
        print(f"{name}: {vgpr} VGPRs, {lds} B LDS, scratch {scratch}, spills {spills}")
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert lds == (10240 if "sum_qtf_kernel" in name else 16384), (name, lds)  # one reduction column against drift_qtf_kernel's four
    # the names a HIP launch looks a kernel up by are plain strings of the built library
    blob = open(hb.MAIN_LIB, "rb").read()
    assert b"sum_qtf_kernel" in blob and b"drift_qtf_kernel" in blob


def test_abi_declares_the_sum_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_sum_qtf", "hc_get_sum_qtf_size", "hc_set_sum_mode", "hc_get_sum_mode", "hc_set_sum_options",
                 "hc_sum_qtf_begin", "hc_sum_qtf_end", "hc_compute_sum_qtf"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_sum_qtf_end(None, None) == capi.HC_ERR_INVALID
    assert lib.hc_set_sum_mode(None, 1) == capi.HC_ERR_INVALID


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/sumfreq_caller.cpp (SetSumQTF / SetSumMode / SetSumOptions / ComputeForceSumQTF of include/hydroc_amd/hydro_forces.h)
    builds with plain g++; tests/test_gpu_sumfreq.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "sumfreq_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "sumfreq_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
