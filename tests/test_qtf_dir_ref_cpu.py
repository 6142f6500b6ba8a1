"""The QTF terms on a heading x frequency grid without a GPU: the projected evaluation form in float64 against the
direct pair sum of the definition in longdouble (tests/qtf_dir_ref.py), inside the derived bound; the reduction to the one-heading
references on a heading node; the build of the kernels (csrc/hc_qtf_dir.hip: no scratch, no spilled register); the entry points.  The
GPU side is tests/test_gpu_qtf_dir.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import drift_ref as dr
import qtf_dir_ref as qd
import sumfreq_ref as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81


def components(nf, seed, tlo, thi, lo=0.25, hi=2.4):
    """nf deep-water components, some of them outside [0.4, 2.0], with directions in [tlo, thi]"""
    rng = np.random.default_rng(seed)
    w = np.sort(rng.uniform(lo, hi, size=nf))
    A = rng.uniform(0.01, 0.3, size=nf)
    return A, w, w * w / G, rng.uniform(0.0, 2 * np.pi, size=nf), rng.uniform(tlo, thi, size=nf)


@pytest.mark.parametrize("nf,nh,nq", [(1, 2, 2), (7, 1, 2), (257, 3, 5), (64, 4, 9)])
def test_projected_form_equals_the_pair_sum(nf, nh, nq):
    table = qd.random_table(nh, nq, 20 + nq, -0.6, 0.9, 0.4, 2.0)
    tlo, thi = (table[0][0], table[0][-1])
    comp = components(nf, 10 + nf, tlo, thi)
    if nf == 1:
        comp = (np.array([0.2]), np.array([1.1]), np.array([1.1 ** 2 / G]), np.array([0.4]), np.array([0.5 * (tlo + thi)]))
    if nf > 7:  # some on heading nodes, both ends among them
        comp[4][:3] = table[0][[0, -1, nh // 2]]
    inside = dr.cells(table[1], comp[1])[0]
    assert inside.any() and (nf < 7 or not inside.all())
    ref = qd.PairSum(comp, table)
    worst = 0.0
    for t, x, y in ((0.0, 0.0, 0.0), (431.0, 850.0, -300.0), (77.7, -120.5, 64.0)):  # |psi| < 1150 * 2.4^2 / g + 2.4 * 431 + 2 pi < 1800
        want, bound = ref.force(t, x, y, ramp=0.5), qd.bounds(comp, table, ramp=0.5)
        for key in qd.KEYS:
            got = qd.projected(comp, table, t, x, y, key, ramp=0.5)
            err = np.abs(got - want[key])
            assert np.all(bound[key] > 0)
            worst = max(worst, float(np.max(err / bound[key])))
            assert np.all(err <= bound[key]), (key, t, x, y, float(np.max(err / bound[key])))
    print(f"nf={nf} nh={nh} nq={nq}: worst |projected - pair sum| / bound = {worst:.3e}")
    # Q = None is Q = 0
    beta, g, P, Q = table
    for key in (3, "sum"):
        assert np.array_equal(qd.projected(comp, (beta, g, P, None), 3.0, 5.0, 2.0, key), qd.projected(comp, (beta, g, P, np.zeros_like(Q)), 3.0, 5.0, 2.0, key))
        assert np.array_equal(qd.PairSum(comp, (beta, g, P, None)).force(3.0, 5.0, 2.0)[key],
                              qd.PairSum(comp, (beta, g, P, np.zeros_like(Q))).force(3.0, 5.0, 2.0)[key])


@pytest.mark.parametrize("a", [0, 1, 2])
def test_on_one_heading_node_it_is_the_one_heading_table(a):
    """every theta_i = beta_a and y = 0: the pair sums of tests/drift_ref.py and tests/sumfreq_ref.py on the sub-table T[a][a]"""
    table = qd.random_table(3, 6, 7, 0.0, 1.1, 0.4, 2.0)
    beta, g, P, Q = table
    A, w, k, phi, _ = components(40, 3, 0.0, 1.0)
    th = beta[a]
    comp = (A, w, k, phi, np.full(40, th))
    # the one-heading references see k x: give them the wavenumber along x, k cos(theta), as this file rounds it
    comp1 = (A, w, (k.astype(qd.LD) * np.cos(qd.LD(th))).astype(np.float64), phi)
    sub = (g, P[:, a, a], Q[:, a, a])
    t, x = 12.5, 30.0
    got = qd.PairSum(comp, table).force(t, x, 0.0, ramp=0.7)
    want, bound = dr.PairSum(comp1, sub).force(t, x, ramp=0.7), dr.bounds(comp1, sub, ramp=0.7)
    for mode in (1, 2, 3):  # two longdouble sums of the same terms: far inside the float64 bound (the rounded k cos theta: 1e-16 * 30)
        assert np.all(np.abs(got[mode] - want[mode]) <= 0.01 * bound[mode]), mode
    assert np.all(np.abs(got["sum"] - sf.PairSum(comp1, sub).force(t, x, ramp=0.7)) <= 0.01 * sf.bound(comp1, sub, ramp=0.7))
    # the bound is the one-heading bound with J^2 for nq^2 in the summation part
    bd = qd.bounds(comp, table, ramp=0.7)
    for mode in (1, 2, 3):
        assert np.all(bd[mode] >= bound[mode]) and np.all(bd[mode] <= 1.01 * bound[mode])


def test_heading_cells_and_ends():
    beta = np.array([-0.5, 0.0, 0.75])
    a, a1, mu, ok = qd.head_cells(beta, np.array([-0.5, 0.0, 0.75, 0.375, np.nextafter(0.75, 1.0), np.nextafter(-0.5, -1.0), -0.25]))
    assert list(ok) == [True, True, True, True, False, False, True]
    assert list(a[:4]) == [0, 1, 2, 1] and list(mu[:4]) == [0.0, 0.0, 0.0, 0.5] and a1[2] == 2 and mu[6] == 0.5
    one = qd.head_cells(np.array([0.3]), np.array([0.3, 0.3000001]))
    assert list(one[3]) == [True, False] and list(one[2]) == [0.0, 0.0]
    table = (beta, np.array([0.4, 2.0]), np.zeros((6, 3, 3, 2, 2)), None)
    with pytest.raises(AssertionError):  # inside the frequency grid, outside the heading grid
        qd.node_weights(table, np.array([1.0]), np.array([0.8]))
    assert not qd.node_weights(table, np.array([2.5]), np.array([0.8])).any()  # outside the frequency grid: no part, whatever its heading
    W = qd.node_weights(table, np.array([0.4]), np.array([0.0]))  # on a heading node and a frequency node: one node
    assert np.count_nonzero(W) == 1 and W[0, 1 * 2 + 0] == 1.0


def test_reference_refuses_large_phases():
    comp = (np.array([1.0]), np.array([1.0]), np.array([0.1]), np.array([0.0]), np.array([0.5]))
    table = qd.random_table(2, 2, 1, 0.0, 1.0, 0.5, 1.5)
    with pytest.raises(AssertionError):
        qd.PairSum(comp, table).force(1.0e4 + 1.0, 0.0, 0.0)
    with pytest.raises(AssertionError):
        qd.PairSum(comp, table).force(0.0, 0.0, 3.0e5)


def test_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf not found"
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_qtf_dir.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_qtf_dir.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(2): (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(1))) for m in re.finditer(
        r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
        r".*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    assert sum("qtf_dir_pair_kernel" in n for n in notes) == 2 and sum("qtf_dir_finish_kernel" in n for n in notes) == 2, sorted(notes)
    for name, (scratch, vgpr, spills, lds) in sorted(notes.items()):
        print(f"{name}: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert lds <= 160 * 1024 // 3, (name, lds)  # at least three workgroups per CU
        assert vgpr <= 128, (name, vgpr)  # and the registers of 256 lanes allow as many
    assert "hc_qtf.hip" in hb.SOURCES and "hc_qtf_dir.hip" in hb.SOURCES


def test_abi_declares_the_heading_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_drift_qtf_headings", "hc_get_drift_qtf_headings", "hc_set_sum_qtf_headings", "hc_get_sum_qtf_headings"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_set_drift_qtf_headings(None, 0, 1, None, 2, None, None, None) == capi.HC_ERR_INVALID
    assert lib.hc_get_sum_qtf_headings(None, 0, None) == capi.HC_ERR_INVALID
    header = open(os.path.join(ROOT, "include", "hydrochrono_amd.h")).read()
    for name in ("hc_set_drift_qtf_headings", "hc_get_drift_qtf_headings", "hc_set_sum_qtf_headings", "hc_get_sum_qtf_headings"):
        assert re.search(r"\bint " + name + r"\(", header), name


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/qtf_dir_caller.cpp (SetDriftQTFHeadings / SetSumQTFHeadings of include/hydroc_amd/hydro_forces.h) builds with plain
    g++; tests/test_gpu_qtf_dir.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "qtf_dir_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "qtf_dir_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
