"""The Morison term on the second-order sea in a short-crested sea without a GPU: the tests' NumPy restatement
(tests/morison2_dir_ref.py) against the long-crested one for equal directions and against itself in float64, the input sets of the
GPU tests (tests/morison2_dir_inputs.py) against the free surface, the entry points, and the build of the new kernels
(csrc/hc_morison.hip: no scratch, no spilled vector register).  The GPU side is tests/test_gpu_morison2_dir.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import morison2_dir_inputs as mdi
import morison2_dir_ref as md
import morison2_inputs as mi
import morison2_ref as m2
import morison_ref as mr
import wave_kinematics_ref as wk
from cases import load_into_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81
LD = np.longdouble


def solve_k(w, depth):
    k = w * w / G
    for _ in range(60):
        k = w * w / (G * np.tanh(k * depth))
    return k


def oracle_components(name):
    s = mdi.SETS[name]
    case = s["case"]()
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**s["waves"])
    comp = wk.irregular_components(orc.irreg_spectrum())
    assert comp[0].size == s["waves"]["nfrequencies"]
    return comp, case


@pytest.mark.parametrize("name", sorted(mdi.SETS))
def test_input_sets_keep_their_distance_from_the_free_surface(name):
    """The GPU comparison is made only where no element is closer than MIN_GAP to eta1 + eta2: shown here on the CPU oracle's
    spectrum (the GPU test asserts it again on the context's own), for every set, option pair and time, no exclusions."""
    comp, case = oracle_components(name)
    s = mdi.SETS[name]
    beta = mdi.directions(name)
    assert beta.size == comp[0].size
    for mwl, stretching in s["options"]:
        for t in s["times"]:
            ref, _ = mdi.reference(name, comp, abs(case["g"]), t, mwl, stretching)
            wet = np.concatenate(ref["wet"])
            print(f"{name} mwl={mwl} stretching={stretching} t={t}: margin {ref['margin']:.3e} m, {int(wet.sum())} of {wet.size} wet")
            assert ref["margin"] >= mdi.MIN_GAP
            assert wet.any() and (wet.size == 1 or not wet.all())  # wet and dry elements wherever there is more than one
            assert max(np.abs(e).max() for e in ref["eta2"] if e.size) > 0
            assert np.all(ref["bound"] < 1e-6 * np.abs(ref["F"]).max())
    # the y components of the increments are there in the spread sets
    if name in ("column_30m_spread", "many_elements", "three_deep_cos2s"):
        assert max(np.abs(u[:, 1]).max() for u in ref["u2"] if u.size) > 0 and max(np.abs(a[:, 1]).max() for a in ref["a2"] if a.size) > 0


def cardan_xyz(R):
    """(a, b, c) with R = Rx(a) Ry(b) Rz(c), |b| < pi / 2."""
    return np.array([np.arctan2(-R[1, 2], R[2, 2]), np.arcsin(R[0, 2]), np.arctan2(-R[0, 1], R[0, 0])], dtype=LD).astype(np.float64)


@pytest.mark.parametrize("depth", [40.0, np.inf])
@pytest.mark.parametrize("beta", [0.7, -2.9])
def test_equal_directions_are_the_long_crested_term_turned_about_z(depth, beta):
    """Every component at the heading beta: the sea is the long-crested one seen from a frame turned by beta about z.  The state
    turned by -beta (positions, velocities, and the orientation Rz(-beta) R written in Cardan angles again), evaluated by
    tests/morison2_ref.py, and the 6-vectors turned back, within the sum of both bounds (the long-crested one turned with |Rz|; the
    turned state is rounded to float64 once more: a few 2^-53 of |pos| + |r| in a phase, far inside either bound)."""
    w = np.array([0.5, 0.8, 1.3])
    k = w * w / G if np.isinf(depth) else solve_k(w, depth)
    comp = (np.array([0.6, 0.4, 0.2]), w, k, np.array([0.3, 1.1, -0.7]))
    elements = [mi.random_elements(20, 5, spread=6.0), None, mi.random_elements(3, 6)]
    t = 4.0
    state = mi.moving_state(3, -2.0, t)
    pos, rpy, lin, ang = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in state)
    c, s = np.cos(LD(beta)), np.sin(LD(beta))
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=LD)  # turns by +beta
    turn = lambda v: (v.astype(LD) @ Rz).astype(np.float64)      # rows: Rz^T v, the turn by -beta
    rpy_t = np.stack([cardan_xyz(Rz.T @ mr.rotation(rpy[b])) for b in range(3)])
    for b in range(3):
        assert np.max(np.abs(mr.rotation(rpy_t[b]) - Rz.T @ mr.rotation(rpy[b]))) < 1e-15
    for stretching in (False, True):
        kw = dict(mwl=0.2, stretching=stretching, ramp=0.5, diff_band=(0.0, 0.9), ramp_duration=8.0)
        got = md.morison2_dir(comp, np.full(3, beta), G, depth, RHO, elements, t, pos, rpy, lin, ang, **kw)
        lc = m2.morison2(comp, G, depth, RHO, elements, t, turn(pos), rpy_t, turn(lin), turn(ang), **kw)
        back = lambda v: np.concatenate([(v[:, :3].astype(LD) @ Rz.T), (v[:, 3:].astype(LD) @ Rz.T)], axis=1).astype(np.float64)
        aRz = np.abs(Rz).astype(np.float64)
        lc_bound = np.concatenate([lc["bound"][:, :3] @ aRz.T, lc["bound"][:, 3:] @ aRz.T], axis=1)
        err = np.abs(got["F"] - back(lc["F"]))
        print(f"depth {depth} beta {beta} stretching {stretching}: worst {np.max(err / np.maximum(got['bound'] + lc_bound, 1e-300)):.3e} of the bounds")
        assert np.all(err <= got["bound"] + lc_bound)
        assert all(np.array_equal(x, y) for x, y in zip(got["wet"], lc["wet"])) and abs(got["margin"] - lc["margin"]) < 1e-12
        assert np.abs(got["F"][[0, 2]][:, [0, 1]]).min() > 1.0 and not got["F"][1].any()  # F_x and F_y are both there
        # the increments: eta2 is a scalar, the vectors turn
        for b in (0, 2):
            assert np.allclose(got["eta2"][b], lc["eta2"][b], rtol=0, atol=1e-12 * np.abs(lc["eta2"][b]).max())
            assert np.allclose(got["u2"][b], (lc["u2"][b].astype(LD) @ Rz.T).astype(np.float64), rtol=0, atol=1e-12 * np.abs(lc["u2"][b]).max())
            assert np.abs(got["u2"][b][:, 1]).max() > 0
        # without the increments the result differs by far more than the bound: they show
        first = md.morison2_dir(comp, np.full(3, beta), G, depth, RHO, elements, t, pos, rpy, lin, ang,
                                **dict(kw, diff_band=(100.0, 200.0), sum_band=(100.0, 200.0)))
        assert np.all(np.abs(first["F"][[0, 2]] - got["F"][[0, 2]]).max(axis=1) > 100 * got["bound"][[0, 2]].max(axis=1))
        assert not any(e.any() for e in first["eta2"])


@pytest.mark.parametrize("name", sorted(mdi.SETS))
def test_float64_restatement_stays_within_its_own_bound(name):
    """The frame algebra and the pair sums in float64 (the first-order sums stay directional_ref's) against the longdouble
    restatement: inside the bound the GPU is held to, on every set."""
    comp, case = oracle_components(name)
    s = mdi.SETS[name]
    mwl, stretching = s["options"][0]
    t = s["times"][-1]
    ref, _ = mdi.reference(name, comp, abs(case["g"]), t, mwl, stretching)
    dbl, _ = mdi.reference(name, comp, abs(case["g"]), t, mwl, stretching, np.float64)
    err = np.abs(dbl["F"] - ref["F"])
    print(f"{name}: float64 off by {np.max(err / np.maximum(ref['bound'], 1e-300)):.3e} of the bound")
    assert np.all(np.isfinite(dbl["F"])) and np.all(err <= ref["bound"])
    assert all(np.array_equal(x, y) for x, y in zip(dbl["wet"], ref["wet"]))


def test_new_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(readelf), "llvm-readelf not found"
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_morison.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_morison.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(2): (int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(1))) for m in re.finditer(
        r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
        r".*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    incr = [n for n in notes if "morison2_incr_kernelILb1E" in n]  # the directional instantiation
    items = [n for n in notes if "morison2_dir_items_kernel" in n]
    assert len(incr) == 1 and len(items) == 1, sorted(notes)
    for name in incr + items:
        scratch, vgpr, spills, lds = notes[name]
        print(f"{name}: {vgpr} VGPRs, {lds} B LDS, {scratch} B scratch, {spills} spills")
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    # the increments kernel keeps the three workgroups per CU of wk2_dir_sum_kernel<true, true> (tests/test_wave2_dir_ref_cpu.py)
    _, vgpr, _, lds = notes[incr[0]]
    assert lds <= 160 * 1024 // 3 and vgpr <= 512 // 3, (vgpr, lds)
    assert "hc_wave_kin2_dir.hpp" in hb.HEADERS


def test_abi_declares_the_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "hydrochrono_amd.h")).read()
    for name in ("hc_set_morison_second_order_directional", "hc_get_morison_second_order_directional"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert lib.hc_set_morison_second_order_directional(None, 1) == capi.HC_ERR_INVALID
    assert lib.hc_get_morison_second_order_directional(None, None) == capi.HC_ERR_INVALID


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/morison2_dir_caller.cpp (SetMorisonSecondOrderDirectional of include/hydroc_amd/hydro_forces.h) builds with plain
    g++; tests/test_gpu_morison2_dir.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "morison2_dir_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison2_dir_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
