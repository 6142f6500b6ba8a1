"""The Morison term on the second-order sea without a GPU: the tests' NumPy restatement (tests/morison2_ref.py) against the
first-order restatement and Stokes' closed form, the input sets of the GPU tests against the free surface, and the build of the
kernels (csrc/hc_morison.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_morison2.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import morison2_inputs as mi
import morison2_ref as m2
import morison_ref as mr
import wave2_inputs as wi
import wave2_ref as w2
import wave_kinematics_ref as wk
from cases import load_into_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81


def solve_k(w, depth):
    k = w * w / G
    for _ in range(60):
        k = w * w / (G * np.tanh(k * depth))
    return k


def test_empty_bands_give_the_first_order_restatement():
    w = np.array([0.5, 0.8, 1.3])
    comp = (np.array([0.6, 0.4, 0.2]), w, solve_k(w, 40.0), np.array([0.3, 1.1, -0.7]))
    elements = [mi.random_elements(20, 5, spread=6.0), None, mi.random_elements(3, 6)]
    state = mi.moving_state(3, -2.0, 4.0)
    for stretching in (False, True):
        kw = dict(mwl=0.2, stretching=stretching, ramp=0.5)
        a = mr.morison(comp, 40.0, RHO, elements, 4.0, *state, **kw)
        b = m2.morison2(comp, G, 40.0, RHO, elements, 4.0, *state, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR, ramp_duration=8.0, **kw)
        assert np.array_equal(a["F"], b["F"]) and a["margin"] == b["margin"]
        assert all(np.array_equal(x, y) for x, y in zip(a["wet"], b["wet"]))
        assert np.allclose(a["bound"], b["bound"], rtol=1e-12, atol=0)
        full = m2.morison2(comp, G, 40.0, RHO, elements, 4.0, *state, ramp_duration=8.0, **kw)
        assert np.all(np.abs(full["F"][[0, 2]] - a["F"][[0, 2]]) > 100 * full["bound"][[0, 2]])  # the increments show
        assert np.all(full["bound"] >= a["bound"]) and not full["F"][1].any()
    still = m2.morison2(None, G, 40.0, RHO, elements, 4.0, *state)
    assert np.array_equal(still["F"], mr.morison(None, 40.0, RHO, elements, 4.0, *state)["F"])


def test_one_regular_component_in_finite_depth_sees_stokes_second_order():
    A, w, depth, phi, t = 0.5, 0.9, 25.0, 0.4, 3.3
    k = solve_k(w, depth)
    comp = wk.regular_components(A, w, k, phi)
    r = np.array([[0.0, 0.0, -4.0], [0.0, 0.0, 2.0]])  # the second one above the mean level: held at z2 = 0, and dry
    el = [(r, np.ones((2, 3)), np.ones((2, 3)))]
    pos = [7.0, 0.0, 0.0]
    out = m2.morison2(comp, G, depth, RHO, el, t, pos, np.zeros(3), np.zeros(3), np.zeros(3))
    theta = k * 7.0 - w * t + phi
    assert np.allclose(out["eta2"][0], w2.stokes_eta2(A, k, depth, theta), rtol=1e-9, atol=0)
    assert out["eta2"][0][0] == out["eta2"][0][1]  # eta2 does not depend on z
    # Stokes' second-order potential 3/8 A^2 w cosh(2 k (z + h)) / sinh^4(k h) sin 2 theta
    c = 0.75 * A * A * w * k / np.sinh(k * depth) ** 4
    for e, z2 in ((0, -4.0), (1, 0.0)):
        ch, sh = np.cosh(2 * k * (z2 + depth)), np.sinh(2 * k * (z2 + depth))
        assert np.allclose(out["u2"][0][e], [c * ch * np.cos(2 * theta), 0.0, c * sh * np.sin(2 * theta)], rtol=1e-9, atol=0)
        assert np.allclose(out["a2"][0][e], [2 * w * c * ch * np.sin(2 * theta), 0.0, -2 * w * c * sh * np.cos(2 * theta)], rtol=1e-9, atol=0)
    assert list(out["wet"][0]) == [True, False]
    first = mr.morison(comp, depth, RHO, el, t, pos, np.zeros(3), np.zeros(3), np.zeros(3))
    assert abs(out["F"][0, 0] - first["F"][0, 0]) > 1e-4 * abs(first["F"][0, 0])
    # twice the ramp duration in: the increments carry ramp^2 = 1; half way in: a quarter
    half = m2.morison2(comp, G, depth, RHO, el, t, pos, np.zeros(3), np.zeros(3), np.zeros(3), ramp_duration=2 * t)
    assert np.allclose(half["u2"][0], 0.25 * out["u2"][0], rtol=1e-15, atol=0)
    assert np.allclose(half["eta2"][0], 0.25 * out["eta2"][0], rtol=1e-15, atol=0)


@pytest.mark.parametrize("name", sorted(mi.SETS))
def test_input_sets_keep_their_distance_from_the_free_surface(name):
    """The GPU comparison is made only where no element is closer than MIN_GAP to eta1 + eta2: shown here on the CPU oracle's
    spectrum (the GPU test asserts it again on the context's own), with wet and dry elements in every set."""
    s = mi.SETS[name]
    case = s["case"]()
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**s["waves"])
    comp = wk.irregular_components(orc.irreg_spectrum())
    assert comp[0].size == s["waves"]["nfrequencies"]
    for mwl, stretching in s["options"]:
        for t in s["times"]:
            ref, _ = mi.reference(name, comp, abs(case["g"]), t, mwl, stretching)
            wet = np.concatenate(ref["wet"])
            print(f"{name} mwl={mwl} stretching={stretching} t={t}: margin {ref['margin']:.3e} m, {int(wet.sum())} of {wet.size} wet")
            assert ref["margin"] >= mi.MIN_GAP
            assert 0 < wet.sum() < wet.size
            assert max(np.abs(e).max() for e in ref["eta2"] if e.size) > 0 and np.all(ref["bound"] < 1e-6 * np.abs(ref["F"]).max())


def test_new_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_morison.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_morison.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    incr = [n for n in notes if "morison2_incr_kernelILb0E" in n]  # the long-crested instantiation
    items = [n for n in notes if "morison_items_kernel" in n]
    assert len(incr) == 1 and len(items) == 2, sorted(notes)  # the increments, and the item kernel of order 1 and of order 2
    for name in incr + items:
        scratch, vgpr, spills = notes[name]
        print(name, "vgpr", vgpr)
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert "hc_wave_kin2_sum.hpp" in hb.HEADERS


def test_abi_declares_the_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_morison_second_order", "hc_get_morison_second_order", "hc_get_morison_increments"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_set_morison_second_order(None, 1, 0.0, 1.0, 0.0, 1.0, 1) == capi.HC_ERR_INVALID
    assert lib.hc_get_morison_increments(None, 0, None, None, None, None) == capi.HC_ERR_INVALID


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/morison2_caller.cpp (SetMorisonSecondOrder / GetMorisonIncrements of include/hydroc_amd/hydro_forces.h) builds with
    plain g++; tests/test_gpu_morison2.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "morison2_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison2_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
