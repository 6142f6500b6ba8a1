"""The Morison strip members on the second-order sea without a GPU: the tests' restatement (tests/morison_members2_ref.py) against
the first-order restatement and a closed form, the inputs of the GPU tests (tests/morison_members2_inputs.py) against the conditions
those tests rely on, the build of the kernels (csrc/hc_morison_members.hip: no scratch, no spilled register, the order-1 kernels
with the registers they had), the entry points, and the host-only bookkeeping of the increment copies under the sanitizers.  The GPU
side is tests/test_gpu_morison_members2.py and tests/test_gpu_morison_members2_dir.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import morison_members2_inputs as mi
import morison_members2_ref as m2
import morison_members_ref as mm
import wave2_inputs as wi
import wave_kinematics_ref as wk
from cases import load_into_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, G = 1025.0, 9.81
Z3 = np.zeros(3)


def test_empty_bands_give_the_first_order_restatement():
    w = np.array([0.5, 0.8, 1.3])
    comp = (np.array([0.6, 0.4, 0.2]), w, w * w / G, np.array([0.3, 1.1, -0.7]))
    lists = [mi.body0(), None, mi.body2(False)]
    st = mi.moving_state(3, -1.0, 4.0)
    for stretching in (False, True):
        kw = dict(mwl=0.2, stretching=stretching, ramp=0.5)
        a = mm.members(comp, np.inf, RHO, lists, 4.0, *st, **kw)
        b = m2.members2(comp, G, np.inf, RHO, lists, 4.0, *st, diff_band=wi.NO_PAIR, sum_band=wi.NO_PAIR, ramp_duration=8.0, **kw)
        assert np.array_equal(a["F"], b["F"]) and a["margin"] == b["margin"] and a["cases"] == b["cases"]
        assert all(np.array_equal(x, y) for x, y in zip(a["members"], b["members"]))
        assert not any(e.any() for e in b["node_eta2"]) and not any(e.any() for e in b["u2"])
        full = m2.members2(comp, G, np.inf, RHO, lists, 4.0, *st, ramp_duration=8.0, **kw)
        assert np.all(np.abs(full["F"][[0, 2]] - a["F"][[0, 2]]) > 100 * full["bound"][[0, 2]])  # the increments show
        assert np.all(full["bound"][[0, 2]] >= a["bound"][[0, 2]]) and not full["F"][1].any()
        assert full["node_eta2"][0].shape == (5 + 4 + 4,) and full["eta2"][2].shape == (2 * (2 + 2 + 1),) and full["p"][1].shape == (0, 3)


def test_deep_water_regular_wave_moves_the_waterline_by_stokes_eta2():
    """One deep-water component on a fixed vertical column: eta2 = 1/2 k A^2 cos 2 theta and u2 = a2 = 0 (the sum-frequency potential
    vanishes in deep water), so the inertia force is the first-order load integrated to eta1 + eta2:
    F_x = rho cm (pi / 4) D^2 w^2 A sin(theta) (e^{k (eta1 + eta2)} - e^{-k draft}) / k, theta = -w t + phi at x = 0.
    With 32 segments the two-point rule is within 2.6e-8 of the integral (tests/test_morison_members_ref_cpu.py); the move of the
    waterline changes the force by k eta2 e^{k eta} / (e^{k eta} - e^{-k draft}), some 1e-2."""
    A, om, phi, t, D, cm, draft, top = 1.0, 1.1, 0.4, 2.0, 2.0, 2.0, 21.0, 6.0
    k = om * om / G
    comp = wk.regular_components(A, om, k, phi)
    th = -om * t + phi
    eta1, eta2 = A * np.cos(th), 0.5 * k * A * A * np.cos(2 * th)
    lists = [mm.member_lists([[0, 0, -draft]], [[0, 0, top]], D, 0.0, cm, 32)]
    ref = m2.members2(comp, G, np.inf, RHO, lists, t, Z3, Z3, Z3, Z3)
    assert np.allclose(ref["node_eta2"][0], eta2, rtol=1e-12, atol=0)
    assert np.abs(ref["u2"][0]).max() <= 1e-12 and np.abs(ref["a2"][0]).max() <= 1e-12
    exact = lambda eta: RHO * cm * np.pi / 4 * D * D * om * om * A * np.sin(th) * (np.exp(k * eta) - np.exp(-k * draft)) / k
    got = ref["F"][0, 0]
    assert abs(got - exact(eta1 + eta2)) <= 1e-6 * abs(exact(eta1 + eta2))
    assert abs(got - exact(eta1)) > 1e-4 * abs(exact(eta1))
    first = mm.members(comp, np.inf, RHO, lists, t, Z3, Z3, Z3, Z3)
    assert abs(first["F"][0, 0] - exact(eta1)) <= 1e-6 * abs(exact(eta1))


def oracle_components(name, directional):
    s = mi.SETS[name]
    case = s["case"]()
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**s["waves"])
    comp = mi.components(orc, name, directional)
    assert comp[0].size == s["waves"]["nfrequencies"]
    return case, comp


@pytest.mark.parametrize("directional", [False, True])
@pytest.mark.parametrize("name", sorted(mi.SETS))
def test_gpu_inputs_keep_the_conditions_the_gpu_tests_rely_on(name, directional):
    """Every node of every set clear of the free surface of eta1 + eta2 by more than its own bound, every segment case met, the
    increments live and the bound small against the force: conditions of the inputs, asserted on the restatement alone."""
    case, comp = oracle_components(name, directional)
    ref = mi.reference(name, comp, abs(case["g"]))
    first = mi.reference(name, comp, abs(case["g"]), second=False)
    print(f"{name} directional={directional}: margin {ref['margin']:.3e} m, eta bound {ref['eta_bound']:.3e} m, cases {ref['cases']}")
    mi.check_conditions(ref, name)
    for b in (0, 2):
        assert np.abs(ref["node_eta2"][b]).min() > 1e-6 and ref["wet"][b].any() and not ref["wet"][b].all()
        assert np.all(np.abs(ref["F"][b] - first["F"][b]).max() > 100 * ref["bound"][b].max())
        assert np.all(ref["bound"][b] < 1e-6 * np.abs(ref["F"][b]).max())
        if directional:
            assert np.abs(ref["u2"][b][:, 1]).max() > 0
    assert not ref["F"][1].any() and ref["node_eta2"][1].size == 0


@pytest.mark.parametrize("directional", [False, True])
def test_the_node_built_to_flip_flips_in_the_restatement(directional):
    name = "nf3_40m"
    case, comp = oracle_components(name, directional)
    g, depth, rd = abs(case["g"]), case["water_depth"], mi.SETS[name]["waves"]["ramp_duration"]
    lists, st, j = mi.flip_inputs(comp, g, depth, rd)
    ref = m2.members2(comp, g, depth, case["rho"], lists, mi.FLIP_T, *st, mwl=mi.MWL, ramp_duration=rd)
    first = mm.members(comp, depth, case["rho"], lists, mi.FLIP_T, *st, mwl=mi.MWL)
    h1, h = ref["node_h1"][0], ref["node_h"][0]
    print(f"flip: h1 {h1[j]:.3e}, h {h[j]:.3e}, eta bound {ref['eta_bound']:.3e}")
    assert h1[j] > ref["eta_bound"] and h[j] < -ref["eta_bound"]  # dry at order 1, wet at order 2
    mi.check_conditions(ref, "flip", need=("wet",))
    mi.check_conditions(first, "flip at order 1", need=("wet", "cut0"))
    assert "cut0" not in ref["cases"][0]
    assert np.all(np.abs(ref["members"][0][0] - first["members"][0][0])[[0, 4]] > ref["member_bound"][0][0][[0, 4]] + first["member_bound"][0][0][[0, 4]])


def test_the_bichromatic_column_keeps_the_conditions_the_gpu_test_relies_on():
    """On the CPU oracle's spectrum: every node clear of the surface, one cut segment, a set-down of one sign above 1e-5 m at every
    node, and a change of F_x above 100 times the bounds (mi.bichromatic_reference asserts them).  With these inputs the
    set-down is negative."""
    case = mi.finite_case()
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**mi.BICHROMATIC)
    comp = wk.irregular_components(orc.irreg_spectrum())
    assert comp[0].size == 2
    ref, first, expected = mi.bichromatic_reference(comp, abs(case["g"]), case)
    print(f"bichromatic: set-down {ref['node_eta2'][0][0]:.3e} m, F_x {first['F'][0, 0]:.6e} -> {ref['F'][0, 0]:.6e}, bound {ref['bound'][0, 0]:.3e}")
    assert expected == -1.0 and not ref["u2"][0][:, 1].any() and ref["wet"][0].any() and not ref["wet"][0].all()


def test_member_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_morison_members.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_morison_members.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {}  # name -> dict(lds, scratch, sgpr_spills, vgpr, vgpr_spills)
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+)"
                         r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S):
        notes[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), sgpr_spills=int(m.group(4)), vgpr=int(m.group(5)),
                                 vgpr_spills=int(m.group(6)))
    for kernel in ("morison_member2_nodes_kernel", "morison_member2_points_kernel", "morison_member2_items_kernel"):
        found = [n for n in notes if kernel in n]
        assert len(found) == 2, (kernel, sorted(notes))  # long-crested and directional
        for n in found:
            print(n, notes[n])
            # nothing goes to memory: no scratch, no spilled vector register (scalar registers the allocator parks in lanes of a
            # vector register -- sgpr_spills, the points kernel has some -- cost no memory access and are printed above)
            assert notes[n]["scratch"] == 0 and notes[n]["vgpr_spills"] == 0, (n, notes[n])
    # the points kernel stays inside the budget of morison2_incr_kernel (178 VGPRs, 43 KB of LDS): three workgroups per CU
    for n in notes:
        if "morison_member2_points_kernel" in n:
            assert notes[n]["vgpr"] <= 168 and notes[n]["lds"] <= 43 * 1024, (n, notes[n])
    # the two order-1 item kernels are the kernels they were (DESIGN.md 3.7c': 140 / 142 VGPRs, 16 / 20 KB of LDS, nothing spilled)
    order1 = sorted((notes[n]["vgpr"], notes[n]["lds"], notes[n]["scratch"], notes[n]["vgpr_spills"], notes[n]["sgpr_spills"])
                    for n in notes if "morison_member_items_kernel" in n)
    assert order1 == [(140, 16384, 0, 0, 0), (142, 20480, 0, 0, 0)], order1
    nodes1 = sorted((notes[n]["vgpr"], notes[n]["lds"], notes[n]["scratch"]) for n in notes if "morison_member_nodes_kernel" in n)
    assert nodes1 == [(80, 12288, 0), (84, 8192, 0)], nodes1
    assert "hc_member_increments.hpp" in hb.HEADERS


def test_abi_declares_the_entry_points():
    from hydrochrono_amd import capi
    lib = capi.load()
    for name in ("hc_set_morison_members_second_order", "hc_get_morison_members_second_order", "hc_get_morison_member_node_increments",
                 "hc_get_morison_member_point_increments", "hc_get_morison_member_increment_counts"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_set_morison_members_second_order(None, 1) == capi.HC_ERR_INVALID
    assert lib.hc_get_morison_member_node_increments(None, 0, None, None) == capi.HC_ERR_INVALID
    assert lib.hc_get_morison_member_point_increments(None, 0, None, None, None, None) == capi.HC_ERR_INVALID


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/morison_members2_caller.cpp (SetMorisonMembersSecondOrder / GetMorisonMemberIncrements of
    include/hydroc_amd/hydro_forces.h) builds with plain g++; tests/test_gpu_morison_members2.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "morison_members2_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "morison_members2_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)


def test_increment_copies_bookkeeping_under_the_sanitizers(tmp_path):
    """csrc/hc_member_increments.hpp, host only: a stand-alone program with its own main under AddressSanitizer and UBSan."""
    flags = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(flags + [str(probe), "-o", str(probe) + ".out"], capture_output=True).returncode != 0:
        pytest.skip("sanitizer runtime not available")
    exe = str(tmp_path / "member_increments_host_check")
    subprocess.run(flags + ["-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "member_increments_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failures"), r.stdout + r.stderr
