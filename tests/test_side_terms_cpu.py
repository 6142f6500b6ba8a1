"""The fixed inputs of tests/test_gpu_side_terms.py without a GPU (tests/side_terms_inputs.py): at every (wave model, time, state) the
GPU tests use, the three references are evaluated on the CPU oracle's spectrum (CreateSpectrum depends on the parameters alone; the GPU
tests take the context's own) and the conditions the references need are asserted --
  * no Morison element and no panel centroid closer than 1e-6 m to the free surface (the wet tests are discontinuities);
  * 0 < wet < n for every list with more than one entry;
  * the drift grids hold the regular wave's frequency, and between 10 and nf - 10 of a spectrum's components (a model with fewer
    than 21 components: at least one inside and one outside); |theta_i| < 1e4 (drift_ref asserts it in force());
  * every term is non-zero on the bodies that carry it (the drift term in waves with components).
These are conditions, not tolerances: an input that misses one is replaced, the condition stays.
Also here: tests/cpp/side_terms_caller.cpp compiles against the C++ mirror with plain g++."""
import os
import subprocess

import numpy as np
import pytest

import drift_ref as dr
import morison_ref as mr
import side_terms_inputs as si
from cases import four_body_case, load_into_oracle, three_body_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_state(case, lists, comp, t, state, ramp, nl_opts, mor_opts, stretching_applies, what):
    ref = si.references(case, lists, comp, t, state, ramp, nl_opts, mor_opts, stretching_applies)
    si.check_conditions(ref, lists, what)
    return ref


def check_nonzero(case, lists, comp, t, state, ramp, ref, what, drift_expected):
    N = len(lists["panels"])
    for b in range(N):
        has = lists["panels"][b] is not None
        assert bool(ref["nl"]["buoy"][b].any()) == has, (what, "buoy", b)
        if comp is not None and ramp > 0.0:
            assert bool(ref["nl"]["fk"][b].any()) == has, (what, "fk", b)
        assert bool(ref["mor"]["F"][b].any()) == (lists["elements"][b] is not None), (what, "morison", b)
    pos = np.asarray(state[0]).reshape(-1, 3)
    for b, ps in enumerate(si.drift_refs(comp, lists)):
        if ps is None:
            continue
        F = ps.force(t, pos[b, 0], ramp=ramp)  # asserts |theta| < 1e4
        if drift_expected:
            for mode in (1, 2, 3):
                assert np.abs(F[mode]).max() > 1.0, (what, "drift", b, mode)


def test_compose_inputs_keep_the_references_conditions():
    """sections 2, 3 and 6: three_body_case() in THREE_IRREG, every step of every combination"""
    case = three_body_case()
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**si.THREE_IRREG)
    comp, rd, stretch = si.model_components(orc, "irregular", si.THREE_IRREG, 0.0)
    orc.close()
    assert comp[0].size == 200
    lists = si.compose_lists()
    assert [0 if p is None else len(p[0]) for p in lists["panels"]] == [257, 0, 5]
    assert [0 if e is None else len(e[0]) for e in lists["elements"]] == [0, 7, 300]
    assert [0 if tb is None else len(tb[0]) for tb in lists["tables"]] == [9, 0, 33] and lists["tables"][2][2] is None
    si.check_grids(comp, lists, "THREE_IRREG")
    motion = si.compose_motion(case)
    times = sorted(set(si.COMPOSE_TIMES.tolist()) | set(si.SUBSET_TIMES.tolist()))
    assert max(times) < rd  # all inside the ramp
    for t in times:
        ramp = mr.ramp_factor(t, rd)
        st = motion.state(t)
        ref = check_state(case, lists, comp, t, st, ramp, si.NL_OPTS, si.MOR_OPTS, stretch, f"compose t={t}")
        if t in (times[0], times[-1], si.SUBSET_TIMES[0]):
            check_nonzero(case, lists, comp, t, st, ramp, ref, f"compose t={t}", True)


def test_sequence_inputs_keep_the_references_conditions():
    """section 4 (and the regular model of section 5): synth_case(3) under every model of SEQUENCE at SEQ_TIMES"""
    case = si.synth_case()
    lists = si.sequence_lists()
    seen_nf = set()
    for name, kind, params, mor_phase in si.SEQUENCE:
        orc = load_into_oracle(case)
        if kind == "regular":
            orc.add_waves_regular(*params)
        elif kind in ("irregular", "spectral"):  # the spectral mode synthesises from the same spectrum
            orc.add_waves_irregular(**params)
        for term_phase, which in ((si.SEQ_PHASE, "nl+drift"), (mor_phase, "morison")):
            comp, rd, stretch = si.model_components(orc, kind, params, term_phase)
            if comp is not None:
                si.check_grids(comp, lists, name, regular=kind == "regular")
                seen_nf.add(comp[0].size)
            for t in si.SEQ_TIMES:
                ramp = mr.ramp_factor(t, rd)
                st = si.sequence_state(t)
                what = f"{name} ({which}) t={t}"
                ref = check_state(case, lists, comp, t, st, ramp, si.NL_OPTS, si.MOR_OPTS, stretch, what)
                check_nonzero(case, lists, comp, t, st, ramp, ref, what, comp is not None)
        orc.close()
    assert seen_nf == {1, 5, 255, 257}
    assert 0.0 < si.SEQ_TIMES[0] < 20.0 < si.SEQ_TIMES[1]


def test_pending_inputs_keep_the_references_conditions():
    """section 5: synth_case(3), irregular nf 257 at the begin, REG1 afterwards, at SEQ_TIMES[1]"""
    case = si.synth_case()
    lists = si.sequence_lists()
    t = si.SEQ_TIMES[1]
    st = si.sequence_state(t)
    for kind, params in (("irregular", si.irreg(257)), ("regular", si.REG1)):
        orc = load_into_oracle(case)
        (orc.add_waves_regular(*params) if kind == "regular" else orc.add_waves_irregular(**params))
        comp, rd, stretch = si.model_components(orc, kind, params, si.SEQ_PHASE)
        orc.close()
        ramp = mr.ramp_factor(t, rd)
        ref = check_state(case, lists, comp, t, st, ramp, si.NL_OPTS, si.MOR_OPTS, stretch, f"pending {kind}")
        check_nonzero(case, lists, comp, t, st, ramp, ref, f"pending {kind}", True)


def test_cpp_caller_inputs_keep_the_references_conditions():
    """section 7: the states, lists and tables tests/cpp/side_terms_caller.cpp builds, on four_body.h5 in THREE_IRREG"""
    case = four_body_case()
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**si.THREE_IRREG)
    comp, rd, stretch = si.model_components(orc, "irregular", si.THREE_IRREG, 0.0)
    orc.close()
    lists = si.cpp_lists()
    for key, bodies in (("panels", si.CPP_PANEL_BODIES), ("elements", si.CPP_ELEMENT_BODIES), ("tables", si.CPP_TABLE_BODIES)):
        assert tuple(b for b in range(4) if lists[key][b] is not None) == bodies
    si.check_grids(comp, lists, "cpp caller")
    for n in range(si.CPP_STEPS + 1):  # the last one is the cleared evaluation: no wet test there, checked all the same
        t, st = si.cpp_state(n)
        assert t < rd
        ramp = mr.ramp_factor(t, rd)
        ref = check_state(case, lists, comp, t, st, ramp, si.CPP_NL_OPTS, si.CPP_MOR_OPTS, stretch, f"cpp step {n}")
        if n in (0, si.CPP_SWITCH, si.CPP_STEPS - 1):
            check_nonzero(case, lists, comp, t, st, ramp, ref, f"cpp step {n}", True)


def test_composition_helper_keeps_the_order():
    """compose() is ((total - hs + buoy [+ fk]) + morison) + drift; with these values every other association rounds differently"""
    total, hs, buoy, fk = (np.full(6, v) for v in (1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53))
    mor, dft = np.full(6, 2.0 ** -53), np.full(6, 2.0 ** -53)
    got = si.compose(total, (buoy, fk, hs), mor, dft, 2, (0,))
    assert si.same_bits(got, ((((total - hs) + buoy) + fk) + mor) + dft)
    assert not si.same_bits(got, total + (mor + dft) + (buoy - hs + fk))
    assert si.same_bits(si.compose(total, None, None, None, 2, (0,)), total)
    big = np.array([1e16, 1.0, -1e16, 3.0, 0.5, 0.25])
    assert not si.same_bits((big + 1.0) + -1e16, (big + -1e16) + 1.0)  # Morison and drift swapped is visible in floating point


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/side_terms_caller.cpp (all three terms on four bodies and a device list through include/hydroc_amd/hydro_forces.h)
    builds with plain g++; tests/test_gpu_side_terms.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "side_terms_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "side_terms_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)


def test_the_margin_condition_is_the_references_own():
    assert si.MIN_GAP == 1e-6 and dr.THETA_MAX == 1e4
    with pytest.raises(AssertionError):
        si.check_conditions(dict(nl=dict(margin=9e-7, wet=[]), mor=dict(margin=1.0, wet=[])), None, "too close")
