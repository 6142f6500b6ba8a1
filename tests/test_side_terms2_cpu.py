"""The fixed inputs of tests/test_gpu_side_terms2.py without a GPU (tests/side_terms2_inputs.py): at every (wave model, time,
state) the GPU test holds to a reference, the references are evaluated on the CPU oracle's spectrum (CreateSpectrum depends on the
parameters alone; the GPU test takes the context's own and asserts the same again) and the conditions they need are asserted --
  * no Morison element and no panel centroid closer than MIN_GAP to eta1 + eta2, no cut edge shorter than MIN_SPAN in h;
  * every list with more than one item partly wet and partly dry; over the times used the triangle body's case counts include 0, 1,
    2 and 3 wet vertices;
  * every drift and sum grid passes si.check_grids for every model of the walk; |theta_i| < 1e4 (the pair sums assert it);
  * every band setting of the walk holds a pair where the walk says order 2 and none where it says order 1;
  * every derived bound is below 1e-6 of the largest component of its result.
These are conditions, not tolerances: an input that misses one is replaced by the next seed, the condition stays.
Also here: compose4 keeps its order, and tests/cpp/side_terms2_caller.cpp compiles against the C++ mirror with plain g++."""
import os
import subprocess
import time

import numpy as np

import nonlinear2_inputs as ni
import side_terms2_inputs as s2
import side_terms_inputs as si
from cases import load_into_oracle, three_body_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_components(case, kind, params, phases):
    orc = load_into_oracle(case)
    if kind == "regular":
        orc.add_waves_regular(*params)
    elif kind in ("irregular", "spectral"):  # the spectral mode synthesises from the same spectrum
        orc.add_waves_irregular(**params)
    out = s2.model_components(orc, kind, params, phases)
    orc.close()
    return out


def check_compose(small, nf, steps):
    case = three_body_case()
    lists = s2.compose_lists(small=small)
    waves = ni.waves(nf)
    comps, rd, stretch = oracle_components(case, "irregular", waves, dict(nl=0.0, mor=0.0, dft=0.0, sum=0.0))
    assert comps["nl"][0].size == nf and max(s2.COMPOSE_TIMES) < rd
    s2.check_grids(comps["dft"], lists, lists["sums"], f"waves({nf})")
    assert min(s2.pair_counts(comps["nl"][1], (s2.FULL, s2.FULL))) > 0
    motion = s2.compose_motion()
    seen = np.zeros(4, dtype=int)
    t0 = time.perf_counter()
    for n in steps:
        t = float(s2.COMPOSE_TIMES[n])
        what = f"compose nf={nf} step {n}"
        ref = s2.references(case, case["g"], lists, lists["sums"], comps, rd, stretch, t, motion.state(t), (s2.FULL, s2.FULL))
        seen += s2.check_conditions(ref, lists, what)
        s2.check_qtf_conditions(ref, what)
        for b in range(3):
            assert bool(ref["nl"]["buoy"][b].any()) == bool(ref["nl"]["fk"][b].any()) == (lists["surfaces"][b] is not None), (what, b)
            assert bool(ref["mor"]["F"][b].any()) == (lists["elements"][b] is not None), (what, b)
    print(f"references of {len(steps)} steps at nf={nf}: {time.perf_counter() - t0:.1f} s; case counts {seen.tolist()}")
    return seen


def test_compose_inputs_keep_the_references_conditions():
    """section 1a: the full lists in waves(5) at the three steps held to the references"""
    lists = s2.compose_lists()
    assert [len(l[1]) if l and l[0] == "tris" else 0 for l in lists["surfaces"]] == [257, 0, 0]
    assert [len(l[1][0]) if l and l[0] == "panels" else 0 for l in lists["surfaces"]] == [0, 0, 5]
    assert [0 if e is None else len(e[0]) for e in lists["elements"]] == [0, 7, 300]
    for key in ("tables", "sums"):
        assert [0 if tb is None else len(tb[0]) for tb in lists[key]] == [9, 0, 33] and lists[key][0][2] is not None and lists[key][2][2] is None
    for b in (0, 2):  # the sum tables sit on another grid than the drift tables
        assert not np.intersect1d(lists["tables"][b][0], lists["sums"][b][0]).size
    seen = check_compose(False, 5, s2.BOUND_STEPS)
    assert np.all(seen > 0), seen.tolist()  # triangles with 0, 1, 2 and 3 wet vertices


def test_large_nf_inputs_keep_the_references_conditions():
    """section 1b: the small lists in waves(300), above one tile of 256 components, at the one step held to the references"""
    lists = s2.compose_lists(small=True)
    assert len(lists["surfaces"][0][1]) == 12 and len(lists["surfaces"][2][1][0]) == 12 and len(lists["elements"][2][0]) == 12
    check_compose(True, 300, (s2.BOUND_STEP_LARGE,))


def test_walk_inputs_keep_the_references_conditions():
    """section 3 (and the two models of section 4): synth_case(3) under every entry of WALK at SEQ_TIMES"""
    case = si.synth_case()
    lists = s2.sequence_lists()
    seen = np.zeros(4, dtype=int)
    seen_nf = set()
    t0 = time.perf_counter()
    for i, (name, kind, params, mor_phase, nl_bands, sums_key, orders, _) in enumerate(s2.WALK):
        sums = s2.walk_sums(lists, sums_key)
        phases = dict(nl=si.SEQ_PHASE, mor=mor_phase, dft=si.SEQ_PHASE, sum=si.SEQ_PHASE)
        comps, rd, stretch = oracle_components(case, kind, params, phases)
        if comps["nl"] is None:
            assert orders == (1, 1), name
            continue
        seen_nf.add(comps["nl"][0].size)
        s2.check_grids(comps["dft"], lists, sums, name, regular=kind == "regular")
        # order 2 where the walk says so: a pair inside a band; order 1: none in either
        for order, bands in ((orders[0], nl_bands), (orders[1], (s2.FULL, s2.FULL))):
            assert (sum(s2.pair_counts(comps["nl"][1], bands)) > 0) == (order == 2), (name, bands)
        if nl_bands == s2.DIFF_ONLY:
            assert s2.pair_counts(comps["nl"][1], nl_bands)[1] == 0 < s2.pair_counts(comps["nl"][1], nl_bands)[0]
        for t in si.SEQ_TIMES:
            st = si.sequence_state(t)
            what = f"{name} t={t}"
            if i in s2.HELD:
                ref = s2.references(case, case["g"], lists, sums, comps, rd, stretch, t, st, nl_bands, drift_modes=(1, 3))
                seen += s2.check_conditions(ref, lists, what)
            else:  # the pair sums assert |theta| < 1e4 for every model of the walk; entry 3 holds them to their bounds
                ref = s2.qtf_references(lists, sums, comps, rd, t, st[0], drift_modes=(1, 3))
            if i in s2.HELD + s2.HELD_QTF:
                s2.check_qtf_conditions(ref, what)
            for rows in (ref["dft"][1], ref["dft"][3], ref["sum"]):
                assert all(r is None or np.abs(r[0]).max() > 0.0 for r in rows), what
    print(f"references of the walk: {time.perf_counter() - t0:.1f} s; case counts {seen.tolist()}")
    assert seen_nf == {1, 5, 255, 257} and np.all(seen > 0), (seen_nf, seen.tolist())
    assert [s2.WALK[i][0][0] for i in s2.HELD] == ["1", "8", "9"] and s2.WALK[s2.HELD_QTF[0]][0].startswith("3 ")
    nine = s2.sum_tables_nine()
    assert nine[0] is None and len(nine[2][0]) == 17


def test_compose4_keeps_the_order():
    """compose4() is (((total - hs + buoy [+ fk]) + morison) + drift) + sum; with these values another association rounds differently"""
    total, tiny = np.full(6, 1.0), np.full(6, 2.0 ** -53)
    got = s2.compose4(total, (tiny, tiny, tiny), tiny, tiny, tiny, 2, (0,))
    assert si.same_bits(got, (((((total - tiny) + tiny) + tiny) + tiny) + tiny) + tiny)
    assert not si.same_bits(got, total + ((tiny + tiny) + (tiny + tiny)))
    assert si.same_bits(s2.compose4(total, None, None, None, None, 2, (0,)), total)
    assert si.same_bits(s2.compose4(total, None, tiny, tiny, None, 2, (0,)), si.compose(total, None, tiny, tiny, 2, (0,)))
    big, one = np.array([1e16, 1.0, -1e16, 3.0, 0.5, 0.25]), np.full(6, 1.0)
    drift_last = s2.compose4(big, None, None, one, -big, 0, ())   # (big + 1) - big
    sum_first = s2.compose4(big, None, None, -big, one, 0, ())    # (big - big) + 1: the drift and sum terms swapped
    assert not si.same_bits(drift_last, sum_first)


def test_cpp_caller_inputs():
    """section 6: dyadic grids and tables, the sum grids beside the drift grids"""
    lists = s2.cpp_lists()
    assert tuple(b for b in range(4) if lists["surfaces"][b] is not None) == s2.CPP_SURFACE_BODIES
    assert tuple(b for b in range(4) if lists["sums"][b] is not None) == s2.CPP_SUM_BODIES
    assert lists["surfaces"][0][1].shape == (12, 3, 3) and np.unique(lists["surfaces"][0][1].reshape(-1, 3), axis=0).shape == (8, 3)
    for tb in lists["sums"]:
        if tb is not None:
            assert np.all(np.diff(tb[0]) > 0) and np.array_equal(tb[0] * 32, np.round(tb[0] * 32))
    assert lists["sums"][2][0][0] != lists["tables"][0][0][0] and np.diff(lists["sums"][2][0])[0] != np.diff(lists["tables"][0][0])[0]
    assert 0 < s2.CPP_SWITCH < s2.CPP_STEPS


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/side_terms2_caller.cpp builds with plain g++ and -Wall -Werror; tests/test_gpu_side_terms2.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "side_terms2_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "side_terms2_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
