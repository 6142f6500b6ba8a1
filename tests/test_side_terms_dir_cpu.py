"""The fixed inputs of tests/test_gpu_side_terms_dir.py without a GPU (tests/side_terms_dir_inputs.py): at every (wave model,
directions, time, state) the GPU test holds to a reference, the references are evaluated on the CPU oracle's spectrum
(CreateSpectrum depends on the parameters alone; the GPU test takes the context's own and asserts the same again) and the
conditions they need are asserted --
  * no Morison element and no panel centroid closer than MIN_GAP to the free surface, no cut edge shorter than MIN_SPAN in h;
  * every list with more than one item partly wet and partly dry; triangles with 0, 1, 2 and 3 wet vertices among the held states;
  * |psi| < 1e4 (qtf_dir_ref asserts it in every pair sum);
  * every derived bound below s2.BOUND_RATIO of the largest component of its result;
  * of more than 20 components more than 10 inside every QTF frequency grid and more than 10 outside (of the five-component
    models at least one on either side, a regular wave inside); every direction of a component inside a frequency grid inside that
    table's heading grid, every direction inside the excitation heading grid; some components of spread A exactly on heading
    nodes, both grid ends among them.
These are conditions, not tolerances; no held state is skipped.  Also here: tests/cpp/side_terms_dir_caller.cpp compiles against
the C++ mirror with plain g++."""
import os
import subprocess
import time

import numpy as np

import nonlinear2_inputs as ni
import side_terms2_inputs as s2
import side_terms_dir_inputs as sd
import side_terms_inputs as si
from cases import load_into_oracle, three_body_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_model(case, kind, params, which, phase=0.0):
    """(comp, ramp_duration, stretching_applies, spectrum or None) from the CPU oracle"""
    orc = load_into_oracle(case)
    spec = None
    if kind == "regular":
        orc.add_waves_regular(*params)
    elif kind in ("irregular", "spectral"):  # the spectral mode synthesises from the same spectrum
        orc.add_waves_irregular(**params)
        spec = orc.irreg_spectrum()
    out = sd.components(orc, kind, params, which, phase=phase)
    orc.close()
    return out + (spec,)


def check_excitation(case, spec, theta, rd, times, what):
    F, B = sd.excitation_reference(case, spec, theta, rd, times)
    for k in range(len(times)):
        s2.check_bound("excitation", np.asarray(F[k], dtype=np.float64), B[k], f"{what} t={times[k]}")


def test_the_tables_and_the_directions():
    for lists in (sd.compose_lists(), sd.compose_lists(small=True), sd.sequence_lists()):
        J = {key: [0 if tb is None else tb[0].size * tb[1].size for tb in lists[key]] for key in ("tables", "sums")}
        assert J == dict(tables=[33, 0, 32], sums=[27, 0, 33])  # two chunks (the second of one row) beside one chunk, in both terms
        has_q = {key: [tb is not None and tb[3] is not None for tb in lists[key]] for key in ("tables", "sums")}
        assert has_q == dict(tables=[True, False, False], sums=[False, False, True])
        for b in (0, 2):  # the sum tables sit on another frequency grid than the drift tables
            assert not np.intersect1d(lists["tables"][b][1], lists["sums"][b][1]).size
            for key in ("tables", "sums"):
                beta = lists[key][b][0]
                assert beta[0] == sd.BLO and beta[-1] == sd.BHI and np.any(beta == 0.0) and set(beta) <= set(sd.NODES)
    full, small = sd.compose_lists(), sd.compose_lists(small=True)
    assert [len(l[1]) if l and l[0] == "tris" else 0 for l in full["surfaces"]] == [257, 0, 0]
    assert [len(l[1][0]) if l and l[0] == "panels" else 0 for l in full["surfaces"]] == [0, 0, 5]
    assert [0 if e is None else len(e[0]) for e in full["elements"]] == [0, 7, 300]
    assert len(small["surfaces"][0][1]) == 12 and len(small["surfaces"][2][1][0]) == 12 and len(small["elements"][2][0]) == 12
    for nf in (5, 257, 300):
        A, B = sd.directions(nf, "A"), sd.directions(nf, "B")
        assert A.shape == B.shape == (nf,) and not np.array_equal(A, B) and np.unique(A).size > min(nf, 10) - 6
        for th in (A, B):
            assert sd.BLO <= th.min() and th.max() <= sd.BHI
        on_node = np.isin(A, sd.NODES)
        assert on_node.sum() >= -(-nf // sd.node_stride(nf)) and (A == sd.BLO).any() and (A == sd.BHI).any() and (A == 0.0).any()
        assert np.array_equal(sd.directions(nf, "zero"), np.zeros(nf)) and np.array_equal(sd.directions(nf, 0.3), np.full(nf, 0.3))
    assert set(sd.EXC_DIRS) <= set(sd.NODES)
    for case in (three_body_case(), si.synth_case()):
        for dirs, w, mag, ph in sd.excitation_headings(case):  # another table at every heading, the two grid ends included
            assert mag.shape == ph.shape == (6, 3, w.size)
            for j, k in ((0, 1), (1, 2), (0, 2)):
                assert not np.array_equal(mag[:, j], mag[:, k]) and not np.array_equal(ph[:, j], ph[:, k])


def check_compose(small, nf, steps):
    case = three_body_case()
    lists = sd.compose_lists(small=small)
    waves = ni.waves(nf)
    comp, rd, stretch, spec = oracle_model(case, "spectral", waves, "A")
    assert comp[0].size == nf and max(sd.COMPOSE_TIMES) < rd and np.unique(comp[4]).size > 3
    sd.check_grids(comp, lists, f"waves({nf})")
    motion = sd.compose_motion()
    seen = np.zeros(4, dtype=int)
    t0 = time.perf_counter()
    for n in steps:
        t = float(sd.COMPOSE_TIMES[n])
        what = f"compose nf={nf} step {n}"
        ref = sd.references(case, case["g"], lists, comp, rd, stretch, t, motion.state(t))
        seen += sd.check_conditions(ref, lists, what)
        sd.check_qtf_conditions(ref, what)
        for b in range(3):
            assert bool(ref["nl"]["buoy"][b].any()) == bool(ref["nl"]["fk"][b].any()) == (lists["surfaces"][b] is not None), (what, b)
            assert bool(ref["mor"]["F"][b].any()) == (lists["elements"][b] is not None), (what, b)
    check_excitation(case, spec, comp[4], rd, [float(sd.COMPOSE_TIMES[n]) for n in steps], f"compose nf={nf}")
    print(f"references of {len(steps)} steps at nf={nf}: {time.perf_counter() - t0:.1f} s; case counts {seen.tolist()}")
    return seen


def test_compose_inputs_keep_the_references_conditions():
    """section 1a: the full lists in five components under spread A at the three steps held to the references"""
    seen = check_compose(False, 5, sd.BOUND_STEPS)
    assert np.all(seen > 0), seen.tolist()  # triangles with 0, 1, 2 and 3 wet vertices


def test_large_nf_inputs_keep_the_references_conditions():
    """section 1b: the small lists in 300 components, above one tile of 256, at the one step held to the references"""
    check_compose(True, 300, (sd.BOUND_STEP_LARGE,))


def test_subset_and_refusal_inputs():
    """sections 2, 4 and 5 run in si.THREE_IRREG (200 components) under spreads A and B: the grids hold them"""
    case = three_body_case()
    lists = sd.compose_lists()
    for which in ("A", "B"):
        comp = oracle_model(case, "spectral", si.THREE_IRREG, which)[0]
        sd.check_grids(comp, lists, f"THREE_IRREG {which}")
    # section 5: components of spread A on BHI lie inside the frequency grid of body 2's drift table and of its sum table, so that
    # a table whose last heading is one ulp below BHI (sd.narrow) refuses that term's begin
    import drift_ref as dr
    comp = oracle_model(case, "spectral", si.THREE_IRREG, "A")[0]
    for key in ("tables", "sums"):
        tb = lists[key][2]
        assert (dr.cells(tb[1], comp[1])[0] & (comp[4] == sd.BHI)).any(), key
        nb = sd.narrow(tb)[0]
        assert nb[-1] < sd.BHI and np.nextafter(nb[-1], np.inf) == sd.BHI and np.array_equal(nb[:-1], tb[0][:-1])
        g, P, Q = sd.one_heading(tb)
        assert P.shape == (6, g.size, g.size)


def test_walk_inputs_keep_the_references_conditions():
    """section 3: synth_case(3) at depth 60 under every entry of WALK at SEQ_TIMES"""
    case = si.synth_case()
    lists = sd.sequence_lists()
    seen = np.zeros(4, dtype=int)
    seen_nf = set()
    t0 = time.perf_counter()
    for i, (name, kind, params, which, changed, moved, still) in enumerate(sd.WALK):
        comp, rd, stretch, spec = oracle_model(case, kind, params, which, phase=sd.SEQ_PHASE)
        if comp is None:
            assert kind == "eta" and i not in sd.HELD + sd.HELD_TERMS
            continue
        seen_nf.add(comp[0].size)
        sd.check_grids(comp, lists, name, regular=kind == "regular")
        for t in sd.SEQ_TIMES:
            st = sd.sequence_state(t)
            what = f"{name} t={t}"
            if i in sd.HELD + sd.HELD_TERMS:
                ref = sd.references(case, case["g"], lists, comp, rd, stretch, t, st, drift_modes=(1, 3))
                seen += sd.check_conditions(ref, lists, what)
                sd.check_qtf_conditions(ref, what)
            else:  # the pair sums assert |psi| < 1e4 for every model of the walk
                ref = sd.qtf_references(lists, comp, rd, t, st[0], drift_modes=(1, 3))
            for rows in (ref["dft"][1], ref["dft"][3], ref["sum"]):
                assert all(r is None or np.abs(r[0]).max() > 0.0 for r in rows), what
        if i in sd.HELD and kind == "spectral":
            check_excitation(case, spec, None if which is None else comp[4], rd, sd.SEQ_TIMES, name)
    print(f"references of the walk: {time.perf_counter() - t0:.1f} s; case counts {seen.tolist()}")
    assert seen_nf == {1, 5, 257} and np.all(seen > 0), (seen_nf, seen.tolist())
    assert [sd.WALK[i][0].split()[0] for i in sd.HELD + sd.HELD_TERMS] == ["1", "3", "5", "7", "8", "9"]
    k = case["bodies"][0]
    assert np.isfinite(case["water_depth"]) and "w" in k


def test_finite_depth_regimes_of_the_walk():
    """depth 60 with 0.01 .. 2 Hz: long-wave (lambda > depth), intermediate and k d > 500 components are all present"""
    case = si.synth_case()
    comp = oracle_model(case, "spectral", si.irreg(257), "A")[0]
    k, d = comp[2], case["water_depth"]
    long_wave, very_deep = 2 * np.pi / k > d, k * d > 500.0
    assert long_wave.any() and very_deep.any() and (~long_wave & ~very_deep).any()


def test_cpp_caller_inputs():
    """section 6: dyadic grids and tables on heading grids; both headings inside every grid"""
    lists = sd.cpp_lists()
    assert tuple(b for b in range(4) if lists["surfaces"][b] is not None) == sd.CPP_SURFACE_BODIES
    for key in ("tables", "sums"):
        for tb in lists[key]:
            if tb is not None:
                beta, g, P, Q = tb
                assert P.shape == (6, 3, 3, g.size, g.size) and np.all(np.diff(g) > 0) and np.array_equal(g * 32, np.round(g * 32))
                assert all(beta[0] <= v <= beta[-1] for v in sd.CPP_HEADINGS) and not np.array_equal(P[:, 0, 0], P[:, 1, 1])
    for b in range(4):
        dirs, w, mag, ph = sd.cpp_excitation_headings(b)
        assert mag.shape == ph.shape == (6, 3, 16) and all(dirs[0] <= v <= dirs[-1] for v in sd.CPP_HEADINGS)
        assert w[0] <= sd.CPP_REG[1] <= w[-1] and not np.array_equal(mag[:, 0], mag[:, 2])
    assert 0 < sd.CPP_SWITCH < sd.CPP_REGULAR < sd.CPP_REGULAR + sd.CPP_SWITCH < sd.CPP_STEPS


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/side_terms_dir_caller.cpp builds with plain g++ and -Wall -Werror; tests/test_gpu_side_terms_dir.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "side_terms_dir_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "side_terms_dir_caller.cpp"), "-o", out,
                    "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
