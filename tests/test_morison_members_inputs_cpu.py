"""The fixed inputs of tests/test_gpu_morison_members_edges.py and tests/test_gpu_morison_members_changes.py without a GPU
(tests/morison_members_inputs.py): for every (model, directions, t, state, lists) those tests hold to tests/morison_members_ref.py,
the restatement is evaluated on the CPU oracle's spectrum (CreateSpectrum depends on the parameters alone; the GPU tests take the
context's own), a record's components come from tests/eta_components_ref.py, and asserted are
  * clear: every node's |h_j| exceeds the bound of its own eta error, and margin > eta_bound;
  * the segment cases the test names under need= are all met;
  * where elements take part, no element closer than 1e-6 m to the free surface (tests/side_terms_inputs.py).
These are conditions on the inputs, not tolerances: an input that misses one is replaced, the condition stays."""
import numpy as np

import morison_members_inputs as mi
import nonlinear2_inputs as ni
import side_terms2_inputs as s2
import side_terms_inputs as si
from cases import load_into_oracle, sphere_case, three_body_case


def test_edge_inputs_keep_the_restatements_conditions():
    """section C: the 50 members, the five bodies of the 48 and the grid tails, long-crested and under the uniform heading"""
    cases = dict(sphere=sphere_case(), many=mi.many_case(1))  # (the spectrum and k of the 48-body case: the parameters and depth alone)
    comps = {}
    for key, case in cases.items():
        orc = load_into_oracle(case)
        orc.add_waves_irregular(**mi.EDGE_SEA)
        comps[key] = {h: mi.edge_components(orc, h) for h in (None, mi.EDGE_HEADING)}
        orc.close()
        assert comps[key][None][0].size == 64
    n = 0
    for what, key, heading, lists, state, need in mi.edge_checks():
        ref = mi.restate(cases[key], lists, comps[key][heading], mi.EDGE_T, state, mi.EDGE_OPTS, mi.EDGE_SEA["ramp_duration"], True)
        mi.check_conditions(ref, what, need)
        n += 1
    assert n == 8
    # the shapes the edges are made of
    assert mi.counts(mi.edge_lists()[0]) == (50, 200, 300) and sorted(set(mi.EDGE_N_SEG.tolist())) == [1, 2, 3, 4, 5]
    tails = mi.tail_lists()
    assert mi.counts(tails["1 member of 1 segment"][0]) == (1, 2, 2)
    assert mi.counts(tails["256 nodes"][0])[1] == 256 and mi.counts(tails["512 points"][0])[2] == 512
    many = mi.many_lists()
    assert tuple(b for b in range(mi.MANY_N) if many[b] is not None) == mi.MANY_BODIES
    assert 6 * 42 < 256 <= 6 * 43 and 6 * mi.MANY_N > 256 and mi.MANY_SHARD[0] <= 42 and 43 < mi.MANY_SHARD[1]


def walk_oracle(case, stop):
    orc = load_into_oracle(case)
    mi.apply_model(orc, stop)
    return orc


def test_walk_inputs_keep_the_restatements_conditions():
    """section D, 4: every stop of the walk at both SEQ_TIMES, members and elements"""
    case = si.synth_case()
    lists, elements = mi.walk_lists(), si.sequence_lists()["elements"]
    assert tuple(b for b in range(3) if lists[b] is not None) == mi.WALK_MEMBER_BODIES
    assert tuple(b for b in range(3) if elements[b] is not None) == mi.WALK_ELEMENT_BODIES
    sizes = {}
    for stop in mi.walk_stops():
        orc = walk_oracle(case, stop)
        comp, rd, stretch = mi.stop_components(orc, stop, case["water_depth"])
        orc.close()
        sizes[stop["name"]] = 0 if comp is None else comp[0].size
        for t in mi.SEQ_TIMES:
            what = f"{stop['name']} t={t}"
            st = mi.walk_state(t)
            mi.check_conditions(mi.restate(case, lists, comp, t, st, mi.MOR_OPTS, rd, stretch), what, mi.ALL_CASES)
            el = mi.elements_ref(case, elements, comp, t, st, mi.MOR_OPTS, rd, stretch)
            assert el["margin"] >= si.MIN_GAP, f"{what}: an element is {el['margin']:.3e} m from the free surface (choose other inputs)"
    assert sizes["6a record with components"] == 20 and sizes["6b a narrower band"] == 9 and sizes["6c components cleared"] == 0
    assert sizes["10a cos-2s spread"] == 257 and len(sizes) == 17


def test_list_change_inputs_keep_the_restatements_conditions():
    """section D, 5: every list of the changes, in the long-crested and in the spread model, at CHANGE_T"""
    case = si.synth_case()
    stops = {s["name"]: s for s in mi.walk_stops()}
    t, st = mi.CHANGE_T, mi.walk_state(mi.CHANGE_T)
    assert mi.counts(mi.walk_big())[1] >= 4 * mi.counts(mi.walk_lists()[0])[1] and mi.counts(mi.walk_one())[0] == 1
    for name in mi.CHANGE_STOPS:
        orc = walk_oracle(case, stops[name])
        comp, rd, stretch = mi.stop_components(orc, stops[name], case["water_depth"])
        orc.close()
        for step, lists, _ in mi.change_steps():
            if any(ml is not None for ml in lists):
                mi.check_conditions(mi.restate(case, lists, comp, t, st, mi.MOR_OPTS, rd, stretch), f"{name}, {step}")


def test_compose_inputs_keep_the_restatements_conditions():
    """section D, 7: the members beside all other terms, at the steps held to the references"""
    case = three_body_case()
    waves = ni.waves(5)
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**waves)
    comp, rd, stretch = si.model_components(orc, "irregular", waves, 0.0)
    orc.close()
    lists, elements = mi.compose_members(), s2.compose_lists()["elements"]
    motion = s2.compose_motion()
    for n in s2.BOUND_STEPS:
        t = float(s2.COMPOSE_TIMES[n])
        st = motion.state(t)
        mi.check_conditions(mi.restate(case, lists, comp, t, st, s2.MOR_OPTS, rd, stretch), f"compose step {n}", mi.ALL_CASES)
        el = mi.elements_ref(case, elements, comp, t, st, s2.MOR_OPTS, rd, stretch)
        assert el["margin"] >= si.MIN_GAP, (n, el["margin"])


def test_dispersion_solver_and_surface_inputs():
    w = np.array([0.05, 0.3, 1.0, 6.0])
    k = mi.solve_k(w, 60.0)
    assert np.allclose(mi.G * k * np.tanh(k * 60.0), w * w, rtol=1e-14)
    # the still-water inputs of the surface-node tests are dyadic: h_j is exactly zero where it is meant to be
    for ml in (mi.surface_column(2), mi.surface_column(4, top_down=True), mi.surface_beam(3)):
        z = np.concatenate([ml[0][:, 2], ml[1][:, 2]])
        assert np.all(z == np.round(z)) and (0.0 in 0.5 * (ml[0][:, 2] + ml[1][:, 2]))
