"""The Morison strip members (csrc/hc_morison_members.hip) beside the other side terms and across changes: one context walked
through the wave models, a record's components and directions; member lists replaced, shrunk, cleared and set again on a live context;
a model change between begin and end; all side terms in flight around one hc_step; and the refusal of members on the second-order
sea through HydroForces.step and HydroGroup.step.  What tests/test_gpu_side_terms*.py check for the other terms, for the members.

  * where the library promises bits, bits are asserted: against a fresh context created directly in the state under test, against
    each term computed alone, against a context that never carried members;
  * values are held to tests/morison_members_ref.py (per body and per member) and tests/morison_ref.py / directional_ref.py (the
    elements) with the bounds they derive.  A body that carries both is held to the sum of the two references within the sum of
    their bounds plus one rounding of the sum.  No tolerance is introduced here.

The inputs are fixed in tests/morison_members_inputs.py; tests/test_morison_members_inputs_cpu.py asserts their conditions on the
CPU, the comparisons below again on the context's own spectrum."""
import numpy as np
import pytest

import morison_members_inputs as mi
import nonlinear2_inputs as ni
import side_terms2_inputs as s2
import side_terms_inputs as si
from cases import three_body_case
from side_terms_inputs import same_bits
from test_gpu_side_terms2 import HF, SURFACED, last_terms, modes_on, prepare, raw_step, same_terms, terms_alone  # noqa: F401

pytestmark = pytest.mark.gpu
EPS = mi.mm.EPS


def set_members(h, lists):
    for b, ml in enumerate(lists):
        if ml is not None:
            h.set_morison_members(b, *ml)


def put_directions(h, stop):
    if stop["dirs"] is None:
        h.set_wave_directions(None)
    elif stop["dirs"][0] == "spread":
        h.set_wave_spreading(**mi.SPREAD)
    else:
        h.set_wave_directions(mi.stop_directions(stop, h.wave_component_count()))


def context(HF, case, stop, members, elements):
    """a context created directly in the state of `stop` with these lists (None: never set)"""
    h = HF.from_case(case)
    for b, tb in enumerate(mi.excitation_headings(case)):
        h.set_body_excitation_rao_headings(b, *tb)
    mi.apply_model(h, stop)
    if stop["band"] is not None:
        h.set_eta_record_components(*stop["band"])
    if stop["dirs"] is not None:
        put_directions(h, stop)
    h.set_morison_options(regular_phase=stop["phase"], **mi.MOR_OPTS)
    set_members(h, members)
    if elements is not None:
        si.set_lists(h, dict(elements=elements), ("elements",))
    return h


def move(h, stop):
    """the change that leads to `stop` on the live context"""
    if stop["change"] == "model":
        mi.apply_model(h, stop)
    elif stop["change"] == "band":
        (h.clear_eta_record_components() if stop["band"] is None else h.set_eta_record_components(*stop["band"]))
    elif stop["change"] == "dirs":
        put_directions(h, stop)
    h.set_morison_options(regular_phase=stop["phase"], **mi.MOR_OPTS)


def evaluate(h, t, st, members):
    """(body vectors [N][6], {body: member rows})"""
    F = h.compute_morison(t, *st).reshape(-1, 6)
    return F, {b: h.morison_member_forces(b) for b, ml in enumerate(members) if ml is not None}


def same_eval(x, y):
    return same_bits(x[0], y[0]) and x[1].keys() == y[1].keys() and all(same_bits(x[1][b], y[1][b]) for b in x[1])


class Worst:
    def __init__(self):
        self.w = dict(body=0.0, member=0.0)

    def hold(self, name, got, want, bound, what):
        err = np.abs(np.asarray(got) - want)
        assert np.all(np.isfinite(got)), (what, name)
        if err.size:
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            self.w[name] = max(self.w[name], worst)
            assert np.all(err <= bound), f"{what} {name}: worst {worst:.3e} of the bound"

    def report(self, test):
        print(f"{test}: worst |gpu - ref| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in self.w.items()))


def hold(worst, case, members, elements, comp, rd, stretch, opts, t, st, got, what, need=()):
    """body vectors against members + elements, member rows against the per-member bound; the conditions first"""
    F, rows = got
    N = F.shape[0]
    want, bound = np.zeros((N, 6)), np.zeros((N, 6))
    if any(ml is not None for ml in members):
        ref = mi.restate(case, members, comp, t, st, opts, rd, stretch)
        mi.check_conditions(ref, what, need)
        want, bound = ref["F"].copy(), ref["bound"].copy()
        for b, r in rows.items():
            assert r.shape == ref["members"][b].shape, (what, b)
            worst.hold("member", r, ref["members"][b], ref["member_bound"][b], f"{what} body {b}")
    if elements is not None:
        el = mi.elements_ref(case, elements, comp, t, st, opts, rd, stretch)
        assert el["margin"] >= si.MIN_GAP, f"{what}: an element is {el['margin']:.3e} m from the free surface (choose other inputs)"
        for b in range(N):
            if elements[b] is None:
                continue
            both = members[b] is not None
            want[b], bound[b] = want[b] + el["F"][b], bound[b] + el["bound"][b]
            if both:  # the one addition of hc_morison_end
                bound[b] = bound[b] + EPS * np.abs(want[b])
    worst.hold("body", F, want, bound, what)


# ------------------------------------------------------------------------------------------------
# 4: the walk
# ------------------------------------------------------------------------------------------------
def test_members_follow_the_wave_model_the_components_and_the_directions(HF):
    from hydrochrono_amd.hydro import HydroError
    case = si.synth_case()
    members, elements = mi.walk_lists(), si.sequence_lists()["elements"]
    stops = mi.walk_stops()
    h = context(HF, case, dict(stops[0], kind="none", params=None), members, elements)
    worst = Worst()
    results = {}
    for stop in stops:
        if stop["name"].startswith("10 "):  # the IRF model refuses a spread: why the walk goes on in the spectral model
            with pytest.raises(HydroError):
                h.set_wave_spreading(**mi.SPREAD)
        move(h, stop)
        fresh = context(HF, case, stop, members, elements)
        comp, rd, stretch = mi.stop_components(h, stop, case["water_depth"])
        assert (len(comp) == 5) == (stop["dirs"] is not None) if comp is not None else stop["dirs"] is None
        for t in mi.SEQ_TIMES:
            st = mi.walk_state(t)
            got = evaluate(h, t, st, members)
            assert same_eval(got, evaluate(fresh, t, st, members)), (stop["name"], t)
            hold(worst, case, members, elements, comp, rd, stretch, mi.MOR_OPTS, t, st, got, f"{stop['name']} t={t}", mi.ALL_CASES)
            assert got[0].any(axis=1).all() and got[1][0].any() and got[1][2].any()
            results[(stop["name"], t)] = got
        fresh.close()
    names = [s["name"] for s in stops]
    for t in mi.SEQ_TIMES:
        for i in range(1, len(names)):  # every change was a change of bits, in the body vectors and in the member rows
            x, y = results[(names[i - 1], t)], results[(names[i], t)]
            assert not same_bits(x[0][0], y[0][0]) and not same_bits(x[0][2], y[0][2]), (names[i - 1], names[i], t)
            assert not same_bits(x[1][0], y[1][0]) and not same_bits(x[1][2], y[1][2]), (names[i - 1], names[i], t)
        back = (("9 irregular nf 257 again", "3 irregular nf 257"), ("6c components cleared", "6 eta record"),
                ("10c directions cleared", "10 spectral nf 257"))
        for i, j in back:  # ... and the way back gives the bits of the first time
            assert same_eval(results[(i, t)], results[(j, t)]), (i, j, t)
    assert len(names) == 17
    worst.report("test_members_follow_the_wave_model_the_components_and_the_directions")
    h.close()


# ------------------------------------------------------------------------------------------------
# 5: list changes on the live context
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mi.CHANGE_STOPS)
def test_list_changes_on_a_live_context(HF, name):
    from hydrochrono_amd import capi
    case = si.synth_case()
    stop = {s["name"]: s for s in mi.walk_stops()}[name]
    all_elements = si.sequence_lists()["elements"]
    t, st = mi.CHANGE_T, mi.walk_state(mi.CHANGE_T)
    h = context(HF, case, stop, [None] * 3, None)
    plain = context(HF, case, stop, [None] * 3, None)
    comp, rd, stretch = mi.stop_components(h, stop, case["water_depth"])
    worst = Worst()
    seen = {}
    buf = np.empty(6 * 1024)
    for step, members, with_elements in mi.change_steps():
        for b in (0, 2):
            h.set_morison_members(b, *(mi.CLEAR if members[b] is None else members[b]))
        if with_elements:
            si.set_lists(h, dict(elements=all_elements), ("elements",))
        else:
            si.clear_lists(h, ("elements",))
        elements = all_elements if with_elements else None
        fresh = context(HF, case, stop, members, elements)  # never carried any other list
        got = evaluate(h, t, st, members)
        assert same_eval(got, evaluate(fresh, t, st, members)), (name, step)
        hold(worst, case, members, elements, comp, rd, stretch, mi.MOR_OPTS, t, st, got, f"{name}, {step}")
        for b in range(3):
            assert h.morison_member_count(b) == (0 if members[b] is None else len(members[b][0])), (step, b)
        if not any(ml is not None for ml in members):  # no member launch: the getter has nothing to answer with
            assert h.lib.hc_get_morison_member_forces(h.ctx, 0, buf.ctypes.data_as(capi.c_double_p)) == capi.HC_ERR_INVALID, step
            assert fresh.lib.hc_get_morison_member_forces(fresh.ctx, 0, buf.ctypes.data_as(capi.c_double_p)) == capi.HC_ERR_INVALID
        seen[step] = got
        fresh.close()
    assert same_eval(seen["members set again"], seen["first"]) and not same_eval(seen["body 0 one member"], seen["first"])
    assert seen["members cleared"][0][1].any() and not seen["members cleared"][0][0].any()  # body 0 carried members only
    assert seen["elements cleared"][0][0].any() and not seen["elements cleared"][0][1].any()
    assert same_bits(seen["all cleared"][0], np.zeros((3, 6)))
    # nothing left: step() is the plain step again
    assert same_bits(h.step(t, *st), plain.step(t, *st)) and not h.morison().any()
    worst.report(f"test_list_changes_on_a_live_context[{name}]")
    h.close()
    plain.close()


# ------------------------------------------------------------------------------------------------
# 6: a model change between begin and end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change", ["model", "directions"])
def test_end_returns_the_model_of_its_begin(HF, change):
    case = si.synth_case()
    stops = {s["name"]: s for s in mi.walk_stops()}
    A = stops["3 irregular nf 257"]
    B = dict(stops["1 regular"], phase=A["phase"]) if change == "model" else dict(stops["9a uniform heading"], phase=A["phase"])
    members, elements = mi.walk_lists(), si.sequence_lists()["elements"]
    t, st = mi.CHANGE_T, mi.walk_state(mi.CHANGE_T)
    h, fa, fb = (context(HF, case, s, members, elements) for s in (A, A, B))
    under_a, under_b = evaluate(fa, t, st, members), evaluate(fb, t, st, members)
    assert not same_eval(under_a, under_b)
    h.morison_begin(t, *st)
    # accepted (neither call asks for an idle lane): the member launches are enqueued on the lane's own table, behind the elements'
    (mi.apply_model(h, B) if change == "model" else put_directions(h, B))
    ended = h.morison_end().reshape(-1, 6)
    assert same_bits(ended, under_a[0])
    assert all(same_bits(h.morison_member_forces(b), under_a[1][b]) for b in (0, 2))
    assert same_eval(evaluate(h, t, st, members), under_b)
    for x in (h, fa, fb):
        x.close()


# ------------------------------------------------------------------------------------------------
# 7 and 8: all terms in flight, and the refusal through the composing layers
# ------------------------------------------------------------------------------------------------
def compose_setup(HF, n_groups):
    """a: everything on, through step().  b: the same, through raw hc_step and the terms' own calls.  twin: a without members.
    monly: the members alone.  plain: nothing set.  Groups of 2 and 3 shards: everything on.  The nonlinear term on the
    second-order sea, the Morison term on the first-order one (members see no other)."""
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    lists, members = s2.compose_lists(), mi.compose_members()
    waves = ni.waves(5)
    a, b, twin, monly, plain = (HF.from_case(case) for _ in range(5))
    groups = [HydroGroup.from_case(case, n) for n in n_groups]
    for h in (a, b, twin, monly, plain, *groups):
        h.add_waves_irregular(**waves)
    for h in (a, b, twin, *groups):
        prepare(h, lists)
        h.set_morison_second_order(False)
        modes_on(h)
    monly.set_morison_options(regular_phase=0.0, **s2.MOR_OPTS)
    for h in (a, b, monly, *groups):
        set_members(h, members)
    assert a.nonlinear_second_order()["on"] and not a.morison_second_order()["on"]
    return case, lists, members, waves, a, b, twin, monly, plain, groups


def test_all_terms_in_flight_with_members(HF):
    case, lists, members, waves, a, b, twin, monly, plain, groups = compose_setup(HF, (2, 3))
    comp, rd, stretch = si.model_components(a, "irregular", waves, 0.0)
    assert comp[0].size == 5 and max(s2.COMPOSE_TIMES) < rd
    motion = s2.compose_motion()
    worst = Worst()
    for n in range(s2.STEPS):
        t = float(s2.COMPOSE_TIMES[n])
        st = motion.state(t)
        what = f"step {n}"
        fa = a.step(t, *st)
        b.nonlinear_begin(t, st[0], st[1])
        b.morison_begin(t, *st)
        b.drift_begin(t, st[0])
        b.sum_qtf_begin(t, st[0])
        total = raw_step(b, t, st)
        nl, mor, dft, smf = b.nonlinear_end(), b.morison_end(), b.drift_end(), b.sum_qtf_end()
        rows = {k: b.morison_member_forces(k) for k in (0, 2)}
        assert same_bits(total, plain.step(t, *st)), what
        assert all(same_bits(x, y) for x, y in zip(b.components(), plain.components())), what
        assert same_terms((nl, mor, dft, smf), terms_alone(b, t, st)), what
        assert all(same_bits(rows[k], b.morison_member_forces(k)) for k in rows), what
        assert same_bits(fa, s2.compose4(total, nl, mor, dft, smf, 2, SURFACED)), what
        assert same_terms(last_terms(a), (nl, mor, dft, smf)), what
        for g in groups:
            assert same_bits(g.step(t, *st), fa), (what, len(g.shards))
            assert same_terms(last_terms(g), (nl, mor, dft, smf)), (what, len(g.shards))
            assert all(same_bits(g.morison_member_forces(k), rows[k]) for k in rows), (what, len(g.shards))
        # the twin without members: the other terms keep their bits, and the Morison term is elements + members
        twin.step(t, *st)
        tnl, tmor, tdft, tsmf = last_terms(twin)
        assert same_terms((tnl, mor, tdft, tsmf), (nl, mor, dft, smf)), what
        mem = monly.compute_morison(t, *st)
        assert same_bits(mor, tmor + mem) and mem[0:6].any() and mem[12:18].any() and not mem[6:12].any(), what
        assert tmor[6:12].any() and tmor[12:18].any() and not tmor[0:6].any(), what
        if n in s2.BOUND_STEPS:
            hold(worst, case, members, lists["elements"], comp, rd, stretch, s2.MOR_OPTS, t, st, (mor.reshape(-1, 6), rows), what, mi.ALL_CASES)
    worst.report("test_all_terms_in_flight_with_members")
    for h in (a, b, twin, monly, plain, *groups):
        h.close()


def test_members_refusal_through_the_composing_layers(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    case, lists, members, waves, a, b, twin, monly, plain, (grp,) = compose_setup(HF, (3,))
    INV, UNS = capi.HC_ERR_INVALID, capi.HC_ERR_UNSUPPORTED
    dp = (lambda x: x.ctypes.data_as(capi.c_double_p))
    lib = a.lib

    def pending(h):
        """the four ends on one context: INVALID where nothing was begun"""
        out = np.empty(h.D_local)
        return (lib.hc_nonlinear_end(h.ctx, None, None, None), lib.hc_morison_end(h.ctx, dp(out)), lib.hc_drift_end(h.ctx, dp(out)),
                lib.hc_sum_qtf_end(h.ctx, dp(out)))

    assert pending(plain) == (INV,) * 4  # as they answer with nothing begun
    motion = s2.compose_motion()
    t0, t1, t2 = (float(t) for t in s2.COMPOSE_TIMES[:3])
    st = motion.state(t0)
    want = b.step(t0, *st)  # b: never refused, the same steps
    assert same_bits(a.step(t0, *st), want) and same_bits(grp.step(t0, *st), want)
    for h in (a, grp):
        h.set_morison_second_order(True)
    st = motion.state(t1)
    for h in (a, grp):
        with pytest.raises(HydroError) as e:
            h.step(t1, *st)
        assert e.value.status == UNS and "member" in str(e.value), str(e.value)
    assert pending(a) == (INV,) * 4
    assert [pending(s) for s in grp.shards] == [(INV,) * 4] * 3
    for h in (a, grp):
        h.set_morison_second_order(False)
    for t in (t1, t2):
        st = motion.state(t)
        want = b.step(t, *st)
        assert same_bits(a.step(t, *st), want) and same_bits(grp.step(t, *st), want), t
        assert same_bits(a.morison(), b.morison()) and same_bits(grp.morison(), b.morison()) and b.morison().any()
    for h in (a, b, twin, monly, plain, grp):
        h.close()
