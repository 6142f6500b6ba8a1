"""The Morison, nonlinear, drift and sum-frequency terms TOGETHER, the first two on the second-order sea, across changes of the wave
model, the bands and the tables: what tests/test_gpu_side_terms.py checks for three first-order terms, for the state added
since -- clipped triangles, the three pair-table sets of csrc/hc_wave_kin2.hip (hc_wave_kinematics2's, the Morison one, the nonlinear one), the surface points
and double-buffered increments of csrc/hc_nonlinear.hip, the bin map and slot layout of csrc/hc_qtf.hip, and the fourth begin
of HydroForces.step, HydroGroup.step and TestHydro::CoordinateFuncForBody.  Each term alone is the subject of
tests/test_gpu_morison2.py, test_gpu_nonlinear2.py, test_gpu_surface_clip.py, test_gpu_drift.py and test_gpu_sumfreq.py; here

  * where the library promises bits, bits are asserted: against the same term computed alone, against a one-context run, and
    against a fresh context created directly in the state under test;
  * values are held to the references of those files (tests/morison2_ref.py, nonlinear2_ref.py, drift_ref.py, sumfreq_ref.py) with
    the bounds they derive.  No tolerance is introduced here.

The inputs are fixed in tests/side_terms2_inputs.py; tests/test_side_terms2_cpu.py asserts on the CPU that every (model, t, state)
held to a reference keeps the references' conditions.  The comparisons below assert them again on the context's own spectrum.

hc_step_many / HydroForces.step_many compose no side term: section 2 holds its rows to step() calls of a context
without a term, and to step() of the context under test where its subset is empty."""
import os
import subprocess
import time

import numpy as np
import pytest

import nonlinear2_inputs as ni
import side_terms2_inputs as s2
import side_terms_inputs as si
from cases import GOLDEN_DIR, three_body_case
from side_terms_inputs import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACED = (0, 2)  # bodies with a surface list (triangles on 0, panels on 2); elements on (1, 2); drift and sum tables on (0, 2)
FULL = s2.FULL
TERMS = ("nonlinear", "morison", "drift", "sum")


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def raw_step(h, t, st):
    """hc_step itself (HydroForces.step composes the side terms)"""
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in st]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def prepare(h, lists, phase=0.0, mor_phase=0.0, nl_bands=(FULL, FULL), mor_bands=(FULL, FULL), sums=None, order2=True):
    """lists, tables, options and both second-order switches on a HydroForces or a HydroGroup; the modes are the caller's"""
    s2.set_lists(h, lists, ("surfaces", "elements", "tables"))
    s2.set_sum_tables(h, lists["sums"] if sums is None else sums)
    h.set_nonlinear_options(regular_phase=phase, **s2.NL_OPTS)
    h.set_morison_options(regular_phase=mor_phase, **s2.MOR_OPTS)
    h.set_drift_options(regular_phase=phase)
    h.set_sum_options(regular_phase=phase)
    h.set_nonlinear_second_order(order2, diff_band=nl_bands[0], sum_band=nl_bands[1])
    h.set_morison_second_order(order2, diff_band=mor_bands[0], sum_band=mor_bands[1])


def modes_on(h):
    h.set_nonlinear_mode(2)
    h.set_drift_mode(3)
    h.set_sum_mode(1)


def terms_alone(h, t, st):
    """(nonlinear (buoy, fk, hs_lin), morison, drift, sum) of a HydroForces or HydroGroup, each term computed alone"""
    return h.compute_nonlinear(t, st[0], st[1]), h.compute_morison(t, *st), h.compute_drift(t, st[0]), h.compute_sum_qtf(t, st[0])


def same_terms(x, y):
    return all(same_bits(p, q) for p, q in zip(x[0], y[0])) and all(same_bits(x[k], y[k]) for k in (1, 2, 3))


def last_terms(h):
    return h.nonlinear(), h.morison(), h.drift(), h.sum_qtf()


class Worst:
    """worst |gpu - ref| / bound per term over a test, printed at its end"""

    def __init__(self):
        self.w = dict(buoy=0.0, fk=0.0, morison=0.0, drift=0.0, sum=0.0)

    def hold(self, name, got, want, bound, what):
        got, want, bound = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want, bound))
        assert got.shape == want.shape and np.all(np.isfinite(got)), (what, name)
        err = np.abs(got - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        self.w[name] = max(self.w[name], worst)
        assert np.all(err <= bound), f"{what} {name}: worst {worst:.3e} of the bound"

    def report(self, test):
        print(f"{test}: worst |gpu - ref| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in self.w.items()))


def hold_qtf(worst, ref, dft, smf, what):
    """dft = {mode: drift}, smf: the GPU's rows inside the pair sums' bounds; exactly zero on a body without a table"""
    for mode, rows in ref["dft"].items():
        got = np.asarray(dft[mode]).reshape(-1, 6)
        for b, row in enumerate(rows):
            if row is None:
                assert same_bits(got[b], np.zeros(6)), (what, "drift", mode, b)
            else:
                worst.hold("drift", got[b], row[0], row[1], f"{what} mode {mode} body {b}")
    got = np.asarray(smf).reshape(-1, 6)
    for b, row in enumerate(ref["sum"]):
        if row is None:
            assert same_bits(got[b], np.zeros(6)), (what, "sum", b)
        else:
            worst.hold("sum", got[b], row[0], row[1], f"{what} body {b}")


def hold_to_references(worst, case, g, lists, sums, comps, rd, stretch, t, st, terms, nl_bands, what, orders=(2, 2), seen=None):
    """terms = (nonlinear, morison, {drift mode: drift}, sum) of the GPU inside the references' bounds at one state; conditions first"""
    ref = s2.references(case, g, lists, sums, comps, rd, stretch, t, st, nl_bands, orders=orders, drift_modes=tuple(terms[2]))
    cases = s2.check_conditions(ref, lists, what)
    s2.check_qtf_conditions(ref, what)
    if seen is not None:
        seen += cases
    (buoy, fk, _), mor, dft, smf = terms
    worst.hold("buoy", buoy, ref["nl"]["buoy"], ref["nl"]["bound_buoy"], what)
    worst.hold("fk", fk, ref["nl"]["fk"], ref["nl"]["bound_fk"], what)
    worst.hold("morison", mor, ref["mor"]["F"], ref["mor"]["bound"], what)
    hold_qtf(worst, ref, dft, smf, what)
    return ref


# ------------------------------------------------------------------------------------------------
# 1: all four together, in order, order 2 on
# ------------------------------------------------------------------------------------------------
def run_compose(HF, small, nf, held, test):
    """a: everything on, through step().  b: the same lists, used through raw hc_step and the terms' own calls only.  plain: nothing
    set.  grp: three shards, everything on."""
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    lists = s2.compose_lists(small=small)
    waves = ni.waves(nf)
    a, b, plain = (HF.from_case(case) for _ in range(3))
    grp = HydroGroup.from_case(case, 3)
    for h in (a, b, plain, grp):
        h.add_waves_irregular(**waves)
    for h in (a, b, grp):
        prepare(h, lists)
        modes_on(h)
    assert a.nonlinear_second_order()["on"] and a.morison_second_order()["on"] and grp.morison_second_order()["on"]
    comps, rd, stretch = s2.model_components(a, "irregular", waves, dict(nl=0.0, mor=0.0, dft=0.0, sum=0.0))
    assert comps["nl"][0].size == nf and max(s2.COMPOSE_TIMES) < rd
    s2.check_grids(comps["dft"], lists, lists["sums"], f"waves({nf})")
    g = abs(a.simulation_parameters()[1])
    motion = s2.compose_motion()
    worst = Worst()
    z6 = np.zeros(6)
    differs = 0
    t_ref = 0.0
    for n in range(s2.STEPS):
        t = float(s2.COMPOSE_TIMES[n])
        st = motion.state(t)
        what = f"nf {nf} step {n}"
        fa = a.step(t, *st)
        # b: all four begun, the raw step, all four ended -- four side streams in flight around one hc_step
        b.nonlinear_begin(t, st[0], st[1])
        b.morison_begin(t, *st)
        b.drift_begin(t, st[0])
        b.sum_qtf_begin(t, st[0])
        total = raw_step(b, t, st)
        nl, mor, dft, smf = b.nonlinear_end(), b.morison_end(), b.drift_end(), b.sum_qtf_end()
        assert same_bits(total, plain.step(t, *st)), what
        assert all(same_bits(x, y) for x, y in zip(b.components(), plain.components())), what
        # ... and each term computed alone has those bits
        assert same_terms((nl, mor, dft, smf), terms_alone(b, t, st)), what
        want = s2.compose4(total, nl, mor, dft, smf, 2, SURFACED)
        assert same_bits(fa, want), what
        assert same_terms(last_terms(a), (nl, mor, dft, smf)), what
        assert same_bits(grp.step(t, *st), fa), what
        assert same_terms(last_terms(grp), (nl, mor, dft, smf)), what
        # rows of a body without a term are untouched by it
        assert same_bits(nl[0][6:12], z6) and same_bits(nl[1][6:12], z6) and same_bits(mor[0:6], z6), what
        assert same_bits(dft[6:12], z6) and same_bits(smf[6:12], z6), what
        assert same_bits(fa[6:12], ((total[6:12] + mor[6:12]) + dft[6:12]) + smf[6:12]), what
        r0 = (total[0:6] - nl[2][0:6] + nl[0][0:6]) + nl[1][0:6]
        assert same_bits(fa[0:6], ((r0 + mor[0:6]) + dft[0:6]) + smf[0:6]), what
        differs += not same_bits(fa, (si.compose(total, nl, mor, None, 2, SURFACED) + smf) + dft)
        for x in (nl[0][0:6], nl[0][12:18], nl[1][0:6], nl[1][12:18], mor[6:12], mor[12:18], dft[0:6], dft[12:18], smf[0:6], smf[12:18]):
            assert x.any(), what
        for body in range(3):  # order 2 did run: the increments are there, and those of the group are the same
            if lists["elements"][body] is not None:
                ia, ig = b.morison_increments(body), grp.morison_increments(body)
                assert ia["eta2"].any() and ia["vel2"].any() and all(same_bits(ia[k], ig[k]) for k in ia), (what, body)
            if lists["surfaces"][body] is not None:
                ia, ig = b.nonlinear_increments(body), grp.nonlinear_increments(body)
                assert ia["eta2"].any() and ia["q2"].any() and all(same_bits(ia[k], ig[k]) for k in ia), (what, body)
        if n in held:
            t0 = time.perf_counter()
            hold_to_references(worst, case, g, lists, lists["sums"], comps, rd, stretch, t, st, (nl, mor, {3: dft}, smf), (FULL, FULL), what)
            t_ref += time.perf_counter() - t0
    assert differs > 0  # the order of the drift and sum additions is visible in these inputs
    worst.report(test)
    print(f"{test}: references {t_ref:.1f} s")
    for h in (a, b, plain, grp):
        h.close()


def test_all_four_compose_in_order(HF):
    """1a: the full lists (257 triangles, 5 panels, 7 and 300 elements) in five components"""
    run_compose(HF, False, 5, s2.BOUND_STEPS, "test_all_four_compose_in_order")


def test_all_four_compose_in_order_above_one_tile(HF):
    """1b: the small lists in 300 components, above one tile of 256 rows and columns of the pair tables"""
    run_compose(HF, True, 300, (s2.BOUND_STEP_LARGE,), "test_all_four_compose_in_order_above_one_tile")


# ------------------------------------------------------------------------------------------------
# 2: every subset
# ------------------------------------------------------------------------------------------------
def test_every_subset_of_terms(HF):
    """a: the context under test.  c: a's twin, on which the order-2 switch or the bands of every ABSENT term are changed besides.
    b: everything on, each term computed alone.  plain: nothing set."""
    case = three_body_case()
    lists = s2.compose_lists()
    a, c, b, plain = (HF.from_case(case) for _ in range(4))
    for h in (a, c, b, plain):
        h.add_waves_irregular(**si.THREE_IRREG)
    for h in (a, c, b):
        prepare(h, lists)
        modes_on(h)
    motion = s2.compose_motion()
    key = dict(nonlinear="surfaces", morison="elements", drift="tables", sum="sums")
    mode_of = dict(nonlinear=("set_nonlinear_mode", 2), drift=("set_drift_mode", 3), sum=("set_sum_mode", 1))  # Morison has no mode
    ways = {name: (["mode", "clear"] if name in mode_of else ["clear"]) for name in TERMS}
    off_by = {}  # term -> the way it was switched off
    used = {name: set() for name in TERMS}
    absent_settings = [dict(on=False), dict(on=True, diff_band=(0.1, 0.7), sum_band=s2.NO_PAIR), dict(on=True, diff_band=s2.NO_PAIR, sum_band=s2.NO_PAIR)]
    n_absent = 0

    def switch(name, on):
        for h in (a, c):
            if on:
                if off_by[name] == "mode":
                    getattr(h, mode_of[name][0])(mode_of[name][1])
                else:
                    s2.set_lists(h, lists, (key[name],))
            elif ways[name][0] == "mode":
                getattr(h, mode_of[name][0])(0)
            else:
                s2.clear_lists(h, (key[name],))
        if on:
            del off_by[name]
        else:
            off_by[name] = ways[name][0]
            used[name].add(ways[name][0])
            ways[name].append(ways[name].pop(0))

    # bit 3: Morison, bit 2: drift, bit 1: sum, bit 0: nonlinear; 15 down to 0, everything on again, everything off again
    sequence = list(range(15, -1, -1)) + [15, 0]
    assert set(sequence) == set(range(16)) and len(sequence) + 7 <= len(s2.SUBSET_TIMES)
    bit = dict(nonlinear=0, sum=1, drift=2, morison=3)
    state = {name: True for name in TERMS}
    for subset, t in zip(sequence, s2.SUBSET_TIMES):
        t = float(t)
        for name in TERMS:
            target = bool(subset >> bit[name] & 1)
            if target != state[name]:
                switch(name, target)
                state[name] = target
                if name in ("nonlinear", "morison"):
                    setter = c.set_nonlinear_second_order if name == "nonlinear" else c.set_morison_second_order
                    if target:
                        setter(True)  # present again: as a
                    else:
                        setter(**absent_settings[n_absent % 3])
                        n_absent += 1
        st = motion.state(t)
        fa, fc = a.step(t, *st), c.step(t, *st)
        total = raw_step(b, t, st)
        nl, mor, dft, smf = terms_alone(b, t, st)
        assert nl[0].any() and nl[1].any() and mor.any() and dft.any() and smf.any()
        want = s2.compose4(total, nl if state["nonlinear"] else None, mor if state["morison"] else None, dft if state["drift"] else None,
                           smf if state["sum"] else None, 2, SURFACED)
        assert same_bits(fa, want), (subset, dict(off_by))
        assert same_bits(fc, fa), (subset, dict(off_by))  # the switches and bands of an absent term are not seen
        assert same_bits(total, plain.step(t, *st))
        assert same_bits(fa, total) == (subset == 0)
        got = last_terms(a)
        assert [bool(got[0][0].any()), bool(got[1].any()), bool(got[2].any()), bool(got[3].any())] == [state[k] for k in TERMS], subset
    assert all(used[name] == ({"mode", "clear"} if name in mode_of else {"clear"}) for name in TERMS), used
    assert not any(state.values())
    # step_many: three rows are three step() calls -- of a context without a term, whatever is set (no side term is composed), and
    # of this very context while its subset is empty (c is a's twin: the same history)
    k = len(sequence)
    ts = s2.SUBSET_TIMES[k:k + 3]
    states = np.stack([motion.packed(float(t)) for t in ts])
    many = a.step_many(ts, states)[0]
    assert same_bits(many, np.stack([c.step(float(t), *motion.state(float(t))) for t in ts]))
    assert same_bits(many, np.stack([plain.step(float(t), *motion.state(float(t))) for t in ts]))
    for name in TERMS:
        switch(name, True)
    c.set_nonlinear_second_order(True)
    c.set_morison_second_order(True)
    ts = s2.SUBSET_TIMES[k + 3:k + 6]
    states = np.stack([motion.packed(float(t)) for t in ts])
    many = a.step_many(ts, states)[0]
    assert same_bits(many, np.stack([plain.step(float(t), *motion.state(float(t))) for t in ts]))
    for t in ts:
        raw_step(c, float(t), motion.state(float(t)))  # c keeps a's history
    t = float(s2.SUBSET_TIMES[k + 6])
    st = motion.state(t)
    fa = a.step(t, *st)
    assert not same_bits(fa, plain.step(t, *st)) and same_bits(fa, c.step(t, *st))  # the terms are on all the while
    for h in (a, c, b, plain):
        h.close()


# ------------------------------------------------------------------------------------------------
# 3: the tables follow the wave model and the bands
# ------------------------------------------------------------------------------------------------
def apply_model(h, kind, params):
    if kind == "regular":
        h.add_waves_regular(*params)
    elif kind == "irregular":
        h.add_waves_irregular(**params)
    elif kind == "spectral":
        h.add_waves_irregular(spectral=True, **params)
    elif kind == "eta":
        h.add_waves_irregular_eta(si.REC_T, si.REC_ETA, si.REC_DT)
    else:
        h.add_waves_none()


def all_terms(h, t, st):
    """(nonlinear, morison, {1: mean drift, 3: full QTF}, sum): the mean drift reads E_m, the full table the bin map"""
    out = {}
    for mode in (1, 3):
        h.set_drift_mode(mode)
        out[mode] = h.compute_drift(t, st[0])
    return h.compute_nonlinear(t, st[0], st[1]), h.compute_morison(t, *st), out, h.compute_sum_qtf(t, st[0])


def increments(h, lists, orders):
    """per term and body the increments of the last evaluation; None where the evaluation had no second-order part (the getter
    refuses: an evaluation of order 1 forgets the one before)"""
    from hydrochrono_amd.hydro import HydroError
    out = {}
    for name, order, key, getter in (("nl", orders[0], "surfaces", h.nonlinear_increments), ("mor", orders[1], "elements", h.morison_increments)):
        for b in range(3):
            if lists[key][b] is None:
                continue
            if order == 2:
                out[(name, b)] = getter(b)
            else:
                with pytest.raises(HydroError):
                    getter(b)
                out[(name, b)] = None
    return out


def same_increments(x, y):
    return x.keys() == y.keys() and all((x[k] is None and y[k] is None) or all(same_bits(x[k][f], y[k][f]) for f in x[k]) for k in x)


def same_nl(x, y):
    return all(same_bits(p, q) for p, q in zip(x[0], y[0]))


def same_dft(x, y):
    return all(same_bits(x[2][m], y[2][m]) for m in (1, 3))


def same_all(x, y):
    return same_nl(x, y) and same_bits(x[1], y[1]) and same_dft(x, y) and same_bits(x[3], y[3])


def test_tables_follow_the_wave_model_and_the_bands(HF):
    from hydrochrono_amd.hydro import HydroGroup
    case = si.synth_case()
    lists = s2.sequence_lists()
    h, grp = HF.from_case(case), HydroGroup.from_case(case, 2)
    first = s2.WALK[0]
    for x in (h, grp):
        prepare(x, lists, phase=si.SEQ_PHASE, mor_phase=first[3], nl_bands=first[4])
        x.set_sum_mode(1)
    g = abs(h.simulation_parameters()[1])
    worst = Worst()
    seen = np.zeros(4, dtype=int)
    kin_points = np.array([[3.0, 0.0, -1.0], [18.5, 1.0, -4.0]])
    results, t_ref = {}, 0.0
    prev = None
    for i, entry in enumerate(s2.WALK):
        name, kind, params, mor_phase, nl_bands, sums_key, orders, changed = entry
        sums = s2.walk_sums(lists, sums_key)
        for x in (h, grp):
            if prev is None or (kind, params) != (prev[1], prev[2]):
                apply_model(x, kind, params)
            if prev is not None and mor_phase != prev[3]:
                x.set_morison_options(regular_phase=mor_phase, **s2.MOR_OPTS)
            if prev is not None and nl_bands != prev[4]:
                x.set_nonlinear_second_order(True, diff_band=nl_bands[0], sum_band=nl_bands[1])
            if prev is not None and sums_key != prev[5]:
                s2.set_sum_tables(x, sums)
        assert grp.nonlinear_second_order() == h.nonlinear_second_order() == dict(on=True, diff_band=nl_bands[0], sum_band=nl_bands[1], apply_ramp=True)
        fresh = HF.from_case(case)  # created directly with this model, these options and these tables
        apply_model(fresh, kind, params)
        prepare(fresh, lists, phase=si.SEQ_PHASE, mor_phase=mor_phase, nl_bands=nl_bands, sums=sums)
        fresh.set_sum_mode(1)
        phases = dict(nl=si.SEQ_PHASE, mor=mor_phase, dft=si.SEQ_PHASE, sum=si.SEQ_PHASE)
        comps, rd, stretch = s2.model_components(h, kind, params, phases)
        if comps["nl"] is not None:
            assert comps["nl"][0].size == (1 if kind == "regular" else params["nfrequencies"])
            s2.check_grids(comps["dft"], lists, sums, name, regular=kind == "regular")
            assert (sum(s2.pair_counts(comps["nl"][1], nl_bands)) > 0) == (orders[0] == 2), name
        else:
            assert orders == (1, 1)
        for t in si.SEQ_TIMES:
            st = si.sequence_state(t)
            what = f"{name} t={t}"
            got = all_terms(h, t, st)
            inc = increments(h, lists, orders)
            # (a) a fresh context in this state: the same bits, increments included (d)
            assert same_all(got, all_terms(fresh, t, st)), what
            assert same_increments(inc, increments(fresh, lists, orders)), what
            # (b) the group
            assert same_all(all_terms(grp, t, st), got), what
            assert same_increments(inc, increments(grp, lists, orders)), what
            # (c) hc_wave_kinematics2 keeps a table set of its own: other bands and another regular phase there change nothing here
            for x in (h, *grp.shards):
                x.wave_kinematics2(kin_points, [t], **s2.KIN2_OTHER)
            assert same_all(all_terms(h, t, st), got) and same_all(all_terms(grp, t, st), got), what
            assert same_increments(inc, increments(h, lists, orders)) and same_increments(inc, increments(grp, lists, orders)), what
            results[(i, t)] = got
            nl, mor, dft, smf = got
            waves = comps["nl"] is not None
            assert nl[0][0:6].any() and nl[0][12:18].any() and mor[6:12].any() and mor[12:18].any() and bool(nl[1].any()) == waves, what
            for b in range(3):
                has_dft, has_sum = waves and lists["tables"][b] is not None, waves and sums[b] is not None
                r = slice(6 * b, 6 * b + 6)
                assert bool(dft[1][r].any()) == bool(dft[3][r].any()) == has_dft and bool(smf[r].any()) == has_sum, (what, b)
                if not has_dft:
                    assert same_bits(dft[1][r], np.zeros(6)) and same_bits(dft[3][r], np.zeros(6)), (what, b)
                if not has_sum:
                    assert same_bits(smf[r], np.zeros(6)), (what, b)  # exactly 0.0: a cleared table, an eta record, no waves
            t0 = time.perf_counter()
            if i in s2.HELD:
                hold_to_references(worst, case, g, lists, sums, comps, rd, stretch, t, st, got, nl_bands, what, orders=orders, seen=seen)
            elif i in s2.HELD_QTF:
                ref = s2.qtf_references(lists, sums, comps, rd, t, st[0], drift_modes=(1, 3))
                s2.check_qtf_conditions(ref, what)
                hold_qtf(worst, ref, dft, smf, what)
            t_ref += time.perf_counter() - t0
            if orders[0] == 1:  # the bits of the switch off (empty bands, an eta record, no waves)
                fresh.set_nonlinear_second_order(False)
                assert same_nl(fresh.compute_nonlinear(t, st[0], st[1]), nl), what
                fresh.set_nonlinear_second_order(True, diff_band=nl_bands[0], sum_band=nl_bands[1])
            if orders[1] == 1:
                fresh.set_morison_second_order(False)
                assert same_bits(fresh.compute_morison(t, *st), mor), what
                fresh.set_morison_second_order(True)
            elif comps["nl"] is not None:  # ... and order 2 is seen in both terms
                if kind != "regular":  # (both regular waves are deep-water waves here: Stokes' second-order velocity vanishes)
                    fresh.set_morison_second_order(False)
                    assert not same_bits(fresh.compute_morison(t, *st), mor), what
                    fresh.set_morison_second_order(True)
                if orders[0] == 2:
                    fresh.set_nonlinear_second_order(False)
                    assert not same_bits(fresh.compute_nonlinear(t, st[0], st[1])[1], nl[1]), what
                    fresh.set_nonlinear_second_order(True, diff_band=nl_bands[0], sum_band=nl_bands[1])
            # (e) what changed against the entry before changed the bits of every term that depends on it, and of no other
            if prev is not None:
                before = results[(i - 1, t)]
                moved = dict(nl=not same_bits(got[0][1], before[0][1]) or not same_bits(got[0][0], before[0][0]),
                             mor=not same_bits(mor, before[1]), dft1=not same_bits(dft[1], before[2][1]),
                             dft3=not same_bits(dft[3], before[2][3]), sum=not same_bits(smf, before[3]))
                expect = dict(model=("nl", "mor", "dft1", "dft3", "sum"), **{"morison phase": ("mor",), "nonlinear bands": ("nl",), "sum tables": ("sum",)})[changed]
                assert {k for k, v in moved.items() if v} == set(expect), (what, changed, moved)
        fresh.close()
        prev = entry
    names = [e[0][:2].strip() for e in s2.WALK]
    at = {n: k for k, n in enumerate(names)}
    for t in si.SEQ_TIMES:
        assert same_all(results[(at["6"], t)], results[(at["3"], t)])    # the nonlinear bands full again: the bits of entry 3
        assert same_all(results[(at["13"], t)], results[(at["3"], t)])   # irregular nf 257 again: every term has the bits of entry 3
        eight, nine = results[(at["8"], t)], results[(at["9"], t)]
        assert same_bits(nine[3][0:6], np.zeros(6)) and nine[3][12:18].any() and not same_bits(nine[3][12:18], eight[3][12:18])
        assert not same_all(results[(at["11"], t)], results[(at["1"], t)])  # another regular wave
    assert np.all(seen > 0), seen.tolist()  # triangles with 0, 1, 2 and 3 wet vertices among the states held to the references
    worst.report("test_tables_follow_the_wave_model_and_the_bands")
    print(f"test_tables_follow_the_wave_model_and_the_bands: references {t_ref:.1f} s")
    h.close()
    grp.close()


# ------------------------------------------------------------------------------------------------
# 4: a model change while evaluations are pending
# ------------------------------------------------------------------------------------------------
def test_end_returns_the_model_of_its_begin(HF):
    """On si.synth_case() with the walk's lists, as the same test of tests/test_gpu_side_terms.py: the two models are entries 8
    (irregular, five components) and 1 (regular) of the walk, whose conditions tests/test_side_terms2_cpu.py has checked."""
    case = si.synth_case()
    lists = s2.sequence_lists()
    h = HF.from_case(case)
    prepare(h, lists, phase=si.SEQ_PHASE, mor_phase=si.SEQ_PHASE)
    modes_on(h)
    h.add_waves_irregular(**si.irreg(5))
    t = si.SEQ_TIMES[1]
    st = si.sequence_state(t)
    under_irregular = terms_alone(h, t, st)
    inc_irregular = increments(h, lists, (2, 2))
    h.nonlinear_begin(t, st[0], st[1])
    h.morison_begin(t, *st)
    h.drift_begin(t, st[0])
    h.sum_qtf_begin(t, st[0])
    h.add_waves_regular(*si.REG1)  # accepted: the launches are enqueued on the terms' own tables
    ended = (h.nonlinear_end(), h.morison_end(), h.drift_end(), h.sum_qtf_end())
    assert same_terms(ended, under_irregular)
    assert same_increments(increments(h, lists, (2, 2)), inc_irregular) and all(v["eta2"].any() for v in inc_irregular.values())
    fresh = HF.from_case(case)
    fresh.add_waves_regular(*si.REG1)
    prepare(fresh, lists, phase=si.SEQ_PHASE, mor_phase=si.SEQ_PHASE)
    modes_on(fresh)
    after = terms_alone(h, t, st)
    assert same_terms(after, terms_alone(fresh, t, st))
    assert same_increments(increments(h, lists, (2, 2)), increments(fresh, lists, (2, 2)))
    assert not same_bits(after[0][0], ended[0][0]) and not same_bits(after[0][1], ended[0][1])
    assert all(not same_bits(after[k], ended[k]) and after[k].any() and ended[k].any() for k in (1, 2, 3))
    h.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------
# 5: unwinding after a refused begin (host-side refusals only)
# ------------------------------------------------------------------------------------------------
def test_failed_begin_leaves_nothing_pending(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError, HydroGroup
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda x: x.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    lists = s2.compose_lists()
    a, b = HF.from_case(case), HF.from_case(case)
    grp = HydroGroup.from_case(case, 3)
    for h in (a, b, grp):
        h.add_waves_irregular(**si.THREE_IRREG)
        prepare(h, lists)
        modes_on(h)
    lib = a.lib
    motion = s2.compose_motion()

    def pending(h):
        """(nonlinear, morison, drift, sum) return codes of the four ends on one context: OK where an evaluation was pending"""
        out = np.empty(h.D_local)
        return (lib.hc_nonlinear_end(h.ctx, None, None, None), lib.hc_morison_end(h.ctx, dp(out)), lib.hc_drift_end(h.ctx, dp(out)),
                lib.hc_sum_qtf_end(h.ctx, dp(out)))

    def expected(t, st):
        total = raw_step(b, t, st)
        nl, mor, dft, smf = terms_alone(b, t, st)
        assert nl[1].any() and mor.any() and dft.any() and smf.any()
        return s2.compose4(total, nl, mor, dft, smf, 2, SURFACED)

    none = (INV, INV, INV, INV)
    t0, t1, t2 = (float(t) for t in s2.SUBSET_TIMES[:3])
    # (i) a sum evaluation begun by hand: the fourth begin of step() is refused, the first three are unwound
    st = motion.state(t0)
    a.sum_qtf_begin(t0, st[0])
    with pytest.raises(HydroError):
        a.step(t0, *st)
    assert pending(a) == (INV, INV, INV, OK)
    want = expected(t0, st)
    assert same_bits(a.step(t0, *st), want) and same_bits(grp.step(t0, *st), want)
    assert pending(a) == none
    # (ii) a drift evaluation begun by hand: refused at the third begin, the first two are unwound, the sum one never begun
    st = motion.state(t1)
    a.drift_begin(t1, st[0])
    with pytest.raises(HydroError):
        a.step(t1, *st)
    assert pending(a) == (INV, INV, OK, INV)
    want = expected(t1, st)
    assert same_bits(a.step(t1, *st), want) and same_bits(grp.step(t1, *st), want)
    # (iii) three shards, a sum evaluation pending on shard 1 only: what shard 0 (and every shard, for the other terms) had begun is unwound
    st = motion.state(t2)
    grp.shards[1].sum_qtf_begin(t2, st[0])
    with pytest.raises(HydroError):
        grp.step(t2, *st)
    assert [pending(s) for s in grp.shards] == [none, (INV, INV, INV, OK), none]
    want = expected(t2, st)
    assert same_bits(grp.step(t2, *st), want) and same_bits(a.step(t2, *st), want)
    assert [pending(s) for s in grp.shards] == [none] * 3 and pending(a) == none
    for h in (a, b, grp):
        h.close()


# ------------------------------------------------------------------------------------------------
# 6: the C++ mirror, several bodies and shards
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_all_terms_on_shards(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "side_terms2_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "side_terms2_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "four_body.h5")
    outputs = []
    for devices in ("0", "0,0", "0,0,0,0"):
        r = subprocess.run([exe, h5, devices], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (devices, r.returncode, r.stderr)
        outputs.append(r.stdout)
    assert outputs[0] and outputs[1] == outputs[0] and outputs[2] == outputs[0]  # identical text whatever the device list
    rows = np.array([[float.fromhex(v) for v in line.split()] for line in outputs[0].strip().splitlines()])
    assert rows.shape == (s2.CPP_STEPS, 1 + 48 + 24 + 24 + 72 + 24 + 24)
    lists = s2.cpp_lists()
    h = HF(4)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(num_bodies=4, **s2.CPP_WAVES)
    for b in range(4):
        if lists["surfaces"][b] is not None:
            kind, data = lists["surfaces"][b]
            (h.set_surface_mesh(b, data, clip=True) if kind == "tris" else h.set_surface_panels(b, *data))
        if lists["elements"][b] is not None:
            h.set_morison_elements(b, *lists["elements"][b])
        if lists["tables"][b] is not None:
            h.set_drift_qtf(b, *lists["tables"][b])
        if lists["sums"][b] is not None:
            h.set_sum_qtf(b, *lists["sums"][b])
    h.set_nonlinear_options(**si.CPP_NL_OPTS)
    h.set_morison_options(**si.CPP_MOR_OPTS)
    h.set_drift_mode(3)
    h.set_sum_mode(1)
    h.set_nonlinear_second_order(True, diff_band=s2.CPP_NL_BANDS[0], sum_band=s2.CPP_NL_BANDS[1])
    h.set_morison_second_order(True, diff_band=s2.CPP_MOR_BANDS[0], sum_band=s2.CPP_MOR_BANDS[1])
    for n, row in enumerate(rows):
        if n == s2.CPP_SWITCH:
            h.add_waves_irregular(num_bodies=4, **s2.CPP_WAVES_AFTER)
        t, st = si.cpp_state(n)
        assert row[0] == t and same_bits(row[1:49].reshape(4, 4, 3), np.stack(st, axis=1)), n  # the state the caller printed
        total = raw_step(h, t, st)
        nl, mor, dft, smf = terms_alone(h, t, st)
        assert same_bits(row[73:97], mor) and same_bits(row[97:169], np.concatenate(nl)) and same_bits(row[169:193], dft), n
        assert same_bits(row[193:217], smf), n
        assert same_bits(row[49:73], s2.compose4(total, nl, mor, dft, smf, 2, s2.CPP_SURFACE_BODIES)), n
        on = (lambda x: [bool(v.any()) for v in x.reshape(4, 6)])
        assert on(nl[0]) == on(nl[1]) == [True, False, True, False] and on(mor) == [False, True, True, False], n
        assert on(dft) == [True, False, False, True] and on(smf) == [False, True, True, False], n
        assert h.nonlinear_increments(0)["eta2"].any() and h.morison_increments(2)["eta2"].any(), n  # order 2 did run
    k = s2.CPP_SWITCH
    for cols in (slice(79, 85), slice(121, 127), slice(169, 175), slice(199, 205)):  # the model did switch: every term moved
        assert not np.allclose(rows[k - 1, cols], rows[k, cols], rtol=1e-3), cols
    h.close()
