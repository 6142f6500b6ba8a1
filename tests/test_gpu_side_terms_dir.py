"""The Morison, nonlinear, drift and sum-frequency terms TOGETHER in directional seas, with the first-order excitation on a heading
grid, across changes of the directions: what tests/test_gpu_side_terms2.py checks for the second-order sea, for the state added
since -- the direction columns of the three privately owned component tables (csrc/hc_morison.hip, hc_nonlinear.hip, hc_qtf.hip),
the node map and heading weights of the QTF terms (csrc/hc_qtf_dir.hip), the excitation tables apply_wave_directions rebuilds
(csrc/hc_directions.cpp), and the refusals the library itself produces under directions.  Each term alone is the subject of
tests/test_gpu_directional.py and tests/test_gpu_qtf_dir.py; here

  * where the library promises bits, bits are asserted: against the same term computed alone, against a
    one-context run, and against a fresh context created directly in the state under test;
  * values are held to the references of those files (tests/directional_ref.py, qtf_dir_ref.py, spectral_ref.py on the tables
    directional_ref.heading_tables interpolates) with the bounds they derive.  No tolerance is introduced here.

The inputs are fixed in tests/side_terms_dir_inputs.py; tests/test_side_terms_dir_cpu.py asserts on the CPU that every (model,
directions, t, state) held to a reference keeps the references' conditions.  The comparisons below assert them again on the
context's own spectrum."""
import os
import subprocess
import time

import numpy as np
import pytest

import nonlinear2_inputs as ni
import side_terms2_inputs as s2
import side_terms_dir_inputs as sd
import side_terms_inputs as si
from cases import GOLDEN_DIR, three_body_case
from side_terms_inputs import same_bits
from test_gpu_side_terms2 import HF, Worst, all_terms, apply_model, hold_qtf, last_terms, raw_step, same_terms, terms_alone  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURFACED = sd.SURFACED
TERMS = ("nonlinear", "morison", "drift", "sum")


class WorstDir(Worst):
    def __init__(self):
        super().__init__()
        self.w["excitation"] = 0.0


def modes_on(h):
    h.set_nonlinear_mode(2)
    h.set_drift_mode(3)
    h.set_sum_mode(1)


def set_directions(h, nf, which):
    h.set_wave_directions(None if which is None else sd.directions(nf, which))


def waves_of(h):
    """the wave component of every owned row at the model's own evaluation, of a HydroForces or a HydroGroup"""
    return lambda t: np.concatenate([s.compute_waves(t) for s in getattr(h, "shards", [h])])


def hold_to_references(worst, case, g, lists, comp, rd, stretch, t, st, terms, what, seen=None):
    """terms = (nonlinear, morison, {drift mode: drift}, sum) of the GPU inside the references' bounds at one state; conditions first"""
    ref = sd.references(case, g, lists, comp, rd, stretch, t, st, drift_modes=tuple(terms[2]))
    cases = sd.check_conditions(ref, lists, what)
    sd.check_qtf_conditions(ref, what)
    if seen is not None:
        seen += cases
    (buoy, fk, _), mor, dft, smf = terms
    worst.hold("buoy", buoy, ref["nl"]["buoy"], ref["nl"]["bound_buoy"], what)
    worst.hold("fk", fk, ref["nl"]["fk"], ref["nl"]["bound_fk"], what)
    worst.hold("morison", mor, ref["mor"]["F"], ref["mor"]["bound"], what)
    hold_qtf(worst, ref, dft, smf, what)
    return ref


def hold_excitation(worst, case, spec, theta, rd, t, got, what):
    F, B = sd.excitation_reference(case, spec, theta, rd, [t])
    assert np.abs(np.asarray(F[0], dtype=np.float64)).max() > 0.0, what
    worst.hold("excitation", got, np.asarray(F[0], dtype=np.float64), B[0], what)


# ------------------------------------------------------------------------------------------------
# 1: all four together, in order, under a spread sea
# ------------------------------------------------------------------------------------------------
def run_compose(HF, small, nf, held, test):
    """a: everything on, through step().  b: the same lists, used through raw hc_step and the terms' own calls only.  plain: the same
    sea and directions, no term.  grp: three shards, everything on."""
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    lists = sd.compose_lists(small=small)
    waves = ni.waves(nf)
    th = sd.directions(nf, "A")
    a, b, plain = (HF.from_case(case) for _ in range(3))
    grp = HydroGroup.from_case(case, 3)
    for h in (a, b, grp):
        sd.prepare(h, case, lists)
        modes_on(h)
    sd.set_excitation_headings(plain, case)
    for h in (a, b, plain, grp):
        h.add_waves_irregular(spectral=True, **waves)
    base = a.set_wave_spreading(**sd.SPREAD)  # spread A is the generator's spread with some components moved onto heading nodes
    k = sd.node_stride(nf)
    assert np.array_equal(np.delete(base, np.arange(0, nf, k)), np.delete(th, np.arange(0, nf, k))) and not np.array_equal(base, th)
    for h in (a, b, plain, grp):
        h.set_wave_directions(th)
    assert np.array_equal(a.wave_directions(), th) and np.array_equal(grp.wave_directions(), th)
    comp, rd, stretch = sd.components(a, "spectral", waves, "A")
    spec = a.irreg_spectrum()
    assert comp[0].size == nf and max(sd.COMPOSE_TIMES) < rd
    sd.check_grids(comp, lists, f"waves({nf})")
    g = abs(a.simulation_parameters()[1])
    motion = sd.compose_motion()
    worst = WorstDir()
    z6 = np.zeros(6)
    differs = 0
    t_ref = 0.0
    for n in range(sd.STEPS):
        t = float(sd.COMPOSE_TIMES[n])
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
        # y enters: a transverse force in every term
        assert nl[1][1] != 0.0 and mor[7] != 0.0 and mor[13] != 0.0, what
        if n in held:
            t0 = time.perf_counter()
            hold_to_references(worst, case, g, lists, comp, rd, stretch, t, st, (nl, mor, {3: dft}, smf), what)
            hold_excitation(worst, case, spec, th, rd, t, b.components()[2], what)
            t_ref += time.perf_counter() - t0
    assert differs > 0  # the order of the drift and sum additions is visible in these inputs
    worst.report(test)
    print(f"{test}: references {t_ref:.1f} s")
    for h in (a, b, plain, grp):
        h.close()


def test_all_four_compose_in_order_under_a_spread_sea(HF):
    """1a: the full lists (257 triangles, 5 panels, 7 and 300 elements, tables of 33, 32, 27 and 33 nodes) in five components"""
    run_compose(HF, False, 5, sd.BOUND_STEPS, "test_all_four_compose_in_order_under_a_spread_sea")


def test_all_four_compose_in_order_above_one_tile(HF):
    """1b: the small lists in 300 components, above one tile of 256"""
    run_compose(HF, True, 300, (sd.BOUND_STEP_LARGE,), "test_all_four_compose_in_order_above_one_tile")


# ------------------------------------------------------------------------------------------------
# 2: every subset
# ------------------------------------------------------------------------------------------------
def three_irreg(HF, n_plain=1, group=True):
    """(case, lists, a, b, [plain ...], grp): three_body_case in the spectral model of si.THREE_IRREG under spread A, everything on
    on a, b and grp"""
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    lists = sd.compose_lists()
    a, b = HF.from_case(case), HF.from_case(case)
    plains = [HF.from_case(case) for _ in range(n_plain)]
    grp = HydroGroup.from_case(case, 3) if group else None
    full = [h for h in (a, b, grp) if h is not None]
    for h in full:
        sd.prepare(h, case, lists)
        modes_on(h)
    for h in plains:
        sd.set_excitation_headings(h, case)
    for h in full + plains:
        h.add_waves_irregular(spectral=True, **si.THREE_IRREG)
        set_directions(h, si.THREE_IRREG["nfrequencies"], "A")
    return case, lists, a, b, plains, grp


def test_every_subset_of_terms_under_directions(HF):
    """a: the context under test.  b: everything on, each term computed alone.  plain: nothing set."""
    case, lists, a, b, (plain,), _ = three_irreg(HF, group=False)
    motion = sd.compose_motion()
    key = dict(nonlinear="surfaces", morison="elements", drift="tables", sum="sums")
    mode_of = dict(nonlinear=("set_nonlinear_mode", 2), drift=("set_drift_mode", 3), sum=("set_sum_mode", 1))  # Morison has no mode
    ways = {name: (["mode", "clear"] if name in mode_of else ["clear"]) for name in TERMS}
    off_by = {}
    used = {name: set() for name in TERMS}

    def switch(name, on):
        if on:
            if off_by[name] == "mode":
                getattr(a, mode_of[name][0])(mode_of[name][1])
            else:
                sd.set_lists(a, lists, (key[name],))
            del off_by[name]
        else:
            if ways[name][0] == "mode":
                getattr(a, mode_of[name][0])(0)
            else:
                sd.clear_lists(a, (key[name],))
            off_by[name] = ways[name][0]
            used[name].add(ways[name][0])
            ways[name].append(ways[name].pop(0))

    # bit 3: Morison, bit 2: drift, bit 1: sum, bit 0: nonlinear; 15 down to 0, everything on again, everything off again
    sequence = list(range(15, -1, -1)) + [15, 0]
    assert len(sequence) + 7 <= len(sd.SUBSET_TIMES)
    bit = dict(nonlinear=0, sum=1, drift=2, morison=3)
    state = {name: True for name in TERMS}
    for subset, t in zip(sequence, sd.SUBSET_TIMES):
        t = float(t)
        for name in TERMS:
            target = bool(subset >> bit[name] & 1)
            if target != state[name]:
                switch(name, target)
                state[name] = target
        st = motion.state(t)
        fa = a.step(t, *st)
        total = raw_step(b, t, st)
        nl, mor, dft, smf = terms_alone(b, t, st)
        assert nl[0].any() and nl[1].any() and mor.any() and dft.any() and smf.any()
        want = s2.compose4(total, nl if state["nonlinear"] else None, mor if state["morison"] else None, dft if state["drift"] else None,
                           smf if state["sum"] else None, 2, SURFACED)
        assert same_bits(fa, want), (subset, dict(off_by))
        assert same_bits(total, plain.step(t, *st))
        assert same_bits(fa, total) == (subset == 0)
        got = last_terms(a)
        assert [bool(got[0][0].any()), bool(got[1].any()), bool(got[2].any()), bool(got[3].any())] == [state[k] for k in TERMS], subset
    assert all(used[name] == ({"mode", "clear"} if name in mode_of else {"clear"}) for name in TERMS), used
    assert not any(state.values())
    # step_many composes no side term: its rows are step() calls of a context without a term, whatever is set
    k = len(sequence)
    for on in (False, True):
        if on:
            for name in TERMS:
                switch(name, True)
        ts = sd.SUBSET_TIMES[k:k + 3]
        k += 3
        states = np.stack([motion.packed(float(t)) for t in ts])
        many = a.step_many(ts, states)[0]
        assert same_bits(many, np.stack([plain.step(float(t), *motion.state(float(t))) for t in ts])), on
        for t in ts:
            raw_step(b, float(t), motion.state(float(t)))  # b keeps a's history
    t = float(sd.SUBSET_TIMES[k])
    st = motion.state(t)
    fa = a.step(t, *st)
    total = raw_step(b, t, st)
    assert not same_bits(fa, plain.step(t, *st)) and same_bits(fa, s2.compose4(total, *terms_alone(b, t, st), 2, SURFACED))
    for h in (a, b, plain):
        h.close()


# ------------------------------------------------------------------------------------------------
# 3: the tables follow the directions and the model
# ------------------------------------------------------------------------------------------------
def nf_of(kind, params):
    return 1 if kind == "regular" else (params["nfrequencies"] if params else 0)


def evaluate(h, t, st, kind):
    """(nonlinear, morison, {1, 3: drift}, sum, excitation or None) of a HydroForces or a HydroGroup"""
    exc = waves_of(h)(t) if kind in ("regular", "spectral") else None
    return all_terms(h, t, st) + (exc,)


def same_eval(x, y):
    return (all(same_bits(p, q) for p, q in zip(x[0], y[0])) and same_bits(x[1], y[1]) and all(same_bits(x[2][m], y[2][m]) for m in (1, 3))
            and same_bits(x[3], y[3]) and ((x[4] is None and y[4] is None) or same_bits(x[4], y[4])))


def moved_terms(got, before):
    out = dict(nl=not same_bits(got[0][1], before[0][1]) or not same_bits(got[0][0], before[0][0]), mor=not same_bits(got[1], before[1]),
               dft1=not same_bits(got[2][1], before[2][1]), dft3=not same_bits(got[2][3], before[2][3]), sum=not same_bits(got[3], before[3]))
    if got[4] is not None and before[4] is not None:
        out["exc"] = not same_bits(got[4], before[4])
    return out


def test_tables_follow_the_directions_and_the_model(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError, HydroGroup
    case = si.synth_case()
    lists = sd.sequence_lists()
    h, grp = HF.from_case(case), HydroGroup.from_case(case, 2)
    for x in (h, grp):
        sd.prepare(x, case, lists, phase=sd.SEQ_PHASE)
        x.set_sum_mode(1)
        x.set_nonlinear_mode(2)
    g = abs(h.simulation_parameters()[1])
    worst = WorstDir()
    seen = np.zeros(4, dtype=int)
    results, t_ref = {}, 0.0
    prev = None

    def refused(fn, code):
        with pytest.raises(HydroError) as e:
            fn()
        assert e.value.status == code, str(e.value)

    for i, (name, kind, params, which, changed, must, still) in enumerate(sd.WALK):
        nf = nf_of(kind, params)
        for x in (h, grp):
            if prev is None or (kind, params) != (prev[1], prev[2]) or changed == "model":
                apply_model(x, kind, params)
                assert x.wave_directions().size == 0, name  # every wave setter drops the directions
            set_directions(x, nf, which)
        want_dirs = np.zeros(0) if which is None else sd.directions(nf, which)
        assert np.array_equal(h.wave_directions(), want_dirs) and np.array_equal(grp.wave_directions(), want_dirs), name
        fresh = HF.from_case(case)  # created directly in this state
        sd.prepare(fresh, case, lists, phase=sd.SEQ_PHASE)
        fresh.set_sum_mode(1)
        fresh.set_nonlinear_mode(2)
        apply_model(fresh, kind, params)
        set_directions(fresh, nf, which)
        comp, rd, stretch = sd.components(h, kind, params, which)
        spec = h.irreg_spectrum() if kind == "spectral" else None
        if comp is not None:
            assert comp[0].size == nf
            sd.check_grids(comp, lists, name, regular=kind == "regular")
        for t in sd.SEQ_TIMES:
            st = sd.sequence_state(t)
            what = f"{name} t={t}"
            got = evaluate(h, t, st, kind)
            assert same_eval(got, evaluate(fresh, t, st, kind)), what   # (a) a fresh context in this state
            assert same_eval(evaluate(grp, t, st, kind), got), what     # (b) the group walked alongside
            results[(i, t)] = got
            nl, mor, dft, smf, exc = got
            has_waves = comp is not None
            assert nl[0][0:6].any() and nl[0][12:18].any() and mor[6:12].any() and mor[12:18].any() and bool(nl[1].any()) == has_waves, what
            for b in range(3):
                has_dft, has_sum = has_waves and lists["tables"][b] is not None, has_waves and lists["sums"][b] is not None
                r = slice(6 * b, 6 * b + 6)
                assert bool(dft[1][r].any()) == bool(dft[3][r].any()) == has_dft and bool(smf[r].any()) == has_sum, (what, b)
                if not has_dft:
                    assert same_bits(dft[1][r], np.zeros(6)) and same_bits(dft[3][r], np.zeros(6)), (what, b)
                if not has_sum:
                    assert same_bits(smf[r], np.zeros(6)), (what, b)
            t0 = time.perf_counter()
            if i in sd.HELD + sd.HELD_TERMS:
                ref = hold_to_references(worst, case, g, lists, comp, rd, stretch, t, st, got[:4], what, seen=seen)
                if i in sd.HELD and kind == "spectral":
                    hold_excitation(worst, case, spec, None if which is None else comp[4], rd, t, exc, what)
                if changed == "zero to none":
                    # (e) all zeros against cleared: the kinematic terms run in other instantiations; either is within the bound
                    # of the exact value
                    zero = results[(i - 1, t)]
                    for x, y, bound in ((nl[0], zero[0][0], ref["nl"]["bound_buoy"]), (nl[1], zero[0][1], ref["nl"]["bound_fk"]),
                                        (mor, zero[1], ref["mor"]["bound"])):
                        assert np.all(np.abs(x - y) <= 2 * np.asarray(bound).reshape(-1)), what
            t_ref += time.perf_counter() - t0
            # (c) what changed against the entry before moved every term that depends on it, and none that does not; (d) all zeros
            # against cleared: the QTF terms keep their bits
            if prev is not None:
                moved = moved_terms(got, results[(i - 1, t)])
                assert all(moved[k] for k in must if k in moved), (what, changed, moved)
                assert not any(moved[k] for k in still), (what, changed, moved)
        if kind in ("regular", "spectral"):  # one step of each: the same total and the same excitation component
            t = sd.SEQ_TIMES[-1]
            st = sd.sequence_state(t)
            steps = []
            for x in (h, fresh, grp):
                x.reset_history()
                x.set_drift_mode(3)
                steps.append((x.step(t, *st), x.components()[2]))
            assert all(same_bits(s[0], steps[0][0]) and same_bits(s[1], steps[0][1]) for s in steps[1:]), name
            assert steps[0][1].any() and not same_bits(steps[0][0], raw_step(fresh, t, st)), name
        # the refusals leave the state and the bits
        before = results[(i, sd.SEQ_TIMES[0])]
        t, st = sd.SEQ_TIMES[0], sd.sequence_state(sd.SEQ_TIMES[0])
        if kind == "irregular":
            for x in (h, grp):
                refused(lambda: x.set_wave_directions(sd.directions(nf, "A")), capi.HC_ERR_UNSUPPORTED)
                assert np.array_equal(x.wave_directions(), want_dirs) and same_eval(evaluate(x, t, st, kind), before), name
        if kind == "eta":
            for x in (h, grp):
                refused(lambda: x.set_wave_directions([0.1]), capi.HC_ERR_INVALID)
                assert x.wave_directions().size == 0 and same_eval(evaluate(x, t, st, kind), before), name
        if name.startswith("5 "):  # a uniform heading: body 0 may lose its heading tables; non-uniform directions are then refused
            for x in (h, grp):
                x.set_body_excitation_rao_headings(0, [], [], [], [])
                without = evaluate(x, t, st, kind)
                assert same_eval(without[:4] + (None,), before[:4] + (None,)) and not same_bits(without[4][0:6], before[4][0:6]), name
                assert same_bits(without[4][6:], before[4][6:]), name
                refused(lambda: x.set_wave_directions(sd.directions(nf, "A")), capi.HC_ERR_INVALID)
                assert np.array_equal(x.wave_directions(), want_dirs) and same_eval(evaluate(x, t, st, kind), without), name
                sd.set_excitation_headings(x, case, only=(0,))
                assert same_eval(evaluate(x, t, st, kind), before), name
        fresh.close()
        prev = sd.WALK[i]
    at = {e[0].split()[0]: k for k, e in enumerate(sd.WALK)}
    for t in sd.SEQ_TIMES:
        assert same_eval(results[(at["11"], t)], results[(at["3"], t)])  # (f)
        assert not same_bits(results[(at["1"], t)][4], results[(at["2"], t)][4])
    assert np.all(seen > 0), seen.tolist()  # triangles with 0, 1, 2 and 3 wet vertices among the states held to the references
    worst.report("test_tables_follow_the_directions_and_the_model")
    print(f"test_tables_follow_the_directions_and_the_model: references {t_ref:.1f} s")
    h.close()
    grp.close()


# ------------------------------------------------------------------------------------------------
# 4: a direction change while evaluations are pending
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after", ["B", None])
def test_end_returns_the_directions_of_its_begin(HF, after):
    case, lists, h, fresh, _, _ = three_irreg(HF, n_plain=0, group=False)
    nf = si.THREE_IRREG["nfrequencies"]
    set_directions(fresh, nf, after)
    t = float(sd.SUBSET_TIMES[1])
    st = sd.compose_motion().state(t)
    under_a = terms_alone(h, t, st)
    h.nonlinear_begin(t, st[0], st[1])
    h.morison_begin(t, *st)
    h.drift_begin(t, st[0])
    h.sum_qtf_begin(t, st[0])
    set_directions(h, nf, after)  # accepted: the launches are enqueued on the terms' own tables
    ended = (h.nonlinear_end(), h.morison_end(), h.drift_end(), h.sum_qtf_end())
    assert same_terms(ended, under_a)
    then = terms_alone(h, t, st)
    assert same_terms(then, terms_alone(fresh, t, st))
    assert not same_bits(then[0][1], ended[0][1])
    assert all(not same_bits(then[k], ended[k]) and then[k].any() and ended[k].any() for k in (1, 2, 3))
    assert same_bits(h.compute_waves(t), fresh.compute_waves(t))
    h.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------
# 5: unwinding after a begin the library refuses under directions
# ------------------------------------------------------------------------------------------------
def test_refused_begins_under_directions_leave_nothing_pending(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    INV, OK, UNS = capi.HC_ERR_INVALID, capi.HC_OK, capi.HC_ERR_UNSUPPORTED
    dp = (lambda x: x.ctypes.data_as(capi.c_double_p))
    case, lists, a, b, _, grp = three_irreg(HF, n_plain=0)
    lib = a.lib
    motion = sd.compose_motion()

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
    drift2, sum0, sum2 = lists["tables"][2], lists["sums"][0], lists["sums"][2]
    restore_drift2 = (lambda h: h.set_drift_qtf(2, *drift2[1:], headings=drift2[0]))
    # cause, its undoing, the status and a word of the message; each is refused by another begin of step()
    cases = [
        ("nonlinear second order", lambda h: h.set_nonlinear_second_order(True), lambda h: h.set_nonlinear_second_order(False), UNS, "direction"),
        ("morison second order", lambda h: h.set_morison_second_order(True), lambda h: h.set_morison_second_order(False), UNS, "direction"),
        ("drift grid of body 2 one ulp short", lambda h: h.set_drift_qtf(2, *sd.narrow(drift2)[1:], headings=sd.narrow(drift2)[0]), restore_drift2,
         INV, "heading grid"),
        ("sum grid of body 2 one ulp short", lambda h: h.set_sum_qtf(2, *sd.narrow(sum2)[1:], headings=sd.narrow(sum2)[0]),
         lambda h: h.set_sum_qtf(2, *sum2[1:], headings=sum2[0]), INV, "heading grid"),
        ("a one-heading sum table on body 0", lambda h: h.set_sum_qtf(0, *sd.one_heading(sum0)),
         lambda h: h.set_sum_qtf(0, *sum0[1:], headings=sum0[0]), UNS, "one heading"),
    ]
    for k, (what, cause, undo, code, word) in enumerate(cases):
        t = float(sd.SUBSET_TIMES[k])
        st = motion.state(t)
        for h in (a, grp):
            cause(h)
            with pytest.raises(HydroError) as e:
                h.step(t, *st)
            assert e.value.status == code and word in str(e.value), (what, str(e.value))
            assert [pending(s) for s in getattr(h, "shards", [h])] == [none] * len(getattr(h, "shards", [h])), what
            undo(h)
        want = expected(t, st)
        assert same_bits(a.step(t, *st), want) and same_bits(grp.step(t, *st), want), what
        assert pending(a) == none and [pending(s) for s in grp.shards] == [none] * 3, what
    # three shards, the too-narrow heading grid on the body of shard 1 only: what shards 0 and 2 had begun is unwound
    t = float(sd.SUBSET_TIMES[len(cases)])
    st = motion.state(t)
    narrow = sd.narrow(drift2)
    grp.set_drift_qtf(1, *narrow[1:], headings=narrow[0])
    own = [s.b0 for s in grp.shards]
    assert own == [0, 1, 2]
    for s, ok in zip(grp.shards, (True, False, True)):  # the refusal is shard 1's alone
        if ok:
            s.drift_begin(t, st[0])
            s.drift_end()
        else:
            with pytest.raises(HydroError):
                s.drift_begin(t, st[0])
    with pytest.raises(HydroError) as e:
        grp.step(t, *st)
    assert e.value.status == INV and "heading grid" in str(e.value)
    assert [pending(s) for s in grp.shards] == [none] * 3
    grp.set_drift_qtf(1, [], None)
    want = expected(t, st)
    assert same_bits(grp.step(t, *st), want) and same_bits(a.step(t, *st), want)
    assert [pending(s) for s in grp.shards] == [none] * 3 and pending(a) == none
    for h in (a, b, grp):
        h.close()


# ------------------------------------------------------------------------------------------------
# 6: the C++ mirror, several bodies and shards
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_all_terms_on_shards_under_a_heading(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "side_terms_dir_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "side_terms_dir_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "four_body.h5")
    outputs = []
    for devices in ("0", "0,0", "0,0,0,0"):
        r = subprocess.run([exe, h5, devices], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (devices, r.returncode, r.stderr)
        outputs.append(r.stdout)
    assert outputs[0] and outputs[1] == outputs[0] and outputs[2] == outputs[0]  # identical text whatever the device list
    rows = np.array([[float.fromhex(v) for v in line.split()] for line in outputs[0].strip().splitlines()])
    assert rows.shape == (sd.CPP_STEPS, 1 + 48 + 24 + 24 + 72 + 24 + 24)
    lists = sd.cpp_lists()
    h = HF(4)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(num_bodies=4, **sd.CPP_WAVES)
    nf = sd.CPP_WAVES["nfrequencies"]
    for b in range(4):
        h.set_body_excitation_rao_headings(b, *sd.cpp_excitation_headings(b))
        if lists["surfaces"][b] is not None:
            kind, data = lists["surfaces"][b]
            (h.set_surface_mesh(b, data, clip=True) if kind == "tris" else h.set_surface_panels(b, *data))
        if lists["elements"][b] is not None:
            h.set_morison_elements(b, *lists["elements"][b])
        for key, setter in (("tables", h.set_drift_qtf), ("sums", h.set_sum_qtf)):
            if lists[key][b] is not None:
                beta, g, P, Q = lists[key][b]
                setter(b, g, P, Q, headings=beta)
    h.set_nonlinear_options(**si.CPP_NL_OPTS)
    h.set_morison_options(**si.CPP_MOR_OPTS)
    modes_on(h)
    h.set_wave_directions(np.full(nf, sd.CPP_HEADINGS[0]))
    switches = (sd.CPP_SWITCH, sd.CPP_REGULAR + sd.CPP_SWITCH)
    for n, row in enumerate(rows):
        if n == sd.CPP_REGULAR:
            h.add_waves_regular(*sd.CPP_REG, num_bodies=4)
            nf = 1
            h.set_wave_directions(np.full(nf, sd.CPP_HEADINGS[0]))
        if n in switches:
            h.set_wave_directions(np.full(nf, sd.CPP_HEADINGS[1]))
        t, st = si.cpp_state(n)
        assert row[0] == t and same_bits(row[1:49].reshape(4, 4, 3), np.stack(st, axis=1)), n  # the state the caller printed
        total = raw_step(h, t, st)
        nl, mor, dft, smf = terms_alone(h, t, st)
        assert same_bits(row[73:97], mor) and same_bits(row[97:169], np.concatenate(nl)) and same_bits(row[169:193], dft), n
        assert same_bits(row[193:217], smf), n
        assert same_bits(row[49:73], s2.compose4(total, nl, mor, dft, smf, 2, sd.CPP_SURFACE_BODIES)), n
        on = (lambda x: [bool(v.any()) for v in x.reshape(4, 6)])
        assert on(nl[0]) == on(nl[1]) == [True, False, True, False] and on(mor) == [False, True, True, False], n
        assert on(dft) == [True, False, False, True] and on(smf) == [False, True, True, False], n
    for k in switches:  # the heading did switch: every term moved (Morison body 2, fk body 1, drift body 1, sum body 2)
        for cols in (slice(79, 85), slice(121, 127), slice(169, 175), slice(199, 205)):
            assert not np.allclose(rows[k - 1, cols], rows[k, cols], rtol=1e-3), (k, cols)
    # in the regular wave the excitation follows the heading tables: the total of a body without any term moves with the heading
    plain = HF(4)
    plain.load_bemio_h5(h5)
    plain.finalize()
    plain.add_waves_regular(*sd.CPP_REG, num_bodies=4)
    for b in range(4):
        plain.set_body_excitation_rao_headings(b, *sd.cpp_excitation_headings(b))
    waves = []
    for heading in sd.CPP_HEADINGS:
        plain.set_wave_directions([heading])
        waves.append(plain.compute_waves(2.25))
    assert not np.allclose(waves[0], waves[1], rtol=1e-3)
    h.close()
    plain.close()
