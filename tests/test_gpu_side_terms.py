"""The Morison, nonlinear and drift terms TOGETHER and across wave-model changes (csrc/hc_morison.hip, hc_nonlinear.hip, hc_qtf.hip and
the three layers that compose them: HydroForces.step, HydroGroup.step, TestHydro::CoordinateFuncForBody).  Each term alone is the
subject of tests/test_gpu_morison.py, test_gpu_nonlinear.py and test_gpu_drift.py; here

  * where the library promises bits, bits are asserted: against the same term computed alone (compute_morison, compute_nonlinear,
    compute_drift, raw hc_step), against a one-context run, and against a fresh context created directly in the state under test;
  * values are held to the references of those files (tests/morison_ref.py, nonlinear_ref.py, drift_ref.py) with the bounds they
    derive.  No tolerance is introduced here.

The inputs are fixed in tests/side_terms_inputs.py; tests/test_side_terms_cpu.py asserts on the CPU that every (model, t, state) used
below keeps the references' conditions (1e-6 m from the free surface, 0 < wet < n, |theta| < 1e4, grids around the components).  The
comparisons below assert the margin again on the context's own spectrum."""
import os
import subprocess

import numpy as np
import pytest

import drift_ref as dr
import morison_ref as mr
import side_terms_inputs as si
from cases import GOLDEN_DIR, three_body_case
from side_terms_inputs import same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANELLED = (0, 2)  # bodies with panels; elements on (1, 2); drift tables on (0, 2)


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


def terms_alone(h, t, st):
    """(nonlinear (buoy, fk, hs_lin), morison, drift) of a HydroForces or HydroGroup, each term computed alone"""
    return h.compute_nonlinear(t, st[0], st[1]), h.compute_morison(t, *st), h.compute_drift(t, st[0])


def same_terms(x, y):
    return all(same_bits(p, q) for p, q in zip(x[0], y[0])) and same_bits(x[1], y[1]) and same_bits(x[2], y[2])


def last_terms(h):
    return h.nonlinear(), h.morison(), h.drift()


class Worst:
    """worst |gpu - ref| / bound per term over a test, printed at its end"""

    def __init__(self):
        self.w = dict(buoy=0.0, fk=0.0, morison=0.0, drift=0.0)

    def hold(self, name, got, want, bound, what):
        got, want, bound = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, want, bound))
        assert got.shape == want.shape and np.all(np.isfinite(got)), (what, name)
        err = np.abs(got - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        self.w[name] = max(self.w[name], worst)
        assert np.all(err <= bound), f"{what} {name}: worst {worst:.3e} of the bound"

    def report(self, test):
        print(f"{test}: worst |gpu - ref| / bound: " + ", ".join(f"{k} {v:.3e}" for k, v in self.w.items()))


def hold_to_references(worst, case, lists, comp, rd, stretch, t, st, terms, drift_modes, what, comp_mor="same"):
    """terms = (nonlinear, morison, {drift mode: drift}) of the GPU inside the references' bounds at one state; margins first.
    comp_mor: the components at the Morison term's own regular phase where that differs."""
    ramp = mr.ramp_factor(t, rd)
    ref = si.references(case, lists, comp, t, st, ramp, si.NL_OPTS, si.MOR_OPTS, stretch, comp_mor=comp_mor)
    si.check_conditions(ref, lists, what)
    (buoy, fk, _), mor, dft = terms
    worst.hold("buoy", buoy, ref["nl"]["buoy"], ref["nl"]["bound_buoy"], what)
    worst.hold("fk", fk, ref["nl"]["fk"], ref["nl"]["bound_fk"], what)
    worst.hold("morison", mor, ref["mor"]["F"], ref["mor"]["bound"], what)
    pos = np.asarray(st[0]).reshape(-1, 3)
    for mode in drift_modes:
        got = np.asarray(dft[mode]).reshape(-1, 6)
        for b, tb in enumerate(lists["tables"]):
            if tb is None or comp is None:
                assert not got[b].any(), (what, "drift", mode, b)
                continue
            want = dr.PairSum(comp, tb).force(t, pos[b, 0], ramp=ramp)[mode]
            worst.hold("drift", got[b], want, dr.bounds(comp, tb, ramp=ramp)[mode], f"{what} mode {mode} body {b}")
    return ref


def prepare(h, lists, nl_opts=si.NL_OPTS, mor_opts=si.MOR_OPTS, phase=None, mor_phase=None):
    si.set_lists(h, lists)
    h.set_nonlinear_options(regular_phase=0.0 if phase is None else phase, **nl_opts)
    h.set_morison_options(regular_phase=0.0 if mor_phase is None else mor_phase, **mor_opts)
    h.set_drift_options(regular_phase=0.0 if phase is None else phase)


# ------------------------------------------------------------------------------------------------
# 2: all three together, in order
# ------------------------------------------------------------------------------------------------
def test_all_three_compose_in_order(HF):
    """a: everything on, through step().  b: the same lists, used through raw hc_step and the terms' own calls only.  plain: nothing
    set.  Groups of 2 and 3 shards: everything on."""
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    lists = si.compose_lists()
    a, b, plain = (HF.from_case(case) for _ in range(3))
    groups = [HydroGroup.from_case(case, 2), HydroGroup.from_case(case, 3)]
    for h in (a, b, plain, *groups):
        h.add_waves_irregular(**si.THREE_IRREG)
    for h in (a, b, *groups):
        prepare(h, lists)
    comp, rd, stretch = si.model_components(a, "irregular", si.THREE_IRREG, 0.0)
    assert comp[0].size == 200
    si.check_grids(comp, lists, "THREE_IRREG")
    motion = si.compose_motion(case)
    worst = Worst()
    z6 = np.zeros(6)
    differs = 0
    times = iter(si.COMPOSE_TIMES)
    for nl_mode, drift_mode in si.COMBOS:
        for h in (a, *groups):
            h.set_nonlinear_mode(nl_mode)
        for h in (a, b, *groups):
            h.set_drift_mode(drift_mode)
        for n in range(si.STEPS_PER_COMBO):
            t = float(next(times))
            st = motion.state(t)
            what = f"nonlinear mode {nl_mode} drift mode {drift_mode} step {n}"
            fa = a.step(t, *st)
            # b: all three begun, the raw step, all three ended -- three side streams in flight around one hc_step
            b.nonlinear_begin(t, st[0], st[1])
            b.morison_begin(t, *st)
            b.drift_begin(t, st[0])
            total = raw_step(b, t, st)
            nl, mor, dft = b.nonlinear_end(), b.morison_end(), b.drift_end()
            comps = b.components()
            assert same_bits(total, plain.step(t, *st)), what
            assert all(same_bits(x, y) for x, y in zip(comps, plain.components())), what
            # ... and each term computed alone has those bits
            assert same_terms((nl, mor, dft), terms_alone(b, t, st)), what
            want = si.compose(total, nl, mor, dft, nl_mode, PANELLED)
            assert same_bits(fa, want), what
            assert same_terms(last_terms(a), (nl, mor, dft)), what
            for g in groups:
                assert same_bits(g.step(t, *st), fa), (what, len(g.shards))
                assert same_terms(last_terms(g), (nl, mor, dft)), (what, len(g.shards))
            # rows of a body without a term are untouched by it
            assert same_bits(nl[0][6:12], z6) and same_bits(nl[1][6:12], z6) and same_bits(mor[0:6], z6) and same_bits(dft[6:12], z6), what
            assert same_bits(fa[6:12], (total[6:12] + mor[6:12]) + dft[6:12]), what
            r0 = total[0:6] - nl[2][0:6] + nl[0][0:6]
            assert same_bits(fa[0:6], ((r0 + nl[1][0:6] if nl_mode == 2 else r0) + mor[0:6]) + dft[0:6]), what
            differs += not same_bits(fa, (si.compose(total, nl, None, None, nl_mode, PANELLED) + dft) + mor)
            if n in si.BOUND_STEPS:
                hold_to_references(worst, case, lists, comp, rd, stretch, t, st, (nl, mor, {drift_mode: dft}), (drift_mode,), what)
                assert nl[0][0:6].any() and nl[0][12:18].any() and nl[1][0:6].any() and mor[6:12].any() and mor[12:18].any()
                assert dft[0:6].any() and dft[12:18].any()
    assert differs > 0  # the order of the Morison and drift additions is visible in these inputs
    worst.report("test_all_three_compose_in_order")
    for h in (a, b, plain, *groups):
        h.close()


# ------------------------------------------------------------------------------------------------
# 3: subsets and call counts
# ------------------------------------------------------------------------------------------------
def test_every_subset_of_terms(HF, monkeypatch):
    case = three_body_case()
    lists = si.compose_lists()
    a, b, plain = (HF.from_case(case) for _ in range(3))
    for h in (a, b, plain):
        h.add_waves_irregular(**si.THREE_IRREG)
    for h in (a, b):
        prepare(h, lists)
        h.set_drift_mode(3)
    a.set_nonlinear_mode(2)
    calls = []
    for name in ("hc_nonlinear_begin", "hc_morison_begin", "hc_drift_begin"):
        fn = getattr(a.lib, name)
        monkeypatch.setattr(a.lib, name, (lambda *args, _fn=fn, _name=name: (calls.append(_name), _fn(*args))[1]))
    motion = si.compose_motion(case)

    def all_on():
        pass

    def nonlinear_off_by_mode():
        a.set_nonlinear_mode(0)

    def morison_off_by_clearing():
        si.clear_lists(a, ("elements",))

    def drift_off_by_mode():
        a.set_drift_mode(0)

    def nonlinear_on_by_mode():
        a.set_nonlinear_mode(2)

    def morison_on_by_setting():
        si.set_lists(a, lists, ("elements",))

    def morison_off_drift_on():
        si.clear_lists(a, ("elements",))
        a.set_drift_mode(3)

    def only_morison_by_clearing_the_others():  # the modes stay on
        si.clear_lists(a, ("panels", "tables"))
        si.set_lists(a, lists, ("elements",))

    def all_set_again():
        si.set_lists(a, lists, ("panels", "tables"))

    walk = [(all_on, (1, 1, 1)), (nonlinear_off_by_mode, (0, 1, 1)), (morison_off_by_clearing, (0, 0, 1)), (drift_off_by_mode, (0, 0, 0)),
            (nonlinear_on_by_mode, (1, 0, 0)), (morison_on_by_setting, (1, 1, 0)), (morison_off_drift_on, (1, 0, 1)),
            (only_morison_by_clearing_the_others, (0, 1, 0)), (all_set_again, (1, 1, 1))]
    assert len({s for _, s in walk}) == 8 and len(walk) + 4 == len(si.SUBSET_TIMES)
    for (change, (nl_on, mor_on, dft_on)), t in zip(walk, si.SUBSET_TIMES):
        change()
        t = float(t)
        st = motion.state(t)
        del calls[:]
        fa = a.step(t, *st)
        seen = list(calls)
        assert seen == ["hc_nonlinear_begin"] * nl_on + ["hc_morison_begin"] * mor_on + ["hc_drift_begin"] * dft_on, (change.__name__, seen)
        total = raw_step(b, t, st)
        nl, mor, dft = terms_alone(b, t, st)
        assert nl[0].any() and nl[1].any() and mor.any() and dft.any()
        want = si.compose(total, nl if nl_on else None, mor if mor_on else None, dft if dft_on else None, 2, PANELLED)
        assert same_bits(fa, want), change.__name__
        assert same_bits(total, plain.step(t, *st))
        if (nl_on, mor_on, dft_on) == (0, 0, 0):
            assert same_bits(fa, total)
        else:
            assert not same_bits(fa, total)
        assert bool(a.nonlinear()[0].any()) == bool(nl_on) and bool(a.morison().any()) == bool(mor_on) and bool(a.drift().any()) == bool(dft_on)
    # step_many composes no side term: the raw hc_step totals, whatever is set
    ts = si.SUBSET_TIMES[len(walk):len(walk) + 3]
    states = np.stack([motion.packed(float(t)) for t in ts])
    del calls[:]
    many = a.step_many(ts, states)[0]
    assert not calls
    assert same_bits(many, plain.step_many(ts, states)[0])
    t = float(si.SUBSET_TIMES[len(walk) + 3])
    st = motion.state(t)
    assert not same_bits(a.step(t, *st), plain.step(t, *st))  # the terms are on all the while
    for h in (a, b, plain):
        h.close()


# ------------------------------------------------------------------------------------------------
# 4: the tables follow the wave model
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
    """(nonlinear, morison, {1: mean drift, 3: full QTF}): the mean drift reads E_m, the full table the bin map"""
    out = {}
    for mode in (1, 3):
        h.set_drift_mode(mode)
        out[mode] = h.compute_drift(t, st[0])
    return h.compute_nonlinear(t, st[0], st[1]), h.compute_morison(t, *st), out


def same_all(x, y):
    return all(same_bits(p, q) for p, q in zip(x[0], y[0])) and same_bits(x[1], y[1]) and all(same_bits(x[2][m], y[2][m]) for m in (1, 3))


def test_tables_follow_the_wave_model(HF):
    from hydrochrono_amd.hydro import HydroGroup
    case = si.synth_case()
    lists = si.sequence_lists()
    h, grp = HF.from_case(case), HydroGroup.from_case(case, 2)
    for x in (h, grp):
        prepare(x, lists, phase=si.SEQ_PHASE, mor_phase=si.SEQ_PHASE)
    worst = Worst()
    kin_points = np.array([[3.0, 0.0, -1.0], [18.5, 1.0, -4.0]])
    results = {}
    for name, kind, params, mor_phase in si.SEQUENCE:
        before = None
        if name.startswith("2"):
            # the same wave; hc_wave_kinematics rebuilds its own table for another phase, then only the Morison phase moves
            before = {t: all_terms(h, t, si.sequence_state(t)) for t in si.SEQ_TIMES}
            for x in (h, *grp.shards):
                x.wave_kinematics(kin_points, [1.0], regular_phase=1.1)
            for t in si.SEQ_TIMES:
                assert same_all(all_terms(h, t, si.sequence_state(t)), before[t]), name
                assert same_all(all_terms(grp, t, si.sequence_state(t)), before[t]), name
            for x in (h, grp):
                x.set_morison_options(regular_phase=mor_phase, **si.MOR_OPTS)
            for x in (h, *grp.shards):
                x.wave_kinematics(kin_points, [1.0], regular_phase=1.1)
        else:
            for x in (h, grp):
                apply_model(x, kind, params)
        fresh = HF.from_case(case)  # created directly with this model and these options
        apply_model(fresh, kind, params)
        prepare(fresh, lists, phase=si.SEQ_PHASE, mor_phase=mor_phase)
        comp_nl, rd, stretch = si.model_components(h, kind, params, si.SEQ_PHASE)
        comp_mor = si.model_components(h, kind, params, mor_phase)[0]
        if comp_nl is not None:
            assert comp_nl[0].size == (1 if kind == "regular" else params["nfrequencies"])
            si.check_grids(comp_nl, lists, name, regular=kind == "regular")
        for t in si.SEQ_TIMES:
            st = si.sequence_state(t)
            got = all_terms(h, t, st)
            assert same_all(got, all_terms(fresh, t, st)), (name, t)
            assert same_all(all_terms(grp, t, st), got), (name, t)
            results[(name, t)] = got
            what = f"{name} t={t}"
            hold_to_references(worst, case, lists, comp_nl, rd, stretch, t, st, got, (1, 3), what, comp_mor=comp_mor)
            nl, mor, dft = got
            assert nl[0].any() and mor.any() and bool(nl[1].any()) == (comp_nl is not None)
            assert all(bool(dft[m].any()) == (comp_nl is not None) for m in (1, 3)), what
            if before is not None:  # nonlinear and drift keep their phase: their bits stay, the Morison term moves
                assert all(same_bits(p, q) for p, q in zip(nl, before[t][0])) and all(same_bits(dft[m], before[t][2][m]) for m in (1, 3))
                assert not same_bits(mor, before[t][1])
        fresh.close()
    names = [s[0] for s in si.SEQUENCE]
    for t in si.SEQ_TIMES:
        assert same_all(results[(names[8], t)], results[(names[2], t)])  # irregular nf 257 again: the bits of the first time
        for i, j in ((2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (0, 6)):  # ... and every change of model was a change of bits
            x, y = results[(names[i], t)], results[(names[j], t)]
            assert not same_bits(x[1], y[1]) and not same_bits(x[2][3], y[2][3]) and not same_bits(x[2][1], y[2][1]), (names[i], names[j], t)
    worst.report("test_tables_follow_the_wave_model")
    h.close()
    grp.close()


# ------------------------------------------------------------------------------------------------
# 5: a model change while evaluations are pending
# ------------------------------------------------------------------------------------------------
def test_end_returns_the_model_of_its_begin(HF):
    case = si.synth_case()
    lists = si.sequence_lists()
    h = HF.from_case(case)
    prepare(h, lists, phase=si.SEQ_PHASE, mor_phase=si.SEQ_PHASE)
    h.set_drift_mode(3)
    h.add_waves_irregular(**si.irreg(257))
    t = si.SEQ_TIMES[1]
    st = si.sequence_state(t)
    under_irregular = terms_alone(h, t, st)
    h.nonlinear_begin(t, st[0], st[1])
    h.morison_begin(t, *st)
    h.drift_begin(t, st[0])
    h.add_waves_regular(*si.REG1)  # accepted: the launches are enqueued on the terms' own tables
    ended = (h.nonlinear_end(), h.morison_end(), h.drift_end())
    assert same_terms(ended, under_irregular)
    fresh = HF.from_case(case)
    fresh.add_waves_regular(*si.REG1)
    prepare(fresh, lists, phase=si.SEQ_PHASE, mor_phase=si.SEQ_PHASE)
    fresh.set_drift_mode(3)
    after = terms_alone(h, t, st)
    assert same_terms(after, terms_alone(fresh, t, st))
    assert not same_bits(after[0][1], ended[0][1]) and not same_bits(after[1], ended[1]) and not same_bits(after[2], ended[2])
    h.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------
# 6: unwinding after a refused begin (host-side refusals only)
# ------------------------------------------------------------------------------------------------
def test_failed_begin_leaves_nothing_pending(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError, HydroGroup
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda x: x.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    lists = si.compose_lists()
    a, b = HF.from_case(case), HF.from_case(case)
    grp = HydroGroup.from_case(case, 3)
    for h in (a, b, grp):
        h.add_waves_irregular(**si.THREE_IRREG)
        prepare(h, lists)
        h.set_drift_mode(3)
    for h in (a, grp):
        h.set_nonlinear_mode(2)
    lib = a.lib
    motion = si.compose_motion(case)

    def pending(h):
        """(nonlinear, morison, drift) return codes of the three ends on one context: OK where an evaluation was pending"""
        out = np.empty(h.D_local)
        return lib.hc_nonlinear_end(h.ctx, None, None, None), lib.hc_morison_end(h.ctx, dp(out)), lib.hc_drift_end(h.ctx, dp(out))

    def expected(t, st):
        total = raw_step(b, t, st)
        nl, mor, dft = terms_alone(b, t, st)
        return si.compose(total, nl, mor, dft, 2, PANELLED)

    t0, t1, t2 = (float(t) for t in si.SUBSET_TIMES[:3])
    # (i) a drift evaluation begun by hand: the third begin of step() is refused, the first two are unwound
    st = motion.state(t0)
    a.drift_begin(t0, st[0])
    with pytest.raises(HydroError):
        a.step(t0, *st)
    assert pending(a) == (INV, INV, OK)
    want = expected(t0, st)
    assert same_bits(a.step(t0, *st), want) and same_bits(grp.step(t0, *st), want)
    assert pending(a) == (INV, INV, INV)
    # (ii) a Morison evaluation begun by hand: refused at the second begin, the nonlinear one is unwound, the drift one never begun
    st = motion.state(t1)
    a.morison_begin(t1, *st)
    with pytest.raises(HydroError):
        a.step(t1, *st)
    assert pending(a) == (INV, OK, INV)
    want = expected(t1, st)
    assert same_bits(a.step(t1, *st), want) and same_bits(grp.step(t1, *st), want)
    # (iii) three shards, a drift evaluation pending on shard 1 only: what shard 0 (and every shard, for the other terms) had begun is unwound
    st = motion.state(t2)
    grp.shards[1].drift_begin(t2, st[0])
    with pytest.raises(HydroError):
        grp.step(t2, *st)
    assert [pending(s) for s in grp.shards] == [(INV, INV, INV), (INV, INV, OK), (INV, INV, INV)]
    want = expected(t2, st)
    assert same_bits(grp.step(t2, *st), want) and same_bits(a.step(t2, *st), want)
    assert [pending(s) for s in grp.shards] == [(INV, INV, INV)] * 3
    for h in (a, b, grp):
        h.close()


# ------------------------------------------------------------------------------------------------
# 7: the C++ mirror, several bodies and shards
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_all_terms_on_shards(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "side_terms_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "side_terms_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "four_body.h5")
    outputs = []
    for devices in ("0", "0,0", "0,0,0,0"):
        r = subprocess.run([exe, h5, devices], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (devices, r.returncode, r.stderr)
        outputs.append(r.stdout)
    assert outputs[0] and outputs[1] == outputs[0] and outputs[2] == outputs[0]  # identical text whatever the device list
    rows = np.array([[float(v) for v in line.split()] for line in outputs[0].strip().splitlines()])
    assert rows.shape == (si.CPP_STEPS, 1 + 48 + 24 + 24 + 72 + 24)
    lists = si.cpp_lists()
    h = HF(4)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_irregular(num_bodies=4, **si.THREE_IRREG)
    for b in range(4):
        if lists["panels"][b] is not None:
            h.set_surface_panels(b, *lists["panels"][b])
        if lists["elements"][b] is not None:
            h.set_morison_elements(b, *lists["elements"][b])
        if lists["tables"][b] is not None:
            h.set_drift_qtf(b, *lists["tables"][b])
    h.set_nonlinear_options(**si.CPP_NL_OPTS)
    h.set_morison_options(**si.CPP_MOR_OPTS)
    h.set_drift_mode(3)
    for n, row in enumerate(rows):
        if n == si.CPP_SWITCH:
            h.set_drift_mode(2)
        t, st = si.cpp_state(n)
        assert row[0] == t and same_bits(row[1:49].reshape(4, 4, 3), np.stack(st, axis=1)), n  # the state the caller printed
        total = raw_step(h, t, st)
        nl, mor, dft = terms_alone(h, t, st)
        assert same_bits(row[73:97], mor) and same_bits(row[97:169], np.concatenate(nl)) and same_bits(row[169:193], dft), n
        assert same_bits(row[49:73], si.compose(total, nl, mor, dft, 2, si.CPP_PANEL_BODIES)), n
        m6, b6, d6 = mor.reshape(4, 6), nl[0].reshape(4, 6), dft.reshape(4, 6)
        assert [bool(x.any()) for x in b6] == [True, False, True, False] and [bool(x.any()) for x in m6] == [False, True, True, False]
        assert [bool(x.any()) for x in d6] == [True, False, False, True]
    assert not np.allclose(rows[si.CPP_SWITCH - 1, 169:175], rows[si.CPP_SWITCH, 169:175], rtol=1e-6)  # the mode did switch
    h.close()
