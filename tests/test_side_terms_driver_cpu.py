"""The driver that composes the side terms with the step (hydrochrono_amd/hydro.py: _SIDE_TERMS, _step_with_side_terms), on the CPU: a
stub library records every begin, step and end and answers with scripted status codes; contexts are plain integers.  For each of
the 32 subsets of enabled terms, on 1 and on 3 contexts, a failure is injected at every begin on every context, at the step and at
every end on every context, and the whole call sequence is asserted: begins in table order up to the one that fails, ends of exactly
the (term, context) pairs that were begun, no step after a refused begin, every end after a failed step.  On success the composition
is held, bit for bit, to the written-out sequence ((((nonlinear) + morison) + drift) + sum) - radm on values where the order of the
FP64 operations matters."""
import itertools
import types

import numpy as np

from hydrochrono_amd import hydro
from hydrochrono_amd.hydro import HydroError

TERMS = hydro._SIDE_TERMS
N, D = 3, 18
LAYOUTS = {1: [(7, 0, 18)], 3: [(11, 0, 6), (12, 6, 6), (13, 12, 6)]}  # contexts (ctx, first row, rows) of one system
SUBSETS = list(itertools.product((False, True), repeat=len(TERMS)))
PANELS = {0: 4, 1: 0, 2: 9}  # bodies 0 and 2 carry a surface list
BIG = 1e16
# per term and output, D values: sizes 1e16, 1, -1e16, 3 in turn, so that every addition rounds and no two orders agree
VALUES = {"total": BIG * (1.0 + np.arange(D) % 3),
          "nonlinear": (1.0 + np.arange(D), -BIG * (1.0 + np.arange(D) % 2), 3.0 + 2.0 * np.arange(D)),  # buoy, fk, hs_lin
          "morison": (1.0 + 2.0 * np.arange(D),), "drift": (-BIG * (1.0 + np.arange(D) % 3),), "sum": (3.0 + np.arange(D),),
          "radm": (5.0 - 4.0 * np.arange(D),)}
STATE = [np.full(3 * N, float(s)) for s in range(4)]  # a[slot] holds its slot number


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


class StubLib:
    """hc_<term>_begin / _end and hc_last_error of the C ABI as the driver calls them.  fail: {("begin" | "end", term, ctx): status}."""

    def __init__(self, layout, fail=()):
        self.rows = {ctx: (row, n) for ctx, row, n in layout}
        self.fail = dict(fail)
        self.calls = []
        self.last_error = {}
        for term in TERMS:
            setattr(self, term.begin, self._begin(term))
            setattr(self, term.end, self._end(term))

    def _answer(self, kind, term, ctx):
        self.calls.append((kind, term.name, ctx))
        rc = self.fail.get((kind, term.name, ctx), 0)
        if rc:
            self.last_error[ctx] = f"{kind} {term.name} {ctx}".encode()
        return rc

    def _begin(self, term):
        def begin(ctx, t, *ptrs):
            assert type(t) is float and tuple(int(p[0]) for p in ptrs) == term.slots  # the arrays of the row's slots, in order
            return self._answer("begin", term, ctx)
        return begin

    def _end(self, term):
        def end(ctx, *ptrs):
            assert len(ptrs) == term.nout
            row, n = self.rows[ctx]
            for p, v in zip(ptrs, VALUES[term.name]):
                for i in range(n):
                    p[i] = v[row + i]
            return self._answer("end", term, ctx)
        return end

    def hc_last_error(self, ctx):
        return self.last_error.get(ctx, b"")


def run(layout, on, fail=(), step_rc=0):
    """One pass of the driver: (owner, stub, the returned total or the HydroError raised)"""
    lib = StubLib(layout, fail)
    owner = types.SimpleNamespace(lib=lib, _nonlinear_mode=2, _panel_counts=PANELS, **{term.last: term.name for term in TERMS})
    out = np.empty(D)

    def step():
        lib.calls.append(("step",))
        out[:] = VALUES["total"]
        if step_rc:
            lib.last_error[layout[0][0]] = b"the step"
        return step_rc
    try:
        got = hydro._step_with_side_terms(owner, owner, layout, on, step, 2.5, STATE, out, 0, N)
    except HydroError as e:
        got = e
    return owner, lib, got


def enabled(on):
    return [term for term, flag in zip(TERMS, on) if flag]


def all_of(kind, terms, layout):
    return [(kind, term.name, ctx) for term in terms for ctx, _, _ in layout]


def untouched(owner):
    return all(getattr(owner, term.last) == term.name for term in TERMS)


def test_the_table_is_the_five_terms_in_todays_order():
    assert [(t.name, t.slots, t.nout, t.last) for t in TERMS] == [
        ("nonlinear", (0, 1), 3, "_nonlinear_last"), ("morison", (0, 1, 2, 3), 1, "_morison_last"), ("drift", (0,), 1, "_drift_last"),
        ("sum", (0,), 1, "_sum_last"), ("radm", (2, 3), 1, "_radm_last")]
    assert [(t.begin, t.end) for t in TERMS] == [
        ("hc_nonlinear_begin", "hc_nonlinear_end"), ("hc_morison_begin", "hc_morison_end"), ("hc_drift_begin", "hc_drift_end"),
        ("hc_sum_qtf_begin", "hc_sum_qtf_end"), ("hc_radiation_modes_begin", "hc_radiation_modes_end")]
    h = types.SimpleNamespace(_nonlinear_on=lambda: "nl", _morison_any="mor", _drift_on=lambda: "dr", _sum_on=lambda: "sm", _radm_any="rm")
    assert [t.on(h) for t in TERMS] == ["nl", "mor", "dr", "sm", "rm"]  # the predicates of HydroForces, as it evaluates them
    assert [t.on(types.SimpleNamespace(_nonlinear_on=lambda: False, _drift_on=lambda: False, _sum_on=lambda: False)) for t in TERMS] == [
        False, None, False, False, None]  # the two flags are looked up the way step() does: absent is off


def test_success_calls_and_composition():
    total = VALUES["total"]
    (buoy, fk, hs), (mor,), (dr,), (sm,), (rm,) = (VALUES[t.name] for t in TERMS)
    nl = total.copy()
    for b, n in PANELS.items():
        if n:
            r = slice(6 * b, 6 * b + 6)
            nl[r] = total[r] - hs[r] + buoy[r]
            nl[r] = nl[r] + fk[r]
    assert not same_bits(((((nl) + mor) + dr) + sm) - rm, nl + (mor + dr + sm - rm))  # on these values the order matters
    assert not same_bits(((((nl) + mor) + dr) + sm) - rm, ((((nl) + dr) + mor) + sm) - rm)
    for G, layout in LAYOUTS.items():
        for on in SUBSETS:
            owner, lib, got = run(layout, on)
            terms = enabled(on)
            assert lib.calls == all_of("begin", terms, layout) + [("step",)] + all_of("end", terms, layout), (G, on)
            want = nl if on[0] else total
            if on[1]:
                want = want + mor
            if on[2]:
                want = want + dr
            if on[3]:
                want = want + sm
            if on[4]:
                want = want - rm
            assert same_bits(got, want), (G, on)
            for term, flag in zip(TERMS, on):
                last = getattr(owner, term.last)
                if not flag:
                    assert last == term.name
                elif term.nout > 1:
                    assert all(same_bits(x, v) for x, v in zip(last, VALUES[term.name])), (G, on, term.name)
                else:
                    assert same_bits(last, VALUES[term.name][0]), (G, on, term.name)  # every context's rows in their place


def test_a_refused_begin_ends_what_was_begun_and_nothing_else():
    for G, layout in LAYOUTS.items():
        for on in SUBSETS:
            terms = enabled(on)
            for k, term in enumerate(terms):
                for g, (ctx, _, _) in enumerate(layout):
                    owner, lib, got = run(layout, on, {("begin", term.name, ctx): 40 + g})
                    want = (all_of("begin", terms[:k], layout) + all_of("begin", [term], layout[:g + 1])  # up to the refused one
                            + all_of("end", [term], layout[:g])       # the term itself on the contexts before
                            + all_of("end", terms[:k], layout))       # then the terms before, in table order; no step
                    assert lib.calls == want, (G, on, term.name, g)
                    begun = {c[1:] for c in lib.calls if c[0] == "begin"} - {(term.name, ctx)}
                    assert {c[1:] for c in lib.calls if c[0] == "end"} == begun
                    assert isinstance(got, HydroError) and got.status == 40 + g and f"begin {term.name} {ctx}" in str(got)
                    assert untouched(owner), (G, on, term.name, g)


def test_a_failed_step_is_followed_by_every_end_and_is_what_is_raised():
    for G, layout in LAYOUTS.items():
        for on in SUBSETS:
            terms = enabled(on)
            fails = [{}] + [{("end", term.name, layout[-1][0]): 9} for term in terms]  # alone, and with an end that fails as well
            for fail in fails:
                owner, lib, got = run(layout, on, fail, step_rc=2)
                assert lib.calls == all_of("begin", terms, layout) + [("step",)] + all_of("end", terms, layout), (G, on, fail)
                assert isinstance(got, HydroError) and got.status == 2 and "the step" in str(got)
                assert untouched(owner), (G, on)


def test_a_failed_end_is_followed_by_every_other_end_and_the_first_is_raised():
    for G, layout in LAYOUTS.items():
        for on in SUBSETS:
            terms = enabled(on)
            pairs = [(term, ctx) for term in terms for ctx, _, _ in layout]  # in table order, then context order
            for i, (term, ctx) in enumerate(pairs):
                # this end alone, and together with every later one: the first in table order, then context order, is reported
                for fail in ({("end", term.name, ctx): 50 + i}, {("end", p.name, c): 50 + j for j, (p, c) in enumerate(pairs) if j >= i}):
                    owner, lib, got = run(layout, on, fail)
                    assert lib.calls == all_of("begin", terms, layout) + [("step",)] + all_of("end", terms, layout), (G, on, fail)
                    assert isinstance(got, HydroError) and got.status == 50 + i and f"end {term.name} {ctx}" in str(got)
                    assert untouched(owner), (G, on, term.name, ctx)
