"""The begin / end protocol the four terms beside the step share (csrc/hc_side.hpp: Morison elements, the nonlinear surface pressure,
the drift and the sum-frequency QTF forces): the same sequence of statuses for each of them, on the smallest input each accepts --
two bodies under a regular wave, one Morison element, one surface panel, a drift and a sum table with nq = 2; and once more for the
Morison lane opened by one strip member alone.  The terms share one
context.  The Morison, nonlinear, drift and sum lanes are each their own; the two Morison cases (and the Morison case of
test_increments_follow_the_completed_evaluation) share the Morison lane and clean up after themselves -- "morison" sets its own
element at its start, "morison members" clears that element first and its member when it leaves -- so the order of the cases does
not matter."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2
Z, OUT = np.zeros(3 * N), np.empty(6 * N)
POS = np.array([0.0, 0.0, 0.0, 30.0, 0.0, 0.0])
LIN = np.tile([0.5, 0.0, 0.0], N)
GRID, TABLE = np.array([0.4, 1.2]), np.full(6 * 2 * 2, 100.0)  # the wave's 0.8 rad/s lies inside
BETA, TABLE_H = np.array([0.0]), np.full(6 * 2 * 2, 100.0)


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.synthetic import many_body_case
    h = HydroForces.from_case(many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7))
    h.add_waves_regular(0.5, 0.8)
    yield h
    h.close()


def dp(a):
    from hydrochrono_amd import capi
    return None if a is None else a.ctypes.data_as(capi.c_double_p)


def element():
    from hydrochrono_amd import capi
    e = (capi.MorisonElement * 1)()
    e[0].r[:], e[0].cd_area[:], e[0].cm_vol[:] = (0, 0, -1.0), (1, 1, 1.0), (0, 0, 0.0)
    return e


def member():
    from hydrochrono_amd import capi
    m = (capi.MorisonMember * 1)()
    m[0].r0[:], m[0].r1[:] = (0, 0, -3.0), (0, 0, 2.0)
    m[0].d0, m[0].d1, m[0].cd, m[0].cm, m[0].n_seg = 1.0, 1.0, 1.0, 0.0, 2
    return m


def panel():
    from hydrochrono_amd import capi
    p = (capi.SurfacePanel * 1)()
    p[0].c[:], p[0].s[:] = (0, 0, -1.0), (0, 0, -1.0)
    return p


class Term:
    """What the sequence needs of a term: begin, end into `outs`, its setters and options calls, and how its input is taken away
    and put back."""

    def __init__(self, lib, c, name):
        self.name, self.null_end = name, name != "nonlinear"
        self.leave = lambda: None
        if name == "morison members":  # the Morison lane opened by hc_set_morison_members alone: it never has an element
            assert lib.hc_set_morison_elements(c, 0, None, 0) == 0
            self.outs = [OUT.copy()]
            self.begin = lambda: lib.hc_morison_begin(c, 0.0, dp(POS), dp(Z), dp(LIN), dp(Z))
            self.end = lambda outs: lib.hc_morison_end(c, *outs)
            self.fill = lambda: lib.hc_set_morison_members(c, 0, member(), 1)
            self.clear = lambda: lib.hc_set_morison_members(c, 0, None, 0)
            self.setters = [self.fill, lambda: lib.hc_set_morison_options(c, None),
                            lambda: lib.hc_set_morison_second_order(c, 0, 0.0, np.inf, 0.0, np.inf, 1)]
            self.leave = self.clear  # (the other Morison cases of this module's one context switch the second-order sea on)
        elif name == "morison":
            self.outs = [OUT.copy()]
            self.begin = lambda: lib.hc_morison_begin(c, 0.0, dp(POS), dp(Z), dp(LIN), dp(Z))
            self.end = lambda outs: lib.hc_morison_end(c, *outs)
            self.fill = lambda: lib.hc_set_morison_elements(c, 0, element(), 1)
            self.clear = lambda: lib.hc_set_morison_elements(c, 0, None, 0)
            self.setters = [self.fill, lambda: lib.hc_set_morison_options(c, None),
                            lambda: lib.hc_set_morison_second_order(c, 0, 0.0, np.inf, 0.0, np.inf, 1)]
        elif name == "nonlinear":
            self.outs = [OUT.copy(), OUT.copy(), OUT.copy()]
            self.begin = lambda: lib.hc_nonlinear_begin(c, 0.0, dp(POS), dp(Z))
            self.end = lambda outs: lib.hc_nonlinear_end(c, *outs)
            self.fill = lambda: lib.hc_set_surface_panels(c, 0, panel(), 1)
            self.clear = lambda: lib.hc_set_surface_panels(c, 0, None, 0)
            self.setters = [self.fill, lambda: lib.hc_set_surface_triangles(c, 1, dp(np.arange(9.0)), 1),
                            lambda: lib.hc_set_nonlinear_options(c, None),
                            lambda: lib.hc_set_nonlinear_second_order(c, 0, 0.0, np.inf, 0.0, np.inf, 1)]
        else:
            term, kind, mode = ("drift", "drift", 3) if name == "drift" else ("sum_qtf", "sum", 1)
            f = lambda what: getattr(lib, what)  # noqa: E731
            self.outs = [OUT.copy()]
            self.begin = lambda: f(f"hc_{term}_begin")(c, 0.0, dp(POS))
            self.end = lambda outs: f(f"hc_{term}_end")(c, *outs)
            self.fill = lambda: f(f"hc_set_{kind}_qtf")(c, 0, 2, dp(GRID), dp(TABLE), None) or f(f"hc_set_{kind}_mode")(c, mode)
            self.clear = lambda: f(f"hc_set_{kind}_mode")(c, 0)
            self.setters = [lambda: f(f"hc_set_{kind}_qtf")(c, 0, 2, dp(GRID), dp(TABLE), None),
                            lambda: f(f"hc_set_{kind}_qtf_headings")(c, 1, 1, dp(BETA), 2, dp(GRID), dp(TABLE_H), None),
                            lambda: f(f"hc_set_{kind}_mode")(c, mode), lambda: f(f"hc_set_{kind}_options")(c, None)]

    def forces(self):  # (hs_lin of the nonlinear term is the linear hydrostatic force, not a launched result)
        return self.outs[:2] if self.name == "nonlinear" else self.outs

    def end_into_outs(self):
        for o in self.outs:
            o[:] = 7.0
        return self.end([dp(o) for o in self.outs])


@pytest.mark.parametrize("name", ["morison", "nonlinear", "drift", "sum", "morison members"])
def test_begin_end_protocol(ctx, name):
    term = Term(ctx.lib, ctx.ctx, name)
    try:
        begin_end_protocol(term, name)
    finally:
        term.leave()


def begin_end_protocol(term, name):
    from hydrochrono_amd import capi
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    assert term.fill() == OK
    # begin twice; no setter and no options call while one is pending; exactly one end per begin
    assert term.begin() == OK
    assert term.begin() == INV
    for k, setter in enumerate(term.setters):
        assert setter() == INV, (name, k)
    assert term.end_into_outs() == OK
    assert all(np.all(np.isfinite(o)) for o in term.outs) and any(o.any() for o in term.forces())
    assert term.end_into_outs() == INV
    # nothing to launch: the begin still needs its end, and yields zeros
    assert term.clear() == OK
    assert term.begin() == OK
    assert term.begin() == INV
    assert term.setters[0]() == INV
    assert term.end_into_outs() == OK
    assert not any(o.any() for o in term.forces())
    assert term.end_into_outs() == INV
    assert term.fill() == OK
    # a null output ends the evaluation all the same: the lane is idle and a fresh begin succeeds
    if term.null_end:
        assert term.begin() == OK
        assert term.end([None]) == INV
        assert term.end_into_outs() == INV
        assert term.begin() == OK
        assert term.end_into_outs() == OK and any(o.any() for o in term.forces())


@pytest.mark.parametrize("name", ["morison", "nonlinear"])
def test_increments_follow_the_completed_evaluation(ctx, name):
    from hydrochrono_amd import capi
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    lib, c = ctx.lib, ctx.ctx
    term = Term(lib, c, name)
    eta2 = np.full(1, 7.0)
    if name == "morison":
        switch = lambda on: lib.hc_set_morison_second_order(c, on, 0.0, np.inf, 0.0, np.inf, 1)  # noqa: E731
        get = lambda: lib.hc_get_morison_increments(c, 0, None, dp(eta2), None, None)  # noqa: E731
    else:
        switch = lambda on: lib.hc_set_nonlinear_second_order(c, on, 0.0, np.inf, 0.0, np.inf, 1)  # noqa: E731
        get = lambda: lib.hc_get_nonlinear_increments(c, 0, 1, None, dp(eta2), None)  # noqa: E731
    assert term.fill() == OK and switch(1) == OK
    try:
        assert get() == INV  # no evaluation has completed
        assert term.begin() == OK
        assert get() == INV  # ... nor has this one yet
        assert term.end_into_outs() == OK
        assert get() == OK and np.isfinite(eta2[0]) and eta2[0] != 7.0
        assert term.fill() == OK  # the lists set anew: the increments are no longer those of the lists
        assert get() == INV
        assert term.begin() == OK and term.end_into_outs() == OK and get() == OK
    finally:
        assert switch(0) == OK
    assert get() == INV
