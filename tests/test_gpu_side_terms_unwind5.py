"""All FIVE side terms on -- nonlinear, Morison, drift, sum-frequency, modal radiation -- and a begin of step() refused at the two
depths that tests/test_gpu_side_terms.py (three terms: depths 2 and 3) and tests/test_gpu_side_terms2.py (four terms: depths 3 and 4)
do not reach: the fifth begin, with four terms to unwind, and the fourth begin with a fifth term that is never begun.  On one
context and on a group of three shards with the evaluation begun by hand on shard 1 only.  After the refusal nothing but the
evaluation begun by hand is pending, and the next step() is, bit for bit, the raw hc_step composed with the five terms computed alone
on a twin context.

The inputs are those of tests/side_terms2_inputs.py (the small lists) in an irregular sea of 32 components; one radiation mode on
body 1, the body shard 1 owns, so that the modal state of the twin sees the times the shard saw."""
import numpy as np
import pytest

import side_terms2_inputs as s2
import side_terms_inputs as si
from cases import three_body_case
from side_terms_inputs import same_bits

pytestmark = pytest.mark.gpu
SURFACED = (0, 2)
WAVES = dict(si.THREE_IRREG, nfrequencies=32)
MODE = (2, 8, -0.8 + 1.7j, 1.3e3 - 0.4e3j)  # heave of body 1 on its own heave velocity


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


def all_five_on(h, lists):
    s2.set_lists(h, lists)
    h.set_nonlinear_options(**s2.NL_OPTS)
    h.set_morison_options(**s2.MOR_OPTS)
    h.set_nonlinear_second_order(True)
    h.set_morison_second_order(True)
    h.set_radiation_modes(1, [MODE])
    h.set_nonlinear_mode(2)
    h.set_drift_mode(3)
    h.set_sum_mode(1)


@pytest.mark.parametrize("by_hand", ["radm", "sum"])
def test_refused_fourth_and_fifth_begin_leave_nothing_pending(HF, by_hand):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError, HydroGroup
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda x: x.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    lists = s2.compose_lists(small=True)
    a, b = HF.from_case(case), HF.from_case(case)
    grp = HydroGroup.from_case(case, 3)
    for h in (a, b, grp):
        h.add_waves_irregular(**WAVES)
        all_five_on(h, lists)
    lib = a.lib
    motion = s2.compose_motion()

    def pending(h):
        """(nonlinear, morison, drift, sum, radm) return codes of the five ends on one context: OK where an evaluation was pending"""
        out = np.empty(h.D_local)
        return (lib.hc_nonlinear_end(h.ctx, None, None, None), lib.hc_morison_end(h.ctx, dp(out)), lib.hc_drift_end(h.ctx, dp(out)),
                lib.hc_sum_qtf_end(h.ctx, dp(out)), lib.hc_radiation_modes_end(h.ctx, dp(out)))

    def expected(t, st, radm_moves):
        total = raw_step(b, t, st)
        nl, mor, dft, smf = b.compute_nonlinear(t, st[0], st[1]), b.compute_morison(t, *st), b.compute_drift(t, st[0]), b.compute_sum_qtf(t, st[0])
        rad = b.compute_radiation_modes(t, st[2], st[3])
        assert nl[1].any() and mor.any() and dft.any() and smf.any() and rad.any() == radm_moves
        return s2.compose4(total, nl, mor, dft, smf, 2, SURFACED) - rad

    def begin_by_hand(h, t, st):
        (h.radiation_modes_begin(t, st[2], st[3]) if by_hand == "radm" else h.sum_qtf_begin(t, st[0]))

    none = (INV,) * 5
    only = (INV, INV, INV, INV, OK) if by_hand == "radm" else (INV, INV, INV, OK, INV)
    tw, t0, t1 = (float(t) for t in s2.SUBSET_TIMES[:3])
    # a first step everywhere: the modal state starts (its first value is zero), the twin in step
    st = motion.state(tw)
    want = expected(tw, st, False)
    assert same_bits(a.step(tw, *st), want) and same_bits(grp.step(tw, *st), want)
    # the evaluation begun by hand, on the context and on shard 1 only: that begin of step() is refused, the terms before it are unwound
    # -- on every shard, and the refused term itself on shard 0 --, a term after it is never begun
    st = motion.state(t0)
    begin_by_hand(a, t0, st)
    begin_by_hand(grp.shards[1], t0, st)
    for h in (a, grp):
        with pytest.raises(HydroError):
            h.step(t0, *st)
    assert pending(a) == only
    assert [pending(s) for s in grp.shards] == [none, only, none]
    if by_hand == "radm":  # the modal state of the context and of shard 1 has seen t0: the twin's sees it as well
        b.compute_radiation_modes(t0, st[2], st[3])
    # the next step is a whole one
    st = motion.state(t1)
    want = expected(t1, st, True)
    assert same_bits(a.step(t1, *st), want) and same_bits(grp.step(t1, *st), want)
    assert same_bits(a.radiation_modes(), grp.radiation_modes()) and a.radiation_modes().any()
    assert pending(a) == none and [pending(s) for s in grp.shards] == [none] * 3
    for h in (a, b, grp):
        h.close()
