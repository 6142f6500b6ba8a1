"""Spectral radiation tail (hc_set_radiation_tail): at C3 size, with the step equal to the IRF spacing, the lags from 256
on of every at-start look-ahead block come from a partitioned FFT convolution made once per superblock of 256 steps.  Against the
full pass (mode 0) and the flat-array CPU oracle over more than three superblocks; row shards bitwise equal to the unsharded context;
a step back in time across a superblock boundary and hc_set_history in the middle of one; and the cases that keep the full pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cases import load_into_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-10
MODE_TOL = 1e-12


@pytest.fixture(scope="module")
def hydro():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hydrochrono_amd.hydro as hydro
    return hydro


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


def c3_case():
    import bench as B
    from hydrochrono_amd.synthetic import many_body_case
    return B, many_body_case(64, S=B.S_RIRF, dt_rirf=B.DT, n_exc=B.N_EXC, dt_exc=B.DT, seed=20251031)


def setup(h, B, motion, dt=None):
    dt = dt or B.DT
    h.add_waves_irregular(num_bodies=64, **dict(B.WAVES, simulation_dt=dt, simulation_duration=B.T0 + 12.0))
    h.set_pass_schedule(0)
    nhist = int(np.ceil(B.S_RIRF * B.DT / dt)) + 5
    t_hist = B.T0 - dt * np.arange(1, nhist + 1)
    v_hist = np.stack([motion.velocity6(t) for t in t_hist])
    h.set_history(t_hist, v_hist)
    return t_hist, v_hist


def test_tail_against_full_pass_and_oracle(hydro):
    import oracle as orc_mod
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    B, case = c3_case()
    motion = PrescribedMotion(64, rest_positions(case), seed=20251031)
    tail, full = hydro.HydroForces.from_case(case), hydro.HydroForces.from_case(case)
    full.set_radiation_tail(0)
    t_hist, v_hist = setup(tail, B, motion)
    setup(full, B, motion)
    orc_mod.set_num_threads(min(64, os.cpu_count() or 1))
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**dict(B.WAVES, simulation_dt=B.DT, simulation_duration=B.T0 + 12.0))
    orc.prefill_history(t_hist, v_hist)
    orc.flat_prepare()
    tail.enable_profiling(1)
    full.enable_profiling(1)
    worst_mode = worst_orc = 0.0
    for n in range(3 * 256 + 40):
        t = B.T0 + n * B.DT
        st = motion.state(t)
        ft, ff, fo = tail.step(t, *st), full.step(t, *st), orc.flat_step(t, *st)
        worst_mode = max(worst_mode, relerr(ft, ff))
        worst_orc = max(worst_orc, relerr(ft, fo), relerr(ff, fo))
        assert worst_mode <= MODE_TOL and worst_orc <= ORACLE_TOL, f"step {n}: mode {worst_mode:.2e}, oracle {worst_orc:.2e}"
    p, q = tail.profile(), full.profile()
    assert p["tail_blocks"] >= 3 * 8 and p["tail_launches"] > 0 and p["tail_bytes"] > 0, p
    assert q["tail_launches"] == 0 and q["tail_blocks"] == 0, q
    assert p["block_kernel_launches"] == q["block_kernel_launches"]  # the head pass replaces the pass one for one
    print(f"spectral tail: mode 1 vs 0 {worst_mode:.2e}, vs oracle {worst_orc:.2e}, {p['tail_blocks']} blocks, {p['tail_launches']} launches")


def test_tail_row_shards_bitwise(hydro):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    B, case = c3_case()
    motion = PrescribedMotion(64, rest_positions(case), seed=7)
    full = hydro.HydroForces.from_case(case)
    group = hydro.HydroGroup.from_case(case, 2)
    setup(full, B, motion)
    setup(group, B, motion)
    full.enable_profiling(1)
    for n in range(2 * 256 + 20):
        t = B.T0 + n * B.DT
        st = motion.state(t)
        a, b = full.step(t, *st), group.step(t, *st)
        assert np.array_equal(a, b), f"step {n}: {relerr(b, a):.2e}"
    assert full.profile()["tail_blocks"] >= 16


def test_tail_rewind_and_set_history(hydro):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    B, case = c3_case()
    motion = PrescribedMotion(64, rest_positions(case), seed=11)
    tail, full = hydro.HydroForces.from_case(case), hydro.HydroForces.from_case(case)
    full.set_radiation_tail(0)
    setup(tail, B, motion)
    setup(full, B, motion)
    tail.enable_profiling(1)
    worst = 0.0
    # forward past the first superblock boundary, back across it (an integrator retrying from an earlier time), forward again
    schedule = list(range(0, 300)) + list(range(240, 560))
    for k, n in enumerate(schedule):
        if k == 430:  # in the middle of a superblock: a fresh history on the same grid
            t_h = B.T0 + n * B.DT - B.DT * np.arange(1, B.S_RIRF + 6)
            v_h = np.stack([motion.velocity6(t) * 0.9 for t in t_h])
            tail.set_history(t_h, v_h)
            full.set_history(t_h, v_h)
        t = B.T0 + n * B.DT
        st = motion.state(t)
        worst = max(worst, relerr(tail.step(t, *st), full.step(t, *st)))
        assert worst <= MODE_TOL, f"call {k} (step {n}): {worst:.2e}"
    p = tail.profile()
    assert p["tail_blocks"] >= 10 and p["history_rewinds"] >= 1, p


@pytest.mark.parametrize("variant", ["step_dt", "ahead"])
def test_tail_not_used_where_ineligible(hydro, variant):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    B, case = c3_case()
    motion = PrescribedMotion(64, rest_positions(case), seed=3)
    h = hydro.HydroForces.from_case(case)
    dt = 0.007 if variant == "step_dt" else B.DT
    setup(h, B, motion, dt)
    if variant == "ahead":
        h.set_pass_schedule(1)
    h.enable_profiling(1)
    for n in range(300):
        t = B.T0 + n * dt
        h.step(t, *motion.state(t))
    p = h.profile()
    assert p["tail_launches"] == 0 and p["tail_blocks"] == 0 and p["block_kernel_launches"] > 0, p
