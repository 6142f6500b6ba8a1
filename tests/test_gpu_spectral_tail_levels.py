"""The LEVELS of the spectral radiation tail (hc_set_radiation_tail 1: lags 128 .. 255 once per 128 steps, 256 .. 511
once per 256 steps, from 512 on once per 512 steps where the IRF has 1024 samples or more) on small systems, so that the index
arithmetic and not the size is tested: against the full pass (mode 0), the uniform form (mode 2) and the flat oracle around every
threshold of S; single impulses whose lag crosses every level boundary, held to the exact lag sum (a lag routed to two levels or to
none shows as a whole term); steps back in time across a 128-, 256- and 512-period boundary, hc_set_history in the middle of each, a
change of form and a change of K mid-period; row shards at odd row counts and the two dispatch paths bitwise; and the shapes that
keep the full pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tail_ref as TR  # noqa: E402
import test_gpu_spectral_tail_edges as E  # noqa: E402  (Run, make, configure, relerr: the drivers of the edge tests)
from cases import load_into_oracle  # noqa: E402
from test_gpu_spectral_tail import MODE_TOL, ORACLE_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

T0 = E.T0
PTOP = 512  # the longest period


@pytest.fixture(scope="module")
def hydro():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hydrochrono_amd.hydro as hydro
    return hydro


def top_period(S):
    return 512 if S >= 1024 else 256


# ---- a. against the full pass, the uniform form and the oracle --------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 32])
@pytest.mark.parametrize("S", [512, 700, 1024, 1030])
@pytest.mark.parametrize("N", [1, 3])
def test_levels_against_full_pass_uniform_form_and_oracle(hydro, N, S, L):
    case = TR.flat_case(N, S, seed=7000 + 10 * S + N)
    ctxs = [E.make(hydro, case, L, tail=mode) for mode in (1, 2, 0)]
    run = E.Run(case, S, seed=S + N + L)
    orc = load_into_oracle(case)
    orc.add_waves_none()
    orc.prefill_history(*run.history())
    orc.flat_prepare()
    for h in ctxs:
        h.set_history(*run.history())
        h.enable_profiling(1)  # (block_kernel_launches counts timed launches)
    worst_mode = worst_orc = 0.0
    for n in range(2 * PTOP + 40):
        out = run.step(ctxs, n)
        w = run.v[-1].reshape(N, 6)
        fo = orc.flat_step(run.time(n), run.pos, run.rpy, w[:, :3].reshape(-1).copy(), w[:, 3:].reshape(-1).copy())
        f1, f2, f0 = out[0][0], out[1][0], out[2][0]
        worst_mode = max(worst_mode, E.relerr(f1, f0), E.relerr(f2, f0), E.relerr(f1, f2))
        worst_orc = max(worst_orc, E.relerr(f1, fo), E.relerr(f2, fo), E.relerr(f0, fo))
        assert worst_mode <= MODE_TOL and worst_orc <= ORACLE_TOL, f"step {n}: between modes {worst_mode:.2e}, against the oracle {worst_orc:.2e}"
    p1, p2, p0 = (h.profile() for h in ctxs)
    assert p1["tail_blocks"] == p2["tail_blocks"] >= (2 * PTOP) // L and p0["tail_blocks"] == 0, (p1["tail_blocks"], p2["tail_blocks"], p0["tail_blocks"])
    assert p1["block_kernel_launches"] == p2["block_kernel_launches"] == p0["block_kernel_launches"] > 0  # the head pass replaces the pass one for one
    assert p1["tail_launches"] > 0 and p2["tail_launches"] > 0 and p0["tail_launches"] == 0
    print(f"N {N} S {S} L {L}: between modes {worst_mode:.2e}, against the oracle {worst_orc:.2e}; tail launches levelled {p1['tail_launches']}, "
          f"uniform {p2['tail_launches']}; tail bytes levelled / uniform {p1['tail_bytes'] / p2['tail_bytes']:.3f}")


# ---- b. impulse routing ----------------------------------------------------------------------------------------------------------
def level_partitions(S):
    """[(lag_lo, lag_hi)] of the head and of every partition of every level: the lags one transform mixes."""
    parts = [(0, 128), (128, 256)]
    if S >= 1024:
        parts += [(256, 512)] + [(lo, min(S, lo + 512)) for lo in range(512, S, 512)]
    else:
        parts += [(lo, min(S, lo + 256)) for lo in range(256, S, 256)]
    return parts


@pytest.mark.parametrize("S,L", [(1030, 32), (1024, 16), (700, 32)])
def test_levels_impulse_routing(hydro, S, L):
    """One body, an i.i.d. K (a distinct value per lag), zero velocities but for ONE unit sample in the history, at 40 offsets; at
    every step of one top period (two where far partitions are made a period ahead, so that both sources of them are met) the
    radiation is that sample's one term w_s G[:, c, s], or nothing once it is older than the window.  The bound is the row-wise one
    of tests/tail_ref.py with the transform's rounding referred to the largest term of the partition the lag lies in, as
    test_tail_impulse_sweep derives it: 1e-12 max |w G| over that partition."""
    N, D = 1, 6
    case = TR.flat_case(N, S, seed=8000 + S)
    h = E.make(hydro, case, L)
    G = TR.kernel_rows(case, range(D))  # [row][col][s]
    WG = G * TR.trapezoid_widths(np.arange(S) * TR.DT)[None, None, :]
    parts = level_partitions(S)
    pmax = np.array([[np.max(np.abs(WG[:, c, lo:hi])) for lo, hi in parts] for c in range(D)])
    part_of = np.zeros(S + 4 * PTOP, dtype=int)
    for i, (lo, hi) in enumerate(parts):
        part_of[lo:] = i  # (a lag past the window is held to the last partition)
    rng = np.random.default_rng(20260 + S)
    must = [127, 128, 255, 256, 511, 512, S - 1]
    offsets = must + sorted(int(x) for x in rng.choice(np.setdiff1d(np.arange(1, S), must), 40 - len(must), replace=False))
    Hn = S + 8
    pos, rpy = TR.rest_state(case)
    zero = np.zeros(3 * N)
    t_h = T0 - TR.DT * np.arange(1, Hn + 1)
    nsteps = top_period(S) * (2 if S < 1024 else 1)
    worst = 0.0
    for i, off in enumerate(offsets):
        c = i % D
        v_h = np.zeros((Hn, D))
        v_h[off - 1, c] = 1.0  # newest first: the sample off steps behind step 0
        h.set_history(t_h, v_h)
        for n in range(nsteps):
            h.step(T0 + n * TR.DT, pos, rpy, zero, zero)
            rad = h.components()[1]
            lag = off + n
            expect = WG[:, c, lag] if lag < S else np.zeros(D)
            bound = TR.REL * float(pmax[c, part_of[lag]])
            err = np.abs(rad - expect)
            worst = max(worst, float(np.max(err)) / bound)
            assert np.max(err) <= bound, (f"S {S} L {L}: impulse {off} behind step 0, column {c}, step {n} (lag {lag}), row {int(np.argmax(err))}: "
                                          f"|rad - expect| {np.max(err):.3e} > {bound:.3e}")
    assert h.profile()["tail_blocks"] >= len(offsets) * (nsteps // L - 1)
    print(f"S {S} L {L}: {len(offsets)} impulses x {nsteps} steps, max |d| / bound {worst:.2e}")


# ---- c. period edges -------------------------------------------------------------------------------------------------------------
def test_levels_period_edges(hydro):
    """Steps back in time across a 128-, a 256- and a 512-period boundary, hc_set_history in the middle of a period of each length,
    the form switched 1 -> 2 -> 1 and the taper (K) changed mid-period: within MODE_TOL of a context that kept the full pass.

    Every step back, hc_set_history and change of form starts a NEW top period (and all levels with it) at the first block planned
    afterwards, so the boundaries lie at r0 + k P counted from that restart r0, not at multiples of P counted from step 0.  The test
    reads r0 off the library -- the block whose pass raises tail_blocks first after a restart is planned behind step r0 - 1 -- lays
    every leg out from it, and asserts each crossing: the last step before the step back lies at or past the boundary (40 steps, so
    the level's rows have been overwritten by the next period's), the step it goes back to before it."""
    N, S, L = 3, 1024, 32
    case = TR.flat_case(N, S, seed=9000)
    taper = [dict(rirf_end_time=7.5, taper_start_percent=0.8, taper_final_amplitude=0.1), dict(rirf_end_time=6.0, taper_start_percent=0.6, taper_final_amplitude=0.0)]
    tail, full = E.make(hydro, case, L, tail=1), E.make(hydro, case, L, tail=0)
    for h in (tail, full):
        h.set_convolution_mode(1)
        h.set_tapered_direct_options(**taper[0])
    run = E.Run(case, S, seed=90)
    for h in (tail, full):
        h.set_history(*run.history())
    st = dict(n=0, r0=None, blocks=0, worst=0.0, calls=0, last=-1)

    def step():
        """the next step on both contexts; notes the start of a top period that a restart left pending"""
        n = st["n"]
        out = run.step([tail, full], n)
        st["worst"] = max(st["worst"], E.relerr(out[0][0], out[1][0]))
        assert st["worst"] <= MODE_TOL, f"call {st['calls']} (step {n}, top period from {st['r0']}): levels vs full pass {st['worst']:.2e}"
        blocks = tail.profile()["tail_blocks"]
        if st["r0"] is None and blocks > st["blocks"]:
            st["r0"] = n + 1  # the pass issued behind step n serves the block whose first step is n + 1
        st["blocks"] = blocks
        st["last"], st["n"], st["calls"] = n, n + 1, st["calls"] + 1

    def restart():
        """forward until the levels have restarted; returns the first step of the new top period"""
        st["r0"] = None
        first = st["n"]
        while st["r0"] is None:
            assert st["n"] - first <= 4 * L, f"no tail block within {4 * L} steps of the restart at step {first}"
            step()
        return st["r0"]

    def forward_to(n_last):
        while st["n"] <= n_last:
            step()

    def set_history():
        n = st["n"]
        assert len(run.v) == run.H + n  # (the samples up to step n - 1 are known)
        t_h = run.time(n) - TR.DT * np.arange(1, S + 9)
        v_h = 0.9 * run.v[run.H + n - (S + 8):run.H + n][::-1].copy()
        for h in (tail, full):
            h.set_history(t_h, v_h)

    crossed = []
    r0 = restart()
    for P in (128, 256, 512):  # a step back across the first boundary of each period length
        boundary = r0 + P
        forward_to(boundary + 40)
        back_to = boundary - 20
        assert st["last"] >= boundary > back_to >= r0
        crossed.append((P, r0, boundary, st["last"], back_to))
        st["n"] = back_to
        r0 = restart()
        assert back_to <= r0 <= back_to + 2 * L, (back_to, r0)
    for into in (60, 128 + 70, 300):  # hc_set_history in the middle of a 128-period, of a 256-period (in its second 128), of a 512-period
        forward_to(r0 + into - 1)
        set_history()
        r0 = restart()
    forward_to(r0 + 40 - 1)           # a change of form 40 steps into a top period, back after 100 steps
    tail.set_radiation_tail(2)
    r0 = restart()
    forward_to(r0 + 100 - 1)
    tail.set_radiation_tail(1)
    r0 = restart()
    forward_to(r0 + 128 + 50 - 1)     # a change of K 50 steps into the second 128-period
    for h in (tail, full):
        h.set_tapered_direct_options(**taper[1])
    r0 = restart()
    forward_to(r0 + 2 * 128 + 20)
    p = tail.profile()
    assert p["history_rewinds"] >= 3 and p["tail_blocks"] >= st["calls"] // (2 * L), p
    print(f"period edges: levels vs full pass {st['worst']:.2e} over {st['calls']} calls, tail blocks {p['tail_blocks']}, rewinds {p['history_rewinds']}; "
          f"steps back (P, period start, boundary, from, to): {crossed}")


# ---- d. row shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,shards", [(3, 2), (5, 3)])
def test_levels_row_shards_bitwise(hydro, N, shards):
    S, L = 1024, 32
    case = TR.flat_case(N, S, seed=9100 + N)
    full = E.make(hydro, case, L)
    group = hydro.HydroGroup.from_case(case, shards)
    E.configure(group, L)
    assert len(group.shards) == shards and sum(h.D_local for h in group.shards) == 6 * N and all(h.D_local > 0 for h in group.shards)
    run = E.Run(case, S, seed=N)
    full.set_history(*run.history())
    group.set_history(*run.history())
    for n in range(2 * PTOP + 20):
        a, b = run.step([full, group], n)
        assert np.array_equal(a[0], b[0]), f"step {n}: {E.relerr(b[0], a[0]):.2e}"
    assert full.profile()["tail_blocks"] >= (2 * PTOP) // L
    assert all(h.profile()["tail_blocks"] == full.profile()["tail_blocks"] for h in group.shards)


# ---- e. HIP launches against the direct dispatch ------------------------------------------------------------------------------------
def child_run(out_path):
    """N = 2, S = 1024, 600 steps in the levelled form; the forces of every step and whether the direct dispatch is in use."""
    import hydrochrono_amd.hydro as hydro
    N, S, L = 2, 1024, 32
    case = TR.flat_case(N, S, seed=9200)
    h = E.make(hydro, case, L)
    run = E.Run(case, S, seed=92)
    h.set_history(*run.history())
    f = np.stack([run.step([h], n)[0][0] for n in range(600)])
    np.savez(out_path, forces=f, direct=int(h.direct_dispatch()[0]), tail_blocks=h.profile()["tail_blocks"])


def test_levels_hip_launches_and_direct_dispatch_bitwise(hydro, tmp_path):
    runs = {}
    for d in ("0", "1"):
        out = str(tmp_path / f"direct{d}.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=dict(os.environ, HC_DIRECT=d), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (d, (r.stdout + r.stderr)[-2000:])
        runs[d] = np.load(out)
    assert int(runs["0"]["direct"]) == 0 and int(runs["1"]["direct"]) == 1, "the direct dispatch is not available here"
    assert int(runs["0"]["tail_blocks"]) == int(runs["1"]["tail_blocks"]) >= 600 // 32 - 1
    a, b = runs["0"]["forces"], runs["1"]["forces"]
    bad = [n for n in range(a.shape[0]) if not np.array_equal(a[n], b[n])]
    assert not bad, f"HIP launches and direct dispatch differ at steps {bad[:8]}: {E.relerr(a[bad[0]], b[bad[0]]):.2e}"


# ---- f. shapes that keep the full pass ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["step_dt", "S511", "ahead"])
def test_levels_ineligible_shapes_keep_the_full_pass_bitwise(hydro, variant):
    N, L = 3, 32
    S = 511 if variant == "S511" else 1024
    dt = 1.5 * TR.DT if variant == "step_dt" else TR.DT
    sched = 1 if variant == "ahead" else 0
    case = TR.flat_case(N, S, seed=9300 + S)
    a, b = E.make(hydro, case, L, tail=1, sched=sched), E.make(hydro, case, L, tail=0, sched=sched)
    run = E.Run(case, S, seed=93, dt=dt)
    for h in (a, b):
        h.set_history(*run.history())
        h.enable_profiling(1)
    for n in range(PTOP + 2 * L):
        out = run.step([a, b], n)
        assert np.array_equal(out[0][0], out[1][0]), f"{variant}: step {n}: {E.relerr(out[0][0], out[1][0]):.2e}"
    p = a.profile()
    assert p["tail_launches"] == 0 and p["tail_blocks"] == 0 and p["block_kernel_launches"] > 0, p


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child_run(sys.argv[2])
