"""Spectral radiation tail at its partition and eligibility edges.  Every eligible case runs a dense random velocity
history on the grid and then at least two whole superblocks and one block; every step's radiation component is held to the exact
longdouble lag sum of tests/tail_ref.py (row-wise, 1e-12 of the absolute sum), every step's total force to a twin context that keeps
the full pass (hc_set_radiation_tail(0)), and the tail must have run.  The IRF is the flat-envelope one of tail_ref.flat_case, so an
error in the far or the last partition is not damped away.  Ineligible shapes must run no tail at all and still match the reference.
Further: unit impulses whose lags sweep across the partition edges and the end of the window, row shards and hc_step_device bitwise
equal to the plain context, TaperedDirect with option and mode changes in the middle of a superblock (K-hat invalidation), and the
life cycle: a cold start, hc_reset_history, depth / tail / schedule switches and a step back in time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tail_ref as TR  # noqa: E402
from cases import load_into_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

MODE_TOL = 1e-12
ORACLE_TOL = 1e-10
P = 256          # hc_tail.hpp: kTailP, steps per superblock
T0 = 64.0        # first step time: a multiple of the grid spacing
REF_OPS = 1.5e8  # longdouble multiply-adds the reference may spend per context and test (more: it checks every few steps)


@pytest.fixture(scope="module")
def hydro():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hydrochrono_amd.hydro as hydro
    return hydro


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, float(np.max(np.abs(b)))))


def configure(h, L, tail=1, sched=0):
    h.add_waves_none()
    h.set_lookahead(L)
    h.set_pass_schedule(sched)
    h.set_radiation_tail(tail)
    return h


def make(hydro, case, L, tail=1, sched=0):
    return configure(hydro.HydroForces.from_case(case), L, tail, sched)


def partitions(S):
    return (S + P - 1) // P - 1 if S >= 2 * P else 0


class Run:
    """Drives contexts along the grid t = T0 + n dt with random velocities and keeps the samples (oldest first) for tail_ref."""

    def __init__(self, case, S, seed, dt=TR.DT, hist=None, t0=T0):
        self.N, self.D, self.dt, self.t0 = case["N"], 6 * case["N"], dt, t0
        self.rng = np.random.default_rng(seed)
        self.pos, self.rpy = TR.rest_state(case)
        self.H = S + 8 if hist is None else hist
        self.v = self.rng.standard_normal((self.H, self.D))  # the history, oldest first: sample k at t0 - (H - k) dt
        self.idx = []  # sample index of each step taken

    def history(self):
        t = self.t0 - self.dt * np.arange(1, self.H + 1)
        return t, self.v[::-1].copy()

    def time(self, n):
        return self.t0 + n * self.dt

    def step(self, ctxs, n, vel=None):
        """Step n (sample index H + n) on every context; returns [(total, radiation)] per context."""
        vel = self.rng.standard_normal(self.D) if vel is None else vel
        m = self.H + n
        self.v = np.concatenate([self.v[:m], vel[None, :]])  # (a step back in time drops the newer samples)
        self.idx.append(m)
        w = vel.reshape(self.N, 6)
        lin, ang = np.ascontiguousarray(w[:, :3]).reshape(-1), np.ascontiguousarray(w[:, 3:]).reshape(-1)
        out = []
        for h in ctxs:
            f = h.step(self.time(n), self.pos, self.rpy, lin, ang)
            out.append((f, h.components()[1].copy()))
        return out


def ref_for(case, S, rows=None, G=None):
    N, D = case["N"], 6 * case["N"]
    if rows is None:
        rows = list(range(D)) if D * D * S <= TR.ROW_BUDGET else TR.check_rows(N)
    if G is None:
        G = TR.kernel_rows(case, rows)
    return TR.TailRef(G, TR.trapezoid_widths(np.arange(S) * TR.DT), rows)


def stride_for(ref, nsteps):
    return max(1, int(np.ceil(nsteps * 2 * ref.R * ref.D * ref.S / REF_OPS)))


def checked(n, stride):
    return n % stride == 0 or n % P in (0, 1, P - 1)


# ---- a. shape matrix --------------------------------------------------------------------------------------------------------------
SHAPES = [  # N, S, L, eligible
    (1, 512, 32, True),     # NP = 1: no far part
    (1, 513, 16, True),     # NP = 2, the last partition holds one lag (half trapezoid weight)
    (5, 767, 32, True),
    (5, 768, 16, True),
    (5, 769, 32, True),     # NP = 3, one lag in the last partition
    (11, 1300, 16, True),   # NP = 5, x HC_DIRECT = 0 / 1
    (11, 1300, 32, True),
    (21, 8448, 32, True),   # NP = 32, NP * D = 4032: near the column cap (63 KB of LDS in tail_gemv)
    (170, 512, 32, True),   # D = 1020: the largest eligible
    (1, 511, 32, False),    # S < 2P
    (22, 8448, 32, False),  # NP * D = 4224 > 4096
    (171, 512, 32, False),  # D = 1026: wide
]


@pytest.mark.parametrize("N,S,L,eligible", SHAPES, ids=[f"N{s[0]}-S{s[1]}-L{s[2]}" for s in SHAPES])
def test_tail_shape_against_exact_reference(hydro, monkeypatch, N, S, L, eligible):
    case = TR.flat_case(N, S, seed=1000 + N + S)
    ctxs = []
    direct_modes = (1, 0) if N == 11 else (None,)
    for d in direct_modes:
        if d is not None:
            monkeypatch.setenv("HC_DIRECT", str(d))
        ctxs.append(make(hydro, case, L))
        if d is not None:
            assert ctxs[-1].direct_dispatch()[0] == bool(d), ctxs[-1].direct_dispatch()[1]
    twin = make(hydro, case, L, tail=0)
    ctxs.append(twin)
    run = Run(case, S, seed=N * 7 + S)
    for h in ctxs:
        h.set_history(*run.history())
    ref = ref_for(case, S)
    if N == 5 and S == 768:  # the reference's G is what the ingest made of the file: rho K in BEMIO order
        assert np.array_equal(twin.rirf_effective(), TR.kernel_rows(case, range(6 * N)))
    nsteps = 2 * P + 3 * L
    stride = stride_for(ref, nsteps)
    steps, rads = [], []
    worst_mode = 0.0
    for n in range(nsteps):
        out = run.step(ctxs, n)
        (ft, rt), (ff, _) = out[0], out[-1]
        worst_mode = max(worst_mode, relerr(ft, ff))
        assert worst_mode <= MODE_TOL, f"step {n}: tail vs full pass {worst_mode:.2e}"
        if len(out) == 3:
            assert np.array_equal(out[1][0], ft), f"step {n}: HIP launches and AQL dispatch differ: {relerr(out[1][0], ft):.2e}"
        if checked(n, stride):
            steps.append(run.idx[-1])
            rads.append(rt)
    worst = ref.check(run.v, steps, rads, f"N {N} S {S} L {L}: ")
    p, q = ctxs[0].profile(), twin.profile()
    assert q["tail_blocks"] == 0 and q["tail_launches"] == 0, q
    if eligible:
        assert p["tail_blocks"] >= 2 * (P // L) and p["tail_launches"] > 0, p
        if len(ctxs) == 3:
            assert ctxs[1].profile()["tail_blocks"] == p["tail_blocks"]
    else:
        assert p["tail_blocks"] == 0 and p["tail_launches"] == 0, p
    print(f"N {N} S {S} NP {partitions(S)} L {L}: max |d|/(1e-12 A_m) {worst:.2e} over {len(steps)} steps, rows {ref.R}; "
          f"tail vs full {worst_mode:.2e}; tail blocks {p['tail_blocks']}")


def test_tail_realistic_irf_with_waves_against_oracle(hydro):
    """many_body_case (decaying IRF) at N = 11, S = 1300 with irregular waves: tail, full pass and the flat oracle."""
    import oracle as orc_mod
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import many_body_case, rest_positions
    N, S, dt = 11, 1300, TR.DT
    case = many_body_case(N, S=S, dt_rirf=dt, n_exc=257, dt_exc=0.02, nw=32, seed=77)
    waves = dict(simulation_dt=dt, simulation_duration=T0 + 12.0, ramp_duration=0.0, wave_height=2.0, wave_period=8.0,
                 frequency_min=0.05, frequency_max=0.6, nfrequencies=32, peak_enhancement_factor=3.3, seed=3)
    tail, full = hydro.HydroForces.from_case(case), hydro.HydroForces.from_case(case)
    full.set_radiation_tail(0)
    motion = PrescribedMotion(N, rest_positions(case), seed=5)
    t_h = T0 - dt * np.arange(1, S + 9)
    v_h = np.stack([motion.velocity6(t) for t in t_h])
    for h in (tail, full):
        h.add_waves_irregular(**waves)
        h.set_pass_schedule(0)
        h.set_history(t_h, v_h)
    orc_mod.set_num_threads(min(16, os.cpu_count() or 1))
    orc = load_into_oracle(case)
    orc.add_waves_irregular(**waves)
    orc.prefill_history(t_h, v_h)
    orc.flat_prepare()
    worst_mode = worst_orc = 0.0
    for n in range(2 * P + 3 * 32):
        t = T0 + n * dt
        st = motion.state(t)
        ft, ff, fo = tail.step(t, *st), full.step(t, *st), orc.flat_step(t, *st)
        worst_mode = max(worst_mode, relerr(ft, ff))
        worst_orc = max(worst_orc, relerr(ft, fo))
        assert worst_mode <= MODE_TOL and worst_orc <= ORACLE_TOL, f"step {n}: mode {worst_mode:.2e}, oracle {worst_orc:.2e}"
    assert tail.profile()["tail_blocks"] >= 2 * (P // 32), tail.profile()


# ---- b. impulse sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [513, 769, 1300])
@pytest.mark.parametrize("L", [16, 32])
def test_tail_impulse_sweep(hydro, S, L):
    """Zero velocities but for unit impulses in the history; their lags cross 255/256/257, 511/512/513 and S-2, S-1, S at
    different places in a superblock.  Expected: rad_m = sum w_s G[:, c, s]; exactly zero once every impulse has left the
    windows of the tail for good."""
    N = 2
    D = 6 * N
    case = TR.flat_case(N, S, seed=2000 + S)
    h = make(hydro, case, L)
    G = TR.kernel_rows(case, range(D))                           # [row][col][s]
    WG = G * TR.trapezoid_widths(np.arange(S) * TR.DT)[None, None, :]
    H = S + 8
    # (sample index q, column): lag at step n = H + n - q; the first lags spread the crossings over the superblock phases
    first_lags = [200, 240 + L // 2, 470, S - 70, S - 3 - L // 4]
    impulses = [(H - lag, c) for lag, c in zip(first_lags, [0, 7, 3, 11, 5])]
    # and a run of P + L + 1 of them in one column: at every step of the first superblock one of them is exactly S - 1 old, so the
    # oldest lag is met at every offset j of a superblock (j = 0 included, where it is the oldest sample of the windows)
    impulses += [(H - lag, 9) for lag in range(S - 2 - P - L, S - 1)]
    v = np.zeros((H, D))
    for q, c in impulses:
        v[q, c] = 1.0
    t_h = T0 - TR.DT * np.arange(1, H + 1)
    h.set_history(t_h, v[::-1].copy())
    pos, rpy = TR.rest_state(case)
    zero = np.zeros(3 * N)
    q_imp, c_imp = np.array([q for q, _ in impulses]), np.array([c for _, c in impulses])
    nparts = (S - 1) // P + 1  # partition 0 = the head; a lag past the window is held to the last partition
    pmax = np.array([[np.max(np.abs(WG[:, c, p * P:min(S, (p + 1) * P)])) for p in range(nparts)] for c in range(D)])
    settle = S - 1 + 2 * P + 2 * L  # lag of the youngest impulse from which on nothing of it may remain anywhere
    nsteps = settle - (H - int(q_imp.max())) + 8
    seen = {s: 0 for s in (255, 256, 257, 511, 512, 513, S - 2, S - 1, S)}
    for n in range(nsteps):
        h.step(T0 + n * TR.DT, pos, rpy, zero, zero)
        rad = h.components()[1]
        lags = H + n - q_imp
        if lags.min() >= settle:
            assert np.all(rad == 0.0), f"step {n}: every impulse is older than the window, rad = {rad}"
            continue
        live = lags < S
        expect = WG[:, c_imp[live], lags[live]].sum(axis=1)
        bound = TR.REL * float(pmax[c_imp, np.minimum(lags // P, nparts - 1)].sum())
        for s in lags:
            if int(s) in seen:
                seen[int(s)] += 1
        err = np.abs(rad - expect)
        if np.max(err) > bound:
            row = int(np.argmax(err))
            bad = sorted({(int(s), int(c)) for s, c in zip(lags, c_imp) if s < S + P})
            raise AssertionError(f"S {S} L {L} step {n}, row {row}: |rad - expect| {err[row]:.3e} > {bound:.3e}; "
                                 f"(lag, column) of the impulses {bad[:12]}{' ...' if len(bad) > 12 else ''}")
    assert all(seen.values()), seen
    assert h.profile()["tail_blocks"] > 0


# ---- c. row shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,shards", [(11, 3), (7, 2)])
def test_tail_row_shards_bitwise_at_odd_row_counts(hydro, N, shards):
    S, L = 1300, 32
    case = TR.flat_case(N, S, seed=3000 + N)
    full = make(hydro, case, L)
    group = hydro.HydroGroup.from_case(case, shards)
    configure(group, L)
    assert [h.D_local for h in group.shards] == ([24, 24, 18] if N == 11 else [24, 18])
    run = Run(case, S, seed=N)
    full.set_history(*run.history())
    group.set_history(*run.history())
    for n in range(2 * P + 2 * L):
        a, b = run.step([full, group], n)
        assert np.array_equal(a[0], b[0]), f"step {n}: {relerr(b[0], a[0]):.2e}"
    assert full.profile()["tail_blocks"] >= 2 * (P // L)
    assert all(h.profile()["tail_blocks"] == full.profile()["tail_blocks"] for h in group.shards)


# ---- d. TaperedDirect and K-hat invalidation ----------------------------------------------------------------------------------------
def test_tail_tapered_direct_and_khat_invalidation(hydro):
    N, S, L = 5, 1300, 32
    case = TR.flat_case(N, S, seed=4000)
    opts = [dict(rirf_end_time=7.0, taper_start_percent=0.8, taper_final_amplitude=0.1),   # end at lag 896: in partition 3
            dict(rirf_end_time=9.5, taper_start_percent=0.6, taper_final_amplitude=0.0)]
    rows = list(range(6 * N))

    def tapered(o, tail=1):
        h = make(hydro, case, L, tail)
        h.set_convolution_mode(1)
        h.set_tapered_direct_options(**o)
        return h

    h = tapered(opts[0])
    orc = load_into_oracle(case)
    orc.add_waves_none()
    orc.set_convolution_mode(1)
    orc.set_tapered_direct_options(**opts[0])
    run = Run(case, S, seed=41)
    h.set_history(*run.history())
    orc.prefill_history(*run.history())
    state = {"mode": 1, "opts": opts[0]}

    def fresh():
        """a new context with the settings in force, given the same history, stepping on from here"""
        if state["mode"] == 1:
            f = tapered(state["opts"])
        else:
            f = make(hydro, case, L)
        n_hist = S + 8
        t = T0 + (len(run.idx) - 1) * TR.DT - TR.DT * np.arange(0, n_hist)
        f.set_history(t, run.v[len(run.v) - n_hist:][::-1].copy())
        return f

    def ref_now():
        return TR.TailRef(h.rirf_effective(), h.rirf_width(), rows)

    twin, ref = None, ref_now()
    changes = {300 + 7: "options", 300 + 7 + 2 * P - 50: "mode 0", 300 + 7 + 2 * P - 50 + 3 * L + 5: "mode 1"}
    n_end = max(changes) + 2 * P + L
    stride = stride_for(ref, n_end)
    worst = 0.0
    blocks_before = 0
    for n in range(n_end):
        if n in changes:
            what = changes[n]
            if what == "options":
                state["opts"] = opts[1]
                for x in (h, orc):
                    x.set_tapered_direct_options(**opts[1])
            else:
                state["mode"] = int(what[-1])
                for x in (h, orc):
                    x.set_convolution_mode(state["mode"])
            twin = fresh()
            ref = ref_now()
            blocks_before = h.profile()["tail_blocks"]
        ctxs = [h] + ([twin] if twin is not None else [])
        out = run.step(ctxs, n)
        w = run.v[-1].reshape(N, 6)
        fo = orc.step(run.time(n), run.pos, run.rpy, w[:, :3].reshape(-1).copy(), w[:, 3:].reshape(-1).copy())
        e_orc = relerr(out[0][0], fo)
        assert e_orc <= ORACLE_TOL, f"step {n} ({state}): tail vs oracle {e_orc:.2e}"
        if twin is not None:
            e = relerr(out[0][0], out[1][0])
            assert e <= MODE_TOL, f"step {n} ({state}): against a fresh context with the same settings {e:.2e}"
        if n == 0:  # the widths are the trapezoid widths, and the reference's sign and scale are those of both components
            assert np.array_equal(h.rirf_width(), TR.trapezoid_widths(np.arange(S) * TR.DT))
            assert relerr(out[0][1], orc.components()[1]) <= ORACLE_TOL
        if checked(n, stride) or any(0 <= n - c < 3 for c in changes):
            worst = max(worst, ref.check(run.v, [run.idx[-1]], [out[0][1]], f"step {n} ({state}): "))
        if n + 1 in changes or n + 1 == n_end:
            assert h.profile()["tail_blocks"] > blocks_before, (n, state, h.profile()["tail_blocks"])
    print(f"TaperedDirect: max |d|/(1e-12 A_m) {worst:.2e}, tail blocks {h.profile()['tail_blocks']}")


# ---- e. life cycle -----------------------------------------------------------------------------------------------------------------
LIFE = [("cold", 769), ("cold", 1300), ("reset", 769), ("reset", 1300), ("switches", 769), ("switches", 1300), ("rewind", 768)]


@pytest.mark.parametrize("scenario,S", LIFE, ids=[f"{a}-S{b}" for a, b in LIFE])
def test_tail_life_cycle(hydro, scenario, S):
    N, L = 3, 32
    case = TR.flat_case(N, S, seed=5000 + S)
    tail, twin = make(hydro, case, L), make(hydro, case, L, tail=0)
    ref = ref_for(case, S)
    cold = scenario == "cold"
    run = Run(case, S, seed=S + len(scenario), hist=0 if cold else None, t0=0.0 if cold else T0)
    if not cold:
        for h in (tail, twin):
            h.set_history(*run.history())
    base = 0          # sample index of the oldest sample the contexts hold
    schedule = list(range(S + 2 * P + 3 * L)) if cold else list(range(3 * P + 2 * L))
    if scenario == "rewind":  # forward past a superblock boundary, back across it (a rejected step), forward again
        schedule = list(range(0, 300)) + list(range(240, 2 * P + 3 * L + 240))
    events = {}
    if scenario == "reset":
        events = {P + 100: "reset"}
        schedule = list(range(P + 100 + S + 2 * P + 2 * L))
    elif scenario == "switches":
        events = {100: ("lookahead", 16), 100 + P + 9: ("lookahead", 32), 100 + 2 * P + 17: ("tail", 0), 100 + 2 * P + 60: ("tail", 1),
                  100 + 3 * P + 3: ("schedule", 1), 100 + 3 * P + 90: ("schedule", 0)}
        schedule = list(range(100 + 5 * P + L))
    worst_mode = worst_ref = 0.0
    blocks_at_fill = None
    for k, n in enumerate(schedule):
        ev = events.get(n)
        if ev == "reset":
            for h in (tail, twin):
                h.reset_history()
            base = run.H + n
            blocks_at_reset = tail.profile()["tail_blocks"]
        elif ev is not None:
            kind, val = ev
            for h in ((tail, twin) if kind != "tail" else (tail,)):
                {"lookahead": h.set_lookahead, "tail": h.set_radiation_tail, "schedule": h.set_pass_schedule}[kind](val)
        out = run.step([tail, twin], n)
        m = run.idx[-1]
        worst_mode = max(worst_mode, relerr(out[0][0], out[1][0]))
        assert worst_mode <= MODE_TOL, f"{scenario}: call {k} (step {n}): tail vs full pass {worst_mode:.2e}"
        full_window = m - base >= S  # samples m - S + 1 .. m and an older one
        if not full_window:
            assert tail.profile()["tail_blocks"] == (0 if base == 0 else blocks_at_reset), (
                f"{scenario}: step {n}: tail blocks before the history covers the window")
        elif blocks_at_fill is None:
            blocks_at_fill = tail.profile()["tail_blocks"]
        if full_window and (checked(n, stride_for(ref, len(schedule))) or ev is not None):
            worst_ref = max(worst_ref, ref.check(run.v, [m], [out[0][1]], f"{scenario}: step {n}: "))
    p = tail.profile()
    assert p["tail_blocks"] >= (blocks_at_fill or 0) + 2 * (P // L) - 2, p
    if scenario == "rewind":
        assert p["history_rewinds"] >= 1, p
    print(f"{scenario} S {S}: tail vs full {worst_mode:.2e}, max |d|/(1e-12 A_m) {worst_ref:.2e}, tail blocks {p['tail_blocks']}")


# ---- f. device steps ---------------------------------------------------------------------------------------------------------------
def test_tail_step_device_matches_host_step(hydro):
    import torch
    N, S, L = 11, 1300, 32
    case = TR.flat_case(N, S, seed=6000)
    a, b = make(hydro, case, L), make(hydro, case, L)
    run = Run(case, S, seed=66)
    for h in (a, b):
        h.set_history(*run.history())
    nsteps = 2 * P + 2 * L
    vel = run.rng.standard_normal((nsteps, 6 * N))
    packed = []
    for n in range(nsteps):
        w = vel[n].reshape(N, 6)
        packed.append(np.concatenate([run.pos, run.rpy, w[:, :3].reshape(-1), w[:, 3:].reshape(-1)]))
    states = torch.tensor(np.stack(packed), device="cuda")
    out = torch.zeros(nsteps, 6 * N, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for n in range(nsteps):
        b.step_device(run.time(n), states[n].data_ptr(), out[n].data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    host = np.stack([run.step([a], n, vel[n])[0][0] for n in range(nsteps)])
    dev = out.cpu().numpy()
    bad = [n for n in range(nsteps) if not np.array_equal(dev[n], host[n])]
    assert not bad, f"hc_step_device differs from hc_step at steps {bad[:8]}: {relerr(dev[bad[0]], host[bad[0]]):.2e}"
    assert a.profile()["tail_blocks"] >= 2 * (P // L) and b.profile()["tail_blocks"] == a.profile()["tail_blocks"]
