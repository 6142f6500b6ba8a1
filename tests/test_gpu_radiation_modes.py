"""State-space radiation by modal recursion on the GPU (include/hydrochrono_amd.h: hc_set_radiation_modes) against the
longdouble restatement (tests/radiation_modes_ref.py), bit for bit across runs, shards, contexts and steps back in time, its errors,
its composition in HydroForces.step, and against the convolution it stands in for.  The CPU side is
tests/test_radiation_modes_ref_cpu.py."""
import os
import subprocess

import numpy as np
import pytest

import radiation_modes_ref as rm
from cases import GOLDEN_DIR, load_into_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 1000.0

# The constant of the bound C eps (steps + items in the row) sum|rho| max|z|, in ulp of the largest |z|, per step and mode.  ocml
# documents 1 ulp for the FP64 exp and 2 ulp for sin and cos of sincos.  e^x = exp(Re x) (cos, sin)(Im x): 1 + 2 + 1/2 for the
# product + 1/2 + 1/2 for the two roundings of x = lambda h that the exp and the sincos amplify by |x| e^-|x| <= 1 -- 4.5.  phi1 and
# phi2 multiply velocities whose h phi v is at most |z|-sized; in closed form (|x| >= 1) the numerators e^x - 1 and phi1 - 1 inherit
# the 4.5 ulp of e^x and are at least 0.36 in size against terms of size 1, a factor below 3, then one complex multiplication by 1/x
# each (2 ulp): 3 * 4.5 + 4 = 17.5 for phi2, the worse of the two; the series has 2 ulp per Horner step that decay geometrically,
# below that.  The recurrence itself: a complex product, two real products and three sums per part, 4 ulp; Re[rho z] and its place in
# the row sum 2.  C = 4.5 + 17.5 + 4 + 2 = 28, rounded up to 32.
C_ULP = 32.0


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def small_case(N):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, S=2, dt_rirf=0.05, n_exc=4, dt_exc=0.1, seed=5, rho=RHO)


_CASES = {}


def context(HF, N, modes_by_body, body_range=None, depth=None):
    """A finalized context of N bodies (the smallest IRF the suite runs; the modal term reads none of it) with the lists set."""
    if N not in _CASES:
        _CASES[N] = small_case(N)
    h = HF.from_case(_CASES[N], body_range=body_range)
    if depth is not None:
        h.set_radiation_modes_depth(depth)
    for b, modes in modes_by_body.items():
        h.set_radiation_modes(b, modes)
    return h


def velocity(D, t):
    c = np.arange(D)
    return (1.0 + 0.07 * c) * np.sin(0.9 * t + 0.61 * c) + 0.3 * np.cos(2.3 * t - 0.2 * c)


def split(v):
    v = np.asarray(v).reshape(-1, 6)
    return np.ascontiguousarray(v[:, :3]).reshape(-1), np.ascontiguousarray(v[:, 3:]).reshape(-1)


def random_mode(rng):
    lam = complex(-rng.uniform(0.05, 3.0), rng.uniform(0.0, 4.0) if rng.uniform() > 0.35 else 0.0)
    rho = complex(rng.normal(), rng.normal() if lam.imag else 0.0)
    return lam, rho


def row_with(n_items, D, row, rng):
    """n_items modes on one row, spread over the D columns as evenly as they go (at most 16 on a pair)"""
    base, extra = divmod(n_items, D)
    assert base + (1 if extra else 0) <= 16
    return [(row, c) + random_mode(rng) for c in range(D) for _ in range(base + (1 if c < extra else 0))]


def shape_modes(shape):
    rng = np.random.default_rng(100 + len(shape))
    if shape == "one":  # N = 1, a single mode on one pair
        return 1, {0: [(2, 2, -0.8 + 1.7j, 1.3 - 0.4j)]}
    if shape == "three":  # N = 3, 0 to 5 modes per pair: empty pairs, and rows without a mode at all (row 3 of body 1, body 2's row 0)
        modes = {}
        for b in range(3):
            lst = []
            for r in range(6):
                if (b, r) in ((1, 3), (2, 0)):
                    continue
                for c in range(18):
                    lst += [(r, c) + random_mode(rng) for _ in range(int(rng.integers(0, 6)))]
            order = rng.permutation(len(lst))  # the caller's order is not the device's
            modes[b] = [lst[i] for i in order]
        return 3, modes
    if shape == "eleven":  # N = 11 (D = 66): rows of exactly 255, 256, 257 and 528 modes, a few light rows, most rows empty
        modes = {0: row_with(255, 66, 1, rng) + row_with(3, 66, 4, rng), 4: row_with(256, 66, 0, rng) + row_with(257, 66, 5, rng),
                 10: row_with(528, 66, 3, rng) + row_with(70, 66, 2, rng)}
        return 11, modes
    raise ValueError(shape)


def step_times(pattern, modes_by_body):
    lams = [m[2] for lst in modes_by_body.values() for m in lst]
    first = lams[0]
    if pattern == "uniform":
        return 0.05 * np.arange(11)
    if pattern == "irregular":
        rng = np.random.default_rng(9)
        return np.concatenate([[0.3], 0.3 + np.cumsum(np.exp(rng.uniform(np.log(1e-4), np.log(0.3), size=10)))])
    if pattern == "threshold":  # |lambda h| of the first mode just below 1, just above, and once more each way; the others fall where they fall
        hs = np.array([1.0 - 1e-9, 1.0 + 1e-9, 0.999, 1.001, 1.0, 0.5, 2.0]) / abs(first)
        return np.concatenate([[0.0], np.cumsum(hs)])
    if pattern == "stiff":  # |Re lambda h| = 800 for the slowest mode, above for all others: e^x underflows everywhere
        h = 800.0 / min(abs(lam.real) for lam in lams)
        return np.concatenate([[0.0], np.cumsum([0.02, 0.05, h, 0.03, h, 0.01])])
    raise ValueError(pattern)


WORST = {}


@pytest.mark.parametrize("pattern", ["uniform", "irregular", "threshold", "stiff"])
@pytest.mark.parametrize("shape", ["one", "three", "eleven"])
def test_against_the_longdouble_reference(HF, shape, pattern):
    """1: row by row inside C eps (steps + items in the row) sum|rho| max|z|, C = C_ULP (derived above).  The worst ratio observed
    over the twelve cases, 8.6e-3 (N = 1, uniform), is recorded in MEASURED.md."""
    N, modes = shape_modes(shape)
    h = context(HF, N, modes)
    ref = rm.ModalRef(rm.device_rows(modes, 0, N, RHO))
    times = step_times(pattern, modes)
    worst = 0.0
    for n, t in enumerate(times):
        v = velocity(6 * N, t)
        got = h.compute_radiation_modes(t, *split(v))
        want = ref.step(t, v)
        assert got.shape == (6 * N,) and np.all(np.isfinite(got)), (shape, pattern, n)
        if n == 0:
            assert not got.any()
            continue
        bound = ref.bound(C_ULP)
        err = np.abs(np.asarray(got, dtype=np.longdouble) - want).astype(np.float64)
        empty = np.array([len(r) == 0 for r in ref.rows])
        assert not got[empty].any()  # a row without modes stores 0
        ratio = float(np.max(err[~empty] / bound[~empty]))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (shape, pattern, n, ratio)
    assert np.abs(got).max() > 0.0
    WORST[(shape, pattern)] = worst
    print(f"radiation modes {shape}/{pattern}: worst |gpu - ref| / bound = {worst:.3e} over {len(times) - 1} steps")


def drive(h, times, N, fn=None):
    fn = fn or h.compute_radiation_modes
    return np.array([fn(t, *split(velocity(6 * N, t))) for t in times])


def test_bits_across_runs_calls_contexts_shards_and_rewinds(HF):
    """2: (a) two runs, (b) compute against begin / end, (c) body 1 of N = 3 -- modes on its own six columns only, every other pair of
    its rows empty, the other bodies with lists of their own -- against the same lists alone in a one-body context, columns moved
    by -6 and the velocities those of body 1, (d) a row shard of hc_create_sharded and a HydroGroup against the whole context,
    (e) t1 t2 t3, back to t2', on -- against a fresh run t1 t2' ..."""
    from hydrochrono_amd.hydro import HydroGroup
    rng = np.random.default_rng(21)
    N, D = 3, 18
    own = [(r, 6 + c) + random_mode(rng) for r in range(6) for c in range(6) for _ in range(int(rng.integers(0, 4)))]
    modes = {0: [(r, c) + random_mode(rng) for r in range(6) for c in range(D) for _ in range(2)], 1: own,
             2: [(r, c) + random_mode(rng) for r in (0, 5) for c in range(D) for _ in range(16)]}  # rows of 288: more than one stride
    times = np.concatenate([[0.0], np.cumsum([0.01, 0.2, 0.013, 0.09, 0.4, 0.002])])
    whole = context(HF, N, modes)
    a = drive(whole, times, N)
    assert np.abs(a[1:]).min(axis=0).max() > 0.0
    # (a)
    again = context(HF, N, modes)
    assert same_bits(a, drive(again, times, N))
    # (b)
    split_calls = context(HF, N, modes)

    def begin_end(t, lv, av):
        split_calls.radiation_modes_begin(t, lv, av)
        return split_calls.radiation_modes_end()
    assert same_bits(a, drive(split_calls, times, N, begin_end))
    # (c)
    alone = context(HF, 1, {0: [(r, c - 6, lam, rho) for r, c, lam, rho in own]})
    b = np.array([alone.compute_radiation_modes(t, *split(velocity(D, t)[6:12])) for t in times])
    assert same_bits(a[:, 6:12], b)
    # (d)
    shard = context(HF, N, modes, body_range=(1, 3))
    assert same_bits(a[:, 6:], drive(shard, times, N))
    grp = HydroGroup([context(HF, N, modes, body_range=(0, 1)), context(HF, N, modes, body_range=(1, 3))])
    assert same_bits(a, drive(grp, times, N))
    # (e)
    t1, t2, t3, t2p = 0.5, 0.61, 0.7, 0.58
    rew, fresh = context(HF, N, modes), context(HF, N, modes)
    drive(rew, [t1, t2, t3], N)
    after_rewind = drive(rew, [t2p, 0.66, 0.9], N)
    drive(fresh, [t1], N)
    assert same_bits(after_rewind, drive(fresh, [t2p, 0.66, 0.9], N))
    # reset_history empties the ring: the next call is a first call again
    rew.reset_history()
    assert not rew.compute_radiation_modes(0.9, *split(velocity(D, 0.9))).any()


def test_errors(HF):
    """3: duplicate time, a rewind past the depth (refused, the next result unchanged), a set while a begin is pending, and the
    setter's refusals."""
    from hydrochrono_amd.hydro import HydroError
    N, D = 2, 12
    modes = {0: [(0, 0, -1.0, 2.0), (3, 7, -0.5 + 2j, 1 - 1j)], 1: [(5, 11, -2.0, 1.0)]}
    h, twin = context(HF, N, modes, depth=3), context(HF, N, modes, depth=3)
    times = [0.0, 0.1, 0.2, 0.3, 0.4]
    drive(h, times, N)
    drive(twin, times, N)
    lv, av = split(velocity(D, 0.4))
    with pytest.raises(HydroError) as ei:
        h.compute_radiation_modes(0.4, lv, av)
    assert ei.value.status == 1 and "twice within the same time step" in str(ei.value)
    with pytest.raises(HydroError) as ei:
        h.compute_radiation_modes(0.15, lv, av)  # depth 3 keeps 0.2, 0.3, 0.4
    assert ei.value.status == 3
    with pytest.raises(HydroError) as ei:
        h.compute_radiation_modes(0.2, lv, av)  # the oldest itself would have to go
    assert ei.value.status == 3
    assert same_bits(drive(h, [0.5, 0.45], N), drive(twin, [0.5, 0.45], N))  # nothing was left behind, nothing pending
    # the protocol
    h.radiation_modes_begin(0.6, lv, av)
    for call in (lambda: h.set_radiation_modes(0, []), lambda: h.set_radiation_modes_depth(5), h.reset_radiation_modes, h.reset_history,
                 lambda: h.radiation_modes_begin(0.7, lv, av)):
        with pytest.raises(HydroError) as ei:
            call()
        assert ei.value.status == 3
    out = h.radiation_modes_end()
    assert same_bits(out, twin.compute_radiation_modes(0.6, lv, av))
    with pytest.raises(HydroError) as ei:
        h.radiation_modes_end()
    assert ei.value.status == 3
    # the setter
    good = (0, 0, -1.0, 1.0)
    for bad in ((6, 0, -1.0, 1.0), (-1, 0, -1.0, 1.0), (0, D, -1.0, 1.0), (0, -1, -1.0, 1.0), (0, 0, 0.0, 1.0), (0, 0, 0.5 + 1j, 1.0),
                (0, 0, complex(-1.0, np.nan), 1.0), (0, 0, -1.0, np.inf), (0, 0, -np.inf, 1.0)):
        with pytest.raises(HydroError) as ei:
            h.set_radiation_modes(0, [good, bad])
        assert ei.value.status == 3, bad
    with pytest.raises(HydroError):
        h.set_radiation_modes(0, [good] * 17)
    with pytest.raises(HydroError):
        h.set_radiation_modes(2, [good])
    for depth in (1, 65):
        with pytest.raises(HydroError):
            h.set_radiation_modes_depth(depth)
    assert h.radiation_mode_count(0) == 2 and h.radiation_mode_count(1) == 1  # a refused list replaces nothing
    h.set_radiation_modes(0, [good] * 16)
    assert h.radiation_mode_count(0) == 16
    # a body outside the shard is accepted and ignored; non-finite input is refused before anything is pending
    sh = context(HF, N, modes, body_range=(1, 2))
    assert sh.radiation_mode_count(0) == 2
    assert drive(sh, [0.0, 0.1], N).shape == (2, 6)
    with pytest.raises(HydroError):
        sh.compute_radiation_modes(np.nan, lv, av)
    with pytest.raises(HydroError):
        sh.compute_radiation_modes(0.2, lv * np.inf, av)
    sh.compute_radiation_modes(0.2, lv, av)
    # the getter the fits are checked against: no rho factor
    tau = np.array([0.0, 0.3, 1.1])
    K = twin.radiation_modes_irf(0, tau)
    assert K.shape == (6, D, 3) and np.count_nonzero(K.any(axis=2)) == 2
    assert np.allclose(K[0, 0], 2.0 * np.exp(-tau), rtol=1e-15) and np.allclose(K[3, 7], ((1 - 1j) * np.exp((-0.5 + 2j) * tau)).real, rtol=1e-14)


def test_step_composition(HF):
    """4: step with modes = step without modes - compute_radiation_modes, elementwise; cleared, the bits from before; with
    set_zero_rirf the total is hs + waves - modal term."""
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import many_body_case, rest_positions
    N = 2
    case = many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7, rho=RHO)
    rng = np.random.default_rng(4)
    modes = {0: [(r, c) + random_mode(rng) for r in range(6) for c in range(12)], 1: [(2, 8, -0.7 + 1.9j, 40.0 - 5j)]}
    a, plain, side = HF.from_case(case), HF.from_case(case), HF.from_case(case)
    grp, gplain = (HydroGroup([HF.from_case(case, body_range=(0, 1)), HF.from_case(case, body_range=(1, 2))]) for _ in range(2))
    for h in (a, plain, side, grp, gplain):
        h.add_waves_regular(0.3, 1.1)
    for b, lst in modes.items():
        for h in (a, side, grp):
            h.set_radiation_modes(b, lst)
    motion = PrescribedMotion(N, rest_positions(case), seed=2)
    t = 0.03
    for n in range(12):
        t += (0.01, 0.037, 0.004)[n % 3]
        st = motion.state(t)
        total, modal = plain.step(t, *st), side.compute_radiation_modes(t, st[2], st[3])
        fa = a.step(t, *st)
        assert same_bits(fa, total - modal) and same_bits(a.radiation_modes(), modal)
        assert same_bits(grp.step(t, *st), gplain.step(t, *st) - modal) and same_bits(grp.radiation_modes(), modal)
    assert np.abs(modal).max() > 0.0
    # cleared: today's calls, today's bits
    for b in modes:
        a.set_radiation_modes(b, [])
    for n in range(3):
        t += 0.01
        st = motion.state(t)
        assert same_bits(a.step(t, *st), plain.step(t, *st)) and not a.radiation_modes().any()
    # modes only: a zero IRF, total = hs + waves - modal
    z = HF(N)
    z.set_simulation_parameters(case["rho"], case["g"], case["water_depth"])
    for b, bd in enumerate(case["bodies"]):
        z.set_body(b, bd["disp_vol"], bd["cg"], bd["cb"], bd["lin"], bd["added_mass_inf"], bd["rirf_t"], bd["rirf_K"])
        z.set_body_excitation_rao(b, bd["w"], bd["ex_mag"], bd["ex_phase"])
    with pytest.raises(Exception):
        z.set_zero_rirf(0)  # the IRF of the case is in: time vectors must agree
    z = HF(N)
    z.set_simulation_parameters(case["rho"], case["g"], case["water_depth"])
    for b, bd in enumerate(case["bodies"]):
        z.set_body(b, bd["disp_vol"], bd["cg"], bd["cb"], bd["lin"], bd["added_mass_inf"], [0.0, 0.05], np.zeros((6, 6 * N, 2)))
        z.set_zero_rirf(b)
        z.set_body_excitation_rao(b, bd["w"], bd["ex_mag"], bd["ex_phase"])
    z.finalize()
    z.add_waves_regular(0.3, 1.1)
    side2 = context(HF, N, modes)
    for b, lst in modes.items():
        z.set_radiation_modes(b, lst)
    tt = 0.2
    for n in range(6):
        tt += (0.03, 0.011)[n % 2]
        st = motion.state(tt)
        f = z.step(tt, *st)
        hs, rad, wv = z.components()
        modal = side2.compute_radiation_modes(tt, st[2], st[3])
        assert not rad.any() and same_bits(f, (hs - rad + wv) - modal)


def test_against_the_convolution(HF):
    """5: K sampled from the modes on a fine IRF grid, v = a_c sin(omega t) on a uniform step: hc_compute_radiation and the modal
    force each within their own discretisation bound of the analytic integral.  The modal bound is the interpolation bound
    (omega h)^2 / 8 v_max sum |rho| / |Re lambda|; the convolution's is twice what the CPU oracle's error against the same integral
    measures here.  Measured on an MI355X: max |rad| 1.701e3; modal error 0.354 (bound 1.097); convolution error 0.994, the
    oracle's 0.994 (bound 1.988)."""
    from hydrochrono_amd.synthetic import many_body_case
    N, D, S, dt, omega = 1, 6, 401, 0.025, 2.0
    rng = np.random.default_rng(8)
    # fast poles: exp(Re lambda * 10 s) < 3e-7, the IRF window holds all of K
    pair = {(r, c): [(complex(-rng.uniform(1.5, 3.0), rng.uniform(0.5, 3.0)), complex(rng.normal(), rng.normal())),
                     (complex(-rng.uniform(1.5, 3.0), 0.0), complex(rng.normal(), 0.0))] for r in range(6) for c in range(6)}
    modes = [(r, c, lam, rho) for (r, c), lst in pair.items() for lam, rho in lst]
    tau = dt * np.arange(S)
    K = np.zeros((6, D, S))
    for r, c, lam, rho in modes:
        K[r, c] += (rho * np.exp(lam * tau)).real
    case = many_body_case(N, S=S, dt_rirf=dt, n_exc=4, dt_exc=0.1, seed=3, rho=RHO)
    case["bodies"][0]["rirf_K"] = K
    conv, modal = HF.from_case(case), HF.from_case(case)
    modal.set_radiation_modes(0, modes)
    assert np.max(np.abs(modal.radiation_modes_irf(0, tau) - K)) <= 1e-14 * np.abs(K).max()
    orc = load_into_oracle(case)
    amp = np.array([1.0, -0.6, 0.8, 0.3, -0.5, 0.2])
    steps = int(round(3 * 2 * np.pi / omega / dt))  # three periods
    zero = np.zeros(3)
    err_conv = err_modal = err_orc = 0.0
    times = dt * np.arange(steps + 1)
    # the analytic integral (radiation_modes_ref.z_sine) at every step time at once, in longdouble
    tl, wl = times.astype(np.longdouble), np.longdouble(omega)
    analytic = np.zeros((steps + 1, 6), dtype=np.longdouble)
    for r, c, lam, rho in modes:
        lam_l = rm.CLD(lam)
        el = np.exp(lam_l * tl)
        z = ((np.exp(rm.CLD(1j) * wl * tl) - el) / (rm.CLD(1j) * wl - lam_l) - (np.exp(rm.CLD(-1j) * wl * tl) - el) / (rm.CLD(-1j) * wl - lam_l)) / rm.CLD(2j)
        analytic[:, r] += (rm.CLD(RHO * rho) * z).real * np.longdouble(amp[c])
    assert abs(analytic[7, 2] - sum((rm.CLD(RHO * rho) * rm.z_sine(lam, omega, times[7])).real * amp[c] for r, c, lam, rho in modes if r == 2)) < 1e-12
    top = float(np.abs(analytic).max())
    for n, t in enumerate(times):
        v = amp * np.sin(omega * t)
        want = analytic[n].astype(np.float64)
        err_conv = max(err_conv, float(np.abs(conv.compute_radiation(t, v[:3], v[3:]) - want).max()))
        err_modal = max(err_modal, float(np.abs(modal.compute_radiation_modes(t, v[:3], v[3:]) - want).max()))
        err_orc = max(err_orc, float(np.abs(orc.compute_radiation(t, v[:3], v[3:]) - want).max()))
    by_row = np.zeros(6)
    for r, c, lam, rho in modes:
        by_row[r] += RHO * abs(rho) / abs(lam.real) * abs(amp[c])
    bound_modal = (omega * dt) ** 2 / 8.0 * float(by_row.max())
    print(f"against the convolution: max |rad| {top:.3e}; modal error {err_modal:.3e} (bound {bound_modal:.3e}); "
          f"convolution error {err_conv:.3e} (oracle {err_orc:.3e}, bound {2 * err_orc:.3e})")
    assert 0.0 < err_modal <= bound_modal
    assert 0.0 < err_conv <= 2.0 * err_orc


def test_cpp_caller_prints_the_c_abi_values(HF, tmp_path):
    """6: tests/cpp/radiation_modes_caller.cpp through the C++ mirror against the same calls made here."""
    from hydrochrono_amd import build as hb
    from hydrochrono_amd import capi
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "radiation_modes_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "radiation_modes_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    lines = r.stdout.strip().splitlines()
    rows = np.array([[float(v) for v in line.split()] for line in lines[:-1]])
    assert rows.shape == (31, 25) and lines[-1].startswith("standalone")
    modes = [(2, 2, -0.9, 30.0), (2, 2, -0.3 + 2.1j, 12.0 - 4.0j), (0, 4, -1.2 + 0.7j, -3.0 + 1.5j), (4, 0, -1.2 + 0.7j, -3.0 + 1.5j)]
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(0.177, 2.094395102, num_bodies=1)
    h.set_radiation_modes(0, modes)
    assert rows[30, 0] < rows[29, 0]  # the last line is the step back in time
    for row in rows:
        t, lv, av, pos, rpy = row[0], row[1:4], row[4:7], row[7:10], row[10:13]
        out = np.empty(6)
        a = [np.ascontiguousarray(x) for x in (pos, rpy, lv, av)]
        rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
        assert rc == capi.HC_OK
        modal = h.compute_radiation_modes(t, lv, av)
        assert same_bits(row[19:25], modal) and same_bits(row[13:19], out - modal), t
    assert np.abs(rows[:, 19:25]).max() > 1.0
    # the line of ComputeForceRadiationModes on a reset state: set_state(1.0, 0), then set_state(1.25, 1)
    h.reset_radiation_modes()

    def state(t, n):
        return np.array([0.1 + 0.3 * t, -0.05 * n, 0.3 - 0.2 * t]), np.array([0.02, -0.03 + 0.01 * t, 0.01 * n])
    assert not h.compute_radiation_modes(1.0, *state(1.0, 0)).any()
    alone = h.compute_radiation_modes(1.25, *state(1.25, 1))
    assert same_bits(alone, [float(v) for v in lines[-1].split()[1:]])
