"""Second-order sum-frequency wave forces on the GPU (hc_set_sum_qtf, hc_sum_qtf_begin / hc_sum_qtf_end, hc_compute_sum_qtf;
csrc/hc_qtf.hip) against the direct longdouble pair sum of the definition (tests/sumfreq_ref.py), fed the context's own spectrum /
regular-wave coefficients.  The device evaluates the projected O(nf + nq^2) form, so the identity between the two is under test as well.

Tolerance: the bound sumfreq_ref derives per body and row, ramp^2 (2 * 1e-11 + (nf + nq^2 + 64) 2^-52) M_d, M_d twice the sum of the
absolute pair terms (its docstring has the derivation); the cross-check against the second-order sea adds the eta2 tolerance of
tests/test_gpu_wave_kinematics2.py for its side.  Every case keeps |theta_i| < 1e4; the reference asserts it."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sumfreq_ref as sr
import wave2_ref as w2
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0, wave_period=12.0,
                    frequency_min=0.001, frequency_max=1.0, nfrequencies=1000)
THREE_IRREG = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
                   frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)
SYNTH_IRREG = dict(simulation_dt=0.05, simulation_duration=200.0, ramp_duration=20.0, wave_height=4.0, wave_period=9.0,
                   frequency_min=0.02, frequency_max=0.6, nfrequencies=512, peak_enhancement_factor=2.0, seed=4)
REG_AMP, REG_OMEGA = 0.177, 2.094395102
WAVE2_TOL = 1e-11  # tests/wave2_inputs.py: TOL, the figure tests/test_gpu_wave_kinematics2.py applies to sum|term|


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def synth_case(N):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def positions(N, x, y=0.0, z=-1.0):
    pos = np.zeros((N, 3))
    pos[:, 0], pos[:, 1], pos[:, 2] = x, y, z
    return pos


def without_q(ref):
    """the pair sum of the same table with Q = None"""
    r = copy.copy(ref)
    r.Qij, r.table = None, (ref.table[0], ref.table[1], None)
    return r


def compare(h, refs, comp, t, pos, what, ramp=1.0):
    """GPU against the pair sum inside the derived bound.  refs: per body None or a sumfreq_ref.PairSum.  Returns [N][6]."""
    got = h.compute_sum_qtf(t, pos).reshape(-1, 6)
    assert np.all(np.isfinite(got)), what
    for b, ref in enumerate(refs):
        if ref is None:
            assert not got[b].any(), (what, b)
            continue
        want, bound = ref.force(t, pos[b, 0], ramp=ramp), sr.bound(comp, ref.table, ramp=ramp)
        err = np.abs(got[b] - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{what} body {b}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(want)):.3e}")
        assert np.all(err <= bound), f"{what} body {b}: worst {worst:.3e} of the bound"
    return got


# ------------------------------------------------------------------------------------------------
# 1: a regular wave on the sphere: both signs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [[1.5, 2.9], [0.7, 1.5, 2.0, 2.5, 3.3]])
def test_regular_wave_oscillates_at_twice_the_frequency(HF, grid):
    h = HF.from_case(sphere_case())
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    h.set_sum_options(regular_phase=0.7)
    k = h.regular_coeffs()[2]
    comp = wk.regular_components(REG_AMP, REG_OMEGA, k, 0.7)
    nq = len(grid)
    rng = np.random.default_rng(nq)
    table = (np.array(grid), rng.normal(0, 1e4, (6, nq, nq)), rng.normal(0, 1e4, (6, nq, nq)))
    h.set_sum_qtf(0, *table)
    h.set_sum_mode(1)
    assert h.sum_qtf_size(0) == nq
    ref, bound = sr.PairSum(comp, table), sr.bound(comp, table)
    Pww, Qww = sr.interp_diag(table, REG_OMEGA)
    states = []
    for t in (0.05, 0.4, 3.7, 41.3):  # the first two would be ramped to almost nothing in an irregular sea
        for x in (0.0, 12.3, -4.1):
            th2 = 2 * (k * x - REG_OMEGA * t + 0.7)
            if min(abs(np.cos(th2)), abs(np.sin(th2))) > 0.2:  # 2 theta away from the multiples of pi / 2: both parts and both signs count
                states.append((t, x, th2 / 2))
    assert len(states) >= 6 and min(s[0] for s in states) <= 0.4 and max(s[0] for s in states) >= 3.7
    for t, x, theta in states:
        got = compare(h, [ref], comp, t, positions(1, x), f"regular nq={nq} t={t} x={x}")[0]
        closed = sr.regular_closed_form(REG_AMP, theta, Pww, Qww)
        assert np.all(np.abs(got - closed) <= bound), (t, x)  # not ramped
        # the other choices of sign miss by far more than the bound
        c, s = float(np.cos(2 * theta)), float(np.sin(2 * theta))
        P, Q = np.asarray(Pww, dtype=float), np.asarray(Qww, dtype=float)
        for wrong in (P * c + Q * s, -P * c - Q * s, Q * s - P * c, P * c, P):  # a sign of Q, of P, of both; no Q; the drift term's constant
            assert np.any(np.abs(got - REG_AMP ** 2 * wrong) > 1e3 * bound)


def test_regular_wave_on_a_node_and_outside_the_grid(HF):
    h = HF.from_case(sphere_case())
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    k = h.regular_coeffs()[2]
    comp = wk.regular_components(REG_AMP, REG_OMEGA, k, 0.0)
    rng = np.random.default_rng(5)
    P, Q = rng.normal(0, 1e4, (6, 3, 3)), rng.normal(0, 1e4, (6, 3, 3))
    on_node = (np.array([1.0, REG_OMEGA, 3.0]), P, Q)
    h.set_sum_qtf(0, *on_node)
    h.set_sum_mode(1)
    t, x = 3.7, 4.0
    got = compare(h, [sr.PairSum(comp, on_node)], comp, t, positions(1, x), "regular, on a node")[0]
    closed = sr.regular_closed_form(REG_AMP, k * x - REG_OMEGA * t, P[:, 1, 1], Q[:, 1, 1])
    assert np.all(np.abs(got - closed) <= sr.bound(comp, on_node)) and np.abs(got).min() > 1.0
    for grid in ([2.2, 2.6, 3.0], [0.5, 1.0, 2.0]):  # the wave is outside the grid: no part
        h.set_sum_qtf(0, np.array(grid), P, Q)
        assert not h.compute_sum_qtf(t, positions(1, x)).any()


# ------------------------------------------------------------------------------------------------
# 2: irregular waves, both synthesised models, the ramp
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("which", ["sphere", "three"])
def test_irregular_waves_and_the_ramp(HF, which, spectral):
    if which == "sphere":
        case, irreg, lo, hi, N, times = sphere_case(), SPHERE_IRREG, 0.3, 2.5, 1, (-1.0, 0.0, 30.0, 60.0, 77.7)
    else:
        case, irreg, lo, hi, N, times = three_body_case(), THREE_IRREG, 0.6, 3.0, 3, (-1.0, 0.0, 2.5, 5.0, 30.0)
    h = HF.from_case(case)
    h.add_waves_irregular(spectral=spectral, **irreg)
    h.set_sum_mode(1)
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == irreg["nfrequencies"]
    tables = [sr.random_table(33, 40, lo, hi)]  # general: neither symmetric nor antisymmetric
    if N == 3:
        tables += [tables[0], sr.random_table(33, 42, lo + 0.1, hi - 0.2)]  # bodies 0 and 1 share a table, 15 m apart
    inside = sr.cells(tables[0][0], comp[1])[0]
    assert 10 < inside.sum() < inside.size - 10 and not inside[0] and not inside[-1]
    refs = []
    for b, tb in enumerate(tables):
        refs.append(refs[0] if b == 1 else sr.PairSum(comp, tb))
    pos = positions(N, 15.0 * np.arange(N) + 3.25)  # displaced in x
    for with_q in (True, False):
        for b, tb in enumerate(tables):
            h.set_sum_qtf(b, tb[0], tb[1], tb[2] if with_q else None)
        use = refs if with_q else [without_q(r) for r in refs]
        got = {}
        for t in times:  # before, inside, at the end of and after the ramp
            ramp = sr.ramp_factor(t, irreg["ramp_duration"])
            got[t] = compare(h, use, comp, t, pos, f"{which} spectral={spectral} Q={with_q} t={t}", ramp=ramp)
        assert sr.ramp_factor(times[2], irreg["ramp_duration"]) == 0.5 and sr.ramp_factor(times[3], irreg["ramp_duration"]) == 1.0
        assert not got[times[0]].any() and not got[times[1]].any() and np.abs(got[times[4]]).max() > 1.0
        if N == 3:  # the same table at another x: another force
            assert not np.allclose(got[times[4]][0], got[times[4]][1], rtol=1e-3)
        else:
            assert not np.allclose(h.compute_sum_qtf(times[4], positions(1, 18.25)), got[times[4]][0], rtol=1e-3)


# ------------------------------------------------------------------------------------------------
# 3: the tile of 256 components and the cap of 256 frequencies
# ------------------------------------------------------------------------------------------------
def edge_grid(nq, w, seed):
    """nq grid points from w[n/8] to w[n - n/8 - 1] (both ends components), half of the interior points components as well"""
    rng = np.random.default_rng(seed)
    lo, hi = w[w.size // 8], w[w.size - w.size // 8 - 1]
    mid = w[(w > lo) & (w < hi)]
    pick = rng.choice(mid, size=min((nq - 2) // 2, mid.size), replace=False)
    g = np.unique(np.concatenate([[lo, hi], pick]))
    while g.size < nq:
        g = np.unique(np.concatenate([g, rng.uniform(lo, hi, size=nq - g.size)]))
    return g


@pytest.mark.parametrize("nf", [255, 256, 257, 513])
def test_tile_and_cap_edges(HF, nf):
    h = HF.from_case(synth_case(1))
    h.add_waves_irregular(**dict(SYNTH_IRREG, nfrequencies=nf))
    h.set_sum_mode(1)
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == nf
    t, pos = 55.5, positions(1, 7.25)
    for nq in (2, 256):
        g = edge_grid(nq, comp[1], 100 + nq)
        inside, m, lam = sr.cells(g, comp[1])
        assert g.size == nq and inside.sum() >= nf - 2 * (nf // 8) and (lam[inside] == 0.0).sum() >= min(nq // 2, 2)  # components on nodes
        rng = np.random.default_rng(nq)
        table = (g, rng.normal(0, 1e4, (6, nq, nq)), rng.normal(0, 1e4, (6, nq, nq)))
        h.set_sum_qtf(0, *table)
        assert h.sum_qtf_size(0) == nq
        ref = sr.PairSum(comp, table)
        got = compare(h, [ref], comp, t, pos, f"nf={nf} nq={nq}")[0]
        assert np.abs(got).max() > 1.0
        # Q = None is Q = 0
        h.set_sum_qtf(0, g, table[1])
        compare(h, [without_q(ref)], comp, t, pos, f"nf={nf} nq={nq} Q=None")
        if nq == 2:
            # a grid that holds no component: zeros, and the next table is evaluated as before (the pointers stayed valid)
            h.set_sum_qtf(0, np.array([50.0, 60.0]), table[1], table[2])
            assert not h.compute_sum_qtf(t, pos).any()
            h.set_sum_qtf(0, *table)
            assert same_bits(h.compute_sum_qtf(t, pos), got)
            # an antisymmetric table: zero within its bound
            anti = (g, table[1] - table[1].transpose(0, 2, 1), table[2] - table[2].transpose(0, 2, 1))
            h.set_sum_qtf(0, *anti)
            assert np.all(np.abs(h.compute_sum_qtf(t, pos)) <= sr.bound(comp, anti))


# ------------------------------------------------------------------------------------------------
# 4: invariance, bitwise
# ------------------------------------------------------------------------------------------------
def test_a_bodys_bits_are_its_own(HF):
    from hydrochrono_amd.hydro import HydroGroup
    table, other = sr.random_table(33, 60, 0.3, 3.0), sr.random_table(64, 61, 0.2, 3.5)
    t, x = 33.0, 41.5
    rows = {}
    for N in (1, 3, 8):
        h = HF.from_case(synth_case(N))
        h.add_waves_irregular(**SYNTH_IRREG)
        h.set_sum_mode(1)
        body = N - 1
        h.set_sum_qtf(body, *table)
        if N > 1:
            h.set_sum_qtf(0, *other)
        pos = positions(N, 3.0 * np.arange(N))
        pos[body, 0] = x
        rows[N] = h.compute_sum_qtf(t, pos).reshape(N, 6)[body]
        assert rows[N].any() and same_bits(rows[N], rows[1])
        assert same_bits(h.compute_sum_qtf(t, pos).reshape(N, 6)[body], rows[1])  # a repeat
        if N != 3:
            continue
        # another body's table and grid replaced, then cleared; the mode there and back; y, z of this body and x of the others moved
        ref = rows[1]
        h.set_sum_qtf(0, *sr.random_table(5, 62, 0.4, 2.0))
        a = h.compute_sum_qtf(t, pos).reshape(3, 6)
        assert same_bits(a[2], ref) and a[0].any() and not a[1].any()
        h.set_sum_qtf(0, [], None)
        a = h.compute_sum_qtf(t, pos).reshape(3, 6)
        assert same_bits(a[2], ref) and not a[0].any() and h.sum_qtf_size(0) == 0
        h.set_sum_mode(0)
        assert not h.compute_sum_qtf(t, pos).any()
        h.set_sum_mode(1)
        assert same_bits(h.compute_sum_qtf(t, pos).reshape(3, 6)[2], ref)
        moved = pos.copy()
        moved[2, 1:] = [17.0, -6.5]
        moved[:2, 0] += 0.37
        assert same_bits(h.compute_sum_qtf(t, moved).reshape(3, 6)[2], ref)
        moved[2, 0] += 1e-3
        assert not same_bits(h.compute_sum_qtf(t, moved).reshape(3, 6)[2], ref)
        # a drift table on the same body changes nothing here
        h.set_drift_qtf(2, *other)
        h.set_drift_mode(3)
        assert same_bits(h.compute_sum_qtf(t, pos).reshape(3, 6)[2], ref)
        # a shard context that owns the body alone, and a group of two shards
        h.set_sum_qtf(0, *other)
        whole = h.compute_sum_qtf(t, pos)
        sh = HF.from_case(synth_case(3), body_range=(2, 3))
        grp = HydroGroup.from_case(synth_case(3), 2)
        for g in (sh, grp):
            g.add_waves_irregular(**SYNTH_IRREG)
            g.set_sum_qtf(0, *other)
            g.set_sum_qtf(2, *table)
            g.set_sum_mode(1)
        assert same_bits(sh.compute_sum_qtf(t, pos), ref)
        assert same_bits(grp.compute_sum_qtf(t, pos), whole) and grp.sum_qtf_size(2) == 33


# ------------------------------------------------------------------------------------------------
# 5: nothing else moves; composition one layer up
# ------------------------------------------------------------------------------------------------
def raw_step(h, t, state):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def test_nothing_else_moves_and_the_layers_compose(HF, monkeypatch):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    sums = [sr.random_table(9, 70, 0.6, 3.0), None, sr.random_table(33, 72, 0.7, 2.8)]
    drifts = [None, sr.random_table(17, 73, 0.6, 3.0), sr.random_table(9, 74, 0.7, 2.8)]
    rng = np.random.default_rng(9)
    elems = (rng.uniform(-5, 5, (12, 3)), rng.uniform(0, 3, (12, 3)), rng.uniform(0, 4, (12, 3)))
    # a: every term through step(); b: the same tables, queried term by term; prev: as a without the sum tables (the layers before);
    # off: sum tables set, mode 0
    a, b, prev, off = (HF.from_case(case) for _ in range(4))
    grp, gprev = HydroGroup.from_case(case, 3), HydroGroup.from_case(case, 3)
    every = (a, b, prev, off, grp, gprev)
    for h in every:
        h.add_waves_irregular(**THREE_IRREG)
        for k, tb in enumerate(drifts):
            if tb is not None:
                h.set_drift_qtf(k, *tb)
        h.set_drift_mode(3)
    for h in (a, b, off, grp):
        for k, tb in enumerate(sums):
            if tb is not None:
                h.set_sum_qtf(k, *tb)
    for h in (a, b, grp):
        h.set_sum_mode(1)
    for h in (a, b, prev, off):
        h.set_morison_elements(1, *elems)  # another side term beside it
    assert not a.sum_qtf().any() and not grp.sum_qtf().any()
    calls = []
    lib = a.lib
    for name in ("hc_sum_qtf_begin", "hc_sum_qtf_end", "hc_compute_sum_qtf"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *args, _fn=fn, _name=name: (calls.append((_name, args[0])), _fn(*args))[1])
    count = lambda h: sum(1 for _, ctx in calls if ctx == h.ctx)
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)
    for n in range(30):
        t = 0.01 * n + 2.0  # inside the ramp of 5 s
        st = motion.state(t)
        n_a, n_off, n_prev = count(a), count(off), count(prev)
        fa = a.step(t, *st)
        assert count(a) == n_a + 2  # one begin, one end
        total, mor, dft = raw_step(b, t, st), b.compute_morison(t, *st), b.compute_drift(t, st[0])
        smf = b.compute_sum_qtf(t, st[0])
        fprev, foff = prev.step(t, *st), off.step(t, *st)
        assert count(off) == n_off and count(prev) == n_prev  # mode 0, no table: no hc_sum_qtf_* call
        assert same_bits(fprev, total + mor + dft) and same_bits(foff, fprev)  # what the layers returned before
        assert same_bits(fa, fprev + smf) and same_bits(a.sum_qtf(), smf) and same_bits(a.drift(), dft) and same_bits(a.morison(), mor)
        assert same_bits(grp.step(t, *st), gprev.step(t, *st) + smf) and same_bits(grp.sum_qtf(), smf)
        # the C ABI's own results do not see the term, whether it is on (a), off (off) or absent (prev)
        comps = [h.components() for h in (a, off, prev)]
        assert all(same_bits(x, y) for c in comps[1:] for x, y in zip(c, comps[0]))
        if n % 10 == 0:
            for mode in (1, 2, 3):
                vals = []
                for h in (a, off, prev):
                    h.set_drift_mode(mode)
                    vals.append(h.compute_drift(t, st[0]))
                    h.set_drift_mode(3)
                assert vals[0].any() and same_bits(vals[0], vals[1]) and same_bits(vals[0], vals[2]), mode
    assert smf.reshape(3, 6)[[0, 2]].any(axis=1).all() and not smf.reshape(3, 6)[1].any() and not prev.sum_qtf().any() and not off.sum_qtf().any()
    # the mode switched off, then the tables cleared: step() is what it was before, with no call
    for t, switch in ((2.5, "mode"), (2.6, "tables")):
        st = motion.state(t)
        if switch == "mode":
            a.set_sum_mode(0)
        else:
            a.set_sum_mode(1)
            for k in (0, 2):
                a.set_sum_qtf(k, [], None)
        n_a = count(a)
        assert same_bits(a.step(t, *st), prev.step(t, *st)) and not a.sum_qtf().any() and count(a) == n_a, switch
    for k, tb in enumerate(sums):
        if tb is not None:
            a.set_sum_qtf(k, *tb)
    # the wave model changed mid-run: the bin map is laid out again and the results follow
    other = dict(THREE_IRREG, seed=11, wave_period=6.0)
    fresh = HF.from_case(case)
    for h in (a, fresh):
        h.add_waves_irregular(**other)
    for k, tb in enumerate(sums):
        if tb is not None:
            fresh.set_sum_qtf(k, *tb)
    fresh.set_sum_mode(1)
    comp = wk.irregular_components(a.irreg_spectrum())
    pos = positions(3, 15.0 * np.arange(3))
    refs = [None if tb is None else sr.PairSum(comp, tb) for tb in sums]
    got = compare(a, refs, comp, 30.0, pos, "after a change of the wave model")
    assert same_bits(got.reshape(-1), fresh.compute_sum_qtf(30.0, pos)) and not same_bits(got.reshape(-1), b.compute_sum_qtf(30.0, pos))


# ------------------------------------------------------------------------------------------------
# 6: against the second-order sea: two independent kernels
# ------------------------------------------------------------------------------------------------
def test_sum_band_of_eta2_is_the_term_on_a_quarter_of_kp(HF):
    """Omega = the component frequencies (W is the identity), every row of P = 1/4 K+ of hc_wave_kinematics2, Q = None: the term is
    the sum-frequency band of eta2 at the body's x."""
    h = HF.from_case(three_body_case())
    irreg = dict(THREE_IRREG, nfrequencies=64)
    h.add_waves_irregular(**irreg)
    comp = wk.irregular_components(h.irreg_spectrum())
    nf = comp[0].size
    assert nf == 64 and np.all(np.diff(comp[1]) > 0)
    assert np.array_equal(sr.weights(comp[1], comp[1]), np.eye(nf))
    Kp = h.wave_pair_tables()["Kp"]
    table = (comp[1], np.broadcast_to(0.25 * Kp, (6, nf, nf)).copy(), None)
    for b in range(3):
        h.set_sum_qtf(b, *table)
    h.set_sum_mode(1)
    _, g, depth = h.simulation_parameters()
    no_diff = (1e9, float("inf"))  # above every difference frequency
    pos = positions(3, np.array([-37.5, 4.0, 61.25]))
    pts = np.stack([pos[:, 0], np.zeros(3), np.zeros(3)], axis=1)
    times = np.array([5.0, 17.3, 33.1])  # at the end of the ramp and past it
    eta2 = h.wave_kinematics2(pts, times, diff_band=no_diff)[0]  # [T][P]
    _, scales = w2.fields(comp, g, depth, pts, times, diff_band=no_diff, ramp_duration=irreg["ramp_duration"])
    bound = sr.bound(comp, table)
    assert np.abs(eta2).max() > 1e-4
    for j, t in enumerate(times):
        got = h.compute_sum_qtf(t, pos).reshape(3, 6)
        for b in range(3):
            tol = bound + WAVE2_TOL * float(scales[0][j, b])
            err = np.abs(got[b] - eta2[j, b])
            print(f"t={t} body {b}: eta2 = {eta2[j, b]:.6e}, worst |term - eta2| / tolerance = {float(np.max(err / tol)):.3e}")
            assert np.all(err <= tol), (t, b)
            assert same_bits(got[b], np.full(6, got[b][0]))  # six equal rows


# ------------------------------------------------------------------------------------------------
# 7: the C++ mirror, several bodies and shards
# ------------------------------------------------------------------------------------------------
def cpp_tables():
    """the tables tests/cpp/sumfreq_caller.cpp builds"""
    d, m, n = np.meshgrid(np.arange(6.0), np.arange(3.0), np.arange(3.0), indexing="ij")
    P, Q, P3 = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n, 500.0 * (m + n) + 62.5 * d, -750.0 * (d + 1) + 50.0 * m * n
    return np.array([0.4, 0.55, 0.9]), P, Q, P3


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "sumfreq_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "sumfreq_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "three_body.h5")
    outputs = []
    for shards in ("1", "2", "3"):
        r = subprocess.run([exe, h5, shards], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (shards, r.returncode, r.stderr)
        outputs.append(r.stdout)
    assert outputs[0] and outputs[1] == outputs[0] and outputs[2] == outputs[0]  # identical text whatever the shards
    rows = np.array([[float(v) for v in line.split()] for line in outputs[0].strip().splitlines()])
    assert rows.shape == (24, 1 + 36 + 18 + 18)
    omega, P, Q, P3 = cpp_tables()
    h = HF(3)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(REG_AMP, 0.6, num_bodies=3)  # inside the BEM frequencies of the file
    h.set_sum_options(regular_phase=0.3)
    h.set_sum_qtf(0, omega, P, Q)
    h.set_sum_qtf(2, omega, P3)
    h.set_sum_mode(1)
    h.set_drift_options(regular_phase=0.3)
    h.set_drift_qtf(1, omega, P)
    h.set_drift_mode(3)
    for row in rows:
        t, state = row[0], row[1:37].reshape(3, 4, 3)
        st = tuple(np.ascontiguousarray(state[:, k, :]).reshape(-1) for k in range(4))
        total, dft, smf = raw_step(h, t, st), h.compute_drift(t, st[0]), h.compute_sum_qtf(t, st[0])
        assert same_bits(row[55:73], smf) and same_bits(row[37:55], total + dft + smf), t
    s6 = rows[:, 55:73].reshape(-1, 3, 6)
    assert np.abs(s6[:, [0, 2]]).max(axis=2).min() > 1.0 and not s6[:, 1].any()
    assert not np.allclose(s6[0, 0], s6[23, 0], rtol=1e-3)  # it oscillates


# ------------------------------------------------------------------------------------------------
# 8: no components, no force
# ------------------------------------------------------------------------------------------------
def test_zero_cases(HF):
    h = HF.from_case(three_body_case())
    table = sr.random_table(9, 80, 0.6, 3.0)
    h.set_sum_qtf(1, *table)
    h.set_sum_mode(1)
    pos = positions(3, 15.0 * np.arange(3))
    rec_t = 0.05 * np.arange(400)
    for model in ("none", "nowave", "eta_record", "none_after_irregular"):
        if model == "nowave":
            h.add_waves_none()
        elif model == "eta_record":
            h.add_waves_irregular_eta(rec_t, 0.5 * np.sin(0.8 * rec_t), 0.05)
        elif model == "none_after_irregular":
            h.add_waves_irregular(**THREE_IRREG)
            got = h.compute_sum_qtf(30.0, pos).reshape(3, 6)
            assert got[1].any() and not got[0].any() and not got[2].any()  # a body without a table
            h.set_sum_mode(0)
            assert not h.compute_sum_qtf(30.0, pos).any()  # mode 0
            h.set_sum_mode(1)
            h.set_sum_qtf(1, [], None)
            assert not h.compute_sum_qtf(30.0, pos).any() and h.sum_qtf_size(1) == 0  # a cleared table
            h.set_sum_qtf(1, *table)
            assert h.compute_sum_qtf(30.0, pos).any()
            h.add_waves_none()
        out = h.compute_sum_qtf(30.0, pos)
        assert out.shape == (18,) and not out.any(), model


# ------------------------------------------------------------------------------------------------
# 9: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    from hydrochrono_amd import capi
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    z9, out = np.zeros(9), np.full(18, 7.0)
    g3 = np.array([0.2, 0.4, 0.8])  # inside the BEM frequencies of the case
    P3, Q3 = np.full(54, 100.0), np.zeros(54)

    # before hc_finalize: a table may be set, nothing can be computed
    raw = HF(3)
    lib = raw.lib
    assert lib.hc_set_sum_qtf(raw.ctx, 0, 3, dp(g3), dp(P3), None) == OK
    assert lib.hc_sum_qtf_begin(raw.ctx, 0.0, dp(z9)) == INV
    assert lib.hc_compute_sum_qtf(raw.ctx, 0.0, dp(z9), dp(out)) == INV
    assert lib.hc_sum_qtf_end(raw.ctx, dp(out)) == INV  # nothing stayed pending
    raw.close()

    h = HF.from_case(case)
    h.add_waves_regular(0.5, 0.4)  # on the middle node, theta = 0 at t = 0, x = 0: A^2 P = 25
    n = C.c_int(-1)

    def good():
        assert lib.hc_set_sum_qtf(h.ctx, 0, 3, dp(g3), dp(P3), dp(Q3)) == OK and lib.hc_set_sum_mode(h.ctx, 1) == OK
        assert lib.hc_compute_sum_qtf(h.ctx, 0.0, dp(z9), dp(out)) == OK
        assert np.allclose(out[:6], 25.0, rtol=1e-12) and not out[6:].any()

    # no table: zeros, and begin / end still pair up
    assert lib.hc_set_sum_mode(h.ctx, 1) == OK
    assert lib.hc_compute_sum_qtf(h.ctx, 0.0, dp(z9), dp(out)) == OK and not out.any()
    good()
    # bad body
    for body in (-1, 3, 100):
        assert lib.hc_set_sum_qtf(h.ctx, body, 3, dp(g3), dp(P3), None) == INV
        assert lib.hc_get_sum_qtf_size(h.ctx, body, C.byref(n)) == INV
    assert lib.hc_get_sum_qtf_size(h.ctx, 0, None) == INV
    good()
    # bad nq, null grid or P
    big = np.arange(1.0, 258.0)
    Pbig = np.zeros(6 * 257 * 257)
    for nq in (1, -1, -7):
        assert lib.hc_set_sum_qtf(h.ctx, 0, nq, dp(g3), dp(P3), None) == INV
    assert lib.hc_set_sum_qtf(h.ctx, 0, 257, dp(big), dp(Pbig), None) == INV
    assert lib.hc_set_sum_qtf(h.ctx, 1, 256, dp(big), dp(Pbig), None) == OK  # the cap itself is allowed
    assert lib.hc_set_sum_qtf(h.ctx, 1, 0, None, None, None) == OK
    assert lib.hc_set_sum_qtf(h.ctx, 0, 3, None, dp(P3), None) == INV
    assert lib.hc_set_sum_qtf(h.ctx, 0, 3, dp(g3), None, dp(Q3)) == INV
    assert lib.hc_get_sum_qtf_size(h.ctx, 0, C.byref(n)) == OK and n.value == 3  # a refused table leaves the one before
    good()
    # non-finite values, a grid that does not increase strictly
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            arrs = [g3.copy(), P3.copy(), Q3.copy()]
            arrs[k][1] = bad
            assert lib.hc_set_sum_qtf(h.ctx, 0, 3, *[dp(x) for x in arrs]) == INV
    for grid in ([0.6, 0.6, 3.0], [0.6, 3.0, 1.4], [3.0, 1.4, 0.6]):
        assert lib.hc_set_sum_qtf(h.ctx, 0, 3, dp(np.array(grid)), dp(P3), None) == INV
    assert b"sum-frequency" in lib.hc_last_error(h.ctx)
    good()
    # mode, options
    for mode in (-1, 2, 100):
        assert lib.hc_set_sum_mode(h.ctx, mode) == INV
    assert lib.hc_get_sum_mode(h.ctx, C.byref(n)) == OK and n.value == 1
    assert lib.hc_get_sum_mode(h.ctx, None) == INV
    for o in (capi.WaveKinematicsOpts(0.0, np.inf, 1), capi.WaveKinematicsOpts(0.0, np.nan, 1)):
        assert lib.hc_set_sum_options(h.ctx, C.byref(o)) == INV
    assert lib.hc_set_sum_options(h.ctx, None) == OK
    good()
    # end without begin, begin twice, no setter while one is pending, exactly one end per begin; the drift calls are another path
    assert lib.hc_sum_qtf_end(h.ctx, dp(out)) == INV
    assert lib.hc_sum_qtf_begin(h.ctx, 0.0, dp(z9)) == OK
    assert lib.hc_sum_qtf_begin(h.ctx, 0.0, dp(z9)) == INV
    assert lib.hc_set_sum_qtf(h.ctx, 1, 3, dp(g3), dp(P3), None) == INV
    assert lib.hc_set_sum_mode(h.ctx, 0) == INV
    assert lib.hc_set_sum_options(h.ctx, None) == INV
    assert lib.hc_drift_end(h.ctx, dp(out)) == INV and lib.hc_set_drift_qtf(h.ctx, 1, 3, dp(g3), dp(P3), None) == OK
    assert lib.hc_sum_qtf_end(h.ctx, dp(out)) == OK and np.allclose(out[:6], 25.0, rtol=1e-12)
    assert lib.hc_sum_qtf_end(h.ctx, dp(out)) == INV
    good()
    # non-finite time or position: refused, nothing pending afterwards
    for bad in (np.nan, np.inf, -np.inf):
        p = z9.copy()
        p[4] = bad
        assert lib.hc_sum_qtf_begin(h.ctx, 0.0, dp(p)) == INV
        assert lib.hc_sum_qtf_end(h.ctx, dp(out)) == INV
        assert lib.hc_compute_sum_qtf(h.ctx, bad, dp(z9), dp(out)) == INV
        assert lib.hc_sum_qtf_end(h.ctx, dp(out)) == INV
    assert lib.hc_sum_qtf_begin(h.ctx, 0.0, None) == INV
    good()
    # a null output ends the evaluation all the same
    assert lib.hc_sum_qtf_begin(h.ctx, 0.0, dp(z9)) == OK
    assert lib.hc_sum_qtf_end(h.ctx, None) == INV
    assert lib.hc_sum_qtf_end(h.ctx, dp(out)) == INV
    good()
    # a shard context takes the tables of all bodies and computes its own
    sh = HF.from_case(case, body_range=(1, 2))
    sh.add_waves_regular(0.5, 0.4)
    for b in range(3):
        assert lib.hc_set_sum_qtf(sh.ctx, b, 3, dp(g3), dp(P3 * (b + 1)), None) == OK
    assert lib.hc_set_sum_mode(sh.ctx, 1) == OK
    o6 = np.empty(6)
    assert lib.hc_compute_sum_qtf(sh.ctx, 0.0, dp(z9), dp(o6)) == OK and np.allclose(o6, 50.0, rtol=1e-12)
    # the Python layer refuses what it can see
    with pytest.raises(ValueError):
        h.set_sum_qtf(0, g3, np.zeros((6, 3, 2)))
    with pytest.raises(Exception):
        h.set_sum_mode(2)


# ------------------------------------------------------------------------------------------------
# 10: the drift and the sum-frequency term are two instances of one implementation: neither sees the other's tables, mode, options,
#     stream or staging, also while the other is pending
# ------------------------------------------------------------------------------------------------
def test_the_two_qtf_terms_share_nothing(HF):
    from hydrochrono_amd import capi
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(capi.c_double_p))
    h = HF.from_case(synth_case(2))
    h.add_waves_irregular(spectral=True, **dict(SYNTH_IRREG, nfrequencies=257))  # one full tile of components plus one
    lib, ctx = h.lib, h.ctx
    omega = wk.irregular_components(h.irreg_spectrum())[1]
    assert omega.size == 257

    def table(nq, lo, hi, seed):
        rng = np.random.default_rng(seed)
        g = np.linspace(lo, hi, nq)
        assert np.count_nonzero((omega >= g[0]) & (omega <= g[-1])) > 20
        return nq, g, rng.normal(0, 1e4, (6, nq, nq)), rng.normal(0, 1e4, (6, nq, nq))

    def set_table(setter, body, tb, status=OK):
        nq, g, P, Q = tb
        keep = (np.ascontiguousarray(g), np.ascontiguousarray(P), np.ascontiguousarray(Q))
        assert setter(ctx, body, nq, *[dp(a) for a in keep]) == status

    drift_tabs = [table(3, 0.3, 3.0, 1), table(5, 0.4, 3.3, 2)]
    drift_new0 = table(4, 0.5, 2.8, 3)
    sum_tabs = [table(5, 0.5, 3.5, 4), table(2, 0.2, 3.7, 5)]
    sum_new0 = table(4, 0.45, 3.2, 6)
    t, pos = 12.5, positions(2, [0.0, 30.0]).reshape(-1)  # inside the ramp
    phase = [capi.WaveKinematicsOpts(0.0, v, 1) for v in (0.9, 1.7)]

    def alone(compute):
        out = np.full(12, 7.0)
        assert compute(ctx, t, dp(pos), dp(out)) == OK and np.all(np.isfinite(out)) and out[:6].any() and out[6:].any()
        return out

    # each term alone, with the tables before and after the change that is made below while the other term is pending
    for b in range(2):
        set_table(lib.hc_set_drift_qtf, b, drift_tabs[b])
        set_table(lib.hc_set_sum_qtf, b, sum_tabs[b])
    assert lib.hc_set_drift_mode(ctx, 3) == OK and lib.hc_set_sum_mode(ctx, 1) == OK
    drift_alone, sum_alone = alone(lib.hc_compute_drift), alone(lib.hc_compute_sum_qtf)
    set_table(lib.hc_set_drift_qtf, 0, drift_new0)
    set_table(lib.hc_set_sum_qtf, 0, sum_new0)
    drift_alone_new, sum_alone_new = alone(lib.hc_compute_drift), alone(lib.hc_compute_sum_qtf)
    assert same_bits(drift_alone[6:], drift_alone_new[6:]) and not np.allclose(drift_alone[:6], drift_alone_new[:6], rtol=1e-3)
    assert same_bits(sum_alone[6:], sum_alone_new[6:]) and not np.allclose(sum_alone[:6], sum_alone_new[:6], rtol=1e-3)
    assert not np.allclose(drift_alone, sum_alone, rtol=1e-3)

    # drift pending: every setter of the sum term succeeds, every setter of the drift term is refused as before
    set_table(lib.hc_set_drift_qtf, 0, drift_tabs[0])
    set_table(lib.hc_set_sum_qtf, 0, sum_tabs[0])
    assert lib.hc_set_sum_mode(ctx, 0) == OK
    d_out, s_out = np.full(12, 7.0), np.full(12, 7.0)
    assert lib.hc_drift_begin(ctx, t, dp(pos)) == OK
    set_table(lib.hc_set_sum_qtf, 0, sum_new0)
    assert lib.hc_set_sum_mode(ctx, 1) == OK
    assert lib.hc_set_sum_options(ctx, C.byref(phase[0])) == OK
    set_table(lib.hc_set_drift_qtf, 0, drift_new0, INV)
    assert b"a drift evaluation is in flight" in lib.hc_last_error(ctx)
    assert lib.hc_set_drift_mode(ctx, 1) == INV and lib.hc_set_drift_options(ctx, C.byref(phase[0])) == INV
    assert lib.hc_drift_begin(ctx, t, dp(pos)) == INV
    assert lib.hc_sum_qtf_begin(ctx, t, dp(pos)) == OK
    assert lib.hc_drift_end(ctx, dp(d_out)) == OK
    assert lib.hc_sum_qtf_end(ctx, dp(s_out)) == OK
    assert same_bits(d_out, drift_alone) and same_bits(s_out, sum_alone_new)

    # the mirror image: sum pending, a drift table, the drift mode and the drift options change
    assert lib.hc_set_drift_mode(ctx, 0) == OK
    d_out, s_out = np.full(12, 7.0), np.full(12, 7.0)
    assert lib.hc_sum_qtf_begin(ctx, t, dp(pos)) == OK
    set_table(lib.hc_set_drift_qtf, 0, drift_new0)
    assert lib.hc_set_drift_mode(ctx, 3) == OK
    assert lib.hc_set_drift_options(ctx, C.byref(phase[1])) == OK
    set_table(lib.hc_set_sum_qtf, 0, sum_tabs[0], INV)
    assert b"a sum-frequency evaluation is in flight" in lib.hc_last_error(ctx)
    assert lib.hc_set_sum_mode(ctx, 0) == INV and lib.hc_set_sum_options(ctx, C.byref(phase[1])) == INV
    assert lib.hc_sum_qtf_begin(ctx, t, dp(pos)) == INV
    assert lib.hc_drift_begin(ctx, t, dp(pos)) == OK
    assert lib.hc_sum_qtf_end(ctx, dp(s_out)) == OK
    assert lib.hc_drift_end(ctx, dp(d_out)) == OK
    assert same_bits(s_out, sum_alone_new) and same_bits(d_out, drift_alone_new)
    h.close()
