"""Second-order wave drift forces on the GPU (hc_set_drift_qtf, hc_drift_begin / hc_drift_end, hc_compute_drift; csrc/hc_qtf.hip)
against the direct longdouble pair sum of the definition (tests/drift_ref.py), fed the context's own spectrum / regular-wave
coefficients.  The device evaluates the projected O(nf + nq^2) form, so the identity between the two is under test as well.

Tolerance: the bound drift_ref derives per body and row, ramp^2 (2 * 1e-11 + (nf + nq^2 + 64) 2^-52) M_d, M_d twice the sum of the
absolute pair terms (its docstring has the derivation).  Every case keeps |theta_i| < 1e4; the reference asserts it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import drift_ref as dr
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
MODES = (1, 2, 3)


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


def compare(h, refs, comp, t, pos, what, ramp=1.0, modes=MODES):
    """GPU against the pair sum for every mode, inside the derived bound.  refs: per body None or a drift_ref.PairSum.  Returns
    {mode: [N][6]}."""
    out = {}
    for mode in modes:
        h.set_drift_mode(mode)
        got = h.compute_drift(t, pos).reshape(-1, 6)
        assert np.all(np.isfinite(got)), what
        for b, ref in enumerate(refs):
            if ref is None:
                assert not got[b].any(), (what, mode, b)
                continue
            want, bound = ref.force(t, pos[b, 0], ramp=ramp)[mode], dr.bounds(comp, ref.table, ramp=ramp)[mode]
            err = np.abs(got[b] - want)
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            print(f"{what} mode {mode} body {b}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(want)):.3e}")
            assert np.all(err <= bound), f"{what} mode {mode} body {b}: worst {worst:.3e} of the bound"
        out[mode] = got
    return out


# ------------------------------------------------------------------------------------------------
# 1: a regular wave on the sphere
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [[1.5, 2.9], [0.7, 1.5, 2.0, 2.5, 3.3]])
def test_regular_wave_is_constant_a2_t(HF, grid):
    h = HF.from_case(sphere_case())
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    h.set_drift_options(regular_phase=0.7)
    comp = wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.7)
    nq = len(grid)
    rng = np.random.default_rng(nq)
    table = (np.array(grid), rng.normal(0, 1e4, (6, nq, nq)), rng.normal(0, 1e4, (6, nq, nq)))
    h.set_drift_qtf(0, *table)
    assert h.drift_qtf_size(0) == nq
    ref = dr.PairSum(comp, table)
    results = []
    for t in (0.0, 3.7, 41.3):  # not ramped
        for x in (0.0, 12.3):
            results.append(compare(h, [ref], comp, t, positions(1, x), f"regular nq={nq} t={t} x={x}"))
    bound = dr.bounds(comp, table)
    for mode in MODES:  # constant over t and x: two results inside the bound of one value are within twice the bound of each other
        assert np.abs(results[0][mode]).max() > 1.0
        for r in results[1:]:
            assert np.all(np.abs(r[mode] - results[0][mode]) <= 2 * bound[mode])
    # the definition in closed form: A^2 T(w, w), the Q part drops out (sin 0), modes 1 and 2 are A^2 D(w)
    inside, m, lam = dr.cells(table[0], comp[1])
    m, lam, P = int(m[0]), float(lam[0]), table[1]
    D = (1 - lam) * P[:, m, m] + lam * P[:, m + 1, m + 1]
    T = (1 - lam) ** 2 * P[:, m, m] + (1 - lam) * lam * (P[:, m, m + 1] + P[:, m + 1, m]) + lam ** 2 * P[:, m + 1, m + 1]
    assert inside.all()
    for mode, closed in ((1, D), (2, D), (3, T)):
        assert np.all(np.abs(results[0][mode][0] - REG_AMP ** 2 * closed) <= bound[mode])


def test_regular_wave_on_a_node_and_outside_the_grid(HF):
    h = HF.from_case(sphere_case())
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    comp = wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.0)
    rng = np.random.default_rng(5)
    P, Q = rng.normal(0, 1e4, (6, 3, 3)), rng.normal(0, 1e4, (6, 3, 3))
    on_node = (np.array([1.0, REG_OMEGA, 3.0]), P, Q)
    h.set_drift_qtf(0, *on_node)
    got = compare(h, [dr.PairSum(comp, on_node)], comp, 3.7, positions(1, 4.0), "regular, on a node")
    bound = dr.bounds(comp, on_node)
    for mode in (2, 3):  # the three modes are A^2 P[1][1]
        assert np.all(np.abs(got[mode] - got[1]) <= bound[mode] + bound[1])
    assert np.allclose(got[1][0], REG_AMP ** 2 * P[:, 1, 1], rtol=1e-12, atol=0)
    for grid in ([2.2, 2.6, 3.0], [0.5, 1.0, 2.0]):  # the wave is outside the grid: no part in any mode
        h.set_drift_qtf(0, np.array(grid), P, Q)
        for mode in MODES:
            h.set_drift_mode(mode)
            assert not h.compute_drift(3.7, positions(1, 4.0)).any()


# ------------------------------------------------------------------------------------------------
# 2: irregular waves, both synthesised models, the ramp
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("which", ["sphere", "three"])
def test_irregular_waves_all_modes_and_the_ramp(HF, which, spectral):
    if which == "sphere":
        case, irreg, lo, hi, N = sphere_case(), SPHERE_IRREG, 0.3, 2.5, 1
    else:
        case, irreg, lo, hi, N = three_body_case(), THREE_IRREG, 0.6, 3.0, 3
    h = HF.from_case(case)
    h.add_waves_irregular(spectral=spectral, **irreg)
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == irreg["nfrequencies"]
    tables = [dr.random_table(33, 40, lo, hi)]  # general: neither symmetric nor antisymmetric
    if N == 3:
        tables += [tables[0], dr.random_table(33, 42, lo + 0.1, hi - 0.2)]  # bodies 0 and 1 share a table, 15 m apart
    inside = dr.cells(tables[0][0], comp[1])[0]
    assert 10 < inside.sum() < inside.size - 10 and not inside[0] and not inside[-1]
    refs = []
    for b, tb in enumerate(tables):
        h.set_drift_qtf(b, *tb)
        refs.append(refs[0] if b == 1 else dr.PairSum(comp, tb))
    got = {}
    for t in (-1.0, 0.0, 30.0, 77.7, 431.25):  # before, inside and after the ramp
        ramp = dr.ramp_factor(t, irreg["ramp_duration"])
        got[t] = compare(h, refs, comp, t, positions(N, 15.0 * np.arange(N)), f"{which} spectral={spectral} t={t}", ramp=ramp)
    for mode in MODES:
        assert not got[-1.0][mode].any() and not got[0.0][mode].any() and np.abs(got[77.7][mode]).max() > 1.0
    if N == 3:  # the same table at another x: another force (the mean drift of mode 1 does not see x)
        assert not np.allclose(got[77.7][3][0], got[77.7][3][1], rtol=1e-3) and same_bits(got[77.7][1][0], got[77.7][1][1])
    else:
        h.set_drift_mode(3)
        assert not np.allclose(h.compute_drift(77.7, positions(1, 15.0)), got[77.7][3][0], rtol=1e-3)


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
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == nf
    t, pos = 55.5, positions(1, 7.25)
    for nq in (2, 3, 64, 256):
        g = edge_grid(nq, comp[1], 100 + nq)
        inside, m, lam = dr.cells(g, comp[1])
        assert g.size == nq and inside.sum() >= nf - 2 * (nf // 8) and (lam[inside] == 0.0).sum() >= min(nq // 2, 2)  # components on nodes
        rng = np.random.default_rng(nq)
        table = (g, rng.normal(0, 1e4, (6, nq, nq)), rng.normal(0, 1e4, (6, nq, nq)))
        h.set_drift_qtf(0, *table)
        assert h.drift_qtf_size(0) == nq
        compare(h, [dr.PairSum(comp, table)], comp, t, pos, f"nf={nf} nq={nq}")
        if nq == 3:
            # P = 0, Q antisymmetric: the force is -sum Q_ij A_i A_j sin(theta_i - theta_j) alone
            Qa = table[2] - table[2].transpose(0, 2, 1)
            anti = (g, np.zeros((6, nq, nq)), Qa)
            h.set_drift_qtf(0, *anti)
            got = compare(h, [dr.PairSum(comp, anti)], comp, t, pos, f"nf={nf} nq={nq} P=0", modes=(3,))[3][0]
            want, bound = dr.PairSum(comp, anti).force(t, pos[0, 0])[3], dr.bounds(comp, anti)[3]
            strong = np.abs(want) > 100 * bound
            assert strong.any() and np.array_equal(np.sign(got[strong]), np.sign(want[strong]))
            h.set_drift_mode(1)
            assert not h.compute_drift(t, pos).any()  # no diagonal
            # Q = None is Q = 0
            h.set_drift_qtf(0, g, table[1])
            compare(h, [dr.PairSum(comp, (g, table[1], None))], comp, t, pos, f"nf={nf} nq={nq} Q=None", modes=(3,))


# ------------------------------------------------------------------------------------------------
# 4: invariance, bitwise
# ------------------------------------------------------------------------------------------------
def test_a_bodys_bits_are_its_own(HF):
    from hydrochrono_amd.hydro import HydroGroup
    table, other = dr.random_table(33, 60, 0.3, 3.0), dr.random_table(64, 61, 0.2, 3.5)
    t, x = 33.0, 41.5
    rows = {}
    for N in (1, 3, 8):
        h = HF.from_case(synth_case(N))
        h.add_waves_irregular(**SYNTH_IRREG)
        body = N - 1
        h.set_drift_qtf(body, *table)
        if N > 1:
            h.set_drift_qtf(0, *other)
        pos = positions(N, 3.0 * np.arange(N))
        pos[body, 0] = x
        for mode in MODES:
            h.set_drift_mode(mode)
            rows[(N, mode)] = h.compute_drift(t, pos).reshape(N, 6)[body]
            assert rows[(N, mode)].any() and same_bits(rows[(N, mode)], rows[(1, mode)])
            assert same_bits(h.compute_drift(t, pos).reshape(N, 6)[body], rows[(1, mode)])  # a repeat
        if N != 3:
            continue
        # another body's table replaced, then cleared; the mode there and back; y, z of this body and x of the others moved
        h.set_drift_mode(3)
        ref = rows[(1, 3)]
        h.set_drift_qtf(0, *dr.random_table(5, 62, 0.4, 2.0))
        a = h.compute_drift(t, pos).reshape(3, 6)
        assert same_bits(a[2], ref) and a[0].any() and not a[1].any()
        h.set_drift_qtf(0, [], None)
        a = h.compute_drift(t, pos).reshape(3, 6)
        assert same_bits(a[2], ref) and not a[0].any() and h.drift_qtf_size(0) == 0
        h.set_drift_mode(0)
        assert not h.compute_drift(t, pos).any()
        h.set_drift_mode(1)
        h.set_drift_mode(3)
        assert same_bits(h.compute_drift(t, pos).reshape(3, 6)[2], ref)
        moved = pos.copy()
        moved[2, 1:] = [17.0, -6.5]
        moved[:2, 0] += 0.37
        assert same_bits(h.compute_drift(t, moved).reshape(3, 6)[2], ref)
        moved[2, 0] += 1e-3
        assert not same_bits(h.compute_drift(t, moved).reshape(3, 6)[2], ref)
        # a shard context that owns the body alone, and a group of two shards
        h.set_drift_qtf(0, *other)
        whole = h.compute_drift(t, pos)
        sh = HF.from_case(synth_case(3), body_range=(2, 3))
        grp = HydroGroup.from_case(synth_case(3), 2)
        for g in (sh, grp):
            g.add_waves_irregular(**SYNTH_IRREG)
            g.set_drift_qtf(0, *other)
            g.set_drift_qtf(2, *table)
            g.set_drift_mode(3)
        assert same_bits(sh.compute_drift(t, pos), ref)
        assert same_bits(grp.compute_drift(t, pos), whole)


# ------------------------------------------------------------------------------------------------
# 5: composition one layer up
# ------------------------------------------------------------------------------------------------
def raw_step(h, t, state):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def test_hydroforces_and_hydrogroup_step_compose(HF, monkeypatch):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    tables = [dr.random_table(9, 70, 0.6, 3.0), None, dr.random_table(33, 72, 0.7, 2.8)]
    rng = np.random.default_rng(9)
    elems = (rng.uniform(-5, 5, (12, 3)), rng.uniform(0, 3, (12, 3)), rng.uniform(0, 4, (12, 3)))
    a, b, plain, off = (HF.from_case(case) for _ in range(4))
    grp, gplain = HydroGroup.from_case(case, 3), HydroGroup.from_case(case, 3)
    for h in (a, b, plain, off, grp, gplain):
        h.add_waves_irregular(**THREE_IRREG)
    for h in (a, b, grp, off):
        for k, tb in enumerate(tables):
            if tb is not None:
                h.set_drift_qtf(k, *tb)
    for h in (a, b, grp):
        h.set_drift_mode(3)
    a.set_morison_elements(1, *elems)  # another side term beside it
    b.set_morison_elements(1, *elems)
    assert not a.drift().any() and not grp.drift().any()
    calls = []
    begin = a.lib.hc_drift_begin
    monkeypatch.setattr(a.lib, "hc_drift_begin", lambda *args: (calls.append(args[0]), begin(*args))[1])
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)
    for n in range(40):
        t = 0.01 * n + 2.0  # inside the ramp of 5 s
        st = motion.state(t)
        n_before = len(calls)
        fa = a.step(t, *st)
        assert len(calls) == n_before + 1
        total, mor, dft = raw_step(b, t, st), b.compute_morison(t, *st), b.compute_drift(t, st[0])
        assert same_bits(fa, total + mor + dft) and same_bits(a.drift(), dft) and same_bits(a.morison(), mor)
        n_before = len(calls)
        assert same_bits(total, plain.step(t, *st)) and same_bits(total, off.step(t, *st))  # no table, mode 0: today's calls, today's bits
        assert len(calls) == n_before
        assert same_bits(grp.step(t, *st), gplain.step(t, *st) + dft) and same_bits(grp.drift(), dft)  # hc_step_multi + the shards' terms
    assert dft.reshape(3, 6)[[0, 2]].any(axis=1).all() and not dft.reshape(3, 6)[1].any() and not plain.drift().any() and not off.drift().any()
    # the mode switched off, and the tables cleared: step() is the step plus the Morison term again
    st = motion.state(2.5)
    want = raw_step(b, 2.5, st) + b.compute_morison(2.5, *st)
    a.set_drift_mode(0)
    n_before = len(calls)
    assert same_bits(a.step(2.5, *st), want) and not a.drift().any() and len(calls) == n_before
    a.set_drift_mode(2)
    for k in (0, 2):
        a.set_drift_qtf(k, [], None)
    assert same_bits(a.step(2.5, *st), want) and not a.drift().any() and len(calls) == n_before


def cpp_table():
    """the table tests/cpp/drift_caller.cpp builds"""
    d, m, n = np.meshgrid(np.arange(6.0), np.arange(3.0), np.arange(3.0), indexing="ij")
    P, Q = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n, 500.0 * (m - n) + 62.5 * d
    D = 2000.0 * (d[:, :, 0] + 1) + 125.0 * m[:, :, 0]
    return np.array([1.5, 2.25, 3.0]), P, Q, D


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "drift_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "drift_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (40, 25)
    omega, P, Q, D = cpp_table()
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
    h.set_drift_options(regular_phase=0.3)
    h.set_drift_qtf(0, omega, P, Q)
    h.set_drift_mode(3)
    for n, row in enumerate(rows):
        if n == 20:
            h.set_drift_mean(0, omega, D)
            h.set_drift_mode(2)
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total, dft = raw_step(h, t, st), h.compute_drift(t, st[0])
        assert same_bits(row[19:25], dft) and same_bits(row[13:19], total + dft), t
    assert np.abs(rows[:, 19:25]).min() > 1.0 and not np.allclose(rows[19, 19:25], rows[20, 19:25], rtol=1e-6)


# ------------------------------------------------------------------------------------------------
# 6: no components, no force
# ------------------------------------------------------------------------------------------------
def test_zero_cases(HF):
    h = HF.from_case(three_body_case())
    table = dr.random_table(9, 80, 0.6, 3.0)
    h.set_drift_qtf(1, *table)
    h.set_drift_mode(3)
    pos = positions(3, 15.0 * np.arange(3))
    rec_t = 0.05 * np.arange(400)
    for model in ("none", "nowave", "eta_record", "none_after_irregular"):
        if model == "nowave":
            h.add_waves_none()
        elif model == "eta_record":
            h.add_waves_irregular_eta(rec_t, 0.5 * np.sin(0.8 * rec_t), 0.05)
        elif model == "none_after_irregular":
            h.add_waves_irregular(**THREE_IRREG)
            got = h.compute_drift(30.0, pos).reshape(3, 6)
            assert got[1].any() and not got[0].any() and not got[2].any()  # a body without a table
            h.add_waves_none()
        for mode in MODES:
            h.set_drift_mode(mode)
            out = h.compute_drift(30.0, pos)
            assert out.shape == (18,) and not out.any(), (model, mode)


# ------------------------------------------------------------------------------------------------
# 7: errors
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
    assert lib.hc_set_drift_qtf(raw.ctx, 0, 3, dp(g3), dp(P3), None) == OK
    assert lib.hc_drift_begin(raw.ctx, 0.0, dp(z9)) == INV
    assert lib.hc_compute_drift(raw.ctx, 0.0, dp(z9), dp(out)) == INV
    assert lib.hc_drift_end(raw.ctx, dp(out)) == INV  # nothing stayed pending
    raw.close()

    h = HF.from_case(case)
    h.add_waves_regular(0.5, 0.4)  # on the middle node: A^2 P = 25 in every mode
    n = C.c_int(-1)

    def good():
        assert lib.hc_set_drift_qtf(h.ctx, 0, 3, dp(g3), dp(P3), dp(Q3)) == OK and lib.hc_set_drift_mode(h.ctx, 3) == OK
        assert lib.hc_compute_drift(h.ctx, 0.0, dp(z9), dp(out)) == OK
        assert np.allclose(out[:6], 25.0, rtol=1e-12) and not out[6:].any()

    # no table: zeros, and begin / end still pair up
    assert lib.hc_set_drift_mode(h.ctx, 3) == OK
    assert lib.hc_compute_drift(h.ctx, 0.0, dp(z9), dp(out)) == OK and not out.any()
    good()
    # bad body
    for body in (-1, 3, 100):
        assert lib.hc_set_drift_qtf(h.ctx, body, 3, dp(g3), dp(P3), None) == INV
        assert lib.hc_get_drift_qtf_size(h.ctx, body, C.byref(n)) == INV
    assert lib.hc_get_drift_qtf_size(h.ctx, 0, None) == INV
    good()
    # bad nq, null grid or P
    big = np.arange(1.0, 258.0)
    Pbig = np.zeros(6 * 257 * 257)
    for nq in (1, -1, -7):
        assert lib.hc_set_drift_qtf(h.ctx, 0, nq, dp(g3), dp(P3), None) == INV
    assert lib.hc_set_drift_qtf(h.ctx, 0, 257, dp(big), dp(Pbig), None) == INV
    assert lib.hc_set_drift_qtf(h.ctx, 1, 256, dp(big), dp(Pbig), None) == OK  # the cap itself is allowed
    assert lib.hc_set_drift_qtf(h.ctx, 1, 0, None, None, None) == OK
    assert lib.hc_set_drift_qtf(h.ctx, 0, 3, None, dp(P3), None) == INV
    assert lib.hc_set_drift_qtf(h.ctx, 0, 3, dp(g3), None, dp(Q3)) == INV
    assert lib.hc_get_drift_qtf_size(h.ctx, 0, C.byref(n)) == OK and n.value == 3  # a refused table leaves the one before
    good()
    # non-finite values, a grid that does not increase strictly
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            arrs = [g3.copy(), P3.copy(), Q3.copy()]
            arrs[k][1] = bad
            assert lib.hc_set_drift_qtf(h.ctx, 0, 3, *[dp(x) for x in arrs]) == INV
    for grid in ([0.6, 0.6, 3.0], [0.6, 3.0, 1.4], [3.0, 1.4, 0.6]):
        assert lib.hc_set_drift_qtf(h.ctx, 0, 3, dp(np.array(grid)), dp(P3), None) == INV
    assert b"drift" in lib.hc_last_error(h.ctx)
    good()
    # mode, options
    for mode in (-1, 4, 100):
        assert lib.hc_set_drift_mode(h.ctx, mode) == INV
    assert lib.hc_get_drift_mode(h.ctx, C.byref(n)) == OK and n.value == 3
    assert lib.hc_get_drift_mode(h.ctx, None) == INV
    for o in (capi.WaveKinematicsOpts(0.0, np.inf, 1), capi.WaveKinematicsOpts(0.0, np.nan, 1)):
        assert lib.hc_set_drift_options(h.ctx, C.byref(o)) == INV
    assert lib.hc_set_drift_options(h.ctx, None) == OK
    good()
    # end without begin, begin twice, no setter while one is pending, exactly one end per begin
    assert lib.hc_drift_end(h.ctx, dp(out)) == INV
    assert lib.hc_drift_begin(h.ctx, 0.0, dp(z9)) == OK
    assert lib.hc_drift_begin(h.ctx, 0.0, dp(z9)) == INV
    assert lib.hc_set_drift_qtf(h.ctx, 1, 3, dp(g3), dp(P3), None) == INV
    assert lib.hc_set_drift_mode(h.ctx, 1) == INV
    assert lib.hc_set_drift_options(h.ctx, None) == INV
    assert lib.hc_drift_end(h.ctx, dp(out)) == OK and np.allclose(out[:6], 25.0, rtol=1e-12)
    assert lib.hc_drift_end(h.ctx, dp(out)) == INV
    good()
    # non-finite time or position: refused, nothing pending afterwards
    for bad in (np.nan, np.inf, -np.inf):
        p = z9.copy()
        p[4] = bad
        assert lib.hc_drift_begin(h.ctx, 0.0, dp(p)) == INV
        assert lib.hc_drift_end(h.ctx, dp(out)) == INV
        assert lib.hc_compute_drift(h.ctx, bad, dp(z9), dp(out)) == INV
        assert lib.hc_drift_end(h.ctx, dp(out)) == INV
    assert lib.hc_drift_begin(h.ctx, 0.0, None) == INV
    good()
    # a null output ends the evaluation all the same
    assert lib.hc_drift_begin(h.ctx, 0.0, dp(z9)) == OK
    assert lib.hc_drift_end(h.ctx, None) == INV
    assert lib.hc_drift_end(h.ctx, dp(out)) == INV
    good()
    # a shard context takes the tables of all bodies and computes its own
    sh = HF.from_case(case, body_range=(1, 2))
    sh.add_waves_regular(0.5, 0.4)
    for b in range(3):
        assert lib.hc_set_drift_qtf(sh.ctx, b, 3, dp(g3), dp(P3 * (b + 1)), None) == OK
    assert lib.hc_set_drift_mode(sh.ctx, 1) == OK
    o6 = np.empty(6)
    assert lib.hc_compute_drift(sh.ctx, 0.0, dp(z9), dp(o6)) == OK and np.allclose(o6, 50.0, rtol=1e-12)
    # the Python layer refuses what it can see
    with pytest.raises(ValueError):
        h.set_drift_qtf(0, g3, np.zeros((6, 3, 2)))
    with pytest.raises(ValueError):
        h.set_drift_mean(0, g3, np.zeros((5, 3)))
    with pytest.raises(Exception):
        h.set_drift_mode(4)
