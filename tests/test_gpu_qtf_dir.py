"""The two QTF terms for tables on a heading x frequency grid on the GPU (hc_set_drift_qtf_headings, hc_set_sum_qtf_headings; DESIGN
3.7l) against the direct pair sum of the definition in longdouble (tests/qtf_dir_ref.py): the drift modes 1 to 3 and the sum term.
The device evaluates the projected O(nf + J^2) form over the nodes, so the identity between the two is under test as well.

Tolerance: the bound qtf_dir_ref derives per body and row, ramp^2 (2 * 1e-11 + (nf + J^2 + 64) 2^-52) M_d, M_d twice the sum of the
absolute pair terms over node pairs (its docstring has the derivation).  Every case keeps the phase magnitude below 1e4; the
reference asserts it."""
import os
import subprocess

import numpy as np
import pytest

import drift_ref as dr
import qtf_dir_ref as qd
import sumfreq_ref as sf
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=60.0, ramp_duration=10.0, wave_height=2.0, wave_period=9.0,
             frequency_min=0.03, frequency_max=0.9, nfrequencies=257, seed=3)
REG_AMP, REG_OMEGA = 0.177, 2.094395102
LD = qd.LD


@pytest.fixture(scope="module")
def hydro():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd import capi, hydro
    return hydro, capi


def synth_case(N):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def spread_sea(h, case, **kw):
    """The spectral model with excitation tables on a heading grid for every body (its own table at both ends of [-3, 3]): what
    non-uniform directions need.  h: HydroForces or HydroGroup."""
    for b, bd in enumerate(case["bodies"]):
        mag, ph = (np.stack([np.asarray(bd[key]).reshape(6, -1)] * 2, axis=1) for key in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-3.0, 3.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, **dict(IRREG, **kw))


def components(h, theta):
    A, w, k, phi = wk.irregular_components(h.irreg_spectrum())[:4]
    return A, w, k, phi, np.broadcast_to(np.asarray(theta, dtype=np.float64), A.shape).copy()


def set_both(h, b, table):
    beta, g, P, Q = table
    h.set_drift_qtf(b, g, P, Q, headings=beta)
    h.set_sum_qtf(b, g, P, Q, headings=beta)


def evaluate(h, key, t, pos):
    if key == "sum":
        h.set_sum_mode(1)
        return h.compute_sum_qtf(t, pos).reshape(-1, 6)
    h.set_drift_mode(key)
    return h.compute_drift(t, pos).reshape(-1, 6)


def compare(h, refs, comp, t, pos, what, ramp=1.0, keys=qd.KEYS):
    """GPU against the pair sum for the drift modes and the sum term, inside the derived bound.  refs: per body None or a
    qtf_dir_ref.PairSum.  Returns {key: [N][6]}."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    want = [None if r is None else r.force(t, pos[b, 0], pos[b, 1], ramp=ramp) for b, r in enumerate(refs)]
    bound = [None if r is None else qd.bounds(comp, r.table, ramp=ramp) for r in refs]
    out = {}
    for key in keys:
        got = evaluate(h, key, t, pos)
        assert np.all(np.isfinite(got)), what
        for b, ref in enumerate(refs):
            if ref is None:
                assert not got[b].any(), (what, key, b)
                continue
            err = np.abs(got[b] - want[b][key])
            worst = float(np.max(err / np.maximum(bound[b][key], 1e-300)))
            print(f"{what} {key} body {b}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(want[b][key])):.3e}")
            assert np.all(err <= bound[b][key]), f"{what} {key} body {b}: worst {worst:.3e} of the bound"
        out[key] = got
    return out


def refused(fn, hydro, code):
    with pytest.raises(hydro[0].HydroError) as e:
        fn()
    assert e.value.status == code, str(e.value)
    return str(e.value)


# ------------------------------------------------------------------------------------------------
# 1: a regular wave under a heading
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [0.2, 0.6, -0.5, 1.0])  # on a node, between two nodes, the two grid ends
def test_regular_wave(hydro, theta):
    h = hydro[0].HydroForces.from_case(sphere_case())
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    h.set_wave_directions([theta])
    h.set_drift_options(regular_phase=0.7)
    h.set_sum_options(regular_phase=0.7)
    A, w, k, phi = wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.7)[:4]
    comp = (A, w, k, phi, np.array([theta]))
    beta, g = np.array([-0.5, 0.2, 1.0]), np.array([0.7, 1.5, 2.0, 2.5, 3.3])
    rng = np.random.default_rng(5)
    table = (beta, g, rng.normal(0, 1e4, (6, 3, 3, 5, 5)), rng.normal(0, 1e4, (6, 3, 3, 5, 5)))
    set_both(h, 0, table)
    assert (h.drift_qtf_headings(0), h.drift_qtf_size(0), h.sum_qtf_headings(0), h.sum_qtf_size(0)) == (3, 5, 3, 5)
    ref = qd.PairSum(comp, table)
    bound = qd.bounds(comp, table)
    states = [(0.0, 0.0, 0.0), (3.7, 12.3, -8.5), (41.3, -4.0, 21.0)]
    results = [compare(h, [ref], comp, t, [[x, y, -1.0]], f"regular theta={theta} t={t} x={x} y={y}") for t, x, y in states]
    for key in (1, 2, 3):  # the constant A^2 T(theta, theta, w, w): over t, x and y inside twice the bound of one another, and the closed form
        closed = REG_AMP ** 2 * np.asarray((ref.Di if key < 3 else ref.Pij[:, :, 0])[:, 0], dtype=np.float64)
        assert np.abs(closed).max() > 1.0
        for r in results:
            assert np.all(np.abs(r[key][0] - closed) <= bound[key])
    for (t, x, y), r in zip(states, results):  # A^2 [P cos 2 psi - Q sin 2 psi], y in psi
        psi = LD(k[0]) * (LD(x) * np.cos(LD(theta)) + LD(y) * np.sin(LD(theta))) - LD(w[0]) * LD(t) + LD(phi[0])
        closed = sf.regular_closed_form(REG_AMP, psi, ref.Pij[:, 0, 0], ref.Qij[:, 0, 0])
        assert np.all(np.abs(r["sum"][0] - closed) <= bound["sum"])
    moved = evaluate(h, "sum", 3.7, np.array([[12.3, 0.0, -1.0]]))
    assert np.any(np.abs(moved[0] - results[1]["sum"][0]) > 4 * bound["sum"])  # y = -8.5 against y = 0: another phase


# ------------------------------------------------------------------------------------------------
# 2: a spread sea
# ------------------------------------------------------------------------------------------------
def test_spread_sea_all_modes_and_the_ramp(hydro):
    case = three_body_case()
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case)
    th = h.set_wave_spreading(0.3, s=4.0, n_bins=15, seed=2)
    assert th.size == 257 and np.unique(th).size > 5
    comp = components(h, th)
    blo, bhi = th.min() - 0.1, th.max() + 0.1
    tables = {0: qd.random_table(3, 5, 40, blo, bhi, 0.6, 3.0), 2: qd.random_table(3, 5, 41, blo, bhi, 0.7, 2.8)}
    inside = dr.cells(tables[0][1], comp[1])[0]
    assert 10 < inside.sum() < inside.size - 10
    refs = [None] * 3
    for b, tb in tables.items():
        set_both(h, b, tb)
        refs[b] = qd.PairSum(comp, tb)
    pos = np.array([[0.0, -7.5, -1.0], [15.0, 0.0, -1.0], [30.0, 23.0, -1.0]])
    got = {}
    for t in (0.0, 4.0, 43.2):  # at the start of, inside and after the ramp
        got[t] = compare(h, refs, comp, t, pos, f"spread t={t}", ramp=dr.ramp_factor(t, IRREG["ramp_duration"]))
    for key in qd.KEYS:
        assert not got[0.0][key].any() and np.abs(got[43.2][key][[0, 2]]).max() > 1.0


# ------------------------------------------------------------------------------------------------
# 3: the tile of 256 components, the chunks of 32 node rows, the four nodes of a lane, the ends of the two grids
# ------------------------------------------------------------------------------------------------
def edge_case(hydro, nf, nh, nq, seed, with_q=True):
    """One body in a spread sea of nf components; a table whose frequency grid runs from w[nf/8] to w[nf - nf/8 - 1] (components
    beyond both ends) with nodes on components, and directions of which some sit on heading nodes, both ends among them."""
    case = synth_case(1)
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case, nfrequencies=nf)
    w = wk.irregular_components(h.irreg_spectrum())[1]
    rng = np.random.default_rng(seed)
    beta, _, P, Q = qd.random_table(nh, nq, seed, -0.7, 0.9, 1.0, 2.0, with_q=with_q)
    lo, hi = w[nf // 8], w[nf - nf // 8 - 1]
    mid = w[(w > lo) & (w < hi)]
    g = np.unique(np.concatenate([[lo, hi], rng.choice(mid, size=min((nq - 2) // 2, mid.size), replace=False)]))
    while g.size < nq:
        g = np.unique(np.concatenate([g, rng.uniform(lo, hi, size=nq - g.size)]))
    th = rng.uniform(beta[0], beta[-1], nf)
    th[::5] = beta[np.arange(th[::5].size) % nh]
    h.set_wave_directions(th)
    comp = components(h, th)
    inside, _, lam = dr.cells(g, comp[1])
    mu = qd.head_cells(beta, th)[2]
    assert g.size == nq and 0 < inside.sum() <= nf - 2 * (nf // 8) + 2 and (lam[inside] == 0).sum() >= 2 and (mu[inside] == 0).sum() >= min(nh, 3)
    return h, comp, (beta, g, P, Q)


@pytest.mark.parametrize("nf", [255, 256, 257])
def test_tile_edges(hydro, nf):
    for nh, nq in ((3, 11), (6, 43)):  # J = 33: the second chunk of one row; J = 258: a lane's second node
        h, comp, table = edge_case(hydro, nf, nh, nq, 100 + nq)
        set_both(h, 0, table)
        compare(h, [qd.PairSum(comp, table)], comp, 33.3, [[7.25, -3.5, -1.0]], f"nf={nf} J={nh * nq}")


@pytest.mark.parametrize("nh,nq,nf,with_q", [(3, 85, 257, True), (4, 64, 257, True), (16, 64, 64, False)])
def test_node_count_edges(hydro, nh, nq, nf, with_q):
    """J = 255, 256 (one lane per node, to the last) and the cap J = 1024 (32 chunks, four nodes per lane, Q = None)"""
    h, comp, table = edge_case(hydro, nf, nh, nq, 200 + nq + nh, with_q=with_q)
    set_both(h, 0, table)
    compare(h, [qd.PairSum(comp, table)], comp, 33.3, [[7.25, -3.5, -1.0]], f"nf={nf} J={nh * nq}")


def test_heading_outside_the_grid_and_one_heading(hydro):
    capi = hydro[1]
    h, comp, table = edge_case(hydro, 64, 3, 5, 7)
    set_both(h, 0, table)
    pos = np.array([[7.25, -3.5, -1.0]])
    first = compare(h, [qd.PairSum(comp, table)], comp, 33.3, pos, "before")
    beta, g = table[0], table[1]
    inside = dr.cells(g, comp[1])[0]
    th = comp[4].copy()
    out_i = np.nonzero(~inside)[0][0]
    th[out_i] = beta[-1] + 0.5  # outside the frequency grid: its heading is never looked at
    h.set_wave_directions(th)
    comp2 = comp[:4] + (th,)
    got = compare(h, [qd.PairSum(comp2, table)], comp2, 33.3, pos, "a heading outside, outside the frequency grid")
    assert all(same_bits(got[key], first[key]) for key in qd.KEYS)  # it takes no part: k x c + y s of that component is not summed
    bad = th.copy()
    bad[np.nonzero(inside)[0][3]] = np.nextafter(beta[-1], 9.0)  # inside the frequency grid, one ulp past the last heading
    h.set_wave_directions(bad)
    h.set_drift_mode(3)
    for call in (lambda: h.compute_drift(33.3, pos), lambda: h.compute_sum_qtf(33.3, pos), lambda: h.compute_drift(33.3, pos)):
        assert "heading grid" in refused(call, hydro, capi.HC_ERR_INVALID)
    refused(h.drift_end, hydro, capi.HC_ERR_INVALID)  # nothing is pending
    refused(h.sum_qtf_end, hydro, capi.HC_ERR_INVALID)
    h.set_wave_directions(th)
    assert all(same_bits(evaluate(h, key, 33.3, pos), first[key]) for key in qd.KEYS)
    # nh = 1: valid for a heading of exactly beta_0
    one = (np.array([0.25]), g, table[2][:, :1, :1], table[3][:, :1, :1])
    set_both(h, 0, one)
    h.set_wave_directions(np.full(64, 0.25))
    comp3 = comp[:4] + (np.full(64, 0.25),)
    compare(h, [qd.PairSum(comp3, one)], comp3, 33.3, pos, "nh = 1")
    h.set_wave_directions(np.full(64, np.nextafter(0.25, 1.0)))
    assert "heading grid" in refused(lambda: h.compute_drift(33.3, pos), hydro, capi.HC_ERR_INVALID)


# ------------------------------------------------------------------------------------------------
# 4: invariance, bitwise
# ------------------------------------------------------------------------------------------------
def test_a_bodys_bits_are_its_own(hydro):
    HF, HG = hydro[0].HydroForces, hydro[0].HydroGroup
    rng = np.random.default_rng(11)
    th = rng.uniform(-0.4, 0.6, 257)
    table = qd.random_table(3, 20, 60, -0.5, 0.7, 0.6, 3.0)
    table[0][1] = 0.0  # a node at beta = 0, for the runs without directions
    others = [qd.random_table(2, 7, 61, -0.5, 0.7, 0.5, 3.2), qd.random_table(5, 9, 62, -0.6, 0.8, 0.7, 2.5)]
    one_heading = dr.random_table(33, 63, 0.6, 3.0)
    t, own = 33.0, np.array([41.5, -12.25, -1.0])

    def run(make, body, N, directions=True, neighbours=(), one=None):
        case = synth_case(N)
        h = make(case)
        spread_sea(h, case)
        if directions:
            h.set_wave_directions(th)
        if body is not None:
            set_both(h, body, table)
        for b, tb in neighbours:
            set_both(h, b, tb)
        if one is not None:
            h.set_drift_qtf(one, *one_heading)
            h.set_sum_qtf(one, *one_heading)
        pos = np.zeros((N, 3))
        pos[:, 0], pos[:, 1] = 3.0 * np.arange(N), -2.0 * np.arange(N)
        if body is not None:
            pos[body] = own
        return {key: evaluate(h, key, t, pos) for key in qd.KEYS}

    alone = run(HF.from_case, 0, 1)
    assert all(np.abs(alone[key]).max() > 1.0 for key in qd.KEYS)
    last = run(HF.from_case, 2, 3, neighbours=[(0, others[0]), (1, others[1])])
    first = run(HF.from_case, 0, 3, neighbours=[(1, others[0]), (2, others[1])])  # another slot, another place in the grid
    shard = run(lambda case: HF.from_case(case, body_range=(2, 3)), 2, 3, neighbours=[(0, others[0]), (1, others[1])])
    group = run(lambda case: HG.from_case(case, 2), 2, 3, neighbours=[(0, others[0])])
    for key in qd.KEYS:
        assert same_bits(last[key][2], alone[key][0]) and same_bits(first[key][0], alone[key][0]), key
        assert same_bits(shard[key][0], alone[key][0]) and same_bits(group[key][2], alone[key][0]), key
    # no directions: beside a body with a one-heading table, each returns the bits it returns without the other
    calm = run(HF.from_case, 0, 1, directions=False)
    beside = run(HF.from_case, 1, 2, directions=False, one=0)
    only_one = run(HF.from_case, None, 2, directions=False, one=0)
    for key in qd.KEYS:
        assert same_bits(beside[key][1], calm[key][0]) and same_bits(beside[key][0], only_one[key][0]), key
        assert np.abs(only_one[key][0]).max() > 1.0 and not only_one[key][1].any()


# ------------------------------------------------------------------------------------------------
# 5: a one-heading table keeps its refusal; 6: a heading table without directions
# ------------------------------------------------------------------------------------------------
def test_refusal_kept_and_the_getters(hydro):
    capi = hydro[1]
    case = sphere_case()
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case)
    h.set_wave_directions(np.full(257, 0.3))
    g = np.linspace(0.6, 3.0, 6)
    table = qd.random_table(2, 6, 3, 0.0, 0.5, 0.6, 3.0)
    pos = np.array([[2.0, 3.0, -1.0]])
    h.set_drift_mode(2)
    h.set_sum_mode(1)
    for setter, compute, size, heads in ((h.set_drift_qtf, h.compute_drift, h.drift_qtf_size, h.drift_qtf_headings),
                                         (h.set_sum_qtf, h.compute_sum_qtf, h.sum_qtf_size, h.sum_qtf_headings)):
        assert (size(0), heads(0)) == (0, 0)
        setter(0, g, np.ones((6, 6, 6)))
        assert (size(0), heads(0)) == (6, 0)
        assert "direction" in refused(lambda: compute(43.2, pos), hydro, capi.HC_ERR_UNSUPPORTED)
        setter(0, table[1], table[2], table[3], headings=table[0])  # replaces the one-heading table
        assert (size(0), heads(0)) == (6, 2)
        assert np.abs(compute(43.2, pos)).max() > 1.0
        setter(0, g, np.ones((6, 6, 6)))  # and the other way round
        assert (size(0), heads(0)) == (6, 0)
        assert "direction" in refused(lambda: compute(43.2, pos), hydro, capi.HC_ERR_UNSUPPORTED)
        setter(0, [], None, headings=table[0])
        assert (size(0), heads(0)) == (0, 0) and not compute(43.2, pos).any()


def test_no_directions_is_the_heading_zero(hydro):
    case = three_body_case()
    h = hydro[0].HydroForces.from_case(case)
    h.add_waves_irregular(**IRREG)
    comp = components(h, 0.0)
    table = qd.random_table(3, 9, 70, -0.8, 0.6, 0.6, 3.0)
    table[0][1] = 0.0
    beta, g, P, Q = table
    set_both(h, 1, table)
    pos = np.array([[0.0, 5.0, -1.0], [15.0, -40.0, -1.0], [30.0, 0.0, -1.0]])
    got = compare(h, [None, qd.PairSum(comp, table), None], comp, 43.2, pos, "no directions")
    sub = (g, P[:, 1, 1], Q[:, 1, 1])
    h.set_drift_qtf(1, *sub)
    h.set_sum_qtf(1, *sub)
    bd, bd1, bs1 = qd.bounds(comp, table), dr.bounds(comp[:4], sub), sf.bound(comp[:4], sub)
    for key in qd.KEYS:
        one = evaluate(h, key, 43.2, pos)
        assert np.all(np.abs(one[1] - got[key][1]) <= bd[key] + (bs1 if key == "sum" else bd1[key])), key


# ------------------------------------------------------------------------------------------------
# 7: rebuilds
# ------------------------------------------------------------------------------------------------
def test_rebuilds_follow_directions_waves_and_tables(hydro):
    case = sphere_case()
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case)
    rng = np.random.default_rng(21)
    thA, thB = rng.uniform(-0.4, 0.6, 257), rng.uniform(-0.4, 0.6, 257)
    table, table2 = qd.random_table(3, 7, 80, -0.5, 0.7, 0.6, 3.0), qd.random_table(2, 5, 81, -0.5, 0.7, 0.6, 3.0)
    set_both(h, 0, table)
    pos, t = np.array([[4.0, -9.0, -1.0]]), 43.2

    def all_keys():
        return {key: evaluate(h, key, t, pos) for key in qd.KEYS}

    h.set_wave_directions(thA)
    a1 = all_keys()
    h.set_wave_directions(thB)
    b1 = compare(h, [qd.PairSum(components(h, thB), table)], components(h, thB), t, pos, "directions B")
    h.set_wave_directions(thA)
    a2 = all_keys()
    spread_sea(h, case, wave_height=3.0)  # another wave model (it drops the directions), and back
    h.set_wave_directions(thA)
    c1 = all_keys()
    spread_sea(h, case)
    h.set_wave_directions(thA)
    a3 = all_keys()
    set_both(h, 0, table2)  # a table replaced between calls takes effect
    compA = components(h, thA)
    d1 = compare(h, [qd.PairSum(compA, table2)], compA, t, pos, "table replaced")
    for key in qd.KEYS:
        assert same_bits(a1[key], a2[key]) and same_bits(a1[key], a3[key]), key
        if key != 1:  # (the mean drift does not see the directions' phases, only their weights)
            assert not np.allclose(a1[key], b1[key], rtol=1e-6)
        assert not np.allclose(a1[key], c1[key], rtol=1e-6) and not np.allclose(a1[key], d1[key], rtol=1e-6), key


# ------------------------------------------------------------------------------------------------
# 8: composition
# ------------------------------------------------------------------------------------------------
def raw_step(h, t, state):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in state]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def test_hydroforces_and_hydrogroup_step_compose(hydro):
    HF, HG = hydro[0].HydroForces, hydro[0].HydroGroup
    case = three_body_case()
    th = np.random.default_rng(31).uniform(-0.4, 0.6, 257)
    tables = {0: qd.random_table(3, 7, 90, -0.5, 0.7, 0.6, 3.0), 2: qd.random_table(2, 5, 91, -0.5, 0.7, 0.6, 3.0)}
    objs = [HF.from_case(case), HF.from_case(case), HG.from_case(case, 3), HG.from_case(case, 3)]
    for k, h in enumerate(objs):
        spread_sea(h, case)
        h.set_wave_directions(th)
        if k % 2 == 0:
            for b, tb in tables.items():
                set_both(h, b, tb)
            h.set_drift_mode(3)
            h.set_sum_mode(1)
    rng = np.random.default_rng(32)
    for n in range(4):
        t = 12.0 + SPHERE_DT * n
        st = [rng.normal(0, 0.3, (3, 3)) for _ in range(4)]
        st[0][:, 0] += 15.0 * np.arange(3)
        for with_terms, plain in ((objs[0], objs[1]), (objs[2], objs[3])):
            total, raw = with_terms.step(t, *st), plain.step(t, *st)
            dft, sm = with_terms.compute_drift(t, st[0]), with_terms.compute_sum_qtf(t, st[0])
            assert same_bits(with_terms.drift(), dft) and same_bits(with_terms.sum_qtf(), sm)
            assert same_bits(total, raw + dft + sm) and np.abs(dft).max() > 1.0 and np.abs(sm).max() > 1.0
        assert same_bits(objs[0].drift(), objs[2].drift()) and same_bits(objs[0].sum_qtf(), objs[2].sum_qtf())


def cpp_tables():
    """the tables tests/cpp/qtf_dir_caller.cpp builds"""
    d, a, b, m, n = np.meshgrid(np.arange(6.0), np.arange(2.0), np.arange(2.0), np.arange(3.0), np.arange(3.0), indexing="ij")
    P = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n + 500.0 * a - 375.0 * b
    Q = 500.0 * (m - n) + 62.5 * d + 31.25 * (a - b)
    S = 800.0 * (d + 1) - 100.0 * m - 50.0 * n + 25.0 * a * b
    return np.array([0.0, 1.0]), np.array([1.5, 2.25, 3.0]), P, Q, S


def test_cpp_mirror_composes_as_the_python_layer(hydro, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "qtf_dir_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "qtf_dir_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (20, 31)
    beta, omega, P, Q, S = cpp_tables()
    h = hydro[0].HydroForces(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
    h.set_wave_directions([0.4])
    h.set_drift_options(regular_phase=0.3)
    h.set_sum_options(regular_phase=0.3)
    h.set_drift_qtf(0, omega, P, Q, headings=beta)
    h.set_sum_qtf(0, omega, S, headings=beta)
    h.set_drift_mode(3)
    h.set_sum_mode(1)
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total, dft, sm = raw_step(h, t, st), h.compute_drift(t, st[0]), h.compute_sum_qtf(t, st[0])
        assert same_bits(row[19:25], dft) and same_bits(row[25:31], sm) and same_bits(row[13:19], total + dft + sm), t
    assert np.abs(rows[:, 19:25]).min() > 1.0 and np.abs(rows[:, 25:31]).max() > 1.0 and not np.allclose(rows[0, 25:31], rows[19, 25:31], rtol=1e-6)


# ------------------------------------------------------------------------------------------------
# 9: errors
# ------------------------------------------------------------------------------------------------
def test_errors(hydro):
    capi = hydro[1]
    h = hydro[0].HydroForces.from_case(sphere_case())
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    g = np.array([1.0, 2.0, 3.0])
    bad = lambda fn: refused(fn, hydro, capi.HC_ERR_INVALID)  # noqa: E731
    for setter in (h.set_drift_qtf, h.set_sum_qtf):
        bad(lambda: setter(0, g, np.ones((6, 0, 0, 3, 3)), headings=[]))  # nh = 0
        bad(lambda: setter(0, g, np.ones((6, 17, 17, 3, 3)), headings=np.arange(17.0)))  # nh above 16
        bad(lambda: setter(0, g, np.ones((6, 2, 2, 3, 3)), headings=[0.5, 0.5]))
        bad(lambda: setter(0, g, np.ones((6, 2, 2, 3, 3)), headings=[0.5, 0.25]))
        bad(lambda: setter(0, g, np.ones((6, 2, 2, 3, 3)), headings=[0.5, np.nan]))
        bad(lambda: setter(0, g, np.ones((6, 2, 2, 3, 3)), headings=[0.5, np.inf]))
        bad(lambda: setter(5, g, np.ones((6, 2, 2, 3, 3)), headings=[0.5, 1.0]))
        for shape in ((6, 3, 3), (6, 2, 3, 3), (6, 3, 3, 2, 2), (5, 2, 2, 3, 3)):
            with pytest.raises(ValueError):
                setter(0, g, np.ones(shape), headings=[0.5, 1.0])
        with pytest.raises(ValueError):
            setter(0, g, np.ones((6, 2, 2, 3, 3)), np.ones((6, 3, 3)), headings=[0.5, 1.0])
    dp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(capi.c_double_p)  # noqa: E731
    ones, beta = np.ones(6 * 2 * 2 * 3 * 3), np.array([0.0, 1.0])
    for fn in (h.lib.hc_set_drift_qtf_headings, h.lib.hc_set_sum_qtf_headings):
        assert fn(h.ctx, 0, 2, None, 3, dp(g), dp(ones), None) == capi.HC_ERR_INVALID
        assert fn(h.ctx, 0, 2, dp(beta), 3, None, dp(ones), None) == capi.HC_ERR_INVALID
        assert fn(h.ctx, 0, 2, dp(beta), 3, dp(g), None, None) == capi.HC_ERR_INVALID
        assert fn(h.ctx, 0, 5, dp(np.arange(5.0)), 205, dp(np.arange(1.0, 206.0)), dp(ones), None) == capi.HC_ERR_INVALID  # J = 1025: refused before P is read
        assert fn(h.ctx, 0, 2, dp(beta), 3, dp(g), dp(ones), None) == capi.HC_OK
    assert h.lib.hc_get_drift_qtf_headings(h.ctx, 0, None) == capi.HC_ERR_INVALID
    assert h.lib.hc_get_sum_qtf_headings(h.ctx, 3, None) == capi.HC_ERR_INVALID
    assert (h.drift_qtf_headings(0), h.sum_qtf_headings(0)) == (2, 2)
    # a setter while an evaluation is in flight
    h.set_wave_directions([0.5])
    h.set_drift_mode(3)
    h.set_sum_mode(1)
    pos = np.array([[1.0, 2.0, -1.0]])
    h.drift_begin(1.0, pos)
    assert "in flight" in bad(lambda: h.set_drift_qtf(0, g, np.ones((6, 2, 2, 3, 3)), headings=beta))
    h.set_sum_qtf(0, g, np.ones((6, 2, 2, 3, 3)), headings=beta)  # the other term is free
    assert np.abs(h.drift_end()).max() > 0
    h.sum_qtf_begin(1.0, pos)
    assert "in flight" in bad(lambda: h.set_sum_qtf(0, g, np.ones((6, 2, 2, 3, 3)), headings=beta))
    assert np.abs(h.sum_qtf_end()).max() > 0
