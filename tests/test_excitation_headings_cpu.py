"""The inputs of tests/test_gpu_excitation_headings.py, checked without a GPU (tests/excitation_headings_inputs.py): every state
the GPU file holds to the reference meets the conditions that keep the comparison from being vacuous, on the spectrum the CPU
oracle builds from the same wave parameters (the GPU tests assert that the context's own spectrum has those bits).

  * for every body and time the largest |reference force| of its six rows is at least 1e6 times its bound;
  * under non-uniform directions the reference differs, in some row of every body, from the reference with every direction moved
    onto the nearest node of that body's grid by at least 1e3 times the bound: a wrong weight or a swapped bracket shows;
  * the reference and the bound have a finite entry for every row of every body at every time, and a plain FP64 evaluation of the
    library's interpolation (the omega interpolation at both headings, then the blend, in the library's operation order) and of
    the sum stays inside the bound: the bound can be met."""
import numpy as np
import pytest

import excitation_headings_inputs as xi
import spectral_ref as sr

pytestmark = pytest.mark.skipif(not sr.longdouble_ok(), reason="np.longdouble is not wider than FP64 here: no high-precision reference")

STATES = xi.held_states()
_spectra, _cases = {}, {}


def spectrum(kw):
    key = tuple(sorted(kw.items()))
    if key not in _spectra:
        _spectra[key] = sr.oracle_spectrum(kw)
    return _spectra[key]


def case_of(N):
    if N not in _cases:
        _cases[N] = xi.build_case(N, S=2)
    return _cases[N]


def fp64_tables(case, spec, tables, theta):
    """the tables as the library forms them, in FP64 and in its operation order"""
    tab = sr.tables(case, spec)
    if theta is None:
        return tab
    rg = case["rho"] * case["g"]
    X, P = tab["X"].copy(), tab["P"].copy()
    for b, tb in enumerate(tables):
        if tb is None:
            continue
        dirs, w, mag, ph = tb
        nw = w.size
        idx = np.clip(tab["omega"] / (w[-1] / nw) - 1.0, 0.0, nw - 1.0)
        k0 = np.minimum(np.floor(idx).astype(int), max(nw - 2, 0))
        k1, fr = np.minimum(k0 + 1, nw - 1), idx - k0
        j0 = np.searchsorted(dirs, theta, side="right") - 1
        j1 = np.minimum(j0 + 1, dirs.size - 1)
        wt = np.where(j1 > j0, (theta - dirs[j0]) / np.where(j1 > j0, dirs[j1] - dirs[j0], 1.0), 0.0)
        i = np.arange(theta.size)
        for r in range(6):
            for out, v in ((X, mag[r] * rg), (P, ph[r])):
                a0 = fr * (v[j0, k1] - v[j0, k0]) + v[j0, k0]
                a1 = fr * (v[j1, k1] - v[j1, k0]) + v[j1, k0]
                out[6 * b + r, i] = wt * (a1 - a0) + a0
    return dict(tab, X=X, P=P)


@pytest.mark.parametrize("k", range(len(STATES)), ids=[s[0] for s in STATES])
def test_held_state_meets_the_conditions(k):
    name, N, tables, kw, which, times = STATES[k]
    case, spec = case_of(N), spectrum(kw)
    nf = kw["nfrequencies"]
    theta = xi.directions(nf, which)
    assert len(tables) == N and spec["f"].size == nf
    if theta is not None:
        for tb in tables:
            assert tb is None or np.all((theta >= tb[0][0]) & (theta <= tb[0][-1])), name
    F, B = xi.reference(case, spec, tables, theta, kw["ramp_duration"], times)
    assert F.shape == B.shape == (len(times), 6 * N) and np.all(np.isfinite(F.astype(np.float64))) and np.all(B > 0.0), name
    signal = xi.check_signal(F, B, name)
    spread = theta is not None and np.unique(theta).size > 1
    move = xi.check_moves(case, spec, tables, theta, kw["ramp_duration"], times, name) if spread else float("nan")
    # a correct FP64 implementation stays inside the bound
    tab = fp64_tables(case, spec, tables, theta)
    for fp64 in (sr.fp64_index_order, sr.fp64_kernel_order):
        err = np.abs(fp64(tab, kw["ramp_duration"], times).astype(np.longdouble) - F).astype(np.float64)
        assert np.all(err <= B), (name, fp64.__name__, float(np.max(err / B)))
    print(f"{name}: smallest largest-row |F| / B = {signal:.2e}, smallest move to the nearest node / B = {move:.2e}")


def test_layouts_are_what_the_cases_need():
    for (kind, N), layout in xi.LAYOUTS.items():
        assert len(layout) == N
        grids = [None if e is None else xi.GRIDS[e[0]] for e in layout]
        if kind == "uniform":
            assert any(g is None for g in grids) and any(g is not None and g.size == 1 for g in grids)
            assert all(g is None or np.any(g == xi.UNIFORM_HEADING) or g.size > 1 for g in grids)
            assert all(g is None or g.size > 1 or g[0] == xi.UNIFORM_HEADING for g in grids)  # a one-node grid: on its node only
        if kind == "spread":
            assert all(g is not None and g.size >= 2 and g[0] <= xi.LO and g[-1] >= xi.HI for g in grids)
            assert any(g.size == 5 and np.unique(np.round(np.diff(g), 12)).size > 2 for g in grids)  # uneven spacing
            assert max(g[0] for g in grids) == xi.LO and min(g[-1] for g in grids) == xi.HI
        if kind == "uniform":  # grids of 1, 2 and 5 nodes among the bodies of one N
            both = layout + xi.LAYOUTS[("spread", N)]
            assert {1, 2, 5} <= {xi.GRIDS[e[0]].size for e in both if e is not None}
        assert any(e is not None and e[1] != 64 for e in layout)  # a frequency list of another length than rao_w (64)
    assert all(np.all(np.diff(g) > 0) for g in xi.GRIDS.values())
    for nf in (12, 257):
        a, b = xi.directions(nf, "A"), xi.directions(nf, "B")
        for th in (a, b):
            assert th.size == nf and np.all((th >= xi.LO) & (th <= xi.HI)) and np.unique(th).size > 1
        assert np.any(a == xi.LO) and np.any(a == xi.HI) and np.any(a == 0.0) and not np.array_equal(a, b)
        nodes = np.concatenate(list(xi.GRIDS.values()))
        assert not np.any(np.isin(b, nodes)) and nf // 3 <= np.count_nonzero(np.isin(a, nodes)) < nf
    # the row shards of five bodies: two shards with / without tables, three shards with / mixed / without
    from hydrochrono_amd.parallel_split import body_shard
    has = [e is not None for e in xi.LAYOUTS[("uniform", 5)]]
    for G, want in ((2, [{True}, {False}]), (3, [{True}, {True, False}, {False}])):
        assert [set(has[slice(*body_shard(5, G, g))]) for g in range(G)] == want
    has = [e is not None for e in xi.LAYOUTS[("regular", 5)]]
    for G in (2, 3):
        owners = [g for g in range(G) for b in range(*body_shard(5, G, g)) if has[b]]
        assert not has[0] and owners and 0 not in owners  # body 0 and the bodies with tables sit on different shards
    assert xi.WIDE_N * 6 >= 1024 and {e is None for e in xi.wide_layout()} == {True, False}


def test_walk_changes_fall_inside_blocks_and_edge_inputs():
    for la in (16, 32):
        segs = xi.walk_segments(la)
        ends = np.cumsum(segs)
        assert len(segs) == len(xi.WALK) and all(n > la for n in segs)
        assert all((e - 1) % la not in (0, la - 1) and e % la != 0 for e in ends[:-1])  # no change on a block boundary, whichever step starts the first block
    assert [w[1] for w in xi.WALK] == [None, "directions", "directions", "tables", "directions", "model"]
    assert not np.array_equal(xi.walk_tables(3, 5)[1][2], xi.walk_tables(3, 0)[1][2]) and np.array_equal(xi.walk_tables(3, 5)[0][2], xi.walk_tables(3, 0)[0][2])
    assert xi.step_count(32) == 67 and xi.step_count(16) == 35
    g = xi.EDGE_GRID
    assert g[0] == 0.0 and np.unique(np.round(np.diff(g), 12)).size == g.size - 1
    dirs, w, mag, ph = xi.edge_tables("jump")[0]
    assert np.all(np.abs(ph[:, 1] - ph[:, 0]) > np.pi) and np.all(np.abs(ph) <= np.pi)
    inside = [s[2] for s in xi.edge_states()[:2]]
    assert 0.0 < inside[0] < 1e-300 and g[-2] < inside[1] < g[-1]
    # the times: inside the ramp, past it, none, large
    assert xi.TIMES[0] < xi.RAMP and xi.TIMES[1] < xi.RAMP < xi.TIMES[2] and xi.TIMES[3] >= 1e4 and xi.KW_NO_RAMP["ramp_duration"] == 0.0
