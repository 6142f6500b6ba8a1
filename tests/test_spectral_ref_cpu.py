"""The reference of the spectral wave excitation (tests/spectral_ref.py) checked without a GPU: a correct FP64 evaluation can meet
the bound B on every input set the GPU tests use, the longdouble value agrees with a second formulation, and the closed forms hold."""
import numpy as np
import pytest

import spectral_ref as sr

pytestmark = pytest.mark.skipif(not sr.longdouble_ok(), reason="np.longdouble is not wider than FP64 here: no high-precision reference")

_cases = {}


def _case(key):
    if key not in _cases:
        _cases[key] = sr.build_case(key)
    return _cases[key]


def _tab(s):
    return sr.tables(_case(s["case"]), sr.oracle_spectrum(s["kw"]))


@pytest.mark.parametrize("sid", list(sr.INPUT_SETS))
def test_fp64_restatements_stay_within_the_bound_and_formulations_agree(sid):
    """Per input set of the GPU tests: |fp64 - longdouble| <= B row by row for the index-order sum and for the kernel's order (16
    strided partial sums, then the pairwise tree); the longdouble value against cos(w t) cos(psi) - sin(w t) sin(psi) to 1e-17 of
    sum |X| a (plus the extended format's own rounding of w t, which only matters at the large times)."""
    s = sr.INPUT_SETS[sid]
    tab = _tab(s)
    ramp, times = s["kw"]["ramp_duration"], s["times"]
    if tab["X"].shape[0] > 200:  # the wide set: every 8th time is enough for the Python loops over the components
        times = times[::8]
    F, B = sr.forces(tab, ramp, times), sr.bound(tab, times)
    assert np.all(np.isfinite(F.astype(np.float64))) and np.all(B >= 0.0)
    worst = 0.0
    for name, fn in (("index order", sr.fp64_index_order), ("kernel order", sr.fp64_kernel_order)):
        err = np.abs(fn(tab, ramp, times).astype(np.longdouble) - F).astype(np.float64)
        assert np.all(err <= B), (sid, name, float(np.max(err[B > 0] / B[B > 0])) if np.any(B > 0) else float(np.max(err)))
        if np.any(B > 0):
            worst = max(worst, float(np.max(err[B > 0] / B[B > 0])))
    print(f"{sid}: worst |fp64 - ref| / B = {worst:.3f}")
    # The two longdouble formulations: 1e-17 of sum |X| a, plus what the number format itself takes: each of them rounds the product
    # w_i t once to the 64-bit significand (2^-64 |w_i t| each, an absolute phase error that nothing later scales down) -- 3e-14 rad at
    # t = 1e5 s, still 8000 times below the 4 u Theta of B.
    G = sr.forces_second_formulation(tab, ramp, times)
    scale = sr.term_scale(tab)[None, :]
    W = np.abs(tab["X"]) * tab["amp"][None, :]
    fmt = np.stack([np.sum(W * np.abs(tab["omega"] * t)[None, :], axis=1) for t in times]) * 2.0 ** -63
    assert np.all(np.abs(F - G).astype(np.float64) <= 1e-17 * scale + fmt), sid
    assert np.all(fmt <= B / 4096.0)
    if s["kw"]["nfrequencies"] == 1:  # one component: its trapezoid width is 0, so the force is exactly zero
        assert np.all(tab["amp"] == 0.0) and np.all(F == 0.0) and np.all(B == 0.0)
    else:
        assert np.all(scale[:, np.any(tab["X"] != 0.0, axis=1)] > 0.0)


def test_one_component_is_the_regular_wave_closed_form():
    case = _case(("many", 2, 16, 7002))
    A, f0 = 0.7, 0.11
    spec = dict(f=np.array([f0]), S=np.array([A * A / 2]), df=np.array([1.0]), phase=np.array([0.0]))
    tab = sr.tables(case, spec)
    assert abs(tab["amp"][0] - A) <= 2e-16
    times = np.array([0.0, 0.3, 4.4, 51.7])
    F = sr.forces(tab, 0.0, times)
    om = np.longdouble(2 * np.pi * f0)
    want = tab["X"].astype(np.longdouble)[None, :, 0] * np.longdouble(tab["amp"][0]) * np.cos(om * times.astype(np.longdouble)[:, None] + tab["P"].astype(np.longdouble)[None, :, 0])
    assert np.all(np.abs(F - want).astype(np.float64) <= 1e-18 * np.abs(tab["X"][None, :, 0]) * A)
    # ... and the RAO of a component that sits on a list entry is that entry, scaled by rho g
    bd = case["bodies"][1]
    w = np.asarray(bd["w"])
    j = 7
    x, p = sr.rao_at(w, np.asarray(bd["ex_mag"]).reshape(6, -1), bd["ex_phase"], np.array([w[-1] / w.size * (j + 1)]))
    assert np.allclose(x[:, 0], np.asarray(bd["ex_mag"]).reshape(6, -1)[:, j], rtol=1e-13, atol=0) and np.allclose(p[:, 0], np.asarray(bd["ex_phase"]).reshape(6, -1)[:, j], rtol=1e-13, atol=1e-15)


def test_ramp_factor():
    assert [sr.ramp_factor(t, 5.0) for t in (-3.0, -1e-300, 0.0)] == [0.0, 0.0, 0.0]
    assert sr.ramp_factor(1.25, 5.0) == 0.25 and sr.ramp_factor(np.nextafter(5.0, 0.0), 5.0) < 1.0
    assert sr.ramp_factor(5.0, 5.0) == 1.0 and sr.ramp_factor(1e5, 5.0) == 1.0
    assert [sr.ramp_factor(t, 0.0) for t in (-1.0, 0.0, 1e-9, 7.0)] == [1.0] * 4
    s = sr.INPUT_SETS["times-ramp_edges"]
    tab = _tab(s)
    F = sr.forces(tab, sr.RAMP, s["times"])
    full = sr.forces(tab, 0.0, s["times"])
    assert np.all(F[:2] == 0.0) and np.all(full[:2] != 0.0)       # t = -1, 0: zero, never a negative factor
    assert np.all(np.abs(F[2] - full[2] * np.longdouble(1e-9) / np.longdouble(sr.RAMP)) <= 1e-18 * np.abs(full[2]))
    assert np.all(np.abs(F[3]) < np.abs(full[3])) and np.all(F[4:] == full[4:])  # one ulp below the ramp's end: still scaled; from it on: not


def test_rao_edge_sets_hit_the_cases_they_are_there_for():
    """The spectra of the RAO-edge sets really put components below the first list entry, exactly on entries, inside the last
    interval and above the last entry -- per body, with energy in them."""
    case = _case(("mixed_rao",))
    nws = [np.asarray(bd["w"]).size for bd in case["bodies"]]
    assert nws == [16, 40, 2, 1]

    def position(b, sid):
        sp = sr.oracle_spectrum(sr.INPUT_SETS[sid]["kw"])
        w = np.asarray(case["bodies"][b]["w"])
        amp = np.sqrt(2 * sp["S"] * sp["df"])
        return (2 * np.pi * sp["f"]) / (w[-1] / w.size) - 1.0, amp / np.sum(amp)

    idx, share = position(0, "rao-on_list")
    exact = (idx == np.round(idx)) & (idx >= 0) & (idx <= 15)
    assert np.count_nonzero(exact) >= 6 and np.sum(share[exact]) > 0.05, (idx, share)   # m = 1, 2, 4, 8, 16 at the least
    assert np.count_nonzero(idx > 15) >= 10 and np.sum(share[idx > 15]) > 0.05          # above the last entry: held constant
    for b in (0, 2):
        idx, share = position(b, "rao-below")
        assert np.count_nonzero(idx < 0) >= 2 and np.sum(share[idx < 0]) > 0.01, (b, idx, share)
    for b in (0, 1):
        idx, share = position(b, "rao-last_two")
        last = (idx > nws[b] - 2) & (idx < nws[b] - 1)
        assert np.count_nonzero(last) >= 1 and np.sum(share[last]) > 0.005, (b, idx)
        assert np.count_nonzero(idx > nws[b] - 1) >= 1
    idx, _ = position(2, "rao-on_list")  # nw = 2: below, inside and above its single interval
    assert np.any(idx < 0) and np.any((idx > 0) & (idx < 1)) and np.any(idx > 1)
    # the held-constant rule itself
    bd = case["bodies"][0]
    x, p = sr.rao_at(bd["w"], np.asarray(bd["ex_mag"]).reshape(6, -1), bd["ex_phase"], np.array([1e-3, 50.0]))
    m = np.asarray(bd["ex_mag"]).reshape(6, -1)
    assert np.array_equal(x[:, 0], m[:, 0]) and np.allclose(x[:, 1], m[:, -1], rtol=4e-16, atol=0)  # (m0 + 1 * (m1 - m0): an ulp of m1)
    bd = case["bodies"][3]  # nw = 1
    x, _ = sr.rao_at(bd["w"], np.asarray(bd["ex_mag"]).reshape(6, -1), bd["ex_phase"], np.array([0.1, 1.0, 9.0]))
    assert np.array_equal(x, np.repeat(np.asarray(bd["ex_mag"]).reshape(6, 1), 3, axis=1))


def test_input_sets_cover_what_the_issue_lists():
    ids = set(sr.INPUT_SETS)
    for N in (1, 2, 3, 5, 9):
        for nf in (1, 2, 15, 16, 17, 64, 1000, 2048):
            assert f"rows-N{N}-nf{nf}" in ids
    assert {"steps-N3", "steps-N8", "wide", "shards-N3", "shards-N4", "shards-N5", "shards-N9"} <= ids
    assert sr.SHARD_SPLITS == ((3, 3), (4, 2), (5, 2), (9, 4)) and 6 * sr.WIDE_N >= 1024
    t = sr.INPUT_SETS["times-large_t"]["times"]
    assert t.min() >= 1e4 and t.max() >= 1e5


def test_the_bound_rejects_the_defects_the_gpu_tests_are_there_for():
    """The FP64 evaluation in the kernel's order with one defect planted each time, on the input sets of the GPU tests: every one of them
    lands far outside B somewhere (a bound that a wrong kernel could meet would prove nothing)."""
    def worst(sid, mutate_tab=None, mutate_times=None, ramp=None):
        s = sr.INPUT_SETS[sid]
        tab = _tab(s)
        times = s["times"][:24]
        F, B = sr.forces(tab, s["kw"]["ramp_duration"], times), sr.bound(tab, times)
        bad = dict(tab)
        if mutate_tab:
            mutate_tab(bad)
        G = sr.fp64_kernel_order(bad, s["kw"]["ramp_duration"] if ramp is None else ramp, mutate_times(times) if mutate_times else times)
        err = np.abs(G.astype(np.longdouble) - F).astype(np.float64)
        return float(np.max(err[B > 0] / B[B > 0]))

    def shard_reads_global_rows(tab):  # the second of two shards of four bodies indexing the table by the global row
        tab["X"], tab["P"] = np.roll(tab["X"], 12, axis=0), np.roll(tab["P"], 12, axis=0)

    def loop_stops_at_a_multiple_of_16(tab):
        tab["amp"] = tab["amp"].copy()
        tab["amp"][16 * (tab["amp"].size // 16):] = 0.0

    def phi_sign_flipped(tab):
        tab["phi"] = -tab["phi"]

    def rao_zero_above_the_list(tab):
        case = _case(("mixed_rao",))
        w = np.asarray(case["bodies"][0]["w"])
        tab["X"] = tab["X"].copy()
        tab["X"][:6, tab["omega"] > w[-1]] = 0.0

    assert worst("shards-N4", shard_reads_global_rows) > 1e6
    assert worst("steps-N3", loop_stops_at_a_multiple_of_16) > 1e3 and worst("rows-N2-nf15", loop_stops_at_a_multiple_of_16) > 1e6
    assert worst("steps-N3", phi_sign_flipped) > 1e6
    assert worst("steps-N3", mutate_times=lambda t: np.full_like(t, t[0])) > 1e6  # a block step using the block's first t
    assert worst("rao-on_list", rao_zero_above_the_list) > 1e6
    # the t <= 0 branch of the ramp removed: a negative time gets a negative factor instead of 0
    s = sr.INPUT_SETS["times-ramp_edges"]
    tab = _tab(s)
    t = s["times"][:1]
    assert t[0] < 0.0
    wrong = sr.fp64_kernel_order(tab, 0.0, t) * (t[0] / sr.RAMP)
    assert np.all(np.abs(wrong[0]) > 1e6 * sr.bound(tab, t)[0]) and np.all(sr.forces(tab, sr.RAMP, t) == 0.0)
