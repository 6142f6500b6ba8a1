"""The first-order excitation on heading grids (hc_set_wave_directions, hc_set_excitation_rao_headings; csrc/hc_directions.cpp,
DESIGN.md 3.7k) across bodies, row shards and step paths: the part of the directional sea that enters the total of every hc_step.

  * values: the tables of directional_ref.heading_tables (longdouble) under spectral_ref.forces, every row of every body within
    spectral_ref.bound, as tests/test_gpu_directional.py::test_spectral_excitation_with_heading_tables holds one body; a regular
    wave by the regular_coeffs comparison of that file and the same bound form.  No tolerance of this file's own;
  * bits: where the library promises them -- a direction on a grid node against hc_set_excitation_rao with that node's table, row
    shards against one context, a context walked through changes against a fresh one created in the state, the hydrostatic and
    radiation components against a twin that never saw a direction.

A fresh context that takes a history through hc_set_history starts a look-ahead block of its own, so its radiation rows are summed
in another order than those of a context in the middle of a block (tests/test_gpu_parity.py::test_history_injection_matches_stepping):
against it the wave and hydrostatic rows are held bitwise, radiation and total at TIGHT_TOL; radiation is held bitwise against the
twin, which runs the same blocks.

The inputs are fixed in tests/excitation_headings_inputs.py; tests/test_excitation_headings_cpu.py asserts on the CPU that every
state held here meets the conditions under which a comparison means something.  Every test prints the worst |gpu - ref| / bound
(pytest -s); MEASURED.md keeps those of the run that went with this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (the wide case runs this file as a script, in a process of its own)
    sys.path.insert(0, ROOT)

import excitation_headings_inputs as xi  # noqa: E402
import spectral_ref as sr  # noqa: E402
from test_gpu_parity import MODE_IDS, MODES, TIGHT_TOL, assert_mode_was_used, make_gpu_mode, relerr  # noqa: E402
from test_gpu_spectral_waves import ENTRIES, HF, _run_entry, check_rows, prefilled  # noqa: E402,F401

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not sr.longdouble_ok(), reason="np.longdouble is not wider than FP64 here: no high-precision reference")]

_cases, _spectra = {}, {}


def case_of(N):
    if N not in _cases:
        _cases[N] = xi.build_case(N)
    return _cases[N]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def spectral(h, kw):
    h.add_waves_irregular(spectral=True, **kw)


def own_spectrum(h, kw):
    """the context's spectrum, which is the one the CPU checks took for these parameters"""
    key = tuple(sorted(kw.items()))
    if key not in _spectra:
        _spectra[key] = sr.oracle_spectrum(kw)
    spec = h.irreg_spectrum()
    assert all(np.array_equal(spec[q], _spectra[key][q]) for q in ("f", "S", "df", "phase")), "the spectrum differs from the CPU oracle's"
    return spec


def waves_at(h, times):
    """the wave rows of every body at the model's own evaluation, of a HydroForces or a HydroGroup"""
    return np.stack([np.concatenate([s.compute_waves(float(t)) for s in getattr(h, "shards", [h])]) for t in times])


def motion_of(N, seed):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    return PrescribedMotion(N, rest_positions(case_of(N)), seed=seed)


def status_of(HydroError, fn):
    with pytest.raises(HydroError) as e:
        fn()
    return e.value.status


# ---- 1. mixed bodies, per-body grids ---------------------------------------------------------------
@pytest.mark.parametrize("N,kw", [(3, xi.KW), (3, xi.KW_TILE), (5, xi.KW)], ids=["N3-nf12", "N3-nf257", "N5-nf12"])
def test_mixed_bodies_on_grids_of_their_own(HF, N, kw):
    """Grids of 1, 2, 3 and 5 (unevenly spaced) nodes, tables on frequency lists of 64, 23 and 40 entries beside rao_w of 64, bodies
    without tables under the uniform heading: every row of every body within the bound inside the ramp, past it, without ramp
    (t <= 0 too) and at t = 1e4 s.  A body without tables keeps its bits, every other body moves; clearing restores the bits."""
    case, nf = case_of(N), kw["nfrequencies"]
    worst = 0.0
    for kind, whiches in (("uniform", (xi.UNIFORM_HEADING,)), ("spread", ("A", "B"))):
        tables = xi.tables_of(kind, N)
        for wkw, times in ((kw, xi.TIMES), (dict(kw, ramp_duration=0.0), xi.TIMES_NO_RAMP)):
            h = HF.from_case(case)
            xi.apply_tables(h, tables)
            assert [h.excitation_rao_headings_size(b) for b in range(N)] == [(0, 0) if tb is None else (tb[0].size, tb[1].size) for tb in tables]
            spectral(h, wkw)
            spec, rd = own_spectrum(h, wkw), wkw["ramp_duration"]
            base = waves_at(h, times)
            F0, B0 = xi.reference(case, spec, tables, None, rd, times)
            worst = max(worst, check_rows(f"N {N} {kind}, no directions", base, F0, B0))
            for which in whiches:
                what = f"N {N} nf {nf} {kind} {which} ramp {rd}"
                theta = xi.directions(nf, which)
                h.set_wave_directions(theta)
                F, B = xi.reference(case, spec, tables, theta, rd, times)
                xi.check_signal(F, B, what)
                if kind == "spread":
                    xi.check_moves(case, spec, tables, theta, rd, times, what)
                got = waves_at(h, times)
                worst = max(worst, check_rows(what, got, F, B))
                for b, tb in enumerate(tables):
                    r = slice(6 * b, 6 * b + 6)
                    assert same_bits(got[:, r], base[:, r]) == (tb is None), (what, b)
            h.set_wave_directions(None)
            assert same_bits(waves_at(h, times), base)
            h.close()
    print(f"mixed bodies N {N} nf {nf}: worst |gpu - ref| / B = {worst:.3f}")


# ---- 2. every way a step can run -------------------------------------------------------------------
_step_refs = {}


def _step_reference(HF, kind, which):
    if kind not in _step_refs:
        case, tables = case_of(3), xi.tables_of(kind, 3)
        times = xi.step_times(xi.step_count(32))
        probe = HF.from_case(case)
        xi.apply_tables(probe, tables)
        spectral(probe, xi.KW)
        theta = xi.directions(xi.KW["nfrequencies"], which)
        probe.set_wave_directions(theta)
        bits = waves_at(probe, times)
        F, B = xi.reference(case, own_spectrum(probe, xi.KW), tables, theta, xi.RAMP, times)
        probe.close()
        xi.check_signal(F, B, f"steps {kind}")
        check_rows(f"steps {kind}: hc_compute_waves", bits, F, B)
        _step_refs[kind] = dict(tables=tables, theta=theta, times=times, F=F, B=B, bits=bits)
    return _step_refs[kind]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_every_way_a_step_can_run_under_directions(HF, mode, monkeypatch):
    """Look-ahead 32 / 16 / 0 x AQL dispatch / HIP launches (HC_DIRECT, read at finalize), and inside each: pass schedules -1 / 0 / 1 x
    hc_step, hc_step_many, hc_step_device on a caller's stream, hc_step_begin / hc_step_end, 2 L + 3 steps on a pre-filled history, under
    the uniform heading (a body without tables, a one-node grid) and under spread A.  Per step: the wave rows within B and the bits of
    hc_compute_waves(t) of a fresh context; hydrostatics and radiation the bits of a twin on the same path that never saw a direction
    or a heading table; the total on the twin's total with the wave rows exchanged."""
    case, motion = case_of(3), motion_of(3, 33)
    worst = 0.0
    for kind, which in (("uniform", xi.UNIFORM_HEADING), ("spread", "A")):
        r = _step_reference(HF, kind, which)
        times = r["times"][:xi.step_count(mode[0])]
        for sched in (-1, 0, 1):
            for entry in ENTRIES:
                what = f"{kind} mode {mode} schedule {sched} {entry}"
                twin_rows = {}
                for directed in (False, True):
                    gpu = make_gpu_mode(HF, case, mode, monkeypatch)
                    gpu.set_pass_schedule(sched)
                    if directed:
                        xi.apply_tables(gpu, r["tables"])
                    spectral(gpu, xi.KW)
                    if directed:
                        gpu.set_wave_directions(r["theta"])
                    prefilled(gpu, motion, times[0], xi.STEP_DT, xi.STEP_S)
                    gpu.enable_profiling(1)
                    seen = []

                    def after_step(k, total, components_valid):
                        nonlocal worst
                        if not components_valid:
                            return
                        hs, rad, wv = gpu.components()
                        if not directed:
                            twin_rows[k] = (hs, rad, wv, total)
                            return
                        worst = max(worst, check_rows(f"{what}: wave rows of step {k}", wv, r["F"][k], r["B"][k]))
                        assert same_bits(wv, r["bits"][k]), f"{what}: wave rows of step {k} differ in bits from hc_compute_waves({times[k]!r})"
                        assert same_bits(hs, twin_rows[k][0]), f"{what}: hydrostatics of step {k} differ from the twin's"
                        assert same_bits(rad, twin_rows[k][1]), f"{what}: radiation of step {k} differs from the twin's"
                        assert not same_bits(wv, twin_rows[k][2]), f"{what}: step {k}"
                        assert relerr(total, (twin_rows[k][3] - twin_rows[k][2]) + wv) <= TIGHT_TOL, f"{what}: total of step {k}"
                        seen.append(k)

                    _run_entry(gpu, entry, motion, times, after_step)
                    if directed:
                        assert seen == sorted(twin_rows) and len(seen) >= len(times) // 5 and seen[-1] == len(times) - 1, what
                        if entry != "hc_step_many":
                            assert seen == list(range(len(times))), what  # no step is left out
                        p = gpu.profile()
                        if entry != "hc_step_device":  # (a caller's stream always takes HIP launches)
                            assert_mode_was_used(gpu, mode, len(times) // 2)
                        if mode[0]:
                            assert p["block_kernel_launches"] > 0 and p["scatter_kernel_launches"] > 0, (what, p)
                        else:
                            assert p["block_kernel_launches"] == 0 and p["conv_kernel_launches"] > 0, (what, p)
                    gpu.close()
    print(f"steps under directions {mode}: worst |gpu - ref| / B = {worst:.3f}")


# ---- 3. changes in the middle of a block -----------------------------------------------------------
def fresh_in_state(make, case, tables, kw, theta, history, lookahead, sched):
    h = make(case)
    h.set_lookahead(lookahead)
    h.set_pass_schedule(sched)
    xi.apply_tables(h, tables)
    spectral(h, kw)
    h.set_wave_directions(theta)
    h.set_history(*history)
    return h


def walk(HF, N, lookahead, sched, make, make_twin, what):
    """One context (or group) through xi.WALK, every change in the middle of a look-ahead block and followed by more than a block.
    Returns the worst |gpu - ref| / B."""
    case, motion = case_of(N), motion_of(N, 60 + N)
    segs = xi.walk_segments(lookahead)
    times = xi.step_times(sum(segs))
    gpu, twin = make(case), make_twin(case)
    for h in (gpu, twin):
        h.set_lookahead(lookahead)
        h.set_pass_schedule(sched)
    xi.apply_tables(gpu, xi.walk_tables(N, 0))
    for h in (gpu, twin):
        spectral(h, xi.KW)
        prefilled(h, motion, times[0], xi.STEP_DT, xi.STEP_S)
    first = getattr(gpu, "shards", [gpu])[0]
    first.enable_profiling(1)
    k, worst, fresh, bitwise_totals, compared = 0, 0.0, None, 0, 0
    for (name, change, seed1, kw, which), n in zip(xi.WALK, segs):
        tables, theta = xi.walk_tables(N, seed1), xi.directions(kw["nfrequencies"], which)
        if change == "directions":
            gpu.set_wave_directions(theta)
        elif change == "tables":
            gpu.set_body_excitation_rao_headings(1, *tables[1])
        elif change == "model":
            for h in (gpu, twin):
                spectral(h, kw)
            assert gpu.wave_directions().size == 0, name  # every wave setter drops the directions
            gpu.set_wave_directions(theta)
        assert np.array_equal(gpu.wave_directions(), np.zeros(0) if theta is None else theta), name
        if change is not None:
            fresh = fresh_in_state(HF.from_case, case, tables, kw, theta, first.get_history(), lookahead, sched)
        F, B = xi.reference(case, own_spectrum(first, kw), tables, theta, xi.RAMP, times[k:k + n])
        xi.check_signal(F, B, f"{what} {name}")
        for j in range(n):
            t = float(times[k + j])
            st = motion.state(t)
            at = f"{what} {name}, step {k + j}"
            fg, ft = gpu.step(t, *st), twin.step(t, *st)
            (hs, rad, wv), (hs_t, rad_t, wv_t) = gpu.components(), twin.components()
            worst = max(worst, check_rows(at, wv, F[j], B[j]))
            assert same_bits(hs, hs_t) and same_bits(rad, rad_t), f"{at}: hydrostatics or radiation differ from the twin's"
            assert same_bits(wv, wv_t) == (theta is None), f"{at}: the wave rows against the twin without directions"
            assert relerr(fg, (ft - wv_t) + wv) <= TIGHT_TOL, f"{at}: the total against the twin's with the wave rows exchanged"
            if fresh is not None:
                ff = fresh.step(t, *st)
                hs_f, rad_f, wv_f = fresh.components()
                assert same_bits(wv, wv_f), f"{at}: the wave rows differ from those of a fresh context created in this state"
                assert same_bits(wv, fresh.compute_waves(t)) and same_bits(hs, hs_f), at
                assert relerr(rad, rad_f) <= TIGHT_TOL and relerr(fg, ff) <= TIGHT_TOL, at
                bitwise_totals += same_bits(fg, ff)
                compared += 1
        if fresh is not None:
            fresh.close()
        k += n
    assert k == len(times) and compared == len(times) - segs[0]
    if lookahead:
        p = first.profile()
        assert p["block_kernel_launches"] >= len(segs) and p["scatter_kernel_launches"] > 0, p
    print(f"{what}: worst |gpu - ref| / B = {worst:.3f}; total bitwise that of the fresh context in {bitwise_totals} of {compared} steps")
    gpu.close()
    twin.close()
    return worst


@pytest.mark.parametrize("sched", [-1, 0, 1], ids=["adaptive", "pass_at_block_start", "pass_one_block_ahead"])
@pytest.mark.parametrize("lookahead", [16, 32])
def test_changes_in_the_middle_of_a_block(HF, lookahead, sched):
    """(a) non-uniform directions set, (b) changed, (c) one body's tables replaced under them, (d) cleared, (e) a wave setter and
    directions again, one after another on one context, each a few steps into a look-ahead block: every later step has the wave rows
    of a fresh context created in that state and given the history (bitwise, and the bits of its hc_compute_waves), stays within B of
    the reference, and keeps the twin's hydrostatic and radiation bits."""
    walk(HF, 3, lookahead, sched, HF.from_case, HF.from_case, f"walk la {lookahead} schedule {sched}")


# ---- 4. row shards ---------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards_under_a_uniform_heading_and_the_walk(HF, G):
    """Five bodies behind hc_step_multi.  Uniform heading: one shard holds only bodies without tables (it returns early and keeps its
    rows), another only bodies with tables; the gathered wave rows are bitwise those of one context and within B.  Then the walk of
    case 3 under non-uniform directions on a group against one context."""
    from hydrochrono_amd.hydro import HydroGroup
    N, case, motion = 5, case_of(5), motion_of(5, 81)
    tables, nf = xi.tables_of("uniform", N), xi.KW["nfrequencies"]
    one, grp = HF.from_case(case), HydroGroup.from_case(case, G)
    owns = [{tables[b] is not None for b in range(s.b0, s.b1)} for s in grp.shards]
    assert {True} in owns and {False} in owns, owns
    times = xi.step_times(12)
    for h in (one, grp):
        xi.apply_tables(h, tables)
        spectral(h, xi.KW)
        prefilled(h, motion, times[0], xi.STEP_DT, xi.STEP_S)
    before, base = [waves_at(s, times) for s in grp.shards], waves_at(one, times)
    theta = xi.directions(nf, xi.UNIFORM_HEADING)
    for h in (one, grp):
        h.set_wave_directions(theta)
    assert all(np.array_equal(s.wave_directions(), theta) for s in grp.shards)
    for s, own, rows in zip(grp.shards, owns, before):
        assert same_bits(waves_at(s, times), rows) == (own == {False}), (s.b0, own)
    F, B = xi.reference(case, own_spectrum(one, xi.KW), tables, theta, xi.RAMP, times)
    xi.check_signal(F, B, f"shards G {G}")
    worst = 0.0
    for k, t in enumerate(times):
        st = motion.state(float(t))
        f1, fg = one.step(float(t), *st), grp.step(float(t), *st)
        w1, wg = one.components()[2], grp.components()[2]
        worst = max(worst, check_rows(f"G {G}: gathered wave rows of step {k}", wg, F[k], B[k]))
        assert same_bits(wg, w1), f"G {G}: step {k}"
        assert relerr(fg, f1) <= TIGHT_TOL
    whole = waves_at(one, times)
    for s in grp.shards:
        assert same_bits(waves_at(s, times), whole[:, 6 * s.b0:6 * s.b1]), (G, s.b0)
    # under the uniform heading a body may lose its tables: it goes back to its {6,1,nw} table at once, the last one of a context
    # or of a shard too (no body with tables is left there to ask for the rebuild)
    for b in [b for b, tb in enumerate(tables) if tb is not None]:
        for h in (one, grp):
            h.set_body_excitation_rao_headings(b, [], [], [], [])
        now = waves_at(one, times)
        assert same_bits(now[:, :6 * b + 6], base[:, :6 * b + 6]) and same_bits(now[:, 6 * b + 6:], whole[:, 6 * b + 6:]), b
        assert same_bits(waves_at(grp, times), now), b
    assert same_bits(waves_at(one, times), base) and np.array_equal(one.wave_directions(), theta)
    one.close()
    grp.close()
    worst = max(worst, walk(HF, N, 32, 0, lambda c: HydroGroup.from_case(c, G), lambda c: HydroGroup.from_case(c, G), f"shards G {G} walk"))
    print(f"shards G {G}: worst |gpu - ref| / B = {worst:.3f}")


@pytest.mark.parametrize("G", [2, 3])
def test_row_shards_under_a_regular_wave(HF, G):
    """A regular wave with a direction: bodies 3 and 4 take their magnitudes from heading tables on their own frequency lists, every
    row its phase from body 0, which has none and lives on another shard.  Coefficients by the regular_coeffs comparison of
    tests/test_gpu_directional.py, step forces within the bound of |m| A cos(w t + phi), the gathered rows bitwise one context's."""
    from hydrochrono_amd.hydro import HydroGroup
    N, case, motion = 5, case_of(5), motion_of(5, 82)
    tables = xi.tables_of("regular", N)
    one, grp, plain = HF.from_case(case), HydroGroup.from_case(case, G), HF.from_case(case)
    plain.add_waves_none()
    assert all(tables[b] is None for b in range(grp.shards[0].b0, grp.shards[0].b1)) and tables[grp.shards[-1].b1 - 1] is not None
    for h in (one, grp):
        xi.apply_tables(h, tables)
        h.add_waves_regular(xi.REG_AMP, xi.REG_OMEGA)
    m0, p0, k0 = one.regular_coeffs()
    t0 = xi.regular_tab(case, tables, None)
    assert np.allclose(m0, t0["X"][:, 0], rtol=1e-14, atol=0) and np.allclose(p0, t0["P_all"][:, 0], rtol=1e-13, atol=1e-15)
    base = waves_at(one, xi.REG_TIMES)
    for h in (one, grp):
        h.set_wave_directions([xi.REG_HEADING])
    m1, p1, k1 = one.regular_coeffs()
    tab = xi.regular_tab(case, tables, xi.REG_HEADING)
    assert k1 == k0 and np.allclose(m1, tab["X"][:, 0], rtol=1e-14, atol=0) and np.allclose(p1, tab["P_all"][:, 0], rtol=1e-13, atol=1e-15)
    for b, tb in enumerate(tables):
        r = slice(6 * b, 6 * b + 6)
        assert (same_bits(m1[r], m0[r]) and same_bits(p1[r], p0[r])) == (tb is None), b
    for s in grp.shards:
        assert all(same_bits(a, b) for a, b in zip(s.regular_coeffs()[:2], (m1, p1))), s.b0
    F, B = xi.regular_reference(case, tables, xi.REG_HEADING, xi.REG_TIMES)
    xi.check_signal(F, B, f"regular G {G}")
    got = waves_at(one, xi.REG_TIMES)
    worst = check_rows(f"regular G {G}: hc_compute_waves", got, F, B)
    assert same_bits(waves_at(grp, xi.REG_TIMES), got) and same_bits(got[:, :18], base[:, :18]) and not same_bits(got[:, 18:24], base[:, 18:24])
    times = xi.step_times(6)
    Fs, Bs = xi.regular_reference(case, tables, xi.REG_HEADING, times)
    for h in (one, grp, plain):
        prefilled(h, motion, times[0], xi.STEP_DT, xi.STEP_S)
    for k, t in enumerate(times):
        st = motion.state(float(t))
        f1, fg, f0 = one.step(float(t), *st), grp.step(float(t), *st), plain.step(float(t), *st)
        (hs, rad, w1), wg = one.components(), grp.components()[2]
        worst = max(worst, check_rows(f"regular G {G}: wave rows of step {k}", wg, Fs[k], Bs[k]))
        assert same_bits(wg, w1) and relerr(fg, f1) <= TIGHT_TOL and relerr(f1, f0 + w1) <= TIGHT_TOL, k
        assert all(same_bits(a, b) for a, b in zip((hs, rad), plain.components()[:2])), k
    for h in (one, grp):
        h.set_wave_directions(None)
    assert same_bits(waves_at(one, xi.REG_TIMES), base) and same_bits(waves_at(grp, xi.REG_TIMES), base)
    assert all(same_bits(a, b) for a, b in zip(one.regular_coeffs()[:2], (m0, p0)))
    print(f"regular wave on {G} shards: worst |gpu - ref| / B = {worst:.3f}")
    for h in (one, grp, plain):
        h.close()


def _wide_run(out_path):
    """(run as a script, in a process of its own, as the wide case of tests/test_gpu_spectral_waves.py)"""
    import torch  # noqa: F401
    from hydrochrono_amd.hydro import HydroForces
    N = xi.WIDE_N
    case, times = xi.build_case(N), xi.step_times(xi.WIDE_STEPS, 1.0)
    gpu = HydroForces.from_case(case)
    xi.apply_tables(gpu, xi.tables_of("spread", N))
    spectral(gpu, xi.KW)
    gpu.set_wave_directions(xi.directions(xi.KW["nfrequencies"], xi.UNIFORM_HEADING))
    gpu.set_lookahead(16)
    _cases[N] = case
    motion = motion_of(N, 71)
    prefilled(gpu, motion, times[0], xi.STEP_DT, xi.WIDE_S)
    tot, comp = [], []
    for t in times:
        tot.append(gpu.step(float(t), *motion.state(float(t))))
        comp.append(np.stack(gpu.components()))
    sp = gpu.irreg_spectrum()
    cw = waves_at(gpu, times)
    gpu.add_waves_none()  # the same steps again without waves: what the totals hold beside the wave rows
    gpu.reset_history()
    prefilled(gpu, motion, times[0], xi.STEP_DT, xi.WIDE_S)
    still = np.stack([gpu.step(float(t), *motion.state(float(t))) for t in times])
    np.savez(out_path, tot=np.stack(tot), comp=np.stack(comp), still=still, cw=cw, fused=gpu.profile()["wide_fused_steps"],
             **{"spec_" + k: v for k, v in sp.items()})


def test_wide_system_under_a_uniform_heading(tmp_path):
    """6 N = 1026 rows (the wide step), a short IRF, three steps, 171 bodies on grids of 2, 5 and 3 nodes or none: the wave rows
    within B and the bits of hc_compute_waves; the total on the same steps without waves plus the wave rows."""
    N = xi.WIDE_N
    out = str(tmp_path / "wide.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("HC_WIDE_FUSED", "HYDROCHRONO_AMD_FLAVOR")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--wide", out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    a = np.load(out)
    assert int(a["fused"]) > 0
    case, tables, times = xi.build_case(N, S=2), xi.tables_of("spread", N), xi.step_times(xi.WIDE_STEPS, 1.0)
    spec = {k: a["spec_" + k] for k in ("f", "S", "df", "phase")}
    ref_spec = sr.oracle_spectrum(xi.KW)
    assert all(np.array_equal(spec[q], ref_spec[q]) for q in spec)
    theta = xi.directions(xi.KW["nfrequencies"], xi.UNIFORM_HEADING)
    F, B = xi.reference(case, spec, tables, theta, xi.RAMP, times)
    xi.check_signal(F, B, "wide")
    wv = a["comp"][:, 2]
    worst = check_rows("wide", wv, F, B)
    assert wv.shape == (xi.WIDE_STEPS, 6 * N) and same_bits(a["cw"], wv)
    for k in range(xi.WIDE_STEPS):
        assert relerr(a["tot"][k], a["still"][k] + wv[k]) <= TIGHT_TOL, k
    print(f"wide: worst |gpu - ref| / B = {worst:.3f}")


# ---- 5. grid edges ---------------------------------------------------------------------------------
def node_context(HF, case, tb, j, kw):
    """a context whose body holds, through hc_set_excitation_rao, the table of heading node j"""
    dirs, w, mag, ph = tb
    o = HF.from_case(dict(case, bodies=[dict(case["bodies"][0], w=w, ex_mag=mag[:, j:j + 1], ex_phase=ph[:, j:j + 1])]))
    spectral(o, kw)
    return o


def test_grid_edges(HF):
    """No extrapolation, no wrap-around, weight exactly 0 on a node, one node valid on the node only -- on an unevenly spaced grid
    whose first node is 0.0, one ulp either side of both ends, at theta +- 2 pi, at -0.0, on a one-node grid, and with neighbouring
    phases more than pi apart (the blend is on the values as given)."""
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    case, kw, times = case_of(1), xi.KW_NO_RAMP, xi.EDGE_TIMES
    nf, g = kw["nfrequencies"], xi.EDGE_GRID
    tb = xi.edge_tables("grid")[0]
    h = HF.from_case(case)
    h.set_body_excitation_rao_headings(0, *tb)
    spectral(h, kw)
    spec = own_spectrum(h, kw)
    # on every node, both ends included: the bits of hc_set_excitation_rao with that node's table
    for j in range(g.size):
        h.set_wave_directions(np.full(nf, g[j]))
        o = node_context(HF, case, tb, j, kw)
        assert same_bits(waves_at(h, times), waves_at(o, times)), f"node {j}"
        o.close()
    # -0.0 on the first node 0.0: accepted, the bits of +0.0
    h.set_wave_directions(np.full(nf, 0.0))
    at_zero = waves_at(h, times)
    h.set_wave_directions(np.full(nf, -0.0))
    assert same_bits(waves_at(h, times), at_zero)
    # accepted and held to the reference: one ulp inside either end, between uneven nodes
    worst, held = 0.0, {name: (tabs, th) for name, tabs, th in xi.edge_states()}
    for name in ("one ulp inside the first node", "one ulp inside the last node", "between uneven nodes"):
        th = np.full(nf, held[name][1])
        h.set_wave_directions(th)
        F, B = xi.reference(case, spec, [tb], th, 0.0, times)
        xi.check_signal(F, B, name)
        worst = max(worst, check_rows(name, waves_at(h, times), F, B))
    # refused, and nothing changes: one ulp outside either end, an in-grid direction +- 2 pi, one component alone outside
    keep_dirs, keep = h.wave_directions(), waves_at(h, times)
    one_out = np.full(nf, 0.4)
    one_out[nf - 1] = np.nextafter(g[-1], np.inf)
    for bad in (np.full(nf, np.nextafter(g[0], -1.0)), np.full(nf, np.nextafter(g[-1], np.inf)), np.full(nf, 0.4 + 2 * np.pi),
                np.full(nf, 0.4 - 2 * np.pi), np.full(nf, 1.0 - 2 * np.pi), one_out):
        assert status_of(HydroError, lambda: h.set_wave_directions(bad)) == capi.HC_ERR_INVALID, bad[-1]
        assert same_bits(h.wave_directions(), keep_dirs) and h.excitation_rao_headings_size(0) == (g.size, tb[1].size)
        assert same_bits(waves_at(h, times), keep), bad[-1]
    h.close()
    # a one-node grid: accepted on the node only, with the bits of that table
    tb1 = xi.edge_tables("one")[0]
    node = float(tb1[0][0])
    h = HF.from_case(case)
    h.set_body_excitation_rao_headings(0, *tb1)
    spectral(h, kw)
    base = waves_at(h, times)
    for bad in (np.nextafter(node, -1.0), np.nextafter(node, 1.0), node + 2 * np.pi):
        assert status_of(HydroError, lambda: h.set_wave_directions(np.full(nf, bad))) == capi.HC_ERR_INVALID, bad
        assert h.wave_directions().size == 0 and same_bits(waves_at(h, times), base)
    h.set_wave_directions(np.full(nf, node))
    o = node_context(HF, case, tb1, 0, kw)
    got = waves_at(h, times)
    assert same_bits(got, waves_at(o, times)) and not same_bits(got, base)
    F, B = xi.reference(case, spec, [tb1], np.full(nf, node), 0.0, times)
    worst = max(worst, check_rows("one-node grid", got, F, B))
    o.close()
    h.close()
    # neighbouring headings whose phases differ by more than pi: the linear blend of the values as given
    tbj = xi.edge_tables("jump")[0]
    th = np.full(nf, held["phases more than pi apart"][1])
    h = HF.from_case(case)
    h.set_body_excitation_rao_headings(0, *tbj)
    spectral(h, kw)
    h.set_wave_directions(th)
    F, B = xi.reference(case, spec, [tbj], th, 0.0, times)
    xi.check_signal(F, B, "phase jump")
    worst = max(worst, check_rows("phases more than pi apart", waves_at(h, times), F, B))
    h.close()
    print(f"grid edges: worst |gpu - ref| / B = {worst:.3f}")


# ---- 6. refused calls leave nothing behind ---------------------------------------------------------
def test_refused_table_replacements_leave_nothing_behind(HF):
    """With non-uniform directions in force: a replacement grid that no longer covers them and a removal (HC_ERR_INVALID); on a
    regular wave with a direction: tables whose frequency list no longer brackets omega (HC_ERR_OUT_OF_RANGE), a grid that does not
    hold the direction, on one context and on a single shard of three.  After each the sizes, the directions, the coefficients and
    the next three steps are those of a twin that never made the call, and a following valid call does what it does on the twin."""
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError, HydroGroup
    N, case, motion = 3, case_of(3), motion_of(3, 91)
    tables, nf = xi.tables_of("spread", N), xi.KW["nfrequencies"]
    theta = xi.directions(nf, "A")
    times = xi.step_times(40)
    narrow = xi.grid_tables(np.array([-0.4, 0.1, 0.8]), 17, 970)   # does not reach the directions at -0.5 and 0.9
    other = xi.layout_tables(xi.LAYOUTS[("spread", N)], 3)[1]        # a valid replacement
    short = xi.grid_tables(xi.GRIDS["G5"], 23, 971)
    short = (short[0], short[1] * (1.0 / 3.2)) + short[2:]           # a frequency list that ends at 1.0 rad/s, below the regular wave
    away = xi.grid_tables(np.array([0.5, 0.9]), 23, 972)             # a grid that does not hold the regular wave's direction

    def prepared(make, regular):
        h = make(case)
        xi.apply_tables(h, tables)
        (h.add_waves_regular(xi.REG_AMP, xi.REG_OMEGA) if regular else spectral(h, xi.KW))
        h.set_wave_directions([xi.REG_HEADING] if regular else theta)
        prefilled(h, motion, times[0], xi.STEP_DT, xi.STEP_S)
        return h

    def state(h, regular):
        s0 = getattr(h, "shards", [h])
        return ([[s.excitation_rao_headings_size(b) for b in range(N)] for s in s0], [s.wave_directions() for s in s0],
                [s.regular_coeffs()[:2] for s in s0] if regular else None)

    def same_state(x, y):
        return (x[0] == y[0] and all(same_bits(a, b) for a, b in zip(x[1], y[1]))
                and (x[2] is None or all(same_bits(a[0], b[0]) and same_bits(a[1], b[1]) for a, b in zip(x[2], y[2]))))

    k = 0
    for regular in (False, True):
        for sharded in (False, True):
            make = (lambda c: HydroGroup.from_case(c, 3)) if sharded else HF.from_case
            h, twin = prepared(make, regular), prepared(make, regular)
            target = h.shards[1] if sharded else h  # body 1 is the body of shard 1
            calls = [("a grid that no longer covers the directions", lambda: target.set_body_excitation_rao_headings(1, *(away if regular else narrow)), capi.HC_ERR_INVALID)]
            if regular:
                calls.append(("a frequency list that no longer brackets omega", lambda: target.set_body_excitation_rao_headings(1, *short), capi.HC_ERR_OUT_OF_RANGE))
            else:
                calls.append(("removal under non-uniform directions", lambda: target.set_body_excitation_rao_headings(1, [], [], [], []), capi.HC_ERR_INVALID))
            for name, call, code in calls:
                what = f"{'regular' if regular else 'spectral'}, {'one shard of three' if sharded else 'one context'}: {name}"
                before = state(h, regular)
                assert status_of(HydroError, call) == code, what
                assert same_state(state(h, regular), before) and same_state(before, state(twin, regular)), what
                for _ in range(3):
                    t = float(times[k])
                    st = motion.state(t)
                    assert same_bits(h.step(t, *st), twin.step(t, *st)), f"{what}: step {k}"
                    assert all(same_bits(a, b) for a, b in zip(h.components(), twin.components())), f"{what}: step {k}"
                    k += 1
                # a following valid call: the directions again (every grid still has to hold them), then a valid replacement
                for x in (h, twin):
                    x.set_wave_directions([xi.REG_HEADING] if regular else theta)
                    x.set_body_excitation_rao_headings(1, *other)
                assert same_state(state(h, regular), state(twin, regular)), what
                t = float(times[k])
                st = motion.state(t)
                fh, ft = h.step(t, *st), twin.step(t, *st)
                assert same_bits(fh, ft) and same_bits(h.components()[2], twin.components()[2]), what
                if not regular:
                    F, B = xi.reference(case, own_spectrum(getattr(h, "shards", [h])[0], xi.KW), tables[:1] + [other] + tables[2:], theta, xi.RAMP, [t])
                    check_rows(what, h.components()[2], F[0], B[0])
                k += 1
                for x in (h, twin):
                    x.set_body_excitation_rao_headings(1, *tables[1])
            h.close()
            twin.close()
            k = 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--wide":
        _wide_run(sys.argv[2])
