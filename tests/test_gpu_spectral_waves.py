"""The spectral (component-sum) wave excitation -- hc_set_wave_irregular_spectral, wave mode 3 of the step kernels -- against the
high-precision reference of tests/spectral_ref.py, row by row: |gpu - ref| <= B with the derived bound B of that file, never
vector-relative.  The CPU oracle has no such mode (the reference project has none), so where a whole step is checked the oracle runs
with add_waves_none() for the hydrostatic and radiation components and the wave rows come from the reference.

Every test prints the worst |gpu - ref| / B it saw (pytest -s); MEASURED.md keeps those of the run that went with this file.
The input sets live in spectral_ref.INPUT_SETS, which tests/test_spectral_ref_cpu.py checks on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (the wide case runs this file as a script, in a process of its own)
    sys.path.insert(0, ROOT)

import spectral_ref as sr  # noqa: E402
from cases import load_into_oracle  # noqa: E402
from test_gpu_parity import MODE_IDS, MODES, TIGHT_TOL, assert_mode_was_used, make_gpu_mode, relerr  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not sr.longdouble_ok(), reason="np.longdouble is not wider than FP64 here: no high-precision reference")]

_cases = {}


def _case(key):
    if key not in _cases:
        _cases[key] = sr.build_case(key)
    return _cases[key]


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def spectral_kw(s):
    return dict(s["kw"], spectral=True)


def check_rows(what, got, F, B):
    """|got - F| <= B for every row of every time; returns the worst ratio (rows with B = 0 must be exact)."""
    got, F, B = np.atleast_2d(got), np.atleast_2d(F), np.atleast_2d(B)
    assert got.shape == F.shape == B.shape, (what, got.shape, F.shape)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got.astype(np.longdouble) - F).astype(np.float64)
    zero = B == 0.0
    assert np.all(err[zero] == 0.0), f"{what}: a row whose bound is zero is not exactly zero"
    ratio = float(np.max(err[~zero] / B[~zero])) if np.any(~zero) else 0.0
    if ratio > 1.0:
        k, r = np.unravel_index(np.argmax(np.where(zero, 0.0, err / np.where(zero, 1.0, B))), err.shape)
        raise AssertionError(f"{what}: |gpu - ref| / B = {ratio:.3f} at time index {k}, row {r}: gpu {got[k, r]!r}, ref {float(F[k, r])!r}, B {B[k, r]:.3e}")
    return ratio


def prefilled(h, motion, t0, dt, S):
    """A history that covers the IRF window before t0, on the step grid (h: a context, a group of shards or an oracle)."""
    nh = S + 4
    th = t0 - dt * np.arange(1, nh + 1)
    vh = np.stack([motion.velocity6(t) for t in th])
    (h.prefill_history if hasattr(h, "prefill_history") else h.set_history)(th, vh)


# ---- a. rows and component counts --------------------------------------------------------------
@pytest.mark.parametrize("sid", [k for k in sr.INPUT_SETS if k.startswith("rows-")])
def test_rows_and_component_counts(HF, sid):
    """N in {1, 2, 3, 5, 9} x nfrequencies in {1, 2, 15, 16, 17, 64, 1000, 2048} (and the sphere, three of whose rows are zero)
    through hc_compute_waves at times on no grid.  nfrequencies = 1: the single trapezoid width is 0, the force exactly zero."""
    s = sr.INPUT_SETS[sid]
    case = _case(s["case"])
    gpu = HF.from_case(case)
    gpu.add_waves_irregular(**spectral_kw(s))
    spec = gpu.irreg_spectrum()
    orc_spec = sr.oracle_spectrum(s["kw"])  # what the CPU test took for this set
    for name in ("f", "S", "df", "phase"):
        assert np.array_equal(spec[name], orc_spec[name]), name
    assert gpu.sizes()["nf"] == s["kw"]["nfrequencies"]
    F, B = sr.reference(case, spec, s["kw"]["ramp_duration"], s["times"])
    got = np.stack([gpu.compute_waves(t) for t in s["times"]])
    ratio = check_rows(sid, got, F, B)
    if s["kw"]["nfrequencies"] == 1:
        assert np.all(got == 0.0) and np.all(B == 0.0)
    else:
        live = np.any(sr.tables(case, spec)["X"] != 0.0, axis=1)
        assert np.all(np.max(np.abs(got), axis=0)[live] > 0.0)
    print(f"{sid}: worst |gpu - ref| / B = {ratio:.3f}")
    gpu.close()


# ---- b. every way a step can run ----------------------------------------------------------------
_step_refs = {}


def _step_reference(HF, N):
    """Per N, once: the oracle's components under add_waves_none(), the reference's wave rows and bound, hc_compute_waves' bits."""
    if N not in _step_refs:
        from hydrochrono_amd.mock_chrono import PrescribedMotion
        from hydrochrono_amd.synthetic import rest_positions
        s = sr.INPUT_SETS[f"steps-N{N}"]
        case = _case(s["case"])
        motion = PrescribedMotion(N, rest_positions(case), seed=30 + N)
        times = s["times"]
        orc = load_into_oracle(case)
        orc.add_waves_none()
        prefilled(orc, motion, times[0], sr.STEP_DT, sr.STEP_S)
        tot, hs, rad = [], [], []
        for t in times:
            tot.append(orc.step(t, *motion.state(t)))
            c = orc.components()
            hs.append(c[0].copy())
            rad.append(c[1].copy())
            assert np.all(c[2] == 0.0)
        orc.close()
        probe = HF.from_case(case)
        probe.add_waves_irregular(**spectral_kw(s))
        spec = probe.irreg_spectrum()
        bits = np.stack([probe.compute_waves(t) for t in times])
        probe.close()
        F, B = sr.reference(case, spec, s["kw"]["ramp_duration"], times)
        check_rows(f"steps-N{N}: hc_compute_waves", bits, F, B)
        _step_refs[N] = dict(s=s, case=case, motion=motion, times=times, tot=np.stack(tot), hs=np.stack(hs), rad=np.stack(rad), F=F, B=B, bits=bits)
    return _step_refs[N]


ENTRIES = ("hc_step", "hc_step_many", "hc_step_device", "hc_step_begin_end")


def _run_entry(gpu, entry, motion, times, after_step):
    """Drives `times` through one entry point of the C ABI; after_step(k, total_force) after every step whose components can be read."""
    from hydrochrono_amd import capi
    lib = capi.load()
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)  # noqa: E731
    if entry == "hc_step":
        for k, t in enumerate(times):
            after_step(k, gpu.step(t, *motion.state(t)), True)
    elif entry == "hc_step_many":  # chunks of 5: the components of every fifth step, the totals of all
        for k0 in range(0, len(times), 5):
            tt = times[k0:k0 + 5]
            forces, _ = gpu.step_many(tt, np.stack([motion.packed(t) for t in tt]))
            for j in range(len(tt)):
                after_step(k0 + j, forces[j], j == len(tt) - 1)
    elif entry == "hc_step_device":
        import torch
        stream = torch.cuda.Stream()
        states = torch.tensor(np.stack([motion.packed(t) for t in times]), device="cuda")
        out = torch.zeros(len(times), gpu.D_local, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for k, t in enumerate(times):
            gpu.step_device(float(t), states[k].data_ptr(), out[k].data_ptr(), stream.cuda_stream)
            stream.synchronize()
            after_step(k, out[k].cpu().numpy(), True)
    else:
        out = np.empty(gpu.D_local)
        for k, t in enumerate(times):
            st = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in motion.state(t)]
            assert lib.hc_step_begin(gpu.ctx, float(t), *[dp(x) for x in st]) == 0
            assert lib.hc_step_end(gpu.ctx, dp(out)) == 0
            after_step(k, out.copy(), True)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("N", sr.STEP_BODIES)
def test_every_way_a_step_can_run(HF, N, mode, monkeypatch):
    """Look-ahead 32 / 16 / 0 x AQL dispatch / HIP launches, and inside each: pass schedules -1 / 0 / 1 x hc_step, hc_step_many,
    hc_step_device on a caller's stream, hc_step_begin / hc_step_end -- past one IRF window, on a pre-filled history, so that look-ahead
    blocks are in use from the second step on.  Per step: the wave rows within B of the reference and the SAME BITS as
    hc_compute_waves(t) of a fresh context (the term depends on t alone and every path runs the same code); hydrostatic and radiation
    components on the oracle (which runs without waves) at TIGHT_TOL; the total on oracle + reference within TIGHT_TOL max|total| + B."""
    r = _step_reference(HF, N)
    s, case, motion, times = r["s"], r["case"], r["motion"], r["times"]
    want_tot = r["tot"].astype(np.longdouble) + r["F"]
    worst = 0.0
    for sched in (-1, 0, 1):
        for entry in ENTRIES:
            what = f"N {N} mode {mode} schedule {sched} {entry}"
            gpu = make_gpu_mode(HF, case, mode, monkeypatch)
            gpu.set_pass_schedule(sched)
            gpu.add_waves_irregular(**spectral_kw(s))
            prefilled(gpu, motion, times[0], sr.STEP_DT, sr.STEP_S)
            gpu.enable_profiling(1)
            seen = []

            def after_step(k, total, components_valid):
                nonlocal worst
                tol = TIGHT_TOL * float(np.max(np.abs(r["tot"][k]))) + r["B"][k]
                err = np.abs(total.astype(np.longdouble) - want_tot[k]).astype(np.float64)
                assert np.all(err <= tol), f"{what}: total of step {k}: {np.max(err / tol):.3e} of its tolerance"
                if not components_valid:
                    return
                hs, rad, wv = gpu.components()
                worst = max(worst, check_rows(f"{what}: wave rows of step {k}", wv, r["F"][k], r["B"][k]))
                assert np.array_equal(wv, r["bits"][k]), f"{what}: wave rows of step {k} differ in bits from hc_compute_waves({times[k]!r})"
                assert relerr(hs, r["hs"][k]) <= TIGHT_TOL, f"{what}: hydrostatics of step {k}"
                assert relerr(rad, r["rad"][k]) <= TIGHT_TOL, f"{what}: radiation of step {k}: {relerr(rad, r['rad'][k]):.3e}"
                seen.append(k)

            _run_entry(gpu, entry, motion, times, after_step)
            assert len(seen) >= len(times) // 5
            p = gpu.profile()
            p = {q: p[q] for q in ("block_kernel_launches", "scatter_kernel_launches", "conv_kernel_launches", "mini_pass_launches", "direct_dispatches", "hip_launches")}
            if entry in ("hc_step", "hc_step_many", "hc_step_begin_end"):  # (a caller's stream always takes HIP launches)
                assert_mode_was_used(gpu, mode, len(times) // 2)
            if mode[0]:
                assert p["block_kernel_launches"] > 0 and p["scatter_kernel_launches"] > 0, (what, p)
            else:
                assert p["block_kernel_launches"] == 0 and p["conv_kernel_launches"] > 0, (what, p)
            gpu.close()
    print(f"steps-N{N} {mode}: worst |gpu - ref| / B = {worst:.3f}")


# ---- c. shards ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,G", sr.SHARD_SPLITS)
def test_row_shards_behind_step_multi(HF, N, G):
    """hc_step_multi over G row shards (uneven shares included): the gathered wave rows within B and bitwise those of one context; each
    shard's hc_compute_waves is its slice -- a shard's table is indexed by the LOCAL row."""
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    s = sr.INPUT_SETS[f"shards-N{N}"]
    case, times = _case(s["case"]), s["times"]
    motion = PrescribedMotion(N, rest_positions(case), seed=50 + N)
    one, grp = HF.from_case(case), HydroGroup.from_case(case, G)
    assert sum(h.n_local for h in grp.shards) == N and (N % G == 0 or len({h.n_local for h in grp.shards}) > 1)
    for h in (one, grp):
        h.add_waves_irregular(**spectral_kw(s))
    prefilled(one, motion, times[0], sr.STEP_DT, sr.STEP_S)
    prefilled(grp, motion, times[0], sr.STEP_DT, sr.STEP_S)
    F, B = sr.reference(case, one.irreg_spectrum(), s["kw"]["ramp_duration"], times)
    worst = 0.0
    for k, t in enumerate(times):
        st = motion.state(t)
        f1, fg = one.step(t, *st), grp.step(t, *st)
        w1, wg = one.components()[2], grp.components()[2]
        worst = max(worst, check_rows(f"N {N} G {G}: gathered wave rows of step {k}", wg, F[k], B[k]))
        assert np.array_equal(wg, w1), f"N {N} G {G}: step {k}"
        assert relerr(fg, f1) <= TIGHT_TOL
    for t in (times[3], 0.37, 33.3):
        whole = one.compute_waves(t)
        for h in grp.shards:
            assert np.array_equal(h.compute_waves(t), whole[6 * h.b0:6 * h.b1]), (N, G, h.b0, t)
    print(f"shards N {N} G {G}: worst |gpu - ref| / B = {worst:.3f}")
    one.close()
    grp.close()


# ---- d. a wide system ---------------------------------------------------------------------------
def _wide_run(out_path):
    """(run as a script, one process per library flavour / HC_WIDE_FUSED value: the switch is read once per process)"""
    import torch  # noqa: F401
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    s = sr.INPUT_SETS["wide"]
    case, times = sr.build_case(s["case"]), s["times"]
    motion = PrescribedMotion(sr.WIDE_N, rest_positions(case), seed=71)
    gpu = HydroForces.from_case(case)
    gpu.add_waves_irregular(**spectral_kw(s))
    gpu.set_lookahead(16)  # (a block may span half the IRF window at most: 0.16 s of 0.47 s)
    prefilled(gpu, motion, times[0], sr.STEP_DT, sr.WIDE_S)
    tot, wv = [], []
    for t in times:
        tot.append(gpu.step(t, *motion.state(t)))
        wv.append(gpu.components()[2])
    cw = np.stack([gpu.compute_waves(t) for t in times[:4]])
    sp = gpu.irreg_spectrum()
    np.savez(out_path, tot=np.stack(tot), wv=np.stack(wv), cw=cw, fused=gpu.profile()["wide_fused_steps"], **{"spec_" + k: v for k, v in sp.items()})


def test_wide_system_fused_and_two_launch_step(tmp_path):
    """6N = 1026 >= 1024: wide_step_kernel shares finalize_tile.  The release library's fused wide step and, on the tuning build with
    HC_WIDE_FUSED=0, the two-launch form: wave rows within B, the same bits in both and as hc_compute_waves gives; totals on the oracle
    (without waves) + reference."""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    s = sr.INPUT_SETS["wide"]
    case, times = _case(s["case"]), s["times"]
    runs = {}
    for name, env in (("release_fused", dict(HYDROCHRONO_AMD_FLAVOR="release")), ("tuning_two_launch", dict(HYDROCHRONO_AMD_FLAVOR="tuning", HC_WIDE_FUSED="0"))):
        out = str(tmp_path / (name + ".npz"))
        e = {k: v for k, v in os.environ.items() if k not in ("HC_WIDE_FUSED", "HYDROCHRONO_AMD_FLAVOR")}
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--wide", out], env=dict(e, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, (r.stdout + r.stderr)[-2000:])
        runs[name] = np.load(out)
    a, b = runs["release_fused"], runs["tuning_two_launch"]
    assert int(a["fused"]) > 0 and int(b["fused"]) == 0, (int(a["fused"]), int(b["fused"]))
    spec = {k: a["spec_" + k] for k in ("f", "S", "df", "phase")}
    F, B = sr.reference(case, spec, s["kw"]["ramp_duration"], times)
    worst = max(check_rows("wide, fused step", a["wv"], F, B), check_rows("wide, two launches", b["wv"], F, B))
    assert np.array_equal(a["wv"], b["wv"]) and np.array_equal(a["cw"], a["wv"][:4]) and np.array_equal(b["cw"], b["wv"][:4])
    motion = PrescribedMotion(sr.WIDE_N, rest_positions(case), seed=71)
    orc = load_into_oracle(case)
    orc.add_waves_none()
    prefilled(orc, motion, times[0], sr.STEP_DT, sr.WIDE_S)
    for k, t in enumerate(times):
        fo = orc.step(t, *motion.state(t))
        tol = TIGHT_TOL * float(np.max(np.abs(fo))) + B[k]
        for run in (a, b):
            assert np.all(np.abs(run["tot"][k].astype(np.longdouble) - (fo.astype(np.longdouble) + F[k])).astype(np.float64) <= tol), k
    orc.close()
    print(f"wide: worst |gpu - ref| / B = {worst:.3f}")


# ---- e. times -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["times-ramp_edges", "times-no_ramp", "times-large_t"])
def test_times_at_the_ramp_edges_without_ramp_and_large(HF, sid):
    """t in {-1, 0, tiny, just below ramp, ramp, just above}: factor 0 for t <= 0 (never negative), t / ramp below the ramp's end, 1 from
    it on; no ramp: the plain sum also at t <= 0; t = 1e4 s, 1e5 s: B grows with Theta and the kernel's cos has to reduce its
    argument properly."""
    s = sr.INPUT_SETS[sid]
    case = _case(s["case"])
    gpu = HF.from_case(case)
    gpu.add_waves_irregular(**spectral_kw(s))
    F, B = sr.reference(case, gpu.irreg_spectrum(), s["kw"]["ramp_duration"], s["times"])
    got = np.stack([gpu.compute_waves(t) for t in s["times"]])
    ratio = check_rows(sid, got, F, B)
    if sid == "times-ramp_edges":
        assert np.all(got[:2] == 0.0) and np.all(got[2:] != 0.0)
    if sid == "times-no_ramp":
        assert np.all(got != 0.0)
    print(f"{sid}: worst |gpu - ref| / B = {ratio:.3f}")
    gpu.close()


def test_same_time_twice_and_a_step_back_in_time(HF):
    """hc_step at the same t twice (the per-time cache, src/hydro_forces.cpp:742-744) and at an earlier t: the wave rows follow t."""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    s = sr.INPUT_SETS["times-cache_and_back"]
    case, times = _case(s["case"]), s["times"]
    motion = PrescribedMotion(3, rest_positions(case), seed=9)
    gpu = HF.from_case(case)
    gpu.add_waves_irregular(**spectral_kw(s))
    F, B = sr.reference(case, gpu.irreg_spectrum(), s["kw"]["ramp_duration"], times)
    prefilled(gpu, motion, times[0], sr.STEP_DT, sr.STEP_S)
    worst, rows = 0.0, []
    for k, t in enumerate(times):
        gpu.step(t, *motion.state(t))
        rows.append(gpu.components()[2])
        worst = max(worst, check_rows(f"step {k} at t = {t!r}", rows[-1], F[k], B[k]))
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(rows[3], rows[4]) and not np.array_equal(rows[2], rows[3])
    assert gpu.profile()["history_rewinds"] >= 1
    print(f"times-cache_and_back: worst |gpu - ref| / B = {worst:.3f}")
    gpu.close()


# ---- f. RAO interpolation edges -------------------------------------------------------------------
@pytest.mark.parametrize("sid", [k for k in sr.INPUT_SETS if k.startswith("rao-")])
def test_rao_interpolation_edges_and_per_body_frequency_lists(HF, sid):
    """Four bodies with different RAO lists (nw = 16, 40, 2, 1) under spectra whose components fall below the first list entry, exactly
    on entries, inside the last interval and above the last entry (tests/test_spectral_ref_cpu.py asserts that they do); whole step on
    two of the bodies' rows would hide a mix-up, so every row is held to its own B."""
    s = sr.INPUT_SETS[sid]
    case = _case(s["case"])
    gpu = HF.from_case(case)
    gpu.add_waves_irregular(**spectral_kw(s))
    spec = gpu.irreg_spectrum()
    if sid == "rao-on_list":  # the context's own frequencies hit list entries exactly
        w = np.asarray(case["bodies"][0]["w"])
        idx = (2 * np.pi * spec["f"]) / (w[-1] / w.size) - 1.0
        assert np.count_nonzero((idx == np.round(idx)) & (idx >= 0) & (idx <= 15)) >= 6
    F, B = sr.reference(case, spec, s["kw"]["ramp_duration"], s["times"])
    got = np.stack([gpu.compute_waves(t) for t in s["times"]])
    ratio = check_rows(sid, got, F, B)
    assert np.all(np.max(np.abs(got), axis=0) > 0.0)
    print(f"{sid}: worst |gpu - ref| / B = {ratio:.3f}")
    gpu.close()


# ---- g. model changes on one context ------------------------------------------------------------------
def test_model_changes_in_the_middle_of_a_block_and_the_queries(HF, tmp_path):
    """irregular (IRF) -> spectral -> regular -> spectral with another seed -> none -> spectral with the first parameters, each change
    in the middle of a look-ahead block.  After each change the wave rows are those of a fresh context with that model, bit for bit, and
    the other two components those of an undisturbed twin (which runs without waves).  In spectral mode: hc_get_spectrum as for the IRF
    model, L = nt = 0, the excitation-IRF queries refused, hc_get_eta_table copies nothing (guard words behind the caller's buffers: a
    context that held the IRF model's table before must not hand it out), the export refused."""
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from hydrochrono_amd.synthetic import rest_positions
    s1, s2 = sr.INPUT_SETS["models-first"], sr.INPUT_SETS["models-second"]
    case, times = _case(s1["case"]), s1["times"]
    motion = PrescribedMotion(3, rest_positions(case), seed=12)
    irf_kw = dict(s1["kw"], simulation_duration=30.0)
    models = [("irregular", irf_kw), ("spectral", s1["kw"]), ("regular", None), ("spectral", s2["kw"]), ("none", None), ("spectral", s1["kw"])]
    lengths = [23, 29, 21, 27, 19, 41]  # every change falls inside a block of 16 or 32 steps
    assert sum(lengths) == len(times)

    def attach(h, kind, kw):
        if kind == "irregular":
            h.add_waves_irregular(**kw)
        elif kind == "spectral":
            h.add_waves_irregular(spectral=True, **kw)
        elif kind == "regular":
            h.add_waves_regular(0.4, 1.3)
        else:
            h.add_waves_none()

    gpu, twin = HF.from_case(case), HF.from_case(case)
    twin.add_waves_none()
    for h in (gpu, twin):
        h.set_lookahead(16)
        prefilled(h, motion, times[0], sr.STEP_DT, sr.STEP_S)
    gpu.enable_profiling(1)
    lib = capi.load()
    k, worst = 0, 0.0
    for (kind, kw), n in zip(models, lengths):
        attach(gpu, kind, kw)
        fresh = HF.from_case(case)
        attach(fresh, kind, kw)
        if kind == "spectral":
            spec = gpu.irreg_spectrum()
            fs = fresh.irreg_spectrum()
            assert all(np.array_equal(spec[q], fs[q]) for q in spec)
            sz = gpu.sizes()
            assert (sz["L"], sz["nt"], sz["nf"]) == (0, 0, kw["nfrequencies"]), sz
            for call in (lambda: gpu.irreg_irf(0), lambda: gpu.export_irregular_inputs_h5(tmp_path / "never.h5")):
                with pytest.raises(HydroError) as ei:
                    call()
                assert ei.value.status == capi.HC_ERR_INVALID
            assert not (tmp_path / "never.h5").exists()
            # the buffers a caller sizes with nt = 0, and guard words behind them -- as many as the table of the IRF model before
            guard = nt_irf + 4
            tb, eb = np.full(guard, 7.25), np.full(guard, -3.5)
            assert lib.hc_get_eta_table(gpu.ctx, tb.ctypes.data_as(capi.c_double_p), eb.ctypes.data_as(capi.c_double_p)) == capi.HC_OK
            assert np.all(tb == 7.25) and np.all(eb == -3.5), "hc_get_eta_table wrote into a buffer of nt = 0 samples"
            t_, e_ = gpu.irreg_eta()
            assert t_.size == 0 and e_.size == 0
            F, B = sr.reference(case, spec, kw["ramp_duration"], times[k:k + n])
        elif kind == "irregular":
            nt_irf = gpu.sizes()["nt"]
            assert nt_irf > 0 and gpu.irreg_eta()[0].size == nt_irf
        for j in range(n):
            t = times[k + j]
            st = motion.state(t)
            fg, ft = gpu.step(t, *st), twin.step(t, *st)
            hs, rad, wv = gpu.components()
            hs_t, rad_t, _ = twin.components()
            wf = fresh.compute_waves(t)
            if kind in ("spectral", "none"):
                assert np.array_equal(wv, wf), f"{kind}, step {k + j}: wave rows differ from a fresh context's"
            else:  # the IRF convolution of a block step comes from the pass (another summation order than the plain evaluation of
                #    hc_compute_waves), the regular term of the hot step kernel from other code: held to the suite's tolerance here
                assert relerr(wv, wf) <= TIGHT_TOL, f"{kind}, step {k + j}: {relerr(wv, wf):.3e}"
            assert relerr(hs, hs_t) <= TIGHT_TOL and relerr(rad, rad_t) <= TIGHT_TOL, f"{kind}, step {k + j}"
            assert relerr(fg, ft + wv) <= TIGHT_TOL
            if kind == "spectral":
                worst = max(worst, check_rows(f"spectral model, step {k + j}", wv, F[j], B[j]))
            if kind == "none":
                assert np.all(wv == 0.0)
        fresh.close()
        k += n
    p = gpu.profile()
    assert p["block_kernel_launches"] >= 6 and p["scatter_kernel_launches"] > 0, p
    print(f"models: worst |gpu - ref| / B = {worst:.3f}")
    gpu.close()
    twin.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--wide":
        _wide_run(sys.argv[2])
