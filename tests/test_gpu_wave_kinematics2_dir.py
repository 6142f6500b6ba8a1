"""Second-order irregular waves in a short-crested sea on the GPU (hc_wave_kinematics2_dir, hc_wave_kinematics2_dir_pair_tables)
against the longdouble restatement tests/wave2_dir_ref.py, fed the context's own spectrum and directions, on the input sets of
tests/wave2_dir_inputs.py (tests/test_wave2_dir_ref_cpu.py shows that plain FP64 reaches the tolerance on each of them).

Tolerances, those of tests/test_gpu_wave_kinematics2.py: a table entry |gpu - ref| <= TOL (|ref| + sum|addends| of the entry), a
field element |gpu - ref| <= TOL sum|term| with each term's magnitude taken over its phase; TOL = 1e-11."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wave2_dir_inputs as di
import wave2_dir_ref as wd
import wave2_inputs as wi
import wave2_ref as w2
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = di.TOL
INF = float("inf")


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def spread_sea(h, case, waves):
    """The spectral model with excitation tables on a heading grid for every body (its own table at both ends of [-4, 4]): what
    non-uniform directions need.  h: HydroForces or HydroGroup."""
    for b, bd in enumerate(case["bodies"]):
        mag, ph = (np.stack([np.asarray(bd[k]).reshape(6, -1)] * 2, axis=1) for k in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-4.0, 4.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, **waves)


_contexts = {}


def context(HF, name):
    """One context per input set, shared by the tests of the module, with the set's directions in force."""
    if name not in _contexts:
        case = di.case_of(name)
        h = HF.from_case(case)
        spread_sea(h, case, di.SETS[name][1])
        _contexts[name] = h
    h = _contexts[name]
    h.set_wave_directions(di.directions(name))
    return h


def comp_of(h):
    return wk.irregular_components(h.irreg_spectrum())


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def assert_fields(got, ref, what, tol=TOL):
    values, scales = ref
    for g, r, s, name in zip(got, values[:3], scales[:3], ("eta2", "vel2", "acc2")):
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        assert np.all(np.isfinite(g)), (what, name)
        err = np.abs(g - r)
        worst = float(np.max(err / np.maximum(s, 1e-300))) if g.size else 0.0
        print(f"{what} {name}: worst {worst:.3e} of sum|term|")
        assert np.all(err <= tol * s), f"{what} {name}: {int((err > tol * s).sum())} elements, worst {worst:.3e} of sum|term|"


# ------------------------------------------------------------------------------------------------
# 1: the pair tables
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(di.SETS))
def test_pair_tables_match_the_reference(HF, name):
    h = context(HF, name)
    comp = comp_of(h)
    _, g, depth = h.simulation_parameters()
    assert np.array_equal(h.wave_directions(), di.directions(name))
    for bands in ("full", "cut", "empty"):
        diff_band, sum_band = di.BANDS[bands]
        got = h.wave_pair_tables(diff_band=diff_band, sum_band=sum_band, directional=True)
        ref, mag = di.reference_tables(name, bands, di.key(comp), g, depth)
        in_diff, in_sum = w2.band_masks(comp[1], diff_band, sum_band)
        for n in ("Kp", "Km", "Bp", "Bm"):
            assert got[n].shape == ref[n].shape and np.all(np.isfinite(got[n])), (bands, n)
            err, bound = np.abs(got[n] - ref[n]), TOL * (np.abs(ref[n]) + mag[n])
            print(f"{name} {bands} {n}: worst {float(np.max(err / np.maximum(bound / TOL, 1e-300))):.3e}")
            assert np.all(err <= bound), (bands, n)
            assert not got[n][~(in_sum if n.endswith("p") else in_diff)].any(), (bands, n)  # zeros outside the band
        if bands == "full":
            assert np.array_equal(np.diag(got["Bm"]), np.zeros(comp[0].size))
            if np.isinf(depth):  # the sum-frequency potential of crossing components: zero for a long-crested sea
                off = ~np.eye(comp[0].size, dtype=bool)
                assert np.count_nonzero(got["Bp"][off]) > 0.4 * off.sum() and np.abs(ref["Bp"][off]).max() > 0


# ------------------------------------------------------------------------------------------------
# 2: the fields, under every choice of bands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", list(di.BANDS))
@pytest.mark.parametrize("name", list(di.SETS))
def test_fields_match_the_reference(HF, name, bands):
    h = context(HF, name)
    comp = comp_of(h)
    _, g, depth = h.simulation_parameters()
    _, _, pts, times, _ = di.SETS[name]
    diff_band, sum_band = di.BANDS[bands]
    got = h.wave_kinematics2(pts, times, mwl=di.MWL, diff_band=diff_band, sum_band=sum_band, directional=True)
    assert_fields(got, di.reference(name, bands, di.key(comp), g, depth), f"{name} {bands}")
    if bands == "empty":
        assert not any(a.any() for a in got)
    else:
        assert got[0].any() and got[1][..., 1].any() and got[2][..., 1].any()  # the y components are there
    # points above the mean level are held at its value: z runs fastest in the grid, above the level first, then at it
    z = pts[:, 2]
    assert np.all(z[0::10] > di.MWL) and np.all(z[1::10] == di.MWL)
    assert same_bits(tuple(a[:, 0::10] for a in got), tuple(a[:, 1::10] for a in got))


# ------------------------------------------------------------------------------------------------
# 3: a uniform heading is a rotation of the long-crested sea; no directions: the long-crested sea itself
# ------------------------------------------------------------------------------------------------
def test_uniform_heading_on_the_irf_model_and_no_directions(HF):
    h = HF.from_case(sphere_case())
    h.add_waves_irregular(**wi.sphere_waves(65))  # the IRF model
    comp = comp_of(h)
    _, g, depth = h.simulation_parameters()
    pts = di.grid(wi.XS[1:3], di.YS, wi.SPHERE_Z[1:6])
    times = wi.TIMES[1:]
    beta = 0.7
    h.set_wave_directions(np.full(65, beta))
    got = h.wave_kinematics2(pts, times, mwl=di.MWL, directional=True)
    _, scales = wd.fields(comp, np.full(65, beta), g, depth, pts, times, mwl=di.MWL, ramp_duration=20.0)
    h.set_wave_directions(None)
    c, s = np.cos(beta), np.sin(beta)
    turned = np.stack([pts[:, 0] * c + pts[:, 1] * s, -pts[:, 0] * s + pts[:, 1] * c, pts[:, 2]], axis=1)
    eta, vel, acc = h.wave_kinematics2(turned, times, mwl=di.MWL)
    back = lambda v: np.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c, v[..., 2]], axis=-1)
    assert_fields(got, ((eta, back(vel), back(acc)), scales), "uniform heading", tol=2 * TOL)
    assert got[1][..., 1].any() and np.abs(got[0]).max() > 1e-4
    # no directions: the directional kernels on the long-crested sea along +x
    lc = h.wave_kinematics2(pts, times, mwl=di.MWL)
    dr = h.wave_kinematics2(pts, times, mwl=di.MWL, directional=True)
    _, scales0 = w2.fields(comp, g, depth, pts, times, mwl=di.MWL, ramp_duration=20.0)
    assert_fields(dr, (lc, scales0), "no directions", tol=2 * TOL)
    assert not dr[1][..., 1].any() and not dr[2][..., 1].any()
    ta, tb = h.wave_pair_tables(directional=True), h.wave_pair_tables()
    _, mag = w2.pair_tables(comp, g, depth)
    for n in ta:
        assert np.all(np.abs(ta[n] - tb[n]) <= 2 * TOL * (np.abs(tb[n]) + mag[n])), n
    h.close()


# ------------------------------------------------------------------------------------------------
# 4: batch invariance, shards, eta2 alone
# ------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch_the_outputs_or_the_shard(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroGroup
    name = "three65_oppose"
    h = context(HF, name)
    pts, times = di.grid(wi.XS, di.YS[:1], wi.THREE_Z), wi.TIMES
    assert pts.shape[0] == 70
    diff_band, sum_band = di.BANDS["cut"]
    for kw in (dict(mwl=di.MWL), dict(mwl=di.MWL, diff_band=diff_band, sum_band=sum_band)):
        big = h.wave_kinematics2(pts, times, directional=True, **kw)
        for i, j in ((0, 0), (69, 2), (33, 1), (7, 2)):
            one = h.wave_kinematics2(pts[i:i + 1], times[j:j + 1], directional=True, **kw)
            assert same_bits(one, tuple(a[j:j + 1, i:i + 1] for a in big)), (i, j)
        # eta2 alone, and every other choice of outputs
        xyz, n = np.ascontiguousarray(pts.reshape(-1)), pts.shape[0] * times.size
        o = h._wave2_opts(kw["mwl"], 0.0, kw.get("diff_band", w2.FULL), kw.get("sum_band", w2.FULL), True)
        dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
        for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (0, 0, 0)):
            outs = [np.full(k * n, 7.0) if m else None for m, k in zip(mask, (1, 3, 3))]
            assert h.lib.hc_wave_kinematics2_dir(h.ctx, C.byref(o), 70, dp(xyz), 3, dp(times), *[dp(a) for a in outs]) == capi.HC_OK
            for a, f in zip(outs, big):
                if a is not None:
                    assert np.array_equal(a.view(np.uint64), f.reshape(-1).view(np.uint64)), mask
    case = di.case_of(name)
    group = HydroGroup.from_case(case, 3)
    spread_sea(group, case, di.SETS[name][1])
    group.set_wave_directions(di.directions(name))
    ref = h.wave_kinematics2(pts, times, mwl=di.MWL, directional=True)
    for sh in group.shards:
        assert same_bits(sh.wave_kinematics2(pts, times, mwl=di.MWL, directional=True), ref), (sh.b0, sh.b1)
    assert same_bits(group.wave_kinematics2(pts, times, mwl=di.MWL, directional=True), ref)
    group.close()


# ------------------------------------------------------------------------------------------------
# 5: a regular wave with a heading is Stokes' second-order wave with its set-down along the heading
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,amp,omega", [("sphere", 0.5, 0.5), ("deep", 0.4, 1.1)])
def test_regular_wave_is_stokes_second_order_along_its_heading(HF, which, amp, omega):
    case = sphere_case() if which == "sphere" else dict(sphere_case(), water_depth=INF)
    h = HF.from_case(case)
    h.add_waves_regular(amp, omega)
    beta = 0.7
    h.set_wave_directions([beta])
    k = h.regular_coeffs()[2]
    _, g, depth = h.simulation_parameters()
    comp = wk.regular_components(amp, omega, k, 0.7)
    pts = di.grid(wi.XS[:3], di.YS, np.array([0.5, 0.0, -2.0, -30.0]))
    times = np.array([0.0, 3.7, 41.3])
    got = h.wave_kinematics2(pts, times, regular_phase=0.7, directional=True)
    assert_fields(got, wd.fields(comp, [beta], g, depth, pts, times), f"regular {which} {omega}")
    c, s = np.cos(beta), np.sin(beta)
    theta = k * (pts[None, :, 0] * c + pts[None, :, 1] * s) - omega * times[:, None] + 0.7
    # (the bound of tests/test_gpu_wave_kinematics2.py: the reference's k is on the dispersion curve to 1e-6 1/m)
    assert k * depth >= 5.0
    assert np.all(np.abs(got[0] - w2.stokes_eta2(amp, k, depth, theta)) <= 1e-5 * amp * amp)
    assert np.abs(got[0]).max() > 0.1 * k * amp * amp
    assert same_bits(h.wave_kinematics2(pts, times, regular_phase=0.7, apply_ramp=False, directional=True), got)  # not ramped
    tabs = h.wave_pair_tables(directional=True)
    assert all(v.shape == (1, 1) for v in tabs.values()) and tabs["Bm"][0, 0] == 0.0
    if np.isinf(depth):
        assert not got[1].any() and not got[2].any()  # one component crosses nothing: no second-order potential in deep water
    else:  # the horizontal velocity points along the heading
        assert np.abs(got[1][..., 0]).max() > 0
        assert np.all(np.abs(got[1][..., 0] * s - got[1][..., 1] * c) <= 1e-14 * np.abs(got[1][..., 0]).max())
    h.close()


# ------------------------------------------------------------------------------------------------
# 6: the ramp; no components, empty batches, bad arguments, the component limit, a change of the directions
# ------------------------------------------------------------------------------------------------
def test_ramp_inside_and_outside_on_and_off(HF):
    name = "sphere63_spread"
    h = context(HF, name)
    comp = comp_of(h)
    beta = di.directions(name)
    _, g, depth = h.simulation_parameters()
    pts = di.grid(wi.XS[:2], di.YS, np.array([0.0, -5.0]))
    times = np.array([-1.0, 0.0, 5.0, 19.999, 20.0, 33.0])  # ramp_duration = 20
    on = h.wave_kinematics2(pts, times, directional=True)
    off = h.wave_kinematics2(pts, times, apply_ramp=False, directional=True)
    assert_fields(on, wd.fields(comp, beta, g, depth, pts, times, ramp_duration=20.0), "ramp on")
    assert_fields(off, wd.fields(comp, beta, g, depth, pts, times), "ramp off")
    assert not any(a[:2].any() for a in on) and all(a[:2].any() for a in off)
    assert same_bits(tuple(a[4:] for a in on), tuple(a[4:] for a in off))
    assert np.allclose(on[0][2], off[0][2] / 16, rtol=1e-14, atol=0)  # (5 / 20)^2


def raw_call(h, P, xyz, T, t, eta=None, vel=None, acc=None, **fields):
    from hydrochrono_amd import capi
    o = capi.WaveKinematics2Opts()
    h.lib.hc_wave_kinematics2_opts_default(C.byref(o))
    for k, v in fields.items():
        setattr(o, k, v)
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    return h.lib.hc_wave_kinematics2_dir(h.ctx, C.byref(o), P, dp(xyz), T, dp(t), dp(eta), dp(vel), dp(acc))


def test_no_components_empty_batches_bad_arguments_the_limit_and_new_directions(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    case = sphere_case()
    pts = di.grid(wi.XS[:2], di.YS, np.array([-10.0, 0.0]))
    times = np.array([25.0, 32.0, 49.0])
    raw = HF(1)  # not finalized
    assert raw_call(raw, 1, np.zeros(3), 1, np.zeros(1), eta=np.empty(1)) == capi.HC_ERR_INVALID
    raw.close()
    h = HF.from_case(case)
    # no model (the NoWave of hc_finalize), NoWave, an imported eta record: zeros, and no tables
    rec_t = np.arange(0.0, 30.0, 0.25)
    for step in range(3):
        e, v, a = h.wave_kinematics2(pts, times, directional=True)
        assert not e.any() and not v.any() and not a.any() and e.shape == (3, 8) and v.shape == (3, 8, 3)
        assert h.wave_pair_tables(directional=True)["Kp"].size == 0
        if step == 0:
            h.add_waves_none()
        elif step == 1:
            h.add_waves_irregular_eta(rec_t, 0.3 * np.sin(0.8 * rec_t), SPHERE_DT)
    spread_sea(h, case, wi.sphere_waves(65))
    h.set_wave_directions(di.spread(65))
    xyz = np.ascontiguousarray(pts.reshape(-1))
    full = h.wave_kinematics2(pts, times, mwl=0.2, directional=True)
    assert np.abs(full[0]).max() > 1e-4 and full[1][..., 1].any()
    # empty batches
    for P, T in ((0, 3), (8, 0), (0, 0)):
        e, v, a = h.wave_kinematics2(pts[:P], times[:T], directional=True)
        assert e.shape == (T, P) and v.shape == (T, P, 3)
    assert raw_call(h, 0, None, 3, times, np.empty(1)) == capi.HC_OK
    assert raw_call(h, 8, xyz, 0, None, np.empty(1)) == capi.HC_OK
    # bad arguments: y has to be finite as well
    one = np.empty(24)
    assert raw_call(h, 8, xyz, 3, times, one) == capi.HC_OK
    assert raw_call(h, -1, xyz, 3, times, one) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, None, 3, times, one) == capi.HC_ERR_INVALID
    assert raw_call(h, 8, xyz, 3, None, one) == capi.HC_ERR_INVALID
    for col, bad in ((0, np.nan), (1, np.nan), (1, np.inf), (2, np.inf)):
        b = xyz.copy()
        b[3 + col] = bad
        assert raw_call(h, 8, b, 3, times, one) == capi.HC_ERR_INVALID, (col, bad)
    assert raw_call(h, 8, xyz, 3, np.array([0.0, np.nan, 1.0]), one) == capi.HC_ERR_INVALID
    for bad in (dict(mwl=np.nan), dict(diff_lo=-0.1), dict(sum_hi=-1.0), dict(diff_lo=0.5, diff_hi=0.4)):
        assert raw_call(h, 8, xyz, 3, times, one, **bad) == capi.HC_ERR_INVALID, bad
    with pytest.raises(HydroError):
        h.wave_pair_tables(sum_band=(-1.0, 2.0), directional=True)
    # other directions, other cut-offs and back: the cached tables follow
    h.set_wave_directions(di.oppose(65))
    other = h.wave_kinematics2(pts, times, mwl=0.2, directional=True)
    comp = comp_of(h)
    _, g, depth = h.simulation_parameters()
    assert not np.array_equal(other[0], full[0])
    assert_fields(other, wd.fields(comp, di.oppose(65), g, depth, pts, times, mwl=0.2, ramp_duration=20.0), "new directions")
    cut = h.wave_kinematics2(pts, times, mwl=0.2, diff_band=(0.0, 0.3), sum_band=wi.NO_PAIR, directional=True)
    assert not np.array_equal(cut[0], other[0])
    h.set_wave_directions(di.spread(65))
    assert same_bits(h.wave_kinematics2(pts, times, mwl=0.2, directional=True), full)
    # more than 4096 components
    h.add_waves_irregular(**wi.sphere_waves(4097))
    assert raw_call(h, 8, xyz, 3, times, one) == capi.HC_ERR_UNSUPPORTED
    assert h.lib.hc_wave_kinematics2_dir_pair_tables(h.ctx, None, None, None, None, None) == capi.HC_ERR_UNSUPPORTED
    h.close()


# ------------------------------------------------------------------------------------------------
# 7: calls between steps change no force
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 32])
def test_calls_between_steps_change_no_force(HF, lookahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_calls in (False, True):
        h = HF.from_case(case)
        h.set_lookahead(lookahead)
        spread_sea(h, case, wi.sphere_waves(65))
        h.set_wave_directions(di.spread(65))
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        pts = di.grid(wi.XS[:3], di.YS[:1], np.array([-5.0, 0.0]))
        forces = []
        for n in range(300):
            t = SPHERE_DT * n
            forces.append(h.step(t, *motion.state(t)))
            if with_calls:
                h.wave_kinematics2(pts, [t], diff_band=(0.0, 0.3 + 0.01 * (n % 3)), directional=True)  # (tables rebuilt now and then)
        runs.append(np.array(forces))
        h.close()
    assert np.abs(runs[0]).max() > 0 and np.array_equal(runs[0].view(np.uint64), runs[1].view(np.uint64))


# ------------------------------------------------------------------------------------------------
# 8: the C++ mirror gives the bits of the Python ABI
# ------------------------------------------------------------------------------------------------
def test_cpp_mirror_matches_the_python_abi(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "wave2_dir_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "wave2_dir_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    for mode in ("regular", "irregular", "long_crested"):
        r = subprocess.run([exe, h5, mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.returncode, r.stderr)
        rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
        assert rows.shape == (12, 11)
        h = HF(1)
        h.load_bemio_h5(h5)
        h.finalize()
        kw = {}
        if mode == "regular":
            h.add_waves_regular(0.5, 0.5, num_bodies=1)
            h.set_wave_directions([0.7])
        else:
            h.add_waves_irregular(**dict(wi.sphere_waves(65), simulation_dt=0.015))
            if mode == "irregular":
                h.set_wave_directions(np.full(65, -0.4))
                kw = dict(diff_band=(0.05, 0.9), sum_band=(1.5, 6.0))
        pts, times = rows[:4, 1:4], rows[::4, 0]
        e, v, a = h.wave_kinematics2(pts, times, mwl=0.3, regular_phase=0.3, directional=True, **kw)
        assert np.array_equal(rows[:, 4], e.reshape(-1)), mode
        assert np.array_equal(rows[:, 5:8], v.reshape(-1, 3)), mode
        assert np.array_equal(rows[:, 8:11], a.reshape(-1, 3)), mode
        assert np.abs(rows[:, 4]).max() > 1e-4
        assert rows[:, 6].any() == (mode != "long_crested")
        h.close()


# ------------------------------------------------------------------------------------------------
# 9: the long-crested call keeps refusing while directions are set
# ------------------------------------------------------------------------------------------------
def test_the_long_crested_call_still_refuses_under_directions(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    h = context(HF, "sphere63_spread")
    pts, times = di.grid(wi.XS[:1], di.YS[:1], np.array([-1.0])), [25.0]
    for call in (lambda: h.wave_kinematics2(pts, times), lambda: h.wave_kinematics2(pts, times, directional=False)):
        with pytest.raises(HydroError) as e:
            call()
        assert e.value.status == capi.HC_ERR_UNSUPPORTED and "direction" in str(e.value)


# ------------------------------------------------------------------------------------------------
# 10: the two calls and the Morison path share one table builder: every cached set follows its own key
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [3, 257])  # 257: one component past a 256-wide tile -- both tile loops and the skipped tile pair run
def test_interleaved_calls_give_the_bits_of_a_fresh_handle(HF, nf):
    """One handle walks through hc_wave_kinematics2, hc_wave_kinematics2_dir and the two pair-table calls in turn, under different
    cut-offs and regular phases, without directions and then with them; a Morison path beside them evaluates while directions are
    set and cleared, so that its tables change layout every time.  Whatever the handle's sets held before, every result has the
    bits of a fresh handle that makes that one call."""
    import morison2_inputs as mi
    case = sphere_case()
    waves = wi.sphere_waves(nf, 0.07, 0.11) if nf == 3 else wi.sphere_waves(nf)
    beta = di.spread(nf)
    elements = mi.random_elements(3, 5, spread=4.0)
    pts = np.array([[-40.0, 0.0, -2.0], [25.0, 7.5, 0.5], [60.0, -11.0, -30.0]])
    times = np.array([7.3, 41.7])  # inside the ramp of 20 s and after it

    def make(directions):
        h = HF.from_case(case)
        spread_sea(h, case, waves)
        if directions:
            h.set_wave_directions(beta)
        h.set_morison_elements(0, *elements)
        h.set_morison_options(mwl=0.1)
        h.set_morison_second_order_directional(True)
        return h

    h = make(False)
    w = comp_of(h)[1]
    assert w.size == nf and np.all(np.diff(w) > 0)
    full = dict(diff_band=w2.FULL, sum_band=w2.FULL)
    cut = dict(diff_band=(0.0, 0.6 * (w[-1] - w[0])), sum_band=(2.0 * w[0], w[0] + w[-1]))  # both cut through the matrix
    diag = dict(diff_band=(0.0, 0.0), sum_band=wi.NO_PAIR)  # the diagonal alone: no row of the first tile reaches the second
    fields = lambda directional, phase, bands: (lambda x: x.wave_kinematics2(pts, times, mwl=0.2, regular_phase=phase,
                                                                            directional=directional, **bands))
    tables = lambda directional, phase, bands: (lambda x: tuple(x.wave_pair_tables(regular_phase=phase, directional=directional,
                                                                                  **bands).values()))

    def morison(bands):
        def call(x):
            x.set_morison_second_order(True, **bands)
            out = [x.compute_morison(t, *mi.moving_state(1, -2.0, t)) for t in times]
            inc = x.morison_increments(0)
            return out + [inc["p"], inc["eta2"], inc["vel2"], inc["acc2"]]
        return call

    fresh = {}
    seen = []

    def check(directions, what, call):
        if (directions, what) not in fresh:
            f = make(directions)
            fresh[directions, what] = call(f)
            f.close()
        got, ref = call(h), fresh[directions, what]
        assert len(got) == len(ref) and same_bits(got, ref), (nf, directions, what, len(seen))
        seen.append(got)

    walk = [("lc full", fields(False, 0.0, full)), ("dir cut", fields(True, 0.4, cut)), ("lc tables cut", tables(False, 0.0, cut)),
            ("morison cut", morison(cut)), ("dir tables diag", tables(True, 0.4, diag)), ("lc full", fields(False, 0.0, full)),
            ("dir diag", fields(True, 0.4, diag)), ("lc diag", fields(False, 0.7, diag)), ("dir cut", fields(True, 0.4, cut)),
            ("lc tables cut", tables(False, 0.0, cut)), ("dir tables full", tables(True, 0.0, full)), ("dir full", fields(True, 0.0, full))]
    for what, call in walk:
        check(False, what, call)
    assert all(a.any() for a in seen[0]) and all(a.any() for a in seen[1]) and seen[3][3].any()
    for rounds in range(2):  # the Morison tables alternate between the two layouts; the directional call's follow the directions
        h.set_wave_directions(beta)
        for what, call in walk:
            if what.startswith(("dir", "morison")):
                check(True, what, call)
        assert seen[-1][1][..., 1].any()  # u2y is there
        h.set_wave_directions(None)
        for what, call in (walk[3], walk[0], walk[1], walk[2]):
            check(False, what, call)
        assert not seen[-4][4][:, 1].any()  # the long-crested increments of the elements again: no u2y
    h.close()
