"""Nonlinear buoyancy and Froude-Krylov forces on surface panels on the GPU (hc_set_surface_panels, hc_nonlinear_begin /
hc_nonlinear_end, hc_compute_nonlinear; csrc/hc_nonlinear.hip) against the tests' NumPy restatement of the definition
(tests/nonlinear_ref.py), fed the context's own spectrum / regular-wave coefficients.

Tolerance: the bounds nonlinear_ref returns per body and component -- the 1e-11 sum|term| of tests/test_gpu_wave_kinematics.py for
the dynamic-pressure sum, propagated through rho |n| and |d|, plus (n_b + 64) 2^-52 sum_e |contribution_e| for the fixed-shape sum
and the frame algebra (the derivation is in nonlinear_ref's docstring).  The wet test is a discontinuity: every comparison first
asserts, on the reference side, that no panel centroid is closer than 1e-9 m to the free surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import morison_ref as mr
import nonlinear_ref as nr
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81
DEPTH = 60.0  # finite depth of the synthetic cases: with 0.01 .. 2 Hz long-wave, finite-depth and k d > 500 components are all present
MIN_GAP = 1e-9
REG_AMP, REG_OMEGA = 0.177, 2.094395102
COUNTS = (1, 255, 256, 257, 513)  # panels per body: one chunk partly filled, full, and across the chunk boundary


def irreg(nf, seed=4):
    return dict(simulation_dt=0.05, simulation_duration=100.0, ramp_duration=20.0, wave_height=3.0, wave_period=8.0, frequency_min=0.01,
                frequency_max=2.0, nfrequencies=nf, peak_enhancement_factor=2.0, seed=seed)


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def synth_case(N, depth=DEPTH):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7, water_depth=depth)


def random_panels(n, seed, spread=6.0):
    """n panels over +-spread metres about the body reference, area vectors of any direction"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, size=(n, 3)), rng.normal(size=(n, 3)) * 0.3


def state(N, t, seed=3, rest_z=-1.0):
    """pos, rpy for every body (angles up to 0.25 rad), and zero velocities for the calls that take them"""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((N, 3))
    rest[:, 0] = 15.0 * np.arange(N)
    rest[:, 2] = rest_z
    return PrescribedMotion(N, rest, seed=seed, amplitude=0.5).state(t)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def set_all(h, panels):
    for b, pl in enumerate(panels):
        if pl is not None:
            h.set_surface_panels(b, *pl)


def compare(h, case, panels, comp, t, pos, rpy, what, mwl=0.0, stretching=False, ramp=1.0):
    """GPU against the restatement, inside the derived bounds, component by component; asserts the surface margin first."""
    ref = nr.nonlinear(comp, case["water_depth"], case["rho"], G, panels, t, pos, rpy, mwl=mwl, stretching=stretching, ramp=ramp)
    assert ref["margin"] >= MIN_GAP, f"{what}: a panel is {ref['margin']:.3e} m from the free surface (choose other inputs)"
    buoy, fk, hs = (x.reshape(-1, 6) for x in h.compute_nonlinear(t, pos, rpy))
    for name, got, want, bound in (("buoy", buoy, ref["buoy"], ref["bound_buoy"]), ("fk", fk, ref["fk"], ref["bound_fk"])):
        assert got.shape == want.shape and np.all(np.isfinite(got)), (what, name)
        err = np.abs(got - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{what} {name}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(want)):.3e}")
        assert np.all(err <= bound), f"{what} {name}: worst {worst:.3e} of the bound"
    return buoy, fk, hs, ref


def raw_step(h, t, st):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in st]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def three_lists(n0, n2, seed):
    """body 1 carries no panel, between two that do"""
    return [random_panels(n0, seed), None, random_panels(n2, seed + 1)]


# ------------------------------------------------------------------------------------------------
# 1: the formula against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,depth", [(1, DEPTH), (3, np.inf)])
def test_regular_wave(HF, N, depth):
    case = synth_case(N, depth)
    h = HF.from_case(case)
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    comp = wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.7)
    for n in COUNTS:
        panels = [random_panels(n, 10 + n)] if N == 1 else three_lists(n, COUNTS[(COUNTS.index(n) + 2) % 5], 20 + n)
        set_all(h, panels)
        for mwl, stretching in ((0.35, True), (-0.2, False)):  # a regular wave has no stretching: the option changes nothing
            h.set_nonlinear_options(mwl=mwl, regular_phase=0.7, wave_stretching=stretching)
            t = 3.7
            pos, rpy = state(N, t)[:2]
            buoy, fk, _, ref = compare(h, case, panels, comp, t, pos, rpy, f"regular N={N} n={n} mwl={mwl}", mwl=mwl)
            if n > 1:
                assert 0 < ref["wet"][0].sum() < n and np.abs(fk[0]).max() > 1.0
            if N == 3:
                assert not buoy[1].any() and not fk[1].any()


@pytest.mark.parametrize("N,depth,nf,spectral", [(3, DEPTH, 5, False), (1, DEPTH, 256, False), (3, DEPTH, 257, True), (3, np.inf, 600, True),
                                                 (1, DEPTH, 600, False)])
def test_irregular_and_spectral(HF, N, depth, nf, spectral):
    case = synth_case(N, depth)
    h = HF.from_case(case)
    h.add_waves_irregular(spectral=spectral, **irreg(nf))
    comp = wk.irregular_components(h.irreg_spectrum())
    assert comp[0].size == nf
    if np.isfinite(depth):
        n_long, n_finite, n_kd = wk.regimes(comp, depth)
        assert n_finite > 0 and n_long + n_kd > 0  # both profile branches
    results = {}
    for n in COUNTS if N == 1 else (257, 513):
        panels = [random_panels(n, 30 + n)] if N == 1 else three_lists(n, 770 - n, 40 + n)
        set_all(h, panels)
        for mwl, stretching in ((0.35, True), (0.35, False), (0.0, True)):
            h.set_nonlinear_options(mwl=mwl, wave_stretching=stretching)
            for t in (7.5, 33.3):  # inside the ramp of 20 s, after it
                pos, rpy = state(N, t)[:2]
                buoy, fk, _, ref = compare(h, case, panels, comp, t, pos, rpy, f"nf={nf} spectral={spectral} N={N} n={n} mwl={mwl} stretching={stretching} t={t}",
                                           mwl=mwl, stretching=stretching, ramp=mr.ramp_factor(t, 20.0))
                results[(n, mwl, stretching, t)] = fk
                if n > 1:
                    assert 0 < ref["wet"][0].sum() < n
    n = 513
    assert not np.array_equal(results[(n, 0.35, True, 33.3)], results[(n, 0.35, False, 33.3)])
    assert not np.array_equal(results[(n, 0.35, True, 33.3)], results[(n, 0.0, True, 33.3)])


def test_still_water_models(HF):
    """NoWave, no model, an imported eta record: eta = p_d = 0, pure nonlinear buoyancy."""
    case = three_body_case()
    h = HF.from_case(case)
    panels = three_lists(257, 255, 50)
    set_all(h, panels)
    h.set_nonlinear_options(mwl=0.3)
    rec_t = 0.05 * np.arange(400)
    first = None
    for model in ("none", "nowave", "eta_record", "none_after_irregular"):
        if model == "nowave":
            h.add_waves_none()
        elif model == "eta_record":
            h.add_waves_irregular_eta(rec_t, 0.5 * np.sin(0.8 * rec_t), 0.05)
        elif model == "none_after_irregular":
            h.add_waves_irregular(**irreg(64))
            assert h.compute_nonlinear(30.0, *state(3, 3.0)[:2])[1].any()
            h.add_waves_none()
        pos, rpy = state(3, 3.0)[:2]
        buoy, fk, _, _ = compare(h, case, panels, None, 3.0, pos, rpy, f"still water ({model})", mwl=0.3)
        assert not fk.any() and buoy[0].any() and buoy[2].any() and not buoy[1].any()
        first = buoy if first is None else first
        assert same_bits(buoy, first)


# ------------------------------------------------------------------------------------------------
# 2: the wet test against hc_wave_kinematics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretching", [True, False])
def test_wet_test_is_the_kinematics_eta(HF, stretching):
    """Single-panel bodies with c = 0 and rpy = 0 (p = pos exactly) placed at eta + mwl, one ulp-scale step above and below it: wet iff
    p.z - mwl <= eta with the eta hc_wave_kinematics returns for that point, time and options."""
    N, mwl, t = 3, 0.35, 33.3
    case = synth_case(N)
    h = HF.from_case(case)
    h.add_waves_irregular(**irreg(257))
    h.set_nonlinear_options(mwl=mwl, wave_stretching=stretching)
    for b in range(N):
        h.set_surface_panels(b, [[0.0, 0.0, 0.0]], [[0.0, 0.0, -1.0]])
    x = np.array([3.0, 18.5, 41.25])
    rpy = np.zeros((N, 3))
    seen = set()
    for shift in (0.0, 1e-12, -1e-12, 3e-16, -3e-16, 1e-3, -1e-3):
        pos = np.column_stack([x, np.zeros(N), np.zeros(N)])
        # eta does not depend on z: ask once, place the bodies, ask again at the final points
        eta0 = h.wave_kinematics(pos, [t], mwl=mwl, wave_stretching=stretching)[0][0]
        pos[:, 2] = eta0 + mwl + shift
        eta = h.wave_kinematics(pos, [t], mwl=mwl, wave_stretching=stretching)[0][0]
        assert same_bits(eta, eta0) and np.abs(eta).max() > 1e-3
        want = pos[:, 2] - mwl <= eta
        buoy = h.compute_nonlinear(t, pos, rpy)[0].reshape(N, 6)
        # a wet panel at depth z' = p.z - mwl gives -p_s n_z = -rho g z'; exactly on the surface that can be 0: classify by fk too
        fk = h.compute_nonlinear(t, pos, rpy)[1].reshape(N, 6)
        got = (buoy[:, 2] != 0.0) | (fk[:, 2] != 0.0)
        assert np.array_equal(got[want == False], np.zeros((want == False).sum(), dtype=bool)), (shift, want, buoy[:, 2], fk[:, 2])  # noqa: E712
        assert got[want].all(), (shift, want, buoy[:, 2], fk[:, 2])
        seen |= set(want.tolist())
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------
# 3: closed forms
# ------------------------------------------------------------------------------------------------
def test_closed_forms_cube_and_box(HF):
    case = three_body_case()
    h = HF.from_case(case)
    rho = case["rho"]
    cube = nr.triangles_to_panels(nr.box_triangles([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], m=3))
    draft, a, b = 3.0, 4.0, 3.0
    box = nr.triangles_to_panels(nr.box_triangles([-a / 2, -b / 2, -draft], [a / 2, b / 2, 2.0], m=4, mz=5))
    h.set_surface_mesh(0, nr.box_triangles([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], m=3))
    h.set_surface_panels(2, *box)
    assert h.surface_panel_count(0) == 108 and h.surface_panel_count(1) == 0 and h.surface_panel_count(2) == len(box[0])
    pos = np.array([[3.0, -2.0, -10.0], [0.0, 0.0, 0.0], [7.0, 1.0, 0.0]])
    rpy = np.array([[0.3, -0.4, 1.1], [0.0, 0.0, 0.0], [0.0, 0.0, 0.6]])
    buoy, fk, _, ref = compare(h, case, [cube, None, box], None, 0.0, pos, rpy, "closed forms")
    assert ref["margin"] > 0.3
    assert np.all(np.abs(buoy[0, :3] - [0.0, 0.0, rho * G * 8.0]) <= ref["bound_buoy"][0, :3])  # (a) Archimedes at any attitude
    assert abs(buoy[2, 2] - rho * G * a * b * draft) <= ref["bound_buoy"][2, 2]  # (b) rho g A_wp draft
    assert np.all(np.abs(buoy[2, :2]) <= ref["bound_buoy"][2, :2])


# ------------------------------------------------------------------------------------------------
# 4: invariance, bitwise
# ------------------------------------------------------------------------------------------------
def subject_cases():
    """A 1-body case and 3-body cases that carry the SAME hydrostatic data at index j (everything hs_lin reads)."""
    one = synth_case(1)
    subject = {k: one["bodies"][0][k] for k in ("disp_vol", "cg", "cb", "lin")}
    threes = []
    for j in range(3):
        c3 = synth_case(3)
        c3["bodies"][j].update(subject)
        threes.append(c3)
    return one, threes


def test_bits_do_not_depend_on_neighbours_index_shard_or_repeats(HF):
    one_case, three_cases = subject_cases()
    pl = random_panels(257, 60)
    t = 33.3
    p1, r1 = state(1, t, seed=5)[:2]

    def prepare(h):
        h.add_waves_irregular(**irreg(300))
        h.set_nonlinear_options(mwl=0.2)

    one = HF.from_case(one_case)
    prepare(one)
    one.set_surface_panels(0, *pl)
    ref = np.concatenate(one.compute_nonlinear(t, p1, r1))
    assert ref[:6].any() and ref[6:12].any() and ref[12:].any()
    for _ in range(3):
        assert same_bits(np.concatenate(one.compute_nonlinear(t, p1, r1)), ref)  # a repeated call

    def rows(res, j):
        return np.concatenate([x[6 * j:6 * j + 6] for x in res])

    for j in range(3):
        three = HF.from_case(three_cases[j])
        prepare(three)
        three.set_surface_panels(j, *pl)
        pos, rpy = state(3, t, seed=9)[:2]
        pos, rpy = pos.reshape(3, 3).copy(), rpy.reshape(3, 3).copy()
        pos[j], rpy[j] = p1.reshape(3), r1.reshape(3)
        for others in (None, 513, 70, 0):  # other bodies' lists: none yet, 513 panels (two full chunks before body j's), 70, cleared
            if others is not None:
                for k in range(3):
                    if k != j:
                        three.set_surface_panels(k, *random_panels(others, 61 + k + others))
            assert same_bits(rows(three.compute_nonlinear(t, pos, rpy), j), ref), (j, others)
        # the shard context that owns body j alone, the lists of all bodies set
        sh = HF.from_case(three_cases[j], body_range=(j, j + 1))
        prepare(sh)
        for k in range(3):
            sh.set_surface_panels(k, *(pl if k == j else random_panels(513, 90 + k)))
        assert same_bits(np.concatenate(sh.compute_nonlinear(t, pos, rpy)), ref), j
        sh.close()
        three.close()


# ------------------------------------------------------------------------------------------------
# 5: beside the steps
# ------------------------------------------------------------------------------------------------
def test_nonlinear_around_every_step_changes_no_force(HF):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    from cases import SPHERE_DT
    case = sphere_case()
    sphere_irreg = dict(simulation_dt=SPHERE_DT, simulation_duration=600.0, ramp_duration=60.0, wave_height=2.0, wave_period=12.0,
                        frequency_min=0.001, frequency_max=1.0, nfrequencies=1000)
    runs = []
    for with_nl in (False, True):
        h = HF.from_case(case)  # default look-ahead and schedule
        h.add_waves_irregular(**sphere_irreg)
        if with_nl:
            h.set_surface_panels(0, *random_panels(513, 2))
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        rows = []
        for n in range(100):  # three look-ahead blocks of 32 steps
            t = SPHERE_DT * n
            st = motion.state(t)
            if with_nl:
                h.nonlinear_begin(t, st[0], st[1])
            total = raw_step(h, t, st)
            if with_nl:
                assert h.nonlinear_end()[0].any()
            rows.append(np.concatenate([total, *h.components()]))
        runs.append(np.array(rows))
        h.close()
    assert same_bits(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# 6: composition one layer up, hs_lin
# ------------------------------------------------------------------------------------------------
THREE_IRREG = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
                   frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)


def test_hydroforces_and_hydrogroup_step_compose(HF):
    from hydrochrono_amd.hydro import HydroGroup
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    panels = [random_panels(300, 70), None, random_panels(5, 72)]
    elements = [None, (np.array([[0.0, 0.0, -4.0]]), np.array([[2.0, 0.5, 1.25]]), np.array([[1.0, 2.0, 3.0]])),
                (np.array([[1.0, 0.0, -3.0]]), np.array([[1.0, 1.0, 1.0]]), np.zeros((1, 3)))]
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)
    for mode in (1, 2):
        a, b, plain, with_mor = (HF.from_case(case) for _ in range(4))
        grp = HydroGroup.from_case(case, 2)
        for h in (a, b, plain, with_mor, grp):
            h.add_waves_irregular(**THREE_IRREG)
        for h in (a, b, with_mor, grp):
            for k, pl in enumerate(panels):
                if pl is not None:
                    h.set_surface_panels(k, *pl)
            h.set_nonlinear_options(mwl=0.1)
        for h in (a, with_mor, grp):
            h.set_nonlinear_mode(mode)
        for k, el in enumerate(elements):
            if el is not None:
                with_mor.set_morison_elements(k, *el)
        assert not a.nonlinear()[0].any() and not grp.nonlinear()[0].any()
        for n in range(36):  # across a look-ahead block
            t = 0.01 * n
            st = motion.state(t)
            fa = a.step(t, *st)
            total = raw_step(b, t, st)
            buoy, fk, hs = b.compute_nonlinear(t, st[0], st[1])
            want = total.copy()
            for k in (0, 2):
                r = slice(6 * k, 6 * k + 6)
                want[r] = total[r] - hs[r] + buoy[r]
                if mode == 2:
                    want[r] = want[r] + fk[r]
            assert same_bits(fa, want) and same_bits(fa[6:12], total[6:12])  # only bodies with panels change
            assert all(same_bits(x, y) for x, y in zip(a.nonlinear(), (buoy, fk, hs)))
            assert same_bits(total, plain.step(t, *st))  # no panels (b: mode 0): today's calls, today's bits
            assert same_bits(grp.step(t, *st), want)  # two shards
            assert all(same_bits(x, y) for x, y in zip(grp.compute_nonlinear(t, st[0], st[1]), (buoy, fk, hs)))
            assert same_bits(with_mor.step(t, *st), want + with_mor.morison())  # together with Morison elements
            assert with_mor.morison().any()
        assert buoy.any() and fk.any() and not same_bits(fa, total)
        # panels set but mode 0 (b), and panels cleared again under mode > 0 (a): step() is the plain step
        for k in (0, 2):
            a.set_surface_panels(k, np.zeros((0, 3)), np.zeros((0, 3)))
        st = motion.state(0.5)
        want = plain.step(0.5, *st)
        assert same_bits(b.step(0.5, *st), want)
        assert same_bits(a.step(0.5, *st), want) and not a.nonlinear()[0].any()
        for h in (a, b, plain, with_mor, grp):
            h.close()


def test_hs_lin_is_the_hydrostatic_component_of_a_step(HF):
    """Within 16 * 2^-52 * sum|term| (the device may contract the 6-term dot product into fused multiply-adds, the host does not)."""
    for case in (three_body_case(), synth_case(3)):
        h = HF.from_case(case)
        h.add_waves_none()
        for t in (0.0, 1.7):
            st = state(3, t, seed=6, rest_z=-2.0)
            raw_step(h, t, st)
            hs = h.components()[0]
            hs_lin = h.compute_nonlinear(t, st[0], st[1])[2]
            ref, scale = nr.hs_linear(case["rho"], [0.0, 0.0, -G], case["bodies"], st[0], st[1])
            assert np.abs(hs).max() > 1.0
            err = np.abs(hs_lin - hs) / scale.reshape(-1)
            print(f"hs_lin against the step's hs: worst {err.max() / nr.EPS:.2f} ulp of sum|term|, bitwise equal: {same_bits(hs_lin, hs)}")
            assert np.all(np.abs(hs_lin - hs) <= 16 * nr.EPS * scale.reshape(-1))
            assert np.all(np.abs(hs_lin - ref.reshape(-1)) <= 16 * nr.EPS * scale.reshape(-1))
        h.close()


def test_cpp_mirror_composes_as_the_python_layer(HF, tmp_path):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "nonlinear_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "nonlinear_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (40, 37)
    h = HF(1)
    h.load_bemio_h5(h5)
    h.finalize()
    h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
    mesh = caller_box(2.0, 1.5, -3.0, 4.0)
    h.set_surface_mesh(0, mesh)
    h.set_nonlinear_options(mwl=0.25, regular_phase=0.3)
    comp = wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.3)
    case = sphere_case()
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total = raw_step(h, t, st)
        buoy, fk, hs = row[19:25], row[25:31], row[31:37]
        assert same_bits(row[13:19], total - hs + buoy + fk), t
        assert all(same_bits(x, y) for x, y in zip(h.compute_nonlinear(t, st[0], st[1]), (buoy, fk, hs))), t
    # ... and the last row against the restatement
    ref = nr.nonlinear(comp, case["water_depth"], case["rho"], G, [nr.triangles_to_panels(mesh)], t, st[0], st[1], mwl=0.25)
    assert ref["margin"] >= MIN_GAP
    assert np.all(np.abs(buoy - ref["buoy"][0]) <= ref["bound_buoy"][0]) and np.all(np.abs(fk - ref["fk"][0]) <= ref["bound_fk"][0])
    assert np.abs(rows[:, 19:22]).max() > 1.0 and np.abs(rows[:, 25:28]).max() > 1.0


def caller_box(a, b, z0, z1):
    """the twelve triangles of tests/cpp/nonlinear_caller.cpp, in its order"""
    x, y, z = (-a, a), (-b, b), (z0, z1)
    v = (lambda i, j, k: [x[i], y[j], z[k]])
    quads = [(v(0, 0, 0), v(0, 1, 0), v(1, 1, 0), v(1, 0, 0)), (v(0, 0, 1), v(1, 0, 1), v(1, 1, 1), v(0, 1, 1)),
             (v(0, 0, 0), v(1, 0, 0), v(1, 0, 1), v(0, 0, 1)), (v(0, 1, 0), v(0, 1, 1), v(1, 1, 1), v(1, 1, 0)),
             (v(0, 0, 0), v(0, 0, 1), v(0, 1, 1), v(0, 1, 0)), (v(1, 0, 0), v(1, 1, 0), v(1, 1, 1), v(1, 0, 1))]
    return np.array([t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])], dtype=float)


# ------------------------------------------------------------------------------------------------
# 7: errors
# ------------------------------------------------------------------------------------------------
def test_errors(HF):
    from hydrochrono_amd import capi
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    z9 = np.zeros(9)
    below = np.tile([0.0, 0.0, -5.0], 3)
    o = [np.full(18, 7.0) for _ in range(3)]

    def pan(c=(0, 0, -1.0), s=(0, 0, -2.0), n=1):
        arr = (capi.SurfacePanel * n)()
        for e in arr:
            e.c[:], e.s[:] = c, s
        return arr

    # before hc_finalize: panels may be set, nothing can be computed
    raw = HF(3)
    lib = raw.lib
    assert lib.hc_set_surface_panels(raw.ctx, 0, pan(), 1) == OK
    assert lib.hc_nonlinear_begin(raw.ctx, 0.0, dp(z9), dp(z9)) == INV
    assert lib.hc_nonlinear_end(raw.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == INV  # nothing stayed pending
    raw.close()

    h = HF.from_case(case)
    n = C.c_int(-1)
    # no panels: buoy = fk = 0, hs_lin all the same, and begin / end still pair up
    assert lib.hc_compute_nonlinear(h.ctx, 0.0, dp(below), dp(z9), dp(o[0]), dp(o[1]), dp(o[2])) == OK
    assert not o[0].any() and not o[1].any() and o[2].any()
    # bad index, count, list
    for body in (-1, 3, 100):
        assert lib.hc_set_surface_panels(h.ctx, body, pan(), 1) == INV
        assert lib.hc_get_surface_panel_count(h.ctx, body, C.byref(n)) == INV
    assert lib.hc_get_surface_panel_count(h.ctx, 0, None) == INV
    assert lib.hc_set_surface_panels(h.ctx, 0, pan(), -1) == INV
    assert lib.hc_set_surface_panels(h.ctx, 0, None, 2) == INV
    assert lib.hc_set_surface_panels(h.ctx, 0, pan(), (1 << 20) + 1) == INV  # the cap (checked before the list is read)
    assert lib.hc_set_surface_panels(h.ctx, 0, pan(n=2048), 2048) == OK
    for bad in (np.nan, np.inf, -np.inf):
        assert lib.hc_set_surface_panels(h.ctx, 0, pan(c=(0, bad, 0)), 1) == INV
        assert lib.hc_set_surface_panels(h.ctx, 0, pan(s=(bad, 0, 0)), 1) == INV
    assert lib.hc_get_surface_panel_count(h.ctx, 0, C.byref(n)) == OK and n.value == 2048  # a refused list leaves the one before
    assert b"surface panel" in lib.hc_last_error(h.ctx)
    assert lib.hc_set_surface_panels(h.ctx, 0, pan(), 1) == OK
    # options
    for opt in (capi.WaveKinematicsOpts(np.nan, 0.0, 1), capi.WaveKinematicsOpts(0.0, np.inf, 1)):
        assert lib.hc_set_nonlinear_options(h.ctx, C.byref(opt)) == INV
    assert lib.hc_set_nonlinear_options(h.ctx, None) == OK
    # end without begin, begin twice, exactly one end per begin
    assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == INV
    assert lib.hc_nonlinear_begin(h.ctx, 0.0, dp(below), dp(z9)) == OK
    assert lib.hc_nonlinear_begin(h.ctx, 0.0, dp(below), dp(z9)) == INV
    assert lib.hc_set_surface_panels(h.ctx, 1, pan(), 1) == INV  # not while one is in flight
    assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), None, None) == OK  # any output pointer may be NULL
    # one panel at z = -6 with s = (0, 0, -2): -p_s n_z = rho g z n_z
    assert o[0][2] == -(-(case["rho"] * G) * -6.0) * -2.0 and not o[0][6:].any()
    assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == INV
    assert lib.hc_nonlinear_begin(h.ctx, 0.0, dp(below), dp(z9)) == OK
    assert lib.hc_nonlinear_end(h.ctx, None, None, None) == OK
    # non-finite state or time: refused, nothing pending afterwards
    for k in range(2):
        for bad in (np.nan, np.inf):
            st = [below.copy(), z9.copy()]
            st[k][4] = bad
            assert lib.hc_nonlinear_begin(h.ctx, 0.0, dp(st[0]), dp(st[1])) == INV
            assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == INV
    for bad in (np.nan, np.inf, -np.inf):
        assert lib.hc_compute_nonlinear(h.ctx, bad, dp(below), dp(z9), dp(o[0]), dp(o[1]), dp(o[2])) == INV
    assert lib.hc_nonlinear_begin(h.ctx, 0.0, None, dp(z9)) == INV
    # gravity that is not (0, 0, -g)
    for g3 in ([0.0, 0.0, 9.81], [0.1, 0.0, -9.81], [0.0, -2.0, -9.81], [0.0, 0.0, 0.0]):
        h.set_gravity(g3)
        assert lib.hc_nonlinear_begin(h.ctx, 0.0, dp(below), dp(z9)) == INV
        assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), dp(o[1]), dp(o[2])) == INV
    h.set_gravity([0.0, 0.0, -9.81])
    assert lib.hc_compute_nonlinear(h.ctx, 0.0, dp(below), dp(z9), dp(o[0]), dp(o[1]), dp(o[2])) == OK and o[0][2] > 0
    # a shard context takes the lists of all bodies and computes its own
    sh = HF.from_case(case, body_range=(1, 2))
    for b in range(3):
        assert lib.hc_set_surface_panels(sh.ctx, b, pan(c=(0, 0, -1.0 - b)), 1) == OK
    o6 = [np.empty(6) for _ in range(3)]
    assert lib.hc_compute_nonlinear(sh.ctx, 0.0, dp(below), dp(z9), dp(o6[0]), dp(o6[1]), dp(o6[2])) == OK
    assert o6[0][2] == -(-(case["rho"] * G) * -7.0) * -2.0
    with pytest.raises(Exception):
        h.set_surface_panels(0, [[0, 0, np.nan]], [[0, 0, 1]])
    with pytest.raises(ValueError):
        h.set_nonlinear_mode(3)
