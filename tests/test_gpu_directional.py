"""Wave heading and short-crested seas on the GPU (hc_set_wave_directions, hc_set_excitation_rao_headings) against
the tests' longdouble restatement (tests/directional_ref.py).  Every tolerance is the bound that file returns: per element
TOL * scale for the kinematics, the compositions' own bounds for the Morison and surface-pressure terms.  Shapes sit at the edges:
nf = 257 is one component past the 256-component LDS tile, nf = 1 the regular wave, the batches a handful of points."""
import os
import subprocess

import numpy as np
import pytest

import directional_ref as dr
import nonlinear_ref
import spectral_ref
import wave_kinematics_ref as wk
from cases import GOLDEN_DIR, SPHERE_DT, sphere_case, three_body_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dr.TOL
IRREG = dict(simulation_dt=SPHERE_DT, simulation_duration=60.0, ramp_duration=10.0, wave_height=2.0, wave_period=9.0,
             frequency_min=0.03, frequency_max=0.9, nfrequencies=257, seed=3)
REG_AMP, REG_OMEGA = 0.177, 2.094395102
POINTS = np.array([[12.0, -7.5, -3.0], [-41.0, 23.0, -0.4], [3.3, 60.0, -25.0]])
TIMES = np.array([1.7, 43.2])


@pytest.fixture(scope="module")
def hydro():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd import capi, hydro
    return hydro, capi


def thetas(nf, seed=4, spread=1.2):
    return np.random.default_rng(seed).uniform(-spread, spread, nf)


def spread_sea(h, case, **kw):
    """The spectral model with excitation tables on a heading grid for every body (its own table at both ends of [-2, 2]): what
    non-uniform directions need.  h: HydroForces or HydroGroup."""
    for b, bd in enumerate(case["bodies"]):
        mag, ph = (np.stack([np.asarray(bd[key]).reshape(6, -1)] * 2, axis=1) for key in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-2.0, 2.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, **dict(IRREG, **kw))


def irregular_comp(h, theta):
    return dr.with_directions(wk.irregular_components(h.irreg_spectrum()), theta)


def assert_matches(got, ref, what):
    values, scales = ref
    for g, r, s, name in zip(got, values, scales, ("eta", "velocity", "acceleration")):
        assert g.shape == r.shape and np.all(np.isfinite(g)), (what, name)
        err = np.abs(g - r)
        print(f"{what} {name}: worst {np.max(err / np.maximum(s, 1e-300)):.3e} of the scale (bound {TOL:.0e})")
        assert np.all(err <= TOL * s), (what, name)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64)) for x, y in zip(a, b))


def status(exc):
    return exc.value.status


# ------------------------------------------------------------------------------------------------
# kinematics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "infinite"])
def test_kinematics_irregular_against_the_reference(hydro, which):
    case = sphere_case() if which == "sphere" else three_body_case()
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case)
    th = thetas(257)
    h.set_wave_directions(th)
    assert np.array_equal(h.wave_directions(), th)
    comp = irregular_comp(h, th)
    for stretching in (True, False):
        got = h.wave_kinematics(POINTS, TIMES, mwl=0.3, wave_stretching=stretching)
        assert_matches(got, dr.kinematics(comp, case["water_depth"], POINTS, TIMES, mwl=0.3, stretching=stretching), f"{which} stretching={stretching}")
        assert np.abs(got[1][..., 1]).max() > 1e-3 and np.abs(got[2][..., 1]).max() > 1e-3
    # eta only: the same bits as with the other outputs
    from hydrochrono_amd.hydro import _dp
    eta = np.empty(TIMES.size * POINTS.shape[0])
    h._chk(h.lib.hc_wave_kinematics(h.ctx, None, POINTS.shape[0], _dp(np.ascontiguousarray(POINTS.reshape(-1))), TIMES.size, _dp(TIMES), _dp(eta), None, None))
    assert np.array_equal(eta, h.wave_kinematics(POINTS, TIMES)[0].reshape(-1))


def test_kinematics_regular_against_the_reference(hydro):
    case = sphere_case()
    h = hydro[0].HydroForces.from_case(case)
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    h.set_wave_directions([0.7])
    comp = dr.with_directions(wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.4), 0.7)
    got = h.wave_kinematics(POINTS, TIMES, mwl=0.2, regular_phase=0.4)
    assert_matches(got, dr.kinematics(comp, case["water_depth"], POINTS, TIMES, mwl=0.2), "regular")
    assert np.abs(got[1][..., 1]).max() > 1e-3


def test_theta_zero_set_then_clear_and_batch_independence(hydro):
    case = sphere_case()
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case)
    before = h.wave_kinematics(POINTS, TIMES, mwl=0.3)
    h.set_wave_directions(np.zeros(257))
    zero = h.wave_kinematics(POINTS, TIMES, mwl=0.3)
    _, scales = dr.kinematics(irregular_comp(h, 0.0), case["water_depth"], POINTS, TIMES, mwl=0.3, stretching=True)
    for a, b, s in zip(zero, before, scales):
        assert np.all(np.abs(a - b) <= 2 * TOL * s)  # either is within TOL * s of the exact sum
    th = thetas(257)
    h.set_wave_directions(th)
    big = h.wave_kinematics(POINTS, TIMES, mwl=0.3)
    assert not np.array_equal(big[0], before[0])
    for p in range(POINTS.shape[0]):
        for j in range(TIMES.size):
            one = h.wave_kinematics(POINTS[p:p + 1], TIMES[j:j + 1], mwl=0.3)
            assert same_bits(one, tuple(a[j:j + 1, p:p + 1] for a in big)), (p, j)
    h.set_wave_directions(None)
    assert h.wave_directions().size == 0
    assert same_bits(h.wave_kinematics(POINTS, TIMES, mwl=0.3), before)
    # y is checked only while directions are set
    bad = POINTS.copy()
    bad[0, 1] = np.nan
    h.wave_kinematics(bad, TIMES)
    h.set_wave_directions(th)
    with pytest.raises(hydro[0].HydroError) as e:
        h.wave_kinematics(bad, TIMES)
    assert status(e) == hydro[1].HC_ERR_INVALID


def test_symmetric_pair_has_no_transverse_flow_on_the_axis(hydro):
    """Two components equal but for +theta and -theta.  A regular wave holds one component, and the sums are linear in the
    components, so the pair's field is the field under [+theta] plus the field under [-theta] of the same regular wave (equal A, w,
    k and phi by construction).  Exact statements, none of which involves the reference's values: v_y of the pair vanishes at y = 0,
    eta of the pair is even in y, and the mirror image of one component is the other -- eta, v_x, v_z at (x, y) under theta equal
    those at (x, -y) under -theta while v_y changes sign.  Each GPU value is within TOL * scale of its exact value (the scales are
    the reference's sums of |term|, equal for +theta and -theta), so a sum or difference of n values is within n * TOL * scale.
    The mirror property is also asserted on the 257-component spread sea."""
    case = sphere_case()
    h = hydro[0].HydroForces.from_case(case)
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    pts = np.array([[5.0, 4.0, -2.0], [5.0, -4.0, -2.0], [5.0, 0.0, -2.0], [-17.0, 0.0, -0.5]])
    mirror = pts * np.array([1.0, -1.0, 1.0])
    theta = 0.6
    comp = dr.with_directions(wk.regular_components(REG_AMP, REG_OMEGA, h.regular_coeffs()[2], 0.4), theta)
    _, (se, sv, sa) = dr.kinematics(comp, case["water_depth"], pts, TIMES)
    h.set_wave_directions([theta])
    P, Pm = h.wave_kinematics(pts, TIMES, regular_phase=0.4), h.wave_kinematics(mirror, TIMES, regular_phase=0.4)
    h.set_wave_directions([-theta])
    M, Mm = h.wave_kinematics(pts, TIMES, regular_phase=0.4), h.wave_kinematics(mirror, TIMES, regular_phase=0.4)
    assert np.abs(P[1][..., 1]).max() > 1e-3
    on_axis = pts[:, 1] == 0.0
    # the pair: v_y and a_y vanish on the axis, eta is even in y
    assert np.all(np.abs(P[1][:, on_axis, 1] + M[1][:, on_axis, 1]) <= 2 * TOL * sv[:, on_axis, 1])
    assert np.all(np.abs(P[2][:, on_axis, 1] + M[2][:, on_axis, 1]) <= 2 * TOL * sa[:, on_axis, 1])
    assert np.all(np.abs((P[0] + M[0]) - (Pm[0] + Mm[0])) <= 4 * TOL * se)
    # the mirror image of one component is the other
    flip = np.array([1.0, -1.0, 1.0])
    assert np.all(np.abs(P[0] - Mm[0]) <= 2 * TOL * se)
    assert np.all(np.abs(P[1] - Mm[1] * flip) <= 2 * TOL * sv) and np.all(np.abs(P[2] - Mm[2] * flip) <= 2 * TOL * sa)
    # ... and so it is for every component of a spread sea
    spread_sea(h, case)
    th = thetas(257)
    _, (se, sv, sa) = dr.kinematics(irregular_comp(h, th), case["water_depth"], pts, TIMES, mwl=0.2, stretching=True)
    h.set_wave_directions(th)
    A = h.wave_kinematics(pts, TIMES, mwl=0.2)
    h.set_wave_directions(-th)
    B = h.wave_kinematics(mirror, TIMES, mwl=0.2)
    assert np.all(np.abs(A[0] - B[0]) <= 2 * TOL * se)
    assert np.all(np.abs(A[1] - B[1] * flip) <= 2 * TOL * sv) and np.all(np.abs(A[2] - B[2] * flip) <= 2 * TOL * sa)


# ------------------------------------------------------------------------------------------------
# Morison, nonlinear panels and clipped triangles
# ------------------------------------------------------------------------------------------------
ELEMENTS = (np.array([[4.0, 6.0, -3.0], [-5.0, -2.0, -6.0], [0.5, 8.0, -1.0]]), np.full((3, 3), 0.8), np.full((3, 3), 0.5))


def morison_state(N, b):
    pos, rpy, lin, ang = (np.zeros((N, 3)) for _ in range(4))
    pos[b], rpy[b], lin[b], ang[b] = [2.0, -3.0, -1.0], [0.05, -0.04, 0.9], [0.3, -0.2, 0.1], [0.02, 0.03, -0.05]
    return pos, rpy, lin, ang


def test_morison_on_a_yawed_body_and_its_independence(hydro):
    HF, HG = hydro[0].HydroForces, hydro[0].HydroGroup
    case1, case3 = sphere_case(), three_body_case()
    th = thetas(257)
    t = 14.2
    h = HF.from_case(case1)
    spread_sea(h, case1)
    h.set_wave_directions(th)
    h.set_morison_elements(0, *ELEMENTS)
    h.set_morison_options(mwl=0.1)
    st = morison_state(1, 0)
    got = h.compute_morison(t, *st)
    ref = dr.morison(irregular_comp(h, th), case1["water_depth"], case1["rho"], [ELEMENTS], t, *st, mwl=0.1, stretching=True,
                     ramp=spectral_ref.ramp_factor(t, IRREG["ramp_duration"]))
    err = np.abs(got - ref["F"][0])
    print("morison worst error / bound", np.max(err / ref["bound"][0]))
    assert np.all(err <= ref["bound"][0]) and abs(got[1]) > 1.0 and ref["margin"] > 1e-6
    # a three-body system (infinite depth): body 1 carries the list; alone, beside other bodies' lists, and on a shard of its own
    st3 = morison_state(3, 1)
    a = HF.from_case(case3)
    spread_sea(a, case3)
    a.set_wave_directions(th)
    a.set_morison_elements(1, *ELEMENTS)
    alone = a.compute_morison(t, *st3)[6:12]
    a.set_morison_elements(0, ELEMENTS[0][:2] + 1.0, ELEMENTS[1][:2], ELEMENTS[2][:2])
    a.set_morison_elements(2, ELEMENTS[0][:1] - 1.0, ELEMENTS[1][:1], ELEMENTS[2][:1])
    assert np.array_equal(a.compute_morison(t, *st3)[6:12], alone)
    g = HG.from_case(case3, 3)
    spread_sea(g, case3)
    g.set_wave_directions(th)
    g.set_morison_elements(1, *ELEMENTS)
    assert np.array_equal(np.asarray(g.compute_morison(t, *st3)).reshape(-1)[6:12], alone)
    ref3 = dr.morison(irregular_comp(a, th), np.inf, case3["rho"], [None, ELEMENTS, None], t, *st3, stretching=True,
                      ramp=spectral_ref.ramp_factor(t, IRREG["ramp_duration"]))
    assert np.all(np.abs(alone - ref3["F"][1]) <= ref3["bound"][1])
    # the number of bodies: the same body data, sea, directions, list and state as the only body of a 1-body system and as body 2
    # of a 3-body one whose other bodies move differently (tests/test_gpu_morison.py does this for the long-crested sea)
    from hydrochrono_amd.synthetic import many_body_case
    s1, s3 = (many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7) for N in (1, 3))
    one, three = HF.from_case(s1), HF.from_case(s3)
    for hh, cs, b in ((one, s1, 0), (three, s3, 2)):
        spread_sea(hh, cs)
        hh.set_wave_directions(th)
        hh.set_morison_elements(b, *ELEMENTS)
        hh.set_morison_options(mwl=0.1)
    three.set_morison_elements(0, ELEMENTS[0][:2] + 1.0, ELEMENTS[1][:2], ELEMENTS[2][:2])
    sa, sb = morison_state(1, 0), morison_state(3, 2)
    for x in sb:
        x[:2] += 0.37
    fa, fb = one.compute_morison(t, *sa), three.compute_morison(t, *sb)
    assert fa.any() and np.array_equal(fa, fb[12:])


BOX = nonlinear_ref.box_triangles([-2.0, -1.0, -3.0], [2.0, 1.0, 1.0], m=2)


@pytest.mark.parametrize("clip", [False, True])
def test_nonlinear_surface_against_the_reference(hydro, clip):
    case = sphere_case()
    h = hydro[0].HydroForces.from_case(case)
    spread_sea(h, case)
    th = thetas(257)
    h.set_wave_directions(th)
    h.set_surface_mesh(0, BOX, clip=clip)
    t, pos, rpy = 21.3, [1.0, 4.0, -0.2], [0.04, -0.03, 0.7]
    buoy, fk, _ = h.compute_nonlinear(t, pos, rpy)
    comp = irregular_comp(h, th)
    kw = dict(stretching=True, ramp=spectral_ref.ramp_factor(t, IRREG["ramp_duration"]))
    if clip:
        ref = dr.clipped(comp, case["water_depth"], case["rho"], case["g"], [BOX], t, pos, rpy, **kw)
    else:
        ref = dr.nonlinear(comp, case["water_depth"], case["rho"], case["g"], [nonlinear_ref.triangles_to_panels(BOX)], t, pos, rpy, **kw)
    for got, key in ((buoy, "buoy"), (fk, "fk")):
        err = np.abs(got - ref[key][0])
        print(key, "worst error / bound", np.max(err / ref["bound_" + key][0]))
        assert np.all(err <= ref["bound_" + key][0]), key
    assert abs(fk[1]) > 1.0


@pytest.mark.parametrize("clip", [False, True])
def test_regular_wave_of_heading_beta_on_a_mesh_rotated_by_beta(hydro, clip):
    case = sphere_case()
    beta = 0.6
    cb, sb = np.cos(beta), np.sin(beta)
    Rz = np.array([[cb, -sb, 0.0], [sb, cb, 0.0], [0.0, 0.0, 1.0]])
    h = hydro[0].HydroForces.from_case(case)
    h.add_waves_regular(REG_AMP * 4, 0.9)
    h.set_surface_mesh(0, BOX, clip=clip)
    t, pos = 3.1, np.array([1.5, 0.0, -0.1])
    _, fk0, _ = h.compute_nonlinear(t, pos, [0.0, 0.0, 0.0])
    h.set_wave_directions([beta])
    h.set_surface_mesh(0, BOX @ Rz.T, clip=clip)
    _, fk1, _ = h.compute_nonlinear(t, Rz @ pos, [0.0, 0.0, 0.0])
    comp = dr.with_directions(wk.regular_components(REG_AMP * 4, 0.9, h.regular_coeffs()[2], 0.0), beta)
    fn = dr.clipped if clip else dr.nonlinear
    mesh = (BOX @ Rz.T) if clip else nonlinear_ref.triangles_to_panels(BOX @ Rz.T)
    ref = fn(comp, case["water_depth"], case["rho"], case["g"], [mesh], t, Rz @ pos, [0.0, 0.0, 0.0])
    bound = ref["bound_fk"][0]
    assert np.all(np.abs(fk1 - ref["fk"][0]) <= bound)
    want = np.concatenate([Rz @ fk0[:3], Rz @ fk0[3:]])
    b3 = np.concatenate([np.full(3, np.linalg.norm(bound[:3])), np.full(3, np.linalg.norm(bound[3:]))])
    assert np.all(np.abs(fk1 - want) <= 2 * b3) and np.linalg.norm(fk0[:2]) > 1.0


# ------------------------------------------------------------------------------------------------
# first-order excitation under a heading
# ------------------------------------------------------------------------------------------------
def heading_tables_for(case, n_dir=3, seed=8):
    bd = case["bodies"][0]
    w = np.asarray(bd["w"], dtype=np.float64)
    mag0, ph0 = np.asarray(bd["ex_mag"]).reshape(6, -1), np.asarray(bd["ex_phase"]).reshape(6, -1)
    rng = np.random.default_rng(seed)
    dirs = np.array([-0.8, 0.1, 1.1])[:n_dir]
    mag = np.stack([mag0 * f for f in rng.uniform(0.5, 1.5, n_dir)], axis=1)
    ph = np.stack([ph0 + d for d in rng.uniform(-1.0, 1.0, n_dir)], axis=1)
    return dirs, w, mag, ph


def test_spectral_excitation_with_heading_tables(hydro):
    case = sphere_case()
    kw = dict(IRREG, nfrequencies=12, ramp_duration=0.0)
    dirs, w, mag, ph = heading_tables_for(case)
    h = hydro[0].HydroForces.from_case(case)
    h.set_body_excitation_rao_headings(0, dirs, w, mag, ph)
    assert h.excitation_rao_headings_size(0) == (3, w.size)
    h.add_waves_irregular(spectral=True, **kw)
    base = np.array([h.compute_waves(t) for t in (0.0, 3.3, 17.1)])
    spec = h.irreg_spectrum()
    A, om, _, phi = wk.irregular_components(spec)
    th = np.random.default_rng(2).uniform(dirs[0], dirs[-1], 12)
    h.set_wave_directions(th)
    m, p = dr.heading_tables(dirs, w, mag * case["rho"] * case["g"], ph, om, th)
    # the sum and the bound of tests/spectral_ref.py on these tables (the interpolation's own rounding, three operations on a
    # magnitude and on a phase, is inside that bound's 4 |theta| + 16 units per term)
    tab = dict(spectral_ref.tables(case, spec), X=np.asarray(m, dtype=np.float64), P=np.asarray(p, dtype=np.float64))
    times = (0.0, 3.3, 17.1)
    ref, bound = spectral_ref.forces(tab, 0.0, times), spectral_ref.bound(tab, times)
    for k, t in enumerate(times):
        err = np.abs(h.compute_waves(t) - np.asarray(ref[k], dtype=np.float64))
        print("heading tables t =", t, "worst error / bound", np.max(err / np.maximum(bound[k], 1e-300)))
        assert np.all(err <= bound[k]), t
    spread = np.array([h.compute_waves(t) for t in times])
    assert not np.array_equal(spread, base)
    # tables replaced while the directions are in force: the excitation follows at once (a factor 2 is exact in every step of the
    # interpolation and the sum); removing them under non-uniform directions is refused and changes nothing
    h.set_body_excitation_rao_headings(0, dirs, w, 2.0 * mag, ph)
    assert np.array_equal(np.array([h.compute_waves(t) for t in times]), 2.0 * spread)
    with pytest.raises(hydro[0].HydroError) as e:
        h.set_body_excitation_rao_headings(0, [], [], [], [])
    assert status(e) == hydro[1].HC_ERR_INVALID and h.excitation_rao_headings_size(0) == (3, w.size)
    assert np.array_equal(np.array([h.compute_waves(t) for t in times]), 2.0 * spread)
    h.set_body_excitation_rao_headings(0, dirs, w, mag, ph)
    assert np.array_equal(np.array([h.compute_waves(t) for t in times]), spread)
    # under a uniform heading a body may lose its tables: it goes back to its {6,1,nw} table
    h.set_wave_directions(np.full(12, 0.3))
    h.set_body_excitation_rao_headings(0, [], [], [], [])
    assert np.array_equal(np.array([h.compute_waves(t) for t in times]), base)
    h.set_body_excitation_rao_headings(0, dirs, w, mag, ph)
    # a wave setter that fails on its arguments leaves the model, its directions and the tables built for them
    h.set_wave_directions(th)
    with pytest.raises(hydro[0].HydroError):
        h.add_waves_regular(REG_AMP, 1e6)  # outside the BEM frequency list
    assert np.array_equal(h.wave_directions(), th) and np.array_equal(np.array([h.compute_waves(t) for t in times]), spread)
    # every direction on a grid node: the bits of set_body_excitation_rao with that node's table
    for j in range(3):
        h.set_wave_directions(np.full(12, dirs[j]))
        node = np.array([h.compute_waves(t) for t in (0.0, 3.3, 17.1)])
        o = hydro[0].HydroForces.from_case(dict(case, bodies=[dict(case["bodies"][0], ex_mag=mag[:, j], ex_phase=ph[:, j])]))
        o.add_waves_irregular(spectral=True, **kw)
        assert np.array_equal(node, np.array([o.compute_waves(t) for t in (0.0, 3.3, 17.1)])), j
    # clearing restores the {6,1,nw} table
    h.set_wave_directions(None)
    assert np.array_equal(np.array([h.compute_waves(t) for t in (0.0, 3.3, 17.1)]), base)
    # outside the grid, and a body without heading tables under non-uniform directions
    with pytest.raises(hydro[0].HydroError) as e:
        h.set_wave_directions(np.full(12, 1.2))
    assert status(e) == hydro[1].HC_ERR_INVALID and h.wave_directions().size == 0
    h.set_body_excitation_rao_headings(0, [], [], [], [])
    h.set_wave_directions(np.full(12, 0.3))  # uniform: the {6,1,nw} table stays
    assert np.array_equal(np.array([h.compute_waves(t) for t in (0.0, 3.3, 17.1)]), base)
    with pytest.raises(hydro[0].HydroError) as e:
        h.set_wave_directions(th)
    assert status(e) == hydro[1].HC_ERR_INVALID


def test_regular_wave_coefficients_follow_the_heading(hydro):
    case = sphere_case()
    dirs, w, mag, ph = heading_tables_for(case)
    h = hydro[0].HydroForces.from_case(case)
    h.set_body_excitation_rao_headings(0, dirs, w, mag, ph)
    h.add_waves_regular(REG_AMP, REG_OMEGA)
    m0, p0, k0 = h.regular_coeffs()
    h.set_wave_directions([0.5])
    m1, p1, k1 = h.regular_coeffs()
    assert k1 == k0 and not np.array_equal(m1, m0)
    # the regular interpolator: index = omega / dw - 1 without clamping (inside the list here), then linear in the heading
    mr, pr = dr.heading_tables(dirs, w, mag * case["rho"] * case["g"], ph, [REG_OMEGA], [0.5])
    assert np.allclose(m1, np.asarray(mr[:, 0], dtype=float), rtol=1e-14, atol=0) and np.allclose(p1, np.asarray(pr[:, 0], dtype=float), rtol=1e-13, atol=1e-15)
    h.set_wave_directions([dirs[1]])
    o = hydro[0].HydroForces.from_case(dict(case, bodies=[dict(case["bodies"][0], ex_mag=mag[:, 1], ex_phase=ph[:, 1])]))
    o.add_waves_regular(REG_AMP, REG_OMEGA)
    assert all(np.array_equal(a, b) for a, b in zip(h.regular_coeffs()[:2], o.regular_coeffs()[:2]))
    assert np.array_equal(h.compute_waves(2.2), o.compute_waves(2.2))
    h.set_wave_directions(None)
    assert all(np.array_equal(a, b) for a, b in zip(h.regular_coeffs()[:2], (m0, p0)))


@pytest.mark.parametrize("ahead", [1])
def test_uniform_heading_between_steps_of_an_irf_run_changes_no_force(hydro, ahead):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = sphere_case()
    runs = []
    for with_calls in (False, True):
        h = hydro[0].HydroForces.from_case(case)
        h.set_pass_schedule(ahead)
        h.add_waves_irregular(**IRREG)
        motion = PrescribedMotion(1, [case["bodies"][0]["cg"]], seed=3)
        forces = []
        for n in range(48):
            t = SPHERE_DT * n
            forces.append(h.step(t, *motion.state(t)))
            if with_calls:
                h.set_wave_directions(np.full(257, 0.4) if n % 2 == 0 else None)
        runs.append(np.array(forces))
        h.close()
    assert np.array_equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------
# errors and refusals
# ------------------------------------------------------------------------------------------------
def test_errors_refusals_and_what_drops_the_directions(hydro):
    HF, HE, capi = hydro[0].HydroForces, hydro[0].HydroError, hydro[1]
    case = sphere_case()
    h = HF.from_case(case)

    def refused(fn, code):
        with pytest.raises(HE) as e:
            fn()
        assert status(e) == code, (status(e), str(e.value))
        return str(e.value)

    # no model, NoWave, an imported record: no components
    refused(lambda: h.set_wave_directions([0.1]), capi.HC_ERR_INVALID)
    h.add_waves_none()
    refused(lambda: h.set_wave_directions([0.1]), capi.HC_ERR_INVALID)
    h.set_wave_directions(None)  # clearing nothing is fine
    tt = np.arange(0.0, 40.0, 0.1)
    h.add_waves_irregular_eta(tt, 0.1 * np.sin(tt), SPHERE_DT)
    refused(lambda: h.set_wave_directions([0.1]), capi.HC_ERR_INVALID)
    # the IRF model: wrong n, non-finite, non-uniform (unsupported, pointing to the spectral model), uniform accepted
    h.add_waves_irregular(**IRREG)
    refused(lambda: h.set_wave_directions(np.zeros(256)), capi.HC_ERR_INVALID)
    refused(lambda: h.set_wave_directions(np.full(257, np.nan)), capi.HC_ERR_INVALID)
    assert "spectral" in refused(lambda: h.set_wave_directions(thetas(257)), capi.HC_ERR_UNSUPPORTED)
    assert h.wave_directions().size == 0
    h.set_wave_directions(np.full(257, 0.3))
    # every wave setter drops them
    for setter, n in ((lambda: h.add_waves_regular(REG_AMP, REG_OMEGA), 1), (lambda: h.add_waves_irregular(**IRREG), 257),
                      (lambda: h.add_waves_irregular_eta(tt, 0.1 * np.sin(tt), SPHERE_DT), 0), (lambda: h.add_waves_irregular(**IRREG), 257),
                      (lambda: h.add_waves_none(), 0), (lambda: h.add_waves_irregular(spectral=True, **IRREG), 257)):
        setter()
        assert h.wave_directions().size == 0
        if n:
            h.set_wave_directions(np.full(n, 0.3))
            assert h.wave_directions().size == n
    # the terms that refuse while directions are set, and work again once they are cleared
    refused(lambda: h.set_wave_directions(np.zeros(1)), capi.HC_ERR_INVALID)
    st = morison_state(1, 0)
    h.set_morison_elements(0, *ELEMENTS)
    h.set_surface_mesh(0, BOX)
    omega = np.linspace(0.2, 2.0, 6)
    h.set_drift_qtf(0, omega, np.ones((6, 6, 6)))
    h.set_sum_qtf(0, omega, np.ones((6, 6, 6)))
    calls = {"wave_kinematics2": lambda: h.wave_kinematics2(POINTS, TIMES),
             "morison2": lambda: h.compute_morison(1.0, *st),
             "nonlinear2": lambda: h.compute_nonlinear(1.0, st[0], st[1]),
             "drift": lambda: h.compute_drift(1.0, st[0]),
             "sum": lambda: h.compute_sum_qtf(1.0, st[0])}
    h.set_morison_second_order(True)
    h.set_nonlinear_second_order(True)
    h.set_drift_mode(2)
    h.set_sum_mode(1)
    assert h.wave_directions().size == 257
    for name, fn in calls.items():
        assert "direction" in refused(fn, capi.HC_ERR_UNSUPPORTED), name
    h.set_morison_second_order(False)
    h.set_nonlinear_second_order(False)
    h.set_drift_mode(0)
    h.set_sum_mode(0)
    for name in ("morison2", "nonlinear2", "drift", "sum"):  # first order, or switched off: fine under directions
        calls[name]()
    h.set_morison_second_order(True)
    h.set_nonlinear_second_order(True)
    h.set_drift_mode(2)
    h.set_sum_mode(1)
    h.set_wave_directions(None)
    for name, fn in calls.items():
        fn()
    # heading tables: the grid must increase strictly
    refused(lambda: h.set_body_excitation_rao_headings(0, [0.1, 0.1], [1.0, 2.0], np.ones((6, 2, 2)), np.ones((6, 2, 2))), capi.HC_ERR_INVALID)
    refused(lambda: h.set_body_excitation_rao_headings(1, [0.1], [1.0, 2.0], np.ones((6, 1, 2)), np.ones((6, 1, 2))), capi.HC_ERR_OUT_OF_RANGE)


def test_spreading_generator_through_the_python_layer(hydro):
    h = hydro[0].HydroForces.from_case(sphere_case())
    h.add_waves_irregular(**IRREG)
    th = h.set_wave_spreading(0.0, s=0.0)
    assert np.array_equal(th, np.zeros(257)) and np.array_equal(h.wave_directions(), th)
    a = hydro[0].wave_spreading_directions(30, 0.3, s=10, n_bins=15, seed=2)
    assert np.array_equal(np.sort(a[:15]), np.sort(a[15:])) and np.array_equal(a, hydro[0].wave_spreading_directions(30, 0.3, s=10, n_bins=15, seed=2))
    with pytest.raises(hydro[0].HydroError):
        h.set_wave_spreading(0.0, s=10)  # a spread sea on the IRF model
    # a group: generated once, set on every shard, returned
    g = hydro[0].HydroGroup.from_case(three_body_case(), 3)
    spread_sea(g, three_body_case())
    tg = g.set_wave_spreading(0.2, s=10, n_bins=16, seed=5)
    assert tg.shape == (257,) and np.array_equal(tg, hydro[0].wave_spreading_directions(257, 0.2, s=10, n_bins=16, seed=5))
    assert all(np.array_equal(sh.wave_directions(), tg) for sh in g.shards) and np.array_equal(g.wave_directions(), tg)


@pytest.mark.parametrize("mode", ["regular", "irregular"])
def test_cpp_caller_composes_as_the_python_layer(hydro, tmp_path, mode):
    from hydrochrono_amd import build as hb
    hb.build()
    assert os.path.exists(hb.BEMIO_LIB), "libhdf5 reader not built"
    exe = str(tmp_path / "directional_caller")
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "directional_caller.cpp"),
                    "-o", exe, "-L", libdir, "-lhydrochrono_amd", f"-Wl,-rpath,{libdir}"], check=True)
    h5 = os.path.join(GOLDEN_DIR, "sphere.h5")
    r = subprocess.run([exe, h5, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()])
    assert rows.shape == (12, 32)
    h = hydro[0].HydroForces(1)
    h.load_bemio_h5(h5)
    h.finalize()
    if mode == "regular":
        h.add_waves_regular(REG_AMP, REG_OMEGA, num_bodies=1)
        h.set_wave_directions([0.7])
    else:
        h.add_waves_irregular(simulation_dt=0.015, simulation_duration=60.0, ramp_duration=10.0, wave_height=2.0, wave_period=9.0,
                              frequency_min=0.03, frequency_max=0.9, nfrequencies=64)
        h.set_wave_directions(np.full(64, 0.4))
    h.set_morison_elements(0, [[1.0, 5.0, -6.0], [2.5, -3.5, -3.0]], [[3, 3, 12.0], [1, 1.5, 0.5]], [[0, 0, 0], [2, 2, 1.0]])
    h.set_morison_options(mwl=0.25, regular_phase=0.3)
    for row in rows:
        t, st = row[0], (row[1:4], row[4:7], row[7:10], row[10:13])
        total = h.step(t, *st)  # total + Morison term, as CoordinateFuncForBody
        assert same_bits((row[13:19], row[19:25]), (total, h.compute_morison(t, *st))), t
        e, v, a = h.wave_kinematics([[3.0, -4.0, -2.0]], [t], mwl=0.25, regular_phase=0.3)
        assert same_bits((row[25:26], row[26:29], row[29:32]), (e.reshape(-1), v.reshape(-1), a.reshape(-1))), t
    assert np.abs(rows[:, 20]).max() > 1.0 and np.abs(rows[:, 27]).max() > 1e-3  # a y force and a y velocity
