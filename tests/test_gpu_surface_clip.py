"""Triangles clipped at the instantaneous free surface on the GPU (hc_set_surface_triangles, nl_tris_kernel of csrc/hc_nonlinear.hip)
against the tests' NumPy restatement of the definition (tests/surface_clip_ref.py), fed the context's own spectrum / regular-wave
coefficients, through the C ABI via capi.py.

Tolerance: the bounds surface_clip_ref returns per body and component (derived in its docstring: the 1e-11 sum|term| of
tests/test_gpu_wave_kinematics.py through p_d, (n_b + 64) 2^-52 sum|contribution| for the algebra and the fixed-shape sum, and the cut
term).  The inputs and the conditions they keep are in tests/surface_clip_inputs.py; every comparison asserts them on the reference
side first (tests/test_surface_clip_ref_cpu.py does so without a GPU)."""
import ctypes as C

import numpy as np
import pytest

import drift_ref as dr
import nonlinear_ref as nr
import surface_clip_inputs as ci
import surface_clip_ref as sc
from cases import three_body_case

pytestmark = pytest.mark.gpu
G = ci.G


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def set_all(h, tris):
    for b, tl in enumerate(tris):
        h.set_surface_mesh(b, np.zeros((0, 3, 3)) if tl is None else tl, clip=True)


def inside(got, ref, what):
    """GPU (buoy, fk) [N][6] inside the reference's bounds, component by component; prints every figure first"""
    for name, g, want, bound in (("buoy", got[0], ref["buoy"], ref["bound_buoy"]), ("fk", got[1], ref["fk"], ref["bound_fk"])):
        g = np.asarray(g).reshape(want.shape)
        assert np.all(np.isfinite(g)), (what, name)
        err = np.abs(g - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{what} {name}: worst |gpu - ref| / bound = {worst:.3e}, max |F| = {np.max(np.abs(want)):.3e}, cases {ref['cases'].sum(axis=0).tolist()}")
        assert np.all(err <= bound), f"{what} {name}: worst {worst:.3e} of the bound"


# ------------------------------------------------------------------------------------------------
# 1: the definition against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ci.SYSTEMS, ids=[s[0] for s in ci.SYSTEMS])
def test_against_the_reference(HF, system):
    name, N, depth, kind, params = system
    case = ci.synth_case(N, depth)
    h = HF.from_case(case)
    seen = np.zeros(4, dtype=int)
    models = ("none", "nowave") if kind == "none" else (kind,)
    results = {}
    for model in models:  # still water: no model at all, then NoWave
        if model == "nowave":
            h.add_waves_none()
        ci.add_waves(h, kind, params)
        comp = ci.components(h, kind, params)
        if kind in ("irregular", "spectral"):
            assert comp[0].size == params["nfrequencies"]
        for n, mwl, stretching, t, ramp in ci.comparisons(kind, N):
            tris = ci.lists(N, n)
            set_all(h, tris)
            assert [h.surface_triangle_count(b) for b in range(N)] == [0 if tl is None else len(tl) for tl in tris]
            h.set_nonlinear_options(mwl=mwl, regular_phase=ci.REG_PHASE, wave_stretching=stretching)
            what = f"{name} ({model}) n={n} mwl={mwl} stretching={stretching} t={t}"
            ref, pos, rpy = ci.reference(case, tris, comp, kind, n, mwl, stretching, t, ramp, what)
            buoy, fk, _ = h.compute_nonlinear(t, pos, rpy)
            inside((buoy, fk), ref, what)
            seen += ref["cases"].sum(axis=0)
            results[(model, n, mwl, stretching, t)] = (buoy, fk)
            if N == 3:
                assert not buoy[6:12].any() and not fk[6:12].any()
            if kind == "none":
                assert not fk.any()
            elif n > 1:
                assert np.abs(fk[:6]).max() > 1.0
    assert np.all(seen > 0), seen.tolist()
    if kind == "none":
        for key, val in results.items():
            if key[0] == "nowave":
                assert same_bits(val[0], results[("none",) + key[1:]][0])
    if kind in ("irregular", "spectral"):  # stretching and mwl are seen
        n = 257
        assert not np.array_equal(results[(kind, n, 0.35, True, 33.3)][1], results[(kind, n, 0.35, False, 33.3)][1])
        assert not np.array_equal(results[(kind, n, 0.35, True, 33.3)][1], results[(kind, n, 0.0, True, 33.3)][1])


# ------------------------------------------------------------------------------------------------
# 2: a vertex exactly on the surface
# ------------------------------------------------------------------------------------------------
def test_a_mesh_row_exactly_on_the_surface(HF):
    """Still water, mwl = 0.5, the upright box [-1, 1] x [-0.5, 0.5] x [-1, 1] at pos.z = 0.5 with two rows per side: the middle row of
    vertices has h = 0 exactly (every coordinate is a dyadic number, R is the identity).  Those vertices count as wet, the sub-triangles
    they span above the surface have no area, and the result is rho g A (mwl - z_bottom)."""
    case = ci.synth_case(1)
    h = HF.from_case(case)
    tri = nr.box_triangles([-1.0, -0.5, -1.0], [1.0, 0.5, 1.0], m=2)
    h.set_surface_mesh(0, tri, clip=True)
    h.set_nonlinear_options(mwl=0.5)
    pos, rpy = np.array([[0.25, -0.5, 0.5]]), np.zeros((1, 3))
    ref = sc.clipped(None, case["water_depth"], case["rho"], G, [tri], 0.0, pos, rpy, mwl=0.5)
    on = ref["h"][0] == 0.0
    assert on.any(axis=1).sum() >= 16 and ref["cases"][0][0] == 8  # only the top face is dry: the upper side rows touch the surface
    upper = on.any(axis=1) & (ref["h"][0] > 0).any(axis=1)
    assert upper.sum() >= 8 and np.all((ref["h"][0][upper] <= 0).sum(axis=1) >= 1)
    buoy, fk, _ = h.compute_nonlinear(0.0, pos, rpy)
    inside((buoy, fk), ref, "row on the surface")
    want = case["rho"] * G * 2.0 * 1.0 * 1.0
    assert abs(buoy[2] - want) <= ref["bound_buoy"][0, 2] and not fk.any()
    # the upper rows alone contribute nothing at all: zero-area sub-triangles
    h.set_surface_mesh(0, tri[upper], clip=True)
    buoy_up = h.compute_nonlinear(0.0, pos, rpy)[0]
    assert np.all(np.abs(buoy_up) <= sc.clipped(None, case["water_depth"], case["rho"], G, [tri[upper]], 0.0, pos, rpy, mwl=0.5)["bound_buoy"][0])
    assert not buoy_up[:3].any()


# ------------------------------------------------------------------------------------------------
# 3: mesh independence in still water
# ------------------------------------------------------------------------------------------------
def test_still_water_result_does_not_depend_on_the_mesh(HF):
    case = ci.synth_case(3)
    h = HF.from_case(case)
    coarse, fine = ci.mesh(12), ci.mesh(768)
    set_all(h, [coarse, fine, None])
    pos, rpy = ci.state(3, 0.0)
    pos[1], rpy[1] = pos[0], rpy[0]  # the two boxes in the same tilted state
    ref = sc.clipped(None, case["water_depth"], case["rho"], G, [coarse, fine, None], 0.0, pos, rpy)
    assert ref["cut_span"] >= ci.MIN_SPAN and np.all(ref["cases"][:2, 1] + ref["cases"][:2, 2] > 0)
    buoy = h.compute_nonlinear(0.0, pos, rpy)[0].reshape(3, 6)
    inside((buoy, np.zeros((3, 6))), ref, "tilted boxes")
    both = ref["bound_buoy"][0] + ref["bound_buoy"][1]
    print("12 against 768 triangles:", np.abs(buoy[0] - buoy[1]).tolist(), "allowed", both.tolist())
    assert np.all(np.abs(buoy[0] - buoy[1]) <= both) and np.all(both < 1e-9 * abs(buoy[0, 2]))
    assert abs(buoy[0, 3]) > 1e-3 * abs(buoy[0, 2])  # tilted: a righting moment
    # upright, draft 1.85 + 0.3: both are the closed form
    pos[:2], rpy[:2] = [2.0, 1.0, -0.15], [0.0, 0.0, 0.9]
    h.set_nonlinear_options(mwl=0.3)
    ref = sc.clipped(None, case["water_depth"], case["rho"], G, [coarse, fine, None], 0.0, pos, rpy, mwl=0.3)
    buoy = h.compute_nonlinear(0.0, pos, rpy)[0].reshape(3, 6)
    want = case["rho"] * G * 2.0 * 1.0 * (0.3 - (-0.15 - 2.0))
    for b in (0, 1):
        assert abs(buoy[b, 2] - want) <= ref["bound_buoy"][b, 2], (b, buoy[b, 2] - want)
        assert np.all(np.abs(buoy[b, :2]) <= ref["bound_buoy"][b, :2])


# ------------------------------------------------------------------------------------------------
# 4: eta at a vertex is hc_wave_kinematics' eta
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stretching", [True, False])
def test_vertex_eta_is_the_kinematics_eta(HF, stretching):
    """Single-triangle bodies, rpy = 0, vertex 0 at the body reference (P_0 = pos exactly) and the two others 5 m above it.  Vertex 0 is
    placed at eta + mwl and ulp-scale steps around it, eta being what hc_wave_kinematics returns for that point, time and options:
    the triangle has a wet part of non-zero area iff (pos.z - mwl) - eta < 0 in float64 -- at exactly 0 the vertex is wet and the
    wet part has no area; above, the triangle is dry."""
    N, mwl, t = 3, 0.35, 33.3
    case = ci.synth_case(N)
    h = HF.from_case(case)
    h.add_waves_irregular(**ci.irreg(257))
    h.set_nonlinear_options(mwl=mwl, wave_stretching=stretching)
    tri = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 5.0], [0.0, 1.0, 5.0]]])
    set_all(h, [tri] * N)
    x = np.array([3.0, 18.5, 41.25])
    rpy = np.zeros((N, 3))
    seen = set()
    for shift in (0.0, 1e-12, -1e-12, 3e-16, -3e-16, 1e-3, -1e-3):
        pos = np.column_stack([x, np.zeros(N), np.zeros(N)])
        eta0 = h.wave_kinematics(pos, [t], mwl=mwl, wave_stretching=stretching)[0][0]  # eta does not depend on z
        pos[:, 2] = eta0 + mwl + shift
        eta = h.wave_kinematics(pos, [t], mwl=mwl, wave_stretching=stretching)[0][0]
        assert same_bits(eta, eta0) and np.abs(eta).max() > 1e-3
        want = (pos[:, 2] - mwl) - eta < 0.0
        buoy, fk, _ = (v.reshape(N, 6) for v in h.compute_nonlinear(t, pos, rpy))
        got = (buoy[:, 2] != 0.0) | (fk[:, 2] != 0.0)
        assert np.array_equal(got, want), (shift, want, buoy[:, 2], fk[:, 2])
        seen |= set(want.tolist())
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------
# 5: invariance, bitwise
# ------------------------------------------------------------------------------------------------
def random_panels(n, seed, spread=6.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, size=(n, 3)), rng.normal(size=(n, 3)) * 0.3


def subject_cases():
    """A 1-body case and 3-body cases that carry the SAME hydrostatic data at index j (everything hs_lin reads)."""
    one = ci.synth_case(1)
    subject = {k: one["bodies"][0][k] for k in ("disp_vol", "cg", "cb", "lin")}
    threes = []
    for j in range(3):
        c3 = ci.synth_case(3)
        c3["bodies"][j].update(subject)
        threes.append(c3)
    return one, threes


def rows(res, j):
    return np.concatenate([x[6 * j:6 * j + 6] for x in res])


def test_bits_do_not_depend_on_neighbours_kind_index_shard_or_resetting(HF):
    from hydrochrono_amd.hydro import HydroGroup
    one_case, three_cases = subject_cases()
    tl = ci.mesh(257)
    t = 33.3
    p1, r1 = ci.state(1, t)

    def prepare(h):
        h.add_waves_irregular(**ci.irreg(300))
        h.set_nonlinear_options(mwl=0.2)

    one = HF.from_case(one_case)
    prepare(one)
    one.set_surface_mesh(0, tl, clip=True)
    ref = np.concatenate(one.compute_nonlinear(t, p1, r1))
    assert ref[:6].any() and ref[6:12].any() and ref[12:].any()
    assert same_bits(np.concatenate(one.compute_nonlinear(t, p1, r1)), ref)  # a repeated call
    one.set_surface_mesh(0, np.zeros((0, 3, 3)), clip=True)  # cleared: zeros, no launch
    assert not np.concatenate(one.compute_nonlinear(t, p1, r1)[:2]).any() and one.surface_triangle_count(0) == 0
    one.set_surface_mesh(0, tl, clip=True)  # ... and set again
    assert same_bits(np.concatenate(one.compute_nonlinear(t, p1, r1)), ref)

    for j in range(3):
        three = HF.from_case(three_cases[j])
        grp = HydroGroup.from_case(three_cases[j], 2)
        pos, rpy = ci.state(3, t + 1.0)
        pos[j], rpy[j] = p1[0], r1[0]
        for h in (three, grp):
            prepare(h)
            h.set_surface_mesh(j, tl, clip=True)
        assert same_bits(rows(three.compute_nonlinear(t, pos, rpy), j), ref), j  # the others carry nothing
        for others in ("triangles", "panels", "mixed", "nothing"):
            for h in (three, grp):
                for k in range(3):
                    if k == j:
                        continue
                    if others == "triangles" or (others == "mixed" and k == (j + 1) % 3):
                        h.set_surface_mesh(k, ci.mesh(768 if k < j else 12), clip=True)  # three chunks before body j's, or one after
                    elif others in ("panels", "mixed"):
                        h.set_surface_panels(k, *random_panels(513, 61 + k))
                    else:
                        h.set_surface_panels(k, np.zeros((0, 3)), np.zeros((0, 3)))
            single = three.compute_nonlinear(t, pos, rpy)
            assert same_bits(rows(single, j), ref), (j, others)
            sharded = grp.compute_nonlinear(t, pos, rpy)  # two shards against the single context: every body, every term
            assert all(same_bits(x, y) for x, y in zip(sharded, single)), (j, others)
            if others == "mixed":
                # a panel body's bits do not depend on the triangle lists beside it
                k_pan = next(k for k in range(3) if k != j and k != (j + 1) % 3)
                kept = rows(single, k_pan)
                assert kept[:6].any()
                three.set_surface_mesh(j, np.zeros((0, 3, 3)), clip=True)
                three.set_surface_mesh((j + 1) % 3, np.zeros((0, 3, 3)), clip=True)
                cleared = three.compute_nonlinear(t, pos, rpy)
                assert same_bits(rows(cleared, k_pan), kept) and not rows(cleared, j)[:12].any()
                three.set_surface_mesh(j, tl, clip=True)
        three.close()
        for h in grp.shards:
            h.close()


# ------------------------------------------------------------------------------------------------
# 6: the layers above
# ------------------------------------------------------------------------------------------------
THREE_IRREG = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
                   frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)


def raw_step(h, t, st):
    from hydrochrono_amd import capi
    a = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in st]
    out = np.empty(h.D_local)
    rc = h.lib.hc_step(h.ctx, float(t), *[x.ctypes.data_as(capi.c_double_p) for x in a], out.ctypes.data_as(capi.c_double_p))
    assert rc == capi.HC_OK, h.lib.hc_last_error(h.ctx)
    return out


def test_step_composes_with_a_triangle_body(HF):
    """HydroForces.step and HydroGroup.step, modes 0, 1, 2: body 0 carries clipped triangles, body 2 the same mesh as centroid panels,
    body 1 Morison elements, body 0 a drift table: ((total - hs_lin + buoy [+ fk]) + morison) + drift on the separately computed terms,
    to the bit."""
    from hydrochrono_amd.hydro import HydroGroup, triangles_to_panels
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    case = three_body_case()
    box = nr.box_triangles([-2.0, -1.5, -3.0], [2.0, 1.5, 4.0], m=3)
    elements = (np.array([[0.0, 0.0, -4.0]]), np.array([[2.0, 0.5, 1.25]]), np.array([[1.0, 2.0, 3.0]]))
    table = dr.random_table(9, 70, 0.3, 5.2)
    motion = PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)

    def configured(h, lists=True):
        h.add_waves_irregular(**THREE_IRREG)
        if lists:
            h.set_surface_mesh(0, box, clip=True)
            h.set_surface_mesh(2, box)  # clip=False: centroid panels
            h.set_nonlinear_options(mwl=0.1)
        h.set_morison_elements(1, *elements)
        h.set_drift_qtf(0, *table)
        h.set_drift_mode(3)
        return h

    terms = configured(HF.from_case(case))  # mode 0: the terms one by one
    plain = configured(HF.from_case(case), lists=False)
    by_panels = configured(HF.from_case(case))
    by_panels.set_surface_panels(2, *triangles_to_panels(box))
    assert terms.surface_triangle_count(0) == 108 and terms.surface_panel_count(0) == 0
    assert terms.surface_triangle_count(2) == 0 and terms.surface_panel_count(2) == 108
    for mode in (0, 1, 2):
        a = configured(HF.from_case(case))
        grp = configured(HydroGroup.from_case(case, 2))
        assert grp.surface_triangle_count(0) == 108 and grp.surface_panel_count(2) == 108
        for h in (a, grp):
            h.set_nonlinear_mode(mode)
        differs = False
        for n in range(34):  # across a look-ahead block
            t = 2.0 + 0.01 * n
            st = motion.state(t)
            total = raw_step(terms, t, st)
            nl = terms.compute_nonlinear(t, st[0], st[1])
            mor, dft = terms.compute_morison(t, *st), terms.compute_drift(t, st[0])
            want = total.copy()
            if mode:
                for k in (0, 2):
                    r = slice(6 * k, 6 * k + 6)
                    want[r] = total[r] - nl[2][r] + nl[0][r]
                    if mode == 2:
                        want[r] = want[r] + nl[1][r]
            want = (want + mor) + dft
            fa = a.step(t, *st)
            assert same_bits(fa, want), (mode, n)
            assert same_bits(grp.step(t, *st), want), (mode, n)
            assert all(same_bits(x, y) for x, y in zip(by_panels.compute_nonlinear(t, st[0], st[1]), nl))  # clip=False is set_surface_panels
            if mode == 0:  # today's calls, today's bits
                assert same_bits(fa, plain.step(t, *st))
            else:
                assert all(same_bits(x, y) for x, y in zip(a.nonlinear(), nl))
            differs |= not same_bits(fa, (total + mor) + dft)
        assert differs == (mode != 0) and nl[0][:6].any() and nl[1][:6].any() and mor.any() and dft.any()
        a.close()
        for h in grp.shards:
            h.close()


# ------------------------------------------------------------------------------------------------
# 7: errors, and the two kinds of list of one body
# ------------------------------------------------------------------------------------------------
def test_errors_and_the_two_kinds_exclude_each_other(HF):
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroError
    INV, OK = capi.HC_ERR_INVALID, capi.HC_OK
    dp = (lambda a: None if a is None else a.ctypes.data_as(capi.c_double_p))
    case = three_body_case()
    h = HF.from_case(case)
    lib = h.lib
    n = C.c_int(-1)
    one = np.array([0.0, 0.0, -1.0, 0.0, 1.0, -2.0, 1.0, 0.0, -1.0])  # the normal points down: a wet one is pushed up
    z9, below = np.zeros(9), np.tile([0.0, 0.0, -5.0], 3)
    o = [np.full(18, 7.0) for _ in range(3)]

    def counts(b):
        return h.surface_panel_count(b), h.surface_triangle_count(b)

    for body in (-1, 3):
        assert lib.hc_set_surface_triangles(h.ctx, body, dp(one), 1) == INV
        assert lib.hc_get_surface_triangle_count(h.ctx, body, C.byref(n)) == INV
    assert lib.hc_get_surface_triangle_count(h.ctx, 0, None) == INV
    assert lib.hc_set_surface_triangles(h.ctx, 0, dp(one), -1) == INV
    assert lib.hc_set_surface_triangles(h.ctx, 0, None, 2) == INV
    assert lib.hc_set_surface_triangles(h.ctx, 0, dp(one), (1 << 20) + 1) == INV  # the cap (checked before the list is read)
    assert lib.hc_set_surface_triangles(h.ctx, 0, dp(np.tile(one, 2048)), 2048) == OK
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 4, 8):
            v = one.copy()
            v[at] = bad
            assert lib.hc_set_surface_triangles(h.ctx, 0, dp(v), 1) == INV
    assert counts(0) == (0, 2048)  # a refused list leaves the one before
    assert b"surface triangle" in lib.hc_last_error(h.ctx)
    assert lib.hc_set_surface_triangles(h.ctx, 0, None, 0) == OK and counts(0) == (0, 0)  # n = 0 clears; the list may then be NULL
    # a degenerate triangle is allowed and contributes nothing
    assert lib.hc_set_surface_triangles(h.ctx, 0, dp(np.tile([0.5, 0.25, -1.0], 3)), 1) == OK
    assert lib.hc_compute_nonlinear(h.ctx, 0.0, dp(below), dp(z9), dp(o[0]), dp(o[1]), dp(o[2])) == OK and not o[0].any() and not o[1].any()
    # while an evaluation is in flight
    assert lib.hc_nonlinear_begin(h.ctx, 0.0, dp(below), dp(z9)) == OK
    assert lib.hc_set_surface_triangles(h.ctx, 1, dp(one), 1) == INV
    assert lib.hc_nonlinear_end(h.ctx, dp(o[0]), None, None) == OK
    assert lib.hc_set_surface_triangles(h.ctx, 1, dp(one), 1) == OK
    assert lib.hc_compute_nonlinear(h.ctx, 0.0, dp(below), dp(z9), dp(o[0]), dp(o[1]), dp(o[2])) == OK and o[0][6 + 2] > 0
    # each setter clears the other list of that body, and of that body only
    h.set_surface_panels(1, [[0, 0, -1.0]], [[0, 0, -2.0]])
    assert counts(1) == (1, 0) and counts(0) == (0, 1)
    h.set_surface_mesh(1, one.reshape(1, 3, 3), clip=True)
    assert counts(1) == (0, 1)
    h.set_surface_mesh(1, np.tile(one, 3).reshape(3, 3, 3))  # clip=False: panels again
    assert counts(1) == (3, 0)
    h.set_surface_mesh(1, np.zeros((0, 3, 3)), clip=True)
    assert counts(1) == (0, 0) and counts(0) == (0, 1)
    with pytest.raises(HydroError):
        bad = one.reshape(1, 3, 3).copy()
        bad[0, 1, 2] = np.nan
        h.set_surface_mesh(0, bad, clip=True)
    # a shard context takes the lists of all bodies and computes those of its own
    sh = HF.from_case(case, body_range=(1, 3))
    for b in range(3):
        v = one.copy()
        v[2::3] -= b
        assert lib.hc_set_surface_triangles(sh.ctx, b, dp(v), 1) == OK
    o6 = [np.empty(12) for _ in range(3)]
    assert lib.hc_compute_nonlinear(sh.ctx, 0.0, dp(below), dp(z9), dp(o6[0]), dp(o6[1]), dp(o6[2])) == OK
    assert o6[0][2] > 0 and o6[0][8] > o6[0][2]
