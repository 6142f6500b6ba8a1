"""The fixed inputs of tests/test_gpu_side_terms.py (Morison + nonlinear + drift together), shared with tests/test_side_terms_cpu.py,
which checks on the CPU that every one of them keeps the references' conditions: no element or panel closer than MIN_GAP to the free
surface, part of every list wet and part dry, the drift grids around the wave components, |theta| < 1e4.  TEST INFRASTRUCTURE ONLY.

Shapes (the smallest that cross every edge of the three kernels):
    body 0: 257 panels (one past a 256-panel chunk), no element,                              drift table nq = 9 with Q
    body 1: no panel, 7 elements,                                                             no table
    body 2: 5 panels, 300 elements (one past a 256-item workgroup),                           drift table nq = 33 without Q
so every term has a neighbour without it."""
import numpy as np

import drift_ref as dr
import morison_ref as mr
import nonlinear_ref as nr
import wave_kinematics_ref as wk

G = 9.81
MIN_GAP = 1e-6
NL_OPTS = dict(mwl=0.1, wave_stretching=True)
MOR_OPTS = dict(mwl=0.05, wave_stretching=True)

# ---- sections 2, 3, 5, 6: three_body_case() in irregular waves, inside the ramp ----
THREE_IRREG = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0,
                   frequency_min=0.05, frequency_max=0.8, nfrequencies=200, seed=3)
COMBOS = [(nl, dm) for nl in (1, 2) for dm in (1, 2, 3)]  # nonlinear mode x drift mode
STEPS_PER_COMBO = 36                                      # across a look-ahead block of 32 steps
COMPOSE_TIMES = 2.0 + 0.01 * np.arange(STEPS_PER_COMBO * len(COMBOS))  # 2.00 .. 4.15 s: inside the ramp of 5 s
BOUND_STEPS = (0, 17, 35)                                 # steps of every combination that are held to the references
SUBSET_TIMES = 2.5 + 0.01 * np.arange(13)                 # the nine steps of section 3's walk, then step_many's three and one more
                                                          # (section 6 uses the first three)

# ---- section 4: synth_case(3) through the wave models ----
SYNTH_DEPTH = 60.0  # long-wave, finite-depth and k d > 500 components are all present between 0.01 and 2 Hz
REG1, REG2 = (0.177, 2.094395102), (0.4, 1.3)
SEQ_PHASE = 0.7
SEQ_TIMES = (7.5, 33.3)  # inside and past the ramp of 20 s
REC_T = 0.05 * np.arange(400)
REC_ETA = 0.5 * np.sin(0.8 * REC_T)
REC_DT = 0.05


def irreg(nf, seed=4):
    return dict(simulation_dt=0.05, simulation_duration=100.0, ramp_duration=20.0, wave_height=3.0, wave_period=8.0, frequency_min=0.01,
                frequency_max=2.0, nfrequencies=nf, peak_enhancement_factor=2.0, seed=seed)


# (name, kind, parameters, Morison phase): the walk of test_tables_follow_the_wave_model; nonlinear and drift keep SEQ_PHASE
SEQUENCE = [
    ("1 regular", "regular", REG1, SEQ_PHASE),
    ("2 regular, Morison phase 0.2", "regular", REG1, 0.2),
    ("3 irregular nf 257", "irregular", irreg(257), 0.2),
    ("4 spectral nf 255", "spectral", irreg(255, seed=11), 0.2),
    ("5 irregular nf 5", "irregular", irreg(5), 0.2),
    ("6 eta record", "eta", None, 0.2),
    ("7 regular, another wave", "regular", REG2, 0.2),
    ("8 none", "none", None, 0.2),
    ("9 irregular nf 257 again", "irregular", irreg(257), 0.2),
]


def synth_case(N=3, depth=SYNTH_DEPTH):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7, water_depth=depth)


def random_panels(n, seed, spread=6.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, size=(n, 3)), rng.normal(size=(n, 3)) * 0.3


def random_elements(n, seed, spread=10.0):
    rng = np.random.default_rng(seed)
    r = rng.uniform(-spread, spread, size=(n, 3))
    cd = rng.uniform(0.0, 3.0, size=(n, 3))
    cm = rng.uniform(0.0, 4.0, size=(n, 3))
    cm[::3] = 0.0
    cd[1::5, 1] = 0.0
    return r, cd, cm


def three_body_lists(lo, hi, seeds):
    """panels, elements and drift tables (grids on [lo, hi] rad/s) per body, None where a body carries none.  seeds: of the four
    random lists, chosen so that tests/test_side_terms_cpu.py passes (the first seeds from 100, 150, 200, 250 that keep the conditions)"""
    g33, P33, _ = dr.random_table(33, 72, lo + 0.1, hi - 0.2)
    return dict(panels=[random_panels(257, seeds[0]), None, random_panels(5, seeds[1])],
                elements=[None, random_elements(7, seeds[2]), random_elements(300, seeds[3])],
                tables=[dr.random_table(9, 70, lo, hi), None, (g33, P33, None)])


def compose_lists():
    return three_body_lists(0.6, 3.0, (100, 150, 201, 250))


def sequence_lists():
    return three_body_lists(0.5, 3.5, (100, 151, 201, 250))  # holds both regular waves and a component of the 5-component model


def set_lists(h, lists, which=("panels", "elements", "tables")):
    """on a HydroForces or a HydroGroup"""
    for b in range(3):
        if "panels" in which and lists["panels"][b] is not None:
            h.set_surface_panels(b, *lists["panels"][b])
        if "elements" in which and lists["elements"][b] is not None:
            h.set_morison_elements(b, *lists["elements"][b])
        if "tables" in which and lists["tables"][b] is not None:
            g, P, Q = lists["tables"][b]
            h.set_drift_qtf(b, g, P, Q)


def clear_lists(h, which):
    for b in range(3):
        if "panels" in which:
            h.set_surface_panels(b, np.zeros((0, 3)), np.zeros((0, 3)))
        if "elements" in which:
            h.set_morison_elements(b, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
        if "tables" in which:
            h.set_drift_qtf(b, [], None)


def compose_motion(case):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    return PrescribedMotion(3, [bd["cg"] for bd in case["bodies"]], seed=4)


def sequence_state(t):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((3, 3))
    rest[:, 0] = 15.0 * np.arange(3)
    rest[:, 2] = -1.0
    return PrescribedMotion(3, rest, seed=3, amplitude=0.5).state(t)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compose(total, nl, mor, dft, nl_mode, panelled):
    """((total - hs_lin + buoy [+ fk]) + morison) + drift in exactly this order; a term that is None is not composed.  `panelled`:
    the bodies that carry panels."""
    out = np.array(total, dtype=np.float64, copy=True)
    if nl is not None and nl_mode:
        buoy, fk, hs = nl
        for b in panelled:
            r = slice(6 * b, 6 * b + 6)
            out[r] = total[r] - hs[r] + buoy[r]
            if nl_mode == 2:
                out[r] = out[r] + fk[r]
    if mor is not None:
        out = out + mor
    if dft is not None:
        out = out + dft
    return out


# ---- the references, with the conditions they need ----
def references(case, lists, comp, t, state, ramp, nl_opts, mor_opts, stretching_applies=True, comp_mor="same"):
    """dict(nl=nonlinear_ref result, mor=morison_ref result) at one state.  comp None: still water.  comp_mor: the components as the
    Morison term sees them where its regular phase differs."""
    pos, rpy, lin, ang = state
    comp_mor = comp if isinstance(comp_mor, str) else comp_mor
    nl = nr.nonlinear(comp, case["water_depth"], case["rho"], G, lists["panels"], t, pos, rpy, mwl=nl_opts["mwl"],
                      stretching=stretching_applies and nl_opts["wave_stretching"], ramp=ramp)
    mor = mr.morison(comp_mor, case["water_depth"], case["rho"], lists["elements"], t, pos, rpy, lin, ang, mwl=mor_opts["mwl"],
                     stretching=stretching_applies and mor_opts["wave_stretching"], ramp=ramp)
    return dict(nl=nl, mor=mor)


def check_conditions(ref, lists, what):
    """the margins and the wet counts of one references() result"""
    for name in ("nl", "mor"):
        r = ref[name]
        assert r["margin"] >= MIN_GAP, f"{what}: {name} is {r['margin']:.3e} m from the free surface (choose other inputs)"
        for b, wet in enumerate(r["wet"]):
            if wet.size > 1:
                assert 0 < wet.sum() < wet.size, (what, name, b, int(wet.sum()), wet.size)


def drift_refs(comp, lists):
    return [None if tb is None or comp is None else dr.PairSum(comp, tb) for tb in lists["tables"]]


def check_grids(comp, lists, what, regular=False):
    nf = comp[1].size
    for tb in lists["tables"]:
        if tb is None:
            continue
        inside = dr.cells(tb[0], comp[1])[0]
        if regular:
            assert inside.all(), what
        elif nf > 20:
            assert 10 <= inside.sum() <= nf - 10, (what, int(inside.sum()), nf)
        else:  # fewer components than the rule has room for: at least one inside and one outside
            assert 0 < inside.sum() < nf, (what, int(inside.sum()), nf)


def model_components(h_or_oracle, kind, params, phase):
    """(comp, ramp_duration, stretching_applies) of a wave model from a context (or the CPU oracle) that has been given it"""
    if kind == "regular":
        return wk.regular_components(params[0], params[1], h_or_oracle.regular_coeffs()[2], phase), 0.0, False
    if kind in ("irregular", "spectral"):
        return wk.irregular_components(h_or_oracle.irreg_spectrum()), params["ramp_duration"], True
    return None, 0.0, False


# ---- section 7: what tests/cpp/side_terms_caller.cpp builds (dyadic values: the same bits in both languages) ----
CPP_STEPS, CPP_SWITCH, CPP_DT = 40, 20, 0.015625
CPP_NL_OPTS = dict(mwl=0.125, wave_stretching=True)
CPP_MOR_OPTS = dict(mwl=0.0625, wave_stretching=True)
CPP_PANEL_BODIES, CPP_ELEMENT_BODIES, CPP_TABLE_BODIES = (0, 2), (1, 2), (0, 3)  # 0-based


def cpp_panels(body, n):
    k = np.arange(n)
    c = np.stack([-3.0 + 0.25 * ((k * 3 + body) % 25), -2.0 + 0.5 * ((k * 7) % 9), -4.0 + 0.125 * ((k * 11 + 5 * body) % 64)], axis=1)
    s = np.stack([0.25 - 0.0625 * (k % 9), -0.5 + 0.125 * ((k * 5) % 8), 0.375 - 0.03125 * ((k * 3) % 23)], axis=1)
    return c, s


def cpp_elements(body, n):
    k = np.arange(n)
    r = np.stack([-4.0 + 0.5 * ((k * 5 + body) % 17), -3.0 + 0.25 * ((k * 3) % 25), -6.0 + 0.125 * ((k * 13 + 7 * body) % 96)], axis=1)
    cd = np.stack([0.5 + 0.125 * (k % 7), 0.25 * ((k * 3) % 5), 1.0 + 0.0625 * (k % 11)], axis=1)
    cm = np.stack([0.5 * (k % 3), 1.5 + 0.25 * (k % 4), 0.125 * ((k * 7) % 13)], axis=1)
    return r, cd, cm


def cpp_table(body, nq, with_q):
    omega = 0.75 + 0.3125 * np.arange(nq)
    d, m, n = np.meshgrid(np.arange(6.0), np.arange(float(nq)), np.arange(float(nq)), indexing="ij")
    P = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n + 31.25 * body
    Q = 500.0 * (m - n) + 62.5 * d
    return omega, P, (Q if with_q else None)


def cpp_lists():
    """per body (four bodies): panels, elements, tables"""
    return dict(panels=[cpp_panels(0, 70), None, cpp_panels(2, 12), None],
                elements=[None, cpp_elements(1, 9), cpp_elements(2, 40), None],
                tables=[cpp_table(0, 9, True), None, None, cpp_table(3, 5, False)])


def cpp_state(n):
    """t, (pos, rpy, linvel, angvel) of step n, each [4][3]"""
    t = 2.0 + CPP_DT * n
    b = np.arange(4.0)
    z3 = np.zeros(4)
    pos = np.stack([15.0 * b + 0.03125 * n, 0.5 * b, -1.0 - 0.25 * b + 0.0078125 * n], axis=1)
    rpy = np.stack([0.001953125 * n + z3, -0.00390625 * n + 0.015625 * b, 0.0009765625 * n + z3], axis=1)
    lin = np.stack([0.125 + z3, 0.03125 * b, 0.25 - 0.0078125 * n + z3], axis=1)
    ang = np.stack([0.015625 + z3, -0.03125 + 0.0009765625 * n + z3, 0.0078125 * (b + 1)], axis=1)
    return t, (pos, rpy, lin, ang)
