"""The fixed inputs of tests/test_gpu_side_terms2.py (the Morison, nonlinear, drift and sum-frequency terms together, the first two
on the second-order sea), shared with tests/test_side_terms2_cpu.py, which checks on the CPU that every (model, time, state) the GPU
test holds to a reference keeps the references' conditions.  It builds on tests/side_terms_inputs.py and writes no
reference mathematics: the references are morison2_ref, nonlinear2_ref (which composes nonlinear_ref and surface_clip_ref),
drift_ref and sumfreq_ref, with the bounds they derive.  TEST INFRASTRUCTURE ONLY.

Shapes:
    body 0: 257 clipped triangles (one past a 256-triangle chunk), no element,    drift table nq = 9 with Q,     sum table nq = 9 with Q
    body 1: no surface, 7 elements,                                               no table
    body 2: 5 panels, 300 elements (one past a 256-item workgroup),               drift table nq = 33 without Q, sum table nq = 33 without Q
so every term has a neighbour without it, triangles and panels sit on different bodies and the sum tables on another grid than the
drift tables.  The small variant (12 triangles, 12 panels, 7 and 12 elements) is for 300 components, where the pair sum of the
references costs nf^2 per point."""
import numpy as np

import drift_ref as dr
import morison2_ref as m2
import morison_ref as mr
import nonlinear2_ref as n2
import nonlinear_ref as nr
import side_terms_inputs as si
import sumfreq_ref as sr
import surface_clip_inputs as ci
import wave2_inputs as wi

INF = float("inf")
FULL = (0.0, INF)
NO_PAIR = wi.NO_PAIR
MIN_GAP, MIN_SPAN = si.MIN_GAP, ci.MIN_SPAN
NL_OPTS, MOR_OPTS = si.NL_OPTS, si.MOR_OPTS
BOUND_RATIO = 1e-6  # every derived bound stays below this part of the largest component of its result

# ---- sections 1, 2 and 5: three_body_case() inside the ramp ----
STEPS = 36                 # across a look-ahead block of 32 steps
BOUND_STEPS = (0, 17, 35)  # 1a: the steps held to the references
BOUND_STEP_LARGE = 17      # 1b: the one step held to them
COMPOSE_TIMES = 9.0 + 0.01 * np.arange(STEPS)  # inside the ramp of 20 s of nonlinear2_inputs.waves()
SUBSET_TIMES = 2.5 + 0.01 * np.arange(26)      # sections 2 and 5, in si.THREE_IRREG: inside its ramp of 5 s


def compose_motion():
    """the bodies 15 m apart along the wave, their origins 0.5 m below the mean level: the box of body 0 crosses the surface"""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((3, 3))
    rest[:, 0] = 15.0 * np.arange(3)
    rest[:, 2] = -0.5
    return PrescribedMotion(3, rest, seed=4, amplitude=0.5)


def surface_lists(n_tri, n_pan, seed):
    """per body None, ("tris", [n][3][3]) or ("panels", (c, s)) as nonlinear2_ref takes them"""
    return [("tris", ci.mesh(n_tri)), None, ("panels", si.random_panels(n_pan, seed) if n_pan == 5 else nr.triangles_to_panels(ci.mesh(n_pan)))]


def make_lists(lo, hi, seeds, small=False, sum_shift=(-0.05, -0.25)):
    """surfaces, elements, drift tables on [lo, hi] rad/s and sum tables on another grid, [lo, hi] + sum_shift.  seeds: of the panel list and
    the two element lists, the first from 150, 200, 250 that keep the conditions of tests/test_side_terms2_cpu.py"""
    g33, P33, _ = dr.random_table(33, 72, lo + 0.1, hi - 0.2)
    s33, S33, _ = sr.random_table(33, 82, lo + sum_shift[0] + 0.1, hi + sum_shift[1] - 0.2)
    return dict(surfaces=surface_lists(12 if small else 257, 12 if small else 5, seeds[0]),
                elements=[None, si.random_elements(7, seeds[1]), si.random_elements(12 if small else 300, seeds[2])],
                tables=[dr.random_table(9, 70, lo, hi), None, (g33, P33, None)],
                sums=[sr.random_table(9, 80, lo + sum_shift[0], hi + sum_shift[1]), None, (s33, S33, None)])


def compose_lists(small=False):
    """sections 1, 2 and 5.  Of the five components of nonlinear2_inputs.waves(5) (0.63 .. 2.2 rad/s) every grid holds some and
    misses some; of the 200 of si.THREE_IRREG and the 300 of waves(300) more than ten on either side."""
    return make_lists(0.7, 2.3, (150, 201, 250), small)


def sequence_lists():
    """sections 3 and 4: grids that hold both regular waves and one component of the 5-component model"""
    return make_lists(0.5, 3.5, (151, 201, 250), sum_shift=(-0.05, 0.1))


def sum_tables_nine():
    """entry 9 of the walk: body 0's sum table cleared, body 2's replaced by one of nq 17 (with Q, on a grid of its own)"""
    return [None, None, sr.random_table(17, 91, 0.6, 3.3)]


def set_lists(h, lists, which=("surfaces", "elements", "tables", "sums")):
    """on a HydroForces or a HydroGroup"""
    for b in range(3):
        if "surfaces" in which and lists["surfaces"][b] is not None:
            kind, data = lists["surfaces"][b]
            (h.set_surface_mesh(b, data, clip=True) if kind == "tris" else h.set_surface_panels(b, *data))
        if "elements" in which and lists["elements"][b] is not None:
            h.set_morison_elements(b, *lists["elements"][b])
        if "tables" in which and lists["tables"][b] is not None:
            h.set_drift_qtf(b, *lists["tables"][b])
        if "sums" in which:
            set_sum_tables(h, lists["sums"], only=(b,))


def set_sum_tables(h, sums, only=(0, 1, 2)):
    """the three sum tables as given: None clears"""
    for b in only:
        (h.set_sum_qtf(b, [], None) if sums[b] is None else h.set_sum_qtf(b, *sums[b]))


def clear_lists(h, which):
    for b in range(3):
        if "surfaces" in which:  # the setter of either kind clears the body's one list
            (h.set_surface_mesh(b, np.zeros((0, 3, 3)), clip=True) if b == 0 else h.set_surface_panels(b, np.zeros((0, 3)), np.zeros((0, 3))))
        if "elements" in which:
            h.set_morison_elements(b, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
        if "tables" in which:
            h.set_drift_qtf(b, [], None)
        if "sums" in which:
            h.set_sum_qtf(b, [], None)


def compose4(total, nl, mor, dft, smf, nl_mode, surfaced):
    """(((total - hs_lin + buoy [+ fk]) + morison) + drift) + sum in exactly this order: si.compose, then the sum-frequency term as
    the last addition; a term that is None is not composed.  `surfaced`: the bodies that carry panels or triangles."""
    out = si.compose(total, nl, mor, dft, nl_mode, surfaced)
    return out if smf is None else out + smf


# ---- section 3: the walk.  si.SEQUENCE's wave models, with band and table changes between them ----
DIFF_ONLY, EMPTY = (FULL, NO_PAIR), (NO_PAIR, NO_PAIR)
# name, kind, parameters, Morison regular phase, nonlinear (diff_band, sum_band), sum tables ("lists" or "nine"), the order the
# nonlinear and Morison terms run at, what changed against the entry before ("model", "morison phase", "nonlinear bands", "sum tables")
WALK = [
    ("1 regular", "regular", si.REG1, si.SEQ_PHASE, (FULL, FULL), "lists", (2, 2), "model"),
    ("2 regular, Morison phase 0.2", "regular", si.REG1, 0.2, (FULL, FULL), "lists", (2, 2), "morison phase"),
    ("3 irregular nf 257", "irregular", si.irreg(257), 0.2, (FULL, FULL), "lists", (2, 2), "model"),
    ("4 nonlinear bands: difference only", "irregular", si.irreg(257), 0.2, DIFF_ONLY, "lists", (2, 2), "nonlinear bands"),
    ("5 nonlinear bands: no pair", "irregular", si.irreg(257), 0.2, EMPTY, "lists", (1, 2), "nonlinear bands"),
    ("6 nonlinear bands full again", "irregular", si.irreg(257), 0.2, (FULL, FULL), "lists", (2, 2), "nonlinear bands"),
    ("7 spectral nf 255", "spectral", si.irreg(255, seed=11), 0.2, (FULL, FULL), "lists", (2, 2), "model"),
    ("8 irregular nf 5", "irregular", si.irreg(5), 0.2, (FULL, FULL), "lists", (2, 2), "model"),
    ("9 sum tables: body 0 cleared, body 2 nq 17", "irregular", si.irreg(5), 0.2, (FULL, FULL), "nine", (2, 2), "sum tables"),
    ("10 eta record", "eta", None, 0.2, (FULL, FULL), "nine", (1, 1), "model"),
    ("11 regular, another wave, the tables of entry 8", "regular", si.REG2, 0.2, (FULL, FULL), "lists", (2, 2), "model"),
    ("12 none", "none", None, 0.2, (FULL, FULL), "lists", (1, 1), "model"),
    ("13 irregular nf 257 again", "irregular", si.irreg(257), 0.2, (FULL, FULL), "lists", (2, 2), "model"),
]
HELD = (0, 7, 8)      # entries 1, 8 and 9: every term held to its reference (0-based indices into WALK)
HELD_QTF = (2,)       # entry 3: the drift and sum terms only (nf nq, not nf^2)
KIN2_OTHER = dict(diff_band=(0.1, 0.7), sum_band=(2.0, 3.0), regular_phase=1.1)  # 3 (c): what hc_wave_kinematics2 is asked between


def walk_sums(lists, key):
    return lists["sums"] if key == "lists" else sum_tables_nine()


# ---- the references, with the conditions they need ----
def references(case, g, lists, sums, comps, rd, stretch, t, state, nl_bands, mor_bands=(FULL, FULL), orders=(2, 2), drift_modes=(3,)):
    """Every term's reference at one state.  comps: dict(nl, mor, dft, sum) of the components as each term sees them (a regular
    phase of its own).  rd: the ramp duration (0: none, a regular wave).  Returns dict(nl=nonlinear2_ref result, mor=morison2_ref
    result, dft={mode: ([N][6], bound [N][6])}, sum=([N][6], bound [N][6])); a body without a table has None rows."""
    pos, rpy, lin, ang = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in state)
    ramp = mr.ramp_factor(t, rd)
    depth, rho = case["water_depth"], case["rho"]
    nl = n2.nonlinear2(comps["nl"], g, depth, rho, lists["surfaces"], t, pos, rpy, mwl=NL_OPTS["mwl"],
                       stretching=stretch and NL_OPTS["wave_stretching"], ramp=ramp, diff_band=nl_bands[0], sum_band=nl_bands[1],
                       ramp_duration=rd, second_order=orders[0] == 2)
    mor = m2.morison2(comps["mor"], g, depth, rho, lists["elements"], t, pos, rpy, lin, ang, mwl=MOR_OPTS["mwl"],
                      stretching=stretch and MOR_OPTS["wave_stretching"], ramp=ramp, diff_band=mor_bands[0], sum_band=mor_bands[1],
                      ramp_duration=rd)
    out = dict(nl=nl, mor=mor, dft={}, sum=None)
    out.update(qtf_references(lists, sums, comps, rd, t, pos, drift_modes))
    return out


def qtf_references(lists, sums, comps, rd, t, pos, drift_modes=(3,)):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    ramp = mr.ramp_factor(t, rd)
    dft = {}
    for mode in drift_modes:
        rows = []
        for b, tb in enumerate(lists["tables"]):
            rows.append(None if tb is None else (dr.PairSum(comps["dft"], tb).force(t, pos[b, 0], ramp=ramp)[mode],
                                                 dr.bounds(comps["dft"], tb, ramp=ramp)[mode]))
        dft[mode] = rows
    smf = [None if tb is None else (sr.PairSum(comps["sum"], tb).force(t, pos[b, 0], ramp=ramp), sr.bound(comps["sum"], tb, ramp=ramp))
           for b, tb in enumerate(sums)]
    return dict(dft=dft, sum=smf)


def check_conditions(ref, lists, what):
    """The margins, the cut span, the wet counts and the size of the bounds of one references() result.  Returns the case counts
    of the triangle body [4]."""
    nl, mor = ref["nl"], ref["mor"]
    assert nl["margin"] >= MIN_GAP, f"{what}: a panel is {nl['margin']:.3e} m from the free surface (choose other inputs)"
    assert mor["margin"] >= MIN_GAP, f"{what}: an element is {mor['margin']:.3e} m from the free surface (choose other inputs)"
    assert nl["cut_span"] >= MIN_SPAN, f"{what}: a cut edge spans {nl['cut_span']:.3e} m in h (choose other inputs)"
    for b, wet in enumerate(mor["wet"]):
        if wet.size > 1:
            assert 0 < wet.sum() < wet.size, (what, "elements", b, int(wet.sum()), wet.size)
    cases = np.asarray(nl["cases"][0])
    n_tri = len(lists["surfaces"][0][1])
    assert cases.sum() == n_tri and cases[0] < n_tri and cases[3] < n_tri, (what, "triangles", cases.tolist())  # partly wet and partly dry
    kind, data = lists["surfaces"][2]
    c = np.asarray(data[0])
    assert kind == "panels" and len(nl["p"][2]) == len(c)
    wet = nl["p"][2][:, 2] - NL_OPTS["mwl"] - (np.asarray(nl["eta1"][2], dtype=np.longdouble) + nl["eta2"][2]) <= 0
    assert 0 < wet.sum() < wet.size, (what, "panels", int(wet.sum()), wet.size)
    for name, val, bound in (("buoy", nl["buoy"], nl["bound_buoy"]), ("fk", nl["fk"], nl["bound_fk"]), ("morison", mor["F"], mor["bound"])):
        check_bound(name, val, bound, what)
    return cases


def check_bound(name, val, bound, what):
    """per body: the bound below BOUND_RATIO of the largest component of the result"""
    val, bound = np.asarray(val, dtype=np.float64).reshape(-1, 6), np.asarray(bound, dtype=np.float64).reshape(-1, 6)
    for b in range(val.shape[0]):
        if val[b].any() or bound[b].any():
            assert bound[b].max() < BOUND_RATIO * np.abs(val[b]).max(), (what, name, b, float(bound[b].max()), float(np.abs(val[b]).max()))


def check_qtf_conditions(ref, what):
    for name, rows in [(f"drift mode {m}", r) for m, r in ref["dft"].items()] + [("sum", ref["sum"])]:
        for b, row in enumerate(rows):
            if row is not None:
                check_bound(name, row[0], row[1], f"{what} body {b}")


def check_grids(comp, lists, sums, what, regular=False):
    """si.check_grids for the drift grids and for the sum grids"""
    si.check_grids(comp, lists, what + " (drift grids)", regular=regular)
    si.check_grids(comp, dict(tables=sums), what + " (sum grids)", regular=regular)


def pair_counts(w, bands):
    """(pairs inside the difference band, pairs inside the sum band) of the components w under (diff_band, sum_band)"""
    import wave2_ref as w2
    md, ms = w2.band_masks(np.asarray(w, dtype=np.float64), bands[0], bands[1])
    return int(np.sum(md)), int(np.sum(ms))


def model_components(h_or_oracle, kind, params, phases):
    """(comps, ramp_duration, stretching_applies): the components as each term sees them, phases = dict(nl, mor, dft, sum)"""
    out = {k: si.model_components(h_or_oracle, kind, params, ph) for k, ph in phases.items()}
    any_ = next(iter(out.values()))
    return {k: v[0] for k, v in out.items()}, any_[1], any_[2]


# ---- section 6: what tests/cpp/side_terms2_caller.cpp builds (dyadic values: the same bits in both languages) ----
CPP_STEPS, CPP_SWITCH = 24, 12
CPP_WAVES = dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=5.0, wave_height=2.0, wave_period=7.0, frequency_min=0.05,
                 frequency_max=0.8, nfrequencies=24, seed=3)
CPP_WAVES_AFTER = dict(CPP_WAVES, wave_height=1.5, wave_period=6.0, nfrequencies=17, seed=11)
CPP_SURFACE_BODIES, CPP_SUM_BODIES = (0, 2), (1, 2)  # 0-based: a clipped box on body 0, panels on body 2; sum tables on bodies 1 and 2
CPP_NL_BANDS, CPP_MOR_BANDS = ((0.0625, 1.0), (1.5, 6.0)), ((0.0, 0.75), FULL)


def cpp_box():
    """the twelve triangles of the box [-2, 2] x [-1.5, 1.5] x [-3, 4] in the order of tests/cpp/side_terms2_caller.cpp"""
    x, y, z = (-2.0, 2.0), (-1.5, 1.5), (-3.0, 4.0)
    v = (lambda i, j, k: [x[i], y[j], z[k]])
    quads = [(v(0, 0, 0), v(0, 1, 0), v(1, 1, 0), v(1, 0, 0)), (v(0, 0, 1), v(1, 0, 1), v(1, 1, 1), v(0, 1, 1)),
             (v(0, 0, 0), v(1, 0, 0), v(1, 0, 1), v(0, 0, 1)), (v(0, 1, 0), v(0, 1, 1), v(1, 1, 1), v(1, 1, 0)),
             (v(0, 0, 0), v(0, 0, 1), v(0, 1, 1), v(0, 1, 0)), (v(1, 0, 0), v(1, 1, 0), v(1, 1, 1), v(1, 0, 1))]
    return np.array([t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])], dtype=float)


def cpp_sum_table(body, nq, with_q):
    """si.cpp_table on another grid (0.625 + 0.28125 m rad/s)"""
    _, P, Q = si.cpp_table(body, nq, with_q)
    return 0.625 + 0.28125 * np.arange(nq), P, Q


def cpp_lists():
    """si.cpp_lists() with the clipped box in place of body 0's panels, and sum tables on bodies 1 and 2"""
    base = si.cpp_lists()
    return dict(surfaces=[("tris", cpp_box()), None, ("panels", base["panels"][2]), None], elements=base["elements"], tables=base["tables"],
                sums=[None, cpp_sum_table(1, 7, False), cpp_sum_table(2, 9, True), None])
