"""The fixed inputs of tests/test_gpu_side_terms_dir.py (the Morison, nonlinear, drift and sum-frequency terms together in
directional seas, across changes of the directions), shared with tests/test_side_terms_dir_cpu.py, which checks on the CPU that
every (model, directions, time, state) the GPU test holds to a reference keeps the references' conditions.  It builds on
tests/side_terms_inputs.py and tests/side_terms2_inputs.py and writes no reference mathematics: the references are
directional_ref (morison, nonlinear, clipped, heading_tables), qtf_dir_ref (PairSum, bounds) and spectral_ref (the excitation sum on
given tables), with the bounds they derive.  TEST INFRASTRUCTURE ONLY.

Shapes (the surfaces and elements of side_terms2_inputs, the QTF tables on heading grids):
    body 0: 257 clipped triangles, no element,   drift table nh 3 x nq 11 = 33 nodes with Q,    sum table nh 3 x nq 9 = 27 nodes without Q
    body 1: no surface, 7 elements,              no table
    body 2: 5 panels, 300 elements,              drift table nh 4 x nq 8 = 32 nodes without Q,  sum table nh 3 x nq 11 = 33 nodes with Q
J = 33 is two chunks of 32 node rows, the second of one row; J <= 32 one chunk: in one launch of qtf_dir_pair_kernel a workgroup
that returns early runs beside a full one.  Every heading grid spans [BLO, BHI] and holds 0, so that a sea without directions is
the heading-zero sea.  The excitation tables of every body sit on three headings and differ per heading."""
import numpy as np

import directional_ref as dref
import drift_ref as dr
import morison_ref as mr
import qtf_dir_ref as qd
import side_terms2_inputs as s2
import side_terms_inputs as si
import spectral_ref

MIN_GAP, MIN_SPAN, BOUND_RATIO = si.MIN_GAP, s2.MIN_SPAN, s2.BOUND_RATIO
NL_OPTS, MOR_OPTS = si.NL_OPTS, si.MOR_OPTS
BLO, BHI = -1.0, 1.25
EXC_DIRS = np.array([BLO, 0.0, BHI])
NODES = np.array([BLO, BHI, 0.0, -0.375])  # every heading node of every grid: the two ends first
SURFACED = (0, 2)

# ---- sections 1, 2, 4 and 5: three_body_case() (infinite depth) in the spectral model, inside the ramp ----
STEPS, BOUND_STEPS, BOUND_STEP_LARGE = s2.STEPS, s2.BOUND_STEPS, s2.BOUND_STEP_LARGE
COMPOSE_TIMES = s2.COMPOSE_TIMES  # 9.00 .. 9.35 s inside the ramp of 20 s of nonlinear2_inputs.waves()
SUBSET_TIMES = s2.SUBSET_TIMES    # 2.50 .. 2.75 s inside the ramp of 5 s of si.THREE_IRREG


def compose_motion():
    """s2.compose_motion() with the bodies off the x axis, so that y enters every phase"""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((3, 3))
    rest[:, 0] = 15.0 * np.arange(3)
    rest[:, 1] = (-7.5, 4.0, 23.0)
    rest[:, 2] = -0.5
    return PrescribedMotion(3, rest, seed=4, amplitude=0.5)


def sequence_state(t):
    """si.sequence_state with the bodies off the x axis"""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((3, 3))
    rest[:, 0] = 15.0 * np.arange(3)
    rest[:, 1] = (6.0, -11.0, 2.5)
    rest[:, 2] = -1.0
    return PrescribedMotion(3, rest, seed=3, amplitude=0.5).state(t)


def heading_table(beta, nq, seed, lo, hi, with_q, scale=1e4):
    """(beta, Omega, P, Q): the given heading grid, a random frequency grid on [lo, hi] and general tables (no symmetry)"""
    beta = np.asarray(beta, dtype=np.float64)
    _, g, P, Q = qd.random_table(beta.size, nq, seed, beta[0], beta[-1], lo, hi, scale=scale, with_q=with_q)
    return beta, g, P, Q


def qtf_tables(lo, hi, sum_shift):
    """the drift tables on [lo, hi] rad/s, the sum tables on another grid [lo, hi] + sum_shift; see the module docstring"""
    b3, b4 = np.array([BLO, 0.0, BHI]), np.array([BLO, -0.375, 0.0, BHI])
    slo, shi = lo + sum_shift[0], hi + sum_shift[1]
    return dict(tables=[heading_table(b3, 11, 170, lo, hi, True), None, heading_table(b4, 8, 172, lo + 0.1, hi - 0.2, False)],
                sums=[heading_table(b3, 9, 180, slo, shi, False), None, heading_table(b3, 11, 182, slo + 0.1, shi - 0.2, True)])


def make_lists(base, lo, hi, sum_shift):
    out = dict(surfaces=base["surfaces"], elements=base["elements"])
    out.update(qtf_tables(lo, hi, sum_shift))
    return out


def compose_lists(small=False):
    """sections 1, 2, 4 and 5: the surfaces and elements of s2.compose_lists, the QTF grids on the same frequencies"""
    return make_lists(s2.compose_lists(small=small), 0.7, 2.3, (-0.05, -0.25))


def sequence_lists():
    """section 3: the surfaces and elements of s2.sequence_lists, grids that hold both regular waves"""
    return make_lists(s2.sequence_lists(), 0.5, 3.5, (-0.05, 0.1))


def narrow(table):
    """the table with its last heading one ulp below BHI: a component on BHI is then one ulp past the heading grid"""
    beta, g, P, Q = table
    b = beta.copy()
    b[-1] = np.nextafter(b[-1], -np.inf)
    return b, g, P, Q


def one_heading(table):
    """(Omega, P, Q) of hc_set_sum_qtf / hc_set_drift_qtf from the node at heading 0 of a heading table"""
    beta, g, P, Q = table
    j = int(np.nonzero(beta == 0.0)[0][0])
    return g, P[:, j, j], None if Q is None else Q[:, j, j]


# ---- the excitation tables on a heading grid ----
def excitation_headings(case):
    """per body (dirs, w, mag [6][3][nw], phase [6][3][nw]): the body's own table scaled and shifted per heading (another factor
    at every heading, both grid ends included), as heading_tables_for of tests/test_gpu_directional.py"""
    out = []
    for b, bd in enumerate(case["bodies"]):
        rng = np.random.default_rng(800 + b)
        w = np.asarray(bd["w"], dtype=np.float64)
        mag0, ph0 = np.asarray(bd["ex_mag"]).reshape(6, -1), np.asarray(bd["ex_phase"]).reshape(6, -1)
        mag = np.stack([mag0 * f for f in rng.uniform(0.5, 1.5, EXC_DIRS.size)], axis=1)
        ph = np.stack([ph0 + d for d in rng.uniform(-1.0, 1.0, EXC_DIRS.size)], axis=1)
        out.append((EXC_DIRS, w, mag, ph))
    return out


def set_excitation_headings(h, case, only=None):
    for b, tb in enumerate(excitation_headings(case)):
        if only is None or b in only:
            h.set_body_excitation_rao_headings(b, *tb)


# ---- the directions ----
SPREAD = dict(heading=0.125, s=8.0, n_bins=15, seed=2)


def node_stride(nf):
    return 7 if nf > 20 else 2


def directions(nf, which):
    """"A": the equal-energy spread of SPREAD with every seventh component (every second of a few) moved onto a heading node, both
    grid ends among them;
    "B": a second draw; a number: the uniform heading; "zero": all zeros; None: none"""
    if which is None:
        return None
    if which == "A":
        from hydrochrono_amd.hydro import wave_spreading_directions
        th = wave_spreading_directions(nf, **SPREAD)
        k = node_stride(nf)
        th[::k] = NODES[np.arange(th[::k].size) % NODES.size]
        return th
    if which == "B":
        return np.random.default_rng(77).uniform(BLO + 0.05, BHI - 0.05, nf)
    if which == "zero":
        return np.zeros(nf)
    return np.full(nf, float(which))


# ---- the lists on a context ----
def set_lists(h, lists, which=("surfaces", "elements", "tables", "sums")):
    """on a HydroForces or a HydroGroup"""
    s2.set_lists(h, lists, tuple(k for k in which if k in ("surfaces", "elements")))
    for b in range(3):
        if "tables" in which and lists["tables"][b] is not None:
            beta, g, P, Q = lists["tables"][b]
            h.set_drift_qtf(b, g, P, Q, headings=beta)
        if "sums" in which and lists["sums"][b] is not None:
            beta, g, P, Q = lists["sums"][b]
            h.set_sum_qtf(b, g, P, Q, headings=beta)


def clear_lists(h, which):
    s2.clear_lists(h, which)


def prepare(h, case, lists, phase=0.0):
    """heading tables of the excitation, lists, tables and options; the modes and the wave model are the caller's"""
    set_excitation_headings(h, case)
    set_lists(h, lists)
    h.set_nonlinear_options(regular_phase=phase, **NL_OPTS)
    h.set_morison_options(regular_phase=phase, **MOR_OPTS)
    h.set_drift_options(regular_phase=phase)
    h.set_sum_options(regular_phase=phase)


# ---- section 3: the walk on si.synth_case() (depth 60: long-wave, intermediate and k d > 500 components) ----
SEQ_PHASE, SEQ_TIMES = si.SEQ_PHASE, si.SEQ_TIMES
KIN, QTF3, ALL = ("nl", "mor"), ("dft3", "sum"), ("nl", "mor", "dft1", "dft3", "sum", "exc")
# name, kind, parameters, directions, what changed against the entry before, the terms that must have moved, those that must not
WALK = [
    ("1 regular, heading 0.4", "regular", si.REG1, 0.4, None, (), ()),
    ("2 the same wave, directions cleared", "regular", si.REG1, None, "directions", KIN + QTF3 + ("exc",), ()),
    ("3 spectral nf 257, spread A", "spectral", si.irreg(257), "A", "model", ALL, ()),
    ("4 spread B", "spectral", si.irreg(257), "B", "directions", KIN + QTF3 + ("exc",), ()),
    ("5 uniform 0.3", "spectral", si.irreg(257), 0.3, "directions", KIN + QTF3 + ("exc",), ()),
    ("6 all zeros", "spectral", si.irreg(257), "zero", "directions", KIN + QTF3 + ("exc",), ()),
    ("7 directions cleared", "spectral", si.irreg(257), None, "zero to none", ("exc",), ("dft1", "dft3", "sum")),
    ("8 spectral nf 5, a spread", "spectral", si.irreg(5), "A", "model", ALL, ()),
    ("9 the IRF model nf 257, uniform 0.3", "irregular", si.irreg(257), 0.3, "model", ALL, ()),
    ("10 eta record", "eta", None, None, "model", ALL, ()),
    ("11 entry 3 again", "spectral", si.irreg(257), "A", "model", ALL, ()),
]
HELD = (0, 2, 4, 6, 7)  # entries 1, 3, 5, 7 and 8: every term and the excitation held to the references (7: the bound of 3 (e))
HELD_TERMS = (8,)     # entry 9: the terms only


def components(h_or_oracle, kind, params, which, phase=SEQ_PHASE):
    """((A, w, k, phi, theta), ramp_duration, stretching_applies) of a model under directions `which`; None without components"""
    comp, rd, stretch = si.model_components(h_or_oracle, kind, params, phase)
    if comp is None:
        return None, rd, stretch
    nf = comp[0].size
    th = directions(nf, which)
    return dref.with_directions(comp, 0.0 if th is None else th), rd, stretch


# ---- the references, with the conditions they need ----
def references(case, g, lists, comp, rd, stretch, t, state, drift_modes=(3,)):
    """Every term's reference at one state under the five-column components `comp`: dict(nl=dict(buoy, fk, bound_buoy, bound_fk
    [N][6], margin, cut_span, cases [4], wet_panels), mor=directional_ref.morison result, dft={mode: rows}, sum=rows), a row None
    for a body without a table, else (F [6], bound [6])."""
    pos, rpy, lin, ang = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in state)
    ramp = mr.ramp_factor(t, rd)
    depth, rho = case["water_depth"], case["rho"]
    tris = [l[1] if l is not None and l[0] == "tris" else None for l in lists["surfaces"]]
    pans = [l[1] if l is not None and l[0] == "panels" else None for l in lists["surfaces"]]
    kw = dict(mwl=NL_OPTS["mwl"], stretching=stretch and NL_OPTS["wave_stretching"], ramp=ramp)
    rc = dref.clipped(comp, depth, rho, g, tris, t, pos, rpy, **kw)
    rp = dref.nonlinear(comp, depth, rho, g, pans, t, pos, rpy, **kw)
    nl = {k: rc[k] + rp[k] for k in ("buoy", "fk", "bound_buoy", "bound_fk")}  # a body carries one kind of list: the other's rows are zero
    nl.update(margin=rp["margin"], cut_span=rc["cut_span"], cases=np.asarray(rc["cases"][0]), wet_panels=rp["wet"][2])
    mor = dref.morison(comp, depth, rho, lists["elements"], t, pos, rpy, lin, ang, mwl=MOR_OPTS["mwl"],
                       stretching=stretch and MOR_OPTS["wave_stretching"], ramp=ramp)
    out = dict(nl=nl, mor=mor)
    out.update(qtf_references(lists, comp, rd, t, pos, drift_modes))
    return out


def qtf_references(lists, comp, rd, t, pos, drift_modes=(3,)):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    ramp = mr.ramp_factor(t, rd)
    rows = {}
    for key in ("tables", "sums"):
        rows[key] = []
        for b, tb in enumerate(lists[key]):
            if tb is None:
                rows[key].append(None)
            else:
                rows[key].append((qd.PairSum(comp, tb).force(t, pos[b, 0], pos[b, 1], ramp=ramp), qd.bounds(comp, tb, ramp=ramp)))
    dft = {m: [None if r is None else (r[0][m], r[1][m]) for r in rows["tables"]] for m in drift_modes}
    return dict(dft=dft, sum=[None if r is None else (r[0]["sum"], r[1]["sum"]) for r in rows["sums"]])


def excitation_reference(case, spec, theta, rd, times):
    """(F [T][6N] longdouble, bound [T][6N]) of the spectral excitation under directions theta [nf] (None: the bodies' own
    {6,1,nw} tables): spectral_ref's sum and bound on the tables directional_ref.heading_tables interpolates"""
    tab = spectral_ref.tables(case, spec)
    if theta is not None:
        rg = case["rho"] * case["g"]
        X, P = [], []
        for dirs, w, mag, ph in excitation_headings(case):
            m, p = dref.heading_tables(dirs, w, mag * rg, ph, tab["omega"], theta)
            X.append(np.asarray(m, dtype=np.float64))
            P.append(np.asarray(p, dtype=np.float64))
        tab = dict(tab, X=np.concatenate(X), P=np.concatenate(P))
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    return spectral_ref.forces(tab, float(rd), times), spectral_ref.bound(tab, times)


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
    cases = nl["cases"]
    n_tri = len(lists["surfaces"][0][1])
    assert cases.sum() == n_tri and cases[0] < n_tri and cases[3] < n_tri, (what, "triangles", cases.tolist())
    wet = nl["wet_panels"]
    assert wet.size == len(lists["surfaces"][2][1][0]) and 0 < wet.sum() < wet.size, (what, "panels", int(wet.sum()), wet.size)
    for name, val, bound in (("buoy", nl["buoy"], nl["bound_buoy"]), ("fk", nl["fk"], nl["bound_fk"]), ("morison", mor["F"], mor["bound"])):
        s2.check_bound(name, val, bound, what)
    return cases


check_qtf_conditions = s2.check_qtf_conditions


def check_grids(comp, lists, what, regular=False):
    """Of more than 20 components more than 10 lie inside every QTF frequency grid and more than 10 outside (of fewer: at least one
    on either side; a regular wave: inside), and every direction of a component inside a frequency grid lies inside that table's
    heading grid; some of them sit on a heading node."""
    nf = comp[1].size
    for key in ("tables", "sums"):
        for b, tb in enumerate(lists[key]):
            if tb is None:
                continue
            inside = dr.cells(tb[1], comp[1])[0]
            if regular:
                assert inside.all(), (what, key, b)
            elif nf > 20:
                assert 10 < inside.sum() < nf - 10, (what, key, b, int(inside.sum()), nf)
            else:
                assert 0 < inside.sum() < nf, (what, key, b, int(inside.sum()), nf)
            ok = qd.head_cells(tb[0], comp[4])[3]
            assert ok[inside].all(), (what, key, b, "a direction outside the heading grid")
            assert tb[0][0] == BLO and tb[0][-1] == BHI and np.any(tb[0] == 0.0), (what, key, b)
    assert np.all((comp[4] >= EXC_DIRS[0]) & (comp[4] <= EXC_DIRS[-1])), (what, "excitation heading grid")


# ---- section 6: what tests/cpp/side_terms_dir_caller.cpp builds (dyadic values: the same bits in both languages) ----
CPP_STEPS, CPP_SWITCH, CPP_REGULAR = 24, 6, 12  # irregular waves to step 11, a regular wave from step 12; the heading changes at 6 and 18
CPP_WAVES = dict(s2.CPP_WAVES)
CPP_REG = (0.25, 0.75)          # amplitude, omega of the regular wave (inside the frequency list of four_body.h5)
CPP_HEADINGS = (0.25, -0.5)     # before and after a switch (uniform: the C++ mirror's IrregularWaves is the IRF model)
CPP_BETA = np.array([-0.75, 0.0, 0.5])
CPP_EXC_DIRS = np.array([-1.0, 0.0, 1.0])
CPP_SURFACE_BODIES = s2.CPP_SURFACE_BODIES


def cpp_heading_table(body, nq, with_q, sum_grid):
    """(beta, Omega, P [6][3][3][nq][nq], Q): si.cpp_table with a heading dependence"""
    omega = (0.625 + 0.28125 * np.arange(nq)) if sum_grid else (0.75 + 0.3125 * np.arange(nq))
    d, a, b, m, n = np.meshgrid(np.arange(6.0), np.arange(3.0), np.arange(3.0), np.arange(float(nq)), np.arange(float(nq)), indexing="ij")
    P = 1000.0 * (d + 1) + 250.0 * m - 125.0 * n + 31.25 * body + 500.0 * a - 375.0 * b
    Q = 500.0 * (m - n) + 62.5 * d + 93.75 * (a - b)
    return CPP_BETA, omega, P, (Q if with_q else None)


def cpp_lists():
    """s2.cpp_lists() with the tables on heading grids (drift on bodies 0 and 3, sum on bodies 1 and 2)"""
    base = s2.cpp_lists()
    return dict(surfaces=base["surfaces"], elements=base["elements"],
                tables=[cpp_heading_table(0, 9, True, False), None, None, cpp_heading_table(3, 5, False, False)],
                sums=[None, cpp_heading_table(1, 7, False, True), cpp_heading_table(2, 9, True, True), None])


def cpp_excitation_headings(body):
    """body's {6, 3, 16} excitation tables on w = 0.25 (j + 1): dyadic values, another table at every heading"""
    w = 0.25 * (np.arange(16) + 1.0)
    r, d, j = np.meshgrid(np.arange(6.0), np.arange(3.0), np.arange(16.0), indexing="ij")
    mag = 0.5 + 0.125 * r + 0.25 * d + 0.0625 * j + 0.03125 * body
    ph = 0.25 * r - 0.5 * d + 0.125 * j
    return CPP_EXC_DIRS, w, mag, ph
