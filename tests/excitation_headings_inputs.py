"""The fixed inputs of tests/test_gpu_excitation_headings.py (the first-order excitation on heading grids across bodies, shards and
step paths), shared with tests/test_excitation_headings_cpu.py, which checks on the CPU that every state held to a
reference meets the conditions that keep the comparison from being vacuous.  No reference mathematics is written here: the
interpolation is directional_ref.heading_tables, the force and its bound spectral_ref.forces / spectral_ref.bound on those tables.
TEST INFRASTRUCTURE ONLY.

Bodies are those of hydrochrono_amd.synthetic.many_body_case (rao_w of 64 entries).  A LAYOUT gives every body a heading grid of its
own or none:
    G1 one node (0.3), G2 two nodes, G3 three, G5 five unevenly spaced ones (0.0 and 0.3 among them), H5 five others;
    a grid's tables sit on a frequency list of their own length (64, 23 or 40: 23 and 40 differ from the body's rao_w).
"uniform" layouts leave bodies without tables and use G1 (valid on its node only: every uniform heading here is 0.3); "spread"
layouts give every body a grid of two nodes or more, as non-uniform directions need."""
import numpy as np

import directional_ref as dref
import spectral_ref as sr

GRIDS = dict(G1=np.array([0.3]), G2=np.array([-0.5, 0.9]), G3=np.array([-0.6, 0.1, 1.0]), G5=np.array([-1.0, -0.75, 0.0, 0.3, 1.25]),
             H5=np.array([-0.5, -0.45, 0.2, 0.3, 0.9]))
LO, HI = -0.5, 0.9          # the intersection of every grid of a spread layout
UNIFORM_HEADING = 0.3       # on the node of G1, on a node of G5 and H5, inside an interval of G2 and G3
LAYOUTS = {
    ("uniform", 3): [("G1", 64), None, ("G5", 23)],
    ("spread", 3): [("G2", 64), ("G5", 23), ("G3", 40)],
    # two shards own bodies [0, 3) and [3, 5): every body of the first has tables, none of the second; three shards own [0, 2), [2, 4)
    # and [4, 5): with, mixed, without
    ("uniform", 5): [("G1", 64), ("G2", 40), ("G5", 23), None, None],
    ("spread", 5): [("G2", 64), ("G5", 23), ("G3", 40), ("H5", 64), ("G2", 23)],
    # regular wave: body 0 (whose phases serve every body) has none and sits on the first shard, the bodies with tables on the last
    ("regular", 5): [None, None, None, ("G5", 23), ("G2", 40)],
}
STEP_S, STEP_DT = sr.STEP_S, sr.STEP_DT
RAMP = 2.5
KW = dict(sr.BASE_KW, nfrequencies=12, ramp_duration=RAMP, frequency_min=0.03, frequency_max=0.3, seed=3)
KW_TILE = dict(KW, nfrequencies=257)                      # one component past the tile of 256
KW_SECOND = dict(KW, seed=9, wave_height=1.4, wave_period=6.0)  # what change (e) of the walk sets
KW_NO_RAMP = dict(KW, ramp_duration=0.0)
# before the ramp ends, after it, large; with KW_NO_RAMP: no ramp (t <= 0 included)
TIMES = np.array([0.731, 2.4999, 7.3, 1.0e4 + 0.37])
TIMES_NO_RAMP = np.array([-1.0, 0.0, 3.3])
REG_AMP, REG_OMEGA, REG_HEADING = 0.4, 1.3, 0.2   # 0.2: inside an interval of G5 and of G2
REG_TIMES = np.array([0.0, 2.2, 1.0e4 + 0.37])
# case 5, one body: a grid whose first node is 0.0, unevenly spaced; a one-node grid; two headings whose phases differ by more than pi
EDGE_GRID = np.array([0.0, 0.4, 1.0, 1.7])
EDGE_TIMES = np.array([0.0, 3.3, 17.1])
WIDE_N, WIDE_S, WIDE_STEPS = sr.WIDE_N, sr.WIDE_S, 3


def build_case(N, S=None):
    """S: the IRF length (the excitation tables do not depend on it: the CPU checks build short ones)"""
    from hydrochrono_amd.synthetic import many_body_case
    S = S or (WIDE_S if N == WIDE_N else STEP_S)
    return many_body_case(N, S=S, dt_rirf=0.01, n_exc=17, dt_exc=0.05, nw=64, seed=7600 + N)


def wide_layout():
    """every third body without tables, the others on G2, G5 and G3 in turn"""
    pick = [("G2", 64), None, ("G5", 23), ("G3", 40)]
    return [pick[b % 4] for b in range(WIDE_N)]


def grid_tables(dirs, nw, seed):
    """(dirs, w [nw], mag [6][n_dir][nw], phase [6][n_dir][nw]): independent draws at every heading, so that a wrong weight, a
    swapped bracket or a neighbour's table moves the force by its own size; w uniform from its spacing up to 3.2 rad/s, the rule
    of the library's interpolator"""
    rng = np.random.default_rng(seed)
    dirs = np.asarray(dirs, dtype=np.float64)
    w = np.linspace(3.2 / nw, 3.2, nw)
    return dirs, w, rng.uniform(0.1, 2.0, size=(6, dirs.size, nw)), rng.uniform(-np.pi, np.pi, size=(6, dirs.size, nw))


def layout_tables(layout, seed=0):
    """per body None or the tables of its grid"""
    return [None if e is None else grid_tables(GRIDS[e[0]], e[1], 900 + 17 * b + seed) for b, e in enumerate(layout)]


def tables_of(kind, N, seed=0):
    return layout_tables(wide_layout() if N == WIDE_N else LAYOUTS[(kind, N)], seed)


def apply_tables(h, tables, only=None):
    """on a HydroForces or a HydroGroup"""
    for b, tb in enumerate(tables):
        if tb is not None and (only is None or b in only):
            h.set_body_excitation_rao_headings(b, *tb)


def directions(nf, which):
    """"A": a draw over [LO, HI] with every third component on a node of some grid, both ends of the narrowest among them;
    "B": another draw, no node; a number: the uniform heading; None: none"""
    if which is None:
        return None
    if which == "A":
        th = np.random.default_rng(41).uniform(LO, HI, nf)
        nodes = np.array([LO, HI, 0.0, 0.3, 0.1, 0.2, -0.45])
        th[::3] = nodes[np.arange(th[::3].size) % nodes.size]
        return th
    if which == "B":
        return np.random.default_rng(43).uniform(LO + 0.01, HI - 0.01, nf)
    return np.full(nf, float(which))


def nearest_node(dirs, theta):
    dirs = np.asarray(dirs, dtype=np.float64)
    return dirs[np.argmin(np.abs(np.asarray(theta)[:, None] - dirs[None, :]), axis=1)]


def heading_tab(case, spec_or_tab, tables, theta, per_body_theta=None):
    """spectral_ref.tables with the rows of every body that has heading tables replaced by directional_ref.heading_tables at theta
    (None: no directions, every body keeps its {6,1,nw} table).  per_body_theta(b, dirs): the directions of body b instead."""
    tab = spec_or_tab if "omega" in spec_or_tab else sr.tables(case, spec_or_tab)
    if theta is None:
        return tab
    rg = case["rho"] * case["g"]
    X, P = tab["X"].copy(), tab["P"].copy()
    for b, tb in enumerate(tables):
        if tb is None:
            continue
        dirs, w, mag, ph = tb
        th = theta if per_body_theta is None else per_body_theta(b, dirs)
        m, p = dref.heading_tables(dirs, w, mag * rg, ph, tab["omega"], th)
        X[6 * b:6 * b + 6], P[6 * b:6 * b + 6] = np.asarray(m, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return dict(tab, X=X, P=P)


def reference(case, spec, tables, theta, ramp_duration, times):
    """(F [T][6N] longdouble, B [T][6N])"""
    tab = heading_tab(case, spec, tables, theta)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    return sr.forces(tab, float(ramp_duration), times), sr.bound(tab, times)


def regular_tab(case, tables, theta, amp=REG_AMP, omega=REG_OMEGA):
    """the table of the one component of a regular wave: |m| A cos(w t + phi), every body's magnitudes from its own tables (heading
    tables under a direction, else its {6,1,nw} table), the phases from body 0 alone (the reference project indexes the phase by
    the degree of freedom only)"""
    N, om, rg = case["N"], np.array([float(omega)]), case["rho"] * case["g"]
    rows = [sr.rao_at(bd["w"], np.asarray(bd["ex_mag"], dtype=np.float64).reshape(6, -1) * rg, bd["ex_phase"], om) for bd in case["bodies"]]
    tab = dict(omega=om, amp=np.array([float(amp)]), phi=np.zeros(1), X=np.concatenate([r[0] for r in rows]), P=np.concatenate([r[1] for r in rows]))
    tab = heading_tab(case, tab, tables, None if theta is None else np.array([float(theta)]))
    return dict(tab, P=np.tile(tab["P"][:6], (N, 1)), P_all=tab["P"])


def regular_reference(case, tables, theta, times, **kw):
    tab = regular_tab(case, tables, theta, **kw)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    return sr.forces(tab, 0.0, times), sr.bound(tab, times)


# ---- the conditions of a held state (tests/test_excitation_headings_cpu.py; asserted again on the GPU on the context's spectrum) ----
MIN_SIGNAL, MIN_MOVE = 1e6, 1e3


def check_signal(F, B, what):
    """for every body and time the largest |reference force| of its six rows is at least MIN_SIGNAL times that row's bound"""
    F, B = np.abs(np.asarray(F, dtype=np.float64)), np.asarray(B)
    T, D = F.shape
    Fb, Bb = F.reshape(T, D // 6, 6), B.reshape(T, D // 6, 6)
    r = np.argmax(Fb, axis=2)[..., None]
    big, bnd = np.take_along_axis(Fb, r, 2)[..., 0], np.take_along_axis(Bb, r, 2)[..., 0]
    ok = big >= MIN_SIGNAL * bnd
    assert np.all(ok) and np.all(big > 0.0), (what, "time, body", np.argwhere(~ok).tolist()[:4], float(np.min(big / np.maximum(bnd, 1e-300))))
    return float(np.min(big / np.maximum(bnd, 1e-300)))


def check_moves(case, spec, tables, theta, ramp_duration, times, what):
    """under non-uniform directions: in some row of every body the reference differs from the one with every direction moved onto
    the nearest node of that body's grid by at least MIN_MOVE times the bound"""
    assert all(tb is not None for tb in tables), what
    F, B = reference(case, spec, tables, theta, ramp_duration, times)
    tab = heading_tab(case, spec, tables, theta, per_body_theta=lambda b, dirs: nearest_node(dirs, theta))
    Fn = sr.forces(tab, float(ramp_duration), np.asarray(times, dtype=np.float64))
    T, D = B.shape
    ratio = (np.abs(F - Fn).astype(np.float64) / B).reshape(T, D // 6, 6).max(axis=2)
    assert np.all(ratio >= MIN_MOVE), (what, "time, body", np.argwhere(ratio < MIN_MOVE).tolist()[:4], float(ratio.min()))
    return float(ratio.min())


def edge_tables(kind):
    if kind == "grid":
        return [grid_tables(EDGE_GRID, 23, 990)]
    if kind == "one":
        return [grid_tables(GRIDS["G1"], 40, 991)]
    dirs, w, mag, ph = grid_tables(GRIDS["G2"], 23, 992)  # "jump": phases near -3 at one heading, near +3 at the other
    ph[:, 0], ph[:, 1] = -3.0 + 0.1 * ph[:, 0] / np.pi, 3.0 + 0.1 * ph[:, 1] / np.pi
    return [(dirs, w, mag, ph)]


def edge_states():
    """(name, tables, theta) of the accepted directions of case 5 that are held to the reference"""
    g = EDGE_GRID
    return [("one ulp inside the first node", edge_tables("grid"), float(np.nextafter(g[0], 1.0))),
            ("one ulp inside the last node", edge_tables("grid"), float(np.nextafter(g[-1], 0.0))),
            ("between uneven nodes", edge_tables("grid"), 0.9),
            ("the one-node grid on its node", edge_tables("one"), float(GRIDS["G1"][0])),
            ("phases more than pi apart", edge_tables("jump"), 0.2)]


# ---- the states held to the reference ----
def step_count(lookahead):
    return 2 * lookahead + 3 if lookahead else 8


def step_times(n, t0=2.0):
    """on the step grid, past one IRF window of a pre-filled history; the first half second inside the ramp"""
    return t0 + STEP_DT * np.arange(n)


# the walk of case 3: name, what the change does, the state after it (layout seed of body 1's tables, wave parameters, directions)
WALK = [
    ("start: tables, no directions", None, 0, KW, None),
    ("(a) non-uniform directions A", "directions", 0, KW, "A"),
    ("(b) directions B", "directions", 0, KW, "B"),
    ("(c) body 1's tables replaced under B", "tables", 5, KW, "B"),
    ("(d) directions cleared", "directions", 5, KW, None),
    ("(e) a wave setter, then directions A", "model", 5, KW_SECOND, "A"),
]


def walk_tables(N, seed1):
    """the spread layout with body 1's tables drawn from another seed where seed1 != 0"""
    tables = tables_of("spread", N)
    if seed1:
        tables[1] = layout_tables(LAYOUTS[("spread", N)], seed1)[1]
    return tables


def walk_segments(lookahead):
    """steps before every change: each change falls inside a block and is followed by more than one block"""
    L = max(lookahead, 16)
    return [L + 5, L + 7, L + 3, L + 9, L + 4, L + 6]


def held_states():
    """(name, N, tables, wave parameters, theta builder nf -> theta, times): every (state, time) a GPU test holds to the reference,
    the steps of the step-path, walk and shard tests included"""
    out = []
    for N in (3, 5):
        for kw, tag in ((KW, "nf12"), (KW_TILE, "nf257")):
            if N == 5 and tag == "nf257":
                continue
            for kind, which in (("uniform", UNIFORM_HEADING), ("spread", "A"), ("spread", "B")):
                out.append((f"N{N} {tag} {kind} {which}", N, tables_of(kind, N), kw, which, TIMES))
                out.append((f"N{N} {tag} {kind} {which} no ramp", N, tables_of(kind, N), dict(kw, ramp_duration=0.0), which, TIMES_NO_RAMP))
    for kind, which in (("uniform", UNIFORM_HEADING), ("spread", "A")):
        out.append((f"steps N3 {kind}", 3, tables_of(kind, 3), KW, which, step_times(step_count(32))))
    for N, la in ((3, 16), (3, 32), (5, 32)):
        k = 0
        for (name, _, seed1, kw, which), n in zip(WALK, walk_segments(la)):
            out.append((f"walk N{N} la{la} {name}", N, walk_tables(N, seed1), kw, which, step_times(n, 2.0 + STEP_DT * k)))
            k += n
    for name, tables, theta in edge_states():
        out.append((f"edge {name}", 1, tables, KW_NO_RAMP, theta, EDGE_TIMES))
    out.append(("shards N5 uniform", 5, tables_of("uniform", 5), KW, UNIFORM_HEADING, step_times(12)))
    out.append(("wide", WIDE_N, tables_of("spread", WIDE_N), KW, UNIFORM_HEADING, step_times(WIDE_STEPS, 1.0)))
    return out
