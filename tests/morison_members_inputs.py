"""The fixed inputs of tests/test_gpu_morison_members_edges.py and tests/test_gpu_morison_members_changes.py (the Morison strip members
at the edges of their launches, and beside the other side terms across wave-model, direction and list changes), shared with
tests/test_morison_members_inputs_cpu.py, which checks on the CPU that every (model, directions, t, state, lists) the GPU tests hold
to tests/morison_members_ref.py keeps that restatement's conditions: every node clear of the free surface by more than the bound of
its own eta error, and the segment cases each test names under need= all met.  It writes no reference mathematics.
TEST INFRASTRUCTURE ONLY.

Shapes (the smallest that cross every edge of the member launches, 256 work items per workgroup):
    EDGE 50:   one body, 50 members, n_seg cycling 1, 2, 3, 5, 4: 300 level-one sum rows (two workgroups), 200 nodes, 300 points
    MANY:      48 bodies, Dloc = 288 level-two sum rows; members on bodies 0, 41, 42, 43, 47 -- bodies 42 and 43 own rows 252..263
    TAILS:     1 member of 1 segment (2 nodes, 2 points, 6 rows); 4 x 63 segments = 256 nodes exactly; 4 x 64 segments = 512 points
               exactly (nodes = segments + members and points = 2 segments: one list cannot have 256 nodes AND 512 points)
    WALK:      si.synth_case(), members on bodies 0 and 2, elements on 1 and 2"""
import numpy as np

import directional_ref as dr
import eta_components_ref as er
import morison_members_ref as mm
import morison_ref as mr
import side_terms_inputs as si
import wave_kinematics_ref as wk
from cases import SPHERE_DT

ALL_CASES = ("wet", "dry", "cut0", "cut1")
G = 9.81
CLEAR = (np.zeros((0, 3)), np.zeros((0, 3)), 1.0, 1.0, 1.0, 1)  # the arguments of set_morison_members that clear a body's list
CLEAR_ELEMENTS = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))


# ---- lists ----
def frame(n_col=5, shift=(0.0, 0.0, 0.0)):
    """frame_members of tests/test_gpu_morison_members.py: a column cut with r0 wet, a column given top down, a tapered brace of one
    segment, a deep brace wholly wet, a member wholly dry, one of zero diameter"""
    r0 = np.array([[0.0, 0.0, -6.0], [1.0, 1.0, 6.5], [-4.0, -3.0, -5.0], [-5.0, 0.5, -8.0], [-2.0, 2.0, 8.0], [2.0, -1.0, -4.0]]) + shift
    r1 = np.array([[0.0, 0.0, 7.0], [1.0, 1.0, -7.0], [4.0, 3.0, 5.5], [5.0, 0.5, -8.5], [2.0, 2.0, 9.0], [2.5, -1.0, 6.0]]) + shift
    dia = [[1.2, 1.2], [0.7, 0.7], [0.9, 0.3], [0.5, 0.6], [0.4, 0.4], [0.0, 0.0]]
    return mm.member_lists(r0, r1, dia, [1.0, 0.8, 1.1, 0.0, 1.0, 1.0], [2.0, 1.5, 0.0, 1.8, 2.0, 2.0], [n_col, 2, 1, 3, 2, 4])


def mixed(n, n_seg, seed):
    """n members in turn bottom up through the surface, top down through it, deep and high: with several segments each, every case"""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 4
    r0 = rng.uniform(-5, 5, (n, 3))
    r1 = r0 + rng.uniform(-4, 4, (n, 3))
    lo, hi = rng.uniform(-9.0, -4.0, n), rng.uniform(4.0, 9.0, n)
    r0[:, 2] = np.choose(kind, [lo, hi, lo, hi])
    r1[:, 2] = np.choose(kind, [hi, lo, lo - 1.5, hi + 1.5])
    return mm.member_lists(r0, r1, rng.uniform(0.2, 1.5, (n, 2)), rng.uniform(0.5, 1.2, n), rng.uniform(0.0, 2.0, n), n_seg)


def counts(ml):
    """(members, nodes, Gauss points) of one list"""
    ns = np.asarray(ml[5])
    return len(ns), int(np.sum(ns + 1)), int(2 * np.sum(ns))


def moving_state(N, rest_z, t, seed=3, dy=0.0):
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((N, 3))
    rest[:, 0] = 15.0 * np.arange(N)
    rest[:, 1] = dy * ((np.arange(N) % 5) - 2.0)
    rest[:, 2] = rest_z
    return PrescribedMotion(N, rest, seed=seed, amplitude=0.5).state(t)


# ---- section C: the edges, on sphere_case() and many_body_case(48) in a 64-component spectral sea ----
EDGE_SEA = dict(simulation_dt=SPHERE_DT, simulation_duration=60.0, ramp_duration=10.0, wave_height=2.0, wave_period=9.0,
                frequency_min=0.03, frequency_max=0.9, nfrequencies=64, seed=3)
EDGE_T = 33.3
EDGE_OPTS = dict(mwl=0.2, wave_stretching=True)
EDGE_HEADING = 0.4
EDGE_N_SEG = np.resize([1, 2, 3, 5, 4], 50)


def edge_lists():
    return [mixed(50, EDGE_N_SEG, 31)]


def edge_state():
    return moving_state(1, -2.0, EDGE_T)


MANY_N, MANY_BODIES, MANY_SHARD = 48, (0, 41, 42, 43, 47), (40, 48)
MANY_KW = dict(S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7)


def many_case(N=MANY_N):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, **MANY_KW)


def many_lists():
    out = [None] * MANY_N
    for i, b in enumerate(MANY_BODIES):
        out[b] = mixed(4 + i, 1 + (np.arange(4 + i) % 3), 40 + i)
    return out


def many_state():
    return moving_state(MANY_N, -2.0, EDGE_T, seed=5)


def tail_lists():
    """name -> (list, need): one body, one list each"""
    one = mm.member_lists([[0.0, 0.0, -6.0]], [[1.0, 0.5, 7.0]], [[1.0, 0.6]], 0.9, 1.7, 1)
    return {"1 member of 1 segment": (one, ("cut0",)), "256 nodes": (mixed(4, 63, 51), ALL_CASES), "512 points": (mixed(4, 64, 52), ALL_CASES)}


def edge_checks():
    """what, case key, directions (None or the uniform heading), lists, bodies evaluated, state, need: everything section C holds to
    the restatement, all at EDGE_T in EDGE_SEA under EDGE_OPTS"""
    yield "50 members", "sphere", None, edge_lists(), edge_state(), ALL_CASES
    yield "48 bodies", "many", None, many_lists(), many_state(), ALL_CASES
    for name, (ml, need) in tail_lists().items():
        for heading in (None, EDGE_HEADING):
            yield f"tails: {name}, heading {heading}", "sphere", heading, [ml], edge_state(), need


def edge_components(src, heading):
    """the five- or four-column components of EDGE_SEA from a context or the CPU oracle that has been given it"""
    comp = wk.irregular_components(src.irreg_spectrum())
    return comp if heading is None else dr.with_directions(comp, heading)


# nodes exactly on the surface (still water, dyadic coordinates): closed forms, no restatement -- compare() refuses these inputs
SURF_D, SURF_CD, SURF_U = 1.25, 0.75, 0.5


def surface_column(n_seg, top_down=False):
    a, b = [0.0, 0.0, -4.0], [0.0, 0.0, 4.0]
    return mm.member_lists([b if top_down else a], [a if top_down else b], SURF_D, SURF_CD, 0.0, n_seg)


def surface_beam(n_seg):
    """horizontal, 8 m long, through the body reference"""
    return mm.member_lists([[-4.0, 0.0, 0.0]], [[4.0, 0.0, 0.0]], SURF_D, SURF_CD, 0.0, n_seg)


# ---- section D: the walk on si.synth_case() ----
MOR_OPTS = si.MOR_OPTS
SEQ_TIMES = si.SEQ_TIMES
WALK_MEMBER_BODIES, WALK_ELEMENT_BODIES = (0, 2), (1, 2)
REC_BAND, REC_BAND_NARROW = (0.04, 1.01), (0.09, 0.51)  # Hz; the record's grid is m / 20 s: bins 1..20 and 2..10
HEADING, SPREAD = 0.4, dict(heading=0.3, s=10, n_bins=15, seed=2)
EXC_DIRS = np.array([-2.0, 2.0])


def walk_lists():
    """members per body; the elements are those of si.sequence_lists()"""
    return [frame(5), None, mixed(6, [8, 3, 1, 5, 2, 4], 61)]


def walk_big():
    """body 0's replacement: more than four times the nodes (the device buffers are reallocated)"""
    return mixed(8, 12, 62)


def walk_one():
    """... and then a single member (stale tails behind it in every buffer)"""
    return mm.member_lists([[0.5, -0.5, -5.0]], [[-0.5, 0.5, 6.0]], [[0.8, 0.5]], 1.0, 1.5, 3)


def walk_stops():
    """dict(name, kind, params, phase, band, dirs, change): si.SEQUENCE with a record's components behind its record and directions
    behind its last entry.  Non-uniform directions need the spectral model (the IRF model refuses them), so the last model is given
    once more in its spectral form before the spread."""
    out = []
    for name, kind, params, phase in si.SEQUENCE:
        change = "phase" if name.startswith("2") else "model"
        out.append(dict(name=name, kind=kind, params=params, phase=phase, band=None, dirs=None, change=change))
        if kind == "eta":
            for nm, band in (("6a record with components", REC_BAND), ("6b a narrower band", REC_BAND_NARROW), ("6c components cleared", None)):
                out.append(dict(name=nm, kind="eta", params=None, phase=phase, band=band, dirs=None, change="band"))
    last = dict(out[-1])
    out.append(dict(last, name="9a uniform heading", dirs=("uniform", HEADING), change="dirs"))
    spec = dict(last, name="10 spectral nf 257", kind="spectral", change="model")
    out.append(spec)
    out.append(dict(spec, name="10a cos-2s spread", dirs=("spread",), change="dirs"))
    out.append(dict(spec, name="10b other directions", dirs=("random", 77), change="dirs"))
    out.append(dict(spec, name="10c directions cleared", dirs=None, change="dirs"))
    return out


def stop_directions(stop, nf):
    d = stop["dirs"]
    if d is None:
        return None
    if d[0] == "uniform":
        return np.full(nf, d[1])
    if d[0] == "spread":
        from hydrochrono_amd.hydro import wave_spreading_directions
        return wave_spreading_directions(nf, **SPREAD)
    return np.random.default_rng(d[1]).uniform(-1.0, 1.0, nf)


def solve_k(w, depth):
    """w^2 = g k tanh(k d) by Newton's iteration from the deep-water value"""
    k = w * w / G
    for _ in range(50):
        th = np.tanh(k * depth)
        k = k - (G * k * th - w * w) / (G * th + G * k * depth * (1.0 - th * th))
    return k


def stop_components(src, stop, depth):
    """(comp, ramp_duration, stretching_applies) of a stop.  src: a context in that state, or the CPU oracle given the stop's model.
    A record's components come from the context (eta_record_components) or, on the CPU, from tests/eta_components_ref.py.  Under a
    record, with or without components, neither the ramp nor the stretching applies (csrc/hc_wave_kin.hip: kin_synthesised is false
    for a record, and kin_ramp is 1 where it is false)."""
    kind = stop["kind"]
    if kind == "eta":
        if stop["band"] is None:
            return None, 0.0, False
        if hasattr(src, "eta_record_components"):
            c = src.eta_record_components()
            comp = (c["A"], 2 * np.pi * c["f"], c["k"], c["phase"])
        else:
            c = er.analyse(si.REC_T, si.REC_ETA, *stop["band"])
            w = 2 * np.pi * c["f"]
            comp = (c["A"], w, solve_k(w, depth), c["phase"])
        rd, stretch = 0.0, False
    else:
        comp, rd, stretch = si.model_components(src, kind, stop["params"], stop["phase"])
    if comp is not None:
        th = stop_directions(stop, comp[0].size)
        if th is not None:
            comp = dr.with_directions(comp, th)
    return comp, rd, stretch


def apply_model(h, stop):
    """the stop's wave model (without its band and directions) on a context or the CPU oracle"""
    kind, params = stop["kind"], stop["params"]
    if kind == "regular":
        h.add_waves_regular(*params)
    elif kind == "irregular" or (kind == "spectral" and not hasattr(h, "set_wave_directions")):
        h.add_waves_irregular(**params)  # (the oracle: the spectral mode synthesises from the same spectrum)
    elif kind == "spectral":
        h.add_waves_irregular(spectral=True, **params)
    elif kind == "eta":
        if hasattr(h, "add_waves_irregular_eta"):
            h.add_waves_irregular_eta(si.REC_T, si.REC_ETA, si.REC_DT)
    elif hasattr(h, "set_wave_directions"):
        h.add_waves_none()


def excitation_headings(case):
    """the bodies' own excitation tables on two headings: what non-uniform directions need of the spectral model"""
    out = []
    for bd in case["bodies"]:
        mag, ph = (np.stack([np.asarray(bd[key]).reshape(6, -1)] * 2, axis=1) for key in ("ex_mag", "ex_phase"))
        out.append((EXC_DIRS, bd["w"], mag, ph))
    return out


def walk_state(t):
    """si.sequence_state with the bodies off the x axis, so that y enters every phase of a directional sea"""
    from hydrochrono_amd.mock_chrono import PrescribedMotion
    rest = np.zeros((3, 3))
    rest[:, 0] = 15.0 * np.arange(3)
    rest[:, 1] = (6.0, -11.0, 2.5)
    rest[:, 2] = -1.0
    return PrescribedMotion(3, rest, seed=3, amplitude=0.5).state(t)


# section 5: the models the list changes are made in, and the lists of every step (body 0, body 2); None: cleared
CHANGE_STOPS = ("3 irregular nf 257", "10a cos-2s spread")
CHANGE_T = SEQ_TIMES[1]


def change_steps():
    """name, members per body, elements set: the list changes of section 5 in order"""
    first = walk_lists()
    return [("first", first, True), ("body 0 four times the nodes", [walk_big(), None, first[2]], True),
            ("body 0 one member", [walk_one(), None, first[2]], True), ("members cleared", [None, None, None], True),
            ("members set again", first, True), ("elements cleared", first, False), ("all cleared", [None, None, None], False)]


# ---- section 7: all terms in flight (s2.compose_lists() on three_body_case(), nonlinear2_inputs.waves(5), s2.COMPOSE_TIMES) ----
def compose_members():
    return [frame(4), None, mixed(5, [6, 2, 1, 3, 4], 71)]


# ---- the references ----
def restate(case, lists, comp, t, state, opts, rd, stretch):
    """mm.members with the options as the context applies them"""
    return mm.members(comp, case["water_depth"], case["rho"], lists, t, *state, mwl=opts["mwl"],
                      stretching=bool(stretch and opts["wave_stretching"]), ramp=mr.ramp_factor(t, rd))


def elements_ref(case, elements, comp, t, state, opts, rd, stretch):
    fn = dr.morison if comp is not None and len(comp) == 5 else mr.morison
    return fn(comp, case["water_depth"], case["rho"], elements, t, *state, mwl=opts["mwl"],
              stretching=bool(stretch and opts["wave_stretching"]), ramp=mr.ramp_factor(t, rd))


def check_conditions(ref, what, need=()):
    assert ref["clear"] and ref["margin"] > ref["eta_bound"], \
        f"{what}: a node is {ref['margin']:.3e} m from the free surface, the eta bound is {ref['eta_bound']:.3e} m (choose other inputs)"
    for c in need:
        assert any(c in s for s in ref["cases"]), (what, c, ref["cases"])
