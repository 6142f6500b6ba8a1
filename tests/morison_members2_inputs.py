"""The fixed inputs of tests/test_gpu_morison_members2.py and tests/test_gpu_morison_members2_dir.py (the Morison strip members on the
second-order sea), shared with tests/test_morison_members2_ref_cpu.py, which checks on the CPU oracle's spectrum the conditions the
GPU tests rely on: every node of every case clear of the free surface of eta1 + eta2 by more than the bound of its own error, every
segment case met, and the node built to flip really flipping in the restatement.  It writes no reference mathematics.
TEST INFRASTRUCTURE ONLY.

Shapes (the smallest at which the kernels can go wrong):
    components  3 (a part-filled tile of the pair sum) and 257 (the pair sum crosses a tile edge: kKinTile = 256)
    depth       40 m with the 3 components, infinite with the 257
    bodies      three; body 1 carries no member (and, in the mixed tests, elements)
    members     a vertical surface-piercing column of 4 segments; an inclined tapered brace cut inside a segment; the same brace
                reversed (r0 above r1: the other cut branch); a submerged horizontal pontoon; a wholly dry member; n_seg 1; and, with
                the 3 components, n_seg 64 once
"""
import functools

import numpy as np

import directional_ref as dr
import morison_members2_ref as m2
import morison_members_ref as mm
import morison_ref as mr
import wave2_dir_inputs as di
import wave2_inputs as wi
import wave_kinematics_ref as wk
from cases import three_body_case
from morison2_dir_inputs import spread_sea  # noqa: F401  (the spectral model a spread sea needs)
from morison_members_inputs import moving_state

INF = float("inf")
FULL = (0.0, INF)
ALL_CASES = ("wet", "dry", "cut0", "cut1")
MWL = 0.15
REST_Z = -1.0


def finite_case():
    return dict(three_body_case(), water_depth=40.0)


def body0():
    """column, brace, brace reversed"""
    r0 = [[0.0, 0.0, -7.0], [-4.0, -3.0, -5.0], [4.5, 3.0, 4.5]]
    r1 = [[0.0, 0.0, 6.0], [4.0, 3.0, 4.5], [-3.5, -3.0, -5.0]]
    return mm.member_lists(r0, r1, [[1.2, 1.2], [0.9, 0.3], [0.3, 0.9]], [1.0, 1.1, 1.1], [2.0, 1.6, 1.6], [4, 3, 3])


def body2(with_64):
    """pontoon, a dry member, one segment through the surface, and 64 segments through it"""
    r0 = [[-5.0, 0.5, -7.0], [-2.0, 2.0, 8.0], [2.0, -1.0, -4.0], [1.0, 1.0, -9.0]]
    r1 = [[5.0, 0.5, -7.5], [2.0, 2.0, 9.0], [2.5, -1.0, 6.0], [1.5, 2.0, 7.0]]
    n = 4 if with_64 else 3
    return mm.member_lists(r0[:n], r1[:n], [[0.5, 0.6], [0.4, 0.4], [0.8, 0.5], [0.7, 0.7]][:n], [0.9, 1.0, 1.0, 0.8][:n],
                           [1.8, 2.0, 1.5, 2.0][:n], [2, 2, 1, 64][:n])


# name -> dict(case, waves, lists, t, stretching, bands); the directional tests run the same sets on di.spread directions
SETS = {
    "nf3_40m": dict(case=finite_case, waves=wi.three_waves(3), lists=lambda: [body0(), None, body2(True)], t=12.5, stretching=True,
                    diff_band=FULL, sum_band=FULL),
    "nf257_deep": dict(case=three_body_case, waves=wi.three_waves(257), lists=lambda: [body0(), None, body2(False)], t=33.3, stretching=False,
                       diff_band=(0.0, 1.5), sum_band=(0.5, 6.0)),
}
# the bichromatic sea of the waterline tests: two components 0.02 Hz apart, a group of 50 s
BICHROMATIC = dict(wi.three_waves(2), frequency_min=0.10, frequency_max=0.12, wave_height=3.0)
BICHROMATIC_T = 31.0
BICHROMATIC_BANDS = dict(diff_band=FULL, sum_band=wi.NO_PAIR)  # the difference band alone: eta2 is the set-down of the group


def bichromatic_inputs():
    """(lists, state): a fixed upright column of 8 segments from -8 m to 6 m on body 0 at x = 0, in finite_case()"""
    lists = [mm.member_lists([[0.0, 0.0, -8.0]], [[0.0, 0.0, 6.0]], 1.5, 1.0, 2.0, 8), None, None]
    pos = np.zeros((3, 3))
    pos[:, 0] = (0.0, 40.0, 80.0)
    z9 = np.zeros((3, 3))
    return lists, (pos, z9, z9, z9)


def bichromatic_reference(comp, g, case):
    """(order 2, order 1, expected sign of the set-down) from the restatements, with the conditions the GPU test relies on:
    every node clear of the surface with one cut segment, the set-down of one sign at every node and above 1e-5 m, and a change of
    F_x above 100 times the two bounds together."""
    lists, st = bichromatic_inputs()
    depth, rd = case["water_depth"], BICHROMATIC["ramp_duration"]
    ref = m2.members2(comp, g, depth, case["rho"], lists, BICHROMATIC_T, *st, mwl=0.0, ramp_duration=rd, **BICHROMATIC_BANDS)
    first = mm.members(comp, depth, case["rho"], lists, BICHROMATIC_T, *st, mwl=0.0)
    check_conditions(ref, "bichromatic", need=("cut0",))
    check_conditions(first, "bichromatic at order 1", need=("cut0",))
    set_down = ref["node_eta2"][0]
    expected = np.sign(set_down[0])
    assert expected != 0 and np.all(np.sign(set_down) == expected) and np.abs(set_down).min() > 1e-5, set_down
    want = ref["F"][0, 0] - first["F"][0, 0]
    assert abs(want) > 100 * (ref["bound"][0, 0] + first["bound"][0, 0]), (want, ref["bound"][0, 0], first["bound"][0, 0])
    return ref, first, expected


def state(name):
    return moving_state(3, REST_Z, SETS[name]["t"])


def directions(name):
    return np.ascontiguousarray(di.spread(SETS[name]["waves"]["nfrequencies"]), dtype=np.float64)


def components(src, name, directional):
    """the components of a set from a context or the CPU oracle that has been given its waves"""
    comp = wk.irregular_components(src.irreg_spectrum())
    return dr.with_directions(comp, directions(name)) if directional else comp


@functools.lru_cache(maxsize=None)
def _reference(name, comp_key, g, second):
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    s = SETS[name]
    case = s["case"]()
    rd, t = s["waves"]["ramp_duration"], s["t"]
    kw = dict(mwl=MWL, stretching=s["stretching"])
    if not second:
        return mm.members(comp, case["water_depth"], case["rho"], s["lists"](), t, *state(name), ramp=mr.ramp_factor(t, rd), **kw)
    return m2.members2(comp, g, case["water_depth"], case["rho"], s["lists"](), t, *state(name), ramp=mr.ramp_factor(t, rd),
                       diff_band=s["diff_band"], sum_band=s["sum_band"], ramp_duration=rd, **kw)


def reference(name, comp, g, second=True):
    """morison_members2_ref.members2 of a set (second=False: morison_members_ref.members, order 1); computed once per argument set
    and shared: do not write into it."""
    return _reference(name, wi.key(comp), float(g), bool(second))


def check_conditions(ref, what, need=ALL_CASES):
    assert ref["clear"] and ref["margin"] > ref["eta_bound"], \
        f"{what}: a node is {ref['margin']:.3e} m from the free surface, the eta bound is {ref['eta_bound']:.3e} m (choose other inputs)"
    for c in need:
        assert any(c in s for s in ref["cases"]), (what, c, ref["cases"])


# ---- the waterline moves: one fixed, upright body; a column whose top node lies between eta1 and eta1 + eta2 ----
FLIP_T, FLIP_X = 31.0, np.arange(0.0, 60.0, 2.5)


def flip_inputs(comp, g, depth, rd):
    """(lists, state, j): a column of 2 segments on body 0 at the first x of FLIP_X where eta2 > 0 by more than 1 mm, its top node
    (j = 2) half way between eta1 and eta1 + eta2: dry at order 1, wet at order 2.  From the restatement of the sea alone."""
    pts = np.stack([FLIP_X, np.zeros_like(FLIP_X), np.full_like(FLIP_X, MWL)], axis=1)
    fn = dr.kinematics if len(comp) == 5 else wk.kinematics
    eta1 = fn(comp, depth, pts, [FLIP_T], mwl=MWL, stretching=False)[0][0][0]
    (eta2, _, _), _ = m2.increments(comp, g, depth, pts, FLIP_T, mwl=MWL, ramp_duration=rd)
    eta2 = np.asarray(eta2, dtype=np.float64)
    i = int(np.argmax(eta2 > 1e-3))
    assert eta2[i] > 1e-3, "no point of FLIP_X has eta2 > 1 mm (choose other inputs)"
    top = MWL + eta1[i] + 0.5 * eta2[i]
    pos = np.zeros((3, 3))
    pos[:, 0] = FLIP_X[i] + 40.0 * np.arange(3)
    z9 = np.zeros((3, 3))
    lists = [mm.member_lists([[0.0, 0.0, -6.0]], [[0.0, 0.0, top]], 1.0, 1.0, 2.0, 2), None, None]
    return lists, (pos, z9, z9, z9), 2
