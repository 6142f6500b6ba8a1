"""Input sets shared by tests/test_morison2_dir_ref_cpu.py (which checks, on the CPU oracle's spectrum, that no element of any set
is closer than MIN_GAP to the free surface of the directional second-order sea) and tests/test_gpu_morison2_dir.py (which asserts it
again on the context's own spectrum before it compares).  Elements, states and bands as tests/morison2_inputs.py; the direction
generators are those of tests/wave2_dir_inputs.py.  Each set is there for a reason:

  column_30m_spread   30 m of water: the finite-depth profile of the pair sum (three exp per pair); a column through the surface, so
                      the wet test decides for some elements; both stretching options; one time inside the ramp
  three_deep_cos2s    three bodies in infinitely deep water, 65 components (wave width + 1), the difference band alone
  sphere2_oppose      two components that oppose each other: the tau branch of |kappa|^2
  wide_257_near       257 components (two LDS tiles of rows and of columns), two neighbours 1e-9 rad apart, a narrow difference band
  many_elements       257 elements on one body (the item kernel's workgroup boundary inside a body), 5 on the next, none on the last
"""
import functools

import numpy as np

import morison2_inputs as mi
import wave2_dir_inputs as di
import wave2_inputs as wi
from cases import sphere_case, three_body_case
from morison2_inputs import MIN_GAP, moving_state  # noqa: F401

INF = float("inf")
FULL = (0.0, INF)

# name -> dict(case, waves, directions, elements [N], rest_z, options [(mwl, stretching)], times, diff_band, sum_band)
SETS = {
    "column_30m_spread": dict(case=mi.shallow_case, waves=wi.sphere_waves(16, 0.04, 0.30), directions=di.spread,
                              elements=lambda: [mi.column_elements(12, -18.0, 6.0, 41)], rest_z=-2.0, options=[(0.3, True), (0.3, False)],
                              times=(7.3, 41.7), diff_band=FULL, sum_band=FULL),
    "three_deep_cos2s": dict(case=three_body_case, waves=wi.three_waves(65), directions=di.cos2s,
                             elements=lambda: [mi.random_elements(9, 51), mi.random_elements(4, 52), mi.random_elements(17, 53)],
                             rest_z=-3.0, options=[(0.25, True)], times=(12.5, 33.3), diff_band=FULL, sum_band=wi.NO_PAIR),
    "sphere2_oppose": dict(case=sphere_case, waves=wi.sphere_waves(2, 0.07, 0.11), directions=di.oppose,
                           elements=lambda: [(np.array([[1.5, -2.0, -4.0]]), np.array([[1.5, 0.7, 2.0]]), np.array([[2.0, 1.0, 0.5]]))], rest_z=-2.0, options=[(0.1, True)], times=(12.5,),
                           diff_band=FULL, sum_band=FULL),
    "wide_257_near": dict(case=sphere_case, waves=wi.sphere_waves(257), directions=di.near,
                          elements=lambda: [mi.column_elements(6, -12.0, 5.0, 61)], rest_z=-2.0, options=[(0.1, True)], times=(33.0,),
                          diff_band=(0.0, 0.07), sum_band=wi.NO_PAIR),
    "many_elements": dict(case=three_body_case, waves=wi.three_waves(8), directions=di.spread,
                          elements=lambda: [mi.random_elements(257, 71), mi.random_elements(5, 72), None], rest_z=-3.0,
                          options=[(0.1, True)], times=(23.0,), diff_band=FULL, sum_band=FULL),
}


def directions(name):
    return np.ascontiguousarray(SETS[name]["directions"](SETS[name]["waves"]["nfrequencies"]), dtype=np.float64)


def spread_sea(h, case, waves):
    """The spectral model with excitation tables on a heading grid for every body, its own table at both ends of [-4, 4] (as
    tests/test_gpu_wave_kinematics2_dir.py): what non-uniform directions need.  h: HydroForces or HydroGroup."""
    for b, bd in enumerate(case["bodies"]):
        mag, ph = (np.stack([np.asarray(bd[k]).reshape(6, -1)] * 2, axis=1) for k in ("ex_mag", "ex_phase"))
        h.set_body_excitation_rao_headings(b, [-4.0, 4.0], bd["w"], mag, ph)
    h.add_waves_irregular(spectral=True, **waves)


@functools.lru_cache(maxsize=None)
def _reference(name, comp_key, g, t, mwl, stretching, dtype):
    import morison2_dir_ref as md
    import morison_ref as mr
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    s = SETS[name]
    case = s["case"]()
    elements = s["elements"]()
    state = moving_state(len(elements), s["rest_z"], t)
    rd = s["waves"]["ramp_duration"]
    ref = md.morison2_dir(comp, directions(name), g, case["water_depth"], case["rho"], elements, t, *state, mwl=mwl, stretching=stretching,
                          ramp=mr.ramp_factor(t, rd), diff_band=s["diff_band"], sum_band=s["sum_band"], ramp_duration=rd, dtype=dtype)
    return ref, state


def reference(name, comp, g, t, mwl, stretching, dtype=np.longdouble):
    """morison2_dir_ref.morison2_dir of a set at one time under one choice of options (and the state it was given); computed once
    per argument set and shared: do not write into it."""
    return _reference(name, wi.key(comp), float(g), float(t), float(mwl), bool(stretching), dtype)
