"""The fixed inputs of tests/test_gpu_nonlinear2_dir.py (panels and clipped triangles on the second-order sea in a short-crested sea),
shared with tests/test_nonlinear2_dir_ref_cpu.py, which evaluates the reference at every one of them on the CPU oracle's spectrum and
asserts the conditions the comparison needs (the GPU test asserts them again on the context's own spectrum).  TEST INFRASTRUCTURE
ONLY.  The sets mirror tests/nonlinear2_inputs.SETS -- the same meshes, states, seas, mean levels, times and bands -- with the
deterministic spread of tests/wave2_dir_inputs.py (within +-1.2 rad) as the directions, and one set more: crossing components have a
sum-frequency potential in infinite depth, so the 257 triangles in deep water run once with the difference band alone and once with
the sum band alone.

Conditions (those of tests/nonlinear2_inputs.py; conditions, not tolerances: an input that misses one is replaced, the condition
stays):
  * over the sets the reference's case counts include triangles with 0, 1, 2 and 3 wet vertices;
  * at least one surface point is wet under eta1 + eta2 and dry under eta1, or the other way round: the one-triangle set places its
    second vertex half an eta2 from the first-order surface (tuned_z below), whatever the spectrum;
  * no panel centroid closer than MIN_GAP to eta1 + eta2, no cut edge whose ends are closer than MIN_SPAN in h;
  * the bound is below 1e-6 of the largest component of the result.
"""
import functools

import numpy as np

import nonlinear2_dir_ref as nd
import nonlinear2_inputs as ni
import wave2_dir_inputs as di
import wave2_inputs as wi
from morison_ref import LD, ramp_factor, rotation
from nonlinear2_inputs import G, INF, MIN_GAP, MIN_SPAN, RAMP, ci, panel_list, tri_list, waves  # noqa: F401

# name -> dict as tests/nonlinear2_inputs.SETS: one triangle; 257 triangles and 257 panels (across a chunk); a panel body, a body
# without a list and a triangle body at 300 components (one more than a tile of the pair sum); finite and infinite depth; stretching
# on and off; mwl != 0; a time inside the ramp of 20 s; cut-offs that drop one sign
SETS = dict(ni.SETS)
SETS["tris257_deep_sum"] = dict(ni.SETS["tris257_deep_diff"], diff_band=wi.NO_PAIR, sum_band=(0.0, INF))


def directions(name):
    return np.ascontiguousarray(di.spread(SETS[name]["nf"]), dtype=np.float64)


def spread_sea(h, case, nf):
    """The spectral model of ni.waves(nf) with heading tables for every body (what non-uniform directions need), on a HydroForces or
    a HydroGroup: tests/morison2_dir_inputs.spread_sea."""
    import morison2_dir_inputs as mdi
    mdi.spread_sea(h, case, waves(nf))


def tuned_z(comp, beta, depth, lists, pos, rpy, t, mwl, diff_band, sum_band, which):
    """pos.z of body 0 that puts surface point `which` of its list at mwl + eta1 + eta2 / 2 (x and y do not depend on pos.z, and
    neither eta1 nor eta2 depends on z)."""
    kind, data = lists[0]
    c0 = np.asarray(data[0] if kind == "panels" else data, dtype=np.float64).reshape(-1, 3)[which]
    d = rotation(rpy[0]) @ c0.astype(LD)
    P = np.array([[float(pos[0, 0] + d[0]), float(pos[0, 1] + d[1]), 0.0]])
    r = nd.point_terms(comp, beta, G, depth, P, t, mwl=mwl, diff_band=diff_band, sum_band=sum_band, ramp_duration=RAMP)
    return float(LD(mwl) + LD(r["eta1"][0]) + r["eta2"][0] / 2 - d[2])


def state(name, comp, t):
    s = SETS[name]
    pos, rpy = ci.state(s["N"], t)
    if s["tuned"] is not None:
        pos[0, 2] = tuned_z(comp, directions(name), s["depth"], s["lists"](), pos, rpy, t, s["mwl"], s["diff_band"], s["sum_band"], s["tuned"])
    return pos, rpy


@functools.lru_cache(maxsize=None)
def _reference(name, comp_key, rho, t, second_order, dtype):
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    s = SETS[name]
    pos, rpy = state(name, comp, t)
    ref = nd.nonlinear2_dir(comp, directions(name), G, s["depth"], rho, s["lists"](), t, pos, rpy, dtype=dtype, mwl=s["mwl"],
                            stretching=s["stretching"], ramp=ramp_factor(t, RAMP), diff_band=s["diff_band"], sum_band=s["sum_band"],
                            ramp_duration=RAMP, second_order=second_order)
    what = f"{name} t={t}"
    assert ref["margin"] >= MIN_GAP, f"{what}: a panel is {ref['margin']:.3e} m from the free surface (choose other inputs)"
    assert ref["cut_span"] >= MIN_SPAN, f"{what}: a cut edge spans {ref['cut_span']:.3e} m in h (choose other inputs)"
    return ref, pos, rpy


def reference(name, comp, rho, t, second_order=True, dtype=LD):
    """nonlinear2_dir_ref.nonlinear2_dir of a set at one time, with the conditions asserted; returns (ref, pos, rpy).  Computed once
    per argument set and shared: do not write into it."""
    return _reference(name, wi.key(comp), float(rho), float(t), bool(second_order), dtype)
