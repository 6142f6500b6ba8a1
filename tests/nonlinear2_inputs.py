"""The fixed inputs of tests/test_gpu_nonlinear2.py (panels and clipped triangles on the second-order sea), shared with
tests/test_nonlinear2_ref_cpu.py, which evaluates the reference at every one of them on the CPU oracle's spectrum and asserts the
conditions the comparison needs (the GPU test asserts them again on the context's own spectrum).  TEST INFRASTRUCTURE ONLY.

Conditions (conditions, not tolerances: an input that misses one is replaced, the condition stays):
  * over the sets the reference's case counts include triangles with 0, 1, 2 and 3 wet vertices;
  * at least one surface point is wet under eta1 + eta2 and dry under eta1, or the other way round: the one-triangle set places
    its second vertex half an eta2 from the first-order surface (tuned_z below), whatever the spectrum;
  * no panel centroid closer than MIN_GAP to eta1 + eta2, no cut edge whose ends are closer than MIN_SPAN in h;
  * the bound is below 1e-6 of the largest component of the result.
"""
import numpy as np

import nonlinear2_ref as n2
import nonlinear_ref as nr
import surface_clip_inputs as ci
import wave2_inputs as wi
from morison_ref import LD, ramp_factor, rotation

G = 9.81
INF = float("inf")
MIN_GAP, MIN_SPAN = 1e-6, ci.MIN_SPAN
RAMP = 20.0


def waves(nf):
    """nf = 5: 0.1 .. 0.35 Hz around the peak, so that every amplitude and eta2 are of the size of the sea; nf = 300: above one tile"""
    fmin, fmax = (0.1, 0.35) if nf <= 16 else (0.05, 1.0)
    return dict(simulation_dt=0.05, simulation_duration=100.0, ramp_duration=RAMP, wave_height=2.0, wave_period=6.0, frequency_min=fmin,
                frequency_max=fmax, nfrequencies=nf, peak_enhancement_factor=2.0, seed=4)


def tri_list(n):
    return ("tris", ci.mesh(n))


def panel_list(n):
    return ("panels", nr.triangles_to_panels(ci.mesh(n)))


# name -> dict(N, depth, nf, lists, mwl, stretching, times, diff_band, sum_band, tuned = the surface point tuned_z places): one triangle; 257 triangles and 257 panels
# (across a chunk); a panel body, a body without a list and a triangle body at 300 components; finite and infinite depth; stretching
# on and off; mwl != 0; a time inside the ramp of 20 s; cut-offs that drop one sign
SETS = {
    "one_triangle": dict(N=1, depth=ci.DEPTH, nf=5, lists=lambda: [tri_list(1)], mwl=0.35, stretching=True, times=(7.5, 33.3),
                         diff_band=(0.0, INF), sum_band=(0.0, INF), tuned=1),
    "tris257_deep_diff": dict(N=1, depth=np.inf, nf=5, lists=lambda: [tri_list(257)], mwl=-0.2, stretching=False, times=(7.5,),
                              diff_band=(0.0, INF), sum_band=wi.NO_PAIR, tuned=None),
    "panels257_sum": dict(N=1, depth=ci.DEPTH, nf=5, lists=lambda: [panel_list(257)], mwl=0.35, stretching=True, times=(33.3,),
                          diff_band=wi.NO_PAIR, sum_band=(0.0, INF), tuned=None),
    "mixed_300": dict(N=3, depth=ci.DEPTH, nf=300, lists=lambda: [panel_list(12), None, tri_list(12)], mwl=0.35, stretching=True,
                      times=(7.5,), diff_band=(0.0, INF), sum_band=(0.0, INF), tuned=None),
}


def tuned_z(comp, depth, lists, pos, rpy, t, mwl, diff_band, sum_band, which):
    """pos.z of body 0 that puts surface point `which` of its list at mwl + eta1 + eta2 / 2 (x does not depend on pos.z)."""
    kind, data = lists[0]
    c0 = np.asarray(data[0] if kind == "panels" else data, dtype=np.float64).reshape(-1, 3)[which]
    d = rotation(rpy[0]) @ c0.astype(LD)
    P = np.array([[float(pos[0, 0] + d[0]), 0.0, 0.0]])
    r = n2.point_terms(comp, G, depth, P, t, mwl=mwl, diff_band=diff_band, sum_band=sum_band, ramp_duration=RAMP)
    return float(LD(mwl) + LD(r["eta1"][0]) + r["eta2"][0] / 2 - d[2])


def state(name, comp, t):
    s = SETS[name]
    pos, rpy = ci.state(s["N"], t)
    if s["tuned"] is not None:
        pos[0, 2] = tuned_z(comp, s["depth"], s["lists"](), pos, rpy, t, s["mwl"], s["diff_band"], s["sum_band"], s["tuned"])
    return pos, rpy


def reference(name, comp, rho, t, second_order=True):
    """nonlinear2_ref.nonlinear2 of a set at one time, with the conditions asserted; returns (ref, pos, rpy)"""
    s = SETS[name]
    pos, rpy = state(name, comp, t)
    ref = n2.nonlinear2(comp, G, s["depth"], rho, s["lists"](), t, pos, rpy, mwl=s["mwl"], stretching=s["stretching"],
                        ramp=ramp_factor(t, RAMP), diff_band=s["diff_band"], sum_band=s["sum_band"], ramp_duration=RAMP,
                        second_order=second_order)
    what = f"{name} t={t}"
    assert ref["margin"] >= MIN_GAP, f"{what}: a panel is {ref['margin']:.3e} m from the free surface (choose other inputs)"
    assert ref["cut_span"] >= MIN_SPAN, f"{what}: a cut edge spans {ref['cut_span']:.3e} m in h (choose other inputs)"
    return ref, pos, rpy
