"""The fixed inputs of tests/test_gpu_surface_clip.py (triangles clipped at the free surface), shared with
tests/test_surface_clip_ref_cpu.py, which evaluates the reference at every one of them on the CPU oracle's spectrum and asserts the
conditions the comparison needs (the GPU test asserts them again on the context's own spectrum).  TEST INFRASTRUCTURE ONLY.

Conditions (conditions, not tolerances: an input that misses one is replaced, the condition stays):
  * over the comparisons of a test the reference's case counts include triangles with 0, 1, 2 and 3 wet vertices; every list of 12
    or more triangles has cut triangles itself;
  * cut_span >= 1e-3 m: no cut edge whose ends are closer than that in h, so the cut term of the bound stays far below the result;
  * the boxes are tilted (roll and pitch of at least 0.05 rad) and tall: on a whole box the top face is dry and the bottom face wet.
"""
import numpy as np

import nonlinear_ref as nr
import surface_clip_ref as sc
import wave_kinematics_ref as wk
from morison_ref import ramp_factor

G = 9.81
DEPTH = 60.0  # with 0.01 .. 2 Hz long-wave, finite-depth and k d > 500 components are all present
MIN_SPAN = 1e-3
COUNTS = (1, 12, 256, 257, 768)  # triangles per body: a partly filled chunk, a whole box, a full chunk, across the boundary, three chunks
REG_AMP, REG_OMEGA, REG_PHASE = 0.177, 2.094395102, 0.7
RAMP = 20.0
BOX_LO, BOX_HI = [-1.0, -0.5, -2.0], [1.0, 0.5, 2.0]
TIMES = (7.5, 33.3)  # inside the ramp of 20 s, after it


def irreg(nf, seed=4):
    return dict(simulation_dt=0.05, simulation_duration=100.0, ramp_duration=RAMP, wave_height=1.0, wave_period=6.0, frequency_min=0.01,
                frequency_max=2.0, nfrequencies=nf, peak_enhancement_factor=2.0, seed=seed)


def synth_case(N, depth=DEPTH):
    from hydrochrono_amd.synthetic import many_body_case
    return many_body_case(N, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7, water_depth=depth)


def mesh(n):
    """n triangles: one that crosses the surface, the 12-triangle box, the 768-triangle box, or the first n of a fixed shuffle of it"""
    if n == 1:
        return np.array([[[-1.0, -0.5, -1.25], [1.0, -0.25, 0.75], [0.0, 0.5, 1.5]]])
    if n == 12:
        return nr.box_triangles(BOX_LO, BOX_HI, m=1)
    fine = nr.box_triangles(BOX_LO, BOX_HI, m=8)
    return fine if n == len(fine) else fine[np.random.default_rng(768).permutation(len(fine))[:n]]


def lists(N, n):
    """body 1 of three carries nothing, between two that carry triangles"""
    return [mesh(n)] if N == 1 else [mesh(n), None, mesh(COUNTS[(COUNTS.index(n) + 2) % len(COUNTS)])]


def state(N, t):
    """pos, rpy [N][3]: every body tilted, the bodies 15 m apart along the wave"""
    b = np.arange(float(N))
    pos = np.stack([15.0 * b + 0.3 + 0.01 * t, -0.1 + 0.2 * b, 0.15 - 0.1 * b + 0.002 * t], axis=1)
    rpy = np.stack([0.31 - 0.1 * b, -0.22 - 0.07 * b + 0.001 * t, 0.4 + 0.3 * b], axis=1)
    return pos, rpy


# (name, N, depth, kind, wave parameters): the systems of section 1
SYSTEMS = [
    ("regular N=1", 1, DEPTH, "regular", (REG_AMP, REG_OMEGA)),
    ("regular N=3 deep", 3, np.inf, "regular", (REG_AMP, REG_OMEGA)),
    ("irregular nf=256 N=1", 1, DEPTH, "irregular", irreg(256)),
    ("spectral nf=257 N=3", 3, DEPTH, "spectral", irreg(257)),
    ("spectral nf=300 N=3 deep", 3, np.inf, "spectral", irreg(300)),
    ("irregular nf=300 N=1", 1, DEPTH, "irregular", irreg(300)),
    ("still water N=3", 3, DEPTH, "none", None),
]


def add_waves(h, kind, params):
    """on a HydroForces, a HydroGroup or the CPU oracle (whose spectrum does not depend on the model that sums it)"""
    if kind == "regular":
        h.add_waves_regular(*params)
    elif kind == "irregular" or (kind == "spectral" and not hasattr(h, "lib")):
        h.add_waves_irregular(**params)
    elif kind == "spectral":
        h.add_waves_irregular(spectral=True, **params)


def components(h, kind, params):
    if kind == "regular":
        return wk.regular_components(params[0], params[1], h.regular_coeffs()[2], REG_PHASE)
    if kind in ("irregular", "spectral"):
        return wk.irregular_components(h.irreg_spectrum())
    return None


def comparisons(kind, N):
    """(n, mwl, stretching, t, ramp) of a system of section 1; a regular wave has no stretching and no ramp, still water neither"""
    out = []
    for n in COUNTS if N == 1 else (12, 257, 768):
        if kind == "regular":
            out += [(n, 0.35, True, 3.7, 1.0), (n, -0.2, False, 3.7, 1.0)]
        elif kind == "none":
            out += [(n, 0.3, True, 3.0, 1.0)]
        else:
            out += [(n, mwl, st, t, ramp_factor(t, RAMP)) for mwl, st in ((0.35, True), (0.35, False), (0.0, True)) for t in TIMES]
    return out


def reference(case, tris, comp, kind, n, mwl, stretching, t, ramp, what):
    """the restatement at one comparison, with the conditions asserted; returns (ref, pos, rpy)"""
    N = len(tris)
    pos, rpy = state(N, t)
    assert np.all(np.abs(rpy[:, :2]) >= 0.05), what
    ref = sc.clipped(comp, case["water_depth"], case["rho"], G, tris, t, pos, rpy, mwl=mwl, stretching=stretching and kind not in ("regular", "none"),
                     ramp=ramp)
    assert ref["cut_span"] >= MIN_SPAN, f"{what}: a cut edge spans {ref['cut_span']:.3e} m in h (choose other inputs)"
    for b, tl in enumerate(tris):
        if tl is None:
            continue
        c = ref["cases"][b]
        if len(tl) >= 12:
            assert c[1] + c[2] > 0, (what, b, c.tolist())
        if len(tl) in (12, 768):  # a whole box: the top face dry, the bottom face wet
            assert c[0] >= len(tl) // 6 and c[3] >= len(tl) // 6, (what, b, c.tolist())
    return ref, pos, rpy
