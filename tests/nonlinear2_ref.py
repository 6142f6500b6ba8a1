"""NumPy restatement of the nonlinear surface forces on the second-order sea (include/hydrochrono_amd.h:
hc_set_nonlinear_second_order), written from its definition (TEST INFRASTRUCTURE ONLY).  It composes the restatements there are:
tests/nonlinear_ref.py (panels) and tests/surface_clip_ref.py (clipped triangles) do the frame algebra, the wet test, the clipping
and the sums in longdouble, unchanged; this file hands them, at every surface point P (a panel's centroid, a triangle's vertex),
    eta  = eta1 + eta2
    p_d / rho = ramp sum_i (w_i^2 A_i / k_i) px_i cos theta_i + q2 - 1/2 ramp^2 (u1x^2 + u1z^2)
in place of their first-order values (they are then called with ramp = 1), with
    eta1, the first sum, u1 = wave_kinematics_ref.kinematics at P (float64; the z_e of p_d: stretching by eta1, second mwl)
    eta2 = wave2_ref.fields at the same float64 P and t (longdouble): mwl, the two bands, ramp^2 through `ramp_duration` (0: none)
    q2   = -d phi2 / dt = sum_{+-} sum_ij B+-_ij Omega C(kappa, z2) cos Theta, from wave2_ref's own pair tables and profiles, times
           the same ramp^2 (q2_field below; tests/test_nonlinear2_ref_cpu.py checks it against a difference quotient of wave2_ref's phi2)

The error bound (per body and component) is the one of those two files with the magnitudes of the new terms in it, as
tests/morison2_ref.py builds its own: every first-order sum and every increment is known to 1e-11 of its sum |term|
(tests/test_gpu_wave_kinematics.py, tests/test_gpu_wave_kinematics2.py), so to first order
    |delta p_d| / rho <= 1e-11 (ramp sum|..px| + sum|B Omega C| + ramp^2 (|u1x| sum|u1x terms| + |u1z| sum|u1z terms|))
and the magnitude of p_d / rho without cancellation is ramp sum|..px| + sum|B Omega C| + 1/2 ramp^2 |u1|^2, which the bracket above
dominates (|u| <= sum|terms|): the bracket is handed over as the files' `pabs`, serving both of its roles.  The cut term of
surface_clip_ref takes delta eta <= 1e-11 (sum|A| + sum|eta2 terms|).
"""
import contextlib

import numpy as np

import nonlinear_ref as nr
import surface_clip_ref as sc
import wave2_ref as w2
import wave_kinematics_ref as wk
from morison_ref import LD

_first_order_sum = nr.dynamic_pressure_sum  # (the name is re-bound for the length of a call of nonlinear2 below)


def q2_field(comp, g, depth, points, t, mwl=0.0, diff_band=w2.FULL, sum_band=w2.FULL, ramp_duration=0.0, dtype=LD):
    """(q2 [P], sum |term| [P]) at one time: -d/dt of wave2_ref's phi2 = sum B C sin Theta, held at z2 = min(z - mwl, 0) and at the bed."""
    tabs, _ = w2.pair_tables(comp, g, depth, diff_band, sum_band, dtype)
    A, w, k, phi = (np.asarray(v, dtype=dtype) for v in comp)
    h = None if np.isinf(depth) else dtype(depth)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    kap = {"m": k[:, None] - k[None, :], "p": k[:, None] + k[None, :]}
    Om = {"m": w[:, None] - w[None, :], "p": w[:, None] + w[None, :]}
    r2 = dtype(w2.ramp2(ramp_duration, t))
    val, sca = np.zeros(len(pts), dtype=dtype), np.zeros(len(pts), dtype=dtype)
    for p in range(len(pts)):
        z2 = min(dtype(pts[p, 2] - np.float64(mwl)), dtype(0))
        if h is not None:
            z2 = max(z2, -h)
        th = k * dtype(pts[p, 0]) - w * dtype(t) + phi
        c, s_ = np.cos(th), np.sin(th)
        cc, ss = c[:, None] * c[None, :], s_[:, None] * s_[None, :]
        for s, cosT in (("m", cc + ss), ("p", cc - ss)):
            C, _ = w2._profiles(np.abs(kap[s]), z2, h)
            coef = tabs["B" + s] * C * Om[s]
            val[p] += np.sum(coef * cosT) * r2
            sca[p] += np.sum(np.abs(coef)) * r2
    return val, sca


def point_terms(comp, g, depth, points, t, mwl=0.0, stretching=False, ramp=1.0, diff_band=w2.FULL, sum_band=w2.FULL, ramp_duration=0.0,
                second_order=True):
    """Everything the definition needs at the points [P][3] and one time; dict of [P] arrays: eta1, eta2, q2 and their sums of
    |term| (eta2_scale, q2_scale), u1x, u1z, eta (= eta1 + eta2), pds (= p_d / rho) and pabs (the bracket of the docstring)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    eta1, pds1, pabs1 = _first_order_sum(comp, depth, pts, t, mwl=mwl, stretching=stretching)
    zero = np.zeros(len(pts), dtype=LD)
    out = dict(eta1=eta1, eta2=zero, q2=zero, eta2_scale=zero, q2_scale=zero, u1x=zero, u1z=zero)
    if second_order:
        (_, v, _), (_, vs, _) = wk.kinematics(comp, depth, pts, [t], mwl=mwl, stretching=stretching)
        (e2, _, _, _), (e2s, _, _, _) = w2.fields(comp, g, depth, pts, [t], mwl=mwl, diff_band=diff_band, sum_band=sum_band,
                                                 ramp_duration=ramp_duration)
        q2, q2s = q2_field(comp, g, depth, pts, t, mwl, diff_band, sum_band, ramp_duration)
        ux, uz, uxs, uzs = (x.astype(LD) for x in (v[0][:, 0], v[0][:, 2], vs[0][:, 0], vs[0][:, 2]))
        out.update(eta2=e2[0], q2=q2, eta2_scale=e2s[0], q2_scale=q2s, u1x=ux, u1z=uz)
        rr = LD(ramp) * LD(ramp)
        out["pds"] = LD(ramp) * pds1.astype(LD) + q2 - LD(0.5) * rr * (ux * ux + uz * uz)
        out["pabs"] = LD(ramp) * pabs1.astype(LD) + q2s + rr * (np.abs(ux) * uxs + np.abs(uz) * uzs)
    else:
        out["pds"], out["pabs"] = LD(ramp) * pds1.astype(LD), LD(ramp) * pabs1.astype(LD)
    out["eta"] = eta1.astype(LD) + out["eta2"]
    return out


@contextlib.contextmanager
def _second_order_sea(terms):
    """nonlinear_ref and surface_clip_ref take eta and p_d / rho from nr.dynamic_pressure_sum: for the length of the block that is
    `terms` (a function of the points), evaluated once per distinct point."""
    first_order = nr.dynamic_pressure_sum

    def patched(comp, depth, points, t, mwl=0.0, stretching=False):
        uniq, inv, _ = distinct_points(points)
        r = terms(uniq)
        return r["eta"][inv], r["pds"][inv], r["pabs"][inv]

    nr.dynamic_pressure_sum = patched
    try:
        yield
    finally:
        nr.dynamic_pressure_sum = first_order


def distinct_points(body_points):
    """The rows of body_points [n][3] (body frame) without repeats, in the order of their first use, and the index of every row into
    them: two points are the same when their doubles have equal bits."""
    seen, idx = {}, []
    rows = np.ascontiguousarray(body_points, dtype=np.float64).reshape(-1, 3)
    for row in rows:
        idx.append(seen.setdefault(row.tobytes(), len(seen)))
    first = np.array([idx.index(i) for i in range(len(seen))], dtype=int)
    return rows[first] if len(seen) else np.zeros((0, 3)), np.array(idx, dtype=int), first


def nonlinear2(comp, g, depth, rho, lists, t, pos, rpy, mwl=0.0, stretching=False, ramp=1.0, diff_band=w2.FULL, sum_band=w2.FULL,
               ramp_duration=0.0, second_order=True):
    """lists: per body None, ("panels", (c, s)) or ("tris", triangles [n][3][3]).  comp: (A, w, k, phi).  ramp: the factor of order 1
    on p_d1; ramp_duration > 0 applies ramp^2 of wave2_ref.ramp2 to the increments (0: apply_ramp off, or a regular wave).
    second_order=False: the first-order restatements themselves.
    Returns dict(buoy, fk, bound_buoy, bound_fk [N][6]; cases [N][4] and cut_span of the triangles; margin of the panels; per body
    p (world, float64), eta1, eta2, q2, eta2_scale, q2_scale of its distinct surface points in the order of their first use; flips =
    the number of distinct points whose wet state differs between eta1 and eta1 + eta2)."""
    pos, rpy = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy))
    N = pos.shape[0]
    panels = [l[1] if l is not None and l[0] == "panels" else None for l in lists]
    tris = [l[1] if l is not None and l[0] == "tris" else None for l in lists]
    kw = dict(mwl=mwl, stretching=stretching, ramp=ramp, diff_band=diff_band, sum_band=sum_band, ramp_duration=ramp_duration,
              second_order=second_order)
    terms = lambda pts: point_terms(comp, g, depth, pts, t, **kw)
    # the cut term of surface_clip_ref reads sum |A| off the components: the largest sum |eta2 terms| joins it
    world_p, world_t = nr.panel_points(panels, pos, rpy), sc.vertex_points(tris, pos, rpy)
    out = dict(p=[], eta1=[], eta2=[], q2=[], eta2_scale=[], q2_scale=[])
    flips, e2s_max = 0, 0.0
    for b in range(N):
        if panels[b] is not None:
            _, _, first = distinct_points(panels[b][0])
            P = world_p[b][first]
        elif tris[b] is not None:
            _, _, first = distinct_points(np.asarray(tris[b]).reshape(-1, 3))
            P = world_t[b].reshape(-1, 3)[first]
        else:
            P = np.zeros((0, 3))
        r = terms(P) if len(P) else {k: np.zeros(0) for k in ("eta1", "eta2", "q2", "eta2_scale", "q2_scale")}
        out["p"].append(P)
        for k in ("eta1", "eta2", "q2", "eta2_scale", "q2_scale"):
            out[k].append(np.asarray(r[k]))
        if len(P):
            h1 = P[:, 2] - mwl - r["eta1"]
            flips += int(np.sum((h1 <= 0) != (h1.astype(LD) - r["eta2"] <= 0)))
            e2s_max = max(e2s_max, float(np.max(r["eta2_scale"])))
    comp_cut = (np.concatenate([np.abs(comp[0]), [e2s_max]]),) + tuple(comp[1:])
    with _second_order_sea(terms):
        a = nr.nonlinear(comp, depth, rho, g, panels, t, pos, rpy, mwl=mwl, stretching=stretching, ramp=1.0)
        c = sc.clipped(comp_cut, depth, rho, g, tris, t, pos, rpy, mwl=mwl, stretching=stretching, ramp=1.0)
    res = {k: a[k] + c[k] for k in ("buoy", "fk", "bound_buoy", "bound_fk")}  # (a body has one kind: the other adds zeros)
    res.update(cases=c["cases"], cut_span=c["cut_span"], margin=a["margin"], flips=flips, **out)
    return res
