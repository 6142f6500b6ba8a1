"""NumPy restatement of the nonlinear surface forces on the second-order sea in a short-crested sea (include/hydrochrono_amd.h:
hc_set_nonlinear_second_order_directional), composed of the restatements there are (TEST INFRASTRUCTURE ONLY):
tests/nonlinear2_ref.nonlinear2 does everything it does for the long-crested sea -- the distinct points, the patching through which
tests/nonlinear_ref.py (panels) and tests/surface_clip_ref.py (clipped triangles) take eta and p_d / rho, the flips, the cut term --
and is handed, for the length of a call, the point terms of this file in place of its own.  At every surface point P, with one
direction beta_i per component:
    eta  = eta1 + eta2
    p_d / rho = ramp sum_i (w_i^2 A_i / k_i) px_i cos theta_i + q2 - 1/2 ramp^2 (u1x^2 + u1y^2 + u1z^2)
    eta1, the first sum = directional_ref.dynamic_pressure_sum at P; u1 = directional_ref.kinematics at P (float64; the z_e of p_d),
           its horizontal part along every component's direction
    eta2 = wave2_dir_ref.fields at the same float64 P and t (longdouble): mwl, the two bands, ramp^2 through `ramp_duration`
    q2   = -d phi2 / dt = sum_{+-} sum_ij B+-_ij Omega+-_ij C(|kappa+-_ij|, z2) cos Theta+-_ij from wave2_dir_ref's own pair tables and
           pair geometry, times the same ramp^2 (q2_field below; tests/test_nonlinear2_dir_ref_cpu.py checks it against a difference
           quotient of wave2_dir_ref's phi2)

The error bound is that of nonlinear2_ref with the directional scales, nothing new: every first-order sum is known to 1e-11 of
directional_ref's scale (which carries the share of the phase argument) and every increment to 1e-11 of its sum |term|
(tests/test_gpu_directional.py, tests/test_gpu_wave_kinematics2_dir.py), so
    |delta p_d| / rho <= 1e-11 (ramp scale(p_d1) + sum|B Omega C| + ramp^2 (|u1x| scale(u1x) + |u1y| scale(u1y) + |u1z| scale(u1z)))
and the bracket is handed over as `pabs`, as there.
"""
import contextlib

import numpy as np

import directional_ref as dr
import nonlinear2_ref as n2
import wave2_dir_ref as wd
import wave2_ref as w2
from morison_ref import LD

FULL = wd.FULL


def q2_field(comp, beta, g, depth, points, t, mwl=0.0, diff_band=FULL, sum_band=FULL, ramp_duration=0.0, dtype=LD):
    """(q2 [P], sum |term| [P]) at one time: -d/dt of wave2_dir_ref's phi2 = sum B C(|kappa|, z2) sin Theta, held at
    z2 = min(z - mwl, 0) and at the bed."""
    tabs, _ = wd.pair_tables(comp, beta, g, depth, diff_band, sum_band, dtype)
    geo = wd.pair_geometry(comp, beta, dtype)
    A, w, k, phi = (np.asarray(v, dtype=dtype) for v in comp)
    c, s = (v.astype(dtype) for v in wd.unit_vectors(beta, A.size))
    h = None if np.isinf(depth) else dtype(depth)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    r2 = dtype(w2.ramp2(ramp_duration, t))
    val, sca = np.zeros(len(pts), dtype=dtype), np.zeros(len(pts), dtype=dtype)
    for p in range(len(pts)):
        z2 = min(dtype(pts[p, 2] - np.float64(mwl)), dtype(0))
        if h is not None:
            z2 = max(z2, -h)
        th = k * (dtype(pts[p, 0]) * c + dtype(pts[p, 1]) * s) - w * dtype(t) + phi
        cs, sn = np.cos(th), np.sin(th)
        cc, ss = cs[:, None] * cs[None, :], sn[:, None] * sn[None, :]
        for sgn, cosT in (("m", cc + ss), ("p", cc - ss)):
            ak, _, _, Om = geo[sgn]
            C, _ = w2._profiles(ak, z2, h)
            coef = tabs["B" + sgn] * C * Om
            val[p] += np.sum(coef * cosT) * r2
            sca[p] += np.sum(np.abs(coef)) * r2
    return val, sca


def point_terms(comp, beta, g, depth, points, t, mwl=0.0, stretching=False, ramp=1.0, diff_band=FULL, sum_band=FULL, ramp_duration=0.0,
                second_order=True, with_u1y=True, dtype=LD):
    """nonlinear2_ref.point_terms in the directional sea; dict of [P] arrays with u1y beside its keys.  with_u1y=False leaves u1y^2
    out of the pressure (for the test that shows the term is needed).  dtype: the precision of the pair sums (np.float64 for the
    self-check of tests/test_nonlinear2_dir_ref_cpu.py; the first-order sums are directional_ref's either way)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    comp5 = dr.with_directions(comp, beta)
    eta1, pds1, pabs1 = dr.dynamic_pressure_sum(comp5, depth, pts, t, mwl=mwl, stretching=stretching)
    zero = np.zeros(len(pts), dtype=LD)
    out = dict(eta1=eta1, eta2=zero, q2=zero, eta2_scale=zero, q2_scale=zero, u1x=zero, u1y=zero, u1z=zero)
    if second_order:
        (_, v, _), (_, vs, _) = dr.kinematics(comp5, depth, pts, [t], mwl=mwl, stretching=stretching)
        (e2, _, _, _), (e2s, _, _, _) = wd.fields(comp, beta, g, depth, pts, [t], mwl=mwl, diff_band=diff_band, sum_band=sum_band,
                                                 ramp_duration=ramp_duration, dtype=dtype)
        q2, q2s = q2_field(comp, beta, g, depth, pts, t, mwl, diff_band, sum_band, ramp_duration, dtype)
        e2, e2s, q2, q2s = (np.asarray(x).astype(LD) for x in (e2, e2s, q2, q2s))
        u = [v[0][:, j].astype(LD) for j in range(3)]
        us = [vs[0][:, j].astype(LD) for j in range(3)]
        out.update(eta2=e2[0], q2=q2, eta2_scale=e2s[0], q2_scale=q2s, u1x=u[0], u1y=u[1], u1z=u[2])
        rr = LD(ramp) * LD(ramp)
        sq = u[0] * u[0] + u[2] * u[2] + (u[1] * u[1] if with_u1y else 0)
        out["pds"] = LD(ramp) * pds1.astype(LD) + q2 - LD(0.5) * rr * sq
        out["pabs"] = LD(ramp) * pabs1.astype(LD) + q2s + rr * (np.abs(u[0]) * us[0] + np.abs(u[1]) * us[1] + np.abs(u[2]) * us[2])
    else:
        out["pds"], out["pabs"] = LD(ramp) * pds1.astype(LD), LD(ramp) * pabs1.astype(LD)
    out["eta"] = eta1.astype(LD) + out["eta2"]
    return out


@contextlib.contextmanager
def _directional_terms(beta, dtype):
    """For the length of the block nonlinear2_ref.nonlinear2 takes its point terms from this file, at the directions beta."""
    keep = n2.point_terms
    n2.point_terms = lambda comp, g, depth, pts, t, **kw: point_terms(comp, beta, g, depth, pts, t, dtype=dtype, **kw)
    try:
        yield
    finally:
        n2.point_terms = keep


def nonlinear2_dir(comp, beta, g, depth, rho, lists, t, pos, rpy, dtype=LD, **kw):
    """comp: (A, w, k, phi); beta: one direction per component.  The other arguments and the result are those of
    nonlinear2_ref.nonlinear2; dtype as point_terms takes it."""
    beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
    assert beta.size == np.asarray(comp[0]).size
    with _directional_terms(beta, dtype):
        return n2.nonlinear2(comp, g, depth, rho, lists, t, pos, rpy, **kw)
