"""NumPy longdouble restatement of the directional wave sums (include/hydrochrono_amd.h: hc_set_wave_directions),
written from the formulas (TEST INFRASTRUCTURE ONLY).

Per component (A, w, k, phi, theta) at a point (x, y, z), z' = z - mwl:
    psi = k (x cos theta + y sin theta) - w t + phi,   eta = sum A cos psi
    u_h = w A p_x cos psi,  velocity = (u_h cos theta, u_h sin theta, w A p_z sin psi)
    a_h = w^2 A p_x sin psi,  acceleration = (a_h cos theta, a_h sin theta, -w^2 A p_z cos psi)
with the profiles, the stretching, the double mwl subtraction and the infinite-depth limit of tests/wave_kinematics_ref.py.  A
component tuple here has five entries; theta = 0 gives the long-crested sums.

Error bound, per output element, derived as tests/wave_kinematics_ref.py derives its own: there the bound is 1e-11 sum_i |term_i|,
a term's magnitude taken over its phase, because the phase argument carries an absolute rounding error of a few ulp of its own
size in any FP64 evaluation.  Here the argument gains k y sin theta, and it is formed in one more step (x cos + y sin, then times
k), so its magnitude |psi|_i = |k| (|x cos| + |y sin|) + |w t| + |phi| enters explicitly: a term's share is
|term_i| (1e-11 + 4 eps |psi|_i), four roundings of half an ulp of at most |psi|_i each in forming psi, doubled for the FP64 side's
own representation of cos theta, sin theta (half an ulp each, times |k x|, |k y|).  For the arguments of the existing tests (|psi|
below 1e4) the second part stays under the first; it keeps the bound honest for points far from the origin.  The reference's own
error (longdouble, 2^-63) is below both.  The Morison and surface-pressure compositions reuse tests/morison_ref.py,
tests/nonlinear_ref.py and tests/surface_clip_ref.py unchanged, with their kinematics callbacks pointed at the sums of this file
(`directional()` below): their bounds are built from the sums of |term| returned here, scaled so that KIN_TOL times them is the
bound above.
"""
import contextlib

import numpy as np

import morison_ref
import nonlinear_ref
import surface_clip_ref
import wave_kinematics_ref as wk

LD = np.longdouble
TOL = 1e-11
EPS = 2.0 ** -52


def with_directions(comp, theta):
    A, w, k, phi = comp[:4]
    return A, w, k, phi, np.broadcast_to(np.asarray(theta, dtype=np.float64), np.shape(A)).copy()


def _psi(comp, pts, t):
    """psi [T][P][nf] in longdouble and its magnitude without cancellation."""
    A, w, k, phi, th = (np.asarray(v, dtype=LD) for v in comp)
    x, y = pts[:, 0].astype(LD)[None, :, None], pts[:, 1].astype(LD)[None, :, None]
    c, s = np.cos(th)[None, None, :], np.sin(th)[None, None, :]
    kk, ww, pp, tt = k[None, None, :], w[None, None, :], phi[None, None, :], t.astype(LD)[:, None, None]
    psi = kk * (x * c + y * s) - ww * tt + pp
    mag = np.abs(kk) * (np.abs(x * c) + np.abs(y * s)) + np.abs(ww * tt) + np.abs(pp)
    return psi, mag, c, s


def _share(mag):
    """a term's tolerance as a multiple of |term|, divided by TOL (so that TOL * scale is the bound)"""
    return 1.0 + (4.0 * EPS / TOL) * mag


def kinematics(comp, depth, points, times, mwl=0.0, stretching=False):
    """(eta [T][P], vel [T][P][3], acc [T][P][3]) in float64 and the matching scales: TOL * scale is the bound of an element."""
    A, w, k, phi, th = (np.asarray(v, dtype=LD) for v in comp)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    psi, mag, c, s = _psi(comp, pts, t)
    share = _share(mag)
    sn, cs = np.sin(psi), np.cos(psi)
    eta = (A[None, None, :] * cs).sum(axis=2)
    eta_scale = (np.abs(A)[None, None, :] * share).sum(axis=2)
    z = np.broadcast_to(pts[None, :, 2].astype(LD), eta.shape)
    depth_l = LD(depth)
    if stretching:
        zr = z - LD(mwl)
        eta64 = eta.astype(np.float64).astype(LD)  # the wet test and the stretching see the FP64 eta's neighbourhood; its error is in the bound of eta
        zs = (zr - eta64) if np.isinf(depth) else depth_l * (zr - eta64) / (depth_l + eta64)
        ze = zs - LD(mwl)
    else:
        ze = z - LD(mwl)
    k64 = np.asarray(comp[2], dtype=np.float64)
    deep = (2 * np.pi / k64 > depth) | (k64 * depth > 500.0)
    kk, zz = k[None, None, :], ze[:, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(kk * zz)
        if np.all(deep):
            px = pz = e
        else:
            q = kk * (zz + depth_l)
            sh = np.sinh(k * depth_l)[None, None, :]
            px = np.where(deep, e, np.cosh(q) / sh)
            pz = np.where(deep, e, np.sinh(q) / sh)
    wa, w2a = (w * A)[None, None, :], (w * w * A)[None, None, :]
    vel, acc = np.zeros(eta.shape + (3,), dtype=LD), np.zeros(eta.shape + (3,), dtype=LD)
    vsc, asc = np.zeros_like(vel), np.zeros_like(acc)
    for col, prof, vph, aph, lay in ((0, px, cs, sn, c), (1, px, cs, sn, s), (2, pz, sn, -cs, LD(1))):
        vel[..., col], vsc[..., col] = (wa * prof * vph * lay).sum(axis=2), (np.abs(wa * prof * lay) * share).sum(axis=2)
        acc[..., col], asc[..., col] = (w2a * prof * aph * lay).sum(axis=2), (np.abs(w2a * prof * lay) * share).sum(axis=2)
    f64 = lambda v: np.asarray(v, dtype=np.float64)  # noqa: E731
    return (f64(eta), f64(vel), f64(acc)), (f64(eta_scale), f64(vsc), f64(asc))


def dynamic_pressure_sum(comp, depth, points, t, mwl=0.0, stretching=False):
    """nonlinear_ref.dynamic_pressure_sum on the directional sea: the horizontal-velocity amplitude sum with w A replaced by
    w^2 A / k and no layout factor (the pressure is a scalar)."""
    A, w, k, phi, th = comp
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    (eta, _, _), _ = kinematics(comp, depth, pts, [t], mwl=mwl, stretching=stretching)
    # a component set with amplitudes A / k and direction 0 layout: x-velocity of `kinematics` evaluated with theta's phase
    psi, mag, _, _ = _psi(comp, pts, np.array([float(t)]))
    z = pts[:, 2].astype(LD)
    e0 = eta[0].astype(LD)
    if stretching:
        zr = z - LD(mwl)
        zs = (zr - e0) if np.isinf(depth) else LD(depth) * (zr - e0) / (LD(depth) + e0)
        ze = zs - LD(mwl)
    else:
        ze = z - LD(mwl)
    kl = np.asarray(k, dtype=LD)
    deep = (2 * np.pi / np.asarray(k) > depth) | (np.asarray(k) * depth > 500.0)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(kl[None, :] * ze[:, None])
        px = e if np.all(deep) else np.where(deep, e, np.cosh(kl[None, :] * (ze[:, None] + LD(depth))) / np.sinh(kl * LD(depth))[None, :])
    amp = (np.asarray(w, dtype=LD) ** 2 * np.asarray(A, dtype=LD) / kl)[None, :] * px
    return eta[0], np.asarray((amp * np.cos(psi[0])).sum(axis=1), dtype=np.float64), np.asarray((np.abs(amp) * _share(mag[0])).sum(axis=1), dtype=np.float64)


@contextlib.contextmanager
def directional():
    """Inside the block, morison_ref.morison, nonlinear_ref.nonlinear and surface_clip_ref.clipped take five-entry component tuples:
    their kinematics callbacks (wk.kinematics, nonlinear_ref.dynamic_pressure_sum) are the sums of this file."""
    keep = wk.kinematics, nonlinear_ref.dynamic_pressure_sum
    wk.kinematics, nonlinear_ref.dynamic_pressure_sum = kinematics, dynamic_pressure_sum
    try:
        yield
    finally:
        wk.kinematics, nonlinear_ref.dynamic_pressure_sum = keep


def morison(comp, *a, **k):
    with directional():
        return morison_ref.morison(comp, *a, **k)


def nonlinear(comp, *a, **k):
    with directional():
        return nonlinear_ref.nonlinear(comp, *a, **k)


def clipped(comp, *a, **k):
    with directional():
        return surface_clip_ref.clipped(comp, *a, **k)


# ---- heading interpolation of the excitation coefficients (hc_set_excitation_rao_headings) ----
def rao_omega(w_grid, vals, omega, clamp=True):
    """The interpolator of hc_set_wave_irregular_spectral on one row: the list taken as uniform from its own spacing
    dw = w[-1] / nw, index = omega / dw - 1, linear between neighbours, held constant outside."""
    nw = len(w_grid)
    idx = np.asarray(omega, dtype=LD) / (LD(w_grid[-1]) / nw) - 1
    idx = np.clip(idx, 0, nw - 1)
    k0 = np.minimum(np.floor(idx).astype(int), max(nw - 2, 0))
    k1 = np.minimum(k0 + 1, nw - 1)
    v = np.asarray(vals, dtype=LD)
    return v[k0] + (idx - k0) * (v[k1] - v[k0])


def heading_tables(dirs, w_grid, mag, phase, omega, theta):
    """(magnitude, phase) [6][nf]: the omega interpolation at the two bracketing headings, then linear in the heading on the
    values as given.  mag, phase [6][n_dir][nw]; theta [nf] inside [dirs[0], dirs[-1]]."""
    dirs = np.asarray(dirs, dtype=np.float64)
    omega, theta = np.asarray(omega, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    assert np.all((theta >= dirs[0]) & (theta <= dirs[-1]))
    out = []
    for tab in (mag, phase):
        tab = np.asarray(tab, dtype=np.float64).reshape(6, len(dirs), len(w_grid))
        res = np.zeros((6, len(omega)), dtype=LD)
        for i, (om, th) in enumerate(zip(omega, theta)):
            j0 = int(np.searchsorted(dirs, th, side="right")) - 1
            j1 = min(j0 + 1, len(dirs) - 1)
            wt = LD(0) if j1 == j0 else (LD(th) - LD(dirs[j0])) / (LD(dirs[j1]) - LD(dirs[j0]))
            for r in range(6):
                v0, v1 = rao_omega(w_grid, tab[r, j0], om), rao_omega(w_grid, tab[r, j1], om)
                res[r, i] = v0 + wt * (v1 - v0)
        out.append(res)
    return out[0], out[1]
