"""NumPy restatement of the reference's wave kinematics, written from the formulas (TEST INFRASTRUCTURE ONLY).

Reference: src/wave_types.cpp:14-44 (eta), :61-158 (velocity, acceleration and their irregular sums), :301-313 (RegularWave),
:515-550 (IrregularWaves with Wheeler stretching).  Per component (A, w, k, phi) at x = position.x, z' = position.z - mwl:
    theta = k x - w t + phi,   eta = A cos(theta)
    exponential profile where 2 pi / k > depth or k depth > 500 (per component):  e^{k z'} for x and z
    otherwise cosh(k (z' + depth)) / sinh(k depth) for x, sinh(k (z' + depth)) / sinh(k depth) for z
    u = w A (p_x cos, 0, p_z sin),   a = w^2 A (p_x sin, 0, -p_z cos)
With stretching, z_s = depth (z' - eta) / (depth + eta) (the limit z' - eta for an infinite depth) is handed to the profiles, which
subtract mwl once more.  Besides the values, every function returns sum_i |term_i| per output element with each term's magnitude
taken over its phase (A_i for eta, w_i A_i |p_i| for a velocity component, ...): the scale of the tolerance.  (The phase itself carries
an absolute rounding error of a few ulp of |theta| in any FP64 evaluation, which a term near its zero crossing cannot scale down.)
"""
import numpy as np


def irregular_components(spec):
    """(A, w, k, phi) of an irregular model from hc_get_spectrum / orc_irreg_get_spectrum (:39-40)."""
    return np.sqrt(2 * spec["S"] * spec["df"]), 2 * np.pi * spec["f"], spec["k"], spec["phase"]


def regular_components(amplitude, omega, wavenumber, phase):
    return np.array([amplitude]), np.array([omega]), np.array([wavenumber]), np.array([phase])


def _theta(comp, x, t):
    A, w, k, phi = comp
    return k[None, None, :] * x[None, :, None] - w[None, None, :] * t[:, None, None] + phi[None, None, :]  # [T][P][nf]


def elevation(comp, points, times):
    """eta [T][P] and sum_i A_i (broadcast to [T][P])."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    terms = comp[0][None, None, :] * np.cos(_theta(comp, pts[:, 0], np.asarray(times, dtype=np.float64)))
    eta = terms.sum(axis=2)
    return eta, np.full(eta.shape, np.sum(np.abs(comp[0])))


def kinematics(comp, depth, points, times, mwl=0.0, stretching=False):
    """eta [T][P], vel [T][P][3], acc [T][P][3] and the matching sums of |term| (eta's, vel's, acc's)."""
    A, w, k, phi = comp
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(times, dtype=np.float64)
    eta, eta_scale = elevation(comp, pts, t)
    z = np.broadcast_to(pts[None, :, 2], eta.shape)
    if stretching:
        zr = z - mwl
        zs = (zr - eta) if np.isinf(depth) else depth * (zr - eta) / (depth + eta)
        ze = zs - mwl
    else:
        ze = z - mwl
    th = _theta(comp, pts[:, 0], t)
    s, c = np.sin(th), np.cos(th)
    deep = (2 * np.pi / k > depth) | (k * depth > 500.0)
    kk = k[None, None, :]
    zz = ze[:, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(kk * zz)
        if np.all(deep):
            px = pz = e
        else:
            q = kk * (zz + depth)
            sh = np.sinh(k * depth)[None, None, :]
            px = np.where(deep, e, np.cosh(q) / sh)
            pz = np.where(deep, e, np.sinh(q) / sh)
    wa, w2a = (w * A)[None, None, :], (w * w * A)[None, None, :]
    vel, acc = np.zeros(eta.shape + (3,)), np.zeros(eta.shape + (3,))
    vsc, asc = np.zeros_like(vel), np.zeros_like(acc)
    for col, prof, vph, aph in ((0, px, c, s), (2, pz, s, -c)):
        vel[..., col], vsc[..., col] = (wa * prof * vph).sum(axis=2), np.abs(wa * prof).sum(axis=2)
        acc[..., col], asc[..., col] = (w2a * prof * aph).sum(axis=2), np.abs(w2a * prof).sum(axis=2)
    return (eta, vel, acc), (eta_scale, vsc, asc)


def regimes(comp, depth):
    """How many components take the exponential profile because the wave is longer than the depth, how many the finite-depth
    profile, and how many the exponential one because k depth > 500."""
    _, _, k, _ = comp
    long_wave = 2 * np.pi / k > depth
    kd_big = ~long_wave & (k * depth > 500.0)
    return int(long_wave.sum()), int((~long_wave & ~kd_big).sum()), int(kd_big.sum())
