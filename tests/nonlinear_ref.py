"""NumPy restatement of the nonlinear buoyancy and Froude-Krylov forces on surface panels (include/hydrochrono_amd.h:
hc_set_surface_panels), written from the definition on top of tests/wave_kinematics_ref.py (TEST INFRASTRUCTURE ONLY).  The frame
algebra and the sums run in longdouble; the wave sums are float64 as wk's.

Per panel e of body b (centroid c, area vector s), with pos, rpy of hc_step:
    R = Rx(rpy0) Ry(rpy1) Rz(rpy2),  d = R c,  p = pos + d,  n = R s
    theta_i = k_i p.x - w_i t + phi_i,  eta = sum_i A_i cos theta_i;  wet: p.z - mwl <= eta
    p_s = -rho g (p.z - mwl)
    p_d = ramp rho sum_i (w_i^2 A_i / k_i) px_i(z_e) cos theta_i,  px_i and z_e those of the kinematics (stretching, second mwl)
    buoy_e = (-p_s n, d x (-p_s n)),  fk_e = (-p_d n, d x (-p_d n))
and a body's buoy and fk are the sums over its wet panels.

The error bound returned with them (per body and component) is derived, not tuned:
  * tests/test_gpu_wave_kinematics.py establishes |delta q| <= KIN_TOL sum_i |term_i| for every kinematic quantity q; p_d is one
    (the x-velocity sum with w A replaced by w^2 A / k), so |delta p_d| <= KIN_TOL ramp rho sum_i |(w_i^2 A_i / k_i) px_i|, which goes
    through |n_j| into the force and through |d| times the Euclidean norm of that into the moment.  (p_s has no wave sum.)
  * the fixed-shape sum, the rotation's and the cross product's own rounding: (n_b + 64) 2^-52 sum_e |contribution_e|, a panel's
    contribution taken WITHOUT cancellation: |p| |n_j| for a force component with |p_s| = rho g (|pos.z| + sum_j |R_2j| |c_j| + |mwl|)
    and |p_d| = ramp rho sum_i |(w_i^2 A_i / k_i) px_i|, |n_j| = sum_k |R_jk| |s_k|; |d| times the Euclidean norm of that for the
    moment.
"""
import numpy as np

import wave_kinematics_ref as wk
from morison_ref import EPS, KIN_TOL, LD, ramp_factor, rotation  # noqa: F401  (KIN_TOL is taken over, not tuned)


def triangles_to_panels(triangles):
    """c = (v0 + v1 + v2) / 3, s = 1/2 (v1 - v0) x (v2 - v0) of triangles [n][3][3]."""
    tri = np.asarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    return (tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3.0, 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])


def panel_points(panels, pos, rpy):
    """World positions p [n][3] of every body's panel centroids (float64), as the kinematics are asked for them."""
    out = []
    for b, pl in enumerate(panels):
        if pl is None or len(pl[0]) == 0:
            out.append(np.zeros((0, 3)))
            continue
        R = rotation(np.asarray(rpy, dtype=np.float64).reshape(-1, 3)[b])
        d = np.asarray(pl[0], dtype=LD).reshape(-1, 3) @ R.T
        out.append((np.asarray(pos, dtype=LD).reshape(-1, 3)[b] + d).astype(np.float64))
    return out


def dynamic_pressure_sum(comp, depth, points, t, mwl=0.0, stretching=False):
    """eta [P], sum_i (w_i^2 A_i / k_i) px_i cos theta_i [P] and sum_i |(w_i^2 A_i / k_i) px_i| [P] at one time: the x-velocity of
    wk.kinematics with the amplitudes w A replaced by w^2 A / k (same profiles, same z_e)."""
    A, w, k, phi = comp
    # wk.kinematics multiplies (w A) into the x-velocity: hand it amplitudes A' = w A / k, then w A' = w^2 A / k; eta needs the true A
    (eta, _, _), _ = wk.kinematics(comp, depth, points, [t], mwl=mwl, stretching=stretching)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    z = pts[:, 2]
    if stretching:
        zr = z - mwl
        zs = (zr - eta[0]) if np.isinf(depth) else depth * (zr - eta[0]) / (depth + eta[0])
        ze = zs - mwl
    else:
        ze = z - mwl
    th = k[None, :] * pts[:, 0][:, None] - w[None, :] * t + phi[None, :]
    deep = (2 * np.pi / k > depth) | (k * depth > 500.0)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(k[None, :] * ze[:, None])
        if np.all(deep):
            px = e
        else:
            px = np.where(deep, e, np.cosh(k[None, :] * (ze[:, None] + depth)) / np.sinh(k * depth)[None, :])
    amp = (w * w * A / k)[None, :] * px
    return eta[0], (amp * np.cos(th)).sum(axis=1), np.abs(amp).sum(axis=1)


def nonlinear(comp, depth, rho, g, panels, t, pos, rpy, mwl=0.0, stretching=False, ramp=1.0):
    """panels: per body None or (c, s), each (n, 3).  comp: (A, w, k, phi) or None for still water.
    Returns dict(buoy [N][6], fk [N][6], bound_buoy [N][6], bound_fk [N][6], margin = min over panels of |p.z - mwl - eta|,
    wet = per-body bool arrays)."""
    pos, rpy = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy))
    N = pos.shape[0]
    buoy, fk, bb, bf = (np.zeros((N, 6)) for _ in range(4))
    margin, wets = np.inf, []
    pts = panel_points(panels, pos, rpy)
    for b in range(N):
        pl = panels[b]
        n = 0 if pl is None else len(pl[0])
        if n == 0:
            wets.append(np.zeros(0, dtype=bool))
            continue
        c, s = (np.asarray(x, dtype=LD).reshape(-1, 3) for x in pl)
        R = rotation(rpy[b])
        aR = np.abs(R)
        d, nv = c @ R.T, s @ R.T
        p = pts[b]
        if comp is None:
            eta, pds, pabs = np.zeros(n), np.zeros(n), np.zeros(n)
        else:
            eta, pds, pabs = dynamic_pressure_sum(comp, depth, p, t, mwl=mwl, stretching=stretching)
        gap = p[:, 2] - mwl - eta
        margin = min(margin, float(np.min(np.abs(gap))))
        wet = gap <= 0.0
        wets.append(wet)
        wl = wet[:, None]
        pz = LD(pos[b, 2]) + d[:, 2]
        ps = -LD(rho) * LD(g) * (pz - LD(mwl))
        pd = LD(ramp) * LD(rho) * pds.astype(LD)
        dlen = np.sqrt(np.sum(d * d, axis=1))
        n_abs = np.abs(s) @ aR.T
        ps_abs = LD(rho) * LD(g) * (abs(LD(pos[b, 2])) + np.abs(c) @ aR[2] + abs(LD(mwl)))
        pd_abs = LD(ramp) * LD(rho) * pabs.astype(LD)
        for out, bound, pr, pr_abs, kin in ((buoy, bb, ps, ps_abs, None), (fk, bf, pd, pd_abs, KIN_TOL * pd_abs)):
            Fe = -pr[:, None] * nv
            Me = np.cross(d, Fe)
            mag_F = pr_abs[:, None] * n_abs
            mag_M = (dlen * np.sqrt(np.sum(mag_F * mag_F, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
            out[b, :3] = np.sum(np.where(wl, Fe, 0), axis=0).astype(np.float64)
            out[b, 3:] = np.sum(np.where(wl, Me, 0), axis=0).astype(np.float64)
            mag = np.concatenate([np.sum(np.where(wl, mag_F, 0), axis=0), np.sum(np.where(wl, mag_M, 0), axis=0)])
            err = (n + 64) * EPS * mag
            if kin is not None:
                dF = kin[:, None] * n_abs
                dM = (dlen * np.sqrt(np.sum(dF * dF, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
                err = err + np.concatenate([np.sum(np.where(wl, dF, 0), axis=0), np.sum(np.where(wl, dM, 0), axis=0)])
            bound[b] = err.astype(np.float64)
    return dict(buoy=buoy, fk=fk, bound_buoy=bb, bound_fk=bf, margin=margin, wet=wets)


def hs_linear(rho, gravity, bodies, pos, rpy):
    """The linear hydrostatic term: -rho |g| K_hs dq + the buoyancy force + the (cb - cg) x moment, and sum |term| per row.
    bodies: dicts with cg, cb, disp_vol, lin (6 x 6)."""
    pos, rpy = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy))
    gravity = np.asarray(gravity, dtype=np.float64)
    glen = np.sqrt(np.sum(gravity * gravity))
    out, scale = np.zeros((len(bodies), 6)), np.zeros((len(bodies), 6))
    for b, bd in enumerate(bodies):
        dq = np.concatenate([pos[b] - np.asarray(bd["cg"], dtype=float), rpy[b]])
        K = np.asarray(bd["lin"], dtype=float).reshape(6, 6)
        fb = rho * (-gravity) * bd["disp_vol"]
        r = np.asarray(bd["cb"], dtype=float) - np.asarray(bd["cg"], dtype=float)
        out[b] = -(rho * glen) * (K @ dq) + np.concatenate([fb, np.cross(r, fb)])
        cross_abs = np.array([abs(r[1] * fb[2]) + abs(r[2] * fb[1]), abs(r[2] * fb[0]) + abs(r[0] * fb[2]), abs(r[0] * fb[1]) + abs(r[1] * fb[0])])
        scale[b] = (rho * glen) * (np.abs(K) @ np.abs(dq)) + np.concatenate([np.abs(fb), cross_abs])
    return out, scale


# ---- meshes the tests share ----
def box_triangles(lo, hi, m=1, mz=None):
    """The closed box [lo, hi] (3-vectors) with m x m squares per face (mz rows along z on the four sides when given), every square
    split into two triangles, normals outward.  Returns [n][3][3]."""
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    mz = m if mz is None else mz
    tris = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        nu, nv = (mz if u == 2 else m), (mz if v == 2 else m)
        gu, gv = np.linspace(lo[u], hi[u], nu + 1), np.linspace(lo[v], hi[v], nv + 1)
        for side, w in ((1, hi[axis]), (-1, lo[axis])):
            for i in range(nu):
                for j in range(nv):
                    q = np.zeros((4, 3))
                    q[:, axis] = w
                    q[:, u] = [gu[i], gu[i + 1], gu[i + 1], gu[i]]
                    q[:, v] = [gv[j], gv[j], gv[j + 1], gv[j + 1]]
                    if side < 0:
                        q = q[::-1]
                    tris.append([q[0], q[1], q[2]])
                    tris.append([q[0], q[2], q[3]])
    return np.array(tris)
