"""NumPy restatement of the Morison term (include/hydrochrono_amd.h: hc_set_morison_elements), written from its definition on top of
tests/wave_kinematics_ref.py (TEST INFRASTRUCTURE ONLY).  The frame algebra runs in longdouble; the kinematics are wk's float64.

Per element e of body b (r, cd_area, cm_vol), with the state of hc_step:
    R = Rx(rpy0) Ry(rpy1) Rz(rpy2),  d = R r,  p = pos + d,  v_e = linvel + angvel x d
    eta, u_f, a_f = wave kinematics at p, t (mwl, stretching), u_f and a_f times `ramp`
    wet: p.z - mwl <= eta
    u = R^T (u_f - v_e),  a = R^T a_f,  F_body,i = 1/2 rho cd_i |u_i| u_i + rho cm_i a_i,  F = R F_body,  M = d x F
and the body's 6-vector is the sum over its elements.

The error bound returned with it (per body and component) is derived, not tuned:
  * tests/test_gpu_wave_kinematics.py establishes |delta q| <= 1e-11 sum_i |term_i| for every kinematic quantity q.  To first order
    through the force: delta F_body,i = rho cd_i |u_i| delta u_i + rho cm_i delta a_i with delta u_i = sum_j |R_ji| delta u_f,j (and
    likewise a), rotated back with |R|; the moment takes |d| times the Euclidean norm of that.
  * the fixed-order summation and the rotations' own rounding: (n_e + 64) 2^-52 sum_e |contribution_e|, where an element's
    contribution is taken WITHOUT cancellation -- U_i = sum_j |R_ji| (|u_f,j| + |linvel_j| + |angvel x d|_j by absolute products),
    A_i = sum_j |R_ji| |a_f,j|, m_i = 1/2 rho cd_i U_i^2 + rho cm_i A_i, rotated with |R|, times |d| for the moment: the rounding of
    u = R^T (u_f - v_e) is a few ulp of U_i, which the square turns into a few ulp of rho cd_i U_i^2 however small u_i itself is.
"""
import numpy as np

import wave_kinematics_ref as wk

LD = np.longdouble
KIN_TOL = 1e-11
EPS = 2.0 ** -52


def rotation(rpy):
    """R = Rx(a) Ry(b) Rz(c) in longdouble."""
    a, b, c = (LD(v) for v in rpy)
    sa, ca, sb, cb, sc, cc = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    one, zero = LD(1), LD(0)
    Rx = np.array([[one, zero, zero], [zero, ca, -sa], [zero, sa, ca]], dtype=LD)
    Ry = np.array([[cb, zero, sb], [zero, one, zero], [-sb, zero, cb]], dtype=LD)
    Rz = np.array([[cc, -sc, zero], [sc, cc, zero], [zero, zero, one]], dtype=LD)
    return Rx @ Ry @ Rz


def ramp_factor(t, ramp_duration):
    """The ramp of the spectral excitation: ramp_duration > 0 and t < ramp_duration: 0 for t <= 0, else t / ramp_duration; else 1."""
    if ramp_duration > 0.0 and t < ramp_duration:
        return 0.0 if t <= 0.0 else t / ramp_duration
    return 1.0


def element_points(elements, pos, rpy):
    """World positions p [n][3] of every body's elements (float64), as the kinematics are asked for them."""
    out = []
    for b, el in enumerate(elements):
        if el is None or len(el[0]) == 0:
            out.append(np.zeros((0, 3)))
            continue
        R = rotation(np.asarray(rpy, dtype=np.float64).reshape(-1, 3)[b])
        d = np.asarray(el[0], dtype=LD).reshape(-1, 3) @ R.T
        out.append((np.asarray(pos, dtype=LD).reshape(-1, 3)[b] + d).astype(np.float64))
    return out


def morison(comp, depth, rho, elements, t, pos, rpy, linvel, angvel, mwl=0.0, stretching=False, ramp=1.0):
    """elements: per body None or (r, cd_area, cm_vol), each (n, 3).  comp: (A, w, k, phi) or None for still water.
    Returns dict(F [N][6], bound [N][6], margin = min over wet-tested elements of |p.z - mwl - eta|, wet = per-body bool arrays)."""
    pos, rpy, linvel, angvel = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy, linvel, angvel))
    N = pos.shape[0]
    F, bound = np.zeros((N, 6)), np.zeros((N, 6))
    margin, wets = np.inf, []
    pts = element_points(elements, pos, rpy)
    for b in range(N):
        el = elements[b]
        n = 0 if el is None else len(el[0])
        if n == 0:
            wets.append(np.zeros(0, dtype=bool))
            continue
        r, cd, cm = (np.asarray(x, dtype=LD).reshape(-1, 3) for x in el)
        R = rotation(rpy[b])
        aR = np.abs(R)
        d = r @ R.T
        p = pts[b]
        if comp is None:
            eta, uf, af = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
            usc, asc = np.zeros((n, 3)), np.zeros((n, 3))
        else:
            (e_, v_, a_), (_, vs_, as_) = wk.kinematics(comp, depth, p, [t], mwl=mwl, stretching=stretching)
            eta, uf, af, usc, asc = e_[0], v_[0] * ramp, a_[0] * ramp, vs_[0] * ramp, as_[0] * ramp
        gap = p[:, 2] - mwl - eta
        margin = min(margin, float(np.min(np.abs(gap))))
        wet = gap <= 0.0
        wets.append(wet)
        w = angvel[b].astype(LD)
        ve = linvel[b].astype(LD) + np.cross(np.broadcast_to(w, d.shape), d)
        ve_abs = np.abs(linvel[b]).astype(LD) + np.stack([np.abs(w[1] * d[:, 2]) + np.abs(w[2] * d[:, 1]),
                                                          np.abs(w[2] * d[:, 0]) + np.abs(w[0] * d[:, 2]),
                                                          np.abs(w[0] * d[:, 1]) + np.abs(w[1] * d[:, 0])], axis=1)
        u = (uf.astype(LD) - ve) @ R          # rows: R^T q
        a = af.astype(LD) @ R
        drag = LD(0.5) * rho * cd * np.abs(u) * u
        inert = LD(rho) * cm * a
        Fe = (drag + inert) @ R.T
        Me = np.cross(d, Fe)
        # first-order kinematics error
        du = (KIN_TOL * usc).astype(LD) @ aR
        da = (KIN_TOL * asc).astype(LD) @ aR
        dFe = (rho * cd * np.abs(u) * du + rho * cm * da) @ aR.T
        dlen = np.sqrt(np.sum(d * d, axis=1))
        dMe = (dlen * np.sqrt(np.sum(dFe * dFe, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
        # magnitudes without cancellation
        U = (np.abs(uf).astype(LD) + ve_abs) @ aR
        A = np.abs(af).astype(LD) @ aR
        mag_F = (LD(0.5) * rho * cd * U * U + rho * cm * A) @ aR.T
        mag_M = (dlen * np.sqrt(np.sum(mag_F * mag_F, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
        wl = wet[:, None]
        F[b, :3] = np.sum(np.where(wl, Fe, 0), axis=0).astype(np.float64)
        F[b, 3:] = np.sum(np.where(wl, Me, 0), axis=0).astype(np.float64)
        kin_err = np.concatenate([np.sum(np.where(wl, dFe, 0), axis=0), np.sum(np.where(wl, dMe, 0), axis=0)])
        mag = np.concatenate([np.sum(np.where(wl, mag_F, 0), axis=0), np.sum(np.where(wl, mag_M, 0), axis=0)])
        bound[b] = (kin_err + (n + 64) * EPS * mag).astype(np.float64)
    return dict(F=F, bound=bound, margin=margin, wet=wets)
