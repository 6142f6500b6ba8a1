"""NumPy restatement of the Morison term on the second-order sea (include/hydrochrono_amd.h: hc_set_morison_second_order), written
from its definition (TEST INFRASTRUCTURE ONLY): the frame algebra in longdouble as tests/morison_ref.py, the first-order kinematics
from tests/wave_kinematics_ref.py (float64), the second-order increments from tests/wave2_ref.fields (longdouble).

Per element e of body b, with R, d, p, v_e of morison_ref:
    eta1, u1, a1 = wave kinematics at p, t (mwl, stretching by eta1), u1 and a1 times `ramp`
    eta2, u2, a2 = wave2_ref.fields at the same float64 p and t: mwl, the two bands, ramp * ramp through `ramp_duration` (0: none);
                   held at z2 = min(z - mwl, 0) and at the bed, no stretching, the true depth
    eta = eta1 + eta2, u_f = u1 + u2, a_f = a1 + a2;  wet: p.z - mwl <= eta;  the force formula of morison_ref

The error bound (per body and component) is derived the way morison_ref derives its own:
  * kinematics: |delta q| <= 1e-11 sum|term| of every first-order quantity (tests/test_gpu_wave_kinematics.py) PLUS 1e-11 sum|term|
    of its increment (tests/test_gpu_wave_kinematics2.py; wave2_ref.fields returns those sums), propagated to first order through
    delta F_body,i = rho cd_i |u_i| delta u_i + rho cm_i delta a_i and the rotations, the moment with |d|;
  * summation and rotations: (n_e + 64) 2^-52 sum_e |contribution_e| with the magnitudes taken without cancellation, |u2| and |a2|
    now among them: U_i = sum_j |R_ji| (|u1_j| + |u2_j| + |v_e|_j), A_i = sum_j |R_ji| (|a1_j| + |a2_j|).
"""
import numpy as np

import morison_ref as mr
import wave2_ref as w2
import wave_kinematics_ref as wk

LD = mr.LD
KIN_TOL = mr.KIN_TOL  # the same figure for both orders
EPS = mr.EPS


def increments(comp, g, depth, p, t, mwl=0.0, diff_band=w2.FULL, sum_band=w2.FULL, ramp_duration=0.0):
    """(eta2 [n], u2 [n][3], a2 [n][3]) at the points p and the time t, and the matching sums of |term|; longdouble."""
    (e, v, a, _), (es, vs, as_, _) = w2.fields(comp, g, depth, p, [t], mwl=mwl, diff_band=diff_band, sum_band=sum_band,
                                               ramp_duration=ramp_duration)
    return (e[0], v[0], a[0]), (es[0], vs[0], as_[0])


def morison2(comp, g, depth, rho, elements, t, pos, rpy, linvel, angvel, mwl=0.0, stretching=False, ramp=1.0, diff_band=w2.FULL,
             sum_band=w2.FULL, ramp_duration=0.0):
    """elements: per body None or (r, cd_area, cm_vol), each (n, 3).  comp: (A, w, k, phi) or None for still water (no increments).
    ramp: the factor on u1 and a1; ramp_duration: > 0 applies ramp * ramp of wave2_ref.ramp2 to the increments.
    Returns dict(F [N][6], bound [N][6], margin = min |p.z - mwl - eta1 - eta2|, wet, p, eta2, u2, a2 = per-body arrays)."""
    pos, rpy, linvel, angvel = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy, linvel, angvel))
    N = pos.shape[0]
    F, bound = np.zeros((N, 6)), np.zeros((N, 6))
    margin, wets = np.inf, []
    pts = mr.element_points(elements, pos, rpy)
    out2 = dict(eta2=[], u2=[], a2=[])
    for b in range(N):
        el = elements[b]
        n = 0 if el is None else len(el[0])
        if n == 0:
            wets.append(np.zeros(0, dtype=bool))
            for k, shape in (("eta2", (0,)), ("u2", (0, 3)), ("a2", (0, 3))):
                out2[k].append(np.zeros(shape))
            continue
        r, cd, cm = (np.asarray(x, dtype=LD).reshape(-1, 3) for x in el)
        R = mr.rotation(rpy[b])
        aR = np.abs(R)
        d = r @ R.T
        p = pts[b]
        zero1, zero3 = np.zeros(n, dtype=LD), np.zeros((n, 3), dtype=LD)
        if comp is None:
            eta, uf, af, usc, asc = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
            (eta2, u2, a2), (_, u2sc, a2sc) = (zero1, zero3, zero3), (zero1, zero3, zero3)
        else:
            (e_, v_, a_), (_, vs_, as_) = wk.kinematics(comp, depth, p, [t], mwl=mwl, stretching=stretching)
            eta, uf, af, usc, asc = e_[0], v_[0] * ramp, a_[0] * ramp, vs_[0] * ramp, as_[0] * ramp
            (eta2, u2, a2), (_, u2sc, a2sc) = increments(comp, g, depth, p, t, mwl, diff_band, sum_band, ramp_duration)
        gap = (p[:, 2] - mwl - eta).astype(LD) - eta2
        margin = min(margin, float(np.min(np.abs(gap))))
        wet = np.asarray(gap <= 0.0)
        wets.append(wet)
        w = angvel[b].astype(LD)
        ve = linvel[b].astype(LD) + np.cross(np.broadcast_to(w, d.shape), d)
        ve_abs = np.abs(linvel[b]).astype(LD) + np.stack([np.abs(w[1] * d[:, 2]) + np.abs(w[2] * d[:, 1]),
                                                          np.abs(w[2] * d[:, 0]) + np.abs(w[0] * d[:, 2]),
                                                          np.abs(w[0] * d[:, 1]) + np.abs(w[1] * d[:, 0])], axis=1)
        u = (uf.astype(LD) + u2 - ve) @ R  # rows: R^T q
        a = (af.astype(LD) + a2) @ R
        drag = LD(0.5) * rho * cd * np.abs(u) * u
        inert = LD(rho) * cm * a
        Fe = (drag + inert) @ R.T
        Me = np.cross(d, Fe)
        # kinematics error: first order plus the increments
        du = (KIN_TOL * (usc.astype(LD) + u2sc)) @ aR
        da = (KIN_TOL * (asc.astype(LD) + a2sc)) @ aR
        dFe = (rho * cd * np.abs(u) * du + rho * cm * da) @ aR.T
        dlen = np.sqrt(np.sum(d * d, axis=1))
        dMe = (dlen * np.sqrt(np.sum(dFe * dFe, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
        # magnitudes without cancellation
        U = (np.abs(uf).astype(LD) + np.abs(u2) + ve_abs) @ aR
        A = (np.abs(af).astype(LD) + np.abs(a2)) @ aR
        mag_F = (LD(0.5) * rho * cd * U * U + rho * cm * A) @ aR.T
        mag_M = (dlen * np.sqrt(np.sum(mag_F * mag_F, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
        wl = wet[:, None]
        F[b, :3] = np.sum(np.where(wl, Fe, 0), axis=0).astype(np.float64)
        F[b, 3:] = np.sum(np.where(wl, Me, 0), axis=0).astype(np.float64)
        kin_err = np.concatenate([np.sum(np.where(wl, dFe, 0), axis=0), np.sum(np.where(wl, dMe, 0), axis=0)])
        mag = np.concatenate([np.sum(np.where(wl, mag_F, 0), axis=0), np.sum(np.where(wl, mag_M, 0), axis=0)])
        bound[b] = (kin_err + (n + 64) * EPS * mag).astype(np.float64)
        out2["eta2"].append(np.asarray(eta2, dtype=np.float64))
        out2["u2"].append(np.asarray(u2, dtype=np.float64))
        out2["a2"].append(np.asarray(a2, dtype=np.float64))
    return dict(F=F, bound=bound, margin=margin, wet=wets, p=pts, **out2)
