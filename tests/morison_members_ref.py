"""NumPy restatement of the Morison strip members (include/hydrochrono_amd.h: hc_set_morison_members; DESIGN.md 3.7c'), written from
the definition on top of tests/wave_kinematics_ref.py and tests/directional_ref.py (TEST INFRASTRUCTURE ONLY).  The frame algebra,
the cut and the quadrature run in longdouble; the kinematics are those files' (float64 sums / longdouble sums).

Per member (r0, r1, d0, d1, cd, cm, n_seg) of body b, with the state of hc_step and R = Rx Ry Rz, d = R r, p = pos + d,
v_e = linvel + angvel x d as tests/morison_ref.py has them:
    nodes    r_j = r0 + (j / n_seg)(r1 - r0),  P_j = pos + R r_j,  h_j = P_j.z - mwl - eta(P_j, t);  wet iff h_j <= 0
    segment  h linear in the local sigma in [0, 1]: wet part [0, 1], nothing, or one cut sigma* = h_x / (h_x - h_y) from the wet end x
             ([0, sigma*] when node j is wet, [1 - sigma*, 1] when node j + 1 is)
    points   sigma_g = sigma_a + (sigma_b - sigma_a)(1/2 -+ 1/(2 sqrt 3)),  w_g = 1/2 (sigma_b - sigma_a) L / n_seg,  L = |r1 - r0|
             s = (j + sigma_g) / n_seg,  r_g = r0 + s (r1 - r0),  D_g = d0 + s (d1 - d0)
             u_f, a_f = kinematics at p, t (mwl, stretching by the point's own eta), times `ramp`;  a^ = R (r1 - r0) / L
             q = u_f - v_e,  q_n = q - (q . a^) a^,  a_n = a_f - (a_f . a^) a^
             dF = w_g [1/2 rho cd D_g |q_n| q_n + rho cm (pi / 4) D_g^2 a_n],  dM = d x dF
A member's vector is the sum of its points, a body's the sum of its members.

The bound returned with it (per body and component) is derived, not tuned.  It has three parts.
  1. Kinematics.  tests/test_gpu_wave_kinematics.py and tests/test_gpu_directional.py establish |delta q| <= KIN_TOL * scale for
     every kinematic quantity (scale = the sums of |term| those files return).  The map q -> |q_n| q_n has the Jacobian
     |q_n| P + q_n q_n^T / |q_n| (P the projector normal to the axis) of norm 2 |q_n|, and a -> a_n has norm 1, so every force
     component of a point moves by at most  e_F = w_g [1/2 rho cd D 2 |q_n| |delta u|_2 + rho cm (pi / 4) D^2 |delta a|_2]  and every
     moment component by |d|_2 sqrt(3) e_F.
  2. The cut.  h_j carries delta h_j = KIN_TOL * scale_eta + 8 eps (|P.z| + |mwl| + sum |A|) (the elevation's bound and the rounding
     of the node itself).  With h_x <= 0 < h_y, sigma* = h_x / (h_x - h_y) moves by at most (delta h_x + delta h_y) / |h_x - h_y|
     (both partial derivatives are below 1 / |h_x - h_y| in size because 0 <= sigma* <= 1).  The quadrature of the cut segment is
     Q(sigma*) = sigma* (L / n) 1/2 [f(g_1) + f(g_2)] with the points g_i proportional to sigma*, so
     |dQ / d sigma*| <= (L / n) (f_mag + f_var): f_mag the load per length WITHOUT cancellation (below), f_var a bound of its change
     over the segment -- the kinematics change by at most k_max times their magnitude per metre (phase and profile together: 2 k_max
     for the squared drag, written out below), the body's own velocity by |angvel| per metre, the diameter by |d1 - d0| / n per
     segment.  Moments take |d|_2 sqrt(3), |d| the larger of the two points' plus the segment length.
  3. Sums and roundings.  (items + 64) 2^-52 times the magnitudes without cancellation, items = the body's Gauss points: the two
     serial sum levels add at most max_m items_m + members <= items + 2 roundings per component, and the rotations, the projection
     and the products a few ulp of the uncancelled magnitude each (the 64).  Per point: U = |(|u_f| + |linvel| + |angvel x d| by
     absolute products)|_2, A = |a_f|_2, f_mag = 1/2 rho cd D U^2 + rho cm (pi / 4) D^2 A, force magnitude w_g f_mag per component,
     moment magnitude |d|_2 sqrt(3) w_g f_mag.
A member's own row carries the same three parts accumulated over that member's points alone, with items_m = 2 n_seg_m (the row is
one serial sum of the member's points, at most items_m roundings, and the 64 are per point, not per sum): `member_bound`.
"""
import numpy as np

import directional_ref as dr
import morison_ref as mr
import wave_kinematics_ref as wk

LD = np.longdouble
KIN_TOL = mr.KIN_TOL
EPS = mr.EPS
G_LO = LD(0.5) - LD(1) / (LD(2) * np.sqrt(LD(3)))
G_HI = LD(0.5) + LD(1) / (LD(2) * np.sqrt(LD(3)))
SQRT3 = float(np.sqrt(3.0))


def _kin(comp, depth, pts, t, mwl, stretching):
    """eta [P], u_f [P][3], a_f [P][3] and their scales at float64 points; still water for comp None"""
    n = len(pts)
    if comp is None or n == 0:
        z1, z3 = np.zeros(n), np.zeros((n, 3))
        return z1, z3, z3, z1, z3, z3
    fn = dr.kinematics if len(comp) == 5 else wk.kinematics
    (e, v, a), (es, vs, as_) = fn(comp, depth, pts, [t], mwl=mwl, stretching=stretching)
    return e[0], v[0], a[0], es[0], vs[0], as_[0]


def member_lists(r0, r1, diameter, cd, cm, n_seg):
    """The tuple this file takes per body, from the arguments of HydroForces.set_morison_members"""
    r0, r1 = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (r0, r1))
    n = len(r0)
    dia = np.asarray(diameter, dtype=np.float64)
    dia = np.broadcast_to(dia[:, None] if dia.ndim == 1 else dia, (n, 2)).copy()
    cd, cm = (np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)).copy() for x in (cd, cm))
    return r0, r1, dia, cd, cm, np.broadcast_to(np.asarray(n_seg, dtype=int), (n,)).copy()


def members(comp, depth, rho, lists, t, pos, rpy, linvel, angvel, mwl=0.0, stretching=False, ramp=1.0):
    """lists: per body None or (r0 (n, 3), r1 (n, 3), diameter (n, 2), cd (n), cm (n), n_seg (n)).  comp: (A, w, k, phi), with a
    fifth entry theta for the directional sea, or None for still water.
    Returns dict(F [N][6], bound [N][6], members = per body [n][6], member_bound = per body [n][6], points = per body and member the
    Gauss points' (dF, dM) [2 x wet or cut segments][6] in index order, margin = min |h_j| over all nodes, eta_bound = max delta h_j,
    clear = every node has |h_j| > delta h_j, cases = per body the set of segment cases met: 'wet', 'dry', 'cut0' (node j wet),
    'cut1' (node j + 1 wet))."""
    pos, rpy, linvel, angvel = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy, linvel, angvel))
    N = pos.shape[0]
    F, bound = np.zeros((N, 6)), np.zeros((N, 6))
    per_member, per_member_bound, per_point, cases = [], [], [], []
    margin, eta_bound, clear = np.inf, 0.0, True
    sumA = 0.0 if comp is None else float(np.sum(np.abs(comp[0])))
    kmax = 0.0 if comp is None else float(np.max(np.abs(comp[2])))
    for b in range(N):
        ml = lists[b]
        n = 0 if ml is None else len(ml[0])
        seen = set()
        cases.append(seen)
        if n == 0:
            per_member.append(np.zeros((0, 6)))
            per_member_bound.append(np.zeros((0, 6)))
            per_point.append([])
            continue
        R = mr.rotation(rpy[b])
        pb = pos[b].astype(LD)
        w = angvel[b].astype(LD)
        wn = float(np.sqrt(np.sum(w * w)))
        rows, row_bound, pts = np.zeros((n, 6), dtype=LD), np.zeros((n, 6), dtype=LD), []
        kin_err, cut_err, mag = np.zeros(6, dtype=LD), np.zeros(6, dtype=LD), np.zeros(6, dtype=LD)
        items = 0
        for m in range(n):
            r0, r1 = ml[0][m].astype(LD), ml[1][m].astype(LD)
            d0, d1, cd, cm, ns = LD(ml[2][m][0]), LD(ml[2][m][1]), LD(ml[3][m]), LD(ml[4][m]), int(ml[5][m])
            e = r1 - r0
            L = np.sqrt(np.sum(e * e))
            axis = R @ (e / L)
            # ---- nodes ----
            sj = np.arange(ns + 1, dtype=LD) / LD(ns)
            P = pb + (r0[None, :] + sj[:, None] * e[None, :]) @ R.T
            P64 = P.astype(np.float64)
            eta, _, _, esc, _, _ = _kin(comp, depth, P64, t, mwl, False)
            h = P64[:, 2].astype(LD) - LD(mwl) - eta.astype(LD)
            dh = KIN_TOL * esc + 8 * EPS * (np.abs(P64[:, 2]) + abs(mwl) + sumA)
            margin = min(margin, float(np.min(np.abs(h))))
            eta_bound = max(eta_bound, float(np.max(dh)))
            clear = clear and bool(np.all(np.abs(h) > dh))
            # ---- wet intervals and Gauss points ----
            sg, wg, dsig = [], [], []
            for j in range(ns):
                hx, hy = h[j], h[j + 1]
                w0, w1 = hx <= 0, hy <= 0
                if w0 and w1:
                    sa, sb, dsg = LD(0), LD(1), 0.0
                    seen.add("wet")
                elif not (w0 or w1):
                    seen.add("dry")
                    continue
                else:
                    hw, hd = (hx, hy) if w0 else (hy, hx)
                    cut = hw / (hw - hd)
                    sa, sb = (LD(0), cut) if w0 else (LD(1) - cut, LD(1))
                    dsg = float((dh[j] + dh[j + 1]) / abs(hw - hd))
                    seen.add("cut0" if w0 else "cut1")
                for gq in (G_LO, G_HI):
                    sg.append((LD(j) + sa + (sb - sa) * gq) / LD(ns))
                    wg.append(LD(0.5) * (sb - sa) * L / LD(ns))
                    dsig.append(dsg)
            items += 2 * ns
            if not sg:
                pts.append(np.zeros((0, 6)))
                continue
            kin_m, cut_m, mag_m = np.zeros(6, dtype=LD), np.zeros(6, dtype=LD), np.zeros(6, dtype=LD)
            sg, wg, dsig = np.array(sg, dtype=LD), np.array(wg, dtype=LD), np.array(dsig)
            rg = r0[None, :] + sg[:, None] * e[None, :]
            D = d0 + sg * (d1 - d0)
            d = rg @ R.T
            p64 = (pb + d).astype(np.float64)
            _, uf, af, _, usc, asc = _kin(comp, depth, p64, t, mwl, stretching)
            uf, af, usc, asc = uf * ramp, af * ramp, usc * ramp, asc * ramp
            ve = linvel[b].astype(LD) + np.cross(np.broadcast_to(w, d.shape), d)
            ve_abs = np.abs(linvel[b]).astype(LD) + np.stack([np.abs(w[1] * d[:, 2]) + np.abs(w[2] * d[:, 1]),
                                                              np.abs(w[2] * d[:, 0]) + np.abs(w[0] * d[:, 2]),
                                                              np.abs(w[0] * d[:, 1]) + np.abs(w[1] * d[:, 0])], axis=1)
            q = uf.astype(LD) - ve
            qn = q - (q @ axis)[:, None] * axis[None, :]
            an = af.astype(LD) - (af.astype(LD) @ axis)[:, None] * axis[None, :]
            speed = np.sqrt(np.sum(qn * qn, axis=1))
            c1 = LD(0.5) * rho * cd * D
            c2 = LD(rho) * cm * (np.pi / LD(4)) * D * D
            dF = wg[:, None] * (c1[:, None] * speed[:, None] * qn + c2[:, None] * an)
            dM = np.cross(d, dF)
            rows[m, :3], rows[m, 3:] = dF.sum(axis=0), dM.sum(axis=0)
            pts.append(np.concatenate([dF, dM], axis=1).astype(np.float64))
            dlen = np.sqrt(np.sum(d * d, axis=1))
            # 1: kinematics
            du = np.sqrt(np.sum((KIN_TOL * usc) ** 2, axis=1))
            da = np.sqrt(np.sum((KIN_TOL * asc) ** 2, axis=1))
            eF = wg * (c1 * 2 * speed * du + c2 * da)
            kin_m[:3], kin_m[3:] = eF.sum(), (dlen * SQRT3 * eF).sum()
            kin_err += kin_m
            # 3: magnitudes without cancellation
            Uf = np.sqrt(np.sum(np.abs(uf) ** 2, axis=1)).astype(LD)
            U = np.sqrt(np.sum((np.abs(uf).astype(LD) + ve_abs) ** 2, axis=1))
            A = np.sqrt(np.sum(af * af, axis=1)).astype(LD)
            fmag = c1 * U * U + c2 * A
            mag_m[:3], mag_m[3:] = (wg * fmag).sum(), (dlen * SQRT3 * wg * fmag).sum()
            mag += mag_m
            # 2: the cut (every point of a cut segment carries its segment's delta sigma*; each segment is counted once, with
            # the larger of its two points' figures)
            Dmax, seg_len = max(d0, d1), L / LD(ns)
            cD, cI = LD(0.5) * rho * cd, LD(rho) * cm * (np.pi / LD(4))
            f_top = cD * Dmax * U * U + cI * Dmax * Dmax * A
            f_var = seg_len * (cD * Dmax * 2 * U * (kmax * Uf + wn) + cI * Dmax * Dmax * kmax * A) \
                + (abs(d1 - d0) / LD(ns)) * (cD * U * U + cI * 2 * Dmax * A)
            per_pt = dsig * seg_len * (f_top + f_var)
            arm = (dlen + seg_len) * SQRT3
            for i in range(0, len(sg), 2):
                cut_err[:3] += max(per_pt[i], per_pt[i + 1])
                cut_err[3:] += max(per_pt[i] * arm[i], per_pt[i + 1] * arm[i + 1])
                cut_m[:3] += max(per_pt[i], per_pt[i + 1])
                cut_m[3:] += max(per_pt[i] * arm[i], per_pt[i + 1] * arm[i + 1])
            row_bound[m] = kin_m + cut_m + (2 * ns + 64) * EPS * mag_m
        per_member.append(rows.astype(np.float64))
        per_member_bound.append(row_bound.astype(np.float64))
        per_point.append(pts)
        F[b] = rows.sum(axis=0).astype(np.float64)
        bound[b] = (kin_err + cut_err + (items + 64) * EPS * mag).astype(np.float64)
    return dict(F=F, bound=bound, members=per_member, member_bound=per_member_bound, points=per_point, margin=margin, eta_bound=eta_bound, clear=clear, cases=cases)
