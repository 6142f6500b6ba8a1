"""NumPy restatement of the nonlinear buoyancy and Froude-Krylov forces on triangles clipped at the instantaneous free surface
(include/hydrochrono_amd.h: hc_set_surface_triangles), written from the definition on top of tests/wave_kinematics_ref.py and
nonlinear_ref.dynamic_pressure_sum (TEST INFRASTRUCTURE ONLY).  The frame algebra, the clipping and the sums run in longdouble; the
wave sums are float64 as wk's.

Per vertex j of a triangle v[3][3] of body b:
    R = Rx(rpy0) Ry(rpy1) Rz(rpy2),  d_j = R v_j,  P_j = pos + d_j
    eta_j, p_s,j = -rho g (P_j.z - mwl), p_d,j = ramp rho sum_i (w_i^2 A_i / k_i) px_i(z_e) cos theta_i: nonlinear_ref's, at P_j
    h_j = P_j.z - mwl - eta_j, wet iff h_j <= 0
h, p_s and p_d are linear over the triangle, the wet part is {h <= 0}: nothing (0 wet vertices), the sub-triangle (a, ab, ac) (1 wet
vertex a, b and c following cyclically), (a, b, bc) and (a, bc, ca) (dry vertex c, a and b following cyclically), the whole triangle
(3); xy lies on x -> y at s = h_x / (h_x - h_y), x the wet end.  Per sub-triangle (q0, q1, q2): S = 1/2 (q1 - q0) x (q2 - q0),
F = sum_m (-p_m S / 3), M = sum_m m x (-p_m S / 3) over the three edge midpoints m, p_m the mean of the two end values.

The error bound returned with the values (per body and component) is derived, not tuned.  With |p|_T the largest vertex magnitude
of a pressure on triangle T taken WITHOUT cancellation (|p_s| = rho g (|pos.z| + sum_k |R_2k| |v_k| + |mwl|),
|p_d| = ramp rho sum_i |(w_i^2 A_i / k_i) px_i|), |d|_T the largest vertex lever and n_j = sum_k |R_jk| |s_k| the triangle's area vector:
  * through p_d (nonlinear_ref): |delta p_d| <= KIN_TOL |p_d| at every vertex, hence at every interpolated point, on a wet part whose
    area vector is at most the triangle's: KIN_TOL |p_d|_T n_j into force component j, |d|_T times the Euclidean norm of that into
    the moment.  (p_s has no wave sum.)
  * rounding of the rotation, the interpolation, the cross products and the fixed-shape sum: (n_b + 64) 2^-52 sum_T |contribution_T|,
    a contribution taken without cancellation: |p|_T S~_j with S~ the area vector formed from edges |d_x| + |d_y| in place of
    d_y - d_x, every product in absolute value (the device forms the edges from rotated vertices, so their rounding scales with the
    levers, not with the edge); |d|_T times the Euclidean norm of that for the moment.
  * the cut: an error delta_eta <= KIN_TOL sum_i |A_i| in a vertex's eta, plus the rounding 8 * 2^-52 (|pos.z| + sum_k |R_2k| |v_k| +
    |mwl| + sum_i |A_i|) of h itself, moves a cut point by |delta s| <= delta_h / (h_y - h_x) (d s / d h_x and d s / d h_y are
    -h_y / (h_y - h_x)^2 and h_x / (h_y - h_x)^2, and |h_x| + |h_y| = h_y - h_x).  Each cut edge adds |delta s| |S_T| max_j |p_j| to
    every force component and that times |d|_T to every moment component, with the vertex pressures themselves.
"""
import numpy as np

import nonlinear_ref as nr
from morison_ref import EPS, KIN_TOL, LD, rotation


def _take(x, idx):
    """x [n][3](...) gathered along the vertex axis by idx [n]."""
    return x[np.arange(len(idx)), idx]


def _sub_triangle(q0, q1, q2):
    """(F, M) [n][3] each for p_s and p_d of the sub-triangles (q0, q1, q2); a vertex is (d [n][3], ps [n], pd [n])."""
    S3 = LD(0.5) * np.cross(q1[0] - q0[0], q2[0] - q0[0]) / LD(3)
    out = [np.zeros_like(S3) for _ in range(4)]
    for x, y in ((q0, q1), (q1, q2), (q2, q0)):
        m = LD(0.5) * (x[0] + y[0])
        for k in (1, 2):
            f = -(LD(0.5) * (x[k] + y[k]))[:, None] * S3
            out[2 * (k - 1)] = out[2 * (k - 1)] + f
            out[2 * (k - 1) + 1] = out[2 * (k - 1) + 1] + np.cross(m, f)
    return out


def _cut(x, y, hx, hy, use):
    """The point of x -> y where h = 0 (x wet: h_x <= 0 < h_y) for the triangles of `use`; x itself elsewhere (never read)."""
    s = np.where(use, hx / np.where(use, hx - hy, LD(1)), LD(0))
    return x[0] + s[:, None] * (y[0] - x[0]), x[1] + s * (y[1] - x[1]), x[2] + s * (y[2] - x[2])


def vertex_points(tris, pos, rpy):
    """World positions P [n][3][3] (float64) of every body's triangle vertices, as the kinematics are asked for them."""
    out = []
    for b, tl in enumerate(tris):
        if tl is None or len(tl) == 0:
            out.append(np.zeros((0, 3, 3)))
            continue
        R = rotation(np.asarray(rpy, dtype=np.float64).reshape(-1, 3)[b])
        d = np.asarray(tl, dtype=LD).reshape(-1, 3, 3) @ R.T
        out.append((np.asarray(pos, dtype=LD).reshape(-1, 3)[b] + d).astype(np.float64))
    return out


def clipped(comp, depth, rho, g, tris, t, pos, rpy, mwl=0.0, stretching=False, ramp=1.0):
    """tris: per body None or triangles [n][3][3].  comp: (A, w, k, phi) or None for still water.
    Returns dict(buoy [N][6], fk [N][6], bound_buoy [N][6], bound_fk [N][6], cases [N][4] = triangles with 0, 1, 2, 3 wet vertices,
    cut_span = min over cut edges of h_y - h_x (inf without a cut), points = per-body P [n][3][3], eta and h = per-body [n][3])."""
    pos, rpy = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy))
    N = pos.shape[0]
    buoy, fk, bb, bf = (np.zeros((N, 6)) for _ in range(4))
    cases = np.zeros((N, 4), dtype=int)
    cut_span = np.inf
    pts = vertex_points(tris, pos, rpy)
    etas, hs = [], []
    a_sum = LD(0) if comp is None else LD(np.sum(np.abs(comp[0])))
    for b in range(N):
        n = 0 if tris[b] is None else len(tris[b])
        if n == 0:
            etas.append(np.zeros((0, 3)))
            hs.append(np.zeros((0, 3)))
            continue
        v = np.asarray(tris[b], dtype=LD).reshape(n, 3, 3)
        R = rotation(rpy[b])
        aR = np.abs(R)
        d = v @ R.T
        P = pts[b]
        if comp is None:
            eta, pds, pabs = (np.zeros((n, 3)) for _ in range(3))
        else:
            eta, pds, pabs = (x.reshape(n, 3) for x in nr.dynamic_pressure_sum(comp, depth, P.reshape(-1, 3), t, mwl=mwl, stretching=stretching))
        h64 = P[:, :, 2] - mwl - eta
        etas.append(eta)
        hs.append(h64)
        wet = h64 <= 0.0
        nw = wet.sum(axis=1)
        cases[b] = [int(np.sum(nw == k)) for k in range(4)]
        h = h64.astype(LD)
        ps = -LD(rho) * LD(g) * (LD(pos[b, 2]) + d[:, :, 2] - LD(mwl))
        pd = LD(ramp) * LD(rho) * pds.astype(LD)
        # (A, B, C): the triangle turned so that A is the one wet vertex (1 wet) or C the one dry vertex (2 wet)
        r = np.where(nw == 1, np.argmax(wet, axis=1), np.where(nw == 2, (np.argmin(wet, axis=1) + 1) % 3, 0))
        A, B, C = ((_take(d, (r + j) % 3), _take(ps, (r + j) % 3), _take(pd, (r + j) % 3)) for j in range(3))
        hA, hB, hC = (_take(h, (r + j) % 3) for j in range(3))
        one, two, three = nw == 1, nw == 2, nw == 3
        ab, ac = _cut(A, B, hA, hB, one), _cut(A, C, hA, hC, one | two)
        bc = _cut(B, C, hB, hC, two)
        parts = ((three, _sub_triangle(A, B, C)), (one, _sub_triangle(A, ab, ac)), (two, _sub_triangle(A, B, bc)), (two, _sub_triangle(A, bc, ac)))
        tot = [np.zeros(3, dtype=LD) for _ in range(4)]
        for mask, sub in parts:
            for k in range(4):
                tot[k] = tot[k] + np.sum(np.where(mask[:, None], sub[k], 0), axis=0)
        buoy[b] = np.concatenate(tot[0:2]).astype(np.float64)
        fk[b] = np.concatenate(tot[2:4]).astype(np.float64)

        # ---- the bound ----
        hit = nw > 0  # a dry triangle contributes nothing and no error
        dlen = np.max(np.sqrt(np.sum(d * d, axis=2)), axis=1)
        s_body = LD(0.5) * np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        n_abs = np.abs(s_body) @ aR.T
        s_len = np.sqrt(np.sum(s_body * s_body, axis=1))
        ad = np.abs(d)
        e1, e2 = ad[:, 1] + ad[:, 0], ad[:, 2] + ad[:, 0]
        s_tilde = LD(0.5) * np.stack([e1[:, 1] * e2[:, 2] + e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] + e1[:, 0] * e2[:, 2],
                                      e1[:, 0] * e2[:, 1] + e1[:, 1] * e2[:, 0]], axis=1)
        z_abs = abs(LD(pos[b, 2])) + np.max(np.abs(v) @ aR[2], axis=1) + abs(LD(mwl))
        ps_abs = LD(rho) * LD(g) * z_abs
        pd_abs = LD(ramp) * LD(rho) * np.max(pabs, axis=1).astype(LD)
        # cut edges: (wet end, dry end) pairs of every triangle, their spans and delta s
        dh = KIN_TOL * a_sum + 8 * EPS * (z_abs + a_sum)
        ds = np.zeros(n, dtype=LD)
        for x, y in ((0, 1), (1, 2), (2, 0)):
            cutting = wet[:, x] != wet[:, y]
            span = np.abs(h[:, y] - h[:, x])
            if np.any(cutting):
                cut_span = min(cut_span, float(np.min(span[cutting])))
            ds = ds + np.where(cutting, dh / np.where(cutting, span, LD(1)), LD(0))
        for bound, pr_abs, pr, kin in ((bb, ps_abs, ps, None), (bf, pd_abs, pd, KIN_TOL * pd_abs)):
            mag_F = pr_abs[:, None] * s_tilde
            mag_M = (dlen * np.sqrt(np.sum(mag_F * mag_F, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
            mag = np.concatenate([np.sum(np.where(hit[:, None], mag_F, 0), axis=0), np.sum(np.where(hit[:, None], mag_M, 0), axis=0)])
            err = (n + 64) * EPS * mag
            if kin is not None:
                dF = kin[:, None] * n_abs
                dM = (dlen * np.sqrt(np.sum(dF * dF, axis=1)))[:, None] * np.ones((1, 3), dtype=LD)
                err = err + np.concatenate([np.sum(np.where(hit[:, None], dF, 0), axis=0), np.sum(np.where(hit[:, None], dM, 0), axis=0)])
            cF = ds * s_len * np.max(np.abs(pr), axis=1)
            err = err + np.concatenate([np.full(3, np.sum(cF)), np.full(3, np.sum(cF * dlen))])
            bound[b] = err.astype(np.float64)
    return dict(buoy=buoy, fk=fk, bound_buoy=bb, bound_fk=bf, cases=cases, cut_span=cut_span, points=pts, eta=etas, h=hs)
