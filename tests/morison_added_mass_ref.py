"""NumPy restatement of the strip members' added-mass matrix on the instantaneous wet length (include/hydrochrono_amd.h:
hc_set_morison_member_added_mass; DESIGN.md 3.7c'''), in longdouble, on top of tests/morison_members_ref.py (TEST INFRASTRUCTURE
ONLY): that file's kinematics (`_kin`), Gauss abscissae, node bound delta h_j and constants, and the lines of its cut and weights,
restated here because `members()` does not hand them out -- tests/test_morison_added_mass_ref_cpu.py holds the two together: the
inertia force of `members()` in a uniform fluid acceleration a, with cm = ca, equals M (a, 0) of this file on cut members.

Per Gauss point of a member (nodes, h_j, wet interval, sigma_g, w_g, D_g, d = R r_g and a^ = R (r1 - r0) / L as in that file):
    m_g = w_g rho ca (pi / 4) D_g^2,   P = I - a^ a^T,   S = [d]x  (S x = d x x)
    M_g = m_g [ P, -P S ; S P, -S P S ]
A member's matrix is the sum of its points, a body's the sum of its members.  `node_eta2` (per body None or the increments at the
body's nodes, members in index order) is taken off h_j before the cut, as the members on the second-order sea do.

The bound returned with it (per entry) is derived, not tuned, from parts 2 and 3 of the bound in morison_members_ref.py; there is no
kinematics part other than eta in the cut.  By block -- force/force, force/moment, moment/moment -- an entry of M_g / m_g is at
most g = (1, 2 |d|, 3 |d|^2) without cancellation (|S_ij| <= |d| and |a^_i (d x a^)_j| <= |d|; |d|^2 delta_ij, d_i d_j and
(d x a^)_i (d x a^)_j are each at most |d|^2).
  2. The cut.  delta h_j as in that file; sigma* moves by at most (delta h_x + delta h_y) / |h_x - h_y|, and the quadrature of the cut
     segment Q(sigma*) by at most (L / n)(f_mag + f_var) per unit of sigma*: f_mag = m' g at the far end of the segment (|d| of the
     larger point plus the segment length, the larger diameter), m' = rho ca (pi / 4) D^2 the load per length; f_var its change over
     the segment: g changes by at most (0, 2, 6 |d|) per metre, D by |d1 - d0| / n per segment.
  3. Sums and roundings.  (items + 64) 2^-52 times sum m_g g, items = the Gauss points of the body (of the member, for its row).
"""
import numpy as np

import morison_members_ref as mm
import morison_ref as mr

LD = np.longdouble
EPS = mm.EPS
KIN_TOL = mm.KIN_TOL
BLOCK = np.array([[0] * 3 + [1] * 3] * 3 + [[1] * 3 + [2] * 3] * 3)  # the power of |d| an entry carries


def cross_matrix(d):
    return np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]], dtype=LD)


def point_matrix(m_g, axis, d):
    """M_g from the definition"""
    P = np.eye(3, dtype=LD) - np.outer(axis, axis)
    S = cross_matrix(d)
    return m_g * np.block([[P, -P @ S], [S @ P, -S @ P @ S]])


def added_mass(comp, depth, rho, lists, ca, t, pos, rpy, mwl=0.0, node_eta2=None):
    """lists: per body None or the tuple of morison_members_ref.member_lists (cd and cm are not read); ca: per body None or (n,).
    comp: (A, w, k, phi), with a fifth entry theta for the directional sea, or None for still water.
    Returns dict(M [N][6][6], bound [N][6][6], members = per body [n][6][6], member_bound = per body [n][6][6], h = per body the h_j
    of its nodes (members in index order), margin = min |h_j| over all nodes, eta_bound = max delta h_j, clear = every node has
    |h_j| > delta h_j, cases = per body the set of segment cases met: 'wet', 'dry', 'cut0' (node j wet), 'cut1' (node j + 1 wet))."""
    pos, rpy = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy))
    N = pos.shape[0]
    M, bound = np.zeros((N, 6, 6)), np.zeros((N, 6, 6))
    per_member, per_member_bound, hs, cases = [], [], [], []
    margin, eta_bound, clear = np.inf, 0.0, True
    sumA = 0.0 if comp is None else float(np.sum(np.abs(comp[0])))
    for b in range(N):
        ml = lists[b]
        n = 0 if ml is None else len(ml[0])
        cab = np.zeros(n) if ca is None or ca[b] is None else np.broadcast_to(np.asarray(ca[b], dtype=np.float64), (n,))
        seen = set()
        cases.append(seen)
        rows, row_bound, hb = np.zeros((n, 6, 6), dtype=LD), np.zeros((n, 6, 6), dtype=LD), []
        cut_err, mag = np.zeros(3, dtype=LD), np.zeros(3, dtype=LD)
        items, node0 = 0, 0
        R = mr.rotation(rpy[b])
        pb = pos[b].astype(LD)
        for m in range(n):
            r0, r1 = ml[0][m].astype(LD), ml[1][m].astype(LD)
            d0, d1, ns, cam = LD(ml[2][m][0]), LD(ml[2][m][1]), int(ml[5][m]), LD(cab[m])
            e = r1 - r0
            L = np.sqrt(np.sum(e * e))
            axis = R @ (e / L)
            # ---- nodes (morison_members_ref.members) ----
            sj = np.arange(ns + 1, dtype=LD) / LD(ns)
            P64 = (pb + (r0[None, :] + sj[:, None] * e[None, :]) @ R.T).astype(np.float64)
            eta, _, _, esc, _, _ = mm._kin(comp, depth, P64, t, mwl, False)
            h = P64[:, 2].astype(LD) - LD(mwl) - eta.astype(LD)
            if node_eta2 is not None and node_eta2[b] is not None:
                h = h - np.asarray(node_eta2[b], dtype=np.float64)[node0:node0 + ns + 1].astype(LD)
            node0 += ns + 1
            dh = KIN_TOL * esc + 8 * EPS * (np.abs(P64[:, 2]) + abs(mwl) + sumA)
            margin = min(margin, float(np.min(np.abs(h))))
            eta_bound = max(eta_bound, float(np.max(dh)))
            clear = clear and bool(np.all(np.abs(h) > dh))
            hb.append(h.astype(np.float64))
            items += 2 * ns
            seg_len, Dmax = L / LD(ns), max(d0, d1)
            cI = LD(rho) * cam * (np.pi / LD(4))
            cut_m, mag_m = np.zeros(3, dtype=LD), np.zeros(3, dtype=LD)
            for j in range(ns):
                hx, hy = h[j], h[j + 1]
                w0, w1 = hx <= 0, hy <= 0
                if w0 and w1:
                    sa, sb, dsg = LD(0), LD(1), LD(0)
                    seen.add("wet")
                elif not (w0 or w1):
                    seen.add("dry")
                    continue
                else:
                    hw, hd = (hx, hy) if w0 else (hy, hx)
                    cut = hw / (hw - hd)
                    sa, sb = (LD(0), cut) if w0 else (LD(1) - cut, LD(1))
                    dsg = (dh[j] + dh[j + 1]) / abs(hw - hd)
                    seen.add("cut0" if w0 else "cut1")
                far = LD(0)
                for gq in (mm.G_LO, mm.G_HI):
                    s = (LD(j) + sa + (sb - sa) * gq) / LD(ns)
                    wg = LD(0.5) * (sb - sa) * L / LD(ns)
                    D = d0 + s * (d1 - d0)
                    d = R @ (r0 + s * e)
                    m_g = wg * cI * D * D
                    rows[m] += point_matrix(m_g, axis, d)
                    dl = np.sqrt(np.sum(d * d))
                    far = max(far, dl)
                    mag_m += m_g * np.array([1, 2 * dl, 3 * dl * dl], dtype=LD)
                far = far + seg_len
                f_mag = cI * Dmax * Dmax * np.array([1, 2 * far, 3 * far * far], dtype=LD)
                f_var = seg_len * cI * Dmax * Dmax * np.array([0, 2, 6 * far], dtype=LD) \
                    + (abs(d1 - d0) / LD(ns)) * cI * 2 * Dmax * np.array([1, 2 * far, 3 * far * far], dtype=LD)
                cut_m += dsg * seg_len * (f_mag + f_var)
            cut_err += cut_m
            mag += mag_m
            row_bound[m] = (cut_m + (2 * ns + 64) * EPS * mag_m)[BLOCK]
        per_member.append(rows.astype(np.float64))
        per_member_bound.append(row_bound.astype(np.float64))
        hs.append(np.concatenate(hb) if hb else np.zeros(0))
        M[b] = rows.sum(axis=0).astype(np.float64)
        bound[b] = ((cut_err + (items + 64) * EPS * mag)[BLOCK]).astype(np.float64)
    return dict(M=M, bound=bound, members=per_member, member_bound=per_member_bound, h=hs, margin=margin, eta_bound=eta_bound, clear=clear,
                cases=cases)
