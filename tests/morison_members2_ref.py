"""NumPy restatement of the Morison strip members on the second-order sea (include/hydrochrono_amd.h:
hc_set_morison_members_second_order; DESIGN.md 3.7c''), long- and short-crested (TEST INFRASTRUCTURE ONLY).  Built on the
restatements there are, not copied from them: the nodes, the cut, the quadrature, the force expression and the bound are
tests/morison_members_ref.members itself, run with another kinematics callback (its module-level `_kin`, the one place it asks for
the sea); the increments are tests/wave2_ref.fields (longdouble) or, for five-entry components, tests/wave2_dir_ref.fields.

What the callback returns at the float64 points it is asked for, with eta1, u1, a1 the first-order values members() asks for today
(mwl, stretching by the point's own eta1) and eta2, u2, a2 the increments at the same float64 points and time (mwl, the two bands,
ramp * ramp through `ramp_duration`; held at z2 = min(z - mwl, 0) and at the bed, the true depth, no stretching):
    eta = eta1 + eta2               -- members() forms h_j = P_j.z - mwl - eta from it: eta2 moves the cut
    u_f = ramp u1 + u2,  a_f = ramp a1 + a2   -- members() is run with ramp = 1: the factor is applied here, to order 1 alone
members() asks at the nodes first and then at the Gauss points the cut yields, so u2 and a2 are taken where the force is evaluated;
a dry segment has no Gauss point and is never asked for.

The bound is members()'s own derivation with the scales of the increments added where the first-order scales enter it:
  * nodes: delta h_j = KIN_TOL (sum|term| of eta1 + sum|term| of eta2) + 8 eps (...): tests/test_gpu_wave_kinematics2.py and
    tests/test_gpu_wave_kinematics2_dir.py establish 1e-11 sum|term| for eta2 as the first-order files do for eta1 (KIN_TOL is
    1e-11 for both orders, as in tests/morison2_ref.py), and the rounding of the one more subtraction, eps |eta2|, is far inside it;
  * Gauss points: |delta u| <= KIN_TOL (ramp sum|term| of u1 + sum|term| of u2), the same for a, propagated through the force
    expression by members() (the Jacobian 2 |q_n| of the drag, 1 of the inertia term, |d| sqrt 3 for the moment);
  * the change of the load along a cut segment (f_var): the second-order fields vary with wave numbers up to k_i + k_j <= 2 k_max,
    so members() is given components whose wave numbers are doubled FOR ITS BOUND ONLY (it reads k for k_max alone; the callback
    evaluates both orders from the true components);
  * sums and roundings: unchanged, with |u_f| and |a_f| the totals of both orders in the magnitudes.
"""
import numpy as np

import morison_members_ref as mm
import wave2_dir_ref as wd
import wave2_ref as w2

LD = np.longdouble
FULL = w2.FULL
KIN_TOL = mm.KIN_TOL


def increments(comp, g, depth, p, t, mwl=0.0, diff_band=FULL, sum_band=FULL, ramp_duration=0.0):
    """(eta2 [n], u2 [n][3], a2 [n][3]) at the points p and the time t, and the matching sums of |term|; longdouble.  comp with a
    fifth entry theta: the short-crested sea."""
    kw = dict(mwl=mwl, diff_band=diff_band, sum_band=sum_band, ramp_duration=ramp_duration)
    if len(comp) == 5:
        (e, v, a, _), (es, vs, as_, _) = wd.fields(comp[:4], comp[4], g, depth, p, [t], **kw)
    else:
        (e, v, a, _), (es, vs, as_, _) = w2.fields(comp, g, depth, p, [t], **kw)
    return (e[0], v[0], a[0]), (es[0], vs[0], as_[0])


def members2(comp, g, depth, rho, lists, t, pos, rpy, linvel, angvel, mwl=0.0, stretching=False, ramp=1.0, diff_band=FULL, sum_band=FULL,
             ramp_duration=0.0):
    """The arguments of morison_members_ref.members with g, the two bands and ramp_duration (> 0: ramp * ramp of wave2_ref.ramp2 on
    the increments) of morison2_ref.morison2.  Returns members()'s dict (F, bound, members, member_bound, points, margin, eta_bound,
    clear, cases -- h, the margin and the cases are those of eta1 + eta2) and, per body, over its members in index order:
        node_p [n][3], node_eta2 [n], node_h1 [n] = P.z - mwl - eta1, node_h [n] = node_h1 - eta2      n = sum (n_seg + 1)
        p [n][3], eta2 [n], u2 [n][3], a2 [n][3], wet [n]                                                  n = sum 2 n_seg
    (float64; the Gauss points of dry segments -- wet False -- carry zeros and no point)."""
    first = mm._kin
    log = []

    def kin2(_, depth_, pts, t_, mwl_, stretching_):
        eta, u, a, esc, usc, asc = first(comp, depth_, pts, t_, mwl_, stretching_)
        if comp is None or len(pts) == 0:
            return eta, u, a, esc, usc, asc
        (e2, u2, a2), (e2s, u2s, a2s) = increments(comp, g, depth_, pts, t_, mwl_, diff_band, sum_band, ramp_duration)
        log.append(dict(p=np.array(pts, dtype=np.float64), eta1=np.asarray(eta, dtype=np.float64), eta2=e2, u2=u2, a2=a2))
        return (eta.astype(LD) + e2, ramp * u.astype(LD) + u2, ramp * a.astype(LD) + a2,
                esc.astype(LD) + e2s, ramp * usc.astype(LD) + u2s, ramp * asc.astype(LD) + a2s)

    for_bound = None if comp is None else (comp[0], comp[1], 2.0 * np.asarray(comp[2]), *comp[3:])
    mm._kin = kin2
    try:
        ref = mm.members(for_bound, depth, rho, lists, t, pos, rpy, linvel, angvel, mwl=mwl, stretching=stretching, ramp=1.0)
    finally:
        mm._kin = first
    # ---- the increments in the layout of the two getters, from the calls in the order members() makes them ----
    calls = iter(log)
    keys = ("node_p", "node_eta2", "node_h1", "node_h", "p", "eta2", "u2", "a2", "wet")
    out = {k: [] for k in keys}
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    for b, ml in enumerate(lists):
        n = 0 if ml is None else len(ml[0])
        acc = {k: [] for k in keys}
        for m in range(n):
            ns = int(ml[5][m])
            if comp is None:
                raise ValueError("still water has no second-order part: use morison_members_ref.members")
            nodes = next(calls)
            assert len(nodes["p"]) == ns + 1
            h1 = nodes["p"][:, 2].astype(LD) - LD(mwl) - nodes["eta1"].astype(LD)
            h = h1 - nodes["eta2"]
            wet_node = h <= 0
            wet_seg = wet_node[:-1] | wet_node[1:]
            wet = np.repeat(wet_seg, 2)
            acc["node_p"].append(nodes["p"]), acc["node_eta2"].append(f64(nodes["eta2"])), acc["node_h1"].append(f64(h1)), acc["node_h"].append(f64(h))
            p, e2, u2, a2 = np.zeros((2 * ns, 3)), np.zeros(2 * ns), np.zeros((2 * ns, 3)), np.zeros((2 * ns, 3))
            if wet.any():
                pts = next(calls)
                assert len(pts["p"]) == int(wet.sum()) == len(ref["points"][b][m])
                p[wet], e2[wet], u2[wet], a2[wet] = pts["p"], f64(pts["eta2"]), f64(pts["u2"]), f64(pts["a2"])
            acc["p"].append(p), acc["eta2"].append(e2), acc["u2"].append(u2), acc["a2"].append(a2), acc["wet"].append(wet)
        for k in keys:
            width = {"node_p": (0, 3), "p": (0, 3), "u2": (0, 3), "a2": (0, 3)}.get(k, (0,))
            out[k].append(np.concatenate(acc[k]) if acc[k] else np.zeros(width, dtype=bool if k == "wet" else np.float64))
    assert next(calls, None) is None
    ref.update(out)
    return ref
