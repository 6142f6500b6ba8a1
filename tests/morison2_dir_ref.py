"""NumPy restatement of the Morison term on the second-order sea in a short-crested sea (include/hydrochrono_amd.h:
hc_set_morison_second_order_directional), composed as tests/morison2_ref.py is (TEST INFRASTRUCTURE ONLY): the frame algebra of
tests/morison_ref.py, the first-order values and scales from tests/directional_ref.kinematics (float64 out of a longdouble sum),
the second-order increments and their sums of |term| from tests/wave2_dir_ref.fields, y components included.

Per element e of body b, with R, d, p, v_e of morison_ref and one direction beta_i per component:
    eta1, u1, a1 = the directional wave kinematics at p, t (mwl, stretching by eta1), u1 and a1 times `ramp`
    eta2, u2, a2 = wave2_dir_ref.fields at the same float64 p and t: mwl, the two bands, ramp * ramp through `ramp_duration`
    eta = eta1 + eta2, u_f = u1 + u2, a_f = a1 + a2 (three components each);  wet: p.z - mwl <= eta;  the force formula of morison_ref

The error bound is that of morison2_ref with these scales, nothing new: KIN_TOL (first-order scale + increment sum of |term|) for
every kinematic quantity -- directional_ref's scale already carries the share of the phase argument, so that KIN_TOL times it is the
bound tests/test_gpu_directional.py holds the first-order kinematics to, and KIN_TOL sum|term| is what
tests/test_gpu_wave_kinematics2_dir.py holds the increments to -- propagated to first order through the force and the rotations,
the moment with |d|; plus (n_e + 64) 2^-52 sum_e |contribution_e| with the magnitudes taken without cancellation.

`dtype`: the precision of the frame algebra and of the increments (np.longdouble; np.float64 for the self-check of
tests/test_morison2_dir_ref_cpu.py).  The first-order sums are directional_ref's either way.
"""
import numpy as np

import directional_ref as dr
import morison_ref as mr
import wave2_dir_ref as wd

LD = mr.LD
KIN_TOL = mr.KIN_TOL
EPS = mr.EPS
FULL = wd.FULL


def increments(comp, beta, g, depth, p, t, mwl=0.0, diff_band=FULL, sum_band=FULL, ramp_duration=0.0, dtype=LD):
    """(eta2 [n], u2 [n][3], a2 [n][3]) at the points p and the time t, and the matching sums of |term|."""
    (e, v, a, _), (es, vs, as_, _) = wd.fields(comp, beta, g, depth, p, [t], mwl=mwl, diff_band=diff_band, sum_band=sum_band,
                                               ramp_duration=ramp_duration, dtype=dtype)
    return (e[0], v[0], a[0]), (es[0], vs[0], as_[0])


def _rotation(rpy, dtype):
    return mr.rotation(rpy).astype(dtype) if dtype is not LD else mr.rotation(rpy)


def morison2_dir(comp, beta, g, depth, rho, elements, t, pos, rpy, linvel, angvel, mwl=0.0, stretching=False, ramp=1.0, diff_band=FULL,
                 sum_band=FULL, ramp_duration=0.0, dtype=LD):
    """comp: (A, w, k, phi); beta: one direction per component.  The other arguments and the result are those of
    morison2_ref.morison2: dict(F [N][6], bound [N][6], margin, wet, p, eta2, u2, a2 = per-body arrays)."""
    pos, rpy, linvel, angvel = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (pos, rpy, linvel, angvel))
    comp5 = dr.with_directions(comp, beta)
    N = pos.shape[0]
    F, bound = np.zeros((N, 6)), np.zeros((N, 6))
    margin, wets = np.inf, []
    pts = mr.element_points(elements, pos, rpy)  # (longdouble, rounded to float64: the points the kinematics are asked for)
    out2 = dict(eta2=[], u2=[], a2=[])
    half = dtype(0.5)
    for b in range(N):
        el = elements[b]
        n = 0 if el is None else len(el[0])
        if n == 0:
            wets.append(np.zeros(0, dtype=bool))
            for k, shape in (("eta2", (0,)), ("u2", (0, 3)), ("a2", (0, 3))):
                out2[k].append(np.zeros(shape))
            continue
        r, cd, cm = (np.asarray(x, dtype=dtype).reshape(-1, 3) for x in el)
        R = _rotation(rpy[b], dtype)
        aR = np.abs(R)
        d = r @ R.T
        p = pts[b]
        (e_, v_, a_), (_, vs_, as_) = dr.kinematics(comp5, depth, p, [t], mwl=mwl, stretching=stretching)
        eta, uf, af, usc, asc = e_[0], v_[0] * ramp, a_[0] * ramp, vs_[0] * ramp, as_[0] * ramp
        (eta2, u2, a2), (_, u2sc, a2sc) = increments(comp, beta, g, depth, p, t, mwl, diff_band, sum_band, ramp_duration, dtype)
        gap = (p[:, 2] - mwl - eta).astype(dtype) - eta2
        margin = min(margin, float(np.min(np.abs(gap))))
        wet = np.asarray(gap <= 0.0)
        wets.append(wet)
        w = angvel[b].astype(dtype)
        ve = linvel[b].astype(dtype) + np.cross(np.broadcast_to(w, d.shape), d)
        ve_abs = np.abs(linvel[b]).astype(dtype) + np.stack([np.abs(w[1] * d[:, 2]) + np.abs(w[2] * d[:, 1]),
                                                             np.abs(w[2] * d[:, 0]) + np.abs(w[0] * d[:, 2]),
                                                             np.abs(w[0] * d[:, 1]) + np.abs(w[1] * d[:, 0])], axis=1)
        u = (uf.astype(dtype) + u2 - ve) @ R  # rows: R^T q
        a = (af.astype(dtype) + a2) @ R
        drag = half * dtype(rho) * cd * np.abs(u) * u
        inert = dtype(rho) * cm * a
        Fe = (drag + inert) @ R.T
        Me = np.cross(d, Fe)
        # kinematics error: first order plus the increments
        du = (KIN_TOL * (usc.astype(dtype) + u2sc)) @ aR
        da = (KIN_TOL * (asc.astype(dtype) + a2sc)) @ aR
        dFe = (rho * cd * np.abs(u) * du + rho * cm * da) @ aR.T
        dlen = np.sqrt(np.sum(d * d, axis=1))
        dMe = (dlen * np.sqrt(np.sum(dFe * dFe, axis=1)))[:, None] * np.ones((1, 3), dtype=dtype)
        # magnitudes without cancellation
        U = (np.abs(uf).astype(dtype) + np.abs(u2) + ve_abs) @ aR
        A = (np.abs(af).astype(dtype) + np.abs(a2)) @ aR
        mag_F = (half * dtype(rho) * cd * U * U + dtype(rho) * cm * A) @ aR.T
        mag_M = (dlen * np.sqrt(np.sum(mag_F * mag_F, axis=1)))[:, None] * np.ones((1, 3), dtype=dtype)
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
