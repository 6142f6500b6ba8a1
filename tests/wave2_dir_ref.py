"""NumPy restatement of the second-order irregular waves in a short-crested sea (hc_wave_kinematics2_dir), written from the
definition in include/hydrochrono_amd.h / DESIGN.md 3.7n (TEST INFRASTRUCTURE ONLY): the direct double sum over all (i, j), vectorised
over the pairs, np.longdouble by default.  The long-crested restatement is tests/wave2_ref.py; its _V (a value with the magnitude of
the addends behind it), band_masks, _profiles and ramp2 are used here as they are.

Components (A, w, k, phi) and one direction beta per component; (c, s) = (cos beta, sin beta) in FP64, as the library's host side
computes them once (they are the inputs of everything below, not beta).  theta_i = k_i (x c_i + y s_i) - w_i t + phi_i.
    sigma = sin^2((beta_i - beta_j) / 2) = 1/4 [(c_i - c_j)^2 + (s_i - s_j)^2],  tau = cos^2(...) = 1/4 [(c_i + c_j)^2 + (s_i + s_j)^2]
    gamma = cos(beta_i - beta_j) = tau - sigma,   q = k_i delta_j + R_j delta_i  (delta = k - R)
    k_i . k_j - R_i R_j = gamma q - 2 sigma R_i R_j,   k_i . k_j + R_i R_j = gamma q + 2 tau R_i R_j
    |kappa+-|^2 = (k_i +- k_j)^2 -+ 4 k_i k_j sigma = (k_i -+ k_j)^2 +- 4 k_i k_j tau   (the form whose second part is the smaller)
    D+-, B+- as in the definition;  K+- = (D+- - gamma q) / (r_i r_j) + 2 sigma r_i r_j + {R_i + R_j, (r_i - r_j)^2}
    eta2 = 1/4 sum A_i A_j (K- cos(theta_i - theta_j) + K+ cos(theta_i + theta_j)),   phi2 = sum B C(|kappa|, z) sin Theta
    u2 = grad phi2 (three components: kappa_x = k_i c_i +- k_j c_j, kappa_y with s),  a2 = d/dt grad phi2
Every function returns the scale of the tolerance beside the values, as tests/wave2_ref.py does.
"""
import numpy as np

import wave2_ref as w2

FULL = w2.FULL
_V = w2._V


def unit_vectors(beta, nf):
    """(c, s) in FP64 for the directions beta (None: the long-crested sea along +x)."""
    if beta is None:
        return np.ones(nf), np.zeros(nf)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    assert beta.size == nf
    return np.cos(beta), np.sin(beta)


def _pick(mask, a, b):
    return _V(np.where(mask, a.v, b.v), np.where(mask, a.m, b.m))


def _angles(c, s, dtype):
    """sigma, tau as _V [nf][nf] and the FP64 choice sigma <= 1/2 the library makes.  A difference (sum) of two FP64 numbers is an
    input with the relative rounding of one operation, so it enters with its own magnitude."""
    c, s = np.asarray(c, dtype=dtype), np.asarray(s, dtype=dtype)
    sq = lambda v: _V(v) * _V(v)
    sig = (sq(c[:, None] - c[None, :]) + sq(s[:, None] - s[None, :])) * dtype(0.25)
    tau = (sq(c[:, None] + c[None, :]) + sq(s[:, None] + s[None, :])) * dtype(0.25)
    c64, s64 = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    low = 0.25 * ((c64[:, None] - c64[None, :]) ** 2 + (s64[:, None] - s64[None, :]) ** 2) <= 0.5
    return sig, tau, low


def _kappa2(ki, kjs, sig, tau, low, dtype):
    """|k_i e_i + kjs e_j|^2, kjs = +-k_j (as _V)."""
    p, m, kk = ki + kjs, ki - kjs, ki * kjs * dtype(4)
    return _pick(low, p * p - kk * sig, m * m + kk * tau)


def pair_tables(comp, beta, g, depth, diff_band=FULL, sum_band=FULL, dtype=np.longdouble):
    """({Kp, Km, Bp, Bm}, {their sums of |addends|}), [nf][nf] each; zero outside the bands."""
    A, w, k = (np.asarray(v, dtype=dtype) for v in comp[:3])
    c, s = unit_vectors(beta, A.size)
    g = dtype(g)
    h = None if np.isinf(depth) else dtype(depth)
    in_diff, in_sum = w2.band_masks(comp[1], diff_band, sum_band)
    col, row = (lambda v: _V(v[:, None])), (lambda v: _V(v[None, :]))
    wi, wj, ki, kj = col(w), row(w), col(k), row(k)
    w64 = np.asarray(comp[1], dtype=np.float64)
    R = (w64 * w64 / np.float64(g)).astype(dtype)
    Ri, Rj, di, dj = col(R), row(R), col(k - R), row(k - R)
    ri, rj = Ri.sqrt(), Rj.sqrt()
    bb = (col(A) * g / wi) * (row(A) * g / wj) * dtype(0.25)
    sig, tau, low = _angles(c, s, dtype)
    gq, RR, rr = (tau - sig) * (ki * dj + Rj * di), Ri * Rj, ri * rj
    kmR, kpR = gq - sig * RR * dtype(2), gq + tau * RR * dtype(2)  # k_i . k_j -+ R_i R_j
    ni, nj = di * (ki + Ri), dj * (kj + Rj)                        # k^2 - R^2

    def T(ak):
        return ak if h is None else ak * (ak * h).tanh()

    same = w64[:, None] == w64[None, :]
    rs, rd = ri + rj, ri - rj
    with np.errstate(divide="ignore", invalid="ignore"):
        akp = _kappa2(ki, kj, sig, tau, low, dtype).sqrt()
        akm = _kappa2(ki, row(-k), sig, tau, low, dtype).sqrt()
        Dp = (rs * (ri * nj + rj * ni) + dtype(2) * (rs * rs) * kmR) / (rs * rs - T(akp))
        Dm = ((rd * (rj * ni - ri * nj) + dtype(2) * (rd * rd) * kpR) / (rd * rd - T(akm))).where(~same)
        Bm = (bb * Dm / (wi - wj)).where(~same & in_diff)
    two_s_rr = sig * rr * dtype(2)
    Kp = ((Dp - gq) / rr + two_s_rr + (Ri + Rj)).where(in_sum)
    Km = ((Dm - gq) / rr + two_s_rr + rd * rd).where(in_diff)
    Bp = (bb * Dp / (wi + wj)).where(in_sum)
    out = dict(Kp=Kp, Km=Km, Bp=Bp, Bm=Bm)
    return {n: v.v for n, v in out.items()}, {n: v.m for n, v in out.items()}


def pair_geometry(comp, beta, dtype=np.longdouble):
    """Per sign ("m", "p"): (|kappa|, kappa_x, kappa_y, Omega), [nf][nf] each."""
    _, w, k = (np.asarray(v, dtype=dtype) for v in comp[:3])
    c, s = unit_vectors(beta, k.size)
    sig, tau, low = _angles(c, s, dtype)
    kc, ks = k * c.astype(dtype), k * s.astype(dtype)
    out = {}
    for name, sg in (("m", dtype(-1)), ("p", dtype(1))):
        ak = np.sqrt(_kappa2(_V(k[:, None]), _V(sg * k[None, :]), sig, tau, low, dtype).v)
        out[name] = (ak, kc[:, None] + sg * kc[None, :], ks[:, None] + sg * ks[None, :], w[:, None] + sg * w[None, :])
    return out


def fields(comp, beta, g, depth, points, times, mwl=0.0, diff_band=FULL, sum_band=FULL, ramp_duration=0.0, dtype=np.longdouble, clamp=True):
    """(eta2 [T][P], vel2 [T][P][3], acc2 [T][P][3], phi2 [T][P]) and the matching sums of |term|.  clamp=False evaluates the
    fields at z - mwl itself (for difference quotients across the mean level)."""
    tabs, _ = pair_tables(comp, beta, g, depth, diff_band, sum_band, dtype)
    A, w, k, phi = (np.asarray(v, dtype=dtype) for v in comp)
    c, s = (v.astype(dtype) for v in unit_vectors(beta, A.size))
    h = None if np.isinf(depth) else dtype(depth)
    pts = np.asarray(points, dtype=dtype).reshape(-1, 3)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    T, P = t.size, pts.shape[0]
    AA = A[:, None] * A[None, :] * dtype(0.25)
    geo = pair_geometry(comp, beta, dtype)
    eta_scale = np.sum(AA * (np.abs(tabs["Km"]) + np.abs(tabs["Kp"])))
    r2 = w2.ramp2(ramp_duration, t).astype(dtype)
    names = ("eta", "ux", "uy", "uz", "ax", "ay", "az", "phi")
    val = {n: np.zeros((T, P), dtype=dtype) for n in names}
    sca = {n: np.zeros((T, P), dtype=dtype) for n in names}
    per_z = {}
    for p in range(P):
        z2 = dtype(np.float64(pts[p, 2]) - np.float64(mwl)) if clamp else pts[p, 2] - dtype(mwl)  # (the FP64 difference, as the library forms it)
        if clamp:
            z2 = min(z2, dtype(0))
            if h is not None:
                z2 = max(z2, -h)
        key = float(z2) if clamp else z2
        if key not in per_z:
            cf = {}
            for sgn in "mp":
                ak, kx, ky, Om = geo[sgn]
                C, S = w2._profiles(ak, z2, h)
                B = tabs["B" + sgn]
                bC, bS = B * C, B * ak * S
                # name -> (coefficient, 0: times cos Theta, 1: times sin Theta)
                cf[sgn] = {"phi": (bC, 1), "ux": (bC * kx, 0), "uy": (bC * ky, 0), "uz": (bS, 1), "ax": (bC * kx * Om, 1),
                           "ay": (bC * ky * Om, 1), "az": (-bS * Om, 0)}
            per_z[key] = cf
        cf = per_z[key]
        for j in range(T):
            th = k * (pts[p, 0] * c + pts[p, 1] * s) - w * dtype(t[j]) + phi
            cs, sn = np.cos(th), np.sin(th)
            cc, ss, sc = cs[:, None] * cs[None, :], sn[:, None] * sn[None, :], sn[:, None] * cs[None, :]
            trig = {"m": (cc + ss, sc - sc.T), "p": (cc - ss, sc + sc.T)}  # cos and sin of theta_i -+ theta_j
            acc = dict.fromkeys(names, 0)
            mag = dict.fromkeys(names, 0)
            acc["eta"] = np.sum(AA * (tabs["Km"] * trig["m"][0] + tabs["Kp"] * trig["p"][0]))
            mag["eta"] = eta_scale
            for sgn in "mp":
                for n, (coef, which) in cf[sgn].items():
                    acc[n] = acc[n] + np.sum(coef * trig[sgn][which])
                    mag[n] = mag[n] + np.sum(np.abs(coef))
            for n in names:
                f = dtype(1) if n == "phi" else r2[j]
                val[n][j, p], sca[n][j, p] = acc[n] * f, mag[n] * f
    pack = lambda d: (d["eta"], np.stack([d["ux"], d["uy"], d["uz"]], axis=-1), np.stack([d["ax"], d["ay"], d["az"]], axis=-1), d["phi"])
    return pack(val), pack(sca)


def first_order(comp, beta, g, depth, x, y, z, t, dtype=np.longdouble):
    """(eta1, phi1) at one point and time: eta1 = sum A cos theta, phi1 = sum b cosh(k (z + h)) / cosh(k h) sin theta at z itself."""
    A, w, k, phi = (np.asarray(v, dtype=dtype) for v in comp)
    c, s = (v.astype(dtype) for v in unit_vectors(beta, A.size))
    h = None if np.isinf(depth) else dtype(depth)
    th = k * (dtype(x) * c + dtype(y) * s) - w * dtype(t) + phi
    C, _ = w2._profiles(k, dtype(z), h)
    return np.sum(A * np.cos(th)), np.sum(A * dtype(g) / w * C * np.sin(th))

