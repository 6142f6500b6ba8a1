"""NumPy restatement of the second-order irregular waves of hc_wave_kinematics2 (Sharma and Dean 1981), written from the definition
in include/hydrochrono_amd.h / DESIGN.md 3.7f (TEST INFRASTRUCTURE ONLY).  np.longdouble by default, vectorised over the pairs.

Components (A, w, k, phi), g, depth h (may be inf).  R = w^2 / g, r = sqrt(R), b = A g / w; per pair and sign kappa = k_i +- k_j,
Omega = w_i +- w_j, Theta = theta_i +- theta_j, T = |kappa| tanh(|kappa| h):
    D+ = [(r_i + r_j)(r_i (k_j^2 - R_j^2) + r_j (k_i^2 - R_i^2)) + 2 (r_i + r_j)^2 (k_i k_j - R_i R_j)] / ((r_i + r_j)^2 - T)
    D- = [(r_i - r_j)(r_j (k_i^2 - R_i^2) - r_i (k_j^2 - R_j^2)) + 2 (r_i - r_j)^2 (k_i k_j + R_i R_j)] / ((r_i - r_j)^2 - T)
    K+- = (D+- - (k_i k_j -+ R_i R_j)) / (r_i r_j) + R_i + R_j,    B+- = b_i b_j D+- / (4 Omega),    D- = B- = 0 where w_i == w_j
(evaluated with R as the FP64 value of w^2 / g and delta = k - R: k^2 - R^2 = delta (k + R), k_i k_j - R_i R_j = k_i delta_j +
R_j delta_i, and K- = (D- - (k_i k_j - R_i R_j)) / (r_i r_j) + (r_i - r_j)^2, the same numbers without the cancellations)
    eta2 = 1/4 sum A_i A_j (K- cos(theta_i - theta_j) + K+ cos(theta_i + theta_j)),   phi2 = sum B C(kappa, z) sin Theta
    u2 = grad phi2,  a2 = d/dt grad phi2;  C = cosh(|kappa| (z + h)) / cosh(|kappa| h), S with sinh in the numerator
The fields are taken at z2 = min(z - mwl, 0), at -h below the bed.

Besides the values every function returns the scale of the tolerance: for a field, sum |term| over the pairs with each term's
magnitude taken over its phase; for a table entry, the sum of the |addends| it is built from, carried through its products and
quotients to first order (class _V: the magnitude of a + b is mag a + mag b, of a b it is mag a |b| + |a| mag b, ...), which is
what bounds the rounding error of any evaluation of the entry in units of the working precision.
"""
import numpy as np

INF = float("inf")
FULL = (0.0, INF)


class _V:
    """A value with the magnitude of the addends behind it."""

    def __init__(self, v, m=None):
        self.v = v
        self.m = np.abs(v) if m is None else m

    @staticmethod
    def of(x):
        return x if isinstance(x, _V) else _V(x)

    def __add__(self, o):
        o = _V.of(o)
        return _V(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        o = _V.of(o)
        return _V(self.v - o.v, self.m + o.m)

    def __mul__(self, o):
        o = _V.of(o)
        return _V(self.v * o.v, self.m * np.abs(o.v) + np.abs(self.v) * o.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _V.of(o)
        return _V(self.v / o.v, self.m / np.abs(o.v) + np.abs(self.v) * o.m / (o.v * o.v))

    def abs(self):
        return _V(np.abs(self.v), self.m)

    def sqrt(self):
        s = np.sqrt(self.v)
        return _V(s, s + 0.5 * self.m / s)

    def tanh(self):
        th = np.tanh(self.v)
        return _V(th, np.abs(th) + self.m * (1 - th * th))

    def where(self, keep):
        return _V(np.where(keep, self.v, 0), np.where(keep, self.m, 0))


def band_masks(w, diff_band=FULL, sum_band=FULL):
    """Which pairs take part: the comparison is made on the FP64 pair frequencies, as the library makes it."""
    w = np.asarray(w, dtype=np.float64)
    dm, sp = np.abs(w[:, None] - w[None, :]), w[:, None] + w[None, :]
    return (dm >= diff_band[0]) & (dm <= diff_band[1]), (sp >= sum_band[0]) & (sp <= sum_band[1])


def pair_tables(comp, g, depth, diff_band=FULL, sum_band=FULL, dtype=np.longdouble):
    """({Kp, Km, Bp, Bm}, {their sums of |addends|}), [nf][nf] each; zero outside the bands."""
    A, w, k = (np.asarray(v, dtype=dtype) for v in comp[:3])
    g = dtype(g)
    h = None if np.isinf(depth) else dtype(depth)
    in_diff, in_sum = band_masks(comp[1], diff_band, sum_band)
    col, row = (lambda v: _V(v[:, None])), (lambda v: _V(v[None, :]))
    wi, wj, ki, kj = col(w), row(w), col(k), row(k)
    # R = w^2 / g as the FP64 component data holds it, and delta = k - R (exact: the two are close), so that k^2 - R^2 and
    # k_i k_j - R_i R_j keep their relative accuracy where the water is deep for a component (delta -> 0)
    w64 = np.asarray(comp[1], dtype=np.float64)
    R = (w64 * w64 / np.float64(g)).astype(dtype)
    Ri, Rj, di, dj = col(R), row(R), col(k - R), row(k - R)
    ri, rj = Ri.sqrt(), Rj.sqrt()
    bb = (col(A) * g / wi) * (row(A) * g / wj) * dtype(0.25)
    kmR, kpR, rr = ki * dj + Rj * di, ki * kj + Ri * Rj, ri * rj  # k_i k_j -+ R_i R_j
    ni, nj = di * (ki + Ri), dj * (kj + Rj)                        # k^2 - R^2

    def T(kap):
        ak = kap.abs()
        return ak if h is None else ak * (ak * h).tanh()

    same = w64[:, None] == w64[None, :]
    rs, rd = ri + rj, ri - rj
    Dp = (rs * (ri * nj + rj * ni) + dtype(2) * (rs * rs) * kmR) / (rs * rs - T(ki + kj))
    with np.errstate(divide="ignore", invalid="ignore"):
        Dm = ((rd * (rj * ni - ri * nj) + dtype(2) * (rd * rd) * kpR) / (rd * rd - T(ki - kj))).where(~same)
        Bm = (bb * Dm / (wi - wj)).where(~same & in_diff)
    Kp = ((Dp - kmR) / rr + (Ri + Rj)).where(in_sum)
    Km = ((Dm - kmR) / rr + rd * rd).where(in_diff)  # (D- - (k_i k_j + R_i R_j)) / (r_i r_j) + R_i + R_j with R = r^2
    Bp = (bb * Dp / (wi + wj)).where(in_sum)
    out = dict(Kp=Kp, Km=Km, Bp=Bp, Bm=Bm)
    return {n: v.v for n, v in out.items()}, {n: v.m for n, v in out.items()}


def _profiles(ak, z, h):
    """C and S at |kappa| = ak, in the overflow-free form (both e^{|kappa| z} for an infinite depth)."""
    e = np.exp(ak * z)
    if h is None:
        return e, e
    q, d = np.exp(-2 * ak * (z + h)), 1 + np.exp(-2 * ak * h)
    return e * (1 + q) / d, e * (1 - q) / d


def ramp2(ramp_duration, t):
    """ramp * ramp of a synthesised irregular model (the Morison term's rule)."""
    t = np.asarray(t, dtype=np.float64)
    if not ramp_duration > 0.0:
        return np.ones_like(t)
    return np.where(t < ramp_duration, np.where(t <= 0.0, 0.0, t / ramp_duration) ** 2, 1.0)


def fields(comp, g, depth, points, times, mwl=0.0, diff_band=FULL, sum_band=FULL, ramp_duration=0.0, dtype=np.longdouble, clamp=True):
    """(eta2 [T][P], vel2 [T][P][3], acc2 [T][P][3], phi2 [T][P]) and the matching sums of |term|.  clamp=False evaluates the
    fields at z - mwl itself (for difference quotients across the mean level)."""
    tabs, _ = pair_tables(comp, g, depth, diff_band, sum_band, dtype)
    A, w, k, phi = (np.asarray(v, dtype=dtype) for v in comp)
    h = None if np.isinf(depth) else dtype(depth)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(times, dtype=np.float64).reshape(-1)
    T, P = t.size, pts.shape[0]
    AA = A[:, None] * A[None, :] * dtype(0.25)
    kap = {"m": k[:, None] - k[None, :], "p": k[:, None] + k[None, :]}
    Om = {"m": w[:, None] - w[None, :], "p": w[:, None] + w[None, :]}
    eta_scale = np.sum(AA * (np.abs(tabs["Km"]) + np.abs(tabs["Kp"])))
    r2 = ramp2(ramp_duration, t).astype(dtype)
    names = ("eta", "ux", "uz", "ax", "az", "phi")
    val = {n: np.zeros((T, P), dtype=dtype) for n in names}
    sca = {n: np.zeros((T, P), dtype=dtype) for n in names}
    per_z = {}
    for p in range(P):
        z2 = dtype(pts[p, 2] - np.float64(mwl))  # (the FP64 difference, as the library forms it: exactly -h at the bed)
        if clamp:
            z2 = min(z2, dtype(0))
            if h is not None:
                z2 = max(z2, -h)
        key = float(z2)
        if key not in per_z:
            cf = {}
            for s in "mp":
                ak = np.abs(kap[s])
                C, S = _profiles(ak, z2, h)
                B = tabs["B" + s]
                cf[s] = (B * C, B * kap[s] * C, B * ak * S)
            per_z[key] = cf
        cf = per_z[key]
        for j in range(T):
            th = k * dtype(pts[p, 0]) - w * dtype(t[j]) + phi
            c, s_ = np.cos(th), np.sin(th)
            cc, ss, sc = c[:, None] * c[None, :], s_[:, None] * s_[None, :], s_[:, None] * c[None, :]
            trig = {"m": (cc + ss, sc - sc.T), "p": (cc - ss, sc + sc.T)}  # cos and sin of theta_i -+ theta_j
            acc = dict.fromkeys(names, 0)
            mag = dict.fromkeys(names, 0)
            acc["eta"] = np.sum(AA * (tabs["Km"] * trig["m"][0] + tabs["Kp"] * trig["p"][0]))
            mag["eta"] = eta_scale
            for s in "mp":
                cosT, sinT = trig[s]
                bC, bkC, bkS = cf[s]
                for n, coef, ph in (("phi", bC, sinT), ("ux", bkC, cosT), ("uz", bkS, sinT), ("ax", bkC * Om[s], sinT),
                                    ("az", -bkS * Om[s], cosT)):
                    acc[n] = acc[n] + np.sum(coef * ph)
                    mag[n] = mag[n] + np.sum(np.abs(coef))
            for n in names:
                f = dtype(1) if n == "phi" else r2[j]
                val[n][j, p], sca[n][j, p] = acc[n] * f, mag[n] * f
    zero = np.zeros((T, P), dtype=dtype)
    pack = lambda d: (d["eta"], np.stack([d["ux"], zero, d["uz"]], axis=-1), np.stack([d["ax"], zero, d["az"]], axis=-1), d["phi"])
    return pack(val), pack(sca)


def first_order(comp, g, depth, x, z, t, dtype=np.longdouble):
    """(eta1, phi1) at one point and time: eta1 = sum A cos theta, phi1 = sum b cosh(k (z + h)) / cosh(k h) sin theta at z itself."""
    A, w, k, phi = (np.asarray(v, dtype=dtype) for v in comp)
    h = None if np.isinf(depth) else dtype(depth)
    th = k * dtype(x) - w * dtype(t) + phi
    C, _ = _profiles(k, dtype(z), h)
    return np.sum(A * np.cos(th)), np.sum(A * dtype(g) / w * C * np.sin(th))


def stokes_eta2(A, k, depth, theta):
    """Stokes' second-order elevation of one component with the set-down of a wave train in finite depth."""
    if np.isinf(depth):
        return 0.5 * k * A * A * np.cos(2 * theta)
    kh = k * depth
    return (k * A * A / 4 * np.cosh(kh) * (2 + np.cosh(2 * kh)) / np.sinh(kh) ** 3 * np.cos(2 * theta)
            - k * A * A / (2 * np.sinh(2 * kh)))
