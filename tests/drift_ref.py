"""NumPy restatement of the second-order wave drift forces (include/hydrochrono_amd.h: hc_set_drift_qtf), test
infrastructure.  There is no oracle counterpart: the reference has no second-order wave force.

The reference value is the DIRECT double sum over component pairs of the definition, in longdouble -- deliberately not the projected
O(nf + nq^2) form the device evaluates, so that the identity between the two is itself under test:

    inside_i  = Omega_0 <= w_i <= Omega_{nq-1};  m_i = largest m with Omega_m <= w_i, capped at nq - 2
    lambda_i  = (w_i - Omega_m) / (Omega_{m+1} - Omega_m);  W[i][m_i] = 1 - lambda_i, W[i][m_i + 1] = lambda_i
    theta_i   = k_i x - w_i t + phi_i
    mode 1    F_d = sum_i A_i^2 D_d(w_i),                                     D_d(w_i) = sum_m W[i][m] P_d[m][m]
    mode 2    F_d = sum_ij A_i A_j 1/2 (D_d(w_i) + D_d(w_j)) cos(theta_i - theta_j)
    mode 3    F_d = sum_ij A_i A_j [P_d(w_i, w_j) cos(theta_i - theta_j) - Q_d(w_i, w_j) sin(theta_i - theta_j)]
              P_d(w_i, w_j) = sum_mn W[i][m] W[j][n] P_d[m][n]
    all times ramp^2.

Bound per body and row (derived, not tuned).  With Abar_m = sum_i W[i][m] A_i:
    M_d (mode 3) = 2 sum_mn (|P_d[m][n]| + |Q_d[m][n]|) Abar_m Abar_n          (twice the sum of |pair term|, no cancellation)
    M_d (mode 2) = 2 (sum_m |D_m| Abar_m)(sum_m Abar_m)
    M_d (mode 1) = 2 sum_m |D_m| E_m,  E_m = sum_i W[i][m] A_i^2
    bound_d = ramp^2 (2 KIN_TOL + (nf + nq^2 + 64) 2^-52) M_d
KIN_TOL = 1e-11 is the per-term tolerance tests/morison_ref.py takes from tests/test_gpu_wave_kinematics.py for the device's sin / cos
of theta_i (argument rounding included): a phase error delta on theta_i changes each pair term by at most A_i A_j (|delta_i| +
|delta_j|) times the table value, hence 2 KIN_TOL of the sum of |pair term|.  The second part is the fixed-order summation over at most
nf + nq^2 terms (plus 64 for the interpolation weights and the products).  Three roundings of theta stay inside KIN_TOL only while
|theta_i| < 1e4 (1e4 * 3 * 2^-53 = 3.3e-12): asserted here."""
import numpy as np

from morison_ref import EPS, KIN_TOL, LD, ramp_factor  # noqa: F401  (ramp_factor: the tests' one import for the ramp rule)

THETA_MAX = 1e4


def cells(omega_grid, w):
    """inside [nf] bool, m [nf] int (cell of every component; 0 outside), lam [nf] float64 as the definition computes it."""
    g = np.asarray(omega_grid, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    nq = g.size
    assert nq >= 2 and np.all(np.diff(g) > 0)
    inside = (w >= g[0]) & (w <= g[-1])
    m = np.clip(np.searchsorted(g, w, side="right") - 1, 0, nq - 2)
    lam = np.where(inside, (w - g[m]) / (g[m + 1] - g[m]), 0.0)
    return inside, m, lam


def weights(omega_grid, w):
    """W [nf][nq] float64 (rows of components outside the grid are zero)."""
    inside, m, lam = cells(omega_grid, w)
    W = np.zeros((w.size, np.size(omega_grid)))
    i = np.nonzero(inside)[0]
    W[i, m[i]] = 1.0 - lam[i]
    W[i, m[i] + 1] = lam[i]
    return W


def _theta(comp, t, x):
    A, w, k, phi = (np.asarray(v, dtype=np.float64) for v in comp)
    th = k.astype(LD) * LD(x) - w.astype(LD) * LD(t) + phi.astype(LD)
    assert np.all(np.abs(th) < THETA_MAX), "the bound assumes |theta_i| < 1e4"
    return th


def bounds(comp, table, ramp=1.0):
    """{mode: bound [6]} for one body's table (Omega, P, Q or None)."""
    A, w = np.asarray(comp[0], dtype=np.float64), np.asarray(comp[1], dtype=np.float64)
    g, P, Q = table
    nq, nf = np.size(g), A.size
    P = np.abs(np.asarray(P, dtype=LD).reshape(6, nq, nq))
    Qa = np.zeros_like(P) if Q is None else np.abs(np.asarray(Q, dtype=LD).reshape(6, nq, nq))
    W = weights(g, w).astype(LD)
    Abar, E = W.T @ A.astype(LD), W.T @ (A.astype(LD) ** 2)
    D = np.stack([np.diagonal(P[d]) for d in range(6)])
    M = {1: 2 * (D @ E), 2: 2 * (D @ Abar) * Abar.sum(), 3: 2 * np.einsum("dmn,m,n->d", P + Qa, Abar, Abar)}
    fac = LD(ramp) ** 2 * (2 * KIN_TOL + (nf + nq * nq + 64) * EPS)
    return {mode: np.asarray(fac * M[mode], dtype=np.float64) for mode in (1, 2, 3)}


class PairSum:
    """The direct pair sum for one body's table over a component set: the interpolated P_d(w_i, w_j), Q_d(w_i, w_j) and D_d(w_i) are
    made once (longdouble, components inside the grid only), every force() is then one cos / sin of the nf_in^2 phase differences."""

    def __init__(self, comp, table):
        self.comp = tuple(np.asarray(v, dtype=np.float64) for v in comp)
        g, P, Q = table
        self.table = table
        nq = np.size(g)
        P = np.asarray(P, dtype=np.float64).reshape(6, nq, nq).astype(LD)
        Q = None if Q is None else np.asarray(Q, dtype=np.float64).reshape(6, nq, nq).astype(LD)
        inside, m, lam = cells(g, self.comp[1])
        self.idx = np.nonzero(inside)[0]
        m, lam = m[self.idx], lam[self.idx].astype(LD)
        w0, w1 = 1 - lam, lam

        def bilinear(T):
            return (np.multiply.outer(w0, w0) * T[:, m[:, None], m[None, :]] + np.multiply.outer(w0, w1) * T[:, m[:, None], m[None, :] + 1]
                    + np.multiply.outer(w1, w0) * T[:, m[:, None] + 1, m[None, :]] + np.multiply.outer(w1, w1) * T[:, m[:, None] + 1, m[None, :] + 1])

        self.Pij = bilinear(P)
        self.Qij = None if Q is None else bilinear(Q)
        self.Di = w0 * P[:, m, m] + w1 * P[:, m + 1, m + 1]  # [6][n_in]
        self.A = self.comp[0][self.idx].astype(LD)

    def force(self, t, x, ramp=1.0):
        """{mode: F [6] float64-rounded longdouble} at time t and body position x."""
        th = _theta(self.comp, t, x)[self.idx]
        dth = th[:, None] - th[None, :]
        c, AA = np.cos(dth), np.multiply.outer(self.A, self.A)
        F1 = self.Di @ (self.A ** 2)
        F2 = np.array([np.sum(AA * (0.5 * (self.Di[d][:, None] + self.Di[d][None, :])) * c) for d in range(6)], dtype=LD)
        F3 = np.array([np.sum(AA * self.Pij[d] * c) for d in range(6)], dtype=LD)
        if self.Qij is not None:
            s = np.sin(dth)
            F3 = F3 - np.array([np.sum(AA * self.Qij[d] * s) for d in range(6)], dtype=LD)
        r2 = LD(ramp) ** 2
        return {1: np.asarray(r2 * F1, dtype=np.float64), 2: np.asarray(r2 * F2, dtype=np.float64), 3: np.asarray(r2 * F3, dtype=np.float64)}


def projected(comp, table, t, x, mode, ramp=1.0):
    """The evaluation form of the device in float64: U_m, V_m, then the mode's short form.  [6]."""
    A, w, k, phi = (np.asarray(v, dtype=np.float64) for v in comp)
    g, P, Q = table
    nq = np.size(g)
    P = np.asarray(P, dtype=np.float64).reshape(6, nq, nq)
    W = weights(g, w)
    D = np.stack([np.diagonal(P[d]) for d in range(6)])
    if mode == 1:
        F = D @ (W.T @ (A * A))
    else:
        th = k * x - w * t + phi
        U, V = W.T @ (A * np.cos(th)), W.T @ (A * np.sin(th))
        if mode == 2:
            F = (D @ U) * U.sum() + (D @ V) * V.sum()
        else:
            F = np.einsum("dmn,mn->d", P, np.outer(U, U) + np.outer(V, V))
            if Q is not None:
                F = F - np.einsum("dmn,mn->d", np.asarray(Q, dtype=np.float64).reshape(6, nq, nq), np.outer(V, U) - np.outer(U, V))
    return F * (ramp * ramp)


def random_table(nq, seed, lo, hi, hermitian=False, scale=1e4):
    """A non-uniform grid on [lo, hi] and general (or Hermitian: P symmetric, Q antisymmetric) tables."""
    rng = np.random.default_rng(seed)
    g = np.sort(rng.uniform(lo, hi, size=nq))
    g[0], g[-1] = lo, hi
    assert np.all(np.diff(g) > 0)
    P, Q = rng.normal(0.0, scale, size=(6, nq, nq)), rng.normal(0.0, scale, size=(6, nq, nq))
    if hermitian:
        P, Q = 0.5 * (P + P.transpose(0, 2, 1)), 0.5 * (Q - Q.transpose(0, 2, 1))
    return g, P, Q
