"""NumPy restatement of the second-order sum-frequency wave forces (include/hydrochrono_amd.h: hc_set_sum_qtf), test
infrastructure.  There is no oracle counterpart: the reference has no second-order wave force.

The reference value is the DIRECT double sum over component pairs of the definition, in longdouble -- deliberately not the projected
O(nf + nq^2) form the device evaluates, so that the identity between the two is itself under test:

    inside_i, m_i, lambda_i, W[i][m]: those of tests/drift_ref.py (cells, weights), both grid ends inside
    theta_i   = k_i x - w_i t + phi_i
    F_s = ramp^2 sum_ij A_i A_j [P_s(w_i, w_j) cos(theta_i + theta_j) - Q_s(w_i, w_j) sin(theta_i + theta_j)]
          P_s(w_i, w_j) = sum_mn W[i][m] W[j][n] P_s[m][n], Q likewise

Bound per body and row (derived, not tuned).  With Abar_m = sum_i W[i][m] A_i:
    M_d     = 2 sum_mn (|P_s[m][n]| + |Q_s[m][n]|) Abar_m Abar_n              (twice the sum of |pair term|, no cancellation)
    bound_d = ramp^2 (2 KIN_TOL + (nf + nq^2 + 64) 2^-52) M_d
The derivation is that of tests/drift_ref.py with theta_i + theta_j in place of theta_i - theta_j: KIN_TOL = 1e-11 is the per-term
tolerance tests/morison_ref.py takes from tests/test_gpu_wave_kinematics.py for the device's sin / cos of theta_i (argument rounding
included); a phase error delta on theta_i changes cos or sin of (theta_i + theta_j) by at most |delta_i| + |delta_j|, hence each pair
term by that times its magnitude, hence 2 KIN_TOL of the sum of |pair term|.  The second part is the fixed-order summation over at
most nf + nq^2 terms (plus 64 for the interpolation weights and the products).  Three roundings of theta stay inside KIN_TOL only
while |theta_i| < 1e4 (1e4 * 3 * 2^-53 = 3.3e-12): asserted here."""
import numpy as np

from drift_ref import cells, random_table, weights  # noqa: F401  (the tests' one import for grids and tables)
from morison_ref import EPS, KIN_TOL, LD, ramp_factor  # noqa: F401  (ramp_factor: the tests' one import for the ramp rule)

THETA_MAX = 1e4


def _theta(comp, t, x):
    A, w, k, phi = (np.asarray(v, dtype=np.float64) for v in comp)
    th = k.astype(LD) * LD(x) - w.astype(LD) * LD(t) + phi.astype(LD)
    assert np.all(np.abs(th) < THETA_MAX), "the bound assumes |theta_i| < 1e4"
    return th


def bound(comp, table, ramp=1.0):
    """bound [6] for one body's table (Omega, P, Q or None)."""
    A, w = np.asarray(comp[0], dtype=np.float64), np.asarray(comp[1], dtype=np.float64)
    g, P, Q = table
    nq, nf = np.size(g), A.size
    P = np.abs(np.asarray(P, dtype=LD).reshape(6, nq, nq))
    Qa = np.zeros_like(P) if Q is None else np.abs(np.asarray(Q, dtype=LD).reshape(6, nq, nq))
    Abar = weights(g, w).astype(LD).T @ A.astype(LD)
    M = 2 * np.einsum("dmn,m,n->d", P + Qa, Abar, Abar)
    fac = LD(ramp) ** 2 * (2 * KIN_TOL + (nf + nq * nq + 64) * EPS)
    return np.asarray(fac * M, dtype=np.float64)


class PairSum:
    """The direct pair sum for one body's table over a component set: the interpolated P_s(w_i, w_j), Q_s(w_i, w_j) are made once
    (longdouble, components inside the grid only), every force() is then one cos / sin of the nf_in^2 phase sums."""

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
        self.A = self.comp[0][self.idx].astype(LD)

    def force(self, t, x, ramp=1.0):
        """F [6], float64-rounded longdouble, at time t and body position x."""
        th = _theta(self.comp, t, x)[self.idx]
        sth = th[:, None] + th[None, :]
        c, AA = np.cos(sth), np.multiply.outer(self.A, self.A)
        F = np.array([np.sum(AA * self.Pij[d] * c) for d in range(6)], dtype=LD)
        if self.Qij is not None:
            s = np.sin(sth)
            F = F - np.array([np.sum(AA * self.Qij[d] * s) for d in range(6)], dtype=LD)
        return np.asarray(LD(ramp) ** 2 * F, dtype=np.float64)


def projected(comp, table, t, x, ramp=1.0):
    """The evaluation form of the device in float64: U_m, V_m, then the sum-frequency signs.  [6]."""
    A, w, k, phi = (np.asarray(v, dtype=np.float64) for v in comp)
    g, P, Q = table
    nq = np.size(g)
    P = np.asarray(P, dtype=np.float64).reshape(6, nq, nq)
    W = weights(g, w)
    th = k * x - w * t + phi
    U, V = W.T @ (A * np.cos(th)), W.T @ (A * np.sin(th))
    F = np.einsum("dmn,mn->d", P, np.outer(U, U) - np.outer(V, V))
    if Q is not None:
        F = F - np.einsum("dmn,mn->d", np.asarray(Q, dtype=np.float64).reshape(6, nq, nq), np.outer(V, U) + np.outer(U, V))
    return F * (ramp * ramp)


def regular_closed_form(A, theta, P_ww, Q_ww):
    """A^2 [P_s(w, w) cos 2 theta - Q_s(w, w) sin 2 theta] for interpolated table values P_ww, Q_ww [6] (longdouble)."""
    th2 = 2 * LD(theta)
    return np.asarray(LD(A) ** 2 * (np.asarray(P_ww, dtype=LD) * np.cos(th2) - np.asarray(Q_ww, dtype=LD) * np.sin(th2)), dtype=np.float64)


def interp_diag(table, w):
    """(P_s(w, w), Q_s(w, w)) [6] each, longdouble, for one frequency inside the grid (Q = None: zeros)."""
    g, P, Q = table
    nq = np.size(g)
    inside, m, lam = cells(g, np.array([w]))
    assert inside.all()
    m, lam = int(m[0]), LD(lam[0])

    def at(T):
        T = np.asarray(T, dtype=np.float64).reshape(6, nq, nq).astype(LD)
        return ((1 - lam) ** 2 * T[:, m, m] + (1 - lam) * lam * (T[:, m, m + 1] + T[:, m + 1, m]) + lam ** 2 * T[:, m + 1, m + 1])

    return at(P), (np.zeros(6, dtype=LD) if Q is None else at(Q))
