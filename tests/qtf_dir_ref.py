"""NumPy restatement of the two QTF terms for tables on a heading x frequency grid (include/hydrochrono_amd.h:
hc_set_drift_qtf_headings, hc_set_sum_qtf_headings), test infrastructure.  There is no oracle counterpart: the reference
has no second-order wave force.

The reference value is the DIRECT double sum over component pairs of the definition, in longdouble, with the quadrilinear
interpolation of T(beta_a, beta_b, Omega_m, Omega_n) written out per pair -- deliberately not the projected O(nf + J^2) form the
device evaluates, so that the identity between the two is itself under test:

    a table is (beta [nh], Omega [nq], P [6][nh][nh][nq][nq], Q likewise or None); a component set is (A, w, k, phi, theta)
    inside_i, m_i, lambda_i: those of tests/drift_ref.py (cells); Wf[i][m_i] = 1 - lambda_i, Wf[i][m_i + 1] = lambda_i
    a_i = largest a with beta_a <= theta_i; mu_i = (theta_i - beta_a) / (beta_{a+1} - beta_a) (0 at the last heading);
    Wh[i][a_i] = 1 - mu_i, Wh[i][a_i + 1] = mu_i.  A component inside the frequency grid must have beta_0 <= theta_i <= beta_{nh-1}
    psi_i     = k_i (x cos theta_i + y sin theta_i) - w_i t + phi_i
    T(i, j)   = sum_{a,b,m,n} Wh[i][a] Wh[j][b] Wf[i][m] Wf[j][n] T[a][b][m][n]       (16 terms)
    D(i)      = sum_{a,m} Wh[i][a] Wf[i][m] P[a][a][m][m]                              (4 terms)
    drift 1   F_d = sum_i A_i^2 D_d(i)
    drift 2   F_d = sum_ij A_i A_j 1/2 (D_d(i) + D_d(j)) cos(psi_i - psi_j)
    drift 3   F_d = sum_ij A_i A_j [P_d(i, j) cos(psi_i - psi_j) - Q_d(i, j) sin(psi_i - psi_j)]
    sum       F_d = sum_ij A_i A_j [P_d(i, j) cos(psi_i + psi_j) - Q_d(i, j) sin(psi_i + psi_j)]
    all times ramp^2.

Bound per body and row: that of tests/drift_ref.py with nodes p = a nq + m for bins, J = nh nq of them.  With the node weight
W[i][p] = Wh[i][a] Wf[i][m], Abar_p = sum_i W[i][p] A_i and E_p = sum_i W[i][p] A_i^2:
    M_d (drift 3, sum) = 2 sum_pq (|P_d[p][q]| + |Q_d[p][q]|) Abar_p Abar_q
    M_d (drift 2)      = 2 (sum_p |D_p| Abar_p)(sum_p Abar_p),  D_p = P_d[a][a][m][m]
    M_d (drift 1)      = 2 sum_p |D_p| E_p
    bound_d = ramp^2 (2 KIN_TOL + (nf + J^2 + 64) 2^-52) M_d
KIN_TOL = 1e-11 stays the per-term tolerance of the device's sin / cos of psi_i: the phase now takes four roundings (x cos + y sin,
times k, minus w t, plus phi), and 1e4 * 4 * 2^-53 = 4.4e-12 < 1e-11 while |k| (|x cos| + |y sin|) + |w t| + |phi| < 1e4: asserted
here, as tests/directional_ref.py forms it."""
import itertools

import numpy as np

from drift_ref import cells
from morison_ref import EPS, KIN_TOL, LD, ramp_factor  # noqa: F401  (ramp_factor: the tests' one import for the ramp rule)

THETA_MAX = 1e4
KEYS = (1, 2, 3, "sum")


def head_cells(beta, theta):
    """a [n] int (largest a with beta_a <= theta), a1 [n] (its neighbour, a itself at the last heading), mu [n] float64 as the
    definition computes it, ok [n] bool (inside the grid)."""
    beta, theta = np.asarray(beta, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    nh = beta.size
    assert nh >= 1 and np.all(np.diff(beta) > 0)
    ok = (theta >= beta[0]) & (theta <= beta[-1])
    a = np.clip(np.searchsorted(beta, theta, side="right") - 1, 0, nh - 1)
    a1 = np.minimum(a + 1, nh - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.where(ok & (a1 > a), (theta - beta[a]) / np.where(a1 > a, beta[a1] - beta[a], 1.0), 0.0)
    return a, a1, mu, ok


def node_weights(table, w, theta):
    """W [nf][J] float64, node p = a nq + m (rows of components outside the frequency grid are zero)."""
    beta, g = table[0], table[1]
    nq, nh = np.size(g), np.size(beta)
    inside, m, lam = cells(g, w)
    a, a1, mu, ok = head_cells(beta, theta)
    assert np.all(ok[inside]), "a component inside the frequency grid lies outside the heading grid"
    W = np.zeros((np.size(w), nh * nq))
    for i in np.nonzero(inside)[0]:
        for aa, hw in ((a[i], 1.0 - mu[i]), (a1[i], mu[i])):
            for mm, fw in ((m[i], 1.0 - lam[i]), (m[i] + 1, lam[i])):
                W[i, aa * nq + mm] += hw * fw
    return W


def node_matrix(T, nh, nq):
    """[6][nh][nh][nq][nq] -> [6][J][J] with node p = a nq + m"""
    return np.asarray(T).reshape(6, nh, nh, nq, nq).transpose(0, 1, 3, 2, 4).reshape(6, nh * nq, nh * nq)


def _psi(comp, t, x, y):
    A, w, k, phi, th = (np.asarray(v, dtype=np.float64).astype(LD) for v in comp)
    c, s = np.cos(th), np.sin(th)
    x, y, t = LD(x), LD(y), LD(t)
    mag = np.abs(k) * (np.abs(x * c) + np.abs(y * s)) + np.abs(w * t) + np.abs(phi)
    assert np.all(mag < THETA_MAX), "the bound assumes |k| (|x cos| + |y sin|) + |w t| + |phi| < 1e4"
    return k * (x * c + y * s) - w * t + phi


def bounds(comp, table, ramp=1.0):
    """{1, 2, 3: the drift modes, "sum": the sum term} -> bound [6] for one body's table."""
    A, w, theta = (np.asarray(comp[i], dtype=np.float64) for i in (0, 1, 4))
    beta, g, P, Q = table
    nh, nq, nf = np.size(beta), np.size(g), A.size
    J = nh * nq
    Pn = np.abs(node_matrix(np.asarray(P, dtype=LD), nh, nq))
    Qn = np.zeros_like(Pn) if Q is None else np.abs(node_matrix(np.asarray(Q, dtype=LD), nh, nq))
    W = node_weights(table, w, theta).astype(LD)
    Abar, E = W.T @ A.astype(LD), W.T @ (A.astype(LD) ** 2)
    D = np.stack([np.diagonal(Pn[d]) for d in range(6)])
    M3 = 2 * np.einsum("dpq,p,q->d", Pn + Qn, Abar, Abar)
    M = {1: 2 * (D @ E), 2: 2 * (D @ Abar) * Abar.sum(), 3: M3, "sum": M3}
    fac = LD(ramp) ** 2 * (2 * KIN_TOL + (nf + J * J + 64) * EPS)
    return {key: np.asarray(fac * M[key], dtype=np.float64) for key in KEYS}


class PairSum:
    """The direct pair sum for one body's table over a component set: the interpolated P(i, j), Q(i, j) and D(i) are made once
    (longdouble, components inside the frequency grid only), every force() is then one cos / sin of the phase differences and sums."""

    def __init__(self, comp, table):
        self.comp = tuple(np.asarray(v, dtype=np.float64) for v in comp)
        beta, g, P, Q = table
        self.table = table
        nh, nq = np.size(beta), np.size(g)
        P = np.asarray(P, dtype=np.float64).reshape(6, nh, nh, nq, nq).astype(LD)
        Q = None if Q is None else np.asarray(Q, dtype=np.float64).reshape(6, nh, nh, nq, nq).astype(LD)
        inside, m, lam = cells(g, self.comp[1])
        a, a1, mu, ok = head_cells(beta, self.comp[4])
        assert np.all(ok[inside]), "a component inside the frequency grid lies outside the heading grid"
        self.idx = np.nonzero(inside)[0]
        m, lam, a, a1, mu = m[self.idx], lam[self.idx].astype(LD), a[self.idx], a1[self.idx], mu[self.idx].astype(LD)
        hs, hw = (a, a1), (1 - mu, mu)      # the two headings of a component and their weights
        fs, fw = (m, m + 1), (1 - lam, lam)  # the two frequencies

        def quadrilinear(T):
            out = np.zeros((6, m.size, m.size), dtype=LD)
            for da, db, dm, dn in itertools.product((0, 1), repeat=4):
                wi, wj = hw[da] * fw[dm], hw[db] * fw[dn]
                out += np.multiply.outer(wi, wj) * T[:, hs[da][:, None], hs[db][None, :], fs[dm][:, None], fs[dn][None, :]]
            return out

        self.Pij = quadrilinear(P)
        self.Qij = None if Q is None else quadrilinear(Q)
        self.Di = np.zeros((6, m.size), dtype=LD)
        for da, dm in itertools.product((0, 1), repeat=2):
            self.Di += hw[da] * fw[dm] * P[:, hs[da], hs[da], fs[dm], fs[dm]]
        self.A = self.comp[0][self.idx].astype(LD)

    def force(self, t, x, y, ramp=1.0):
        """{1, 2, 3, "sum": F [6] float64-rounded longdouble} at time t and body position (x, y)."""
        psi = _psi(self.comp, t, x, y)[self.idx]
        AA = np.multiply.outer(self.A, self.A)
        dif, tot = psi[:, None] - psi[None, :], psi[:, None] + psi[None, :]
        c = np.cos(dif)
        F = {1: self.Di @ (self.A ** 2),
             2: np.array([np.sum(AA * (0.5 * (self.Di[d][:, None] + self.Di[d][None, :])) * c) for d in range(6)], dtype=LD)}
        for key, arg in ((3, dif), ("sum", tot)):
            ca = np.cos(arg)
            F[key] = np.array([np.sum(AA * self.Pij[d] * ca) for d in range(6)], dtype=LD)
            if self.Qij is not None:
                sa = np.sin(arg)
                F[key] = F[key] - np.array([np.sum(AA * self.Qij[d] * sa) for d in range(6)], dtype=LD)
        r2 = LD(ramp) ** 2
        return {key: np.asarray(r2 * F[key], dtype=np.float64) for key in KEYS}


def projected(comp, table, t, x, y, key, ramp=1.0):
    """The evaluation form of the device in float64: U_p, V_p over the nodes, then the short form of `key`.  [6]."""
    A, w, k, phi, th = (np.asarray(v, dtype=np.float64) for v in comp)
    beta, g, P, Q = table
    nh, nq = np.size(beta), np.size(g)
    Pn = node_matrix(np.asarray(P, dtype=np.float64), nh, nq)
    W = node_weights(table, w, th)
    D = np.stack([np.diagonal(Pn[d]) for d in range(6)])
    if key == 1:
        F = D @ (W.T @ (A * A))
    else:
        psi = k * (x * np.cos(th) + y * np.sin(th)) - w * t + phi
        U, V = W.T @ (A * np.cos(psi)), W.T @ (A * np.sin(psi))
        sg = -1.0 if key == "sum" else 1.0
        if key == 2:
            F = (D @ U) * U.sum() + (D @ V) * V.sum()
        else:
            F = np.einsum("dpq,pq->d", Pn, np.outer(U, U) + sg * np.outer(V, V))
            if Q is not None:
                F = F - np.einsum("dpq,pq->d", node_matrix(np.asarray(Q, dtype=np.float64), nh, nq), np.outer(V, U) - sg * np.outer(U, V))
    return F * (ramp * ramp)


def random_table(nh, nq, seed, blo, bhi, lo, hi, scale=1e4, with_q=True):
    """Non-uniform grids on [blo, bhi] x [lo, hi] and general tables (no symmetry)."""
    rng = np.random.default_rng(seed)
    beta = np.sort(rng.uniform(blo, bhi, size=nh))
    if nh > 1:
        beta[0], beta[-1] = blo, bhi
    g = np.sort(rng.uniform(lo, hi, size=nq))
    g[0], g[-1] = lo, hi
    assert np.all(np.diff(g) > 0) and np.all(np.diff(beta) > 0)
    P = rng.normal(0.0, scale, size=(6, nh, nh, nq, nq))
    Q = rng.normal(0.0, scale, size=(6, nh, nh, nq, nq)) if with_q else None
    return beta, g, P, Q
