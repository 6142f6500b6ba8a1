"""Host-side helpers of the modal radiation term (HydroForces.set_radiation_modes): a state-space model to modes,
and a fit of modes to a sampled impulse response.  NumPy only; nothing here runs per step.

A mode is a pair (lambda, rho) of a complex pole and a complex residue, K(tau) = sum Re[rho exp(lambda tau)]: a real pole has a
zero imaginary part, a conjugate pair is ONE mode (the one with Im lambda > 0) whose residue is twice the pair's."""
import numpy as np


def modes_irf(modes, tau):
    """sum Re[rho exp(lambda tau)] of a list of (lambda, rho) at the times tau."""
    tau = np.asarray(tau, dtype=np.float64)
    out = np.zeros(tau.shape)
    for lam, rho in modes:
        out += (complex(rho) * np.exp(complex(lam) * tau)).real
    return out


def _fold_conjugates(poles, residues, imag_of, tol):
    """One mode per real pole and per conjugate pair: `imag_of[i]` decides what pole i is (> tol: the kept half of a pair, its
    residue doubled; < -tol: the dropped half; else real)."""
    modes = []
    for lam, r, im in zip(poles, residues, imag_of):
        if im > tol:
            modes.append((complex(lam), 2.0 * complex(r)))
        elif im >= -tol:
            # a pole on its own: real, or (a fit's negative real discrete pole) with Im lambda = pi / dt
            real = abs(lam.imag) <= tol
            modes.append((complex(lam.real, 0.0), complex(r.real, 0.0)) if real else (complex(lam), complex(r)))
    return modes


def state_space_to_modes(A, B, C, cond_max=1e10):
    """K(tau) = C exp(A tau) B of a real (n, n) matrix A, n-vectors B and C, as modes: A = V diag(lambda) V^-1 (numpy.linalg.eig),
    rho_i = (C V)_i (V^-1 B)_i.  ValueError when A is not diagonalisable to working accuracy (cond V above cond_max: a defective
    matrix has no modal form) or has a pole with Re lambda >= 0."""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    n = A.shape[0]
    if A.shape != (n, n):
        raise ValueError("A must be square")
    B = np.asarray(B, dtype=np.float64).reshape(-1)
    C = np.asarray(C, dtype=np.float64).reshape(-1)
    if B.size != n or C.size != n:
        raise ValueError("B and C must have the order of A")
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.all(np.isfinite(C))):
        raise ValueError("non-finite value in the state-space model")
    lam, V = np.linalg.eig(A)
    if np.any(lam.real >= 0.0):
        raise ValueError("unstable state-space model: a pole with Re lambda >= 0")
    if np.linalg.cond(V) > cond_max:
        raise ValueError("defective state matrix: no modal form (eigenvector matrix singular to working accuracy)")
    res = (C @ V) * np.linalg.solve(V, B.astype(np.complex128))
    tol = 1e-12 * max(1.0, float(np.max(np.abs(lam))))
    return _fold_conjugates(lam, res, lam.imag, tol)


def state_space_pairs_to_modes(A, B, C, D):
    """The (row, col, lambda, rho) list of one body from nested [6][D] A, B, C (lists or object arrays): state_space_to_modes of
    every pair that holds a model, in row-major pair order; None or an empty A is a pair without one."""
    modes = []
    for r in range(6):
        for c in range(int(D)):
            if A[r][c] is None or np.size(A[r][c]) == 0:
                continue
            modes += [(r, c, lam, rho) for lam, rho in state_space_to_modes(A[r][c], B[r][c], C[r][c])]
    return modes


def fit_radiation_modes(K_row_col, t, max_order=10, r2_min=0.99):
    """Modes of one (row, column) pair from its impulse response sampled on the uniform grid t (t[0] = 0): a Hankel-SVD realisation
    (Kung's method, as BEMIO's state-space fit) of the samples taken as the Markov parameters K_k = C A^k B, its discrete poles mu
    mapped to lambda = log(mu) / dt.  The order rises from 1 until R^2 >= r2_min or max_order is reached; orders that give a pole
    on or outside the unit circle are passed over.  Returns (modes, R^2 achieved); ValueError if no order gives a stable model.
    A pair with no response (every sample zero) has no modes: ([], 1.0)."""
    K = np.asarray(K_row_col, dtype=np.float64).reshape(-1)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    if K.size != t.size or K.size < 4:
        raise ValueError("K and t must have the same length, at least 4")
    dt = (t[-1] - t[0]) / (t.size - 1)
    if not dt > 0.0 or np.max(np.abs(np.diff(t) - dt)) > 1e-9 * dt:
        raise ValueError("t must be uniform and increasing")
    if not K.any():
        return [], 1.0
    rows = K.size // 2
    cols = K.size - rows
    H = K[np.arange(rows)[:, None] + np.arange(cols)[None, :]]
    U, s, Vt = np.linalg.svd(H, full_matrices=False)
    var = float(np.sum((K - K.mean()) ** 2))
    best = None
    for n in range(1, min(int(max_order), rows - 1, int(np.sum(s > 0.0))) + 1):
        sq = np.sqrt(s[:n])
        O = U[:, :n] * sq[None, :]
        Ad = np.linalg.lstsq(O[:-1], O[1:], rcond=None)[0]
        Bd = sq * Vt[:n, 0]
        Cd = O[0]
        mu, V = np.linalg.eig(Ad)
        if np.any(np.abs(mu) >= 1.0) or np.any(mu == 0.0) or np.linalg.cond(V) > 1e10:
            continue
        res = (Cd @ V) * np.linalg.solve(V, Bd.astype(np.complex128))
        lam = np.log(mu.astype(np.complex128)) / dt
        modes = _fold_conjugates(lam, res, mu.imag, 1e-12)
        r2 = 1.0 - float(np.sum((K - modes_irf(modes, t - t[0])) ** 2)) / var if var > 0.0 else 1.0
        if best is None or r2 > best[1]:
            best = (modes, r2)
        if r2 >= r2_min:
            break
    if best is None:
        raise ValueError("no stable model up to max_order")
    return best
