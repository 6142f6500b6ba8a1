"""numpy.longdouble restatement of the modal radiation term (hydrochrono_amd/csrc/hc_radiation_modes.hip): the
recurrence z_n+1 = e^x z_n + h [(phi1 - phi2) v_n + phi2 v_n+1] per mode, the row sums, and the snapshot ring with its rule for a
step back in time.  Written from the definitions, not from the kernel: phi1 and phi2 have their own series threshold and length
here.  tests/test_radiation_modes_ref_cpu.py keeps it honest against closed forms.  Below it, what the fit and state-space tests
share (tests/test_radiation_modes_fit_cpu.py, tests/test_gpu_radiation_modes_fit.py): expm_taylor, z_sine_phase, fit_body, the
nested state-space structure and the samples with a negative real discrete pole."""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS = float(np.finfo(np.float64).eps)


def phi12(x):
    """phi1 = (e^x - 1) / x and phi2 = (e^x - 1 - x) / x^2 of a complex longdouble x, accurate as |x| -> 0 (series below 1/2,
    40 terms) and finite as Re x -> -inf."""
    x = CLD(x)
    if abs(x) < 0.5:
        p1, p2 = CLD(0), CLD(0)
        for k in range(40, 0, -1):
            p1 = (1 + p1) * x / LD(k + 1)
            p2 = (1 + p2) * x / LD(k + 2)
        return 1 + p1, (1 + p2) / LD(2)
    e = np.exp(x)
    p1 = (e - 1) / x
    return p1, (p1 - 1) / x


def z_linear(lam, a, b, t):
    """z(t) from z(0) = 0 under v = a + b t: a t phi1(lambda t) + b t^2 phi2(lambda t)."""
    t = LD(t)
    p1, p2 = phi12(CLD(lam) * t)
    return LD(a) * t * p1 + LD(b) * t * t * p2


def z_sine(lam, omega, t):
    """z(t) from z(0) = 0 under v = sin(omega t): the analytic integral of e^{lambda (t - s)} sin(omega s)."""
    lam, t, w = CLD(lam), LD(t), LD(omega)
    el = np.exp(lam * t)
    plus = (np.exp(CLD(1j) * w * t) - el) / (CLD(1j) * w - lam)
    minus = (np.exp(CLD(-1j) * w * t) - el) / (CLD(-1j) * w - lam)
    return (plus - minus) / CLD(2j)


class DuplicateTime(RuntimeError):
    pass


class NoSnapshot(ValueError):
    pass


class ModalRef:
    """rows: a list per row of (col, lambda, rho) in the order the device keeps them (by column, within a pair as given); rho
    already carries the water density.  step(t, v) advances as hc_compute_radiation_modes does and returns the row sums
    (longdouble); `zmax[r]` is the largest |z| the row has held, `sum_rho[r]` its sum of |rho|."""

    def __init__(self, rows, depth=4):
        self.rows = [[(int(c), CLD(lam), CLD(rho)) for c, lam, rho in row] for row in rows]
        self.depth = int(depth)
        self.snaps = []  # (t, v, z per row), newest last
        self.zmax = [0.0] * len(self.rows)
        self.sum_rho = [float(sum(abs(rho) for _, _, rho in row)) for row in self.rows]
        self.steps = 0

    def reset(self):
        self.snaps = []

    def step(self, t, v):
        t = float(t)
        v = np.asarray(v, dtype=np.float64)
        if not self.snaps:
            self.snaps = [(t, v.copy(), [[CLD(0)] * len(row) for row in self.rows])]
            return np.zeros(len(self.rows), dtype=LD)
        if t == self.snaps[-1][0]:
            raise DuplicateTime(t)
        keep = [s for s in self.snaps if s[0] < t]
        if not keep:
            raise NoSnapshot(t)  # (the state stays as it was)
        t0, v0, z0 = keep[-1]
        h = LD(t - t0)  # the difference in double, as the library forms it
        znew, out = [], np.zeros(len(self.rows), dtype=LD)
        for r, row in enumerate(self.rows):
            zr, acc = [], LD(0)
            for (c, lam, rho), z in zip(row, z0[r]):
                x = lam * h
                p1, p2 = phi12(x)
                zn = np.exp(x) * z + h * ((p1 - p2) * LD(v0[c]) + p2 * LD(v[c]))
                zr.append(zn)
                acc += (rho * zn).real
                self.zmax[r] = max(self.zmax[r], float(abs(zn)))
            znew.append(zr)
            out[r] = acc
        self.snaps = (keep + [(t, v.copy(), znew)])[-self.depth:]
        self.steps += 1
        return out

    def bound(self, C):
        """C eps (steps + items in the row) sum|rho| max|z| per row."""
        return np.array([C * EPS * (self.steps + len(row)) * s * zm for row, s, zm in zip(self.rows, self.sum_rho, self.zmax)])


def device_rows(modes_by_body, b0, b1, rho_water):
    """The rows of bodies [b0, b1) as the device lays them out: modes_by_body[b] = [(row, col, lambda, rho)], row-major, within a
    row stably by column; the residues times the water density."""
    rows = []
    for b in range(b0, b1):
        for r in range(6):
            sel = [m for m in modes_by_body.get(b, []) if m[0] == r]
            sel.sort(key=lambda m: m[1])
            rows.append([(m[1], m[2], rho_water * complex(m[3])) for m in sel])
    return rows


def expm_taylor(A, tau):
    """exp(A tau) from its Taylor series in longdouble (scaling and squaring: |A tau| / 2^s < 1/2)."""
    A = np.asarray(A, dtype=LD) * LD(tau)
    s = max(0, int(np.ceil(np.log2(max(float(np.max(np.sum(np.abs(A), axis=1))), 1e-30)))) + 1)
    A = A / LD(2 ** s)
    E, term = np.eye(A.shape[0], dtype=LD), np.eye(A.shape[0], dtype=LD)
    for k in range(1, 40):
        term = term @ A / LD(k)
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def z_sine_phase(lam, omega, phase, t):
    """z(t) from z(0) = 0 under v = sin(omega t + phase): the two quadratures superposed.  t may be an array."""
    lam, t, w = CLD(lam), np.asarray(t, dtype=LD), LD(omega)
    el = np.exp(lam * t)
    plus = (np.exp(CLD(1j) * w * t) - el) / (CLD(1j) * w - lam)
    minus = (np.exp(CLD(-1j) * w * t) - el) / (CLD(-1j) * w - lam)
    return np.cos(LD(phase)) * (plus - minus) / CLD(2j) + np.sin(LD(phase)) * (plus + minus) / CLD(2)


def fit_body(K, t, D, **fit_opts):
    """fit_radiation_modes over the pairs of one body's K [6][D][S] that carry a response, max |K_rc| > 1e-6 max |K|: (modes,
    per_pair) with modes the (row, col, lambda, rho) list for set_radiation_modes and per_pair[(r, c)] = (n_modes, R^2, L1),
    L1 = dt sum_k |K_fit(tau_k) - K(tau_k)|."""
    from hydrochrono_amd.radiation_modes import fit_radiation_modes, modes_irf
    K = np.asarray(K, dtype=np.float64).reshape(6, int(D), -1)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    dt = (t[-1] - t[0]) / (t.size - 1)
    top = float(np.abs(K).max())
    modes, per_pair = [], {}
    for r in range(6):
        for c in range(int(D)):
            if not np.abs(K[r, c]).max() > 1e-6 * top:
                continue
            fitted, r2 = fit_radiation_modes(K[r, c], t, **fit_opts)
            modes += [(r, c, lam, rho) for lam, rho in fitted]
            per_pair[(r, c)] = (len(fitted), r2, float(dt * np.sum(np.abs(modes_irf(fitted, t - t[0]) - K[r, c]))))
    return modes, per_pair


def nested_state_space(D, seed=11):
    """[6][D] A, B, C: pairs of orders 1, 2, 3, 4 and 7 (the matrices of the conversion's own test), the rest None or empty, in
    lists and in object arrays alike.  Returns (A, B, C, {(r, c): (A, B, C)})."""
    rng = np.random.default_rng(seed)
    where = {(0, 0): 1, (0, D - 1): 2, (2, 7): 3, (3, 3): 4, (5, 6): 7, (5, D - 1): 2, (1, 0): 3}
    A = [[None] * D for _ in range(6)]
    B = [[None] * D for _ in range(6)]
    C = [[None] * D for _ in range(6)]
    pairs = {}
    for (r, c), n in where.items():
        A[r][c] = rng.normal(size=(n, n)) - (1.5 + np.sqrt(n)) * np.eye(n)
        B[r][c], C[r][c] = rng.normal(size=n), rng.normal(size=n)
        pairs[(r, c)] = (A[r][c], B[r][c], C[r][c])
    for r, c in ((0, 1), (4, 4), (5, 0)):  # "no model" spelled as an empty array; B and C are not looked at
        A[r][c] = np.zeros((0, 0))
    A[4][2], B[4][2], C[4][2] = [], [], []
    return A, B, C, pairs


def negative_pole_samples():
    """K_k = 3 (-0.8)^k + 2 0.9^k on 60 samples of dt = 0.05: (K, t).  Its fit holds a negative real discrete pole."""
    k = np.arange(60)
    return 3.0 * (-0.8) ** k + 2.0 * 0.9 ** k, 0.05 * k


def pack_velocity(linvel, angvel):
    """[D] by DoF column from linvel, angvel [3N]."""
    lv, av = np.asarray(linvel, dtype=np.float64).reshape(-1, 3), np.asarray(angvel, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([lv, av], axis=1).reshape(-1)
