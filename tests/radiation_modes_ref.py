"""numpy.longdouble restatement of the modal radiation term (hydrochrono_amd/csrc/hc_radiation_modes.hip): the
recurrence z_n+1 = e^x z_n + h [(phi1 - phi2) v_n + phi2 v_n+1] per mode, the row sums, and the snapshot ring with its rule for a
step back in time.  Written from the definitions, not from the kernel: phi1 and phi2 have their own series threshold and length
here.  tests/test_radiation_modes_ref_cpu.py keeps it honest against closed forms."""
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


def pack_velocity(linvel, angvel):
    """[D] by DoF column from linvel, angvel [3N]."""
    lv, av = np.asarray(linvel, dtype=np.float64).reshape(-1, 3), np.asarray(angvel, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([lv, av], axis=1).reshape(-1)
