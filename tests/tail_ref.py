"""Exact reference of the radiation component on the common grid, for the tests of the spectral radiation tail.

With the step equal to the IRF spacing and every history sample on the grid, the radiation component of step m is the plain lag sum
    rad_m[row] = sum_{s < S} w_s G[row, col, s] v_{m-s}[col]
with G = rho K (BEMIO order, as the ingest scales it; under TaperedDirect the processed kernel of HydroForces.rirf_effective()) and w
the trapezoid widths of rirf_t.  TailRef evaluates it in np.longdouble on a fixed set of rows and bounds the GPU's answer row by row by
    |rad_gpu - rad_ref| <= 1e-12 * A_m,   A_m = sum_s |w_s G_s| |v_{m-s}|,
which leaves room for the rounding of the FFT but not for one wrong, missing or doubled lag (whose term is about A_m / S).

The grid spacing is a power of two, so every step time, history time and lag is exact and the history lookups land on the samples
themselves (no interpolation weight).  flat_case() draws every body's rirf_K i.i.d. N(0, 1) (same-body blocks x10, as synthetic.py
does): every lag weighs the same, so a defect confined to the far or the last partition is not damped away as it is under the
decaying kernels of synthetic.many_body_case.  Its bodies are generated on demand (a system of 170 bodies and 512 lags would be
4 GB of K on the host).
"""
from collections.abc import Sequence

import numpy as np

DT = 2.0 ** -7   # grid spacing (s): exact times, exact lags
REL = 1e-12      # the row-wise bound, relative to A_m
ROW_BUDGET = 2e7  # D * D * S above this: the reference covers a subset of rows (check_rows)


def trapezoid_widths(t):
    """The widths the ingest gives the IRF samples (the reference's rirf_width_vector)."""
    t = np.asarray(t, dtype=np.float64)
    w = np.zeros(t.size)
    d = 0.5 * np.abs(np.diff(t))
    w[:-1] += d
    w[1:] += d
    return w


class FlatBodies(Sequence):
    """The bodies of a flat-envelope case, made when asked for: the same arrays for the same (seed, b) every time."""

    def __init__(self, N, S, dt, seed):
        self.N, self.S, self.dt, self.seed = N, S, dt, seed

    def __len__(self):
        return self.N

    def rirf(self, b):
        D = 6 * self.N
        K = np.random.default_rng([self.seed, b, 1]).standard_normal((6, D, self.S))
        K[:, 6 * b:6 * b + 6, :] *= 10.0
        return K

    def __getitem__(self, b):
        if not 0 <= b < self.N:
            raise IndexError(b)
        D = 6 * self.N
        rng = np.random.default_rng([self.seed, b, 0])
        side = int(np.ceil(np.sqrt(self.N)))
        cg = np.array([20.0 * (b % side), 20.0 * (b // side), -2.0])
        lin = rng.normal(size=(6, 6))
        A = 0.05 * rng.normal(size=(6, D))
        A[:, 6 * b:6 * b + 6] += np.diag(100.0 + 50.0 * rng.uniform(size=6))
        nw, ne = 8, 21
        ex_t = (np.arange(ne) - (ne - 1) * 0.5) * 0.05
        return dict(disp_vol=200.0 + 100.0 * rng.uniform(), cg=cg, cb=cg + np.array([0.0, 0.0, 0.1]),
                    lin=0.5 * (lin + lin.T) + np.diag(50.0 + 50.0 * rng.uniform(size=6)), added_mass_inf=A,
                    rirf_t=np.arange(self.S) * self.dt, rirf_K=self.rirf(b),
                    w=np.linspace(0.05, 0.4, nw), ex_mag=rng.uniform(0.1, 2.0, size=(6, 1, nw)),
                    ex_phase=rng.uniform(-np.pi, np.pi, size=(6, 1, nw)), ex_irf_t=ex_t,
                    ex_irf_f=rng.normal(size=(6, 1, ne)))


def flat_case(N, S, dt=DT, seed=1):
    """Raw-array case (the schema of tests/cases.py) whose IRF has a flat envelope."""
    return dict(N=N, rho=1000.0, g=9.81, water_depth=float("inf"), bodies=FlatBodies(N, S, dt, seed))


def rest_state(case):
    """pos, rpy of the bodies at rest (flattened), for steps whose velocities are drawn freely."""
    N = case["N"]
    if isinstance(case["bodies"], FlatBodies):  # (without making the bodies' K)
        side = int(np.ceil(np.sqrt(N)))
        pos = np.concatenate([[20.0 * (b % side), 20.0 * (b // side), -2.0] for b in range(N)])
    else:
        pos = np.concatenate([np.asarray(case["bodies"][b]["cg"], dtype=np.float64) for b in range(N)])
    return pos.astype(np.float64), np.zeros(3 * N)


def check_rows(N):
    """The rows the longdouble reference covers where D * D * S is large: the first body, the last body, and one row of each
    body in between (at most 12 bodies, spread evenly), each at a different DoF."""
    D = 6 * N
    bodies = np.unique(np.linspace(0, N - 1, min(N, 12)).round().astype(int))
    rows = {0, D - 1} | {6 * int(b) + int(b) % 6 for b in bodies}
    return sorted(rows)


def kernel_rows(case, rows):
    """G = rho K_raw of the given global rows: [R][D][S]."""
    out = []
    cache = {}
    for r in rows:
        b, i = divmod(int(r), 6)
        if b not in cache:
            bd = case["bodies"][b]
            cache = {b: np.asarray(bd["rirf_K"], dtype=np.float64)}
        out.append(case["rho"] * cache[b][i])
    return np.stack(out)


class TailRef:
    """rad_m on `rows` from G rows [R][D][S] and the widths w [S]; velocity samples are handed in as an array, oldest first."""

    def __init__(self, G, w, rows):
        G = np.asarray(G, dtype=np.float64)
        self.R, self.D, self.S = G.shape
        self.rows = list(rows)
        wg = np.asarray(w, dtype=np.longdouble)[None, None, :] * G.astype(np.longdouble)  # [R][D][S]
        self.WG = np.ascontiguousarray(np.transpose(wg, (0, 2, 1)).reshape(self.R, self.S * self.D))  # [R][s * D + col]
        self.absWG = np.abs(self.WG)

    def window(self, v, m):
        """[S * D]: v_{m-s}[col] at s * D + col; v [T][D] oldest first, m an index into it with m >= S - 1."""
        if m < self.S - 1:
            raise ValueError(f"sample {m}: the history does not cover the IRF window")
        return np.ascontiguousarray(v[m - self.S + 1:m + 1][::-1]).reshape(-1).astype(np.longdouble)

    def rad(self, v, m):
        x = self.window(v, m)
        return self.WG @ x, self.absWG @ np.abs(x)

    def check(self, v, steps, got, what=""):
        """got[k] = the GPU's radiation rows (all D_local of them, global order) at sample index steps[k].  Returns the largest
        |delta| / (1e-12 A_m); fails with the step and the row where the bound breaks."""
        worst = 0.0
        for m, g in zip(steps, got):
            ref, A = self.rad(v, m)
            d = np.abs(np.asarray(g, dtype=np.longdouble)[self.rows] - ref)
            ratio = np.where(A > 0, d / (REL * np.where(A > 0, A, 1)), np.where(d > 0, np.inf, 0.0)).astype(np.float64)
            k = int(np.argmax(ratio))
            assert ratio[k] <= 1.0, (f"{what}sample {m}, row {self.rows[k]}: |rad - ref| = {float(d[k]):.3e}, "
                                     f"1e-12 A_m = {float(REL * A[k]):.3e} (ratio {ratio[k]:.2e})")
            worst = max(worst, float(ratio[k]))
        return worst
