"""NumPy restatement of the component analysis of an imported eta record (include/hydrochrono_amd.h, hc_set_eta_record_components;
hydrochrono_amd/csrc/hc_eta_components.hpp / .hip), in long double: the yardstick of tests/test_eta_components_cpu.py and
tests/test_gpu_eta_components.py.

Convention (hc_wave_kinematics): eta(0, t) = sum A cos(phi - w t).  With t_j = t0 + j h, w_m = 2 pi m / T_w, T_w = n h:
c_m = (2 / n) sum_j eta_j exp(+i 2 pi ((m j) mod n) / n) = A exp(i (phi - w_m t0)); turned by exp(i w_m t0) it is A exp(i phi)."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
# pi to long double precision (np.pi is a double)
PI_LD = LD(3) + LD("0.14159265358979323846264338327950288")
UNIFORM_TOL = 1e-9


def _ld(fr):
    """A rational number to long double: its nearest double plus the remainder's."""
    hi = float(fr)
    return LD(hi) + LD(float(fr - Fraction(hi)))


def mean_spacing(t):
    return (t[-1] - t[0]) / (len(t) - 1)


def is_uniform(t):
    t = np.asarray(t, dtype=np.float64)
    h = mean_spacing(t)
    return bool(np.all(np.abs(t - (t[0] + np.arange(t.size) * h)) <= UNIFORM_TOL * h))


def grid_samples(t, eta):
    """The n analysed values: the record as given on a uniform grid, else its piecewise-linear interpolant at t0 + j h."""
    t, eta = np.asarray(t, dtype=np.float64), np.asarray(eta, dtype=np.float64)
    if is_uniform(t):
        return eta.copy()
    h = mean_spacing(t)
    return np.interp(np.minimum(t[0] + np.arange(t.size) * h, t[-1]), t, eta)


def band_bins(n, T_w, f_min, f_max):
    m = np.arange(1, n // 2 + 1)
    f = m / T_w
    return m[(f_min <= f) & (f <= f_max)]


def _unit_roots(n):
    """exp(i 2 pi r / n), r = 0 .. n-1, in long double"""
    ang = 2 * PI_LD * np.arange(n).astype(LD) / LD(n)
    return np.cos(ang) + 1j * np.sin(ang)


def coefficients(samples, bins, T_w, t0):
    """c_m exp(i w_m t0) per bin in long double; the integer phases are exact (64-bit integers), the origin product is reduced as a
    rational number."""
    x = np.asarray(samples, dtype=LD)
    n = x.size
    j = np.arange(n, dtype=np.int64)  # m j < 2^63 for every record an int counts
    out = np.zeros(len(bins), dtype=np.clongdouble)
    unit = _unit_roots(n)
    for i, m in enumerate(int(v) for v in bins):
        c = (x * unit[(m * j) % n]).sum() * (LD(1) if 2 * m == n else LD(2)) / LD(n)
        cyc = Fraction(m) * Fraction(float(t0)) / Fraction(float(T_w))
        cyc -= cyc.numerator // cyc.denominator
        rot = 2 * PI_LD * _ld(cyc)
        out[i] = c * (np.cos(rot) + 1j * np.sin(rot))
    return out


def select(A, max_components):
    A = np.asarray(A, dtype=np.float64)
    if max_components <= 0 or max_components >= A.size:
        return np.arange(A.size)
    order = sorted(range(A.size), key=lambda i: (-A[i], i))  # the largest first, ties to the lower bin
    return np.array(sorted(order[:max_components]), dtype=np.int64)


def analyse(t, eta, f_min, f_max, max_components=0):
    t = np.asarray(t, dtype=np.float64)
    x = grid_samples(t, eta)
    n = x.size
    h = mean_spacing(t)
    T_w = n * h
    bins = band_bins(n, T_w, f_min, f_max)
    c = coefficients(x, bins, T_w, t[0])
    A, phi = np.abs(c).astype(np.float64), np.angle(c).astype(np.float64)
    keep = select(A, max_components)
    m, A, phi = bins[keep], A[keep], phi[keep]
    mean = float(x.astype(LD).mean())
    var = float(((x.astype(LD) - mean) ** 2).mean())
    jj = np.arange(n, dtype=np.int64)
    rec = np.zeros(n, dtype=LD)
    c0 = coefficients(x, m, T_w, 0.0)  # against sample 0: the reconstruction at the sample times with the exact integer phases
    unit = _unit_roots(n)
    for mi, ci in zip((int(v) for v in m), c0):
        u = unit[(mi * jj) % n]
        rec += ci.real * u.real + ci.imag * u.imag
    res = x.astype(LD) - mean - rec
    return dict(m=m, f=m / T_w, A=A, phase=phi, mean=mean, variance_share=float((A ** 2 / 2).sum() / var) if var > 0 else 0.0,
                rms_residual=float(np.sqrt((res ** 2).mean())), std=float(np.sqrt(var)), T_w=T_w, h=h, samples=x)


def on_grid_record(n, t0, h, comps):
    """A record of cosines on its own Fourier grid: comps = [(m, A, phi)], eta_j = sum A cos(phi - w_m t_j) in long double, rounded
    once, with w_m = 2 pi m / T_w for the T_w the analysis forms from the times (n times their mean spacing) and t_j = t0 + j T_w / n;
    the phases w_m t_j are exact rationals, reduced to a cycle before the cosine."""
    t = float(t0) + np.arange(n) * float(h)
    T = Fraction(float(n * mean_spacing(t)))
    eta = np.zeros(n, dtype=LD)
    for m, A, phi in comps:
        base = Fraction(m) * Fraction(float(t[0])) / T
        cyc = [(base + Fraction(m * j, n)) % 1 for j in range(n)]
        cyc = np.array([_ld(c) for c in cyc], dtype=LD)
        eta += LD(A) * np.cos(LD(phi) - 2 * PI_LD * cyc)
    return t, eta.astype(np.float64)


def five_cosines(n):
    """Five cosines on the grid of an n-sample record; the Nyquist bin of an even n among them, with the one phase it can have there
    (phi - w t0 a multiple of pi: the tests use t0 = 0 for it)."""
    ms = [3, 7, n // 5, n // 3, n // 2 if n % 2 == 0 and n <= 64 else n // 2 - 1]
    return [(m, 0.1 + 0.07 * i, 0.0 if 2 * m == n else 0.4 + 1.1 * i - 3.0) for i, m in enumerate(ms)]
