"""The NumPy restatement of the second-order waves (tests/wave2_ref.py) checked without trusting the formulas it was written from:
the second-order free-surface conditions by difference quotients of its own fields, Stokes' closed form for one component, and
the error a plain FP64 evaluation makes on every input set of the GPU tests (which is what entitles those to their tolerance)."""
import numpy as np
import pytest

import wave2_inputs as wi
import wave2_ref as w2
from cases import load_into_oracle

LD = np.longdouble
G = 9.81


def solve_k(w, depth, g=G):
    """k of w^2 = g k tanh(k h) in longdouble, to 1e-14 and better (Newton from the deep-water root)."""
    w = np.asarray(w, dtype=LD)
    k = w * w / LD(g)
    if np.isinf(depth):
        return k
    h = LD(depth)
    k = np.maximum(k, w / np.sqrt(LD(g) * h))
    for _ in range(100):
        th = np.tanh(k * h)
        f = LD(g) * k * th - w * w
        k = k - f / (LD(g) * (th + k * h * (1 - th * th)))
    assert np.all(np.abs(LD(g) * k * np.tanh(k * h) - w * w) <= 1e-14 * w * w)
    return k


def d1(f, i, d):
    """d f / d arg_i by the five-point central quotient: error d^4 f^(5) / 30."""
    def df(*a):
        s = lambda m: f(*[v + m * d if n == i else v for n, v in enumerate(a)])
        return (-s(2) + 8 * s(1) - 8 * s(-1) + s(-2)) / (12 * d)
    return df


def d2(f, i, d):
    """d^2 f / d arg_i^2 by the five-point central quotient: error d^4 f^(6) / 90."""
    def df(*a):
        s = lambda m: f(*[v + m * d if n == i else v for n, v in enumerate(a)])
        return (-s(2) + 16 * s(1) - 30 * s(0) + 16 * s(-1) - s(-2)) / (12 * d * d)
    return df


@pytest.mark.parametrize("depth", [8.0, 30.0, np.inf])
def test_free_surface_conditions_laplace_and_bed(depth):
    """At z = 0:  phi2_tt + g phi2_z = -d/dt |grad phi1|^2 + (phi1_t / g) d/dz (phi1_tt + g phi1_z)  and
    eta2 = -(phi2_t + 1/2 |grad phi1|^2 + eta1 phi1_zt) / g;  Laplace at a submerged point, no flow through the bed.
    Tolerance: every quantity is a sum of harmonics whose rates (rad/s, rad/m) are at most rho = w_3 + w_3 resp. k_3 + k_3, so an
    n-th derivative is at most rho^n times the sum M of the |terms|; the five-point quotients of step d are off by at most
    d^4 rho^6 M / 30 (nested ones a few times that), and their rounding by a few eps M / d^2.  With d = 1e-3 in longdouble that is
    below 1e-8 M, far below the 1e-6 a double-precision quotient reaches."""
    A = np.array([1.0, 0.7, 0.4])
    w = np.array([0.6, 0.85, 1.3])
    k = solve_k(w, depth)
    comp = (A, w, k, np.array([0.3, 1.1, -0.7]))
    d = LD(1e-3)
    eps = np.finfo(LD).eps
    rho = float(max(2 * w[-1], 2 * k[-1], 1.0))
    slack = 20 * float(d) ** 4 * rho ** 6 + 200 * float(eps) / float(d) ** 2
    assert slack < 1e-8

    def f2(name):
        idx = {"eta": 0, "phi": 3}[name]
        return lambda x, z, t: w2.fields(comp, G, depth, [[x, 0.0, z]], [t], clamp=False)[0][idx][0, 0]

    eta1 = lambda x, z, t: w2.first_order(comp, G, depth, x, z, t)[0]
    phi1 = lambda x, z, t: w2.first_order(comp, G, depth, x, z, t)[1]
    phi2, eta2 = f2("phi"), f2("eta")
    X, Z, T = 0, 1, 2
    grad2 = lambda x, z, t: d1(phi1, X, d)(x, z, t) ** 2 + d1(phi1, Z, d)(x, z, t) ** 2
    lin = lambda x, z, t: d2(phi1, T, d)(x, z, t) + G * d1(phi1, Z, d)(x, z, t)  # (zero at z = 0; its z derivative is not)
    tabs, _ = w2.pair_tables(comp, G, depth)
    kap = {"m": np.abs(k[:, None] - k[None, :]), "p": k[:, None] + k[None, :]}
    Om = {"m": np.abs(w[:, None] - w[None, :]), "p": w[:, None] + w[None, :]}
    M_kin = sum(np.sum(np.abs(tabs["B" + s]) * (Om[s] ** 2 + G * kap[s])) for s in "mp")
    M_eta = np.sum(0.25 * np.outer(A, A) * (np.abs(tabs["Km"]) + np.abs(tabs["Kp"])))
    M_lap = sum(np.sum(np.abs(tabs["B" + s]) * 2 * kap[s] ** 2) for s in "mp")
    M_bed = sum(np.sum(np.abs(tabs["B" + s]) * kap[s]) for s in "mp")
    assert M_kin > 0.01 and M_eta > 0.01
    for x, t in ((LD(1.7), LD(2.3)), (LD(-40.0), LD(11.9))):
        z0 = LD(0)
        lhs = d2(phi2, T, d)(x, z0, t) + G * d1(phi2, Z, d)(x, z0, t)
        rhs = -d1(grad2, T, d)(x, z0, t) + d1(phi1, T, d)(x, z0, t) / G * d1(lin, Z, d)(x, z0, t)
        assert abs(lhs - rhs) <= slack * M_kin, (depth, float(lhs), float(rhs))
        assert abs(lhs) > 1e-3 * M_kin  # (the condition is not met by zeros)
        e2 = -(d1(phi2, T, d)(x, z0, t) + grad2(x, z0, t) / 2 + eta1(x, z0, t) * d1(d1(phi1, Z, d), T, d)(x, z0, t)) / G
        assert abs(e2 - eta2(x, z0, t)) <= slack * M_eta, (depth, float(e2), float(eta2(x, z0, t)))
        zs = LD(-2.5)
        assert abs(d2(phi2, X, d)(x, zs, t) + d2(phi2, Z, d)(x, zs, t)) <= slack * M_lap
        if np.isfinite(depth):
            assert abs(d1(phi2, Z, d)(x, LD(-depth), t)) <= slack * M_bed
    # the fields the library returns are these derivatives of phi2 (at a submerged point, where nothing is held)
    x, z, t = LD(1.7), LD(-2.5), LD(2.3)
    (_, vel, acc, _), (_, vs, as_, _) = w2.fields(comp, G, depth, [[x, 0.0, z]], [t])
    for col, var in ((0, X), (2, Z)):
        assert abs(d1(phi2, var, d)(x, z, t) - vel[0, 0, col]) <= slack * rho * vs[0, 0, col]
        assert abs(d1(d1(phi2, var, d), T, d)(x, z, t) - acc[0, 0, col]) <= slack * rho * rho * as_[0, 0, col]


def test_stokes_second_order_of_one_component():
    A, w = 0.8, 1.1
    for depth in (10.0, np.inf):
        k = solve_k([w], depth).astype(np.float64).astype(LD)  # FP64 component data, as the library holds it
        comp = (np.array([A]), np.array([w]), k, np.array([0.4]))
        pts = [[x, 0.0, -1.0] for x in (0.0, 3.3, -17.0)]
        times = [0.0, 1.9, 7.7]
        (eta2, vel, _, phi2), (scale, _, _, _) = w2.fields(comp, G, depth, pts, times)
        theta = k[0] * np.asarray(pts, dtype=LD)[None, :, 0] - LD(w) * np.asarray(times, dtype=LD)[:, None] + LD(0.4)
        want = w2.stokes_eta2(LD(A), k[0], LD(depth) if np.isfinite(depth) else depth, theta)
        # k solves the dispersion relation to 1e-16 after its rounding; the closed form and K+- weigh that differently
        assert np.all(np.abs(eta2 - want) <= 1e-12 * scale), depth
        if np.isinf(depth):
            assert not phi2.any() and not vel.any()
        else:
            assert np.abs(phi2).max() > 1e-4
            assert np.all(eta2.mean() < 0)  # (not a proof of set-down: the constant term is checked through `want`)


def oracle_components(name):
    case = wi.case_of(name)
    orc = load_into_oracle(case)
    waves = dict(wi.SETS[name][1])
    orc.add_waves_irregular(**waves)
    from wave_kinematics_ref import irregular_components
    return irregular_components(orc.irreg_spectrum()), case


@pytest.mark.parametrize("name", sorted(wi.SETS))
def test_plain_fp64_reaches_a_quarter_of_the_tolerance(name):
    """The GPU tests allow TOL * sum|term| (fields) and TOL * (|ref| + sum|addends|) (tables).  The same restatement evaluated in
    float64 stays within a quarter of that on every input set they use, under every choice of bands."""
    comp, case = oracle_components(name)
    assert comp[0].size == wi.SETS[name][1]["nfrequencies"] and np.all(np.isfinite(comp[0])) and np.all(comp[1] > 0)
    g, depth = case["g"], case["water_depth"]
    for bands in wi.BANDS:
        ref, mag = wi.reference_tables(bands, wi.key(comp), g, depth)
        dbl, _ = wi.reference_tables(bands, wi.key(comp), g, depth, np.float64)
        for n in ref:
            assert np.all(np.isfinite(dbl[n])), (bands, n)
            worst = np.max(np.abs(dbl[n] - ref[n]) / np.maximum(np.abs(ref[n]) + mag[n], 1e-300))
            print(f"{name} {bands} table {n}: float64 off by {float(worst):.2e} of |ref| + sum|addends|")
            assert worst <= wi.TOL / 4, (bands, n, float(worst))
        vals, scales = wi.reference(name, bands, wi.key(comp), g, depth)
        dvals, _ = wi.reference(name, bands, wi.key(comp), g, depth, np.float64)
        for v, dv, s, what in zip(vals[:3], dvals[:3], scales[:3], ("eta2", "vel2", "acc2")):
            assert np.all(np.isfinite(dv)), (bands, what)
            worst = np.max(np.abs(dv - v) / np.maximum(s, 1e-300)) if v.size else 0.0
            print(f"{name} {bands} {what}: float64 off by {float(worst):.2e} of sum|term|")
            assert np.all(np.abs(dv - v) <= wi.TOL / 4 * s), (bands, what, float(worst))
            if bands == "empty":
                assert not v.any() and not s.any()
