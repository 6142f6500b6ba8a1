"""The way modes reach the modal radiation term, without a GPU: fit_radiation_modes on the impulse responses of the golden BEMIO data
(tests/radiation_modes_ref.fit_body), its degenerate inputs, the negative real discrete pole, and the nested [6][D] state-space form
behind HydroForces.set_radiation_state_space (radiation_modes.state_space_pairs_to_modes).  The GPU side is
tests/test_gpu_radiation_modes_fit.py."""
import numpy as np
import pytest

import radiation_modes_ref as rm
from cases import sphere_case, three_body_case

SPHERE_FIT = dict(max_order=16, r2_min=0.999999)
THREE_BODY_FIT = dict(max_order=14, r2_min=1.0 - 1e-8)


def check_pairs(K, t, modes, per_pair, r2_min):
    """The setter's own rules and the R^2 asked for, per pair; returns max |K_fit - K| / max |K_rc| and L1 / (dt sum |K_rc|), the
    worst over the pairs."""
    from hydrochrono_amd.radiation_modes import modes_irf
    dt = t[1] - t[0]
    worst_max = worst_l1 = 0.0
    for (r, c), (n, r2, l1) in per_pair.items():
        own = [(lam, rho) for rr, cc, lam, rho in modes if (rr, cc) == (r, c)]
        assert len(own) == n and 1 <= n <= 16, (r, c, n)
        for lam, rho in own:
            assert np.isfinite(lam.real) and np.isfinite(lam.imag) and np.isfinite(rho.real) and np.isfinite(rho.imag), (r, c, lam, rho)
            assert lam.real < 0.0, (r, c, lam)
        assert r2 >= r2_min, (r, c, r2)
        fit = modes_irf(own, t)
        assert abs(l1 - dt * np.sum(np.abs(fit - K[r, c]))) <= 1e-12 * l1 + 1e-300
        worst_max = max(worst_max, float(np.abs(fit - K[r, c]).max() / np.abs(K[r, c]).max()))
        worst_l1 = max(worst_l1, float(l1 / (dt * np.sum(np.abs(K[r, c])))))
    return worst_max, worst_l1


def test_fit_of_the_sphere_file():
    """The sphere's IRF (S = 1001, dt = 0.015): 9 of its 36 pairs rise above 1e-6 of the largest |K| (the diagonal and the
    surge-pitch, sway-roll couplings), 4 to 6 modes each, 52 in all.  Measured here: max |K_fit - K| = 1.61e-3 of the pair's own
    max |K| at worst (pair (2, 2)), R^2 deficit at most 9.3e-7; the test allows ten times 1.7e-3."""
    bd = sphere_case()["bodies"][0]
    K, t = np.asarray(bd["rirf_K"], dtype=np.float64).reshape(6, 6, -1), np.asarray(bd["rirf_t"], dtype=np.float64)
    modes, per_pair = rm.fit_body(K, t, 6, **SPHERE_FIT)
    top = np.abs(K).max()
    assert sorted(per_pair) == sorted((r, c) for r in range(6) for c in range(6) if np.abs(K[r, c]).max() > 1e-6 * top)
    assert len(per_pair) == 9 and len(modes) == 52 and all(4 <= v[0] <= 6 for v in per_pair.values())
    worst_max, worst_l1 = check_pairs(K, t, modes, per_pair, SPHERE_FIT["r2_min"])
    print(f"sphere fit: {len(per_pair)} pairs, {len(modes)} modes, max |K_fit - K| / max |K_rc| {worst_max:.3e}, "
          f"L1 / L1(K) {worst_l1:.3e}, largest L1 {max(v[2] for v in per_pair.values()):.3e}, "
          f"R^2 deficit {1.0 - min(v[1] for v in per_pair.values()):.3e}")
    assert worst_max <= 10 * 1.7e-3


def test_fit_of_the_three_body_file():
    """The generated three-body file (D = 18, 32 samples of 0.02, one exponential per pair, cross-body columns): all 324 pairs fit
    with one mode each.  Measured here: L1 = 1.46e-14 of dt sum |K_rc| at worst; the test allows ten times 1.5e-14."""
    total = 0
    worst_max = worst_l1 = 0.0
    for bd in three_body_case()["bodies"]:
        K, t = np.asarray(bd["rirf_K"], dtype=np.float64).reshape(6, 18, -1), np.asarray(bd["rirf_t"], dtype=np.float64)
        modes, per_pair = rm.fit_body(K, t, 18, **THREE_BODY_FIT)
        assert len(per_pair) == 108 and len(modes) == 108
        total += len(per_pair)
        a, b = check_pairs(K, t, modes, per_pair, THREE_BODY_FIT["r2_min"])
        worst_max, worst_l1 = max(worst_max, a), max(worst_l1, b)
    print(f"three-body fit: {total} pairs, max |K_fit - K| / max |K_rc| {worst_max:.3e}, L1 / L1(K) {worst_l1:.3e}")
    assert total == 324
    assert worst_l1 <= 10 * 1.5e-14


def test_fit_degenerate_inputs():
    from hydrochrono_amd.radiation_modes import fit_radiation_modes, modes_irf
    t = 0.05 * np.arange(60)
    assert fit_radiation_modes(np.zeros(60), t) == ([], 1.0)
    assert fit_radiation_modes(np.zeros(4), t[:4], max_order=1, r2_min=1.0) == ([], 1.0)
    K = 2.0 * np.exp(-0.7 * t) + np.exp(-0.2 * t) * np.cos(1.3 * t)
    with pytest.raises(ValueError):
        fit_radiation_modes(K[:3], t[:3])  # a length below 4
    with pytest.raises(ValueError):
        fit_radiation_modes(np.zeros(3), t[:3])  # ... also of a zero pair
    bent = t.copy()
    bent[17] += 1e-4
    with pytest.raises(ValueError):
        fit_radiation_modes(K, bent)
    with pytest.raises(ValueError):
        fit_radiation_modes(K, t[::-1])
    with pytest.raises(ValueError):
        fit_radiation_modes(K, t[:-1])
    # t[0] != 0: the modes of the shifted grid.  On a grid of binary fractions the shift is exact, so the modes are the same bits.
    tb = 0.0625 * np.arange(60)
    Kb = 2.0 * np.exp(-0.7 * tb) + np.exp(-0.2 * tb) * np.cos(1.3 * tb)
    modes, r2 = fit_radiation_modes(Kb, tb, max_order=6, r2_min=1.0 - 1e-12)
    shifted, r2s = fit_radiation_modes(Kb, tb + 0.375, max_order=6, r2_min=1.0 - 1e-12)
    assert len(modes) == 2 and r2 >= 1.0 - 1e-12
    assert shifted == modes and r2s == r2
    assert np.max(np.abs(modes_irf(shifted, tb) - Kb)) <= 1e-11 * np.abs(Kb).max()
    # and on a grid where it is not: the same modes to rounding (dt differs in its last bits)
    other, _ = fit_radiation_modes(K, t + 0.37, max_order=6, r2_min=1.0 - 1e-12)
    base, _ = fit_radiation_modes(K, t, max_order=6, r2_min=1.0 - 1e-12)
    assert len(other) == len(base) == 2
    for (lam, rho), (lam_s, rho_s) in zip(base, other):
        assert abs(lam - lam_s) <= 1e-12 * abs(lam) and abs(rho - rho_s) <= 1e-12 * abs(rho)


def test_fit_of_a_negative_real_discrete_pole():
    """K_k = 3 (-0.8)^k + 2 0.9^k: mu = -0.8 has no real logarithm; the mode is lambda = (ln 0.8 + i pi) / dt with a REAL residue
    (not half of a pair: its conjugate is the same discrete pole).  Recovered to 1e-13 at the samples (measured 1.9e-15)."""
    from hydrochrono_amd.radiation_modes import fit_radiation_modes, modes_irf
    K, t = rm.negative_pole_samples()
    modes, r2 = fit_radiation_modes(K, t)
    resid = float(np.max(np.abs(modes_irf(modes, t) - K)))
    print(f"negative real pole: residual at the samples {resid:.3e}, modes {modes}")
    assert resid <= 1e-13
    assert len(modes) == 2
    osc = [m for m in modes if m[0].imag != 0.0]
    assert len(osc) == 1
    lam, rho = osc[0]
    assert lam.imag == np.pi / 0.05 and rho.imag == 0.0
    assert abs(lam.real - np.log(0.8) / 0.05) <= 1e-12 * abs(lam.real) and abs(rho.real - 3.0) <= 1e-12
    (lam_r, rho_r), = [m for m in modes if m[0].imag == 0.0]
    assert abs(lam_r.real - np.log(0.9) / 0.05) <= 1e-12 * abs(lam_r.real) and abs(rho_r - 2.0) <= 1e-12 and rho_r.imag == 0.0


def test_nested_state_space_is_the_concatenation_of_its_pairs():
    from hydrochrono_amd.radiation_modes import state_space_pairs_to_modes, state_space_to_modes
    D = 12
    A, B, C, pairs = rm.nested_state_space(D)
    assert sorted(np.shape(a)[0] for a, _, _ in pairs.values()) == [1, 2, 2, 3, 3, 4, 7]
    want = []
    for r, c in sorted(pairs):  # row-major pair order
        want += [(r, c, lam, rho) for lam, rho in state_space_to_modes(*pairs[(r, c)])]
    got = state_space_pairs_to_modes(A, B, C, D)
    assert got == want and len(got) >= len(pairs)
    # object arrays, as np.load(allow_pickle) or h5py hand them over
    Ao, Bo, Co = (np.empty((6, D), dtype=object) for _ in range(3))
    for r in range(6):
        for c in range(D):
            Ao[r, c], Bo[r, c], Co[r, c] = A[r][c], B[r][c], C[r][c]
    assert state_space_pairs_to_modes(Ao, Bo, Co, D) == want
    # every mode a list for the setter: ints in range, Re lambda < 0, at most 16 on a pair
    assert all(0 <= r < 6 and 0 <= c < D and lam.real < 0.0 for r, c, lam, _ in got)
    # nothing at all
    none = [[None] * D for _ in range(6)]
    assert state_space_pairs_to_modes(none, none, none, D) == []
    # the refusals reach the caller, whichever pair holds them
    for bad, match in (([[-1.0, 1.0], [0.0, -1.0]], "defective"), ([[0.1, 0.0], [0.0, -1.0]], "unstable")):
        A2 = [list(row) for row in A]
        B2 = [list(row) for row in B]
        C2 = [list(row) for row in C]
        A2[4][9], B2[4][9], C2[4][9] = bad, [0.0, 1.0], [1.0, 0.0]
        with pytest.raises(ValueError, match=match):
            state_space_pairs_to_modes(A2, B2, C2, D)
    A2 = [list(row) for row in A]
    A2[0][0] = np.zeros((2, 2)) - np.eye(2)  # the order of A against B and C of order 1
    with pytest.raises(ValueError):
        state_space_pairs_to_modes(A2, B, C, D)


def test_phase_shifted_sine_integral():
    """z_sine_phase, the analytic integral the three-body GPU test leans on: z_sine at phase 0, and with a phase the longdouble
    recurrence on a fine grid stays within its interpolation bound (omega h)^2 / 8 / |Re lambda| of it, without being vacuous."""
    omega, h = 5.0, 0.004
    for lam in (-0.8, -0.3 + 2.0j, -2.5 - 0.7j):
        assert abs(rm.z_sine_phase(lam, omega, 0.0, 0.37) - rm.z_sine(lam, omega, 0.37)) < 1e-18
        for phase in (0.61, 2.0, -1.1):
            ref = rm.ModalRef([[(0, lam, 1.0)]])
            worst = 0.0
            for tn in h * np.arange(160):
                ref.step(tn, [np.sin(omega * tn + phase)])
                worst = max(worst, float(abs(ref.snaps[-1][2][0][0] - rm.z_sine_phase(lam, omega, phase, tn))))
            bound = (omega * h) ** 2 / 8.0 / abs(complex(lam).real)
            assert 1e-3 * bound < worst <= bound, (lam, phase, worst, bound)
    many = rm.z_sine_phase(-0.8, omega, 0.61, h * np.arange(5))
    assert many.shape == (5,) and many[3] == rm.z_sine_phase(-0.8, omega, 0.61, 3 * h)
