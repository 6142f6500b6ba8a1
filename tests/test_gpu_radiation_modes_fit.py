"""The modal radiation term from fitted and state-space data to forces, on the GPU: a body described by its file's IRF and the same
body described by modes fitted to that IRF (tests/radiation_modes_ref.fit_body) give the same force within what the fit, the
modal term's interpolation and the convolution's own quadrature allow -- (a) compute_radiation_modes against the CPU oracle's
convolution, (b) through step, (c) three bodies with cross-body columns, where a transposed pair shows; (d)
HydroForces.set_radiation_state_space on the device; (e) a mode from a negative real discrete pole, x.y = pi at h = dt.  The CPU
side is tests/test_radiation_modes_fit_cpu.py; the kernel's own ulp tests are tests/test_gpu_radiation_modes.py.

The bound of (a) to (c), row by row at every step:  |M - O| <= B_interp + |A - O_fit| + rho sum_c |amp_c| L1_rc  with
  M      the modal term of the GPU, O the convolution of the file's K (CPU oracle; in (b) the GPU's own),
  A      the analytic integral of K_fit against v (longdouble), O_fit the oracle's convolution of K_fit,
  B_interp = (omega dt)^2 / 8 sum rho |res| |amp_c| / |Re lambda|: the modal term interpolates v linearly over a step (|M - A|),
  |A - O_fit| the oracle's own discretisation error at that step, computed, not bounded,
  L1_rc = dt sum_k |K_fit(tau_k) - K(tau_k)|: the oracle's quadrature weights are at most dt (trapezoid widths on a uniform
         grid) and its interpolated |v_c| at most |amp_c|, so |O_fit - O| <= rho sum_c |amp_c| L1_rc; asserted on the oracle alone.
A pair the fit leaves without modes (max |K_rc| <= 1e-6 max |K|) has K_fit = 0 and L1_rc = dt sum |K_rc|."""
import copy

import numpy as np
import pytest

import radiation_modes_ref as rm
from cases import load_into_oracle, sphere_case, three_body_case
from test_gpu_radiation_modes import C_ULP, same_bits, small_case

pytestmark = pytest.mark.gpu
LD = np.longdouble
SPHERE_FIT = dict(max_order=16, r2_min=0.999999)
THREE_BODY_FIT = dict(max_order=14, r2_min=1.0 - 1e-8)
SPHERE_AMP = np.array([1.0, -0.6, 0.8, 0.3, -0.5, 0.2])
SPHERE_OMEGA = 2.0


@pytest.fixture(scope="module")
def HF():
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces
    return HydroForces


def split(v):
    v = np.asarray(v).reshape(-1, 6)
    return np.ascontiguousarray(v[:, :3]).reshape(-1), np.ascontiguousarray(v[:, 3:]).reshape(-1)


def fit_case(case, fit_opts):
    """{body: modes}, the L1 matrix [6N][D] (fitted pairs: fit_body's; the others: dt sum |K_rc|) and the smallest R^2."""
    D = 6 * case["N"]
    modes, L1, r2 = {}, np.zeros((D, D)), 1.0
    for b, bd in enumerate(case["bodies"]):
        K, t = np.asarray(bd["rirf_K"], dtype=np.float64).reshape(6, D, -1), np.asarray(bd["rirf_t"], dtype=np.float64)
        modes[b], per_pair = rm.fit_body(K, t, D, **fit_opts)
        L1[6 * b:6 * b + 6] = (t[1] - t[0]) * np.abs(K).sum(axis=2)
        for (r, c), (n, pair_r2, l1) in per_pair.items():
            L1[6 * b + r, c] = l1
            r2 = min(r2, pair_r2)
    return modes, L1, r2


class Reference:
    """Everything of the bound that no GPU force enters, computed once per case: the oracle on the file's K (O) and on K_fit
    (O_fit, K_fit as the device evaluates it), the analytic integral A, B_interp and the L1 term.  v_c(t) = amp_c sin(omega t +
    phase_c) at times n dt."""

    def __init__(self, case, modes, L1, K_fit, amp, omega, phase, dt, steps):
        N, rho = case["N"], case["rho"]
        D = 6 * N
        self.amp, self.omega, self.phase = np.asarray(amp, dtype=np.float64), float(omega), np.asarray(phase, dtype=np.float64)
        self.times = dt * np.arange(steps + 1)
        fitted = copy.deepcopy(case)
        for b, bd in enumerate(fitted["bodies"]):
            bd["rirf_K"] = np.ascontiguousarray(K_fit[b])
        orc, orc_fit = load_into_oracle(case), load_into_oracle(fitted)
        self.O, self.O_fit = np.zeros((steps + 1, D)), np.zeros((steps + 1, D))
        for n, t in enumerate(self.times):
            lv, av = split(self.velocity(t))
            self.O[n], self.O_fit[n] = orc.compute_radiation(t, lv, av), orc_fit.compute_radiation(t, lv, av)
        A = np.zeros((steps + 1, D), dtype=LD)
        self.B_interp = np.zeros(D)
        for b, lst in modes.items():
            for r, c, lam, res in lst:
                z = rm.z_sine_phase(lam, omega, self.phase[c], self.times)
                A[:, 6 * b + r] += (rm.CLD(rho * complex(res)) * z).real * LD(self.amp[c])
                self.B_interp[6 * b + r] += rho * abs(res) * abs(self.amp[c]) / abs(complex(lam).real)
        self.B_interp *= (omega * dt) ** 2 / 8.0
        self.A = A.astype(np.float64)
        self.L1_term = rho * (L1 @ np.abs(self.amp))
        self.rhs = self.B_interp[None, :] + np.abs(self.A - self.O_fit) + self.L1_term[None, :]

    def velocity(self, t):
        return self.amp * np.sin(self.omega * t + self.phase)

    def check_alone(self, cap=0.05):
        """The last link on the reference alone, and the condition that keeps the bound a check: the largest right-hand side is
        at most 5 % of max |O|."""
        assert np.all(np.abs(self.O_fit - self.O) <= self.L1_term[None, :]), float(np.max(np.abs(self.O_fit - self.O) - self.L1_term[None, :]))
        top = float(np.abs(self.O).max())
        assert top > 0.0 and float(self.rhs.max()) <= cap * top, (float(self.rhs.max()), top)
        return float(self.rhs.max()) / top

    def report(self, what, got, against=None):
        """Asserts |got - O| <= rhs row by row at every step; prints the worst ratio and the three parts there."""
        err = np.abs(got - (self.O if against is None else against))
        live = self.rhs > 0.0
        assert not err[~live].any()  # a row the bound leaves nothing: exact zeros on both sides
        ratio = np.zeros_like(err)
        ratio[live] = err[live] / self.rhs[live]
        n, r = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print(f"{what}: worst |M - O| / RHS = {ratio[n, r]:.3e} at step {n}, row {r}: |M - O| {err[n, r]:.3e}, B_interp {self.B_interp[r]:.3e}, "
              f"|A - O_fit| {abs(self.A[n, r] - self.O_fit[n, r]):.3e}, L1 term {self.L1_term[r]:.3e}; max |O| {np.abs(self.O).max():.3e}, "
              f"largest RHS {self.rhs.max():.3e} ({self.rhs.max() / np.abs(self.O).max():.2%} of max |O|)")
        assert np.all(err <= self.rhs), (what, int(n), int(r), float(ratio[n, r]))
        return float(ratio[n, r])


_SPHERE = {}


def sphere_reference(HF):
    if not _SPHERE:
        from hydrochrono_amd.radiation_modes import modes_irf
        case = sphere_case()
        modes, L1, r2 = fit_case(case, SPHERE_FIT)
        assert r2 >= SPHERE_FIT["r2_min"] and len(modes[0]) == 52
        h = HF.from_case(case)
        h.set_radiation_modes(0, modes[0])
        tau = np.asarray(case["bodies"][0]["rirf_t"], dtype=np.float64)
        K = np.asarray(case["bodies"][0]["rirf_K"], dtype=np.float64).reshape(6, 6, -1)
        K_fit = h.radiation_modes_irf(0, tau)
        want = np.zeros_like(K_fit)
        for r, c, lam, res in modes[0]:
            want[r, c] += modes_irf([(lam, res)], tau)
        assert np.max(np.abs(K_fit - want)) <= 1e-14 * np.abs(K).max()
        dt = 0.015
        steps = int(round(3 * 2 * np.pi / SPHERE_OMEGA / dt))  # three periods, 9.4 s: inside the file's 15 s window
        assert steps * dt < tau[-1]
        ref = Reference(case, modes, L1, [K_fit], SPHERE_AMP, SPHERE_OMEGA, np.zeros(6), dt, steps)
        _SPHERE.update(case=case, modes=modes[0], ref=ref, share=ref.check_alone())
    return _SPHERE


def test_sphere_fitted_modes_against_the_files_convolution(HF):
    """(a) compute_radiation_modes with the 52 fitted modes against the oracle's convolution of the file's K, v = amp sin 2t on the
    file's own dt = 0.015 for three periods."""
    s = sphere_reference(HF)
    ref = s["ref"]
    h = HF.from_case(s["case"])
    h.set_radiation_modes(0, s["modes"])
    M = np.array([h.compute_radiation_modes(t, *split(ref.velocity(t))) for t in ref.times])
    assert not M[0].any() and np.all(np.isfinite(M))
    ref.report("sphere, fitted modes against the file's convolution", M)
    assert np.abs(M).max() > 0.5 * np.abs(ref.O).max()


def test_sphere_modes_only_against_irf_only_through_step(HF):
    """(b) step of a handle with a zero IRF and the fitted modes against step of the plain sphere handle, the same regular wave and
    the same prescribed state: the radiation parts within the bound of (a), the hydrostatic and wave parts the same bits."""
    s = sphere_reference(HF)
    ref, case = s["ref"], s["case"]
    bd = case["bodies"][0]
    plain = HF.from_case(case)
    only = HF(1)
    only.set_simulation_parameters(case["rho"], case["g"], case["water_depth"])
    only.set_body(0, bd["disp_vol"], bd["cg"], bd["cb"], bd["lin"], bd["added_mass_inf"], [0.0, 0.05], np.zeros((6, 6, 2)))
    only.set_zero_rirf(0)
    only.set_body_excitation_rao(0, bd["w"], bd["ex_mag"], bd["ex_phase"])
    only.set_body_excitation_irf(0, bd["ex_irf_t"], bd["ex_irf_f"])
    only.finalize()
    for h in (plain, only):
        h.add_waves_regular(0.3, 1.1)
    only.set_radiation_modes(0, s["modes"])
    cg = np.asarray(bd["cg"], dtype=np.float64)
    eps = np.finfo(np.float64).eps
    conv, modal = np.zeros_like(ref.O), np.zeros_like(ref.O)
    for n, t in enumerate(ref.times):
        q = SPHERE_AMP * (1.0 - np.cos(SPHERE_OMEGA * t)) / SPHERE_OMEGA  # the motion whose velocity is v
        lv, av = split(ref.velocity(t))
        st = (cg + 0.2 * q[:3], 0.05 * q[3:], lv, av)
        f_plain, f_only = plain.step(t, *st), only.step(t, *st)
        hs_p, conv[n], wv_p = plain.components()
        hs_o, rad_o, wv_o = only.components()
        modal[n] = only.radiation_modes()
        assert same_bits(hs_p, hs_o) and same_bits(wv_p, wv_o) and not rad_o.any(), n
        assert same_bits(f_only, (hs_o - rad_o + wv_o) - modal[n]) and same_bits(f_plain, hs_p - conv[n] + wv_p), n
        # the totals differ by conv - modal, but for the roundings of the two sums
        round_off = 4.0 * eps * (np.abs(hs_p) + np.abs(wv_p) + np.abs(conv[n]) + np.abs(modal[n]))
        assert np.all(np.abs((f_only - f_plain) - (conv[n] - modal[n])) <= round_off), n
    assert np.abs(conv).max() > 0.5 * np.abs(ref.O).max() and np.abs(hs_p).max() > 0.0 and np.abs(wv_p).max() > 0.0
    # the GPU's convolution is the oracle's to 1e-6 (the suite's contract, far below every term of the bound)
    assert np.max(np.abs(conv - ref.O)) <= 1e-6 * np.abs(ref.O).max()
    ref.report("sphere, modes only against IRF only through step", modal, against=conv)


def test_three_bodies_cross_body_columns(HF):
    """(c) the three-body file, 324 one-mode pairs with cross-body columns, v_c = (1 + 0.07 c) sin(5 t + 0.61 c) over 31 steps of
    0.02 (inside the 0.62 s window): the bound of (a) with the per-column analytic integral, and the bits of the whole context on
    HydroGroup shards (0, 1) and (1, 3).  K is not symmetric here: a transposed pair misses the bound."""
    from hydrochrono_amd.hydro import HydroGroup
    case = three_body_case()
    N, D = 3, 18
    modes, L1, r2 = fit_case(case, THREE_BODY_FIT)
    assert r2 >= THREE_BODY_FIT["r2_min"] and sum(len(m) for m in modes.values()) == 324
    K0 = np.asarray(case["bodies"][0]["rirf_K"], dtype=np.float64).reshape(6, D, -1)
    assert np.abs(K0[:, :6] - K0[:, :6].transpose(1, 0, 2)).max() > 0.1 * np.abs(K0).max()

    def handle(body_range=None):
        h = HF.from_case(case, body_range=body_range)
        for b, lst in modes.items():
            h.set_radiation_modes(b, lst)
        return h
    whole = handle()
    tau = np.asarray(case["bodies"][0]["rirf_t"], dtype=np.float64)
    K_fit = [whole.radiation_modes_irf(b, tau) for b in range(N)]
    c = np.arange(D)
    ref = Reference(case, modes, L1, K_fit, 1.0 + 0.07 * c, 5.0, 0.61 * c, 0.02, 31)
    assert ref.times[-1] <= tau[-1] + 1e-12
    ref.check_alone()
    M = np.array([whole.compute_radiation_modes(t, *split(ref.velocity(t))) for t in ref.times])
    ref.report("three bodies, fitted modes against the file's convolution", M)
    assert np.abs(M).max() > 0.5 * np.abs(ref.O).max()
    grp = HydroGroup([handle((0, 1)), handle((1, 3))])
    G = np.array([grp.compute_radiation_modes(t, *split(ref.velocity(t))) for t in ref.times])
    assert same_bits(M, G)


def irregular_times(n, seed, t0=0.2):
    rng = np.random.default_rng(seed)
    return np.concatenate([[t0], t0 + np.cumsum(np.exp(rng.uniform(np.log(1e-3), np.log(0.3), size=n)))])


def drive_velocity(D, t):
    c = np.arange(D)
    return (1.0 + 0.07 * c) * np.sin(0.9 * t + 0.61 * c) + 0.3 * np.cos(2.3 * t - 0.2 * c)


def test_set_radiation_state_space_on_the_device(HF):
    """(d) N = 2: the nested [6][D] structure of orders 1, 2, 3, 4 and 7 with None and empty pairs on both bodies, through
    set_radiation_state_space: the device's K against C exp(A tau) B (longdouble Taylor series), the forces with the bits of a handle
    given state_space_pairs_to_modes' lists, the same through a HydroGroup, and the refusals."""
    from hydrochrono_amd.hydro import HydroError, HydroGroup
    from hydrochrono_amd.radiation_modes import state_space_pairs_to_modes
    N, D = 2, 12
    case = small_case(N)
    nested = {b: rm.nested_state_space(D, seed=11 + b) for b in range(N)}
    ss, direct = HF.from_case(case), HF.from_case(case)
    grp = HydroGroup([HF.from_case(case, body_range=(0, 1)), HF.from_case(case, body_range=(1, 2))])
    for b, (A, B, C, pairs) in nested.items():
        ss.set_radiation_state_space(b, A, B, C)
        grp.set_radiation_state_space(b, A, B, C)
        lst = state_space_pairs_to_modes(A, B, C, D)
        direct.set_radiation_modes(b, lst)
        assert ss.radiation_mode_count(b) == len(lst) == grp.radiation_mode_count(b) and len(lst) >= len(pairs)
    taus = np.array([0.0, 0.013, 0.4, 2.5])
    for b, (A, B, C, pairs) in nested.items():
        K = ss.radiation_modes_irf(b, taus)
        assert K.shape == (6, D, 4)
        for r in range(6):
            for c in range(D):
                if (r, c) not in pairs:
                    assert not K[r, c].any(), (b, r, c)
                    continue
                Ap, Bp, Cp = pairs[(r, c)]
                for k, tau in enumerate(taus):
                    want = float(np.asarray(Cp, dtype=LD) @ rm.expm_taylor(Ap, tau) @ np.asarray(Bp, dtype=LD))
                    assert abs(K[r, c, k] - want) <= 1e-12 * max(1.0, np.abs(Bp).max() * np.abs(Cp).max() * len(Bp)), (b, r, c, tau)
    times = irregular_times(8, 13)
    F = [np.array([h.compute_radiation_modes(t, *split(drive_velocity(D, t))) for t in times]) for h in (ss, direct, grp)]
    assert np.abs(F[0]).max() > 0.0
    assert same_bits(F[0], F[1]) and same_bits(F[0], F[2])
    # a defective, an unstable or an oversized pair raises and leaves the body's modes as they were
    before = ss.radiation_mode_count(1)
    A, B, C, _ = nested[1]
    for bad, b_vec, c_vec, exc in (([[-1.0, 1.0], [0.0, -1.0]], [0.0, 1.0], [1.0, 0.0], ValueError),
                                   ([[0.1, 0.0], [0.0, -1.0]], [1.0, 1.0], [1.0, 1.0], ValueError),
                                   (np.diag(-1.0 - np.arange(17.0)), np.ones(17), np.ones(17), HydroError)):  # 17 modes on one pair
        A2, B2, C2 = ([list(row) for row in X] for X in (A, B, C))
        A2[4][9], B2[4][9], C2[4][9] = bad, b_vec, c_vec
        for h in (ss, grp):
            with pytest.raises(exc):
                h.set_radiation_state_space(1, A2, B2, C2)
            assert h.radiation_mode_count(1) == before
    t_next = times[-1] + 0.07
    v = split(drive_velocity(D, t_next))
    assert same_bits(ss.compute_radiation_modes(t_next, *v), direct.compute_radiation_modes(t_next, *v))


def test_negative_real_pole_mode_on_the_device(HF):
    """(e) the two-mode fit of 3 (-0.8)^k + 2 0.9^k on one pair: Im lambda = pi / dt with a real residue, so Im(lambda h) = pi
    exactly at h = dt.  Ten steps of h = dt and ten irregular ones against the longdouble restatement within the C_ULP bound."""
    from hydrochrono_amd.radiation_modes import fit_radiation_modes
    K, t = rm.negative_pole_samples()
    fitted, _ = fit_radiation_modes(K, t)
    assert len(fitted) == 2 and any(lam.imag == np.pi / 0.05 and res.imag == 0.0 for lam, res in fitted)
    modes = {0: [(1, 4, lam, res) for lam, res in fitted]}
    case = small_case(1)
    h = HF.from_case(case)
    h.set_radiation_modes(0, modes[0])
    assert np.max(np.abs(h.radiation_modes_irf(0, t)[1, 4] - K)) <= 1e-13
    ref = rm.ModalRef(rm.device_rows(modes, 0, 1, case["rho"]))
    times = 0.05 * np.arange(11)
    times = np.concatenate([times, irregular_times(10, 17, t0=times[-1])[1:]])
    worst = 0.0
    for n, tn in enumerate(times):
        v = drive_velocity(6, tn)
        got = h.compute_radiation_modes(tn, *split(v))
        want = ref.step(tn, v)
        if n == 0:
            assert not got.any()
            continue
        bound = ref.bound(C_ULP)
        err = np.abs(np.asarray(got, dtype=LD) - want).astype(np.float64)
        assert not np.delete(got, 1).any() and got[1] != 0.0
        worst = max(worst, float(err[1] / bound[1]))
        assert err[1] <= bound[1], (n, worst)
    print(f"negative real pole on the device: worst |gpu - ref| / bound = {worst:.3e} over {len(times) - 1} steps")
