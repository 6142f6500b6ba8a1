"""CPU test of the spectral radiation tail's index arithmetic (hydrochrono_amd/csrc/hc_tail.hpp, host-only C++): an overlap-save
convolution in NumPy that takes its windows, partitions, K-hat / X-hat columns and far-chunk bin ranges from the header reproduces
the direct lag sum  sum_{s >= P} G_s v_{m-s}  for the P steps of a superblock -- this superblock's near partition from this
superblock's windows, the far partitions from the windows of the superblock BEFORE it (as the far chunks make them), and the
fallback that makes the far part from this superblock's own windows.  S a multiple of P and not, both look-ahead depths."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tail") / "tail_index_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tail_index_dump.cpp"), "-o", exe], check=True)
    return exe


def load(exe, S, L, D):
    out = subprocess.run([exe, str(S), str(L), str(D)], capture_output=True, text=True, check=True).stdout.splitlines()
    head = out[0].split()
    g = dict(zip(head[0::2], map(int, head[1::2])))
    g["chunks"] = [tuple(map(int, ln.split()[2:])) for ln in out if ln.startswith("chunk ")]
    win = {}
    cols = {}
    for ln in out:
        f = ln.split()
        if f[0] == "win":
            win[(int(f[1]), int(f[2]))] = (int(f[3]), int(f[4]))
        elif f[0] == "col":
            cols[(int(f[1]), int(f[2]))] = int(f[3])
        elif f[0] == "shift":
            g["shift_cur"], g["shift_next"] = int(f[1]), int(f[2])
    g["win"], g["cols"] = win, cols
    return g


def windows(g, S, D, vhist):
    """X-hat [bins][NP*D] of the windows at a superblock start; vhist[b] = sample b behind the newest (b = 0: step m0 - 1)."""
    P, N, NP = g["P"], g["N"], g["NP"]
    X = np.zeros((NP, D, N))
    for a in range(1, NP + 1):
        for k in range(N):
            back, live = g["win"][(a, k)]
            if live:
                X[a - 1, :, k] = vhist[back]
    Xh = np.fft.rfft(X, axis=-1)  # [NP][D][bins]
    return np.transpose(Xh, (2, 0, 1)).reshape(Xh.shape[2], NP * D)


def khat(g, G, D):
    """K-hat [bins][rows][NP*D] from G[s][row][col] (S lags)."""
    P, N, NP = g["P"], g["N"], g["NP"]
    S, rows = G.shape[0], G.shape[1]
    Kh = np.zeros((g["bins"], rows, NP * D), dtype=complex)
    for p in range(1, NP + 1):
        h = np.zeros((rows, D, N))
        seg = G[p * P:min(S, (p + 1) * P)]  # [r][row][col]
        h[:, :, :seg.shape[0]] = np.transpose(seg, (1, 2, 0))
        H = np.fft.rfft(h, axis=-1)  # [row][col][bins]
        for c in range(D):
            Kh[:, :, g["cols"][(p, c)]] = H[:, c, :].T
    return Kh


def gemv(Kh, X, bins, col_lo, col_hi, shift):
    lo, hi = bins
    return np.einsum("brc,bc->br", Kh[lo:hi, :, col_lo:col_hi], X[lo:hi, col_lo + shift:col_hi + shift])


def direct_tail(G, v, m0, P, S):
    """sum_{s = P .. S-1} G_s v_{m-s} for the P steps m = m0 .. m0 + P - 1 of a superblock: [j][row]."""
    Gm = np.transpose(G[P:S], (1, 0, 2)).reshape(G.shape[1], -1)  # [row][(s - P) * D + col]
    return np.stack([Gm @ v[m0 + j - S + 1:m0 + j - P + 1][::-1].reshape(-1) for j in range(P)])


@pytest.mark.parametrize("S", [1024, 700, 512])
@pytest.mark.parametrize("L", [16, 32])
def test_overlap_save_with_header_indices_equals_direct_sum(dump_exe, S, L):
    overlap_save_against_direct_sum(dump_exe, S, L, 6, seed=S + L)


@pytest.mark.parametrize("S", [512, 513, 700, 767, 768, 769, 1024, 1300, 8448])
@pytest.mark.parametrize("L", [16, 32])
@pytest.mark.parametrize("D", [6, 30])
def test_overlap_save_at_partition_edges_and_widths(dump_exe, S, L, D):
    """One lag in the last partition (513, 769), S around a partition boundary, many partitions (8448: NP = 32), two widths."""
    overlap_save_against_direct_sum(dump_exe, S, L, D, seed=S + L + D)


def overlap_save_against_direct_sum(dump_exe, S, L, D, seed):
    rows = 4
    g = load(dump_exe, S, L, D)
    P, NP, Q = g["P"], g["NP"], g["Q"]
    assert NP == -(-S // P) - 1 and Q * L == P
    assert g["chunks"][0][0] == 0 and g["chunks"][-1][1] == g["bins"]
    assert len(g["chunks"]) == Q - 1 and all(g["chunks"][i][1] == g["chunks"][i + 1][0] for i in range(Q - 2))
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((S, rows, D))  # a flat envelope: the oldest lag weighs as much as the newest
    T = 3 * P + S  # samples 0 .. T-1; superblock q starts at step m0
    v = rng.standard_normal((T, D))
    Kh = khat(g, G, D)
    m_prev, m0 = T - 2 * P, T - P  # two consecutive superblocks
    X_prev = windows(g, S, D, v[m_prev - 1::-1])
    X_cur = windows(g, S, D, v[m0 - 1::-1])
    Y_far = np.zeros((g["bins"], rows), dtype=complex)
    for lo, hi in g["chunks"]:  # made during the superblock before, one chunk per block after its first
        Y_far[lo:hi] = gemv(Kh, X_prev, (lo, hi), D, NP * D, g["shift_next"]) if NP > 1 else 0.0
    Y_fallback = gemv(Kh, X_cur, (0, g["bins"]), D, NP * D, g["shift_cur"]) if NP > 1 else 0.0
    Y_near = gemv(Kh, X_cur, (0, g["bins"]), 0, D, g["shift_cur"])
    direct = direct_tail(G, v, m0, P, S)
    for name, Yf in (("far chunks", Y_far), ("fallback", Y_fallback)):
        y = np.fft.irfft(Yf + Y_near, n=g["N"], axis=0)[P:]  # [j][row]
        err = np.max(np.abs(y - direct), axis=1)
        j = int(np.argmax(err))
        assert err[j] <= 1e-11 * np.max(np.abs(direct)), f"{name}: step j = {j} of the superblock, error {err[j]:.3e}"


# ---- tail_grid_ok (hc_tail.hpp): the eligibility test of a superblock's grid --------------------------------------------------------
def grid_ok(exe, times, tau, dt, t_first):
    """hc::tail_grid_ok(times newest first, tau, dt, t_first) through the driver's "grid" mode."""
    arg = " ".join(["%d %d" % (len(times), len(tau))] + ["%.17g" % x for x in list(times) + list(tau) + [dt, t_first]])
    out = subprocess.run([exe, "grid"], input=arg, capture_output=True, text=True, check=True).stdout.split()
    return out == ["1"]


def tols(dt, t_first, tau_last):
    eps = np.finfo(np.float64).eps
    return max(1e-9 * dt, 64.0 * eps * abs(t_first)), max(1e-9 * dt, 64.0 * eps * abs(tau_last))


@pytest.mark.parametrize("S", [512, 700])
def test_tail_grid_ok_edges(dump_exe, S):
    dt, t0 = 2.0 ** -7, 64.0  # t0: the newest history sample; t_first = t0 + dt
    tau = np.arange(S) * dt
    t_first = t0 + dt
    tol_t, tol_s = tols(dt, t_first, tau[-1])

    def hist(n):
        return t0 - dt * np.arange(n)

    # the history must hold S samples on the grid (and reach past the oldest query: S samples reach S dt back)
    assert grid_ok(dump_exe, hist(S), tau, dt, t_first)
    assert not grid_ok(dump_exe, hist(S - 1), tau, dt, t_first)
    # the first predicted step: on the grid within the planner's tolerance
    assert grid_ok(dump_exe, hist(S + 4), tau, dt, t_first + 0.9 * tol_t)
    assert grid_ok(dump_exe, hist(S + 4), tau, dt, t_first - 0.9 * tol_t)
    assert not grid_ok(dump_exe, hist(S + 4), tau, dt, t_first + 1.1 * tol_t)
    assert not grid_ok(dump_exe, hist(S + 4), tau, dt, t_first - 1.1 * tol_t)
    # one history time of the window off the grid
    for k in (1, S // 2, S - 1):
        h = hist(S + 4)
        h[k] += 0.9 * tol_t
        assert grid_ok(dump_exe, h, tau, dt, t_first), k
        h[k] += 0.2 * tol_t
        assert not grid_ok(dump_exe, h, tau, dt, t_first), k
    # one IRF time off the grid of the step
    for s in (1, 256, S - 1):
        ts = tau.copy()
        ts[s] += 0.9 * tol_s
        assert grid_ok(dump_exe, hist(S + 4), ts, dt, t_first), s
        ts[s] += 0.2 * tol_s
        assert not grid_ok(dump_exe, hist(S + 4), ts, dt, t_first), s
    # the margin: the oldest kept sample must lie more than tau_{S-1} + 8 tol_t before t_first (samples past index S - 1 are not
    # held to the grid)
    margin = 8.0 * tol_t
    for delta, ok in ((0.25 * margin, True), (-0.25 * margin, False)):
        h = hist(S + 1)
        h[-1] = t_first - tau[-1] - margin - delta
        assert grid_ok(dump_exe, h, tau, dt, t_first) == ok, delta
    # a step other than the IRF spacing
    assert not grid_ok(dump_exe, t0 - 1.5 * dt * np.arange(S + 4), tau, 1.5 * dt, t0 + 1.5 * dt)


def test_tail_grid_ok_needs_two_partitions(dump_exe):
    dt, t0 = 2.0 ** -7, 64.0
    for S, ok in ((511, False), (512, True)):
        assert grid_ok(dump_exe, t0 - dt * np.arange(S + 4), np.arange(S) * dt, dt, t0 + dt) == ok, S
