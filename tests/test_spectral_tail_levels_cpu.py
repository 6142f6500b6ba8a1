"""CPU test of the LEVELS of the spectral radiation tail (hydrochrono_amd/csrc/hc_tail.hpp: tail_levels, host-only C++).  For window
lengths around every threshold and both look-ahead depths: the level set, lag ranges and partition counts; every lag from 128 on is
covered by exactly one (level, partition, tap) and no lag below 128 by any; and a NumPy restatement of the levelled overlap-save --
each level's windows and zero rule as the header gives them, every level restarting on its own period inside the top period, the far
partitions of a level that makes them ahead taken from the windows of the period before -- equals the direct longdouble lag sum over
the lags from 128 on at every step of three top periods, to the row-wise bound of tests/tail_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tail_ref as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [512, 513, 700, 1023, 1024, 1030, 1536, 2049]
HEAD = 128  # the lags below stay with the head pass


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("levels") / "tail_levels_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "tail_levels_dump.cpp"), "-o", exe], check=True)
    return exe


_cache = {}


def load(exe, S, L, form=1):
    key = (S, L, form)
    if key in _cache:
        return _cache[key]
    out = subprocess.run([exe, str(S), str(L), str(form)], capture_output=True, text=True, check=True).stdout.splitlines()
    g = {"levels": [], "head": int(out[0].split()[3])}
    assert int(out[0].split()[1]) >= 0
    for ln in out[1:]:
        f = ln.split()
        if f[0] == "level":
            lv = dict(zip(f[2::2], map(int, f[3::2])))
            lv.update(starts=[], chunks=[], win={}, tap={})
            g["levels"].append(lv)
        elif f[0] == "start":
            g["levels"][int(f[1])]["starts"].append(int(f[2]))
        elif f[0] == "chunk":
            g["levels"][int(f[1])]["chunks"].append((int(f[3]), int(f[4])))
        elif f[0] == "win":
            g["levels"][int(f[1])]["win"][(int(f[2]), int(f[3]))] = (int(f[4]), int(f[5]))
        elif f[0] == "tap":
            g["levels"][int(f[1])]["tap"][(int(f[2]), int(f[3]))] = (int(f[4]), int(f[5]))
    assert len(g["levels"]) == int(out[0].split()[1])
    _cache[key] = g
    return g


def expected_levels(S):
    """(P, NP, lag_lo, lag_hi), largest P first -- DESIGN.md 3.2a."""
    if S >= 1024:
        return [(512, -(-S // 512) - 1, 512, S), (256, 1, 256, 512), (128, 1, 128, 256)]
    return [(256, -(-S // 256) - 1, 256, S), (128, 1, 128, 256)]


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("L", [16, 32])
def test_level_set_lag_ranges_and_partitions(dump_exe, S, L):
    g = load(dump_exe, S, L)
    got = [(lv["P"], lv["NP"], lv["lag_lo"], lv["lag_hi"]) for lv in g["levels"]]
    assert got == expected_levels(S)
    assert g["head"] == HEAD
    top = g["levels"][0]
    for lv in g["levels"]:
        assert lv["N"] == 2 * lv["P"] and lv["bins"] == lv["P"] + 1 and lv["period"] == lv["P"] and lv["blocks"] * L == lv["P"]
        # every period is aligned to the start of the largest one, and starts on a block
        assert lv["starts"] == list(range(0, top["P"], lv["P"]))
        assert lv["NP"] <= -(-S // 256) - 1  # never more partitions than the uniform form: NP_level * D <= kTailMaxCols wherever that is eligible
        if lv["far_ahead"]:
            assert lv is top and lv["P"] == 256 and lv["NP"] > 1
            ch = lv["chunks"]
            assert len(ch) == lv["blocks"] - 1 and ch[0][0] == 0 and ch[-1][1] == lv["bins"]
            assert all(ch[i][1] == ch[i + 1][0] for i in range(len(ch) - 1))
    # the uniform form is the one level of 256 with all its partitions
    u = load(dump_exe, S, L, 2)
    assert [(lv["P"], lv["NP"], lv["lag_lo"], lv["lag_hi"]) for lv in u["levels"]] == [(256, -(-S // 256) - 1, 256, S)] and u["head"] == 256


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("L", [16, 32])
def test_every_lag_from_128_on_is_covered_exactly_once(dump_exe, S, L):
    g = load(dump_exe, S, L)
    count = np.zeros(S + 2048, dtype=int)
    for lv in g["levels"]:
        for (p, r), (lag, live) in lv["tap"].items():
            if live:
                assert lv["lag_lo"] <= lag < lv["lag_hi"], (lv["P"], p, r, lag)
                count[lag] += 1
    assert np.all(count[:HEAD] == 0), np.flatnonzero(count[:HEAD])
    assert np.all(count[HEAD:S] == 1), HEAD + np.flatnonzero(count[HEAD:S] != 1)
    assert np.all(count[S:] == 0)


def level_rows(lv, G, v, m0, m_prev):
    """The P rows [j][row] of one level's period that starts at sample index m0 (v [T][D] oldest first; G [R][D][S]); the far
    partitions of a level that makes them ahead come from the windows taken at m_prev, the start of the period before (None: the
    fallback, this period's own windows)."""
    P, N, NP = lv["P"], lv["N"], lv["NP"]
    R, D, S = G.shape

    def windows(at):
        X = np.zeros((NP + 1, D, N))
        for (a, k), (back, live) in lv["win"].items():
            if live:
                X[a, :, k] = v[at - 1 - back]
        return np.fft.rfft(X, axis=-1)  # [a][col][bin]

    H = np.zeros((NP + 1, R, D, N))
    for (p, r), (lag, live) in lv["tap"].items():
        if live:
            H[p, :, :, r] = G[:, :, lag]
    Kh = np.fft.rfft(H, axis=-1)  # [p][row][col][bin]
    X_cur = windows(m0)
    Y = np.einsum("rcb,cb->br", Kh[1], X_cur[1])
    if NP > 1:
        if lv["far_ahead"] and m_prev is not None:
            X_prev = windows(m_prev)
            for lo, hi in lv["chunks"]:  # a chunk of bins beside each block of the period before: window p - 1 for partition p
                for p in range(2, NP + 1):
                    Y[lo:hi] += np.einsum("rcb,cb->br", Kh[p][:, :, lo:hi], X_prev[p - 1][:, lo:hi])
        else:
            for p in range(2, NP + 1):
                Y += np.einsum("rcb,cb->br", Kh[p], X_cur[p])
    return np.fft.irfft(Y, n=N, axis=0)[P:]


@pytest.mark.parametrize("S", SHAPES)
@pytest.mark.parametrize("L", [16, 32])
def test_levelled_overlap_save_equals_direct_sum(dump_exe, S, L):
    g = load(dump_exe, S, L)
    R, D = 2, 3
    rng = np.random.default_rng(S * 100 + L)
    G = rng.standard_normal((R, D, S))  # a flat envelope: the oldest lag weighs as much as the newest
    top = g["levels"][0]
    T = S + 8 + 3 * top["P"]
    v = rng.standard_normal((T, D))
    G_tail = G.copy()
    G_tail[:, :, :HEAD] = 0.0  # the reference: the lags from 128 on
    ref = TR.TailRef(G_tail, np.ones(S), list(range(R)))
    first = S + 8  # sample index of the first step of the first top period
    rows = {}      # level index -> (period start, [j][row])
    starts_before = {}
    steps, got = [], []
    for n in range(3 * top["P"]):
        m, j_top = first + n, n % top["P"]
        total = np.zeros(R)
        for i, lv in enumerate(g["levels"]):
            if j_top % L == 0 and j_top in lv["starts"]:
                rows[i] = (m, level_rows(lv, G, v, m, starts_before.get(i)))
                starts_before[i] = m
            m0, y = rows[i]
            assert 0 <= m - m0 < lv["P"]
            total = total + y[m - m0]
        steps.append(m)
        got.append(total)
    worst = ref.check(v, steps, got, f"S {S} L {L}: ")
    print(f"S {S} L {L}: max |d| / (1e-12 A_m) = {worst:.2e} over {len(steps)} steps")
