"""CPU checks of the directional sea: the tests' longdouble reference (tests/directional_ref.py) against the long-crested references
and under rotation; the spreading-direction generator of the host math (hc::spreading_directions) through a stand-alone driver,
built plainly and under AddressSanitizer + UBSan; the code-object notes of the directional kernel instantiations."""
import os
import re
import subprocess

import numpy as np
import pytest

import directional_ref as dr
import morison_ref
import nonlinear_ref
import wave_kinematics_ref as wk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hydrochrono_amd", "csrc")


def components(nf=37, seed=2):
    rng = np.random.default_rng(seed)
    w = np.linspace(0.3, 2.4, nf)
    k = w * w / 9.81
    return rng.uniform(0.01, 0.2, nf), w, k, rng.uniform(0, 2 * np.pi, nf)


POINTS = np.array([[3.0, -7.0, -4.0], [-40.0, 12.5, -0.3], [0.0, 0.0, 0.4], [17.0, 3.0, -30.0]])
TIMES = np.array([0.0, 13.7])


# ---- the reference against the long-crested references ----
@pytest.mark.parametrize("depth,stretching,mwl", [(50.0, True, 0.3), (50.0, False, 0.0), (np.inf, True, 0.2)])
def test_theta_zero_is_the_long_crested_reference(depth, stretching, mwl):
    comp = components()
    got, _ = dr.kinematics(dr.with_directions(comp, 0.0), depth, POINTS, TIMES, mwl=mwl, stretching=stretching)
    (ref, scale) = wk.kinematics(comp, depth, POINTS, TIMES, mwl=mwl, stretching=stretching)
    for g, r, s in zip(got, ref, scale):
        assert np.all(np.abs(g - r) <= wk_tol() * s)
    assert not got[1][..., 1].any() and not got[2][..., 1].any()


def wk_tol():
    return 1e-11  # the bound of tests/test_gpu_wave_kinematics.py on the float64 restatement


def test_theta_zero_compositions_are_the_long_crested_ones():
    comp = components(nf=9)
    el = [(np.array([[1.0, 2.0, -3.0], [-2.0, 0.5, -1.0]]), np.full((2, 3), 0.7), np.full((2, 3), 0.4))]
    state = ([0.5, -1.0, 0.2], [0.1, -0.2, 0.6], [0.3, 0.1, -0.2], [0.02, 0.01, -0.03])
    a = dr.morison(dr.with_directions(comp, 0.0), 40.0, 1025.0, el, 3.3, *state, mwl=0.1, stretching=True)
    b = morison_ref.morison(comp, 40.0, 1025.0, el, 3.3, *state, mwl=0.1, stretching=True)
    assert np.all(np.abs(a["F"] - b["F"]) <= a["bound"] + b["bound"]) and np.abs(b["F"]).max() > 1.0
    tris = nonlinear_ref.box_triangles([-1.0, -1.5, -2.0], [1.0, 1.5, 0.5], m=2)
    pl = [nonlinear_ref.triangles_to_panels(tris)]
    a = dr.nonlinear(dr.with_directions(comp, 0.0), 40.0, 1025.0, 9.81, pl, 3.3, state[0], state[1], stretching=True)
    b = nonlinear_ref.nonlinear(comp, 40.0, 1025.0, 9.81, pl, 3.3, state[0], state[1], stretching=True)
    assert np.all(np.abs(a["fk"] - b["fk"]) <= a["bound_fk"] + b["bound_fk"]) and np.abs(b["fk"]).max() > 1.0
    assert wk.kinematics is not dr.kinematics  # the callbacks are restored


@pytest.mark.parametrize("depth", [35.0, np.inf])
def test_rotating_points_and_directions_together_rotates_the_vectors(depth):
    comp = components()
    rng = np.random.default_rng(5)
    theta = rng.uniform(-1.0, 1.0, comp[0].size)
    al = 0.83
    ca, sa = np.cos(al), np.sin(al)
    Rz = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
    (e0, v0, a0), (se, sv, sa_) = dr.kinematics(dr.with_directions(comp, theta), depth, POINTS, TIMES, mwl=0.1, stretching=True)
    (e1, v1, a1), _ = dr.kinematics(dr.with_directions(comp, theta + al), depth, POINTS @ Rz.T, TIMES, mwl=0.1, stretching=True)
    assert np.all(np.abs(e1 - e0) <= 1e-11 * se)
    for x0, x1, s in ((v0, v1, sv), (a0, a1, sa_)):
        assert np.all(np.abs(x1 - x0 @ Rz.T) <= 1e-11 * 2 * np.linalg.norm(s, axis=-1, keepdims=True))
    assert np.abs(v0[..., 1]).max() > 1e-3


def test_heading_interpolation_reference_hits_the_nodes():
    rng = np.random.default_rng(1)
    dirs, w = np.array([-0.5, 0.1, 0.9]), np.linspace(0.2, 2.0, 10)
    mag, ph = rng.uniform(1, 2, (6, 3, 10)), rng.uniform(-3, 3, (6, 3, 10))
    om = np.array([0.5, 1.234, 5.0])
    for j in range(3):
        m, p = dr.heading_tables(dirs, w, mag, ph, om, np.full(3, dirs[j]))
        for r in range(6):
            assert np.array_equal(m[r], dr.rao_omega(w, mag[r, j], om)) and np.array_equal(p[r], dr.rao_omega(w, ph[r, j], om))
    m, _ = dr.heading_tables(dirs, w, mag, ph, om, np.full(3, 0.5))
    assert np.allclose(np.asarray(m, dtype=float), 0.5 * (np.asarray(dr.heading_tables(dirs, w, mag, ph, om, np.full(3, 0.1))[0], dtype=float)
                                                          + np.asarray(dr.heading_tables(dirs, w, mag, ph, om, np.full(3, 0.9))[0], dtype=float)))


# ---- the spreading generator ----
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spread") / ("driver_" + request.param))
    flags = ["g++", "-std=c++17", "-g", "-O1"]
    if request.param == "sanitized":
        flags += ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]
    if request.param == "sanitized":  # is the sanitizer runtime there at all?  A failure of the real build below fails the test
        probe = tmp_path_factory.mktemp("probe") / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(flags + [str(probe), "-o", str(probe) + ".out"], capture_output=True).returncode != 0:
            pytest.skip("sanitizer runtime not available")
    r = subprocess.run(flags + ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "spreading_driver.cpp"), os.path.join(CSRC, "hc_host_math.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(nf, heading, s, n_bins, seed, expect=0):
        p = subprocess.run([out] + [repr(v) for v in (nf, heading, s, n_bins, seed)], capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        text = p.stdout + p.stderr
        assert p.returncode == expect, text[-2000:]
        assert "Sanitizer" not in text and "runtime error" not in text, text[-2000:]
        return np.array([float(v) for v in p.stdout.split()]) if expect == 0 else None
    return run


def quantiles(s, n_bins):
    """offsets with G(phi) = (m + 1/2) / n_bins from a numpy quadrature of cos^{2s}(phi / 2): composite Simpson on 2^20 cells,
    inverted by linear interpolation of the inverse between nodes 6e-6 rad apart (error ~ h^2 |D'| / D / 8, below 1e-10)"""
    n = 1 << 20
    phi = np.linspace(-np.pi, np.pi, 2 * n + 1).astype(np.longdouble)
    d = np.maximum(np.cos(phi / 2), 0) ** np.longdouble(2 * s)
    h = phi[2] - phi[0]
    cum = np.concatenate([[0], np.cumsum(h / 6 * (d[0:-2:2] + 4 * d[1::2] + d[2::2]))])
    target = (np.arange(n_bins) + 0.5) / n_bins * cum[-1]
    return np.interp(np.asarray(target, dtype=float), np.asarray(cum, dtype=float), np.asarray(phi[::2], dtype=float))


@pytest.mark.parametrize("s", [1, 10, 75])
def test_spreading_bins_are_the_quantiles_each_once_per_run(driver, s):
    n_bins, beta, nf = 9, 0.4, 9 * 5 + 4
    th = driver(nf, beta, float(s), n_bins, 7)
    assert th.size == nf
    q = quantiles(s, n_bins)
    bins = np.sort(th[:n_bins] - beta)
    assert np.max(np.abs(bins - q)) <= 1e-9, np.max(np.abs(bins - q))
    assert np.max(np.abs(bins + bins[::-1])) <= 4e-16  # symmetric about the heading (beta + phi, beta - phi round separately)
    for r in range(nf // n_bins):  # every run holds every bin once
        assert np.array_equal(np.sort(th[r * n_bins:(r + 1) * n_bins]), np.sort(th[:n_bins]))
    assert np.all(np.isin(th[-4:], th[:n_bins])) and len(set(th[-4:])) == 4


def test_spreading_collapse_seed_and_bad_arguments(driver):
    for s, nb in ((0.0, 9), (-2.0, 9), (10.0, 1)):
        assert np.array_equal(driver(12, -1.25, s, nb, 3), np.full(12, -1.25))
    a, b, c = driver(64, 0.0, 10.0, 16, 5), driver(64, 0.0, 10.0, 16, 5), driver(64, 0.0, 10.0, 16, 6)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.array_equal(np.sort(a[:16]), np.sort(c[:16]))
    assert not np.array_equal(a[:16], a[16:32])  # the runs are permuted independently
    assert driver(0, 0.0, 10.0, 4, 1).size == 0
    driver(4, 0.0, 10.0, 0, 1, expect=3)
    driver(4, float("nan"), 10.0, 4, 1, expect=3)


# ---- code-object notes of the directional instantiations ----
def test_directional_kernels_have_no_spills_and_no_scratch(tmp_path):
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    # kernel -> the long-crested kernel whose scalar-register figure it may not exceed (None: none spilled at all)
    wanted = {"hc_wave_kin.hip": {"wave_kinematics_kernelILb1E": None}, "hc_morison.hip": {"morison_dir_items_kernel": None},
              "hc_nonlinear.hip": {"nl_panels_dir_kernel": None, "nl_tris_dir_kernel": "nl_tris_kernel"}}
    for src, names in wanted.items():
        asm = str(tmp_path / (src + ".s"))
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"),
                        os.path.join(CSRC, src), "-o", asm], check=True)
        text = open(asm).read()
        blocks = re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s*\d+", text, flags=re.S)

        def note_of(name):
            m = [b for b in blocks if re.search(r"\.name:\s+\S*\d" + name + r"(E|I)", b)]
            assert len(m) == 1, (src, name, len(m))
            return lambda key: int(re.search(r"\." + key + r":\s*(\d+)", m[0]).group(1))

        for name, sibling in names.items():
            get = note_of(name)
            print(name, "vgpr", get("vgpr_count"), "sgpr spills", get("sgpr_spill_count"), "LDS", get("group_segment_fixed_size"))
            # no scratch, no spilled vector register (as tests/test_morison_ref_cpu.py reads it) and no spilled scalar register --
            # but for nl_tris_dir_kernel, which parks scalar registers in lanes of a vector register as the long-crested
            # nl_tris_kernel does (15 each; no memory is touched): no more of them than that kernel
            assert get("vgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
            assert get("sgpr_spill_count") <= (0 if sibling is None else note_of(sibling)("sgpr_spill_count")), name
            assert get("group_segment_fixed_size") <= 64 * 1024
