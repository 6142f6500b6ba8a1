"""The component analysis of an imported eta record without a GPU: the host parts (hydrochrono_amd/csrc/hc_eta_components.hpp --
uniformity test, resampling, band, modular phase, origin rotation, selection) against the NumPy restatement
(tests/eta_components_ref.py), the restatement itself against records of known cosines, and the build of the kernels
(csrc/hc_eta_components.hip: no scratch, no spilled register).  The GPU side is tests/test_gpu_eta_components.py.

The driver is built twice with plain g++: -Wall -Werror, and once more as a stand-alone program with -fsanitize=address,undefined;
every case runs through both."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import eta_components_ref as er
from cases import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN_DIR, "sphere_eta_record.txt")
STUB = os.path.join(ROOT, "tests", "cpp", "chrono_stub")
SRC = os.path.join(ROOT, "tests", "cpp", "eta_components_driver.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("etac") / f"eta_components_driver_{request.param}")
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True)
    return exe


def run(driver, *args):
    r = subprocess.run([driver, *map(repr_arg, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return r.stdout.splitlines()


def repr_arg(v):
    return repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)


def write_record(tmp_path, t, eta, name="rec.txt"):
    p = tmp_path / name
    p.write_text("".join(f"{float(a)!r} : {float(b)!r}\n" for a, b in zip(t, eta)))
    return str(p)


def test_uniform_record_is_used_as_given(driver):
    out = run(driver, "grid", FIXTURE)
    from hydrochrono_amd import read_eta_file
    t, eta = read_eta_file(FIXTURE)
    assert float(out[0].split()[1]) == er.mean_spacing(t) and out[1] == "uniform 1" and er.is_uniform(t)
    assert np.array_equal(np.array([float(v) for v in out[2:]]), eta)


def test_uniformity_threshold(driver, tmp_path):
    """|t[j] - (t[0] + j h)| <= 1e-9 h: a sample moved by a little less is uniform, by a little more is not."""
    n, h = 33, 0.25  # (every grid value is exact in binary)
    for shift, uniform in ((0.9e-9 * h, 1), (1.1e-9 * h, 0)):
        t = 2.0 + np.arange(n) * h
        t[7] += shift
        out = run(driver, "grid", write_record(tmp_path, t, np.sin(t)))
        assert out[1] == f"uniform {uniform}" and er.is_uniform(t) == bool(uniform)


def test_resampling_is_the_linear_interpolant_at_mean_spacing(driver, tmp_path):
    rng = np.random.default_rng(5)
    n, h = 257, 0.05
    t = 3.7 + np.arange(n) * h
    t[1:-1] += rng.uniform(-0.3, 0.3, n - 2) * h
    eta = np.cos(1.3 * t) + 0.3 * np.sin(4.1 * t + 0.2)
    out = run(driver, "grid", write_record(tmp_path, t, eta))
    assert out[1] == "uniform 0"
    got = np.array([float(v) for v in out[2:]])
    ref = er.grid_samples(t, eta)
    assert got.shape == ref.shape == (n,)
    # two evaluations of the same interpolant, w1 e1 + w2 e2 against e1 + slope (q - t1): a few roundings of max|eta| apart
    assert np.abs(got - ref).max() <= 8 * np.finfo(float).eps * np.abs(eta).max()
    assert got[0] == eta[0] and got[-1] == eta[-1]


@pytest.mark.parametrize("n,T_w,f_min,f_max", [(64, 3.2, 0.0, 1e9), (64, 3.2, 5 / 3.2, 9 / 3.2), (257, 12.85, 0.3, 0.31), (8001, 120.015, 0.03, 0.4),
                                               (8001, 120.015, -1.0, 0.001), (8001, 120.015, 40.0, 50.0), (5, 1.0, 1.0, 2.0),
                                               (4096, 204.8, 10.0, 10.0), (4096, 204.8, 2.0, 1.0)])
def test_band_is_the_set_of_bins_inside_the_closed_interval(driver, n, T_w, f_min, f_max):
    lo, hi = (int(v) for v in run(driver, "bins", n, T_w, f_min, f_max)[0].split())
    ref = er.band_bins(n, T_w, f_min, f_max)
    if ref.size == 0:
        assert lo > hi
    else:
        assert (lo, hi) == (ref[0], ref[-1]) and ref.size == hi - lo + 1


@pytest.mark.parametrize("n,m,s,stride", [(64, 32, 0, 256), (8001, 4000, 255, 256), (2 ** 31 - 1, 2 ** 30 - 1, 200, 256),
                                          (2 ** 31 - 2, 2 ** 30 - 1, 2 ** 31 - 3, 1), (1048576, 4096, 17, 256)])
def test_modular_phase_is_exact_in_64_bit_integers(driver, n, m, s, stride):
    got = [int(v) for v in run(driver, "phase", n, m, s, stride, 40)]
    assert got == [(m * (s + i * stride)) % n for i in range(40)]


@pytest.mark.parametrize("m,T_w,t0", [(16, 25.6, 0.0), (51, 12.85, 3.7), (1365, 204.8, -5.0), (4000, 120.015, 1.0e6), (7, 3.2, -123456.789)])
def test_origin_rotation_reduces_the_product_before_the_trigonometry(driver, m, T_w, t0):
    re, im = 0.3, -0.4
    got = [float(v) for v in run(driver, "rotate", re, im, m, T_w, t0)[0].split()]
    cyc = (Fraction(m) * Fraction(t0) / Fraction(T_w)) % 1  # exact
    ang = 2 * er.PI_LD * er._ld(cyc)
    ref = complex((er.LD(re) + 1j * er.LD(im)) * (np.cos(ang) + 1j * np.sin(ang)))
    # the long double product m t0 / T_w carries 2^-64 of its size into the angle: |m t0 / T_w| 2^-63 pi, plus the rounding to double
    tol = 0.5 * (abs(m * t0 / T_w) * 2.0 ** -63 * 2 * np.pi + 4 * np.finfo(float).eps)
    assert abs(complex(*got) - ref) <= tol, (got, ref)


@pytest.mark.parametrize("amps,k", [([0.1, 0.5, 0.3, 0.5, 0.2], 2), ([0.1, 0.5, 0.3, 0.5, 0.2], 1), ([0.2, 0.2, 0.2, 0.2], 3), ([0.4, 0.1, 0.3], 3),
                                    ([0.4, 0.1, 0.3], 7), ([0.4, 0.1, 0.3], 0), ([0.4, 0.1, 0.3], -2), ([0.0, 1.0, 0.0, 1.0, 1.0, 0.5], 4)])
def test_selection_keeps_the_largest_with_ties_to_the_lower_bin(driver, amps, k):
    got = [int(v) for v in run(driver, "select", k, *[float(a) for a in amps])]
    assert got == list(er.select(amps, k)) and got == sorted(got)
    if k == 2 and len(amps) == 5:
        assert got == [1, 3]
    if k == 1 and len(amps) == 5:
        assert got == [1]  # the tie between bins 1 and 3 goes to bin 1
    if k == 3 and len(amps) == 4:
        assert got == [0, 1, 2]


@pytest.mark.parametrize("n,t0", [(64, 0.0), (257, 3.7), (4096, -5.0)])
def test_the_yardstick_recovers_cosines_on_the_grid(n, t0):
    """What tests/test_gpu_eta_components.py leans on: the long double restatement returns the (A, phi) a record was built from."""
    comps = er.five_cosines(n)
    t, eta = er.on_grid_record(n, t0, 0.05, comps)
    r = er.analyse(t, eta, 0.0, np.inf)
    assert list(r["m"]) == list(range(1, n // 2 + 1))
    amax = max(a for _, a, _ in comps)
    A = r["A"].copy()
    for m, a, phi in comps:
        assert abs(A[m - 1] - a) <= 3e-15
        assert abs((r["phase"][m - 1] - phi + np.pi) % (2 * np.pi) - np.pi) <= 3e-13
        A[m - 1] = 0.0
    assert A.max() <= 7e-14 * amax


def test_kernels_build_without_scratch_or_spills(tmp_path):
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not found")
    from hydrochrono_amd import build as hb
    co = str(tmp_path / "hc_eta_components.co")
    subprocess.run([hb._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--genco", "--no-gpu-bundle-output", "-Wno-unused-result",
                    "-I", os.path.join(ROOT, "include"), os.path.join(hb.CSRC, "hc_eta_components.hip"), "-o", co], check=True)
    txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    notes = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4))) for m in re.finditer(
        r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", txt, re.S)}
    assert any("eta_dft_kernel" in n for n in notes) and any("eta_residual_kernel" in n for n in notes), sorted(notes)
    for name, (scratch, vgpr, spills) in notes.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert "hc_eta_components.hip" in hb.SOURCES and "hc_eta_components.hpp" in hb.HEADERS


def test_abi_declares_the_entry_points():
    from hydrochrono_amd import capi
    from hydrochrono_amd.hydro import HydroForces, HydroGroup
    lib = capi.load()
    for name in ("hc_set_eta_record_components", "hc_clear_eta_record_components", "hc_get_eta_record_components"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    assert lib.hc_set_eta_record_components(None, 0.0, 1.0, 0) == capi.HC_ERR_INVALID
    assert lib.hc_clear_eta_record_components(None) == capi.HC_ERR_INVALID
    for cls in (HydroForces, HydroGroup):
        for name in ("set_eta_record_components", "clear_eta_record_components", "eta_record_components"):
            assert callable(getattr(cls, name))


def test_cpp_caller_compiles_against_the_mirror(tmp_path):
    """tests/cpp/eta_components_caller.cpp (IrregularWaves::SetRecordComponents / GetRecordComponents / GetSpectrum of
    include/hydroc_amd/wave_types.h) builds warning-free; tests/test_gpu_eta_components.py runs it."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "eta_components_caller")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", STUB, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "eta_components_caller.cpp"), "-o", out, "-L", libdir, "-lhydrochrono_amd",
                    f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
