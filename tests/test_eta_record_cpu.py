"""Imported free-surface records without a GPU: the reference's eta file format (IrregularWaves::ReadEtaFromFile,
src/wave_types.cpp:480-500) as hydrochrono_amd/csrc/hc_eta_record.hpp parses it, the record validation, the zero extension the
kernels interpolate in (include/hydrochrono_amd.h, hc_set_wave_irregular_eta), and the C ABI / Python reader hc_read_eta_file."""
import math
import os
import subprocess

import pytest

from cases import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(GOLDEN_DIR, "sphere_eta_record.txt")
STUB = os.path.join(ROOT, "tests", "cpp", "chrono_stub")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eta") / "eta_record_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "eta_record_driver.cpp"), "-o", exe],
                   check=True)
    return exe


def run(driver, *args):
    r = subprocess.run([driver, *map(str, args)], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout.splitlines()


def write(tmp_path, text, name="eta.txt"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_parser_reads_the_sphere_record(driver):
    rc, out = run(driver, "parse", FIXTURE)
    assert rc == 0, out
    assert out[0] == "n 8001"
    assert out[1].split()[1:] == ["0", "-0"]
    last = out[2].split()
    assert float(last[1]) == 120.0 and float(last[2]) == -0.201588
    assert math.copysign(1.0, float(out[1].split()[2])) == -1.0  # "-0" is read as -0.0, as operator>> reads it


@pytest.mark.parametrize("text,bad", [("0 : 1\n0.5 ; 2\n", "0.5 ; 2"), ("0 : 1\n\n1 : 2\n", ""), ("0 : 1\n1 2\n", "1 2"),
                                      ("x : 1\n", "x : 1"), ("0 :\n", "0 :")])
def test_parser_rejects_bad_lines_with_the_reference_message(driver, tmp_path, text, bad):
    rc, out = run(driver, "parse", write(tmp_path, text))
    assert rc == 1 and out == [f"error Could not parse line: {bad}."]


def test_parser_rejects_a_missing_file(driver, tmp_path):
    path = str(tmp_path / "no_such_eta.txt")
    rc, out = run(driver, "parse", path)
    assert rc == 1 and out == [f"error Unable to open file at: {path}."]


def test_parser_takes_spaces_and_trailing_text_as_operator_extraction_does(driver, tmp_path):
    text = "  0.5   :   -1.25   trailing words\n1:2\t\n\t2.5 :3e-1xyz\n3 :4 : 5\n"
    rc, out = run(driver, "parse", write(tmp_path, text))
    assert rc == 0, out
    assert out == ["n 4", "first 0.5 -1.25", "last 3 4"]


@pytest.mark.parametrize("text", ["0 : 0\n1 : 0\n1 : 0\n", "0 : 0\n2 : 0\n1 : 0\n", "5 : 1\n"])
def test_validation_rejects_short_or_non_increasing_records(driver, tmp_path, text):
    rc, out = run(driver, "validate", write(tmp_path, text))
    assert rc == 1 and out[0].startswith("error "), out
    assert ("strictly increasing" in out[0]) or ("at least two" in out[0])


def test_zero_extension_covers_the_excitation_irf(driver, tmp_path):
    # record 0 .. 1 s at 0.25 s, IRF on [-0.6, 0.3]: ceil(0.3/0.25)+1 = 3 zeros before, ceil(0.6/0.25)+1 = 4 after
    path = write(tmp_path, "".join(f"{0.25 * i} : {i + 1}\n" for i in range(5)))
    rc, out = run(driver, "extend", path, -0.6, 0.3)
    assert rc == 0, out
    head = dict(line.split(" ", 1) for line in out[:6])
    assert float(head["h"]) == 0.25 and head["front"] == "3" and head["back"] == "4" and head["size"] == "12"
    assert [float(v) for v in head["t"].split()] == [-0.75, 2.0]
    assert [float(v) for v in head["record"].split()] == [0.0, 1.0]
    rows = [tuple(map(float, line.split())) for line in out[6:]]
    assert [r[0] for r in rows] == [-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0]
    assert [r[1] for r in rows] == [0, 0, 0, 1, 2, 3, 4, 5, 0, 0, 0, 0]
    # a causal IRF (tau_min = 0) still gets one zero after the record; a non-uniform record is extended at its MEAN spacing
    path = write(tmp_path, "10 : 1\n10.1 : 2\n10.4 : 3\n", "jitter.txt")
    rc, out = run(driver, "extend", path, 0.0, 0.5)
    head = dict(line.split(" ", 1) for line in out[:6])
    assert float(head["h"]) == (10.4 - 10.0) / 2 and head["front"] == str(math.ceil(0.5 / ((10.4 - 10.0) / 2)) + 1) and head["back"] == "1"
    rows = [tuple(map(float, line.split())) for line in out[6:]]
    assert all(b[0] > a[0] for a, b in zip(rows, rows[1:]))
    assert rows[-1][0] == 10.4 + (10.4 - 10.0) / 2 and rows[-1][1] == 0.0


def test_c_abi_and_python_reader(tmp_path):
    """hc_read_eta_file needs no context (and no GPU); hydrochrono_amd.read_eta_file wraps it."""
    import ctypes as C

    import numpy as np

    from hydrochrono_amd import HydroError, capi, read_eta_file
    t, eta = read_eta_file(FIXTURE)
    assert t.shape == eta.shape == (8001,)
    assert t[0] == 0.0 and t[-1] == 120.0 and eta[-1] == -0.201588 and t[1] == 0.015
    assert np.all(np.diff(t) > 0)
    lib = capi.load()
    n = C.c_int()
    small = np.empty(10)
    rc = lib.hc_read_eta_file(FIXTURE.encode(), small.ctypes.data_as(capi.c_double_p), small.ctypes.data_as(capi.c_double_p), 10, C.byref(n))
    assert rc == capi.HC_ERR_OUT_OF_RANGE and n.value == 8001
    with pytest.raises(HydroError, match=r"Could not parse line: 1 ; 2\."):
        read_eta_file(write(tmp_path, "0 : 1\n1 ; 2\n"))
    missing = str(tmp_path / "missing.txt")
    with pytest.raises(HydroError) as e:
        read_eta_file(missing)
    assert e.value.status == capi.HC_ERR_RUNTIME and f"Unable to open file at: {missing}." in str(e.value)


def test_demo_shaped_caller_compiles_against_the_chrono_stub(tmp_path):
    """The eta-import demo's hydro lines (IrregularWaveParams::eta_file_path_ -> IrregularWaves -> TestHydro::AddWaves) build
    warning-free; tests/test_gpu_eta_record.py runs them."""
    from hydrochrono_amd import build as hb
    hb.build()
    libdir = os.path.join(ROOT, "hydrochrono_amd", "lib")
    out = str(tmp_path / "eta_import_demo")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", STUB, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "eta_import_demo.cpp"), "-o", out, "-L", libdir, "-lhydrochrono_amd",
                    f"-Wl,-rpath,{libdir}"], check=True)
    assert os.path.exists(out)
