"""The host side of the second-order wave kinematics (hydrochrono_amd/csrc/hc_wave_kin2.hpp: argument validation, band limits of the
pair matrix, ramp factor) in a stand-alone program under AddressSanitizer and UBSan; no GPU, no library."""
import os

from test_host_sanitizers import ROOT, build, run_clean


def test_validation_and_band_limits_under_sanitizers(tmp_path):
    exe = build(str(tmp_path / "wave_kin2_host_check"), [os.path.join(ROOT, "tests", "cpp", "wave_kin2_host_check.cpp")], [])
    assert "wave_kin2 host check: 0 failures" in run_clean([exe])
