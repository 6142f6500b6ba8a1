"""Input sets shared by tests/test_wave2_ref_cpu.py (which establishes that plain FP64 reaches the tolerance on each of them) and
tests/test_gpu_wave_kinematics2.py: the sphere case (200 m depth) and the three-body case (infinite depth) of the wave-kinematics
tests with small spectra of 1, 2, 63, 64, 65 and 257 components -- the sizes around the wave width and the 256-component LDS tile --
up to 70 points and 3 times, with z above the mean level, at it, deep enough that e^{k z} underflows for most components, at the
bed and below it.  The references are computed once per (set, bands) and shared."""
import functools

import numpy as np

import wave2_ref as w2
from cases import SPHERE_DT, sphere_case, three_body_case

TOL = 1e-11  # the project's figure for the wave kinematics (tests/test_gpu_wave_kinematics.py)
NO_PAIR = (100.0, 200.0)  # rad/s: a band no pair of these spectra reaches
BANDS = {  # name -> (diff_band, sum_band)
    "full": (w2.FULL, w2.FULL),
    "diff_only": (w2.FULL, NO_PAIR),
    "sum_only": (NO_PAIR, w2.FULL),
    "cut": ((0.05, 0.9), (1.5, 6.0)),  # both cut through the matrix; the difference band leaves the diagonal out
    "empty": (NO_PAIR, NO_PAIR),
}
MWL = 0.3


def _grid(xs, zs):
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    return np.stack([X.ravel(), np.full(X.size, 1.5), Z.ravel()], axis=1)


SPHERE_Z = np.array([1.5, MWL, -0.4, -3.0, -12.0, -60.0, -150.0, -199.0, -200.0 + MWL, -260.0])  # k h = 800 at the bed for the 1 Hz component
THREE_Z = np.array([1.0, MWL, -0.5, -3.0, -20.0, -80.0, -300.0, -1000.0, -3000.0, -8000.0])      # e^{k z} = 0 from k = 0.25 on
XS = np.linspace(-140.0, 160.0, 7)
TIMES = np.array([7.3, 20.0, 41.7])  # inside the ramp of 20 s, at its end, after it


def sphere_waves(nf, frequency_min=0.02, frequency_max=1.0):
    return dict(simulation_dt=SPHERE_DT, simulation_duration=60.0, ramp_duration=20.0, wave_height=2.0, wave_period=12.0,
                frequency_min=frequency_min, frequency_max=frequency_max, nfrequencies=nf, seed=2)


def three_waves(nf):
    return dict(simulation_dt=0.01, simulation_duration=40.0, ramp_duration=20.0, wave_height=2.0, wave_period=7.0,
                frequency_min=0.05, frequency_max=0.8, nfrequencies=nf, seed=3)


# name -> (case, wave parameters, points, times)
SETS = {
    # one and two components between 0.07 and 0.11 Hz (k h = 4 .. 10): on the range of the larger sets a two-component JONSWAP
    # spectrum has an amplitude of 2e-80 at 0.02 Hz, and the products of such amplitudes lie below the range of FP64 altogether
    # (tests/test_wave2_ref_cpu.py: no FP64 evaluation reaches the tolerance there), so that range was not kept for these two
    "sphere1": ("sphere", sphere_waves(1, 0.07, 0.11), _grid(XS[:2], SPHERE_Z), TIMES[:2]),
    "sphere2": ("sphere", sphere_waves(2, 0.07, 0.11), _grid(XS[:2], SPHERE_Z), TIMES[:2]),
    "sphere63": ("sphere", sphere_waves(63), _grid(XS[:3], SPHERE_Z), TIMES),
    "three64": ("three", three_waves(64), _grid(XS[:3], THREE_Z), TIMES),
    "sphere65": ("sphere", sphere_waves(65), _grid(XS, SPHERE_Z), TIMES),  # the batch of 70 x 3
    "three65": ("three", three_waves(65), _grid(XS[:2], THREE_Z), TIMES[1:]),
    "sphere257": ("sphere", sphere_waves(257), _grid(XS[2:4], SPHERE_Z), TIMES[:1]),
    "three257": ("three", three_waves(257), _grid(XS[:2], THREE_Z), TIMES[2:]),
}


def case_of(name):
    return sphere_case() if SETS[name][0] == "sphere" else three_body_case()


@functools.lru_cache(maxsize=None)
def reference(name, bands, comp_key, g, depth, dtype=np.longdouble):
    """(values, scales) of wave2_ref.fields for a set under the named bands; comp_key = the components as bytes (cache key)."""
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    _, waves, pts, times = SETS[name]
    diff_band, sum_band = BANDS[bands]
    return w2.fields(comp, g, depth, pts, times, mwl=MWL, diff_band=diff_band, sum_band=sum_band,
                     ramp_duration=waves["ramp_duration"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference_tables(bands, comp_key, g, depth, dtype=np.longdouble):
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    diff_band, sum_band = BANDS[bands]
    return w2.pair_tables(comp, g, depth, diff_band, sum_band, dtype)


def key(comp):
    return tuple(np.ascontiguousarray(v, dtype=np.float64).tobytes() for v in comp)
