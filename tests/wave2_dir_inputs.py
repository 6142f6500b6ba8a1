"""Input sets shared by tests/test_wave2_dir_ref_cpu.py (which establishes that plain FP64 reaches the tolerance on each of them) and
tests/test_gpu_wave_kinematics2_dir.py: the sphere case (200 m) and the three-body case (infinite depth) of tests/wave2_inputs.py
with spectra of 2, 63, 64, 65 and 257 components -- around the wave width and the 256-component LDS tile -- and one direction per
component; at most 3 x-values x 2 y-values x the ten depths of wave2_inputs, 1 to 3 of its times.  The direction sets: a
deterministic spread within +-1.2 rad, the cos-2s generator, the spread with two neighbouring components 1e-9 rad apart (what the
sigma form of DESIGN.md 3.7n exists for), and components that oppose each other (beta and beta + pi).  The references are computed
once per (set, bands) and shared."""
import functools

import numpy as np

import wave2_dir_ref as wd
import wave2_inputs as wi
from wave2_inputs import BANDS, MWL, TOL, key  # noqa: F401  (the same bands, mean level, tolerance and cache key)

YS = np.array([-35.0, 50.0])


def grid(xs, ys, zs):
    X, Y, Z = np.meshgrid(xs, ys, zs, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def spread(nf):
    return 1.2 * np.sin(2.3 * np.arange(nf) + 0.4)


def near(nf):
    th = spread(nf)
    th[nf // 2 + 1] = th[nf // 2] + 1e-9
    return th


def oppose(nf):
    return 0.4 + np.pi * (np.arange(nf) % 2)


def cos2s(nf):
    from hydrochrono_amd.hydro import wave_spreading_directions  # host math of the library: no GPU
    return wave_spreading_directions(nf, 0.3, s=10, n_bins=15, seed=2)


# name -> (case, wave parameters, points, times, directions of nf components)
SETS = {
    "sphere2_oppose": ("sphere", wi.sphere_waves(2, 0.07, 0.11), grid(wi.XS[:3], YS, wi.SPHERE_Z), wi.TIMES[:2], oppose),
    "sphere63_spread": ("sphere", wi.sphere_waves(63), grid(wi.XS[:3], YS, wi.SPHERE_Z), wi.TIMES, spread),
    "three64_cos2s": ("three", wi.three_waves(64), grid(wi.XS[:3], YS, wi.THREE_Z), wi.TIMES[:2], cos2s),
    "sphere65_near": ("sphere", wi.sphere_waves(65), grid(wi.XS[1:3], YS, wi.SPHERE_Z), wi.TIMES[1:], near),
    "three65_oppose": ("three", wi.three_waves(65), grid(wi.XS[:2], YS, wi.THREE_Z), wi.TIMES[2:], oppose),
    "sphere257_cos2s": ("sphere", wi.sphere_waves(257), grid(wi.XS[3:4], YS, wi.SPHERE_Z), wi.TIMES[:1], cos2s),
    "three257_spread": ("three", wi.three_waves(257), grid(wi.XS[:1], YS, wi.THREE_Z), wi.TIMES[2:], spread),
}


def case_of(name):
    from cases import sphere_case, three_body_case
    return sphere_case() if SETS[name][0] == "sphere" else three_body_case()


def directions(name):
    return np.ascontiguousarray(SETS[name][4](SETS[name][1]["nfrequencies"]), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, bands, comp_key, g, depth, dtype=np.longdouble):
    """(values, scales) of wave2_dir_ref.fields for a set under the named bands; comp_key = the components as bytes (cache key)."""
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    _, waves, pts, times, _ = SETS[name]
    diff_band, sum_band = BANDS[bands]
    return wd.fields(comp, directions(name), g, depth, pts, times, mwl=MWL, diff_band=diff_band, sum_band=sum_band,
                     ramp_duration=waves["ramp_duration"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference_tables(name, bands, comp_key, g, depth, dtype=np.longdouble):
    comp = tuple(np.frombuffer(b, dtype=np.float64) for b in comp_key)
    diff_band, sum_band = BANDS[bands]
    return wd.pair_tables(comp, directions(name), g, depth, diff_band, sum_band, dtype)
