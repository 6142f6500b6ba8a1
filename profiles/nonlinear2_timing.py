"""Time of one hc_compute_nonlinear on a closed 1000-triangle mesh (a UV sphere: 502 vertices) at 512 wave components, clipped
triangles, order 1 against order 2 (hc_set_nonlinear_second_order): host clock around the call, copies and launches
included, median of the repeats after a warm-up, in alternating windows of one run.  Prints one JSON line.
    python profiles/nonlinear2_timing.py [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def uv_sphere(radius=3.0, n_lon=25, n_lat=21):
    """2 * n_lon + 2 * n_lon * (n_lat - 2) triangles, normals outward"""
    th = np.linspace(0.0, np.pi, n_lat + 1)[1:-1]
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = lambda t: np.stack([radius * np.sin(t) * np.cos(ph), radius * np.sin(t) * np.sin(ph), np.full(n_lon, radius * np.cos(t))], axis=1)
    rings = [ring(t) for t in th]
    top, bot = np.array([0.0, 0.0, radius]), np.array([0.0, 0.0, -radius])
    tris = []
    for i in range(n_lon):
        j = (i + 1) % n_lon
        tris.append([top, rings[0][i], rings[0][j]])
        tris.append([bot, rings[-1][j], rings[-1][i]])
        for a, b in zip(rings[:-1], rings[1:]):
            tris.append([a[i], b[i], b[j]])
            tris.append([a[i], b[j], a[j]])
    return np.array(tris)


def main():
    import torch  # noqa: F401
    from hydrochrono_amd.hydro import HydroForces
    from hydrochrono_amd.synthetic import many_body_case
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    h = HydroForces.from_case(many_body_case(1, S=64, dt_rirf=0.05, n_exc=64, dt_exc=0.25, seed=7, water_depth=60.0))
    h.add_waves_irregular(simulation_dt=0.05, simulation_duration=100.0, ramp_duration=20.0, wave_height=2.0, wave_period=8.0,
                          frequency_min=0.03, frequency_max=0.6, nfrequencies=512, peak_enhancement_factor=2.0, seed=4)
    mesh = uv_sphere()
    h.set_surface_mesh(0, mesh, clip=True)
    pos, rpy = np.array([[0.3, -0.1, -0.4]]), np.array([[0.1, -0.05, 0.2]])
    times = {1: [], 2: []}
    for window in range(4):
        for order in (1, 2):
            h.set_nonlinear_second_order(order == 2)
            for r in range(repeats + 3):
                t0 = time.perf_counter()
                h.compute_nonlinear(33.0, pos, rpy)
                if r >= 3:  # the first calls of a window build tables and point lists
                    times[order].append(time.perf_counter() - t0)
    points = h.nonlinear_point_count(0)
    h.close()
    print(json.dumps(dict(triangles=len(mesh), points=points, components=512, order1_us=1e6 * float(np.median(times[1])),
                          order2_us=1e6 * float(np.median(times[2])), samples=len(times[1]))))


if __name__ == "__main__":
    main()
