"""Clipped surface triangles on the GPU (hc_set_surface_triangles, nl_tris_kernel of csrc/hc_nonlinear.hip) beside the centroid panels
of the same mesh (nl_panels_kernel): the time of one hc_compute_nonlinear at 64 bodies x 2048 triangles x 512 components (the C3
system of bench.py, as profiles/nonlinear_probe.py), stretching on (an eta pass and a pressure pass) and off (one pass).

Both kinds are timed in ONE run on one context pair, in alternating windows (clipped, panels, clipped, ...), each call a host clock
around hc_compute_nonlinear, which ends in a stream synchronise; the figure of a kind is the median over all of its windows, the
windows' own medians give the spread.  --parts k runs the launches alone for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/surface_clip_probe.py --parts k --stretching 1

    python profiles/surface_clip_probe.py [--out DIR] [--tag TAG] [--quick]

Writes DIR/probe<tag>.json (default profiles/surface_clip) and prints it.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import nonlinear_probe as nlp  # noqa: E402  (the C3 system, the states, the clock)

N_TRI = 2048


def mesh(n, seed):
    """n triangles of about 0.5 m over a hull-sized region that spans the surface: all four wet / dry cases occur"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-10.0, 10.0, size=(n, 1, 3))
    centre[:, 0, 2] = rng.uniform(-6.0, 3.0, size=n)
    return centre + rng.uniform(-0.5, 0.5, size=(n, 3, 3))


def configured(HF, clip, stretching):
    from hydrochrono_amd.hydro import triangles_to_panels
    h = nlp.c3(HF)
    for b in range(nlp.N_BODIES):
        tri = mesh(N_TRI, 50 + b)
        if clip:
            h.set_surface_mesh(b, tri, clip=True)
        else:
            h.set_surface_panels(b, *triangles_to_panels(tri))
    h.set_nonlinear_options(wave_stretching=bool(stretching))
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_clip"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--stretching", type=int, default=1)
    args = ap.parse_args()
    import torch  # noqa: F401  (loads the ROCm runtime the library binds to)
    from hydrochrono_amd.hydro import HydroForces as HF
    st = nlp.states(nlp.N_BODIES, [37.1])[0]
    if "k" in args.parts:
        for clip in (True, False):
            h = configured(HF, clip, args.stretching)
            for _ in range(70):
                h.compute_nonlinear(37.1, st[0], st[1])
            h.close()
        return
    windows, per = (3, 20) if args.quick else (5, 100)
    res = {}
    for stretching in (1, 0):
        hs = {"clipped": configured(HF, True, stretching), "panels": configured(HF, False, stretching)}
        nf = hs["clipped"].sizes()["nf"]
        samples = {k: [] for k in hs}
        for h in hs.values():
            for _ in range(20):
                h.compute_nonlinear(37.1, st[0], st[1])
        for _ in range(windows):
            for kind, h in hs.items():
                samples[kind].append(nlp.timed(lambda: h.compute_nonlinear(37.1, st[0], st[1]), per))
        out = {}
        for kind, h in hs.items():
            buoy, fk, _ = h.compute_nonlinear(37.1, st[0], st[1])
            out[kind] = dict(nlp.stats_us(np.concatenate(samples[kind])), window_medians_us=[float(1e6 * np.median(w)) for w in samples[kind]],
                             max_abs_buoy=float(np.abs(buoy).max()), max_abs_fk=float(np.abs(fk).max()))
            h.close()
        out["items"], out["nf"] = nlp.N_BODIES * N_TRI, nf
        out["point_component_evaluations"] = dict(clipped=3 * nlp.N_BODIES * N_TRI * nf, panels=nlp.N_BODIES * N_TRI * nf)
        out["ratio_of_medians_clipped_over_panels"] = out["clipped"]["median_us"] / out["panels"]["median_us"]
        res[f"c3_{nlp.N_BODIES}x{N_TRI}x{nf}_stretching{stretching}"] = out
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"probe{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
