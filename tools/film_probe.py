#!/usr/bin/env python
"""The film pass on one 1024^2 Cornell frame: python tools/film_probe.py [--spp 64] [--repeats 5]
Prints ms_film of the three ways records reach the packed gather — fused by k_raygen (the default), re-laid (film_fused 0), in place (film_relayout 0) — and of the
wide pass (a filter radius of 1.5), alternating between them for `--repeats` rounds so that drift lands on all of them alike.  Against another build of the library:
TRHIP_LIB=/path/to/libtracehip.so python tools/film_probe.py."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()
scene, cam = T.scenes.cornell_scene(), T.scenes.cornell_camera(1024)
f = cam.film
wide = T.PerspectiveCamera(cam.camera_to_world, T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0,
                           T.Film(list(f.resolution), T.Bounds2(f.crop_window[:2], f.crop_window[2:]), T.LanczosSincFilter([1.5, 1.5], 3.0), f.diagonal_mm, f.scale, ""))
ctx = T.default_context()
VARIANTS = (("fused", cam, {}), ("re-laid", cam, {"film_fused": 0}), ("in place", cam, {"film_relayout": 0}), ("wide", wide, {}))
ms = {name: [] for name, _, _ in VARIANTS}
for r in range(a.repeats + 1):  # round 0 warms up
    for name, c, opts in VARIANTS:
        for o, v in opts.items():
            ctx.set_option(o, v)
        try:
            integ = T.PathIntegrator(c, T.SeededSampler(a.spp, seed=1), 8)
            integ.render(scene, ctx)
        finally:
            for o in opts:
                ctx.set_option(o, 1)
        if r:
            ms[name].append(integ.stats.ms_film)
            print(f"round {r} {name:9s} ms_film {integ.stats.ms_film:.3f} ms_total {integ.stats.ms_total:.2f}", flush=True)
for name, v in ms.items():
    print(f"{name:9s} ms_film median {statistics.median(v):.3f} min {min(v):.3f} max {max(v):.3f}  ({' '.join(f'{x:.3f}' for x in v)})")
