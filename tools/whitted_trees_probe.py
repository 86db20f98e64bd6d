#!/usr/bin/env python
"""tools/whitted_trees_probe.py LABEL: what cutting wide Whitted trees into smaller batches costs (docs/design/09-whitted.md, profiles/r12/whitted_trees.txt).

C1's Whitted leg (shadows, 256 x 256, 8 spp, depth 5): stats.ms_total of five runs after a warm-up — a frame that fits its queues must cost what it did.  Then the frames of
tests/test_gpu_whitted_trees.py whose trees are wider than the queues of a sample pass, twice each: ms_total, n_batches and the ray counts, or the library's refusal.
A/B against another build of the library: TRHIP_LIB=/path/to/libtracehip.so python tools/whitted_trees_probe.py parent"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
T = g.load_package()
import whitted_trees as wt
label = sys.argv[1]
ctx = T.default_context()
scene = T.scenes.shadows_scene()
cam = T.scenes.shadows_camera(256)
ms, nb = [], []
for i in range(6):
    integ = T.WhittedIntegrator(cam, T.SeededSampler(8, seed=0x5EED0001), 5)
    integ.render(scene)
    if i:
        ms.append(integ.stats.ms_total); nb.append(integ.stats.n_batches)
print(f"{label}: C1 whitted shadows 256x256 8spp depth5 ms_total (5 runs after a warm-up): " + " ".join(f"{m:.3f}" for m in ms) + f" | median {np.median(ms):.3f} min {min(ms):.3f} max {max(ms):.3f} spread {max(ms) - min(ms):.3f} | n_batches {nb}", flush=True)
for name, lights, res, depth in (("window", "point", 96, 5), ("window", "point", 128, 4), ("window", "point", 32, 8), ("pane_sphere", "point_spot", 128, 7), ("window", "point_front", 96, 5)):
    sc = wt.make_scene(T, name, lights)
    for rep in range(2):
        integ = T.WhittedIntegrator(T.scenes.cornell_camera(res), T.SeededSampler(1, seed=wt.SEED), depth)
        try:
            integ.render(sc)
            print(f"{label}: {name} / {lights} {res}x{res} 1spp depth {depth} run {rep}: ms_total {integ.stats.ms_total:.3f} n_batches {integ.stats.n_batches} closest {integ.stats.closest_rays} shadow {integ.stats.shadow_rays}", flush=True)
        except T.TraceHipError as e:
            print(f"{label}: {name} / {lights} {res}x{res} 1spp depth {depth} run {rep}: TraceHipError: {e}", flush=True)
