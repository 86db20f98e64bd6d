#!/usr/bin/env python
"""Every option combination that changes HOW a frame is computed must leave WHAT is computed alone: renders one small frame of a two-tree scene under each set and compares film and
per-sample radiance, bit for bit, with the default configuration's.

    python tools/option_exactness.py [--workload mesh64|blob24|cornell] [--spp 4] [--res 96]
"""
import argparse, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="mesh64")
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--res", type=int, default=96)
a = ap.parse_args()
scene = {"mesh64": lambda: T.scenes.mesh_scene(64), "blob24": lambda: T.scenes.blob_scene(24), "cornell": T.scenes.cornell_scene, "shadows": T.scenes.shadows_scene}[a.workload]()
cam = T.scenes.shadows_camera(a.res) if a.workload == "shadows" else T.scenes.cornell_camera(a.res)
SETS = [{}, {"hybrid": 0}, {"wide4": 0}, {"wide4": 0, "overlap": 0}, {"leaf_queue": 1}, {"any_on_accelerator": 1}, {"any_on_accelerator": 0}, {"node_layout": 1}, {"overlap": 0}, {"pipelines": 2}, {"band_tile_rows": 2},
        {"traversal": 2}, {"traversal": 6}, {"traversal": 7}, {"traversal": 1}, {"traversal": 4}, {"slab_margin_log2": 0}, {"count_visits": 1}, {"bvh_builder": 2}, {"bvh_builder": 4},
        {"film_fused": 0}, {"film_relayout": 0}, {"occluder_pretest": 0}, {"leaf_kernel": 0}, {"batch_paths": 20000}, {"tiny_scene_prims": 0, "bvh_builder": 2},
        {"leaf_queue": 1, "count_visits": 1}, {"hybrid": 0, "traversal": 7}, {"overlap": 0, "leaf_queue": 1}]
ref = None
bad = 0
for opts in SETS:
    ctx = T.Context(0)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        integ = T.PathIntegrator(cam, T.SeededSampler(a.spp, seed=7), 6)
        film = integ.render(scene, ctx).copy()
        try:
            L = integ.sample_radiance(scene).copy()
        except T.TraceHipError:  # (frames rendered in bands keep no per-sample radiance)
            L = None
        mode = scene._flat.bvh_mode()[0]
        st = integ.stats
        if ref is None:
            ref = (film, L, mode)
        if mode == 0 and ref[2] != 0:  # (traversal 4 commits its own tree — the library's, with the spheres chained above the triangles: not the reference's answers, by request)
            print(f"{str(opts):55s} mode {mode} traversal {st.traversal:2d}: the library's tree alone, not compared", flush=True)
            continue
        pairs = [(film, ref[0])] + ([(L, ref[1])] if L is not None else [])
        same = all(not ((x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))).any() for x, y in pairs)
        print(f"{str(opts):55s} mode {mode} traversal {st.traversal:2d} fallback {st.fallback_rays:7d} of {st.closest_rays:9d}  {'equal' if same else 'DIFFERENT'}", flush=True)
        bad += not same
    except T.TraceHipError as e:
        print(f"{str(opts):55s} refused: {e}", flush=True)
    finally:
        if scene._flat is not None:
            scene._flat.free()
            scene._flat = None
        ctx.close()
print("total:", len(SETS), "option sets,", bad, "with a different film")
sys.exit(1 if bad else 0)
