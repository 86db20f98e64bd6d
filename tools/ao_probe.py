#!/usr/bin/env python
"""Ambient occlusion on the 1 M-triangle mesh scene: python tools/ao_probe.py [--spp 8] [--res 1024] [--runs 20] [--warmup 5] [--max-distance inf] [--albedo]

Renders the frame with trhip_render_ao_device (film left in HBM) and prints one JSON stats line: median / min / max of the device time over the runs and the stage times of
the median run.  Beside it, the same line for trhip_render_aov_device (planes only) and for trhip_render_path_device with max_depth = 1 on the same scene, sensor, spp and
seed: the same camera rays, then a full shading kernel and shadow rays to the light instead of one occlusion ray."""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--max-distance", type=float, default=float("inf"))
ap.add_argument("--albedo", action="store_true")
a = ap.parse_args()
scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), T.scenes.cornell_camera(a.res)
flat = scene.flatten()
ctx, L, sn, seed = flat.ctx, T.lib(), cam.sensor(), 0x5EED0001
h, w = cam.film.size
d_planes = T._ffi.DeviceBuffer(h * w * 12 * 4)
d_film = T._ffi.DeviceBuffer(h * w * 4 * 4)
prm = T._ffi.AoParams()
ctx.check(L.trhip_ao_default_params(C.byref(prm)))
prm.max_distance, prm.flags = a.max_distance, T._ffi.AO_ALBEDO if a.albedo else 0


def ao(st):
    ctx.check(L.trhip_render_ao_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, C.byref(prm), C.c_void_p(d_film.ptr), C.byref(st)))


def aov(st):
    ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, C.c_void_p(d_planes.ptr), None, C.byref(st)))


def path1(st):
    ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, 1, seed, 0, C.c_void_p(d_film.ptr), C.byref(st)))


def measure(name, call):
    runs = []
    for i in range(a.warmup + a.runs):
        st = T.Stats()
        call(st)
        if i >= a.warmup:
            runs.append(st.as_dict())
    runs.sort(key=lambda r: r["ms_total"])
    ms = [r["ms_total"] for r in runs]
    med = runs[len(runs) // 2]
    keep = ("camera_samples", "closest_rays", "shadow_rays", "fallback_rays", "traversal", "ms_raygen", "ms_trace_closest", "ms_fallback", "ms_shade", "ms_trace_any", "ms_film", "launches_raygen",
            "launches_trace_closest", "launches_shade", "launches_trace_any", "launches_film")
    print(json.dumps({"frame": name, "scene": a.scene, "res": a.res, "spp": a.spp, "runs": a.runs, "warmup": a.warmup, "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3),
                      "ms_max": round(ms[-1], 3), "ms_p25": round(ms[len(ms) // 4], 3), "ms_p75": round(ms[(3 * len(ms)) // 4], 3),
                      "median_run": {k: (round(med[k], 3) if isinstance(med[k], float) else med[k]) for k in keep}}), flush=True)


measure("ao", ao)
measure("aov", aov)
measure("path_depth1", path1)
