#!/usr/bin/env python
"""The sky-lit frame beside the AO frame on the 1 M-triangle mesh scene: python tools/sky_probe.py [--spp 8] [--res 1024] [--runs 20] [--warmup 5] [--map 256] [--albedo]

Renders trhip_render_sky_device (a 256 x 256 gradient map, film left in HBM) and trhip_render_ao_device of the same build on the same scene, sensor, spp and seed.  The two
candidates ALTERNATE in one process — sky, ao, sky, ao, … — so that clocks, caches and whatever else drifts during the run drift under both.  Prints one JSON line per
candidate: median / min / max / quartiles of the device time over the runs and the stage times of the median run (ms_shade is the spawn kernel: k_sky_spawn / k_ao_spawn).
Then one line with the differences of the medians per stage."""
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
ap.add_argument("--map", type=int, default=256)
ap.add_argument("--max-distance", type=float, default=float("inf"))
ap.add_argument("--albedo", action="store_true")
a = ap.parse_args()
scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), T.scenes.cornell_camera(a.res)
flat = scene.flatten()
ctx, L, sn, seed = flat.ctx, T.lib(), cam.sensor(), 0x5EED0001
h, w = cam.film.size
d_film = T._ffi.DeviceBuffer(h * w * 4 * 4)
env = T.Environment.gradient((0.1, 0.3, 1.0), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1), up=(0, 1, 0), n=a.map)
h_env = env._handle(ctx)
sky_prm, ao_prm = T._ffi.SkyParams(), T._ffi.AoParams()
ctx.check(L.trhip_sky_default_params(C.byref(sky_prm)))
ctx.check(L.trhip_ao_default_params(C.byref(ao_prm)))
sky_prm.max_distance, sky_prm.flags = a.max_distance, T._ffi.SKY_ALBEDO if a.albedo else 0
ao_prm.max_distance, ao_prm.background, ao_prm.flags = a.max_distance, 1.0, T._ffi.AO_ALBEDO if a.albedo else 0


def sky(st):
    ctx.check(L.trhip_render_sky_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, h_env, C.byref(sky_prm), C.c_void_p(d_film.ptr), C.byref(st)))


def ao(st):
    ctx.check(L.trhip_render_ao_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, C.byref(ao_prm), C.c_void_p(d_film.ptr), C.byref(st)))


CANDIDATES = (("sky", sky), ("ao", ao))
STAGES = ("ms_raygen", "ms_trace_closest", "ms_fallback", "ms_shade", "ms_trace_any", "ms_film")
KEEP = ("camera_samples", "closest_rays", "shadow_rays", "fallback_rays", "traversal") + STAGES + ("launches_raygen", "launches_trace_closest", "launches_shade", "launches_trace_any", "launches_film")
runs = {name: [] for name, _ in CANDIDATES}
for i in range(a.warmup + a.runs):
    for name, call in CANDIDATES:
        st = T.Stats()
        call(st)
        if i >= a.warmup:
            runs[name].append(st.as_dict())


def median(xs):
    return sorted(xs)[len(xs) // 2]


summary = {}
for name, _ in CANDIDATES:
    rs = sorted(runs[name], key=lambda r: r["ms_total"])
    ms = [r["ms_total"] for r in rs]
    med = rs[len(rs) // 2]
    summary[name] = {"ms_total": ms[len(ms) // 2], **{k: median([r[k] for r in rs]) for k in STAGES}}
    print(json.dumps({"frame": name, "scene": a.scene, "res": a.res, "spp": a.spp, "map": a.map if name == "sky" else None, "runs": a.runs, "warmup": a.warmup, "alternating": True,
                      "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "ms_p25": round(ms[len(ms) // 4], 3),
                      "ms_p75": round(ms[(3 * len(ms)) // 4], 3), "median_run": {k: (round(med[k], 3) if isinstance(med[k], float) else med[k]) for k in KEEP}}), flush=True)
print(json.dumps({"sky_minus_ao_ms (medians of each stage over the runs)": {k: round(summary["sky"][k] - summary["ao"][k], 3) for k in ("ms_total",) + STAGES},
                  "ao_spread_ms (p75 - p25 of the frame)": round(sorted(r["ms_total"] for r in runs["ao"])[(3 * a.runs) // 4] - sorted(r["ms_total"] for r in runs["ao"])[a.runs // 4], 3)}), flush=True)
env.close()
