#!/usr/bin/env python
"""The path-env frame beside the path frame on the 1 M-triangle mesh scene: python tools/path_env_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 20] [--warmup 5] [--map 256]

Renders trhip_render_path_env_device (a 256 x 256 gradient map, film left in HBM) and trhip_render_path_device of the same build on the same scene, sensor, spp, depth and
seed — with "streaming" 0 for both, so that both are the classic wavefront.  The two candidates ALTERNATE in one process — env, path, env, path, … — so that clocks, caches
and whatever else drifts during the run drift under both.  Prints one JSON line per candidate: median / min / max / quartiles of the device time over the runs and the stage
times of the median run (the escape kernels are timed with the shade stage, the fold with the film stage), one line with the differences of the medians per stage, one line
for trhip_path_env_relight_device alone (host wall time around the call, which synchronises), and the escape counts per depth of the frame."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
import numpy as np
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--map", type=int, default=256)
ap.add_argument("--only-path", action="store_true", help="the path frame alone: the yardstick run of a build without the feature")
a = ap.parse_args()
scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), T.scenes.cornell_camera(a.res)
flat = scene.flatten()
ctx, L, sn, seed = flat.ctx, T.lib(), cam.sensor(), 0x5EED0001
ctx.set_option("streaming", 0)
h, w = cam.film.size
d_film = T._ffi.DeviceBuffer(h * w * 4 * 4)


def path(st):
    ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, 0, C.c_void_p(d_film.ptr), C.byref(st)))


CANDIDATES = [("path", path)]
if not a.only_path:
    env = T.Environment.gradient((0.1, 0.3, 1.0), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1), up=(0, 1, 0), n=a.map)
    h_env = env._handle(ctx)
    prm = T._ffi.PathEnvParams()
    ctx.check(L.trhip_path_env_default_params(C.byref(prm)))

    def path_env(st):
        ctx.check(L.trhip_render_path_env_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, 0, h_env, C.byref(prm), C.c_void_p(d_film.ptr), C.byref(st)))

    CANDIDATES.insert(0, ("env", path_env))
STAGES = ("ms_raygen", "ms_trace_closest", "ms_fallback", "ms_shade", "ms_trace_any", "ms_film")
KEEP = ("camera_samples", "closest_rays", "shadow_rays", "fallback_rays", "traversal", "n_batches") + STAGES + ("launches_raygen", "launches_trace_closest", "launches_shade", "launches_trace_any",
                                                                                                                "launches_film")
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
    print(json.dumps({"frame": name, "scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "map": a.map if name == "env" else None, "runs": a.runs, "warmup": a.warmup,
                      "alternating": len(CANDIDATES) > 1, "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "ms_p25": round(ms[len(ms) // 4], 3),
                      "ms_p75": round(ms[(3 * len(ms)) // 4], 3), "median_run": {k: (round(med[k], 3) if isinstance(med[k], float) else med[k]) for k in KEEP}}), flush=True)
if not a.only_path:
    spread = sorted(r["ms_total"] for r in runs["path"])
    print(json.dumps({"env_minus_path_ms (medians of each stage over the runs)": {k: round(summary["env"][k] - summary["path"][k], 3) for k in ("ms_total",) + STAGES},
                      "path_spread_ms (p75 - p25 of the frame)": round(spread[(3 * a.runs) // 4] - spread[a.runs // 4], 3)}), flush=True)
    st = T.Stats()
    path_env(st)
    rec = np.empty((a.spp * int(st.camera_samples // a.spp), 8), np.float32)
    ctx.check(L.trhip_last_escapes(ctx._h, T._ffi.fptr(rec), rec.size))
    depth = rec[:, 3].astype(np.int64)
    relit = []
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        ctx.check(L.trhip_path_env_relight_device(ctx._h, h_env, C.byref(prm), C.c_void_p(d_film.ptr)))
        if i >= a.warmup:
            relit.append((time.perf_counter() - t0) * 1e3)
    relit.sort()
    print(json.dumps({"relight_ms (host wall time of the call: upload of the sensor block, fold, film pass, synchronise)": {"median": round(relit[len(relit) // 2], 3), "min": round(relit[0], 3),
                                                                                                                          "max": round(relit[-1], 3)},
                      "camera_samples": int(depth.size), "escapes_per_depth": [int((depth == k).sum()) for k in range(1, a.depth + 1)], "no_escape": int((depth == 0).sum())}), flush=True)
    env.close()
