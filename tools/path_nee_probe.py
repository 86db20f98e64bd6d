#!/usr/bin/env python
"""The path-env frame with next-event estimation beside the path-env frame: python tools/path_nee_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 20] [--warmup 5]
[--map 256] [--mix 0.5] [--existing] | --quality

Time (the default): trhip_render_path_env_nee_device and trhip_render_path_env_device of the same build on the 1 M-triangle mesh scene, same sensor, spp, depth and seed, a
256 x 256 gradient map with a 3 x 3-texel sun, film left in HBM.  The two candidates ALTERNATE in one process — nee, env, nee, env, … — so that clocks, caches and whatever
else drifts during the run drift under both.  Prints one JSON line per candidate (median / min / max / quartiles of the device time over the runs; the stage times, ray counts
and launch counts of the median run: k_path_nee is timed with the shade stage, the NEE rays with the any-hit stage, the fold with the film stage), one line with the
differences of the stage medians, and the NEE frame's escape counts.  --existing: trhip_render_path_device and trhip_render_path_env_device alone, alternating — the
yardstick run, which a build without the feature can make too.

Quality (--quality): at 64 x 64 on the Cornell box without lights and on mesh_scene(16), depth 8: the MSE of the linear RGB film of NEE frames and of path-env frames (depth
8) at 4 and 16 spp over 8 seeds against the mean of two 4096-spp references — a NEE frame at depth 8 and a path-env frame at depth 9 — with the frames' device times, so
that the ratio can be read at equal spp and at equal time; the references' own disagreement, mean (A - B)^2 / 4, bounds the noise (and the depth-cut term) in that mean."""
import argparse, ctypes as C, json, os, sys
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
ap.add_argument("--mix", type=float, default=0.5)
ap.add_argument("--sun", type=float, default=5000.0, help="radiance of the 3 x 3 sun texels")
ap.add_argument("--existing", action="store_true", help="trhip_render_path and trhip_render_path_env alone: the yardstick run of a build with or without the feature")
ap.add_argument("--quality", action="store_true")
ap.add_argument("--ref-spp", type=int, default=4096)
a = ap.parse_args()
SEED = 0x5EED0001
L = T.lib()


def sun_sky(n):
    """tools/sky_is_probe.py's map: the gradient sky (+y up) with a sun, a 3 x 3 block of texels of --sun, 40 degrees above the horizon."""
    env = T.Environment.gradient((0.1, 0.3, 1.0), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1), up=(0, 1, 0), n=n)
    d = T.octahedral_directions(n)
    s = np.array([0.45, 0.64, 0.62])
    j, i = np.unravel_index(np.argmax(d @ (s / np.linalg.norm(s))), (n, n))
    t = env.texels.copy()
    t[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2] = np.float32(a.sun)
    return T.Environment(t)


def params(struct, entry, **over):
    p = struct()
    assert getattr(L, entry)(C.byref(p)) == 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


STAGES = ("ms_raygen", "ms_trace_closest", "ms_fallback", "ms_shade", "ms_trace_any", "ms_film")
KEEP = ("camera_samples", "closest_rays", "shadow_rays", "fallback_rays", "traversal", "n_batches") + STAGES + ("launches_raygen", "launches_trace_closest", "launches_shade", "launches_trace_any",
                                                                                                                "launches_film")


def timing():
    scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), T.scenes.cornell_camera(a.res)
    flat = scene.flatten()
    ctx, sn = flat.ctx, cam.sensor()
    ctx.set_option("streaming", 0)
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 4 * 4)
    env = sun_sky(a.map)
    out = C.c_void_p(d_film.ptr)
    pe = params(T._ffi.PathEnvParams, "trhip_path_env_default_params")

    def path(st):
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, SEED, 0, out, C.byref(st)))

    def path_env(st):
        ctx.check(L.trhip_render_path_env_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, SEED, 0, env._handle(ctx), C.byref(pe), out, C.byref(st)))

    if a.existing:
        cands = [("env", path_env), ("path", path)]
    else:
        pn = params(T._ffi.PathNeeParams, "trhip_path_nee_default_params", mix=a.mix)
        h_env = env._sampler_handle(ctx)

        def path_nee(st):
            ctx.check(L.trhip_render_path_env_nee_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, SEED, 0, h_env, C.byref(pn), out, C.byref(st)))

        cands = [("nee", path_nee), ("env", path_env)]
    runs = {name: [] for name, _ in cands}
    for i in range(a.warmup + a.runs):
        for name, call in cands:
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                runs[name].append(st.as_dict())
    median = lambda xs: sorted(xs)[len(xs) // 2]
    summary = {}
    for name, _ in cands:
        rs = sorted(runs[name], key=lambda r: r["ms_total"])
        ms = [r["ms_total"] for r in rs]
        med = rs[len(rs) // 2]
        summary[name] = {"ms_total": ms[len(ms) // 2], **{k: median([r[k] for r in rs]) for k in STAGES}}
        print(json.dumps({"frame": name, "scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "map": a.map, "mix": a.mix if name == "nee" else None, "runs": a.runs,
                          "warmup": a.warmup, "alternating": True, "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                          "ms_p25": round(ms[len(ms) // 4], 3), "ms_p75": round(ms[(3 * len(ms)) // 4], 3),
                          "median_run": {k: (round(med[k], 3) if isinstance(med[k], float) else med[k]) for k in KEEP}}), flush=True)
    (x, _), (y, _) = cands
    print(json.dumps({f"{x}_minus_{y}_ms (medians of each stage over the runs)": {k: round(summary[x][k] - summary[y][k], 3) for k in ("ms_total",) + STAGES}}), flush=True)
    if not a.existing:
        st = T.Stats()
        path_nee(st)
        rec = np.empty((int(st.camera_samples), 8), np.float32)
        ctx.check(L.trhip_last_escapes(ctx._h, T._ffi.fptr(rec), rec.size))
        depth, mark = rec[:, 3].astype(np.int64), rec[:, 7] != 0
        print(json.dumps({"camera_samples": int(depth.size), "escapes_per_depth": [int((depth == k).sum()) for k in range(1, a.depth + 1)],
                          "suppressed_per_depth": [int(((depth == k) & mark).sum()) for k in range(1, a.depth + 1)], "no_escape": int((depth == 0).sum())}), flush=True)
    env.close()


XYZ_TO_RGB = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])


def rgb(xyzw):
    """Linear RGB of a film, unclamped: XYZ over the filter weights (spectrum.jl:16-22's matrix)."""
    x = xyzw[..., :3].astype(np.float64) / np.where(xyzw[..., 3:] != 0, xyzw[..., 3:], 1.0)
    return x @ XYZ_TO_RGB.T


def quality():
    env = sun_sky(a.map)
    scenes = {"cornell_unlit": T.Scene([], T.BVHAccel(T.scenes.cornell_primitives()[0], 1)), "mesh_16": T.scenes.mesh_scene(16)}
    print(json.dumps({"quality": True, "res": 64, "depth": 8, "map": a.map, "sun": a.sun, "mix": a.mix, "ref_spp": a.ref_spp, "seeds": 8,
                      "note": "one map, one mix, one session"}), flush=True)
    for name, scene in scenes.items():
        cam = T.scenes.cornell_camera(64)

        def frame(nee, spp, depth, seed):
            integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed), depth)
            film = integ.render(scene, environment=env, env_importance=a.mix if nee else None).copy()
            return rgb(film), integ.stats.ms_total

        ref_a, _ = frame(True, a.ref_spp, 8, 0xA11CE)
        ref_b, _ = frame(False, a.ref_spp, 9, 0xB0B)
        ref = 0.5 * (ref_a + ref_b)
        disagreement = float(((ref_a - ref_b) ** 2).mean() / 4.0)
        print(json.dumps({"scene": name, "reference": "mean of NEE depth 8 and path-env depth 9", "mean (A - B)^2 / 4": disagreement, "mean of the reference": float(ref.mean()),
                          "mean A": float(ref_a.mean()), "mean B": float(ref_b.mean())}), flush=True)
        for spp in (4, 16):
            row = {}
            for nee in (True, False):
                frame(nee, spp, 8, 1)  # warm
                mses, times = [], []
                for seed in range(1, 9):
                    f, ms = frame(nee, spp, 8, seed)
                    mses.append(float(((f - ref) ** 2).mean()))
                    times.append(ms)
                row["nee" if nee else "env"] = {"mse_mean": float(np.mean(mses)), "mse_min": min(mses), "mse_max": max(mses), "ms_median": sorted(times)[4]}
            n, e = row["nee"], row["env"]
            row.update(scene=name, spp=spp, mse_ratio_equal_spp=n["mse_mean"] / e["mse_mean"],
                       mse_ratio_equal_time=(n["mse_mean"] * n["ms_median"]) / (e["mse_mean"] * e["ms_median"]),  # MSE falls as 1 / spp, and time grows with spp
                       reference_share_of_nee_mse=disagreement / n["mse_mean"], reference_share_of_env_mse=disagreement / e["mse_mean"])
            print(json.dumps(row), flush=True)
    env.close()


quality() if a.quality else timing()
