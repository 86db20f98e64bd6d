#!/usr/bin/env python
"""The importance-sampled sky frame beside the sky frame: python tools/sky_is_probe.py [time|quality] [--mix 0.5] [--spp 8] [--res 1024] [--runs 20] [--warmup 5] [--map 256]

time     renders trhip_render_sky_is_device and trhip_render_sky_device of the same build on the 1 M-triangle scene (a 256 x 256 gradient map with a sun of a few texels, film
         left in HBM).  The two candidates ALTERNATE in one process — is, sky, is, sky, … — so that clocks, caches and whatever else drifts during the run drift under both.
         Prints one JSON line per candidate (median / min / max / quartiles of the device time, the per-stage medians; ms_shade is the spawn kernel: k_sky_spawn_is /
         k_sky_spawn), then one line with the differences of the medians per stage.
quality  Cornell without its lights and mesh_scene(16) at 64 x 64 under the same map: the MSE of the importance-sampled and of the cosine frame at 4 and 16 spp (mean over
         --seeds seeds), each against the mean of a 4096 spp cosine frame and a 4096 spp importance-sampled frame, their ratio, and the equal-time ratio from --ms-is and
         --ms-sky (the frame times `time` measured: MSE times time, the cost of reaching an error at 1 / N convergence)."""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", default="time", choices=["time", "quality"])
ap.add_argument("--mix", type=float, default=0.5)
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--map", type=int, default=256)
ap.add_argument("--sun", type=float, default=5000.0)
ap.add_argument("--albedo", action="store_true")
ap.add_argument("--seeds", type=int, default=8)
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--ms-is", type=float, default=None)
ap.add_argument("--ms-sky", type=float, default=None)
a = ap.parse_args()


def sun_sky(n):
    """The gradient map of tools/sky_probe.py with a sun: a 3 x 3 block of texels of --sun, 40 degrees above the horizon (up is +y)."""
    env = T.Environment.gradient((0.1, 0.3, 1.0), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1), up=(0, 1, 0), n=n)
    d = T.octahedral_directions(n)
    s = np.array([0.45, 0.64, 0.62])
    j, i = np.unravel_index(np.argmax(d @ (s / np.linalg.norm(s))), (n, n))
    t = env.texels.copy()
    t[max(j - 1, 0):j + 2, max(i - 1, 0):i + 2] = np.float32(a.sun)
    return T.Environment(t)


def is_integrator(cam, spp, seed, env, **kw):
    return T.SkyIntegrator(cam, T.SeededSampler(spp, seed=seed), env, importance=a.mix, **kw)


def time_mode():
    scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), T.scenes.cornell_camera(a.res)
    flat = scene.flatten()
    ctx, L, sn, seed = flat.ctx, T.lib(), cam.sensor(), 0x5EED0001
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 4 * 4)
    env = sun_sky(a.map)
    h_env = env._sampler_handle(ctx)
    sky_prm, is_prm = T._ffi.SkyParams(), T._ffi.SkyIsParams()
    ctx.check(L.trhip_sky_default_params(C.byref(sky_prm)))
    ctx.check(L.trhip_sky_is_default_params(C.byref(is_prm)))
    sky_prm.flags = is_prm.flags = T._ffi.SKY_ALBEDO if a.albedo else 0
    is_prm.mix = a.mix

    def sky_is(st):
        ctx.check(L.trhip_render_sky_is_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, h_env, C.byref(is_prm), C.c_void_p(d_film.ptr), C.byref(st)))

    def sky(st):
        ctx.check(L.trhip_render_sky_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, h_env, C.byref(sky_prm), C.c_void_p(d_film.ptr), C.byref(st)))

    candidates = (("sky_is", sky_is), ("sky", sky))
    stages = ("ms_raygen", "ms_trace_closest", "ms_fallback", "ms_shade", "ms_trace_any", "ms_film")
    keep = ("camera_samples", "closest_rays", "shadow_rays") + stages
    runs = {name: [] for name, _ in candidates}
    for i in range(a.warmup + a.runs):
        for name, call in candidates:
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                runs[name].append(st.as_dict())
    median = lambda xs: sorted(xs)[len(xs) // 2]
    summary = {}
    for name, _ in candidates:
        rs = sorted(runs[name], key=lambda r: r["ms_total"])
        ms = [r["ms_total"] for r in rs]
        med = rs[len(rs) // 2]
        summary[name] = {"ms_total": ms[len(ms) // 2], **{k: median([r[k] for r in rs]) for k in stages}}
        print(json.dumps({"frame": name, "lib": os.path.basename(T._ffi.LIB_PATH), "scene": a.scene, "res": a.res, "spp": a.spp, "map": a.map, "mix": a.mix if name == "sky_is" else None,
                          "runs": a.runs, "warmup": a.warmup, "alternating": True, "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                          "ms_p25": round(ms[len(ms) // 4], 3), "ms_p75": round(ms[(3 * len(ms)) // 4], 3), "stage_medians": {k: round(summary[name][k], 3) for k in stages},
                          "median_run": {k: (round(med[k], 3) if isinstance(med[k], float) else med[k]) for k in keep}}), flush=True)
    print(json.dumps({"sky_is_minus_sky_ms (medians of each stage over the runs)": {k: round(summary["sky_is"][k] - summary["sky"][k], 3) for k in ("ms_total",) + stages}}), flush=True)
    env.close()


def quality_mode():
    env = sun_sky(a.map)
    cornell = T.Scene([], T.BVHAccel(T.scenes.cornell_primitives()[0], 1))  # Cornell without its lights (the sky frame reads none anyway)
    for name, scene in (("cornell", cornell), ("mesh16", T.scenes.mesh_scene(16))):
        cam = T.scenes.cornell_camera(64)
        rgb = lambda xyzw: xyzw[..., :3] / np.maximum(xyzw[..., 3:4], 1e-20)
        ref_cos = rgb(T.SkyIntegrator(cam, T.SeededSampler(a.ref_spp, seed=0xBEEF), env).render(scene)).astype(np.float64)
        ref_is = rgb(is_integrator(cam, a.ref_spp, 0xFEED, env).render(scene)).astype(np.float64)
        ref = 0.5 * (ref_cos + ref_is)
        print(json.dumps({"scene": name, "reference": f"mean of a {a.ref_spp} spp cosine and a {a.ref_spp} spp importance-sampled frame", "mse_between_the_two_references": float(((ref_cos - ref_is) ** 2).mean()),
                          "mean_of_reference": float(ref.mean())}), flush=True)
        for spp in (4, 16):
            mse = {"sky_is": [], "sky": []}
            for s in range(a.seeds):
                mse["sky_is"].append(float(((rgb(is_integrator(cam, spp, 100 + s, env).render(scene)) - ref) ** 2).mean()))
                mse["sky"].append(float(((rgb(T.SkyIntegrator(cam, T.SeededSampler(spp, seed=100 + s), env).render(scene)) - ref) ** 2).mean()))
            m_is, m_cos = float(np.mean(mse["sky_is"])), float(np.mean(mse["sky"]))
            out = {"scene": name, "res": 64, "spp": spp, "mix": a.mix, "seeds": a.seeds, "mse_sky_is": m_is, "mse_sky": m_cos, "ratio_is_over_sky": m_is / m_cos}
            if a.ms_is and a.ms_sky:
                out["equal_time_ratio (mse x frame time)"] = (m_is * a.ms_is) / (m_cos * a.ms_sky)
            print(json.dumps(out), flush=True)
    env.close()


time_mode() if a.mode == "time" else quality_mode()
