#!/usr/bin/env python
"""Adaptive sampling, measured: python tools/adaptive_probe.py cost|quality [...]

cost     [--res 1024] [--spp 8] [--depth 8] [--rounds 9] [--warmup 2] [--only path]
         1 M-triangle mesh scene.  Candidates ALTERNATE inside one process, round after round; one JSON line each with the medians over the rounds of the frame's device time
         and of its raygen, closest-hit and film classes: trhip_render_path(spp), trhip_render_path_map with counts == spp, with spp / 2 and 3 spp / 2 in a 16 x 16 checker, and
         with the same two counts in a per-pixel checker (all three maps have the uniform frame's mean).  --only path measures the uniform frame alone: run it with
         TRHIP_LIB=<another build> to hold that build's frame against this one's.
quality  [--res 64] [--depth 8] [--ref-spp 1024] [--budget 32] [--pilots 4,8,16] [--max-extra 120]
         Cornell and mesh_scene(16): MSE of xyz / w over the pixels of positive weight against the --ref-spp frame, for uniform --budget and --budget / 2 spp and for
         AdaptivePathIntegrator with tau from tau_for_budget so that pilot + extra samples total --budget per sample pixel; then a sweep of tau per pilot count."""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["cost", "quality"])
ap.add_argument("--res", type=int, default=0)
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--only", default="")
ap.add_argument("--ref-spp", type=int, default=1024)
ap.add_argument("--budget", type=int, default=32)
ap.add_argument("--pilots", default="4,8,16")
ap.add_argument("--max-extra", type=int, default=120)
a = ap.parse_args()
SEED = 0x5EED0001
L = T.lib()


def cost():
    res = a.res or 1024
    scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N["mesh_1m"]), T.scenes.cornell_camera(res)
    flat = scene.flatten()
    ctx, sn = flat.ctx, cam.sensor()
    h, w = cam.film.size
    sbh, sbw, _, _ = T.api.sample_bounds_shape(cam.film)
    d_film = T._ffi.DeviceBuffer(h * w * 16)
    lo, hi = a.spp // 2, a.spp + a.spp // 2
    yy, xx = np.mgrid[0:sbh, 0:sbw]
    maps = {"map_uniform": np.full((sbh, sbw), a.spp), "map_checker16": np.where(((yy // 16) + (xx // 16)) % 2 == 0, lo, hi), "map_checker1": np.where((yy + xx) % 2 == 0, lo, hi)}
    bufs = {k: (T._ffi.DeviceBuffer(sbh * sbw * 4).from_host(v.astype(np.uint32)), int(v.max()), int(v.sum())) for k, v in maps.items()}

    def path(st):
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, SEED, 0, C.c_void_p(d_film.ptr), C.byref(st)))

    def mapped(name):
        buf, max_spp, _ = bufs[name]
        return lambda st: ctx.check(L.trhip_render_path_map_device(ctx._h, flat._h, C.byref(sn), C.c_void_p(buf.ptr), max_spp, a.depth, SEED, 0, C.c_void_p(d_film.ptr), C.byref(st)))

    cands = {"path": path}
    if hasattr(L, "trhip_render_path_map_device") and not a.only:
        cands.update({k: mapped(k) for k in maps})
    if a.only:
        cands = {k: v for k, v in cands.items() if k == a.only}
    runs = {k: [] for k in cands}
    for r in range(a.warmup + a.rounds):
        for k, call in cands.items():  # alternate: one frame of each candidate per round
            st = T.Stats()
            call(st)
            if r >= a.warmup:
                runs[k].append(st.as_dict())
    med = lambda v: float(np.median(v))  # noqa: E731
    for k, rs in runs.items():
        print(json.dumps({"probe": "cost", "frame": k, "lib": os.path.basename(T.lib()._name), "res": res, "spp": a.spp, "depth": a.depth, "rounds": a.rounds,
                          "camera_samples": rs[0]["camera_samples"], "closest_rays": rs[0]["closest_rays"], "n_batches": rs[0]["n_batches"],
                          **{f: round(med([x[f] for x in rs]), 3) for f in ("ms_total", "ms_raygen", "ms_trace_closest", "ms_shade", "ms_trace_any", "ms_film")},
                          "ms_total_min": round(min(x["ms_total"] for x in rs), 3), "ms_total_max": round(max(x["ms_total"] for x in rs), 3)}), flush=True)


def mse(xyzw, ref):
    ok = (ref[..., 3] > 0) & (xyzw[..., 3] > 0)
    d = xyzw[..., :3][ok] / xyzw[..., 3:][ok] - ref[..., :3][ok] / ref[..., 3:][ok]
    return float(np.mean(d.astype(np.float64) ** 2))


def quality():
    res = a.res or 64
    for name, scene in (("cornell", T.scenes.cornell_scene()), ("mesh16", T.scenes.mesh_scene(16))):
        cam = lambda: T.scenes.cornell_camera(res)  # noqa: E731
        ref = T.PathIntegrator(cam(), T.SeededSampler(a.ref_spp, seed=SEED + 99), a.depth).render(scene)
        sbh, sbw, _, _ = T.api.sample_bounds_shape(cam().film)
        npix = sbh * sbw
        for spp in (a.budget, a.budget // 2):
            i = T.PathIntegrator(cam(), T.SeededSampler(spp, seed=SEED), a.depth)
            x = i.render(scene)
            print(json.dumps({"probe": "quality", "scene": name, "frame": f"uniform_{spp}", "camera_samples": i.stats.camera_samples, "mse": mse(x, ref)}), flush=True)
        for pilot in (int(p) for p in a.pilots.split(",")):
            probe = T.AdaptivePathIntegrator(cam(), T.SeededSampler(pilot, seed=SEED), a.depth, tau=float("inf"), max_extra=a.max_extra)
            probe.render(scene)  # the pilot alone: its (m, v) drive the bisection
            target = (a.budget - pilot) * npix
            tau_b, total_b = probe.tau_for_budget(probe.mv, target)
            for tag, tau in [("budget", float(tau_b))] + [(f"tau_{t}", t) for t in (0.05, 0.1, 0.2, 0.4)]:
                i = T.AdaptivePathIntegrator(cam(), T.SeededSampler(pilot, seed=SEED), a.depth, tau=tau, max_extra=a.max_extra)
                x = i.render(scene)
                n = pilot * npix + i.total
                print(json.dumps({"probe": "quality", "scene": name, "frame": f"adaptive_pilot{pilot}_{tag}", "tau": tau, "eps": float(i.params.eps), "max_extra": a.max_extra,
                                  "camera_samples": n, "spp_mean": round(n / npix, 3), "budget_met": bool(tag != "budget" or abs(i.total - target) <= 0.01 * target),
                                  "pixels_with_extra": int((i.counts > 0).sum()), "mse": mse(x, ref)}), flush=True)


{"cost": cost, "quality": quality}[a.mode]()
