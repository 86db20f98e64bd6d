#!/usr/bin/env python
"""Temporal upsampling: python tools/temporal_upsample_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3] [--frames 12]
[--skip-timing] [--skip-frames] [--skip-quality] [--skip-sweep]

1. Kernel times on the 1 M-triangle mesh scene, `--res`^2 <- (`--res` / 2)^2, second frame of a camera 0.75 degrees on (so that the history is found): the fused
   trhip_temporal_upsample_device with radius 1 and 2 against what the library needed for the same result class before it existed, trhip_upscale_device with that radius
   followed by trhip_temporal_device on the upscaled film at full size — alternating in one process, `--repeats` times over.  Device events around the launches
   (trhip_stats.ms_film); first quartile, median, third quartile of the runs after the warm-up; the ratio fused / pair of the same repeat.  Compulsory bytes per full-size
   pixel: fused 48 + 48 in and 16 + 48 out = 160 and 64 per low pixel (176 at 2 x); the pair 48 in, 16 out, then 16 + 48 + 48 in and 16 + 48 out = 240 and 64 per low pixel (256).
2. Frame times on the same scene at `--res`^2, `--spp` spp, depth `--depth`, a still camera: PreviewSession native, upscaled (guide_spp 1) and in the new mode (guide_spp 1),
   alternating, `--frames` frames each after two warm-up frames: sums of the calls' device times, medians.
3. Quality on Cornell and mesh_scene(16), 64^2 <- 32^2, 4 spp, depth 5, MSE of xyz / w over all pixels of positive weight against the 1024 spp full-size frame of the last
   camera, three camera paths (still, 16 frames; the 8-frame arc and the 40-frame arc of tools/temporal_probe.py, 0.75 degrees a frame): the upscaled session (the
   yardstick), the native session at the same spp, and the new mode with "grid", "halton" and no jitter.  Then the sweep for the defaults:
   rho in {0, 1, 2} x kappa_0 in {2^-4, 2^-2, 1} x max_history in {8, 16, 32} x R in {1, 2}, jitter "grid".
   THE RULE, stated before the sweep is run: the cell with the lowest geometric mean of the four ratios to the upscaled session (two scenes x {still, 8-frame arc}); among
   cells within 1 % of it the cheaper one (R = 1 before R = 2, then the shorter history, then the lower rho).  The 40-frame arcs are reported beside it, not used.
Prints JSON lines."""
import argparse, ctypes as C, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--runs", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--skip-frames", action="store_true")
ap.add_argument("--skip-quality", action="store_true")
ap.add_argument("--skip-sweep", action="store_true", help="the session table of part 3 without the sweep")
a = ap.parse_args()
CENTRE = np.array([0.5, 0.4, -2.5])
CAMERAS = {}


def camera(resolution, degrees=0.0):
    """The scenes' camera turned about the vertical axis through the box's centre (tools/temporal_probe.py)."""
    if (resolution, degrees) not in CAMERAS:
        CAMERAS[resolution, degrees] = make_camera(resolution, degrees)
    return CAMERAS[resolution, degrees]


def make_camera(resolution, degrees):
    r = math.radians(degrees)
    R = np.array([[math.cos(r), 0.0, math.sin(r)], [0.0, 1.0, 0.0], [-math.sin(r), 0.0, math.cos(r)]])
    eye, target = CENTRE + R @ (np.array([0.0, 15.0, 50.0]) - CENTRE), CENTRE + R @ (np.array([0.0, 0.0, -2.0]) - CENTRE)
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at(eye.tolist(), target.tolist(), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def timing():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    flat = scene.flatten()
    ctx, L, seed = flat.ctx, T.lib(), 0x5EED0001
    cams = [camera(a.res, 0.0), camera(a.res, 0.75)]
    tu = T.TemporalUpsampler()
    los = [T.Upscaler.low_camera(c, 2, jitter=tu.jitter_for(k, 2)) for k, c in enumerate(cams)]
    (h, w), (lh, lw) = cams[0].film.size, los[0].film.size
    npix, nlo = h * w, lh * lw
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    d_lo, d_lo_planes, d_hi_planes, d_up, d_out, d_hist0, d_hist1, d_mask = (T._ffi.DeviceBuffer(n) for n in (nlo * 16, nlo * 48, npix * 48, npix * 16, npix * 16, npix * 48, npix * 48,
                                                                                                                    npix))

    def frame(k):
        sn_lo, sn_hi = los[k].sensor(), cams[k].sensor()
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn_lo), a.spp, a.depth, seed, k * a.spp, ptr(d_lo), C.byref(T.Stats())))
        ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn_lo), a.spp, seed, k * a.spp, ptr(d_lo_planes), None, C.byref(T.Stats())))
        ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn_hi), 1, seed, k * a.spp, ptr(d_hi_planes), None, C.byref(T.Stats())))
    frame(0)
    tu.accumulate_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_hi_planes.ptr, None, w, h, T.Upscaler.pixel_map(cams[0], los[0]), None, d_out.ptr, d_hist0.ptr, None, ctx)
    frame(1)
    m = T.Upscaler.pixel_map(cams[1], los[1])
    tp = T.TemporalAccumulator()._params_for(cams[0])

    def series(call):
        ms = []
        for i in range(a.warmup + a.runs):
            v = call()
            if i >= a.warmup:
                ms.append(v)
        return [round(float(v), 5) for v in np.percentile(ms, [25, 50, 75])]

    def fused(p):
        st = T.Stats()
        ctx.check(L.trhip_temporal_upsample_device(ctx._h, ptr(d_lo), ptr(d_lo_planes), lw, lh, ptr(d_hi_planes), ptr(d_hist0), w, h, C.byref(p), ptr(d_out), ptr(d_hist1), ptr(d_mask),
                                                   C.byref(st)))
        return st.ms_film

    def pair(p):
        s1, s2 = T.Stats(), T.Stats()
        ctx.check(L.trhip_upscale_device(ctx._h, ptr(d_lo), ptr(d_lo_planes), lw, lh, ptr(d_hi_planes), w, h, C.byref(p), ptr(d_up), ptr(d_mask), C.byref(s1)))
        ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_up), ptr(d_hi_planes), ptr(d_hist0), w, h, C.byref(tp), ptr(d_out), ptr(d_hist1), C.byref(s2)))
        return s1.ms_film + s2.ms_film
    fused(tu._params_for(m, cams[0]))
    mask = d_mask.to_host(np.uint8, (h, w))
    print(json.dumps({"scene": a.scene, "res": a.res, "low": [lw, lh], "spp": a.spp, "depth": a.depth, "runs": a.runs, "pixel_map": m,
                      "compulsory_bytes_fused": npix * 160 + nlo * 64, "compulsory_bytes_pair": npix * 240 + nlo * 64,
                      "mask_counts_0_to_7": [int((mask == k).sum()) for k in range(8)]}), flush=True)
    for rep in range(a.repeats):
        for R in (1, 2):
            pf = T.TemporalUpsampler(radius=R)._params_for(m, cams[0])
            pu = T.Upscaler(radius=R)._params_for(m)
            qp = series(lambda: pair(pu))
            qf = series(lambda: fused(pf))
            print(json.dumps({"repeat": rep, "radius": R, "pair_upscale_then_temporal_ms_q25_median_q75": qp, "fused_ms_q25_median_q75": qf, "fused_over_pair": round(qf[1] / qp[1], 3),
                              "fused_TB_per_s_of_compulsory_bytes": round((npix * 160 + nlo * 64) / (qf[1] * 1e-3) * 1e-12, 3)}), flush=True)


def sessions(scene, spp, depth, seed, **modes):
    return {name: T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, **kw) for name, kw in modes.items()}


def frame_times():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    ctx = scene.flatten().ctx
    hi = camera(a.res)
    ss = sessions(scene, a.spp, a.depth, 0x5EED0001, native=dict(), upscaled=dict(upscaler=T.Upscaler(), guide_spp=1),
                  temporal_upsample=dict(upscaler=T.Upscaler(), guide_spp=1, temporal_upsample=T.TemporalUpsampler()))
    dev, parts = {}, {}
    for k in range(a.frames + 2):
        for name, s in ss.items():
            s.render(hi, ctx)
            if k >= 2:
                dev.setdefault(name, []).append(sum(st.ms_total for st in s.render_stats))
                parts[name] = [round(st.ms_total, 3) for st in s.render_stats]
    for name, s in ss.items():
        s.close()
        print(json.dumps({"session": name, "res": a.res, "spp": a.spp, "depth": a.depth, "n": len(dev[name]), "device_ms_median": round(float(np.median(dev[name])), 3),
                          "speed_up_over_native": round(float(np.median(dev["native"]) / np.median(dev[name])), 3), "last_frame_ms_by_call": parts[name]}), flush=True)


def quality():
    res, spp, depth, seed, step = 64, 4, 5, 0xBEEF, 0.75
    paths = {"still16": [0.0] * 16, "arc8": [step * k for k in range(8)], "arc40": [step * k for k in range(40)]}
    scenes = (("cornell", T.scenes.cornell_scene), ("mesh16", lambda: T.scenes.mesh_scene(16)))
    made, targets = {}, {}
    for which, make in scenes:
        made[which] = make()
        ctx = made[which].flatten().ctx
        for path, angles in paths.items():
            targets[which, path] = T.PathIntegrator(camera(res, angles[-1]), T.SeededSampler(1024, seed=0x7A26E7), depth).render(made[which], ctx)

    def run(which, path, **kw):
        scene, target = made[which], targets[which, path]
        ctx = scene.flatten().ctx
        session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, **kw)
        for deg in paths[path]:
            x = session.render(camera(res, deg), ctx)
        session.close()
        weighted = (x[..., 3] > 0) & (target[..., 3] > 0)
        with np.errstate(all="ignore"):
            diff = x[weighted][:, :3].astype(np.float64) / x[weighted][:, 3:4] - target[weighted][:, :3].astype(np.float64) / target[weighted][:, 3:4]
        return float(np.mean(diff * diff))
    base = {}
    for which, _ in scenes:
        for path in paths:
            base[which, path] = run(which, path, upscaler=T.Upscaler())
            row = {"scene": which, "path": path, "mse_upscaled_session": round(base[which, path], 6), "native_over_upscaled": round(run(which, path) / base[which, path], 4)}
            for jitter in ("grid", "halton", None):
                row[f"temporal_upsample_{jitter}_over_upscaled"] = round(run(which, path, upscaler=T.Upscaler(), temporal_upsample=T.TemporalUpsampler(jitter=jitter)) / base[which, path], 4)
            print(json.dumps(row), flush=True)
    if a.skip_sweep:
        return
    cells = {}
    for R in (1, 2):
        for max_history in (8.0, 16.0, 32.0):
            for rho in (0.0, 1.0, 2.0):
                for k0 in (2.0 ** -4, 2.0 ** -2, 1.0):
                    mk = lambda: T.TemporalUpsampler(radius=R, max_history=max_history, confidence_sharpness=rho, confidence_floor=k0)  # noqa: E731
                    r = {(w, p): run(w, p, upscaler=T.Upscaler(), temporal_upsample=mk()) / base[w, p] for w, _ in scenes for p in ("still16", "arc8")}
                    gm = float(np.exp(np.mean(np.log(list(r.values())))))
                    cells[R, max_history, rho, k0] = gm
                    print(json.dumps({"radius": R, "max_history": max_history, "rho": rho, "kappa0": k0, "ratios_cornell_still_arc8_mesh16_still_arc8": [round(v, 4) for v in r.values()],
                                      "geometric_mean": round(gm, 4)}), flush=True)
    best = min(cells.values())
    near = sorted((c for c, gm in cells.items() if gm <= best * 1.01), key=lambda c: (c[0], c[1], c[2], cells[c]))
    fav = near[0]
    mk = lambda: T.TemporalUpsampler(radius=fav[0], max_history=fav[1], confidence_sharpness=fav[2], confidence_floor=fav[3])  # noqa: E731
    arcs = {f"{w}_{p}": round(run(w, p, upscaler=T.Upscaler(), temporal_upsample=mk()) / base[w, p], 4) for w, _ in scenes for p in paths}
    print(json.dumps({"lowest_geometric_mean": round(best, 4), "cells_within_1_percent_R_maxhistory_rho_kappa0": [list(c) for c in near], "favoured_cell": list(fav),
                      "favoured_cell_ratios_to_the_upscaled_session": arcs, "cells_below_1": sum(1 for v in cells.values() if v < 1.0), "cells": len(cells)}), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_frames:
    frame_times()
if not a.skip_quality:
    quality()
