#!/usr/bin/env python
"""Edge-aware upscaling: python tools/upscale_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3] [--frames 12]
[--skip-timing] [--skip-frames] [--skip-quality]

1. Kernel times on the 1 M-triangle mesh scene, `--res`^2 <- (`--res` / 2)^2: trhip_upscale_device with radius 1 and 2 and k_temporal on the full-size frame beside them,
   alternating in one process, `--repeats` times over.  Device events around the launches (trhip_stats.ms_film); first quartile, median, third quartile of the runs after the
   warm-up; the multiple of k_temporal of the same repeat; TB/s against the pass's compulsory bytes: 48 in and 16 + 1 out per full-size pixel, 64 per low pixel.  (The gathered
   form these were measured against is no longer in the tree: profiles/r14/upscale.txt keeps its times.)
2. Frame times on the same scene at `--res`^2, `--spp` spp, depth `--depth`: Denoiser.render native against Upscaler.render at factor 2 with guide_spp in {spp, 2, 1}
   (denoiser where Upscaler.render puts it by default), alternating, `--frames` frames each after two warm-up frames: wall-clock medians of the whole call and the sums of
   the calls' device times.
3. Quality on Cornell and mesh_scene(16), 64^2 <- 32^2, 4 spp, depth 5, against the 64^2 1024 spp frame, MSE of xyz / w over all pixels of positive weight:
   (Q1) Upscaler.render / the same low film upscaled bilinearly (the model's H5 on every pixel); (Q2) upscaled from 1/4 of the paths / native Denoiser.render at the same
   spp; (Q3) equal paths: low frame at 4 x spp / native at spp; (Q4) about equal TIME: upscaled from spp / native at spp / 2; (O) orphans among surface pixels.  Then the
   sweep for the defaults: R x flags x denoise_at x sigma_plane in {0.1, 0.2, 0.4} at sigma_normal 0.25.  THE RULE, stated before the sweep is run: the cell with the lowest geometric mean of Q2 over the two scenes; among cells within 1 %
   of it the cheaper one (R = 1 before R = 2, "low" before "high").
Prints JSON lines."""
import argparse, ctypes as C, json, os, sys, time
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
a = ap.parse_args()


def camera(resolution):
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def timing():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    flat = scene.flatten()
    ctx, L, seed = flat.ctx, T.lib(), 0x5EED0001
    hi = camera(a.res)
    lo = T.Upscaler.low_camera(hi, 2)
    (h, w), (lh, lw) = hi.film.size, lo.film.size
    npix, nlo = h * w, lh * lw
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    d_lo, d_lo_planes, d_hi_film, d_hi_planes, d_out, d_hist, d_mask = (T._ffi.DeviceBuffer(n) for n in (nlo * 16, nlo * 48, npix * 16, npix * 48, npix * 16, npix * 48, npix))
    sn_lo, sn_hi = lo.sensor(), hi.sensor()
    ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn_lo), a.spp, a.depth, seed, 0, ptr(d_lo), C.byref(T.Stats())))
    ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn_lo), a.spp, seed, 0, ptr(d_lo_planes), None, C.byref(T.Stats())))
    ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn_hi), 1, a.depth, seed, 0, ptr(d_hi_film), C.byref(T.Stats())))
    ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn_hi), a.spp, seed, 0, ptr(d_hi_planes), None, C.byref(T.Stats())))
    m = T.Upscaler.pixel_map(hi, lo)
    bytes_total = npix * (48 + 16 + 1) + nlo * 64

    def series(call):
        ms = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                ms.append(st.ms_film)
        return [round(float(v), 5) for v in np.percentile(ms, [25, 50, 75])]
    tp = T.TemporalAccumulator()._params_for(None)
    calls = {"k_temporal": lambda st: ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_hi_film), ptr(d_hi_planes), None, w, h, C.byref(tp), ptr(d_out), ptr(d_hist), C.byref(st)))}
    for R in (1, 2):
        p = T.Upscaler(radius=R)._params_for(m)
        calls[f"upscale R={R}"] = lambda st, p=p: ctx.check(L.trhip_upscale_device(ctx._h, ptr(d_lo), ptr(d_lo_planes), lw, lh, ptr(d_hi_planes), w, h, C.byref(p), ptr(d_out), ptr(d_mask),
                                                                                    C.byref(st)))
    u = T.Upscaler()
    u.upscale_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_hi_planes.ptr, w, h, m, d_out.ptr, d_mask.ptr, ctx)
    mask = d_mask.to_host(np.uint8, (h, w))
    print(json.dumps({"scene": a.scene, "res": a.res, "low": [lw, lh], "spp": a.spp, "depth": a.depth, "runs": a.runs, "pixel_map": m, "compulsory_bytes": bytes_total,
                      "mask_counts_0_1_2_3": [int((mask == k).sum()) for k in range(4)]}), flush=True)
    for rep in range(a.repeats):
        q = {"k_temporal": series(calls["k_temporal"])}
        for R in (1, 2):
            q[f"upscale R={R}"] = series(calls[f"upscale R={R}"])
        for name, v in q.items():
            row = {"repeat": rep, "kernel": name, "ms_q25_median_q75": v, "multiple_of_k_temporal": round(v[1] / q["k_temporal"][1], 3)}
            if name.startswith("upscale"):
                row["TB_per_s_of_compulsory_bytes"] = round(bytes_total / (v[1] * 1e-3) * 1e-12, 3)
            print(json.dumps(row), flush=True)


def frame_times():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    ctx = scene.flatten().ctx
    hi, seed = camera(a.res), 0x5EED0001
    d, u = T.Denoiser(), T.Upscaler()
    guides = [a.spp] + [s for s in (2, 1) if s < a.spp]

    def native(k):
        d.render(scene, hi, T.SeededSampler(a.spp, seed=seed, sample_offset=k * a.spp), a.depth, ctx)
        return sum(s.ms_total for s in d.render_stats)

    def upscaled(k, guide_spp):
        u.render(scene, hi, T.SeededSampler(a.spp, seed=seed, sample_offset=k * a.spp), a.depth, factor=2, guide_spp=guide_spp, denoiser=d, ctx=ctx)
        return sum(s.ms_total for s in u.render_stats if s is not None), [round(s.ms_total, 3) if s is not None else None for s in u.render_stats]
    wall, dev, parts = {}, {}, {}
    for k in range(a.frames + 2):
        for name, call in [("native", lambda: (native(k), None))] + [(f"upscaled guide_spp={s}", lambda s=s: upscaled(k, s)) for s in guides]:
            t0 = time.perf_counter()
            ms, p = call()
            t1 = time.perf_counter()
            if k >= 2:
                wall.setdefault(name, []).append((t1 - t0) * 1e3)
                dev.setdefault(name, []).append(ms)
                parts[name] = p
    for name in wall:
        print(json.dumps({"frames": name, "res": a.res, "spp": a.spp, "depth": a.depth, "n": len(wall[name]), "wall_ms_median": round(float(np.median(wall[name])), 3),
                          "device_ms_median": round(float(np.median(dev[name])), 3), "speed_up_device": round(float(np.median(dev["native"]) / np.median(dev[name])), 3),
                          "speed_up_wall": round(float(np.median(wall["native"]) / np.median(wall[name])), 3),
                          "last_frame_ms_path_lowplanes_fullplanes_denoise_upscale": parts[name]}), flush=True)


def quality():
    import upscale_model as um
    res, spp, depth, seed = 64, 4, 5, 0xBEEF
    q2 = {}
    for which, make in (("cornell", T.scenes.cornell_scene), ("mesh16", lambda: T.scenes.mesh_scene(16))):
        scene, hi = make(), camera(res)
        ctx = scene.flatten().ctx
        lo = T.Upscaler.low_camera(hi, 2)
        target = T.PathIntegrator(hi, T.SeededSampler(1024, seed=0x7A26E7), depth).render(scene)
        smp = lambda n=spp: T.SeededSampler(n, seed=seed)  # noqa: E731
        native_raw = T.PathIntegrator(hi, smp(), depth).render(scene)
        native = T.Denoiser().render(scene, hi, smp(), depth, ctx)
        native_half = T.Denoiser().render(scene, hi, smp(spp // 2), depth, ctx)
        weighted = (native[..., 3] > 0) & (target[..., 3] > 0)

        def mse(x, weighted=weighted, target=target):
            with np.errstate(all="ignore"):
                diff = x[weighted][:, :3].astype(np.float64) / x[weighted][:, 3:4] - target[weighted][:, :3].astype(np.float64) / target[weighted][:, 3:4]
            return float(np.mean(diff * diff))
        u = T.Upscaler()
        shipped, mask = u.render(scene, hi, smp(), depth, ctx=ctx, want_mask=True)
        lo_xyzw = T.PathIntegrator(lo, smp(), depth).render(scene)
        lo_planes, hi_planes = T.AOVIntegrator(lo, smp()).render(scene).planes, T.AOVIntegrator(hi, smp()).render(scene).planes
        m = T.Upscaler.pixel_map(hi, lo)
        p = u.params
        bilinear = um.upscale(lo_xyzw, lo_planes, hi_planes, um.Params(m, p.radius, bool(p.flags & 1), bool(p.flags & 2), p.sigma_normal, p.sigma_plane, p.albedo_floor, p.min_coverage),
                              unguided_only=True)[0]
        surface = np.isin(mask, (1, 3))
        print(json.dumps({"scene": which, "pixels_of_positive_weight": int(weighted.sum()), "mse_native_4spp": round(mse(native_raw), 6), "mse_native_denoised": round(mse(native), 6), "mse_native_half_spp_denoised": round(mse(native_half), 6),
                          "mse_upscaled_no_denoiser": round(mse(shipped), 6), "mse_bilinear": round(mse(bilinear), 6), "Q1_guided_over_bilinear": round(mse(shipped) / mse(bilinear), 4),
                          "O_orphans": int((mask == 3).sum()), "surface_pixels": int(surface.sum()), "O_share": round(float((mask == 3).sum() / max(1, surface.sum())), 4)}), flush=True)
        for R in (1, 2):
            for flags in (True, False):
                for sp in (0.1, 0.2, 0.4):
                    for at in ("low", "high"):
                        uu = T.Upscaler(radius=R, demodulate=flags, coverage=flags, sigma_normal=0.25, sigma_plane=sp)
                        out = uu.render(scene, hi, smp(), depth, denoiser=T.Denoiser(), denoise_at=at, ctx=ctx)
                        eq = uu.render(scene, hi, smp(4 * spp), depth, denoiser=T.Denoiser(), denoise_at=at, ctx=ctx)
                        cell = (R, flags, sp, at)
                        q2.setdefault(cell, []).append(mse(out) / mse(native))
                        print(json.dumps({"scene": which, "radius": R, "flags": flags, "sigma_plane": sp, "denoise_at": at, "Q2_quarter_paths_over_native": round(mse(out) / mse(native), 4),
                                          "Q3_equal_paths_over_native": round(mse(eq) / mse(native), 4), "Q4_over_native_at_half_spp": round(mse(out) / mse(native_half), 4)}), flush=True)
    best = min(float(np.exp(np.mean(np.log(v)))) for v in q2.values())
    rows = []
    for cell, v in sorted(q2.items()):
        gmean = float(np.exp(np.mean(np.log(v))))
        rows.append((gmean, cell))
        print(json.dumps({"radius": cell[0], "flags": cell[1], "sigma_plane": cell[2], "denoise_at": cell[3], "geometric_mean_of_Q2": round(gmean, 4)}), flush=True)
    gmean_of = {c: gm for gm, c in rows}
    near = sorted((c for gm, c in rows if gm <= best * 1.01), key=lambda c: (c[0], c[3] != "low", gmean_of[c]))
    print(json.dumps({"lowest_geometric_mean_of_Q2": round(best, 4), "cells_within_1_percent": [list(c) for c in near], "favoured_cell": list(near[0])}), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_frames:
    frame_times()
if not a.skip_quality:
    quality()
