#!/usr/bin/env python
"""Temporal reprojection: python tools/temporal_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3] [--frames 8,40] [--skip-timing] [--skip-sweep]

1. Times k_temporal on the 1 M-triangle mesh scene: two frames through cameras 0.75 degrees apart, the second accumulated against the first one's history, in both
   lane-to-pixel mappings (option "temporal_patch"), alternating, `--repeats` times over — beside k_denoise_prepare and k_denoise_finish on the same frame.  Kernel times are
   device events around the launch (trhip_stats.ms_film / ms_sub), medians over the runs; bytes per second against the compulsory traffic per pixel: temporal 176 B (film 16 +
   planes 48 in, one 48-byte history record in — the four taps of neighbouring pixels share theirs —, film 16 + history 48 out), prepare 128 B (64 in, four float4 out),
   finish 80 B (film, flag, colour, base colour in; film out).
2. Sweeps max_history over 8, 16, 32, 64 on the test sequence of tests/test_gpu_temporal.py (Cornell and mesh_scene(16), 64 x 64, 2 spp, depth 5, cameras 0.75 degrees apart on
   an arc) for each length in --frames: MSE of xyz / w over the surface pixels of the last frame against its own 1024 spp frame, PreviewSession / Denoiser alone.
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
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--frames", default="8,40")
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--skip-sweep", action="store_true")
a = ap.parse_args()
CENTRE = np.array([0.5, 0.4, -2.5])


def camera(resolution, degrees):
    """The scenes' camera turned about the vertical axis through the box's centre."""
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
    h, w = cams[0].film.size
    npix = h * w
    buf = lambda n: T._ffi.DeviceBuffer(npix * n)  # noqa: E731
    d_film, d_planes, d_hist0, d_hist1, d_out = buf(16), buf(48), buf(48), buf(48), buf(16)
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    acc, den = T.TemporalAccumulator(), T.Denoiser()

    def frame(k, st_path=None, st_aov=None):
        sn = cams[k].sensor()
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, k * a.spp, ptr(d_film), C.byref(st_path or T.Stats())))
        ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, k * a.spp, ptr(d_planes), None, C.byref(st_aov or T.Stats())))

    frame(0)
    acc.accumulate_device(d_film.ptr, d_planes.ptr, None, w, h, None, d_out.ptr, d_hist0.ptr, ctx)
    st_path, st_aov = T.Stats(), T.Stats()
    frame(1, st_path, st_aov)
    prm = acc._params_for(cams[0])

    def temporal(st):
        ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), w, h, C.byref(prm), ptr(d_out), ptr(d_hist1), C.byref(st)))

    def denoise1(st):
        p = T._ffi.DenoiseParams.from_buffer_copy(den.params)
        p.iterations = 1
        ctx.check(L.trhip_denoise_device(ctx._h, ptr(d_film), ptr(d_planes), w, h, C.byref(p), ptr(d_out), C.byref(st)))

    def series(call, key):
        ms = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                ms.append(key(st))
        q = np.percentile(ms, [25, 50, 75])
        return [round(float(v), 5) for v in q]

    hist = d_hist1
    temporal(T.Stats())
    N = hist.to_host(np.float32, (h, w, 3, 4))[..., 0, 3]
    print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "ms_path": round(st_path.ms_total, 3), "ms_aov": round(st_aov.ms_total, 3),
                      "surface_pixels": int((N > 0).sum()), "pixels_with_history": int((N > 1).sum()), "pixels": npix}), flush=True)
    tb = lambda bytes_per_pixel, ms: round(bytes_per_pixel * npix / (ms * 1e-3) * 1e-12, 3)  # noqa: E731
    for rep in range(a.repeats):
        for name, patch in (("film order", 0), ("16 x 4 patches", 1)):
            ctx.set_option("temporal_patch", patch)
            q = series(temporal, lambda st: st.ms_film)
            print(json.dumps({"repeat": rep, "kernel": "k_temporal", "mapping": name, "ms_q25_median_q75": q, "TB_per_s_of_176B_per_pixel": tb(176.0, q[1])}), flush=True)
    ctx.set_option("temporal_patch", 1)
    for rep in range(a.repeats):
        q = series(denoise1, lambda st: st.ms_sub[0])
        print(json.dumps({"repeat": rep, "kernel": "k_denoise_prepare", "ms_q25_median_q75": q, "TB_per_s_of_128B_per_pixel": tb(128.0, q[1])}), flush=True)
        q = series(denoise1, lambda st: st.ms_sub[2])
        print(json.dumps({"repeat": rep, "kernel": "k_denoise_finish", "ms_q25_median_q75": q, "TB_per_s_of_80B_per_pixel": tb(80.0, q[1])}), flush=True)
    q = series(temporal, lambda st: st.ms_total)
    print(json.dumps({"call": "trhip_temporal_device", "ms_total_q25_median_q75": q}), flush=True)


def sweep():
    import denoise_model as dm
    res, spp, depth, seed, step = 64, 2, 5, 0xBEEF, 0.75
    for which, make in (("cornell", T.scenes.cornell_scene), ("mesh16", lambda: T.scenes.mesh_scene(16))):
        scene = make()
        ctx = scene.flatten().ctx
        for frames in [int(v) for v in a.frames.split(",")]:
            cams = [camera(res, step * k) for k in range(frames)]
            last, offset = cams[-1], (frames - 1) * spp
            smp = T.SeededSampler(spp, seed=seed, sample_offset=offset)
            noisy = T.PathIntegrator(last, smp, depth).render(scene)
            planes = T.AOVIntegrator(last, smp).render(scene).planes
            alone = T.Denoiser().render(scene, last, smp, depth, ctx)
            target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), depth).render(scene)
            surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))

            def mse(x):
                with np.errstate(all="ignore"):
                    diff = x[surface][:, :3].astype(np.float64) / x[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
                return float(np.mean(diff * diff))
            row = {"scene": which, "frames": frames, "surface_pixels": int(surface.sum()), "mse_2spp": round(mse(noisy), 6), "mse_denoiser_alone": round(mse(alone), 6)}
            for max_history in (8, 16, 32, 64):
                session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=T.TemporalAccumulator(max_history=max_history))
                for cam in cams:
                    preview = session.render(cam, ctx)
                session.close()
                row[f"ratio_max_history_{max_history}"] = round(mse(preview) / mse(alone), 4)
            print(json.dumps(row), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_sweep:
    sweep()
