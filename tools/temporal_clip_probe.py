#!/usr/bin/env python
"""Variance clipping of the reprojected history: python tools/temporal_clip_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3]
[--skip-timing] [--skip-sweep] [--skip-relight]

1. Times k_temporal_clip<R>, R = 1, 2, 3, beside k_temporal (16 x 4 patches, what ships) on the frame pair of tools/temporal_probe.py: the 1 M-triangle mesh scene, two
   cameras 0.75 degrees apart, the second frame accumulated against the first one's history; the four kernels alternate in one process, `--repeats` times over.  Device
   events around the launch (trhip_stats.ms_film); first quartile, median, third quartile of the runs after the warm-up; each median as a multiple of k_temporal's median of
   the same repeat.
2. Sweeps gamma in {0.5, 1, 2, 4, +Inf} x R in {1, 2, 3} x max_history in {8, 16, 32, 64} on the arcs of tools/temporal_probe.py (Cornell and mesh_scene(16), 64 x 64, 2 spp,
   depth 5, seed 0xBEEF, cameras 0.75 degrees apart), 8 and 40 frames: MSE of xyz / w over the surface pixels of the last frame against its own 1024 spp frame,
   PreviewSession / Denoiser alone.  The eight-frame arc is the first eight frames of the forty-frame one, so one session gives both.  gamma = +Inf is the unclipped pass
   bit for bit: its cells must repeat profiles/r11/temporal.txt.  Then the geometric mean of the four ratios at max_history 8 per (gamma, R): the rule for the defaults
   (the lowest among the cells with a finite gamma).
3. The relight sequence of tests/test_gpu_temporal_clip.py (Cornell, static camera, 48 x 48, 4 spp, depth 3; four frames, every light x 0.25 without reset(), two more): per-frame
   MSE against the 1024 spp frame of the lighting the frame was rendered with, unclipped and for every (gamma, R).
Prints JSON lines."""
import argparse, copy, ctypes as C, json, math, os, sys
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
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--skip-sweep", action="store_true")
ap.add_argument("--skip-relight", action="store_true")
a = ap.parse_args()
CENTRE = np.array([0.5, 0.4, -2.5])
INF = float("inf")
GAMMAS, RADII, CAPS = (0.5, 1.0, 2.0, 4.0, INF), (1, 2, 3), (8, 16, 32, 64)


def camera(resolution, degrees):
    """The scenes' camera turned about the vertical axis through the box's centre."""
    r = math.radians(degrees)
    R = np.array([[math.cos(r), 0.0, math.sin(r)], [0.0, 1.0, 0.0], [-math.sin(r), 0.0, math.cos(r)]])
    eye, target = CENTRE + R @ (np.array([0.0, 15.0, 50.0]) - CENTRE), CENTRE + R @ (np.array([0.0, 0.0, -2.0]) - CENTRE)
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at(eye.tolist(), target.tolist(), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def jf(v):
    return "inf" if v == INF else v


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
    acc = T.TemporalAccumulator()

    def frame(k):
        sn = cams[k].sensor()
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, k * a.spp, ptr(d_film), C.byref(T.Stats())))
        ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, k * a.spp, ptr(d_planes), None, C.byref(T.Stats())))

    frame(0)
    acc.accumulate_device(d_film.ptr, d_planes.ptr, None, w, h, None, d_out.ptr, d_hist0.ptr, ctx)
    frame(1)
    prm = acc._params_for(cams[0])
    clip = {R: T.TemporalAccumulator(clip_gamma=1.0, clip_radius=R)._clip_params_for(cams[0]) for R in RADII}

    def temporal(st):
        ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), w, h, C.byref(prm), ptr(d_out), ptr(d_hist1), C.byref(st)))

    def clipped(R):
        def call(st):
            ctx.check(L.trhip_temporal_clip_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), w, h, C.byref(clip[R]), ptr(d_out), ptr(d_hist1), C.byref(st)))
        return call

    def series(call, key):
        ms = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                ms.append(key(st))
        return [round(float(v), 5) for v in np.percentile(ms, [25, 50, 75])]

    clipped(3)(T.Stats())
    hist = d_hist1.to_host(np.float32, (h, w, 3, 4))
    temporal(T.Stats())
    plain = d_hist1.to_host(np.float32, (h, w, 3, 4))
    N = plain[..., 0, 3]
    print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "surface_pixels": int((N > 0).sum()), "pixels_with_history": int((N > 1).sum()),
                      "pixels": npix, "pixels_changed_by_clipping_gamma1_R3": int((hist[..., 0, :3] != plain[..., 0, :3]).any(-1).sum())}), flush=True)
    for rep in range(a.repeats):
        q0 = series(temporal, lambda st: st.ms_film)
        print(json.dumps({"repeat": rep, "kernel": "k_temporal", "mapping": "16 x 4 patches", "ms_q25_median_q75": q0}), flush=True)
        for R in RADII:
            q = series(clipped(R), lambda st: st.ms_film)
            print(json.dumps({"repeat": rep, "kernel": f"k_temporal_clip<{R}>", "ms_q25_median_q75": q, "multiple_of_k_temporal": round(q[1] / q0[1], 3)}), flush=True)
    q = series(clipped(3), lambda st: st.ms_total)
    print(json.dumps({"call": "trhip_temporal_clip_device, R = 3", "ms_total_q25_median_q75": q}), flush=True)


def accumulator(gamma, R, cap):
    """gamma None: the unclipped pass through trhip_temporal."""
    return T.TemporalAccumulator(max_history=cap) if gamma is None else T.TemporalAccumulator(max_history=cap, clip_gamma=gamma, clip_radius=R)


def sweep():
    import denoise_model as dm
    res, spp, depth, seed, step, lengths = 64, 2, 5, 0xBEEF, 0.75, (8, 40)
    ratios = {}
    for which, make in (("cornell", T.scenes.cornell_scene), ("mesh16", lambda: T.scenes.mesh_scene(16))):
        scene = make()
        ctx = scene.flatten().ctx
        cams = [camera(res, step * k) for k in range(max(lengths))]
        ref = {}
        for frames in lengths:
            last, offset = cams[frames - 1], (frames - 1) * spp
            smp = T.SeededSampler(spp, seed=seed, sample_offset=offset)
            noisy = T.PathIntegrator(last, smp, depth).render(scene)
            planes = T.AOVIntegrator(last, smp).render(scene).planes
            alone = T.Denoiser().render(scene, last, smp, depth, ctx)
            target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), depth).render(scene)
            surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))

            def mse(x, surface=surface, target=target):
                with np.errstate(all="ignore"):
                    diff = x[surface][:, :3].astype(np.float64) / x[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
                return float(np.mean(diff * diff))
            ref[frames] = (mse, mse(alone))
            print(json.dumps({"scene": which, "frames": frames, "surface_pixels": int(surface.sum()), "mse_2spp": round(mse(noisy), 6), "mse_denoiser_alone": round(mse(alone), 6)}), flush=True)
        for gamma, R in [(None, 0)] + [(gm, R) for R in RADII for gm in GAMMAS]:
            row = {"scene": which, "gamma": "unclipped" if gamma is None else jf(gamma), "R": R}
            for cap in CAPS:
                session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=accumulator(gamma, R, cap))
                for k, cam in enumerate(cams):
                    preview = session.render(cam, ctx)
                    if k + 1 in lengths:
                        mse, alone = ref[k + 1]
                        row[f"frames_{k + 1}_cap_{cap}"] = round(mse(preview) / alone, 4)
                        if cap == 8:
                            ratios.setdefault((gamma, R), []).append(mse(preview) / alone)
                session.close()
            print(json.dumps(row), flush=True)
    best = None
    for (gamma, R), v in ratios.items():
        gmean = float(np.exp(np.mean(np.log(v))))
        print(json.dumps({"gamma": "unclipped" if gamma is None else jf(gamma), "R": R, "geometric_mean_of_4_ratios_at_cap_8": round(gmean, 4)}), flush=True)
        if gamma is not None and gamma != INF and (best is None or gmean < best[0]):  # of the cells that clip: +Inf is the unclipped pass
            best = (gmean, gamma, R)
    print(json.dumps({"favoured_cell_among_those_that_clip": {"gamma": jf(best[1]), "R": best[2], "geometric_mean": round(best[0], 4)}}), flush=True)


def relight():
    import denoise_model as dm
    res, spp, depth, seed, before, after, factor = 48, 4, 3, 0x7E3A, 4, 2, 0.25
    scene = T.scenes.cornell_scene()
    lights = []
    for light in scene.lights:
        light = copy.copy(light)
        light.i = T.RGBSpectrum(*[float(np.float32(factor) * v) for v in light.i.c])
        lights.append(light)
    dim = scene.with_lights(lights)
    ctx = scene.flatten().ctx
    cam = camera(res, 0.0)
    targets = [T.PathIntegrator(cam, T.SeededSampler(1024, seed=0x7A26E7), depth).render(s) for s in (scene, dim)]
    smp = T.SeededSampler(spp, seed=seed, sample_offset=before * spp)
    noisy = T.PathIntegrator(cam, smp, depth).render(dim)
    planes = T.AOVIntegrator(cam, smp).render(dim).planes
    surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))

    def mse(x, target):
        with np.errstate(all="ignore"):
            diff = x[surface][:, :3].astype(np.float64) / x[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
        return float(np.mean(diff * diff))
    print(json.dumps({"relight": "cornell", "res": res, "spp": spp, "depth": depth, "frames_before": before, "frames_after": after, "factor": factor, "max_history": 8,
                      "surface_pixels": int(surface.sum()), "mse_4spp_first_frame_after": round(mse(noisy, targets[1]), 6),
                      "mse_denoiser_alone_first_frame_after": round(mse(T.Denoiser().render(dim, cam, smp, depth, ctx), targets[1]), 6)}), flush=True)
    unclipped = None
    for gamma, R in [(None, 0)] + [(gm, R) for R in RADII for gm in GAMMAS]:
        session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=accumulator(gamma, R, 8))
        series = []
        for k in range(before + after):
            if k == before:
                session.scene = dim
            series.append(mse(session.render(cam, ctx), targets[k >= before]))
        session.close()
        if gamma is None:
            unclipped = series
        print(json.dumps({"relight_gamma": "unclipped" if gamma is None else jf(gamma), "R": R, "mse_per_frame": [round(v, 6) for v in series],
                          "first_frame_after_over_unclipped": round(series[before] / unclipped[before], 4)}), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_sweep:
    sweep()
if not a.skip_relight:
    relight()
