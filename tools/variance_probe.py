#!/usr/bin/env python
"""Luminance moments and the variance-guided filter: python tools/variance_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3]
[--skip-timing] [--skip-sweep] [--skip-single]

1. Times, on the 1 M-triangle mesh scene, k_temporal, k_temporal_clip<3>, k_temporal_moments, k_denoise_atrous and k_denoise_var_atrous gathered and staged, alternating in one process, `--repeats`
   times over.  Two frame states: a FIRST frame (no history: every pixel takes the spatial estimate) and a STEADY-STATE frame (the ninth camera of an arc of 0.75-degree
   steps, accumulated against eight frames of history and moments).  Device events around the launches (trhip_stats.ms_film, ms_sub[1]); first quartile, median, third
   quartile of the runs after the warm-up; ratios to k_temporal_clip<3> and to k_denoise_atrous of the same repeat; TB/s against the compulsory bytes per pixel
   (moments: film 16 + planes 48 + one history record 48 + one moment pair 8 in, film 16 + history 48 + moments 8 + variance 4 out = 196, 140 on a first frame;
   an à-trous iteration 64, a variance-guided one 72).  The time of iteration i is the iterations' kernel time of a call with i + 1 iterations minus that of a call with i.
2. Sweeps sigma_colour in {1, 2, 4, 8} x var_eps in {2^-12, 2^-6} x spatial_below in {2, 4} x max_history in {8, 16, 32, 64} on the arcs of tools/temporal_probe.py and
   tools/temporal_clip_probe.py (Cornell and mesh_scene(16), 64 x 64, 2 spp, depth 5, seed 0xBEEF, cameras 0.75 degrees apart), 8 and 40 frames: MSE of xyz / w over the
   surface pixels of the last frame against its own 1024 spp frame, guided preview / Denoiser alone.  The frames are rendered once; a cell chains trhip_temporal_moments over
   them and filters the two frames that are measured, which is PreviewSession(variance_guided=True) call for call (checked here for one cell against the session itself).
   The unguided PreviewSession cells of profiles/r11/temporal.txt are recomputed through the session.  Then the geometric mean of the four ratios per cell: the rule for
   the defaults (the lowest).
3. A single 4 spp frame through Denoiser.render(variance_guided=True) against Denoiser.render on the frames of tests/test_gpu_denoise.py, per sigma_colour and var_eps.
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
ap.add_argument("--history-frames", type=int, default=8)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--skip-sweep", action="store_true")
ap.add_argument("--skip-single", action="store_true")
a = ap.parse_args()
CENTRE = np.array([0.5, 0.4, -2.5])
SIGMAS, EPSILONS, BELOWS, CAPS = (1.0, 2.0, 4.0, 8.0), (2.0 ** -12, 2.0 ** -6), (2.0, 4.0), (8, 16, 32, 64)


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
    cams = [camera(a.res, 0.75 * k) for k in range(a.history_frames + 1)]
    h, w = cams[0].film.size
    npix = h * w
    buf = lambda n: T._ffi.DeviceBuffer(npix * n)  # noqa: E731
    d_film, d_planes, d_out, d_var, d_den = buf(16), buf(48), buf(16), buf(4), buf(16)
    d_hist, d_mom = [buf(48), buf(48)], [buf(8), buf(8)]
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    acc, plain, clip, den = T.TemporalAccumulator(moments=True), T.TemporalAccumulator(), T.TemporalAccumulator(clip_gamma=1.0, clip_radius=3), T.Denoiser()

    def frame(k):
        sn = cams[k].sensor()
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, k * a.spp, ptr(d_film), C.byref(T.Stats())))
        ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, k * a.spp, ptr(d_planes), None, C.byref(T.Stats())))

    def series(call, key):
        ms = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                ms.append(key(st))
        return [round(float(v), 5) for v in np.percentile(ms, [25, 50, 75])]

    def temporal_calls(prev_cam, have):
        """The three temporal passes on the frame in d_film / d_planes against d_hist[0] / d_mom[0] (or nothing), writing d_hist[1] / d_mom[1]."""
        prm, cp, mp = plain._params_for(prev_cam), clip._clip_params_for(prev_cam), acc._moments_params_for(prev_cam)
        hist, mom = (ptr(d_hist[0]), ptr(d_mom[0])) if have else (None, None)
        return {
            "k_temporal": lambda st: ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_film), ptr(d_planes), hist, w, h, C.byref(prm), ptr(d_out), ptr(d_hist[1]), C.byref(st))),
            "k_temporal_clip<3>": lambda st: ctx.check(L.trhip_temporal_clip_device(ctx._h, ptr(d_film), ptr(d_planes), hist, w, h, C.byref(cp), ptr(d_out), ptr(d_hist[1]), C.byref(st))),
            "k_temporal_moments": lambda st: ctx.check(L.trhip_temporal_moments_device(ctx._h, ptr(d_film), ptr(d_planes), hist, mom, w, h, C.byref(mp), ptr(d_out), ptr(d_hist[1]),
                                                                                       ptr(d_mom[1]), ptr(d_var), C.byref(st))),
        }

    def time_temporal(state, calls, bytes_per_pixel):
        for rep in range(a.repeats):
            q = {}
            q["k_temporal"] = series(calls["k_temporal"], lambda st: st.ms_film)
            q["k_temporal_clip<3>"] = series(calls["k_temporal_clip<3>"], lambda st: st.ms_film)
            q["k_temporal_moments"] = series(calls["k_temporal_moments"], lambda st: st.ms_film)
            for name, v in q.items():
                row = {"state": state, "repeat": rep, "kernel": name, "ms_q25_median_q75": v, "multiple_of_k_temporal_clip3": round(v[1] / q["k_temporal_clip<3>"][1], 3)}
                if name.startswith("k_temporal_moments"):
                    row[f"TB_per_s_of_{bytes_per_pixel}B_per_pixel"] = round(bytes_per_pixel * npix / (v[1] * 1e-3) * 1e-12, 3)
                print(json.dumps(row), flush=True)

    def time_denoise(state):
        """Per-iteration times of the plain and the variance-guided iteration on the frame in d_out (the accumulated film) with the variance in d_var."""
        def plain_call(st, k):
            p = T._ffi.DenoiseParams.from_buffer_copy(den.params)
            p.iterations = k
            ctx.check(L.trhip_denoise_device(ctx._h, ptr(d_out), ptr(d_planes), w, h, C.byref(p), ptr(d_den), C.byref(st)))

        def var_call(st, k):
            vp = den._var_params()
            vp.base.iterations = k
            ctx.check(L.trhip_denoise_var_device(ctx._h, ptr(d_out), ptr(d_planes), ptr(d_var), w, h, C.byref(vp), ptr(d_den), None, C.byref(st)))
        for rep in range(a.repeats):
            rows = {}
            for kernel, call, option, bytes_pp in (("k_denoise_atrous", plain_call, "denoise_lds", 64), ("k_denoise_var_atrous", var_call, "denoise_var_lds", 72)):
                for form, mask in (("gather", 0), ("lds", 3)):
                    ctx.set_option(option, mask)
                    n_it = 2 if form == "lds" else 5  # the staged kernels exist for steps 1 and 2
                    cum = [0.0] + [series(lambda st, k=k: call(st, k), lambda st: st.ms_sub[1])[1] for k in range(1, n_it + 1)]
                    for i in range(n_it):
                        rows[(kernel, form, i)] = (cum[i + 1] - cum[i], bytes_pp)
                ctx.set_option(option, 3)
            for (kernel, form, i), (ms, bytes_pp) in rows.items():
                base = rows[("k_denoise_atrous", form, i)][0]
                print(json.dumps({"state": state, "repeat": rep, "kernel": kernel, "form": form, "iteration": i, "step": 1 << i, "ms": round(ms, 5),
                                  "multiple_of_k_denoise_atrous_same_form": round(ms / base, 3) if base > 0 else None,
                                  f"TB_per_s_of_{bytes_pp}B_per_pixel": round(bytes_pp * npix / (ms * 1e-3) * 1e-12, 3) if ms > 0 else None}), flush=True)
            edges = series(lambda st: var_call(st, 1), lambda st: st.ms_sub[0] + st.ms_sub[2])
            print(json.dumps({"state": state, "repeat": rep, "kernels": "prepare + seed + finish of trhip_denoise_var (no export)", "ms_q25_median_q75": edges}), flush=True)

    # ---- a first frame
    frame(0)
    calls = temporal_calls(None, False)
    calls["k_temporal_moments"](T.Stats())
    var = d_var.to_host(np.float32, (h, w))
    N = d_hist[1].to_host(np.float32, (h, w, 3, 4))[..., 0, 3]
    print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "state": "first frame", "pixels": npix, "surface_pixels": int((N > 0).sum()),
                      "variance_median_over_surface": float(np.median(var[N > 0]))}), flush=True)
    time_temporal("first frame", calls, 140)
    time_denoise("first frame")
    # ---- a steady-state frame: a.history_frames frames of history behind it
    for k in range(a.history_frames):
        frame(k)
        mp = acc._moments_params_for(cams[k - 1] if k else None)
        ctx.check(L.trhip_temporal_moments_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist[0]) if k else None, ptr(d_mom[0]) if k else None, w, h, C.byref(mp), ptr(d_out),
                                                  ptr(d_hist[1]), ptr(d_mom[1]), ptr(d_var), C.byref(T.Stats())))
        d_hist.reverse(), d_mom.reverse()
    frame(a.history_frames)
    calls = temporal_calls(cams[a.history_frames - 1], True)
    calls["k_temporal_moments"](T.Stats())
    N = d_hist[1].to_host(np.float32, (h, w, 3, 4))[..., 0, 3]
    below = (N > 0) & (N < acc.moments_params.spatial_below)
    patches = below.reshape(h // 4, 4, w // 16, 16).any(axis=(1, 3)) if h % 4 == 0 and w % 16 == 0 else None
    print(json.dumps({"state": "steady state", "history_frames": a.history_frames, "surface_pixels": int((N > 0).sum()), "pixels_at_the_cap": int((N == acc.params.max_history).sum()),
                      "pixels_below_spatial_below": int(below.sum()), "spatial_below": acc.moments_params.spatial_below,
                      "patches_16x4_with_such_a_pixel": None if patches is None else int(patches.sum()), "patches_16x4": None if patches is None else int(patches.size)}), flush=True)
    time_temporal("steady state", calls, 196)
    time_denoise("steady state")
    q = series(calls["k_temporal_moments"], lambda st: st.ms_total)
    print(json.dumps({"call": "trhip_temporal_moments_device, steady state", "ms_total_q25_median_q75": q}), flush=True)


def arc_frames(scene, cams, spp, depth, seed):
    return [(T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed, sample_offset=k * spp), depth).render(scene),
             T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed, sample_offset=k * spp)).render(scene).planes) for k, cam in enumerate(cams)]


def sweep():
    import denoise_model as dm
    res, spp, depth, seed, step, lengths = 64, 2, 5, 0xBEEF, 0.75, (8, 40)
    ratios, unguided = {}, {}
    for which, make in (("cornell", T.scenes.cornell_scene), ("mesh16", lambda: T.scenes.mesh_scene(16))):
        scene = make()
        ctx = scene.flatten().ctx
        cams = [camera(res, step * k) for k in range(max(lengths))]
        frames = arc_frames(scene, cams, spp, depth, seed)
        ref = {}
        for n in lengths:
            last, offset = cams[n - 1], (n - 1) * spp
            noisy, planes = frames[n - 1]
            alone = T.Denoiser().render(scene, last, T.SeededSampler(spp, seed=seed, sample_offset=offset), depth, ctx)
            target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), depth).render(scene)
            surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))

            def mse(x, surface=surface, target=target):
                with np.errstate(all="ignore"):
                    diff = x[surface][:, :3].astype(np.float64) / x[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
                return float(np.mean(diff * diff))
            ref[n] = (mse, mse(alone))
            print(json.dumps({"scene": which, "frames": n, "surface_pixels": int(surface.sum()), "mse_2spp": round(mse(noisy), 6), "mse_denoiser_alone": round(mse(alone), 6)}), flush=True)
        row = {"scene": which, "session": "unguided PreviewSession"}
        for cap in CAPS:
            session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=T.TemporalAccumulator(max_history=cap))
            for k, cam in enumerate(cams):
                preview = session.render(cam, ctx)
                if k + 1 in lengths:
                    mse, alone = ref[k + 1]
                    row[f"frames_{k + 1}_cap_{cap}"] = round(mse(preview) / alone, 4)
                    unguided.setdefault(cap, []).append(mse(preview) / alone)
            session.close()
        print(json.dumps(row), flush=True)
        for below in BELOWS:
            for cap in CAPS:
                t = T.TemporalAccumulator(max_history=cap, moments=True, spatial_below=below)
                hist = mom = prev = None
                kept = {}
                for k, (xyzw, planes) in enumerate(frames):
                    acc, hist, mom, var = t.accumulate_moments(xyzw, planes, hist, mom, prev, ctx)
                    prev = cams[k]
                    if k + 1 in lengths:
                        kept[k + 1] = (acc if k else xyzw, planes, var)
                for sigma in SIGMAS:
                    for eps in EPSILONS:
                        d = T.Denoiser(variance_sigma=sigma, var_eps=eps)
                        cell = (sigma, eps, below, cap)
                        for n in lengths:
                            mse, alone = ref[n]
                            out = d.denoise_variance(*kept[n], ctx)[0]
                            ratios.setdefault(cell, []).append(mse(out) / alone)
                        if cell == (4.0, EPSILONS[1], 4.0, 8):  # the chain is the session, call for call
                            session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, denoiser=T.Denoiser(variance_sigma=sigma, var_eps=eps),
                                                       temporal=T.TemporalAccumulator(max_history=cap, moments=True, spatial_below=below), variance_guided=True)
                            for k, cam in enumerate(cams):
                                preview = session.render(cam, ctx)
                            session.close()
                            assert np.array_equal(preview.view(np.uint32), out.view(np.uint32)), "the chained calls are not the session's bits"
                            print(json.dumps({"scene": which, "check": "chained calls == PreviewSession(variance_guided=True), 40 frames", "equal": True}), flush=True)
        for below in BELOWS:
            for sigma in SIGMAS:
                for eps in EPSILONS:
                    row = {"scene": which, "sigma_colour": sigma, "var_eps": eps, "spatial_below": below}
                    for cap in CAPS:
                        v = ratios[(sigma, eps, below, cap)][-2:]
                        row[f"frames_8_cap_{cap}"], row[f"frames_40_cap_{cap}"] = round(v[0], 4), round(v[1], 4)
                    print(json.dumps(row), flush=True)
    for cap in CAPS:
        print(json.dumps({"session": "unguided PreviewSession", "max_history": cap, "geometric_mean_of_4_ratios": round(float(np.exp(np.mean(np.log(unguided[cap])))), 4)}), flush=True)
    best = None
    for cell, v in sorted(ratios.items()):
        gmean = float(np.exp(np.mean(np.log(v))))
        print(json.dumps({"sigma_colour": cell[0], "var_eps": cell[1], "spatial_below": cell[2], "max_history": cell[3], "geometric_mean_of_4_ratios": round(gmean, 4)}), flush=True)
        if best is None or gmean < best[0]:
            best = (gmean, cell)
    print(json.dumps({"favoured_cell": dict(zip(("sigma_colour", "var_eps", "spatial_below", "max_history"), best[1])), "geometric_mean": round(best[0], 4)}), flush=True)


def single():
    """tests/test_gpu_denoise.py's quality frames: 64 x 64, 4 spp, depth 5; ratio to the 4 spp frame's own MSE."""
    import denoise_model as dm
    for which, make in (("cornell", T.scenes.cornell_scene), ("mesh16", lambda: T.scenes.mesh_scene(16))):
        scene, cam = make(), camera(64, 0.0)
        ctx = scene.flatten().ctx
        smp = lambda: T.SeededSampler(4, seed=0xBEEF)  # noqa: E731
        noisy = T.PathIntegrator(cam, smp(), 5).render(scene)
        planes = T.AOVIntegrator(cam, smp()).render(scene).planes
        target = T.PathIntegrator(cam, T.SeededSampler(1024, seed=0x7A26E7), 5).render(scene)
        surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))

        def mse(x):
            with np.errstate(all="ignore"):
                diff = x[surface][:, :3].astype(np.float64) / x[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
            return float(np.mean(diff * diff))
        before = mse(noisy)
        row = {"single_frame": which, "spp": 4, "mse_4spp": round(before, 6), "Denoiser.render": round(mse(T.Denoiser().render(scene, cam, smp(), 5, ctx)) / before, 4),
               "Denoiser.render(variance_guided=True), defaults": round(mse(T.Denoiser().render(scene, cam, smp(), 5, ctx, variance_guided=True)) / before, 4)}
        for sigma in SIGMAS:
            for eps in EPSILONS:
                out = T.Denoiser(variance_sigma=sigma, var_eps=eps).render(scene, cam, smp(), 5, ctx, variance_guided=True)
                row[f"guided_sigma_{sigma:g}_eps_{eps:g}"] = round(mse(out) / before, 4)
        print(json.dumps(row), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_sweep:
    sweep()
if not a.skip_single:
    single()
