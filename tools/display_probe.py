#!/usr/bin/env python
"""Display pass: python tools/display_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3] [--frames 12] [--skip-timing] [--skip-frames]

1. Kernel times at `--res`^2 on a path frame of the 1 M-triangle mesh scene and on a frame of one constant luminance (every metered pixel in one bin: the worst case for
   the histogram's LDS adds): trhip_display_device with the default parameters (meter, resolve, encode: trhip_stats.ms_sub[0..2]), with auto exposure off (encode alone), the
   `save` look, and k_temporal on the same frame beside them, alternating in one process, `--repeats` times over.  Device events around the launches; first quartile, median,
   third quartile of the runs after the warm-up; the multiple of k_temporal of the same repeat; TB/s against the compulsory bytes: 16 in for the meter, 16 in and 4 out for
   the encode, 36 per pixel for the pass.  (The meter with one LDS atomic per lane that the shipped one was measured against is no longer in the tree:
   profiles/r15/display.txt keeps its times.)
2. Wall-clock of a PreviewSession frame on the same scene at `--res`^2, `--spp` spp, depth `--depth`, ending in render_display (4 bytes per pixel leave the device) against
   the same frame ending the way it had to end before: render(), film.set_xyzw, film.to_rgb, np.rint to bytes.  Two sessions, alternating frame by frame, medians over
   `--frames` frames after two warm-up frames; native and with an upscaler (factor 2, guide_spp 1).
Prints JSON lines."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
a = ap.parse_args()


def camera(resolution):
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def display_calls(ctx, L, ptr, d_film, w, h, d_rgba, d_state):
    """{row name: call(stats)}: the display variants timed on one frame."""
    calls = {}
    for name, d in (("display default", T.Display()), ("display manual", T.Display(auto_exposure=False)), ("display save look", T.Display.reference())):
        calls[name] = lambda st, d=d: ctx.check(L.trhip_display_device(ctx._h, ptr(d_film), w, h, 1.0, C.byref(d.params), ptr(d_state), ptr(d_rgba), None, C.byref(st)))
    return calls


def timing():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    flat = scene.flatten()
    ctx, L, seed = flat.ctx, T.lib(), 0x5EED0001
    cam = camera(a.res)
    h, w = cam.film.size
    npix = h * w
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    d_film, d_flat, d_planes, d_out, d_hist, d_rgba, d_state = (T._ffi.DeviceBuffer(n) for n in (npix * 16, npix * 16, npix * 48, npix * 16, npix * 48, npix * 4, 16))
    sn = cam.sensor()
    ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, 0, ptr(d_film), C.byref(T.Stats())))
    ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, ptr(d_planes), None, C.byref(T.Stats())))
    d_flat.from_host(np.tile(np.array([0.2, 0.2, 0.2, 1.0], np.float32), (h, w, 1)))
    d_state.zero()
    hist = np.zeros(256, np.uint32)
    d = T.Display()
    rgba, _, hist = d.encode(d_film.to_host(np.float32, (h, w, 4)), 1.0, ctx=ctx, want_histogram=True)
    top = np.sort(hist)[::-1]
    print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "metered": int(hist.sum()), "non_empty_bins": int((hist > 0).sum()),
                      "share_of_the_four_fullest_bins": round(float(top[:4].sum() / max(1, hist.sum())), 3), "launches": d.stats.launches_film,
                      "bytes_per_pixel": {"meter": 16, "encode": 20, "pass": 36}}), flush=True)

    def series(call):
        rows = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                rows.append([st.ms_film, st.ms_sub[0], st.ms_sub[1], st.ms_sub[2]])
        return np.percentile(np.array(rows), [25, 50, 75], axis=0)  # (3, 4)
    tp = T.TemporalAccumulator()._params_for(None)
    for frame_name, d_in in (("path frame", d_film), ("constant luminance", d_flat)):
        calls = {"k_temporal": lambda st, d_in=d_in: ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_in), ptr(d_planes), None, w, h, C.byref(tp), ptr(d_out), ptr(d_hist), C.byref(st)))}
        calls.update(display_calls(ctx, L, ptr, d_in, w, h, d_rgba, d_state))
        for rep in range(a.repeats):
            q = {name: series(call) for name, call in calls.items()}
            yard = q["k_temporal"][1, 0]
            for name, v in q.items():
                r5 = lambda x: [round(float(t), 5) for t in x]  # noqa: E731
                row = {"frame": frame_name, "repeat": rep, "kernels": name, "ms_q25_median_q75": r5(v[:, 0]), "multiple_of_k_temporal": round(float(v[1, 0] / yard), 3)}
                if name.startswith("display"):
                    auto = name == "display default"
                    row["TB_per_s_of_compulsory_bytes"] = round(npix * (36 if auto else 20) / (v[1, 0] * 1e-3) * 1e-12, 3)
                    row["encode_ms_q25_median_q75"] = r5(v[:, 3])
                    row["encode_TB_per_s"] = round(npix * 20 / (v[1, 3] * 1e-3) * 1e-12, 3)
                    if auto:
                        row["meter_ms_q25_median_q75"], row["resolve_ms_q25_median_q75"] = r5(v[:, 1]), r5(v[:, 2])
                        row["meter_TB_per_s"] = round(npix * 16 / (v[1, 1] * 1e-3) * 1e-12, 3)
                print(json.dumps(row), flush=True)


def frame_times():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    ctx = scene.flatten().ctx
    cam, seed = camera(a.res), 0x5EED0001
    film = cam.film
    for label, kw in (("native", {}), ("upscaled factor 2 guide_spp 1", dict(upscaler=T.Upscaler(), factor=2, guide_spp=1))):
        shown = T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth, display=T.Display.reference(), **kw)
        toned = T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth, display=T.Display(), **kw)
        plain = T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth, **kw)

        def host_route():
            film.set_xyzw(plain.render(cam, ctx))
            return np.clip(np.rint(film.to_rgb(ctx)[::-1] * 255.0), 0, 255).astype(np.uint8)
        routes = [("host route: render, set_xyzw, to_rgb, rint", host_route), ("render_display, save look", lambda: shown.render_display(cam, ctx)),
                  ("render_display, defaults", lambda: toned.render_display(cam, ctx))]
        wall, last = {}, {}
        for k in range(a.frames + 2):
            for name, call in routes:
                t0 = time.perf_counter()
                last[name] = call()
                t1 = time.perf_counter()
                if k >= 2:
                    wall.setdefault(name, []).append((t1 - t0) * 1e3)
        same = bool(np.array_equal(last[routes[0][0]], last[routes[1][0]][..., :3]))
        base = float(np.median(wall[routes[0][0]]))
        for name in wall:
            print(json.dumps({"session": label, "route": name, "res": a.res, "spp": a.spp, "depth": a.depth, "n": len(wall[name]), "wall_ms_median": round(float(np.median(wall[name])), 3),
                              "wall_ms_q25_q75": [round(float(v), 3) for v in np.percentile(wall[name], [25, 75])], "speed_up_over_host_route": round(base / float(np.median(wall[name])), 3),
                              "display_device_ms": round(shown.render_stats[-1].ms_total, 4) if "save look" in name else (round(toned.render_stats[-1].ms_total, 4) if "defaults" in name else None),
                              "save_look_bytes_equal_host_route": same}), flush=True)
        for s in (shown, toned, plain):
            s.close()


if not a.skip_timing:
    timing()
if not a.skip_frames:
    frame_times()
