#!/usr/bin/env python
"""Direct light kept out of a preview's history: python tools/direct_split_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3]
                                                                                      [--skip-timing] [--skip-quality] [--skip-sweep]

1. Times on the 1 M-triangle mesh scene, set up as tools/motion_probe.py sets it up (two frames through cameras 0.75 degrees apart, the height field one moving body):
   - k_temporal_split alternating with k_temporal_motion in one process, `--repeats` times over, device events around the launch (trhip_stats.ms_film), quartiles over the
     runs; compulsory traffic 208 B per pixel against 192 (the direct film's 16 more);
   - k_film_add: 48 B per pixel, with its achieved bandwidth;
   - the depth-1 path frame and the depth-1 Whitted frame (ms_total), with the scene's one light and with a second one;
   - the session's frame, split_direct=True against False, with one light and with two, motion={the height field}; host clock around the call, alternating sessions.
2. Quality: the figures of tests/test_gpu_direct_split.py with the MSEs they are made of, and the plain session at 3 spp as the about-equal-time comparison.
3. The max_history sweep {8, 16, 32, 64} of the split and the plain session on the 8- and 40-frame arcs of tools/temporal_probe.py (Cornell and mesh_scene(16) under the front
   light, 64 x 64, 2 spp, depth 5, 0.75 degrees a frame; MSE over the last frame against its 1024 spp frame).  The rule, fixed before the sweep: the cap with the lowest
   geometric mean over the four arcs.
Prints JSON lines."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import __graft_entry__ as g
import motion_scenes as ms
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--runs", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--session-frames", type=int, default=12)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--skip-timing", action="store_true")
ap.add_argument("--skip-quality", action="store_true")
ap.add_argument("--skip-sweep", action="store_true")
a = ap.parse_args()
FRONT_LIGHT, SECOND_LIGHT = ((0.5, 0.5, -1.5), 2.5), ((0.2, 0.6, -2.2), 1.0)


def lights(*which):
    return [T.PointLight(T.translate(list(at)), T.RGBSpectrum(power)) for at, power in which]


def quartiles(ms_list):
    return [round(float(v), 5) for v in np.percentile(ms_list, [25, 50, 75])]


def timing():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    flat = scene.flatten()
    ctx, L, seed = flat.ctx, T.lib(), 0x5EED0001
    cams = [ms.camera(T, a.res, 0.0), ms.camera(T, a.res, 0.75)]
    h, w = cams[0].film.size
    npix = h * w
    buf = lambda n: T._ffi.DeviceBuffer(npix * n)  # noqa: E731
    d_film, d_direct, d_planes, d_hist0, d_hist1, d_out, d_ids = buf(16), buf(16), buf(48), buf(48), buf(48), buf(16), buf(16)
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    acc = T.TemporalAccumulator()
    counts = T.top_level_counts(scene)
    mesh_entry = int(np.argmax(counts))  # the height field
    table = flat.body_table([0 if i == mesh_entry else None for i in range(len(counts))])
    mats = T.TemporalAccumulator.prev_from_cur(T.translate([0.002, 0.0, -0.001])).reshape(1, 12)
    d_table, d_mats = T._ffi.DeviceBuffer(table.nbytes).from_host(table), T._ffi.DeviceBuffer(mats.nbytes).from_host(mats)

    def frame(k):
        sn = cams[k].sensor()
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, k * a.spp, ptr(d_film), None))
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, 1, seed, k * a.spp, ptr(d_direct), None))
        ctx.check(L.trhip_render_aov_ids_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, k * a.spp, ptr(d_planes), None, ptr(d_ids), None))

    frame(0)
    acc.accumulate_split_device(d_film.ptr, d_direct.ptr, d_planes.ptr, None, None, None, 0, None, 0, w, h, None, d_out.ptr, d_hist0.ptr, ctx)
    frame(1)
    mprm = acc._motion_params_for(cams[0], table.size, 1)

    def motion(st):
        ctx.check(L.trhip_temporal_motion_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), ptr(d_ids), ptr(d_table), ptr(d_mats), w, h, C.byref(mprm), ptr(d_out), ptr(d_hist1),
                                                 C.byref(st)))

    def split(st):
        ctx.check(L.trhip_temporal_split_device(ctx._h, ptr(d_film), ptr(d_direct), ptr(d_planes), ptr(d_hist0), ptr(d_ids), ptr(d_table), ptr(d_mats), w, h, C.byref(mprm), ptr(d_out),
                                                ptr(d_hist1), C.byref(st)))

    def add(st):
        ctx.check(L.trhip_film_add_device(ctx._h, ptr(d_film), ptr(d_direct), w, h, ptr(d_out), C.byref(st)))

    def series(call, key, runs=a.runs, warmup=a.warmup):
        out = []
        for i in range(warmup + runs):
            st = T.Stats()
            call(st)
            if i >= warmup:
                out.append(key(st))
        return quartiles(out)

    split(T.Stats())
    N = d_hist1.to_host(np.float32, (h, w, 3, 4))[..., 0, 3]
    direct = d_direct.to_host(np.float32, (h, w, 4))
    film = d_film.to_host(np.float32, (h, w, 4))
    print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "pixels": npix, "surface_pixels": int((N > 0).sum()),
                      "pixels_with_history": int((N > 1).sum()), "share_of_Y_that_is_first_hit_direct": round(float(direct[..., 1].sum() / film[..., 1].sum()), 4)}), flush=True)
    tb = lambda bytes_per_pixel, t: round(bytes_per_pixel * npix / (t * 1e-3) * 1e-12, 3)  # noqa: E731
    medians = {"k_temporal_motion": [], "k_temporal_split": [], "k_film_add": []}
    for rep in range(a.repeats):
        for name, call, nbytes in (("k_temporal_motion", motion, 192.0), ("k_temporal_split", split, 208.0), ("k_film_add", add, 48.0)):
            q = series(call, lambda st: st.ms_film)
            medians[name].append(q[1])
            print(json.dumps({"repeat": rep, "kernel": name, "ms_q25_median_q75": q, f"TB_per_s_of_{int(nbytes)}B_per_pixel": tb(nbytes, q[1])}), flush=True)
    print(json.dumps({"ratio_k_temporal_split_over_k_temporal_motion": round(float(np.median(medians["k_temporal_split"]) / np.median(medians["k_temporal_motion"])), 4),
                      "predicted_from_compulsory_bytes": round(208.0 / 192.0, 4), "k_film_add_ms": float(np.median(medians["k_film_add"])),
                      "k_film_add_TB_per_s": tb(48.0, float(np.median(medians["k_film_add"])))}), flush=True)
    # the direct frames and the session's frame, with one light and with two
    sn = cams[1].sensor()
    two = scene.with_lights(list(scene.lights) + lights(SECOND_LIGHT))
    runs, warm = max(a.runs // 10, 5), max(a.warmup // 10, 2)
    motion_dict = {mesh_entry: T.translate([0.002, 0.0, -0.001])}
    for name, sc in (("one light", scene), ("two lights", two)):
        fl = sc.flatten()
        rows = {}
        for what, entry, depth in (("path frame, full depth", L.trhip_render_path_device, a.depth), ("path frame, depth 1", L.trhip_render_path_device, 1),
                                   ("Whitted frame, depth 1", L.trhip_render_whitted_device, 1)):
            rows[what] = series(lambda st: ctx.check(entry(ctx._h, fl._h, C.byref(sn), a.spp, depth, seed, a.spp, ptr(d_out), C.byref(st))), lambda st: st.ms_total, runs, warm)
        print(json.dumps({"lights": name, "n_lights": len(sc.lights), "runs": runs, "ms_total_q25_median_q75": rows}), flush=True)
        sessions = {"split_direct=False": T.PreviewSession(sc, T.SeededSampler(a.spp, seed=seed), a.depth),
                    "split_direct=True": T.PreviewSession(sc, T.SeededSampler(a.spp, seed=seed), a.depth, split_direct=True)}
        wall = {k: [] for k in sessions}
        for k in range(a.session_frames):
            cam = ms.camera(T, a.res, 0.75 * k)
            for key, session in sessions.items():
                t0 = time.perf_counter()
                session.render(cam, ctx, motion=motion_dict)
                if k >= 2:
                    wall[key].append((time.perf_counter() - t0) * 1e3)
        for session in sessions.values():
            session.close()
        q = {k: quartiles(v) for k, v in wall.items()}
        print(json.dumps({"lights": name, "session_frame_ms_q25_median_q75": q, "ratio_split_over_plain": round(q["split_direct=True"][1] / q["split_direct=False"][1], 4),
                          "frames": a.session_frames - 2}), flush=True)


def quality():
    import test_gpu_direct_split as tg
    ctx = T.default_context()
    for n_lights in sorted(tg.QUALITY_LIGHTS):
        for which in sorted(tg.QUALITY_CAMERAS):
            case = tg.QualityCase(T, ctx, which, n_lights)
            rows = {"plain": case.mse(case.last_frame(False)), "split": case.mse(case.last_frame(True)), "plain at 3 spp": case.mse(case.last_frame(False, spp=3))}
            if n_lights == "two lights":
                rows["split, the depth-1 path film put back"] = case.mse(case.last_frame(True, whitted=False))
            print(json.dumps({"lights": n_lights, "sequence": which, **tg.QUALITY, "pixels": {k: int(m.sum()) for k, m in case.masks.items()},
                              "mse": {k: {m: round(x, 8) for m, x in v.items()} for k, v in rows.items()},
                              "ratio_over_plain": {k: {m: round(v[m] / rows["plain"][m], 4) for m in v} for k, v in rows.items() if k != "plain"}}), flush=True)


def sweep():
    ctx = T.default_context()
    res, spp, depth, seed, step, lengths, caps = 64, 2, 5, 0xBEEF, 0.75, (8, 40), (8.0, 16.0, 32.0, 64.0)
    scenes = {"cornell": T.scenes.cornell_scene().with_lights(lights(FRONT_LIGHT)), "mesh16": T.scenes.mesh_scene(16).with_lights(lights(FRONT_LIGHT))}
    table = {}
    for name, scene in scenes.items():
        for n in lengths:
            cams = [ms.camera(T, res, step * k) for k in range(n)]
            target = T.PathIntegrator(cams[-1], T.SeededSampler(1024, seed=0x7A26E7), depth).render(scene)
            mask = target[..., 3] > 0
            for split in (False, True):
                for cap in caps:
                    session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=T.TemporalAccumulator(max_history=cap), split_direct=split)
                    for cam in cams:
                        out = session.render(cam, ctx)
                    session.close()
                    ok = mask & (out[..., 3] > 0)
                    diff = out[ok][:, :3].astype(np.float64) / out[ok][:, 3:4] - target[ok][:, :3].astype(np.float64) / target[ok][:, 3:4]
                    table[(name, n, split, cap)] = float(np.mean(diff * diff))
            print(json.dumps({"scene": name, "frames": n, **{f"{'split' if s else 'plain'}, cap {int(c)}": round(table[(name, n, s, c)], 8) for s in (False, True) for c in caps}}), flush=True)
    for split in (False, True):
        means = {int(c): round(float(np.exp(np.mean([np.log(table[(name, n, split, c)]) for name in scenes for n in lengths]))), 8) for c in caps}
        print(json.dumps({"session": "split" if split else "plain", "geometric_mean_mse_over_the_four_arcs_by_cap": means, "lowest": min(means, key=means.get)}), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_quality:
    quality()
if not a.skip_sweep:
    sweep()
