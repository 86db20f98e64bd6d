#!/usr/bin/env python
"""Moving geometry in a preview: python tools/motion_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3] [--skip-timing] [--skip-quality]

1. Times on the 1 M-triangle mesh scene, two frames through cameras 0.75 degrees apart, the second accumulated against the first one's history:
   - k_temporal_motion alternating with k_temporal (the 16 x 4 patch mapping both) in one process, `--repeats` times over; the height field (a million triangles, most of the
     picture) is one body with a small prev_from_cur, the walls and spheres are static.  Device events around the launch (trhip_stats.ms_film), quartiles over the runs;
     bytes per second against the compulsory traffic per pixel: 176 B for k_temporal (tools/temporal_probe.py), 192 B for k_temporal_motion (the id record's 16 more).
   - k_aov_ids: trhip_render_aov_ids_device with the id plane alone (ms_film is then the one launch), and the whole feature-buffer frame with and without the id plane,
     alternating (ms_total).
   - the session's frame: PreviewSession.render with motion={the height field: a small motion} against motion=None on the same static scene, host clock around the call
     (it ends in the download of the frame), alternating sessions.  A scene that really moved commits in full besides (not timed here: docs/design/20-motion.md).
2. Quality: the figures of tests/test_gpu_motion.py (eight frames at 64 x 64, 2 spp; still camera and arc) with the MSEs they are made of.
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
a = ap.parse_args()


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
    d_film, d_planes, d_hist0, d_hist1, d_out, d_ids = buf(16), buf(48), buf(48), buf(48), buf(16), buf(16)
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
        ctx.check(L.trhip_render_aov_ids_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, k * a.spp, ptr(d_planes), None, ptr(d_ids), None))

    frame(0)
    acc.accumulate_device(d_film.ptr, d_planes.ptr, None, w, h, None, d_out.ptr, d_hist0.ptr, ctx)
    frame(1)
    prm, mprm = acc._params_for(cams[0]), acc._motion_params_for(cams[0], table.size, 1)

    def temporal(st):
        ctx.check(L.trhip_temporal_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), w, h, C.byref(prm), ptr(d_out), ptr(d_hist1), C.byref(st)))

    def motion(st):
        ctx.check(L.trhip_temporal_motion_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), ptr(d_ids), ptr(d_table), ptr(d_mats), w, h, C.byref(mprm), ptr(d_out), ptr(d_hist1),
                                                 C.byref(st)))

    def series(call, key):
        out = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                out.append(key(st))
        return quartiles(out)

    motion(T.Stats())
    N = d_hist1.to_host(np.float32, (h, w, 3, 4))[..., 0, 3]
    ids = d_ids.to_host(T._ffi.AOV_ID_DTYPE, (h, w))
    moving = (ids["prim"] >= 0) & (table[np.where(ids["prim"] >= 0, ids["prim"], 0)] == 0)
    print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "pixels": npix, "surface_pixels": int((N > 0).sum()),
                      "pixels_with_history": int((N > 1).sum()), "pixels_on_the_moving_body": int(moving.sum()), "n_prims": int(table.size)}), flush=True)
    tb = lambda bytes_per_pixel, t: round(bytes_per_pixel * npix / (t * 1e-3) * 1e-12, 3)  # noqa: E731
    medians = {"k_temporal": [], "k_temporal_motion": []}
    for rep in range(a.repeats):
        for name, call, nbytes in (("k_temporal", temporal, 176.0), ("k_temporal_motion", motion, 192.0)):
            q = series(call, lambda st: st.ms_film)
            medians[name].append(q[1])
            print(json.dumps({"repeat": rep, "kernel": name, "ms_q25_median_q75": q, f"TB_per_s_of_{int(nbytes)}B_per_pixel": tb(nbytes, q[1])}), flush=True)
    print(json.dumps({"ratio_k_temporal_motion_over_k_temporal": round(float(np.median(medians["k_temporal_motion"]) / np.median(medians["k_temporal"])), 4),
                      "predicted_from_compulsory_bytes": round(192.0 / 176.0, 4)}), flush=True)
    # the id plane
    sn = cams[1].sensor()

    def aov(st, planes, ids_out):
        ctx.check(L.trhip_render_aov_ids_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, a.spp, ptr(d_planes) if planes else None, None, ptr(d_ids) if ids_out else None, C.byref(st)))

    runs, warm = max(a.runs // 10, 5), max(a.warmup // 10, 2)
    for rep in range(a.repeats):
        rows = {}
        for name, call, key in (("k_aov_ids (id plane alone: ms_film)", lambda st: aov(st, False, True), lambda st: st.ms_film),
                                ("feature-buffer frame, planes (ms_total)", lambda st: aov(st, True, False), lambda st: st.ms_total),
                                ("feature-buffer frame, planes and ids (ms_total)", lambda st: aov(st, True, True), lambda st: st.ms_total)):
            out = []
            for i in range(warm + runs):
                st = T.Stats()
                call(st)
                if i >= warm:
                    out.append(key(st))
            rows[name] = quartiles(out)
        print(json.dumps({"repeat": rep, "runs": runs, **rows}), flush=True)
    # the session's frame
    motion_dict = {mesh_entry: T.translate([0.002, 0.0, -0.001])}
    sessions = {"motion=None": (T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth), None),
                "motion={height field}": (T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth), motion_dict),
                "motion={}": (T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth), {})}
    wall = {k: [] for k in sessions}
    for k in range(a.session_frames):
        cam = ms.camera(T, a.res, 0.75 * k)
        for name, (session, m) in sessions.items():
            t0 = time.perf_counter()
            session.render(cam, ctx, motion=m)
            if k >= 2:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    for session, _ in sessions.values():
        session.close()
    print(json.dumps({"session_frame_ms_q25_median_q75": {k: quartiles(v) for k, v in wall.items()}, "frames": a.session_frames - 2}), flush=True)


def quality():
    import test_gpu_motion as tg
    ctx = T.default_context()
    for which in sorted(tg.QUALITY_CAMERAS):
        on_bodies, on_frame, n_bodies, figures = tg.quality_ratios(T, ctx, which)
        print(json.dumps({"sequence": which, **tg.QUALITY, "pixels_on_the_moving_bodies": n_bodies, "ratio_motion_over_plain_on_the_bodies": round(on_bodies, 4),
                          "ratio_motion_over_plain_on_the_frame": round(on_frame, 4), "mse": {f"{m}, {n}": round(v, 7) for (m, n), v in figures.items()}}), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_quality:
    quality()
