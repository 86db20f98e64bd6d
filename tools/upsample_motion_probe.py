#!/usr/bin/env python
"""Temporal upsampling under motion: python tools/upsample_motion_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3] [--skip-session]

Times on the 1 M-triangle mesh scene, full size `res`^2 from (`res` / 2)^2, two frames through cameras 0.75 degrees apart and two jitters of the grid, the second
accumulated against the first one's full-size history, the height field one moving body (tools/clip_motion_probe.py's frame, at two sizes):
k_temporal_upsample_motion<R> alternating with k_temporal_upsample<R> (R = 1, 2) in one process, `--repeats` times over.  Device events around the launch
(trhip_stats.ms_film), quartiles over the runs; the ratio to k_temporal_upsample<R> beside the one predicted from the compulsory bytes per full-size pixel (192 against 176:
the id record's line is the only new stream).  Then the session's frame: PreviewSession(upscaler, temporal_upsample=TemporalUpsampler(carry_bodies=True)).render with
motion={the height field} against the same session with motion=None, host clock around the call, alternating sessions.
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
ap.add_argument("--skip-session", action="store_true")
a = ap.parse_args()
RADII = (1, 2)


def quartiles(ms_list):
    return [round(float(v), 5) for v in np.percentile(ms_list, [25, 50, 75])]


def main():
    scene = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene])
    flat = scene.flatten()
    ctx, L, seed = flat.ctx, T.lib(), 0x5EED0001
    cams = [ms.camera(T, a.res, 0.0), ms.camera(T, a.res, 0.75)]
    tu = T.TemporalUpsampler()
    lo_cams = [T.Upscaler.low_camera(c, 2, jitter=tu.jitter_for(k, 2)) for k, c in enumerate(cams)]
    (h, w), (lh, lw) = cams[0].film.size, lo_cams[0].film.size
    npix, nlo = h * w, lh * lw
    d_lo, d_lo_planes = T._ffi.DeviceBuffer(nlo * 16), T._ffi.DeviceBuffer(nlo * 48)
    buf = lambda n: T._ffi.DeviceBuffer(npix * n)  # noqa: E731
    d_planes, d_hist0, d_hist1, d_out, d_ids, d_mask = buf(48), buf(48), buf(48), buf(16), buf(16), buf(1)
    ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
    counts = T.top_level_counts(scene)
    mesh_entry = int(np.argmax(counts))  # the height field
    table = flat.body_table([0 if i == mesh_entry else None for i in range(len(counts))])
    mats = T.TemporalAccumulator.prev_from_cur(T.translate([0.002, 0.0, -0.001])).reshape(1, 12)
    d_table, d_mats = T._ffi.DeviceBuffer(table.nbytes).from_host(table), T._ffi.DeviceBuffer(mats.nbytes).from_host(mats)

    def frame(k):
        lo_sn, sn = lo_cams[k].sensor(), cams[k].sensor()
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(lo_sn), a.spp, a.depth, seed, k * a.spp, ptr(d_lo), None))
        ctx.check(L.trhip_render_aov_ids_device(ctx._h, flat._h, C.byref(lo_sn), a.spp, seed, k * a.spp, ptr(d_lo_planes), None, None, None))
        ctx.check(L.trhip_render_aov_ids_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, k * a.spp, ptr(d_planes), None, ptr(d_ids), None))

    frame(0)
    tu.accumulate_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_planes.ptr, None, w, h, T.Upscaler.pixel_map(cams[0], lo_cams[0]), None, d_out.ptr, d_hist0.ptr, None, ctx)
    frame(1)
    m = T.Upscaler.pixel_map(cams[1], lo_cams[1])
    plain = {R: T.TemporalUpsampler(radius=R)._params_for(m, cams[0]) for R in RADII}
    both = {R: T.TemporalUpsampler(radius=R, carry_bodies=True)._motion_params_for(m, cams[0], table.size, 1) for R in RADII}

    def parent(R):
        return lambda st: ctx.check(L.trhip_temporal_upsample_device(ctx._h, ptr(d_lo), ptr(d_lo_planes), lw, lh, ptr(d_planes), ptr(d_hist0), w, h, C.byref(plain[R]), ptr(d_out),
                                                                     ptr(d_hist1), ptr(d_mask), C.byref(st)))

    def motion(R):
        return lambda st: ctx.check(L.trhip_temporal_upsample_motion_device(ctx._h, ptr(d_lo), ptr(d_lo_planes), lw, lh, ptr(d_planes), ptr(d_hist0), ptr(d_ids), ptr(d_table),
                                                                            ptr(d_mats), w, h, C.byref(both[R]), ptr(d_out), ptr(d_hist1), ptr(d_mask), C.byref(st)))

    def series(call):
        out = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                out.append(st.ms_film)
        return quartiles(out)

    motion(1)(T.Stats())
    mask = d_mask.to_host(np.uint8, (h, w))
    parent(1)(T.Stats())
    mask_blind = d_mask.to_host(np.uint8, (h, w))
    ids = d_ids.to_host(T._ffi.AOV_ID_DTYPE, (h, w))
    moving = (ids["prim"] >= 0) & (table[np.where(ids["prim"] >= 0, ids["prim"], 0)] == 0)
    print(json.dumps({"library": os.path.basename(T._ffi.LIB_PATH), "scene": a.scene, "res": a.res, "low_res": [lw, lh], "spp": a.spp, "depth": a.depth, "runs": a.runs, "pixels": npix,
                      "pixels_with_history_with_motion": int((mask >= 4).sum()), "pixels_with_history_motion_blind": int((mask_blind >= 4).sum()),
                      "pixels_on_the_moving_body": int(moving.sum()), "n_prims": int(table.size)}), flush=True)
    medians = {}
    for rep in range(a.repeats):
        calls = []
        for R in RADII:
            calls += [(f"k_temporal_upsample<{R}>", parent(R)), (f"k_temporal_upsample_motion<{R}>", motion(R))]
        for name, call in calls:
            q = series(call)
            medians.setdefault(name, []).append(q[1])
            print(json.dumps({"repeat": rep, "kernel": name, "ms_q25_median_q75": q}), flush=True)
    med = {k: float(np.median(v)) for k, v in medians.items()}
    for R in RADII:
        print(json.dumps({"R": R, "k_temporal_upsample_motion_ms": round(med[f"k_temporal_upsample_motion<{R}>"], 5), "k_temporal_upsample_ms": round(med[f"k_temporal_upsample<{R}>"], 5),
                          "ratio_over_k_temporal_upsample": round(med[f"k_temporal_upsample_motion<{R}>"] / med[f"k_temporal_upsample<{R}>"], 4),
                          "predicted_from_compulsory_bytes_at_most": round(192.0 / 176.0, 4)}), flush=True)
    if a.skip_session:
        return
    motion_dict = {mesh_entry: T.translate([0.002, 0.0, -0.001])}
    sessions = {"motion=None": (T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth, upscaler=T.Upscaler(), factor=2,
                                                 temporal_upsample=T.TemporalUpsampler(carry_bodies=True)), None),
                "motion={height field}": (T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth, upscaler=T.Upscaler(), factor=2,
                                                           temporal_upsample=T.TemporalUpsampler(carry_bodies=True)), motion_dict)}
    wall = {k: [] for k in sessions}
    for k in range(a.session_frames):
        cam = ms.camera(T, a.res, 0.75 * k)
        for name, (session, mo) in sessions.items():
            t0 = time.perf_counter()
            session.render(cam, ctx, motion=mo)
            if k >= 2:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    for session, _ in sessions.values():
        session.close()
    print(json.dumps({"session_frame_ms_q25_median_q75": {k: quartiles(v) for k, v in wall.items()}, "frames": a.session_frames - 2}), flush=True)


main()
