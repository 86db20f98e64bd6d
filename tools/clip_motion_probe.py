#!/usr/bin/env python
"""Clipped reprojection under motion: python tools/clip_motion_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 200] [--warmup 20] [--repeats 3]
[--skip-timing] [--skip-sweep] [--skip-relight]

1. Times on the 1 M-triangle mesh scene, two frames through cameras 0.75 degrees apart, the second accumulated against the first one's history, the height field one moving
   body (tools/motion_probe.py's frame): k_temporal_clip_motion<R> alternating with k_temporal_clip<R> (R = 1, 2, 3) and k_temporal_motion in one process, `--repeats` times
   over.  Device events around the launch (trhip_stats.ms_film), quartiles over the runs; the ratio to k_temporal_clip<R> beside the one predicted from the compulsory bytes
   per pixel (192 against 176).  Then the session's frame: PreviewSession.render with motion={the height field} through the carry_bodies accumulator against baseline (i),
   the plain accumulator, host clock around the call, alternating sessions.
2. The sweep of tests/test_gpu_clip_motion.py's quality figures: gamma {1, 2, 4, inf} x R {1, 2, 3} x clip_max_history {0, 1, 2, 4, inf}, both sequences, every mask, the
   ratios to baselines (i) and (ii), (iii) beside them; and the cell the rule picks: among the cells with finite gamma the lowest geometric mean over the two sequences of the
   whole-frame ratio to (i), ties to the larger clip_max_history.
3. The relight series of tools/temporal_clip_probe.py (Cornell, static camera, 48 x 48, 4 spp; four frames, every light x 0.25 without reset(), two more) through the new
   entry point with no bodies, per clip_max_history.
Prints JSON lines."""
import argparse, copy, ctypes as C, json, os, sys, time
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
ap.add_argument("--skip-session", action="store_true")
ap.add_argument("--skip-sweep", action="store_true")
ap.add_argument("--skip-relight", action="store_true")
a = ap.parse_args()
INF = float("inf")
GAMMAS, RADII, CUTS = (1.0, 2.0, 4.0, INF), (1, 2, 3), (0.0, 1.0, 2.0, 4.0, INF)


def jf(v):
    return "inf" if v == INF else v


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
    mprm = acc._motion_params_for(cams[0], table.size, 1)
    clip = {R: T.TemporalAccumulator(clip_gamma=1.0, clip_radius=R)._clip_params_for(cams[0]) for R in RADII}
    both = {R: T.TemporalAccumulator(clip_gamma=1.0, clip_radius=R, carry_bodies=True, clip_max_history=2.0)._clip_motion_params_for(cams[0], table.size, 1) for R in RADII}

    def motion(st):
        ctx.check(L.trhip_temporal_motion_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), ptr(d_ids), ptr(d_table), ptr(d_mats), w, h, C.byref(mprm), ptr(d_out), ptr(d_hist1),
                                                 C.byref(st)))

    def clipped(R):
        return lambda st: ctx.check(L.trhip_temporal_clip_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), w, h, C.byref(clip[R]), ptr(d_out), ptr(d_hist1), C.byref(st)))

    def clip_motion(R):
        return lambda st: ctx.check(L.trhip_temporal_clip_motion_device(ctx._h, ptr(d_film), ptr(d_planes), ptr(d_hist0), ptr(d_ids), ptr(d_table), ptr(d_mats), w, h, C.byref(both[R]),
                                                                        ptr(d_out), ptr(d_hist1), C.byref(st)))

    def series(call):
        out = []
        for i in range(a.warmup + a.runs):
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                out.append(st.ms_film)
        return quartiles(out)

    clip_motion(3)(T.Stats())
    hist = d_hist1.to_host(np.float32, (h, w, 3, 4))
    motion(T.Stats())
    plain = d_hist1.to_host(np.float32, (h, w, 3, 4))
    ids = d_ids.to_host(T._ffi.AOV_ID_DTYPE, (h, w))
    moving = (ids["prim"] >= 0) & (table[np.where(ids["prim"] >= 0, ids["prim"], 0)] == 0)
    print(json.dumps({"library": os.path.basename(T._ffi.LIB_PATH), "scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "pixels": npix,
                      "surface_pixels": int((plain[..., 0, 3] > 0).sum()), "pixels_with_history": int((plain[..., 0, 3] > 1).sum()), "pixels_on_the_moving_body": int(moving.sum()),
                      "pixels_changed_by_clipping_gamma1_R3_cut2": int((hist[..., 0, :] != plain[..., 0, :]).any(-1).sum()), "n_prims": int(table.size)}), flush=True)
    medians = {}
    for rep in range(a.repeats):
        calls = [("k_temporal_motion", motion)]
        for R in RADII:
            calls += [(f"k_temporal_clip<{R}>", clipped(R)), (f"k_temporal_clip_motion<{R}>", clip_motion(R))]
        for name, call in calls:
            q = series(call)
            medians.setdefault(name, []).append(q[1])
            print(json.dumps({"repeat": rep, "kernel": name, "ms_q25_median_q75": q}), flush=True)
    med = {k: float(np.median(v)) for k, v in medians.items()}
    for R in RADII:
        print(json.dumps({"R": R, "k_temporal_clip_motion_ms": round(med[f"k_temporal_clip_motion<{R}>"], 5), "k_temporal_clip_ms": round(med[f"k_temporal_clip<{R}>"], 5),
                          "ratio_over_k_temporal_clip": round(med[f"k_temporal_clip_motion<{R}>"] / med[f"k_temporal_clip<{R}>"], 4), "predicted_from_compulsory_bytes_at_most": round(192.0 / 176.0, 4),
                          "ratio_over_k_temporal_motion": round(med[f"k_temporal_clip_motion<{R}>"] / med["k_temporal_motion"], 4)}), flush=True)
    if a.skip_session:
        return
    motion_dict = {mesh_entry: T.translate([0.002, 0.0, -0.001])}
    sessions = {"(i) plain accumulator, motion={height field}": T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth),
                "carry_bodies accumulator (defaults), motion={height field}": T.PreviewSession(scene, T.SeededSampler(a.spp, seed=seed), a.depth,
                                                                                                  temporal=T.TemporalAccumulator(clip_gamma=4.0, carry_bodies=True))}
    wall = {k: [] for k in sessions}
    for k in range(a.session_frames):
        cam = ms.camera(T, a.res, 0.75 * k)
        for name, session in sessions.items():
            t0 = time.perf_counter()
            session.render(cam, ctx, motion=motion_dict)
            if k >= 2:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    for session in sessions.values():
        session.close()
    print(json.dumps({"session_frame_ms_q25_median_q75": {k: quartiles(v) for k, v in wall.items()}, "frames": a.session_frames - 2}), flush=True)


def sweep():
    import test_gpu_clip_motion as tg
    ctx = T.default_context()
    whole = {}
    for which in sorted(tg.QUALITY_CAMERAS):
        case = tg.QualityCase(T, ctx, which)
        print(json.dumps({"sequence": which, **{k: jf(v) for k, v in tg.QUALITY.items()}, "pixels": {k: int(m.sum()) for k, m in case.masks.items()}}), flush=True)
        plain = case.baselines(4.0, 3)
        print(json.dumps({"sequence": which, "mse_baseline_i": plain["i"], "mse_baseline_iii": plain["iii"]}), flush=True)
        for R in RADII:
            for gamma in GAMMAS:
                ii = case.mse(case.last_frame(T.TemporalAccumulator(max_history=tg.QUALITY["max_history"], clip_gamma=gamma, clip_radius=R), False))
                print(json.dumps({"sequence": which, "gamma": jf(gamma), "R": R, "mse_baseline_ii": {k: round(v, 7) for k, v in ii.items()}}), flush=True)
                for cut in CUTS:
                    new = case.cell(gamma, R, cut)
                    row = {"sequence": which, "gamma": jf(gamma), "R": R, "clip_max_history": jf(cut)}
                    for m in tg.MASKS:
                        row[f"{m}_over_i"], row[f"{m}_over_ii"], row[f"{m}_over_iii"] = (round(new[m] / b[m], 4) for b in (plain["i"], ii, plain["iii"]))
                    if gamma == INF:
                        row["repeats_baseline_i_digit_for_digit"] = bool(new == plain["i"])
                    row["mse"] = {k: round(v, 7) for k, v in new.items()}
                    whole.setdefault((gamma, R, cut), []).append(new["frame"] / plain["i"]["frame"])
                    print(json.dumps(row), flush=True)
    best = None
    for (gamma, R, cut), v in sorted(whole.items()):
        gmean = float(np.exp(np.mean(np.log(v))))
        print(json.dumps({"gamma": jf(gamma), "R": R, "clip_max_history": jf(cut), "geometric_mean_of_the_whole_frame_ratio_to_i": round(gmean, 4)}), flush=True)
        if gamma != INF and (best is None or gmean < best[0] or (gmean == best[0] and cut > best[3])):
            best = (gmean, gamma, R, cut)
    print(json.dumps({"cell_the_rule_picks": {"gamma": jf(best[1]), "R": best[2], "clip_max_history": jf(best[3]), "geometric_mean": round(best[0], 4)}}), flush=True)
    at_default = {cut: float(np.exp(np.mean(np.log(whole[(4.0, 3, cut)])))) for cut in CUTS}
    pick = max((c for c in CUTS if at_default[c] == min(at_default.values())))
    print(json.dumps({"clip_max_history_the_rule_picks_at_gamma_4_R_3": jf(pick), "geometric_means": {str(jf(c)): round(v, 4) for c, v in at_default.items()}}), flush=True)


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
    cam = ms.camera(T, res, 0.0)
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
                      "surface_pixels": int(surface.sum())}), flush=True)
    for gamma, R in ((None, 0), (4.0, 3), (1.0, 1)):
        for cut in ((None,) if gamma is None else (None,) + CUTS):
            if gamma is None:
                temporal = T.TemporalAccumulator(max_history=8)
            elif cut is None:
                temporal = T.TemporalAccumulator(max_history=8, clip_gamma=gamma, clip_radius=R)
            else:
                temporal = T.TemporalAccumulator(max_history=8, clip_gamma=gamma, clip_radius=R, carry_bodies=True, clip_max_history=cut)
            session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=temporal)
            series = []
            for k in range(before + after):
                if k == before:
                    session.scene = dim
                series.append(mse(session.render(cam, ctx), targets[k >= before]))
            session.close()
            entry = "trhip_temporal" if gamma is None else ("trhip_temporal_clip" if cut is None else "trhip_temporal_clip_motion, no bodies")
            print(json.dumps({"relight_entry": entry, "gamma": "unclipped" if gamma is None else gamma, "R": R, "clip_max_history": None if cut is None else jf(cut),
                              "mse_per_frame": [round(v, 6) for v in series]}), flush=True)


if not a.skip_timing:
    timing()
if not a.skip_sweep:
    sweep()
if not a.skip_relight:
    relight()
