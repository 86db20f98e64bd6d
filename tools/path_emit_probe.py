#!/usr/bin/env python
"""The emit frame beside the path frame: python tools/path_emit_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 20] [--warmup 5] [--strip 4] [--hits-only] [--existing]
| --quality

Time (the default): trhip_render_path_emit_device and trhip_render_path_device of the same build on the 1 M-triangle mesh scene under a strip light of 2 * strip^2 emissive
triangles (heightfield_mesh(strip), narrowed and lifted under the ceiling, with a material of its own), same sensor, spp, depth and seed, film left in HBM.  The two
candidates ALTERNATE in one process — emit, path, emit, path, … — so that clocks, caches and whatever else drifts during the run drift under both.  Prints one JSON line per
candidate (median / min / max / quartiles of the device time over the runs; the stage times, ray counts and launch counts of the median run: k_path_emit is timed with the
shade stage, the emitter rays with the any-hit stage, the fold with the film stage), one line with the differences of the stage medians, and the emit frame's counted hits.
--existing: trhip_render_path_device alone, twice per round — the yardstick run, which a build without the feature can make too (the scene then has the strip as plain geometry).

Quality (--quality): at 64 x 64 on the Cornell box without lights under a ceiling quad and on mesh_scene(16) under the 32-triangle strip, depth 8: the MSE of the linear RGB
film of NEE frames and of HITS_ONLY frames (depth 8) at 4 and 16 spp over 8 seeds against the mean of two 4096-spp references — a NEE frame at depth 8 and a HITS_ONLY frame
at depth 9 — with the frames' device times, so that the ratio can be read at equal spp and at equal time; the references' own disagreement, mean (A - B)^2 / 4, bounds the
noise (and the depth-cut term) in that mean."""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
import numpy as np
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--strip", type=int, default=4, help="the strip light is heightfield_mesh(strip): 2 * strip^2 emissive triangles")
ap.add_argument("--le", type=float, default=20.0, help="radiance of the emitters")
ap.add_argument("--hits-only", action="store_true", help="time the frame under TRHIP_PATH_EMIT_HITS_ONLY")
ap.add_argument("--existing", action="store_true", help="trhip_render_path alone: the yardstick run of a build with or without the feature")
ap.add_argument("--quality", action="store_true")
ap.add_argument("--ref-spp", type=int, default=4096)
a = ap.parse_args()
SEED = 0x5EED0001
L = T.lib()
F = np.float32


def lamp_material():
    return T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0))


def strip_prims(n, material):
    verts, idx, nrm = T.scenes.heightfield_mesh(n)
    v = np.array(verts, F)
    v[:, 0] = F(0.35) + F(0.3) * v[:, 0]
    v[:, 1] = v[:, 1] + F(0.8)
    return [T.create_mesh_primitives(T.ShapeCore(T.translate([0, 0, 0]), False), idx, v, nrm, material)]


def quad_prims(material):
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    v = F([[0.35, 0.999, -2.35], [0.35, 0.999, -2.65], [0.65, 0.999, -2.65], [0.65, 0.999, -2.35]])
    return [T.GeometricPrimitive(t, material) for t in T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, v, F([[0, -1, 0]] * 4))]


def with_prims(scene, extra, lights=None):
    return T.Scene(scene.lights if lights is None else lights, T.BVHAccel(list(scene.aggregate.primitives) + extra, 1))


STAGES = ("ms_raygen", "ms_trace_closest", "ms_fallback", "ms_shade", "ms_trace_any", "ms_film")
KEEP = ("camera_samples", "closest_rays", "shadow_rays", "fallback_rays", "traversal", "n_batches") + STAGES + ("launches_raygen", "launches_trace_closest", "launches_shade", "launches_trace_any",
                                                                                                                "launches_film")


def timing():
    lamp = lamp_material()
    scene, cam = with_prims(T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), strip_prims(a.strip, lamp)), T.scenes.cornell_camera(a.res)
    flat = scene.flatten()
    ctx, sn = flat.ctx, cam.sensor()
    ctx.set_option("streaming", 0)
    h, w = cam.film.size
    d_film = T._ffi.DeviceBuffer(h * w * 4 * 4)
    out = C.c_void_p(d_film.ptr)

    def path(st):
        ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, SEED, 0, out, C.byref(st)))

    if a.existing:
        cands = [("path_a", path), ("path_b", path)]
    else:
        em = T.Emitters(scene, {lamp: T.RGBSpectrum(a.le)})
        pe = T._ffi.default_params(T._ffi.PathEmitParams, "trhip_path_emit_default_params")
        pe.flags = T._ffi.PATH_EMIT_HITS_ONLY if a.hits_only else 0

        def path_emit(st):
            ctx.check(L.trhip_render_path_emit_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, SEED, 0, em._h, C.byref(pe), out, C.byref(st)))

        cands = [("emit", path_emit), ("path", path)]
    runs = {name: [] for name, _ in cands}
    for i in range(a.warmup + a.runs):
        for name, call in cands:
            st = T.Stats()
            call(st)
            if i >= a.warmup:
                runs[name].append(st.as_dict())
    median = lambda xs: sorted(xs)[len(xs) // 2]
    summary = {}
    for name, _ in cands:
        rs = sorted(runs[name], key=lambda r: r["ms_total"])
        ms = [r["ms_total"] for r in rs]
        med = rs[len(rs) // 2]
        summary[name] = {"ms_total": ms[len(ms) // 2], **{k: median([r[k] for r in rs]) for k in STAGES}}
        print(json.dumps({"frame": name, "scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "emissive_triangles": 2 * a.strip * a.strip,
                          "hits_only": bool(a.hits_only) if name == "emit" else None, "runs": a.runs, "warmup": a.warmup, "alternating": True, "ms_median": round(ms[len(ms) // 2], 3),
                          "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3), "ms_p25": round(ms[len(ms) // 4], 3), "ms_p75": round(ms[(3 * len(ms)) // 4], 3),
                          "median_run": {k: (round(med[k], 3) if isinstance(med[k], float) else med[k]) for k in KEEP}}), flush=True)
    (x, _), (y, _) = cands
    print(json.dumps({f"{x}_minus_{y}_ms (medians of each stage over the runs)": {k: round(summary[x][k] - summary[y][k], 3) for k in ("ms_total",) + STAGES}}), flush=True)
    if not a.existing:
        st = T.Stats()
        path_emit(st)
        rec = np.empty((int(st.camera_samples), 4), np.float32)
        ctx.check(L.trhip_last_emitted(ctx._h, T._ffi.fptr(rec), rec.size))
        print(json.dumps({"camera_samples": int(rec.shape[0]), "samples_with_a_counted_hit": int((rec[:, 3] > 0).sum()), "counted_hits": int(rec[:, 3].sum()),
                          "n_triangles": em.n_triangles}), flush=True)
        em.close()


XYZ_TO_RGB = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])


def rgb(xyzw):
    """Linear RGB of a film, unclamped: XYZ over the filter weights (spectrum.jl:16-22's matrix)."""
    x = xyzw[..., :3].astype(np.float64) / np.where(xyzw[..., 3:] != 0, xyzw[..., 3:], 1.0)
    return x @ XYZ_TO_RGB.T


def quality():
    lamp = lamp_material()
    scenes = {"cornell_unlit_quad": T.Scene([], T.BVHAccel(T.scenes.cornell_primitives()[0] + quad_prims(lamp), 1)),
              "mesh_16_strip": with_prims(T.scenes.mesh_scene(16), strip_prims(4, lamp))}
    print(json.dumps({"quality": True, "res": 64, "depth": 8, "le": a.le, "ref_spp": a.ref_spp, "seeds": 8, "note": "one radiance, one session"}), flush=True)
    for name, scene in scenes.items():
        cam = T.scenes.cornell_camera(64)
        em = T.Emitters(scene, {lamp: T.RGBSpectrum(a.le)})

        def frame(nee, spp, depth, seed):
            integ = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed), depth)
            film = integ.render(scene, emitters=em, emit_hits_only=not nee).copy()
            return rgb(film), integ.stats.ms_total

        ref_a, _ = frame(True, a.ref_spp, 8, 0xA11CE)
        ref_b, _ = frame(False, a.ref_spp, 9, 0xB0B)
        ref = 0.5 * (ref_a + ref_b)
        disagreement = float(((ref_a - ref_b) ** 2).mean() / 4.0)
        print(json.dumps({"scene": name, "reference": "mean of NEE depth 8 and HITS_ONLY depth 9", "mean (A - B)^2 / 4": disagreement, "mean of the reference": float(ref.mean()),
                          "mean A": float(ref_a.mean()), "mean B": float(ref_b.mean())}), flush=True)
        for spp in (4, 16):
            row = {}
            for nee in (True, False):
                frame(nee, spp, 8, 1)  # warm
                mses, times = [], []
                for seed in range(1, 9):
                    f, ms = frame(nee, spp, 8, seed)
                    mses.append(float(((f - ref) ** 2).mean()))
                    times.append(ms)
                row["nee" if nee else "hits_only"] = {"mse_mean": float(np.mean(mses)), "mse_min": min(mses), "mse_max": max(mses), "ms_median": sorted(times)[4]}
            n, e = row["nee"], row["hits_only"]
            row.update(scene=name, spp=spp, mse_ratio_equal_spp=n["mse_mean"] / e["mse_mean"],
                       mse_ratio_equal_time=(n["mse_mean"] * n["ms_median"]) / (e["mse_mean"] * e["ms_median"]),  # MSE falls as 1 / spp, and time grows with spp
                       reference_share_of_nee_mse=disagreement / n["mse_mean"], reference_share_of_hits_only_mse=disagreement / e["mse_mean"])
            print(json.dumps(row), flush=True)
        em.close()


quality() if a.quality else timing()
