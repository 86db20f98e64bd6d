#!/usr/bin/env python
"""The edge-avoiding denoiser on a low-spp frame of the 1 M-triangle mesh scene: python tools/denoise_probe.py [--spp 8] [--res 1024] [--depth 8] [--runs 30] [--warmup 5] [--png PREFIX]

Renders the path frame and the feature planes on the device (same sampler settings), denoises there, and prints JSON lines: the median device time of the three calls, and
per à-trous iteration the kernel time of BOTH kernels (gathered from memory / staged in LDS where that kernel exists) with the effective bytes per second against the compulsory
64 bytes per pixel and iteration (read {n, flag}, {p}, {c, Y}; write {c, Y}).  The time of iteration i is the iterations' kernel time (trhip_stats.ms_sub[1]) of a call with
i + 1 iterations minus that of a call with i, medians over the runs.  --png writes PREFIX_noisy.png and PREFIX_denoised.png."""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as g
T = g.load_package()
ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=8)
ap.add_argument("--res", type=int, default=1024)
ap.add_argument("--depth", type=int, default=8)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--scene", default="mesh_1m", choices=sorted(T.scenes.MESH_N))
ap.add_argument("--png", default="")
a = ap.parse_args()
scene, cam = T.scenes.mesh_scene(T.scenes.MESH_N[a.scene]), T.scenes.cornell_camera(a.res)
flat = scene.flatten()
ctx, L, sn, seed = flat.ctx, T.lib(), cam.sensor(), 0x5EED0001
h, w = cam.film.size
d_film, d_planes, d_out = T._ffi.DeviceBuffer(h * w * 16), T._ffi.DeviceBuffer(h * w * 48), T._ffi.DeviceBuffer(h * w * 16)
ptr = lambda b: C.c_void_p(b.ptr)  # noqa: E731
den = T.Denoiser()


def median_of(call, key=lambda st: st.ms_total):
    ms = []
    for i in range(a.warmup + a.runs):
        st = T.Stats()
        call(st)
        if i >= a.warmup:
            ms.append(key(st))
    return float(np.median(ms))


def denoise(st, iterations=None):
    p = T._ffi.DenoiseParams.from_buffer_copy(den.params)
    if iterations is not None:
        p.iterations = iterations
    ctx.check(L.trhip_denoise_device(ctx._h, ptr(d_film), ptr(d_planes), w, h, C.byref(p), ptr(d_out), C.byref(st)))


ms_path = median_of(lambda st: ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), a.spp, a.depth, seed, 0, ptr(d_film), C.byref(st))))
ms_aov = median_of(lambda st: ctx.check(L.trhip_render_aov_device(ctx._h, flat._h, C.byref(sn), a.spp, seed, 0, ptr(d_planes), None, C.byref(st))))
ms_denoise = median_of(denoise)
ms_kernels = median_of(denoise, key=lambda st: st.ms_film)
print(json.dumps({"scene": a.scene, "res": a.res, "spp": a.spp, "depth": a.depth, "runs": a.runs, "iterations": den.params.iterations, "ms_path": round(ms_path, 3), "ms_aov": round(ms_aov, 3),
                  "ms_denoise": round(ms_denoise, 4), "ms_denoise_kernels": round(ms_kernels, 4)}), flush=True)
for name, mask in (("gather", 0), ("lds", 3)):
    ctx.set_option("denoise_lds", mask)
    cum = [0.0] + [median_of(lambda st, k=k: denoise(st, k), key=lambda st: st.ms_sub[1]) for k in range(1, 7)]
    edges = median_of(lambda st: denoise(st, 1), key=lambda st: st.ms_sub[0] + st.ms_sub[2])
    for i in range(6):
        if name == "lds" and i >= 2:
            break  # (the staged kernel exists for steps 1 and 2: from step 4 on the gather runs whatever the option says)
        ms = cum[i + 1] - cum[i]
        print(json.dumps({"kernel": name, "iteration": i, "step": 1 << i, "ms": round(ms, 4), "TB_per_s_of_64B_per_pixel": round(64.0 * h * w / (ms * 1e-3) * 1e-12, 3) if ms > 0 else None}), flush=True)
    print(json.dumps({"kernel": name, "prepare_plus_finish_ms": round(edges, 4)}), flush=True)
ctx.set_option("denoise_lds", 3)
if a.png:
    for suffix, buf in (("noisy", d_film), ("denoised", d_out)):
        denoise(T.Stats())
        cam.film.filename = f"{a.png}_{suffix}.png"
        cam.film.set_xyzw(buf.to_host(np.float32, (h, w, 4)))
        print(json.dumps({"png": T.save(cam.film, ctx)}), flush=True)
