#!/usr/bin/env python
"""The reference's caustic video (docs/code/caustic_moving.jl): one BVHAccel, then one frame per light position, each frame rendered two ways —
a full commit of Scene(lights, bvh) per frame, and Scene.with_lights on one committed scene (trhip_scene_relight: the light stage alone).

    python tools/caustic_moving.py [--frames 5] [--res 1024] [--iterations 25] [--photons 1250000] [--depth 5] [--radius 0.055]
    python tools/caustic_moving.py --workload mesh_1m [--frames 5] [--res 1024] [--spp 16] [--depth 5]

caustic (default): caustic-glass.ply (tests/golden) under glass of index 1.2 on the plastic floor, the PointLight and the moving SpotLight of the script
(scenes.caustic_moving_lights), SPPMIntegrator(camera, 0.055, 5, 25, 1_250_000) at 1024^2 as the script renders it.  The two ways must agree: M, N, radius and Ld bit
for bit, phi and the image within the bounds of tests/test_gpu_sppm.py (the photon splats are atomic float sums).
mesh_1m: S-mesh (1 M triangles) lit by one PointLight that moves across the box, PathIntegrator: the two films bit for bit.

Per frame: the commit (or relight) time and the render time, host clocks around the library's calls, which synchronise their streams before they return.
Exits 1 when a frame disagrees.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PLY = os.path.join(ROOT, "tests", "golden", "caustic-glass.ply")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def caustic_frame(T, ctx, scene, cam, args):
    integ = T.SPPMIntegrator(cam, args.radius, args.depth, args.iterations, args.photons)
    t0 = time.perf_counter()
    film = integ.render(scene, ctx).copy()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, film, integ.state()


def caustic_agree(a, b):
    """(ok, note): b (relit) against a (full commit)."""
    (fa, sa), (fb, sb) = a, b
    bad = [k for k in ("M", "N", "radius", "Ld") if not same_bits(sa[k], sb[k])]
    scale = max(float(np.abs(sa["phi"]).max()), 1e-30)
    phi_ok = np.allclose(sb["phi"], sa["phi"], rtol=2e-5, atol=2e-5 * scale)
    img_ok = np.allclose(fb[..., :3], fa[..., :3], rtol=1e-4, atol=1e-4 * max(float(np.abs(fa[..., :3]).max()), 1e-30))
    ok = not bad and phi_ok and img_ok and sa["M"].sum() > 0
    note = "M N radius Ld bit-equal, phi and image within bounds" if ok else f"differ: {bad}{'' if phi_ok else ' phi'}{'' if img_ok else ' image'}"
    return ok, note


def path_frame(T, ctx, scene, cam, args):
    integ = T.PathIntegrator(cam, T.SeededSampler(args.spp, seed=7), args.depth)
    t0 = time.perf_counter()
    film = integ.render(scene, ctx).copy()
    return (time.perf_counter() - t0) * 1e3, film, None


def path_agree(a, b):
    ok = same_bits(a[0], b[0]) and np.isfinite(a[0]).all()
    return ok, "film bit-equal" if ok else f"film differs in {int((a[0].view(np.uint32) != b[0].view(np.uint32)).sum())} values"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["caustic", "mesh_1m"], default="caustic")
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--photons", type=int, default=1_250_000)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.055)
    ap.add_argument("--spp", type=int, default=16)
    args = ap.parse_args()
    import __graft_entry__ as g
    T = g.load_package()
    ctx = T.default_context()
    if args.workload == "caustic":
        base = T.scenes.caustic_scene(PLY, eta=1.2)
        cam = T.scenes.caustic_camera(args.res)
        shifts = [i / 10 for i in range(51)][:args.frames]  # 0:0.1:5
        frame_lights = [T.scenes.caustic_moving_lights(s) for s in shifts]
        render, agree = caustic_frame, caustic_agree
        what = (f"caustic_moving.jl: caustic-glass.ply, {args.res}^2, SPPM radius {args.radius}, depth {args.depth}, {args.iterations} iterations x {args.photons} photons")
    else:
        base = T.scenes.mesh_scene(T.scenes.MESH_N["mesh_1m"])
        cam = T.scenes.cornell_camera(args.res)
        xs = np.linspace(0.15, 0.85, max(args.frames, 2))[:args.frames]
        frame_lights = [[T.PointLight(T.translate([float(x), 0.9, -2.5]), T.RGBSpectrum(2.5))] for x in xs]
        render, agree = path_frame, path_agree
        what = f"S-mesh 1 M triangles, a PointLight moving along x, {args.res}^2, PathIntegrator {args.spp} spp, depth {args.depth}"
    base = T.Scene(frame_lights[0], base.aggregate)
    t0 = time.perf_counter()
    flat = base.flatten(ctx)
    base_ms = (time.perf_counter() - t0) * 1e3
    print(f"# {what}")
    print(f"# {flat.bvh()[3].size} primitives, bvh_mode {flat.bvh_mode()[0]}; base commit (once) {base_ms:.1f} ms, geometry {flat.geometry_id}")
    print(f"{'frame':>5} {'full commit ms':>15} {'render ms':>10} {'relight ms':>11} {'render ms':>10}  agreement")
    full_c, full_r, rel_c, rel_r, all_ok = [], [], [], [], True
    for i, lights in enumerate(frame_lights):
        full = T.Scene(lights, base.aggregate)
        t0 = time.perf_counter()
        ff = full.flatten(ctx)
        fc = (time.perf_counter() - t0) * 1e3
        fr, film_a, st_a = render(T, ctx, full, cam, args)
        ff.free()
        relit = base.with_lights(lights)
        t0 = time.perf_counter()
        fv = relit.flatten(ctx)
        rc = (time.perf_counter() - t0) * 1e3
        rr, film_b, st_b = render(T, ctx, relit, cam, args)
        assert fv.geometry_id == flat.geometry_id
        fv.free()
        ok, note = agree((film_a, st_a), (film_b, st_b))
        all_ok = all_ok and ok
        full_c.append(fc), full_r.append(fr), rel_c.append(rc), rel_r.append(rr)
        print(f"{i + 1:>5} {fc:>15.1f} {fr:>10.1f} {rc:>11.2f} {rr:>10.1f}  {note}", flush=True)
    fc, fr, rc, rr = (float(np.median(v)) for v in (full_c, full_r, rel_c, rel_r))
    print(f"# median per frame: full commit {fc:.1f} ms + render {fr:.1f} ms = {fc + fr:.1f} ms; relight {rc:.2f} ms + render {rr:.1f} ms = {rc + rr:.1f} ms "
          f"({(fc + fr) / (rc + rr):.2f}x); commit share of a full-commit frame {fc / (fc + fr) * 100:.1f} %")
    print(f"# {'all frames agree' if all_ok else 'SOME FRAMES DISAGREE'}")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
