#!/usr/bin/env python
"""Soak test of the film pass (add_sample! + merge_film_tile!, film.jl:134-193) on the GPU against the oracle: random film sizes (not
multiples of the 16-pixel tiles), crop windows, anisotropic Lanczos filters with radii on both sides of 1 (0.3-1: the packed pass, up to 3.5: the wide
one), 1-5 spp, and the three ways records reach the packed gather: fused by k_raygen (the default, in a frame), re-laid (film_fused 0, or a caller's
records) and in place (film_relayout 0).  The oracle renders the shadows scene and keeps its per-sample radiance; trhip_film_accumulate must turn those
samples — some of them poisoned with NaNs — into the oracle's film bit for bit, and a path frame must give the oracle's film.
Run on a GPU: python tools/soak_film.py --cases 60"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft

graft.build_library()
graft.build_oracle()
T = graft.load_package()
import oracle_bridge as ob
import sample_map_model as sm

VARIANTS = (("default", {}), ("relayout0", {"film_relayout": 0}), ("fused0", {"film_fused": 0}))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and not ((a.view(np.uint32) != b.view(np.uint32)) & ~na).any()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=30)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    ctx = T.default_context()
    scene = T.scenes.shadows_scene()
    osc = ob.OracleScene.from_scene(scene, bvh=scene.flatten(ctx).bvh())  # (the frames walk the library's tree)
    bad = 0
    for k in range(a.cases):
        rng = np.random.default_rng(a.seed * 1000 + k)
        res = [int(rng.integers(9, 90)), int(rng.integers(9, 90))]
        lo = rng.uniform(0.0, 0.4, 2) if k % 3 == 1 else np.zeros(2)
        hi = rng.uniform(0.6, 1.0, 2) if k % 3 == 1 else np.ones(2)
        rmax = 1.0 if k % 2 == 0 else 3.5  # half of the cases inside the packed descriptor's range (radius <= 1: the default path), half beyond it
        flt = T.LanczosSincFilter([float(rng.uniform(0.3, rmax)), float(rng.uniform(0.3, rmax))], float(rng.uniform(1.0, 4.0)))
        film = T.Film(res, T.Bounds2([float(lo[0]), float(lo[1])], [float(hi[0]), float(hi[1])]), flt, 1.0, float(rng.uniform(0.5, 2.0)), "")
        cam = T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)
        spp = int(rng.integers(1, 6))
        seed = 900 + k
        ref_xyzw, ref_L, _ = osc.render(cam, "path", spp, 3, seed=seed, want_samples=True)
        frame_xyzw = ref_xyzw  # what a path frame of the same scene must give
        if k % 4 == 0:  # NaN samples are zeroed (integrators/sampler.jl:46): poison a few, and take the film the oracle's film-tile calls make of the records after the rule
            idx = rng.integers(0, ref_L.size // 3, 5)
            ref_L.reshape(-1, 3)[idx, int(rng.integers(0, 3))] = np.nan
            ruled = ref_L.reshape(-1, 3).copy()
            ruled[np.isnan(ruled).any(axis=1)] = 0.0
            sbh, sbw, _, _ = sm.sample_shape(cam)
            ref_xyzw = sm.film_model(ob, cam, ruled.reshape(spp, sbh, sbw, 3), np.full((sbh, sbw), spp), seed)
        sn = cam.sensor()
        msgs = []
        for name, opts in VARIANTS:
            for o, v in opts.items():
                ctx.set_option(o, v)
            try:
                out = np.empty((cam.film.size[0], cam.film.size[1], 4), np.float32)
                ctx.check(T.lib().trhip_film_accumulate(ctx._h, C.byref(sn), spp, seed, 0, T._ffi.fptr(ref_L), T._ffi.fptr(out)))
                frame = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed), 3).render(scene, ctx)  # (film_fused only shows in a frame: k_raygen writes its records)
            finally:
                for o in opts:
                    ctx.set_option(o, 1)
            if not same_bits(out, ref_xyzw):
                msgs.append(name + " (accumulate)")
            if not same_bits(frame, frame_xyzw):
                msgs.append(name + " (frame)")
        bad += 1 if msgs else 0
        print(f"case {k:3d}: film {res[0]} x {res[1]}, crop {'yes' if k % 3 == 1 else 'no '}, radius ({flt.radius[0]:.2f}, {flt.radius[1]:.2f}), {spp} spp"
              f"{', NaN samples' if k % 4 == 0 else ''}: {'equal' if not msgs else 'MISMATCH ' + ', '.join(msgs)}", flush=True)
    print(f"total: {a.cases} cases x {len(VARIANTS)} record paths x (accumulate, frame), {bad} with a mismatch")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
