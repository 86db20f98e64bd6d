"""Models for adaptive sampling (docs/design/24-adaptive.md), none of which calls the library under test.

film_model: the film of a frame with a per-pixel sample count, built from the oracle's film pieces alone — per tile in k order orc_filmtile_new, orc_filmtile_add_sample
for the tile's sample pixels in Bounds2 order and the samples s < counts[p] in index order at px + orc_sampler_u(seed, px, py, s + offset, 0 / 1), orc_filmtile_merge, and the
merged tile added onto the film inside the tile's film bounds: integrators/sampler.jl:24-52 with samples_per_pixel replaced by counts[p].  The radiance of a sample comes in
from outside (the oracle's render, or a GPU frame whose samples were checked against it).

stats_model / map_model: trhip_last_sample_stats and trhip_sample_map operation by operation in Float32, written as plain loops over the 3 x 3 neighbourhood
(trace_jl_amd.api.sample_map_model is a second, vectorised copy that the package's tau_for_budget uses; the tests hold the kernel against both)."""
import ctypes as C

import numpy as np

import denoise_model as dm

F = np.float32


def sample_shape(cam):
    sb = cam.film.get_sample_bounds()
    return int(sb.p_max[1] - sb.p_min[1]) + 1, int(sb.p_max[0] - sb.p_min[0]) + 1, int(sb.p_min[0]), int(sb.p_min[1])


def film_model(ob, cam, L, counts, seed, sample_offset=0):
    """L: (max_spp, sb_h, sb_w, 3) radiance after the NaN rule; counts: (sb_h, sb_w).  Returns the film's (H, W, 4) xyz sums and weight sum."""
    lib = ob.lib()
    sn = ob.make_sensor(cam)
    sbh, sbw, x0, y0 = sample_shape(cam)
    counts = np.asarray(counts).reshape(sbh, sbw)
    h, w = cam.film.size
    cx0, cy0 = int(cam.film.crop_bounds.p_min[0]), int(cam.film.crop_bounds.p_min[1])
    film = np.zeros((h, w, 4), F)
    tiles_x, tiles_y = (sbw - 1 + 16) // 16, (sbh - 1 + 16) // 16
    for k in range(tiles_x * tiles_y):
        tx, ty = k % tiles_x, k // tiles_x
        bx0, by0 = x0 + 16 * tx, y0 + 16 * ty
        bx1, by1 = min(bx0 + 15, x0 + sbw - 1), min(by0 + 15, y0 + sbh - 1)
        tb = np.array([bx0, by0, bx1, by1], F)
        bounds, size = np.empty(4, F), np.empty(2, np.int32)
        t = lib.orc_filmtile_new(C.byref(sn), ob.fp(tb), ob.fp(bounds), size.ctypes.data_as(C.POINTER(C.c_int32)))
        for py in range(by0, by1 + 1):
            for px in range(bx0, bx1 + 1):
                for s in range(int(counts[py - y0, px - x0])):
                    fx = F(px) + F(lib.orc_sampler_u(seed, px, py, s + sample_offset, 0))
                    fy = F(py) + F(lib.orc_sampler_u(seed, px, py, s + sample_offset, 1))
                    rgb = np.ascontiguousarray(L[s, py - y0, px - x0], F)
                    lib.orc_filmtile_add_sample(t, float(fx), float(fy), ob.fp(rgb), 1.0)
        merged = np.empty((h, w, 4), F)
        lib.orc_filmtile_merge(t, ob.fp(merged))
        lib.orc_filmtile_free(t)
        ys, xs = slice(int(bounds[1]) - cy0, int(bounds[3]) - cy0 + 1), slice(int(bounds[0]) - cx0, int(bounds[2]) - cx0 + 1)
        if size[0] > 0 and size[1] > 0:
            film[ys, xs] = film[ys, xs] + merged[ys, xs]
    return film


def stats_model(L):
    """(spp, sb_h, sb_w, 3) radiance records (NaN lanes allowed) -> (sb_h, sb_w, 2): (m, v)."""
    L = np.asarray(L, F)
    n = F(L.shape[0])
    s1, s2 = np.zeros(L.shape[1:3], F), np.zeros(L.shape[1:3], F)
    with np.errstate(all="ignore"):
        for s in range(L.shape[0]):
            c = np.where(np.isnan(L[s]).any(axis=-1, keepdims=True), F(0), L[s]).astype(F)
            y = dm.to_Y(c)
            s1 = s1 + y
            s2 = s2 + y * y
        m = s1 / n
        x = s2 / n - m * m
        v = np.where(x < F(0), F(0), x)
    return np.stack([m, v], axis=-1).astype(F)


def map_model(mv, tau, eps, pilot, max_extra):
    """(sb_h, sb_w, 2) -> (counts (sb_h, sb_w) uint32, their sum)."""
    mv = np.asarray(mv, F)
    h, w = mv.shape[:2]
    tau, eps = F(tau), F(eps)
    counts = np.zeros((h, w), np.uint32)
    with np.errstate(all="ignore"):
        a = np.abs(mv[..., 0]) + eps
        e = mv[..., 1] / (a * a)
        e = np.where(np.isfinite(e), e, F(np.inf)).astype(F)
        tt = tau * tau
        for y in range(h):
            for x in range(w):
                E = F(0)
                for qy in range(max(y - 1, 0), min(y + 1, h - 1) + 1):
                    for qx in range(max(x - 1, 0), min(x + 1, w - 1) + 1):
                        if e[qy, qx] > E:
                            E = e[qy, qx]
                xs = F(E / tt)
                if xs < F(pilot + max_extra):
                    counts[y, x] = max(0, int(np.ceil(xs)) - pilot)
                else:
                    counts[y, x] = max_extra
    return counts, int(counts.sum(dtype=np.uint64))
