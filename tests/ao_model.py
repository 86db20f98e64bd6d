"""The ambient-occlusion integrator (trhip_render_ao, docs/design/13-ao.md) restated from what already exists: the Python sampler arithmetic for the camera samples and u, the
oracle's camera rays, closest hits with their geometry and any-hit verdicts, the library's host detmath entry point (no GPU) for sin / cos, and numpy Float32 for the rest — one
Float32 operation per step, in the kernel's order.  The GPU tests compare per-sample radiance with this model bit for bit."""
import sys

import numpy as np

import oracle_bridge as ob

F = np.float32
PI = F(np.pi)
MISS, OCCLUDED, OPEN = 0, 1, 2
TS_V_BSDF_U0, TS_V_BSDF_U1 = 5 + 5, 5 + 6  # ts_vertex_dim(0, TS_V_BSDF_U0 / U1), include/trace_sampler.h


def _T():
    return sys.modules["trace_jl_amd"]


def sample_keys(cam, spp, seed, sample_offset=0):
    """Stream keys of every camera sample, sample-major over the sample bounds (k_raygen's order)."""
    S = _T().scenes
    sb = cam.film.get_sample_bounds()
    X, Y = np.meshgrid(np.arange(int(sb.p_min[0]), int(sb.p_max[0]) + 1), np.arange(int(sb.p_min[1]), int(sb.p_max[1]) + 1), indexing="xy")
    return np.concatenate([S.ts_stream_key(seed, X.ravel(), Y.ravel(), sample_offset + s) for s in range(spp)]), np.tile(X.ravel(), spp), np.tile(Y.ravel(), spp)


def camera_samples(cam, spp, seed, sample_offset=0):
    """(film.x, film.y, lens.x, lens.y, time) per camera sample and the samples' stream keys."""
    S = _T().scenes
    key, X, Y = sample_keys(cam, spp, seed, sample_offset)
    c = np.stack([X.astype(F) + S.ts_uniform(key, 0), Y.astype(F) + S.ts_uniform(key, 1), S.ts_uniform(key, 2), S.ts_uniform(key, 3), S.ts_uniform(key, 4)], axis=1).astype(F)
    return c, key


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cosine_sample_hemisphere(u):
    """Trace.jl:48-73 as th_math.h evaluates it: concentric disk (sin / cos from trace_detmath.h's tm_sincosf), z = sqrt(max(0, 1 - x x - y y))."""
    detmath = _T()._ffi.detmath
    u = np.asarray(u, F)
    ox, oy = F(2.0) * u[:, 0] - F(1.0), F(2.0) * u[:, 1] - F(1.0)
    first = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        th_a = ((oy / ox) * PI) / F(4.0)
        th_b = PI / F(2.0) - ((ox / oy) * PI) / F(4.0)
    r = np.where(first, ox, oy)
    th = np.where(first, th_a, th_b).astype(F)
    zero = (ox == 0) & (oy == 0)
    th[zero] = 0
    sn, cs = detmath(6, th), detmath(7, th)
    dx, dy = np.where(zero, F(0.0), r * cs).astype(F), np.where(zero, F(0.0), r * sn).astype(F)
    z2 = (F(1.0) - dx * dx) - dy * dy
    return np.stack([dx, dy, np.sqrt(np.where(z2 > 0, z2, F(0.0)).astype(F))], axis=1).astype(F)


def coordinate_system(v1):
    """Trace.jl:139-146."""
    x, y, z = v1[:, 0], v1[:, 1], v1[:, 2]
    first = np.abs(x) > np.abs(y)
    zero = np.zeros_like(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.stack([-z, zero, x], axis=1) / np.sqrt(x * x + z * z)[:, None]
        b = np.stack([zero, z, -y], axis=1) / np.sqrt(y * y + z * z)[:, None]
    v2 = np.where(first[:, None], a, b).astype(F)
    v3 = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2], v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], axis=1).astype(F)
    return v2, v3


def directions(ns, wo, u):
    """(nf, wi): the face-forwarded shading normal and the occlusion ray's direction for shading normals ns, outgoing directions wo and sample points u."""
    ns, wo = np.asarray(ns, F), np.asarray(wo, F)
    nf = np.where((dot3(ns, wo) < 0)[:, None], -ns, ns).astype(F)
    s, t = coordinate_system(nf)
    wl = cosine_sample_hemisphere(u)
    wi = (s * wl[:, 0:1] + t * wl[:, 1:2]) + nf * wl[:, 2:3]
    return nf, wi.astype(F)


class Result(dict):
    __getattr__ = dict.__getitem__


def render(osc, cam, spp, seed, sample_offset=0, max_distance=np.inf, background=0.0, albedo=None):
    """Per-sample L (spp, sb_h, sb_w, 3) and class (MISS / OCCLUDED / OPEN) of an AO frame.  osc: the OracleScene (on the tree the frame walks); albedo: None, or the per-sample
    base colour (n, 3) that TRHIP_AO_ALBEDO multiplies the visibility with."""
    S = _T().scenes
    samples, key = camera_samples(cam, spp, seed, sample_offset)
    rays = ob.generate_rays(cam, samples)
    _, prim, geom, _ = osc.trace_closest(rays, want_geom=True)
    hit = prim >= 0
    n = rays.shape[0]
    cls = np.full(n, MISS, np.int32)
    L = np.full((n, 3), F(background), F)
    idx = np.flatnonzero(hit)
    wi = np.zeros((n, 3), F)
    nf = np.zeros((n, 3), F)
    orays = np.zeros((idx.size, 8), F)
    if idx.size:
        p, ns = geom[idx, 0:3], geom[idx, 6:9]
        u = np.stack([S.ts_uniform(key[idx], TS_V_BSDF_U0), S.ts_uniform(key[idx], TS_V_BSDF_U1)], axis=1)
        nf[idx], wi[idx] = directions(ns, -rays[idx, 4:7], u)
        orays[:, 0:3] = p + F(1e-6) * wi[idx]  # spawn_ray(si, wi), Trace.jl:206-211
        orays[:, 3] = F(max_distance)
        orays[:, 4:7] = wi[idx]
        orays[:, 7] = rays[idx, 7]
        occ, _ = osc.trace_any(orays)
        cls[idx] = np.where(occ != 0, OCCLUDED, OPEN)
        v = np.where(occ != 0, F(0.0), F(1.0)).astype(F)[:, None]
        L[idx] = v * (np.ones((idx.size, 3), F) if albedo is None else np.asarray(albedo, F).reshape(-1, 3)[idx])
    sb = cam.film.get_sample_bounds()
    shape = (spp, int(sb.p_max[1] - sb.p_min[1]) + 1, int(sb.p_max[0] - sb.p_min[0]) + 1)
    return Result(L=L.reshape(*shape, 3), cls=cls.reshape(shape), hit=hit.reshape(shape), wi=wi, nf=nf, rays=rays, occlusion_rays=orays, hit_index=idx)


def shares(cls):
    """Fractions of the frame's samples that are misses, occluded and open."""
    return tuple(float((cls == k).mean()) for k in (MISS, OCCLUDED, OPEN))
