"""Importance sampling of the environment map and the importance-sampled sky frame (trhip_env_make_sampler, trhip_env_sample, trhip_env_pdf, trhip_render_sky_is;
docs/design/27-sky-importance.md) restated from the specification: the tables in numpy Float64 with the specification's order of every sum, env_sample and env_pdf in numpy
Float32, one operation per step, and the frame as tests/sky_model.py's frame with the one substitution per hit.  Nothing here calls the library's sampler; the GPU tests
compare trhip_env_sample, trhip_env_pdf and the per-sample radiance with this model bit for bit."""
import sys

import numpy as np

import ao_model as am
import oracle_bridge as ob
import sky_model as sm

F = np.float32
MISS, OCCLUDED, OPEN, NO_RAY = am.MISS, am.OCCLUDED, am.OPEN, 3  # NO_RAY: a hit whose direction has cos <= 0 or p <= 0: no occlusion ray, L = 0
ONE_MINUS = F(1.0 - 2.0 ** -24)
INV_PI = F(1.0) / F(np.pi)
TS_V_LIGHT_PICK, TS_V_LIGHT_U0, TS_V_LIGHT_U1 = 5 + 0, 5 + 1, 5 + 2  # ts_vertex_dim(0, TS_V_LIGHT_*), include/trace_sampler.h


class Tables:
    """m: the marginal (n + 1,) Float32; c: the conditionals (n, n + 1) Float32, row j; w: the Float64 weights [j, i] they were made from."""

    def __init__(self, m, c, w):
        self.m, self.c, self.w, self.n = m, c, w, c.shape[0]

    def flat(self):
        """The device layout: the marginal, then the conditionals: (n + 1)(n + 1) floats."""
        return np.concatenate([self.m, self.c.reshape(-1)])


def jacobian(n):
    """d(omega) / d(area of the square) = 1 / |P|^3 at every cell centre, [j, i] Float64, P the centre's point of the octahedron |x| + |y| + |z| = 1."""
    c = np.abs(((np.arange(n, dtype=np.float64) + 0.5) / n) * 2.0 - 1.0)
    a, b = c[None, :], c[:, None]
    upper = a + b <= 1.0
    px, py, pz = np.where(upper, a, 1.0 - b), np.where(upper, b, 1.0 - a), np.where(upper, (1.0 - a) - b, (a + b) - 1.0)
    r2 = (px * px + py * py) + pz * pz
    return 1.0 / (r2 * np.sqrt(r2))


def weights(texels):
    """w[j, i] Float64: the 3 x 3 kernel k (x) k, k = (1/8, 3/4, 1/8), over the channel sum of the gutter storage — a (the offset in i) outside, b (in j) inside — times the
    Jacobian of the cell's centre."""
    st = sm.gutter(texels).astype(np.float64)
    n = st.shape[0] - 2
    y = (st[..., 0] + st[..., 1]) + st[..., 2]
    k = (0.125, 0.75, 0.125)
    W = np.zeros((n, n))
    for a in range(3):
        for b in range(3):
            W = W + (k[a] * k[b]) * y[b:b + n, a:a + n]
    return W * jacobian(n)


def tables(texels):
    """The sampler's tables, or None where every weight is zero.  np.cumsum accumulates in order, as the specification's sums do (np.sum does not)."""
    w = weights(texels)
    n = w.shape[0]
    cum = np.cumsum(w, axis=1)
    rows = cum[:, -1]
    rcum = np.cumsum(rows)
    total = rcum[-1]
    if not total > 0.0:
        return None
    m = np.concatenate([[0.0], rcum[:-1] / total]).astype(F)
    with np.errstate(all="ignore"):
        c = np.concatenate([np.zeros((n, 1)), cum[:, :-1]], axis=1) / rows[:, None]
    c = np.where(rows[:, None] > 0.0, c, (np.arange(n, dtype=np.float64) / n)[None, :]).astype(F)
    return Tables(np.concatenate([m, [F(1.0)]]).astype(F), np.concatenate([c, np.ones((n, 1), F)], axis=1).astype(F), w)


def search(T, n, u):
    """The largest k in [0, n - 1] with T(k) <= u by the fixed-trip search; T: a function of an index array (the read is made only where k <= n - 1)."""
    lo = np.zeros(u.shape, np.int64)
    step = 1 << ((n - 1).bit_length() - 1) if n > 1 else 0
    while step:
        k = lo + step
        inside = k <= n - 1
        lo = np.where(inside & (T(np.minimum(k, n - 1)) <= u), k, lo)
        step >>= 1
    return lo


def env_sample(tab, u0, u1, R=None, cells=False):
    """wi (m, 3) Float32 for the points (u0, u1); with `cells` also the chosen (i, j) and the point (qx, qy) of the square."""
    u0, u1 = np.asarray(u0, F).reshape(-1), np.asarray(u1, F).reshape(-1)
    R = np.eye(3, dtype=F) if R is None else np.asarray(R, F)
    n, nf = tab.n, F(tab.n)
    with np.errstate(all="ignore"):
        j = search(lambda k: tab.m[k], n, u1)
        pj = tab.m[j + 1] - tab.m[j]
        v = np.minimum((u1 - tab.m[j]) / pj, ONE_MINUS)
        i = search(lambda k: tab.c[j, k], n, u0)
        pi = tab.c[j, i + 1] - tab.c[j, i]
        t = np.minimum((u0 - tab.c[j, i]) / pi, ONE_MINUS)
        qx = ((i.astype(F) + t) / nf) * F(2.0) - F(1.0)
        qy = ((j.astype(F) + v) / nf) * F(2.0) - F(1.0)
        a, b = np.abs(qx), np.abs(qy)
        ez = (F(1.0) - a) - b
        lower = ez < 0
        ex = np.where(lower, (F(1.0) - b) * sm.sgn(qx), qx).astype(F)
        ey = np.where(lower, (F(1.0) - a) * sm.sgn(qy), qy).astype(F)
        w = [(R[0, c] * ex + R[1, c] * ey) + R[2, c] * ez for c in range(3)]
        l = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        out = np.stack([w[0] / l, w[1] / l, w[2] / l], axis=1)
    assert out.dtype == F
    return (out, i, j, qx, qy) if cells else out


def pdf_cells(n, dirs, R=None):
    """(ok, r2, i, j): whether the direction has a lookup, |P|^2 of its point of the octahedron, and the cell env_pdf indexes."""
    w = np.asarray(dirs, F).reshape(-1, 3)
    R = np.eye(3, dtype=F) if R is None else np.asarray(R, F)
    with np.errstate(all="ignore"):
        e = [(R[r, 0] * w[:, 0] + R[r, 1] * w[:, 1]) + R[r, 2] * w[:, 2] for r in range(3)]
        s = (np.abs(e[0]) + np.abs(e[1])) + np.abs(e[2])
        ok = (s > 0) & np.isfinite(s)
        s = np.where(ok, s, F(1.0)).astype(F)
        e = [np.where(ok, c, F(0.0)).astype(F) for c in e]
        px, py, pz = e[0] / s, e[1] / s, e[2] / s
        r2 = (px * px + py * py) + pz * pz
        qx = (F(1.0) - np.abs(py)) * sm.sgn(px)
        qy = (F(1.0) - np.abs(px)) * sm.sgn(py)
        lower = e[2] < 0
        px, py = np.where(lower, qx, px).astype(F), np.where(lower, qy, py).astype(F)
        i = np.clip(np.floor((px * F(0.5) + F(0.5)) * F(n)).astype(np.int64), 0, n - 1)
        j = np.clip(np.floor((py * F(0.5) + F(0.5)) * F(n)).astype(np.int64), 0, n - 1)
    return ok, r2.astype(F), i, j


def env_pdf(tab, dirs, R=None):
    """The density with respect to solid angle of every direction: (m,) Float32, +0 where the lookup has no answer."""
    n, nf = tab.n, F(tab.n)
    ok, r2, i, j = pdf_cells(n, dirs, R)
    pm = tab.m[j + 1] - tab.m[j]
    pc = tab.c[j, i + 1] - tab.c[j, i]
    p = ((pm * pc) * ((nf * nf) * F(0.25))) * (r2 * np.sqrt(r2))
    assert p.dtype == F
    return np.where(ok, p, F(0.0)).astype(F)


def weight(tab, R, nf, wc, xi, u0, u1, mix):
    """The substitution's geometry: (wi, ray, g) for hits with face-forwarded normals nf, cosine directions wc, and the three light-dimension numbers.  ray: whether an
    occlusion ray is cast (cos > 0 and p > 0); g = pc / p, 0 where there is no ray."""
    mix = F(mix)
    om = F(1.0) - mix
    we = env_sample(tab, u0, u1, R)
    wi = np.where((np.asarray(xi, F) < mix)[:, None], we, wc).astype(F)
    with np.errstate(all="ignore"):
        c0 = am.dot3(nf, wi)
        pc = c0 * INV_PI
        pe = env_pdf(tab, wi, R)
        p = om * pc + mix * pe
        ray = (c0 > 0) & (p > 0)
        g = np.where(ray, pc / np.where(ray, p, F(1.0)), F(0.0)).astype(F)
    return wi, ray, g


def estimate(tab, texels, R, nf, wc, xi, u0, u1, mix, scale=1.0):
    """(wi, ray, c): c the contribution (E(wi) * scale) * g of every hit, zero rows where there is no ray."""
    wi, ray, g = weight(tab, R, nf, wc, xi, u0, u1, mix)
    c = (sm.env_eval(texels, wi, R) * F(scale)) * g[:, None]
    assert c.dtype == F
    c[~ray] = F(0.0)
    return wi, ray, c


def trace(osc, cam, spp, seed, texels, R=None, mix=0.5, sample_offset=0, max_distance=np.inf, tab=None):
    """Everything of an importance-sampled sky frame that does not depend on scale and flags: tests/ao_model.py's camera samples and hits, the substitution's directions and
    weights, and the oracle's any-hit verdict on the rays that are cast.  shade() makes the radiance from it."""
    S = sys.modules["trace_jl_amd"].scenes
    tab = tab if tab is not None else tables(texels)
    samples, key = am.camera_samples(cam, spp, seed, sample_offset)
    rays = ob.generate_rays(cam, samples)
    _, prim, geom, _ = osc.trace_closest(rays, want_geom=True)
    hit = prim >= 0
    n = rays.shape[0]
    cls = np.full(n, MISS, np.int32)
    wi = np.zeros((n, 3), F)
    g = np.zeros(n, F)
    idx = np.flatnonzero(hit)
    if idx.size:
        k = key[idx]
        u = np.stack([S.ts_uniform(k, am.TS_V_BSDF_U0), S.ts_uniform(k, am.TS_V_BSDF_U1)], axis=1)
        nf, wc = am.directions(geom[idx, 6:9], -rays[idx, 4:7], u)
        wi[idx], ray, g[idx] = weight(tab, R, nf, wc, S.ts_uniform(k, TS_V_LIGHT_PICK), S.ts_uniform(k, TS_V_LIGHT_U0), S.ts_uniform(k, TS_V_LIGHT_U1), mix)
        cls[idx] = NO_RAY
        cast = idx[ray]
        orays = np.zeros((cast.size, 8), F)
        orays[:, 0:3] = geom[cast, 0:3] + F(1e-6) * wi[cast]  # spawn_ray(si, wi), Trace.jl:206-211
        orays[:, 3] = F(max_distance)
        orays[:, 4:7] = wi[cast]
        orays[:, 7] = rays[cast, 7]
        if cast.size:
            occ, _ = osc.trace_any(orays)
            cls[cast] = np.where(occ != 0, OCCLUDED, OPEN)
    sb = cam.film.get_sample_bounds()
    shape = (spp, int(sb.p_max[1] - sb.p_min[1]) + 1, int(sb.p_max[0] - sb.p_min[0]) + 1)
    return am.Result(cls=cls.reshape(shape), hit=hit.reshape(shape), wi=wi, g=g, rays=rays, texels=np.asarray(texels, F), R=R, mix=F(mix))


def shade(tr, scale=1.0, albedo=None, hide_background=False):
    """Per-sample L (spp, sb_h, sb_w, 3) of the frame trace() walked: c = (E(wi) * scale) * g (times the per-sample base colour `albedo`, (n, 3), under TRHIP_SKY_ALBEDO)
    where the ray is open, the sky frame's E(d) * scale (0 with hide_background) for a camera ray that misses, 0 elsewhere.  Also `c`, every cast ray's contribution."""
    cls = tr.cls.reshape(-1)
    L = np.zeros((cls.size, 3), F)
    c = np.zeros((cls.size, 3), F)
    cast = (cls == OCCLUDED) | (cls == OPEN)
    c[cast] = (sm.env_eval(tr.texels, tr.wi[cast], tr.R) * F(scale)) * tr.g[cast][:, None]
    if albedo is not None:
        c[cast] = c[cast] * np.asarray(albedo, F).reshape(-1, 3)[cast]
    L[cls == OPEN] = c[cls == OPEN]
    if not hide_background:
        L[cls == MISS] = sm.env_eval(tr.texels, tr.rays[cls == MISS, 4:7], tr.R) * F(scale)
    return am.Result(L=L.reshape(*tr.cls.shape, 3), cls=tr.cls, c=c.reshape(*tr.cls.shape, 3))


def render(osc, cam, spp, seed, texels, R=None, mix=0.5, sample_offset=0, max_distance=np.inf, scale=1.0, albedo=None, hide_background=False, tab=None):
    """trace() and shade() in one call."""
    return shade(trace(osc, cam, spp, seed, texels, R, mix, sample_offset, max_distance, tab), scale, albedo, hide_background)


def sun_map(n=64, at=(0.3, 0.2), sky=0.05, sun=2000.0):
    """An n x n map of `sky` with one texel of `sun` at the cell that contains the point `at` of the square: the statistics' map."""
    t = np.full((n, n, 3), sky, F)
    i, j = int(np.floor((at[0] * 0.5 + 0.5) * n)), int(np.floor((at[1] * 0.5 + 0.5) * n))
    t[j, i] = F(sun)
    return t, (i, j)


def test_map(n, seed=5):
    """tests/sky_model.py's random map with what the sampler has to get right, from n = 7 on: the middle rows of zero texels (rows 2 .. 4 of 7, 30 .. 33 of 64: the edge
    wrap continues them with each other, so the rows between them have no weight at all), a zero texel, and a bright texel in each hemisphere (one above the centre of the
    square, one in a corner)."""
    t = sm.random_map(n, seed)
    if n >= 7:
        t[(n - 3) // 2:n - (n - 3) // 2] = F(0.0)
        t[n // 4, n // 2] = F(300.0)
        t[0, n - 1] = F(500.0)
        t[n - 1, 1] = F(0.0)
    return t


def u_set(tab, count=2000, seed=3):
    """(u0, u1) Float32: the corners of [0, 1 - 2^-24]^2, every table entry below 1 with its two Float32 neighbours (u1 from the marginal, u0 from every conditional), then
    `count` random points."""
    rng = np.random.default_rng(seed)

    def around(v):
        v = np.unique(np.asarray(v, F).reshape(-1))
        v = np.concatenate([v, np.nextafter(v, F(-1.0)), np.nextafter(v, F(2.0))]).astype(F)
        return v[(v >= 0) & (v < 1)]

    corners = F([[0, 0], [ONE_MINUS, ONE_MINUS], [0, ONE_MINUS], [ONE_MINUS, 0]])
    on_m = around(tab.m)
    on_c = around(tab.c)
    a = np.stack([rng.random(on_m.size).astype(F), on_m], axis=1)
    b = np.stack([on_c, rng.random(on_c.size).astype(F)], axis=1)
    r = rng.random((count, 2)).astype(F)
    # u0 exactly on an entry of the row that u1 selects
    j = search(lambda k: tab.m[k], tab.n, r[:, 1])
    e = np.stack([tab.c[j, rng.integers(0, tab.n, size=count)], r[:, 1]], axis=1)
    u = np.concatenate([corners, a, b, e, r]).astype(F)
    u[u >= 1] = ONE_MINUS
    return np.ascontiguousarray(u)
