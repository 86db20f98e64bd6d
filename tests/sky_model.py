"""The environment lookup and the sky-lit frame (trhip_env, trhip_render_sky; docs/design/25-sky.md) restated from the specification: the gutter and env_eval in numpy Float32,
one operation per step in the specification's order, and the frame as tests/ao_model.py's frame (its camera samples, directions, oracle rays and verdicts) with the two
substitutions.  Nothing here calls the library's lookup; the GPU tests compare trhip_env_eval and the per-sample radiance with this model bit for bit."""
import numpy as np

import ao_model as am
from ao_model import camera_samples, directions  # noqa: F401  (the frame's samples and occlusion directions are the AO model's)

F = np.float32
MISS, OCCLUDED, OPEN = am.MISS, am.OCCLUDED, am.OPEN


def gutter(texels):
    """(n + 2, n + 2, 3) storage, indexed [j + 1, i + 1]: the map and its one-texel gutter.  A column i outside [0, n) takes the interior texel (clamp(i), n - 1 - j), a row j
    outside (n - 1 - i, clamp(j)); a corner both, which is the texel diagonally opposite: (n - 1 - clamp(i), n - 1 - clamp(j))."""
    t = np.asarray(texels, F)
    n = t.shape[0]
    assert t.shape == (n, n, 3)
    idx = np.arange(-1, n + 1)
    j, i = np.meshgrid(idx, idx, indexing="ij")
    out_i, out_j = (i < 0) | (i >= n), (j < 0) | (j >= n)
    ci, cj = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)
    si = np.where(out_i & out_j, n - 1 - ci, np.where(out_j, n - 1 - i, ci))
    sj = np.where(out_i & out_j, n - 1 - cj, np.where(out_i, n - 1 - j, cj))
    return np.ascontiguousarray(t[sj, si])


def sgn(v):
    return np.where(v < 0, F(-1.0), F(1.0)).astype(F)


def coords(dirs, n, R=None):
    """(ok, fx, fy) of the lookup: whether the direction has a lookup at all (s > 0 and finite), and the continuous texel coordinates."""
    w = np.asarray(dirs, F).reshape(-1, 3)
    R = np.eye(3, dtype=F) if R is None else np.asarray(R, F)
    with np.errstate(all="ignore"):
        e = [(R[r, 0] * w[:, 0] + R[r, 1] * w[:, 1]) + R[r, 2] * w[:, 2] for r in range(3)]
        s = (np.abs(e[0]) + np.abs(e[1])) + np.abs(e[2])
        ok = (s > 0) & np.isfinite(s)
        px, py = e[0] / s, e[1] / s
        qx = (F(1.0) - np.abs(py)) * sgn(px)
        qy = (F(1.0) - np.abs(px)) * sgn(py)
        lower = e[2] < 0
        px, py = np.where(lower, qx, px).astype(F), np.where(lower, qy, py).astype(F)
        fx = (px * F(0.5) + F(0.5)) * F(n) - F(0.5)
        fy = (py * F(0.5) + F(0.5)) * F(n) - F(0.5)
    assert fx.dtype == fy.dtype == F
    return ok, fx, fy


def lerp(a, b, t):
    return a + t * (b - a)


def env_eval(texels, dirs, R=None):
    """E(w) for every direction: (m, 3) Float32."""
    st = gutter(texels)
    n = st.shape[0] - 2
    ok, fx, fy = coords(dirs, n, R)
    fx, fy = np.where(ok, fx, F(0.0)).astype(F), np.where(ok, fy, F(0.0)).astype(F)
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    ix, iy = np.clip(x0.astype(np.int64), -1, n - 1) + 1, np.clip(y0.astype(np.int64), -1, n - 1) + 1
    top = lerp(st[iy, ix], st[iy, ix + 1], tx)
    bottom = lerp(st[iy + 1, ix], st[iy + 1, ix + 1], tx)
    out = lerp(top, bottom, ty)
    assert out.dtype == F
    out[~ok] = F(0.0)
    return out


def centre_directions(n):
    """A direction through the centre of every texel, (n, n, 3) Float32 indexed [j, i], from the inverse of the map — not normalised: the lookup divides by the 1-norm."""
    c = ((np.arange(n, dtype=np.float64) + 0.5) / n) * 2.0 - 1.0
    px, py = np.meshgrid(c, c, indexing="xy")
    z = 1.0 - np.abs(px) - np.abs(py)
    x = np.where(z < 0, (1.0 - np.abs(py)) * np.where(px < 0, -1.0, 1.0), px)
    y = np.where(z < 0, (1.0 - np.abs(px)) * np.where(py < 0, -1.0, 1.0), py)
    return np.stack([x, y, z], axis=-1).astype(F)


def adversarial_directions(count=1000, seed=11):
    """`count` directions: the axes and their negatives, -0 components, denormals, huge and tiny lengths, the diagonals of the octants and of the faces (the edges of the
    octahedral square and its corners), then random ones.  All finite with a finite, positive 1-norm under a rotation."""
    tiny, den = np.finfo(F).tiny, F(1e-42)
    fixed = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-0.0, 0, 1], [0, -0.0, 1], [-0.0, -0.0, -1], [1, -0.0, -0.0], [-0.0, 1, -0.0], [den, 0, 0], [0, -den, 0],
             [0, 0, -den], [den, den, -den], [-den, den, den], [tiny, -tiny, tiny], [1e-30, 2e-30, -3e-30], [1e30, -2e30, 1e29], [-1e37, 1e37, -1e37], [1, 1, 0], [-1, 1, 0], [1, -1, 0],
             [-1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, -1], [0, -1, -1], [-1, 0, -1e-20], [1, 0, -1e-20], [0, 1, -1e-20], [0, -1, -1e-20], [1, 1, 1], [-1, 1, 1], [1, -1, 1], [-1, -1, 1],
             [1, 1, -1], [-1, 1, -1], [1, -1, -1], [-1, -1, -1], [1e-8, 1e-8, -1], [-1e-8, 1e-8, -1], [1e-8, -1e-8, -1], [-1e-8, -1e-8, -1]]
    rng = np.random.default_rng(seed)
    rnd = rng.normal(size=(count - len(fixed), 3))
    rnd[::7] *= 10.0 ** rng.uniform(-30, 30, size=rnd[::7].shape[:1])[:, None]
    rnd[3::11, 2] = -np.abs(rnd[3::11, 2]) * 1e-6  # grazing from below: the fold near the diamond's edges
    return np.concatenate([np.array(fixed, np.float64), rnd]).astype(F)


def rotation(axis=(0.3, -0.5, 0.8), angle=1.1):
    """A turned world_to_env (Rodrigues), Float32."""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).astype(F)


def random_map(n, seed=5):
    """n x n x 3 texels in [0, 4): data for the lookup tests."""
    return (np.random.default_rng(seed + n).random((n, n, 3)) * 4.0).astype(F)


def render(osc, cam, spp, seed, texels, R=None, sample_offset=0, max_distance=np.inf, scale=1.0, albedo=None, hide_background=False, frame=None):
    """Per-sample L (spp, sb_h, sb_w, 3) and class of a sky frame: the AO model's frame (same camera samples, hits, occlusion rays and verdicts), with
    c = env_eval(wi) * scale (times the per-sample base colour `albedo`, (n, 3), under TRHIP_SKY_ALBEDO) for an open ray and env_eval(d) * scale (0 with hide_background)
    for a camera ray that misses.  Also `c`, the contribution of every sample's occlusion ray whatever its verdict (zero rows for misses).  `frame`: the AO model's result for
    the same (osc, cam, spp, seed, sample_offset, max_distance), when the caller already has it."""
    r = frame if frame is not None else am.render(osc, cam, spp, seed, sample_offset, max_distance)
    cls = r.cls.reshape(-1)
    L = np.zeros((cls.size, 3), F)
    c = np.zeros((cls.size, 3), F)
    hit = cls != MISS
    c[hit] = env_eval(texels, r.wi[hit], R) * F(scale)
    if albedo is not None:
        c[hit] = c[hit] * np.asarray(albedo, F).reshape(-1, 3)[hit]
    L[cls == OPEN] = c[cls == OPEN]
    if not hide_background:
        L[~hit] = env_eval(texels, r.rays[~hit, 4:7], R) * F(scale)
    return am.Result(L=L.reshape(*r.cls.shape, 3), cls=r.cls, hit=r.hit, wi=r.wi, nf=r.nf, rays=r.rays, c=c.reshape(*r.cls.shape, 3))
