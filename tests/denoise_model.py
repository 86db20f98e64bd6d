"""A numpy Float32 model of the edge-avoiding à-trous denoiser, written from its specification (docs/design/12-denoise.md) and from nothing else: it imports nothing from the library.
Vectorised over pixels, a Python loop over the 25 taps in the specified order (dy outer, dx inner); every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_denoise_api.py (CPU) checks the model's own properties, tests/test_gpu_denoise.py compares the kernels with it bit for bit."""
from dataclasses import dataclass

import numpy as np

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))


@dataclass
class Params:
    sigma_colour: float
    sigma_normal: float
    sigma_plane: float
    iterations: int = 5
    demodulate: bool = True
    albedo_floor: float = 1.0 / 64.0
    min_coverage: float = 0.5


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def to_Y(c):
    return (F(0.212671) * c[..., 0] + F(0.715160) * c[..., 1]) + F(0.072169) * c[..., 2]


def xyz_to_rgb(c):
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([(F(3.240479) * x - F(1.537150) * y) - F(0.498535) * z, (F(-0.969256) * x + F(1.875991) * y) + F(0.041556) * z,
                     (F(0.055648) * x - F(0.204043) * y) + F(1.057311) * z], axis=-1)


def rgb_to_xyz(c):
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([(F(0.412453) * r + F(0.357580) * g) + F(0.180423) * b, (F(0.212671) * r + F(0.715160) * g) + F(0.072169) * b,
                     (F(0.019334) * r + F(0.119193) * g) + F(0.950227) * b], axis=-1)


def tukey(x):
    """g(x) = x < 1 ? (1 - x*x)^2 : 0, literally: NaN gives 0, a negative argument is < 1."""
    t = F(1.0) - x * x
    return np.where(x < F(1.0), t * t, F(0.0)).astype(F)


def prepare(B, P, prm):
    """(surface mask, n, p, c, Y, a, W) of every pixel.  B: (H, W, 4) film, P: (H, W, 3, 4) planes."""
    W, A, H = B[..., 3], P[..., 0, 3], P[..., 1, 3]
    surface = (W > 0) & (A > 0) & (H > 0) & (H >= F(prm.min_coverage) * A)
    iH = F(1.0) / H
    n = P[..., 1, :3] * iH[..., None]
    length = np.sqrt(dot3(n, n))
    surface &= length > 0
    n = n / length[..., None]
    p = P[..., 2, :3] * iH[..., None]
    iW = F(1.0) / W
    c = xyz_to_rgb(B[..., :3] * iW[..., None])
    a = np.zeros_like(c)
    if prm.demodulate:
        iA = F(1.0) / A
        a = P[..., 0, :3] * iA[..., None]
        a = np.where(a > F(prm.albedo_floor), a, F(prm.albedo_floor)).astype(F)
        c = c / a
    surface &= np.isfinite(n).all(-1) & np.isfinite(p).all(-1) & np.isfinite(c).all(-1)
    return surface, n, p, c, to_Y(c), a, W


def denoise(B, P, prm, tally=None):
    """The denoised film, (H, W, 4) Float32.  `tally`, a dict, receives per weight ('normal', 'plane', 'colour') the number of (pixel, off-centre neighbour) pairs whose
    weight was exactly 0 and the number whose weight lay strictly between 0 and 1, over all iterations."""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    assert B.ndim == 3 and B.shape[2] == 4 and P.shape == B.shape[:2] + (3, 4) and 0 <= prm.iterations <= 6
    if prm.iterations == 0:
        return B.copy()
    h, w = B.shape[:2]
    with np.errstate(all="ignore"):
        surface, n, p, c, Y, a, W = prepare(B, P, prm)
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for i in range(prm.iterations):
            s = 1 << i
            sigma_c = F(prm.sigma_colour) * F(2.0 ** -i)
            total, ws = np.zeros((h, w, 3), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    valid = surface & inside & surface[qy, qx]
                    k = K[abs(dy)] * K[abs(dx)]
                    wn = tukey((F(1.0) - dot3(n, n[qy, qx])) / F(prm.sigma_normal))
                    wp = tukey(np.abs(dot3(n, p[qy, qx] - p)) / F(prm.sigma_plane))
                    wc = tukey(np.abs(Y[qy, qx] - Y) / sigma_c)
                    wt = ((k * wn) * wp) * wc
                    total = np.where(valid[..., None], total + wt[..., None] * c[qy, qx], total)
                    ws = np.where(valid, ws + wt, ws)
                    if tally is not None and (dy or dx):
                        for name, v in (("normal", wn), ("plane", wp), ("colour", wc)):
                            t = tally.setdefault(name, [0, 0])
                            t[0] += int(np.sum(valid & (v == 0)))
                            t[1] += int(np.sum(valid & (v > 0) & (v < 1)))
            c = np.where(surface[..., None], total / ws[..., None], c).astype(F)
            Y = to_Y(c)
        if prm.demodulate:
            c = c * a
        xyz = rgb_to_xyz(c) * W[..., None]
    out = B.copy()
    out[surface, :3] = xyz[surface]
    return out


def surface_mask(B, P, prm):
    with np.errstate(all="ignore"):
        return prepare(np.ascontiguousarray(B, F), np.ascontiguousarray(P, F), prm)[0]


def planes_of(n, p, albedo, total_w, hit_w, depth=None):
    """Feature planes in the layout of the library's feature-buffer call from per-pixel normal, position, base colour and the two weights (all Float32)."""
    h, w = total_w.shape
    P = np.zeros((h, w, 3, 4), F)
    P[..., 0, :3], P[..., 0, 3] = albedo * total_w[..., None], total_w
    P[..., 1, :3], P[..., 1, 3] = n * hit_w[..., None], hit_w
    P[..., 2, :3] = p * hit_w[..., None]
    P[..., 2, 3] = (np.ones((h, w), F) if depth is None else depth) * hit_w
    return P


def synthetic(h, w, seed):
    """A noisy film and its planes: unit normals in three clusters (two vertical cuts at slanted positions), jittered; piecewise-planar positions with a little relief;
    noisy colours over a few base colours; misses, thin-coverage pixels, and the poisoned pixels: W = 0, negative H, a NaN in the position plane, an Inf in the film.
    Returns (B, P, poisoned (y, x) list)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    region = ((xs + ys // 3) * 3 // (w + h // 3)).clip(0, 2)
    base_n = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], F)
    n = base_n[region] + rng.normal(0.0, 0.06, (h, w, 3)).astype(F)
    n = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(F)
    p = np.stack([xs * 0.1, ys * 0.1, region * 0.5 + 0.02 * xs], -1).astype(F) + (rng.normal(0.0, 0.01, (h, w, 1)).astype(F) * base_n[region])
    albedo = np.array([[0.8, 0.3, 0.2], [0.25, 0.4, 0.85], [0.004, 0.9, 0.9]], F)[region] * rng.uniform(0.9, 1.1, (h, w, 1)).astype(F)
    rgb = albedo * (F(0.5) + rng.exponential(0.25, (h, w, 3)).astype(F)) * np.array([1.0, 0.6, 1.5], F)[(xs // 7 + ys // 5) % 3][..., None]
    rgb_to = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F)
    total_w = rng.uniform(0.6, 1.4, (h, w)).astype(F)
    B = np.concatenate([(rgb @ rgb_to.T) * total_w[..., None], total_w[..., None]], -1).astype(F)
    cover = np.ones((h, w), F)
    cover[rng.random((h, w)) < 0.06] = F(0.3)   # silhouette pixels under min_coverage = 0.5
    cover[rng.random((h, w)) < 0.05] = F(0.75)  # … and over it
    miss = rng.random((h, w)) < 0.05
    miss[h // 2:h // 2 + 3, w // 3:w // 3 + 4] = True  # a hole wider than one tap
    cover[miss] = F(0.0)
    B[miss, :3] = F(0.0)
    P = planes_of(n, p, albedo.astype(F), total_w, (total_w * cover).astype(F))
    poisoned = [(1, 2), (h // 3, w // 2), (h - 2, w - 3), (h // 2 + 5, 1)]
    (y0, x0), (y1, x1), (y2, x2), (y3, x3) = poisoned
    B[y0, x0, 3] = F(0.0)            # W = 0
    P[y1, x1, 1, 3] = F(-0.7)        # negative hit weight
    P[y2, x2, 2, 1] = F(np.nan)      # NaN in the position plane
    B[y3, x3, 0] = F(np.inf)         # Inf radiance
    return B, P, poisoned
