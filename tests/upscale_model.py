"""A numpy Float32 model of the edge-aware upscaler, written from its specification (docs/design/17-upscale.md) and from nothing else: it imports the denoiser's model for
Prepare and the colour matrices, and nothing from the library.  Vectorised over full-size pixels, a Python loop over the taps in the specified order (j outer, i inner); every
line is one Float32 operation, in the order the text gives.

Not a test: tests/test_upscale_api.py (CPU) checks the model's own properties, tests/test_gpu_upscale.py compares the kernels with it bit for bit."""
from dataclasses import dataclass

import numpy as np

import denoise_model as dm

F = np.float32
TALLY_KEYS = ("guided", "unguided", "orphan", "nothing", "tap_off_image", "tap_rejected_normal", "tap_rejected_plane", "guided_not_finite", "zero_weight_tap_tx0")


@dataclass
class Params:
    lo_from_hi: tuple  # (ax, bx, ay, by)
    radius: int = 2
    demodulate: bool = True
    coverage: bool = True
    sigma_normal: float = 0.25
    sigma_plane: float = 0.1
    albedo_floor: float = 1.0 / 64.0
    min_coverage: float = 0.5


def finite3(v):
    return np.isfinite(v).all(-1)


def low_records(B, P, prm):
    """Steps L1-L3: (s, n, p, c, valid, u) of every low pixel."""
    with np.errstate(all="ignore"):
        return _low_records(B, P, prm)


def _low_records(B, P, prm):
    s, n, p, c, _, _, W = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=prm.demodulate, albedo_floor=prm.albedo_floor, min_coverage=prm.min_coverage))
    A, H = P[..., 0, 3], P[..., 1, 3]
    if prm.coverage:  # L2
        v = H / A
        c = c / v[..., None]
        s = s & finite3(c)
    valid = W > 0  # L3
    iW = F(1.0) / W
    u = dm.xyz_to_rgb(B[..., :3] * iW[..., None])
    valid = valid & finite3(u)
    zero = np.zeros_like(c)
    n, p, c = (np.where(s[..., None], a, zero).astype(F) for a in (n, p, c))
    u = np.where(valid[..., None], u, zero).astype(F)
    return s, n, p, c, valid, u


def tent(i, t, inv_r):
    d = t + F(-i) if i <= 0 else F(i) - t
    return F(1.0) - d * inv_r


def unguided(valid, u, x0, y0, tx, ty):
    """H5 for every full-size pixel: (ok, colour).  The four taps j = 0, 1 outer, i = 0, 1 inner."""
    lh, lw = valid.shape
    su, sb = np.zeros(x0.shape + (3,), F), np.zeros(x0.shape, F)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            inside = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
            cx, cy = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)
            b = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
            acc = inside & valid[cy, cx]
            su = np.where(acc[..., None], su + b[..., None] * u[cy, cx], su)
            sb = np.where(acc, sb + b, sb)
    cu = su / sb[..., None]
    ok = (sb > 0) & finite3(cu)
    return ok, np.where(ok[..., None], cu, F(0.0)).astype(F)


def positions(prm, h, w):
    """H3: (x0, tx) per column and (y0, ty) per row, broadcast to (h, w)."""
    ax, bx, ay, by = (F(v) for v in prm.lo_from_hi)
    fx = np.arange(w, dtype=F) * ax
    fx = fx + bx
    fy = np.arange(h, dtype=F) * ay
    fy = fy + by
    fx0, fy0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - fx0, fy - fy0
    bc = lambda col, row: (np.broadcast_to(col[None, :], (h, w)), np.broadcast_to(row[:, None], (h, w)))  # noqa: E731
    x0, y0 = bc(fx0.astype(np.int64), fy0.astype(np.int64))
    txx, tyy = bc(tx.astype(F), ty.astype(F))
    return x0, y0, txx, tyy


def upscale(lo_xyzw, lo_planes, hi_planes, prm, tally=None, unguided_only=False, want_colour=False, records=None):
    """(out_xyzw (h, w, 4) Float32, mask (h, w) uint8).  `tally`, a dict, receives the number of pixels per class and of (pixel, tap) pairs per tap event (TALLY_KEYS).
    `unguided_only`: H5 applied to every pixel of positive weight (the baseline of the quality figure).  `want_colour`: also returns c' (h, w, 3).  `records`: what
    low_records would return, given instead of computed (the tests of the model's own properties)."""
    B, PL, PH = np.ascontiguousarray(lo_xyzw, F), np.ascontiguousarray(lo_planes, F), np.ascontiguousarray(hi_planes, F)
    assert B.ndim == 3 and B.shape[2] == 4 and PL.shape == B.shape[:2] + (3, 4) and PH.ndim == 4 and PH.shape[2:] == (3, 4) and prm.radius in (1, 2)
    h, w = PH.shape[:2]
    lh, lw = B.shape[:2]
    R, inv_r = prm.radius, F(1.0) / F(prm.radius)
    t = dict.fromkeys(TALLY_KEYS, 0)
    with np.errstate(all="ignore"):
        s_q, n_q, p_q, c_q, valid_q, u_q = low_records(B, PL, prm) if records is None else records
        A, H = PH[..., 0, 3], PH[..., 1, 3]
        weighted = A > 0  # H1
        # H2
        surface = (H > 0) & (H >= F(prm.min_coverage) * A)
        iH = F(1.0) / H
        n = PH[..., 1, :3] * iH[..., None]
        length = np.sqrt(dm.dot3(n, n))
        surface &= length > 0
        n = n / length[..., None]
        p = PH[..., 2, :3] * iH[..., None]
        surface &= finite3(n) & finite3(p)
        a = v = None
        if prm.demodulate:
            iA = F(1.0) / A
            a = PH[..., 0, :3] * iA[..., None]
            a = np.where(a > F(prm.albedo_floor), a, F(prm.albedo_floor)).astype(F)
            surface &= finite3(a)
        if prm.coverage:
            v = H / A
            surface &= np.isfinite(v)
        surface &= weighted
        x0, y0, tx, ty = positions(prm, h, w)  # H3
        # H4
        guided = np.zeros((h, w), bool)
        cg = np.zeros((h, w, 3), F)
        if not unguided_only:
            total, ws = np.zeros((h, w, 3), F), np.zeros((h, w), F)
            for j in range(1 - R, R + 1):
                ky = tent(j, ty, inv_r)
                for i in range(1 - R, R + 1):
                    kx = tent(i, tx, inv_r)
                    k = ky * kx
                    qx, qy = x0 + i, y0 + j
                    inside = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
                    cx, cy = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)
                    counts = surface & inside & s_q[cy, cx]
                    wn = dm.tukey((F(1.0) - dm.dot3(n, n_q[cy, cx])) / F(prm.sigma_normal))
                    wp = dm.tukey(np.abs(dm.dot3(n, p_q[cy, cx] - p)) / F(prm.sigma_plane))
                    wt = (k * wn) * wp
                    total = np.where(counts[..., None], total + wt[..., None] * c_q[cy, cx], total)
                    ws = np.where(counts, ws + wt, ws)
                    t["tap_off_image"] += int(np.sum(surface & ~inside))
                    t["tap_rejected_normal"] += int(np.sum(counts & (wn == 0)))
                    t["tap_rejected_plane"] += int(np.sum(counts & (wn > 0) & (wp == 0)))
                    t["zero_weight_tap_tx0"] += int(np.sum(counts & (k == 0) & ((tx == 0) | (ty == 0))))
            cg = total / ws[..., None]
            if prm.demodulate:
                cg = cg * a
            if prm.coverage:
                cg = cg * v[..., None]
            summed = surface & (ws > 0)
            guided = summed & finite3(cg)
            t["guided_not_finite"] += int(np.sum(summed & ~guided))
        ok_u, cu = unguided(valid_q, u_q, x0, y0, tx, ty)  # H5
        c = np.where(guided[..., None], cg, cu).astype(F)
        mask = np.where(guided, 1, np.where(ok_u, np.where(surface, 3, 2), 0))
        mask = np.where(weighted, mask, 0).astype(np.uint8)
        c = np.where(weighted[..., None], c, F(0.0)).astype(F)
        xyz = dm.rgb_to_xyz(c) * A[..., None]  # H6
        out = np.concatenate([np.where(weighted[..., None], xyz, F(0.0)), A[..., None]], -1).astype(F)
    t["guided"], t["unguided"], t["orphan"], t["nothing"] = (int(np.sum(mask == m)) for m in (1, 2, 3, 0))
    if tally is not None:
        tally.update(t)
    return (out, mask, c) if want_colour else (out, mask)


def geometry(hh, hw, ys, xs):
    """Analytic geometry at continuous full-size pixel coordinates (ys, xs): two planes meeting in a vertical step near the middle, a slanted floor strip at the bottom.
    Returns (n, p, albedo) Float32."""
    u, v = xs / F(hw), ys / F(hh)
    right = u > F(0.55)
    floor = v > F(0.8)
    n = np.where(right[..., None], np.array([0.6, 0.0, 0.8], F), np.array([0.0, 0.0, 1.0], F))
    n = np.where(floor[..., None], np.array([0.0, 1.0, 0.0], F), n).astype(F)
    n = n + np.stack([F(0.3) * (u - F(0.5)), F(0.3) * (v - F(0.5)), np.zeros_like(u)], -1).astype(F)  # a smooth bend: neighbours' normal weights lie inside (0, 1)
    n = (n / np.sqrt(dm.dot3(n, n))[..., None]).astype(F)
    z = np.where(right, F(2.0) - F(0.75) * (u - F(0.55)) * F(4.0), F(1.0))  # the step: z jumps from 1 to 2 at u = 0.55, then follows the right plane's slope
    z = np.where(floor, F(1.0) + (v - F(0.8)) * F(0.0), z)
    p = np.stack([u * F(4.0), np.where(floor, F(3.2), v * F(4.0)), np.where(floor, F(1.0) + (v - F(0.8)) * F(4.0), z)], -1).astype(F)
    albedo = np.where(right[..., None], np.array([0.25, 0.4, 0.85], F), np.array([0.8, 0.3, 0.2], F))
    albedo = np.where(floor[..., None], np.array([0.004, 0.9, 0.9], F), albedo).astype(F)
    return n, p, albedo


def low_window(hh, hw, lh, lw, lo_from_hi):
    """(y0, x0, rows, columns): the part of the low image that the full-size image's positions fall on (H3 in Float64, clipped to the low image; rows or columns may be 0).
    Without a map: the whole low image."""
    if lo_from_hi is None:
        return 0, 0, lh, lw
    ax, bx, ay, by = (float(F(v)) for v in lo_from_hi)
    x0, x1 = max(0, int(np.floor(bx))), min(lw, int(np.floor((hw - 1) * ax + bx)) + 2)
    y0, y1 = max(0, int(np.floor(by))), min(lh, int(np.floor((hh - 1) * ay + by)) + 2)
    return y0, x0, max(0, y1 - y0), max(0, x1 - x0)


def synthetic_pair(hh, hw, lh, lw, seed, lo_from_hi=None):
    """(lo_xyzw, lo_planes, hi_planes, lo_from_hi): the analytic geometry of `geometry` evaluated at the pixel centres of both resolutions (full frames of one camera, so the
    guides agree), a noisy low colour, and the cases that drive every branch: a stripe one full-size pixel wide that falls between low pixel centres (orphans), misses, pixels
    under min_coverage = 0.5, non-positive W and A, NaN and +-Inf in a low colour, a low normal, a low position and a full-size plane, and two neighbouring low colours near
    FLT_MAX whose guided sum overflows.  `lo_from_hi` = (ax, bx, ay, by): an explicit map instead of the one the sizes give (tests/upsample_maps.py); the low guides are then
    the geometry at (q - b) / a, and the planted low pixels sit in the part of the low image the full-size image falls on (`low_window`).  Without it the arrays are what
    they always were, bit for bit."""
    rng = np.random.default_rng(seed)
    explicit = lo_from_hi is not None
    wy, wx, wh, ww = low_window(hh, hw, lh, lw, lo_from_hi)
    if explicit:
        lo_from_hi = tuple(F(v) for v in lo_from_hi)
        ax, bx, ay, by = (float(v) for v in lo_from_hi)
    else:
        ax, ay = lw / hw, lh / hh
        bx, by = 1.5 * ax - 1.5, 1.5 * ay - 1.5
        lo_from_hi = (F(ax), F(bx), F(ay), F(by))  # full frames whose 1-based pixels start at 1 (docs/design/17-upscale.md): -0.75 at 2 x, 0 at ratio 1
    ys, xs = np.mgrid[0:hh, 0:hw].astype(F)
    n_h, p_h, alb_h = geometry(hh, hw, ys, xs)
    lys, lxs = np.mgrid[0:lh, 0:lw].astype(F)
    if explicit:
        n_l, p_l, alb_l = geometry(hh, hw, ((lys - F(by)) / F(ay)).astype(F), ((lxs - F(bx)) / F(ax)).astype(F))
    else:
        n_l, p_l, alb_l = geometry(hh, hw, ((lys + F(1.5)) / F(ay) - F(1.5)).astype(F), ((lxs + F(1.5)) / F(ax) - F(1.5)).astype(F))
    # the stripe: one full-size column on a plane of its own, between two low pixel centres (at ratio 1 there is no such column: any column then)
    between = (lambda x: x * ax + bx) if explicit else (lambda x: x * ax + 1.5 * ax - 1.5)
    sx = next((x for x in range(hw // 5, hw) if 0.3 < (between(x) % 1.0) < 0.7), hw // 5)
    if not explicit or hw >= 8:  # (a column image with a map keeps its guided pixels: the stripe would be all of it)
        n_h[:, sx], p_h[:, sx, 2] = np.array([0.0, 0.8, 0.6], F), p_h[:, sx, 2] - F(0.5)
    A_h = rng.uniform(0.6, 1.4, (hh, hw)).astype(F)
    cover_h = np.ones((hh, hw), F)
    cover_h[rng.random((hh, hw)) < 0.06] = F(0.3)
    cover_h[rng.random((hh, hw)) < 0.05] = F(0.75)
    miss_h = np.zeros((hh, hw), bool)
    miss_h[hh // 2:hh // 2 + 4, hw // 3:hw // 3 + 5] = True
    miss_h |= rng.random((hh, hw)) < 0.03
    cover_h[miss_h] = F(0.0)
    hi_planes = dm.planes_of(n_h, p_h, alb_h, A_h, (A_h * cover_h).astype(F))
    A_l = rng.uniform(0.6, 1.4, (lh, lw)).astype(F)
    cover_l = np.ones((lh, lw), F)
    cover_l[rng.random((lh, lw)) < 0.06] = F(0.3)
    cover_l[rng.random((lh, lw)) < 0.05] = F(0.75)
    miss_l = np.zeros((lh, lw), bool)
    my, mx = (max(0, int(np.floor(by))), max(0, int(np.floor(bx)))) if explicit else (0, 0)  # the low pixels under the full-size block of misses
    miss_l[my + int(hh // 2 * ay):my + int((hh // 2 + 4) * ay) + 1, mx + int(hw // 3 * ax):mx + int((hw // 3 + 5) * ax) + 1] = True
    cover_l[miss_l] = F(0.0)
    lo_planes = dm.planes_of(n_l, p_l, alb_l, A_l, (A_l * cover_l).astype(F))
    rgb = alb_l * (F(0.5) + rng.exponential(0.25, (lh, lw, 3)).astype(F)) * cover_l[..., None]
    rgb_to = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F)
    W_l = rng.uniform(0.6, 1.4, (lh, lw)).astype(F)
    lo_xyzw = np.concatenate([(rgb @ rgb_to.T) * W_l[..., None], W_l[..., None]], -1).astype(F)
    if wh >= 8 and ww >= 8 and hh >= 3 and hw >= 4:  # the poisoned pixels, away from each other
        lo_xyzw[wy + 1, wx + 2, 3] = F(0.0)               # W = 0
        lo_xyzw[wy + 2, wx + ww - 2, 3] = F(-1.0)         # W < 0
        lo_xyzw[wy + wh // 3, wx + ww // 2, 0] = F(np.nan)   # NaN colour
        lo_xyzw[wy + wh // 3 + 2, wx + 1, 1] = F(np.inf)     # +Inf colour
        lo_xyzw[wy + wh - 2, wx + 3, 2] = F(-np.inf)         # -Inf colour
        lo_planes[wy + wh // 2, wx + 1, 1, 0] = F(np.nan)    # NaN normal
        lo_planes[wy + wh // 2 + 2, wx + ww - 3, 2, 1] = F(np.inf)  # Inf position
        lo_planes[wy + 3, wx + ww // 2, 0, 3] = F(0.0)       # A = 0 in the low planes
        # two neighbours near FLT_MAX: grey 1e38 (every product of xyz_to_rgb stays finite) over a base colour of 0.3, so c = 3.3e38 is finite after Prepare and the guided
        # sum of the two, whose tent weights add up to 1.5 at radius 2, is not
        g, yb = F(1.0e38), wy + wh // 4
        for x in (wx + 1, wx + 2):
            lo_xyzw[yb, x] = np.array([F(0.412453) * g + F(0.357580) * g + F(0.180423) * g, g, F(0.019334) * g + F(0.119193) * g + F(0.950227) * g, F(1.0)], F)
            one = np.ones((1, 1), F)
            lo_planes[yb, x] = dm.planes_of(n_l[yb:yb + 1, x:x + 1], p_l[yb:yb + 1, x:x + 1], np.full((1, 1, 3), 0.3, F), one, one)[0, 0]
        hi_planes[1, 1, 0, 3] = F(0.0)            # A = 0
        hi_planes[2, hw - 2, 0, 3] = F(-0.5)      # A < 0
        hi_planes[hh // 3, hw // 4, 1, 2] = F(np.nan)   # NaN normal
        hi_planes[hh // 3 + 1, hw // 4, 2, 0] = F(-np.inf)  # -Inf position
        hi_planes[hh // 3 + 2, hw // 4, 0, 1] = F(np.inf)   # Inf base colour
    return lo_xyzw, lo_planes, hi_planes, lo_from_hi
