"""A numpy Float32 model of the two variance passes, written from their specification (docs/design/16-variance.md): the reprojection that carries luminance moments and returns
a variance plane (trhip_temporal_moments) and the à-trous filter whose colour sigma comes from that plane (trhip_denoise_var).  It imports the denoiser's, the temporal pass's
and the clipping pass's models and nothing from the library: Prepare, the colour functions, the projection and Tukey's weight are theirs, and the colour and the history of the
moments pass ARE temporal_model.accumulate's outputs.  What is written here is what is new: the moments along the taps, the luminance window, the variance-driven iteration.
Vectorised over pixels, Python loops over taps and windows in the specified order; every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_variance_api.py (CPU) checks the model's own properties, tests/test_gpu_variance.py compares the kernels with it bit for bit."""
from dataclasses import dataclass

import numpy as np

import denoise_model as dm
import temporal_clip_model as cm
import temporal_model as tm

F = dm.F
count = tm.count
RADIUS = 3  # the window of the spatial estimate: the clipping pass's at R = 3
G = (F(0.5), F(0.25))


@dataclass
class MomentsParams(tm.Params):
    albedo_floor: float = 1.0 / 64.0
    spatial_below: float = 4.0
    demodulate: bool = True


@dataclass
class VarParams(dm.Params):
    var_eps: float = 1.0 / 64.0


def luminance(B, P, prm):
    """(surface, n, p, Yd): the temporal pass's surface pixels (Prepare without demodulation) and the luminance the denoiser compares at them."""
    base = dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=False, min_coverage=prm.min_coverage)
    surface, n, p, c, _, _, _ = dm.prepare(B, P, base)
    if prm.demodulate:
        a = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=True, albedo_floor=prm.albedo_floor, min_coverage=prm.min_coverage))[5]
        c = c / a
    return surface, n, p, dm.to_Y(c)


def spatial_variance(surface, n, p, Yd, prm, tally=None):
    """vs (H, W): the clipping pass's window walk at R = 3 on the luminance.  The positions that count are window_bounds': the centre, and a position inside the image that is
    a surface pixel with 1 - n.n_q < sigma_normal and |n.(p_q - p)| < sigma_plane."""
    h, w = surface.shape
    ys, xs = np.arange(h)[:, None] + np.zeros((1, w), np.int64), np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    S1, S2, cnt = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            qy, qx = ys + dy, xs + dx
            if dy == 0 and dx == 0:
                counts = np.ones((h, w), bool)
            else:
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                count(tally, "window_cut", surface & ~inside)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                counts = (inside & surface[qy, qx] & ((F(1.0) - dm.dot3(n, n[qy, qx])) < F(prm.sigma_normal)) & (np.abs(dm.dot3(n, p[qy, qx] - p)) < F(prm.sigma_plane)))
                count(tally, "window_rejected", surface & inside & ~counts)
            Y_q = Yd[qy, qx]
            S1 = np.where(counts, S1 + Y_q, S1)
            S2 = np.where(counts, S2 + Y_q * Y_q, S2)
            cnt = np.where(counts, cnt + F(1.0), cnt)
    mean = S1 / cnt
    var = S2 / cnt - mean * mean
    count(tally, "spatial_floored", surface & ~(var > 0))
    return np.where(var > 0, var, F(0.0)).astype(F)


def accumulate(B, P, history, moments, M, prm, tally=None):
    """(out_xyzw (H, W, 4), out_history (H, W, 3, 4), out_moments (H, W, 2), out_variance (H, W)).  `tally` receives, over surface pixels: 'temporal' / 'spatial' (which
    estimate the variance is), 'short' (a history, N' < spatial_below), 'colour_restart' (the blend was not finite), 'moments_restart' (m1' or m2' was not), 'no_taps',
    'moments_zeroed' (Yd or its square not finite), 'variance_zeroed' (v / N' not finite), 'temporal_floored', and the window's names."""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    h, w = B.shape[:2]
    assert (history is None) == (moments is None)
    out, out_history = tm.accumulate(B, P, history, M, prm)  # steps 1-5, untouched
    with np.errstate(all="ignore"):
        surface, n, p, Yd = luminance(B, P, prm)
        N_new = out_history[..., 0, 3]
        m1, m2 = Yd, Yd * Yd
        vt, have_vt = np.zeros((h, w), F), np.zeros((h, w), bool)
        if history is not None:
            Hs, Ms = np.ascontiguousarray(history, F), np.ascontiguousarray(moments, F)
            assert Hs.shape == P.shape and Ms.shape == (h, w, 2)
            hx, hy, hz = tm.project(M, p)
            fx, fy = hx / hz, hy / hz
            pos = surface & (hz > 0) & (np.abs(fx) < tm.MAX_POSITION) & (np.abs(fy) < tm.MAX_POSITION)
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ix, iy = np.where(pos, x0, 0).astype(np.int64), np.where(pos, y0, 0).astype(np.int64)
            c = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=False, min_coverage=prm.min_coverage))[3]
            sc, sN, s1, s2, sb = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    q, mq = Hs[qy, qx], Ms[qy, qx]
                    b = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                    accepted = (pos & inside & (q[..., 1, 3] == F(1.0)) & (q[..., 0, 3] > 0) & ((F(1.0) - dm.dot3(n, q[..., 1, :3])) < F(prm.sigma_normal))
                                & (np.abs(dm.dot3(n, q[..., 2, :3] - p)) < F(prm.sigma_plane)))
                    sc = np.where(accepted[..., None], sc + b[..., None] * q[..., 0, :3], sc)  # (step 4's two sums again, only to know where it restarted)
                    sN = np.where(accepted, sN + b * q[..., 0, 3], sN)
                    s1 = np.where(accepted, s1 + b * mq[..., 0], s1)
                    s2 = np.where(accepted, s2 + b * mq[..., 1], s2)
                    sb = np.where(accepted, sb + b, sb)
            taps = pos & (sb > 0)
            count(tally, "no_taps", surface & ~taps)
            c_h, N_1 = sc / sb[..., None], sN / sb + F(1.0)
            N_b = np.where(N_1 < F(prm.max_history), N_1, F(prm.max_history)).astype(F)
            a_N = F(1.0) / N_b
            restart = taps & ~np.isfinite(c_h + a_N[..., None] * (c - c_h)).all(-1)  # step 4's fallback: c' = c, N' = 1
            assert np.array_equal(np.where(taps & ~restart, N_b, F(1.0))[surface], N_new[surface]), "the history lengths are the temporal model's"
            count(tally, "colour_restart", restart)
            m1_h, m2_h = s1 / sb, s2 / sb
            b1 = m1_h + a_N * (Yd - m1_h)
            b2 = m2_h + a_N * (Yd * Yd - m2_h)
            ok = taps & ~restart & np.isfinite(b1) & np.isfinite(b2)
            count(tally, "moments_restart", taps & ~restart & ~ok)
            m1, m2 = np.where(ok, b1, m1).astype(F), np.where(ok, b2, m2).astype(F)
            var = m2 - m1 * m1
            count(tally, "temporal_floored", ok & ~(var > 0))
            vt = np.where(var > 0, var, F(0.0)).astype(F)
            have_vt = ok
        vs = spatial_variance(surface, n, p, Yd, prm, tally)
        short = N_new < F(prm.spatial_below)
        count(tally, "short", surface & have_vt & short)
        temporal = have_vt & ~short
        count(tally, "temporal", surface & temporal)
        count(tally, "spatial", surface & ~temporal)
        v = np.where(temporal, vt, vs).astype(F)
        finite = np.isfinite(m1) & np.isfinite(m2)
        count(tally, "moments_zeroed", surface & ~finite)
        m1, m2 = np.where(finite, m1, F(0.0)).astype(F), np.where(finite, m2, F(0.0)).astype(F)
        vn = v / N_new
        count(tally, "variance_zeroed", surface & ~np.isfinite(vn))
        vn = np.where(np.isfinite(vn), vn, F(0.0)).astype(F)
    out_moments = np.zeros((h, w, 2), F)
    out_moments[surface, 0], out_moments[surface, 1] = m1[surface], m2[surface]
    out_variance = np.where(surface, vn, F(0.0)).astype(F)
    return out, out_history, out_moments, out_variance


def seed_variance(surface, variance):
    with np.errstate(all="ignore"):
        v = np.ascontiguousarray(variance, F)
        return np.where(surface, np.where(v > 0, v, F(0.0)), F(-1.0)).astype(F)


def denoise(B, P, variance, prm, tally=None):
    """(out_xyzw (H, W, 4), out_variance (H, W)).  `tally` receives 'colour' [pairs with weight exactly 0, pairs strictly between 0 and 1] over valid off-centre taps, and
    'nan_variance' (a V_{i+1} that was NaN and is stored as 0), 'inf_sigma' (pixels whose sig was +Inf)."""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    assert B.ndim == 3 and B.shape[2] == 4 and P.shape == B.shape[:2] + (3, 4) and 0 <= prm.iterations <= 6
    h, w = B.shape[:2]
    with np.errstate(all="ignore"):
        surface, n, p, c, Y, a, W = dm.prepare(B, P, prm)
        V = seed_variance(surface, variance)  # -1 where the pixel is no surface pixel: such a position never counts
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for i in range(prm.iterations):
            s = 1 << i
            gs, gw = np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = ys + dy, xs + dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    counts = inside & surface[qy, qx]
                    g = G[abs(dy)] * G[abs(dx)]
                    gs = np.where(counts, gs + g * V[qy, qx], gs)
                    gw = np.where(counts, gw + g, gw)
            gv = gs / gw
            sd = np.sqrt(gv)
            sig = F(prm.sigma_colour) * sd + F(prm.var_eps)
            count(tally, "inf_sigma", surface & np.isinf(sig))
            total, ws, vsum = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    valid = surface & inside & surface[qy, qx]
                    k = dm.K[abs(dy)] * dm.K[abs(dx)]
                    wn = dm.tukey((F(1.0) - dm.dot3(n, n[qy, qx])) / F(prm.sigma_normal))
                    wp = dm.tukey(np.abs(dm.dot3(n, p[qy, qx] - p)) / F(prm.sigma_plane))
                    wc = dm.tukey(np.abs(Y[qy, qx] - Y) / sig)
                    wt = ((k * wn) * wp) * wc
                    total = np.where(valid[..., None], total + wt[..., None] * c[qy, qx], total)
                    ws = np.where(valid, ws + wt, ws)
                    vsum = np.where(valid, vsum + (wt * wt) * V[qy, qx], vsum)
                    if tally is not None and (dy or dx):
                        t = tally.setdefault("colour", [0, 0])
                        t[0] += int(np.sum(valid & (wc == 0)))
                        t[1] += int(np.sum(valid & (wc > 0) & (wc < 1)))
            c = np.where(surface[..., None], total / ws[..., None], c).astype(F)
            Y = dm.to_Y(c)
            vn = vsum / (ws * ws)
            count(tally, "nan_variance", surface & np.isnan(vn))
            V = np.where(surface, np.where(vn > 0, vn, F(0.0)), F(-1.0)).astype(F)
        if prm.demodulate:
            c = c * a
        xyz = dm.rgb_to_xyz(c) * W[..., None]
    out = B.copy()
    if prm.iterations:
        out[surface, :3] = xyz[surface]
    return out, np.where(V > 0, V, F(0.0)).astype(F)


# ---- the synthetic cases of the tests -------------------------------------------------------------------------------------------------------------------------------
def moments_params(demodulate, spatial_below=4.0):
    s = tm.SYNTHETIC_PARAMS
    return MomentsParams(s.max_history, s.sigma_normal, s.sigma_plane, s.min_coverage, 1.0 / 64.0, spatial_below, demodulate)


def synthetic_moments(h, w, seed):
    """(B, P, history, moments, M): cm.synthetic's frame, history and matrix (NaN history colours, lengths of 1..12 — they straddle spatial_below = 4 from lane to lane —,
    non-surface pixels inside windows, reprojections off every edge, patches of one dyadic colour), one pixel of luminance 1e20, and moments to go with the history: plausible ones (a mean near the
    history colour's luminance, a second moment above its square), every 19th pixel poisoned in turn with a NaN m1, an Inf m2, a negative m2."""
    B, P, Hs, M = cm.synthetic(h, w, seed)
    if h >= 16:  # a colour whose luminance is finite and whose square is not: no moments are kept of it, and a window that holds it has no finite variance
        y, x = h // 3, w // 3
        tm.set_exact_pixel(B, P, y, x, [0.1 * x, 0.1 * y, 0.0])
        B[y, x, :3] = dm.rgb_to_xyz(np.full(3, 1.0e20, F))
    rng = np.random.default_rng(seed + 5)
    with np.errstate(all="ignore"):
        Yh = dm.to_Y(np.nan_to_num(Hs[..., 0, :3], nan=0.5, posinf=1.0, neginf=0.0))
    Ms = np.stack([Yh, Yh * Yh + rng.uniform(0.0, 0.2, (h, w)).astype(F)], -1).astype(F)
    flat = np.arange(h * w).reshape(h, w)
    kind = np.where(flat % 19 == 7, (flat // 19) % 3, -1)
    Ms[kind == 0, 0] = F(np.nan)
    Ms[kind == 1, 1] = F(np.inf)
    Ms[kind == 2, 1] = F(-1.0)
    Ms[Hs[..., 1, 3] != 1] = F(0.0)
    return B, P, Hs, Ms, M


def synthetic_steady(h, w, seed, split=24):
    """(B, P, history, moments, M) of a steady-state frame: a plane seen head-on whose positions are the pixel indices, every weight 1, noisy colours, under the identity
    reprojection (every pixel's own record is its first tap with weight 1, the other three weigh 0), with histories of length 6 left of column `split` and 1 from it on.
    With spatial_below = 4 the pixels left of it take the temporal estimate (N' = 7) and the others the spatial one (N' = 2): at split = 24 the 16 x 4 patches of columns
    0..15 need no window walk, those of columns 16..31 need it for half their lanes, the rest for all."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    ones = np.ones((h, w), F)
    n = np.zeros((h, w, 3), F)
    n[..., 2] = 1
    p = np.stack([xs, ys, np.zeros((h, w))], -1).astype(F)
    albedo = rng.uniform(0.2, 0.9, (h, w, 3)).astype(F)
    P = dm.planes_of(n, p, albedo, ones, ones)
    rgb = (albedo * rng.uniform(0.3, 1.5, (h, w, 3))).astype(F)
    B = np.concatenate([dm.rgb_to_xyz(rgb), ones[..., None]], -1).astype(F)
    Hs = np.zeros((h, w, 3, 4), F)
    Hs[..., 0, :3], Hs[..., 0, 3] = (albedo * rng.uniform(0.3, 1.5, (h, w, 3))).astype(F), np.where(xs < split, F(6.0), F(1.0))
    Hs[..., 1, :3], Hs[..., 1, 3] = n, F(1.0)
    Hs[..., 2, :3] = p
    Yh = rng.uniform(0.5, 1.2, (h, w)).astype(F)
    Ms = np.stack([Yh, Yh * Yh + rng.uniform(0.0, 0.2, (h, w)).astype(F)], -1).astype(F)
    return B, P, Hs, Ms, F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])


def synthetic_variance(h, w, seed, kind):
    """A variance plane for dm.synthetic(h, w, seed): 'zero', 'one', 'random' (0 .. 0.5, squared: many small, a few large), 'poisoned' (random with NaN, +Inf, -Inf and
    negative entries, one in seven pixels)."""
    rng = np.random.default_rng(seed + 900)
    if kind == "zero":
        return np.zeros((h, w), F)
    if kind == "one":
        return np.ones((h, w), F)
    v = (rng.uniform(0.0, 0.7, (h, w)) ** 2).astype(F)
    if kind == "poisoned":
        flat = np.arange(h * w).reshape(h, w)
        for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.25)):
            v[flat % 28 == 7 * k + 3] = F(bad)
    return v
