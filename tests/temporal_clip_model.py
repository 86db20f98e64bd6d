"""A numpy Float32 model of temporal reprojection with variance clipping of the history, written from its specification (docs/design/15-temporal-clip.md, which extends
docs/design/14-temporal.md): it imports the denoiser's and the temporal pass's models and nothing from the library.  Step 1 is the denoiser model's `prepare` without
demodulation; the window statistics are a Python loop over the window in the specified order (dy outer, dx inner), vectorised over pixels; steps 2-5 are the temporal model's
lines with the one new line of step 4'.  Every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_temporal_clip_api.py (CPU) checks the model's own properties — with gamma = +Inf it must equal temporal_model.accumulate in every bit —,
tests/test_gpu_temporal_clip.py compares the kernel with it bit for bit."""
from dataclasses import dataclass

import numpy as np

import denoise_model as dm
import temporal_model as tm

F = dm.F
count = tm.count


@dataclass
class Params(tm.Params):
    clip_gamma: float = 1.0
    clip_radius: int = 3


def window_bounds(surface, n, p, c, prm, tally=None):
    """(lo, hi), each (H, W, 3): mean -+ gamma * sd of the colours of the counting positions of every pixel's window.  Meaningful at surface pixels only.  `tally` receives,
    over surface pixels: window positions 'cut_left', 'cut_right', 'cut_top', 'cut_bottom' (outside the image past that edge), 'reject_flag', 'reject_normal', 'reject_plane'
    (inside, in that order of tests), 'counted' (off-centre positions that count); pixels 'cnt_one' (nothing but the centre counted); channels 'var_floored' (var > 0 false)."""
    h, w = surface.shape
    R, gamma = int(prm.clip_radius), F(prm.clip_gamma)
    assert R in (1, 2, 3) and gamma >= 0
    ys, xs = np.arange(h)[:, None] + np.zeros((1, w), np.int64), np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    m1, m2, cnt = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            qy, qx = ys + dy, xs + dx
            if dy == 0 and dx == 0:
                counts = np.ones((h, w), bool)
            else:
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                for name, m in (("cut_left", qx < 0), ("cut_right", qx >= w), ("cut_top", qy < 0), ("cut_bottom", qy >= h)):
                    count(tally, name, surface & m)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                ok_flag = surface[qy, qx]
                ok_normal = (F(1.0) - dm.dot3(n, n[qy, qx])) < F(prm.sigma_normal)
                ok_plane = np.abs(dm.dot3(n, p[qy, qx] - p)) < F(prm.sigma_plane)
                live = surface & inside
                count(tally, "reject_flag", live & ~ok_flag)
                count(tally, "reject_normal", live & ok_flag & ~ok_normal)
                count(tally, "reject_plane", live & ok_flag & ok_normal & ~ok_plane)
                counts = inside & ok_flag & ok_normal & ok_plane
                count(tally, "counted", surface & counts)
            c_q = c[qy, qx]
            m1 = np.where(counts[..., None], m1 + c_q, m1)
            m2 = np.where(counts[..., None], m2 + c_q * c_q, m2)
            cnt = np.where(counts, cnt + F(1.0), cnt)
    count(tally, "cnt_one", surface & (cnt == 1))
    mean = m1 / cnt[..., None]
    var = m2 / cnt[..., None] - mean * mean
    count(tally, "var_floored", surface[..., None] & ~(var > 0))
    var = np.where(var > 0, var, F(0.0)).astype(F)
    sd = np.sqrt(var)
    lo = mean - gamma * sd
    hi = mean + gamma * sd
    return lo.astype(F), hi.astype(F)


def accumulate(B, P, history, M, prm, tally=None):
    """(out_xyzw (H, W, 4), out_history (H, W, 3, 4)), as temporal_model.accumulate with step 4'.  `tally` receives window_bounds' names and, over the channels of the pixels
    that have a history colour (sb > 0): 'clipped_low', 'clipped_high', 'inside'; over those pixels: 'pixels_clipped' (a channel clipped), 'pixels_inside' (none); and
    'blended', 'nan_colour' as in the temporal model."""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    assert B.ndim == 3 and B.shape[2] == 4 and P.shape == B.shape[:2] + (3, 4)
    h, w = B.shape[:2]
    with np.errstate(all="ignore"):
        surface, n, p, c, _, _, W = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=False, min_coverage=prm.min_coverage))
        count(tally, "surface", surface)
        lo, hi = window_bounds(surface, n, p, c, prm, tally)
        c_new, N_new = c, np.ones((h, w), F)
        if history is not None:
            Hs = np.ascontiguousarray(history, F)
            assert Hs.shape == P.shape
            hx, hy, hz = tm.project(M, p)
            front = surface & (hz > 0)
            fx, fy = hx / hz, hy / hz
            pos = front & (np.abs(fx) < tm.MAX_POSITION) & (np.abs(fy) < tm.MAX_POSITION)
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ix, iy = np.where(pos, x0, 0).astype(np.int64), np.where(pos, y0, 0).astype(np.int64)
            sc, sN, sb = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    q = Hs[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                    b = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                    accepted = (pos & inside & (q[..., 1, 3] == F(1.0)) & (q[..., 0, 3] > 0) & ((F(1.0) - dm.dot3(n, q[..., 1, :3])) < F(prm.sigma_normal))
                                & (np.abs(dm.dot3(n, q[..., 2, :3] - p)) < F(prm.sigma_plane)))
                    sc = np.where(accepted[..., None], sc + b[..., None] * q[..., 0, :3], sc)
                    sN = np.where(accepted, sN + b * q[..., 0, 3], sN)
                    sb = np.where(accepted, sb + b, sb)
            blend = pos & (sb > 0)
            c_h, N_h = sc / sb[..., None], sN / sb
            below, above = c_h < lo, c_h > hi  # step 4': comparisons with NaN are false
            count(tally, "clipped_low", blend[..., None] & below)
            count(tally, "clipped_high", blend[..., None] & ~below & above)
            count(tally, "inside", blend[..., None] & ~below & ~above)
            count(tally, "pixels_clipped", blend & (below | above).any(-1))
            count(tally, "pixels_inside", blend & ~(below | above).any(-1))
            c_h = np.where(below, lo, np.where(above, hi, c_h)).astype(F)
            N_1 = N_h + F(1.0)
            N_b = np.where(N_1 < F(prm.max_history), N_1, F(prm.max_history)).astype(F)
            a = F(1.0) / N_b
            c_b = c_h + a[..., None] * (c - c_h)
            finite = np.isfinite(c_b).all(-1)
            count(tally, "nan_colour", blend & ~finite)
            blend &= finite
            count(tally, "blended", blend)
            c_new = np.where(blend[..., None], c_b, c).astype(F)
            N_new = np.where(blend, N_b, F(1.0)).astype(F)
        xyz = dm.rgb_to_xyz(c_new) * W[..., None]
    out = B.copy()
    out[surface, :3] = xyz[surface]
    out_history = np.zeros((h, w, 3, 4), F)
    out_history[surface, 0, :3], out_history[surface, 0, 3] = c_new[surface], N_new[surface]
    out_history[surface, 1, :3], out_history[surface, 1, 3] = n[surface], F(1.0)
    out_history[surface, 2, :3] = p[surface]
    return out, out_history


# ---- the synthetic case of the tests: tm.synthetic's frame, history and matrix with poisoned neighbours added ------------------------------------------------------------
BRANCHES = ("clipped_low", "clipped_high", "inside", "cut_left", "cut_right", "cut_top", "cut_bottom", "reject_flag", "reject_normal", "reject_plane", "cnt_one", "var_floored")


def params(gamma, radius):
    s = tm.SYNTHETIC_PARAMS
    return Params(s.max_history, s.sigma_normal, s.sigma_plane, s.min_coverage, gamma, radius)


def synthetic(h, w, seed):
    """(B, P, history, M).  h, w >= 16: tm.synthetic(h, w, seed) with tm.SYNTHETIC_M, and among the neighbours of its pixels, every 23rd pixel in turn: a NaN colour, a pixel
    that is no surface pixel (W = 0), a flipped normal, a position 5 units off its plane; and two patches of one exactly representable colour with the neighbours all round
    them taken away (the window then holds the centre alone, or equal colours: cnt == 1, var == 0).
    Smaller sizes (no film of tm.synthetic is that small): the window [8:8+h, 8:8+w] of synthetic(29, 37, seed), with the matrix's translation moved so that the window
    reprojects onto itself as the whole film does (stretched by 1.6 and 1.2 about a point near its corner)."""
    if h < 16 or w < 16:
        B, P, Hs, M = synthetic(29, 37, seed)
        M = M.copy()
        M[0, 3], M[1, 3] = F(-16.0 * 0.8 - 0.5), F(-12.0 * 0.8 - 0.25)
        return B[8:8 + h, 8:8 + w].copy(), P[8:8 + h, 8:8 + w].copy(), Hs[8:8 + h, 8:8 + w].copy(), M
    B, P, Hs = tm.synthetic(h, w, seed)
    flat = np.arange(h * w).reshape(h, w)
    kind = np.where(flat % 23 == 0, (flat // 23) % 4, -1)
    B[kind == 0, 1] = F(np.nan)
    B[kind == 1, 3] = F(0.0)
    P[kind == 2, 1, :3] *= F(-1.0)
    P[kind == 3, 2, :3] += F(5.0) * P[kind == 3, 1, :3]
    for (y, x), rgb in (((4, 5), (0.5, 0.25, 0.125)), ((h - 6, w - 7), (2.0, 1.0, 0.5))):
        # a 2 x 1 patch of one dyadic colour (weights 1: the colour survives XYZ -> RGB only approximately, but both pixels hold the same bits) inside a ring of misses 3 wide
        B[y - 3:y + 4, x - 3:x + 5, 3] = F(0.0)
        for xx in (x, x + 1):
            tm.set_exact_pixel(B, P, y, xx, [0.1 * xx, 0.1 * y, 0.0])
            B[y, xx, :3] = dm.rgb_to_xyz(F(rgb))
    tm.set_exact_pixel(B, P, h // 2, w // 2, [0.1 * (w // 2), 0.1 * (h // 2), 0.0])
    B[h // 2 - 3:h // 2 + 4, w // 2 - 3:w // 2 + 4, 3] = np.where(np.arange(7)[:, None] * 7 + np.arange(7)[None, :] == 24, B[h // 2, w // 2, 3], F(0.0))  # a pixel alone in its window
    return B, P, Hs, tm.SYNTHETIC_M.copy()
