"""A numpy Float32 model of the temporal upsampling pass, written from its specification (docs/design/19-temporal-upsample.md): it imports nothing from the library.  Part U
is the upscaler's model (upscale_model: the low records, the positions, the colour and the class come from it) with one more tap loop for the confidence; part T is the
temporal model's projection (temporal_model.project) and its tap order, with the accumulated weight in the place of the history length.  Vectorised over full-size pixels;
every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_temporal_upsample_api.py (CPU) checks the model's own properties, tests/test_gpu_temporal_upsample.py compares the kernel with it bit for bit."""
from dataclasses import dataclass

import numpy as np

import denoise_model as dm
import temporal_model as tm
import upscale_model as um

F = np.float32
TALLY_KEYS = ("guided", "orphan", "unguided", "nothing", "nothing_on_surface", "kmax_below_floor", "kmax_above_floor", "behind", "non_finite", "integer_x", "integer_y",
              "all_rejected", "blended", "capped", "below_cap", "nan_colour", "orphan_with_history", "orphan_without_history", "tap_off_image", "tap_reject_flag",
              "tap_reject_weight", "tap_reject_normal", "tap_reject_plane", "tap_accepted")


@dataclass
class Params:
    lo_from_hi: tuple  # (ax, bx, ay, by)
    radius: int = 2
    max_history: float = 8.0
    sigma_normal: float = 0.25
    sigma_plane: float = 0.1
    min_coverage: float = 0.5
    guide_sigma_normal: float = 0.25
    guide_sigma_plane: float = 0.4
    confidence_floor: float = 0.25
    confidence_sharpness: float = 2.0


def upscale_params(prm):
    """The upscaler's parameters of part U: both flags off."""
    return um.Params(prm.lo_from_hi, radius=prm.radius, demodulate=False, coverage=False, sigma_normal=prm.guide_sigma_normal, sigma_plane=prm.guide_sigma_plane,
                     min_coverage=prm.min_coverage)


def distance(i, t):
    """The distance inside um.tent."""
    return t + F(-i) if i <= 0 else F(i) - t


def sharp(d, rho):
    g = F(1.0) - d * rho
    return np.where(g > 0, g, F(0.0)).astype(F)


def surface_and_confidence(lo_xyzw, lo_planes, hi_planes, prm, records=None):
    """(surface, n, p, kmax) of every full-size pixel: H2 of 17-upscale.md with the flags off, and the largest e = ((gy gx) wn) wp over the accepted guided taps.
    `records`: what um.low_records returns for these frames and upscale_params(prm), given instead of computed."""
    up = upscale_params(prm)
    PH = np.ascontiguousarray(hi_planes, F)
    h, w = PH.shape[:2]
    lh, lw = lo_xyzw.shape[:2]
    R, rho = prm.radius, F(prm.confidence_sharpness)
    with np.errstate(all="ignore"):
        s_q, n_q, p_q, _, _, _ = um.low_records(np.ascontiguousarray(lo_xyzw, F), np.ascontiguousarray(lo_planes, F), up) if records is None else records
        A, H = PH[..., 0, 3], PH[..., 1, 3]
        surface = (H > 0) & (H >= F(prm.min_coverage) * A)
        iH = F(1.0) / H
        n = PH[..., 1, :3] * iH[..., None]
        length = np.sqrt(dm.dot3(n, n))
        surface &= length > 0
        n = n / length[..., None]
        p = PH[..., 2, :3] * iH[..., None]
        surface &= um.finite3(n) & um.finite3(p)
        surface &= A > 0
        x0, y0, tx, ty = um.positions(up, h, w)
        kmax = np.zeros((h, w), F)
        for j in range(1 - R, R + 1):
            gy = sharp(distance(j, ty), rho)
            for i in range(1 - R, R + 1):
                gx = sharp(distance(i, tx), rho)
                g = gy * gx
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
                cx, cy = np.clip(qx, 0, lw - 1), np.clip(qy, 0, lh - 1)
                counts = surface & inside & s_q[cy, cx]
                wn = dm.tukey((F(1.0) - dm.dot3(n, n_q[cy, cx])) / F(prm.guide_sigma_normal))
                wp = dm.tukey(np.abs(dm.dot3(n, p_q[cy, cx] - p)) / F(prm.guide_sigma_plane))
                e = (g * wn) * wp
                kmax = np.where(counts & (e > kmax), e, kmax).astype(F)
    n = np.where(surface[..., None], n, F(0.0)).astype(F)
    p = np.where(surface[..., None], p, F(0.0)).astype(F)
    return surface, n, p, kmax


def accumulate(lo_xyzw, lo_planes, hi_planes, history, M, prm, tally=None):
    """(out_xyzw (h, w, 4), out_history (h, w, 3, 4), out_mask (h, w) uint8).  history: the previous frame's out_history at full size or None; M: the previous full-size
    camera's 3 x 4 matrix.  `tally`, a dict, receives how many pixels or history taps took each branch (TALLY_KEYS)."""
    t = dict.fromkeys(TALLY_KEYS, 0)
    count = lambda name, m: tm.count(t, name, m)  # noqa: E731
    PH = np.ascontiguousarray(hi_planes, F)
    h, w = PH.shape[:2]
    A = PH[..., 0, 3]
    # U: colour and class are the upscaler's
    records = um.low_records(np.ascontiguousarray(lo_xyzw, F), np.ascontiguousarray(lo_planes, F), upscale_params(prm))  # once for both halves of part U
    up_out, m, c = um.upscale(lo_xyzw, lo_planes, PH, upscale_params(prm), want_colour=True, records=records)
    surface, n, p, kmax = surface_and_confidence(lo_xyzw, lo_planes, PH, prm, records)
    assert not (np.isin(m, (1, 3)) & ~surface).any() and not ((m == 2) & surface).any(), "H2 here is not the upscaler's"
    assert not ((m == 1) & ~(kmax >= 0)).any()
    k0 = F(prm.confidence_floor)
    kappa = np.where(m == 1, np.where(kmax > k0, kmax, k0), np.where(m == 3, k0, F(0.0))).astype(F)
    count("guided", m == 1), count("orphan", m == 3), count("unguided", m == 2), count("nothing", (m == 0) & ~surface), count("nothing_on_surface", (m == 0) & surface)
    count("kmax_below_floor", (m == 1) & ~(kmax > k0)), count("kmax_above_floor", (m == 1) & (kmax > k0))
    with np.errstate(all="ignore"):
        c_new, O_new, found = c, kappa, np.zeros((h, w), bool)
        if history is not None:
            Hs = np.ascontiguousarray(history, F)
            assert Hs.shape == PH.shape
            hx, hy, hz = tm.project(M, p)
            front = surface & (hz > 0)
            count("behind", surface & ~front)
            fx, fy = hx / hz, hy / hz
            pos = front & (np.abs(fx) < tm.MAX_POSITION) & (np.abs(fy) < tm.MAX_POSITION)
            count("non_finite", front & ~pos)
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            count("integer_x", pos & (tx == 0)), count("integer_y", pos & (ty == 0))
            ix, iy = np.where(pos, x0, 0).astype(np.int64), np.where(pos, y0, 0).astype(np.int64)
            sc, sO, sb = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    q = Hs[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                    b = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                    live = pos & inside
                    ok_flag = q[..., 1, 3] == F(1.0)
                    ok_weight = q[..., 0, 3] > 0
                    ok_normal = (F(1.0) - dm.dot3(n, q[..., 1, :3])) < F(prm.sigma_normal)
                    ok_plane = np.abs(dm.dot3(n, q[..., 2, :3] - p)) < F(prm.sigma_plane)
                    count("tap_off_image", pos & ~inside)
                    count("tap_reject_flag", live & ~ok_flag)
                    count("tap_reject_weight", live & ok_flag & ~ok_weight)
                    count("tap_reject_normal", live & ok_flag & ok_weight & ~ok_normal)
                    count("tap_reject_plane", live & ok_flag & ok_weight & ok_normal & ~ok_plane)
                    accepted = live & ok_flag & ok_weight & ok_normal & ok_plane
                    count("tap_accepted", accepted)
                    sc = np.where(accepted[..., None], sc + b[..., None] * q[..., 0, :3], sc)
                    sO = np.where(accepted, sO + b * q[..., 0, 3], sO)
                    sb = np.where(accepted, sb + b, sb)
            found = pos & (sb > 0)
            count("all_rejected", pos & ~found)
            c_h, O_h = sc / sb[..., None], sO / sb
            O_1 = O_h + kappa
            O_b = np.where(O_1 < F(prm.max_history), O_1, F(prm.max_history)).astype(F)
            a = kappa / O_b
            c_b = c_h + a[..., None] * (c - c_h)
            finite = np.isfinite(c_b).all(-1)
            count("nan_colour", found & ~finite)
            blend = found & finite
            count("blended", blend)
            count("capped", blend & (O_b == F(prm.max_history))), count("below_cap", blend & (O_b < F(prm.max_history)))
            c_new = np.where(blend[..., None], c_b, c).astype(F)
            O_new = np.where(blend, O_b, kappa).astype(F)
        count("orphan_with_history", (m == 3) & found), count("orphan_without_history", (m == 3) & ~found)
        xyz = dm.rgb_to_xyz(c_new) * A[..., None]
    out = up_out.copy()
    out[surface, :3] = xyz[surface]
    out_history = np.zeros((h, w, 3, 4), F)
    out_history[surface, 0, :3], out_history[surface, 0, 3] = c_new[surface], O_new[surface]
    out_history[surface, 1, :3], out_history[surface, 1, 3] = n[surface], F(1.0)
    out_history[surface, 2, :3] = p[surface]
    out_mask = (m + 4 * (found & surface)).astype(np.uint8)
    assert np.array_equal(out_mask & 3, m) and np.array_equal(out[..., 3].view(np.uint32), up_out[..., 3].view(np.uint32))
    if history is None:
        assert np.array_equal(out_mask, m)
    if tally is not None:
        tally.update(t)
    return out, out_history, out_mask


# ---- the synthetic case of the tests: a pair of frames, a full-size history and a matrix that between them take every branch ------------------------------------------
def set_exact_pixel(P, y, x, p):
    """Gives full-size pixel (y, x) the weights 1, 1, so that the position the pass recovers is `p` to the bit."""
    P[y, x, 0] = F([0.5, 0.5, 0.5, 1.0])
    P[y, x, 1] = F([0.0, 0.0, 1.0, 1.0])
    P[y, x, 2, :3], P[y, x, 2, 3] = F(p), F(1.0)


def synthetic_matrix(hh, hw, lo_from_hi):
    """um.geometry's points are (4 x / hw, 4 y / hh or 3.2, z in [0.5, 2]): the matrix stretches the image by about 1.05 and 1.03 and adds a mild perspective in z, so that
    the displacement between a pixel and its reprojected position grows from a few pixels one way to a few the other, off two edges; the offsets are whole numbers (integer
    points reproject to integer positions) chosen so that the stripe of orphans, which has z = 0.5, comes back near itself."""
    ax, bx = float(lo_from_hi[0]), float(lo_from_hi[1])
    sx = next((x for x in range(hw // 5, hw) if 0.3 < ((x * ax + bx) % 1.0) < 0.7), hw // 5)  # um.synthetic_pair's stripe
    m00, m11 = float(max(1, round(hw * 1.1 / 4))), float(max(1, round(hh * 1.08 / 4)))
    m03 = float(round(sx * 1.03125 - m00 * 4.0 * sx / hw))
    return np.array([[m00, 0.0, 0.0, m03], [0.0, m11, 0.0, -1.0], [0.0, 0.0, 0.0625, 1.0]], F)


def synthetic(hh, hw, lh, lw, seed, lo_from_hi=None):
    """`lo_from_hi`: an explicit map, handed to um.synthetic_pair (the block of weight 0 then lies in um.low_window); without it, today's arrays bit for bit.
    (lo_xyzw, lo_planes, hi_planes, lo_from_hi, history, M): um.synthetic_pair's frames with a block of 4 x 4 low pixels of weight 0 (full-size surface pixels nothing
    is found for), groups of full-size pixels of exactly known position — behind the previous camera, on its plane, at positions that overflow, at exact integer positions —
    and as history what the pass makes of the pair of the next seed, given weights of 0.25 .. 12 (the cap of the tests is 8) and poisoned: NaN, +Inf and -Inf colours, weights
    of 0, -1, NaN and +Inf, a flag that is not 1."""
    wy, wx, wh, ww = um.low_window(hh, hw, lh, lw, lo_from_hi)
    given = lo_from_hi
    lo_xyzw, lo_planes, hi_planes, lo_from_hi = um.synthetic_pair(hh, hw, lh, lw, seed, given)
    M = synthetic_matrix(hh, hw, lo_from_hi)
    rng = np.random.default_rng(seed + 77)
    big = wh >= 12 and ww >= 16 and hh >= 16 and hw >= 16
    if big:
        y0, x0 = wy + wh - 7, wx + ww // 2 + 2
        lo_xyzw[y0:y0 + 4, x0:x0 + 4, 3] = F(0.0)
        cells = [(y, x) for y in range(2, hh - 2) for x in range(2, hw - 2)]
        picks = [cells[k] for k in rng.choice(len(cells), 40, replace=False)]
        for k, (y, x) in enumerate(picks):
            kind, r = k % 5, k // 5
            if kind == 0:
                p = [4.0 * x / hw, 4.0 * y / hh, -20.0]              # h.z = -0.25
            elif kind == 1:
                p = [4.0 * x / hw, 4.0 * y / hh, -16.0]              # h.z = 0
            elif kind == 2:
                p = [4.0 * x / hw, 4.0 * y / hh, -16.0 + 2.0 ** -18] if r % 2 else [3.0e38, 4.0 * y / hh, 0.0]   # h.z = 2^-22, |position| > 2^20; +Inf
            elif kind == 3:
                p = [float(1 + r % 3), 4.0 * y / hh, 0.0]            # x position m00 (1 + r % 3) + m03, an integer
            else:
                p = [float(1 + r % 3), float(1 + r % 2), 0.0]        # ... and y position m11 (1 + r % 2) - 1
            set_exact_pixel(hi_planes, y, x, p)
    lo2, lp2, hp2, _ = um.synthetic_pair(hh, hw, lh, lw, seed + 1, given)
    _, Hs, _ = accumulate(lo2, lp2, hp2, None, None, Params(lo_from_hi))
    was_surface = Hs[..., 1, 3] == 1
    Hs[..., 0, 3] = np.where(was_surface, rng.integers(1, 49, (hh, hw)).astype(F) * F(0.25), F(0.0))
    if big:
        u = rng.random((hh, hw))
        Hs[(u < 0.03) & was_surface, 0, 1] = F(np.nan)
        Hs[(u >= 0.03) & (u < 0.045) & was_surface, 0, 0] = F(np.inf)
        Hs[(u >= 0.045) & (u < 0.06) & was_surface, 0, 2] = F(-np.inf)
        Hs[(u >= 0.06) & (u < 0.08), 0, 3] = F(0.0)
        Hs[(u >= 0.08) & (u < 0.10), 0, 3] = F(-1.0)
        Hs[(u >= 0.10) & (u < 0.12), 0, 3] = F(np.nan)
        Hs[(u >= 0.12) & (u < 0.13) & was_surface, 0, 3] = F(np.inf)
        Hs[(u >= 0.13) & (u < 0.15), 1, 3] = F(0.5)
    return lo_xyzw, lo_planes, hi_planes, lo_from_hi, Hs, M
