"""A numpy Float32 model of the temporal reprojection pass, written from its specification (docs/design/14-temporal.md): it imports nothing from the library.  Step 1 is
the denoiser model's `prepare` without demodulation, and the colour functions are that model's.  Vectorised over pixels, a Python loop over the four taps in the specified
order (j outer, i inner); every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_temporal_api.py (CPU) checks the model's own properties, tests/test_gpu_temporal.py compares the kernel with it bit for bit."""
from dataclasses import dataclass

import numpy as np

import denoise_model as dm

F = dm.F
MAX_POSITION = F(2.0 ** 20)


@dataclass
class Params:
    max_history: float = 32.0
    sigma_normal: float = 0.25
    sigma_plane: float = 0.1
    min_coverage: float = 0.5


def project(M, p):
    """h = M (p, 1): component i is ((M[i][0]*p.x + M[i][1]*p.y) + M[i][2]*p.z) + M[i][3]."""
    M = np.asarray(M, F).reshape(3, 4)
    return [((M[i, 0] * p[..., 0] + M[i, 1] * p[..., 1]) + M[i, 2] * p[..., 2]) + M[i, 3] for i in range(3)]


def count(tally, name, mask):
    if tally is not None:
        tally[name] = tally.get(name, 0) + int(np.sum(mask))


def accumulate(B, P, history, M, prm, tally=None):
    """(out_xyzw (H, W, 4), out_history (H, W, 3, 4)).  B: the film, P: its planes, history: the previous frame's out_history or None, M: the previous camera's 3 x 4 matrix.
    `tally`, a dict, receives how many pixels or taps took each branch:
      pixels  'surface', 'behind' (h.z > 0 false), 'non_finite' (position not finite or beyond 2^20), 'integer_x' / 'integer_y' (tx / ty == 0), 'all_rejected' (a position, no
              tap with weight), 'blended', 'capped' / 'below_cap' (N' == / < max_history), 'nan_colour' (the blend was not finite)
      taps    'off_left', 'off_right', 'off_top', 'off_bottom', 'reject_flag', 'reject_length' (N > 0 false), 'reject_normal', 'reject_plane', 'accepted'"""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    assert B.ndim == 3 and B.shape[2] == 4 and P.shape == B.shape[:2] + (3, 4)
    h, w = B.shape[:2]
    with np.errstate(all="ignore"):
        surface, n, p, c, _, _, W = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=False, min_coverage=prm.min_coverage))
        count(tally, "surface", surface)
        c_new, N_new = c, np.ones((h, w), F)
        if history is not None:
            Hs = np.ascontiguousarray(history, F)
            assert Hs.shape == P.shape
            hx, hy, hz = project(M, p)
            front = surface & (hz > 0)
            count(tally, "behind", surface & ~front)
            fx, fy = hx / hz, hy / hz
            pos = front & (np.abs(fx) < MAX_POSITION) & (np.abs(fy) < MAX_POSITION)
            count(tally, "non_finite", front & ~pos)
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            count(tally, "integer_x", pos & (tx == 0))
            count(tally, "integer_y", pos & (ty == 0))
            ix, iy = np.where(pos, x0, 0).astype(np.int64), np.where(pos, y0, 0).astype(np.int64)
            sc, sN, sb = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = ix + i, iy + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    for name, m in (("off_left", qx < 0), ("off_right", qx >= w), ("off_top", qy < 0), ("off_bottom", qy >= h)):
                        count(tally, name, pos & m)
                    q = Hs[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]
                    b = (tx if i else F(1.0) - tx) * (ty if j else F(1.0) - ty)
                    live = pos & inside
                    ok_flag = q[..., 1, 3] == F(1.0)
                    ok_length = q[..., 0, 3] > 0
                    ok_normal = (F(1.0) - dm.dot3(n, q[..., 1, :3])) < F(prm.sigma_normal)
                    ok_plane = np.abs(dm.dot3(n, q[..., 2, :3] - p)) < F(prm.sigma_plane)
                    count(tally, "reject_flag", live & ~ok_flag)
                    count(tally, "reject_length", live & ok_flag & ~ok_length)
                    count(tally, "reject_normal", live & ok_flag & ok_length & ~ok_normal)
                    count(tally, "reject_plane", live & ok_flag & ok_length & ok_normal & ~ok_plane)
                    accepted = live & ok_flag & ok_length & ok_normal & ok_plane
                    count(tally, "accepted", accepted)
                    sc = np.where(accepted[..., None], sc + b[..., None] * q[..., 0, :3], sc)
                    sN = np.where(accepted, sN + b * q[..., 0, 3], sN)
                    sb = np.where(accepted, sb + b, sb)
            blend = pos & (sb > 0)
            count(tally, "all_rejected", pos & ~blend)
            c_h, N_h = sc / sb[..., None], sN / sb
            N_1 = N_h + F(1.0)
            N_b = np.where(N_1 < F(prm.max_history), N_1, F(prm.max_history)).astype(F)
            a = F(1.0) / N_b
            c_b = c_h + a[..., None] * (c - c_h)
            finite = np.isfinite(c_b).all(-1)
            count(tally, "nan_colour", blend & ~finite)
            blend &= finite
            count(tally, "blended", blend)
            count(tally, "capped", blend & (N_b == F(prm.max_history)))
            count(tally, "below_cap", blend & (N_b < F(prm.max_history)))
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


# ---- the synthetic case of the tests: a frame, a history and a matrix that between them take every branch ----------------------------------------------------------
SYNTHETIC_PARAMS = Params(max_history=8.0, sigma_normal=0.02, sigma_plane=0.1, min_coverage=0.5)
# dm.synthetic's points are (0.1 x, 0.1 y, z in [0, 2.3]): the matrix stretches the image by 1.6 and 1.2 about a point near its corner and adds a mild perspective in z, so the
# displacement between a pixel and its reprojected position grows from a few pixels one way to many the other — off every edge, across the region cuts, along the slopes
SYNTHETIC_M = np.array([[16.0, 0.0, 0.0, -3.0], [0.0, 12.0, 0.0, -2.5], [0.0, 0.0, 0.0625, 1.0]], F)


def set_exact_pixel(B, P, y, x, p):
    """Gives pixel (y, x) the weights 1, 1, 1, so that the position the pass recovers is `p` to the bit."""
    B[y, x] = F([0.4, 0.5, 0.3, 1.0])
    P[y, x, 0] = F([0.5, 0.5, 0.5, 1.0])
    P[y, x, 1] = F([0.0, 0.0, 1.0, 1.0])
    P[y, x, 2, :3], P[y, x, 2, 3] = F(p), F(1.0)


def synthetic(h, w, seed):
    """(B, P, history): dm.synthetic's frame with four groups of pixels of exactly known position — behind the previous camera, on its plane, at positions that overflow
    or exceed 2^20, and at exact integer positions —, and as history what the pass makes of another such frame, given lengths of 1..12 (the cap of the tests is 8) and poisoned:
    NaN colours, lengths of 0, -1 and NaN, a flag that is not 1."""
    B, P, _ = dm.synthetic(h, w, seed)
    rng = np.random.default_rng(seed + 77)
    cells = [(y, x) for y in range(3, h - 3) for x in range(3, w - 3)]
    picks = [cells[k] for k in rng.choice(len(cells), 150, replace=False)]
    for k, (y, x) in enumerate(picks):
        kind, r = k % 5, k // 5
        if kind == 0:
            p = [0.1 * x, 0.1 * y, -20.0]                     # h.z = -0.25
        elif kind == 1:
            p = [0.1 * x, 0.1 * y, -16.0]                     # h.z = 0
        elif kind == 2:
            p = [0.1 * x, 0.1 * y, -16.0 + 2.0 ** -18] if r % 2 else [3.0e38, 0.1 * y, 0.0]   # h.z = 2^-22, |position| > 2^20; +Inf
        elif kind == 3:
            p = [0.25 * (1 + r % 12), 0.1 * y, 0.0]           # x position 4 (1 + r % 12) - 3, an integer
        else:
            p = [0.25 * (1 + r % 12), 0.25 * (1 + r % 9) + 0.125, 0.0]   # … and y position 3 (1 + r % 9) - 1
        set_exact_pixel(B, P, y, x, p)
    B2, P2, _ = dm.synthetic(h, w, seed + 1)
    _, Hs = accumulate(B2, P2, None, None, SYNTHETIC_PARAMS)
    was_surface = Hs[..., 1, 3] == 1
    Hs[..., 0, 3] = np.where(was_surface, rng.integers(1, 13, (h, w)).astype(F), F(0.0))
    u = rng.random((h, w))
    Hs[(u < 0.06) & was_surface, 0, 1] = F(np.nan)
    Hs[(u >= 0.06) & (u < 0.08), 0, 3] = F(0.0)
    Hs[(u >= 0.08) & (u < 0.10), 0, 3] = F(-1.0)
    Hs[(u >= 0.10) & (u < 0.12), 0, 3] = F(np.nan)
    Hs[(u >= 0.12) & (u < 0.14), 1, 3] = F(0.5)
    return B, P, Hs
