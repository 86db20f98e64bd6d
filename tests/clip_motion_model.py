"""A numpy Float32 model of trhip_temporal_clip_motion, written from its specification (docs/design/21-clip-motion.md): step 1 and the window statistics are
temporal_clip_model's (on the CURRENT n, p, c), step 1b is motion_model's body carry, steps 2 and 3 are motion_model's with p', n', and step 4' clips the history colour and
cuts the history length of a clipped pixel to clip_max_history.  It imports the two models and nothing from the library.  Vectorised over pixels; every line is one Float32
operation, in the order the text gives.

Not a test: tests/test_clip_motion_api.py (CPU) checks the model's own properties — the identities with the two models it descends from —, tests/test_gpu_clip_motion.py
compares the kernel with it bit for bit."""
from dataclasses import dataclass

import numpy as np

import denoise_model as dm
import motion_model as mm
import temporal_clip_model as tcm
import temporal_model as tm

F = dm.F
count = tm.count
ID_DTYPE = mm.ID_DTYPE
INF = float("inf")


@dataclass
class Params(tcm.Params):
    clip_max_history: float = INF


def params(gamma, radius, clip_max_history=INF):
    s = tm.SYNTHETIC_PARAMS
    return Params(s.max_history, s.sigma_normal, s.sigma_plane, s.min_coverage, gamma, radius, clip_max_history)


def accumulate(B, P, history, M, ids, body_of_prim, bodies, prm, tally=None):
    """(out_xyzw (H, W, 4), out_history (H, W, 3, 4)).  B, P, history, M as in temporal_model.accumulate; ids: (H, W) of ID_DTYPE (prim alone is read) or None — every pixel
    is then static before anything is read —; body_of_prim, bodies as in motion_model.accumulate.  `tally` receives temporal_clip_model.window_bounds' names, 'moving',
    'moving_non_finite', and over the pixels that have a history colour (sb > 0): 'pixels_clipped', 'pixels_inside', 'history_cut' (clipped and clip_max_history < N_h),
    'moving_clipped'; 'blended', 'nan_colour' as in the temporal model."""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    assert B.ndim == 3 and B.shape[2] == 4 and P.shape == B.shape[:2] + (3, 4)
    h, w = B.shape[:2]
    cmh = F(prm.clip_max_history)
    assert cmh >= 0
    with np.errstate(all="ignore"):
        surface, n, p, c, _, _, W = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=False, min_coverage=prm.min_coverage))
        count(tally, "surface", surface)
        lo, hi = tcm.window_bounds(surface, n, p, c, prm, tally)  # the current n, p, c: no motion enters the window
        # step 1b
        if ids is None:
            moving, body = np.zeros((h, w), bool), np.zeros((h, w), np.int64)
        else:
            prim = np.ascontiguousarray(ids).view(np.int32).reshape(h, w, 4)[..., 0]
            moving, body = mm.select_body(prim, body_of_prim, bodies)[:2]
        count(tally, "moving", surface & moving)
        pr, nr, carried = p, n, np.ones((h, w), bool)
        if moving.any():
            A = np.ascontiguousarray(bodies, F).reshape(-1, 3, 4)[body]
            pm, nm = mm.carry(A, p), mm.carry(A, n, point=False)
            pr = np.where(moving[..., None], pm, p).astype(F)  # a static pixel keeps its bits: no identity is applied
            nr = np.where(moving[..., None], nm, n).astype(F)
            carried = ~moving | (np.isfinite(pm).all(-1) & np.isfinite(nm).all(-1))
            count(tally, "moving_non_finite", surface & moving & ~carried)
        c_new, N_new = c, np.ones((h, w), F)
        if history is not None:
            Hs = np.ascontiguousarray(history, F)
            assert Hs.shape == P.shape
            hx, hy, hz = tm.project(M, pr)
            front = surface & carried & (hz > 0)
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
                    accepted = (pos & inside & (q[..., 1, 3] == F(1.0)) & (q[..., 0, 3] > 0) & ((F(1.0) - dm.dot3(nr, q[..., 1, :3])) < F(prm.sigma_normal))
                                & (np.abs(dm.dot3(nr, q[..., 2, :3] - pr)) < F(prm.sigma_plane)))
                    sc = np.where(accepted[..., None], sc + b[..., None] * q[..., 0, :3], sc)
                    sN = np.where(accepted, sN + b * q[..., 0, 3], sN)
                    sb = np.where(accepted, sb + b, sb)
            blend = pos & (sb > 0)
            c_h, N_h = sc / sb[..., None], sN / sb
            below, above = c_h < lo, c_h > hi  # step 4': comparisons with NaN are false
            clipped = (below | above).any(-1)
            count(tally, "pixels_clipped", blend & clipped)
            count(tally, "pixels_inside", blend & ~clipped)
            count(tally, "moving_clipped", blend & clipped & moving)
            c_h = np.where(below, lo, np.where(above, hi, c_h)).astype(F)
            cut = clipped & (cmh < N_h)
            count(tally, "history_cut", blend & cut)
            N_h = np.where(cut, cmh, N_h).astype(F)
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
    out_history[surface, 1, :3], out_history[surface, 1, 3] = n[surface], F(1.0)  # the CURRENT surface
    out_history[surface, 2, :3] = p[surface]
    return out, out_history


# ---- the synthetic case of the tests -----------------------------------------------------------------------------------------------------------------------------
BRANCHES = ("pixels_clipped", "pixels_inside", "history_cut", "moving", "moving_clipped", "moving_non_finite", "cut_left", "cut_top", "reject_normal", "reject_plane", "nan_colour")


def synthetic(h, w, seed):
    """(B, P, history, M, ids, body_of_prim, bodies): temporal_clip_model.synthetic's frame, history and matrix (any size: its poisoned neighbours, its lone and one-colour
    pixels) with motion_model.synthetic's id plane and body table laid over it — every branch of step 1b, and its garbage: prims from INT32_MIN to INT32_MAX, body words of
    every magnitude between n_bodies and 0xFFFFFFFF, random bits in the id words the pass does not read, an infinite matrix.  Added here: NaN and +-Inf colours in film and
    history, every 31st pixel in turn."""
    B, P, Hs, M = tcm.synthetic(h, w, seed)
    small = h < 16 or w < 16  # temporal_clip_model's small frames are the window [8:8+h, 8:8+w] of its 37 x 29 frame: the ids of the same window
    src = mm.synthetic(29, 37, seed) if small else mm.synthetic(h, w, seed)
    ids, table, bodies = (src[3][8:8 + h, 8:8 + w] if small else src[3]).copy(), src[4], src[5]
    flat = np.arange(h * w).reshape(h, w)
    kind = np.where(flat % 31 == 7, (flat // 31) % 6, -1)
    B[kind == 0, 0] = F(np.inf)
    B[kind == 1, 2] = F(-np.inf)
    B[kind == 2, 1] = F(np.nan)
    Hs[kind == 3, 0, 0] = F(np.inf)
    Hs[kind == 4, 0, 1] = F(-np.inf)
    Hs[kind == 5, 0, 2] = F(np.nan)
    return B, P, Hs, M, ids, table, bodies
