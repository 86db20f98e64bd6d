"""A numpy Float32 model of trhip_temporal_upsample_motion, written from its specification (docs/design/22-upsample-motion.md): part U is temporal_upsample_model's (the
upscaler's colour and class, the surface rule, the confidence: the low frame and the full-size planes are this frame's, so no motion enters it), step 1b is motion_model's
body carry (select_body, carry) on the FULL-SIZE id plane, and part T is temporal_upsample_model's with p', n' in the projection and in both tap tests.  It imports the
models and nothing from the library.  Vectorised over full-size pixels; every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_temporal_upsample_motion_api.py (CPU) checks the model's own properties — the identities with temporal_upsample_model and upscale_model —,
tests/test_gpu_temporal_upsample_motion.py compares the kernel with it bit for bit."""
import numpy as np

import denoise_model as dm
import motion_model as mm
import temporal_model as tm
import temporal_upsample_model as tum
import upscale_model as um

F = np.float32
Params = tum.Params
ID_DTYPE = mm.ID_DTYPE
MOTION_KEYS = ("moving", "moving_non_finite", "moving_found", "moving_behind", "moving_tap_reject_normal", "moving_tap_reject_plane", "static_no_ids", "static_no_hit",
               "static_prim_out_of_range", "static_no_table", "static_by_index")
TALLY_KEYS = tum.TALLY_KEYS + MOTION_KEYS


def accumulate(lo_xyzw, lo_planes, hi_planes, history, M, ids, body_of_prim, bodies, prm, tally=None):
    """(out_xyzw (h, w, 4), out_history (h, w, 3, 4), out_mask (h, w) uint8).  The first five and prm as in temporal_upsample_model.accumulate; ids: (h, w) of ID_DTYPE at
    FULL size (prim alone is read) or None — every pixel is then static before anything is read —; body_of_prim: uint32 per primitive slot or None; bodies:
    (n_bodies, 3, 4) prev_from_cur or None.  `tally` receives temporal_upsample_model's counts and, over surface pixels, why a pixel is static ('static_no_ids',
    'static_no_hit': prim < 0, 'static_prim_out_of_range': prim >= n_prims, 'static_no_table': the table or the matrices missing, 'static_by_index': body word >=
    n_bodies), 'moving', 'moving_non_finite' (p' or n' not finite), 'moving_behind', 'moving_found', and over the taps of moving pixels the two rejections."""
    t = dict.fromkeys(TALLY_KEYS, 0)
    count = lambda name, m: tm.count(t, name, m)  # noqa: E731
    PH = np.ascontiguousarray(hi_planes, F)
    h, w = PH.shape[:2]
    A = PH[..., 0, 3]
    # U: colour and class are the upscaler's, surface, n, p and the confidence temporal_upsample_model's
    records = um.low_records(np.ascontiguousarray(lo_xyzw, F), np.ascontiguousarray(lo_planes, F), tum.upscale_params(prm))  # once for both halves of part U
    up_out, m, c = um.upscale(lo_xyzw, lo_planes, PH, tum.upscale_params(prm), want_colour=True, records=records)
    surface, n, p, kmax = tum.surface_and_confidence(lo_xyzw, lo_planes, PH, prm, records)
    k0 = F(prm.confidence_floor)
    kappa = np.where(m == 1, np.where(kmax > k0, kmax, k0), np.where(m == 3, k0, F(0.0))).astype(F)
    count("guided", m == 1), count("orphan", m == 3), count("unguided", m == 2), count("nothing", (m == 0) & ~surface), count("nothing_on_surface", (m == 0) & surface)
    count("kmax_below_floor", (m == 1) & ~(kmax > k0)), count("kmax_above_floor", (m == 1) & (kmax > k0))
    with np.errstate(all="ignore"):
        # step 1b: the body (a pixel that is no surface pixel is not looked at: `surface &` in every count, and nothing of it is used below)
        if ids is None:
            moving, body = np.zeros((h, w), bool), np.zeros((h, w), np.int64)
            count("static_no_ids", surface)
        else:
            assert np.ascontiguousarray(ids).nbytes == h * w * 16, "ids is the FULL-SIZE frame's id plane"
            prim = np.ascontiguousarray(ids).view(np.int32).reshape(h, w, 4)[..., 0]
            moving, body, no_hit, out_of_range, rest = mm.select_body(prim, body_of_prim, bodies)
            count("static_no_hit", surface & no_hit), count("static_prim_out_of_range", surface & out_of_range)
            count("static_no_table" if body_of_prim is None or bodies is None else "static_by_index", surface & rest)
        count("moving", surface & moving)
        pr, nr, carried = p, n, np.ones((h, w), bool)
        if moving.any() and (history is not None or tally is not None):  # (without history p', n' are used by nothing but the tally)
            Ab = np.ascontiguousarray(bodies, F).reshape(-1, 3, 4)[body]
            pm, nm = mm.carry(Ab, p), mm.carry(Ab, n, point=False)
            pr = np.where(moving[..., None], pm, p).astype(F)  # a static pixel keeps its bits: no identity is applied
            nr = np.where(moving[..., None], nm, n).astype(F)
            carried = ~moving | (np.isfinite(pm).all(-1) & np.isfinite(nm).all(-1))
            count("moving_non_finite", surface & moving & ~carried)
        # T with p', n'
        c_new, O_new, found = c, kappa, np.zeros((h, w), bool)
        if history is not None:
            Hs = np.ascontiguousarray(history, F)
            assert Hs.shape == PH.shape
            hx, hy, hz = tm.project(M, pr)
            live_px = surface & carried
            front = live_px & (hz > 0)
            count("behind", live_px & ~front), count("moving_behind", live_px & ~front & moving)
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
                    ok_normal = (F(1.0) - dm.dot3(nr, q[..., 1, :3])) < F(prm.sigma_normal)
                    ok_plane = np.abs(dm.dot3(nr, q[..., 2, :3] - pr)) < F(prm.sigma_plane)
                    count("tap_off_image", pos & ~inside)
                    count("tap_reject_flag", live & ~ok_flag)
                    count("tap_reject_weight", live & ok_flag & ~ok_weight)
                    count("tap_reject_normal", live & ok_flag & ok_weight & ~ok_normal)
                    count("tap_reject_plane", live & ok_flag & ok_weight & ok_normal & ~ok_plane)
                    count("moving_tap_reject_normal", moving & live & ok_flag & ok_weight & ~ok_normal)
                    count("moving_tap_reject_plane", moving & live & ok_flag & ok_weight & ok_normal & ~ok_plane)
                    accepted = live & ok_flag & ok_weight & ok_normal & ok_plane
                    count("tap_accepted", accepted)
                    sc = np.where(accepted[..., None], sc + b[..., None] * q[..., 0, :3], sc)
                    sO = np.where(accepted, sO + b * q[..., 0, 3], sO)
                    sb = np.where(accepted, sb + b, sb)
            found = pos & (sb > 0)
            count("all_rejected", pos & ~found), count("moving_found", found & moving)
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
    out_history[surface, 1, :3], out_history[surface, 1, 3] = n[surface], F(1.0)  # the CURRENT surface: the next frame's previous world
    out_history[surface, 2, :3] = p[surface]
    out_mask = (m + 4 * (found & surface)).astype(np.uint8)
    if tally is not None:
        tally.update(t)
    return out, out_history, out_mask


# ---- the synthetic case of the tests ---------------------------------------------------------------------------------------------------------------------------
N_PRIMS, N_MOVING_PRIMS = mm.N_PRIMS, mm.N_MOVING_PRIMS
BRANCHES = tuple(k for k in TALLY_KEYS if k not in ("static_no_ids", "static_no_table"))  # what one call with ids, table and matrices can take; the other two: calls without


def synthetic_bodies():
    """motion_model.synthetic_bodies' six matrices serve upscale_model.geometry's world as they stand (points (4 x / hw, 4 y / hh or 3.2, z in [0.5, 2]), the previous
    camera's h.z = z / 16 + 1): 0 a shift of a fraction of a pixel, 1 a turn of 2 degrees about z through the image, 2 a turn of 30 degrees about x (the normal test fails),
    3 a shift of 0.5 along z (the plane test fails), 4 a shift of -40 along z (behind the previous camera), 5 an infinite matrix (p' is not finite)."""
    return mm.synthetic_bodies()


def synthetic(hh, hw, lh, lw, seed, lo_from_hi=None):
    """`lo_from_hi`: an explicit map, handed to temporal_upsample_model.synthetic; without it, today's arrays bit for bit.
    (lo_xyzw, lo_planes, hi_planes, lo_from_hi, history, M, ids, body_of_prim, bodies): temporal_upsample_model.synthetic's frames, history and matrix with
    20-motion.md's garbage laid over them at FULL size — motion_model.synthetic's id plane and body table (prims from INT32_MIN to INT32_MAX, body words of every magnitude
    between n_bodies and 0xFFFFFFFF, random bits in the id words the pass does not read) and its six matrices, one of them infinite.  temporal_upsample_model's pixels of
    exactly known position stay static, so that its own branches (behind, overflow, integer positions) are taken as often as there.  Added here: NaN and +-Inf in the low
    film and in the history's colours, every 31st pixel in turn."""
    lo_xyzw, lo_planes, hi_planes, lo_from_hi, Hs, M = tum.synthetic(hh, hw, lh, lw, seed, lo_from_hi)
    small = hh < 16 or hw < 16  # motion_model's generator is made for frames of some size: a small frame takes the window [8:8+hh, 8:8+hw] of its 37 x 29 id plane
    src = mm.synthetic(29, 37, seed) if small else mm.synthetic(hh, hw, seed)
    if small and (hh > 21 or hw > 29):  # a strip: the 37 x 29 id plane laid side by side
        plane = np.tile(src[3], (-(-hh // 29), -(-hw // 37)))[:hh, :hw]
    else:
        plane = src[3][8:8 + hh, 8:8 + hw] if small else src[3]
    ids, table, bodies = np.ascontiguousarray(plane).copy(), src[4], synthetic_bodies()
    exact = np.all(hi_planes[..., 0, :] == F([0.5, 0.5, 0.5, 1.0]), axis=-1) & np.all(hi_planes[..., 1, :] == F([0.0, 0.0, 1.0, 1.0]), axis=-1)
    prim = ids["prim"].astype(np.int64)
    to_static = exact & (prim >= 0) & (prim < N_MOVING_PRIMS)
    ids["prim"] = np.where(to_static, N_MOVING_PRIMS + prim % (N_PRIMS - N_MOVING_PRIMS), prim).astype(np.int32)
    flat = np.arange(lh * lw).reshape(lh, lw)
    kind = np.where(flat % 31 == 7, (flat // 31) % 3, -1)
    lo_xyzw[kind == 0, 0] = F(np.inf)
    lo_xyzw[kind == 1, 2] = F(-np.inf)
    lo_xyzw[kind == 2, 1] = F(np.nan)
    flat = np.arange(hh * hw).reshape(hh, hw)
    kind = np.where(flat % 31 == 7, (flat // 31) % 3, -1)
    Hs[kind == 0, 0, 0] = F(np.inf)
    Hs[kind == 1, 0, 1] = F(-np.inf)
    Hs[kind == 2, 0, 2] = F(np.nan)
    return lo_xyzw, lo_planes, hi_planes, lo_from_hi, Hs, M, ids, table, bodies
