"""A numpy Float32 model of the two kernels of docs/design/20-motion.md, written from that specification: it imports nothing from the library.  `id_plane` is the definition
of trhip_render_aov_ids' third output in terms of the per-sample records; `accumulate` is trhip_temporal_motion — tests/temporal_model.py's pass with step 1b in front of the
projection.  Vectorised over pixels; every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_motion_api.py (CPU) checks the model's own properties, tests/test_gpu_motion.py compares the kernels with it bit for bit."""
import numpy as np

import denoise_model as dm
import temporal_model as tm

F = dm.F
Params = tm.Params
count = tm.count
ID_DTYPE = np.dtype([("prim", np.int32), ("material", np.int32), ("t", np.float32), ("n_hit", np.uint32)])
STATIC = 0xFFFFFFFF


def id_plane(records, offset, size):
    """records: (spp, sb_h, sb_w) with fields t, prim, material; offset = (crop_min.y - sb.min.y, crop_min.x - sb.min.x); size = (H, W) of the film.  Film pixel (x, y) looks
    at its own spp records: n_hit counts those with prim >= 0; among them the first candidate is any t that is not NaN, afterwards only a strictly smaller t replaces it."""
    (oy, ox), (h, w) = offset, size
    own = records[:, oy:oy + h, ox:ox + w]
    assert own.shape[1:] == (h, w)
    out = np.empty((h, w), ID_DTYPE)
    out["prim"], out["material"], out["t"], out["n_hit"] = -1, -1, np.inf, 0
    for s in range(own.shape[0]):
        r = own[s]
        hit = r["prim"] >= 0
        out["n_hit"] += hit.astype(np.uint32)
        with np.errstate(invalid="ignore"):
            wins = hit & np.where(out["prim"] < 0, ~np.isnan(r["t"]), r["t"] < out["t"])
        out["prim"][wins], out["material"][wins], out["t"][wins] = r["prim"][wins], r["material"][wins], r["t"][wins]
    return out


def carry(A, p, point=True):
    """A (p, 1) for a row-major 3 x 4 matrix (per pixel: A is (..., 3, 4)): component i is ((A[i][0]*p.x + A[i][1]*p.y) + A[i][2]*p.z) + A[i][3]; a direction (point=False)
    leaves the last column out."""
    out = []
    for i in range(3):
        v = (A[..., i, 0] * p[..., 0] + A[..., i, 1] * p[..., 1]) + A[..., i, 2] * p[..., 2]
        out.append(v + A[..., i, 3] if point else v)
    return np.stack(out, axis=-1).astype(F)


def select_body(prim, body_of_prim, bodies):
    """Step 1b: (moving mask, body index where moving else 0, and the three static reasons) for an int32 plane of prims."""
    n_prims = 0 if body_of_prim is None else len(body_of_prim)
    n_bodies = 0 if bodies is None else len(bodies)
    no_hit = prim < 0
    out_of_range = ~no_hit & (prim.astype(np.int64) >= n_prims)
    in_range = ~no_hit & ~out_of_range
    if body_of_prim is None or bodies is None:
        return np.zeros(prim.shape, bool), np.zeros(prim.shape, np.int64), no_hit, out_of_range, in_range
    body = np.asarray(body_of_prim, np.uint32)[np.where(in_range, prim, 0)].astype(np.int64)
    moving = in_range & (body < n_bodies)
    return moving, np.where(moving, body, 0), no_hit, out_of_range, in_range & ~moving


def accumulate(B, P, history, M, ids, body_of_prim, bodies, prm, tally=None):
    """(out_xyzw (H, W, 4), out_history (H, W, 3, 4)).  B, P, history, M, prm as in temporal_model.accumulate; ids: (H, W) of ID_DTYPE (prim alone is read); body_of_prim:
    uint32 per primitive slot or None; bodies: (n_bodies, 3, 4) prev_from_cur or None.  `tally` receives temporal_model's counts and, over surface pixels,
      'static_no_hit' (prim < 0), 'prim_out_of_range' (prim >= n_prims), 'static_by_index' (body word >= n_bodies, or a table / matrices missing), 'moving',
      'moving_non_finite' (p' or n' not finite), 'moving_behind_camera' (h.z > 0 false for p'), 'moving_accepted' (a moving pixel that blended),
    and over the taps of moving pixels 'moving_rejected_normal', 'moving_rejected_plane'."""
    B, P = np.ascontiguousarray(B, F), np.ascontiguousarray(P, F)
    assert B.ndim == 3 and B.shape[2] == 4 and P.shape == B.shape[:2] + (3, 4)
    h, w = B.shape[:2]
    prim = np.ascontiguousarray(ids).view(np.int32).reshape(h, w, 4)[..., 0]
    with np.errstate(all="ignore"):
        surface, n, p, c, _, _, W = dm.prepare(B, P, dm.Params(1.0, prm.sigma_normal, prm.sigma_plane, demodulate=False, min_coverage=prm.min_coverage))
        count(tally, "surface", surface)
        moving, body, no_hit, out_of_range, by_index = select_body(prim, body_of_prim, bodies)
        count(tally, "static_no_hit", surface & no_hit)
        count(tally, "prim_out_of_range", surface & out_of_range)
        count(tally, "static_by_index", surface & by_index)
        count(tally, "moving", surface & moving)
        pr, nr, carried = p, n, np.ones((h, w), bool)
        if moving.any():
            A = np.ascontiguousarray(bodies, F).reshape(-1, 3, 4)[body]
            pm, nm = carry(A, p), carry(A, n, point=False)
            pr = np.where(moving[..., None], pm, p).astype(F)  # a static pixel keeps its bits: no identity is applied
            nr = np.where(moving[..., None], nm, n).astype(F)
            carried = ~moving | (np.isfinite(pm).all(-1) & np.isfinite(nm).all(-1))
            count(tally, "moving_non_finite", surface & moving & ~carried)
        c_new, N_new = c, np.ones((h, w), F)
        if history is not None:
            Hs = np.ascontiguousarray(history, F)
            assert Hs.shape == P.shape
            hx, hy, hz = tm.project(M, pr)
            live_px = surface & carried
            front = live_px & (hz > 0)
            count(tally, "behind", live_px & ~front)
            count(tally, "moving_behind_camera", live_px & ~front & moving)
            fx, fy = hx / hz, hy / hz
            pos = front & (np.abs(fx) < tm.MAX_POSITION) & (np.abs(fy) < tm.MAX_POSITION)
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
                    ok_normal = (F(1.0) - dm.dot3(nr, q[..., 1, :3])) < F(prm.sigma_normal)
                    ok_plane = np.abs(dm.dot3(nr, q[..., 2, :3] - pr)) < F(prm.sigma_plane)
                    count(tally, "reject_flag", live & ~ok_flag)
                    count(tally, "reject_length", live & ok_flag & ~ok_length)
                    count(tally, "reject_normal", live & ok_flag & ok_length & ~ok_normal)
                    count(tally, "reject_plane", live & ok_flag & ok_length & ok_normal & ~ok_plane)
                    count(tally, "moving_rejected_normal", moving & live & ok_flag & ok_length & ~ok_normal)
                    count(tally, "moving_rejected_plane", moving & live & ok_flag & ok_length & ok_normal & ~ok_plane)
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
            count(tally, "moving_accepted", blend & moving)
            count(tally, "capped", blend & (N_b == F(prm.max_history)))
            count(tally, "below_cap", blend & (N_b < F(prm.max_history)))
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


# ---- the synthetic case of the tests ---------------------------------------------------------------------------------------------------------------------
SYNTHETIC_PARAMS = tm.SYNTHETIC_PARAMS
SYNTHETIC_M = tm.SYNTHETIC_M
BRANCHES = ("integer_x", "integer_y", "off_left", "off_right", "off_top", "off_bottom", "behind", "non_finite", "reject_normal", "reject_plane", "reject_flag", "all_rejected", "capped",
            "below_cap", "nan_colour", "accepted",
            "static_by_index", "static_no_hit", "prim_out_of_range", "moving_accepted", "moving_rejected_plane", "moving_rejected_normal", "moving_behind_camera", "moving_non_finite")
N_PRIMS, N_MOVING_PRIMS = 40, 24


def synthetic_bodies():
    """Six prev_from_cur matrices for temporal_model.synthetic's world (points (0.1 x, 0.1 y, z in [0, 2.3]), SYNTHETIC_M 16 and 12 pixels per unit): 0 a shift of a fraction of a
    pixel and 1 a turn of 2 degrees about z through the image (their taps are mostly accepted); 2 a turn of 30 degrees about x through the points' mid depth (the normal
    test fails); 3 a shift of 0.5 along z (the plane test fails); 4 a shift of -40 along z (behind the previous camera: h.z = z / 16 + 1); 5 a scale of 3e38 with an
    infinite entry (p' is not finite)."""
    a, b = np.deg2rad(2.0), np.deg2rad(30.0)
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    cx, cy, cz = 2.0, 1.5, 1.0
    return np.array([
        [[1, 0, 0, 0.03], [0, 1, 0, -0.02], [0, 0, 1, 0.0]],
        [[ca, -sa, 0, cx - ca * cx + sa * cy], [sa, ca, 0, cy - sa * cx - ca * cy], [0, 0, 1, 0.0]],
        [[1, 0, 0, 0.0], [0, cb, -sb, cy - cb * cy + sb * cz], [0, sb, cb, cz - sb * cy - cb * cz]],
        [[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 0.5]],
        [[1, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, -40.0]],
        [[3.0e38, 3.0e38, 0, 0.0], [0, 1, 0, np.inf], [0, 0, 1, 0.0]],
    ], F)


def synthetic(h, w, seed):
    """(B, P, history, ids, body_of_prim, bodies): temporal_model.synthetic's frame and history with an id plane and a body table that between them take every branch of step
    1b — and garbage: negative prims down to INT32_MIN, prims far beyond n_prims, body words of every magnitude from n_bodies to 0xFFFFFFFF, and id words beside prim that
    the pass must not read as anything."""
    B, P, Hs = tm.synthetic(h, w, seed)
    rng = np.random.default_rng(seed + 4711)
    bodies = synthetic_bodies()
    nb = len(bodies)
    table = np.empty(N_PRIMS, np.uint32)
    table[:N_MOVING_PRIMS] = np.arange(N_MOVING_PRIMS) % nb
    static_words = np.array([nb, nb + 1, 255, 256, 65535, 65536, 1 << 24, (1 << 31) - 1, 1 << 31, (1 << 31) + 7, 0xFFFFFFFE, STATIC], np.uint32)
    table[N_MOVING_PRIMS:] = static_words[np.arange(N_PRIMS - N_MOVING_PRIMS) % len(static_words)]
    u = rng.random((h, w))
    prim = rng.integers(0, N_MOVING_PRIMS, (h, w)).astype(np.int64)                                                   # 52 %: a moving body
    prim = np.where(u < 0.48, rng.integers(N_MOVING_PRIMS, N_PRIMS, (h, w)), prim)                                    # 22 %: static by index
    prim = np.where(u < 0.26, -1, prim)                                                                               # 8 %: no hit …
    negatives = np.array([-2, -3, -N_PRIMS, -65536, -(1 << 31), -(1 << 31) + 1], np.int64)
    prim = np.where(u < 0.18, negatives[rng.integers(0, len(negatives), (h, w))], prim)                               # 6 %: … and other negative words
    beyond = np.array([N_PRIMS, N_PRIMS + 1, 1 << 10, 1 << 20, 1 << 30, (1 << 31) - 1], np.int64)
    prim = np.where(u < 0.12, beyond[rng.integers(0, len(beyond), (h, w))], prim)                                     # 12 %: beyond the table
    # temporal_model's pixels of exactly known position (set_exact_pixel's film value) stay static, so that its integer and overflow branches are taken as often as there
    exact = np.all(B == F([0.4, 0.5, 0.3, 1.0]), axis=-1) & (prim >= 0) & (prim < N_MOVING_PRIMS)
    prim = np.where(exact, N_MOVING_PRIMS + prim % (N_PRIMS - N_MOVING_PRIMS), prim)
    ids = np.empty((h, w), ID_DTYPE)
    ids["prim"] = prim.astype(np.int32)
    ids["material"] = rng.integers(-(1 << 31), 1 << 31, (h, w)).astype(np.int32)
    ids["t"] = rng.integers(0, 1 << 32, (h, w)).astype(np.uint32).view(np.float32)
    ids["n_hit"] = rng.integers(0, 1 << 32, (h, w)).astype(np.uint32)
    return B, P, Hs, ids, table, bodies
