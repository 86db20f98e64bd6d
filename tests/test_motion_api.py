"""Moving geometry in a preview (trhip_render_aov_ids, trhip_temporal_motion), the part that needs no GPU: the entry points and the parameter block's layout (header text ==
ctypes mirror, 80 bytes), the default parameters, the refusals and their order through a NULL context, the properties of the numpy model (tests/motion_model.py) the kernels
are compared with bit for bit in tests/test_gpu_motion.py, Scene.moved and FlatScene.body_table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import julia_replay as jr
import motion_model as mm
import motion_scenes as ms
import temporal_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_render_aov_ids", "trhip_render_aov_ids_device", "trhip_temporal_motion_default_params", "trhip_temporal_motion", "trhip_temporal_motion_device")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_entry_points_are_exported_with_the_headers_signatures(T):
    protos = jr.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, f"include/tracehip.h does not declare {name}"
        assert getattr(T.lib(), name) is not None
        ret, args = T._ffi.SIGNATURES[name]
        c_ret, c_args = jr.ctypes_sig(protos[name])
        assert ret is c_ret and len(args) == len(c_args), name
        for k, (a, c) in enumerate(zip(args, c_args)):
            if c is C.c_void_p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, k, a)
            else:
                assert a is c, (name, k, a, c)
    assert protos["trhip_temporal_motion"][1] == ["ptr:void", "ptr:f32", "ptr:f32", "ptr:f32", "ptr:void", "ptr:u32", "ptr:f32", "u32", "u32", "ptr:void", "ptr:f32", "ptr:f32", "ptr:stats"]
    assert protos["trhip_temporal_motion_device"][1] == ["ptr:void"] * 7 + ["u32", "u32"] + ["ptr:void"] * 3 + ["ptr:stats"]
    assert protos["trhip_render_aov_ids"][1] == protos["trhip_render_aov"][1][:-1] + ["ptr:void", "ptr:stats"], "trhip_render_aov's arguments and the id plane before the stats"
    assert T.lib().trhip_version() == 3001, "added without a version change"


def test_params_and_id_record_mirror_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracehip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_temporal_motion_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1), m.group(3)) for m in re.finditer(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)]
    assert [n for n, _, _ in fields] == ["prev_world_to_pixel", "max_history", "sigma_normal", "sigma_plane", "min_coverage", "n_prims", "n_bodies", "flags", "reserved"]
    S = T._ffi.TemporalMotionParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    for (name, ctype), (n, t, dim) in zip(S._fields_, fields):
        assert name == n and C.sizeof(ctype) == C.sizeof(ctypes_of[t]) * int(dim or 1), name
    assert C.sizeof(S) == 80
    assert [getattr(S, n).offset for n, _, _ in fields] == [0, 48, 52, 56, 60, 64, 68, 72, 76]
    # the fields trhip_temporal_params has lie where it has them: temporal_const<> serves both blocks
    for n in ("prev_world_to_pixel", "max_history", "sigma_normal", "sigma_plane", "min_coverage"):
        assert getattr(S, n).offset == getattr(T._ffi.TemporalParams, n).offset
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_aov_id\s*;", src).group(1)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == [("prim", "int32_t"), ("material", "int32_t"), ("t", "float"), ("n_hit", "uint32_t")]
    for dt in (T._ffi.AOV_ID_DTYPE, mm.ID_DTYPE):
        assert dt.itemsize == 16 and list(dt.names) == [n for n, _ in fields] and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]
        assert [dt.fields[n][0] for n in dt.names] == [np.int32, np.int32, np.float32, np.uint32]


def good_params(T, **over):
    p = T._ffi.TemporalMotionParams()
    assert T.lib().trhip_temporal_motion_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "matrix_entry":
            p.prev_world_to_pixel[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def test_default_params_need_no_context(T):
    p = T._ffi.TemporalMotionParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert T.lib().trhip_temporal_motion_default_params(C.byref(p)) == 0
    base = T._ffi.TemporalParams()
    assert T.lib().trhip_temporal_default_params(C.byref(base)) == 0
    assert list(p.prev_world_to_pixel) == [0.0] * 12
    assert (p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage) == (base.max_history, base.sigma_normal, base.sigma_plane, base.min_coverage) == (8.0, 0.25, F(0.1), 0.5)
    assert (p.n_prims, p.n_bodies, p.flags, p.reserved) == (0, 0, 0, 0)
    assert T.lib().trhip_temporal_motion_default_params(None) == INVALID


# trhip_temporal's checks of the shared fields in its order, then flags, then reserved
BAD_PARAMS = [(dict(matrix_entry=(0, float("nan"))), b"prev_world_to_pixel"), (dict(matrix_entry=(11, float("inf"))), b"prev_world_to_pixel"),
              (dict(max_history=0.5), b"max_history"), (dict(max_history=float("inf")), b"max_history"), (dict(max_history=float("nan")), b"max_history"),
              (dict(min_coverage=-0.1), b"min_coverage"), (dict(min_coverage=1.5), b"min_coverage"), (dict(min_coverage=float("nan")), b"min_coverage"),
              (dict(flags=1), b"flag"), (dict(reserved=1), b"reserved")]
for _name in ("sigma_normal", "sigma_plane"):
    BAD_PARAMS += [({_name: v}, _name.encode()) for v in (0.0, -1.0, float("inf"), float("nan"))]
ORDER = [dict(matrix_entry=(5, float("nan"))), dict(max_history=0.0), dict(sigma_normal=0.0), dict(sigma_plane=-1.0), dict(min_coverage=2.0), dict(flags=2), dict(reserved=7)]
ORDER_WORDS = [b"prev_world_to_pixel", b"max_history", b"sigma_normal", b"sigma_plane", b"min_coverage", b"flag", b"reserved"]


@pytest.mark.parametrize("entry", ["trhip_temporal_motion", "trhip_temporal_motion_device"])
def test_refusals_and_their_order_without_a_device(T, entry):
    """No context exists here, so every call is refused.  The parameter block is checked first — the message kept for trhip_last_error(NULL) names the field, and of two bad
    fields the earlier one —, then the pointers."""
    fn, L = getattr(T.lib(), entry), T.lib()
    host = entry == "trhip_temporal_motion"
    film, planes, out, out_h = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F)
    ids, table, mats = np.zeros((2, 2), mm.ID_DTYPE), np.zeros(3, np.uint32), np.zeros((1, 12), F)
    fp = (lambda a: T._ffi.fptr(a)) if host else (lambda a: C.c_void_p(a.ctypes.data))
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    up = (lambda a: T._ffi.u32ptr(a)) if host else vp

    def call(prm, xyzw=film, idp=ids, tb=table, mt=mats):
        return fn(None, fp(xyzw) if xyzw is not None else None, fp(planes), None, vp(idp) if idp is not None else None, up(tb) if tb is not None else None,
                  fp(mt) if mt is not None else None, 2, 2, C.byref(prm) if prm is not None else None, fp(out), fp(out_h), None)
    for over, word in BAD_PARAMS:
        assert call(good_params(T, **over)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    for k in range(len(ORDER)):
        for j in range(k + 1, len(ORDER)):
            assert call(good_params(T, **ORDER[k], **ORDER[j])) == INVALID
            assert ORDER_WORDS[k] in L.trhip_last_error(None), (ORDER[k], ORDER[j], L.trhip_last_error(None))
    assert call(None) == INVALID and b"null argument" in L.trhip_last_error(None)  # no parameter block
    # a bad block and missing pointers: the block is reported
    assert call(good_params(T, reserved=1), xyzw=None, idp=None) == INVALID and b"reserved" in L.trhip_last_error(None)
    # a good block: the null context is a null pointer, reported before the table rules
    for prm in (good_params(T), good_params(T, n_prims=3, n_bodies=1), good_params(T, n_prims=3)):
        assert call(prm) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert call(good_params(T, n_prims=3, n_bodies=1), tb=None, mt=None) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any() and not out_h.any()


def test_aov_ids_refuses_null_handles(T):
    L = T.lib()
    ids = np.zeros((2, 2), mm.ID_DTYPE)
    assert L.trhip_render_aov_ids(None, None, None, 1, 0, 0, None, None, C.c_void_p(ids.ctypes.data), None) == INVALID
    assert L.trhip_render_aov_ids_device(None, None, None, 1, 0, 0, None, None, None, None) == INVALID
    assert not ids.view(np.uint32).any()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------------
def test_id_plane_model_on_hand_made_records():
    rec = np.zeros((4, 3, 4), np.dtype([("t", F), ("prim", np.int32), ("material", np.int32)]))
    rec["prim"], rec["material"], rec["t"] = -1, -1, np.inf
    rec[:, 1, 1] = [(5.0, 3, 1), (2.0, 7, 2), (2.0, 9, 3), (np.nan, 4, 0)]      # the smallest t; the tie stays with the lower s; NaN never wins
    rec[:, 1, 2] = [(np.nan, 4, 0), (np.inf, -1, -1), (np.nan, 6, 1), (np.inf, -1, -1)]  # hits, none with a t
    rec[:, 2, 1] = [(np.inf, -1, -1), (np.inf, 8, -1), (np.inf, -1, -1), (1.0e30, 2, 5)]  # a hit at +Inf loses to a later finite one; a hit without a material
    rec[:, 2, 2] = [(np.nan, 4, 0), (3.0, 1, 2), (np.inf, -1, -1), (3.5, 0, 0)]   # a NaN first does not block what follows
    got = mm.id_plane(rec, (1, 1), (2, 2))
    want = np.array([[(7, 2, 2.0, 4), (-1, -1, np.inf, 2)], [(2, 5, 1.0e30, 2), (1, 2, 3.0, 3)]], mm.ID_DTYPE)
    assert got.tobytes() == want.tobytes(), (got, want)
    none = mm.id_plane(rec, (0, 0), (1, 1))
    assert none.tobytes() == np.array([[(-1, -1, np.inf, 0)]], mm.ID_DTYPE).tobytes()


def test_model_with_every_pixel_static_is_the_temporal_model_bit_for_bit():
    for h, w in ((29, 37), (64, 64)):
        B, P, Hs, ids, table, bodies = mm.synthetic(h, w, 2000 + h)
        ref_tally, ref = {}, None
        ref = tm.accumulate(B, P, Hs, mm.SYNTHETIC_M, mm.SYNTHETIC_PARAMS, ref_tally)
        all_static = np.full_like(table, mm.STATIC)
        beyond = np.arange(len(table), dtype=np.uint32) + len(bodies)
        no_hit = ids.copy()
        no_hit["prim"] = -1
        for what, args in (("no table, no matrices", (ids, None, None)), ("no matrices", (ids, table, None)), ("no table", (ids, None, bodies)),
                           ("every word 0xFFFFFFFF", (ids, all_static, bodies)), ("every word >= n_bodies", (ids, beyond, bodies)), ("no pixel hit", (no_hit, table, bodies))):
            tally = {}
            got = mm.accumulate(B, P, Hs, mm.SYNTHETIC_M, *args, mm.SYNTHETIC_PARAMS, tally)
            assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1])), (h, w, what)
            assert tally.get("moving", 0) == 0 and {k: tally[k] for k in ref_tally} == ref_tally, (h, w, what)
        # and with the bodies in place something does change
        got = mm.accumulate(B, P, Hs, mm.SYNTHETIC_M, ids, table, bodies, mm.SYNTHETIC_PARAMS)
        assert not np.array_equal(bits(got[0]), bits(ref[0]))
        # out_history holds the CURRENT n and p whatever moved
        assert np.array_equal(bits(got[1][..., 1:, :]), bits(ref[1][..., 1:, :]))
        # without history the bodies decide nothing
        a, b = mm.accumulate(B, P, None, None, ids, table, bodies, mm.SYNTHETIC_PARAMS), tm.accumulate(B, P, None, None, mm.SYNTHETIC_PARAMS)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_model_synthetic_case_takes_every_branch():
    """The condition of the GPU test, checked here so that the generator is chosen on the CPU: every branch at least 20 times at 37 x 29 and at 64 x 64."""
    for h, w in ((29, 37), (64, 64)):
        B, P, Hs, ids, table, bodies = mm.synthetic(h, w, 2000 + h)
        tally = {}
        mm.accumulate(B, P, Hs, mm.SYNTHETIC_M, ids, table, bodies, mm.SYNTHETIC_PARAMS, tally)
        for name in mm.BRANCHES:
            assert tally.get(name, 0) >= 20, (h, w, name, tally)
        prim = ids["prim"]
        assert (prim < -1).sum() >= 20 and (prim == np.iinfo(np.int32).min).any() and (prim > 1 << 20).sum() >= 20 and (prim == np.iinfo(np.int32).max).any()
        assert {int(x) for x in table[mm.N_MOVING_PRIMS:]} >= {len(bodies), 65536, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF}


def format_bound(M, p, hz, fx, fy, dp):
    """What Float32 allows for the position of a point p whose coordinates are themselves uncertain by dp: tests/test_temporal_api.py's bound, derived in
    docs/design/14-temporal.md — every h_i carries at most 6 * 2^-24 * (|M_i0 p.x| + |M_i1 p.y| + |M_i2 p.z| + |M_i3|) from the evaluation —, and |M_i0| dp.x + |M_i1| dp.y +
    |M_i2| dp.z from the point; f = h.x / h.z turns that into (dh_x + |f| dh_z) / h.z."""
    M64, p64 = np.abs(M.astype(np.float64)), np.abs(p.astype(np.float64))
    dh = [6.0 * 2.0 ** -24 * (M64[i, 0] * p64[:, 0] + M64[i, 1] * p64[:, 1] + M64[i, 2] * p64[:, 2] + M64[i, 3]) + M64[i, 0] * dp[:, 0] + M64[i, 1] * dp[:, 1] + M64[i, 2] * dp[:, 2]
          for i in range(3)]
    hz = hz.astype(np.float64)
    return np.maximum((dh[0] + np.abs(fx) * dh[2]) / hz, (dh[1] + np.abs(fy) * dh[2]) / hz)


def carry_bound(A, q):
    """The error of carry(A, q) against the exact product: 6 * 2^-24 * (|A_i0 q.x| + |A_i1 q.y| + |A_i2 q.z| + |A_i3|) per component, as above."""
    A64, q64 = np.abs(A.astype(np.float64)), np.abs(q.astype(np.float64))
    return np.stack([6.0 * 2.0 ** -24 * (A64[i, 0] * q64[:, 0] + A64[i, 1] * q64[:, 1] + A64[i, 2] * q64[:, 2] + A64[i, 3]) for i in range(3)], axis=-1)


@pytest.mark.parametrize("which", ["translation", "rotation", "both"])
def test_a_motion_composed_into_camera_and_scene_projects_where_the_point_was(T, which):
    """A body and the camera are carried by the same rigid motion S.  Points p of the body seen at position f through the previous camera lie at S p now; step 1b's
    p' = prev_from_cur (S p) must project through the PREVIOUS camera's matrix where p did, and S p through the moved camera's matrix as well (nothing moved relative to it),
    both within what the Float32 formats allow (the bound of docs/design/14-temporal.md, with the uncertainty of the carried point added: two matrix products, and S^-1 S = 1
    only up to the Float32 rounding of both matrices' entries, 2^-24 relative each)."""
    cam = ms.camera(T, 64, 3.0)
    S = {"translation": T.translate([0.21, -0.08, 0.13]), "rotation": ms.rotation_about(T, ms.CUBE_CENTRE, 1, 17.0),
         "both": ms.rotation_about(T, (0.2, 0.1, -2.2), 0, -23.0) * T.translate([0.05, 0.02, -0.3])}[which]
    if which == "both":  # Transformation.__mul__ multiplies the inverses in the same order (the reference's load-bearing bug): the true inverse, from Float64
        S = T.Transformation(S.m, np.linalg.inv(S.m.astype(np.float64)).astype(F))
    moved_cam = T.PerspectiveCamera(T.Transformation(S.m.astype(np.float64) @ cam.camera_to_world.m.astype(np.float64),
                                                     np.linalg.inv(S.m.astype(np.float64) @ cam.camera_to_world.m.astype(np.float64))), cam.screen_window, 0.0, 1.0, 0.0, 1e6, 90.0, cam.film)
    M, M_moved = cam.world_to_pixel(), moved_cam.world_to_pixel()
    rng = np.random.default_rng(11)
    p = (ms.CENTRE + rng.uniform(-0.5, 0.5, (400, 3))).astype(F)
    hx, hy, hz = tm.project(M, p)
    assert np.all(hz > 0)
    fx, fy = (hx / hz).astype(np.float64), (hy / hz).astype(np.float64)
    assert (np.abs(fx - 32) < 40).all() and (np.abs(fy - 32) < 40).all(), "the points are in or near the 64 x 64 image"
    A_fwd, A = np.ascontiguousarray(S.m[:3], F), T.TemporalAccumulator.prev_from_cur(S)
    assert A.dtype == F and A.shape == (3, 4) and np.array_equal(A, S.inv_m[:3])
    q = mm.carry(A_fwd[None], p)            # the body's points now
    back = mm.carry(A[None], q)             # step 1b
    # S^-1 S differs from 1 by the rounding of the entries: 2 * 2^-24 * sum |A_ik| |S_kj| |p_j| bounds what that moves the point by
    entries = 2.0 * 2.0 ** -24 * (np.abs(A[:, :3].astype(np.float64)) @ (np.abs(A_fwd[:, :3].astype(np.float64)) @ np.abs(p.astype(np.float64)).T + np.abs(A_fwd[:, 3:4].astype(np.float64)))).T
    dp = carry_bound(A, q) + (np.abs(A[:, :3].astype(np.float64)) @ carry_bound(A_fwd, p).T).T + entries + 2.0 ** -24 * np.abs(A[:, 3].astype(np.float64))
    assert np.abs(back.astype(np.float64) - p).max() <= dp.max() and np.all(np.abs(back.astype(np.float64) - p) <= dp)
    bx, by, bz = tm.project(M, back)
    gx, gy = (bx / bz).astype(np.float64), (by / bz).astype(np.float64)
    allowed = format_bound(M, p, hz, fx, fy, np.zeros_like(dp)) + format_bound(M, back, bz, gx, gy, dp)
    err = np.maximum(np.abs(gx - fx), np.abs(gy - fy))
    print(f"motion composed into camera and scene ({which}): p' projects within {err.max():.2e} px of p, {float((err / allowed).max()):.3f} of what the formats allow")
    assert np.all(err <= allowed) and err.max() < 1.0 / 32.0
    # and through the moved camera the moved points stand where they stood: the moved camera's matrix is built from Float64 products rounded once, like M
    mx, my, mz = tm.project(M_moved, q)
    ex, ey = (mx / mz).astype(np.float64), (my / mz).astype(np.float64)
    allowed = format_bound(M, p, hz, fx, fy, np.zeros_like(dp)) + format_bound(M_moved, q, mz, ex, ey, carry_bound(A_fwd, p)) + format_bound(M_moved, q, mz, ex, ey, np.zeros_like(dp))
    err = np.maximum(np.abs(ex - fx), np.abs(ey - fy))
    assert np.all(mz > 0) and np.all(err <= allowed) and err.max() < 1.0 / 32.0, (err.max(), allowed.min())


def centre_ray_frame(T, ob, scene, cam):
    """(film, planes, ids, body table builder) of a frame made from the ORACLE's geometry: one ray through every pixel's centre, its hit's shading normal and position with
    weight 1, a constant colour.  No filter and no noise — what remains is the geometry of the reprojection."""
    import denoise_model as dm
    h, w = cam.film.size
    cmin = np.asarray(cam.film.crop_bounds.p_min, np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    samples = np.stack([cmin[0] + xs + 0.5, cmin[1] + ys + 0.5, np.full((h, w), 0.5), np.full((h, w), 0.5), np.zeros((h, w))], -1).reshape(-1, 5).astype(F)
    osc = ob.OracleScene.from_scene(scene)
    _, prim, geom, _ = osc.trace_closest(ob.generate_rays(cam, samples), want_geom=True)
    hit = (prim >= 0).reshape(h, w)
    ones = np.ones((h, w), F)
    P = dm.planes_of(geom[:, 6:9].reshape(h, w, 3), geom[:, 0:3].reshape(h, w, 3), np.full((h, w, 3), 0.5, F), ones, hit.astype(F))
    B = np.concatenate([dm.rgb_to_xyz(np.full((h, w, 3), 0.5, F)), ones[..., None]], -1).astype(F)
    ids = np.zeros((h, w), mm.ID_DTYPE)
    ids["prim"] = prim.reshape(h, w)
    return B, P, ids, osc.get_bvh()[3]


def test_moving_bodies_keep_their_history_on_frames_from_the_oracles_geometry(T, ob):
    """The real sequence of tests/test_gpu_motion.py — the sphere slides, the cube turns about its own centre, the camera turns —, three frames at 48 x 48, with frames made
    from the oracle's hits at the pixel centres: at frame 3 more than half of the surface pixels of each moving body have N' >= 2 through the motion-aware pass.  Measured
    here: every one of the 195 sphere pixels and of the 201 cube pixels; the pass that ignores the motion (temporal_model) keeps 0.826 and 0.891 of them — with steps this
    small many a wrong tap still passes both tests, which is what tests/test_gpu_motion.py's quality figures are about."""
    prm = tm.Params(8.0, 0.25, 0.1, 0.5)
    hist, hist_plain, prev = None, None, None
    for k, ((scene, motion), deg) in enumerate(zip(ms.scene_sequence(T, 3), (0.0, 3.0, 6.0))):
        cam = ms.camera(T, 48, deg)
        B, P, ids, order = centre_ray_frame(T, ob, scene, cam)
        counts = T.top_level_counts(scene)
        keys = sorted(motion)
        words = np.full(len(counts), mm.STATIC, np.uint32)
        words[keys] = np.arange(len(keys))
        table = np.repeat(words, counts)[order]
        mats = np.stack([T.TemporalAccumulator.prev_from_cur(motion[i]) for i in keys]) if keys else None
        M = prev.world_to_pixel() if prev is not None else None
        tally = {}
        _, hist = mm.accumulate(B, P, hist, M, ids, table if keys else None, mats, prm, tally)
        _, hist_plain = tm.accumulate(B, P, hist_plain, M, prm)
        prev = cam
    caller = np.repeat(np.arange(len(counts)), counts)[order]  # slot -> top-level entry
    surface = hist[..., 1, 3] == 1
    for name, index in (("sphere", ms.SPHERE_INDEX), ("cube", ms.CUBE_INDEX)):
        on_body = surface & (ids["prim"] >= 0) & (caller[np.where(ids["prim"] >= 0, ids["prim"], 0)] == index)
        share, share_plain = float((hist[on_body][:, 0, 3] >= 2).mean()), float((hist_plain[on_body][:, 0, 3] >= 2).mean())
        print(f"oracle-geometry sequence, {name}: {int(on_body.sum())} surface pixels, N' >= 2 at {share:.3f} of them with the motion, {share_plain:.3f} without")
        assert on_body.sum() >= 30 and share > 0.5 and share >= share_plain, (name, int(on_body.sum()), share, share_plain)
    assert tally["moving_accepted"] > 100 and tally["static_by_index"] > 1000


# ---- Scene.moved and FlatScene.body_table ------------------------------------------------------------------------------------------------------------------
def test_scene_moved_on_a_sphere_and_on_a_mesh_with_normals(T):
    scene = ms.moving_scene(T)
    slide, turn = T.translate([0.1, 0.0, -0.05]), ms.rotation_about(T, ms.CUBE_CENTRE, 1, 30.0)
    new = scene.moved({ms.SPHERE_INDEX: slide, ms.CUBE_INDEX: turn})
    old_p, new_p = scene.aggregate.primitives, new.aggregate.primitives
    assert new is not scene and new.lights == scene.lights and all(a is b for a, b in zip(new.lights, scene.lights))
    assert T.top_level_counts(new) == T.top_level_counts(scene) == [1] * 11 + [12] and new.aggregate.max_node_primitives == scene.aggregate.max_node_primitives
    assert all(new_p[i] is old_p[i] for i in range(ms.N_WALL_ENTRIES)), "entries without a motion are shared"
    assert all(a.material is b.material for a, b in zip(new_p, old_p)), "the same material objects"
    # the sphere: the composed object_to_world with its true inverse
    s_old, s_new = old_p[ms.SPHERE_INDEX].shape, new_p[ms.SPHERE_INDEX].shape
    assert (s_new.radius, s_new.z_min, s_new.z_max, s_new.phi_max_deg) == (s_old.radius, s_old.z_min, s_old.z_max, s_old.phi_max_deg)
    assert np.allclose(s_new.core.object_to_world.m[:3, 3], np.array(ms.SPHERE_CENTRE) + [0.1, 0.0, -0.05], atol=1e-6)
    assert np.allclose(s_new.core.object_to_world.m @ s_new.core.object_to_world.inv_m, np.eye(4), atol=1e-6)
    assert np.allclose(s_new.core.world_to_object.m, s_new.core.object_to_world.inv_m) and s_new.core.reverse_orientation == s_old.core.reverse_orientation
    assert np.array_equal(s_old.core.object_to_world.m[:3, 3], F(ms.SPHERE_CENTRE)), "the old scene is left alone"
    # the mesh: vertices through transform_points, normals through the linear part, Float32 left to right
    m_old, m_new = old_p[ms.CUBE_INDEX].mesh, new_p[ms.CUBE_INDEX].mesh
    assert np.array_equal(bits(m_new.vertices), bits(T.transform_points(turn, m_old.vertices))) and np.array_equal(m_new.indices, m_old.indices)
    want_n = np.stack([turn.vector(v) for v in m_old.normals])
    assert np.array_equal(bits(m_new.normals), bits(want_n)) and not np.array_equal(bits(m_new.normals), bits(m_old.normals))
    a = np.deg2rad(30.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    assert np.allclose(m_new.normals, m_old.normals @ R.T, atol=1e-6) and np.allclose(np.linalg.norm(m_new.normals, axis=1), 1.0, atol=1e-6)
    assert np.allclose(m_new.vertices, (m_old.vertices - ms.CUBE_CENTRE) @ R.T + ms.CUBE_CENTRE, atol=1e-5)
    assert np.allclose(m_new.vertices.mean(0), ms.CUBE_CENTRE, atol=1e-5), "a turn about its own centre"
    assert m_new.tangents is None and m_new.uv is None and m_new.n_triangles == 12
    flip = lambda m: m.core.reverse_orientation != m.core.transform_swaps_handedness  # noqa: E731
    assert flip(m_new) == flip(m_old)
    # a second step composes; tangents turn with the normals; single triangles of one mesh share one moved mesh; a nested aggregate moves as a whole
    quad = T.create_triangle_mesh(T.ShapeCore(T.translate([0, 0, 0]), False), 2, np.array([1, 2, 3, 1, 3, 4], np.uint32), 4, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]],
                                  [[0, 0, 1]] * 4, [[1, 0, 0]] * 4)
    inner = T.BVHAccel([T.GeometricPrimitive(t, None) for t in quad] + [old_p[ms.SPHERE_INDEX]], 1)
    nested = T.Scene([], T.BVHAccel([inner, old_p[0]], 4))
    quarter = ms.rotation_about(T, (0, 0, 0), 1, 90.0)
    moved = nested.moved({0: quarter})
    q0, q1, sph = moved.aggregate.primitives[0].primitives
    assert q0.shape.mesh is q1.shape.mesh and (q0.shape.k, q1.shape.k) == (0, 1) and moved.aggregate.primitives[1] is old_p[0]
    assert np.allclose(q0.shape.mesh.normals, [[1, 0, 0]] * 4, atol=1e-6) and np.allclose(q0.shape.mesh.tangents, [[0, 0, -1]] * 4, atol=1e-6)
    assert np.allclose(sph.shape.core.object_to_world.m[:3, 3], [ms.SPHERE_CENTRE[2], ms.SPHERE_CENTRE[1], -ms.SPHERE_CENTRE[0]], atol=1e-6)
    assert T.top_level_counts(moved) == [3, 1]
    for bad in ({12: slide}, {-1: slide}, {"a": slide}):
        with pytest.raises(T.TraceHipError):
            scene.moved(bad)


def test_body_table_against_a_hand_built_scene_with_a_nested_aggregate(T):
    """Top-level entries: a nested aggregate of two triangles and a sphere (3 primitives), a wall triangle, a 12-triangle MeshPrimitives, a sphere: 17 primitives in caller
    order.  The table is in slot order through prim_order, which a stand-in for FlatScene.prim_order() supplies (no device here)."""
    walls, _ = T.scenes.cornell_primitives(spheres=False)
    sphere = ms.moving_scene(T).aggregate.primitives[ms.SPHERE_INDEX]
    inner = T.BVHAccel([walls[0], walls[1], sphere], 1)
    scene = T.Scene([], T.BVHAccel([inner, walls[2], ms.cube_primitives(T, None), sphere], 1))
    assert T.top_level_counts(scene) == [3, 1, 12, 1]
    flat = T.FlatScene.__new__(T.FlatScene)
    flat.top_counts = T.top_level_counts(scene)
    flat._h = None  # nothing to free
    order = np.random.default_rng(5).permutation(17).astype(np.uint32)
    flat.prim_order = lambda: order
    caller = np.array([2] * 3 + [0xFFFFFFFF] + [0] * 12 + [1], np.uint32)
    table = flat.body_table([2, None, 0, 1])
    assert table.dtype == np.uint32 and table.shape == (17,) and np.array_equal(table, caller[order])
    assert np.array_equal(flat.body_table([None] * 4), np.full(17, 0xFFFFFFFF, np.uint32))
    with pytest.raises(T.TraceHipError):
        flat.body_table([0, 1, 2])
    flat.prim_order = lambda: order[:16]
    with pytest.raises(T.TraceHipError):
        flat.body_table([2, None, 0, 1])


def test_python_classes_refuse_what_motion_cannot_be_combined_with(T):
    t = T.TemporalAccumulator(max_history=4)
    p = t._motion_params_for(None, 7, 2)
    assert (p.max_history, p.n_prims, p.n_bodies, p.flags, p.reserved) == (4.0, 7, 2, 0, 0) and list(p.prev_world_to_pixel) == [0.0] * 12
    cam = ms.camera(T, 16)
    assert list(t._motion_params_for(cam, 0, 0).prev_world_to_pixel) == cam.world_to_pixel().reshape(-1).tolist()
    for bad in (T.TemporalAccumulator(clip_gamma=1.0), T.TemporalAccumulator(moments=True)):
        with pytest.raises(T.TraceHipError, match="plain accumulator"):
            bad._motion_params_for(None, 0, 0)
    with pytest.raises(T.TraceHipError):
        t.accumulate_motion(np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F), None, np.zeros((4, 3), mm.ID_DTYPE), None, None, None)
    scene, sampler = ms.moving_scene(T), T.SeededSampler(2, seed=3)
    sessions = {"an upscaler": T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler()), "variance_guided": T.PreviewSession(scene, sampler, 3, variance_guided=True),
                "temporal_upsample": T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler(), temporal_upsample=T.TemporalUpsampler()),
                "clipping or moments": T.PreviewSession(scene, sampler, 3, temporal=T.TemporalAccumulator(clip_gamma=2.0))}
    for sentence, session in sessions.items():
        with pytest.raises(T.TraceHipError, match=sentence):  # refused before anything touches a device
            session.render(cam, motion={})
        with pytest.raises(T.TraceHipError, match=sentence):
            session._check_motion({ms.SPHERE_INDEX: T.translate([0.1, 0, 0])})
    with pytest.raises(T.TraceHipError, match="dict"):
        T.PreviewSession(scene, sampler, 3).render(cam, motion=[T.translate([0.1, 0, 0])])
    with pytest.raises(T.TraceHipError, match="device_out"):
        T.AOVIntegrator(cam, sampler).render(scene, device_ids=1234)
