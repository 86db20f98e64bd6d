"""Temporal upsampling under motion (trhip_temporal_upsample_motion; docs/design/22-upsample-motion.md), the part that needs no GPU: the entry points and the parameter
block's layout (header text == ctypes mirror, 128 bytes), the default parameters, the refusals and their order through a NULL context, the identities (a) - (c) of the
numpy model (tests/temporal_upsample_motion_model.py) with the two models it descends from, the branch tally on the frames the kernel is given, the Python classes'
refusals, and the history kept on frames made from the oracle's geometry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import julia_replay as jr
import motion_model as mm
import motion_scenes as ms
import temporal_upsample_model as tum
import temporal_upsample_motion_model as tumm
import upscale_model as um
from test_motion_api import centre_ray_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
NAN = float("nan")
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_temporal_upsample_motion_default_params", "trhip_temporal_upsample_motion", "trhip_temporal_upsample_motion_device")
# the sizes of tests/test_gpu_temporal_upsample_motion.py: (full-size h, w) <- (low h, w)
SIZES = {"1x1<-1x1": ((1, 1), (1, 1)), "5x3<-3x2": ((3, 5), (2, 3)), "37x29<-19x15": ((29, 37), (15, 19)), "64x64<-32x32": ((64, 64), (32, 32)),
         "48x32<-12x8": ((32, 48), (8, 12)), "33x17<-33x17": ((17, 33), (17, 33))}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def synthetic(name):
    (hh, hw), (lh, lw) = SIZES[name]
    return tumm.synthetic(hh, hw, lh, lw, 4000 + hw)


# ---- the C interface -------------------------------------------------------------------------------------------------------------------------------------------------
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
    # trhip_temporal_upsample's arguments in its order, with trhip_temporal_motion's ids, body_of_prim, bodies directly after history
    for suffix in ("", "_device"):
        parent, motion = protos["trhip_temporal_upsample" + suffix][1], protos["trhip_temporal_motion" + suffix][1]
        assert protos["trhip_temporal_upsample_motion" + suffix][1] == parent[:7] + motion[4:7] + parent[7:], suffix
    assert T.lib().trhip_version() == 3001, "added without a version change"


def test_params_mirror_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracehip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_temporal_upsample_motion_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == [("base", "trhip_temporal_upsample_params"), ("n_prims", "uint32_t"), ("n_bodies", "uint32_t"), ("motion_flags", "uint32_t"), ("reserved2", "uint32_t")]
    S = T._ffi.TemporalUpsampleMotionParams
    assert [n for n, _ in S._fields_] == [n for n, _ in fields]
    assert S._fields_[0][1] is T._ffi.TemporalUpsampleParams and [t for _, t in S._fields_[1:]] == [C.c_uint32] * 4
    assert C.sizeof(S) == 128 and C.sizeof(T._ffi.TemporalUpsampleParams) == 112
    assert [getattr(S, n).offset for n, _ in fields] == [0, 112, 116, 120, 124]


def good_params(T, **over):
    p = T._ffi.TemporalUpsampleMotionParams()
    assert T.lib().trhip_temporal_upsample_motion_default_params(C.byref(p)) == 0
    p.base.lo_from_hi[:] = [0.5, -0.25, 0.5, -0.25]  # the defaults leave the map zero, which is refused: the map has to be given
    for k, v in over.items():
        if k == "matrix_entry":
            p.base.prev_world_to_pixel[v[0]] = v[1]
        elif k == "map_entry":
            p.base.lo_from_hi[v[0]] = v[1]
        elif k == "reserved":
            p.base.reserved[v[0]] = v[1]
        elif hasattr(p.base, k) and not hasattr(p, k):
            setattr(p.base, k, v)
        else:
            setattr(p, k, v)
    return p


def test_default_params_need_no_context(T):
    p = T._ffi.TemporalUpsampleMotionParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert T.lib().trhip_temporal_upsample_motion_default_params(C.byref(p)) == 0
    base = T._ffi.TemporalUpsampleParams()
    assert T.lib().trhip_temporal_upsample_default_params(C.byref(base)) == 0
    assert bytes(p.base) == bytes(base), "trhip_temporal_upsample_default_params' base"
    assert (p.base.radius, p.base.max_history, p.base.confidence_floor, p.base.confidence_sharpness) == (1, 8.0, 0.0625, 2.0), "19's defaults stay"
    assert (p.n_prims, p.n_bodies, p.motion_flags, p.reserved2) == (0, 0, 0, 0)
    assert T.lib().trhip_temporal_upsample_motion_default_params(None) == INVALID


# trhip_temporal_upsample's block checks in its order, then motion_flags, then reserved2
BAD_PARAMS = [(dict(map_entry=(0, NAN)), b"lo_from_hi"), (dict(map_entry=(0, 0.2)), b"lo_from_hi"), (dict(map_entry=(2, 1.5)), b"lo_from_hi"), (dict(map_entry=(1, 2.0 ** 21)), b"lo_from_hi"),
              (dict(radius=0), b"radius"), (dict(radius=3), b"radius"), (dict(guide_sigma_normal=0.0), b"guide_sigma_normal"), (dict(guide_sigma_plane=NAN), b"guide_sigma_plane"),
              (dict(min_coverage=-0.1), b"min_coverage"), (dict(min_coverage=NAN), b"min_coverage"), (dict(flags=1), b"flag bits"), (dict(reserved=(0, 1)), b"reserved must"),
              (dict(reserved=(1, 5)), b"reserved must"), (dict(matrix_entry=(0, NAN)), b"prev_world_to_pixel"), (dict(matrix_entry=(11, INF)), b"prev_world_to_pixel"),
              (dict(max_history=0.5), b"max_history"), (dict(max_history=INF), b"max_history"), (dict(sigma_normal=0.0), b" sigma_normal"), (dict(sigma_plane=-1.0), b" sigma_plane"),
              (dict(confidence_floor=0.0), b"confidence_floor"), (dict(confidence_floor=1.5), b"confidence_floor"), (dict(confidence_floor=NAN), b"confidence_floor"),
              (dict(confidence_sharpness=-1.0), b"confidence_sharpness"), (dict(confidence_sharpness=4.5), b"confidence_sharpness"),
              (dict(motion_flags=1), b"motion_flags"), (dict(motion_flags=0x80000000), b"motion_flags"), (dict(reserved2=1), b"reserved2")]
ORDER = [dict(map_entry=(2, NAN)), dict(radius=7), dict(guide_sigma_normal=-1.0), dict(guide_sigma_plane=0.0), dict(min_coverage=2.0), dict(flags=2), dict(reserved=(1, 7)),
         dict(matrix_entry=(5, NAN)), dict(max_history=0.0), dict(sigma_normal=0.0), dict(sigma_plane=-1.0), dict(confidence_floor=2.0), dict(confidence_sharpness=9.0),
         dict(motion_flags=4), dict(reserved2=3)]
ORDER_WORDS = [b"lo_from_hi", b"radius", b"guide_sigma_normal", b"guide_sigma_plane", b"min_coverage", b"flag bits", b"reserved must", b"prev_world_to_pixel", b"max_history",
               b" sigma_normal", b" sigma_plane", b"confidence_floor", b"confidence_sharpness", b"motion_flags", b"reserved2"]


@pytest.mark.parametrize("entry", ["trhip_temporal_upsample_motion", "trhip_temporal_upsample_motion_device"])
def test_refusals_and_their_order_without_a_device(T, entry):
    """No context exists here, so every call is refused.  The parameter block is checked first, all of it — the message kept for trhip_last_error(NULL) names the field, and
    of two bad fields the earlier one —, then the pointers."""
    fn, L = getattr(T.lib(), entry), T.lib()
    host = entry == "trhip_temporal_upsample_motion"
    lo, lp, hp = np.zeros((1, 1, 4), F), np.zeros((1, 1, 3, 4), F), np.zeros((2, 2, 3, 4), F)
    out, out_h, mask = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((2, 2), np.uint8)
    ids, table, mats = np.zeros((2, 2), mm.ID_DTYPE), np.zeros(3, np.uint32), np.zeros((1, 12), F)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    fp = (lambda a: T._ffi.fptr(a)) if host else vp
    up = (lambda a: T._ffi.u32ptr(a)) if host else vp
    bp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))) if host else vp

    def call(prm, lo_=lo, idp=ids, tb=table, mt=mats):
        return fn(None, fp(lo_) if lo_ is not None else None, fp(lp), 1, 1, fp(hp), None, vp(idp) if idp is not None else None, up(tb) if tb is not None else None,
                  fp(mt) if mt is not None else None, 2, 2, C.byref(prm) if prm is not None else None, fp(out), fp(out_h), bp(mask), None)
    for over, word in BAD_PARAMS:
        assert call(good_params(T, **over)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    assert len(ORDER) == len(ORDER_WORDS)
    for k in range(len(ORDER)):
        for j in range(k + 1, len(ORDER)):
            assert call(good_params(T, **ORDER[k], **ORDER[j])) == INVALID
            assert ORDER_WORDS[k] in L.trhip_last_error(None), (ORDER[k], ORDER[j], L.trhip_last_error(None))
    assert call(None) == INVALID and b"null argument" in L.trhip_last_error(None)  # no parameter block
    # a bad block and missing pointers: the block is reported
    assert call(good_params(T, reserved2=1), lo_=None, idp=None) == INVALID and b"reserved2" in L.trhip_last_error(None)
    assert call(good_params(T, motion_flags=1, n_prims=3), idp=None, tb=None) == INVALID and b"motion_flags" in L.trhip_last_error(None)
    # a good block: the null context is a null pointer, reported before the table rules and before the rule about ids
    for prm in (good_params(T), good_params(T, n_prims=3, n_bodies=1), good_params(T, n_prims=3)):
        assert call(prm) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert call(good_params(T, n_prims=3, n_bodies=1), idp=None, tb=None, mt=None) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any() and not out_h.any() and not mask.any()


# ---- the model's identities ----------------------------------------------------------------------------------------------------------------------------------------
def static_variants(ids, table, bodies):
    """The ways of saying "every pixel is static"."""
    words = np.where(np.arange(table.size) % 2 == 0, np.uint32(mm.STATIC), np.uint32(len(bodies)) + np.arange(table.size, dtype=np.uint32)).astype(np.uint32)
    return {"ids NULL": (None, None, None), "ids NULL, tables given": (None, table, bodies), "no table": (ids, None, bodies), "no matrices": (ids, table, None),
            "no table, no matrices": (ids, None, None), "every table word >= n_bodies": (ids, words, bodies)}


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_model_identities_a_b_c(size, radius):
    """(a) every pixel static: temporal_upsample_model bit for bit, film, history and mask.  (b) history None: upscale_model's film and mask bit for bit, whatever the bodies
    are.  (c) words 1 and 2 of out_history and the .w lane never depend on the bodies."""
    lo, lp, hp, m, Hs, M, ids, table, bodies = synthetic(size)
    prm = tumm.Params(m, radius=radius)
    want = tum.accumulate(lo, lp, hp, Hs, M, prm)
    moved = tumm.accumulate(lo, lp, hp, Hs, M, ids, table, bodies, prm)
    for what, (i, t, b) in static_variants(ids, table, bodies).items():
        tally = {}
        got = tumm.accumulate(lo, lp, hp, Hs, M, i, t, b, prm, tally)
        assert same_bits(got, want), ("(a)", what)
        assert tally["moving"] == 0
    up_film, up_mask = um.upscale(lo, lp, hp, tum.upscale_params(prm))[:2]
    for what, (i, t, b) in {"the bodies": (ids, table, bodies), **static_variants(ids, table, bodies)}.items():
        film, hist, mask = tumm.accumulate(lo, lp, hp, None, None, i, t, b, prm)
        assert same_bits((film, mask), (up_film, up_mask)), ("(b)", what)
        assert same_bits((hist,), (tum.accumulate(lo, lp, hp, None, None, prm)[1],)), ("without history the bodies decide nothing", what)
    assert same_bits((moved[1][..., 1:, :], moved[0][..., 3]), (want[1][..., 1:, :], want[0][..., 3])), "(c): the CURRENT n and p, plane 0's weight"
    assert same_bits((moved[0][..., 3],), (np.ascontiguousarray(hp[..., 0, 3]),))
    assert np.array_equal(moved[2] & 3, want[2] & 3), "the class is part U's"
    if hp.shape[0] * hp.shape[1] > 100:
        assert not same_bits(moved, want), "the bodies change something"
    assert np.isfinite(moved[0][..., :3]).all() and np.isfinite(moved[1]).all(), "every output is finite whatever the inputs hold"


def test_model_takes_every_branch_on_the_frames_the_kernel_is_given():
    """Over the sizes of the GPU test every branch is taken, with R = 1 and with R = 2: moving, moving with a non-finite carry, static by each of the four reasons (the table
    or the matrices missing: on the frames of identity (a), as is 'ids NULL'), and every branch of 19-temporal-upsample.md's own tally; on the 37 x 29 frame alone every
    one that a single call can take."""
    for radius in (1, 2):
        total = dict.fromkeys(tumm.TALLY_KEYS, 0)
        for size in sorted(SIZES):
            lo, lp, hp, m, Hs, M, ids, table, bodies = synthetic(size)
            for args in ((ids, table, bodies), (ids, table, None), (None, None, None)):
                tally = {}
                tumm.accumulate(lo, lp, hp, Hs, M, *args, tumm.Params(m, radius=radius), tally)
                for k, v in tally.items():
                    total[k] += v
                if size == "37x29<-19x15" and args[2] is not None:
                    assert all(tally[k] > 0 for k in tumm.BRANCHES), (radius, {k: tally[k] for k in tumm.BRANCHES if tally[k] == 0})
                    assert tally["moving"] >= 100 and tally["moving_non_finite"] >= 20 and tally["moving_found"] >= 20, tally
                    assert min(tally["static_no_hit"], tally["static_prim_out_of_range"], tally["static_by_index"]) >= 20, tally
        assert all(total[k] > 0 for k in tumm.TALLY_KEYS), (radius, {k: v for k, v in total.items() if v == 0})
    lo, lp, hp, m, Hs, M, ids, table, bodies = synthetic("64x64<-32x32")
    prim = ids["prim"]
    assert (prim < -1).sum() >= 20 and (prim == np.iinfo(np.int32).min).any() and (prim > 1 << 20).sum() >= 20 and (prim == np.iinfo(np.int32).max).any()
    assert {int(x) for x in table[mm.N_MOVING_PRIMS:]} >= {len(bodies), 65536, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF}
    assert np.isinf(bodies).any(), "one infinite matrix"
    assert np.isinf(lo).sum() >= 2 and np.isnan(lo).sum() >= 1 and np.isinf(Hs).sum() >= 2 and np.isnan(Hs).sum() >= 1, "NaN and +-Inf in film and history"
    assert len(np.unique(ids["material"])) > 1000 and len(np.unique(ids["n_hit"])) > 1000, "random bits in the id words the pass does not read"


# ---- Python --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_classes(T):
    plain, tu = T.TemporalUpsampler(), T.TemporalUpsampler(carry_bodies=True, max_history=4)
    assert plain.carry_bodies is False and tu.carry_bodies is True
    cam = ms.camera(T, 16)
    p = tu._motion_params_for((0.5, 0.25, 0.5, -0.25), cam, 7, 2)
    assert isinstance(p, T._ffi.TemporalUpsampleMotionParams)
    assert (p.n_prims, p.n_bodies, p.motion_flags, p.reserved2, p.base.max_history, p.base.radius) == (7, 2, 0, 0, 4.0, 1)
    assert list(p.base.lo_from_hi) == [0.5, 0.25, 0.5, -0.25] and list(p.base.prev_world_to_pixel) == cam.world_to_pixel().reshape(-1).tolist()
    assert bytes(p.base) == bytes(tu._params_for((0.5, 0.25, 0.5, -0.25), cam)), "the base is the block trhip_temporal_upsample would get"
    lo, lp, hp = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((4, 4, 3, 4), F)
    ids = np.zeros((4, 4), mm.ID_DTYPE)
    m = (0.5, -0.25, 0.5, -0.25)
    # without carry_bodies: a sentence that says to build the upsampler with it
    with pytest.raises(T.TraceHipError, match="carry_bodies=True"):
        plain.accumulate_motion(lo, lp, hp, None, ids, None, None, m, None)
    with pytest.raises(T.TraceHipError, match="carry_bodies=True"):
        plain.accumulate_motion_device(1, 2, 2, 2, 3, None, 4, None, 0, None, 0, 4, 4, m, None, 5, 6)
    # shapes are checked before anything touches a device; ids is the FULL-SIZE frame's
    for bad in (dict(ids=np.zeros((2, 2), mm.ID_DTYPE)), dict(ids=np.zeros((4, 3), mm.ID_DTYPE)), dict(lp=lp[:1]), dict(hp=hp[..., :2, :]), dict(hist=np.zeros((4, 3, 3, 4), F)),
                dict(m=m[:3])):
        a = dict(lo=lo, lp=lp, hp=hp, hist=None, ids=ids, m=m)
        a.update(bad)
        with pytest.raises(T.TraceHipError):
            tu.accumulate_motion(a["lo"], a["lp"], a["hp"], a["hist"], a["ids"], None, None, a["m"], None)
    with pytest.raises(T.TraceHipError):
        tu.accumulate(lo, lp[:1], hp, None, m, None)
    # the session: motion with temporal_upsample only when the upsampler carries bodies
    scene, sampler = ms.moving_scene(T), T.SeededSampler(2, seed=3)
    motion = {ms.SPHERE_INDEX: T.translate([0.1, 0, 0])}
    refused = T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler(), temporal_upsample=T.TemporalUpsampler())
    for mo in ({}, motion):
        with pytest.raises(T.TraceHipError, match=r"temporal_upsample.*carry_bodies=True"):
            refused._check_motion(mo)
    with pytest.raises(T.TraceHipError, match="temporal_upsample"):  # refused before anything touches a device
        refused.render(cam, motion={})
    ok = T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler(), temporal_upsample=tu)
    ok._check_motion({})
    ok._check_motion(motion)
    with pytest.raises(T.TraceHipError, match="dict"):
        ok._check_motion([motion])
    # what stays refused as it was
    with pytest.raises(T.TraceHipError, match="an upscaler"):
        T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler())._check_motion({})
    with pytest.raises(T.TraceHipError, match="variance_guided"):
        T.PreviewSession(scene, sampler, 3, variance_guided=True)._check_motion({})
    with pytest.raises(T.TraceHipError, match="clipping or moments"):
        T.PreviewSession(scene, sampler, 3, temporal=T.TemporalAccumulator(moments=True))._check_motion({})
    with pytest.raises(T.TraceHipError, match="variance_guided"):
        T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler(), temporal_upsample=tu, variance_guided=True)
    with pytest.raises(T.TraceHipError, match="clipping or moments"):
        T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler(), temporal_upsample=tu, temporal=T.TemporalAccumulator(clip_gamma=1.0))


# ---- history kept --------------------------------------------------------------------------------------------------------------------------------------------------
def test_moving_bodies_keep_their_full_size_history_on_frames_from_the_oracles_geometry(T, ob):
    """motion_scenes' sequence — the sphere rises, the cube turns about its own centre, the camera turns —, three frames, 48 x 48 <- 24 x 24 through the jittered low camera
    of each frame, with frames made from the oracle's hits at the pixel centres (tests/test_motion_api.py's centre_ray_frame at both sizes).  At frame 3, per body: the
    full-size surface pixels whose mask has bit 4 (history found), through this model and through temporal_upsample_model, which ignores the motion.  Strictly more with
    the motion, and more than half.  Whether a tap is found depends on the full-size planes, the stored n, p and Omega > 0 alone — not on the low frame —, so the figures
    are those of 20-motion.md on the same planes.  Counted here: sphere 195 of 195 (161 motion-blind, 0.826), cube 201 of 201 (179, 0.891)."""
    tu = T.TemporalUpsampler()
    hist, hist_blind, prev = None, None, None
    for k, ((scene, motion), deg) in enumerate(zip(ms.scene_sequence(T, 3), (0.0, 3.0, 6.0))):
        cam = ms.camera(T, 48, deg)
        lo_cam = T.Upscaler.low_camera(cam, 2, jitter=tu.jitter_for(k, 2))
        lo, lp, _, _ = centre_ray_frame(T, ob, scene, lo_cam)
        _, hp, ids, order = centre_ray_frame(T, ob, scene, cam)
        assert lo.shape == (24, 24, 4) and hp.shape == (48, 48, 3, 4)
        counts = T.top_level_counts(scene)
        keys = sorted(motion)
        words = np.full(len(counts), mm.STATIC, np.uint32)
        words[keys] = np.arange(len(keys))
        table = np.repeat(words, counts)[order]
        mats = np.stack([T.TemporalAccumulator.prev_from_cur(motion[i]) for i in keys]) if keys else None
        p = tu.params
        prm = tumm.Params(T.Upscaler.pixel_map(cam, lo_cam), radius=p.radius, max_history=p.max_history, sigma_normal=p.sigma_normal, sigma_plane=p.sigma_plane,
                          min_coverage=p.min_coverage, guide_sigma_normal=p.guide_sigma_normal, guide_sigma_plane=p.guide_sigma_plane, confidence_floor=p.confidence_floor,
                          confidence_sharpness=p.confidence_sharpness)
        M = prev.world_to_pixel() if prev is not None else None
        tally = {}
        _, hist, mask = tumm.accumulate(lo, lp, hp, hist, M, ids, table if keys else None, mats, prm, tally)
        _, hist_blind, mask_blind = tum.accumulate(lo, lp, hp, hist_blind, M, prm)
        prev = cam
    caller = np.repeat(np.arange(len(counts)), counts)[order]  # slot -> top-level entry
    surface = hist[..., 1, 3] == 1
    for name, index in (("sphere", ms.SPHERE_INDEX), ("cube", ms.CUBE_INDEX)):
        on_body = surface & (ids["prim"] >= 0) & (caller[np.where(ids["prim"] >= 0, ids["prim"], 0)] == index)
        n, kept, kept_blind = int(on_body.sum()), int((mask[on_body] & 4 != 0).sum()), int((mask_blind[on_body] & 4 != 0).sum())
        print(f"oracle-geometry sequence at 48^2 <- 24^2, {name}: {n} full-size surface pixels, history found at {kept} with the motion, {kept_blind} motion-blind")
        assert n >= 30 and kept > kept_blind and 2 * kept > n, (name, n, kept, kept_blind)
    assert tally["moving_found"] > 100 and tally["static_by_index"] > 1000, tally
