"""Clipped reprojection under motion (trhip_temporal_clip_motion; docs/design/21-clip-motion.md), the part that needs no GPU: the entry points and the parameter block's layout
(header text == ctypes mirror, 96 bytes), the default parameters, the refusals and their order through a NULL context, the identities (a) - (e) of the numpy model
(tests/clip_motion_model.py) with the two models it descends from, the dyadic one-colour surface, the Python classes' refusals, and the measurement scene's swept mask on the
oracle's frames."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clip_motion_model as cmm
import clip_motion_scenes as cs
import denoise_model as dm
import julia_replay as jr
import motion_model as mm
import motion_scenes as ms
import temporal_clip_model as tcm
import temporal_model as tm
from test_temporal_clip_api import uniform_surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
NAN = float("nan")
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_temporal_clip_motion_default_params", "trhip_temporal_clip_motion", "trhip_temporal_clip_motion_device")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


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
    # trhip_temporal_motion's arguments, in its order
    assert protos["trhip_temporal_clip_motion"][1] == protos["trhip_temporal_motion"][1]
    assert protos["trhip_temporal_clip_motion_device"][1] == protos["trhip_temporal_motion_device"][1]
    assert T.lib().trhip_version() == 3001, "added without a version change"


def test_params_mirror_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracehip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_temporal_clip_motion_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]
    assert fields == [("base", "trhip_temporal_motion_params"), ("clip_gamma", "float"), ("clip_radius", "uint32_t"), ("clip_max_history", "float"), ("reserved2", "uint32_t")]
    S = T._ffi.TemporalClipMotionParams
    assert [n for n, _ in S._fields_] == [n for n, _ in fields]
    assert S._fields_[0][1] is T._ffi.TemporalMotionParams and [t for _, t in S._fields_[1:]] == [C.c_float, C.c_uint32, C.c_float, C.c_uint32]
    assert C.sizeof(S) == 96 and C.sizeof(T._ffi.TemporalMotionParams) == 80
    assert [getattr(S, n).offset for n, _ in fields] == [0, 80, 84, 88, 92]
    # the fields trhip_temporal_params has lie where it has them: temporal_const<> serves base
    for n in ("prev_world_to_pixel", "max_history", "sigma_normal", "sigma_plane", "min_coverage"):
        assert getattr(T._ffi.TemporalMotionParams, n).offset == getattr(T._ffi.TemporalParams, n).offset


def good_params(T, **over):
    p = T._ffi.TemporalClipMotionParams()
    assert T.lib().trhip_temporal_clip_motion_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "matrix_entry":
            p.base.prev_world_to_pixel[v[0]] = v[1]
        elif hasattr(p.base, k) and not hasattr(p, k):
            setattr(p.base, k, v)
        else:
            setattr(p, k, v)
    return p


def test_default_params_need_no_context(T):
    p = T._ffi.TemporalClipMotionParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert T.lib().trhip_temporal_clip_motion_default_params(C.byref(p)) == 0
    base, clip = T._ffi.TemporalMotionParams(), T._ffi.TemporalClipParams()
    assert T.lib().trhip_temporal_motion_default_params(C.byref(base)) == 0 and T.lib().trhip_temporal_clip_default_params(C.byref(clip)) == 0
    assert bytes(p.base) == bytes(base), "trhip_temporal_motion_default_params' base"
    assert (p.clip_gamma, p.clip_radius) == (clip.clip_gamma, clip.clip_radius) == (4.0, 3), "the clip pass's defaults"
    assert p.clip_max_history >= 0.0 and p.reserved2 == 0
    assert p.clip_max_history == DEFAULT_CLIP_MAX_HISTORY, "the cell the rule of docs/design/21-clip-motion.md picked"
    assert T.lib().trhip_temporal_clip_motion_default_params(None) == INVALID


DEFAULT_CLIP_MAX_HISTORY = INF

# trhip_temporal_motion's block checks in its order, then clip_gamma, clip_radius, clip_max_history, reserved2
BAD_PARAMS = [(dict(matrix_entry=(0, NAN)), b"prev_world_to_pixel"), (dict(matrix_entry=(11, INF)), b"prev_world_to_pixel"),
              (dict(max_history=0.5), b"max_history"), (dict(max_history=INF), b"max_history"), (dict(max_history=NAN), b"max_history"),
              (dict(min_coverage=-0.1), b"min_coverage"), (dict(min_coverage=1.5), b"min_coverage"), (dict(min_coverage=NAN), b"min_coverage"),
              (dict(flags=1), b"flag"), (dict(reserved=1), b"reserved must"),
              (dict(clip_gamma=NAN), b"clip_gamma"), (dict(clip_gamma=-1.0), b"clip_gamma"), (dict(clip_gamma=-INF), b"clip_gamma"),
              (dict(clip_radius=0), b"clip_radius"), (dict(clip_radius=4), b"clip_radius"),
              (dict(clip_max_history=NAN), b"clip_max_history"), (dict(clip_max_history=-0.5), b"clip_max_history"), (dict(clip_max_history=-INF), b"clip_max_history"),
              (dict(reserved2=1), b"reserved2")]
for _name in ("sigma_normal", "sigma_plane"):
    BAD_PARAMS += [({_name: v}, _name.encode()) for v in (0.0, -1.0, INF, NAN)]
ORDER = [dict(matrix_entry=(5, NAN)), dict(max_history=0.0), dict(sigma_normal=0.0), dict(sigma_plane=-1.0), dict(min_coverage=2.0), dict(flags=2), dict(reserved=7),
         dict(clip_gamma=NAN), dict(clip_radius=9), dict(clip_max_history=-1.0), dict(reserved2=3)]
ORDER_WORDS = [b"prev_world_to_pixel", b"max_history must be finite", b"sigma_normal", b"sigma_plane", b"min_coverage", b"flag", b"reserved must", b"clip_gamma", b"clip_radius",
               b"clip_max_history", b"reserved2"]


@pytest.mark.parametrize("entry", ["trhip_temporal_clip_motion", "trhip_temporal_clip_motion_device"])
def test_refusals_and_their_order_without_a_device(T, entry):
    """No context exists here, so every call is refused.  The parameter block is checked first — the message kept for trhip_last_error(NULL) names the field, and of two bad
    fields the earlier one —, then the pointers."""
    fn, L = getattr(T.lib(), entry), T.lib()
    host = entry == "trhip_temporal_clip_motion"
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
    assert call(good_params(T, reserved2=1), xyzw=None, idp=None) == INVALID and b"reserved2" in L.trhip_last_error(None)
    # a good block: the null context is a null pointer, reported before the table rules and before the rule about ids
    for prm in (good_params(T), good_params(T, n_prims=3, n_bodies=1), good_params(T, n_prims=3), good_params(T, clip_gamma=INF, clip_max_history=INF),
                good_params(T, clip_gamma=0.0, clip_max_history=0.0)):
        assert call(prm) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert call(good_params(T, n_prims=3, n_bodies=1), idp=None, tb=None, mt=None) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any() and not out_h.any()


# ---- the model's identities ----------------------------------------------------------------------------------------------------------------------------------------
SIZES = [(29, 37), (3, 5), (1, 1)]


def static_variants(ids, table, bodies):
    """The ways of saying "every pixel is static"."""
    words = np.where(np.arange(table.size) % 2 == 0, np.uint32(mm.STATIC), np.uint32(len(bodies)) + np.arange(table.size, dtype=np.uint32)).astype(np.uint32)
    no_hit = ids.copy()
    no_hit["prim"] = -1
    return {"ids NULL": (None, None, None), "ids NULL, tables given": (None, table, bodies), "no table": (ids, None, bodies), "no matrices": (ids, table, None),
            "every word static": (ids, words, bodies), "no pixel hit": (no_hit, table, bodies)}


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for h, w in SIZES])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_model_identities_a_b_c(size, radius):
    """(a) every pixel static and clip_max_history = +Inf: temporal_clip_model bit for bit.  (b) gamma = +Inf: motion_model bit for bit, whatever clip_max_history is.
    (c) both: temporal_model."""
    h, w = size
    B, P, Hs, M, ids, table, bodies = cmm.synthetic(h, w, 2000 + h)
    for history in (Hs, None):
        Mh = M if history is not None else None
        for gamma in (0.0, 1.0, 4.0):
            want = tcm.accumulate(B, P, history, Mh, tcm.params(gamma, radius))
            for what, (i, t, b) in static_variants(ids, table, bodies).items():
                got = cmm.accumulate(B, P, history, Mh, i, t, b, cmm.params(gamma, radius, INF))
                assert same_bits(got, want), ("(a)", what, gamma, history is None)
        want = mm.accumulate(B, P, history, Mh, ids, table, bodies, mm.SYNTHETIC_PARAMS)
        for cmh in (0.0, 1.0, 2.5, INF):
            assert same_bits(cmm.accumulate(B, P, history, Mh, ids, table, bodies, cmm.params(INF, radius, cmh)), want), ("(b)", cmh, history is None)
        want = tm.accumulate(B, P, history, Mh, tm.SYNTHETIC_PARAMS)
        for cmh in (0.0, INF):
            assert same_bits(cmm.accumulate(B, P, history, Mh, None, None, None, cmm.params(INF, radius, cmh)), want), ("(c)", cmh, history is None)
    if h * w > 100:
        moved = cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, radius, INF))
        assert not same_bits(moved, tcm.accumulate(B, P, Hs, M, tcm.params(1.0, radius))), "the bodies change something"
        assert not same_bits(moved, cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, radius, 0.0))), "clip_max_history changes something"
        assert same_bits([moved[1][..., 1:, :]], [mm.accumulate(B, P, Hs, M, ids, table, bodies, mm.SYNTHETIC_PARAMS)[1][..., 1:, :]]), "out_history holds the CURRENT n and p"


def test_model_synthetic_case_takes_every_branch():
    for radius in (1, 2, 3):
        tally = {}
        B, P, Hs, M, ids, table, bodies = cmm.synthetic(29, 37, 2029)
        cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, radius, 2.0), tally)
        for name in cmm.BRANCHES:
            assert tally.get(name, 0) >= 1, (radius, name, tally)
        assert tally["pixels_clipped"] >= 20 and tally["pixels_inside"] >= 20 and tally["history_cut"] >= 20 and tally["moving_clipped"] >= 5 and tally["blended"] >= 100, tally
    assert np.isinf(B).sum() >= 2 and np.isnan(B).sum() >= 1 and np.isinf(Hs).sum() >= 2 and np.isnan(Hs).sum() >= 1, "NaN and +-Inf colours in film and history"


def test_model_d_a_nan_history_colour_is_never_clipped():
    """(d): a NaN c_h holds none of the six comparisons, so `clipped` is false and clip_max_history is not looked at; the pixel then meets the non-finite fallback.  An
    infinite c_h IS clipped (Inf > hi) to a finite bound and blends."""
    h, w = 9, 10
    B, P, n, p = uniform_surface(h, w, 0.25)
    M = F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    Hs = np.zeros((h, w, 3, 4), F)
    Hs[..., 0, :3], Hs[..., 0, 3] = F(0.25), F(8.0)
    Hs[..., 1, :3], Hs[..., 1, 3] = n, F(1.0)
    Hs[..., 2, :3] = p
    Hs[4, 5, 0, 1] = F(NAN)
    Hs[2, 3, 0, 2] = F(INF)
    for cmh in (0.0, 3.0, INF):
        tally = {}
        _, hist = cmm.accumulate(B, P, Hs, M, None, None, None, cmm.Params(8.0, 0.25, 0.1, 0.5, 1.0, 2, cmh), tally)
        # (the taps of weight 0 on the two poisoned records make their left and upper neighbours' c_h NaN as well: 0 * NaN, 0 * Inf)
        assert tally["pixels_clipped"] == 1 and tally["nan_colour"] >= 1 and tally["history_cut"] == (1 if cmh < 8 else 0), (cmh, tally)
        assert np.all(hist[4, 5, 0] == F([0.25, 0.25, 0.25, 1.0])), "the fallback: the frame's own colour, N' = 1"
        assert np.all(hist[2, 3, 0] == F([0.25, 0.25, 0.25, min(cmh, 8.0) + 1 if cmh < 7 else 8.0]))


@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 4.0])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("cmh", [0.0, 1.0, 2.0, 4.0, 7.0, 8.0, 100.0, INF])
def test_model_on_a_uniform_dyadic_surface(gamma, radius, cmh):
    """Colour 0.25, history colour 1.0 with N = 8 under an identity reprojection (tests/test_temporal_clip_api.py explains why the sums are exact): lo = hi = 0.25 for any
    finite gamma, every pixel is clipped, the output is exactly 0.25 and N' = min(min(clip_max_history, 8) + 1, max_history).  With clip_max_history = 0 that is (e): the
    blend with weight 1 and N' = 1."""
    h, w = 9, 10
    B, P, n, p = uniform_surface(h, w, 0.25)
    M = F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    Hs = np.zeros((h, w, 3, 4), F)
    Hs[..., 0, :3], Hs[..., 0, 3] = F(1.0), F(8.0)
    Hs[..., 1, :3], Hs[..., 1, 3] = n, F(1.0)
    Hs[..., 2, :3] = p
    for max_history in (8.0, 16.0):
        tally = {}
        out, hist = cmm.accumulate(B, P, Hs, M, None, None, None, cmm.Params(max_history, 0.25, 0.1, 0.5, gamma, radius, cmh), tally)
        assert tally["blended"] == h * w and tally["pixels_clipped"] == h * w and tally["history_cut"] == (h * w if cmh < 8 else 0)
        assert np.all(hist[..., 0, :3] == F(0.25)), "exactly 0.25 after one frame"
        assert np.all(hist[..., 0, 3] == F(min(min(cmh, 8.0) + 1.0, max_history))), "N' = min(clip_max_history, 8) + 1, capped"
        assert np.array_equal(bits(out[..., :3]), bits(np.broadcast_to(dm.rgb_to_xyz(np.full(3, 0.25, F)), (h, w, 3))))


def test_model_e_zero_clip_max_history_restarts_a_clipped_pixel():
    """(e) on the synthetic frame: with clip_max_history = 0 every pixel that was clipped (and blended) has N' = 1, and its colour is c_h + 1 * (c - c_h)."""
    B, P, Hs, M, ids, table, bodies = cmm.synthetic(29, 37, 2029)
    _, cut = cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, 2, 0.0))
    _, kept = cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, 2, INF))
    differs = cut[..., 0, 3] != kept[..., 0, 3]
    assert differs.sum() >= 20 and np.all(cut[differs][:, 0, 3] == 1.0) and np.all(kept[differs][:, 0, 3] > 1.0)
    assert np.all(cut[..., 0, 3] <= kept[..., 0, 3])


# ---- Python --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_classes(T):
    t = T.TemporalAccumulator(clip_gamma=2.0, carry_bodies=True)
    assert t.clip_params is not None and t.clip_motion_params is not None and t.clip_motion_params.clip_max_history == DEFAULT_CLIP_MAX_HISTORY
    cam = ms.camera(T, 16)
    p = T.TemporalAccumulator(max_history=4, clip_gamma=0.5, clip_radius=1, carry_bodies=True, clip_max_history=2.0)._clip_motion_params_for(cam, 7, 2)
    assert isinstance(p, T._ffi.TemporalClipMotionParams)
    assert (p.base.max_history, p.base.n_prims, p.base.n_bodies, p.base.flags, p.base.reserved) == (4.0, 7, 2, 0, 0)
    assert (p.clip_gamma, p.clip_radius, p.clip_max_history, p.reserved2) == (0.5, 1, 2.0, 0)
    assert list(p.base.prev_world_to_pixel) == cam.world_to_pixel().reshape(-1).tolist()
    assert T.TemporalAccumulator(clip_gamma=1.0, carry_bodies=True, clip_max_history=INF).clip_motion_params.clip_max_history == INF
    with pytest.raises(T.TraceHipError, match="clip_gamma"):
        T.TemporalAccumulator(carry_bodies=True)
    with pytest.raises(T.TraceHipError, match="clip_gamma"):
        T.TemporalAccumulator(clip_radius=2, carry_bodies=True)
    with pytest.raises(T.TraceHipError, match="carry_bodies"):
        T.TemporalAccumulator(clip_gamma=1.0, clip_max_history=2.0)
    with pytest.raises(T.TraceHipError, match="carry_bodies"):
        T.TemporalAccumulator(clip_max_history=2.0)
    with pytest.raises(T.TraceHipError, match="moments=True cannot be combined with carry_bodies"):
        T.TemporalAccumulator(moments=True, carry_bodies=True)
    # what stays: without carry_bodies a clipping accumulator has no motion call, and the session refuses it with `motion`
    with pytest.raises(T.TraceHipError, match="plain accumulator"):
        T.TemporalAccumulator(clip_gamma=1.0)._motion_params_for(None, 0, 0)
    scene, sampler = ms.moving_scene(T), T.SeededSampler(2, seed=3)
    with pytest.raises(T.TraceHipError, match=r"clipping or moments.*carry_bodies=True"):
        T.PreviewSession(scene, sampler, 3, temporal=T.TemporalAccumulator(clip_gamma=2.0))._check_motion({})
    ok = T.PreviewSession(scene, sampler, 3, temporal=t)
    ok._check_motion({})
    ok._check_motion({ms.SPHERE_INDEX: T.translate([0.1, 0, 0])})
    for sentence, kw in (("an upscaler", dict(upscaler=T.Upscaler())), ("variance_guided", dict(variance_guided=True, temporal=None))):
        session = T.PreviewSession(scene, sampler, 3, **{"temporal": t, **kw})
        with pytest.raises(T.TraceHipError, match=sentence):
            session._check_motion({})
    with pytest.raises(T.TraceHipError, match="clipping or moments"):
        T.PreviewSession(scene, sampler, 3, upscaler=T.Upscaler(), temporal_upsample=T.TemporalUpsampler(), temporal=t)
    with pytest.raises(T.TraceHipError):  # shapes are checked before anything touches a device
        t.accumulate_motion(np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F), None, np.zeros((4, 3), mm.ID_DTYPE), None, None, None)
    with pytest.raises(T.TraceHipError):
        t.accumulate(np.zeros((4, 4, 4), F), np.zeros((4, 3, 3, 4), F), None, None)


# ---- the measurement scene -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_shadow_sweeps_enough_static_surface_on_the_oracles_frames(T, ob):
    """The swept mask of tests/test_gpu_clip_motion.py's quality figures, formed from the ORACLE's frames before anything goes to a GPU: 64 x 64, still camera, the first and
    the eighth pose of clip_motion_scenes.scene_sequence at 1024 spp, depth 5; static surface pixels from one ray through each pixel centre at the last pose.  It must hold at
    least 2 % of the static surface pixels.  Counted here: 1001 of 3228 (31 %) — the sphere's shadow falls on the floor and climbs the back wall, and both its old and its new
    place count; on the 0.75-degree arc's last camera 1026 of 3338."""
    frames = cs.scene_sequence(T, 8)
    cam = ms.camera(T, 64, 0.0)
    h, w = cam.film.size
    threads = min(16, os.cpu_count() or 1)
    films = [ob.OracleScene.from_scene(scene).render(cam, "path", 1024, 5, seed=0x7A26E7, threads=threads)[0] for scene in (frames[0][0], frames[-1][0])]
    scene = frames[-1][0]
    cmin = np.asarray(cam.film.crop_bounds.p_min, np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    samples = np.stack([cmin[0] + xs + 0.5, cmin[1] + ys + 0.5, np.full((h, w), 0.5), np.full((h, w), 0.5), np.zeros((h, w))], -1).reshape(-1, 5).astype(F)
    osc = ob.OracleScene.from_scene(scene)
    prim = osc.trace_closest(ob.generate_rays(cam, samples), want_geom=True)[1].reshape(h, w)
    counts = T.top_level_counts(scene)
    entry = np.repeat(np.arange(len(counts)), counts)[osc.get_bvh()[3]][np.where(prim >= 0, prim, 0)]
    static = (prim >= 0) & (entry != ms.SPHERE_INDEX) & (entry != ms.CUBE_INDEX)
    swept = cs.swept_mask(static, films[0], films[1])
    print(f"swept mask on the oracle's frames: {int(swept.sum())} of {int(static.sum())} static surface pixels")
    assert static.sum() > 2000 and swept.sum() >= 0.02 * static.sum(), (int(swept.sum()), int(static.sum()))
    assert ((prim >= 0) & (entry == ms.SPHERE_INDEX)).sum() >= 100, "the sphere is still in view at the last pose"
