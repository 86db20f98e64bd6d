"""Clipped reprojection under motion on the GPU (trhip_temporal_clip_motion; docs/design/21-clip-motion.md): the kernel against the numpy model of tests/clip_motion_model.py
bit for bit — on synthetic frames that take every branch and hold garbage ids, body words and non-finite colours, at every radius, with and without history, and on the real
three-frame sequence of motion_scenes —; the identities with trhip_temporal_clip and trhip_temporal_motion on the device; host == device, aliasing, ids NULL, the refusals
that need a context; PreviewSession with a carry_bodies accumulator; and the quality figures (QUALITY_MEASURED, also in docs/design/21-clip-motion.md)."""
import ctypes as C

import numpy as np
import pytest

import clip_motion_model as cmm
import clip_motion_scenes as cs
import denoise_model as dm
import motion_scenes as ms
from test_gpu_motion import SEQUENCE, assert_bits_equal, bits, body_inputs, frame, slot_to_entry

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")
SIZES = [(1, 1), (5, 3), (37, 29), (64, 64)]  # a single lane, smaller than a window, several tiles and off the tile edge, sixteen blocks
SYNTHETIC = {}


def synthetic(w, h):
    """(B, P, history, M, ids, table, bodies): computed once per size and left unchanged."""
    if (w, h) not in SYNTHETIC:
        SYNTHETIC[(w, h)] = cmm.synthetic(h, w, 2000 + h)
    return tuple(a.copy() for a in SYNTHETIC[(w, h)])


def accumulator(T, gamma, radius, cmh=None, carry=True):
    s = cmm.params(gamma, radius)
    kw = dict(carry_bodies=True, clip_max_history=cmh) if carry else {}
    return T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage, clip_gamma=gamma, clip_radius=radius, **kw)


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_frames_equal_the_model(T, ctx, size, radius):
    w, h = size
    B, P, Hs, M, ids, table, bodies = synthetic(w, h)
    for cmh in (0.0, 2.0, INF):
        prm, tally = cmm.params(1.0, radius, cmh), {}
        ref_out, ref_hist = cmm.accumulate(B, P, Hs, M, ids, table, bodies, prm, tally)
        if w * h > 1000 and cmh == 2.0:
            for name in cmm.BRANCHES:
                assert tally.get(name, 0) >= 1, (name, tally)
            assert tally["history_cut"] >= 20 and tally["moving_clipped"] >= 5, tally
        t = accumulator(T, 1.0, radius, cmh)
        out, hist = t.accumulate_motion(B, P, Hs, ids, table, bodies, M, ctx)
        assert_bits_equal(out, ref_out, f"clip_max_history {cmh}: out_xyzw")
        assert_bits_equal(hist, ref_hist, f"clip_max_history {cmh}: out_history")
        assert t.stats.launches_film == 1
    assert_bits_equal(out[..., 3], B[..., 3], "the weight lane")
    # without history
    ref0 = cmm.accumulate(B, P, None, None, ids, table, bodies, prm)
    out0, hist0 = t.accumulate_motion(B, P, None, ids, table, bodies, None, ctx)
    assert_bits_equal(out0, ref0[0], "history = NULL, out_xyzw")
    assert_bits_equal(hist0, ref0[1], "history = NULL, out_history")
    # gamma = 0 (every history colour goes to the window's mean) and the default gamma
    for gamma in (0.0, 4.0):
        ref = cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(gamma, radius, 2.0))
        got = accumulator(T, gamma, radius, 2.0).accumulate_motion(B, P, Hs, ids, table, bodies, M, ctx)
        assert_bits_equal(got[0], ref[0], f"gamma {gamma}: out_xyzw")
        assert_bits_equal(got[1], ref[1], f"gamma {gamma}: out_history")


@pytest.mark.parametrize("size", [(37, 29), (64, 64)], ids=["37x29", "64x64"])
def test_identities_with_the_two_shipped_kernels_on_the_device(T, ctx, size):
    """(a) every pixel static and clip_max_history = +Inf: trhip_temporal_clip's bits.  (b) clip_gamma = +Inf: trhip_temporal_motion's, whatever clip_max_history is.
    (c) both: trhip_temporal's."""
    w, h = size
    B, P, Hs, M, ids, table, bodies = synthetic(w, h)
    s = cmm.params(1.0, 1)
    plain = T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage)
    words = np.where(np.arange(table.size) % 2 == 0, np.uint32(0xFFFFFFFF), np.uint32(len(bodies)) + np.arange(table.size, dtype=np.uint32)).astype(np.uint32)
    for history in (Hs, None):
        Mh = M if history is not None else None
        motion_out, motion_hist = plain.accumulate_motion(B, P, history, ids, table, bodies, Mh, ctx)
        for radius in (1, 2, 3):
            for gamma in (0.5, 4.0):
                clip_out, clip_hist = accumulator(T, gamma, radius, carry=False).accumulate(B, P, history, Mh, ctx)
                t = accumulator(T, gamma, radius, INF)
                for what, got in (("accumulate (ids NULL)", t.accumulate(B, P, history, Mh, ctx)), ("no table", t.accumulate_motion(B, P, history, ids, None, bodies, Mh, ctx)),
                                  ("no matrices", t.accumulate_motion(B, P, history, ids, table, None, Mh, ctx)),
                                  ("every word static", t.accumulate_motion(B, P, history, ids, words, bodies, Mh, ctx))):
                    assert_bits_equal(got[0], clip_out, f"(a) R {radius}, gamma {gamma}, {what}: out_xyzw against trhip_temporal_clip")
                    assert_bits_equal(got[1], clip_hist, f"(a) R {radius}, gamma {gamma}, {what}: out_history against trhip_temporal_clip")
            for cmh in (0.0, 2.0, INF):
                got = accumulator(T, INF, radius, cmh).accumulate_motion(B, P, history, ids, table, bodies, Mh, ctx)
                assert_bits_equal(got[0], motion_out, f"(b) R {radius}, clip_max_history {cmh}: out_xyzw against trhip_temporal_motion")
                assert_bits_equal(got[1], motion_hist, f"(b) R {radius}, clip_max_history {cmh}: out_history against trhip_temporal_motion")
            got = accumulator(T, INF, radius, 0.0).accumulate(B, P, history, Mh, ctx)
            want = plain.accumulate(B, P, history, Mh, ctx)
            assert_bits_equal(got[0], want[0], f"(c) R {radius}: out_xyzw against trhip_temporal")
            assert_bits_equal(got[1], want[1], f"(c) R {radius}: out_history against trhip_temporal")
        assert history is None or not np.array_equal(bits(motion_out), bits(clip_out)), "with a history the two parents differ on this frame"


def test_host_device_aliased_and_null_ids_calls_agree(T, ctx):
    B, P, Hs, M, ids, table, bodies = synthetic(37, 29)
    h, w = B.shape[:2]
    t = accumulator(T, 1.0, 2, 2.0)
    ref_out, ref_hist = cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, 2, 2.0))
    inputs = (B, P, Hs, ids, table, bodies)
    d_in, d_pl, d_hs, d_ids, d_tb, d_mt = (T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in inputs)
    d_out, d_oh = T._ffi.DeviceBuffer(B.nbytes).zero(), T._ffi.DeviceBuffer(P.nbytes).zero()
    t.accumulate_motion_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_ids.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, M, d_out.ptr, d_oh.ptr, ctx)
    assert_bits_equal(d_out.to_host(F, B.shape), ref_out, "device variant, out_xyzw")
    assert_bits_equal(d_oh.to_host(F, P.shape), ref_hist, "device variant, out_history")
    for buf, a, what in zip((d_in, d_pl, d_hs, d_ids, d_tb, d_mt), inputs, ("xyzw", "planes", "history", "ids", "body_of_prim", "bodies")):
        assert buf.to_host(a.dtype, a.shape).tobytes() == a.tobytes(), f"the input {what} is left alone"
    # ids NULL == an id plane of all -1 == accumulate_device
    none = ids.copy()
    none["prim"] = -1
    d_none = T._ffi.DeviceBuffer(none.nbytes).from_host(none)
    static_out, static_hist = cmm.accumulate(B, P, Hs, M, None, None, None, cmm.params(1.0, 2, 2.0))
    for what, call in (("ids of -1", lambda: t.accumulate_motion_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_none.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, M, d_out.ptr, d_oh.ptr, ctx)),
                       ("ids NULL", lambda: t.accumulate_motion_device(d_in.ptr, d_pl.ptr, d_hs.ptr, None, None, 0, None, 0, w, h, M, d_out.ptr, d_oh.ptr, ctx)),
                       ("accumulate_device", lambda: t.accumulate_device(d_in.ptr, d_pl.ptr, d_hs.ptr, w, h, M, d_out.ptr, d_oh.ptr, ctx))):
        d_out.zero(), d_oh.zero()
        call()
        assert_bits_equal(d_out.to_host(F, B.shape), static_out, f"{what}: out_xyzw")
        assert_bits_equal(d_oh.to_host(F, P.shape), static_hist, f"{what}: out_history")
    got = t.accumulate_motion(B, P, Hs, none, table, bodies, M, ctx)
    assert_bits_equal(got[0], static_out, "host, ids of -1")
    assert_bits_equal(got[1], static_hist, "host, ids of -1, out_history")
    got = t.accumulate(B, P, Hs, M, ctx)
    assert_bits_equal(got[0], static_out, "host, ids NULL")
    assert_bits_equal(got[1], static_hist, "host, ids NULL, out_history")
    # out_xyzw == xyzw: the window reads neighbours' film pixels, so the result goes through a film of its own
    d_oh.zero()
    t.accumulate_motion_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_ids.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, M, d_in.ptr, d_oh.ptr, ctx)
    assert_bits_equal(d_in.to_host(F, B.shape), ref_out, "out aliasing xyzw, device")
    assert_bits_equal(d_oh.to_host(F, P.shape), ref_hist, "out aliasing xyzw, device, out_history")
    buf, hist = B.copy(), np.empty_like(P)
    p = t._clip_motion_params_for(M, table.size, len(bodies))
    rc = T.lib().trhip_temporal_clip_motion(ctx._h, T._ffi.fptr(buf), T._ffi.fptr(P), T._ffi.fptr(Hs), ids.ctypes.data_as(C.c_void_p), T._ffi.u32ptr(table), T._ffi.fptr(bodies), w, h,
                                            C.byref(p), T._ffi.fptr(buf), T._ffi.fptr(hist), None)
    assert rc == 0
    assert_bits_equal(buf, ref_out, "out aliasing xyzw, host")
    assert_bits_equal(hist, ref_hist, "out aliasing xyzw, host, out_history")
    for b in (d_in, d_pl, d_hs, d_ids, d_tb, d_mt, d_out, d_oh, d_none):
        b.free()


def test_refusals(T, ctx):
    B, P, Hs, M, ids, table, bodies = synthetic(37, 29)
    h, w = B.shape[:2]
    L, t = T.lib(), accumulator(T, 1.0, 3, 2.0)
    p = t._clip_motion_params_for(M, table.size, len(bodies))
    out, hist = np.zeros_like(B), np.zeros_like(P)
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    fp = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731

    def call(xyzw=B, planes=P, history=Hs, idp=ids, tb=table, mt=bodies, w=w, h=h, prm=p, o=out, oh=hist, handle=ctx._h):
        return L.trhip_temporal_clip_motion(handle, fp(xyzw), fp(planes), fp(history), vp(idp), T._ffi.u32ptr(tb) if tb is not None else None, fp(mt), w, h,
                                            C.byref(prm) if prm is not None else None, fp(o), fp(oh), None)
    assert call() == 0
    for kw in (dict(prm=None), dict(xyzw=None), dict(planes=None), dict(o=None), dict(oh=None), dict(w=0), dict(h=0), dict(handle=None)):
        assert call(**kw) == -1, kw
        assert L.trhip_last_error(None if "handle" in kw else ctx._h).decode(), kw
    # ids may be NULL only with n_prims = 0
    assert call(idp=None) == -1 and "ids" in L.trhip_last_error(ctx._h).decode()
    none = t._clip_motion_params_for(M, 0, 0)
    assert call(idp=None, tb=None, mt=None, prm=none) == 0 and call(idp=None, prm=none) == 0 and call(prm=none) == 0, "with n_prims = n_bodies = 0 the three pointers are not looked at"
    only_bodies = t._clip_motion_params_for(M, 0, len(bodies))
    assert call(idp=None, tb=None, prm=only_bodies) == 0, "n_prims = 0: every pixel is static, the matrices are not read"
    # a table or matrices announced and not given
    assert call(tb=None) == -1 and "body_of_prim" in L.trhip_last_error(ctx._h).decode()
    assert call(mt=None) == -1 and "bodies" in L.trhip_last_error(ctx._h).decode()
    # out_history may overlap nothing that is read or written beside it, in whole or in part; out_xyzw none of the three arrays
    in_hist = lambda a: hist.reshape(-1).view(np.uint8)[16:16 + a.nbytes].view(a.dtype).reshape(a.shape)  # noqa: E731
    for kw in (dict(oh=Hs), dict(oh=P), dict(history=hist), dict(planes=hist), dict(idp=in_hist(ids)), dict(tb=in_hist(table)), dict(mt=in_hist(bodies))):
        assert call(**kw) == -1, list(kw)
        assert "overlap" in L.trhip_last_error(ctx._h).decode()
    big = np.zeros(P.size + B.size, F)
    tail = big[B.size // 2:B.size // 2 + P.size].reshape(P.shape)
    assert call(o=big[:B.size].reshape(B.shape), oh=tail) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    assert call(xyzw=big[:B.size].reshape(B.shape), oh=tail) == -1
    in_out = out.reshape(-1).view(np.uint8)[:ids.nbytes].view(ids.dtype).reshape(ids.shape)
    assert call(idp=in_out) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    for field, value in (("clip_max_history", -1.0), ("clip_gamma", float("nan")), ("clip_radius", 0), ("reserved2", 1)):
        bad = T._ffi.TemporalClipMotionParams.from_buffer_copy(p)
        setattr(bad, field, value)
        assert call(prm=bad) == -1 and field in L.trhip_last_error(ctx._h).decode()
    bad = T._ffi.TemporalClipMotionParams.from_buffer_copy(p)
    bad.base.max_history = 0.0
    assert call(prm=bad) == -1 and "max_history" in L.trhip_last_error(ctx._h).decode()
    out[:], hist[:] = 0, 0
    assert call() == 0, "a refused call leaves the context usable"
    ref = cmm.accumulate(B, P, Hs, M, ids, table, bodies, cmm.params(1.0, 3, 2.0))
    assert_bits_equal(out, ref[0], "after the refusals, out_xyzw")
    assert_bits_equal(hist, ref[1], "after the refusals, out_history")


# ---- a real sequence -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def motion_sequence(T, ctx):
    """[(scene, motion, camera, xyzw, planes, ids)] of motion_scenes.scene_sequence's three frames at 48 x 48: the bodies move, the camera turns."""
    s, out = SEQUENCE, []
    for k, ((scene, motion), deg) in enumerate(zip(ms.scene_sequence(T, 3), s["degrees"])):
        cam = ms.camera(T, s["resolution"], deg)
        xyzw, planes = frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"])
        ids = T.AOVIntegrator(cam, T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])).ids(scene)
        out.append((scene, motion, cam, xyzw, planes, ids))
    return out


@pytest.mark.parametrize("cell", [(1.0, 1, 0.0), (2.0, 2, 2.0), (4.0, 3, INF)], ids=["g1-R1-cmh0", "g2-R2-cmh2", "g4-R3-cmhInf"])
def test_moving_sequence_equals_the_model(T, ctx, motion_sequence, cell):
    gamma, radius, cmh = cell
    t = T.TemporalAccumulator(clip_gamma=gamma, clip_radius=radius, carry_bodies=True, clip_max_history=cmh)
    prm = cmm.Params(t.params.max_history, t.params.sigma_normal, t.params.sigma_plane, t.params.min_coverage, gamma, radius, cmh)
    hist, prev, tally = None, None, {}
    for k, (scene, motion, cam, xyzw, planes, ids) in enumerate(motion_sequence):
        table, mats = body_inputs(T, scene, motion)
        M = prev.world_to_pixel() if prev is not None else None
        ref_out, ref_hist = cmm.accumulate(xyzw, planes, hist, M, ids, table, mats, prm, tally)
        out, new_hist = t.accumulate_motion(xyzw, planes, hist, ids, table, mats, prev, ctx)
        assert_bits_equal(out, ref_out, f"frame {k}, out_xyzw")
        assert_bits_equal(new_hist, ref_hist, f"frame {k}, out_history")
        hist, prev = new_hist, cam
    print(f"moving sequence tally {cell}: {tally}")
    assert tally["moving"] > 300 and tally["blended"] > 2000 and (gamma > 2 or tally["pixels_clipped"] > 20), tally
    assert hist[..., 0, 3].max() == 3.0 and (cmh > 1 or tally["history_cut"] > 20), tally


# ---- PreviewSession ------------------------------------------------------------------------------------------------------------------------------------------
def test_preview_session_with_motion_equals_the_calls_by_hand(T, ctx):
    s = SEQUENCE
    frames = ms.scene_sequence(T, 3)
    make = lambda: T.TemporalAccumulator(clip_gamma=1.0, clip_radius=2, carry_bodies=True, clip_max_history=1.0)  # noqa: E731
    session = T.PreviewSession(frames[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], temporal=make())
    t, d = make(), T.Denoiser()
    hist, prev = None, None
    for k, ((scene, motion), deg) in enumerate(zip(frames, s["degrees"])):
        cam = ms.camera(T, s["resolution"], deg)
        session.scene = scene
        got = session.render(cam, ctx, motion=motion)
        xyzw, planes = frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"])
        ids = T.AOVIntegrator(cam, T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])).ids(scene, ctx)
        table, mats = body_inputs(T, scene, motion)
        acc, hist = t.accumulate_motion(xyzw, planes, hist, ids, table, mats, prev, ctx)
        want = d.denoise(acc if k else xyzw, planes, ctx)
        assert_bits_equal(got, want, f"frame {k}: path + planes and ids + temporal_clip_motion + denoise by hand")
        assert len(session.render_stats) == 4 and session.render_stats[2].launches_film == 1
        assert session._motion_buffers is not None, "planes and id plane in one call"
        prev = cam
    assert session.frame == 3
    session.close()
    shown = T.PreviewSession(frames[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], temporal=make(), display=T.Display())
    rgba = shown.render_display(ms.camera(T, s["resolution"], 0.0), ctx, motion={})
    assert rgba.shape == (s["resolution"], s["resolution"], 4) and rgba.dtype == np.uint8 and len(shown.render_stats) == 5
    shown.close()


def test_preview_session_without_motion_on_a_static_scene_is_the_clipping_session(T, ctx):
    """motion=None, clip_max_history = +Inf, a static scene on a three-frame arc: the session with the carry_bodies accumulator (trhip_temporal_clip_motion, ids NULL) equals
    the session with the same accumulator without carry_bodies (trhip_temporal_clip) bit for bit, and draws no id plane."""
    s = SEQUENCE
    scene = ms.moving_scene(T)
    sessions = [T.PreviewSession(scene, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], temporal=T.TemporalAccumulator(clip_gamma=1.0, clip_radius=2, **kw))
                for kw in (dict(carry_bodies=True, clip_max_history=INF), {})]
    cut = T.PreviewSession(scene, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], temporal=T.TemporalAccumulator(clip_gamma=1.0, clip_radius=2, carry_bodies=True, clip_max_history=0.0))
    for k, deg in enumerate(s["degrees"]):
        cam = ms.camera(T, s["resolution"], deg)
        got, want, other = sessions[0].render(cam, ctx), sessions[1].render(cam, ctx), cut.render(cam, ctx)
        assert_bits_equal(got, want, f"frame {k}: against the clipping session")
        assert sessions[0]._motion_buffers is None, "no id plane"
        assert k == 0 or not np.array_equal(bits(other), bits(got)), "clip_max_history = 0 is another session"
    for session in sessions + [cut]:
        session.close()


# ---- quality ---------------------------------------------------------------------------------------------------------------------------------------------------
QUALITY = dict(resolution=64, spp=2, depth=5, seed=0xBEEF, frames=8, max_history=8.0)
QUALITY_CAMERAS = {"still": tuple(0.0 for _ in range(8)), "arc": tuple(0.75 * k for k in range(8))}
MASKS = ("bodies", "static", "frame", "swept")
DEFAULT_CELL = (4.0, 3, INF)  # trhip_temporal_clip_motion_default_params' gamma, R, clip_max_history
# mse(new session) / mse(baseline) at the eighth frame over (bodies, static surface pixels, whole frame, swept pixels), for the default cell; baseline (i) is motion={...} with
# the plain accumulator, (ii) motion=None with the clipping accumulator of the same gamma and R.  Filled from profiles/r18/clip_motion.txt
QUALITY_MEASURED = {
    "still": {("i", "bodies"): 1.1489, ("i", "static"): 1.0019, ("i", "frame"): 1.0107, ("i", "swept"): 1.0024,
              ("ii", "bodies"): 1.0645, ("ii", "static"): 0.9758, ("ii", "frame"): 0.9816, ("ii", "swept"): 0.9571},
    "arc": {("i", "bodies"): 1.0173, ("i", "static"): 1.0174, ("i", "frame"): 1.0174, ("i", "swept"): 1.0113,
            ("ii", "bodies"): 0.2335, ("ii", "static"): 1.0545, ("ii", "frame"): 0.5751, ("ii", "swept"): 1.1332}}


class QualityCase:
    """The sequence of clip_motion_scenes, its cameras, the 1024 spp frame of the last pose, and the four masks (definitions, not measurements): the bodies — id -> a body —,
    the static surface pixels, the whole frame, and the swept pixels — static surface pixels whose 1024 spp luminance differs between the first and the last pose, both through
    the last camera, by more than 10 % of the larger."""

    def __init__(self, T, ctx, which):
        q = QUALITY
        self.T, self.ctx = T, ctx
        self.frames = cs.scene_sequence(T, q["frames"])
        self.cams = [ms.camera(T, q["resolution"], deg) for deg in QUALITY_CAMERAS[which]]
        scene, last, offset = self.frames[-1][0], self.cams[-1], (q["frames"] - 1) * q["spp"]
        noisy, planes = frame(T, scene, last, q["spp"], q["depth"], q["seed"], offset)
        ids = T.AOVIntegrator(last, T.SeededSampler(q["spp"], seed=q["seed"], sample_offset=offset)).ids(scene, ctx)
        target = lambda sc: T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), q["depth"]).render(sc)  # noqa: E731
        self.target, first = target(scene), target(self.frames[0][0])
        surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))
        entry = slot_to_entry(T, scene)[np.where(ids["prim"] >= 0, ids["prim"], 0)]
        bodies = surface & (ids["prim"] >= 0) & ((entry == ms.SPHERE_INDEX) | (entry == ms.CUBE_INDEX))
        static = surface & ~bodies
        self.masks = {"bodies": bodies, "static": static, "frame": (self.target[..., 3] > 0) & (noisy[..., 3] > 0), "swept": cs.swept_mask(static, first, self.target)}

    def last_frame(self, temporal, with_motion):
        q = QUALITY
        session = self.T.PreviewSession(self.frames[0][0], self.T.SeededSampler(q["spp"], seed=q["seed"]), q["depth"], temporal=temporal)
        for (scene, motion), cam in zip(self.frames, self.cams):
            session.scene = scene
            out = session.render(cam, self.ctx, motion=motion if with_motion else None)
        session.close()
        return out

    def mse(self, a):
        """{mask: MSE of xyz / w against the 1024 spp frame}"""
        out = {}
        for name, mask in self.masks.items():
            with np.errstate(all="ignore"):
                diff = a[mask][:, :3].astype(np.float64) / a[mask][:, 3:4] - self.target[mask][:, :3].astype(np.float64) / self.target[mask][:, 3:4]
            out[name] = float(np.mean(diff * diff))
        return out

    def cell(self, gamma, radius, cmh):
        T = self.T
        return self.mse(self.last_frame(T.TemporalAccumulator(max_history=QUALITY["max_history"], clip_gamma=gamma, clip_radius=radius, carry_bodies=True, clip_max_history=cmh), True))

    def baselines(self, gamma, radius):
        """(i) motion={...} with the plain accumulator, (ii) motion=None with the clipping accumulator, (iii) motion=None with the plain accumulator: the parent's behaviour."""
        T, cap = self.T, QUALITY["max_history"]
        return {"i": self.mse(self.last_frame(T.TemporalAccumulator(max_history=cap), True)),
                "ii": self.mse(self.last_frame(T.TemporalAccumulator(max_history=cap, clip_gamma=gamma, clip_radius=radius), False)),
                "iii": self.mse(self.last_frame(T.TemporalAccumulator(max_history=cap), False))}


@pytest.mark.parametrize("which", sorted(QUALITY_CAMERAS))
def test_quality_against_the_three_baselines(T, ctx, which):
    """Eight frames at 2 spp, the sphere sliding sideways so that its shadow sweeps floor and back wall, the cube turning; the last frame of the session with the default cell
    against baselines (i) and (ii), both measured against the 1024 spp frame of the last pose, over the four masks.  The frames are bit-reproducible, so each ratio is a
    number; each is asserted within 10 % of its measured value (QUALITY_MEASURED; docs/design/21-clip-motion.md has the whole sweep).  Measured on an MI355X: still camera, 573
    pixels on the bodies, 3213 static surface pixels, 984 of them swept; arc 546, 3324, 1019.  Against (i): still 1.149 on the bodies, 1.002 static, 1.011 frame, 1.002 swept;
    arc 1.017, 1.017, 1.017, 1.011.  Against (ii): still 1.065, 0.976, 0.982, 0.957; arc 0.234, 1.055, 0.575, 1.133.  THE EXPECTATION "WELL BELOW 1 ON THE SWEPT MASK AGAINST
    (i)" DOES NOT HOLD: at 2 spp no cell of the sweep that clips beats not clipping there (best 0.996, gamma 4, R 3, clip_max_history 1, still camera).  What holds: on the
    arc the bodies' error is 0.23 of the motion-blind clipping session's.  With a still camera the bodies are 6 % WORSE than (ii)."""
    case = QualityCase(T, ctx, which)
    counts = {name: int(mask.sum()) for name, mask in case.masks.items()}
    new, base = case.cell(*DEFAULT_CELL), case.baselines(*DEFAULT_CELL[:2])
    ratios = {(b, m): new[m] / base[b][m] for b in ("i", "ii") for m in MASKS}
    print(f"clip-motion quality {which}: pixels {counts}; new {new}; baselines {base}; ratios {ratios}")
    assert counts["bodies"] >= 100 and counts["swept"] >= 0.02 * counts["static"], counts
    inf_cell = case.cell(INF, DEFAULT_CELL[1], 0.0)
    assert inf_cell == base["i"], "clip_gamma = +Inf repeats baseline (i) digit for digit"
    for key, want in QUALITY_MEASURED[which].items():
        assert abs(ratios[key] / want - 1.0) <= 0.10, (key, ratios[key], want)
    assert set(QUALITY_MEASURED[which]) == set(ratios)
