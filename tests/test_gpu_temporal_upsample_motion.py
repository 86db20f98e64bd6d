"""trhip_temporal_upsample_motion on the GPU (docs/design/22-upsample-motion.md): the kernel against the numpy model of tests/temporal_upsample_motion_model.py, bit for
bit in every value of the film, of the history and every mask byte, at the sizes where the tiling, the border and the footprint change, R = 1 and 2, with and without
history, on frames whose id plane and body table hold garbage; identity (a) against trhip_temporal_upsample_device and (b) against trhip_upscale_device on the device; host
== device; run-to-run identity; the refusals that need a context; PreviewSession(temporal_upsample=TemporalUpsampler(carry_bodies=True)) with `motion` against the calls by
hand and without it against the calls it always made; the history kept on the device's own frames; and the quality figures.

Measured on an MI355X (profiles/r19/upsample_motion.txt, docs/design/22-upsample-motion.md).  History found at frame 3 of the 48^2 <- 24^2 sequence at 2 spp (mask bit 4):
205 of the sphere's 209 full-size surface pixels (153 motion-blind), 196 of the cube's 206 (190).  Quality (eight frames at 64^2 <- 32^2, 4 spp, depth 5, max_history 8; MSE
of xyz / w at the last frame against the 1024 spp full-size frame of that frame's pose; the session with motion={...} over the same session with the moved scene and
motion=None, which is what the library did before; QUALITY_MEASURED below): still camera 0.5280 over the moving bodies' 646 pixels and 0.7550 over the whole frame; ON THE
0.75-DEGREE ARC 1.4867 OVER THE BODIES' 643 PIXELS AND 1.1826 OVER THE WHOLE FRAME — THERE THE MOTION-AWARE SESSION IS WORSE THAN THE MOTION-BLIND ONE, not "not above 1" as
expected.  Beside them, the ratio to the native motion={...} session at the same spp: still 1.114 and 1.561, arc 0.994 and 1.061."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import motion_model as mm
import motion_scenes as ms
import temporal_upsample_motion_model as tumm

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1

# (full-size h, w) <- (low h, w): a single lane; smaller than a footprint; non-integer ratio with partial tiles; the 2 x case; the ratio limit; ratio 1, the largest footprint
SIZES = {"1x1<-1x1": ((1, 1), (1, 1)), "5x3<-3x2": ((3, 5), (2, 3)), "37x29<-19x15": ((29, 37), (15, 19)), "64x64<-32x32": ((64, 64), (32, 32)),
         "48x32<-12x8": ((32, 48), (8, 12)), "33x17<-33x17": ((17, 33), (17, 33))}
FRAMES = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def frame(name):
    """(lo_xyzw, lo_planes, hi_planes, lo_from_hi, history, M, ids, body_of_prim, bodies): computed once per size and left unchanged."""
    if name not in FRAMES:
        (hh, hw), (lh, lw) = SIZES[name]
        FRAMES[name] = tumm.synthetic(hh, hw, lh, lw, 4000 + hw)
    return tuple(a.copy() if isinstance(a, np.ndarray) else a for a in FRAMES[name])


def model_params(tu, m):
    p = tu.params
    return tumm.Params(m, radius=p.radius, max_history=p.max_history, sigma_normal=p.sigma_normal, sigma_plane=p.sigma_plane, min_coverage=p.min_coverage,
                       guide_sigma_normal=p.guide_sigma_normal, guide_sigma_plane=p.guide_sigma_plane, confidence_floor=p.confidence_floor,
                       confidence_sharpness=p.confidence_sharpness)


def device(T, *arrays):
    return [T._ffi.DeviceBuffer(a.nbytes).from_host(a) if a is not None else None for a in arrays]


def ptr(b):
    return b.ptr if b is not None else None


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_synthetic_frames_equal_the_model(T, ctx, size, radius):
    lo, lp, hp, m, Hs, M, ids, table, bodies = frame(size)
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    tu = T.TemporalUpsampler(radius=radius, confidence_floor=0.25, max_history=8.0, carry_bodies=True)
    for history in (Hs, None):
        what = f"{size} R={radius} {'with' if history is not None else 'without'} history"
        ref, ref_hist, ref_mask = tumm.accumulate(lo, lp, hp, history, M, ids, table, bodies, model_params(tu, m))
        out, hist, mask = tu.accumulate_motion(lo, lp, hp, history, ids, table, bodies, m, M, ctx)
        assert_bits_equal(out, ref, "out_xyzw, " + what)
        assert_bits_equal(hist, ref_hist, "out_history, " + what)
        assert_bits_equal(mask, ref_mask, "out_mask, " + what)
        assert tu.stats.launches_film == 1
        assert_bits_equal(out[..., 3], hp[..., 0, 3], "the .w lane is plane 0's weight")
        assert np.isfinite(out[..., :3]).all() and np.isfinite(hist).all(), "every output is finite whatever the inputs hold"
        # (c): words 1 and 2 of the history never depend on the bodies
        plain = T.TemporalUpsampler(radius=radius, confidence_floor=0.25, max_history=8.0).accumulate(lo, lp, hp, history, m, M, ctx)
        assert_bits_equal(hist[..., 1:, :], plain[1][..., 1:, :], "out_history holds the CURRENT n and p, " + what)
        if history is None:
            assert_bits_equal(out, plain[0], "without history the bodies decide nothing, " + what)
            assert_bits_equal(mask, plain[2], "without history the bodies decide nothing: mask, " + what)
        elif h * w > 100:
            assert not np.array_equal(bits(out), bits(plain[0])), "the bodies change something"


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("size", ["37x29<-19x15", "64x64<-32x32"])
def test_identities_a_and_b_on_the_device(T, ctx, size, radius):
    """(a) every pixel static — ids NULL, no table, no matrices, every table word >= n_bodies —: film, history and mask are trhip_temporal_upsample_device's bit for bit.
    (b) history NULL: film and mask are trhip_upscale_device's bit for bit, with the bodies in place."""
    lo, lp, hp, m, Hs, M, ids, table, bodies = frame(size)
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    tu, plain = T.TemporalUpsampler(radius=radius, carry_bodies=True), T.TemporalUpsampler(radius=radius)
    words = np.where(np.arange(table.size) % 2 == 0, np.uint32(mm.STATIC), np.uint32(len(bodies)) + np.arange(table.size, dtype=np.uint32)).astype(np.uint32)
    d_lo, d_lp, d_hp, d_hs, d_ids, d_tb, d_mt, d_words = device(T, lo, lp, hp, Hs, ids, table, bodies, words)
    outs = [T._ffi.DeviceBuffer(n) for n in (h * w * 16, h * w * 48, h * w)]

    def fetch():
        got = outs[0].to_host(F, (h, w, 4)), outs[1].to_host(F, (h, w, 3, 4)), outs[2].to_host(np.uint8, (h, w))
        for b in outs:
            b.zero()
        return got
    plain.accumulate_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, d_hs.ptr, w, h, m, M, outs[0].ptr, outs[1].ptr, outs[2].ptr, ctx)
    want = fetch()
    n_prims, n_bodies = table.size, len(bodies)
    variants = {"ids NULL": (None, None, 0, None, 0), "ids NULL, tables given": (None, d_tb, n_prims, d_mt, n_bodies), "no table": (d_ids, None, 0, d_mt, n_bodies),
                "no matrices": (d_ids, d_tb, n_prims, None, 0), "no table, no matrices": (d_ids, None, 0, None, 0), "every table word >= n_bodies": (d_ids, d_words, n_prims, d_mt, n_bodies)}
    for what, (i, t, np_, b, nb) in variants.items():
        tu.accumulate_motion_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, d_hs.ptr, ptr(i), ptr(t), np_, ptr(b), nb, w, h, m, M, outs[0].ptr, outs[1].ptr, outs[2].ptr, ctx)
        for g, r, name in zip(fetch(), want, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"(a) {what}: {name} against trhip_temporal_upsample_device")
    tu.accumulate_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, d_hs.ptr, w, h, m, M, outs[0].ptr, outs[1].ptr, outs[2].ptr, ctx)
    for g, r, name in zip(fetch(), want, ("out_xyzw", "out_history", "out_mask")):
        assert_bits_equal(g, r, f"(a) accumulate_device of a carry_bodies upsampler: {name}")
    # (b)
    u = T.Upscaler(radius=radius, demodulate=False, coverage=False, sigma_normal=tu.params.guide_sigma_normal, sigma_plane=tu.params.guide_sigma_plane,
                   min_coverage=tu.params.min_coverage)
    u.upscale_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, w, h, m, outs[0].ptr, outs[2].ptr, ctx)
    up_film, _, up_mask = fetch()
    tu.accumulate_motion_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, None, d_ids.ptr, d_tb.ptr, n_prims, d_mt.ptr, n_bodies, w, h, m, M, outs[0].ptr, outs[1].ptr, outs[2].ptr, ctx)
    film, _, mask = fetch()
    assert_bits_equal(film, up_film, "(b) out_xyzw against trhip_upscale_device")
    assert_bits_equal(mask, up_mask, "(b) out_mask against trhip_upscale_device")
    for b in [d_lo, d_lp, d_hp, d_hs, d_ids, d_tb, d_mt, d_words] + outs:
        b.free()


def test_host_and_device_agree_and_two_runs_give_the_same_bits(T, ctx):
    lo, lp, hp, m, Hs, M, ids, table, bodies = frame("64x64<-32x32")
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    tu = T.TemporalUpsampler(carry_bodies=True)
    first = tu.accumulate_motion(lo, lp, hp, Hs, ids, table, bodies, m, M, ctx)
    second = tu.accumulate_motion(lo, lp, hp, Hs, ids, table, bodies, m, M, ctx)
    for a, b, what in zip(first, second, ("out_xyzw", "out_history", "out_mask")):
        assert_bits_equal(a, b, "run to run: " + what)
    inputs = (lo, lp, hp, Hs, ids, table, bodies)
    bufs = device(T, *inputs)
    d_lo, d_lp, d_hp, d_hs, d_ids, d_tb, d_mt = bufs
    outs = [T._ffi.DeviceBuffer(n).zero() for n in (h * w * 16, h * w * 48, h * w)]
    for with_mask in (True, False):
        tu.accumulate_motion_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, d_hs.ptr, d_ids.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, m, M, outs[0].ptr, outs[1].ptr,
                                    outs[2].ptr if with_mask else None, ctx)
        assert tu.stats.launches_film == 1
        assert_bits_equal(outs[0].to_host(F, (h, w, 4)), first[0], f"device variant, out_xyzw (mask {with_mask})")
        assert_bits_equal(outs[1].to_host(F, (h, w, 3, 4)), first[1], f"device variant, out_history (mask {with_mask})")
        assert_bits_equal(outs[2].to_host(np.uint8, (h, w)), first[2], "device variant, out_mask")  # the second call leaves it alone
        outs[0].zero(), outs[1].zero()
    for buf, a, what in zip(bufs, inputs, ("lo_xyzw", "lo_planes", "hi_planes", "history", "ids", "body_of_prim", "bodies")):
        assert buf.to_host(a.dtype, a.shape).tobytes() == a.tobytes(), f"the input {what} is left alone"
    # the host entry point without a mask and without stats
    p = tu._motion_params_for(m, M, table.size, len(bodies))
    out2, hist2 = np.full_like(first[0], 7.0), np.full_like(first[1], 7.0)
    fp = T._ffi.fptr
    ctx.check(T.lib().trhip_temporal_upsample_motion(ctx._h, fp(lo), fp(lp), lw, lh, fp(hp), fp(Hs), ids.ctypes.data_as(C.c_void_p), T._ffi.u32ptr(table), fp(bodies), w, h, C.byref(p),
                                                     fp(out2), fp(hist2), None, None))
    assert_bits_equal(out2, first[0], "out_mask NULL, out_xyzw")
    assert_bits_equal(hist2, first[1], "out_mask NULL, out_history")
    for b in bufs + outs:
        b.free()


def test_overlaps_and_device_side_refusals(T, ctx):
    lo, lp, hp, m, Hs, M, ids, table, bodies = frame("37x29<-19x15")
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    tu, L = T.TemporalUpsampler(carry_bodies=True), T.lib()
    p = tu._motion_params_for(m, M, table.size, len(bodies))
    none = tu._motion_params_for(m, M, 0, 0)
    out, hist, mask = np.zeros((h, w, 4), F), np.zeros((h, w, 3, 4), F), np.zeros((h, w), np.uint8)
    fp = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    bp = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None  # noqa: E731

    def call(lo_=lo, lp_=lp, hp_=hp, hs_=Hs, idp=ids, tb=table, mt=bodies, out_=out, hist_=hist, mask_=mask, w_=w, h_=h, lw_=lw, lh_=lh, prm=p, handle=ctx._h):
        return L.trhip_temporal_upsample_motion(handle, fp(lo_), fp(lp_), lw_, lh_, fp(hp_), fp(hs_), vp(idp), T._ffi.u32ptr(tb) if tb is not None else None, fp(mt), w_, h_,
                                                C.byref(prm) if prm is not None else None, fp(out_), fp(hist_), bp(mask_), None)
    err = lambda: L.trhip_last_error(ctx._h)  # noqa: E731
    assert call() == 0 and call(hs_=None) == 0 and call(mask_=None) == 0
    for kw in (dict(lo_=None), dict(lp_=None), dict(hp_=None), dict(out_=None), dict(hist_=None)):
        assert call(**kw) == INVALID and b"null argument" in err(), kw
    for kw in (dict(w_=0), dict(h_=0), dict(lw_=0), dict(lh_=0)):
        assert call(**kw) == INVALID and b"empty" in err(), kw
    assert call(prm=None) == INVALID and call(handle=None) == INVALID
    # a table, an id plane or matrices announced and not given
    assert call(tb=None) == INVALID and b"body_of_prim" in err()
    assert call(idp=None) == INVALID and b"ids may be null only" in err()
    assert call(mt=None) == INVALID and b"bodies is null" in err()
    assert call(idp=None, tb=None, mt=None, prm=none) == 0 and call(prm=none) == 0, "with n_prims = n_bodies = 0 the three pointers are not looked at"
    # every output over each input, ids, body_of_prim and bodies counted among them; the outputs over each other
    inside = lambda host, a, at=16: host.reshape(-1).view(np.uint8)[at:at + a.nbytes].view(a.dtype).reshape(a.shape)  # noqa: E731
    for kw in (dict(hist_=lo), dict(hist_=lp), dict(hist_=hp), dict(hist_=Hs), dict(idp=inside(hist, ids)), dict(tb=inside(hist, table)), dict(mt=inside(hist, bodies))):
        assert call(**kw) == INVALID and b"out_history overlaps an input" in err(), list(kw)
    for kw in (dict(out_=hp), dict(out_=Hs), dict(idp=inside(out, ids, 0)), dict(tb=inside(out, table)), dict(mt=inside(out, bodies))):
        assert call(**kw) == INVALID and b"out_xyzw overlaps an input" in err(), list(kw)
    big_mask = np.zeros(max(mask.size, table.nbytes + 16, bodies.nbytes + 16), np.uint8)
    for kw in (dict(tb=inside(big_mask, table)), dict(mt=inside(big_mask, bodies)), dict(hs_=Hs, mask_=Hs), dict(idp=ids, mask_=ids.view(np.uint8))):
        kw.setdefault("mask_", big_mask)
        assert call(**kw) == INVALID and b"out_mask overlaps an input" in err(), list(kw)
    assert call(out_=hist) == INVALID and b"out_xyzw overlaps out_history" in err()
    assert call(mask_=hist) == INVALID and b"out_mask overlaps out_history" in err()
    assert call(mask_=out) == INVALID and b"out_mask overlaps out_xyzw" in err()
    # an overlap is reported before a missing table
    assert call(hist_=Hs, tb=None) == INVALID and b"overlaps" in err()
    # with n_prims = 0 the caller's table pointer is not an input: it may lie anywhere
    assert call(tb=inside(hist, table), mt=inside(hist, bodies), prm=none) == 0
    # the block comes first, and a refused call leaves the context usable
    bad = T._ffi.TemporalUpsampleMotionParams.from_buffer_copy(p)
    bad.motion_flags = 2
    assert call(prm=bad, lo_=None) == INVALID and b"motion_flags" in err()
    ref = tumm.accumulate(lo, lp, hp, Hs, M, ids, table, bodies, model_params(tu, m))
    out[...], hist[...], mask[...] = 0, 0, 0
    assert call() == 0, "a refused call leaves the context usable"
    for g, r, what in zip((out, hist, mask), ref, ("out_xyzw", "out_history", "out_mask")):
        assert_bits_equal(g, r, "after the refusals: " + what)


# ---- a real sequence ---------------------------------------------------------------------------------------------------------------------------------------------
SEQUENCE = dict(resolution=48, spp=2, depth=3, seed=0x7E3A, degrees=(0.0, 3.0, 6.0))


def body_inputs(T, scene, motion):
    """(body_of_prim, bodies) of a frame: the motion's keys in order are the bodies."""
    keys = sorted(motion)
    if not keys:
        return None, None
    of_entry = [None] * len(T.top_level_counts(scene))
    for i, k in enumerate(keys):
        of_entry[k] = i
    return scene.flatten().body_table(of_entry), np.stack([T.TemporalAccumulator.prev_from_cur(motion[k]) for k in keys])


def slot_to_entry(T, scene):
    counts = T.top_level_counts(scene)
    return np.repeat(np.arange(len(counts)), counts)[scene.flatten().bvh()[3]]


def frames_by_hand(T, ctx, tu, k, scene, cam, s, guide_spp=None):
    """(lo_xyzw, lo_planes, hi_planes, ids, lo_from_hi) of frame k as the session draws them: the path frame and its planes through the jittered low camera, the full-size
    planes and id plane with the guide sampler."""
    lo_cam = T.Upscaler.low_camera(cam, 2, jitter=tu.jitter_for(k, 2))
    smp = T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])
    guide = T.SeededSampler(s["spp"] if guide_spp is None else guide_spp, seed=s["seed"], sample_offset=k * s["spp"])
    lo_xyzw = T.PathIntegrator(lo_cam, smp, s["depth"]).render(scene, ctx)
    lo_planes = T.AOVIntegrator(lo_cam, smp).render(scene, ctx).planes
    aov = T.AOVIntegrator(cam, guide)
    return lo_xyzw, lo_planes, aov.render(scene, ctx).planes, aov.ids(scene, ctx), T.Upscaler.pixel_map(cam, lo_cam)


@pytest.fixture(scope="module")
def sequence_by_hand(T, ctx):
    """The three frames of SEQUENCE through trhip_temporal_upsample_motion with the bodies and through trhip_temporal_upsample without: per frame
    (scene, motion, camera, ids, filtered frame with the motion, mask, filtered motion-blind frame, mask, surface mask).  Computed once."""
    s, d = SEQUENCE, T.Denoiser()
    tu, blind = T.TemporalUpsampler(carry_bodies=True), T.TemporalUpsampler()
    out, hist, hist_blind, prev = [], None, None, None
    for k, ((scene, motion), deg) in enumerate(zip(ms.scene_sequence(T, 3), s["degrees"])):
        cam = ms.camera(T, s["resolution"], deg)
        lo_xyzw, lo_planes, hi_planes, ids, m = frames_by_hand(T, ctx, tu, k, scene, cam, s)
        table, mats = body_inputs(T, scene, motion)
        if k == 1:  # on the device's own frames the kernel is the model as well
            ref = tumm.accumulate(lo_xyzw, lo_planes, hi_planes, hist, prev.world_to_pixel(), ids, table, mats, model_params(tu, m))
        acc, hist, mask = tu.accumulate_motion(lo_xyzw, lo_planes, hi_planes, hist, ids, table, mats, m, prev, ctx)
        if k == 1:
            for g, r, what in zip((acc, hist, mask), ref, ("out_xyzw", "out_history", "out_mask")):
                assert_bits_equal(g, r, f"frame 1 against the model: {what}")
        acc_blind, hist_blind, mask_blind = blind.accumulate(lo_xyzw, lo_planes, hi_planes, hist_blind, m, prev, ctx)
        assert_bits_equal(hist[..., 1:, :], hist_blind[..., 1:, :], f"frame {k}: the stored surface never depends on the bodies")
        out.append((scene, motion, cam, ids, d.denoise(acc, hi_planes, ctx), mask, d.denoise(acc_blind, hi_planes, ctx), mask_blind, hist[..., 1, 3] == 1))
        prev = cam
    return out


def test_preview_session_with_motion_equals_the_calls_by_hand(T, ctx, sequence_by_hand):
    """Three frames of the moving scene: path frame and planes through the jittered low camera, full-size planes AND id plane in one call with the guide sampler,
    trhip_temporal_upsample_motion_device, the filter."""
    s = SEQUENCE
    session = T.PreviewSession(sequence_by_hand[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], upscaler=T.Upscaler(), factor=2,
                               temporal_upsample=T.TemporalUpsampler(carry_bodies=True))
    for k, (scene, motion, cam, _, want, _, _, _, _) in enumerate(sequence_by_hand):
        session.scene = scene
        got = session.render(cam, ctx, motion=motion)
        assert got.shape == (s["resolution"], s["resolution"], 4)
        assert_bits_equal(got, want, f"frame {k}: low path + low planes + full-size planes and ids + temporal_upsample_motion + denoise by hand")
        assert len(session.render_stats) == 5 and session.render_stats[3].launches_film == 1
        assert session._motion_buffers[0].nbytes == s["resolution"] ** 2 * 16, "the id plane is the FULL-SIZE frame's"
    assert session.frame == 3
    # a scene of another structure: refused with a sentence that names reset(), and rendered after it
    session.scene = ms.id_scene(T)
    with pytest.raises(T.TraceHipError, match=r"reset\(\)"):
        session.render(cam, ctx, motion={})
    assert session.frame == 3
    session.reset()
    assert session.render(cam, ctx, motion={}).shape == (s["resolution"], s["resolution"], 4)
    with pytest.raises(T.TraceHipError, match="top-level"):
        session.render(cam, ctx, motion={99: T.translate([0.1, 0, 0])})
    session.close()
    # the display path takes the same argument
    shown = T.PreviewSession(sequence_by_hand[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], upscaler=T.Upscaler(), factor=2, display=T.Display(),
                             temporal_upsample=T.TemporalUpsampler(carry_bodies=True))
    rgba = shown.render_display(ms.camera(T, s["resolution"], 0.0), ctx, motion={})
    assert rgba.shape == (s["resolution"], s["resolution"], 4) and rgba.dtype == np.uint8 and len(shown.render_stats) == 6
    shown.close()


@pytest.mark.parametrize("carry_bodies", [False, True])
def test_preview_session_without_motion_makes_the_calls_it_made(T, ctx, sequence_by_hand, carry_bodies):
    """motion=None over the moving scenes: low path, low planes, full-size planes, the temporal-upsampling pass, the filter — bit for bit what the session made before this
    pass existed, and no id plane is drawn.  An upsampler built with carry_bodies=True goes through the new entry point with every pixel static: the same bits."""
    s = SEQUENCE
    session = T.PreviewSession(sequence_by_hand[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], upscaler=T.Upscaler(), factor=2,
                               temporal_upsample=T.TemporalUpsampler(carry_bodies=carry_bodies))
    for k, (scene, _, cam, _, _, _, want, _, _) in enumerate(sequence_by_hand):
        session.scene = scene
        got = session.render(cam, ctx) if k else session.render(cam, ctx, motion=None)
        assert_bits_equal(got, want, f"frame {k}: the motion-blind calls by hand")
        assert session._motion_buffers is None, "no id plane"
        assert len(session.render_stats) == 5
    session.close()


def test_moving_sequence_keeps_the_bodies_history_on_the_device(T, ctx, sequence_by_hand):
    """The device's own frames, 48^2 <- 24^2, 2 spp, three frames.  At frame 3, per body: the full-size surface pixels whose mask has bit 4, through the calls the
    motion={...} session makes and through the calls the motion=None session makes (both sessions are those calls bit for bit: the two tests above).  Strictly more with
    the motion, and more than half.  Measured on an MI355X: sphere 205 of 209 (0.981) against 153 (0.732) motion-blind, cube 196 of 206 (0.951) against 190 (0.922) — the
    figures of the native pass on the same planes (20-motion.md).  On frames from the oracle's geometry every pixel: 195 / 195 and 201 / 201 against 161 and 179
    (tests/test_temporal_upsample_motion_api.py); the 2 spp planes' silhouette pixels mix two surfaces and some find no tap."""
    scene, _, _, ids, _, mask, _, mask_blind, surface = sequence_by_hand[-1]
    entry = slot_to_entry(T, scene)[np.where(ids["prim"] >= 0, ids["prim"], 0)]
    for name, index in (("sphere", ms.SPHERE_INDEX), ("cube", ms.CUBE_INDEX)):
        on_body = surface & (ids["prim"] >= 0) & (entry == index)
        n, kept, kept_blind = int(on_body.sum()), int((mask[on_body] & 4 != 0).sum()), int((mask_blind[on_body] & 4 != 0).sum())
        print(f"moving sequence at 48^2 <- 24^2, {name}: {n} full-size surface pixels, history found at {kept} ({kept / n:.3f}) with the motion, {kept_blind} "
              f"({kept_blind / n:.3f}) motion-blind")
        assert n >= 30 and kept > kept_blind and 2 * kept > n, (name, n, kept, kept_blind)


# ---- quality -------------------------------------------------------------------------------------------------------------------------------------------------------
QUALITY = dict(resolution=64, spp=4, depth=5, seed=0xBEEF, frames=8, max_history=8.0)
QUALITY_CAMERAS = {"still": tuple(0.0 for _ in range(8)), "arc": tuple(0.75 * k for k in range(8))}
# mse(temporal-upsampling session with motion) / mse(the same session with the moved scene and motion=None) at the eighth frame:
# (over the moving bodies' full-size surface pixels, over the whole frame)
QUALITY_MEASURED = {"still": (0.5280, 0.7550), "arc": (1.4867, 1.1826)}


def quality_ratios(T, ctx, which):
    q = QUALITY
    frames = ms.scene_sequence(T, q["frames"])
    cams = [ms.camera(T, q["resolution"], deg) for deg in QUALITY_CAMERAS[which]]
    results = {}
    for mode in ("motion", "blind", "native"):
        kw = dict() if mode == "native" else dict(upscaler=T.Upscaler(), factor=2, temporal_upsample=T.TemporalUpsampler(max_history=q["max_history"], carry_bodies=mode == "motion"))
        session = T.PreviewSession(frames[0][0], T.SeededSampler(q["spp"], seed=q["seed"]), q["depth"], **kw)
        for (scene, motion), cam in zip(frames, cams):
            session.scene = scene
            results[mode] = session.render(cam, ctx, motion=None if mode == "blind" else motion)
        session.close()
    scene, last, offset = frames[-1][0], cams[-1], (q["frames"] - 1) * q["spp"]
    smp = T.SeededSampler(q["spp"], seed=q["seed"], sample_offset=offset)
    noisy, planes = T.PathIntegrator(last, smp, q["depth"]).render(scene, ctx), T.AOVIntegrator(last, smp).render(scene, ctx).planes
    ids = T.AOVIntegrator(last, smp).ids(scene, ctx)
    target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), q["depth"]).render(scene)
    surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))
    entry = slot_to_entry(T, scene)[np.where(ids["prim"] >= 0, ids["prim"], 0)]
    bodies = surface & (ids["prim"] >= 0) & ((entry == ms.SPHERE_INDEX) | (entry == ms.CUBE_INDEX))
    everything = (target[..., 3] > 0) & (noisy[..., 3] > 0)

    def mse(a, mask):
        with np.errstate(all="ignore"):
            diff = a[mask][:, :3].astype(np.float64) / a[mask][:, 3:4] - target[mask][:, :3].astype(np.float64) / target[mask][:, 3:4]
        return float(np.mean(diff * diff))
    figures = {(mode, name): mse(results[mode], mask) for mode in results for name, mask in (("bodies", bodies), ("frame", everything))}
    return figures, int(bodies.sum())


@pytest.mark.parametrize("which", sorted(QUALITY_CAMERAS))
def test_quality_against_the_motion_blind_temporal_upsampling_session(T, ctx, which):
    """Eight frames at 64^2 <- 32^2, 4 spp, depth 5, max_history 8, the sphere rising and the cube turning, once with a still camera and once on the 0.75-degree arc: the last
    frame through PreviewSession(temporal_upsample=TemporalUpsampler(carry_bodies=True)) with motion={...} against the same session with the moved scene and motion=None
    (the library's behaviour before), both against the 1024 spp full-size frame of the last frame's own pose.  The ratio to the native motion={...} session at the same spp
    is printed beside it, for context.  The frames are bit-reproducible, so each ratio is a number; it is asserted within 10 % of its measured value (QUALITY_MEASURED).
    Measured: still camera 0.5280 on the bodies and 0.7550 on the frame (mse 0.05635 against 0.10672; 0.025570 against 0.033869); arc 1.4867 and 1.1826 (0.04989 against
    0.03356; 0.016666 against 0.014092).  The expectation — below 1 on the bodies with the still camera, not above 1 on the whole frame — holds for the still camera and
    does NOT hold on the arc.  What is measured there: this session's error on the bodies is the native motion session's (0.994 of it), while the motion-blind session's own
    error on the bodies is three times lower on the arc (0.0336) than with the still camera (0.1067).  The cause was not isolated (docs/design/22-upsample-motion.md says
    what is supposed).  Nothing was tuned; the defaults are 19's."""
    figures, n_bodies = quality_ratios(T, ctx, which)
    on_bodies, on_frame = figures[("motion", "bodies")] / figures[("blind", "bodies")], figures[("motion", "frame")] / figures[("blind", "frame")]
    to_native = figures[("motion", "bodies")] / figures[("native", "bodies")], figures[("motion", "frame")] / figures[("native", "frame")]
    print(f"upsample motion quality {which}: {n_bodies} pixels on the moving bodies; mse ratio motion / motion-blind on the bodies {on_bodies:.4f}, on the whole frame {on_frame:.4f}; "
          f"to the native motion session {to_native[0]:.4f} and {to_native[1]:.4f}; {figures}")
    assert n_bodies >= 100
    want_bodies, want_frame = QUALITY_MEASURED[which]
    assert abs(on_bodies / want_bodies - 1.0) <= 0.10, (on_bodies, want_bodies)
    assert abs(on_frame / want_frame - 1.0) <= 0.10, (on_frame, want_frame)
