"""trhip_upscale, trhip_temporal_upsample and trhip_temporal_upsample_motion over the pixel-map table of tests/upsample_maps.py (docs/design/17-upscale.md, "The
pixel-map space"): every map at R = 1 and 2, bit for bit in every value of the film, the history and the mask against the numpy models, through the host and the device
entry points; the three large maps (the spare staged column, 65 535 blocks on either axis) through the host entry point, one call per kernel; and the maps the product
itself makes — PreviewSession at factors 3, 2.6 on a cropped film, 1 and 4, with the temporal-upsampling mode, with the upscaler alone and with moving bodies — each frame
against the calls by hand and each upsampling call by hand against its model.  tests/test_upsample_maps.py shows on the CPU that the models reach, on these inputs, what each
map is named for."""
import numpy as np
import pytest

import motion_scenes as ms
import temporal_upsample_model as tum
import temporal_upsample_motion_model as tumm
import upsample_maps as maps
import upscale_model as um

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = [(n, R) for n in maps.SMALL for R in maps.CASES[n].radii]
SMALL_IDS = [f"{n}-R{R}" for n, R in SMALL]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def upscale_model_params(u, m):
    p = u.params
    return um.Params(m, radius=p.radius, demodulate=bool(p.flags & 1), coverage=bool(p.flags & 2), sigma_normal=p.sigma_normal, sigma_plane=p.sigma_plane,
                     albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)


def temporal_model_params(tu, m):
    p = tu.params
    return tum.Params(m, radius=p.radius, max_history=p.max_history, sigma_normal=p.sigma_normal, sigma_plane=p.sigma_plane, min_coverage=p.min_coverage,
                      guide_sigma_normal=p.guide_sigma_normal, guide_sigma_plane=p.guide_sigma_plane, confidence_floor=p.confidence_floor,
                      confidence_sharpness=p.confidence_sharpness)


def guide_upscaler(T, tu):
    """The Upscaler whose film and mask the temporal passes reproduce without history: their part U."""
    p = tu.params
    return T.Upscaler(radius=p.radius, demodulate=False, coverage=False, sigma_normal=p.guide_sigma_normal, sigma_plane=p.guide_sigma_plane, min_coverage=p.min_coverage)


def device(T, *arrays):
    return [T._ffi.DeviceBuffer(a.nbytes).from_host(a) if a is not None else None for a in arrays]


def ptr(b):
    return b.ptr if b is not None else None


def free(*buffers):
    for b in buffers:
        if b is not None:
            b.free()


def check_far(name, out, mask, hist=None):
    """`far`: everything lies off the low image — the film is (0, 0, 0, A), the mask 0 (the history bit apart), the history finite."""
    if name == "far":
        assert not out[..., :3].any() and not (mask & 3).any()
        assert hist is None or np.isfinite(hist).all()


# ---- the table, small maps -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,radius", SMALL, ids=SMALL_IDS)
def test_upscale_equals_the_model_on_every_map(T, ctx, name, radius):
    lo, lp, hp, m = maps.upscale_frames(name)
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    d_lo, d_lp, d_hp = device(T, lo, lp, hp)
    d_out, d_mask = T._ffi.DeviceBuffer(h * w * 16), T._ffi.DeviceBuffer(h * w)
    for flags in (False, True):
        u = T.Upscaler(radius=radius, demodulate=flags, coverage=flags)
        what = f"{name} R={radius} flags={flags}"
        ref, ref_mask = um.upscale(lo, lp, hp, upscale_model_params(u, m))
        out, mask = u.upscale(lo, lp, hp, m, ctx)
        assert_bits_equal(out, ref, "host out_xyzw, " + what)
        assert_bits_equal(mask, ref_mask, "host out_mask, " + what)
        assert u.stats.launches_film == 1
        d_out.zero(), d_mask.zero()
        u.upscale_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, w, h, m, d_out.ptr, d_mask.ptr, ctx)
        assert_bits_equal(d_out.to_host(F, ref.shape), ref, "device out_xyzw, " + what)
        assert_bits_equal(d_mask.to_host(np.uint8, ref_mask.shape), ref_mask, "device out_mask, " + what)
        assert u.stats.launches_film == 1
        check_far(name, out, mask)
    free(d_lo, d_lp, d_hp, d_out, d_mask)


@pytest.mark.parametrize("name,radius", SMALL, ids=SMALL_IDS)
def test_temporal_upsample_equals_the_model_on_every_map(T, ctx, name, radius):
    lo, lp, hp, m, Hs, M = maps.temporal_frames(name)
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    tu = T.TemporalUpsampler(radius=radius, confidence_floor=0.25, max_history=8.0)
    d_lo, d_lp, d_hp, d_hs = device(T, lo, lp, hp, Hs)
    outs = [T._ffi.DeviceBuffer(n) for n in (h * w * 16, h * w * 48, h * w)]
    for history in (Hs, None):
        what = f"{name} R={radius} {'with' if history is not None else 'without'} history"
        ref = tum.accumulate(lo, lp, hp, history, M, temporal_model_params(tu, m))
        got = tu.accumulate(lo, lp, hp, history, m, M, ctx)
        for g, r, part in zip(got, ref, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"host {part}, {what}")
        assert tu.stats.launches_film == 1
        for b in outs:
            b.zero()
        tu.accumulate_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, d_hs.ptr if history is not None else None, w, h, m, M, outs[0].ptr, outs[1].ptr, outs[2].ptr, ctx)
        assert tu.stats.launches_film == 1
        for g, r, part in zip((outs[0].to_host(F, ref[0].shape), outs[1].to_host(F, ref[1].shape), outs[2].to_host(np.uint8, ref[2].shape)), ref, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"device {part}, {what}")
        check_far(name, got[0], got[2], got[1])
        if history is None:
            up, up_mask = guide_upscaler(T, tu).upscale(lo, lp, hp, m, ctx)
            assert_bits_equal(got[0], up, "without history the film is trhip_upscale's, " + what)
            assert_bits_equal(got[2], up_mask, "without history the mask is trhip_upscale's, " + what)
    free(d_lo, d_lp, d_hp, d_hs, *outs)


@pytest.mark.parametrize("name,radius", SMALL, ids=SMALL_IDS)
def test_temporal_upsample_motion_equals_the_model_on_every_map(T, ctx, name, radius):
    lo, lp, hp, m, Hs, M, ids, table, bodies = maps.motion_frames(name)
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    tu = T.TemporalUpsampler(radius=radius, confidence_floor=0.25, max_history=8.0, carry_bodies=True)
    d_lo, d_lp, d_hp, d_hs, d_ids, d_tb, d_mt = device(T, lo, lp, hp, Hs, ids, table, bodies)
    outs = [T._ffi.DeviceBuffer(n) for n in (h * w * 16, h * w * 48, h * w)]
    for history in (Hs, None):
        what = f"{name} R={radius} {'with' if history is not None else 'without'} history"
        ref = tumm.accumulate(lo, lp, hp, history, M, ids, table, bodies, temporal_model_params(tu, m))
        got = tu.accumulate_motion(lo, lp, hp, history, ids, table, bodies, m, M, ctx)
        for g, r, part in zip(got, ref, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"host {part}, {what}")
        assert tu.stats.launches_film == 1
        for b in outs:
            b.zero()
        tu.accumulate_motion_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, d_hs.ptr if history is not None else None, d_ids.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, m, M,
                                    outs[0].ptr, outs[1].ptr, outs[2].ptr, ctx)
        assert tu.stats.launches_film == 1
        for g, r, part in zip((outs[0].to_host(F, ref[0].shape), outs[1].to_host(F, ref[1].shape), outs[2].to_host(np.uint8, ref[2].shape)), ref, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"device {part}, {what}")
        check_far(name, got[0], got[2], got[1])
        if history is None:
            up, up_mask = guide_upscaler(T, tu).upscale(lo, lp, hp, m, ctx)
            assert_bits_equal(got[0], up, "without history the film is trhip_upscale's, " + what)
            assert_bits_equal(got[2], up_mask, "without history the mask is trhip_upscale's, " + what)
    free(d_lo, d_lp, d_hp, d_hs, d_ids, d_tb, d_mt, *outs)


# ---- the table, large maps: the host entry point, one call per kernel ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    yield maps.large_frames
    for name in maps.LARGE:
        maps.release(name)


@pytest.mark.parametrize("kernel", ["upscale", "temporal", "motion"])
@pytest.mark.parametrize("name", maps.LARGE)
def test_large_maps_equal_the_model(T, ctx, large, name, kernel):
    """spare_column: the lanes whose tap x0 + R lies on staged column or row T - 1.  Its tent weight is 0, so the temporal two run with confidence_sharpness = 0, where the
    confidence does weight that tap and the record staged there decides kmax (tests/test_upsample_maps.py shows it on the model).  strip_x / strip_y: 65 535 blocks on an axis, fx rounded at
    a spacing of 1 / 32 (R = 1, no history: upsample_maps.large_frames)."""
    lo, lp, hp, m, Hs, M, ids, table, bodies = large(name)
    R, rho = 1, 0.0 if name == "spare_column" else 2.0
    if kernel == "upscale":
        u = T.Upscaler(radius=R, demodulate=False, coverage=False)
        ref = um.upscale(lo, lp, hp, upscale_model_params(u, m))
        got, stats = u.upscale(lo, lp, hp, m, ctx), u.stats
        parts = ("out_xyzw", "out_mask")
    elif kernel == "temporal":
        tu = T.TemporalUpsampler(radius=R, confidence_floor=0.25, confidence_sharpness=rho, max_history=8.0)
        ref = tum.accumulate(lo, lp, hp, Hs, M, temporal_model_params(tu, m))
        got, stats = tu.accumulate(lo, lp, hp, Hs, m, M, ctx), tu.stats
        parts = ("out_xyzw", "out_history", "out_mask")
    else:
        tu = T.TemporalUpsampler(radius=R, confidence_floor=0.25, confidence_sharpness=rho, max_history=8.0, carry_bodies=True)
        ref = tumm.accumulate(lo, lp, hp, Hs, M, ids, table, bodies, temporal_model_params(tu, m))
        got, stats = tu.accumulate_motion(lo, lp, hp, Hs, ids, table, bodies, m, M, ctx), tu.stats
        parts = ("out_xyzw", "out_history", "out_mask")
    assert stats.launches_film == 1
    for g, r, part in zip(got, ref, parts):
        assert_bits_equal(g, r, f"{kernel} {part}, {name}")
    assert (ref[-1] & 3 == 1).sum() * 4 >= ref[-1].size, "a quarter of the pixels are guided"


# ---- the maps the product makes ---------------------------------------------------------------------------------------------------------------------------------------
SESSION = dict(spp=2, depth=3, seed=0xBEEF, guide_spp=1, degrees=(0.0, 1.5, 3.0))
CROPPED = dict(resolution=[96, 64], crop=([0.2, 0.1], [0.9, 0.7]))
# factor -> the full-size camera's arguments (ms.camera): films of at most 48 x 48 pixels, the cropped one 67 x 38
SESSION_CAMERAS = {"3": (3, dict(resolution=48)), "2.6-cropped": (2.6, CROPPED), "1": (1, dict(resolution=32)), "4": (4, dict(resolution=48))}


def session_cameras(T, which):
    factor, kw = SESSION_CAMERAS[which]
    return factor, [ms.camera(T, kw["resolution"], deg, crop=kw.get("crop")) for deg in SESSION["degrees"]]


def new_map(hi_cam, lo_cam, T, what, identity=False):
    """The frame's map, printed; it is none of the maps the suite launched before this module.  `identity`: the one exception — factor 1 without jitter IS the identity
    (1, 0, 1, 0), the map of the old 33 x 17 case; the session is run all the same, on a film of 2 x 2 blocks."""
    m = T.Upscaler.pixel_map(hi_cam, lo_cam)
    print(f"{what}: {hi_cam.film.size} <- {lo_cam.film.size}, lo_from_hi = {m}, T = {maps.staged_width(m, 1)} / {maps.staged_width(m, 2)}")
    if identity:
        assert m == (1.0, 0.0, 1.0, 0.0)
    else:
        assert not maps.is_old_map(m), f"{what}: {m} is a map the suite launched before"
    return m


@pytest.mark.parametrize("which", sorted(SESSION_CAMERAS))
def test_temporal_upsampling_sessions_at_other_factors_equal_the_calls_by_hand_and_the_model(T, ctx, which):
    """Three frames of a moving camera with jitter="halton": frame k is the path frame and its planes through the low camera shifted by jitter_for(k, factor), the full-size
    planes at guide_spp, trhip_temporal_upsample against the previous full-size camera and history, and the filter; every trhip_temporal_upsample call by hand is the
    model's on those inputs."""
    s = SESSION
    scene, (factor, cams) = T.scenes.cornell_scene(), session_cameras(T, which)
    tu, d = T.TemporalUpsampler(jitter="halton"), T.Denoiser()
    session = T.PreviewSession(scene, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], upscaler=T.Upscaler(), factor=factor, guide_spp=s["guide_spp"],
                               temporal_upsample=T.TemporalUpsampler(jitter="halton"))
    history, prev = None, None
    for k, cam in enumerate(cams):
        lo_cam = T.Upscaler.low_camera(cam, factor, jitter=tu.jitter_for(k, factor))
        smp = T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])
        lo_xyzw = T.PathIntegrator(lo_cam, smp, s["depth"]).render(scene, ctx)
        lo_planes = T.AOVIntegrator(lo_cam, smp).render(scene, ctx).planes
        hi_planes = T.AOVIntegrator(cam, T.SeededSampler(s["guide_spp"], seed=s["seed"], sample_offset=k * s["spp"])).render(scene, ctx).planes
        m = new_map(cam, lo_cam, T, f"temporal-upsampling session, factor {which}, frame {k}")
        ref = tum.accumulate(lo_xyzw, lo_planes, hi_planes, history, prev.world_to_pixel() if prev is not None else None, temporal_model_params(tu, m))
        acc, history_next, mask = tu.accumulate(lo_xyzw, lo_planes, hi_planes, history, m, prev, ctx)
        for g, r, part in zip((acc, history_next, mask), ref, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"factor {which}, frame {k}: {part} against the model")
        assert (mask & 3 == 1).sum() * 2 > mask.size, "most of the frame is guided"
        if k > 0:
            assert (mask >= 4).sum() * 2 > mask.size, "most of the frame finds its history"
        got = session.render(cam, ctx)
        assert_bits_equal(got, d.denoise(acc, hi_planes, ctx), f"factor {which}, session frame {k}")
        assert len(session.render_stats) == 5 and session.render_stats[3].launches_film == 1
        history, prev = history_next, cam
    session.close()


@pytest.mark.parametrize("which", sorted(SESSION_CAMERAS))
def test_upscaled_sessions_at_other_factors_equal_the_calls_by_hand_and_the_model(T, ctx, which):
    """PreviewSession(upscaler=Upscaler(), factor=...) without the temporal-upsampling mode: the low session's calls (path frame, planes, temporal pass, filter through the low
    camera), the full-size planes at guide_spp, trhip_upscale — and every trhip_upscale call by hand is the model's."""
    s = SESSION
    scene, (factor, cams) = T.scenes.cornell_scene(), session_cameras(T, which)
    u, d, t = T.Upscaler(), T.Denoiser(), T.TemporalAccumulator()
    session = T.PreviewSession(scene, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], upscaler=T.Upscaler(), factor=factor, guide_spp=s["guide_spp"])
    history, prev = None, None
    for k, cam in enumerate(cams):
        lo_cam = T.Upscaler.low_camera(cam, factor)
        smp = T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])
        xyzw = T.PathIntegrator(lo_cam, smp, s["depth"]).render(scene, ctx)
        lo_planes = T.AOVIntegrator(lo_cam, smp).render(scene, ctx).planes
        acc, history_next = t.accumulate(xyzw, lo_planes, history, prev, ctx)
        low = d.denoise(acc if history is not None else xyzw, lo_planes, ctx)
        hi_planes = T.AOVIntegrator(cam, T.SeededSampler(s["guide_spp"], seed=s["seed"], sample_offset=k * s["spp"])).render(scene, ctx).planes
        m = new_map(cam, lo_cam, T, f"upscaled session, factor {which}, frame {k}", identity=which == "1")
        ref, ref_mask = um.upscale(low, lo_planes, hi_planes, upscale_model_params(u, m))
        out, mask = u.upscale(low, lo_planes, hi_planes, m, ctx)
        assert_bits_equal(out, ref, f"factor {which}, frame {k}: out_xyzw against the model")
        assert_bits_equal(mask, ref_mask, f"factor {which}, frame {k}: out_mask against the model")
        assert (mask == 1).sum() * 2 > mask.size, "most of the frame is guided"
        got = session.render(cam, ctx)
        assert_bits_equal(got, out, f"factor {which}, session frame {k}")
        assert len(session.render_stats) == 6 and session.render_stats[5].launches_film == 1
        history, prev = history_next, lo_cam
    session.close()


def test_moving_bodies_session_at_factor_3_equals_the_calls_by_hand_and_the_model(T, ctx):
    """PreviewSession(temporal_upsample=TemporalUpsampler(carry_bodies=True, jitter="halton"), factor=3) over three frames of the moving scene on a turning camera: the
    low path frame and planes, the full-size planes and id plane with the guide sampler, trhip_temporal_upsample_motion, the filter; every call by hand is the model's."""
    s, factor = SESSION, 3
    frames = ms.scene_sequence(T, 3)
    tu, d = T.TemporalUpsampler(carry_bodies=True, jitter="halton"), T.Denoiser()
    session = T.PreviewSession(frames[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], upscaler=T.Upscaler(), factor=factor, guide_spp=s["guide_spp"],
                               temporal_upsample=T.TemporalUpsampler(carry_bodies=True, jitter="halton"))
    history, prev = None, None
    for k, ((scene, motion), deg) in enumerate(zip(frames, s["degrees"])):
        cam = ms.camera(T, 48, deg)
        lo_cam = T.Upscaler.low_camera(cam, factor, jitter=tu.jitter_for(k, factor))
        smp = T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])
        lo_xyzw = T.PathIntegrator(lo_cam, smp, s["depth"]).render(scene, ctx)
        lo_planes = T.AOVIntegrator(lo_cam, smp).render(scene, ctx).planes
        aov = T.AOVIntegrator(cam, T.SeededSampler(s["guide_spp"], seed=s["seed"], sample_offset=k * s["spp"]))
        hi_planes, ids = aov.render(scene, ctx).planes, aov.ids(scene, ctx)
        keys = sorted(motion)
        table = mats = None
        if keys:
            of_entry = [None] * len(T.top_level_counts(scene))
            for i, key in enumerate(keys):
                of_entry[key] = i
            table, mats = scene.flatten().body_table(of_entry), np.stack([T.TemporalAccumulator.prev_from_cur(motion[key]) for key in keys])
        m = new_map(cam, lo_cam, T, f"moving-bodies session, factor 3, frame {k}")
        tally = {}
        ref = tumm.accumulate(lo_xyzw, lo_planes, hi_planes, history, prev.world_to_pixel() if prev is not None else None, ids, table, mats, temporal_model_params(tu, m), tally)
        acc, history_next, mask = tu.accumulate_motion(lo_xyzw, lo_planes, hi_planes, history, ids, table, mats, m, prev, ctx)
        for g, r, part in zip((acc, history_next, mask), ref, ("out_xyzw", "out_history", "out_mask")):
            assert_bits_equal(g, r, f"frame {k}: {part} against the model")
        if k > 0:
            assert tally["moving"] > 50 and tally["moving_found"] > 25, tally
        session.scene = scene
        got = session.render(cam, ctx, motion=motion)
        assert_bits_equal(got, d.denoise(acc, hi_planes, ctx), f"session frame {k}")
        assert len(session.render_stats) == 5 and session.render_stats[3].launches_film == 1
        history, prev = history_next, cam
    session.close()
