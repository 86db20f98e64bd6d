"""Variance clipping of the reprojected history (trhip_temporal_clip, TemporalAccumulator(clip_gamma=, clip_radius=)) on the GPU: every output value against the numpy model
of tests/temporal_clip_model.py bit for bit — on synthetic frames that take every branch of the window walk and of the clip, at sizes below a window, off the 16 x 16 tile and
of several tiles, and on a real Cornell sequence —; gamma = +Inf against trhip_temporal bit for bit; host == device == aliased; the refusals that need a context; the relight
sequence; PreviewSession with a clipping accumulator.

Relight ratio measured on an MI355X with the default gamma and radius (MSE of xyz / w to the NEW lighting's 1024 spp frame over surface pixels, first frame after
Scene.with_lights with every intensity x 0.25, PreviewSession clipped / unclipped, both max_history = 8; profiles/r12/temporal_clip.txt): RELIGHT_MEASURED below."""
import copy
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import temporal_clip_model as cm
import temporal_model as tm
from test_gpu_temporal import SEQUENCE, assert_bits_equal, bits, camera, frame

pytestmark = pytest.mark.gpu

INF = float("inf")
SIZES = [(5, 3), (37, 29), (64, 64)]  # (w, h): smaller than a window both ways; partial tiles on both edges; 16 whole tiles
RADII = (1, 2, 3)
GAMMAS = (0.0, 1.0, INF)
SYNTHETIC = {}


def synthetic(h, w, radius, gamma):
    """(B, P, history, M, model outputs, tally): computed once per case and left unchanged."""
    if (h, w) not in SYNTHETIC:
        SYNTHETIC[(h, w)] = cm.synthetic(h, w, 2000 + h)
    if (h, w, radius, gamma) not in SYNTHETIC:
        B, P, Hs, M = SYNTHETIC[(h, w)]
        tally = {}
        SYNTHETIC[(h, w, radius, gamma)] = (cm.accumulate(B, P, Hs, M, cm.params(gamma, radius), tally), tally)
    (B, P, Hs, M), (ref, tally) = SYNTHETIC[(h, w)], SYNTHETIC[(h, w, radius, gamma)]
    return B.copy(), P.copy(), Hs.copy(), M.copy(), ref, tally


def synthetic_accumulator(T, radius, gamma):
    s = tm.SYNTHETIC_PARAMS
    return T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage, clip_gamma=gamma, clip_radius=radius)


def default_clip(T):
    p = T._ffi.TemporalClipParams()
    assert T.lib().trhip_temporal_clip_default_params(C.byref(p)) == 0
    return p.clip_gamma, p.clip_radius


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("size", SIZES, ids=["5x3", "37x29", "64x64"])
def test_synthetic_frames_equal_the_model(T, ctx, size, radius):
    w, h = size
    summed = {}
    for gamma in GAMMAS:
        B, P, Hs, M, (ref_out, ref_hist), tally = synthetic(h, w, radius, gamma)
        for name, v in tally.items():
            summed[name] = summed.get(name, 0) + v
    if size == (37, 29):  # checked on the CPU before anything goes to the GPU
        for name in cm.BRANCHES:
            assert summed.get(name, 0) >= 1, (name, summed)
    for gamma in GAMMAS:
        B, P, Hs, M, (ref_out, ref_hist), tally = synthetic(h, w, radius, gamma)
        t = synthetic_accumulator(T, radius, gamma)
        out, hist = t.accumulate(B, P, Hs, M, ctx)
        assert_bits_equal(out, ref_out, f"gamma {gamma}: out_xyzw")
        assert_bits_equal(hist, ref_hist, f"gamma {gamma}: out_history")
        assert t.stats.launches_film == 1
        surface = ref_hist[..., 1, 3] == 1
        assert_bits_equal(out[~surface], B[~surface], "non-surface pixels")
        assert not hist[~surface].any()
        assert_bits_equal(out[..., 3], B[..., 3], "the weight lane")
    # (the last gamma is +Inf) the unclipped pass on the same frames; and without history there is nothing to clip
    s = tm.SYNTHETIC_PARAMS
    plain = T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage)
    out_plain, hist_plain = plain.accumulate(B, P, Hs, M, ctx)
    assert_bits_equal(out, out_plain, "gamma = +Inf is trhip_temporal, out_xyzw")
    assert_bits_equal(hist, hist_plain, "gamma = +Inf is trhip_temporal, out_history")
    t = synthetic_accumulator(T, radius, 1.0)
    out0, hist0 = t.accumulate(B, P, None, None, ctx)
    ref0_out, ref0_hist = tm.accumulate(B, P, None, None, tm.SYNTHETIC_PARAMS)
    assert_bits_equal(out0, ref0_out, "history = NULL, out_xyzw")
    assert_bits_equal(hist0, ref0_hist, "history = NULL, out_history")
    try:  # the option has no effect on this kernel
        ctx.set_option("temporal_patch", 0)
        out1, hist1 = synthetic_accumulator(T, radius, 1.0).accumulate(B, P, Hs, M, ctx)
    finally:
        ctx.set_option("temporal_patch", 1)
    ref_out, ref_hist = synthetic(h, w, radius, 1.0)[4]
    assert_bits_equal(out1, ref_out, "temporal_patch = 0, out_xyzw")
    assert_bits_equal(hist1, ref_hist, "temporal_patch = 0, out_history")


@pytest.fixture(scope="module")
def cornell_sequence(T, ctx):
    """[(camera, xyzw, planes)] of the existing test's sequence: 48 x 48, 4 spp, depth 3, three cameras, frame k at sample_offset k * spp."""
    scene, s = T.scenes.cornell_scene(), SEQUENCE
    out = []
    for k, deg in enumerate(s["degrees"]):
        cam = camera(T, s["resolution"], deg)
        out.append((cam,) + frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"]))
    return out


@pytest.mark.parametrize("radius", RADII)
def test_infinite_gamma_is_the_unclipped_pass_on_the_cornell_sequence(T, ctx, cornell_sequence, radius):
    """trhip_temporal_clip_device with gamma = +Inf against trhip_temporal_device, chained over the three frames, each on its own device buffers."""
    clipped, plain = T.TemporalAccumulator(clip_gamma=INF, clip_radius=radius), T.TemporalAccumulator()
    h = w = SEQUENCE["resolution"]
    film_shape, planes_shape = (h, w, 4), (h, w, 3, 4)
    buf = lambda n: T._ffi.DeviceBuffer(h * w * n)  # noqa: E731
    d_film, d_planes, d_out, d_out_plain = buf(16), buf(48), buf(16), buf(16)
    hists, hists_plain = [buf(48), buf(48)], [buf(48), buf(48)]
    prev = None
    for k, (cam, xyzw, planes) in enumerate(cornell_sequence):
        d_film.from_host(xyzw)
        d_planes.from_host(planes)
        clipped.accumulate_device(d_film.ptr, d_planes.ptr, hists[k & 1].ptr if k else None, w, h, prev, d_out.ptr, hists[(k & 1) ^ 1].ptr, ctx)
        plain.accumulate_device(d_film.ptr, d_planes.ptr, hists_plain[k & 1].ptr if k else None, w, h, prev, d_out_plain.ptr, hists_plain[(k & 1) ^ 1].ptr, ctx)
        assert_bits_equal(d_out.to_host(np.float32, film_shape), d_out_plain.to_host(np.float32, film_shape), f"frame {k}, out_xyzw")
        new_hist = hists[(k & 1) ^ 1].to_host(np.float32, planes_shape)
        assert_bits_equal(new_hist, hists_plain[(k & 1) ^ 1].to_host(np.float32, planes_shape), f"frame {k}, out_history")
        prev = cam
    assert new_hist[..., 0, 3].max() == 3.0 and (new_hist[..., 0, 3] > 1).sum() > 1000, "the history was in use"
    for b in [d_film, d_planes, d_out, d_out_plain] + hists + hists_plain:
        b.free()


def test_cornell_sequence_with_the_defaults_equals_the_model(T, ctx, cornell_sequence):
    gamma, radius = default_clip(T)
    t = T.TemporalAccumulator(clip_gamma=gamma)
    assert t.clip_params.clip_radius == radius
    p = t.params
    prm = cm.Params(p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage, gamma, radius)
    hist, prev, tally = None, None, {}
    for k, (cam, xyzw, planes) in enumerate(cornell_sequence):
        M = prev.world_to_pixel() if prev is not None else None
        ref_out, ref_hist = cm.accumulate(xyzw, planes, hist, M, prm, tally)
        out, new_hist = t.accumulate(xyzw, planes, hist, prev, ctx)
        assert_bits_equal(out, ref_out, f"frame {k}, out_xyzw")
        assert_bits_equal(new_hist, ref_hist, f"frame {k}, out_history")
        assert_bits_equal(out[..., 3], xyzw[..., 3], f"frame {k}, the weight lane")
        hist, prev = new_hist, cam
    print(f"cornell sequence, gamma {gamma}, radius {radius}, tally: {tally}")
    assert tally["pixels_clipped"] > 100 and tally["pixels_inside"] > 100, tally
    assert hist[..., 0, 3].max() == 3.0


def test_host_device_and_aliased_calls_agree(T, ctx):
    for radius, gamma in ((3, 1.0), (1, 0.0)):
        B, P, Hs, M, (ref_out, ref_hist), _ = synthetic(29, 37, radius, gamma)
        h, w = B.shape[:2]
        t = synthetic_accumulator(T, radius, gamma)
        d_in, d_pl, d_hs, d_out, d_oh = (T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in (B, P, Hs, np.zeros_like(B), np.zeros_like(P)))
        t.accumulate_device(d_in.ptr, d_pl.ptr, d_hs.ptr, w, h, M, d_out.ptr, d_oh.ptr, ctx)
        assert_bits_equal(d_out.to_host(np.float32, B.shape), ref_out, "device variant, out_xyzw")
        assert_bits_equal(d_oh.to_host(np.float32, P.shape), ref_hist, "device variant, out_history")
        for buf, a, what in ((d_in, B, "xyzw"), (d_pl, P, "planes"), (d_hs, Hs, "history")):
            assert_bits_equal(buf.to_host(np.float32, a.shape), a, f"the input {what} is left alone")
        d_oh.zero()
        # a window reads its neighbours' film pixels: an aliased result goes through a film of the context's, and is the same bits
        t.accumulate_device(d_in.ptr, d_pl.ptr, d_hs.ptr, w, h, M, d_in.ptr, d_oh.ptr, ctx)
        assert_bits_equal(d_in.to_host(np.float32, B.shape), ref_out, "out aliasing xyzw, device")
        assert_bits_equal(d_oh.to_host(np.float32, P.shape), ref_hist, "out aliasing xyzw, device, out_history")
        buf, hist = B.copy(), np.empty_like(P)
        p = t._clip_params_for(M)
        rc = T.lib().trhip_temporal_clip(ctx._h, T._ffi.fptr(buf), T._ffi.fptr(P), T._ffi.fptr(Hs), w, h, C.byref(p), T._ffi.fptr(buf), T._ffi.fptr(hist), None)
        assert rc == 0
        assert_bits_equal(buf, ref_out, "out aliasing xyzw, host")
        assert_bits_equal(hist, ref_hist, "out aliasing xyzw, host, out_history")
        for b in (d_in, d_pl, d_hs, d_out, d_oh):
            b.free()


def test_refusals(T, ctx):
    B, P, Hs, M, (ref_out, ref_hist), _ = synthetic(29, 37, 2, 1.0)
    h, w = B.shape[:2]
    L, t = T.lib(), synthetic_accumulator(T, 2, 1.0)
    p = t._clip_params_for(M)
    out, hist = np.zeros_like(B), np.zeros_like(P)
    ptr = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731

    def call(xyzw=B, planes=P, history=Hs, w=w, h=h, prm=p, o=out, oh=hist, handle=ctx._h):
        return L.trhip_temporal_clip(handle, ptr(xyzw), ptr(planes), ptr(history), w, h, C.byref(prm) if prm is not None else None, ptr(o), ptr(oh), None)
    assert call() == 0
    for kw in (dict(prm=None), dict(xyzw=None), dict(planes=None), dict(o=None), dict(oh=None), dict(w=0), dict(h=0), dict(handle=None)):
        assert call(**kw) == -1, kw
        assert L.trhip_last_error(None if "handle" in kw else ctx._h).decode(), kw
    for kw in (dict(oh=Hs), dict(oh=P), dict(history=hist), dict(planes=hist)):
        assert call(**kw) == -1, list(kw)
        assert "overlap" in L.trhip_last_error(ctx._h).decode()
    big = np.zeros(P.size + B.size, np.float32)
    tail = big[B.size // 2:B.size // 2 + P.size].reshape(P.shape)
    assert call(o=big[:B.size].reshape(B.shape), oh=tail) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    assert call(xyzw=big[:B.size].reshape(B.shape), oh=tail) == -1
    for field, value, word in (("clip_gamma", -1.0, "clip_gamma"), ("clip_radius", 4, "clip_radius"), ("flags", 2, "flag"), ("reserved", 1, "reserved")):
        bad = T._ffi.TemporalClipParams.from_buffer_copy(p)
        setattr(bad, field, value)
        assert call(prm=bad) == -1 and word in L.trhip_last_error(ctx._h).decode(), field
    bad = T._ffi.TemporalClipParams.from_buffer_copy(p)
    bad.base.max_history = 0.0
    assert call(prm=bad) == -1 and "max_history" in L.trhip_last_error(ctx._h).decode()
    with pytest.raises(T.TraceHipError):
        T.TemporalAccumulator(clip_radius=5).accumulate(B, P, None, None, ctx)
    with pytest.raises(T.TraceHipError):
        T.TemporalAccumulator(clip_gamma=float("nan")).accumulate(B, P, None, None, ctx)
    out[:], hist[:] = 0, 0
    assert call() == 0, "a refused call leaves the context usable"
    assert_bits_equal(out, ref_out, "after the refusals, out_xyzw")
    assert_bits_equal(hist, ref_hist, "after the refusals, out_history")


def dimmed(T, scene, factor):
    lights = []
    for light in scene.lights:
        light = copy.copy(light)
        light.i = T.RGBSpectrum(*[float(np.float32(factor) * v) for v in light.i.c])
        lights.append(light)
    return scene.with_lights(lights)


RELIGHT = dict(resolution=48, spp=4, depth=3, seed=0x7E3A, before=4, after=2, factor=0.25)
RELIGHT_MEASURED = 0.2800  # mse(clipped session) / mse(unclipped session), first frame after the change of lights


def test_relight_without_reset(T, ctx):
    """Cornell through a static camera: four frames with the scene's own lights, then `session.scene = scene.with_lights(...)` with every intensity x 0.25 and NO reset(), then
    two more frames; two sessions with max_history = 8, one clipping at the default gamma and radius, one not.  MSE of xyz / w over surface pixels against the NEW lighting's
    1024 spp frame, for the first frame after the change.  The frames are bit-reproducible, so the ratio clipped / unclipped is a number, not a distribution; the assertion
    is that it lies below the midpoint between its measured value and 1 (the convention of QUALITY_MEASURED in tests/test_gpu_temporal.py).  By the arithmetic it is far
    below 1: the unclipped history carries 7/8 of a 4 x error into the frame, the clipped one at most about gamma * sd of the new frame's own colours."""
    r = RELIGHT
    scene = T.scenes.cornell_scene()
    dim = dimmed(T, scene, r["factor"])
    cam = camera(T, r["resolution"], 0.0)
    gamma, radius = default_clip(T)
    sessions = {"clipped": T.PreviewSession(scene, T.SeededSampler(r["spp"], seed=r["seed"]), r["depth"], temporal=T.TemporalAccumulator(max_history=8, clip_gamma=gamma, clip_radius=radius)),
                "unclipped": T.PreviewSession(scene, T.SeededSampler(r["spp"], seed=r["seed"]), r["depth"], temporal=T.TemporalAccumulator(max_history=8))}
    frames = {name: [] for name in sessions}
    for name, session in sessions.items():
        for k in range(r["before"] + r["after"]):
            if k == r["before"]:
                session.scene = dim
            frames[name].append(session.render(cam, ctx))
        session.close()
    assert_bits_equal(frames["clipped"][0], frames["unclipped"][0], "the first frame has no history to clip")
    offset = r["before"] * r["spp"]
    noisy, planes = frame(T, dim, cam, r["spp"], r["depth"], r["seed"], offset)
    surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))
    assert surface.sum() >= 1000

    def mse(a, target):
        with np.errstate(all="ignore"):
            diff = a[surface][:, :3].astype(np.float64) / a[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
        return float(np.mean(diff * diff))
    new = T.PathIntegrator(cam, T.SeededSampler(1024, seed=0x7A26E7), r["depth"]).render(dim)
    old = T.PathIntegrator(cam, T.SeededSampler(1024, seed=0x7A26E7), r["depth"]).render(scene)
    series = {name: [round(mse(f, new if k >= r["before"] else old), 6) for k, f in enumerate(fs)] for name, fs in frames.items()}
    print(f"relight, gamma {gamma}, radius {radius}: per-frame mse against the lighting of the frame: {series}")
    k = r["before"]
    clipped, unclipped = mse(frames["clipped"][k], new), mse(frames["unclipped"][k], new)
    ratio = clipped / unclipped
    print(f"relight: first frame after the change: mse 4 spp {mse(noisy, new):.6g}, unclipped session {unclipped:.6g}, clipped session {clipped:.6g}, ratio {ratio:.4f}")
    assert_bits_equal(frames["clipped"][k][..., 3], noisy[..., 3], "the weight lane")
    assert ratio < 0.5 * (RELIGHT_MEASURED + 1.0)


def test_preview_session_with_a_clipping_accumulator(T, ctx):
    scene = T.scenes.cornell_scene()
    spp, depth, seed = 4, 3, 0x7E3A
    make = lambda: T.TemporalAccumulator(clip_gamma=0.5, clip_radius=2)  # noqa: E731
    session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, temporal=make())
    t, d = make(), T.Denoiser()
    hist, prev = None, None
    for k, deg in enumerate((0.0, 3.0, 6.0)):
        cam = camera(T, 48, deg)
        got = session.render(cam, ctx)
        xyzw, planes = frame(T, scene, cam, spp, depth, seed, k * spp)
        acc, hist = t.accumulate(xyzw, planes, hist, prev, ctx)
        want = d.denoise(acc if k else xyzw, planes, ctx)
        assert_bits_equal(got, want, f"frame {k}: path + planes + clipped temporal + denoise by hand")
        assert_bits_equal(got[..., 3], xyzw[..., 3], f"frame {k}: the weight lane")
        assert len(session.render_stats) == 4 and session.render_stats[2].launches_film == 1
        prev = cam
    plain = T.TemporalAccumulator().accumulate(xyzw, planes, None, None, ctx)[0]
    assert (bits(acc) != bits(plain)).mean() > 0.3, "the clipped history is in use"
    assert session.frame == 3
    # reset() and a film of another size behave as in the unclipped session: the next frame is Denoiser.render's
    session.reset()
    cam = camera(T, 48, 9.0)
    got = session.render(cam, ctx)
    assert_bits_equal(got, T.Denoiser().render(scene, cam, T.SeededSampler(spp, seed=seed, sample_offset=3 * spp), depth, ctx), "after reset(): Denoiser.render of that frame")
    small = camera(T, 32, 9.0)
    got = session.render(small, ctx)
    assert got.shape == (32, 32, 4)
    assert_bits_equal(got, T.Denoiser().render(scene, small, T.SeededSampler(spp, seed=seed, sample_offset=4 * spp), depth, ctx), "after a change of size")
    again = session.render(small, ctx)
    assert (bits(again) != bits(T.Denoiser().render(scene, small, T.SeededSampler(spp, seed=seed, sample_offset=5 * spp), depth, ctx))).mean() > 0.3, "the history is in use again"
    session.close()
