"""Temporal reprojection (trhip_temporal, TemporalAccumulator, PreviewSession) on the GPU: every output value against the numpy model of tests/temporal_model.py bit for bit — on
synthetic inputs that take every branch of the specification, and on a real Cornell sequence of three cameras —, both lane-to-pixel mappings, determinism, host == device,
aliasing, the refusals that need a context, the static-camera property, the quality condition against 1024 spp frames, and PreviewSession.

Quality ratios measured on an MI355X with the default parameters (MSE of xyz / w to the 1024 spp frame over surface pixels of the eighth frame of an arc, PreviewSession /
Denoiser alone; profiles/r11/temporal.txt): Cornell 0.0919, mesh_scene(16) 0.0984 (QUALITY_MEASURED below)."""
import ctypes as C
import math

import numpy as np
import pytest

import denoise_model as dm
import temporal_model as tm

pytestmark = pytest.mark.gpu

BRANCHES = ("integer_x", "integer_y", "off_left", "off_right", "off_top", "off_bottom", "behind", "non_finite", "reject_normal", "reject_plane", "reject_flag", "all_rejected", "capped",
            "below_cap", "nan_colour", "accepted")
CENTRE = np.array([0.5, 0.4, -2.5])  # of the Cornell box: the cameras of a sequence turn about it


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def model_params(t):
    p = t.params
    return tm.Params(p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage)


def camera(T, resolution, degrees=0.0):
    """The denoiser tests' camera, turned about the vertical axis through the box's centre."""
    a = math.radians(degrees)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    eye, target = CENTRE + R @ (np.array([0.0, 15.0, 50.0]) - CENTRE), CENTRE + R @ (np.array([0.0, 0.0, -2.0]) - CENTRE)
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at(eye.tolist(), target.tolist(), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def frame(T, scene, cam, spp, depth, seed, offset=0):
    """(xyzw, planes) of a path frame and its feature planes with the same sampler settings."""
    xyzw = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed, sample_offset=offset), depth).render(scene)
    planes = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed, sample_offset=offset)).render(scene).planes
    return xyzw, planes


SYNTHETIC = {}


def synthetic(h, w):
    """(B, P, history, model outputs, tally): computed once per size and left unchanged."""
    if (h, w) not in SYNTHETIC:
        B, P, Hs = tm.synthetic(h, w, 2000 + h)
        tally = {}
        ref = tm.accumulate(B, P, Hs, tm.SYNTHETIC_M, tm.SYNTHETIC_PARAMS, tally)
        SYNTHETIC[(h, w)] = (B, P, Hs, ref, tally)
    B, P, Hs, ref, tally = SYNTHETIC[(h, w)]
    return B.copy(), P.copy(), Hs.copy(), ref, tally


def synthetic_accumulator(T):
    s = tm.SYNTHETIC_PARAMS
    return T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage)


@pytest.mark.parametrize("size", [(37, 29), (64, 64)], ids=["37x29", "64x64"])
def test_synthetic_frames_equal_the_model(T, ctx, size):
    """Both lane-to-pixel mappings must give the model's bits; 37 x 29 is no multiple of the 16 x 16 block or of a wave, 64 x 64 is 16 blocks."""
    w, h = size
    B, P, Hs, (ref_out, ref_hist), tally = synthetic(h, w)
    for name in BRANCHES:
        assert tally.get(name, 0) >= 20, (name, tally)
    t = synthetic_accumulator(T)
    surface = ref_hist[..., 1, 3] == 1
    assert surface.sum() > 500 and (~surface).sum() > 50
    try:
        for patch in (0, 1):
            ctx.set_option("temporal_patch", patch)
            out, hist = t.accumulate(B, P, Hs, tm.SYNTHETIC_M, ctx)
            assert_bits_equal(out, ref_out, f"out_xyzw, temporal_patch = {patch}")
            assert_bits_equal(hist, ref_hist, f"out_history, temporal_patch = {patch}")
            assert t.stats.launches_film == 1
            out2, hist2 = t.accumulate(B, P, Hs, tm.SYNTHETIC_M, ctx)
            assert_bits_equal(out2, out, "second run, out_xyzw")
            assert_bits_equal(hist2, hist, "second run, out_history")
            # without history: XYZ -> RGB -> XYZ of every surface pixel, the input elsewhere, per the model
            ref0_out, ref0_hist = tm.accumulate(B, P, None, None, tm.SYNTHETIC_PARAMS)
            out0, hist0 = t.accumulate(B, P, None, None, ctx)
            assert_bits_equal(out0, ref0_out, "history = NULL, out_xyzw")
            assert_bits_equal(hist0, ref0_hist, "history = NULL, out_history")
            # a history, but the default parameters' zero matrix: nothing is found through it
            out00, hist00 = t.accumulate(B, P, Hs, None, ctx)
            assert_bits_equal(out00, ref0_out, "zero matrix, out_xyzw")
            assert_bits_equal(hist00, ref0_hist, "zero matrix, out_history")
    finally:
        ctx.set_option("temporal_patch", 1)
    assert_bits_equal(out[~surface], B[~surface], "non-surface pixels")
    assert not hist[~surface].any()
    assert_bits_equal(out[..., 3], B[..., 3], "the weight lane")
    with np.errstate(all="ignore"):
        back = dm.rgb_to_xyz(dm.xyz_to_rgb(B[..., :3] * (np.float32(1.0) / B[..., 3])[..., None])) * B[..., 3][..., None]
    assert_bits_equal(out0[surface][:, :3], back[surface], "history = NULL is the colour round trip")


def test_host_device_and_aliased_calls_agree(T, ctx):
    B, P, Hs, (ref_out, ref_hist), _ = synthetic(29, 37)
    h, w = B.shape[:2]
    t = synthetic_accumulator(T)
    d_in, d_pl, d_hs, d_out, d_oh = (T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in (B, P, Hs, np.zeros_like(B), np.zeros_like(P)))
    t.accumulate_device(d_in.ptr, d_pl.ptr, d_hs.ptr, w, h, tm.SYNTHETIC_M, d_out.ptr, d_oh.ptr, ctx)
    assert_bits_equal(d_out.to_host(np.float32, B.shape), ref_out, "device variant, out_xyzw")
    assert_bits_equal(d_oh.to_host(np.float32, P.shape), ref_hist, "device variant, out_history")
    for buf, a, what in ((d_in, B, "xyzw"), (d_pl, P, "planes"), (d_hs, Hs, "history")):
        assert_bits_equal(buf.to_host(np.float32, a.shape), a, f"the input {what} is left alone")
    d_oh.zero()
    t.accumulate_device(d_in.ptr, d_pl.ptr, d_hs.ptr, w, h, tm.SYNTHETIC_M, d_in.ptr, d_oh.ptr, ctx)
    assert_bits_equal(d_in.to_host(np.float32, B.shape), ref_out, "out aliasing xyzw, device")
    assert_bits_equal(d_oh.to_host(np.float32, P.shape), ref_hist, "out aliasing xyzw, device, out_history")
    buf, hist = B.copy(), np.empty_like(P)
    p = t._params_for(tm.SYNTHETIC_M)
    rc = T.lib().trhip_temporal(ctx._h, T._ffi.fptr(buf), T._ffi.fptr(P), T._ffi.fptr(Hs), w, h, C.byref(p), T._ffi.fptr(buf), T._ffi.fptr(hist), None)
    assert rc == 0
    assert_bits_equal(buf, ref_out, "out aliasing xyzw, host")
    assert_bits_equal(hist, ref_hist, "out aliasing xyzw, host, out_history")


def test_refusals(T, ctx):
    B, P, Hs, _, _ = synthetic(29, 37)
    h, w = B.shape[:2]
    L, t = T.lib(), synthetic_accumulator(T)
    p = t._params_for(tm.SYNTHETIC_M)
    out, hist = np.zeros_like(B), np.zeros_like(P)
    ptr = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731

    def call(xyzw=B, planes=P, history=Hs, w=w, h=h, prm=p, o=out, oh=hist, handle=ctx._h):
        return L.trhip_temporal(handle, ptr(xyzw), ptr(planes), ptr(history), w, h, C.byref(prm) if prm is not None else None, ptr(o), ptr(oh), None)
    assert call() == 0
    for kw in (dict(prm=None), dict(xyzw=None), dict(planes=None), dict(o=None), dict(oh=None), dict(w=0), dict(h=0), dict(handle=None)):
        assert call(**kw) == -1, kw
        assert L.trhip_last_error(None if "handle" in kw else ctx._h).decode(), kw
    # out_history may overlap nothing that is read or written beside it, in whole or in part
    for kw in (dict(oh=Hs), dict(oh=P), dict(history=hist), dict(planes=hist)):
        assert call(**kw) == -1, list(kw)
        assert "overlap" in L.trhip_last_error(ctx._h).decode()
    big = np.zeros(P.size + B.size, np.float32)
    tail = big[B.size // 2:B.size // 2 + P.size].reshape(P.shape)
    assert call(o=big[:B.size].reshape(B.shape), oh=tail) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    assert call(xyzw=big[:B.size].reshape(B.shape), oh=tail) == -1
    bad = T._ffi.TemporalParams.from_buffer_copy(p)
    bad.max_history = 0.0
    assert call(prm=bad) == -1 and "max_history" in L.trhip_last_error(ctx._h).decode()
    with pytest.raises(T.TraceHipError):
        T.TemporalAccumulator(sigma_plane=-1.0).accumulate(B, P, None, None, ctx)
    assert call() == 0, "a refused call leaves the context usable"


SEQUENCE = dict(resolution=48, spp=4, depth=3, seed=0x7E3A, degrees=(0.0, 3.0, 6.0))


@pytest.fixture(scope="module")
def cornell_sequence(T, ctx):
    """[(camera, xyzw, planes)] of three cameras a few degrees apart, frame k at sample_offset k * spp."""
    scene, s = T.scenes.cornell_scene(), SEQUENCE
    out = []
    for k, deg in enumerate(s["degrees"]):
        cam = camera(T, s["resolution"], deg)
        out.append((cam,) + frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"]))
    return out


def test_cornell_sequence_equals_the_model(T, ctx, cornell_sequence):
    t = T.TemporalAccumulator()
    prm = model_params(t)
    hist, prev, tally = None, None, {}
    for k, (cam, xyzw, planes) in enumerate(cornell_sequence):
        M = prev.world_to_pixel() if prev is not None else None
        ref_out, ref_hist = tm.accumulate(xyzw, planes, hist, M, prm, tally)
        out, new_hist = t.accumulate(xyzw, planes, hist, prev, ctx)
        assert_bits_equal(out, ref_out, f"frame {k}, out_xyzw")
        assert_bits_equal(new_hist, ref_hist, f"frame {k}, out_history")
        assert_bits_equal(out[..., 3], xyzw[..., 3], f"frame {k}, the weight lane")
        hist, prev = new_hist, cam
    print(f"cornell sequence tally: {tally}")
    rejected = tally["reject_flag"] + tally["reject_normal"] + tally["reject_plane"]
    assert tally["accepted"] > 1000 and tally["blended"] > 1000, tally
    assert tally["reject_normal"] + tally["reject_plane"] > 0 and rejected > 20, ("no disoccluded tap", tally)
    assert hist[..., 0, 3].max() == 3.0, "three frames: the longest history is 3"


def test_static_camera_doubles_the_history(T, ctx, cornell_sequence):
    """The same camera twice: every surface pixel with full coverage ends with N' = 2 (each of its accepted taps has N = 1, so N_h = sN / sb = 1 exactly).

    Asserted for EVERY such pixel on the frame shown twice: its own history record then has its very normal and position, lies among its four taps (the mean of hit points
    within a filter footprint of one pixel's radius projects less than a pixel from the centre) and is accepted.  With new samples in the second frame — what a session
    renders — the pixels whose footprint straddles a sphere's silhouette or an edge carry another mixture of the two surfaces each frame, and some of them find no tap within
    sigma_plane / sigma_normal: measured on an MI355X at 48 x 48, 4 spp, 1974 of 1987 full-coverage pixels end with N' = 2 and 13 with N' = 1, as the model says bit for
    bit.  That is the specified arithmetic at work (a mixed pixel is its own small disocclusion), so for that frame the assertion is the part that follows from the
    specification: N' is 1 or 2 everywhere, and 2 wherever the pixel's own record passes both tests at a position less than a pixel away."""
    scene, s = T.scenes.cornell_scene(), SEQUENCE
    cam, xyzw0, planes0 = cornell_sequence[0]
    t = T.TemporalAccumulator()
    prm = model_params(t)
    _, hist0 = t.accumulate(xyzw0, planes0, None, None, ctx)
    full0 = (hist0[..., 1, 3] == 1) & (bits(planes0[..., 1, 3]) == bits(planes0[..., 0, 3]))
    assert full0.sum() > 1000
    # the frame itself, again
    _, hist_same = t.accumulate(xyzw0, planes0, hist0, cam, ctx)
    N = hist_same[..., 0, 3]
    print(f"static camera, the same frame: {int(full0.sum())} surface pixels with full coverage, N' == 2 at {int((N[full0] == 2).sum())}")
    assert np.all(N[full0] == 2.0), f"{int((N[full0] != 2).sum())} full-coverage pixels found no history in their own frame"
    # the next frame of a session: new samples
    xyzw1, planes1 = frame(T, scene, cam, s["spp"], s["depth"], s["seed"], s["spp"])
    _, hist1 = t.accumulate(xyzw1, planes1, hist0, cam, ctx)
    surface = hist1[..., 1, 3] == 1
    full = surface & full0 & (bits(planes1[..., 1, 3]) == bits(planes1[..., 0, 3]))
    N = hist1[..., 0, 3]
    print(f"static camera, new samples: {int(surface.sum())} surface pixels, {int(full.sum())} with full coverage in both frames, N' == 2 at {int((N[full] == 2).sum())}, "
          f"N' == 1 at {int((N[full] == 1).sum())}")
    assert set(np.unique(N[surface])) <= {1.0, 2.0}
    n1, p1, n0, p0 = hist1[..., 1, :3], hist1[..., 2, :3], hist0[..., 1, :3], hist0[..., 2, :3]
    hx, hy, hz = tm.project(cam.world_to_pixel(), p1)
    ys, xs = np.mgrid[0:surface.shape[0], 0:surface.shape[1]]
    with np.errstate(all="ignore"):
        near = (hz > 0) & (np.abs(hx / hz - xs) < 0.999) & (np.abs(hy / hz - ys) < 0.999)
        own_passes = (np.float32(1.0) - dm.dot3(n1, n0) < np.float32(prm.sigma_normal)) & (np.abs(dm.dot3(n1, p0 - p1)) < np.float32(prm.sigma_plane))
    must = full & near & own_passes
    assert must.sum() > 0.5 * full.sum(), (int(must.sum()), int(full.sum()))
    assert np.all(N[must] == 2.0)


QUALITY = dict(resolution=64, spp=2, depth=5, seed=0xBEEF, degrees=tuple(0.75 * k for k in range(8)))
QUALITY_SCENES = {"cornell": lambda T: T.scenes.cornell_scene(), "mesh16": lambda T: T.scenes.mesh_scene(16)}
QUALITY_MEASURED = {"cornell": 0.0919, "mesh16": 0.0984}  # mse(PreviewSession) / mse(Denoiser alone), eighth frame


@pytest.mark.parametrize("which", sorted(QUALITY_SCENES))
def test_history_brings_the_preview_closer_to_the_1024spp_frame(T, ctx, which):
    """Eight cameras on an arc at 2 spp: the last frame through PreviewSession against the same frame through Denoiser alone, both measured (MSE of xyz / w over surface
    pixels) against that camera's 1024 spp frame.  The frames are bit-reproducible, so the ratio is a number, not a distribution; the assertion is that it lies below the
    midpoint between its measured value and 1 — it fails when the history stops being used."""
    scene, q = QUALITY_SCENES[which](T), QUALITY
    sampler = T.SeededSampler(q["spp"], seed=q["seed"])
    session = T.PreviewSession(scene, sampler, q["depth"])
    cams = [camera(T, q["resolution"], deg) for deg in q["degrees"]]
    for cam in cams:
        preview = session.render(cam, ctx)
    session.close()
    last, offset = cams[-1], (len(cams) - 1) * q["spp"]
    alone = T.Denoiser().render(scene, last, T.SeededSampler(q["spp"], seed=q["seed"], sample_offset=offset), q["depth"], ctx)
    noisy, planes = frame(T, scene, last, q["spp"], q["depth"], q["seed"], offset)
    target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), q["depth"]).render(scene)
    surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))
    assert surface.sum() >= 1000
    assert_bits_equal(preview[..., 3], noisy[..., 3], "the weight lane")

    def mse(a):
        with np.errstate(all="ignore"):
            diff = a[surface][:, :3].astype(np.float64) / a[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
        return float(np.mean(diff * diff))
    raw, without, with_history = mse(noisy), mse(alone), mse(preview)
    ratio = with_history / without
    print(f"temporal quality {which}: mse 2 spp {raw:.6g}, Denoiser alone {without:.6g}, PreviewSession {with_history:.6g}, ratio {ratio:.4f}")
    assert ratio < 0.5 * (QUALITY_MEASURED[which] + 1.0)


def test_preview_session_chains_resets_and_keeps_the_weights(T, ctx):
    scene = T.scenes.cornell_scene()
    spp, depth, seed = 4, 3, 0x7E3A
    session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth)
    t, d = T.TemporalAccumulator(), T.Denoiser()
    hist, prev = None, None
    for k, deg in enumerate((0.0, 3.0, 6.0)):
        cam = camera(T, 48, deg)
        got = session.render(cam, ctx)
        xyzw, planes = frame(T, scene, cam, spp, depth, seed, k * spp)
        acc, hist = t.accumulate(xyzw, planes, hist, prev, ctx)
        want = d.denoise(acc if k else xyzw, planes, ctx)
        assert_bits_equal(got, want, f"frame {k}: path + planes + temporal + denoise by hand")
        assert_bits_equal(got[..., 3], xyzw[..., 3], f"frame {k}: the weight lane")
        assert len(session.render_stats) == 4 and session.render_stats[2].launches_film == 1
        prev = cam
    assert session.frame == 3
    session.reset()
    cam = camera(T, 48, 9.0)
    got = session.render(cam, ctx)
    assert_bits_equal(got, T.Denoiser().render(scene, cam, T.SeededSampler(spp, seed=seed, sample_offset=3 * spp), depth, ctx), "after reset(): Denoiser.render of that frame")
    # a film of another size resets as well
    small = camera(T, 32, 9.0)
    got = session.render(small, ctx)
    assert got.shape == (32, 32, 4)
    assert_bits_equal(got, T.Denoiser().render(scene, small, T.SeededSampler(spp, seed=seed, sample_offset=4 * spp), depth, ctx), "after a change of size")
    again = session.render(small, ctx)
    assert (bits(again) != bits(T.Denoiser().render(scene, small, T.SeededSampler(spp, seed=seed, sample_offset=5 * spp), depth, ctx))).mean() > 0.3, "the history is in use again"
    session.close()
    small.film.set_xyzw(again)
