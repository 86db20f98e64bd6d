"""trhip_upscale on the GPU: the kernel against the numpy model of tests/upscale_model.py, bit for bit in every
output value and every mask byte, at the sizes where the tiling, the border and the footprint change; host and device entry points; the overlap refusals; a Cornell frame
through Upscaler.render and by hand; PreviewSession without an upscaler against the call sequence it has always made; and one quality figure per scene.

Quality ratios measured on an MI355X (MSE of xyz / w to the 64^2 1024 spp frame over all pixels of positive weight, Upscaler().render at factor 2 from a 32^2 4 spp frame /
the same low film upscaled bilinearly, H5 on every pixel; profiles/r14/upscale.txt): Cornell 0.6881, mesh_scene(16) 0.6920 (QUALITY_MEASURED below)."""
import ctypes as C

import numpy as np
import pytest

import upscale_model as um

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1

# (full-size h, w) <- (low h, w): smaller than a footprint; non-integer ratio with partial tiles; the 2 x case with its -0.75; the ratio limit; ratio 1, the largest staged
# footprint, two tiles
SIZES = {"5x3<-3x2": ((3, 5), (2, 3)), "37x29<-19x15": ((29, 37), (15, 19)), "64x64<-32x32": ((64, 64), (32, 32)), "48x32<-12x8": ((32, 48), (8, 12)),
         "33x17<-33x17": ((17, 33), (17, 33))}
PAIRS = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def pair(name):
    if name not in PAIRS:
        (hh, hw), (lh, lw) = SIZES[name]
        PAIRS[name] = um.synthetic_pair(hh, hw, lh, lw, 4000 + hw)
    lo, lp, hp, m = PAIRS[name]
    return lo.copy(), lp.copy(), hp.copy(), m


def model_params(u, m):
    p = u.params
    return um.Params(m, radius=p.radius, demodulate=bool(p.flags & 1), coverage=bool(p.flags & 2), sigma_normal=p.sigma_normal, sigma_plane=p.sigma_plane,
                     albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)


@pytest.mark.parametrize("flags", [True, False], ids=["demodulated+coverage", "plain"])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_synthetic_pairs_equal_the_model(T, ctx, size, radius, flags):
    lo, lp, hp, m = pair(size)
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    u = T.Upscaler(radius=radius, demodulate=flags, coverage=flags)
    ref, ref_mask = um.upscale(lo, lp, hp, model_params(u, m))
    if size == "64x64<-32x32":
        assert m == (0.5, -0.75, 0.5, -0.75)
    out, mask = u.upscale(lo, lp, hp, m, ctx)
    assert_bits_equal(out, ref, "out_xyzw")
    assert_bits_equal(mask, ref_mask, "out_mask")
    assert u.stats.launches_film == 1
    # host entry point without a mask
    p = u._params_for(m)
    out2 = np.full_like(out, 7.0)
    ctx.check(T.lib().trhip_upscale(ctx._h, T._ffi.fptr(lo), T._ffi.fptr(lp), lw, lh, T._ffi.fptr(hp), w, h, C.byref(p), T._ffi.fptr(out2), None, None))
    assert_bits_equal(out2, ref, "out_mask NULL")
    # device entry point, with and without a mask
    d_lo, d_lp, d_hp = (T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in (lo, lp, hp))
    d_out, d_mask = T._ffi.DeviceBuffer(ref.nbytes).zero(), T._ffi.DeviceBuffer(ref_mask.nbytes).zero()
    u.upscale_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, w, h, m, d_out.ptr, d_mask.ptr, ctx)
    assert_bits_equal(d_out.to_host(np.float32, ref.shape), ref, "device")
    assert_bits_equal(d_mask.to_host(np.uint8, ref_mask.shape), ref_mask, "device mask")
    d_out.zero()
    u.upscale_device(d_lo.ptr, d_lp.ptr, lw, lh, d_hp.ptr, w, h, m, d_out.ptr, None, ctx)
    assert_bits_equal(d_out.to_host(np.float32, ref.shape), ref, "device, no mask")
    assert_bits_equal(d_lo.to_host(np.float32, lo.shape), lo, "the inputs are left alone")
    for b in (d_lo, d_lp, d_hp, d_out, d_mask):
        b.free()
    assert_bits_equal(out[..., 3], hp[..., 0, 3], "the .w lane is plane 0's weight")


def test_model_takes_every_branch_on_the_pair_the_kernels_are_given():
    lo, lp, hp, m = pair("37x29<-19x15")
    tally = {}
    um.upscale(lo, lp, hp, um.Params(m), tally)
    assert all(tally[k] > 0 for k in um.TALLY_KEYS), tally


def test_overlaps_and_device_side_refusals(T, ctx):
    lo, lp, hp, m = pair("37x29<-19x15")
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    u, L = T.Upscaler(), T.lib()
    p = u._params_for(m)
    out, mask = np.zeros((h, w, 4), F), np.zeros((h, w), np.uint8)
    fp, bp = T._ffi.fptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))  # noqa: E731

    def call(lo_=lo, lp_=lp, hp_=hp, out_=fp(out), mask_=bp(mask), w_=w, h_=h, lw_=lw, lh_=lh, ctx_=ctx._h):
        return L.trhip_upscale(ctx_, fp(lo_) if lo_ is not None else None, fp(lp_) if lp_ is not None else None, lw_, lh_, fp(hp_) if hp_ is not None else None, w_, h_, C.byref(p),
                               out_, mask_, None)
    assert call() == 0
    for kw in (dict(lo_=None), dict(lp_=None), dict(hp_=None), dict(out_=None)):
        assert call(**kw) == INVALID and b"null argument" in L.trhip_last_error(ctx._h), kw
    for kw in (dict(w_=0), dict(h_=0), dict(lw_=0), dict(lh_=0)):
        assert call(**kw) == INVALID and b"empty" in L.trhip_last_error(ctx._h), kw
    # out_xyzw over each input; out_mask over each input and over out_xyzw
    as_f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    big = np.zeros(h * w * 16 + 64, F)  # the planes and, behind them, room for a whole film: views of it stand for overlapping and for adjacent buffers
    big_hp = big[:hp.size].reshape(hp.shape)
    big_hp[...] = hp
    assert call(hp_=big_hp, out_=as_f(big[8:])) == INVALID and b"out_xyzw overlaps" in L.trhip_last_error(ctx._h)
    assert call(hp_=big_hp, out_=as_f(big[hp.size - 4:])) == INVALID and b"out_xyzw overlaps" in L.trhip_last_error(ctx._h), "the last pixel"
    assert call(hp_=big_hp, out_=as_f(big[hp.size:])) == 0, "adjacent is not overlapping"
    assert call(out_=fp(lo)) == INVALID and b"out_xyzw overlaps" in L.trhip_last_error(ctx._h)
    assert call(out_=fp(lp)) == INVALID and b"out_xyzw overlaps" in L.trhip_last_error(ctx._h)
    lo2, lp2, hp2, _ = pair("37x29<-19x15")
    assert call(lo_=lo2, mask_=bp(lo2)) == INVALID and b"out_mask overlaps an input" in L.trhip_last_error(ctx._h)
    assert call(lp_=lp2, mask_=bp(lp2)) == INVALID and b"out_mask overlaps an input" in L.trhip_last_error(ctx._h)
    assert call(hp_=hp2, mask_=bp(hp2)) == INVALID and b"out_mask overlaps an input" in L.trhip_last_error(ctx._h)
    assert call(mask_=bp(out)) == INVALID and b"out_mask overlaps out_xyzw" in L.trhip_last_error(ctx._h)
    assert call(ctx_=None) == INVALID
    with pytest.raises(T.TraceHipError):
        u.upscale(lo, lp[:-1], hp, m, ctx)
    with pytest.raises(T.TraceHipError):
        u.upscale(lo, lp, hp, m[:3], ctx)


def camera(T, resolution):
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def frames(T, scene, hi, spp, depth, seed, guide_spp=None):
    """(lo_xyzw, lo_planes, hi_planes, pixel_map) as Upscaler.render draws them at factor 2."""
    lo = T.Upscaler.low_camera(hi, 2)
    lo_xyzw = T.PathIntegrator(lo, T.SeededSampler(spp, seed=seed), depth).render(scene)
    lo_planes = T.AOVIntegrator(lo, T.SeededSampler(spp, seed=seed)).render(scene).planes
    hi_planes = T.AOVIntegrator(hi, T.SeededSampler(guide_spp or spp, seed=seed)).render(scene).planes
    return lo_xyzw, lo_planes, hi_planes, T.Upscaler.pixel_map(hi, lo)


def test_cornell_frame_equals_the_model_by_hand_and_through_render(T, ctx):
    scene, hi = T.scenes.cornell_scene(), camera(T, 64)
    lo_xyzw, lo_planes, hi_planes, m = frames(T, scene, hi, 4, 5, 0xD1CE)
    assert lo_xyzw.shape == (32, 32, 4) and hi_planes.shape == (64, 64, 3, 4)
    for kw in (dict(), dict(radius=1, demodulate=True, coverage=True)):
        u = T.Upscaler(**kw)
        tally = {}
        ref, ref_mask = um.upscale(lo_xyzw, lo_planes, hi_planes, model_params(u, m), tally)
        out, mask = u.upscale(lo_xyzw, lo_planes, hi_planes, m, ctx)
        assert_bits_equal(out, ref, f"cornell by hand {kw}")
        assert_bits_equal(mask, ref_mask, f"cornell mask {kw}")
        assert tally["guided"] > 3000 and (out[..., 3] > 0).all()
        rendered, rmask = u.render(scene, hi, T.SeededSampler(4, seed=0xD1CE), 5, ctx=ctx, want_mask=True)
        assert_bits_equal(rendered, ref, f"Upscaler.render {kw}")
        assert_bits_equal(rmask, ref_mask, f"Upscaler.render mask {kw}")
        assert len(u.render_stats) == 5 and u.render_stats[3] is None and u.render_stats[4].launches_film >= 1
    # the guides at a lower spp, and the denoiser at either end: the same calls by hand
    u, d = T.Upscaler(demodulate=True, coverage=True), T.Denoiser()
    lo_xyzw, lo_planes, hi_planes1, m = frames(T, scene, hi, 4, 5, 0xD1CE, guide_spp=1)
    low = u.render(scene, hi, T.SeededSampler(4, seed=0xD1CE), 5, guide_spp=1, denoiser=d, denoise_at="low", ctx=ctx)
    assert_bits_equal(low, u.upscale(d.denoise(lo_xyzw, lo_planes, ctx), lo_planes, hi_planes1, m, ctx)[0], "denoise_at = low")
    high = u.render(scene, hi, T.SeededSampler(4, seed=0xD1CE), 5, guide_spp=1, denoiser=d, ctx=ctx)  # denoise_at defaults to "high"
    assert_bits_equal(high, d.denoise(u.upscale(lo_xyzw, lo_planes, hi_planes1, m, ctx)[0], hi_planes1, ctx), "denoise_at = high")
    none = u.render(scene, hi, T.SeededSampler(4, seed=0xD1CE), 5, guide_spp=1, denoiser=d, denoise_at=None, ctx=ctx)
    assert_bits_equal(none, u.upscale(lo_xyzw, lo_planes, hi_planes1, m, ctx)[0], "denoise_at = None")
    with pytest.raises(T.TraceHipError):
        u.render(scene, hi, T.SeededSampler(4, seed=0xD1CE), 5, denoise_at="both", ctx=ctx)


def test_default_session_is_todays_session_and_the_upscaled_one_is_its_calls(T, ctx):
    """PreviewSession(upscaler=None), two frames, against the call sequence the session has always made: path film and planes at sample_offset k * spp, the temporal pass
    against the previous history and camera, the filter on the accumulated film (on the frame's own bits without history).  Then the upscaled session against its calls."""
    scene, spp, depth, seed = T.scenes.cornell_scene(), 2, 3, 0xBEEF
    cams = [camera(T, 48), camera(T, 48)]
    session = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth)
    d, t = T.Denoiser(), T.TemporalAccumulator()

    def by_hand(cameras):
        outs, history, prev = [], None, None
        for k, cam in enumerate(cameras):
            smp = T.SeededSampler(spp, seed=seed, sample_offset=k * spp)
            xyzw = T.PathIntegrator(cam, smp, depth).render(scene, ctx)
            planes = T.AOVIntegrator(cam, smp).render(scene, ctx).planes
            acc, history_next = t.accumulate(xyzw, planes, history, prev, ctx)
            outs.append((d.denoise(acc if history is not None else xyzw, planes, ctx), planes))
            history, prev = history_next, cam
        return outs
    want = by_hand(cams)
    for k, cam in enumerate(cams):
        assert_bits_equal(session.render(cam, ctx), want[k][0], f"default session, frame {k}")
        assert len(session.render_stats) == 4
    session.close()
    hi_cams = [camera(T, 96), camera(T, 96)]
    u = T.Upscaler()
    up = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, upscaler=u, factor=2, guide_spp=1)
    low = by_hand([T.Upscaler.low_camera(c, 2) for c in hi_cams])
    for k, cam in enumerate(hi_cams):
        assert low[k][0].shape == want[k][0].shape == (48, 48, 4)
        assert_bits_equal(low[k][0], want[k][0], "the low session of a 96^2 camera is the 48^2 session")
        hi_planes = T.AOVIntegrator(cam, T.SeededSampler(1, seed=seed, sample_offset=k * spp)).render(scene, ctx).planes
        ref = u.upscale(low[k][0], low[k][1], hi_planes, T.Upscaler.pixel_map(cam, T.Upscaler.low_camera(cam, 2)), ctx)[0]
        got = up.render(cam, ctx)
        assert got.shape == (96, 96, 4)
        assert_bits_equal(got, ref, f"upscaled session, frame {k}")
        assert len(up.render_stats) == 6
    up.close()


QUALITY = dict(resolution=64, spp=4, depth=5, seed=0xBEEF)
QUALITY_SCENES = {"cornell": lambda T: T.scenes.cornell_scene(), "mesh16": lambda T: T.scenes.mesh_scene(16)}
QUALITY_MEASURED = {"cornell": 0.6881, "mesh16": 0.6920}  # mse(Upscaler().render) / mse(the same low film upscaled bilinearly)


@pytest.mark.parametrize("which", sorted(QUALITY_SCENES))
def test_guided_upscaling_beats_bilinear_upscaling_of_the_same_low_film(T, ctx, which):
    """64^2 <- 32^2, 4 spp, depth 5.  MSE of xyz / w against the 64^2 1024 spp frame over all pixels of positive weight: the shipped Upscaler.render over the same low film
    upscaled unguided (H5 on every pixel, computed by the model).  The frames are bit-reproducible, so the ratio is a number; the assertion is the midpoint rule of
    tests/test_gpu_temporal.py."""
    q = QUALITY
    scene, hi = QUALITY_SCENES[which](T), camera(T, q["resolution"])
    target = T.PathIntegrator(hi, T.SeededSampler(1024, seed=0x7A26E7), q["depth"]).render(scene)
    u = T.Upscaler()
    shipped, mask = u.render(scene, hi, T.SeededSampler(q["spp"], seed=q["seed"]), q["depth"], ctx=ctx, want_mask=True)
    lo_xyzw, lo_planes, hi_planes, m = frames(T, scene, hi, q["spp"], q["depth"], q["seed"])
    bilinear, _ = um.upscale(lo_xyzw, lo_planes, hi_planes, model_params(u, m), unguided_only=True)
    weighted = (shipped[..., 3] > 0) & (target[..., 3] > 0)
    assert weighted.sum() >= 3000

    def mse(a):
        diff = a[weighted][:, :3].astype(np.float64) / a[weighted][:, 3:4] - target[weighted][:, :3].astype(np.float64) / target[weighted][:, 3:4]
        return float(np.mean(diff * diff))
    guided, plain = mse(shipped), mse(bilinear)
    ratio = guided / plain
    surface = np.isin(mask, (1, 3))
    print(f"upscale quality {which}: mse guided {guided:.6g}, bilinear {plain:.6g}, ratio {ratio:.4f}; orphans {int((mask == 3).sum())} of {int(surface.sum())} surface pixels")
    assert ratio < 0.5 * (QUALITY_MEASURED[which] + 1.0)
