"""The edge-avoiding denoiser (trhip_denoise, Denoiser) on the GPU: every output value against the numpy model of tests/denoise_model.py bit for bit — on synthetic inputs
that exercise each weight's zero and its interior, and on a real Cornell frame —, determinism, host == device, aliasing, a cropped film, the quality condition against a
1024 spp frame, the refusals and Denoiser.render.

Quality ratios measured on an MI355X with the default parameters (MSE of xyz / w to the 1024 spp frame over surface pixels, denoised / 4 spp; profiles/r9/denoise.txt):
Cornell 0.568, mesh_scene(16) 0.431."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm

pytestmark = pytest.mark.gpu

SIGMAS = dict(sigma_colour=0.6, sigma_normal=0.02, sigma_plane=0.1)  # on dm.synthetic: each weight is 0 for some pairs and inside (0, 1) for others (asserted below)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def model_params(d):
    p = d.params
    return dm.Params(p.sigma_colour, p.sigma_normal, p.sigma_plane, iterations=p.iterations, demodulate=bool(p.flags & 1), albedo_floor=p.albedo_floor, min_coverage=p.min_coverage)


def camera(T, resolution, crop=None):
    film = T.Film([resolution, resolution], T.Bounds2(*(crop or ([0.0, 0.0], [1.0, 1.0]))), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def frame(T, scene, cam, spp, depth, seed):
    """(xyzw, planes) of a path frame and its feature planes with the same sampler settings."""
    xyzw = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed), depth).render(scene)
    planes = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed)).render(scene).planes
    return xyzw, planes


SYNTHETIC = {}


def synthetic(h, w):
    if (h, w) not in SYNTHETIC:
        SYNTHETIC[(h, w)] = dm.synthetic(h, w, 1000 + h)
    B, P, poisoned = SYNTHETIC[(h, w)]
    return B.copy(), P.copy(), poisoned


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("iterations", [1, 3, 6])
@pytest.mark.parametrize("size", [(37, 29), (64, 64)], ids=["37x29", "64x64"])
def test_synthetic_frames_equal_the_model(T, ctx, size, iterations, demodulate):
    """At 6 iterations the last step, 32 pixels, exceeds the smaller image.  Both à-trous kernels (gathered from memory, staged in LDS) must give the model's bits."""
    w, h = size
    B, P, poisoned = synthetic(h, w)
    d = T.Denoiser(iterations=iterations, demodulate=demodulate, **SIGMAS)
    tally = {}
    ref = dm.denoise(B, P, model_params(d), tally)
    for name in ("normal", "plane", "colour"):
        assert tally[name][0] > 50 and tally[name][1] > 50, (name, tally[name])
    surface = dm.surface_mask(B, P, model_params(d))
    assert not any(surface[y, x] for y, x in poisoned) and (~surface).sum() > 30
    try:
        for mask in (0, 3):
            ctx.set_option("denoise_lds", mask)
            out = d.denoise(B, P, ctx)
            assert_bits_equal(out, ref, f"denoise_lds = {mask}")
            assert d.stats.launches_film == iterations + 2
    finally:
        ctx.set_option("denoise_lds", 3)
    assert_bits_equal(out[~surface], B[~surface], "non-surface pixels")


@pytest.fixture(scope="module")
def cornell_frame(T, ctx):
    scene, cam = T.scenes.cornell_scene(), camera(T, 48)
    return frame(T, scene, cam, 4, 3, 0xD1CE)


def test_cornell_frame_equals_the_model(T, ctx, cornell_frame):
    xyzw, planes = cornell_frame
    d = T.Denoiser()
    out = d.denoise(xyzw, planes, ctx)
    assert_bits_equal(out, dm.denoise(xyzw, planes, model_params(d)), "cornell 48^2")
    assert (bits(out) != bits(xyzw)).mean() > 0.3, "the filter must act"
    assert_bits_equal(d.denoise(xyzw, planes, ctx), out, "second call")


def test_host_device_and_aliased_calls_agree(T, ctx, cornell_frame):
    xyzw, planes = cornell_frame
    h, w = xyzw.shape[:2]
    d = T.Denoiser()
    out = d.denoise(xyzw, planes, ctx)
    d_in, d_pl, d_out = (T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in (xyzw, planes, np.zeros_like(xyzw)))
    d.denoise_device(d_in.ptr, d_pl.ptr, w, h, d_out.ptr, ctx)
    assert_bits_equal(d_out.to_host(np.float32, xyzw.shape), out, "device variant")
    assert_bits_equal(d_in.to_host(np.float32, xyzw.shape), xyzw, "the input is left alone")
    d.denoise_device(d_in.ptr, d_pl.ptr, w, h, d_in.ptr, ctx)
    assert_bits_equal(d_in.to_host(np.float32, xyzw.shape), out, "out aliasing xyzw, device")
    buf = xyzw.copy()
    rc = T.lib().trhip_denoise(ctx._h, T._ffi.fptr(buf), T._ffi.fptr(planes), w, h, C.byref(d.params), T._ffi.fptr(buf), None)
    assert rc == 0
    assert_bits_equal(buf, out, "out aliasing xyzw, host")


def test_cropped_film_equals_the_model(T, ctx):
    scene, cam = T.scenes.cornell_scene(), camera(T, 48, crop=([0.2, 0.1], [0.9, 0.7]))
    xyzw, planes = frame(T, scene, cam, 4, 3, 0xD1CE)
    h, w = cam.film.size
    assert xyzw.shape == (h, w, 4) and h != w and h < 48 and w < 48
    d = T.Denoiser()
    assert_bits_equal(d.denoise(xyzw, planes, ctx), dm.denoise(xyzw, planes, model_params(d)), "cropped film")


QUALITY_SCENES = {"cornell": lambda T: T.scenes.cornell_scene(), "mesh16": lambda T: T.scenes.mesh_scene(16)}


@pytest.mark.parametrize("which", sorted(QUALITY_SCENES))
def test_default_parameters_bring_a_4spp_frame_closer_to_the_1024spp_frame(T, ctx, which):
    """A condition, not a tuned number: with the default parameters the denoised frame is strictly closer (MSE of xyz / w over surface pixels) to the 1024 spp frame."""
    scene, cam = QUALITY_SCENES[which](T), camera(T, 64)
    noisy, planes = frame(T, scene, cam, 4, 5, 0xBEEF)
    target = T.PathIntegrator(cam, T.SeededSampler(1024, seed=0x7A26E7), 5).render(scene)
    d = T.Denoiser()
    out = d.denoise(noisy, planes, ctx)
    surface = dm.surface_mask(noisy, planes, model_params(d))
    assert (~surface).sum() >= 100 and surface.sum() >= 1000
    assert_bits_equal(out[~surface], noisy[~surface], "non-surface pixels")

    def mse(a):
        with np.errstate(all="ignore"):
            diff = a[surface][:, :3].astype(np.float64) / a[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
        return float(np.mean(diff * diff))
    before, after = mse(noisy), mse(out)
    print(f"denoise quality {which}: mse 4 spp {before:.6g}, denoised {after:.6g}, ratio {after / before:.4f}")
    assert after < before


def test_refusals(T, ctx):
    B, P, _ = synthetic(29, 37)
    L = T.lib()
    out = np.empty_like(B)

    def call(p, xyzw=B, planes=P, w=37, h=29, o=out):
        ptr = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731
        return L.trhip_denoise(ctx._h, ptr(xyzw), ptr(planes), w, h, C.byref(p) if p is not None else None, ptr(o), None)

    def params(**kw):
        p = T.Denoiser(**SIGMAS).params
        q = T._ffi.DenoiseParams.from_buffer_copy(p)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    assert call(params()) == 0
    bad = [dict(iterations=7), dict(reserved=1), dict(min_coverage=-0.1), dict(min_coverage=1.5), dict(min_coverage=float("nan"))]
    for name in ("sigma_colour", "sigma_normal", "sigma_plane", "albedo_floor"):
        bad += [{name: 0.0}, {name: -1.0}, {name: float("inf")}, {name: float("nan")}]
    for kw in bad:
        assert call(params(**kw)) == -1, kw
        assert L.trhip_last_error(ctx._h).decode(), kw
    for kw in (dict(p=None), dict(p=params(), xyzw=None), dict(p=params(), planes=None), dict(p=params(), o=None), dict(p=params(), w=0), dict(p=params(), h=0)):
        assert call(**kw) == -1, kw
        assert L.trhip_last_error(ctx._h).decode(), kw
    assert L.trhip_denoise(None, T._ffi.fptr(B), T._ffi.fptr(P), 37, 29, C.byref(params()), T._ffi.fptr(out), None) == -1
    with pytest.raises(T.TraceHipError):
        T.Denoiser(iterations=7, **SIGMAS).denoise(B, P, ctx)
    copied = T.Denoiser(iterations=0, **SIGMAS).denoise(B, P, ctx)
    assert_bits_equal(copied, B, "iterations = 0 copies")


def test_render_equals_the_three_calls(T, ctx):
    scene, cam = T.scenes.cornell_scene(), camera(T, 48)
    sampler = T.SeededSampler(4, seed=0xD1CE)
    d = T.Denoiser()
    out = d.render(scene, cam, sampler, 3, ctx)
    xyzw, planes = frame(T, scene, cam, 4, 3, 0xD1CE)
    assert_bits_equal(out, d.denoise(xyzw, planes, ctx), "Denoiser.render")
    assert len(d.render_stats) == 3 and d.render_stats[2].launches_film == d.params.iterations + 2
    cam.film.set_xyzw(out)
