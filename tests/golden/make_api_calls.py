#!/usr/bin/env python
"""Writes tests/golden/api_calls.json: every libtracehip call the Python binding (trace.jl_amd/api.py) makes for the public host and `_device` methods of its integrators and
image-space passes, and the text of what those methods refuse — recorded WITHOUT a GPU, behind a stand-in for `_ffi.lib` that forwards the entries that need no device and
writes every other call down as (entry, normalised arguments).  tests/test_api_calls.py records the same cases again and compares.

THE COMMITTED FILE IS THIS SCRIPT'S OUTPUT AT THE COMMIT BEFORE THE BINDING'S CALL PATHS WERE SHARED ("One call path per kind of library call in the Python binding"): it
was written once, from the api.py that still held one copy of every call per method, and is never regenerated from the code it pins.  A change of the binding that changes
an entry, an argument's order, NULL against a pointer, a byte of a parameter block or a refusal's text fails the test; only a change of the C interface itself is a reason
to write the file again, and then from a commit whose calls were checked on a device.

    python tests/golden/make_api_calls.py

Normalisation: None -> null; Python numbers as they are; c_void_p -> its value, or "c_void_p(array)" when it is the address of a host array; byref(struct) -> [type name, hex of its bytes] (trhip_stats, an output: the name alone);
byref of a plain ctypes value (an output handle) -> "out:" + type name; a typed array pointer -> its pointer type's name.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "api_calls.json")
F = np.float32
H, W = 3, 4            # the film: 4 x 3 pixels
LH, LW = 2, 2          # the low-resolution film of the upscaling passes
FORWARDED = ("trhip_detmath_f32", "trhip_display_srgb_table", "trhip_sensor_world_to_pixel", "trhip_option_in_build", "trhip_last_error")  # and every *_default_params
CTX_HANDLE, SCENE_HANDLE, ENV_HANDLE, FIRST_BUFFER = 0xC0DE000, 0x5CE7E000, 0xE7700000, 0xB0000000


def normalise(a):
    if a is None or isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, np.integer):
        return int(a)
    if isinstance(a, np.floating):
        return float(a)
    if isinstance(a, C.c_void_p):
        return "c_void_p(array)" if hasattr(a, "_arr") else a.value  # ndarray.ctypes.data_as keeps its array in _arr: a host address, another one in every run
    if type(a).__name__ == "CArgObject":  # byref(x)
        x = a._obj
        if isinstance(x, C.Structure):
            return type(x).__name__ if type(x).__name__ == "Stats" else [type(x).__name__, bytes(x).hex()]
        return "out:" + type(x).__name__
    if isinstance(a, C._Pointer):
        return type(a).__name__
    raise TypeError(f"an argument the record has no form for: {a!r}")


class StubLib:
    """Stands in for the loaded library: the entries that need no device go to the real one, every other call is checked against its prototype, logged, and returns 0."""

    def __init__(self, real, signatures, log):
        self._real, self._signatures, self._log = real, signatures, log

    def __getattr__(self, name):
        if name.endswith("_default_params") or name in FORWARDED:
            return getattr(self._real, name)
        _, argtypes = self._signatures[name]  # a KeyError: an entry include/tracehip.h does not declare

        def call(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)}"
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError(f"{name}: argument {k} ({a!r}) is no {t.__name__}: {e}")
            if name == "trhip_env_create":
                args[-1]._obj.value = ENV_HANDLE
            self._log.append([name] + [normalise(a) for a in args])
            return 0
        return call


class FakeContext:
    def __init__(self):
        self._h = C.c_void_p(CTX_HANDLE)

    def check(self, rc):
        assert rc == 0, rc


class FakeFlat:
    top_counts = [1, 1]

    def __init__(self, ctx):
        self.ctx, self._h = ctx, C.c_void_p(SCENE_HANDLE)


class FakeScene:
    lights = ()

    def __init__(self, ctx):
        self._flat = FakeFlat(ctx)

    def flatten(self, ctx=None):
        return self._flat


def fake_buffers():
    """A DeviceBuffer class whose addresses count up from FIRST_BUFFER in the order of allocation; nothing is allocated, to_host gives zeros."""
    made = []

    class Buffer:
        def __init__(self, nbytes):
            self.nbytes, self.ptr = int(nbytes), FIRST_BUFFER + 0x1000 * len(made)
            made.append(self)

        def from_host(self, a):
            assert np.ascontiguousarray(a).nbytes == self.nbytes
            return self

        def zero(self):
            return self

        def to_host(self, dtype, shape):
            out = np.zeros(shape, dtype=dtype)
            assert out.nbytes == self.nbytes
            return out

        def free(self):
            self.ptr = None
    return Buffer


def camera(T, width=W, height=H):
    film = T.Film([width, height], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0.0, 0.0, 5.0], [0.0, 0.0, 0.0], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 60.0, film)


def environment(T):
    return T.Environment(np.full((2, 2, 3), 0.5, F), np.eye(3, dtype=F))


# ---- the cases: name -> function(T, ctx, scene); everything it makes the library do is the case's record ------------------------------------------------------------------
def case_whitted(T, ctx, scene):
    integ = T.WhittedIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4)
    out = integ.render(scene, ctx)
    assert out.shape == (H, W, 4) and integ.stats is not None
    assert integ.render(scene, ctx, device_out=0x1000) is None
    assert integ.sample_radiance(scene).shape == (2, 5, 6, 3)
    integ(scene)


def case_path(T, ctx, scene):
    integ = T.PathIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4)
    assert integ.render(scene, ctx).shape == (H, W, 4)
    assert integ.render(scene, ctx, device_out=0x1000) is None
    assert integ.sample_radiance(scene).shape == (2, 5, 6, 3)


def case_path_sample_map(T, ctx, scene):
    integ = T.PathIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4)
    smap = T.SampleMap(np.arange(30).reshape(5, 6) % 4, 3)
    assert integ.render(scene, ctx, sample_map=smap).shape == (H, W, 4)
    assert integ.render(scene, ctx, device_out=0x1000, sample_map=smap) is None


def case_path_environment(T, ctx, scene):
    integ, env = T.PathIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4), environment(T)
    assert integ.render(scene, ctx, environment=env).shape == (H, W, 4)
    assert integ.render(scene, ctx, environment=env, env_scale=0.5, hide_background=True).shape == (H, W, 4)
    assert integ.render(scene, ctx, device_out=0x1000, environment=env, env_scale=0.5) is None
    beta, depth, dirs = integ.escapes(scene)
    assert beta.shape == (2, 5, 6, 3) and depth.shape == (2, 5, 6) and dirs.shape == (2, 5, 6, 3)
    assert integ.relight(scene, env, env_scale=2.0, hide_background=True).shape == (H, W, 4)
    assert integ.relight(scene, env, device_out=0x2000) is None
    env.close()


def case_ambient_occlusion(T, ctx, scene):
    integ = T.AmbientOcclusionIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), max_distance=2.0, albedo=True, background=0.25)
    assert integ.render(scene, ctx).shape == (H, W, 4)
    assert integ.render(scene, ctx, device_out=0x1000) is None
    plain = T.AmbientOcclusionIntegrator(camera(T), T.SeededSampler(1))
    assert plain.render(scene, ctx).shape == (H, W, 4)


def case_sky(T, ctx, scene):
    env = environment(T)
    integ = T.SkyIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), env, max_distance=3.0, albedo=True, scale=2.0, hide_background=True)
    assert integ.render(scene, ctx).shape == (H, W, 4)
    assert integ.render(scene, ctx, device_out=0x1000) is None
    env.close()


def case_sky_importance(T, ctx, scene):
    env = environment(T)
    for importance in (True, 0.25):
        integ = T.SkyIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), env, max_distance=3.0, scale=2.0, hide_background=True, importance=importance)
        assert integ.render(scene, ctx).shape == (H, W, 4)
        assert integ.render(scene, ctx, device_out=0x1000) is None
    env.close()


def case_environment(T, ctx, scene):
    env = environment(T)
    assert env.eval(np.zeros((5, 3), F), ctx).shape == (5, 3)
    assert env.sample(np.zeros((5, 2), F), ctx).shape == (5, 3)
    assert env.pdf(np.zeros((7, 3), F), ctx).shape == (7,)
    env.close()


def case_aov(T, ctx, scene):
    integ = T.AOVIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3))
    assert integ.render(scene, ctx).planes.shape == (H, W, 3, 4)
    assert integ.render(scene, ctx, device_out=0x1000) is None
    assert integ.render(scene, ctx, device_out=0x1000, device_ids=0x2000) is None
    assert integ.ids(scene, ctx).shape == (H, W)
    assert integ.samples(scene, ctx).shape == (2, 5, 6)
    assert integ._sample_shape() == (5, 6)


def case_adaptive(T, ctx, scene):
    integ = T.AdaptivePathIntegrator(camera(T), T.SeededSampler(2, seed=7, sample_offset=3), 4, tau=0.5, max_extra=6, eps=0.01)
    assert integ.render(scene, ctx).shape == (H, W, 4) and integ.total == 0


def case_denoiser(T, ctx, scene):
    d = T.Denoiser(iterations=2, demodulate=False, sigma_colour=0.5, sigma_normal=0.2, sigma_plane=0.3, albedo_floor=0.01, min_coverage=0.4, variance_sigma=1.5, var_eps=1e-3)
    film, planes, var = np.zeros((H, W, 4), F), np.zeros((H, W, 3, 4), F), np.zeros((H, W), F)
    assert d.denoise(film, planes, ctx).shape == (H, W, 4)
    d.denoise_device(0x1000, 0x2000, W, H, 0x3000, ctx)
    out, out_var = d.denoise_variance(film, planes, var, ctx)
    assert out.shape == (H, W, 4) and out_var.shape == (H, W)
    d.denoise_variance_device(0x1000, 0x2000, 0x3000, W, H, 0x4000, None, ctx)
    d.denoise_variance_device(0x1000, 0x2000, 0x3000, W, H, 0x4000, 0x5000, ctx)
    default = T.Denoiser()
    assert default.denoise(film, planes, ctx).shape == (H, W, 4)
    default.denoise_variance(film, planes, var, ctx)


def case_denoiser_render(T, ctx, scene):
    d, smp = T.Denoiser(), T.SeededSampler(2, seed=7, sample_offset=3)
    assert d.render(scene, camera(T), smp, 4, ctx).shape == (H, W, 4) and len(d.render_stats) == 3
    assert d.render(scene, camera(T), smp, 4, ctx, variance_guided=True).shape == (H, W, 4) and len(d.render_stats) == 4


def case_upscaler(T, ctx, scene):
    u = T.Upscaler(radius=1, demodulate=False, coverage=True, sigma_normal=0.2, sigma_plane=0.3, albedo_floor=0.01, min_coverage=0.4)
    lo, lo_planes, hi_planes = np.zeros((LH, LW, 4), F), np.zeros((LH, LW, 3, 4), F), np.zeros((H, W, 3, 4), F)
    pixel_map = (0.5, -0.25, 0.5, 0.25)
    out, mask = u.upscale(lo, lo_planes, hi_planes, pixel_map, ctx)
    assert out.shape == (H, W, 4) and mask.shape == (H, W) and mask.dtype == np.uint8
    u.upscale_device(0x1000, 0x2000, LW, LH, 0x3000, W, H, pixel_map, 0x4000, None, ctx)
    u.upscale_device(0x1000, 0x2000, LW, LH, 0x3000, W, H, pixel_map, 0x4000, 0x5000, ctx)
    T.Upscaler().upscale(lo, lo_planes, hi_planes, pixel_map, ctx)


def case_upscaler_render(T, ctx, scene):
    u, smp = T.Upscaler(), T.SeededSampler(2, seed=7, sample_offset=3)
    assert u.render(scene, camera(T, 8, 6), smp, 4, factor=2, ctx=ctx).shape == (6, 8, 4)
    out, mask = u.render(scene, camera(T, 8, 6), smp, 4, factor=2, guide_spp=1, denoiser=T.Denoiser(), denoise_at="low", ctx=ctx, want_mask=True)
    assert out.shape == (6, 8, 4) and mask.shape == (6, 8)
    u.render(scene, camera(T, 8, 6), smp, 4, factor=2, denoiser=T.Denoiser(), ctx=ctx)


def case_display(T, ctx, scene):
    d = T.Display(curve="aces", transfer="srgb", auto_exposure=True, flip_rows=False, exposure=1.5, key=0.2, percentile=0.9, adapt_rate=0.5, min_exposure=0.1, max_exposure=8.0, white=4.0)
    film = np.zeros((H, W, 4), F)
    assert d.encode(film, ctx=ctx).shape == (H, W, 4)
    state = T._ffi.DisplayState()
    state.exposure, state.valid = 1.25, 1
    rgba, new_state = d.encode(film, 2.0, state, ctx)
    assert rgba.dtype == np.uint8 and new_state is not state
    rgba, none, hist = d.encode(film, 2.0, None, ctx, want_histogram=True)
    assert none is None and hist.shape == (256,)
    d.encode(film, 2.0, state, ctx, want_histogram=True)
    d.encode_device(0x1000, W, H, 2.0, 0x2000, None, None, ctx)
    d.encode_device(0x1000, W, H, 2.0, 0x2000, 0x3000, 0x4000, ctx)
    T.Display.reference().encode(film, ctx=ctx)
    assert T.Display.srgb_table().shape == (256,)


def temporal_inputs(T):
    film, planes, history = np.zeros((H, W, 4), F), np.zeros((H, W, 3, 4), F), np.zeros((H, W, 3, 4), F)
    ids, table, bodies = np.zeros((H, W), T._ffi.AOV_ID_DTYPE), np.zeros(5, np.uint32), np.zeros((2, 3, 4), F)
    return film, planes, history, ids, table, bodies


def drive_accumulate(T, t, ctx):
    """accumulate / accumulate_device with every nullable input once None and once given: the history, the previous camera as a camera and as a matrix."""
    film, planes, history, _, _, _ = temporal_inputs(T)
    cam = camera(T)
    for hist, prev in ((None, None), (history, cam), (history, cam.world_to_pixel())):
        out, out_history = t.accumulate(film, planes, hist, prev, ctx)
        assert out.shape == (H, W, 4) and out_history.shape == (H, W, 3, 4) and t.stats is not None
    t.accumulate_device(0x1000, 0x2000, None, W, H, None, 0x3000, 0x4000, ctx)
    t.accumulate_device(0x1000, 0x2000, 0x5000, W, H, cam, 0x3000, 0x4000, ctx)


def drive_accumulate_motion(T, t, ctx):
    film, planes, history, ids, table, bodies = temporal_inputs(T)
    cam = camera(T)
    for hist, tb, mt, prev in ((None, None, None, None), (history, table, bodies, cam), (history, table, None, cam), (None, None, bodies, None)):
        out, out_history = t.accumulate_motion(film, planes, hist, ids, tb, mt, prev, ctx)
        assert out.shape == (H, W, 4) and out_history.shape == (H, W, 3, 4)
    t.accumulate_motion_device(0x1000, 0x2000, None, 0x6000, None, 0, None, 0, W, H, None, 0x3000, 0x4000, ctx)
    t.accumulate_motion_device(0x1000, 0x2000, 0x5000, 0x6000, 0x7000, 5, 0x8000, 2, W, H, cam, 0x3000, 0x4000, ctx)
    t.accumulate_motion_device(0x1000, 0x2000, 0x5000, 0x6000, None, 5, 0x8000, 2, W, H, cam, 0x3000, 0x4000, ctx)
    t.accumulate_motion_device(0x1000, 0x2000, 0x5000, None, 0x7000, 5, 0x8000, 2, W, H, cam, 0x3000, 0x4000, ctx)


def case_temporal_plain(T, ctx, scene):
    t = T.TemporalAccumulator(max_history=4, sigma_normal=0.2, sigma_plane=0.3, min_coverage=0.4)
    drive_accumulate(T, t, ctx)
    drive_accumulate(T, T.TemporalAccumulator(), ctx)


def case_temporal_plain_motion(T, ctx, scene):
    drive_accumulate_motion(T, T.TemporalAccumulator(max_history=4, sigma_normal=0.2), ctx)


def case_temporal_plain_split(T, ctx, scene):
    t = T.TemporalAccumulator(max_history=4, sigma_normal=0.2)
    film, planes, history, ids, table, bodies = temporal_inputs(T)
    direct, cam = np.zeros((H, W, 4), F), camera(T)
    for d, hist, idp, tb, mt, prev in ((None, None, None, None, None, None), (direct, history, ids, table, bodies, cam), (direct, None, None, table, bodies, cam),
                                       (None, history, ids, None, bodies, None), (direct, history, ids, table, None, cam)):
        out, out_history = t.accumulate_split(film, d, planes, hist, idp, tb, mt, prev, ctx)
        assert out.shape == (H, W, 4) and out_history.shape == (H, W, 3, 4)
    t.accumulate_split_device(0x1000, None, 0x2000, None, None, None, 0, None, 0, W, H, None, 0x3000, 0x4000, ctx)
    t.accumulate_split_device(0x1000, 0x9000, 0x2000, 0x5000, 0x6000, 0x7000, 5, 0x8000, 2, W, H, cam, 0x3000, 0x4000, ctx)
    t.accumulate_split_device(0x1000, 0x9000, 0x2000, 0x5000, None, 0x7000, 5, 0x8000, 2, W, H, cam, 0x3000, 0x4000, ctx)
    t.accumulate_split_device(0x1000, None, 0x2000, None, 0x6000, None, 5, 0x8000, 2, W, H, cam, 0x3000, 0x4000, ctx)


def case_temporal_clip(T, ctx, scene):
    drive_accumulate(T, T.TemporalAccumulator(max_history=4, clip_gamma=1.5, clip_radius=2), ctx)
    drive_accumulate(T, T.TemporalAccumulator(clip_radius=1), ctx)


def case_temporal_moments(T, ctx, scene):
    t = T.TemporalAccumulator(max_history=4, moments=True, spatial_below=3.0, demodulate=False, albedo_floor=0.02)
    film, planes, history, _, _, _ = temporal_inputs(T)
    moments, cam = np.zeros((H, W, 2), F), camera(T)
    for hist, mom, prev in ((None, None, None), (history, moments, cam)):
        out, out_history, out_moments, var = t.accumulate_moments(film, planes, hist, mom, prev, ctx)
        assert out.shape == (H, W, 4) and out_history.shape == (H, W, 3, 4) and out_moments.shape == (H, W, 2) and var.shape == (H, W)
    t.accumulate_moments_device(0x1000, 0x2000, None, None, W, H, None, 0x3000, 0x4000, 0x5000, 0x6000, ctx)
    t.accumulate_moments_device(0x1000, 0x2000, 0x7000, 0x8000, W, H, cam, 0x3000, 0x4000, 0x5000, 0x6000, ctx)
    drive_accumulate(T, t, ctx)  # a moments accumulator's plain calls go through trhip_temporal
    T.TemporalAccumulator(moments=True).accumulate_moments(film, planes, None, None, None, ctx)


def case_temporal_clip_carry_bodies(T, ctx, scene):
    t = T.TemporalAccumulator(max_history=4, clip_gamma=1.5, clip_radius=2, carry_bodies=True, clip_max_history=2.0)
    drive_accumulate(T, t, ctx)
    drive_accumulate_motion(T, t, ctx)
    film, planes, history, ids, table, bodies = temporal_inputs(T)
    t.accumulate_motion(film, planes, history, None, table, bodies, camera(T), ctx)  # no id plane: the tables are dropped
    drive_accumulate(T, T.TemporalAccumulator(clip_gamma=2.0, carry_bodies=True), ctx)


def upsample_inputs(T):
    lo, lo_planes, hi_planes, history = np.zeros((LH, LW, 4), F), np.zeros((LH, LW, 3, 4), F), np.zeros((H, W, 3, 4), F), np.zeros((H, W, 3, 4), F)
    ids, table, bodies = np.zeros((H, W), T._ffi.AOV_ID_DTYPE), np.zeros(5, np.uint32), np.zeros((2, 3, 4), F)
    return lo, lo_planes, hi_planes, history, ids, table, bodies


PIXEL_MAP = (0.5, -0.25, 0.5, 0.25)


def drive_upsample(T, u, ctx):
    lo, lo_planes, hi_planes, history, _, _, _ = upsample_inputs(T)
    cam = camera(T)
    for hist, prev in ((None, None), (history, cam), (history, cam.world_to_pixel())):
        out, out_history, mask = u.accumulate(lo, lo_planes, hi_planes, hist, PIXEL_MAP, prev, ctx)
        assert out.shape == (H, W, 4) and out_history.shape == (H, W, 3, 4) and mask.shape == (H, W) and mask.dtype == np.uint8
    u.accumulate_device(0x1000, 0x2000, LW, LH, 0x3000, None, W, H, PIXEL_MAP, None, 0x4000, 0x5000, None, ctx)
    u.accumulate_device(0x1000, 0x2000, LW, LH, 0x3000, 0x6000, W, H, PIXEL_MAP, cam, 0x4000, 0x5000, 0x7000, ctx)


def case_temporal_upsampler(T, ctx, scene):
    u = T.TemporalUpsampler(radius=1, max_history=4, sigma_normal=0.2, sigma_plane=0.3, guide_sigma_normal=0.25, guide_sigma_plane=0.35, confidence_floor=0.05,
                            confidence_sharpness=2.0, min_coverage=0.4, jitter="halton")
    drive_upsample(T, u, ctx)
    drive_upsample(T, T.TemporalUpsampler(), ctx)


def case_temporal_upsampler_carry_bodies(T, ctx, scene):
    u = T.TemporalUpsampler(radius=1, max_history=4, carry_bodies=True)
    drive_upsample(T, u, ctx)
    lo, lo_planes, hi_planes, history, ids, table, bodies = upsample_inputs(T)
    cam = camera(T)
    for hist, idp, tb, mt, prev in ((None, None, None, None, None), (history, ids, table, bodies, cam), (history, None, table, bodies, cam), (None, ids, None, bodies, None),
                                    (history, ids, table, None, cam)):
        out, out_history, mask = u.accumulate_motion(lo, lo_planes, hi_planes, hist, idp, tb, mt, PIXEL_MAP, prev, ctx)
        assert out.shape == (H, W, 4) and out_history.shape == (H, W, 3, 4) and mask.shape == (H, W)
    u.accumulate_motion_device(0x1000, 0x2000, LW, LH, 0x3000, None, None, None, 0, None, 0, W, H, PIXEL_MAP, None, 0x4000, 0x5000, None, ctx)
    u.accumulate_motion_device(0x1000, 0x2000, LW, LH, 0x3000, 0x6000, 0x8000, 0x9000, 5, 0xA000, 2, W, H, PIXEL_MAP, cam, 0x4000, 0x5000, 0x7000, ctx)
    u.accumulate_motion_device(0x1000, 0x2000, LW, LH, 0x3000, 0x6000, None, 0x9000, 5, 0xA000, 2, W, H, PIXEL_MAP, cam, 0x4000, 0x5000, 0x7000, ctx)
    u.accumulate_motion_device(0x1000, 0x2000, LW, LH, 0x3000, 0x6000, 0x8000, None, 5, 0xA000, 2, W, H, PIXEL_MAP, cam, 0x4000, 0x5000, None, ctx)


def case_film_add(T, ctx, scene):
    a, b = np.zeros((H, W, 4), F), np.ones((H, W, 4), F)
    assert T.Film.add(a, b, ctx).shape == (H, W, 4)
    assert isinstance(T.Film.add_device(0x1000, 0x2000, W, H, 0x1000, ctx), T._ffi.Stats)


def case_flat_scene(T, ctx, scene):
    """The scene calls, optional vertex arrays NULL and given: a sphere, a mesh with normals alone, one with tangents and corner uvs, one with nothing, two lights."""
    matte = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.5)), T.ConstantTexture(0.0))
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    verts, idx = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F), np.array([1, 2, 3, 2, 4, 3], np.uint32)
    nrm, tan, uv = np.tile(np.array([0, 0, 1], F), (4, 1)), np.tile(np.array([1, 0, 0], F), (4, 1)), np.zeros((6, 2), F)
    prims = [T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0, 0, 1]), False), 0.5, 360.0), matte), T.create_mesh_primitives(core, idx, verts, nrm, matte),
             T.create_mesh_primitives(core, idx, verts, nrm, matte, tan, uv), T.create_mesh_primitives(core, idx, verts, None, matte, None, uv),
             T.create_mesh_primitives(core, idx, verts, None, None)]
    prims += [T.GeometricPrimitive(t, matte) for t in T.create_triangle_mesh(core, 2, idx, 4, verts, None, tan)]
    lights = [T.PointLight(T.translate([0, 0, 3]), T.RGBSpectrum(2.0)), T.SpotLight(T.translate([0, 0, 3]), T.RGBSpectrum(2.0), 30.0, 20.0)]
    flat = T.FlatScene(T.Scene(lights, T.BVHAccel(prims, 1)), ctx)
    assert flat.n_prims == 7 and flat.top_counts == [1, 2, 2, 2, 2, 1, 1]


CASES = {name[5:]: fn for name, fn in sorted(globals().items()) if name.startswith("case_")}


# ---- the refusals: name -> function(T, ctx, scene) that must raise TraceHipError before anything reaches the library -----------------------------------------------------
def refusals(T, ctx, scene):
    film, planes, history, ids, table, bodies = temporal_inputs(T)
    lo, lo_planes, hi_planes, _, _, _, _ = upsample_inputs(T)
    bad_film, bad_planes, bad_history, bad_ids = np.zeros((H, W, 3), F), np.zeros((H, W + 1, 3, 4), F), np.zeros((H, W, 3, 3), F), np.zeros((H, W - 1), T._ffi.AOV_ID_DTYPE)
    var, moments, cam, smp = np.zeros((H, W), F), np.zeros((H, W, 2), F), camera(T), T.SeededSampler(2, seed=7)
    plain, clip, mom = T.TemporalAccumulator(), T.TemporalAccumulator(clip_gamma=1.5), T.TemporalAccumulator(moments=True)
    carry = T.TemporalAccumulator(clip_gamma=1.5, carry_bodies=True)
    up, up_carry = T.TemporalUpsampler(), T.TemporalUpsampler(carry_bodies=True)
    den, usc, path, env = T.Denoiser(), T.Upscaler(), T.PathIntegrator(cam, smp, 4), environment(T)
    out = {
        "film_add.b": lambda: T.Film.add(film, np.zeros((H, W - 1, 4), F), ctx),
        "film_add.a": lambda: T.Film.add(bad_film, bad_film, ctx),
        "denoise.xyzw": lambda: den.denoise(bad_film, planes, ctx),
        "denoise.planes": lambda: den.denoise(film, bad_planes, ctx),
        "denoise_variance.xyzw": lambda: den.denoise_variance(bad_film, planes, var, ctx),
        "denoise_variance.planes": lambda: den.denoise_variance(film, bad_planes, var, ctx),
        "denoise_variance.variance": lambda: den.denoise_variance(film, planes, np.zeros((H, W, 1), F), ctx),
        "upscale.lo_xyzw": lambda: usc.upscale(np.zeros((LH, LW, 3), F), lo_planes, hi_planes, PIXEL_MAP, ctx),
        "upscale.lo_planes": lambda: usc.upscale(lo, np.zeros((LH, LW + 1, 3, 4), F), hi_planes, PIXEL_MAP, ctx),
        "upscale.hi_planes": lambda: usc.upscale(lo, lo_planes, np.zeros((H, W, 4), F), PIXEL_MAP, ctx),
        "upscale.pixel_map": lambda: usc.upscale(lo, lo_planes, hi_planes, (1.0, 0.0, 1.0), ctx),
        "upscale_device.pixel_map": lambda: usc.upscale_device(1, 2, LW, LH, 3, W, H, (1.0, 0.0, 1.0), 4, None, ctx),
        "display.xyzw": lambda: T.Display().encode(bad_film, ctx=ctx),
        "accumulate.xyzw": lambda: plain.accumulate(bad_film, planes, None, None, ctx),
        "accumulate.planes": lambda: plain.accumulate(film, bad_planes, None, None, ctx),
        "accumulate.history": lambda: plain.accumulate(film, planes, bad_history, None, ctx),
        "accumulate.prev_camera": lambda: plain.accumulate(film, planes, None, np.zeros(11, F), ctx),
        "accumulate_device.prev_camera": lambda: plain.accumulate_device(1, 2, None, W, H, np.zeros(11, F), 3, 4, ctx),
        "accumulate.clip.planes": lambda: clip.accumulate(film, bad_planes, None, None, ctx),
        "accumulate.clip.history": lambda: clip.accumulate(film, planes, bad_history, None, ctx),
        "accumulate.carry.xyzw": lambda: carry.accumulate(bad_film, planes, None, None, ctx),
        "accumulate.carry.planes": lambda: carry.accumulate(film, bad_planes, None, None, ctx),
        "accumulate.carry.history": lambda: carry.accumulate(film, planes, bad_history, None, ctx),
        "accumulate_moments.no_moments_accumulator": lambda: plain.accumulate_moments(bad_film, planes, None, None, None, ctx),
        "accumulate_moments_device.no_moments_accumulator": lambda: clip.accumulate_moments_device(1, 2, None, None, W, H, None, 3, 4, 5, 6, ctx),
        "accumulate_moments.xyzw": lambda: mom.accumulate_moments(bad_film, planes, None, None, None, ctx),
        "accumulate_moments.planes": lambda: mom.accumulate_moments(film, bad_planes, None, None, None, ctx),
        "accumulate_moments.history_without_moments": lambda: mom.accumulate_moments(film, planes, history, None, None, ctx),
        "accumulate_moments.moments_without_history": lambda: mom.accumulate_moments(film, planes, None, moments, None, ctx),
        "accumulate_moments.history": lambda: mom.accumulate_moments(film, planes, bad_history, moments, None, ctx),
        "accumulate_moments.moments": lambda: mom.accumulate_moments(film, planes, history, np.zeros((H, W, 3), F), None, ctx),
        "accumulate_motion.xyzw": lambda: plain.accumulate_motion(bad_film, planes, None, ids, None, None, None, ctx),
        "accumulate_motion.planes": lambda: plain.accumulate_motion(film, bad_planes, None, ids, None, None, None, ctx),
        "accumulate_motion.history": lambda: plain.accumulate_motion(film, planes, bad_history, ids, None, None, None, ctx),
        "accumulate_motion.ids": lambda: plain.accumulate_motion(film, planes, None, bad_ids, None, None, None, ctx),
        "accumulate_motion.ids_none": lambda: plain.accumulate_motion(film, planes, None, None, None, None, None, ctx),
        "accumulate_motion.clip_accumulator": lambda: clip.accumulate_motion(film, planes, None, ids, None, None, None, ctx),
        "accumulate_motion.clip_accumulator.shape_first": lambda: clip.accumulate_motion(film, planes, None, bad_ids, None, None, None, ctx),
        "accumulate_motion.moments_accumulator": lambda: mom.accumulate_motion(film, planes, None, ids, None, None, None, ctx),
        "accumulate_motion_device.clip_accumulator": lambda: clip.accumulate_motion_device(1, 2, None, 3, None, 0, None, 0, W, H, None, 4, 5, ctx),
        "accumulate_motion.carry.xyzw": lambda: carry.accumulate_motion(bad_film, planes, None, ids, None, None, None, ctx),
        "accumulate_motion.carry.planes": lambda: carry.accumulate_motion(film, bad_planes, None, ids, None, None, None, ctx),
        "accumulate_motion.carry.history": lambda: carry.accumulate_motion(film, planes, bad_history, ids, None, None, None, ctx),
        "accumulate_motion.carry.ids": lambda: carry.accumulate_motion(film, planes, None, bad_ids, None, None, None, ctx),
        "accumulate_split.xyzw": lambda: plain.accumulate_split(bad_film, None, planes, None, None, None, None, None, ctx),
        "accumulate_split.direct": lambda: plain.accumulate_split(film, np.zeros((H, W - 1, 4), F), planes, None, None, None, None, None, ctx),
        "accumulate_split.planes": lambda: plain.accumulate_split(film, None, bad_planes, None, None, None, None, None, ctx),
        "accumulate_split.history": lambda: plain.accumulate_split(film, None, planes, bad_history, None, None, None, None, ctx),
        "accumulate_split.ids": lambda: plain.accumulate_split(film, None, planes, None, bad_ids, None, None, None, ctx),
        "accumulate_split.direct_before_history": lambda: plain.accumulate_split(film, np.zeros((H, W - 1, 4), F), planes, bad_history, bad_ids, None, None, None, ctx),
        "accumulate_split.clip_accumulator": lambda: clip.accumulate_split(film, None, planes, None, None, None, None, None, ctx),
        "accumulate_split.clip_accumulator.shape_first": lambda: clip.accumulate_split(film, None, planes, bad_history, None, None, None, None, ctx),
        "accumulate_split.carry_accumulator": lambda: carry.accumulate_split(film, None, planes, None, None, None, None, None, ctx),
        "accumulate_split.moments_accumulator": lambda: mom.accumulate_split(film, None, planes, None, None, None, None, None, ctx),
        "accumulate_split_device.clip_accumulator": lambda: clip.accumulate_split_device(1, None, 2, None, None, None, 0, None, 0, W, H, None, 3, 4, ctx),
        "upsample.lo_xyzw": lambda: up.accumulate(np.zeros((LH, LW, 3), F), lo_planes, hi_planes, None, PIXEL_MAP, None, ctx),
        "upsample.lo_planes": lambda: up.accumulate(lo, np.zeros((LH, LW + 1, 3, 4), F), hi_planes, None, PIXEL_MAP, None, ctx),
        "upsample.hi_planes": lambda: up.accumulate(lo, lo_planes, np.zeros((H, W, 4), F), None, PIXEL_MAP, None, ctx),
        "upsample.history": lambda: up.accumulate(lo, lo_planes, hi_planes, np.zeros((H, W + 1, 3, 4), F), PIXEL_MAP, None, ctx),
        "upsample.pixel_map": lambda: up.accumulate(lo, lo_planes, hi_planes, None, (1.0, 0.0, 1.0), None, ctx),
        "upsample.prev_camera": lambda: up.accumulate(lo, lo_planes, hi_planes, None, PIXEL_MAP, np.zeros(11, F), ctx),
        "upsample_device.pixel_map": lambda: up.accumulate_device(1, 2, LW, LH, 3, None, W, H, (1.0, 0.0, 1.0), None, 4, 5, None, ctx),
        "upsample_motion.no_carry_bodies": lambda: up.accumulate_motion(np.zeros((LH, LW, 3), F), lo_planes, hi_planes, None, None, None, None, PIXEL_MAP, None, ctx),
        "upsample_motion_device.no_carry_bodies": lambda: up.accumulate_motion_device(1, 2, LW, LH, 3, None, None, None, 0, None, 0, W, H, PIXEL_MAP, None, 4, 5, None, ctx),
        "upsample_motion.lo_xyzw": lambda: up_carry.accumulate_motion(np.zeros((LH, LW, 3), F), lo_planes, hi_planes, None, None, None, None, PIXEL_MAP, None, ctx),
        "upsample_motion.lo_planes": lambda: up_carry.accumulate_motion(lo, np.zeros((LH, LW + 1, 3, 4), F), hi_planes, None, None, None, None, PIXEL_MAP, None, ctx),
        "upsample_motion.hi_planes": lambda: up_carry.accumulate_motion(lo, lo_planes, np.zeros((H, W, 4), F), None, None, None, None, PIXEL_MAP, None, ctx),
        "upsample_motion.history": lambda: up_carry.accumulate_motion(lo, lo_planes, hi_planes, np.zeros((H, W + 1, 3, 4), F), None, None, None, PIXEL_MAP, None, ctx),
        "upsample_motion.ids": lambda: up_carry.accumulate_motion(lo, lo_planes, hi_planes, None, bad_ids, None, None, PIXEL_MAP, None, ctx),
        "upsample_motion.pixel_map": lambda: up_carry.accumulate_motion(lo, lo_planes, hi_planes, None, ids, None, None, (1.0, 0.0, 1.0), None, ctx),
        "upsample.carry.hi_planes": lambda: up_carry.accumulate(lo, lo_planes, np.zeros((H, W, 4), F), None, PIXEL_MAP, None, ctx),
        "path.sample_map_and_environment": lambda: path.render(scene, ctx, sample_map=T.SampleMap(np.ones((5, 6)), 1), environment=env),
        "path.environment": lambda: path.render(scene, ctx, environment=np.zeros((2, 2, 3), F)),
        "path.env_scale": lambda: path.render(scene, ctx, environment=env, env_scale=-1.0),
        "path.sample_map": lambda: path.render(scene, ctx, sample_map=T.SampleMap(np.ones((5, 5)), 1)),
        "path.relight.environment": lambda: path.relight(scene, None),
        "path.relight.env_scale": lambda: path.relight(scene, env, env_scale=float("inf")),
        "aov.device_ids_without_device_out": lambda: T.AOVIntegrator(cam, smp).render(scene, ctx, device_ids=0x2000),
        "environment.eval": lambda: env.eval(np.zeros((5, 2), F), ctx),
        "environment.sample": lambda: env.sample(np.zeros((5, 3), F), ctx),
        "environment.sample.range": lambda: env.sample(np.ones((5, 2), F), ctx),
        "environment.pdf": lambda: env.pdf(np.zeros((5, 4), F), ctx),
    }
    return out


def record(T):
    """{"calls": {case: [[entry, arguments...], ...]}, "refusals": {case: message}} of the binding that is loaded, with nothing reaching a device."""
    ffi = T._ffi
    real_lib, real_buffer = ffi.lib, ffi.DeviceBuffer
    real, log = real_lib(), []
    stub = StubLib(real, ffi.SIGNATURES, log)
    out = {"calls": {}, "refusals": {}}
    ffi.lib = lambda: stub
    try:
        for name, fn in CASES.items():
            del log[:]
            ffi.DeviceBuffer = fake_buffers()
            ctx = FakeContext()
            with np.errstate(all="ignore"):  # nothing fills the output arrays here: what AOVIntegrator.normalise divides is whatever np.empty held
                fn(T, ctx, FakeScene(ctx))
            out["calls"][name] = list(log)
        del log[:]
        ctx = FakeContext()
        for name, fn in refusals(T, ctx, FakeScene(ctx)).items():
            try:
                fn()
            except T.TraceHipError as e:
                out["refusals"][name] = str(e)
            else:
                raise AssertionError(f"{name}: nothing was refused")
            assert not log, f"{name}: refused after a call was made: {log}"
    finally:
        ffi.lib, ffi.DeviceBuffer = real_lib, real_buffer
    return json.loads(json.dumps(out))  # what a reader of the file sees: lists, not tuples


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    graft.build_library()
    rec = record(graft.load_package())
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {sum(len(v) for v in rec['calls'].values())} calls of {len(rec['calls'])} cases, {len(rec['refusals'])} refusals")
