"""The variance passes on the GPU (trhip_temporal_moments, trhip_denoise_var, TemporalAccumulator(moments=True), Denoiser.denoise_variance, PreviewSession(variance_guided=True)):
every output value against the numpy model of tests/variance_model.py bit for bit — on synthetic frames at sizes below a window, off the 16 x 16 tile and of several tiles, with
the gathering and staged forms of the filter, and on a Cornell sequence —; the three identities (the moments pass's colour and history are
trhip_temporal's, one iteration on a unit variance is trhip_denoise, the unguided session is unchanged); host == device == aliased; the refusals that need a context; the
invariants; and one quality figure per scene.

Quality ratios measured on an MI355X with the shipped defaults (MSE of xyz / w to the 1024 spp frame over the surface pixels of the eighth frame of the arcs of
tests/test_gpu_temporal.py, PreviewSession(variance_guided=True) / PreviewSession(); profiles/r13/variance.txt): Cornell 1.1303, mesh_scene(16) 1.1461 (QUALITY_MEASURED
below) — on these eight-frame arcs the guided session with the swept defaults is WORSE than the unguided one; the defaults were chosen over 8- and 40-frame arcs together."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import temporal_model as tm
import variance_model as vm
from test_gpu_temporal import QUALITY, QUALITY_SCENES, assert_bits_equal, bits, camera, frame

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(5, 3), (37, 29), (64, 64)]  # (w, h): smaller than a window both ways; partial tiles on both edges; 16 whole tiles
SIZE_IDS = ["5x3", "37x29", "64x64"]
KINDS = ("zero", "one", "random", "poisoned")
CACHE = {}


def cached(key, make):
    """Inputs and model outputs are computed once per case and left unchanged: callers copy what they pass on."""
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def moments_accumulator(T, demodulate, spatial_below=4.0, **kw):
    s = tm.SYNTHETIC_PARAMS
    base = dict(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage)
    base.update(kw)
    return T.TemporalAccumulator(moments=True, spatial_below=spatial_below, demodulate=demodulate, albedo_floor=1.0 / 64.0, **base)


def check_moments_outputs(got, ref, B, what):
    out, hist, mom, var = got
    for g, r, name in zip(got, ref, ("out_xyzw", "out_history", "out_moments", "out_variance")):
        assert_bits_equal(g, r, f"{what}: {name}")
    surface = ref[1][..., 1, 3] == 1
    assert np.isfinite(var).all() and np.all(var >= 0) and np.isfinite(mom).all(), what
    assert not var[~surface].any() and not mom[~surface].any() and not hist[~surface].any(), what
    assert_bits_equal(out[~surface], B[~surface], f"{what}: non-surface pixels")
    assert_bits_equal(out[..., 3], B[..., 3], f"{what}: the weight lane")


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_moments_on_synthetic_frames_equal_the_model(T, ctx, size, demodulate):
    w, h = size
    B, P, Hs, Ms, M = cached(("moments", h, w), lambda: vm.synthetic_moments(h, w, 2000 + h))
    prm = vm.moments_params(demodulate)
    ref, tally = cached(("moments", h, w, demodulate), lambda: (lambda t: (vm.accumulate(B, P, Hs, Ms, M, prm, t), t))({}))
    ref0 = cached(("moments0", h, w, demodulate), lambda: vm.accumulate(B, P, None, None, None, prm))
    if size == (37, 29):  # checked on the CPU before anything goes to the GPU: a NaN in a moment and in a history colour, non-surface pixels inside windows, off the image
        for name in ("temporal", "spatial", "short", "colour_restart", "moments_restart", "no_taps", "window_cut", "window_rejected", "moments_zeroed"):
            assert tally.get(name, 0) >= 1, (name, tally)
    t = moments_accumulator(T, demodulate)
    check_moments_outputs(t.accumulate_moments(B.copy(), P.copy(), Hs.copy(), Ms.copy(), M, ctx), ref, B, "with history")
    assert t.stats.launches_film == 1
    got = t.accumulate_moments(B.copy(), P.copy(), None, None, None, ctx)
    check_moments_outputs(got, ref0, B, "history = NULL")
    # the first identity: colour and history are trhip_temporal's
    s = tm.SYNTHETIC_PARAMS
    plain = T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage)
    out_plain, hist_plain = plain.accumulate(B, P, Hs, M, ctx)
    out, hist = t.accumulate_moments(B, P, Hs, Ms, M, ctx)[:2]
    assert_bits_equal(out, out_plain, "out_xyzw is trhip_temporal's")
    assert_bits_equal(hist, hist_plain, "out_history is trhip_temporal's")
    out0_plain, hist0_plain = plain.accumulate(B, P, None, None, ctx)
    assert_bits_equal(got[0], out0_plain, "history = NULL: out_xyzw is trhip_temporal's")
    assert_bits_equal(got[1], hist0_plain, "history = NULL: out_history is trhip_temporal's")


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
def test_moments_on_a_steady_state_frame_skip_and_walk(T, ctx, demodulate):
    """64 x 64, histories of 6 frames left of column 24 and of 1 frame right of it, spatial_below = 4: of the 64 patches of 16 x 4 pixels in a column of tiles, those of the
    first column of tiles need no window walk and skip it, those of the second need it for half their lanes, the others for all."""
    h = w = 64
    B, P, Hs, Ms, M = cached(("steady",), lambda: vm.synthetic_steady(h, w, 4242))
    prm = vm.MomentsParams(8.0, 0.25, 0.1, 0.5, 1.0 / 64.0, 4.0, demodulate)
    ref, tally = cached(("steady", demodulate), lambda: (lambda t: (vm.accumulate(B, P, Hs, Ms, M, prm, t), t))({}))
    assert tally["temporal"] == 24 * h and tally["spatial"] == tally["short"] == (w - 24) * h, tally
    N = ref[1][..., 0, 3]
    assert np.all(N[:, :24] == 7.0) and np.all(N[:, 24:] == 2.0)
    assert (ref[3][:, :24] > 0).mean() > 0.9 and (ref[3][:, 24:] > 0).mean() > 0.9, "both estimates are real variances"
    t = T.TemporalAccumulator(max_history=8.0, sigma_normal=0.25, sigma_plane=0.1, min_coverage=0.5, moments=True, spatial_below=4.0, demodulate=demodulate, albedo_floor=1.0 / 64.0)
    check_moments_outputs(t.accumulate_moments(B, P, Hs, Ms, M, ctx), ref, B, "spatial_below 4")
    # spatial_below = 1: every pixel with a history takes the temporal estimate, no wave walks
    ref1 = vm.accumulate(B, P, Hs, Ms, M, vm.MomentsParams(8.0, 0.25, 0.1, 0.5, 1.0 / 64.0, 1.0, demodulate))
    t1 = T.TemporalAccumulator(max_history=8.0, sigma_normal=0.25, sigma_plane=0.1, min_coverage=0.5, moments=True, spatial_below=1.0, demodulate=demodulate, albedo_floor=1.0 / 64.0)
    check_moments_outputs(t1.accumulate_moments(B, P, Hs, Ms, M, ctx), ref1, B, "spatial_below 1")


def test_moments_of_a_dyadic_surface_are_exact(T, ctx):
    """One luminance, 0.25 to the bit: every sum is exact, both estimates are exactly 0 (tests/test_variance_api.py has the argument)."""
    from test_temporal_clip_api import uniform_surface
    h, w = 9, 10
    B, P, n, p = uniform_surface(h, w, 0.25)
    M = F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    t = T.TemporalAccumulator(max_history=8.0, moments=True, spatial_below=4.0, demodulate=False)
    out, hist, mom, var = t.accumulate_moments(B, P, None, None, None, ctx)
    assert not var.any() and np.all(mom[..., 0] == F(0.25)) and np.all(mom[..., 1] == F(0.0625))
    hist[..., 0, 3] = np.where(np.arange(w)[None, :] % 2 == 0, F(1.0), F(6.0))
    out, hist2, mom2, var2 = t.accumulate_moments(B, P, hist, mom, M, ctx)
    assert not var2.any() and set(np.unique(hist2[..., 0, 3])) == {2.0, 7.0}
    assert_bits_equal(mom2, mom, "the moments of a constant luminance stay")


CORNELL = dict(resolution=48, spp=2, depth=3, seed=0x7E3A, degrees=(0.0, 3.0, 6.0, 9.0))


@pytest.fixture(scope="module")
def cornell_sequence(T, ctx):
    """[(camera, xyzw, planes)]: 48 x 48, 2 spp, depth 3, four cameras on an arc, frame k at sample_offset k * spp."""
    scene, s = T.scenes.cornell_scene(), CORNELL
    out = []
    for k, deg in enumerate(s["degrees"]):
        cam = camera(T, s["resolution"], deg)
        out.append((cam,) + frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"]))
    return out


def test_cornell_sequence_keeps_trhip_temporals_bits_and_equals_the_model(T, ctx, cornell_sequence):
    t, plain = T.TemporalAccumulator(moments=True), T.TemporalAccumulator()
    p, mp = t.params, t.moments_params
    prm = vm.MomentsParams(p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage, mp.albedo_floor, mp.spatial_below, bool(mp.flags & 1))
    hist = mom = prev = hist_plain = None
    tally = {}
    for k, (cam, xyzw, planes) in enumerate(cornell_sequence):
        M = prev.world_to_pixel() if prev is not None else None
        ref = vm.accumulate(xyzw, planes, hist, mom, M, prm, tally)
        got = t.accumulate_moments(xyzw, planes, hist, mom, prev, ctx)
        check_moments_outputs(got, ref, xyzw, f"frame {k}")
        out_plain, hist_plain = plain.accumulate(xyzw, planes, hist_plain, prev, ctx)
        assert_bits_equal(got[0], out_plain, f"frame {k}: out_xyzw is trhip_temporal's")
        assert_bits_equal(got[1], hist_plain, f"frame {k}: out_history is trhip_temporal's")
        hist, mom, prev = got[1], got[2], cam
    print(f"cornell sequence, moments tally: {tally}")
    assert hist[..., 0, 3].max() == 4.0 and tally["temporal"] > 500 and tally["short"] > 500, tally


def var_params(sigma, eps, iterations, demodulate):
    return vm.VarParams(sigma, 0.25, 0.1, iterations=iterations, demodulate=demodulate, var_eps=eps)


def var_denoiser(T, prm):
    return T.Denoiser(iterations=prm.iterations, demodulate=prm.demodulate, sigma_normal=prm.sigma_normal, sigma_plane=prm.sigma_plane, variance_sigma=prm.sigma_colour, var_eps=prm.var_eps)


def lds_masks(ctx, call):
    try:
        for mask in (0, 3):
            ctx.set_option("denoise_var_lds", mask)
            yield mask, call()
    finally:
        ctx.set_option("denoise_var_lds", 3)


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_denoise_var_on_synthetic_frames_equals_the_model(T, ctx, size, demodulate):
    w, h = size
    if h < 16:
        big = cached(("film", 29, 37), lambda: dm.synthetic(29, 37, 3029)[:2])
        B, P = big[0][8:8 + h, 8:8 + w].copy(), big[1][8:8 + h, 8:8 + w].copy()  # dm.synthetic poisons fixed positions: no film of it is that small
    else:
        B, P = cached(("film", h, w), lambda: dm.synthetic(h, w, 3000 + h)[:2])
    finite_film = np.isfinite(B).all(-1) & np.isfinite(P).all((-1, -2))
    tally = {}
    for kind in KINDS:
        V = vm.synthetic_variance(h, w, 3000 + h, kind)
        for iterations in (1, 3, 6):
            prm = var_params(2.0, 2.0 ** -6, iterations, demodulate)
            ref_out, ref_var = vm.denoise(B, P, V, prm, tally)
            d = var_denoiser(T, prm)
            for mask, (out, var) in lds_masks(ctx, lambda: d.denoise_variance(B, P, V, ctx)):
                what = f"{kind}, {iterations} iterations, denoise_var_lds {mask}"
                assert_bits_equal(out, ref_out, what + ": out_xyzw")
                assert_bits_equal(var, ref_var, what + ": out_variance")
                assert d.stats.launches_sub[1] == iterations
                surface = dm.surface_mask(B, P, prm)
                assert np.isfinite(out[surface]).all(), what + ": every output colour is finite whatever the variance plane holds"
                assert not np.isnan(var).any() and np.all(var >= 0) and not var[~surface].any(), what
                if kind != "poisoned":
                    assert np.isfinite(var).all(), what
                assert_bits_equal(out[~surface], B[~surface], what + ": non-surface pixels")
                assert_bits_equal(out[..., 3], B[..., 3], what + ": the weight lane")
    if h >= 16:
        assert finite_film.sum() > 0 and tally["colour"][0] > 0 and tally["colour"][1] > 0 and tally["inf_sigma"] > 0 and tally["nan_variance"] > 0, tally
    # iterations = 0 copies the film; the variance comes back clamped, 0 off surfaces
    prm = var_params(2.0, 2.0 ** -6, 0, demodulate)
    V = vm.synthetic_variance(h, w, 3000 + h, "poisoned")
    ref_out, ref_var = vm.denoise(B, P, V, prm)
    out, var = var_denoiser(T, prm).denoise_variance(B, P, V, ctx)
    assert_bits_equal(out, B, "iterations = 0: out_xyzw")
    assert_bits_equal(var, ref_var, "iterations = 0: out_variance")


@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("size", SIZES[1:], ids=SIZE_IDS[1:])
def test_one_iteration_on_a_unit_variance_is_trhip_denoise(T, ctx, size, demodulate):
    """The second identity: gv = 1, sd = 1, sig = 3.5 * 1 + 0.5 = 4 exactly, so out_xyzw is trhip_denoise(iterations = 1, sigma_colour = 4)'s bit for bit."""
    w, h = size
    B, P = cached(("film", h, w), lambda: dm.synthetic(h, w, 3000 + h)[:2])
    want = T.Denoiser(iterations=1, demodulate=demodulate, sigma_colour=4.0).denoise(B, P, ctx)
    d = T.Denoiser(iterations=1, demodulate=demodulate, variance_sigma=3.5, var_eps=0.5)
    for mask, (out, var) in lds_masks(ctx, lambda: d.denoise_variance(B, P, np.ones((h, w), F), ctx)):
        assert_bits_equal(out, want, f"denoise_var_lds {mask}")
    assert (bits(out) != bits(B)).mean() > 0.3, "the film was filtered"


def test_host_device_and_aliased_calls_agree(T, ctx):
    h, w = 29, 37
    B, P, Hs, Ms, M = cached(("moments", h, w), lambda: vm.synthetic_moments(h, w, 2000 + h))
    ref = cached(("moments", h, w, True), lambda: (vm.accumulate(B, P, Hs, Ms, M, vm.moments_params(True), {}), {}))[0]
    t = moments_accumulator(T, True)
    zeros = (np.zeros_like(B), np.zeros_like(P), np.zeros_like(Ms), np.zeros((h, w), F))
    bufs = [T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in (B, P, Hs, Ms) + zeros]
    d_in, d_pl, d_hs, d_ms, d_out, d_oh, d_om, d_ov = bufs
    shapes = (B.shape, P.shape, Ms.shape, (h, w))
    t.accumulate_moments_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_ms.ptr, w, h, M, d_out.ptr, d_oh.ptr, d_om.ptr, d_ov.ptr, ctx)
    for b, r, shape, name in zip((d_out, d_oh, d_om, d_ov), ref, shapes, ("out_xyzw", "out_history", "out_moments", "out_variance")):
        assert_bits_equal(b.to_host(np.float32, shape), r, f"device variant, {name}")
    for b, a, what in ((d_in, B, "xyzw"), (d_pl, P, "planes"), (d_hs, Hs, "history"), (d_ms, Ms, "moments")):
        assert_bits_equal(b.to_host(np.float32, a.shape), a, f"the input {what} is left alone")
    for b in (d_oh, d_om, d_ov):
        b.zero()
    # the staging reads neighbours' film pixels: an aliased result goes through a film of the context's, and is the same bits
    t.accumulate_moments_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_ms.ptr, w, h, M, d_in.ptr, d_oh.ptr, d_om.ptr, d_ov.ptr, ctx)
    for b, r, shape, name in zip((d_in, d_oh, d_om, d_ov), ref, shapes, ("out_xyzw", "out_history", "out_moments", "out_variance")):
        assert_bits_equal(b.to_host(np.float32, shape), r, f"out aliasing xyzw, device, {name}")
    buf, hist, mom, var = B.copy(), np.empty_like(P), np.empty_like(Ms), np.empty((h, w), F)
    mp, f = t._moments_params_for(M), T._ffi.fptr
    assert T.lib().trhip_temporal_moments(ctx._h, f(buf), f(P), f(Hs), f(Ms), w, h, C.byref(mp), f(buf), f(hist), f(mom), f(var), None) == 0
    for g, r, name in zip((buf, hist, mom, var), ref, ("out_xyzw", "out_history", "out_moments", "out_variance")):
        assert_bits_equal(g, r, f"out aliasing xyzw, host, {name}")
    # the filter: device pointers, the film and the variance plane filtered in place
    prm = var_params(2.0, 2.0 ** -6, 3, True)
    V = vm.synthetic_variance(h, w, 77, "random")
    B2, P2 = dm.synthetic(h, w, 3029)[:2]
    ref_out, ref_var = vm.denoise(B2, P2, V, prm)
    d = var_denoiser(T, prm)
    d_in.from_host(B2), d_pl.from_host(P2), d_ov.from_host(V)
    d.denoise_variance_device(d_in.ptr, d_pl.ptr, d_ov.ptr, w, h, d_out.ptr, None, ctx)
    assert_bits_equal(d_out.to_host(np.float32, B.shape), ref_out, "device variant, out_variance = NULL")
    assert_bits_equal(d_ov.to_host(np.float32, (h, w)), V, "the variance plane is left alone")
    d.denoise_variance_device(d_in.ptr, d_pl.ptr, d_ov.ptr, w, h, d_in.ptr, d_ov.ptr, ctx)
    assert_bits_equal(d_in.to_host(np.float32, B.shape), ref_out, "in place, out_xyzw")
    assert_bits_equal(d_ov.to_host(np.float32, (h, w)), ref_var, "in place, out_variance")
    buf, var = B2.copy(), V.copy()
    vp = d._var_params()
    assert T.lib().trhip_denoise_var(ctx._h, f(buf), f(P2), f(var), w, h, C.byref(vp), f(buf), f(var), None) == 0
    assert_bits_equal(buf, ref_out, "in place, host, out_xyzw")
    assert_bits_equal(var, ref_var, "in place, host, out_variance")
    for b in bufs:
        b.free()


def test_refusals(T, ctx):
    h, w = 29, 37
    B, P, Hs, Ms, M = cached(("moments", h, w), lambda: vm.synthetic_moments(h, w, 2000 + h))
    ref = cached(("moments", h, w, True), lambda: (vm.accumulate(B, P, Hs, Ms, M, vm.moments_params(True), {}), {}))[0]
    L, t = T.lib(), moments_accumulator(T, True)
    p = t._moments_params_for(M)
    out, hist, mom, var = np.zeros_like(B), np.zeros_like(P), np.zeros_like(Ms), np.zeros((h, w), F)
    ptr = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731

    def call(xyzw=B, planes=P, history=Hs, moments=Ms, w=w, h=h, prm=p, o=out, oh=hist, om=mom, ov=var, handle=ctx._h):
        return L.trhip_temporal_moments(handle, ptr(xyzw), ptr(planes), ptr(history), ptr(moments), w, h, C.byref(prm) if prm is not None else None, ptr(o), ptr(oh), ptr(om), ptr(ov), None)
    assert call() == 0
    for kw in (dict(prm=None), dict(xyzw=None), dict(planes=None), dict(o=None), dict(oh=None), dict(om=None), dict(ov=None), dict(w=0), dict(h=0), dict(handle=None)):
        assert call(**kw) == -1, kw
        assert L.trhip_last_error(None if "handle" in kw else ctx._h).decode(), kw
    for kw in (dict(moments=None), dict(history=None)):
        assert call(**kw) == -1 and "exactly when" in L.trhip_last_error(ctx._h).decode(), kw
    flat = lambda a, n: a.reshape(-1)[:n]  # noqa: E731
    for kw in (dict(oh=Hs), dict(oh=P), dict(history=hist), dict(planes=hist), dict(om=Ms), dict(om=flat(Hs, Ms.size).reshape(Ms.shape)), dict(om=flat(hist, Ms.size).reshape(Ms.shape)),
               dict(ov=flat(Ms, var.size).reshape(var.shape)), dict(ov=flat(mom, var.size).reshape(var.shape)), dict(ov=flat(B, var.size).reshape(var.shape)),
               dict(ov=flat(out, var.size).reshape(var.shape))):
        assert call(**kw) == -1, list(kw)
        assert "overlap" in L.trhip_last_error(ctx._h).decode(), (list(kw), L.trhip_last_error(ctx._h))
    big = np.zeros(B.size, F)  # out_xyzw over the moments
    big[:Ms.size] = Ms.reshape(-1)
    assert call(moments=big[:Ms.size].reshape(Ms.shape), o=big.reshape(B.shape)) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    for field, value, word in (("albedo_floor", 0.0, "albedo_floor"), ("spatial_below", 0.5, "spatial_below"), ("flags", 2, "flag"), ("reserved", 1, "reserved")):
        bad = T._ffi.TemporalMomentsParams.from_buffer_copy(p)
        setattr(bad, field, value)
        assert call(prm=bad) == -1 and word in L.trhip_last_error(ctx._h).decode(), field
    bad = T._ffi.TemporalMomentsParams.from_buffer_copy(p)
    bad.base.max_history = 0.0
    assert call(prm=bad) == -1 and "max_history" in L.trhip_last_error(ctx._h).decode()
    for a in (out, hist, mom, var):
        a[:] = 0
    assert call() == 0, "a refused call leaves the context usable"
    for g, r, name in zip((out, hist, mom, var), ref, ("out_xyzw", "out_history", "out_moments", "out_variance")):
        assert_bits_equal(g, r, f"after the refusals, {name}")
    # the filter
    d = T.Denoiser()
    vp = d._var_params()
    V = np.ones((h, w), F)

    def call_var(xyzw=B, planes=P, variance=V, w=w, h=h, prm=vp, o=out, ov=var, handle=ctx._h):
        return L.trhip_denoise_var(handle, ptr(xyzw), ptr(planes), ptr(variance), w, h, C.byref(prm) if prm is not None else None, ptr(o), ptr(ov), None)
    assert call_var() == 0 and call_var(ov=None) == 0
    for kw in (dict(prm=None), dict(xyzw=None), dict(planes=None), dict(variance=None), dict(o=None), dict(w=0), dict(h=0), dict(handle=None)):
        assert call_var(**kw) == -1, kw
    for field, value, word in (("var_eps", 0.0, "var_eps"), ("flags", 1, "flag")):
        bad = T._ffi.DenoiseVarParams.from_buffer_copy(vp)
        setattr(bad, field, value)
        assert call_var(prm=bad) == -1 and word in L.trhip_last_error(ctx._h).decode(), field
    with pytest.raises(T.TraceHipError):
        T.Denoiser(var_eps=float("nan")).denoise_variance(B, P, V, ctx)
    with pytest.raises(T.TraceHipError):
        T.TemporalAccumulator(moments=True, spatial_below=0.0).accumulate_moments(B, P, None, None, None, ctx)


def test_preview_sessions_guided_equals_the_models_and_unguided_is_unchanged(T, ctx, cornell_sequence):
    """The four-frame Cornell sequence through PreviewSession(variance_guided=True) against the models chained the same way; and PreviewSession() against the three existing
    entry points called as before this argument existed (the third identity)."""
    scene, s = T.scenes.cornell_scene(), CORNELL
    guided = T.PreviewSession(scene, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], variance_guided=True)
    plain = T.PreviewSession(scene, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"])
    t, d = T.TemporalAccumulator(), T.Denoiser()
    p, mp = guided.temporal.params, guided.temporal.moments_params
    mprm = vm.MomentsParams(p.max_history, p.sigma_normal, p.sigma_plane, p.min_coverage, mp.albedo_floor, mp.spatial_below, bool(mp.flags & 1))
    dp = guided.denoiser.params
    vprm = vm.VarParams(guided.denoiser.variance_sigma, dp.sigma_normal, dp.sigma_plane, dp.iterations, bool(dp.flags & 1), dp.albedo_floor, dp.min_coverage, guided.denoiser.var_eps)
    hist = mom = prev = hist_plain = None
    for k, (cam, xyzw, planes) in enumerate(cornell_sequence):
        got, got_plain = guided.render(cam, ctx), plain.render(cam, ctx)
        M = prev.world_to_pixel() if prev is not None else None
        acc, hist, mom, var = vm.accumulate(xyzw, planes, hist, mom, M, mprm)
        want = vm.denoise(acc if k else xyzw, planes, var, vprm)[0]
        assert_bits_equal(got, want, f"frame {k}: the guided session against the models")
        assert_bits_equal(got[..., 3], xyzw[..., 3], f"frame {k}: the weight lane")
        assert len(guided.render_stats) == 4 and guided.render_stats[2].launches_film == 1
        acc_plain, hist_plain = t.accumulate(xyzw, planes, hist_plain, prev, ctx)
        assert_bits_equal(got_plain, d.denoise(acc_plain if k else xyzw, planes, ctx), f"frame {k}: the unguided session is path + planes + temporal + denoise by hand")
        if k == 0:
            alone = T.Denoiser().render(scene, cam, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], ctx, variance_guided=True)
            assert_bits_equal(got, alone, "a frame without history is Denoiser.render(variance_guided=True)'s")
            assert_bits_equal(got_plain, T.Denoiser().render(scene, cam, T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], ctx), "… and unguided, Denoiser.render's")
        prev = cam
    assert (bits(got) != bits(got_plain)).mean() > 0.3, "the variance is in use"
    guided.reset()
    cam = camera(T, s["resolution"], 12.0)
    got = guided.render(cam, ctx)
    want = T.Denoiser().render(scene, cam, T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=4 * s["spp"]), s["depth"], ctx, variance_guided=True)
    assert_bits_equal(got, want, "after reset(): Denoiser.render(variance_guided=True) of that frame")
    guided.close(), plain.close()


QUALITY_MEASURED = {"cornell": 1.1303, "mesh16": 1.1461}  # mse(PreviewSession(variance_guided=True)) / mse(PreviewSession()), eighth frame


@pytest.mark.parametrize("which", sorted(QUALITY_SCENES))
def test_guided_preview_against_the_unguided_one(T, ctx, which):
    """The arcs of tests/test_gpu_temporal.py (64 x 64, 2 spp, eight cameras 0.75 degrees apart): the last frame through PreviewSession(variance_guided=True) against the
    same frame through PreviewSession() — the session as it was before this argument, computed here —, both measured (MSE of xyz / w over surface pixels) against that
    camera's 1024 spp frame.  The renders are bit-reproducible, so the ratio is a number; the assertion is that number as measured on an MI355X with the shipped defaults,
    within 10 % for compiler drift.  The direction is not presupposed: a ratio above 1 says the guided session is worse there, and it is — measured 1.1303 (Cornell: MSE
    0.0393655 against 0.0348275) and 1.1461 (mesh_scene(16): 0.0345715 against 0.0301647)."""
    scene, q = QUALITY_SCENES[which](T), QUALITY
    cams = [camera(T, q["resolution"], deg) for deg in q["degrees"]]
    results = {}
    for name, kw in (("guided", dict(variance_guided=True)), ("unguided", dict())):
        session = T.PreviewSession(scene, T.SeededSampler(q["spp"], seed=q["seed"]), q["depth"], **kw)
        for cam in cams:
            results[name] = session.render(cam, ctx)
        session.close()
    last, offset = cams[-1], (len(cams) - 1) * q["spp"]
    noisy, planes = frame(T, scene, last, q["spp"], q["depth"], q["seed"], offset)
    target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), q["depth"]).render(scene)
    surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))
    assert surface.sum() >= 1000
    assert_bits_equal(results["guided"][..., 3], noisy[..., 3], "the weight lane")

    def mse(a):
        with np.errstate(all="ignore"):
            diff = a[surface][:, :3].astype(np.float64) / a[surface][:, 3:4] - target[surface][:, :3].astype(np.float64) / target[surface][:, 3:4]
        return float(np.mean(diff * diff))
    guided, unguided = mse(results["guided"]), mse(results["unguided"])
    ratio = guided / unguided
    print(f"variance quality {which}: mse 2 spp {mse(noisy):.6g}, PreviewSession() {unguided:.6g}, PreviewSession(variance_guided=True) {guided:.6g}, ratio {ratio:.4f}")
    assert QUALITY_MEASURED[which] / 1.10 <= ratio <= QUALITY_MEASURED[which] * 1.10
