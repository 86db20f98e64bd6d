"""Temporal upsampling, the part that needs no GPU: the entry points and the parameter block's layout (header text == ctypes mirror, 112 bytes), the default parameters, the
refusals of the parameter block in the header's order (checked before any handle, so the message tells which check fired even without a device), the jittered low camera —
by its effect on Upscaler.pixel_map and against the cameras themselves through the oracle's generate_rays —, the jitter sequences, the session's constructor refusals, and the
properties of the numpy model (tests/temporal_upsample_model.py) the kernels are compared with bit for bit in tests/test_gpu_temporal_upsample.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import julia_replay as jr
import temporal_model as tm
import temporal_upsample_model as tum
import upscale_model as um
from test_temporal_api import format_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_temporal_upsample_default_params", "trhip_temporal_upsample", "trhip_temporal_upsample_device")
FIELDS = ["lo_from_hi", "prev_world_to_pixel", "max_history", "sigma_normal", "sigma_plane", "min_coverage", "guide_sigma_normal", "guide_sigma_plane", "confidence_floor",
          "confidence_sharpness", "radius", "flags", "reserved"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_entry_points_are_exported_with_the_headers_signatures(T):
    protos = jr.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, f"include/tracehip.h does not declare {name}"
        assert getattr(T.lib(), name) is not None
        ret, args = T._ffi.SIGNATURES[name]
        c_ret, c_args = jr.ctypes_sig(protos[name])
        assert ret is c_ret and len(args) == len(c_args), name
        for k, (a, c) in enumerate(zip(args, c_args)):
            if c is C.c_void_p:  # a pointer in the header: any pointer type in the table
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, k, a)
            else:
                assert a is c, (name, k, a, c)
    assert protos["trhip_temporal_upsample"][1] == ["ptr:void", "ptr:f32", "ptr:f32", "u32", "u32", "ptr:f32", "ptr:f32", "u32", "u32", "ptr:void", "ptr:f32", "ptr:f32", "ptr:u8",
                                                    "ptr:stats"]
    assert protos["trhip_temporal_upsample_device"][1] == ["ptr:void"] * 3 + ["u32", "u32", "ptr:void", "ptr:void", "u32", "u32"] + ["ptr:void"] * 4 + ["ptr:stats"]
    assert T.lib().trhip_version() == 3001, "added without a version change: nothing existing moved"


def test_params_mirror_matches_the_header(T):
    header = open(os.path.join(ROOT, "include", "tracehip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_temporal_upsample_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1), m.group(3)) for m in re.finditer(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)]
    assert [n for n, _, _ in fields] == FIELDS
    S = T._ffi.TemporalUpsampleParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    for (name, ctype), (n, t, dim) in zip(S._fields_, fields):
        assert name == n and C.sizeof(ctype) == C.sizeof(ctypes_of[t]) * int(dim or 1), name
    assert C.sizeof(S) == 112
    assert [getattr(S, n).offset for n in FIELDS] == [0, 16, 64, 68, 72, 76, 80, 84, 88, 92, 96, 100, 104]


def good_params(T, **over):
    p = T._ffi.TemporalUpsampleParams()
    assert T.lib().trhip_temporal_upsample_default_params(C.byref(p)) == 0
    p.lo_from_hi[:] = [0.5, -0.25, 0.5, -1.25]
    for k, v in over.items():
        if k == "map_entry":
            p.lo_from_hi[v[0]] = v[1]
        elif k == "matrix_entry":
            p.prev_world_to_pixel[v[0]] = v[1]
        elif k == "reserved_entry":
            p.reserved[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def test_default_params_need_no_context(T):
    p = T._ffi.TemporalUpsampleParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert T.lib().trhip_temporal_upsample_default_params(C.byref(p)) == 0
    assert list(p.lo_from_hi) == [0.0] * 4, "the map is the caller's to fill: a zero scale is refused"
    assert list(p.prev_world_to_pixel) == [0.0] * 12, "h.z = 0 for every point: no history through a forgotten matrix"
    assert (p.flags, list(p.reserved)) == (0, [0, 0]) and p.radius in (1, 2)
    t, u = T._ffi.TemporalParams(), T._ffi.UpscaleParams()
    assert T.lib().trhip_temporal_default_params(C.byref(t)) == 0 and T.lib().trhip_upscale_default_params(C.byref(u)) == 0
    assert (p.sigma_normal, p.sigma_plane, p.min_coverage) == (t.sigma_normal, t.sigma_plane, t.min_coverage) == (0.25, F(0.1), 0.5), "the history taps: trhip_temporal's"
    assert (p.guide_sigma_normal, p.guide_sigma_plane) == (u.sigma_normal, u.sigma_plane) == (0.25, F(0.4)), "the low taps: trhip_upscale's"
    assert (p.radius, p.max_history, p.confidence_floor, p.confidence_sharpness) == (1, 8.0, 0.0625, 2.0), "the sweep's cell (profiles/r16/temporal_upsample.txt)"
    assert T.lib().trhip_temporal_upsample_default_params(None) == INVALID
    tu = T.TemporalUpsampler()
    assert bytes(tu.params) == bytes(p) and tu.jitter == "grid" and tu.stats is None
    tu = T.TemporalUpsampler(radius=1, max_history=16.0, sigma_normal=0.5, sigma_plane=0.2, guide_sigma_normal=0.125, guide_sigma_plane=0.3, confidence_floor=0.0625,
                             confidence_sharpness=1.0, min_coverage=0.25, jitter=None)
    q = tu.params
    assert (q.radius, q.max_history, q.sigma_normal, q.sigma_plane, q.guide_sigma_normal, q.guide_sigma_plane, q.confidence_floor, q.confidence_sharpness, q.min_coverage) == \
        (1, 16.0, 0.5, F(0.2), 0.125, F(0.3), 0.0625, 1.0, 0.25)
    with pytest.raises(T.TraceHipError):
        T.TemporalUpsampler(radius=1.5)
    with pytest.raises(T.TraceHipError):
        T.TemporalUpsampler(jitter="sobol")


# one violation each, in the header's order: trhip_upscale's fields in its order, then trhip_temporal's own in its order, then the two new ones; then pairs: of two violations
# the earlier check must fire
BAD_PARAMS = [(dict(map_entry=(0, float("nan"))), b"lo_from_hi[0]"), (dict(map_entry=(3, float("inf"))), b"lo_from_hi[3]"), (dict(map_entry=(0, 0.2)), b"lo_from_hi[0]"),
              (dict(map_entry=(2, 1.5)), b"lo_from_hi[2]"), (dict(map_entry=(0, 0.0)), b"lo_from_hi[0]"), (dict(map_entry=(1, 1048576.0)), b"lo_from_hi[1]"),
              (dict(map_entry=(3, -1048576.0)), b"lo_from_hi[3]"), (dict(radius=0), b"radius"), (dict(radius=3), b"radius"),
              (dict(min_coverage=-0.1), b"min_coverage"), (dict(min_coverage=1.5), b"min_coverage"), (dict(min_coverage=float("nan")), b"min_coverage"),
              (dict(flags=1), b"flag"), (dict(flags=2), b"flag"), (dict(flags=0x80000000), b"flag"), (dict(reserved_entry=(0, 1)), b"reserved"), (dict(reserved_entry=(1, 7)), b"reserved"),
              (dict(matrix_entry=(0, float("nan"))), b"prev_world_to_pixel[0]"), (dict(matrix_entry=(11, float("inf"))), b"prev_world_to_pixel[11]"),
              (dict(max_history=0.5), b"max_history"), (dict(max_history=float("inf")), b"max_history"), (dict(max_history=float("nan")), b"max_history"),
              (dict(confidence_floor=0.0), b"confidence_floor"), (dict(confidence_floor=-0.5), b"confidence_floor"), (dict(confidence_floor=1.5), b"confidence_floor"),
              (dict(confidence_floor=float("nan")), b"confidence_floor"), (dict(confidence_sharpness=-0.5), b"confidence_sharpness"),
              (dict(confidence_sharpness=4.5), b"confidence_sharpness"), (dict(confidence_sharpness=float("nan")), b"confidence_sharpness")]
for _name in ("guide_sigma_normal", "guide_sigma_plane", "sigma_normal", "sigma_plane"):
    BAD_PARAMS += [({_name: v}, (b" " + _name.encode())) for v in (0.0, -1.0, float("inf"), float("nan"))]
ORDER = [dict(map_entry=(2, 9.0)), dict(radius=5), dict(guide_sigma_normal=0.0), dict(guide_sigma_plane=-1.0), dict(min_coverage=2.0), dict(flags=8), dict(reserved_entry=(0, 1)),
         dict(matrix_entry=(5, float("nan"))), dict(max_history=0.0), dict(sigma_normal=0.0), dict(sigma_plane=-1.0), dict(confidence_floor=2.0), dict(confidence_sharpness=5.0)]
ORDER_WORDS = [b"lo_from_hi", b"radius", b"guide_sigma_normal", b"guide_sigma_plane", b"min_coverage", b"flag", b"reserved", b"prev_world_to_pixel", b"max_history",
               b" sigma_normal", b" sigma_plane", b"confidence_floor", b"confidence_sharpness"]


@pytest.mark.parametrize("entry", ["trhip_temporal_upsample", "trhip_temporal_upsample_device"])
def test_invalid_parameter_blocks_are_refused_in_order_without_a_device(T, entry):
    """No context exists here, so every call is refused; the parameter block is checked first, and the message (kept for trhip_last_error(NULL)) names the field."""
    fn, L = getattr(T.lib(), entry), T.lib()
    lo, lp, hp, out, oh = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((4, 4, 3, 4), F), np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F)
    ptr = (lambda a: T._ffi.fptr(a)) if entry == "trhip_temporal_upsample" else (lambda a: C.c_void_p(a.ctypes.data))

    def call(p):
        return fn(None, ptr(lo), ptr(lp), 2, 2, ptr(hp), None, 4, 4, C.byref(p) if p is not None else None, ptr(out), ptr(oh), None, None)
    for over, word in BAD_PARAMS:
        assert call(good_params(T, **over)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    for i in range(len(ORDER)):
        for j in range(i + 1, len(ORDER)):
            assert call(good_params(T, **ORDER[i], **ORDER[j])) == INVALID
            assert ORDER_WORDS[i] in L.trhip_last_error(None), (ORDER[i], ORDER[j], L.trhip_last_error(None))
    assert call(None) == INVALID  # no parameter block
    for ok in (dict(), dict(map_entry=(0, 0.25)), dict(map_entry=(2, 1.0)), dict(radius=1), dict(min_coverage=0.0), dict(max_history=1.0), dict(confidence_floor=1.0),
               dict(confidence_floor=2.0 ** -20), dict(confidence_sharpness=0.0), dict(confidence_sharpness=4.0)):
        assert call(good_params(T, **ok)) == INVALID and b"null argument" in L.trhip_last_error(None), ("a valid block, and no context", ok)
    assert not out.any() and not oh.any()


# ---- the jittered low camera ---------------------------------------------------------------------------------------------------------------
def camera(T, resolution, crop=None, eye=(0, 15, 50), target=(0, 0, -2)):
    film = T.Film(list(resolution), T.Bounds2(*(crop or ([0.0, 0.0], [1.0, 1.0]))), T.LanczosSincFilter([1.5, 1.0], 3.0), 35.0, 0.75, "frame.png")
    return T.PerspectiveCamera(T.look_at(list(eye), list(target), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


JITTER_CAMERAS = {
    "64-full-from-32": (dict(resolution=(64, 64)), 2, (0.25, -0.25)),
    "1024-cropped-far-eye-from-512": (dict(resolution=(1024, 1024), crop=([0.25, 0.5], [0.75, 1.0]), eye=(0.0, 0.0, 1000.0), target=(0.0, 0.0, 0.0)), 2, (-0.25, 0.25)),
    "96x64-cropped-from-odd": (dict(resolution=(96, 64), crop=([0.2, 0.1], [0.9, 0.7])), 2.6, (1.0 / 3.0 - 0.5, 0.4375)),
}


@pytest.mark.parametrize("which", sorted(JITTER_CAMERAS))
def test_jitter_is_defined_by_its_effect_on_the_pixel_map(T, which):
    kw, factor, (jx, jy) = JITTER_CAMERAS[which]
    hi = camera(T, **kw)
    plain, shifted = T.Upscaler.low_camera(hi, factor), T.Upscaler.low_camera(hi, factor, jitter=(jx, jy))
    ax, bx, ay, by = T.Upscaler.pixel_map(hi, plain)
    jax, jbx, jay, jby = T.Upscaler.pixel_map(hi, shifted)
    assert (jax, jay) == (ax, ay), "the jitter moves the grid, it does not scale it"
    # Float32 rounding aside: the window corners, the matrices and their inverses are Float32; the axis position comes out of a quotient of two of their entries
    tol = 2.0 ** -17 * max(1.0, abs(bx), abs(by))
    assert abs(jbx - (bx + jx)) <= tol and abs(jby - (by + jy)) <= tol, (which, (jbx, bx + jx), (jby, by + jy))
    assert shifted.film is plain.film or (shifted.film.size == plain.film.size and list(shifted.film.crop_bounds.p_min) == list(plain.film.crop_bounds.p_min) and
                                          list(shifted.film.resolution) == list(plain.film.resolution) and shifted.film.filter is plain.film.filter)
    assert shifted.camera_to_world is hi.camera_to_world and shifted.fov == hi.fov
    for k in (0, 1):  # the same field of view: the raster-to-camera scale is unchanged but for the Float32 rounding of the window's extent
        a, b = float(shifted.raster_to_camera.m[k, k]), float(plain.raster_to_camera.m[k, k])
        assert abs(a - b) <= 2.0 ** -21 * abs(b)
    same = T.Upscaler.low_camera(hi, factor, jitter=(0.0, 0.0))
    assert bytes(same.sensor()) == bytes(plain.sensor()), "no jitter: today's low camera"
    with pytest.raises(T.TraceHipError):
        T.Upscaler.low_camera(hi, factor, jitter=(float("nan"), 0.0))


@pytest.mark.parametrize("which", sorted(JITTER_CAMERAS))
def test_jittered_low_camera_against_the_cameras(T, ob, which):
    """The referee of tests/test_upscale_api.py with a jittered low camera: points on the oracle's generate_rays ray through the centre of full-size pixel (x, y) land, through
    the jittered LOW camera's world_to_pixel, at (x * ax + bx + jx, y * ay + by + jy), bx and by the UNJITTERED map's, within the bound tests/test_temporal_api.py holds
    world_to_pixel to: what the Float32 formats allow, point by point (format_bound), and 1/32 px."""
    kw, factor, (jx, jy) = JITTER_CAMERAS[which]
    hi = camera(T, **kw)
    ax, bx, ay, by = T.Upscaler.pixel_map(hi, T.Upscaler.low_camera(hi, factor))
    lo = T.Upscaler.low_camera(hi, factor, jitter=(jx, jy))
    M = lo.world_to_pixel()
    h, w = hi.film.size
    cmin = np.asarray(hi.film.crop_bounds.p_min, np.float64)
    pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (w // 3, 2 * h // 3), (7, h - 5), (w - 9, 11)]
    samples = np.array([[cmin[0] + ix + 0.5, cmin[1] + iy + 0.5, 0.5, 0.5, 0.0] for ix, iy in pixels], F)
    rays = ob.generate_rays(hi, samples).astype(np.float64)
    eye_distance = float(np.linalg.norm(np.asarray(kw.get("eye", (0, 15, 50)), np.float64)))
    depths = np.geomspace(eye_distance / 50.0, 300.0, 12)
    worst = 0.0
    for (ix, iy), ray in zip(pixels, rays):
        o, d = ray[:3], ray[4:7]
        p = (o[None, :] + depths[:, None] * d[None, :]).astype(F)
        hx, hy, hz = tm.project(M, p)
        assert np.all(hz > 0)
        fx, fy = (hx / hz).astype(np.float64), (hy / hz).astype(np.float64)
        err = np.maximum(np.abs(fx - (ix * ax + bx + jx)), np.abs(fy - (iy * ay + by + jy)))
        worst = max(worst, float(err.max()))
        # + the one rounding of bx, by themselves and the Float32 rounding of the shifted window corners
        assert np.all(err <= format_bound(M, p, hz, fx, fy) + 2.0 ** -20 + 2.0 ** -23 * max(w, h)), (which, (ix, iy), err)
        assert err.max() <= 1.0 / 32.0, (which, (ix, iy), err)
    print(f"jittered low camera {which}: jitter ({jx}, {jy}), worst error {worst:.5f} low px")


def test_jitter_sequences(T):
    grid = T.TemporalUpsampler()
    assert [grid.jitter_for(k, 2) for k in range(6)] == [(0.25, 0.25), (-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25), (0.25, 0.25), (-0.25, -0.25)]
    # with the 2 x map's fractional parts of 1/4 and 3/4 (offsets -0.25 and -1.25) every full-size pixel centre lies on a low pixel centre once in four frames
    x = np.arange(8, dtype=np.float64)
    on = np.zeros((8, 8), int)
    for k in range(4):
        jx, jy = grid.jitter_for(k, 2)
        fx, fy = x * 0.5 - 0.25 + jx, x * 0.5 - 1.25 + jy
        on += ((fy == np.floor(fy))[:, None] & (fx == np.floor(fx))[None, :]).astype(int)
    assert (on == 1).all()
    for factor in (1, 1.5, 3, 4):
        with pytest.raises(T.TraceHipError):
            grid.jitter_for(0, factor)
    halton = T.TemporalUpsampler(jitter="halton")
    want = [(1 / 2, 1 / 3), (1 / 4, 2 / 3), (3 / 4, 1 / 9), (1 / 8, 4 / 9), (5 / 8, 7 / 9), (3 / 8, 2 / 9), (7 / 8, 5 / 9), (1 / 16, 8 / 9), (9 / 16, 1 / 27)]
    for k, (a, b) in enumerate(want):
        for factor in (2, 3, 1.5):
            jx, jy = halton.jitter_for(k, factor)
            assert abs(jx - (a - 0.5)) < 1e-15 and abs(jy - (b - 0.5)) < 1e-15, k
    assert all(-0.5 <= v < 0.5 for k in range(200) for v in halton.jitter_for(k, 2))
    none = T.TemporalUpsampler(jitter=None)
    assert [none.jitter_for(k, 3) for k in range(3)] == [(0.0, 0.0)] * 3
    with pytest.raises(T.TraceHipError):
        grid.jitter_for(-1, 2)


def test_session_constructor_refusals(T):
    smp = T.SeededSampler(1, seed=1)
    ok = T.PreviewSession(None, smp, 3, upscaler=T.Upscaler(), temporal_upsample=T.TemporalUpsampler())
    assert ok.temporal_upsample is not None and ok.frame == 0
    assert T.PreviewSession(None, smp, 3).temporal_upsample is None and T.PreviewSession(None, smp, 3, upscaler=T.Upscaler()).temporal_upsample is None
    T.PreviewSession(None, smp, 3, upscaler=T.Upscaler(), temporal=T.TemporalAccumulator(), temporal_upsample=T.TemporalUpsampler())  # a plain accumulator is no obstacle
    T.PreviewSession(None, smp, 3, upscaler=T.Upscaler(), factor=3, temporal_upsample=T.TemporalUpsampler(jitter="halton"))
    for kw, word in ((dict(), "upscaler"), (dict(upscaler=T.Upscaler(), variance_guided=True), "variance_guided"),
                     (dict(upscaler=T.Upscaler(), temporal=T.TemporalAccumulator(clip_gamma=2.0)), "clipping"),
                     (dict(upscaler=T.Upscaler(), temporal=T.TemporalAccumulator(moments=True)), "moments"),
                     (dict(upscaler=T.Upscaler(), factor=3), "grid")):
        with pytest.raises(T.TraceHipError, match=word):
            T.PreviewSession(None, smp, 3, temporal_upsample=T.TemporalUpsampler(), **kw)


# ---- the model's own properties -------------------------------------------------------------------------------------------------------------
SYNTH = {}


def synth():
    if not SYNTH:
        SYNTH["frame"] = tum.synthetic(29, 37, 15, 19, 4037)
    return SYNTH["frame"]


def test_model_synthetic_frame_takes_every_branch():
    lo, lp, hp, m, Hs, M = synth()
    tally = {}
    tum.accumulate(lo, lp, hp, Hs, M, tum.Params(m), tally)
    assert set(tally) == set(tum.TALLY_KEYS)
    for key in tum.TALLY_KEYS:
        assert tally[key] > 0, (key, tally)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("rho", [0.0, 2.0])
def test_model_without_history_is_the_upscaler(radius, rho):
    lo, lp, hp, m, _, M = synth()
    prm = tum.Params(m, radius=radius, confidence_sharpness=rho)
    out, hist, mask = tum.accumulate(lo, lp, hp, None, M, prm)
    ref, ref_mask, c = um.upscale(lo, lp, hp, tum.upscale_params(prm), want_colour=True)
    assert np.array_equal(bits(out), bits(ref)) and np.array_equal(mask, ref_mask), "history NULL: trhip_upscale's film and mask bit for bit"
    assert np.array_equal(bits(out[..., 3]), bits(hp[..., 0, 3])), "the .w lane is the full-size plane 0's weight"
    surface = hist[..., 1, 3] == 1
    assert np.array_equal(bits(hist[surface][:, 0, :3]), bits(c[surface])), "the history starts from the upscaled colour"
    assert np.isin(mask[surface], (0, 1, 3)).all() and np.isin(mask[~surface], (0, 2)).all() and not hist[~surface].any()
    k0 = F(prm.confidence_floor)
    O = hist[..., 0, 3]
    assert (O[surface & (mask == 3)] == k0).all() and (O[surface & (mask == 0)] == 0).all() and (O[mask == 1] >= k0).all() and (O <= 1).all()
    # rho = 0: geometry alone decides, wherever the pixel sits between the low centres; a sharper confidence only ever lowers it (gx, gy <= 1)
    O0 = tum.accumulate(lo, lp, hp, None, M, tum.Params(m, radius=radius, confidence_sharpness=0.0))[1][..., 0, 3]
    assert (O <= O0).all() and np.median(O0[mask == 1]) > 0.9
    if rho > 0.0:
        assert (O[mask == 1] < O0[mask == 1]).sum() > 500


def test_model_outputs_are_finite_whatever_the_inputs_hold():
    lo, lp, hp, m, Hs, M = synth()
    assert not np.isfinite(Hs).all() and not np.isfinite(lo).all() and not np.isfinite(hp).all()
    for R in (1, 2):
        for rho in (0.0, 2.0, 4.0):
            out, hist, mask = tum.accumulate(lo, lp, hp, Hs, M, tum.Params(m, radius=R, confidence_sharpness=rho))
            assert np.isfinite(out[..., :3]).all() and np.isfinite(hist).all()
            assert np.array_equal(bits(out[..., 3]), bits(hp[..., 0, 3]))
            assert (hist[..., 0, 3] >= 0).all() and (hist[..., 0, 3] <= 8).all() and set(np.unique(mask)) <= {0, 1, 2, 3, 4, 5, 7}
            assert (mask >= 4).sum() > 300 and ((mask & 3) == um.upscale(lo, lp, hp, tum.upscale_params(tum.Params(m, radius=R)))[1]).all()


def test_model_with_full_confidence_blends_as_the_temporal_pass_does():
    """kappa_0 = 1 makes kappa = 1 on every guided pixel and orphan (kmax <= 1), and the blend lines become 14-temporal.md's step 4 operation for operation: the accumulated
    weight of the temporal model run on the upscaled film with the same planes, history and matrix is the same number, and the colours differ by the rounding of the film's
    XYZ -> RGB round trip alone."""
    lo, lp, hp, m, Hs, M = synth()
    prm = tum.Params(m, confidence_floor=1.0, sigma_normal=0.02)
    out, hist, mask = tum.accumulate(lo, lp, hp, Hs, M, prm)
    up, _ = um.upscale(lo, lp, hp, tum.upscale_params(prm))
    t_out, t_hist = tm.accumulate(up, hp, Hs, M, tm.Params(max_history=8.0, sigma_normal=0.02, sigma_plane=0.1, min_coverage=0.5))
    both = (hist[..., 1, 3] == 1) & (t_hist[..., 1, 3] == 1) & np.isin(mask & 3, (1, 3))
    assert both.sum() > 800
    assert np.array_equal(bits(hist[both][:, 1:]), bits(t_hist[both][:, 1:])), "n and p"
    blended = both & (mask >= 4)
    assert blended.sum() > 300
    same_branch = blended & (t_hist[..., 0, 3] == hist[..., 0, 3])
    assert same_branch.sum() >= blended.sum() - 8, "a blend that overflows in one colour and not in the other by a rounding"
    a, b = hist[same_branch][:, 0, :3].astype(np.float64), t_hist[same_branch][:, 0, :3].astype(np.float64)
    assert np.all(np.abs(a - b) <= 1e-5 * np.maximum(1.0, np.maximum(np.abs(a), np.abs(b))))
    assert (hist[both & (mask < 4)][:, 0, 3] == 1).all(), "no history: the weight is kappa = 1, as N' = 1"


def test_model_orphan_with_history_keeps_the_history():
    """An orphan's confidence is the floor: with a history of weight 4 and kappa_0 = 2^-4 it moves 1 / 65 of the way from the history to its bilinear fill."""
    lo, lp, hp, m, Hs, M = synth()
    Hs = Hs.copy()
    was_surface = Hs[..., 1, 3] == 1
    Hs[..., 0, :3] = np.where(was_surface[..., None], F(1.0), F(0.0))
    Hs[..., 0, 3] = np.where(was_surface, F(4.0), F(0.0))
    prm = tum.Params(m, confidence_floor=2.0 ** -4)
    out, hist, mask = tum.accumulate(lo, lp, hp, Hs, M, prm)
    _, _, c = um.upscale(lo, lp, hp, tum.upscale_params(prm), want_colour=True)
    orphans = mask == 7
    assert orphans.sum() >= 10 and (mask == 3).sum() >= 10
    assert (hist[orphans][:, 0, 3] == F(4.0625)).all()
    moved = np.abs(hist[orphans][:, 0, :3].astype(np.float64) - 1.0)
    assert np.all(moved <= np.abs(c[orphans].astype(np.float64) - 1.0) / 65.0 * (1 + 1e-5) + 1e-6)
    assert np.array_equal(bits(hist[mask == 3][:, 0, :3]), bits(c[mask == 3])) and (hist[mask == 3][:, 0, 3] == F(2.0 ** -4)).all(), "without history: the fill, at the floor"
    nothing = (mask & 3 == 0) & (hist[..., 1, 3] == 1)
    assert nothing.sum() > 0 and (hist[nothing & (mask == 0)][:, 0, 3] == 0).all()
    kept = nothing & (mask == 4)
    if kept.any():  # kappa = 0: the history passes through untouched
        assert np.all(np.abs(hist[kept][:, 0, :3] - 1.0) < 1e-6) and (hist[kept][:, 0, 3] == 4.0).all()
