"""Edge-aware upscaling, the part that needs no GPU: the entry points and the parameter block's layout (header text == ctypes mirror, 48 bytes), the default parameters, the
refusals of the parameter block in the header's order (checked before any handle, so the message tells which check fired even without a device), with_resolution,
Upscaler.pixel_map against the cameras themselves through the oracle's generate_rays, and the properties of the numpy model (tests/upscale_model.py) the kernels are
compared with bit for bit in tests/test_gpu_upscale.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_model as dm
import julia_replay as jr
import temporal_model as tm
import upscale_model as um
from test_temporal_api import format_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_upscale_default_params", "trhip_upscale", "trhip_upscale_device")


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
    assert protos["trhip_upscale"][1] == ["ptr:void", "ptr:f32", "ptr:f32", "u32", "u32", "ptr:f32", "u32", "u32", "ptr:void", "ptr:f32", "ptr:u8", "ptr:stats"]
    assert protos["trhip_upscale_device"][1] == ["ptr:void"] * 3 + ["u32", "u32", "ptr:void", "u32", "u32"] + ["ptr:void"] * 3 + ["ptr:stats"]
    assert T.lib().trhip_version() == 3001, "added without a version change: nothing existing moved"


def test_params_mirror_matches_the_header(T):
    header = open(os.path.join(ROOT, "include", "tracehip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_upscale_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1), m.group(3)) for m in re.finditer(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)]
    assert [n for n, _, _ in fields] == ["lo_from_hi", "radius", "flags", "sigma_normal", "sigma_plane", "albedo_floor", "min_coverage", "reserved"]
    S = T._ffi.UpscaleParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    for (name, ctype), (n, t, dim) in zip(S._fields_, fields):
        assert name == n and C.sizeof(ctype) == C.sizeof(ctypes_of[t]) * int(dim or 1), name
    assert C.sizeof(S) == 48
    assert [getattr(S, n).offset for n, _, _ in fields] == [0, 16, 20, 24, 28, 32, 36, 40]
    assert re.search(r"#define\s+TRHIP_UPSCALE_DEMODULATE\s+1u", header) and re.search(r"#define\s+TRHIP_UPSCALE_COVERAGE\s+2u", header)
    assert (T._ffi.UPSCALE_DEMODULATE, T._ffi.UPSCALE_COVERAGE) == (1, 2)


def good_params(T, **over):
    p = T._ffi.UpscaleParams()
    assert T.lib().trhip_upscale_default_params(C.byref(p)) == 0
    p.lo_from_hi[:] = [0.5, -0.75, 0.5, -0.75]
    for k, v in over.items():
        if k == "map_entry":
            p.lo_from_hi[v[0]] = v[1]
        elif k == "reserved_entry":
            p.reserved[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def test_default_params_need_no_context(T):
    p = T._ffi.UpscaleParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert T.lib().trhip_upscale_default_params(C.byref(p)) == 0
    assert list(p.lo_from_hi) == [0.0] * 4, "the map is the caller's to fill: a zero scale is refused"
    assert (p.radius, p.flags, p.sigma_normal, p.sigma_plane, p.albedo_floor, p.min_coverage, list(p.reserved)) == (2, 0, 0.25, F(0.4), 1.0 / 64.0, 0.5, [0, 0])
    d = T._ffi.DenoiseParams()
    assert T.lib().trhip_denoise_default_params(C.byref(d)) == 0
    assert (p.sigma_normal, p.albedo_floor, p.min_coverage) == (d.sigma_normal, d.albedo_floor, d.min_coverage), "the denoiser's"
    assert T.lib().trhip_upscale_default_params(None) == INVALID
    u = T.Upscaler()
    assert bytes(u.params) == bytes(p)
    u = T.Upscaler(radius=1, coverage=True, sigma_plane=0.2)
    assert (u.params.radius, u.params.flags, u.params.sigma_plane) == (1, 2, F(0.2))
    assert T.Upscaler(demodulate=True, coverage=True).params.flags == 3 and T.Upscaler(demodulate=True, coverage=False).params.flags == 1
    with pytest.raises(T.TraceHipError):
        T.Upscaler(radius=1.5)


# one violation each, in the header's order; then pairs: of two violations the earlier check must fire
BAD_PARAMS = [(dict(map_entry=(0, float("nan"))), b"lo_from_hi[0]"), (dict(map_entry=(3, float("inf"))), b"lo_from_hi[3]"), (dict(map_entry=(0, 0.2)), b"lo_from_hi[0]"),
              (dict(map_entry=(2, 1.5)), b"lo_from_hi[2]"), (dict(map_entry=(0, 0.0)), b"lo_from_hi[0]"), (dict(map_entry=(1, 1048576.0)), b"lo_from_hi[1]"),
              (dict(map_entry=(3, -1048576.0)), b"lo_from_hi[3]"), (dict(radius=0), b"radius"), (dict(radius=3), b"radius"),
              (dict(min_coverage=-0.1), b"min_coverage"), (dict(min_coverage=1.5), b"min_coverage"), (dict(min_coverage=float("nan")), b"min_coverage"),
              (dict(flags=4), b"flag"), (dict(flags=0x80000001), b"flag"), (dict(reserved_entry=(0, 1)), b"reserved"), (dict(reserved_entry=(1, 7)), b"reserved")]
for _name in ("sigma_normal", "sigma_plane", "albedo_floor"):
    BAD_PARAMS += [({_name: v}, _name.encode()) for v in (0.0, -1.0, float("inf"), float("nan"))]
ORDER = [dict(map_entry=(2, 9.0)), dict(radius=5), dict(sigma_normal=0.0), dict(sigma_plane=-1.0), dict(albedo_floor=0.0), dict(min_coverage=2.0), dict(flags=8),
         dict(reserved_entry=(0, 1))]
ORDER_WORDS = [b"lo_from_hi", b"radius", b"sigma_normal", b"sigma_plane", b"albedo_floor", b"min_coverage", b"flag", b"reserved"]


@pytest.mark.parametrize("entry", ["trhip_upscale", "trhip_upscale_device"])
def test_invalid_parameter_blocks_are_refused_in_order_without_a_device(T, entry):
    """No context exists here, so every call is refused; the parameter block is checked first, and the message (kept for trhip_last_error(NULL)) names the field."""
    fn, L = getattr(T.lib(), entry), T.lib()
    lo, lp, hp, out = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F), np.zeros((4, 4, 3, 4), F), np.zeros((4, 4, 4), F)
    ptr = (lambda a: T._ffi.fptr(a)) if entry == "trhip_upscale" else (lambda a: C.c_void_p(a.ctypes.data))

    def call(p):
        return fn(None, ptr(lo), ptr(lp), 2, 2, ptr(hp), 4, 4, C.byref(p) if p is not None else None, ptr(out), None, None)
    for over, word in BAD_PARAMS:
        assert call(good_params(T, **over)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    for i in range(len(ORDER)):
        for j in range(i + 1, len(ORDER)):
            assert call(good_params(T, **ORDER[i], **ORDER[j])) == INVALID
            assert ORDER_WORDS[i] in L.trhip_last_error(None), (ORDER[i], ORDER[j], L.trhip_last_error(None))
    assert call(None) == INVALID  # no parameter block
    for ok in (dict(), dict(map_entry=(0, 0.25)), dict(map_entry=(2, 1.0)), dict(radius=1), dict(flags=0), dict(min_coverage=0.0), dict(min_coverage=1.0)):
        assert call(good_params(T, **ok)) == INVALID and b"null argument" in L.trhip_last_error(None), ("a valid block, and no context", ok)
    assert not out.any()


def camera(T, resolution, crop=None, eye=(0, 15, 50), target=(0, 0, -2)):
    film = T.Film(list(resolution), T.Bounds2(*(crop or ([0.0, 0.0], [1.0, 1.0]))), T.LanczosSincFilter([1.5, 1.0], 3.0), 35.0, 0.75, "frame.png")
    return T.PerspectiveCamera(T.look_at(list(eye), list(target), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def test_with_resolution_keeps_what_it_must(T):
    cam = camera(T, (64, 48), crop=([0.25, 0.5], [0.75, 1.0]))
    assert cam.fov == 90.0 and list(cam.screen_window.p_min) == [-1.0, -1.0]
    lo = cam.with_resolution([32, 24])
    assert lo is not cam and lo.film is not cam.film
    assert list(lo.film.resolution) == [32.0, 24.0] and lo.film.size == (12, 16) and cam.film.size == (24, 32)
    assert lo.film.crop_window == cam.film.crop_window and lo.film.filter is cam.film.filter
    assert lo.film.diagonal == cam.film.diagonal and lo.film.scale == cam.film.scale == F(0.75) and lo.film.filename == "frame.png"
    for name in ("shutter_open", "shutter_close", "lens_radius", "focal_distance", "fov"):
        assert getattr(lo, name) == getattr(cam, name), name
    assert lo.camera_to_world is cam.camera_to_world and lo.screen_window is cam.screen_window
    same = cam.with_resolution(cam.film.resolution)
    assert bytes(same.sensor()) == bytes(cam.sensor()), "the same resolution gives the same sensor"
    assert T.Upscaler.low_camera(cam, 2).film.size == (12, 16)
    with pytest.raises(T.TraceHipError):
        T.Upscaler.low_camera(cam, 5)


def test_pixel_map_of_full_frames(T):
    """ax is the ratio of the resolutions, exactly.  The offsets: with a principal point that scaled with the resolution (o_lo = ax * o_hi) full frames at 2 x would give
    (crop_min + 0.5) / 2 - 0.5 - crop_min = -0.75, crop_min being 1; the reference's raster_to_camera keeps it at raster (1, -1) at EVERY resolution, which moves the
    offsets by +-(1 - ax): -0.25 and -1.25 (test_pixel_map_against_the_cameras is the check; docs/design/17-upscale.md derives it)."""
    hi = camera(T, (64, 64))
    o = [-float(hi.raster_to_camera.m[k, 3]) / float(hi.raster_to_camera.m[k, k]) for k in (0, 1)]
    assert np.allclose(o, [1.0, -1.0], atol=1e-4)
    ax, bx, ay, by = T.Upscaler.pixel_map(hi, hi.with_resolution([32, 32]))
    assert (ax, ay) == (0.5, 0.5) and abs(bx - (-0.75 + 0.5 * o[0])) < 1e-4 and abs(by - (-0.75 + 0.5 * o[1])) < 1e-4
    assert T.Upscaler.pixel_map(hi, hi) == (1.0, 0.0, 1.0, 0.0)
    ax, bx, ay, by = T.Upscaler.pixel_map(camera(T, (37, 29)), camera(T, (19, 15)))
    assert (ax, ay) == (float(F(19 / 37)), float(F(15 / 29)))


PIXEL_MAP_CAMERAS = {
    "64-full-from-32": (dict(resolution=(64, 64)), (32, 32)),
    "1024-cropped-far-eye-from-512": (dict(resolution=(1024, 1024), crop=([0.25, 0.5], [0.75, 1.0]), eye=(0.0, 0.0, 1000.0), target=(0.0, 0.0, 0.0)), (512, 512)),
    "96x64-cropped-from-odd": (dict(resolution=(96, 64), crop=([0.2, 0.1], [0.9, 0.7])), (37, 29)),
}


@pytest.mark.parametrize("which", sorted(PIXEL_MAP_CAMERAS))
def test_pixel_map_against_the_cameras(T, ob, which):
    """Points on the oracle's generate_rays ray through the centre of full-size pixel (x, y) land, through the LOW camera's world_to_pixel, at (x * ax + bx, y * ay + by),
    within the bound tests/test_temporal_api.py holds world_to_pixel to for such cameras: what the Float32 formats allow, point by point (format_bound), and 1/32 px.  That
    is the accuracy of the yardstick, not of pixel_map."""
    kw, lo_res = PIXEL_MAP_CAMERAS[which]
    hi = camera(T, **kw)
    lo = hi.with_resolution(list(lo_res))
    ax, bx, ay, by = T.Upscaler.pixel_map(hi, lo)
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
        err = np.maximum(np.abs(fx - (ix * ax + bx)), np.abs(fy - (iy * ay + by)))
        worst = max(worst, float(err.max()))
        assert np.all(err <= format_bound(M, p, hz, fx, fy) + 2.0 ** -20), (which, (ix, iy), err)  # + the one rounding of bx, by themselves
        assert err.max() <= 1.0 / 32.0, (which, (ix, iy), err)
    print(f"pixel_map {which}: ({ax}, {bx}, {ay}, {by}), worst error {worst:.5f} low px")


# ---- the model's own properties -----------------------------------------------------------------------------------------------------------
def flat_pair(hh, hw, lh, lw, rgb, lo_from_hi):
    """One colour on one plane at both sizes, full coverage."""
    def planes(h, w, ax, bx, ay, by):
        ys, xs = np.mgrid[0:h, 0:w].astype(F)
        p = np.stack([(xs - F(bx)) / F(ax), (ys - F(by)) / F(ay), np.ones((h, w), F)], -1).astype(F) * F(0.01)
        n = np.broadcast_to(np.array([0.0, 0.0, 1.0], F), (h, w, 3))
        return dm.planes_of(n, p, np.full((h, w, 3), 0.5, F), np.ones((h, w), F), np.ones((h, w), F))
    xyz = dm.rgb_to_xyz(np.asarray(rgb, F))
    lo = np.concatenate([np.broadcast_to(xyz, (lh, lw, 3)), np.ones((lh, lw, 1), F)], -1).astype(F)
    return lo, planes(lh, lw, *lo_from_hi), planes(hh, hw, 1.0, 0.0, 1.0, 0.0)


def test_model_dyadic_colour_comes_back_to_the_bit():
    """Flags off, one low colour c_q on one plane: every product w * c_q is exact when the channels of c_q are powers of two, so sum = ws * c_q and c' = c_q to the bit on
    guided pixels.  XYZ -> RGB rounds, so the dyadic colour is put into the low records themselves; every other record is the film's."""
    m = (0.5, -0.75, 0.5, -0.75)
    dyadic = np.array([2.0, 0.5, 0.125], F)
    lo, lp, hp = flat_pair(24, 20, 12, 10, dyadic, m)
    for R in (1, 2):
        prm = um.Params(m, radius=R, demodulate=False, coverage=False)
        s_q, n_q, p_q, c_q, valid_q, u_q = um.low_records(lo, lp, prm)
        assert s_q.all() and np.abs(c_q - dyadic).max() < 1e-5
        c_q = np.broadcast_to(dyadic, c_q.shape).astype(F)
        out, mask, c = um.upscale(lo, lp, hp, prm, want_colour=True, records=(s_q, n_q, p_q, c_q, valid_q, u_q))
        assert (mask == 1).all() and np.array_equal(c.view(np.uint32), c_q[:1, :1].repeat(24, 0).repeat(20, 1).view(np.uint32)), R
        assert np.array_equal(out[..., :3].view(np.uint32), (dm.rgb_to_xyz(c) * hp[..., 0, 3:4]).astype(F).view(np.uint32))


def test_model_ratio_one_returns_the_pixels_own_colour():
    """Ratio 1, R = 1, flags off: tx = ty = 0, the only tap of non-zero weight is the pixel itself, c' = (w * c) / w: within one rounding of each of the two operations."""
    lo, lp, hp, m = um.synthetic_pair(17, 33, 17, 33, 5)
    assert m == (1.0, 0.0, 1.0, 0.0)
    prm = um.Params(m, radius=1, demodulate=False, coverage=False)
    out, mask, c = um.upscale(lo, lp, hp, prm, want_colour=True)
    s_q, _, _, c_q, _, _ = um.low_records(lo, lp, prm)
    g = mask == 1
    assert g.sum() > 300 and s_q[g].all(), "a guided pixel at ratio 1 has a surface pixel under it or beside it"
    own = g & s_q
    with np.errstate(all="ignore"):
        rel = np.abs(c[own].astype(np.float64) - c_q[own]) / np.abs(c_q[own].astype(np.float64))
    assert np.nanmax(rel) <= 2.0 ** -23, np.nanmax(rel)


def test_model_weight_lane_and_mask_classes():
    lo, lp, hp, m = um.synthetic_pair(29, 37, 15, 19, 7)
    for R in (1, 2):
        for flags in (True, False):
            out, mask = um.upscale(lo, lp, hp, um.Params(m, radius=R, demodulate=flags, coverage=flags))
            assert np.array_equal(out[..., 3].view(np.uint32), hp[..., 0, 3].view(np.uint32)), "the .w lane is plane 0's weight bit for bit"
            A, H = hp[..., 0, 3], hp[..., 1, 3]
            assert set(np.unique(mask)) == {0, 1, 2, 3}
            assert (mask[~(A > 0)] == 0).all() and not out[~(A > 0), :3].any()
            assert not out[mask == 0, :3].any(), "nothing: colour 0"
            no_surface = (A > 0) & ~((H > 0) & (H >= F(0.5) * A))
            assert np.isin(mask[no_surface], (0, 2)).all(), "guided and orphan are classes of surface pixels"
            poisoned = [(29 // 3, 37 // 4), (29 // 3 + 1, 37 // 4), (29 // 3 + 2, 37 // 4)]  # NaN normal, -Inf position, Inf base colour: no surface pixels (the last with demodulation)
            assert [int(mask[y, x]) for y, x in poisoned][:2] == [2, 2] and (mask[poisoned[2]] == 2) == flags
            assert ((mask == 2) & (A > 0) & ~no_surface).sum() <= 3
            assert np.isfinite(out[..., :3]).all(), "every colour is finite whatever the inputs hold"
            un, umask = um.upscale(lo, lp, hp, um.Params(m, radius=R, demodulate=flags, coverage=flags), unguided_only=True)
            assert not (umask == 1).any() and np.array_equal(un[mask != 1].view(np.uint32), out[mask != 1].view(np.uint32)), "H5 is what a failed pixel falls back to"


def test_model_synthetic_pair_takes_every_branch():
    lo, lp, hp, m = um.synthetic_pair(29, 37, 15, 19, 7)
    tally = {}
    um.upscale(lo, lp, hp, um.Params(m), tally)
    assert set(tally) == set(um.TALLY_KEYS)
    for key in um.TALLY_KEYS:
        assert tally[key] > 0, (key, tally)
    assert tally["orphan"] >= 20, "the stripe between the low pixel centres"
