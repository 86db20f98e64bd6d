"""The edge-avoiding denoiser, the part that needs no GPU: the parameter block's layout (header text == ctypes mirror, 32 bytes), the entry points, the default parameters, and
the properties of the numpy model (tests/denoise_model.py) the kernels are compared with bit for bit in tests/test_gpu_denoise.py."""
import ctypes as C
import os
import re

import numpy as np

import denoise_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
H, W = 17, 23  # the synthetic inputs: 23 x 17 pixels


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def header_fields():
    """(name, C type) of every member of trhip_denoise_params, from the text of include/tracehip.h (all members are 4-byte scalars: no padding)."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracehip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_denoise_params\s*;", src).group(1)
    return [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]


def test_params_mirror_matches_the_header(T):
    fields = header_fields()
    assert [n for n, _ in fields] == ["iterations", "flags", "sigma_colour", "sigma_normal", "sigma_plane", "albedo_floor", "min_coverage", "reserved"]
    S = T._ffi.DenoiseParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    assert [(n, ct) for n, ct in S._fields_] == [(n, ctypes_of[t]) for n, t in fields]
    assert C.sizeof(S) == 32 == 4 * len(fields)
    assert [getattr(S, n).offset for n, _ in fields] == list(range(0, 32, 4))
    header = open(os.path.join(ROOT, "include", "tracehip.h")).read()
    assert re.search(r"#define\s+TRHIP_DENOISE_DEMODULATE\s+1u?\b", header) and T._ffi.DENOISE_DEMODULATE == 1


def test_entry_points_are_declared_and_bound(T):
    header = open(os.path.join(ROOT, "include", "tracehip.h")).read()
    for name, nargs in (("trhip_denoise_default_params", 1), ("trhip_denoise", 8), ("trhip_denoise_device", 8)):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in T._ffi.SIGNATURES and len(T._ffi.SIGNATURES[name][1]) == nargs
        assert getattr(T.lib(), name) is not None
    assert T.lib().trhip_version() == 3001


def test_default_params_need_no_context(T):
    p = T._ffi.DenoiseParams()
    p.reserved = 7
    assert T.lib().trhip_denoise_default_params(C.byref(p)) == 0
    assert (p.iterations, p.flags, p.reserved) == (5, T._ffi.DENOISE_DEMODULATE, 0)
    assert p.albedo_floor == 1.0 / 64.0 and p.min_coverage == 0.5
    for s in (p.sigma_colour, p.sigma_normal, p.sigma_plane):
        assert np.isfinite(s) and s > 0
    assert T.lib().trhip_denoise_default_params(None) == -1
    d = T.Denoiser(iterations=2, demodulate=False, sigma_plane=0.5)  # unspecified fields come from the defaults
    assert (d.params.iterations, d.params.flags, d.params.sigma_plane) == (2, 0, 0.5)
    assert bits(d.params.sigma_colour) == bits(p.sigma_colour) and bits(d.params.sigma_normal) == bits(p.sigma_normal)


PRM = dm.Params(sigma_colour=0.6, sigma_normal=0.02, sigma_plane=0.1)


def test_model_zero_iterations_returns_the_input_bits():
    B, P, _ = dm.synthetic(H, W, 11)
    out = dm.denoise(B, P, dm.Params(0.6, 0.02, 0.1, iterations=0))
    assert np.array_equal(bits(out), bits(B))


def test_model_leaves_weights_and_non_surface_pixels_alone():
    B, P, poisoned = dm.synthetic(H, W, 12)
    assert B[poisoned[0]][3] == 0 and P[poisoned[1]][1, 3] < 0 and np.isnan(P[poisoned[2]][2]).any()
    for demodulate in (True, False):
        prm = dm.Params(0.6, 0.02, 0.1, iterations=4, demodulate=demodulate)
        out = dm.denoise(B, P, prm)
        surface = dm.surface_mask(B, P, prm)
        assert not any(surface[y, x] for y, x in poisoned)
        assert 30 < (~surface).sum() < surface.sum()
        assert np.array_equal(bits(out[..., 3]), bits(B[..., 3]))
        assert np.array_equal(bits(out[~surface]), bits(B[~surface]))
        changed = (bits(out[surface][:, :3]) != bits(B[surface][:, :3])).any(-1)
        assert changed.mean() > 0.9, "the filter must act on the surface pixels"
        assert np.isfinite(out[surface]).all()


def test_model_does_not_filter_across_an_edge():
    """Two half-images with perpendicular normals and different constant colours: every neighbour across the edge weighs exactly 0, so a pixel averages copies of its own value.
    Nothing may move by more than 25 * 2^-22 relative (25 taps; colour-space round trip included), and so nothing crosses the edge."""
    h, w = H, W
    left = np.arange(w)[None, :] < w // 2
    left = np.broadcast_to(left, (h, w))
    n = np.where(left[..., None], F([0, 0, 1]), F([1, 0, 0])).astype(F)
    ys, xs = np.mgrid[0:h, 0:w]
    p = np.where(left[..., None], np.stack([xs, ys, 0 * xs], -1), np.stack([0 * xs + w // 2, ys, xs - w // 2], -1)).astype(F) * F(0.125)
    albedo = np.where(left[..., None], F([0.75, 0.5, 0.25]), F([0.25, 0.5, 0.875])).astype(F)
    xyz = np.where(left[..., None], F([0.5, 0.625, 0.25]), F([1.5, 1.25, 2.0])).astype(F)
    wt = np.full((h, w), F(1.25))
    B = np.concatenate([xyz * wt[..., None], wt[..., None]], -1).astype(F)
    P = dm.planes_of(n, p, albedo, wt, wt)
    for demodulate in (True, False):
        prm = dm.Params(sigma_colour=4.0, sigma_normal=0.5, sigma_plane=100.0, iterations=5, demodulate=demodulate)
        tally = {}
        out = dm.denoise(B, P, prm, tally)
        assert dm.surface_mask(B, P, prm).all()
        assert tally["normal"][0] > 0, "pairs across the edge exist and weigh exactly 0"
        rel = np.abs(out[..., :3].astype(np.float64) - B[..., :3]) / np.abs(B[..., :3])
        assert rel.max() <= 25 * 2.0 ** -22, rel.max()
        # a left pixel stays nearer to the left colour than to the right one by orders of magnitude: nothing crossed
        assert np.abs(out[left][:, :3] / F(1.25) - F([0.5, 0.625, 0.25])).max() < 1e-4 and np.abs(out[~left][:, :3] / F(1.25) - F([1.5, 1.25, 2.0])).max() < 1e-4


def test_model_reduces_the_variance_of_a_flat_region():
    h, w = H, W
    rng = np.random.default_rng(5)
    ys, xs = np.mgrid[0:h, 0:w]
    n = np.broadcast_to(F([0, 0, 1]), (h, w, 3)).astype(F)
    p = np.stack([xs, ys, 0 * xs], -1).astype(F) * F(0.125)
    albedo = np.full((h, w, 3), F(0.5))
    wt = np.ones((h, w), F)
    rgb = (F(0.5) + rng.normal(0.0, 0.1, (h, w, 3))).astype(F)
    B = np.concatenate([dm.rgb_to_xyz(rgb), wt[..., None]], -1).astype(F)
    P = dm.planes_of(n, p, albedo, wt, wt)
    out = dm.denoise(B, P, dm.Params(sigma_colour=4.0, sigma_normal=0.5, sigma_plane=1.0, iterations=3))
    for ch in range(3):
        assert out[..., ch].var() < 0.25 * B[..., ch].var(), ch
    assert abs(out[..., 1].mean() - B[..., 1].mean()) < 0.02


def test_model_weights_take_both_kinds_of_value_on_the_synthetic_inputs():
    """What the GPU comparison relies on: with these sigmas each of the three weights is exactly 0 for some pairs and strictly between 0 and 1 for others."""
    B, P, _ = dm.synthetic(H, W, 13)
    tally = {}
    dm.denoise(B, P, dm.Params(PRM.sigma_colour, PRM.sigma_normal, PRM.sigma_plane, iterations=3), tally)
    for name in ("normal", "plane", "colour"):
        assert tally[name][0] > 50 and tally[name][1] > 50, (name, tally[name])
