"""The ambient-occlusion integrator, the part that needs no GPU: the parameter block's layout (header text == ctypes mirror, 16 bytes), the entry points, the default parameters,
the refusals (the parameter block is checked before any handle, so the message tells which check fired even without a device), the Python class's own checks, and the
properties of the numpy model (tests/ao_model.py) the kernels are compared with bit for bit in tests/test_gpu_ao.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ao_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = -1  # TRHIP_ERR_INVALID


def header():
    return open(os.path.join(ROOT, "include", "tracehip.h")).read()


def test_params_mirror_matches_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_ao_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]
    assert [n for n, _ in fields] == ["max_distance", "background", "flags", "reserved"]
    S = T._ffi.AoParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    assert [(n, ct) for n, ct in S._fields_] == [(n, ctypes_of[t]) for n, t in fields]
    assert C.sizeof(S) == 16
    assert [getattr(S, n).offset for n, _ in fields] == [0, 4, 8, 12]
    assert re.search(r"#define\s+TRHIP_AO_ALBEDO\s+1u?\b", header()) and T._ffi.AO_ALBEDO == 1


def test_entry_points_are_declared_and_bound(T):
    for name, nargs in (("trhip_ao_default_params", 1), ("trhip_render_ao", 9), ("trhip_render_ao_device", 9)):
        assert re.search(r"\bint " + name + r"\(", header()), name
        assert name in T._ffi.SIGNATURES and len(T._ffi.SIGNATURES[name][1]) == nargs
        assert getattr(T.lib(), name) is not None
    assert T.lib().trhip_version() == 3001


def test_default_params_need_no_context(T):
    p = T._ffi.AoParams(1.0, 2.0, 3, 4)
    assert T.lib().trhip_ao_default_params(C.byref(p)) == 0
    assert math.isinf(p.max_distance) and p.max_distance > 0
    assert (p.background, p.flags, p.reserved) == (0.0, 0, 0)
    assert T.lib().trhip_ao_default_params(None) == INVALID


BAD_PARAMS = [
    (dict(max_distance=float("nan")), b"max_distance"),
    (dict(max_distance=0.0), b"max_distance"),
    (dict(max_distance=-1.0), b"max_distance"),
    (dict(max_distance=-math.inf), b"max_distance"),
    (dict(background=-0.5), b"background"),
    (dict(background=math.inf), b"background"),
    (dict(background=float("nan")), b"background"),
    (dict(flags=2), b"flag"),
    (dict(flags=0x80000001), b"flag"),
    (dict(reserved=1), b"reserved"),
]


def good_params(T, **over):
    p = T._ffi.AoParams()
    assert T.lib().trhip_ao_default_params(C.byref(p)) == 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("entry", ["trhip_render_ao", "trhip_render_ao_device"])
def test_invalid_arguments_are_refused_without_a_device(T, entry):
    """No context exists here, so every call is refused; the parameter block is checked first, and the message (kept for trhip_last_error(NULL)) names the field."""
    fn, L = getattr(T.lib(), entry), T.lib()
    sn, st, out = T._ffi.Sensor(), T.Stats(), np.zeros(4, F)
    outp = T._ffi.fptr(out) if entry == "trhip_render_ao" else C.c_void_p(out.ctypes.data)
    for over, word in BAD_PARAMS:
        assert fn(None, None, C.byref(sn), 1, 0, 0, C.byref(good_params(T, **over)), outp, C.byref(st)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    assert fn(None, None, C.byref(sn), 1, 0, 0, None, outp, C.byref(st)) == INVALID  # no parameter block
    assert fn(None, None, C.byref(sn), 0, 0, 0, C.byref(good_params(T)), outp, C.byref(st)) == INVALID
    assert b"spp" in L.trhip_last_error(None)
    assert fn(None, None, C.byref(sn), 1, 0, 0, C.byref(good_params(T)), outp, C.byref(st)) == INVALID  # null context and scene
    assert b"null argument" in L.trhip_last_error(None)
    assert not out.any()


def camera(T):
    film = T.Film([16, 12], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def test_python_class_validates_its_arguments(T):
    cam, smp = camera(T), T.SeededSampler(3, seed=1)
    a = T.AmbientOcclusionIntegrator(cam, smp)
    assert math.isinf(a.params.max_distance) and (a.params.background, a.params.flags, a.params.reserved) == (0.0, 0, 0)
    b = T.AmbientOcclusionIntegrator(cam, smp, max_distance=0.5, albedo=True, background=0.25)
    assert (b.params.max_distance, b.params.background, b.params.flags, b.params.reserved) == (0.5, 0.25, T._ffi.AO_ALBEDO, 0)
    assert isinstance(b, T.api._SamplerIntegrator) and callable(b) and hasattr(b, "sample_radiance")
    for kw in (dict(max_distance=0.0), dict(max_distance=-2.0), dict(max_distance=float("nan")), dict(background=-1.0), dict(background=math.inf), dict(background=float("nan"))):
        with pytest.raises(T.TraceHipError):
            T.AmbientOcclusionIntegrator(cam, smp, **kw)


def random_frames(n, seed):
    rng = np.random.default_rng(seed)
    ns = rng.normal(size=(n, 3))
    ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(F)
    wo = rng.normal(size=(n, 3))
    wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(F)
    u = (rng.integers(0, 1 << 24, size=(n, 2)).astype(F) * F(2.0 ** -24)).astype(F)  # what ts_uniform returns: multiples of 2^-24 in [0, 1)
    return ns, wo, u


def test_model_directions_lie_in_the_hemisphere_and_have_unit_length(T):
    ns, wo, u = random_frames(4096, 3)
    # axis-aligned normals (both branches of coordinate_system, zero components) and the corners and centre of the unit square
    ns[:6] = F([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])
    u[:5] = F([[0, 0], [0.5, 0.5], [1 - 2.0 ** -24, 0], [0, 1 - 2.0 ** -24], [1 - 2.0 ** -24, 1 - 2.0 ** -24]])
    nf, wi = am.directions(ns, wo, u)
    assert nf.dtype == wi.dtype == F and np.isfinite(wi).all()
    d64 = lambda a, b: (a.astype(np.float64) * b.astype(np.float64)).sum(axis=1)
    assert np.all(d64(nf, wo) >= 0), "nf faces the viewer"
    assert np.array_equal(np.abs(nf), np.abs(ns))
    assert np.all(d64(wi, nf) >= 0)
    assert np.abs(np.sqrt(d64(wi, wi)) - 1.0).max() < 1e-5
    assert np.array_equal(wi[1], nf[1]), "u = (0.5, 0.5) is the pole"
    # cosine-distributed: E[wi . nf] = 2/3 (standard error 0.24 / sqrt(n) = 0.004)
    assert abs(d64(wi, nf)[6:].mean() - 2.0 / 3.0) < 0.02


def test_model_classes_on_the_oracle_alone(T, ob):
    """The model runs end to end without a GPU (the reference's own tree); every class holds at least 5 % of the samples of the frame the GPU tests use, and a finite reach
    opens rays that an infinite one finds occluded, never the reverse."""
    scene, cam = T.scenes.cornell_scene(), camera(T)
    osc = ob.OracleScene.from_scene(scene)
    far = am.render(osc, cam, 3, 0xA0)
    near = am.render(osc, cam, 3, 0xA0, max_distance=0.3)
    assert min(am.shares(far.cls)) >= 0.05 and min(am.shares(near.cls)) >= 0.05
    assert np.array_equal(far.hit, near.hit)
    assert not ((near.cls == am.OCCLUDED) & (far.cls == am.OPEN)).any()
    assert ((near.cls == am.OPEN) & (far.cls == am.OCCLUDED)).sum() >= 0.05 * far.hit.sum()
    assert set(np.unique(far.L)) == {0.0, 1.0} and np.array_equal(far.L[far.cls == am.OPEN], np.ones((int((far.cls == am.OPEN).sum()), 3), F))
    bg = am.render(osc, cam, 3, 0xA0, background=0.25)
    assert np.all(bg.L[bg.cls == am.MISS] == F(0.25)) and np.array_equal(bg.L[bg.hit], far.L[far.hit])
    # shards: the samples of (spp 1, offset 2) are the third sample pass of (spp 3, offset 0)
    third = am.render(osc, cam, 1, 0xA0, sample_offset=2)
    assert np.array_equal(third.L[0], far.L[2]) and np.array_equal(third.cls[0], far.cls[2])
