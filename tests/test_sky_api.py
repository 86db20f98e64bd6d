"""The environment map and the sky-lit frame (trhip_env, trhip_render_sky; docs/design/25-sky.md), the part that needs no GPU: the numpy model of the lookup (tests/sky_model.py)
against the properties the specification promises — a constant map returns its constant in every bit, directions without a lookup return +0, a direction through a texel
centre returns that texel, the gutter is the octahedral edge wrap and the lookup is continuous across the four edges —, the cancelled cosine pdf against a quadrature, every
refusal that needs no device, the default parameters, the parameter block's layout, the Julia file and its manifest, and the Python classes' argument checks."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import julia_replay as jr
import sky_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = -1  # TRHIP_ERR_INVALID
SIZES = [1, 2, 7, 64]
SKY_SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPSky.jl")
MANIFEST = os.path.join(ROOT, "tests", "golden", "julia_shim_sky_calls.json")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def header():
    return open(os.path.join(ROOT, "include", "tracehip.h")).read()


# ---- the model of the lookup --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_a_constant_map_returns_its_constant_in_every_bit(n, turned):
    dirs = sm.adversarial_directions(1000)
    assert dirs.shape == (1000, 3) and np.isfinite(dirs).all()
    assert (np.signbit(dirs) & (dirs == 0)).any() and ((dirs != 0) & (np.abs(dirs) < np.finfo(F).tiny)).any(), "-0 components and denormals are in the set"
    rgb = F([0.1, 1.7, 3.0e-5])
    out = sm.env_eval(np.broadcast_to(rgb, (n, n, 3)), dirs, sm.rotation() if turned else None)
    assert np.array_equal(bits(out), np.broadcast_to(bits(rgb), out.shape))


@pytest.mark.parametrize("n", SIZES)
def test_directions_without_a_lookup_return_plus_zero(n):
    inf, nan = np.inf, np.nan
    dirs = F([[0, 0, 0], [-0.0, 0, -0.0], [inf, 0, 0], [0, -inf, 1], [inf, inf, -inf], [nan, 0, 1], [1, nan, 0], [0, 1, nan], [nan, nan, nan], [3e38, 3e38, 3e38]])
    for R in (None, sm.rotation()):
        out = sm.env_eval(sm.random_map(n) + F(1.0), dirs, R)
        assert not bits(out).any(), "+0 in every bit"


@pytest.mark.parametrize("n", SIZES)
def test_a_direction_through_a_texel_centre_returns_that_texel(n):
    t = sm.random_map(n)
    d = sm.centre_directions(n).reshape(-1, 3)
    ok, fx, fy = sm.coords(d, n)
    assert ok.all()
    j, i = np.divmod(np.arange(n * n), n)
    exact = (fx == i) & (fy == j)  # the reconstructed coordinates are integral, and the texel's own
    assert exact.any()
    if n in (1, 2, 64):
        assert exact.all(), "every centre of a power-of-two map is exact in Float32"
    out = sm.env_eval(t, d)
    assert np.array_equal(bits(out[exact]), bits(t.reshape(-1, 3)[exact]))
    assert np.abs(out - t.reshape(-1, 3)).max() <= 4.0 * n * 2.0 ** -22, "the others are within the rounding of fx, fy times the map's range"


def wrapped_texel(t, i, j):
    """The octahedral map continued over the edges of its square, from the geometry: crossing a vertical edge mirrors the row, crossing a horizontal edge the column."""
    n = t.shape[0]
    if i < 0 or i >= n:
        i, j = (-1 - i if i < 0 else 2 * n - 1 - i), n - 1 - j
    if j < 0 or j >= n:
        i, j = n - 1 - i, (-1 - j if j < 0 else 2 * n - 1 - j)
    return t[j, i]


@pytest.mark.parametrize("n", SIZES)
def test_the_gutter_is_the_octahedral_edge_wrap(n):
    t = sm.random_map(n)
    st = sm.gutter(t)
    assert st.shape == (n + 2, n + 2, 3) and st.dtype == F
    assert np.array_equal(st[1:-1, 1:-1], t)
    for j in range(-1, n + 1):
        for i in range(-1, n + 1):
            assert np.array_equal(st[j + 1, i + 1], wrapped_texel(t, i, j)), (i, j)
    # the rule as the header states it, on the four sides and one corner
    last = n - 1
    assert np.array_equal(st[1:-1, 0], t[::-1, 0]) and np.array_equal(st[1:-1, n + 1], t[::-1, last])
    assert np.array_equal(st[0, 1:-1], t[0, ::-1]) and np.array_equal(st[n + 1, 1:-1], t[last, ::-1])
    assert np.array_equal(st[0, 0], t[last, last]) and np.array_equal(st[0, n + 1], t[last, 0])


@pytest.mark.parametrize("n", SIZES)
def test_the_lookup_is_continuous_across_the_four_edges(n):
    """A point ON an edge of the square is reached from two sides: the lower-hemisphere direction whose vanishing component is +tiny lands at (edge, q), the one with -tiny at
    (edge, -q) — the same direction in the limit, the two ends of the wrap.  Both read the gutter (x0 = -1 or n - 1, tx = 1/2 exactly) and must agree.  In exact
    arithmetic they do (the four texels are the same, the weights mirrored); in Float32 fy and n - 1 - fy each carry three roundings of at most ulp(n) / 2, so the two ty
    differ from mirror images by at most 6 n 2^-24, and the three nested lerps of each side round by at most 3 ulp(M) for texels in [0, M]:
    |difference| <= (6 n 2^-24 + 6 2^-23) M = (3 n + 6) 2^-23 M."""
    t = sm.random_map(n)
    M = float(t.max())
    tol = (3 * n + 6) * 2.0 ** -23 * M
    tiny = F(1e-30)
    a = np.linspace(0.05, 0.95, 19).astype(F)
    b = (F(1.0) - a).astype(F)
    worst = 0.0
    for axis in (0, 1):
        for sign in (-1.0, 1.0):
            d = np.zeros((a.size, 3), F)
            d[:, axis], d[:, 2] = F(sign) * a, -b
            plus, minus = d.copy(), d.copy()
            plus[:, 1 - axis], minus[:, 1 - axis] = tiny, -tiny
            _, fx, fy = sm.coords(plus, n)
            on_edge = (fx, fy)[axis]
            assert np.all(on_edge == (F(-0.5) if sign < 0 else F(n - 0.5))), "the points lie on the edge: the lookup reads the gutter"
            _, gx, gy = sm.coords(minus, n)
            assert np.allclose((fx, fy)[1 - axis] + (gx, gy)[1 - axis], n - 1, atol=1e-3), "the two ends of the wrap"
            worst = max(worst, float(np.abs(sm.env_eval(t, plus) - sm.env_eval(t, minus)).max()))
    print(f"n = {n}: largest difference across an edge {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol


def test_just_inside_and_just_outside_an_edge_read_the_same_texels():
    """Just inside an edge the lookup blends an interior column with the gutter; the gutter rule makes that the blend a map continued by wrapped_texel gives in Float64."""
    n = 7
    t = sm.random_map(n)
    eps = 2.0 ** -12
    for axis in (0, 1):
        for sign in (-1.0, 1.0):
            q = np.linspace(-0.9, 0.9, 12)  # (an even count: no point at q = 0, which is the upper hemisphere's)
            p = np.empty((q.size, 2))
            p[:, axis], p[:, 1 - axis] = sign * (1.0 - eps), q
            # inverse map of a point outside the diamond: the lower hemisphere
            z = 1.0 - np.abs(p[:, 0]) - np.abs(p[:, 1])
            assert (z < 0).all()
            x = (1.0 - np.abs(p[:, 1])) * np.where(p[:, 0] < 0, -1.0, 1.0)
            y = (1.0 - np.abs(p[:, 0])) * np.where(p[:, 1] < 0, -1.0, 1.0)
            got = sm.env_eval(t, np.stack([x, y, z], axis=1).astype(F)).astype(np.float64)
            f = (p * 0.5 + 0.5) * n - 0.5
            i0, j0 = np.floor(f[:, 0]).astype(int), np.floor(f[:, 1]).astype(int)
            tx, ty = (f[:, 0] - i0)[:, None], (f[:, 1] - j0)[:, None]
            assert np.all((i0 == -1) | (i0 == n - 1) | (j0 == -1) | (j0 == n - 1)), "the blend reaches into the gutter"
            tex = lambda di, dj: np.array([wrapped_texel(t, i + di, j + dj) for i, j in zip(i0, j0)], np.float64)
            ref = (tex(0, 0) * (1 - tx) + tex(1, 0) * tx) * (1 - ty) + (tex(0, 1) * (1 - tx) + tex(1, 1) * tx) * ty
            assert np.abs(got - ref).max() <= 4.0 * n * 2.0 ** -22, "Float32 rounding of the coordinates times the map's range (4)"


# ---- the frame's model ----------------------------------------------------------------------------------------------------------------------
def ground_scene(T):
    """Two triangles: a square in the plane y = 0 facing up, nothing above it."""
    white = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(1.0)), T.ConstantTexture(0.0))
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    tris = T.create_triangle_mesh(core, 2, np.array([1, 2, 3, 1, 3, 4], dtype=np.uint32), 4, [[-1, 0, 1], [1, 0, 1], [1, 0, -1], [-1, 0, -1]], [[0, 1, 0]] * 4)
    return T.Scene([], T.BVHAccel([T.GeometricPrimitive(tr, white) for tr in tris], 1))


def test_the_cosine_pdf_cancels(T, ob):
    """The mean contribution of cosine-distributed rays is the cosine-weighted integral of the environment over the hemisphere, divided by pi: 4096 samples of one pixel
    on open ground under a gradient sky, against a quadrature of env_eval * cos / pi (256 x 256 cells in (cos^2 theta, phi), where that measure is uniform)."""
    scene = ground_scene(T)
    env = T.Environment.gradient((0.1, 0.3, 1.0), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1), up=(0.2, 1.0, -0.1), n=64)
    film = T.Film([1, 1], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    # a camera close to the ground: the hit point's rounding (2^-24 of a distance of 0.014) stays far below spawn_ray's 1e-6 offset, so no occlusion ray starts under the plane
    cam = T.PerspectiveCamera(T.look_at([0, 0.01, 0.01], [0, 0, 0], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 20.0, film)
    r = sm.render(ob.OracleScene.from_scene(scene), cam, 4096, 0x5C1, env.texels, env.world_to_env)
    assert r.cls.shape[0] == 4096
    sb = film.get_sample_bounds()
    y, x = -int(sb.p_min[1]), -int(sb.p_min[0])  # the film's one pixel inside the sample bounds
    c = r.c[:, y, x].astype(np.float64)
    assert np.all(r.cls[:, y, x] == sm.OPEN), "every sample hits the ground and its ray escapes"
    assert np.array_equal(r.L[:, y, x], r.c[:, y, x])
    mean, sem = c.mean(axis=0), c.std(axis=0, ddof=1) / math.sqrt(c.shape[0])
    m = 256
    mu2, phi = np.meshgrid((np.arange(m) + 0.5) / m, (np.arange(m) + 0.5) / m * 2.0 * np.pi, indexing="ij")
    cos_t, sin_t = np.sqrt(mu2), np.sqrt(1.0 - mu2)
    dirs = np.stack([sin_t * np.cos(phi), cos_t, sin_t * np.sin(phi)], axis=-1).reshape(-1, 3)  # the hemisphere about the ground's normal, +y
    quad = sm.env_eval(env.texels, dirs.astype(F), env.world_to_env).astype(np.float64).mean(axis=0)  # d(cos^2 theta) d(phi) / (2 pi) = cos / pi d(omega)
    print(f"mean c {mean}, quadrature {quad}, standard error {sem}")
    assert np.all(sem > 0)
    assert np.all(np.abs(mean - quad) <= 4.0 * sem)


def test_model_frame_on_the_oracle_alone(T, ob):
    """The frame's model runs end to end without a GPU: under the constant map (1, 1, 1) it is the AO model's frame with background 1, hide_background is background 0,
    scale multiplies, and a scale of 0 is black."""
    import ao_model as am
    scene = T.scenes.cornell_scene()
    film = T.Film([16, 12], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    cam = T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)
    osc = ob.OracleScene.from_scene(scene)
    one = np.ones((1, 1, 3), F)
    assert np.array_equal(bits(sm.render(osc, cam, 2, 0xA0, one).L), bits(am.render(osc, cam, 2, 0xA0, background=1.0).L))
    assert np.array_equal(bits(sm.render(osc, cam, 2, 0xA0, one, hide_background=True).L), bits(am.render(osc, cam, 2, 0xA0).L))
    t = sm.random_map(7)
    full, half, none = (sm.render(osc, cam, 2, 0xA0, t, sm.rotation(), scale=s) for s in (1.0, 0.5, 0.0))
    assert min(am.shares(full.cls)) >= 0.05
    assert np.array_equal(bits(half.L), bits(full.L * F(0.5))) and not bits(none.L).any()
    assert len(np.unique(full.L[full.cls == sm.OPEN], axis=0)) > 10 and len(np.unique(full.L[full.cls == sm.MISS], axis=0)) > 10


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------------------
def test_params_mirror_matches_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_sky_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1)) for m in re.finditer(r"(\w+)\s+(\w+)\s*;", body)]
    assert [n for n, _ in fields] == ["max_distance", "scale", "flags", "reserved"]
    S = T._ffi.SkyParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    assert [(n, ct) for n, ct in S._fields_] == [(n, ctypes_of[t]) for n, t in fields]
    assert C.sizeof(S) == 16 and [getattr(S, n).offset for n, _ in fields] == [0, 4, 8, 12]
    assert re.search(r"#define\s+TRHIP_SKY_ALBEDO\s+1u\b", header()) and T._ffi.SKY_ALBEDO == 1
    assert re.search(r"#define\s+TRHIP_SKY_HIDE_BACKGROUND\s+2u\b", header()) and T._ffi.SKY_HIDE_BACKGROUND == 2


def test_entry_points_are_declared_and_bound(T):
    for name, nargs in (("trhip_env_create", 5), ("trhip_env_free", 1), ("trhip_env_size", 2), ("trhip_env_eval", 5), ("trhip_sky_default_params", 1), ("trhip_render_sky", 10),
                        ("trhip_render_sky_device", 10)):
        assert re.search(r"\b(int|void) " + name + r"\(", header()), name
        assert name in T._ffi.SIGNATURES and len(T._ffi.SIGNATURES[name][1]) == nargs
        assert getattr(T.lib(), name) is not None
    assert T.lib().trhip_version() == 3001


def test_default_params_need_no_context(T):
    p = T._ffi.SkyParams(1.0, 2.0, 3, 4)
    assert T.lib().trhip_sky_default_params(C.byref(p)) == 0
    assert math.isinf(p.max_distance) and p.max_distance > 0
    assert (p.scale, p.flags, p.reserved) == (1.0, 0, 0)
    assert T.lib().trhip_sky_default_params(None) == INVALID


def test_env_create_refusals_need_no_device(T):
    """Everything about the map is checked before the context is looked at: with no context every call is refused, and the message tells which check fired."""
    L = T.lib()
    eye = np.eye(3, dtype=F)
    good = np.ones((2, 2, 3), F)
    h = C.c_void_p()

    def create(texels=good, n=2, R=eye, out=h):
        return L.trhip_env_create(None, T._ffi.fptr(texels) if texels is not None else None, n, T._ffi.fptr(R) if R is not None else None, C.byref(out) if out is not None else None)

    for kw in (dict(texels=None), dict(R=None), dict(out=None)):
        assert create(**kw) == INVALID and b"null argument" in L.trhip_last_error(None), kw
    for n in (0, 4097, 0xFFFFFFFF):
        assert create(n=n) == INVALID and b"n must be" in L.trhip_last_error(None), n
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-45):
        for where in ((0, 0, 0), (1, 0, 2), (1, 1, 1)):
            t = good.copy()
            t[where] = bad
            assert create(texels=t) == INVALID and b"texel" in L.trhip_last_error(None), (bad, where)
    named = good.copy()
    named[0, 1, 2] = -1.0  # row 0, column 1, channel 2
    assert create(texels=named) == INVALID and b"texel (1, 0) channel 2" in L.trhip_last_error(None)
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 4, 8):
            R = eye.copy()
            R.flat[k] = bad
            assert create(R=R) == INVALID and b"world_to_env" in L.trhip_last_error(None), (bad, k)
    zero = np.zeros((2, 2, 3), F)
    zero[0, 0, 0] = -0.0  # -0 is not negative
    assert create(texels=zero) == INVALID and b"null argument" in L.trhip_last_error(None), "a good map without a context stops at the context"
    assert create() == INVALID and b"null argument" in L.trhip_last_error(None)
    assert h.value is None
    L.trhip_env_free(None)  # a no-op
    n = C.c_uint32(7)
    assert L.trhip_env_size(None, C.byref(n)) == INVALID and n.value == 7
    d = np.zeros((1, 3), F)
    assert L.trhip_env_eval(None, None, T._ffi.fptr(d), 1, T._ffi.fptr(d)) == INVALID


BAD_PARAMS = [
    (dict(max_distance=float("nan")), b"max_distance"),
    (dict(max_distance=0.0), b"max_distance"),
    (dict(max_distance=-1.0), b"max_distance"),
    (dict(max_distance=-math.inf), b"max_distance"),
    (dict(scale=-0.5), b"scale"),
    (dict(scale=math.inf), b"scale"),
    (dict(scale=float("nan")), b"scale"),
    (dict(flags=4), b"flag"),
    (dict(flags=0x80000001), b"flag"),
    (dict(reserved=1), b"reserved"),
]


def good_params(T, **over):
    p = T._ffi.SkyParams()
    assert T.lib().trhip_sky_default_params(C.byref(p)) == 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("entry", ["trhip_render_sky", "trhip_render_sky_device"])
def test_invalid_arguments_are_refused_without_a_device(T, entry):
    """trhip_render_ao's order: the parameter block first, then spp, then the handles.  No context exists here, so every call is refused."""
    fn, L = getattr(T.lib(), entry), T.lib()
    sn, st, out = T._ffi.Sensor(), T.Stats(), np.zeros(4, F)
    outp = T._ffi.fptr(out) if entry == "trhip_render_sky" else C.c_void_p(out.ctypes.data)
    for over, word in BAD_PARAMS:
        assert fn(None, None, C.byref(sn), 1, 0, 0, None, C.byref(good_params(T, **over)), outp, C.byref(st)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    for flags in (1, 2, 3):  # the two flags are known
        assert fn(None, None, C.byref(sn), 0, 0, 0, None, C.byref(good_params(T, flags=flags)), outp, C.byref(st)) == INVALID and b"spp" in L.trhip_last_error(None)
    assert fn(None, None, C.byref(sn), 1, 0, 0, None, None, outp, C.byref(st)) == INVALID  # no parameter block
    assert fn(None, None, C.byref(sn), 1, 0, 0, None, C.byref(good_params(T)), outp, C.byref(st)) == INVALID  # null context and scene
    assert b"null argument" in L.trhip_last_error(None)
    assert not out.any()


# ---- the Julia file ------------------------------------------------------------------------------------------------------------------------
def test_every_sky_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SKY_SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPSky.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    for need in ("trhip_env_create", "trhip_env_free", "trhip_env_eval", "trhip_sky_default_params", "trhip_render_sky", "trhip_render_sky_device", "trhip_film_reduce", "trhip_scene_free"):
        assert need in calls, need


def test_sky_params_mirror_the_header(T):
    src = open(SKY_SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipSkyParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::(\w+)", body, re.M)
    ct = {"Float32": C.c_float, "UInt32": C.c_uint32}
    assert [(n, ct[t]) for n, t in fields] == list(T._ffi.SkyParams._fields_)
    assert sum(C.sizeof(ct[t]) for _, t in fields) == C.sizeof(T._ffi.SkyParams) == 16
    assert int(re.search(r"const TRHIP_SKY_ALBEDO = UInt32\((\d+)\)", src).group(1)) == T._ffi.SKY_ALBEDO
    assert int(re.search(r"const TRHIP_SKY_HIDE_BACKGROUND = UInt32\((\d+)\)", src).group(1)) == T._ffi.SKY_HIDE_BACKGROUND


def test_sky_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SKY_SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPSky.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPSky.jl changed: bring tests/golden/julia_shim_sky_calls.json in step with its ccalls"


def test_the_shim_includes_the_sky_file_inside_its_module():
    """After the AO file, whose frame it extends, and after every name it uses.  (It is the last include but one: tests/test_julia_shim_adaptive.py pins TraceHIPAdaptive.jl,
    which it neither uses nor is used by, as the last.)"""
    src = open(jr.SHIM, encoding="utf-8").read()
    at = src.index('include("TraceHIPSky.jl")')
    assert src.index("module TraceHIP") < src.index('include("TraceHIPAO.jl")') < src.index('include("TraceHIPDirectSplit.jl")') < at < src.rindex("end # module")
    assert [m.start() for m in re.finditer(r'^include\("', src, re.M)][-2] == at
    for name in ("mutable struct TrhipStats", "function context()", "check(rc) =", "function flatten(", "function sensor(", "seed_of(", "const JOB", "function shard_samples(",
                 "function write_film!("):
        assert 0 <= src.index(name) < at, name
    # TraceHIP.jl's own ccalls are what its manifest says: the include adds none
    own = json.load(open(os.path.join(ROOT, "tests", "golden", "julia_shim_calls.json")))
    assert own["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(jr.parse_ccalls(jr.SHIM).items())}


# ---- the Python classes ----------------------------------------------------------------------------------------------------------------------
def camera(T):
    film = T.Film([16, 12], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def test_environment_validates_its_arguments(T):
    e = T.Environment(np.ones((4, 4, 3)))
    assert e.n == 4 and e.texels.dtype == F and e.texels.flags.c_contiguous and np.array_equal(e.world_to_env, np.eye(3, dtype=F))
    assert T.Environment([[[1, 2, 3]]]).n == 1
    for bad in (np.ones((4, 3, 3)), np.ones((4, 4)), np.ones((4, 4, 4)), np.ones((0, 0, 3)), np.full((2, 2, 3), np.nan), np.full((2, 2, 3), np.inf), np.full((2, 2, 3), -1.0)):
        with pytest.raises(T.TraceHipError):
            T.Environment(bad)
    with pytest.raises(T.TraceHipError):
        T.Environment(np.broadcast_to(F(1.0), (4097, 4097, 3)))
    for bad in (np.eye(4), np.ones(9), np.full((3, 3), np.nan), np.full((3, 3), np.inf)):
        with pytest.raises(T.TraceHipError):
            T.Environment(np.ones((2, 2, 3)), bad)
    with pytest.raises(T.TraceHipError):
        e.eval(np.zeros((5, 2)), ctx=object())  # the shape is checked before the context is touched


def test_environment_constructors(T):
    c = T.Environment.constant((0.25, 0.5, 2.0))
    assert c.n == 1 and np.array_equal(c.texels, F([[[0.25, 0.5, 2.0]]]))
    zen, hor, gnd = (0.1, 0.3, 1.0), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1)
    g = T.Environment.gradient(zen, hor, gnd)
    assert g.n == 64 and g.texels.min() >= 0
    up, down, side = F([[0, 0, 1]]), F([[0, 0, -1]]), F([[1, 0, 0], [0, -1, 0], [-1, 1, 0]])
    # a 64 x 64 map has no texel centre at the poles or on the horizon: within a texel's width of the gradient (the colours differ by < 1, directions by < 2 / 64 * 2)
    assert np.abs(sm.env_eval(g.texels, up) - F(zen)).max() < 0.07 and np.abs(sm.env_eval(g.texels, down) - F(gnd)).max() < 0.07
    assert np.abs(sm.env_eval(g.texels, side) - F(hor)).max() < 0.07
    gy = T.Environment.gradient(zen, hor, gnd, up=(0, 2, 0), n=32)
    assert gy.n == 32 and np.abs(sm.env_eval(gy.texels, F([[0, 1, 0]])) - F(zen)).max() < 0.13
    d = T.octahedral_directions(8)
    assert d.shape == (8, 8, 3) and np.allclose(np.linalg.norm(d, axis=-1), 1.0)
    _, fx, fy = sm.coords(d.reshape(-1, 3), 8)
    j, i = np.divmod(np.arange(64), 8)
    assert np.abs(fx - i).max() < 1e-4 and np.abs(fy - j).max() < 1e-4, "the inverse map lands on the texel centres of the lookup"
    for kw in (dict(up=(0, 0, 0)), dict(up=(1, 2)), dict(up=(np.nan, 0, 1)), dict(n=0), dict(n=5000)):
        with pytest.raises(T.TraceHipError):
            T.Environment.gradient(zen, hor, gnd, **kw)
    # a latitude-longitude image: rows are bands of latitude (zenith first), columns run in azimuth from +x towards +y
    img = np.zeros((8, 16, 3))
    img[:4, :, 2] = 1.0   # the upper hemisphere is blue
    img[4:, :, 0] = 0.5   # the lower one red
    img[:, :4, 1] = 0.25  # azimuth 0 .. 90 degrees carries green
    e = T.Environment.from_latlong(img, n=16)
    assert e.n == 16 and T.Environment.from_latlong(img).n == 8
    assert np.allclose(sm.env_eval(e.texels, F([[0.1, 0.1, 1.0]])), [[0, 0.25, 1.0]], atol=0.02)
    assert np.allclose(sm.env_eval(e.texels, F([[-0.1, -0.1, -1.0]])), [[0.5, 0, 0]], atol=0.02)
    assert np.allclose(sm.env_eval(e.texels, F([[-1.0, 1.0, 0.5]])), [[0, 0, 1.0]], atol=0.02)
    for bad in (np.zeros((4, 4)), np.zeros((4, 4, 4)), np.zeros((0, 4, 3))):
        with pytest.raises(T.TraceHipError):
            T.Environment.from_latlong(bad)
    with pytest.raises(T.TraceHipError):
        T.Environment.from_latlong(-np.ones((4, 8, 3)))


def test_sky_integrator_validates_its_arguments(T):
    cam, smp, env = camera(T), T.SeededSampler(3, seed=1), T.Environment.constant((1, 1, 1))
    a = T.SkyIntegrator(cam, smp, env)
    assert math.isinf(a.params.max_distance) and (a.params.scale, a.params.flags, a.params.reserved) == (1.0, 0, 0) and a.environment is env
    b = T.SkyIntegrator(cam, smp, env, max_distance=0.5, albedo=True, scale=0.25, hide_background=True)
    assert (b.params.max_distance, b.params.scale, b.params.flags, b.params.reserved) == (0.5, 0.25, T._ffi.SKY_ALBEDO | T._ffi.SKY_HIDE_BACKGROUND, 0)
    assert T.SkyIntegrator(cam, smp, env, hide_background=True).params.flags == T._ffi.SKY_HIDE_BACKGROUND and T.SkyIntegrator(cam, smp, env, scale=0).params.scale == 0.0
    assert isinstance(b, T.api._SamplerIntegrator) and callable(b) and hasattr(b, "sample_radiance")
    for kw in (dict(max_distance=0.0), dict(max_distance=-2.0), dict(max_distance=float("nan")), dict(scale=-1.0), dict(scale=math.inf), dict(scale=float("nan"))):
        with pytest.raises(T.TraceHipError):
            T.SkyIntegrator(cam, smp, env, **kw)
    for bad in (None, np.ones((1, 1, 3)), (1, 1, 1)):
        with pytest.raises(T.TraceHipError):
            T.SkyIntegrator(cam, smp, bad)
