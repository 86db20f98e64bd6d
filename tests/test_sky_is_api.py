"""Importance sampling of the environment map and the importance-sampled sky frame (trhip_env_make_sampler, trhip_render_sky_is; docs/design/27-sky-importance.md), the part
that needs no GPU: the numpy model (tests/sky_is_model.py) against the properties the specification promises — monotone tables, the Jacobian's integral, the symmetries of
a constant map, the sampler at the ends of [0, 1), on table entries, on maps with one texel, a corner texel and empty rows, the round trip through env_pdf —, the
estimator's statistics (unbiased, lower variance, bounded), every refusal that needs no device, the defaults, the parameter block's layout, the Julia file and its
manifest, and the Python classes' argument checks."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import ao_model as am
import julia_replay as jr
import sky_is_model as im
import sky_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = -1  # TRHIP_ERR_INVALID
SIZES = [1, 2, 7, 64]
SHIM = os.path.join(os.path.dirname(jr.SHIM), "TraceHIPSkyIS.jl")
MANIFEST = os.path.join(ROOT, "tests", "golden", "julia_shim_sky_is_calls.json")


def header():
    return open(os.path.join(ROOT, "include", "tracehip.h")).read()


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_tables_are_monotone_and_end_at_one(n):
    for t in (sm.random_map(n), im.test_map(n), np.ones((n, n, 3), F)):
        tab = im.tables(t)
        assert tab.m.dtype == tab.c.dtype == F and tab.m.shape == (n + 1,) and tab.c.shape == (n, n + 1) and tab.flat().size == (n + 1) * (n + 1)
        assert tab.m[0] == 0 and tab.m[n] == 1 and np.all(np.diff(tab.m) >= 0)
        assert np.all(tab.c[:, 0] == 0) and np.all(tab.c[:, n] == 1) and np.all(np.diff(tab.c, axis=1) >= 0)
    assert im.tables(np.zeros((n, n, 3), F)) is None, "a map whose weights are all zero has no tables"


def test_the_jacobian_integrates_to_the_sphere():
    rel = abs(float((im.jacobian(64) * 4.0 / 64 ** 2).sum()) / (4.0 * math.pi) - 1.0)
    print(f"sum J 4 / n^2 against 4 pi at n = 64: {rel:.2e} relative")
    assert rel <= 1e-6


@pytest.mark.parametrize("n", SIZES)
def test_a_constant_map_is_symmetric_under_the_octahedrons_reflections(n):
    """x -> -x and y -> -y mirror the square's columns and rows, x <-> y transposes it: the weights of a constant map are unchanged by all three, so its marginal's steps
    are a palindrome, every row's steps are, and row j's steps are row n - 1 - j's.  (The steps are differences of rounded prefix sums taken from one end, so they agree to
    the rounding of the tables, 2^-24 each, not bit for bit.)"""
    tab = im.tables(np.full((n, n, 3), 0.7, F))
    assert np.allclose(tab.w, tab.w[::-1], rtol=1e-14) and np.allclose(tab.w, tab.w[:, ::-1], rtol=1e-14) and np.allclose(tab.w, tab.w.T, rtol=1e-14)
    dm, dc = np.diff(tab.m.astype(np.float64)), np.diff(tab.c.astype(np.float64), axis=1)
    tol = 2.0 ** -22
    assert np.abs(dm - dm[::-1]).max() <= tol and np.abs(dc - dc[:, ::-1]).max() <= tol and np.abs(dc - dc[::-1]).max() <= tol
    assert np.abs((tab.m[None, :].astype(np.float64) + tab.m[::-1][None, :]) - 1.0).max() <= tol


# ---- env_sample ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("turned", [False, True], ids=["identity", "turned"])
def test_sampled_directions_are_unit_and_have_a_density(n, turned):
    R = sm.rotation() if turned else None
    t = im.test_map(n)
    tab = im.tables(t)
    u = im.u_set(tab)
    assert (u[:4] == F([[0, 0], [im.ONE_MINUS, im.ONE_MINUS], [0, im.ONE_MINUS], [im.ONE_MINUS, 0]])).all(), "u = 0 and u = 1 - 2^-24 lead the set"
    on_entries = np.isin(u[:, 1], tab.m).sum() + np.isin(u[:, 0], tab.c).sum()
    assert on_entries >= 0.2 * u.shape[0], "u exactly on table entries"
    w, i, j, qx, qy = im.env_sample(tab, u[:, 0], u[:, 1], R, cells=True)
    assert w.dtype == F and np.isfinite(w).all()
    assert np.all((i >= 0) & (i < n) & (j >= 0) & (j < n)) and np.all(np.abs(qx) <= 1) and np.all(np.abs(qy) <= 1)
    assert np.abs(np.linalg.norm(w.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    assert (im.env_pdf(tab, w, R) > 0).all()
    # a bin of no width is never selected
    assert (tab.m[j + 1] > tab.m[j]).all() and (tab.c[j, i + 1] > tab.c[j, i]).all()
    empty = np.flatnonzero(tab.w.sum(axis=1) == 0)
    assert (empty.size > 0) == (n >= 7) and not np.isin(j, empty).any(), "whole rows of zero weight are in the map from n = 7 on, and are never chosen"
    if empty.size:
        assert np.array_equal(tab.c[empty[0]], (np.arange(n + 1) / n).astype(F)) and tab.m[empty[0] + 1] == tab.m[empty[0]]


@pytest.mark.parametrize("n", [2, 7, 64])
@pytest.mark.parametrize("where", ["inside", "corner"])
def test_a_map_with_one_texel_is_sampled_in_its_neighbourhood(n, where):
    """The interpolated map of one non-zero texel is its tent: it reaches the 3 x 3 cells around it and no further.  A corner texel's neighbourhood continues over the
    edges of the square by the octahedral wrap (the gutter rule puts it there), and the corner lies in the lower hemisphere."""
    ti, tj = (n // 2, n // 2 - 1) if where == "inside" else (n - 1, 0)
    t = np.zeros((n, n, 3), F)
    t[tj, ti] = F([3.0, 0.5, 0.0])
    tab = im.tables(t)
    hood = tab.w > 0
    expect = np.zeros((n + 2, n + 2), bool)  # the cells whose 3 x 3 gutter neighbourhood holds the texel
    g = sm.gutter(t)[..., 0] > 0
    for a in range(3):
        for b in range(3):
            expect[1:-1, 1:-1] |= g[b:b + n, a:a + n]
    assert np.array_equal(hood, expect[1:-1, 1:-1]) and hood[tj, ti]
    if where == "inside" and n >= 7:
        assert hood.sum() == 9
    rng = np.random.default_rng(n)
    u = rng.random((4000, 2)).astype(F)
    w, i, j, _, _ = im.env_sample(tab, u[:, 0], u[:, 1], cells=True)
    assert hood[j, i].all(), "every sample lands in the texel's neighbourhood"
    assert (im.env_pdf(tab, w) > 0).all() and np.abs(np.linalg.norm(w.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    if where == "corner" and n >= 7:
        assert (w[(i == ti) & (j == tj), 2] < 0).all() and ((i == ti) & (j == tj)).any(), "the corner cell is the lower hemisphere: the sampler unfolds it"
        # the tent covers the texel's cell and the inner halves of its neighbours, which hold 1/8 of the weight on either side: about (7/8)^2 of the samples
        assert (sm.env_eval(t, w)[:, 0] > 0).mean() > 0.5, "the sampled directions see the texel"


@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_round_trip_through_the_density(n):
    """The cell env_pdf indexes is the cell env_sample chose, except within 2^-20 of a cell border in the square (the direction is normalised, turned and projected again:
    a point that close to a border may land on its other side)."""
    t = im.test_map(n)
    tab = im.tables(t)
    rng = np.random.default_rng(17)
    u = rng.random((20000, 2)).astype(F)
    for R in (None, sm.rotation()):
        w, i, j, qx, qy = im.env_sample(tab, u[:, 0], u[:, 1], R, cells=True)
        fx, fy = (qx.astype(np.float64) * 0.5 + 0.5) * n, (qy.astype(np.float64) * 0.5 + 0.5) * n
        near = (np.abs(fx - np.round(fx)) * 2.0 / n <= 2.0 ** -20) | (np.abs(fy - np.round(fy)) * 2.0 / n <= 2.0 ** -20)
        _, _, pi, pj = im.pdf_cells(n, w, R)
        same = (pi == i) & (pj == j)
        print(f"n = {n}, {'identity' if R is None else 'turned'}: excluded share {near.mean():.2e}, cells that differ {(~same).mean():.2e}")
        assert near.mean() < 0.01
        assert same[~near].all()


# ---- statistics ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def open_ground(T):
    """An upward normal with no occluder under the sun map, 400 000 samples from a fixed seed: the cosine estimator's contributions, the quadrature, and what the
    mixtures need."""
    t, (si, sj) = im.sun_map()
    assert (si, sj) == (41, 38) and t[sj, si, 0] == 2000 and (t == F(0.05)).sum() == 3 * (64 * 64 - 1)
    N = 400000
    rng = np.random.default_rng(0x5C1)
    xi, u0, u1, b0, b1 = (np.minimum(rng.random(N).astype(F), im.ONE_MINUS) for _ in range(5))
    nf = np.broadcast_to(F([0, 0, 1]), (N, 3)).copy()
    _, wc = am.directions(nf, nf, np.stack([b0, b1], axis=1))
    cosine = sm.env_eval(t, wc)[:, 0].astype(np.float64)  # the pdf cancels cos / pi: the contribution is E(wi)
    m = 512
    mu2, phi = np.meshgrid((np.arange(m) + 0.5) / m, (np.arange(m) + 0.5) / m * 2.0 * np.pi, indexing="ij")
    ct, st = np.sqrt(mu2), np.sqrt(1.0 - mu2)
    dirs = np.stack([st * np.cos(phi), st * np.sin(phi), ct], axis=-1).reshape(-1, 3)
    quad = float(sm.env_eval(t, dirs.astype(F)).astype(np.float64).mean(axis=0)[0])  # d(cos^2 theta) d(phi) / (2 pi) = cos / pi d(omega)
    return dict(t=t, tab=im.tables(t), nf=nf, wc=wc, xi=xi, u0=u0, u1=u1, cosine=cosine, quad=quad, N=N)


@pytest.mark.parametrize("mix", [0.25, 0.5])
def test_the_mixture_estimator_is_unbiased_bounded_and_quieter(open_ground, mix):
    g = open_ground
    _, ray, c3 = im.estimate(g["tab"], g["t"], None, g["nf"], g["wc"], g["xi"], g["u0"], g["u1"], mix)
    c = c3[:, 0].astype(np.float64)
    N = g["N"]
    mean, sem = c.mean(), c.std(ddof=1) / math.sqrt(N)
    cmean, csem = g["cosine"].mean(), g["cosine"].std(ddof=1) / math.sqrt(N)
    ratio = c.var(ddof=1) / g["cosine"].var(ddof=1)
    bound = float(g["t"].max()) * 1.0 / (1.0 - mix)
    print(f"mix {mix}: mean {mean:.5f} +- {sem:.5f}, cosine {cmean:.5f} +- {csem:.5f}, quadrature {g['quad']:.5f}; variance ratio {ratio:.4f}; largest contribution {c3.max():.2f} "
          f"(bound {bound:.1f}); samples without a ray {(~ray).mean():.4f}")
    assert sem > 0 and abs(mean - g["quad"]) <= 4.0 * sem
    assert abs(cmean - g["quad"]) <= 4.0 * csem, "the cosine estimator of the same numbers, as tests/test_sky_api.py has it"
    assert ratio < 0.1
    assert c3.max() <= bound


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------------------
def test_params_mirror_matches_the_header(T):
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_sky_is_params\s*;", src).group(1)
    fields = [(m.group(2), m.group(1), m.group(3)) for m in re.finditer(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)]
    assert [(n, k) for n, _, k in fields] == [("max_distance", None), ("scale", None), ("mix", None), ("flags", None), ("reserved", "4")]
    S = T._ffi.SkyIsParams
    ctypes_of = {"float": C.c_float, "uint32_t": C.c_uint32}
    assert [(n, ct) for n, ct in S._fields_] == [(n, ctypes_of[t] * int(k) if k else ctypes_of[t]) for n, t, k in fields]
    assert C.sizeof(S) == 32 and [getattr(S, n).offset for n, _, _ in fields] == [0, 4, 8, 12, 16]


def test_entry_points_are_declared_and_bound(T):
    for name, nargs in (("trhip_env_make_sampler", 2), ("trhip_env_sample", 5), ("trhip_env_pdf", 5), ("trhip_sky_is_default_params", 1), ("trhip_render_sky_is", 10),
                        ("trhip_render_sky_is_device", 10)):
        assert re.search(r"\bint " + name + r"\(", header()), name
        assert name in T._ffi.SIGNATURES and len(T._ffi.SIGNATURES[name][1]) == nargs
        assert getattr(T.lib(), name) is not None
    assert T.lib().trhip_version() == 3001


def test_default_params_need_no_context(T):
    p = T._ffi.SkyIsParams(1.0, 2.0, 3.0, 4, (5, 6, 7, 8))
    assert T.lib().trhip_sky_is_default_params(C.byref(p)) == 0
    assert math.isinf(p.max_distance) and p.max_distance > 0
    assert (p.scale, p.mix, p.flags, list(p.reserved)) == (1.0, 0.5, 0, [0, 0, 0, 0])
    assert T.lib().trhip_sky_is_default_params(None) == INVALID


def good_params(T, **over):
    p = T._ffi.SkyIsParams()
    assert T.lib().trhip_sky_is_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k.startswith("reserved"):
            p.reserved[int(k[-1])] = v
        else:
            setattr(p, k, v)
    return p


BAD_PARAMS = [
    (dict(max_distance=float("nan")), b"max_distance"),
    (dict(max_distance=0.0), b"max_distance"),
    (dict(max_distance=-math.inf), b"max_distance"),
    (dict(scale=-0.5), b"scale"),
    (dict(scale=math.inf), b"scale"),
    (dict(scale=float("nan")), b"scale"),
    (dict(flags=4), b"flag"),
    (dict(flags=0x80000001), b"flag"),
    (dict(reserved0=1), b"reserved"),
    (dict(reserved3=7), b"reserved"),
    (dict(mix=0.0), b"mix"),
    (dict(mix=1.0), b"mix"),
    (dict(mix=-0.25), b"mix"),
    (dict(mix=float("nan")), b"mix"),
    (dict(mix=math.inf), b"mix"),
    # the order: the sky frame's checks in its order, then mix, then spp
    (dict(max_distance=0.0, scale=-1.0, flags=4, reserved1=1, mix=0.0), b"max_distance"),
    (dict(scale=-1.0, flags=4, reserved1=1, mix=0.0), b"scale"),
    (dict(flags=4, reserved1=1, mix=0.0), b"flag"),
    (dict(reserved1=1, mix=0.0), b"reserved"),
]


@pytest.mark.parametrize("entry", ["trhip_render_sky_is", "trhip_render_sky_is_device"])
def test_invalid_arguments_are_refused_without_a_device(T, entry):
    fn, L = getattr(T.lib(), entry), T.lib()
    sn, st, out = T._ffi.Sensor(), T.Stats(), np.zeros(4, F)
    outp = T._ffi.fptr(out) if entry == "trhip_render_sky_is" else C.c_void_p(out.ctypes.data)
    for over, word in BAD_PARAMS:
        assert fn(None, None, C.byref(sn), 0, 0, 0, None, C.byref(good_params(T, **over)), outp, C.byref(st)) == INVALID, over
        assert word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    for flags in (1, 2, 3):  # the two flags are known
        assert fn(None, None, C.byref(sn), 0, 0, 0, None, C.byref(good_params(T, flags=flags, mix=2.0 ** -24)), outp, C.byref(st)) == INVALID and b"spp" in L.trhip_last_error(None)
    assert fn(None, None, C.byref(sn), 1, 0, 0, None, None, outp, C.byref(st)) == INVALID  # no parameter block
    assert fn(None, None, C.byref(sn), 1, 0, 0, None, C.byref(good_params(T)), outp, C.byref(st)) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any()
    u, d = np.zeros((1, 2), F), np.ones((1, 3), F)
    assert L.trhip_env_make_sampler(None, None) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert L.trhip_env_sample(None, None, T._ffi.fptr(u), 1, T._ffi.fptr(d)) == INVALID and L.trhip_env_pdf(None, None, T._ffi.fptr(d), 1, T._ffi.fptr(u)) == INVALID


# ---- the Julia file ------------------------------------------------------------------------------------------------------------------------
def test_every_ccall_binds_a_header_prototype():
    calls, protos = jr.parse_ccalls(SHIM), jr.parse_header()
    for fn, sigs in calls.items():
        assert fn in protos, f"TraceHIPSkyIS.jl calls {fn}, which include/tracehip.h does not declare"
        for sig in sigs:
            assert jr.compatible(sig, protos[fn]), f"{fn}: ccall {sig} does not match the C prototype {protos[fn]}"
    for need in ("trhip_env_make_sampler", "trhip_env_sample", "trhip_env_pdf", "trhip_env_free", "trhip_sky_is_default_params", "trhip_render_sky_is", "trhip_render_sky_is_device",
                 "trhip_film_reduce", "trhip_scene_free"):
        assert need in calls, need


def test_params_struct_mirrors_the_header(T):
    src = open(SHIM, encoding="utf-8").read()
    body = re.search(r"mutable struct TrhipSkyIsParams\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"^\s+(\w+)::(\w+)", body, re.M)
    assert fields == [("max_distance", "Float32"), ("scale", "Float32"), ("mix", "Float32"), ("flags", "UInt32")] + [(f"reserved{k}", "UInt32") for k in range(4)]
    assert 4 * len(fields) == C.sizeof(T._ffi.SkyIsParams) == 32


def test_manifest_matches_the_shim_source():
    manifest = json.load(open(MANIFEST))
    calls = jr.parse_ccalls(SHIM)
    assert manifest["shim"] == "trace.jl_amd/julia/TraceHIPSkyIS.jl"
    assert manifest["ccalls"] == {fn: [[ret, args] for ret, args in sigs] for fn, sigs in sorted(calls.items())}, \
        "TraceHIPSkyIS.jl changed: bring tests/golden/julia_shim_sky_is_calls.json in step with its ccalls"


def test_the_path_env_file_includes_this_file_after_what_it_uses():
    """At the end of TraceHIPPathEnv.jl, which TraceHIPSky.jl includes after Environment, env_handle and the flags: TraceHIPSky.jl and TraceHIP.jl keep their text."""
    pe = open(os.path.join(os.path.dirname(SHIM), "TraceHIPPathEnv.jl"), encoding="utf-8").read()
    assert pe.rstrip().endswith('include("TraceHIPSkyIS.jl")') and pe.count('include("') == 1
    sky = open(os.path.join(os.path.dirname(SHIM), "TraceHIPSky.jl"), encoding="utf-8").read()
    at = sky.index('include("TraceHIPPathEnv.jl")')
    for name in ("struct Environment", "function env_handle(", "const TRHIP_SKY_ALBEDO", "const TRHIP_SKY_HIDE_BACKGROUND"):
        assert 0 <= sky.index(name) < at, name
    assert 'include("TraceHIPSkyIS.jl")' not in sky and 'include("TraceHIPSkyIS.jl")' not in open(jr.SHIM, encoding="utf-8").read()


# ---- the Python classes ----------------------------------------------------------------------------------------------------------------------
def camera(T):
    film = T.Film([16, 12], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def test_environment_sample_and_pdf_validate_their_arguments(T):
    e = T.Environment(np.ones((4, 4, 3)))
    for bad in (np.zeros((5, 3)), np.zeros(2 * 3).reshape(3, 2) + 1.0, np.full((1, 2), -0.1), np.full((1, 2), np.nan)):
        with pytest.raises(T.TraceHipError):
            e.sample(bad, ctx=object())  # shape and range are checked before the context is touched
    with pytest.raises(T.TraceHipError):
        e.pdf(np.zeros((5, 2)), ctx=object())


def test_sky_integrator_importance_argument(T, monkeypatch):
    cam, smp, env = camera(T), T.SeededSampler(3, seed=1), T.Environment.constant((1, 1, 1))
    plain = T.SkyIntegrator(cam, smp, env)
    assert plain.is_params is None and T.SkyIntegrator(cam, smp, env, importance=None).is_params is None
    a = T.SkyIntegrator(cam, smp, env, max_distance=0.5, albedo=True, scale=0.25, hide_background=True, importance=True)
    p = a.is_params
    assert (p.max_distance, p.scale, p.mix, p.flags, list(p.reserved)) == (0.5, 0.25, 0.5, T._ffi.SKY_ALBEDO | T._ffi.SKY_HIDE_BACKGROUND, [0, 0, 0, 0])
    assert T.SkyIntegrator(cam, smp, env, importance=0.25).is_params.mix == 0.25 and T.SkyIntegrator(cam, smp, env, importance=np.float32(0.75)).is_params.mix == 0.75
    for bad in (0.0, 1.0, -0.5, 2, float("nan"), math.inf, False, "0.5", (0.5,)):
        with pytest.raises(T.TraceHipError):
            T.SkyIntegrator(cam, smp, env, importance=bad)
    # which entry point a render reaches, without a device: the library is replaced by a recorder that refuses every call
    called = []

    class Recorder:
        def __getattr__(self, name):
            def fn(*args):
                called.append(name)
                return INVALID
            return fn

    class Flat:
        ctx = type("Ctx", (), {"_h": None, "check": staticmethod(lambda rc: None)})()
        _h = None

    scene = type("S", (), {"flatten": lambda self, ctx=None: Flat()})()
    monkeypatch.setattr(T._ffi, "lib", lambda: Recorder())
    monkeypatch.setattr(env, "_handle", lambda ctx: None)
    plain.render(scene)
    assert called == ["trhip_render_sky"], "importance=None is today's frame: the same call"
    del called[:]
    a.render(scene)
    assert called == ["trhip_env_make_sampler", "trhip_render_sky_is"]
