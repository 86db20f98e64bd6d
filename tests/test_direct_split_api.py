"""Direct light kept out of a preview's history (trhip_temporal_split, trhip_film_add; docs/design/23-direct-split.md), the part that needs no GPU: the entry points
against the header, the refusals and their order through a NULL context, the identities of the numpy model (tests/direct_split_model.py) the kernels are compared with bit
for bit in tests/test_gpu_direct_split.py, the facts about the integrators the decomposition rests on, checked on the CPU oracle, what the Python classes refuse, and the
calls a PreviewSession makes with and without split_direct."""
import ctypes as C
import sys

import numpy as np
import pytest

import direct_split_model as dsm
import julia_replay as jr
import motion_model as mm
import motion_scenes as ms
import temporal_model as tm

F = np.float32
NAN = float("nan")
INVALID = -1  # TRHIP_ERR_INVALID
ENTRY_POINTS = ("trhip_temporal_split", "trhip_temporal_split_device", "trhip_film_add", "trhip_film_add_device")
FRONT_LIGHT, SECOND_LIGHT = ((0.5, 0.5, -1.5), 2.5), ((0.2, 0.6, -2.2), 1.0)  # (position, intensity): in front of the box, and inside it beside the sphere


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def lights(T, *which):
    return [T.PointLight(T.translate(list(at)), T.RGBSpectrum(power)) for at, power in which]


# ---- the C interface -------------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_with_the_headers_signatures(T):
    protos = jr.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, f"include/tracehip.h does not declare {name}"
        assert getattr(T.lib(), name) is not None
        ret, args = T._ffi.SIGNATURES[name]
        c_ret, c_args = jr.ctypes_sig(protos[name])
        assert ret is c_ret and len(args) == len(c_args), name
        for k, (a, c) in enumerate(zip(args, c_args)):
            if c is C.c_void_p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, k, a)
            else:
                assert a is c, (name, k, a, c)
    # trhip_temporal_motion's arguments in its order, with the direct film directly after the film; its parameter block, no new one
    for suffix in ("", "_device"):
        parent = protos["trhip_temporal_motion" + suffix][1]
        assert protos["trhip_temporal_split" + suffix][1] == parent[:2] + [parent[1]] + parent[2:], suffix
    assert T._ffi.SIGNATURES["trhip_temporal_split"][1][10] is T._ffi.SIGNATURES["trhip_temporal_motion"][1][9]
    assert protos["trhip_film_add"][1] == ["ptr:void", "ptr:f32", "ptr:f32", "u32", "u32", "ptr:f32", "ptr:stats"]
    assert protos["trhip_film_add_device"][1] == ["ptr:void"] * 3 + ["u32", "u32", "ptr:void", "ptr:stats"]
    assert not any("split_default_params" in name or "split_params" in name for name in protos), "no new struct"
    assert T.lib().trhip_version() == 3001, "added without a version change"


def good_params(T, **over):
    p = T._ffi.TemporalMotionParams()
    assert T.lib().trhip_temporal_motion_default_params(C.byref(p)) == 0
    for k, v in over.items():
        if k == "matrix_entry":
            p.prev_world_to_pixel[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


# trhip_temporal_motion's block checks, in its order, under this entry's name
ORDER = [dict(matrix_entry=(5, NAN)), dict(max_history=0.0), dict(sigma_normal=0.0), dict(sigma_plane=-1.0), dict(min_coverage=2.0), dict(flags=4), dict(reserved=3)]
ORDER_WORDS = [b"prev_world_to_pixel", b"max_history", b"sigma_normal", b"sigma_plane", b"min_coverage", b"flag bits", b"reserved must"]


@pytest.mark.parametrize("entry", ["trhip_temporal_split", "trhip_temporal_split_device"])
def test_split_refusals_and_their_order_without_a_device(T, entry):
    """No context exists here, so every call is refused.  The parameter block is checked first, all of it — the message kept for trhip_last_error(NULL) names this entry and
    the field, and of two bad fields the earlier one —, then the pointers."""
    fn, L = getattr(T.lib(), entry), T.lib()
    host = entry == "trhip_temporal_split"
    film, direct, planes = np.zeros((2, 2, 4), F), np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F)
    out, out_h = np.zeros((2, 2, 4), F), np.zeros((2, 2, 3, 4), F)
    ids, table, mats = np.zeros((2, 2), mm.ID_DTYPE), np.zeros(3, np.uint32), np.zeros((1, 12), F)
    vp = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    fp = (lambda a: T._ffi.fptr(a)) if host else vp
    up = (lambda a: T._ffi.u32ptr(a)) if host else vp

    def call(prm, film_=film, direct_=direct, idp=ids, tb=table, mt=mats):
        return fn(None, fp(film_) if film_ is not None else None, fp(direct_) if direct_ is not None else None, fp(planes), None, vp(idp) if idp is not None else None,
                  up(tb) if tb is not None else None, fp(mt) if mt is not None else None, 2, 2, C.byref(prm) if prm is not None else None, fp(out), fp(out_h), None)
    for over, word in zip(ORDER, ORDER_WORDS):
        assert call(good_params(T, **over)) == INVALID, over
        assert b"trhip_temporal_split: " in L.trhip_last_error(None) and word in L.trhip_last_error(None), (over, L.trhip_last_error(None))
    for k in range(len(ORDER)):
        for j in range(k + 1, len(ORDER)):
            assert call(good_params(T, **ORDER[k], **ORDER[j])) == INVALID
            assert ORDER_WORDS[k] in L.trhip_last_error(None), (ORDER[k], ORDER[j], L.trhip_last_error(None))
    assert call(None) == INVALID and b"null argument" in L.trhip_last_error(None)  # no parameter block
    # a bad block and missing pointers: the block is reported
    assert call(good_params(T, reserved=1), film_=None, idp=None) == INVALID and b"reserved" in L.trhip_last_error(None)
    # a good block: the null context is a null pointer, reported before the table rules, with or without a direct film
    for prm in (good_params(T), good_params(T, n_prims=3, n_bodies=1), good_params(T, n_prims=3)):
        for d in (direct, None):
            assert call(prm, direct_=d) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert call(good_params(T, n_prims=3, n_bodies=1), idp=None, tb=None, mt=None) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any() and not out_h.any()


@pytest.mark.parametrize("entry", ["trhip_film_add", "trhip_film_add_device"])
def test_film_add_refuses_null_pointers_without_a_device(T, entry):
    fn, L = getattr(T.lib(), entry), T.lib()
    a, b, out = np.ones((2, 2, 4), F), np.ones((2, 2, 4), F), np.zeros((2, 2, 4), F)
    fp = (lambda x: T._ffi.fptr(x)) if entry == "trhip_film_add" else (lambda x: C.c_void_p(x.ctypes.data))
    for args in ((fp(a), fp(b), 2, 2, fp(out)), (None, fp(b), 2, 2, fp(out)), (fp(a), None, 0, 2, fp(out)), (fp(a), fp(b), 2, 2, None), (fp(a), fp(b), 0, 0, fp(b))):
        assert fn(None, *args, None) == INVALID and b"null argument" in L.trhip_last_error(None)
    assert not out.any()


# ---- the model's identities ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 29)], ids=["1x1", "5x3", "37x29"])
def test_model_identities(size):
    """direct NULL or all +0: motion_model's outputs bit for bit; with no tables as well, temporal_model's.  A direct film that is not zero changes the film and the history's
    colour, and never the weight lane or the history's surface words."""
    w, h = size
    if w * h > 100:
        B, P, Hs, ids, table, bodies = mm.synthetic(h, w, 2000 + h)
        M = mm.SYNTHETIC_M
    else:
        B, P, Hs, ids, table, bodies = mm.synthetic(29, 37, 2029)
        B, P, Hs, ids = (np.ascontiguousarray(a[10:10 + h, 12:12 + w]) for a in (B, P, Hs, ids))
        M = np.array([[10.0, 0.0, 0.0, -12.0], [0.0, 10.0, 0.0, -10.0], [0.0, 0.0, 0.0, 1.0]], F)
    prm = mm.SYNTHETIC_PARAMS
    for history, matrix in ((Hs, M), (None, None)):
        want = mm.accumulate(B, P, history, matrix, ids, table, bodies, prm)
        plain = tm.accumulate(B, P, history, matrix, prm)
        for what, direct in (("NULL", None), ("zero", dsm.synthetic_direct(B, 1, "zero"))):
            got = dsm.accumulate(B, direct, P, history, matrix, ids, table, bodies, prm)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), f"direct {what}: motion_model"
            for tb, mt, idp in ((None, None, ids), (None, None, None), (table, None, ids)):
                got = dsm.accumulate(B, direct, P, history, matrix, idp, tb, mt, prm)
                assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1]), f"direct {what}, no tables: temporal_model"
        for kind in ("finite", "special"):
            D = dsm.synthetic_direct(B, 7, kind)
            got = dsm.accumulate(B, D, P, history, matrix, ids, table, bodies, prm)
            assert same_bits(got[0][..., 3], B[..., 3]), "the weight lane"
            garbage_w = D.copy()
            garbage_w[..., 3] = F(NAN)
            again = dsm.accumulate(B, garbage_w, P, history, matrix, ids, table, bodies, prm)
            assert same_bits(again[0], got[0]) and same_bits(again[1], got[1]), "D.w is not read"
            if w * h > 100:
                assert not same_bits(got[0], want[0]) and not same_bits(got[1][..., 0, :], want[1][..., 0, :])
                both = (got[1][..., 1, 3] == 1) & (want[1][..., 1, 3] == 1)
                assert both.sum() > 100 and same_bits(got[1][both][:, 1:, :], want[1][both][:, 1:, :]), "n and p of the history do not depend on the direct film"


def test_model_film_add_and_the_round_trip():
    rng = np.random.default_rng(5)
    a, b = rng.normal(0, 1, (7, 5, 4)).astype(F), rng.normal(0, 1, (7, 5, 4)).astype(F)
    b[0, 0, :3], b[1, 1, 0], a[2, 2, 1] = F(-0.0), F(np.inf), F(NAN)
    out = dsm.film_add(a, b)
    assert same_bits(out[..., 3], a[..., 3]) and same_bits(out[..., :3], (a[..., :3] + b[..., :3]).astype(F))
    assert same_bits(dsm.film_add(a, np.zeros_like(a))[np.isfinite(a).all(-1)], a[np.isfinite(a).all(-1)])
    # taking a film out and putting it back is exact where the subtraction was (Sterbenz: D <= B <= 2 D), and within one rounding of B otherwise
    B = np.abs(a) + F(0.5)
    D = (B * rng.uniform(0.5, 1.0, B.shape)).astype(F)
    back = dsm.film_add(dsm.remainder(B, D), D)
    assert same_bits(back, B)


# ---- what the decomposition rests on, on the CPU oracle ------------------------------------------------------------------------------------------------------------------
ORACLE = dict(resolution=32, spp=4, depth=5, seed=0x5D17)


@pytest.fixture(scope="module")
def oracle_films(T, ob):
    """{n_lights: {(integrator, depth): (xyzw, samples)}} of moving_scene under the front light, and under the front and the second light: rendered once."""
    q, out = ORACLE, {}
    cam = ms.camera(T, q["resolution"])
    for n, which in ((1, (FRONT_LIGHT,)), (2, (FRONT_LIGHT, SECOND_LIGHT))):
        osc = ob.OracleScene.from_scene(ms.moving_scene(T).with_lights(lights(T, *which)))
        out[n] = {(name, depth): osc.render(cam, name, q["spp"], depth, seed=q["seed"], want_samples=True)[:2] for name, depth in (("path", q["depth"]), ("path", 1), ("whitted", 1))}
    return out


@pytest.mark.parametrize("n_lights", [1, 2])
def test_the_depth_1_frame_is_the_first_vertex_of_the_full_frame(oracle_films, n_lights):
    """path_li starts L = 0 + 1 * Ld(first vertex) and only adds to it: with the same seed the depth-1 frame has the full frame's camera samples and film weights — the .w
    lanes of the three films are bit-equal — and no sample of the full frame lies below its depth-1 sample in any channel; no film pixel has a negative T - D in Y."""
    films = oracle_films[n_lights]
    (full, L_full), (first, L_first), (whitted, _) = films[("path", ORACLE["depth"])], films[("path", 1)], films[("whitted", 1)]
    assert same_bits(full[..., 3], first[..., 3]) and same_bits(full[..., 3], whitted[..., 3]), "the weight lanes"
    assert np.isfinite(L_full).all() and np.isfinite(L_first).all()
    assert not (L_full < L_first).any(), int((L_full < L_first).sum())
    assert (L_first > 0).mean() > 0.1 and (L_full > L_first).mean() > 0.1, "both terms are there"
    lit = full[..., 3] > 0
    assert not ((full[..., 1] - first[..., 1])[lit] / full[..., 3][lit] < 0).any()


def test_one_light_path_and_whitted_depth_1_samples_agree(oracle_films):
    """With one light uniform_sample_one_light picks it with probability 1, and Whitted's sum over the lights has one term: the two depth-1 samples are a handful of roundings
    of the same product apart — asserted within 1e-5 relative (measured: 1.6e-7, 77 % of the samples bit-equal)."""
    (_, a), (_, b) = oracle_films[1][("path", 1)], oracle_films[1][("whitted", 1)]
    scale = np.maximum(np.abs(a), np.abs(b))
    err = float((np.abs(a.astype(np.float64) - b) / np.where(scale > 0, scale, 1.0)).max())
    print(f"one light, path depth 1 against Whitted depth 1: largest relative difference {err:.3g}, {float((bits(a) == bits(b)).mean()):.3f} of the values bit-equal")
    assert (scale > 0).mean() > 0.1 and err <= 1e-5, err


def test_two_lights_whitted_depth_1_has_the_path_depth_1_films_mean(oracle_films):
    """With two lights the depth-1 path film picks one light per vertex and doubles it; Whitted sums both: the same expectation, without the picking noise.  The ratio of the
    films' means is asserted within 5 % of 1 (measured: 1.0024), and the films do differ."""
    (first, _), (whitted, _) = oracle_films[2][("path", 1)], oracle_films[2][("whitted", 1)]
    ratio = float(whitted[..., :3].astype(np.float64).mean() / first[..., :3].astype(np.float64).mean())
    print(f"two lights: mean of the Whitted depth-1 film over the path depth-1 film's {ratio:.4f}")
    assert abs(ratio - 1.0) <= 0.05, ratio
    assert not same_bits(first, whitted) and np.abs(first[..., :3] - whitted[..., :3]).max() > 1e-3


# ---- Python --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_python_classes_refuse_what_the_split_cannot_be_combined_with(T):
    t = T.TemporalAccumulator(max_history=4)
    p = t._split_params_for(None, 7, 2)
    assert isinstance(p, T._ffi.TemporalMotionParams) and (p.max_history, p.n_prims, p.n_bodies, p.flags, p.reserved) == (4.0, 7, 2, 0, 0)
    for bad in (T.TemporalAccumulator(clip_gamma=1.0), T.TemporalAccumulator(moments=True), T.TemporalAccumulator(clip_gamma=1.0, carry_bodies=True)):
        with pytest.raises(T.TraceHipError, match="plain accumulator"):
            bad._split_params_for(None, 0, 0)
        with pytest.raises(T.TraceHipError, match="plain accumulator"):
            bad.accumulate_split_device(1, 2, 3, None, None, None, 0, None, 0, 4, 4, None, 5, 6)
    film, planes = np.zeros((4, 4, 4), F), np.zeros((4, 4, 3, 4), F)
    for kw in (dict(direct=np.zeros((4, 3, 4), F)), dict(history=np.zeros((4, 4, 3, 3), F)), dict(ids=np.zeros((4, 3), mm.ID_DTYPE)), dict(planes=np.zeros((4, 4, 4), F))):
        args = dict(xyzw=film, direct=None, planes=planes, history=None, ids=None, body_of_prim=None, bodies=None, prev_camera=None)
        args.update(kw)
        with pytest.raises(T.TraceHipError, match="accumulate_split"):  # refused before anything touches a device
            t.accumulate_split(**args)
    with pytest.raises(T.TraceHipError, match="Film.add"):
        T.Film.add(film, np.zeros((4, 3, 4), F))
    scene, sampler = ms.moving_scene(T), T.SeededSampler(2, seed=3)
    refused = {"an upscaler": dict(upscaler=T.Upscaler()), "temporal_upsample": dict(upscaler=T.Upscaler(), temporal_upsample=T.TemporalUpsampler()),
               "variance_guided": dict(variance_guided=True), "a clipping or moments": dict(temporal=T.TemporalAccumulator(clip_gamma=2.0))}
    for sentence, kw in refused.items():
        with pytest.raises(T.TraceHipError, match="split_direct cannot be combined with " + sentence):
            T.PreviewSession(scene, sampler, 3, split_direct=True, **kw)
        T.PreviewSession(scene, sampler, 3, **kw)  # without the split each is a session
    for temporal in (T.TemporalAccumulator(moments=True), T.TemporalAccumulator(clip_gamma=2.0, carry_bodies=True)):
        with pytest.raises(T.TraceHipError, match="clipping or moments"):
            T.PreviewSession(scene, sampler, 3, split_direct=True, temporal=temporal)
    assert T.PreviewSession(scene, sampler, 3).split_direct is False and T.PreviewSession(scene, sampler, 3, split_direct=True).split_direct is True


class Recorder:
    """Stands in for the device side of a PreviewSession: every integrator, buffer, accumulator and filter call lands in `calls` with its buffers named by the order in which
    the session allocated them."""

    def __init__(self):
        self.calls, self.buffers = [], []

    def name(self, v):
        if isinstance(v, np.ndarray):
            return "matrix"
        return f"b{self.buffers.index(v)}" if isinstance(v, int) and v in self.buffers else v

    def log(self, what, *args):
        self.calls.append((what,) + tuple(self.name(a) for a in args if not isinstance(a, Recorder.Context)))

    class Context:
        pass


def recorded_session(T, monkeypatch, n_lights, frames, motion=None, **session_kw):
    """The calls `frames` renders of a PreviewSession make, with nothing of them reaching a device."""
    api, rec, ctx = sys.modules[T.PreviewSession.__module__], Recorder(), Recorder.Context()

    class Buffer:
        def __init__(self, nbytes):
            self.nbytes, self.ptr = nbytes, 4096 * (len(rec.buffers) + 1)
            rec.buffers.append(self.ptr)

        def from_host(self, a):
            return self

        def free(self):
            pass

    def integrator(kind):
        class Integrator:
            def __init__(self, camera, sampler, max_depth=None):
                self.sampler, self.max_depth, self.stats = sampler, max_depth, kind

            def render(self, scene, ctx, device_out=None, device_ids=None):
                rec.log(kind, self.max_depth, self.sampler.sample_offset, device_out, *(() if device_ids is None else (device_ids,)))
        return Integrator

    class Stage:
        clip_params = moments_params = clip_motion_params = None
        stats = "stage"

        def __getattr__(self, name):
            if not name.endswith("_device"):
                raise AttributeError(name)
            return lambda *args: rec.log(name, *args)

    class Flat:
        top_counts = [1, 1]

        def body_table(self, body_of_top):
            return np.zeros(2, np.uint32)
    flat = Flat()
    flat.ctx = ctx

    class FakeScene:
        lights = [object()] * n_lights

        def flatten(self, ctx=None):
            return flat
    for name, kind in (("PathIntegrator", "path"), ("WhittedIntegrator", "whitted"), ("AOVIntegrator", "aov")):
        monkeypatch.setattr(api, name, integrator(kind))
    monkeypatch.setattr(api._ffi, "DeviceBuffer", Buffer)
    monkeypatch.setattr(api.Film, "add_device", staticmethod(lambda *args: rec.log("film_add_device", *args) or "add"))
    session = T.PreviewSession(FakeScene(), T.SeededSampler(2, seed=9), 5, denoiser=Stage(), temporal=Stage(), **session_kw)
    cam = ms.camera(T, 8)
    for _ in range(frames):
        session._render_device(cam, None, motion)
    return rec.calls, session


def test_the_default_session_makes_todays_calls_and_the_split_session_its_own(T, monkeypatch):
    """split_direct=False: path, planes, trhip_temporal, the filter — on the frame's own bits without a history —, call for call what the session made before the split
    existed, and no buffer more.  split_direct=True: the depth-1 path frame with the frame's sampler (with two lights the depth-1 Whitted frame as well), trhip_temporal_split
    with NULL tables, the filter on the pass's output on every frame, the addition last."""
    w = h = 8
    today = [("path", 5, 0, "b0"), ("aov", None, 0, "b1"), ("accumulate_device", "b0", "b1", None, w, h, None, "b2", "b4"), ("denoise_device", "b0", "b1", w, h, "b2"),
             ("path", 5, 2, "b0"), ("aov", None, 2, "b1"), ("accumulate_device", "b0", "b1", "b4", w, h, "matrix", "b2", "b3"), ("denoise_device", "b2", "b1", w, h, "b2")]
    calls, session = recorded_session(T, monkeypatch, 1, 2)
    assert calls == today and len(session._buffers) == 5 and session._split_buffers is None and session.render_stats == ("path", "aov", "stage", "stage")
    calls, _ = recorded_session(T, monkeypatch, 2, 2, split_direct=False)
    assert calls == today
    motion_today = [("path", 5, 0, "b0"), ("aov", None, 0, "b1", "b5"), ("accumulate_motion_device", "b0", "b1", None, "b5", None, 0, None, 0, w, h, None, "b2", "b4"),
                    ("denoise_device", "b0", "b1", w, h, "b2")]
    calls, _ = recorded_session(T, monkeypatch, 1, 1, motion={})
    assert calls == motion_today
    # one light: the depth-1 path film is taken out and put back
    calls, session = recorded_session(T, monkeypatch, 1, 2, split_direct=True)
    assert calls == [("path", 5, 0, "b0"), ("path", 1, 0, "b5"), ("aov", None, 0, "b1"),
                     ("accumulate_split_device", "b0", "b5", "b1", None, None, None, 0, None, 0, w, h, None, "b2", "b4"), ("denoise_device", "b2", "b1", w, h, "b2"),
                     ("film_add_device", "b2", "b5", w, h, "b2"),
                     ("path", 5, 2, "b0"), ("path", 1, 2, "b5"), ("aov", None, 2, "b1"),
                     ("accumulate_split_device", "b0", "b5", "b1", "b4", None, None, 0, None, 0, w, h, "matrix", "b2", "b3"), ("denoise_device", "b2", "b1", w, h, "b2"),
                     ("film_add_device", "b2", "b5", w, h, "b2")]
    assert len(session._split_buffers) == 2 and session.render_stats == ("path", "aov", "stage", "stage", "path", "add")
    session.close()
    assert session._split_buffers is None and session._buffers is None
    # two lights: Whitted's depth-1 film is what comes back
    calls, session = recorded_session(T, monkeypatch, 2, 1, split_direct=True)
    assert calls == [("path", 5, 0, "b0"), ("path", 1, 0, "b5"), ("whitted", 1, 0, "b6"), ("aov", None, 0, "b1"),
                     ("accumulate_split_device", "b0", "b5", "b1", None, None, None, 0, None, 0, w, h, None, "b2", "b4"), ("denoise_device", "b2", "b1", w, h, "b2"),
                     ("film_add_device", "b2", "b6", w, h, "b2")]
    assert session.render_stats == ("path", "aov", "stage", "stage", "path", "whitted", "add")
    # with a motion dict the id plane is drawn as before and goes into the pass
    calls, _ = recorded_session(T, monkeypatch, 1, 1, motion={}, split_direct=True)
    assert calls == [("path", 5, 0, "b0"), ("path", 1, 0, "b6"), ("aov", None, 0, "b1", "b5"),
                     ("accumulate_split_device", "b0", "b6", "b1", None, "b5", None, 0, None, 0, w, h, None, "b2", "b4"), ("denoise_device", "b2", "b1", w, h, "b2"),
                     ("film_add_device", "b2", "b6", w, h, "b2")]
    # no lights: no direct render, direct=None, nothing to add
    calls, session = recorded_session(T, monkeypatch, 0, 1, split_direct=True)
    assert calls == [("path", 5, 0, "b0"), ("aov", None, 0, "b1"), ("accumulate_split_device", "b0", None, "b1", None, None, None, 0, None, 0, w, h, None, "b2", "b4"),
                     ("denoise_device", "b2", "b1", w, h, "b2")]
    assert session._split_buffers is None and session.render_stats == ("path", "aov", "stage", "stage")
