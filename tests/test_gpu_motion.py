"""Moving geometry in a preview on the GPU (docs/design/20-motion.md): the id plane of trhip_render_aov_ids against its definition, computed in numpy from the records of the
same call; trhip_temporal_motion against the numpy model of tests/motion_model.py bit for bit — on synthetic inputs that take every branch and hold garbage ids and body
words, and on a real three-frame sequence with a sliding sphere, a turning cube and a turning camera —; host == device, aliasing, the refusals that need a context;
PreviewSession with and without `motion`; and the quality figures.

Quality, measured on an MI355X (eight frames at 64 x 64, 2 spp, max_history 8; MSE of xyz / w at the last frame against the 1024 spp frame of that frame's pose; the session
with motion={...} over the same session with motion=None, which is what the library did before; QUALITY_MEASURED below, also in docs/design/20-motion.md):
still camera 0.8202 over the moving bodies' 621 surface pixels and 0.8918 over the whole frame; on the 0.75-degree arc 0.9974 over the bodies' 627 pixels and 1.0011 over
the whole frame — ON THE ARC THE MOTION-AWARE PASS GAINS NOTHING MEASURABLE, and the whole frame is 0.1 % worse, not "not above 1" as expected.  History kept at frame 3 of
the 48 x 48 sequence (N' >= 2): 0.981 of the sphere's 209 surface pixels (0.732 through trhip_temporal), 0.951 of the cube's 206 (0.922)."""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import motion_model as mm
import motion_scenes as ms
import temporal_model as tm

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits_equal(got, ref, what):
    g, r = bits(got), bits(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {int((g != r).sum())} of {g.size} values differ"


def assert_ids_equal(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name in ("prim", "material", "n_hit"):
        assert np.array_equal(got[name], ref[name]), f"{what}: {int((got[name] != ref[name]).sum())} of {got.size} pixels differ in {name}"
    assert_bits_equal(got["t"], ref["t"], f"{what}: t")
    assert got.tobytes() == ref.tobytes(), what


def frame(T, scene, cam, spp, depth, seed, offset=0):
    """(xyzw, planes) of a path frame and its feature planes with the same sampler settings."""
    xyzw = T.PathIntegrator(cam, T.SeededSampler(spp, seed=seed, sample_offset=offset), depth).render(scene)
    planes = T.AOVIntegrator(cam, T.SeededSampler(spp, seed=seed, sample_offset=offset)).render(scene).planes
    return xyzw, planes


def slot_to_entry(T, scene):
    """Ordered-primitive slot -> index of the top-level entry of scene.aggregate.primitives it belongs to."""
    counts = T.top_level_counts(scene)
    return np.repeat(np.arange(len(counts)), counts)[scene.flatten().bvh()[3]]


# ---- the id plane ------------------------------------------------------------------------------------------------------------------------------------------
# 5 x 3: less than a wave; 37 x 29 out of a 64 x 64 film (columns 28 - 64, past the box's right edge, rows 17 - 45): the crop's minimum (28, 17) is not the sample bounds'
# (27, 15) with a filter of radius (1.5, 2), so the film pixel's own records start at offset (2, 1); 64 x 64: sixteen blocks
ID_CASES = {"5x3-spp1": dict(resolution=[5, 3], spp=1), "5x3-spp3": dict(resolution=[5, 3], spp=3),
            "37x29-spp4-cropped": dict(resolution=64, crop=([0.421875, 0.25], [1.0, 0.703125]), radius=(1.5, 2.0), spp=4), "64x64-spp2": dict(resolution=64, spp=2)}


def render_ids(T, ctx, scene, cam, sampler, planes=True, samples=True, ids=True):
    """One trhip_render_aov_ids call with host pointers: (rc, planes, samples, ids)."""
    flat = scene.flatten(ctx)
    h, w = cam.film.size
    sbh, sbw = T.AOVIntegrator(cam, sampler)._sample_shape()
    P = np.zeros((h, w, 3, 4), F) if planes else None
    S = np.zeros((sampler.samples_per_pixel, sbh, sbw), T._ffi.AOV_DTYPE) if samples else None
    I = np.zeros((h, w), T._ffi.AOV_ID_DTYPE) if ids else None
    sn = cam.sensor()
    rc = T.lib().trhip_render_aov_ids(ctx._h, flat._h, C.byref(sn), sampler.samples_per_pixel, sampler.seed, sampler.sample_offset, T._ffi.fptr(P) if planes else None,
                                      S.ctypes.data_as(C.c_void_p) if samples else None, I.ctypes.data_as(C.c_void_p) if ids else None, None)
    return rc, P, S, I


@pytest.mark.parametrize("which", sorted(ID_CASES))
def test_id_plane_equals_its_definition(T, ctx, which):
    case = dict(ID_CASES[which])
    spp = case.pop("spp")
    scene, cam, sampler = ms.id_scene(T), ms.camera(T, **case), T.SeededSampler(spp, seed=0x1D5, sample_offset=3)
    h, w = cam.film.size
    assert (w, h) == tuple(int(v) for v in which.split("-")[0].split("x"))
    rc, planes, samples, ids = render_ids(T, ctx, scene, cam, sampler)
    assert rc == 0, T.lib().trhip_last_error(ctx._h)
    # planes and records of the same call are trhip_render_aov's bits
    aov = T.AOVIntegrator(cam, sampler)
    assert_bits_equal(planes, aov.render(scene, ctx).planes, "planes")
    assert samples.tobytes() == aov.samples(scene, ctx).tobytes(), "per-sample records"
    # the definition, from the records of the same call
    cmin, sb = np.asarray(cam.film.crop_bounds.p_min), cam.film.get_sample_bounds()
    offset = (int(cmin[1] - sb.p_min[1]), int(cmin[0] - sb.p_min[0]))
    if "cropped" in which:
        assert offset == (2, 1) and cmin.tolist() == [28.0, 17.0]
    ref = mm.id_plane(samples, offset, (h, w))
    assert_ids_equal(ids, ref.astype(T._ffi.AOV_ID_DTYPE), "id plane")
    hit = ids["prim"] >= 0
    assert np.array_equal(ids["n_hit"] > 0, hit) and ids["n_hit"].max() <= spp and np.isposinf(ids["t"][~hit]).all() and (ids["material"][~hit] == -1).all()
    if h * w > 100:
        entry = slot_to_entry(T, scene)[np.where(hit, ids["prim"], 0)]
        assert (~hit).sum() > 20 and (hit & (entry < 10)).sum() > 20, "misses and wall triangles"
        assert (hit & ((entry == 10) | (entry == 11))).sum() > 20 and (hit & (entry == 12)).sum() > 10, "spheres and the cube's triangles"
    if spp > 1 and h * w > 100:
        assert ((ids["n_hit"] > 0) & (ids["n_hit"] < spp)).any(), "a pixel some of whose samples miss"
    # the id plane alone, through the Python surface; again: identical from run to run
    assert_ids_equal(aov.ids(scene, ctx), ids, "AOVIntegrator.ids")
    assert_ids_equal(render_ids(T, ctx, scene, cam, sampler, planes=False)[3], ids, "second run, without the planes")
    # the device variant: all three outputs, then planes and ids through AOVIntegrator.render
    d_planes, d_samples, d_ids = (T._ffi.DeviceBuffer(a.nbytes).zero() for a in (planes, samples, ids))
    sn, flat = cam.sensor(), scene.flatten(ctx)
    rc = T.lib().trhip_render_aov_ids_device(ctx._h, flat._h, C.byref(sn), spp, sampler.seed, sampler.sample_offset, C.c_void_p(d_planes.ptr), C.c_void_p(d_samples.ptr),
                                             C.c_void_p(d_ids.ptr), None)
    assert rc == 0, T.lib().trhip_last_error(ctx._h)
    assert_bits_equal(d_planes.to_host(F, planes.shape), planes, "device variant, planes")
    assert d_samples.to_host(T._ffi.AOV_DTYPE, samples.shape).tobytes() == samples.tobytes(), "device variant, records"
    assert_ids_equal(d_ids.to_host(T._ffi.AOV_ID_DTYPE, ids.shape), ids, "device variant, id plane")
    d_planes.zero(), d_ids.zero()
    assert aov.render(scene, ctx, device_out=d_planes.ptr, device_ids=d_ids.ptr) is None
    assert_bits_equal(d_planes.to_host(F, planes.shape), planes, "AOVIntegrator.render(device_ids=...), planes")
    assert_ids_equal(d_ids.to_host(T._ffi.AOV_ID_DTYPE, ids.shape), ids, "AOVIntegrator.render(device_ids=...), id plane")
    for b in (d_planes, d_samples, d_ids):
        b.free()
    # all three outputs NULL
    assert render_ids(T, ctx, scene, cam, sampler, planes=False, samples=False, ids=False)[0] == -1 and b"null" in T.lib().trhip_last_error(ctx._h)


# ---- the temporal pass on synthetic inputs ----------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (5, 3), (37, 29), (64, 64)]  # a single lane, less than a wave, off the 16 x 16 block, sixteen blocks
# the small cases are windows of the 37 x 29 case at (12, 10): the points there are (0.1 x, 0.1 y, z), which this matrix sends back to the window's own pixels
SMALL_AT = (10, 12)
SMALL_M = np.array([[10.0, 0.0, 0.0, -12.0], [0.0, 10.0, 0.0, -10.0], [0.0, 0.0, 0.0, 1.0]], F)
SYNTHETIC = {}


def synthetic(w, h):
    """(B, P, history, ids, table, bodies, M, model outputs, tally): computed once per size and left unchanged."""
    if (w, h) not in SYNTHETIC:
        if w * h > 100:
            B, P, Hs, ids, table, bodies = mm.synthetic(h, w, 2000 + h)
            M = mm.SYNTHETIC_M
        else:
            B, P, Hs, ids, table, bodies = mm.synthetic(29, 37, 2029)
            y, x = SMALL_AT
            B, P, Hs, ids = (np.ascontiguousarray(a[y:y + h, x:x + w]) for a in (B, P, Hs, ids))
            M = SMALL_M
        tally = {}
        ref = mm.accumulate(B, P, Hs, M, ids, table, bodies, mm.SYNTHETIC_PARAMS, tally)
        SYNTHETIC[(w, h)] = (B, P, Hs, ids, table, bodies, M, ref, tally)
    B, P, Hs, ids, table, bodies, M, ref, tally = SYNTHETIC[(w, h)]
    return B.copy(), P.copy(), Hs.copy(), ids.copy(), table.copy(), bodies.copy(), M, ref, tally


def synthetic_accumulator(T):
    s = mm.SYNTHETIC_PARAMS
    return T.TemporalAccumulator(max_history=s.max_history, sigma_normal=s.sigma_normal, sigma_plane=s.sigma_plane, min_coverage=s.min_coverage)


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic_frames_equal_the_model(T, ctx, size):
    w, h = size
    B, P, Hs, ids, table, bodies, M, (ref_out, ref_hist), tally = synthetic(w, h)
    if w * h > 100:
        for name in mm.BRANCHES:
            assert tally.get(name, 0) >= 20, (name, tally)
    t = synthetic_accumulator(T)
    out, hist = t.accumulate_motion(B, P, Hs, ids, table, bodies, M, ctx)
    assert_bits_equal(out, ref_out, "out_xyzw")
    assert_bits_equal(hist, ref_hist, "out_history")
    assert t.stats.launches_film == 1
    out2, hist2 = t.accumulate_motion(B, P, Hs, ids, table, bodies, M, ctx)
    assert_bits_equal(out2, out, "second run, out_xyzw")
    assert_bits_equal(hist2, hist, "second run, out_history")
    # without history
    ref0 = mm.accumulate(B, P, None, None, ids, table, bodies, mm.SYNTHETIC_PARAMS)
    out0, hist0 = t.accumulate_motion(B, P, None, ids, table, bodies, None, ctx)
    assert_bits_equal(out0, ref0[0], "history = NULL, out_xyzw")
    assert_bits_equal(hist0, ref0[1], "history = NULL, out_history")
    # no table and no matrices, and every body static by index: trhip_temporal's bits
    plain_out, plain_hist = t.accumulate(B, P, Hs, M, ctx)
    static_words = np.where(np.arange(table.size) % 2 == 0, np.uint32(mm.STATIC), np.uint32(len(bodies)) + np.arange(table.size, dtype=np.uint32)).astype(np.uint32)
    for what, tb, mt in (("body_of_prim and bodies NULL", None, None), ("bodies NULL", table, None), ("body_of_prim NULL", None, bodies), ("all bodies static by index", static_words, bodies)):
        got_out, got_hist = t.accumulate_motion(B, P, Hs, ids, tb, mt, M, ctx)
        assert_bits_equal(got_out, plain_out, f"{what}: out_xyzw against trhip_temporal")
        assert_bits_equal(got_hist, plain_hist, f"{what}: out_history against trhip_temporal")
    if w * h > 100:
        assert not np.array_equal(bits(plain_out), bits(out)), "the bodies change something"
    assert_bits_equal(out[..., 3], B[..., 3], "the weight lane")
    assert_bits_equal(hist[..., 1:, :], plain_hist[..., 1:, :], "out_history holds the CURRENT n and p")


def test_host_device_and_aliased_calls_agree(T, ctx):
    B, P, Hs, ids, table, bodies, M, (ref_out, ref_hist), _ = synthetic(37, 29)
    h, w = B.shape[:2]
    t = synthetic_accumulator(T)
    inputs = (B, P, Hs, ids, table, bodies)
    d_in, d_pl, d_hs, d_ids, d_tb, d_mt = (T._ffi.DeviceBuffer(a.nbytes).from_host(a) for a in inputs)
    d_out, d_oh = T._ffi.DeviceBuffer(B.nbytes).zero(), T._ffi.DeviceBuffer(P.nbytes).zero()
    t.accumulate_motion_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_ids.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, M, d_out.ptr, d_oh.ptr, ctx)
    assert_bits_equal(d_out.to_host(F, B.shape), ref_out, "device variant, out_xyzw")
    assert_bits_equal(d_oh.to_host(F, P.shape), ref_hist, "device variant, out_history")
    for buf, a, what in zip((d_in, d_pl, d_hs, d_ids, d_tb, d_mt), inputs, ("xyzw", "planes", "history", "ids", "body_of_prim", "bodies")):
        assert buf.to_host(a.dtype, a.shape).tobytes() == a.tobytes(), f"the input {what} is left alone"
    d_oh.zero()
    t.accumulate_motion_device(d_in.ptr, d_pl.ptr, d_hs.ptr, d_ids.ptr, d_tb.ptr, table.size, d_mt.ptr, len(bodies), w, h, M, d_in.ptr, d_oh.ptr, ctx)
    assert_bits_equal(d_in.to_host(F, B.shape), ref_out, "out aliasing xyzw, device")
    assert_bits_equal(d_oh.to_host(F, P.shape), ref_hist, "out aliasing xyzw, device, out_history")
    buf, hist = B.copy(), np.empty_like(P)
    p = t._motion_params_for(M, table.size, len(bodies))
    rc = T.lib().trhip_temporal_motion(ctx._h, T._ffi.fptr(buf), T._ffi.fptr(P), T._ffi.fptr(Hs), ids.ctypes.data_as(C.c_void_p), T._ffi.u32ptr(table), T._ffi.fptr(bodies), w, h, C.byref(p),
                                       T._ffi.fptr(buf), T._ffi.fptr(hist), None)
    assert rc == 0
    assert_bits_equal(buf, ref_out, "out aliasing xyzw, host")
    assert_bits_equal(hist, ref_hist, "out aliasing xyzw, host, out_history")


def test_refusals(T, ctx):
    B, P, Hs, ids, table, bodies, M, _, _ = synthetic(37, 29)
    h, w = B.shape[:2]
    L, t = T.lib(), synthetic_accumulator(T)
    p = t._motion_params_for(M, table.size, len(bodies))
    out, hist = np.zeros_like(B), np.zeros_like(P)
    vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    fp = lambda a: T._ffi.fptr(a) if a is not None else None  # noqa: E731

    def call(xyzw=B, planes=P, history=Hs, idp=ids, tb=table, mt=bodies, w=w, h=h, prm=p, o=out, oh=hist, handle=ctx._h):
        return L.trhip_temporal_motion(handle, fp(xyzw), fp(planes), fp(history), vp(idp), T._ffi.u32ptr(tb) if tb is not None else None, fp(mt), w, h,
                                       C.byref(prm) if prm is not None else None, fp(o), fp(oh), None)
    assert call() == 0
    for kw in (dict(prm=None), dict(xyzw=None), dict(planes=None), dict(idp=None), dict(o=None), dict(oh=None), dict(w=0), dict(h=0), dict(handle=None)):
        assert call(**kw) == -1, kw
        assert L.trhip_last_error(None if "handle" in kw else ctx._h).decode(), kw
    # a table or matrices announced and not given
    assert call(tb=None) == -1 and "body_of_prim" in L.trhip_last_error(ctx._h).decode()
    assert call(mt=None) == -1 and "bodies" in L.trhip_last_error(ctx._h).decode()
    none = t._motion_params_for(M, 0, 0)
    assert call(tb=None, mt=None, prm=none) == 0 and call(prm=none) == 0, "with n_prims = n_bodies = 0 the two pointers are not looked at"
    # out_history may overlap nothing that is read or written beside it, in whole or in part; out_xyzw none of the three arrays
    in_hist = lambda a: hist.reshape(-1).view(np.uint8)[16:16 + a.nbytes].view(a.dtype).reshape(a.shape)  # noqa: E731
    for kw in (dict(oh=Hs), dict(oh=P), dict(history=hist), dict(planes=hist), dict(idp=in_hist(ids)), dict(tb=in_hist(table)), dict(mt=in_hist(bodies))):
        assert call(**kw) == -1, list(kw)
        assert "overlap" in L.trhip_last_error(ctx._h).decode()
    big = np.zeros(P.size + B.size, F)
    tail = big[B.size // 2:B.size // 2 + P.size].reshape(P.shape)
    assert call(o=big[:B.size].reshape(B.shape), oh=tail) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    assert call(xyzw=big[:B.size].reshape(B.shape), oh=tail) == -1
    in_out = out.reshape(-1).view(np.uint8)[:ids.nbytes].view(ids.dtype).reshape(ids.shape)
    assert call(idp=in_out) == -1 and "overlap" in L.trhip_last_error(ctx._h).decode()
    bad = T._ffi.TemporalMotionParams.from_buffer_copy(p)
    bad.max_history = 0.0
    assert call(prm=bad) == -1 and "max_history" in L.trhip_last_error(ctx._h).decode()
    assert call() == 0, "a refused call leaves the context usable"


# ---- a real sequence -----------------------------------------------------------------------------------------------------------------------------------------
SEQUENCE = dict(resolution=48, spp=2, depth=3, seed=0x7E3A, degrees=(0.0, 3.0, 6.0))


def body_inputs(T, scene, motion):
    """(body_of_prim, bodies) of a frame: the motion's keys in order are the bodies."""
    keys = sorted(motion)
    if not keys:
        return None, None
    of_entry = [None] * len(T.top_level_counts(scene))
    for i, k in enumerate(keys):
        of_entry[k] = i
    return scene.flatten().body_table(of_entry), np.stack([T.TemporalAccumulator.prev_from_cur(motion[k]) for k in keys])


@pytest.fixture(scope="module")
def motion_sequence(T, ctx):
    """[(scene, motion, camera, xyzw, planes, ids)] of three frames: the bodies move, the camera turns, frame k at sample_offset k * spp."""
    s, out = SEQUENCE, []
    for k, ((scene, motion), deg) in enumerate(zip(ms.scene_sequence(T, 3), s["degrees"])):
        cam = ms.camera(T, s["resolution"], deg)
        xyzw, planes = frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"])
        ids = T.AOVIntegrator(cam, T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])).ids(scene)
        out.append((scene, motion, cam, xyzw, planes, ids))
    return out


def test_moving_sequence_equals_the_model_and_keeps_the_bodies_history(T, ctx, motion_sequence):
    """The kernel equals the model on the device's own films, planes and ids, and at frame 3 more than half of the surface pixels of each moving body have N' >= 2 (on frames
    from the oracle's geometry the model says all of them: tests/test_motion_api.py; with 2 spp films the pixels on a silhouette mix two surfaces and some find no tap).
    Measured on an MI355X: sphere 0.981 of 209 pixels (0.732 through trhip_temporal on the same frames), cube 0.951 of 206 (0.922)."""
    t = T.TemporalAccumulator()
    prm = tm.Params(t.params.max_history, t.params.sigma_normal, t.params.sigma_plane, t.params.min_coverage)
    hist, plain_hist, prev, tally = None, None, None, {}
    for k, (scene, motion, cam, xyzw, planes, ids) in enumerate(motion_sequence):
        table, mats = body_inputs(T, scene, motion)
        M = prev.world_to_pixel() if prev is not None else None
        ref_out, ref_hist = mm.accumulate(xyzw, planes, hist, M, ids, table, mats, prm, tally)
        out, new_hist = t.accumulate_motion(xyzw, planes, hist, ids, table, mats, prev, ctx)
        assert_bits_equal(out, ref_out, f"frame {k}, out_xyzw")
        assert_bits_equal(new_hist, ref_hist, f"frame {k}, out_history")
        _, plain_hist = t.accumulate(xyzw, planes, plain_hist, prev, ctx)
        hist, prev = new_hist, cam
    print(f"moving sequence tally: {tally}")
    assert tally["moving_accepted"] > 100 and tally["static_by_index"] > 1000, tally
    scene, _, _, _, _, ids = motion_sequence[-1]
    entry = slot_to_entry(T, scene)[np.where(ids["prim"] >= 0, ids["prim"], 0)]
    surface = hist[..., 1, 3] == 1
    for name, index in (("sphere", ms.SPHERE_INDEX), ("cube", ms.CUBE_INDEX)):
        on_body = surface & (ids["prim"] >= 0) & (entry == index)
        share, plain = float((hist[on_body][:, 0, 3] >= 2).mean()), float((plain_hist[on_body][:, 0, 3] >= 2).mean())
        print(f"moving sequence, {name}: {int(on_body.sum())} surface pixels, N' >= 2 at {share:.3f} of them with the motion, {plain:.3f} through trhip_temporal")
        assert on_body.sum() >= 30 and share > 0.5, (name, int(on_body.sum()), share)
    assert hist[..., 0, 3].max() == 3.0, "three frames: the longest history is 3"


# ---- PreviewSession ------------------------------------------------------------------------------------------------------------------------------------------
def test_preview_session_with_motion_equals_the_calls_by_hand(T, ctx):
    s = SEQUENCE
    frames = ms.scene_sequence(T, 3)
    session = T.PreviewSession(frames[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"])
    t, d = T.TemporalAccumulator(), T.Denoiser()
    hist, prev = None, None
    for k, ((scene, motion), deg) in enumerate(zip(frames, s["degrees"])):
        cam = ms.camera(T, s["resolution"], deg)
        session.scene = scene
        got = session.render(cam, ctx, motion=motion)
        xyzw, planes = frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"])
        ids = T.AOVIntegrator(cam, T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=k * s["spp"])).ids(scene, ctx)
        table, mats = body_inputs(T, scene, motion)
        acc, hist = t.accumulate_motion(xyzw, planes, hist, ids, table, mats, prev, ctx)
        want = d.denoise(acc if k else xyzw, planes, ctx)
        assert_bits_equal(got, want, f"frame {k}: path + planes and ids + temporal_motion + denoise by hand")
        assert_bits_equal(got[..., 3], xyzw[..., 3], f"frame {k}: the weight lane")
        assert len(session.render_stats) == 4 and session.render_stats[2].launches_film == 1
        prev = cam
    assert session.frame == 3
    # a scene of another structure: refused with a sentence that names reset(), and rendered after it
    session.scene = ms.id_scene(T)
    with pytest.raises(T.TraceHipError, match=r"reset\(\)"):
        session.render(cam, ctx, motion={})
    assert session.frame == 3
    session.reset()
    got = session.render(cam, ctx, motion={})
    assert_bits_equal(got, T.Denoiser().render(session.scene, cam, T.SeededSampler(s["spp"], seed=s["seed"], sample_offset=3 * s["spp"]), s["depth"], ctx), "after reset(): Denoiser.render")
    with pytest.raises(T.TraceHipError, match="top-level"):
        session.render(cam, ctx, motion={99: T.translate([0.1, 0, 0])})
    session.close()
    # the display path takes the same argument
    shown = T.PreviewSession(frames[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"], display=T.Display())
    rgba = shown.render_display(ms.camera(T, s["resolution"], 0.0), ctx, motion={})
    assert rgba.shape == (s["resolution"], s["resolution"], 4) and rgba.dtype == np.uint8 and len(shown.render_stats) == 5
    shown.close()


def test_preview_session_without_motion_is_the_parents_session(T, ctx):
    """motion=None on a three-frame arc over the moving scenes: exactly the calls the session made before this pass existed — path, planes, trhip_temporal, denoise —, bit for
    bit, and no id plane is drawn."""
    s = SEQUENCE
    frames = ms.scene_sequence(T, 3)
    session = T.PreviewSession(frames[0][0], T.SeededSampler(s["spp"], seed=s["seed"]), s["depth"])
    t, d = T.TemporalAccumulator(), T.Denoiser()
    hist, prev = None, None
    for k, ((scene, _), deg) in enumerate(zip(frames, s["degrees"])):
        cam = ms.camera(T, s["resolution"], deg)
        session.scene = scene
        got = session.render(cam, ctx) if k else session.render(cam, ctx, motion=None)
        xyzw, planes = frame(T, scene, cam, s["spp"], s["depth"], s["seed"], k * s["spp"])
        acc, hist = t.accumulate(xyzw, planes, hist, prev, ctx)
        want = d.denoise(acc if k else xyzw, planes, ctx)
        assert_bits_equal(got, want, f"frame {k}: path + planes + temporal + denoise by hand")
        assert session._motion_buffers is None, "no id plane"
        prev = cam
    session.close()


# ---- quality ---------------------------------------------------------------------------------------------------------------------------------------------------
QUALITY = dict(resolution=64, spp=2, depth=5, seed=0xBEEF, frames=8)
QUALITY_CAMERAS = {"still": tuple(0.0 for _ in range(8)), "arc": tuple(0.75 * k for k in range(8))}
# mse(session with motion) / mse(the same session with motion=None) at the eighth frame: (over the moving bodies' surface pixels, over the whole frame)
QUALITY_MEASURED = {"still": (0.8202, 0.8918), "arc": (0.9974, 1.0011)}


def quality_ratios(T, ctx, which):
    q = QUALITY
    frames = ms.scene_sequence(T, q["frames"])
    cams = [ms.camera(T, q["resolution"], deg) for deg in QUALITY_CAMERAS[which]]
    results = {}
    for mode in ("motion", "plain"):
        session = T.PreviewSession(frames[0][0], T.SeededSampler(q["spp"], seed=q["seed"]), q["depth"])
        for (scene, motion), cam in zip(frames, cams):
            session.scene = scene
            results[mode] = session.render(cam, ctx, motion=motion if mode == "motion" else None)
        session.close()
    scene, last, offset = frames[-1][0], cams[-1], (q["frames"] - 1) * q["spp"]
    noisy, planes = frame(T, scene, last, q["spp"], q["depth"], q["seed"], offset)
    ids = T.AOVIntegrator(last, T.SeededSampler(q["spp"], seed=q["seed"], sample_offset=offset)).ids(scene, ctx)
    target = T.PathIntegrator(last, T.SeededSampler(1024, seed=0x7A26E7), q["depth"]).render(scene)
    surface = dm.surface_mask(noisy, planes, dm.Params(1.0, 1.0, 1.0, demodulate=False, min_coverage=0.5))
    entry = slot_to_entry(T, scene)[np.where(ids["prim"] >= 0, ids["prim"], 0)]
    bodies = surface & (ids["prim"] >= 0) & ((entry == ms.SPHERE_INDEX) | (entry == ms.CUBE_INDEX))
    everything = (target[..., 3] > 0) & (noisy[..., 3] > 0)

    def mse(a, mask):
        with np.errstate(all="ignore"):
            diff = a[mask][:, :3].astype(np.float64) / a[mask][:, 3:4] - target[mask][:, :3].astype(np.float64) / target[mask][:, 3:4]
        return float(np.mean(diff * diff))
    figures = {(mode, name): mse(results[mode], mask) for mode in results for name, mask in (("bodies", bodies), ("frame", everything))}
    return figures[("motion", "bodies")] / figures[("plain", "bodies")], figures[("motion", "frame")] / figures[("plain", "frame")], int(bodies.sum()), figures


@pytest.mark.parametrize("which", sorted(QUALITY_CAMERAS))
def test_motion_brings_the_moving_bodies_closer_to_their_1024spp_frame(T, ctx, which):
    """Eight frames at 2 spp, the sphere sliding and the cube turning, once with a still camera and once on the arc of the temporal tests: the last frame through the session
    with motion={...} against the same session with motion=None (the library's behaviour before), both measured against the 1024 spp frame of the last frame's own pose.  The
    frames are bit-reproducible, so each ratio is a number; it is asserted within 10 % of its measured value (QUALITY_MEASURED).  Measured: still camera 0.8202 on the bodies,
    0.8918 on the frame (mse 0.05917 against 0.07214; 0.016056 against 0.018003); arc 0.9974 and 1.0011 (0.05503 against 0.05517; 0.016306 against 0.016288): with the camera
    turning as well, the taps the motion-blind pass accepts on a slowly moving body cost it no more than the ones this pass finds — the expectation "below 1 on the bodies,
    not above 1 on the frame" holds for the still camera and NOT for the arc's whole frame.  PreviewSession's default stays motion=None."""
    on_bodies, on_frame, n_bodies, figures = quality_ratios(T, ctx, which)
    print(f"motion quality {which}: {n_bodies} pixels on the moving bodies; mse ratio motion / plain on the bodies {on_bodies:.4f}, on the whole frame {on_frame:.4f}; {figures}")
    assert n_bodies >= 100
    want_bodies, want_frame = QUALITY_MEASURED[which]
    assert abs(on_bodies / want_bodies - 1.0) <= 0.10, (on_bodies, want_bodies)
    assert abs(on_frame / want_frame - 1.0) <= 0.10, (on_frame, want_frame)
