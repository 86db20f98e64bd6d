"""The life of the host objects on the MI355X: contexts, scenes and relit views made and freed in the orders a host may choose, the three frames that create a pipe's
streams in the unusual order, and what trhip_last_sample_radiance describes after each kind of frame.  The shadows scene at 16 x 16, 2 spp, depth 3 throughout; at most one
context beside the session's at a time."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED, SPP, DEPTH, RES = 7, 2, 3, 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    bad = bits(a) != bits(b)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} values differ"


def close(c, *scenes):
    """Scenes go before their context."""
    for s in scenes:
        if s._flat is not None:
            s._flat.free()
    c.close()


def path(T, spp=SPP):
    return T.PathIntegrator(T.scenes.shadows_camera(RES), T.SeededSampler(spp, seed=SEED), DEPTH)


def test_scene_view_and_context_teardown_orders(T):
    """(a) A base and its relit view render the same film; the view outlives its base; a second context after the first is closed renders it again."""
    c = T.Context(0)
    base = T.scenes.shadows_scene()
    view = base.with_lights(base.lights)
    try:
        A = path(T).render(base, c).copy()
        assert np.isfinite(A).all() and A[..., :3].max() > 0
        assert_bits_equal(path(T).render(view, c), A, "relit to the same lights")
        assert view.flatten(c).geometry_id == base.flatten(c).geometry_id
        base.flatten(c).free()
        assert_bits_equal(path(T).render(view, c), A, "the view after its base was freed")
        view.flatten(c).free()
    finally:
        close(c, base, view)
    c = T.Context(0)
    again = T.scenes.shadows_scene()
    try:
        assert_bits_equal(path(T).render(again, c), A, "a second fresh context")
    finally:
        close(c, again)


def three_frames(T, c):
    """One SPPM iteration, a streaming path frame, a classic frame on two pipes with the second stream: the three callers that make a pipe's streams and events, SPPM first."""
    scene = T.scenes.shadows_scene()
    out = []
    try:
        sppm = T.SPPMIntegrator(T.scenes.shadows_camera(RES), 0.05, DEPTH, 1, 256, seed=SEED)
        out.append(("sppm", sppm.render(scene, c).copy()))
        c.set_option("streaming", 1)
        out.append(("streaming", path(T).render(scene, c).copy()))
        c.set_option("streaming", 0)
        c.set_option("pipelines", 2)
        c.set_option("overlap", 1)
        integ = path(T)
        out.append(("two pipes", integ.render(scene, c).copy()))
        assert integ.stats.n_batches == 2
    finally:
        for name, value in (("streaming", 0), ("pipelines", 1), ("overlap", 1)):
            c.set_option(name, value)
        if scene._flat is not None:
            scene._flat.free()
    return out


def test_pipe_callers_in_the_unusual_order(T, ctx):
    """(b) On a fresh context each of the three frames equals the same call on the session context."""
    c = T.Context(0)
    try:
        got = three_frames(T, c)
    finally:
        c.close()
    want = three_frames(T, ctx)
    for (what, g), (_, w) in zip(got, want):
        assert np.isfinite(g).all(), what
        assert_bits_equal(g, w, what)


def test_last_records(T):
    """(c) What trhip_last_sample_radiance describes: the path frame's records, the same after a refused call, a Whitted frame's count, nothing after a banded frame."""
    L = T.lib()
    c = T.Context(0)
    scene = T.scenes.shadows_scene()
    try:
        integ = path(T)
        integ.render(scene, c)
        rec = integ.sample_radiance(scene).copy()
        assert np.isfinite(rec).all() and rec.max() > 0
        flat, sn, st = scene.flatten(c), integ.camera.sensor(), T.Stats()
        film = np.empty((RES, RES, 4), np.float32)
        fptr = film.ctypes.data_as(C.POINTER(C.c_float))
        assert L.trhip_render_path(c._h, flat._h, C.byref(sn), 0, DEPTH, SEED, 0, fptr, C.byref(st)) == -1  # spp = 0: refused
        assert "spp must be >= 1" in L.trhip_last_error(c._h).decode()
        assert_bits_equal(integ.sample_radiance(scene), rec, "the records after a refused call")
        # Whitted at another sample count: the count is that frame's, and the path frame's size is now refused with it
        whitted = T.WhittedIntegrator(integ.camera, T.SeededSampler(1, seed=SEED), DEPTH)
        whitted.render(scene, c)
        w = whitted.sample_radiance(scene)
        assert w.shape == (1,) + rec.shape[1:] and np.isfinite(w).all()
        with pytest.raises(T.TraceHipError, match=f"expected {w.size} floats"):
            integ.sample_radiance(scene)
        c.set_option("band_tile_rows", 1)
        banded = path(T).render(scene, c)
        c.set_option("band_tile_rows", 0)
        with pytest.raises(T.TraceHipError, match="expected 0 floats"):
            integ.sample_radiance(scene)
        assert_bits_equal(banded, path(T).render(scene, c), "banded frame vs one band")
        assert_bits_equal(integ.sample_radiance(scene), rec, "the records of the frame after")
    finally:
        close(c, scene)
