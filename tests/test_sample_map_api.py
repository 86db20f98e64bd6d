"""Adaptive sampling without a GPU (docs/design/24-adaptive.md): the film model of tests/sample_map_model.py against the oracle's own render, the numpy models of the
statistics and map rules on hand-checked values and against the package's vectorised copy, SampleMap.from_film / region on 3 x 2 films checked by hand,
AdaptivePathIntegrator.tau_for_budget on a synthetic field, the parameter block and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import sample_map_model as sm

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def camera(T, resolution, radius):
    film = T.Film(list(resolution), T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter(list(radius), 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


@pytest.mark.parametrize("resolution,radius", [((37, 29), (2.5, 1.5)), ((37, 29), (1.0, 1.0)), ((5, 3), (1.0, 1.0))])
def test_film_model_with_uniform_counts_is_the_oracles_film(T, ob, resolution, radius):
    """counts == spp: the model built from the oracle's film pieces is the oracle's render, bit for bit (wide filter: several tiles reach a pixel, negative lobes)."""
    spp, depth, seed, offset = 3, 3, 5, 2
    scene = T.scenes.shadows_scene()
    cam = camera(T, resolution, radius)
    osc = ob.OracleScene.from_scene(scene)
    xyzw, L, _ = osc.render(cam, "path", spp, depth, seed=seed, sample_offset=offset, want_samples=True)
    sbh, sbw, _, _ = sm.sample_shape(cam)
    model = sm.film_model(ob, cam, L, np.full((sbh, sbw), spp), seed, offset)
    assert np.array_equal(bits(model), bits(xyzw))
    # and a sample that is not drawn is skipped: with one pixel's count lowered only films within its reach change, and its weight falls
    counts = np.full((sbh, sbw), spp)
    counts[sbh // 2, sbw // 2] = 1
    fewer = sm.film_model(ob, cam, L, counts, seed, offset)
    changed = np.argwhere(bits(fewer)[..., 3] != bits(xyzw)[..., 3])
    reach = [2 * int(np.ceil(r)) + 2 for r in radius]  # a sample reaches at most 2 r + 1 pixels on an axis (film.jl:145-146), its pixel's samples one more
    assert 0 < len(changed) <= reach[0] * reach[1]
    assert np.ptp(changed[:, 0]) < reach[1] and np.ptp(changed[:, 1]) < reach[0]


def test_stats_model_on_hand_checked_records():
    L = np.zeros((2, 1, 3, 3), F)
    L[:, 0, 0] = [[1, 1, 1], [3, 3, 3]]          # Y = 1, 3 (the weights sum to 1 in Float32): m = 2, v = (1 + 9) / 2 - 4 = 1
    L[:, 0, 1] = [[np.nan, 5, 5], [2, 2, 2]]      # the NaN record is black: Y = 0, 2: m = 1, v = 2 - 1 = 1
    L[:, 0, 2] = [[np.inf, 0, 0], [0, 0, 0]]      # Y = Inf: m = Inf, x = Inf - Inf = NaN, which stays
    mv = sm.stats_model(L)
    y1 = sm.dm.to_Y(np.ones(3, F))
    assert y1 == F(1.0)
    assert mv[0, 0].tolist() == [2.0, 1.0] and mv[0, 1].tolist() == [1.0, 1.0]
    assert mv[0, 2, 0] == np.inf and np.isnan(mv[0, 2, 1])


def test_map_model_on_hand_checked_fields(T):
    # one row of five pixels, eps 0, tau 0.5: e = v / m^2, x = 4 E
    mv = np.zeros((1, 5, 2), F)
    mv[0, :, 0] = 1.0
    mv[0, :, 1] = [0.0, 0.0, 1.0, 0.0, 0.0]       # e = 1 at pixel 2: E = 1 at pixels 1..3 -> x = 4
    counts, total = sm.map_model(mv, 0.5, 0.0, 2, 10)
    assert counts.tolist() == [[0, 2, 2, 2, 0]] and total == 6
    counts, _ = sm.map_model(mv, 0.5, 0.0, 2, 1)  # x = 4 is not below pilot + max_extra = 3: the cap
    assert counts.tolist() == [[0, 1, 1, 1, 0]]
    mv[0, 4] = [0.0, 0.0]                          # 0 / 0 = NaN counts as +Inf: the cap at pixels 3 and 4
    counts, _ = sm.map_model(mv, 0.5, 0.0, 2, 10)
    assert counts.tolist() == [[0, 2, 2, 10, 10]]
    counts, total = sm.map_model(mv[:, :3], np.inf, 0.0, 2, 10)  # tau = +Inf: nothing where E is finite
    assert total == 0
    assert np.array_equal(T.api.sample_map_model(mv, 0.5, 0.0, 2, 10), [[0, 2, 2, 10, 10]])


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (29, 37), (64, 64)])
def test_the_packages_vectorised_map_model_is_the_loop_model(T, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    mv = np.stack([rng.normal(0.5, 0.5, shape), rng.gamma(1.0, 0.3, shape)], axis=-1).astype(F)
    flat = mv.reshape(-1, 2)
    for k, bad in enumerate([(np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (0.0, 0.0), (-np.inf, 0.5)]):
        if k < len(flat):
            flat[(k * 7) % len(flat)] = bad
    for tau, eps, pilot, max_extra in [(0.25, 0.01, 8, 56), (1.0, 0.0, 2, 3), (np.inf, 0.01, 4, 5), (0.05, 0.5, 16, 120)]:
        ref, total = sm.map_model(mv, tau, eps, pilot, max_extra)
        got = T.api.sample_map_model(mv, tau, eps, pilot, max_extra)
        assert np.array_equal(got, ref) and int(got.sum()) == total
        assert ref.max(initial=0) <= max_extra


def test_sample_map_from_film_and_region_on_a_3_by_2_film(T):
    film = camera(T, (3, 2), (1.0, 1.0)).film
    assert film.size == (2, 3) and T.api.sample_bounds_shape(film) == (4, 5, 0, 0)  # raster pixels 1..3 x 1..2, one border pixel on each side
    m = T.SampleMap.from_film(film, [[1, 2, 3], [4, 5, 6]])
    assert m.max_spp == 6 and m.counts.dtype == np.uint32
    assert m.counts.tolist() == [[1, 1, 2, 3, 3], [1, 1, 2, 3, 3], [4, 4, 5, 6, 6], [4, 4, 5, 6, 6]]
    assert m.total == 2 * (1 + 1 + 2 + 3 + 3) + 2 * (4 + 4 + 5 + 6 + 6)
    r = T.SampleMap.region(film, (1, 0, 3, 1), 7, 2)  # film pixels x 1..2 of row 0
    assert r.max_spp == 7
    assert r.counts.tolist() == [[2, 2, 7, 7, 7], [2, 2, 7, 7, 7], [2, 2, 2, 2, 2], [2, 2, 2, 2, 2]]
    wide = camera(T, (3, 2), (2.5, 1.5)).film
    assert T.api.sample_bounds_shape(wide) == (4, 7, -1, 0)
    assert T.SampleMap.from_film(wide, [[1, 2, 3], [4, 5, 6]]).counts[0].tolist() == [1, 1, 1, 2, 3, 3, 3]
    with pytest.raises(T.TraceHipError):
        T.SampleMap(np.full((4, 5), 3), 2)
    with pytest.raises(T.TraceHipError):
        T.SampleMap(np.zeros((4, 4)), 2).for_film(film)


def test_tau_for_budget_lands_within_one_percent(T):
    rng = np.random.default_rng(24)
    shape = (64, 64)
    m = rng.uniform(0.05, 2.0, shape)
    mv = np.stack([m, (m * rng.lognormal(-1.0, 1.0, shape)) ** 2], axis=-1).astype(F)
    integ = T.AdaptivePathIntegrator(camera(T, (62, 62), (1.0, 1.0)), T.SeededSampler(8, seed=1), 4, max_extra=120)
    target = 24 * 64 * 64
    tau, total = integ.tau_for_budget(mv, target)
    assert abs(total - target) <= 0.01 * target, (tau, total, target)
    assert total == int(sm.map_model(mv, tau, integ.params.eps, 8, 120)[1])


def test_parameter_block_and_the_refusals_that_need_no_device(T):
    L = T.lib()
    p = T._ffi.SampleMapParams()
    assert C.sizeof(p) == 24
    assert L.trhip_sample_map_default_params(C.byref(p)) == 0 and L.trhip_sample_map_default_params(None) == -1
    assert (p.tau, p.eps, p.pilot, p.max_extra, p.flags, p.reserved) == (0.25, F(0.01), 8, 56, 0, 0)
    mv, counts, total = np.zeros((2, 3, 2), F), np.zeros((2, 3), np.uint32), C.c_uint64(0)
    call = lambda prm: L.trhip_sample_map(None, T._ffi.fptr(mv), 3, 2, prm, T._ffi.u32ptr(counts), C.byref(total))  # noqa: E731
    err = lambda: L.trhip_last_error(None)  # noqa: E731
    assert call(None) == -1 and b"null argument" in err()
    for field, value, word in [("tau", 0.0, b"tau"), ("tau", float("nan"), b"tau"), ("eps", -1.0, b"eps"), ("eps", float("inf"), b"eps"), ("max_extra", 1 << 24, b"pilot + max_extra"),
                               ("flags", 1, b"flag"), ("reserved", 1, b"reserved")]:
        q = T._ffi.SampleMapParams.from_buffer_copy(p)
        setattr(q, field, value)
        assert call(C.byref(q)) == -1 and word in err(), field
    assert call(C.byref(p)) == -1 and b"null argument" in err()  # the block is good: now the null context
    one = np.ones(1, np.uint32)
    sn = camera(T, (3, 2), (1.0, 1.0)).sensor()
    assert L.trhip_render_path_map(None, None, C.byref(sn), T._ffi.u32ptr(one), 1, 4, 0, 0, T._ffi.fptr(mv), None) == -1 and b"null argument" in err()
    assert L.trhip_last_sample_stats(None, T._ffi.fptr(mv)) == -1 and b"null argument" in err()
    assert L.trhip_film_sum(None, T._ffi.fptr(mv), T._ffi.fptr(mv), 1, 1, T._ffi.fptr(mv)) == -1 and b"null argument" in err()
    with pytest.raises(T.TraceHipError):
        T.AdaptivePathIntegrator(camera(T, (3, 2), (1.0, 1.0)), T.SeededSampler(1), 4)
