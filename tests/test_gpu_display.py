"""trhip_display on the GPU: the kernels against the numpy model of tests/display_model.py, bit for bit in every RGBA byte, every histogram count and the four words
of the exposure state, at the sizes where the tiling, the grid-stride loop and the row flip change; host and device entry points, with and without a histogram and a state;
run-to-run identity; a three-frame adaptation with the state on the device; the look of `save` on a Cornell frame; PreviewSession.render_display against the same calls by
hand; the overlap refusal."""
import ctypes as C

import numpy as np
import pytest

import display_model as dm

pytestmark = pytest.mark.gpu
F = np.float32
INVALID = -1

# (h, w): smaller than a wave's 16 x 4 patch; partial tiles; partial tiles in both axes, several meter rounds; whole tiles; wider than any block, seventeen tiles in a row
SIZES = {"1x1": (1, 1), "5x3": (3, 5), "37x29": (29, 37), "64x64": (64, 64), "257x3": (3, 257)}
CURVES = {"clamp": dm.CLAMP, "reinhard": dm.REINHARD, "aces": dm.ACES}
TRANSFERS = {"linear": dm.LINEAR, "srgb": dm.SRGB}
FRAMES = {}


@pytest.fixture(scope="module")
def table(T):
    return T.Display.srgb_table()


def frame(name, table):
    if name not in FRAMES:
        h, w = SIZES[name]
        FRAMES[name] = dm.synthetic_frame(h, w, 5000 + w, table)
    return FRAMES[name].copy()


def model_params(d):
    p = d.params
    return dm.Params(curve=p.curve, transfer=p.transfer, auto_exposure=bool(p.flags & 1), flip_rows=bool(p.flags & 2), exposure=p.exposure, key=p.key,
                     permille=p.percentile_permille, adapt_rate=p.adapt_rate, min_exposure=p.min_exposure, max_exposure=p.max_exposure, white=p.white)


def state_words(s):
    """A _ffi.DisplayState, a model State or four raw words -> (4,) uint32."""
    if isinstance(s, dm.State):
        return s.words()
    if isinstance(s, np.ndarray):
        return s.view(np.uint32).reshape(4)
    return np.frombuffer(bytes(s), np.uint32)


def ffi_state(T, s: dm.State):
    return T._ffi.DisplayState(float(s.exposure), s.valid, s.counted, s.key_bin)


def check_cell(T, ctx, table, B, d, scale, prior: dm.State):
    """Every route of one parameter cell on frame B against the model."""
    h, w = B.shape[:2]
    prm = model_params(d)
    auto = prm.auto_exposure
    ref, ref_state, ref_hist = dm.display(B, scale, prm, table, prior)
    ref_none, _, _ = dm.display(B, scale, prm, table, None)
    given = B.copy()
    # host: bytes alone; with a state; with state and histogram; histogram without a state
    assert np.array_equal(d.encode(B, scale, ctx=ctx), ref_none), "host, no state"
    assert d.stats.launches_film == (3 if auto else 1)
    rgba, st = d.encode(B, scale, state=ffi_state(T, prior), ctx=ctx)
    assert np.array_equal(rgba, ref), "host, with a state"
    assert np.array_equal(state_words(st), state_words(ref_state)), (state_words(st), state_words(ref_state))
    rgba, st, hist = d.encode(B, scale, state=ffi_state(T, prior), ctx=ctx, want_histogram=True)
    assert np.array_equal(rgba, ref) and np.array_equal(hist, ref_hist) and np.array_equal(state_words(st), state_words(ref_state)), "host, state and histogram"
    rgba, st, hist = d.encode(B, scale, ctx=ctx, want_histogram=True)
    assert st is None and np.array_equal(rgba, ref_none) and np.array_equal(hist, ref_hist), "host, histogram without a state"
    assert np.array_equal(B.view(np.uint32), given.view(np.uint32)), "the input is left alone"
    # device: the same four
    d_in = T._ffi.DeviceBuffer(B.nbytes).from_host(B)
    d_out, d_state, d_hist = T._ffi.DeviceBuffer(h * w * 4), T._ffi.DeviceBuffer(16), T._ffi.DeviceBuffer(1024)
    try:
        for use_state in (False, True):
            for use_hist in (False, True):
                d_out.from_host(np.full((h, w, 4), 0x5A, np.uint8))
                d_state.from_host(prior.words())
                d_hist.from_host(np.full(256, 0xDEAD, np.uint32))
                d.encode_device(d_in.ptr, w, h, scale, d_out.ptr, d_state.ptr if use_state else None, d_hist.ptr if use_hist else None, ctx)
                what = f"device, state {use_state}, histogram {use_hist}"
                assert np.array_equal(d_out.to_host(np.uint8, (h, w, 4)), ref if use_state else ref_none), what
                want_state = ref_state if use_state else prior  # a state that was not passed is not touched
                assert np.array_equal(d_state.to_host(np.uint32, (4,)), state_words(want_state)), what
                assert np.array_equal(d_hist.to_host(np.uint32, (256,)), ref_hist if use_hist else np.full(256, 0xDEAD, np.uint32)), what
        assert np.array_equal(d_in.to_host(np.uint32, B.shape), given.view(np.uint32)), "the device input is left alone"
    finally:
        for b in (d_in, d_out, d_state, d_hist):
            b.free()


def make_display(T, curve, transfer, flip, auto):
    # CLAMP cells run at scale 1 and exposure 1, where the frame's exact thresholds reach the search unchanged
    return T.Display(curve=curve, transfer=transfer, flip_rows=flip, auto_exposure=auto, exposure=1.0 if curve == "clamp" else 1.75, adapt_rate=0.5, white=3.0)


PRIOR = dm.State(F(0.625), 1, 11, 7)  # a valid state from "the frame before": adapt_rate 0.5 moves half the way from it


@pytest.mark.parametrize("auto", [False, True], ids=["manual", "auto"])
@pytest.mark.parametrize("flip", [False, True], ids=["unflipped", "flipped"])
@pytest.mark.parametrize("transfer", sorted(TRANSFERS))
@pytest.mark.parametrize("curve", sorted(CURVES))
def test_every_cell_equals_the_model_at_37x29(T, ctx, table, curve, transfer, flip, auto):
    check_cell(T, ctx, table, frame("37x29", table), make_display(T, curve, transfer, flip, auto), 1.0 if curve == "clamp" else 1.25, PRIOR)


@pytest.mark.parametrize("cell", [("clamp", "linear"), ("reinhard", "srgb")], ids=["clamp-linear", "reinhard-srgb"])
@pytest.mark.parametrize("size", [s for s in sorted(SIZES) if s != "37x29"])
def test_diagonal_cells_equal_the_model_at_the_other_sizes(T, ctx, table, size, cell):
    for flip in (False, True):
        for auto in (False, True):
            check_cell(T, ctx, table, frame(size, table), make_display(T, cell[0], cell[1], flip, auto), 1.0 if cell[0] == "clamp" else 1.25, PRIOR if size != "1x1" else dm.State())


def test_auto_exposure_is_identical_from_run_to_run(T, ctx, table):
    B = frame("64x64", table)
    d = T.Display()
    first = d.encode(B, 1.0, state=T._ffi.DisplayState(), ctx=ctx, want_histogram=True)
    second = d.encode(B, 1.0, state=T._ffi.DisplayState(), ctx=ctx, want_histogram=True)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[2], second[2]) and bytes(first[1]) == bytes(second[1])
    assert first[1].valid == 1 and first[1].counted == int(first[2].sum()) > 1000


def test_adaptation_over_three_frames_with_the_state_on_the_device(T, ctx, table):
    base = frame("37x29", table)
    bright = (base * np.array([4, 4, 4, 1], F)).astype(F)
    black = np.zeros_like(base)
    black[..., 3] = 1.0
    d = T.Display(adapt_rate=0.5)
    prm = model_params(d)
    h, w = base.shape[:2]
    d_in, d_out, d_state = T._ffi.DeviceBuffer(base.nbytes), T._ffi.DeviceBuffer(h * w * 4), T._ffi.DeviceBuffer(16).zero()
    state, exposures = dm.State(), []
    try:
        for k, B in enumerate((base, bright, black)):
            ref, state, _ = dm.display(B, 1.0, prm, table, state)
            d_in.from_host(B)
            d.encode_device(d_in.ptr, w, h, 1.0, d_out.ptr, d_state.ptr, None, ctx)
            got = d_state.to_host(np.uint32, (4,))
            assert np.array_equal(got, state.words()), (k, got, state.words())
            assert np.array_equal(d_out.to_host(np.uint8, (h, w, 4)), ref), k
            exposures.append(got[:1].view(F)[0])
    finally:
        for b in (d_in, d_out, d_state):
            b.free()
    assert exposures[1] < exposures[0], "a brighter frame lowers the exposure"
    assert exposures[2] == exposures[1] and state.valid == 1 and state.counted == 0, "nothing metered: the exposure is kept"


def camera(T, resolution):
    film = T.Film([resolution, resolution], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at([0, 15, 50], [0, 0, -2], [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def test_reference_display_has_the_look_of_save(T, ctx, tmp_path):
    scene, cam = T.scenes.cornell_scene(), camera(T, 32)
    xyzw = T.PathIntegrator(cam, T.SeededSampler(4, seed=0xD15), 5).render(scene)
    assert not np.isnan(xyzw).any(), "the comparison is stated for NaN-free pixels"
    film = cam.film
    film.set_xyzw(xyzw)
    want = np.clip(np.rint(film.to_rgb(ctx)[::-1] * 255), 0, 255).astype(np.uint8)
    rgba = T.Display.reference().encode(xyzw, film.scale, ctx=ctx)
    assert rgba.shape == (32, 32, 4) and np.array_equal(rgba[..., :3], want)
    assert np.array_equal(rgba[..., 3], np.where(xyzw[::-1, :, 3] != 0, 255, 0))
    assert len(np.unique(want)) > 32, "a frame with content"
    # Display.save writes those bytes
    from PIL import Image
    film.filename = str(tmp_path / "reference.png")
    T.Display.reference().save(film, ctx)
    assert np.array_equal(np.asarray(Image.open(film.filename)), want)


@pytest.mark.parametrize("upscaled", [False, True], ids=["native", "upscaled"])
def test_render_display_is_render_then_encode_with_the_state_carried(T, ctx, upscaled):
    scene, spp, depth, seed = T.scenes.cornell_scene(), 2, 3, 0xBEEF
    cams = [camera(T, 32), camera(T, 32)]
    kw = dict(upscaler=T.Upscaler(), factor=2, guide_spp=1) if upscaled else {}
    d = T.Display(adapt_rate=0.5)
    shown = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, display=d, **kw)
    plain = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, **kw)
    by_hand = T.Display(adapt_rate=0.5)
    state = T._ffi.DisplayState()
    try:
        for k, cam in enumerate(cams):
            xyzw = plain.render(cam, ctx)
            assert xyzw.shape == (32, 32, 4)
            want, state = by_hand.encode(xyzw, cam.film.scale, state=state, ctx=ctx)
            got = shown.render_display(cam, ctx)
            assert got.dtype == np.uint8 and np.array_equal(got, want), f"frame {k}"
            assert len(shown.render_stats) == len(plain.render_stats) + 1 and shown.render_stats[-1].launches_film == 3
            held = shown._display_buffers[1].to_host(np.uint32, (4,))
            assert np.array_equal(held, state_words(state)), f"the state on the device after frame {k}"
        assert state.valid == 1 and state.counted > 500
        shown.reset()
        assert not shown._display_buffers[1].to_host(np.uint32, (4,)).any(), "reset() clears the exposure state"
        # render() of a session that has a display makes the calls of one that has none
        shown.close()
        plain.close()
        a = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, display=d, **kw)
        b = T.PreviewSession(scene, T.SeededSampler(spp, seed=seed), depth, **kw)
        for k, cam in enumerate(cams):
            ra, rb = a.render(cam, ctx), b.render(cam, ctx)
            assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), f"render(), frame {k}"
            assert len(a.render_stats) == len(b.render_stats)
        a.close()
        b.close()
    finally:
        shown.close()
        plain.close()


def test_overlap_and_device_side_refusals(T, ctx, table):
    B = frame("37x29", table)
    h, w = B.shape[:2]
    d, L = T.Display(), T.lib()
    big = T._ffi.DeviceBuffer(B.nbytes + h * w * 4)
    try:
        def call(out, w_=w, h_=h, in_=big.ptr):
            return L.trhip_display_device(ctx._h, C.c_void_p(in_) if in_ else None, w_, h_, 1.0, C.byref(d.params), None, C.c_void_p(out) if out else None, None, None)
        big.from_host(np.concatenate([B.reshape(-1).view(np.uint8), np.zeros(h * w * 4, np.uint8)]))
        assert call(big.ptr) == INVALID and b"out_rgba overlaps" in L.trhip_last_error(ctx._h)
        assert call(big.ptr + B.nbytes - 4) == INVALID and b"out_rgba overlaps" in L.trhip_last_error(ctx._h), "the last pixel"
        assert call(big.ptr + 16, in_=big.ptr + h * w * 4) == INVALID and b"out_rgba overlaps" in L.trhip_last_error(ctx._h), "the output's tail over the input's head"
        assert call(big.ptr + B.nbytes) == 0, "adjacent is not overlapping"
        assert np.array_equal(big.to_host(np.uint8, (B.nbytes + h * w * 4,))[B.nbytes:].reshape(h, w, 4), dm.display(B, 1.0, model_params(d), table)[0])
        assert call(None) == INVALID and b"null argument" in L.trhip_last_error(ctx._h)
        assert call(big.ptr + B.nbytes, in_=None) == INVALID and b"null argument" in L.trhip_last_error(ctx._h)
        assert call(big.ptr + B.nbytes, w_=0) == INVALID and b"empty" in L.trhip_last_error(ctx._h)
        assert call(big.ptr + B.nbytes, h_=0) == INVALID and b"empty" in L.trhip_last_error(ctx._h)
        assert call(big.ptr + B.nbytes, w_=1 << 16, h_=1 << 15) == INVALID and b"2^31" in L.trhip_last_error(ctx._h)
    finally:
        big.free()
    with pytest.raises(T.TraceHipError):
        d.encode(B[..., :3], 1.0, ctx=ctx)
