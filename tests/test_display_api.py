"""The display pass without a GPU: the default parameter block, every refusal of the block in the header's order (reported with a NULL context: the code is the
parameter's), the sRGB threshold table against the Float64 OETF, and the numpy model of tests/display_model.py against its own specification."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import display_model as dm

F = np.float32
INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(T):
    return T.Display.srgb_table()


def pred(v):
    return np.nextafter(F(v), F(-np.inf))


def succ(v):
    return np.nextafter(F(v), F(np.inf))


def test_defaults_need_no_gpu(T):
    p = T._ffi.DisplayParams()
    assert T.lib().trhip_display_default_params(C.byref(p)) == 0
    assert C.sizeof(p) == 48 and C.sizeof(T._ffi.DisplayState) == 16
    assert (p.curve, p.transfer, p.flags, p.percentile_permille) == (1, 1, 3, 500)
    assert (p.exposure, p.key, p.adapt_rate, p.min_exposure, p.max_exposure, p.white) == (1.0, float(F(0.18)), 1.0, 2.0 ** -8, 2.0 ** 8, 4.0)
    assert tuple(p.reserved) == (0, 0)
    assert T.lib().trhip_display_default_params(None) == INVALID
    assert T.lib().trhip_display_srgb_table(None) == INVALID
    d = T.Display()
    assert bytes(d.params) == bytes(p)
    r = T.Display.reference().params
    assert (r.curve, r.transfer, r.flags, r.exposure) == (0, 0, 2, 1.0)
    d = T.Display(curve="aces", transfer="linear", auto_exposure=False, flip_rows=False, exposure=2.0, key=0.25, percentile=0.9, adapt_rate=0.5, min_exposure=0.5, max_exposure=4.0,
                  white=8.0).params
    assert (d.curve, d.transfer, d.flags, d.exposure, d.key, d.percentile_permille, d.adapt_rate, d.min_exposure, d.max_exposure, d.white) == (2, 0, 0, 2.0, 0.25, 900, 0.5, 0.5, 4.0, 8.0)
    with pytest.raises(T.TraceHipError):
        T.Display(curve="filmic")
    with pytest.raises(T.TraceHipError):
        T.PreviewSession(None, None, 1).render_display(None)


# (what to break, the words of the message), in the order the header gives; each case also carries every LATER fault, so the first one reported shows the order
REFUSALS = [
    ("curve", dict(curve=3), b"curve"),
    ("transfer", dict(transfer=2), b"transfer"),
    ("flags", dict(flags=7), b"unknown flag bits"),
    ("exposure", dict(exposure=0.0), b"exposure must be"),
    ("exposure nan", dict(exposure=float("nan")), b"exposure must be"),
    ("key", dict(key=float("inf")), b"key must be"),
    ("min_exposure", dict(min_exposure=-1.0), b"min_exposure must be"),
    ("max_exposure", dict(max_exposure=float("nan")), b"max_exposure must be"),
    ("min > max", dict(min_exposure=2.0, max_exposure=1.0), b"min_exposure exceeds"),
    ("permille 0", dict(percentile_permille=0), b"percentile_permille"),
    ("permille 1001", dict(percentile_permille=1001), b"percentile_permille"),
    ("adapt_rate 0", dict(adapt_rate=0.0), b"adapt_rate"),
    ("adapt_rate > 1", dict(adapt_rate=1.5), b"adapt_rate"),
    ("adapt_rate nan", dict(adapt_rate=float("nan")), b"adapt_rate"),
    ("white small", dict(white=2.0 ** -11), b"white"),
    ("white large", dict(white=2.0 ** 21), b"white"),
    ("white nan", dict(white=float("nan")), b"white"),
    ("scale", dict(scale=float("inf")), b"scale is not finite"),
    ("scale nan", dict(scale=float("nan")), b"scale is not finite"),
    ("reserved", dict(reserved=1), b"reserved"),
]
ORDER = ["curve", "transfer", "flags", "exposure", "key", "min_exposure", "max_exposure", "min > max", "permille 0", "adapt_rate 0", "white small", "scale", "reserved"]


def _broken(T, faults):
    p = T._ffi.DisplayParams.from_buffer_copy(T.Display().params)
    scale = 1.0
    for name, value in faults.items():
        if name == "scale":
            scale = value
        elif name == "reserved":
            p.reserved[1] = value
        else:
            setattr(p, name, value)
    return p, scale


def _call(T, p, scale, device=False):
    L = T.lib()
    if device:
        return L.trhip_display_device(None, None, 4, 4, scale, C.byref(p) if p is not None else None, None, None, None, None)
    return L.trhip_display(None, None, 4, 4, scale, C.byref(p) if p is not None else None, None, None, None, None)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_parameter_refusals_in_the_stated_order(T, device):
    L = T.lib()
    assert _call(T, None, 1.0, device) == INVALID and b"null argument" in L.trhip_last_error(None)
    cases = dict((name, (faults, words)) for name, faults, words in REFUSALS)
    for name, faults, words in REFUSALS:
        p, scale = _broken(T, faults)
        assert _call(T, p, scale, device) == INVALID, name
        assert words in L.trhip_last_error(None), (name, L.trhip_last_error(None))
    # the order: a block with faults k, k + 1, ... reports fault k
    for k, name in enumerate(ORDER):
        faults = {}
        for later in reversed(ORDER[k:]):  # ORDER[k]'s own values are applied last and win the fields two faults share
            faults.update(cases[later][0])
        p, scale = _broken(T, faults)
        assert _call(T, p, scale, device) == INVALID
        assert cases[name][1] in L.trhip_last_error(None), (name, faults, L.trhip_last_error(None))
    # a sound block with a NULL context: the null pointer is reported only now
    p, scale = _broken(T, {})
    assert _call(T, p, scale, device) == INVALID and b"null argument" in L.trhip_last_error(None)


def test_table_is_strictly_increasing_and_brackets_the_oetf(table):
    assert table.dtype == np.float32 and table.shape == (256,) and table[0] == 0
    assert np.all(np.diff(table) > 0)
    assert abs(float(table[1]) - 1.5176e-4) < 1e-8 and abs(float(table[255]) - 0.995545) < 1e-6
    k = np.arange(1, 256)
    at = 255.0 * dm.oetf64(table[1:].astype(np.float64))
    below = 255.0 * dm.oetf64(pred(table[1:]).astype(np.float64))
    assert np.all(at >= k - 0.5 - 1e-9), "T[k] lies below eotf((k - 0.5) / 255)"
    assert np.all(below < k - 0.5 + 1e-9), "T[k] is not the smallest Float32 at or above eotf((k - 0.5) / 255)"


def test_committed_table_is_what_the_generator_writes():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_srgb_table.py"), "--check"]) == 0, \
        "trace.jl_amd/csrc/th_display_srgb.h is not what tools/gen_srgb_table.py writes"


def test_model_quantisation_is_the_rounded_oetf(table):
    rng = np.random.default_rng(2718)
    t = np.concatenate([rng.random(1 << 16, dtype=np.float32), table, pred(table[1:]), succ(table), np.array([0.0, 1.0], F)])
    t = t[(t >= 0) & (t <= 1)].astype(F)
    ref = np.floor(255.0 * dm.oetf64(t.astype(np.float64)) + 0.5).astype(np.uint32)
    got = dm.quantise(t, dm.SRGB, table)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} of {t.size} codes differ"
    # the search the kernel runs: eight steps over T[0..255]
    q = np.zeros(t.shape, np.uint32)
    for step in (128, 64, 32, 16, 8, 4, 2, 1):
        q += np.where(t >= table[q + step], step, 0).astype(np.uint32)
    assert np.array_equal(q, got)


def test_model_takes_every_branch_on_the_frame_the_kernels_are_given(table):
    B = dm.synthetic_frame(29, 37, 5037, table)
    tally = {}
    dm.display(B, 1.0, dm.Params(), table, None, tally)
    dm.display(B, 1.0, dm.Params(curve=dm.CLAMP, transfer=dm.LINEAR, auto_exposure=False), table, None, tally)
    assert all(tally.get(k, 0) > 0 for k in dm.TALLY_KEYS), tally
    # every threshold and its lower neighbour reach the search unchanged: both codes of every k appear in the blue channel
    out, _, _ = dm.display(B, 1.0, dm.Params(curve=dm.CLAMP, transfer=dm.SRGB, auto_exposure=False, flip_rows=False), table)
    blue = out[..., 2].reshape(-1)
    w0 = B[..., 3].reshape(-1) == 0
    with np.errstate(all="ignore"):
        t = dm.xyz_to_rgb(B[..., :3]).reshape(-1, 3)[:, 2]
    for k in range(1, 256):
        assert np.any(w0 & (t == table[k]) & (blue == k)) and np.any(w0 & (t == pred(table[k])) & (blue == k - 1)), k


def test_bytes_are_monotone_in_t_per_curve(table):
    c = np.concatenate([np.exp2(np.linspace(-24, 41, 4000)), [0.0]]).astype(F)
    c.sort()
    frame = np.zeros((1, c.size, 4), F)
    frame[0, :, 2] = c / F(1.057311)  # blue = 1.057311f * z, w = 0: monotone in z
    for curve in (dm.CLAMP, dm.REINHARD, dm.ACES):
        for transfer in (dm.LINEAR, dm.SRGB):
            for white in (0.5, 4.0):
                out, _, _ = dm.display(frame, 1.0, dm.Params(curve=curve, transfer=transfer, auto_exposure=False, white=white), table)
                assert np.all(np.diff(out[0, :, 2].astype(int)) >= 0), (curve, transfer, white)
                assert out[0, 0, 2] == 0 and (out[0, -1, 2] == 255 or curve == dm.ACES)


def test_flip_is_a_row_reversal(table):
    B = dm.synthetic_frame(29, 37, 5037, table)
    for auto in (False, True):
        up, s_up, h_up = dm.display(B, 1.0, dm.Params(flip_rows=False, auto_exposure=auto), table)
        down, s_down, h_down = dm.display(B, 1.0, dm.Params(flip_rows=True, auto_exposure=auto), table)
        assert np.array_equal(down, up[::-1]) and np.array_equal(h_up, h_down) and s_up == s_down


def test_state_carries_the_exposure(table):
    B = dm.synthetic_frame(29, 37, 5037, table)
    black = np.zeros_like(B)
    black[..., 3] = 1.0
    tally = {}
    prm = dm.Params(adapt_rate=1.0)
    _, s1, h1 = dm.display(B, 1.0, prm, table, dm.State(), tally)
    E1, _ = dm.resolve(h1, prm, None)
    assert s1.valid == 1 and s1.counted == int(h1.sum()) and s1.exposure == E1, "with adapt_rate 1 the state's exposure is Et"
    # nothing to meter: a valid state keeps its exposure, no state falls back to params.exposure
    _, s2, h2 = dm.display(black, 1.0, prm, table, s1, tally)
    assert h2.sum() == 0 and (s2.exposure, s2.valid, s2.counted, s2.key_bin) == (s1.exposure, 1, 0, 0)
    _, s3, _ = dm.display(black, 1.0, dm.Params(exposure=0.75), table, dm.State(), tally)
    assert (s3.exposure, s3.valid, s3.counted, s3.key_bin) == (F(0.75), 0, 0, 0)
    _, s4, _ = dm.display(black, 1.0, dm.Params(exposure=0.75), table, None, tally)
    assert s4.exposure == F(0.75)
    # smoothing moves half the way; a narrow range clamps
    half = dm.Params(adapt_rate=0.5)
    _, s5, _ = dm.display(B * F(4.0) * np.array([1, 1, 1, 0.25], F), 1.0, half, table, s1, tally)
    Et, _ = dm.resolve(dm.meter(B * F(4.0) * np.array([1, 1, 1, 0.25], F), 1.0), half, None)
    assert s5.exposure == s1.exposure + (Et - s1.exposure) * F(0.5) and Et < s1.exposure
    _, s6, _ = dm.display(B, 1.0, dm.Params(min_exposure=8.0, max_exposure=16.0), table, None, tally)
    assert s6.exposure == F(8.0)
    assert all(tally.get(k, 0) > 0 for k in dm.SEQUENCE_TALLY_KEYS), tally
