"""A numpy Float32 model of the display pass, written from its specification (docs/design/18-display.md: M metering, R resolve, D encode) and from nothing else.  Of the
library it takes only the threshold table, which the caller passes in (trhip_display_srgb_table: the table IS the specification of the sRGB encode).  Vectorised over
pixels; every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_display_api.py (CPU) checks the model's own properties, tests/test_gpu_display.py compares the kernels with it bit for bit."""
from dataclasses import dataclass, replace  # noqa: F401 (replace: for the tests)

import numpy as np

F = np.float32
CLAMP, REINHARD, ACES = 0, 1, 2
LINEAR, SRGB = 0, 1
BIN_BASE = 856  # bits(2^-20) >> 20
MIN_Y, MAX_C = F(2.0 ** -20), F(2.0 ** 40)
# what one frame can hit (auto exposure, and LINEAR for the tie), and what only a sequence of frames or a narrow exposure range can
TALLY_KEYS = ("metered", "not_metered_w", "not_metered_dark", "not_metered_not_finite", "bin_255_clamped", "capped_2p40", "t_above_1", "t_below_0", "t_nan", "alpha_0",
              "w_nonzero_floor_0", "resolve_interpolated", "quantise_tie")
SEQUENCE_TALLY_KEYS = ("resolve_empty", "resolve_adapted", "resolve_clamped")


@dataclass
class Params:
    curve: int = REINHARD
    transfer: int = SRGB
    auto_exposure: bool = True
    flip_rows: bool = True
    exposure: float = 1.0
    key: float = 0.18
    permille: int = 500
    adapt_rate: float = 1.0
    min_exposure: float = 2.0 ** -8
    max_exposure: float = 2.0 ** 8
    white: float = 4.0


@dataclass
class State:
    exposure: np.float32 = F(0.0)
    valid: int = 0
    counted: int = 0
    key_bin: int = 0

    def words(self):
        """The 16 bytes as four uint32."""
        return np.array([np.asarray(F(self.exposure)).view(np.uint32), self.valid, self.counted, self.key_bin], np.uint32)


def _count(tally, key, n):
    if tally is not None:
        tally[key] = tally.get(key, 0) + int(n)


def xyz_to_rgb(c):
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    return np.stack([(F(3.240479) * x - F(1.537150) * y) - F(0.498535) * z, (F(-0.969256) * x + F(1.875991) * y) + F(0.041556) * z,
                     (F(0.055648) * x - F(0.204043) * y) + F(1.057311) * z], axis=-1)


def jmax0(v):
    """Base.max(0f0, v): NaN propagates, max(0, -0) = 0."""
    return np.where(np.isnan(v), v, np.where(v > 0, v, F(0.0))).astype(F)


def edge(b):
    """L(b): the lower edge of bin b, L(256) = 2^12."""
    return np.asarray((np.asarray(b, np.uint32) + np.uint32(BIN_BASE)) << np.uint32(20), np.uint32).view(F)


def meter(xyzw, scale, tally=None):
    """M: the 256 uint32 counts."""
    B = np.asarray(xyzw, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        iw = F(1.0) / B[:, 3]
        Y = (B[:, 1] * iw) * F(scale)
    wpos = B[:, 3] > 0
    counted = wpos & (Y >= MIN_Y) & (Y < F(np.inf))
    raw = (Y.view(np.uint32) >> np.uint32(20)).astype(np.int64) - BIN_BASE
    bins = np.minimum(raw[counted], 255)
    _count(tally, "metered", counted.sum())
    _count(tally, "not_metered_w", (~wpos).sum())
    _count(tally, "not_metered_dark", (wpos & (Y < MIN_Y)).sum())
    _count(tally, "not_metered_not_finite", (wpos & ~(Y < F(np.inf)) & ~(Y < MIN_Y)).sum())
    _count(tally, "bin_255_clamped", (raw[counted] > 255).sum())
    return np.bincount(bins, minlength=256).astype(np.uint32)


def resolve(hist, prm, state, tally=None):
    """R: (E, new state).  `state` None = none given: read as no state, and the returned state is what a caller who gave an all-zero one would hold."""
    s = state if state is not None else State()
    total = int(hist.astype(np.uint64).sum())
    if total == 0:
        _count(tally, "resolve_empty", 1)
        E = F(s.exposure) if s.valid else F(prm.exposure)
        return E, State(E, s.valid, 0, 0)
    cum = np.cumsum(hist.astype(np.uint64))
    want = total * int(prm.permille)
    b = int(np.argmax(cum * np.uint64(1000) >= np.uint64(want)))
    need = (want + 999) // 1000
    before = int(cum[b - 1]) if b else 0
    frac = F(need - before) / F(int(hist[b]))
    _count(tally, "resolve_interpolated", frac < 1)
    Lm = edge(b) + frac * (edge(b + 1) - edge(b))
    q = F(prm.key) / Lm
    lo, hi = F(prm.min_exposure), F(prm.max_exposure)
    Et = hi if q > hi else (lo if q < lo else q)
    _count(tally, "resolve_clamped", Et != q)
    E = Et
    if s.valid and F(prm.adapt_rate) < 1:
        _count(tally, "resolve_adapted", 1)
        E = F(s.exposure) + (Et - F(s.exposure)) * F(prm.adapt_rate)
    return F(E), State(F(E), 1, total, b)


def curve(c, prm):
    """D3: t per channel."""
    with np.errstate(all="ignore"):
        if prm.curve == CLAMP:
            return c
        if prm.curve == REINHARD:
            ww = F(prm.white) * F(prm.white)
            return (c * (F(1.0) + c / ww)) / (F(1.0) + c)
        return (c * (F(2.51) * c + F(0.03))) / (c * (F(2.43) * c + F(0.59)) + F(0.14))


def clamp01(t, tally=None):
    """D4."""
    _count(tally, "t_above_1", (t > 1).sum())
    _count(tally, "t_below_0", (t < 0).sum())
    _count(tally, "t_nan", np.isnan(t).sum())
    t = np.where(t > 1, F(1.0), np.where(t < 0, F(0.0), t))
    return np.where(np.isnan(t), F(0.0), t).astype(F)


def quantise(t, transfer, table, tally=None):
    """D5: t in [0, 1], no NaN -> uint32 codes."""
    if transfer == LINEAR:
        v = t * F(255.0)
        _count(tally, "quantise_tie", (v - np.floor(v) == F(0.5)).sum())
        return np.rint(v).astype(np.uint32)  # ties to even
    return np.searchsorted(np.asarray(table, F)[1:], t, side="right").astype(np.uint32)  # the number of k in 1..255 with T[k] <= t


def encode(xyzw, scale, prm, E, table, tally=None):
    """D: (H, W, 4) uint8."""
    B = np.asarray(xyzw, F)
    if prm.flip_rows:
        B = B[::-1]
    w = B[..., 3]
    with np.errstate(all="ignore"):
        c = xyz_to_rgb(B[..., :3])  # D1
        iw = F(1.0) / w
        floored = jmax0(c * iw[..., None])
        _count(tally, "w_nonzero_floor_0", ((w != 0)[..., None] & (c * iw[..., None] < 0)).sum())
        c = np.where((w != 0)[..., None], floored, c).astype(F)
        c = c * F(scale)
        c = c * F(E)  # D2
        _count(tally, "capped_2p40", (c > MAX_C).sum())
        c = np.where(c > MAX_C, MAX_C, c).astype(F)
        t = clamp01(np.asarray(curve(c, prm), F), tally)
    q = quantise(t, prm.transfer, table, tally)
    a = np.where(w != 0, 255, 0).astype(np.uint32)
    _count(tally, "alpha_0", (w == 0).sum())
    return np.concatenate([q, a[..., None]], axis=-1).astype(np.uint8)


def display(xyzw, scale, prm, table, state=None, tally=None):
    """The whole pass: (rgba uint8 (H, W, 4), new state or None, histogram (256,) uint32).  Without auto_exposure the state comes back as given and the histogram is zero."""
    if prm.auto_exposure:
        hist = meter(xyzw, scale, tally)
        E, new_state = resolve(hist, prm, state, tally)
    else:
        hist, E, new_state = np.zeros(256, np.uint32), F(prm.exposure), state
    return encode(xyzw, scale, prm, E, table, tally), new_state, hist


def oetf64(t):
    """IEC 61966-2-1 in Float64: linear light in [0, 1] -> encoded value."""
    t = np.asarray(t, np.float64)
    return np.where(t <= 0.0031308, 12.92 * t, 1.055 * np.power(np.maximum(t, 0.0031308), 1.0 / 2.4) - 0.055)


def synthetic_frame(h, w, seed, table):
    """(h, w, 4) Float32 with every special the specification names, wherever the frame has room for them (29 x 37 holds them all): random colours over eight
    octaves with positive weights, then, written over it from the front, NaN, +-Inf, w = 0, w < 0, negative colours, luminances at 2^-20, just below it, at 2^12 and above, a
    run of pixels in one bin, for every k a blue channel exactly T[k] and one at the Float32 just below (pixels of weight 0, whose xyz_to_rgb is used as it stands: see
    `exact_channel`; they reach D5 unchanged under CLAMP with scale and exposure 1), and blue channels whose t * 255 is an exact half-integer."""
    rng = np.random.default_rng(seed)
    n = h * w
    lum = np.exp2(rng.uniform(-6.0, 2.0, n)).astype(F)  # the median near 0.25, inside the run of one bin below
    rgb = lum[:, None] * rng.uniform(0.2, 1.0, (n, 3)).astype(F)
    wt = rng.uniform(0.5, 4.0, n).astype(F)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], F)
    xyz = (rgb @ M.T).astype(F) * wt[:, None]
    B = np.concatenate([xyz, wt[:, None]], axis=1).astype(F)
    specials = []
    inf = F(np.inf)
    specials += [(np.nan, 1, 1, 1), (1, np.nan, 1, 1), (1, 1, 1, np.nan), (inf, inf, inf, 1), (-inf, -inf, -inf, 1), (1, 1, 1, inf), (1, inf, 1, 2), (0.3, 0.2, 0.1, 0), (0, 0, 0, 0),
                 (0.3, 0.2, 0.1, -1), (-0.3, -0.2, -0.1, 1), (-0.3, 0.2, -0.1, 0), (1e30, 1e30, 1e30, 1e-8)]
    pred = lambda v: np.nextafter(F(v), F(-np.inf))  # noqa: E731
    for y in (MIN_Y, pred(MIN_Y), F(2.0 ** 12), pred(F(2.0 ** 12)), F(2.0 ** 13), F(2.0 ** 30)):  # luminance exactly y at w = 1, scale 1
        specials.append((y, y, y, 1))
    specials += [(0.25, 0.25, 0.25, 1)] * 70  # more than a wave of one bin
    B[:min(len(specials), n)] = np.array(specials, F)[:n]
    at = len(specials)
    exact = []
    for k in range(1, 256):
        for target in (table[k], pred(table[k])):
            exact.append(exact_channel(F(target)))
    for v in (F(0.5), F(1.5), F(2.5), F(126.5), F(127.5), F(254.5)):  # t * 255 an exact half-integer: t = v / 255 rounded, kept only when the product is exact
        t = v / F(255.0)
        for cand in (t, np.nextafter(t, F(0)), np.nextafter(t, F(1))):
            if cand * F(255.0) == v:
                exact.append(exact_channel(F(cand)))
                break
    room = max(0, n - at)
    for i, px in enumerate(exact[:room]):
        B[at + i] = px
    return B.reshape(h, w, 4)


def exact_channel(target):
    """A pixel (x, 0, z, 0) whose blue channel after D1 is exactly `target` > 0.  w = 0: no division and no floor.  B = (0.055648f * x - 0.204043f * 0) + 1.057311f * z: z is
    chosen so that p = 1.057311f * z lies a few ulps below the target, x so that 0.055648f * x is the (exactly representable) rest; the sum then rounds to the target."""
    bx, bz = F(0.055648), F(1.057311)
    z = F(target / bz)
    for _ in range(4):
        z = np.nextafter(z, F(0))
    p = bz * z
    x = F((target - p) / bx)
    got = (bx * x - F(0.204043) * F(0)) + p
    assert got == target and p < target, (target, got)
    return (x, F(0), z, F(0))
