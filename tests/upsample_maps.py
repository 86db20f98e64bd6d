"""The pixel maps the three upsampling kernels (trhip_upscale, trhip_temporal_upsample, trhip_temporal_upsample_motion) are tested over: named maps
lo_from_hi = (ax, bx, ay, by), each with the smallest images that exercise it, and the frames the three synthetic generators make of them
(docs/design/17-upscale.md, "The pixel-map space").

Not a test: tests/test_upsample_maps.py (CPU) checks from the models alone that every map reaches what it is named for, tests/test_gpu_upsample_maps.py compares the
kernels with the models bit for bit on every one."""
import math
from dataclasses import dataclass

import numpy as np

import temporal_upsample_model as tum
import temporal_upsample_motion_model as tumm
import upscale_model as um

F = np.float32
TILE = 16  # the kernels' block is 16 x 16 full-size pixels


@dataclass(frozen=True)
class Case:
    name: str
    lo_from_hi: tuple  # (ax, bx, ay, by)
    hi: tuple          # full-size (h, w)
    lo: tuple          # low (h, w)
    radii: tuple = (1, 2)
    large: bool = False     # host entry point only, one call per kernel
    in_image: bool = True   # the full-size image falls (mostly) on the low image: the guided share is asserted


def staged_width(lo_from_hi, R):
    """T of docs/design/17-upscale.md: ceil(15 a) + 1 + 2 R, a the larger scale (the scales as Float32, the product in Float64)."""
    a = max(float(F(lo_from_hi[0])), float(F(lo_from_hi[2])))
    return int(math.ceil(15.0 * a)) + 1 + 2 * R


def stride_of(tw):
    return 16 if tw <= 16 else 32


def fit(hi, m, R=2):
    """The low (h, w) that holds the farthest tap x0 + R of the last full-size column and row (and at least 8 x 8, for the generators' planted pixels)."""
    (hh, hw), (ax, bx, ay, by) = hi, (float(F(v)) for v in m)
    return (max(8, int(math.floor((hh - 1) * ay + by)) + R + 1), max(8, int(math.floor((hw - 1) * ax + bx)) + R + 1))


BELOW_1024 = float(np.nextafter(F(1024.0), F(0.0)))
STRIP = TILE * 65535  # 1 048 560: the largest grid on an axis


def _case(name, m, hi, lo=None, **kw):
    return Case(name, tuple(float(F(v)) for v in m), hi, lo if lo is not None else fit(hi, m, max(kw.get("radii", (1, 2)))), **kw)


CASES = {c.name: c for c in (
    _case("tw16_r1", (0.86, -0.3, 0.86, 0.4), (45, 70)),                    # T = 16 at R = 1 (the last square on stride 16), 18 at R = 2
    _case("tw16_r2", (0.73, 0.2, 0.73, -0.6), (45, 70)),                    # T = 16 at R = 2, 14 at R = 1
    _case("tw17", (0.875, 0.1, 0.875, 0.1), (45, 70)),                      # T = 17 at R = 1 (the first square on stride 32), 19 at R = 2
    _case("tw17_edge", (0.875, 0.9, 0.875, 0.95), (45, 70)),                # the same T with blocks that start at 14 k + 0.9: floor(fx) grows by 14, staged index T - 2 is used
    _case("wide_x", (0.3, -0.4, 1.0, 0.25), (45, 40)),                      # T decided by y; three blocks along y
    _case("wide_y", (1.0, -1.5, 0.25, 0.6), (45, 70)),                      # T decided by x; five blocks along x
    _case("third", (1.0 / 3.0, -1.0, 1.0 / 3.0, -1.0), (45, 70)),           # many integer positions
    _case("f2_6", (1.0 / 2.6, 0.37, 1.0 / 2.6, -0.81), (45, 70)),
    _case("window", (0.5, 7.3, 0.7, 5.1), (45, 70), (46, 52)),              # the mapped extent is [7.3, 41.8] x [5.1, 35.9]: six low pixels to spare on every side
    _case("off_left_top", (0.5, -3.4, 0.5, -2.7), (45, 70)),
    _case("off_right_bottom", (0.5, 0.3, 0.5, 0.6), (45, 70), (14, 30), in_image=False),  # the last block column starts at 32.3, the last block row at 16.6: R = 2 stages from 31 and 15
    _case("far", (0.5, 1000.25, 0.5, -1000.25), (29, 37), (16, 16), in_image=False),
    _case("spare_column", (1.0, BELOW_1024, 1.0, BELOW_1024), (17, 33), (1060, 1100), large=True),     # x + bx rounds up to an integer from x = 1: the tap x0 + R lies on staged column T - 1
    _case("strip_x", (0.5, 0.3, 1.0, 0.0), (1, STRIP), (2, STRIP // 2 + 2), radii=(1,), large=True),
    _case("strip_y", (1.0, 0.0, 0.5, 0.3), (STRIP, 1), (STRIP // 2 + 2, 2), radii=(1,), large=True),
)}
SMALL = tuple(n for n, c in CASES.items() if not c.large)
LARGE = tuple(n for n, c in CASES.items() if c.large)

# what the GPU suite launched before this table existed (worked out from the SIZES tables of the three GPU modules and the factor-2 sessions): the scales and the T values
OLD_SCALES = ((0.5, 0.5), (19 / 37, 15 / 29), (3 / 5, 2 / 3), (0.25, 0.25), (1.0, 1.0))
OLD_STAGED_WIDTHS = (7, 9, 11, 13, 15, 18, 20)




def _halton(k):
    def radical_inverse(base, i):
        f, r = 1.0, 0.0
        while i > 0:
            f /= base
            r += f * (i % base)
            i //= base
        return r
    return radical_inverse(2, k + 1) - 0.5, radical_inverse(3, k + 1) - 0.5


# ... and the maps themselves: upscale_model.synthetic_pair's (a, 1.5 a - 1.5) for the six size pairs, the arithmetic case, and the factor-2 sessions on an uncropped film,
# (0.5, -0.25 + jx, 0.5, -1.25 + jy) without jitter, on the grid and on the first Halton frames
OLD_MAPS = tuple((ax, 1.5 * ax - 1.5, ay, 1.5 * ay - 1.5) for ax, ay in OLD_SCALES) + ((0.5, -0.75, 0.5, -0.75),) + tuple(
    (0.5, -0.25 + jx, 0.5, -1.25 + jy) for jx, jy in ((0.0, 0.0), (0.25, 0.25), (-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25)) + tuple(_halton(k) for k in range(16)))


def is_old_map(m):
    """Is (ax, bx, ay, by) one of the maps the GPU suite launched before this table existed?"""
    return any(all(abs(float(v) - o) < 1e-5 for v, o in zip(m, old)) for old in OLD_MAPS)


_FRAMES = {}


def seed_of(case):
    return 4000 + case.hi[1] % 1000


def upscale_frames(name):
    """(lo_xyzw, lo_planes, hi_planes, lo_from_hi): computed once per case, handed out as copies."""
    return _cached("u", name, um.synthetic_pair)


def temporal_frames(name):
    """(lo_xyzw, lo_planes, hi_planes, lo_from_hi, history, M)"""
    return _cached("t", name, tum.synthetic)


def motion_frames(name):
    """(lo_xyzw, lo_planes, hi_planes, lo_from_hi, history, M, ids, body_of_prim, bodies)"""
    return _cached("m", name, tumm.synthetic)


def large_frames(name):
    """The nine arrays of motion_frames for a large case, shared by the three kernels' one call each.  spare_column: motion_frames.  The strips, whose subject is the
    rounding of fx in part U: upscale_frames, NO history (the history lookup does not involve the map, and the generator's history costs a model evaluation of a million
    pixels), temporal_upsample_model's matrix, and motion_model's 29 x 37 id plane laid side by side with its table and matrices."""
    if name == "spare_column":
        return motion_frames(name)
    key = ("l", name)
    for other in [k for k in _FRAMES if k[0] == "l" and k != key]:  # one strip at a time
        del _FRAMES[other]
    if key not in _FRAMES:
        c = CASES[name]
        lo, lp, hp, m = upscale_frames(name)
        src = tumm.mm.synthetic(29, 37, seed_of(c))
        ids = np.ascontiguousarray(np.tile(src[3], (-(-c.hi[0] // 29), -(-c.hi[1] // 37)))[:c.hi[0], :c.hi[1]])
        _FRAMES[key] = (lo, lp, hp, m, None, tum.synthetic_matrix(c.hi[0], c.hi[1], m), ids, src[4], tumm.synthetic_bodies())
        _FRAMES.pop(("u", name), None)
    return _FRAMES[key]  # not copied: nobody writes into them


def _cached(kind, name, make):
    key = (kind, name)
    if key not in _FRAMES:
        c = CASES[name]
        _FRAMES[key] = make(c.hi[0], c.hi[1], c.lo[0], c.lo[1], seed_of(c), c.lo_from_hi)
    return tuple(a.copy() if isinstance(a, np.ndarray) else a for a in _FRAMES[key])


def release(name):
    """Drops the cached frames of a case (the large ones hold hundreds of megabytes)."""
    for kind in "utml":
        _FRAMES.pop((kind, name), None)


# ---- H3 and the staged square, from docs/design/17-upscale.md alone --------------------------------------------------------------------------------------------
def positions_1d(a, b, xs):
    """H3's two Float32 operations for integer coordinates xs (a lane's, or a block's first column): (x0 int64, t Float32)."""
    f = np.asarray(xs, np.int64).astype(F) * F(a)
    f = f + F(b)
    f0 = np.floor(f)
    return f0.astype(np.int64), (f - f0).astype(F)


def local_indices(a, b, n, R):
    """Per full-size coordinate 0 .. n - 1: the staged index of its first guided tap x0 + 1 - R (the last one is 2 R - 1 further), and t."""
    xs = np.arange(n, dtype=np.int64)
    x0, t = positions_1d(a, b, xs)
    ox = positions_1d(a, b, (xs // TILE) * TILE)[0] + 1 - R
    return x0 + 1 - R - ox, t
