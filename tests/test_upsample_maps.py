"""The pixel-map table of tests/upsample_maps.py, checked on the CPU from the specification and the numpy models alone (docs/design/17-upscale.md, "The pixel-map space"):

(a) the footprint claim of the staged kernels — every tap of every lane lies inside the square its block stages — swept in Float32 over the maps the ABI accepts, with a
    count of how often the spare staged column T - 1 is reached and whether it ever carries weight;
(b) the preconditions of tests/test_gpu_upsample_maps.py: each named map reaches, in the models, the branch or the staged index it is named for, so nothing on the device
    can hide behind inputs that never get there.

Nothing here calls into the library."""
import math
import time

import numpy as np
import pytest

import temporal_upsample_model as tum
import temporal_upsample_motion_model as tumm
import upsample_maps as maps
import upscale_model as um

F = np.float32
TILE = maps.TILE
MAX_BLOCK = 65534


# ---- (a) the footprint ---------------------------------------------------------------------------------------------------------------------------------------------
def footprint(a, offsets, blocks):
    """One axis, H3 in Float32 for every lane of `blocks` and every offset.  With d = floor(fx) - floor(fx of the block's first column) and C = ceil(15 a), the guided taps
    x0 + 1 - R .. x0 + R have the staged indices d .. d + 2 R - 1 of T = C + 1 + 2 R (the unguided ones, x0 and x0 + 1, lie between them), whatever R is: a tap lies outside
    the square iff d < 0 or d > C + 1, and the last one lies on the spare column T - 1 iff d = C + 1.  T is taken from this axis's scale alone (the kernels' T is that of
    the larger scale: never smaller).  Returns (lanes with a tap outside, lanes on the spare column, those of them with t > 0, lanes)."""
    a, b = F(a), np.asarray(offsets, F)[:, None, None]
    C = int(math.ceil(15.0 * float(a)))
    first = (blocks.astype(np.int32) * TILE)[None, :, None]
    x = first + np.arange(TILE, dtype=np.int32)[None, None, :]
    f = x.astype(F) * a
    f = f + b
    f0 = np.floor(f)
    fb = first.astype(F) * a
    fb = fb + b
    d = f0 - np.floor(fb)  # whole numbers below 2^21: exact in Float32
    spare = d == C + 1
    return int(np.sum((d < 0) | (d > C + 1))), int(spare.sum()), int((spare & (f > f0)).sum()), int(d.size)


def sweep_scales():
    rng = np.random.default_rng(1517)
    scales = []
    for k in range(4, 16):
        s = F(k / 15.0)
        scales += [np.nextafter(np.nextafter(s, F(0)), F(0)), np.nextafter(s, F(0)), s, np.nextafter(s, F(2)), np.nextafter(np.nextafter(s, F(2)), F(2))]
    scales += list(rng.uniform(0.25, 1.0, 200).astype(F))
    scales += [F(v) for c in maps.CASES.values() for v in (c.lo_from_hi[0], c.lo_from_hi[2])]
    return sorted({float(s) for s in scales if 0.25 <= float(s) <= 1.0})


def sweep_offsets():
    out = [0.0, 0.25, -0.75, 0.999, -0.001]
    for e in range(8, 20):
        p = F(2.0 ** e)
        for v in (np.nextafter(p, F(0)), p, np.nextafter(p, F(np.inf))):
            out += [float(v), -float(v)]
        out += [float(-p + F(0.4375)), float(-p / 2 + F(0.96875))]  # the sums cancel into a finer binade than the products'
    out += [2.0 ** 20 - 40, -(2.0 ** 20 - 40), float(np.nextafter(F(2.0 ** 20), F(0))), -float(np.nextafter(F(2.0 ** 20), F(0)))]
    out += [float(v) for c in maps.CASES.values() for v in (c.lo_from_hi[1], c.lo_from_hi[3])]
    return sorted(set(out))


def sweep_blocks(a):
    """0 .. 199, the last one, and the blocks at which x * a crosses a power of two (the product's rounding step doubles there)."""
    blocks = [np.arange(200), [MAX_BLOCK - 1, MAX_BLOCK]]
    for e in range(8, 20):
        k = int(2.0 ** e / float(a)) // TILE
        blocks.append(np.clip(np.arange(k - 2, k + 3), 0, MAX_BLOCK))
    return np.unique(np.concatenate([np.asarray(b, np.int64) for b in blocks]))


def test_footprint_every_tap_lies_in_the_staged_square_and_the_spare_column_carries_no_weight():
    """Per scale: blocks 0 .. 199 and the blocks around every power of two of x * a against every offset, and 3000 random blocks up to 65 534 against the offsets of
    magnitude >= 2^16 (2^20 - 40 among them) and sixteen of the others drawn per scale.  Both radii are covered by one pass (see `footprint`).  Measured: see
    docs/design/17-upscale.md, "The pixel-map space", which also gives the argument for the assertion on the spare column: the only tap that can lie on staged column T - 1
    is the guided tap x0 + R, whose tent weight is tx / R, and it gets there only when fx was rounded up onto a whole number."""
    rng = np.random.default_rng(2017)
    scales, offsets = sweep_scales(), np.array(sweep_offsets())
    assert len(scales) >= 250 and len(offsets) >= 80
    always = np.abs(offsets) >= 2.0 ** 16
    total = dict.fromkeys(("lanes", "outside", "spare", "spare_with_weight"), 0)
    t0 = time.perf_counter()
    for a in scales:
        some = always | np.isin(np.arange(len(offsets)), rng.choice(len(offsets), 16, replace=False))
        for blocks, offs in ((sweep_blocks(a), offsets), (rng.integers(200, MAX_BLOCK + 1, 3000), offsets[some])):
            outside, spare, weighted, lanes = footprint(a, offs, blocks)
            for k, v in zip(("lanes", "outside", "spare", "spare_with_weight"), (lanes, outside, spare, weighted)):
                total[k] += v
            assert outside == 0, (a, outside)
    print(f"footprint sweep: {len(scales)} scales, {len(offsets)} offsets, R = 1 and 2 alike, {total['lanes']} lanes: {total['outside']} with a tap outside the square, "
          f"{total['spare']} whose tap x0 + R lies on staged column T - 1, {total['spare_with_weight']} of them with tx > 0; {time.perf_counter() - t0:.1f} s")
    assert total["spare"] > 0, "the sweep reaches the spare column"
    assert total["spare_with_weight"] == 0


def test_the_smallest_example_on_the_spare_column():
    """ax = 1, bx = nextafter(1024, 0): x + bx lies halfway between two Float32 numbers from x = 1 and is rounded to the even one, the whole number x + 1024; the first
    block's own first column (x = 0) keeps 1023.99994, so floor(fx) grows by 16 = ceil(15 ax) + 1 over that block, at its lane 15 — with tx = 0.  Later blocks start on a
    rounded-up position themselves."""
    outside, spare, weighted, _ = footprint(1.0, [maps.BELOW_1024], np.arange(3))
    assert (outside, spare, weighted) == (0, 1, 0)


# ---- (b) preconditions, from the models ----------------------------------------------------------------------------------------------------------------------------
def guided_taps(lo, lp, hp, m, R):
    """Per guided tap (j outer, i inner) of H4 with the temporal passes' parameters: (accepted, off_image, staged x index, staged y index, qx, qy) over the full-size pixels."""
    prm = tum.Params(m, radius=R)
    up = tum.upscale_params(prm)
    surface = tum.surface_and_confidence(lo, lp, hp, prm)[0]
    s_q = um.low_records(np.ascontiguousarray(lo, F), np.ascontiguousarray(lp, F), up)[0]
    (h, w), (lh, lw) = hp.shape[:2], lo.shape[:2]
    x0, y0, _, _ = um.positions(up, h, w)
    lx = maps.local_indices(m[0], m[1], w, R)[0][None, :]
    ly = maps.local_indices(m[2], m[3], h, R)[0][:, None]
    for j in range(2 * R):
        for i in range(2 * R):
            qx, qy = x0 + 1 - R + i, y0 + 1 - R + j
            inside = (qx >= 0) & (qx < lw) & (qy >= 0) & (qy < lh)
            accepted = surface & inside & s_q[np.clip(qy, 0, lh - 1), np.clip(qx, 0, lw - 1)]
            yield accepted, surface & ~inside, np.broadcast_to(lx + i, (h, w)), np.broadcast_to(ly + j, (h, w)), qx, qy


def accepted_indices(name, R):
    lo, lp, hp, m = maps.upscale_frames(name)
    xs, ys = set(), set()
    for accepted, _, ix, iy, _, _ in guided_taps(lo, lp, hp, m, R):
        xs |= set(np.unique(ix[accepted]).tolist())
        ys |= set(np.unique(iy[accepted]).tolist())
    return xs, ys


def test_table_reaches_the_staged_widths_and_strides_it_names():
    tw = {(n, R): maps.staged_width(maps.CASES[n].lo_from_hi, R) for n in maps.CASES for R in (1, 2)}
    assert (tw["tw16_r1", 1], tw["tw16_r1", 2]) == (16, 18) and (tw["tw16_r2", 1], tw["tw16_r2", 2]) == (14, 16)
    assert (tw["tw17", 1], tw["tw17", 2]) == (17, 19) and (tw["tw17_edge", 1], tw["tw17_edge", 2]) == (17, 19)
    assert maps.stride_of(16) == 16 and maps.stride_of(17) == 32
    new = sorted(set(tw.values()) - set(maps.OLD_STAGED_WIDTHS))
    print("staged widths of the table:", sorted(set(tw.values())), "new:", new)
    assert {14, 16, 17, 19} <= set(new)
    for c in maps.CASES.values():
        assert not maps.is_old_map(c.lo_from_hi), f"{c.name} is a map the old suite launched"
        for v in c.lo_from_hi[::2]:
            assert 0.25 <= v <= 1.0
        for v in c.lo_from_hi[1::2]:
            assert abs(v) < 2.0 ** 20
        assert c.hi[0] <= TILE * 65535 and c.hi[1] <= TILE * 65535


@pytest.mark.parametrize("name", [n for n in maps.SMALL if maps.CASES[n].in_image] + ["spare_column"])
def test_guided_share_of_every_in_image_map(name):
    """At least a quarter of the pixels of positive weight are guided (mask 1), in each of the three models, with history."""
    c = maps.CASES[name]
    lo, lp, hp, m, Hs, M, ids, table, bodies = maps.motion_frames(name)
    weighted = hp[..., 0, 3] > 0
    for R in c.radii:
        _, mask_u = um.upscale(lo, lp, hp, tum.upscale_params(tum.Params(m, radius=R)))
        _, _, mask_t = tum.accumulate(lo, lp, hp, Hs, M, tum.Params(m, radius=R))
        _, _, mask_m = tumm.accumulate(lo, lp, hp, Hs, M, ids, table, bodies, tumm.Params(m, radius=R))
        shares = [float(((mk & 3) == 1).sum()) / float(weighted.sum()) for mk in (mask_u, mask_t, mask_m)]
        print(f"guided share {name} R={R}: {shares[0]:.3f} {shares[1]:.3f} {shares[2]:.3f}; history found at {int((mask_t >= 4).sum())} and {int((mask_m >= 4).sum())} pixels")
        assert min(shares) >= 0.25, (name, R, shares)


def test_window_has_no_tap_off_the_image():
    lo, lp, hp, m = maps.upscale_frames("window")
    for R in (1, 2):
        tally = {}
        um.upscale(lo, lp, hp, tum.upscale_params(tum.Params(m, radius=R)), tally)
        assert tally["tap_off_image"] == 0 and tally["guided"] > 0
        assert not any(off.any() for _, off, _, _, _, _ in guided_taps(lo, lp, hp, m, R))
    assert m[1] > 0 and m[3] > 0


@pytest.mark.parametrize("name,sides", [("off_left_top", ("left", "top")), ("off_right_bottom", ("right", "bottom"))])
def test_off_image_maps_have_accepted_taps_beside_skipped_ones(name, sides):
    """On each named side some pixel has an accepted tap on the image's border column (row) and a skipped one just beyond it; off_right_bottom's last block column and
    last block row stage nothing of the image."""
    lo, lp, hp, m = maps.upscale_frames(name)
    lh, lw = lo.shape[:2]
    for R in (1, 2):
        taps = list(guided_taps(lo, lp, hp, m, R))
        on = {"left": lambda qx, qy: qx == 0, "right": lambda qx, qy: qx == lw - 1, "top": lambda qx, qy: qy == 0, "bottom": lambda qx, qy: qy == lh - 1}
        beyond = {"left": lambda qx, qy: qx == -1, "right": lambda qx, qy: qx == lw, "top": lambda qx, qy: qy == -1, "bottom": lambda qx, qy: qy == lh}
        for side in sides:
            border = np.any([acc & on[side](qx, qy) for acc, _, _, _, qx, qy in taps], axis=0)
            skipped = np.any([off & beyond[side](qx, qy) for _, off, _, _, qx, qy in taps], axis=0)
            assert (border & skipped).any(), (name, R, side)
    if name == "off_right_bottom":
        (h, w), (ax, bx, ay, by) = hp.shape[:2], m
        for R in (1, 2):
            assert maps.positions_1d(ax, bx, [(w - 1) // TILE * TILE])[0][0] + 1 - R >= lw, "the last block column's square lies beyond the image"
            assert maps.positions_1d(ay, by, [(h - 1) // TILE * TILE])[0][0] + 1 - R >= lh, "the last block row's square lies beyond the image"
        assert maps.positions_1d(ax, bx, [(w - 1) // TILE * TILE - TILE])[0][0] < lw, "the block column before it lies partly on it"


@pytest.mark.parametrize("name,axis", [("wide_x", "y"), ("wide_y", "x")])
def test_anisotropic_maps_use_staged_indices_the_other_axis_would_clamp(name, axis):
    """On the axis of scale 1 accepted taps lie at staged indices >= the T that the other axis's scale alone would give, in more than two blocks along that axis."""
    c = maps.CASES[name]
    ax, _, ay, _ = c.lo_from_hi
    small = min(ax, ay)
    assert max(ax, ay) == 1.0 and (c.hi[0] if axis == "y" else c.hi[1]) > 2 * TILE
    for R in (1, 2):
        wrong = int(math.ceil(15.0 * small)) + 1 + 2 * R
        xs, ys = accepted_indices(name, R)
        beyond = [v for v in (ys if axis == "y" else xs) if v >= wrong]
        print(f"{name} R={R}: T = {maps.staged_width(c.lo_from_hi, R)}, from the other axis alone {wrong}; accepted taps at staged {axis} indices {sorted(beyond)}")
        assert len(beyond) >= 8 and max(beyond) == maps.staged_width(c.lo_from_hi, R) - 2
        assert max(xs if axis == "y" else ys) < wrong, "the narrow axis stays inside its own bound"


@pytest.mark.parametrize("name,R", [("tw16_r1", 1), ("tw16_r2", 2), ("tw17_edge", 1), ("tw17", 1)])
def test_stride_edge_maps_use_the_last_staged_columns_and_rows(name, R):
    """Accepted taps at the two highest staged indices a lane reaches without the spare column, T - 3 and T - 2, on both axes.  `tw17` is the issue's map: its blocks start
    at 14 k + 0.1, floor(fx) grows by 13 only, and T - 3 = 14 is its highest index; `tw17_edge` has the same scale at offsets 0.9 and 0.95 and reaches 15."""
    tw = maps.staged_width(maps.CASES[name].lo_from_hi, R)
    xs, ys = accepted_indices(name, R)
    top = tw - 3 if name == "tw17" else tw - 2
    assert max(xs) == top and max(ys) == top and {top - 1, top} <= xs and {top - 1, top} <= ys, (name, tw, sorted(xs), sorted(ys))
    assert 0 in xs and 0 in ys


def test_spare_column_has_an_in_image_tap_on_the_last_staged_column():
    lo, lp, hp, m = maps.upscale_frames("spare_column")
    for R in (1, 2):
        tw = maps.staged_width(m, R)
        n = 0
        for accepted, _, ix, iy, _, _ in guided_taps(lo, lp, hp, m, R):
            n += int((accepted & ((ix == tw - 1) | (iy == tw - 1))).sum())
        print(f"spare_column R={R}: {n} accepted (pixel, tap) pairs on staged column or row T - 1 = {tw - 1}")
        assert n > 0
    maps.release("spare_column")


def test_union_of_the_maps_takes_every_branch_of_every_model():
    """Every key of each model's TALLY_KEYS is taken by some small map (R = 2, with history; the motion model's two keys of calls without ids or table by such calls)."""
    union = {k: dict.fromkeys(keys, 0) for k, keys in (("upscale", um.TALLY_KEYS), ("temporal", tum.TALLY_KEYS), ("motion", tumm.TALLY_KEYS))}
    slowest = 0.0
    for name in maps.SMALL:
        lo, lp, hp, m, Hs, M, ids, table, bodies = maps.motion_frames(name)
        t0 = time.perf_counter()
        tallies = {"upscale": {}, "temporal": {}, "motion": {}}
        um.upscale(lo, lp, hp, um.Params(m), tallies["upscale"])
        tum.accumulate(lo, lp, hp, Hs, M, tum.Params(m), tallies["temporal"])
        tumm.accumulate(lo, lp, hp, Hs, M, ids, table, bodies, tumm.Params(m), tallies["motion"])
        slowest = max(slowest, time.perf_counter() - t0)
        if name == "tw16_r1":
            for kw in (dict(ids=None, bodies=bodies), dict(ids=ids, bodies=None)):  # a call without an id plane, a call without matrices
                extra = {}
                tumm.accumulate(lo, lp, hp, Hs, M, kw["ids"], table, kw["bodies"], tumm.Params(m), extra)
                for k in ("static_no_ids", "static_no_table"):
                    tallies["motion"][k] = tallies["motion"].get(k, 0) + extra[k]
        for which, t in tallies.items():
            for k, v in t.items():
                union[which][k] += v
    for which, t in union.items():
        print(f"tallies over the small maps, {which}: {t}")
        assert all(v > 0 for v in t.values()), (which, [k for k, v in t.items() if v == 0])
    print(f"slowest small case, three models: {slowest:.2f} s")
    assert slowest < 3.0


@pytest.mark.parametrize("name", maps.LARGE)
def test_model_time_of_the_large_cases(name):
    """The one model evaluation each kernel's GPU case makes of a large map (maps.large_frames: R = 1; the strips without history) stays under about 3 s.  Measured
    here: spare_column 0.4 - 0.5 s, strip_x 1.6 / 2.8 / 2.9 s, strip_y 1.9 / 3.0 / 3.0 s (upscale / temporal / motion); the line is drawn at 3.5 s."""
    c = maps.CASES[name]
    lo, lp, hp, m, Hs, M, ids, table, bodies = maps.large_frames(name)
    assert hp.shape[:2] == c.hi and lo.shape[:2] == c.lo and ids.shape == c.hi
    times = []
    for call in (lambda: um.upscale(lo, lp, hp, tum.upscale_params(tum.Params(m, radius=1))), lambda: tum.accumulate(lo, lp, hp, Hs, M, tum.Params(m, radius=1)),
                 lambda: tumm.accumulate(lo, lp, hp, Hs, M, ids, table, bodies, tumm.Params(m, radius=1))):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    print(f"model time {name}: upscale {times[0]:.2f} s, temporal {times[1]:.2f} s, motion {times[2]:.2f} s")
    maps.release(name)
    assert max(times) < 3.5


def test_spare_column_decides_the_confidence_when_the_sharpness_is_below_one_over_R():
    """The tent weight of the tap on staged column T - 1 is 0, but 19-temporal-upsample.md's confidence weights the same tap by max(0, 1 - rho R) at tx = 0: positive for
    rho < 1 / R.  With confidence_sharpness = 0, taking the low column that only lane 15 of the first block column reads through staged column T - 1 (x0 + 1 = 1040 for
    x = 15) out of the surface changes kmax at x = 15: the record staged there is used, so the GPU case runs the temporal two with rho = 0."""
    lo, lp, hp, m = maps.upscale_frames("spare_column")
    prm = tum.Params(m, radius=1, confidence_sharpness=0.0)
    x0, t = maps.positions_1d(m[0], m[1], [15])
    assert (int(x0[0]), float(t[0])) == (1039, 0.0) and maps.local_indices(m[0], m[1], 16, 1)[0][15] + 1 == maps.staged_width(m, 1) - 1
    kmax = tum.surface_and_confidence(lo, lp, hp, prm)[3]
    without = lp.copy()
    without[:, 1040, 1, 3] = F(0.0)  # H = 0: no surface pixel, the tap is skipped
    changed = kmax[:, 15] != tum.surface_and_confidence(lo, without, hp, prm)[3][:, 15]
    print(f"spare_column, rho = 0: kmax at x = 15 depends on the record on staged column T - 1 in {int(changed.sum())} of {changed.size} rows")
    assert changed.any()
    sharp = tum.Params(m, radius=1, confidence_sharpness=2.0)
    assert np.array_equal(tum.surface_and_confidence(lo, lp, hp, sharp)[3][:, 15], tum.surface_and_confidence(lo, without, hp, sharp)[3][:, 15]), "at rho = 2 it does not"
    maps.release("spare_column")
