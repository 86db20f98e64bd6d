"""Trees that fill the 64-entry traversal stack, the rays that fill it, and two plain models of the walks (no GPU, no library).

Every traversal kernel keeps the first levels of its per-ray stack in LDS and the rest in a global overflow slab or in scratch, 64 entries in all (bvh.jl:222).  The
number of fast levels differs per kernel (FAST_LEVELS below); the code on either side of that boundary is different code.  The trees here are CATERPILLARS — every interior
node is {one leaf of one triangle, the rest} — handed over through trhip_scene_set_bvh, so a ray whose direction makes the interior child the near one at every node pushes
one entry per level and holds D - 1 entries on a chain of D triangles.

  caterpillar(D, layout)    D "slat" triangles along x, node arrays in the reference's depth-first layout (the get_bvh / set_bvh format), boxes from the Float32 vertices
  ray_families(tree)        reverse / forward (open and through the slats), origins between every two slats, finite t_max, d.x = +-0 and axis-parallel rays
  model_a(...)              accel/bvh.jl:212-299 written plainly over the node arrays, the primitive test a callable: hit primitive, occlusion, stack entries held
  fold4 / model_b(...)      the four-wide fold of the accelerator and the order and count of the pushes of the four-wide walk
  brute_force(...)          every ray against every triangle, Moeller-Trumbore in Float64, with the "safe ray" predicate

What "D" counts.  trhip_scene_set_bvh and trhip_scene_commit refuse a tree whose max_depth exceeds 64, where max_depth counts NODES on the longest root-to-leaf path, the root
being 1.  A chain of D triangles has D - 1 interior nodes; its two deepest leaves sit at depth D.  The deepest accepted chain is D = 64 and the reference's loop holds at most
63 entries on it (one per interior node); D = 65 is refused.  (bvh.jl:222 itself has room for 64 entries, i.e. D = 65: the library refuses one level early, never late.)
"""
import numpy as np

f32 = np.float32

STACK_TOTAL = 64  # kStack2Total = kStackLds + kStackSpill
# kernel -> stack levels it keeps in LDS; the rest of the 64 live in scratch (k_trace_closest / k_trace_any) or in the global overflow slab (all others)
FAST_LEVELS = {"k_trace_closest": 32, "k_trace_any": 32, "k_trace2": 16, "k_trace3 closest": 12, "k_trace3 any": 10, "k_trace3c": 11, "k_trace3c4": 12}
LEVELS = tuple(sorted(set(FAST_LEVELS.values())))  # (10, 11, 12, 16, 32)
DEEPEST = 64  # the deepest chain set_bvh accepts (tests/test_gpu_deep_trees.py asserts it and the refusal of 65)
# a chain of D slats holds at most D - 1 entries: D = L, L + 1, L + 2 put the deepest entry at level L - 1, L, L + 1 of every fast-level count L
DEPTHS = tuple(sorted({L + k for L in LEVELS for k in (0, 1, 2)} | {40, DEEPEST}))
LAYOUTS = ("leaf_first", "leaf_second")

SLAT_HALF = 0.2  # half extent of a slat along x (the slats are tilted: their boxes have a thickness)
TAPER = 0.002    # slat i spans [TAPER * i, 1 - TAPER * i] in y and z: the boxes of the chain nest strictly
WINDOW = (0.52, 0.73)  # y and z of the "open" rays: above the hypotenuse y + z = 1 every slat shares, inside every slat's box


class Tree:
    """bounds (n, 6) Float32, a, flags, order (the set_bvh arrays), tris (D, 3, 3) Float32 in caller order, and the chain's description."""

    def __init__(self, D, layout, tris, bounds, a, flags, order):
        self.D, self.layout, self.tris = D, layout, tris
        self.bounds, self.a, self.flags, self.order = bounds, a, flags, order
        self.mirror = layout == "leaf_second"

    @property
    def arrays(self):
        return self.bounds, self.a, self.flags, self.order

    @property
    def name(self):
        return f"D={self.D},{self.layout}"

    def x_of(self, s):
        """World x of chain coordinate s (slat i sits at s = i)."""
        return (self.D - 1) - s if self.mirror else s

    @property
    def deep_sign(self):
        """Sign of d.x that makes the interior child the near one at every node."""
        return 1.0 if self.mirror else -1.0

    def leaf_box(self, i):
        node = (2 * i + 1 if i < self.D - 1 else 2 * self.D - 2) if not self.mirror else (self.D - 1 if i == self.D - 1 else 2 * self.D - 2 - i)
        return self.bounds[node]


def slat_triangles(D, mirror):
    """Slat i at chain coordinate i: vertices A (t, t), B (1 - t, t), C (t, 1 - t) in (y, z), t = TAPER * i — the lower-left half of its box, hypotenuse on y + z = 1 —, tilted
    along the chain (A at -SLAT_HALF, B at +SLAT_HALF, C at 0).  Float64, then rounded once to Float32: the scene IS what Float32 holds."""
    tris = np.empty((D, 3, 3), np.float64)
    for i in range(D):
        t = TAPER * i
        s = np.array([i - SLAT_HALF, i + SLAT_HALF, float(i)])
        tris[i, :, 0] = (D - 1) - s if mirror else s
        tris[i, :, 1] = [t, 1.0 - t, t]
        tris[i, :, 2] = [t, t, 1.0 - t]
    return tris.astype(f32)


def caterpillar(D, layout):
    """leaf_first: interior i = node 2 i, its first child (node 2 i + 1) the leaf of slat i, its second child a[i] the rest; the slats run along +x.
    leaf_second: interior i = node i, its first child (node i + 1) the rest, its second child a[i] the leaf of slat i; the slats run along -x (the chain mirrored), so that in
    both layouts the rays that fill the stack meet the deepest leaf first.  Split axis x everywhere; one primitive per leaf."""
    assert D >= 2 and layout in LAYOUTS
    mirror = layout == "leaf_second"
    tris = slat_triangles(D, mirror)
    lb = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)  # Float32 boxes of the Float32 vertices
    n = 2 * D - 1
    bounds = np.empty((n, 6), f32)
    a = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint32)
    leaf_flag = np.uint32((1 << 2) | 3)
    rest = lb[D - 1].copy()  # box of slats i .. D - 1, built from the deep end
    rest_boxes = [None] * D
    rest_boxes[D - 1] = rest.copy()
    for i in range(D - 2, -1, -1):
        rest = np.concatenate([np.minimum(rest[:3], lb[i, :3]), np.maximum(rest[3:], lb[i, 3:])])
        rest_boxes[i] = rest.copy()
    if not mirror:
        order = np.arange(D, dtype=np.uint32)
        for i in range(D - 1):
            bounds[2 * i], a[2 * i], flags[2 * i] = rest_boxes[i], 2 * i + 2, 0
            bounds[2 * i + 1], a[2 * i + 1], flags[2 * i + 1] = lb[i], i, leaf_flag
        bounds[n - 1], a[n - 1], flags[n - 1] = lb[D - 1], D - 1, leaf_flag
    else:
        order = np.arange(D - 1, -1, -1).astype(np.uint32)  # depth-first: slat D - 1 is the first leaf of the array
        for i in range(D - 1):
            bounds[i], a[i], flags[i] = rest_boxes[i], 2 * D - 2 - i, 0
            bounds[2 * D - 2 - i], a[2 * D - 2 - i], flags[2 * D - 2 - i] = lb[i], D - 1 - i, leaf_flag
        bounds[D - 1], a[D - 1], flags[D - 1] = lb[D - 1], 0, leaf_flag
    return Tree(D, layout, tris, bounds, a, flags, order)


def twin_chains(D):
    """Two leaf_first chains of D slats side by side under one root (split axis y): chain A as caterpillar(D, "leaf_first") in y 0 .. 1, chain B its mirror image in y 1 .. 2
    (the open halves of both face the plane y = 1).  max_depth D + 1.  Rays that start on y = 1 and drift to either side descend one chain or the other: at the same stack level
    two such rays hold DIFFERENT entries, which a single chain cannot offer (there every deep ray's entry at level l is the leaf of slat l).  Returns (tris (2 D, 3, 3), arrays)."""
    ta = slat_triangles(D, False)
    tb = ta.astype(np.float64)
    tb[:, :, 1] = 2.0 - tb[:, :, 1]
    tb = tb.astype(f32)
    A, B = caterpillar_arrays(ta), caterpillar_arrays(tb)
    nA = A[1].size
    n = 1 + 2 * nA
    bounds, a, flags = np.empty((n, 6), f32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    bounds[0] = np.concatenate([np.minimum(A[0][0, :3], B[0][0, :3]), np.maximum(A[0][0, 3:], B[0][0, 3:])])
    a[0], flags[0] = 1 + nA, 1
    for off, slot0, (b, aa, ff) in ((1, 0, A), (1 + nA, D, B)):
        leaf = (ff & 3) == 3
        bounds[off:off + nA], flags[off:off + nA] = b, ff
        a[off:off + nA] = np.where(leaf, aa + slot0, aa + off)  # a leaf's first slot, an interior node's second child
    return np.concatenate([ta, tb]), (bounds, a, flags, np.arange(2 * D, dtype=np.uint32))


def caterpillar_arrays(tris):
    """(bounds, a, flags) of the leaf_first caterpillar over tris[0], tris[1], ...: node 2 i = {leaf of tris[i] at 2 i + 1, the rest at 2 i + 2}, slot i = triangle i."""
    D = tris.shape[0]
    lb = np.concatenate([tris.min(axis=1), tris.max(axis=1)], axis=1)
    n = 2 * D - 1
    bounds, a, flags = np.empty((n, 6), f32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rest = lb[D - 1].copy()
    for i in range(D - 2, -1, -1):
        rest = np.concatenate([np.minimum(rest[:3], lb[i, :3]), np.maximum(rest[3:], lb[i, 3:])])
        bounds[2 * i], a[2 * i], flags[2 * i] = rest, 2 * i + 2, 0
        bounds[2 * i + 1], a[2 * i + 1], flags[2 * i + 1] = lb[i], i, (1 << 2) | 3
    bounds[n - 1], a[n - 1], flags[n - 1] = lb[D - 1], D - 1, (1 << 2) | 3
    return bounds, a, flags


def tree_depth(a, flags):
    """max_depth as trhip_scene_set_bvh counts it: nodes on the longest root-to-leaf path, the root being 1."""
    best, todo = 0, [(0, 1)]
    while todo:
        i, dep = todo.pop()
        best = max(best, dep)
        if (int(flags[i]) & 3) != 3:
            todo.append((i + 1, dep + 1))
            todo.append((int(a[i]), dep + 1))
    return best


def nests(bounds, a, flags):
    """Every child box inside its parent's (what set_bvh requires before it lets the default kernels at a tree)."""
    for i in range(a.size):
        if (int(flags[i]) & 3) != 3:
            for c in (i + 1, int(a[i])):
                if not (np.all(bounds[c, :3] >= bounds[i, :3]) and np.all(bounds[c, 3:] <= bounds[i, 3:])):
                    return False
    return True


# ---- rays ----------------------------------------------------------------------------------------------------------------------------------------------------------
def rays8(o, d, tmax=np.inf):
    """The project's 8-float ray: origin, t_max, direction, time (attack_scenes.rays8)."""
    r = np.empty((o.shape[0], 8), f32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmax, d, 0.0
    return r


def _window(rng, n):
    return rng.uniform(WINDOW[0], WINDOW[1], (n, 2))


def _segment_rays(tree, s0, s1, yz0, yz1, tmax=np.inf):
    """Rays from chain coordinate s0 at (y, z) = yz0 towards s1 at yz1 (direction not normalised: t runs 0 .. 1 over the segment, scaled below to a chain-length of order 1)."""
    s0, s1 = np.broadcast_to(np.asarray(s0, np.float64), (yz0.shape[0],)), np.broadcast_to(np.asarray(s1, np.float64), (yz0.shape[0],))
    o = np.stack([tree.x_of(s0), yz0[:, 0], yz0[:, 1]], axis=1)
    e = np.stack([tree.x_of(s1), yz1[:, 0], yz1[:, 1]], axis=1)
    d = e - o
    d /= np.abs(d[:, :1])  # |d.x| = 1: t is the distance along the chain
    return rays8(o.astype(f32), d.astype(f32), tmax)


def _through_slat(tree, rng, n, k, deep):
    """(y, z) at both ends of the chain of rays that cross the shared hypotenuse y + z = 1 half way between slat k and the slat met before it: open at every slat met before k,
    a hit on slat k, 0.002 away (in y + z) from the edge on either side."""
    D = tree.D
    k = np.asarray(k, np.float64)
    sc = k + 0.5 if deep else k - 0.5  # chain coordinate of the crossing
    u = rng.uniform(-0.15, 0.15, n)
    slope = 0.004  # change of y + z per unit of chain length
    w = rng.uniform(0.2, 0.8, n)  # how the slope is shared between y and z

    def yz(s):  # y + z - 1 is > 0 (open) on the side the ray comes from
        g = slope * (s - sc) * (1.0 if deep else -1.0)
        return np.stack([0.5 + u + w * g, 0.5 - u + (1.0 - w) * g], axis=1)

    s_start, s_end = (D + 0.5, -1.5) if deep else (-1.5, D + 0.5)
    return s_start, s_end, yz(np.full(n, s_start)), yz(np.full(n, s_end))


def ray_families(tree, seed=1):
    """About 4 000 rays in named families (dict name -> (n, 8) Float32).  "deep" rays have the sign of d.x that makes the interior child the near one at every node (one push per
    level); "forward" rays the other sign (never more than one entry)."""
    D = tree.D
    rng = np.random.default_rng(seed * 1000 + D * 2 + tree.mirror)
    fam = {}
    far_deep, far_fwd = D + 0.5, -1.5  # chain coordinates beyond either end
    for name, deep in (("reverse", True), ("forward", False)):
        s0, s1 = (far_deep, far_fwd) if deep else (far_fwd, far_deep)
        fam[f"{name}, open"] = _segment_rays(tree, s0, s1, _window(rng, 256), _window(rng, 256))
        k = rng.integers(0, D, 512)
        a, b, y0, y1 = _through_slat(tree, rng, 512, k, deep)
        fam[f"{name}, through the slats"] = _segment_rays(tree, a, b, y0, y1)
    # origins between slats j and j + 1 (and before slat 0), heading the deep way.  The reference's box test keeps the LARGER of the x and y exits (bounds.jl:190), so it enters the
    # boxes BEHIND an origin that lies inside their y range: such a ray ("in the cross-section") holds D - 1 entries in the reference's loop whatever j is, and j in the kernels
    # that add the two lost clauses (model_a(kernel_like=True)).  A ray that starts just below the boxes' y range and climbs into it ("from below") fails `ty_min > tx_max` on every
    # box behind it: I_0 .. I_j push, the reference's peak is j + 1.  Per gap 16 rays from below and 8 in the cross-section, 64 more of each at every level a fast-level count puts on a
    # boundary and at the top
    special = [peak - 1 for L in LEVELS for peak in (L - 1, L, L + 1) if peak <= D - 1] + [D - 2]
    lo, hi = TAPER * (D - 1) + 0.01, 1.0 - TAPER * (D - 1) - 0.01
    gaps = np.asarray(list(range(-1, D - 1)) * 16 + [j for j in special for _ in range(64)], np.float64)
    z0 = rng.uniform(lo, hi, gaps.size)
    yz0 = np.stack([np.full(gaps.size, -0.01), z0], axis=1)
    yz1 = np.stack([-0.01 + 0.5 * (gaps + 2.0), np.clip(z0 + rng.uniform(-0.05, 0.05, gaps.size), lo, hi)], axis=1)  # y climbs 0.5 per unit of chain length
    fam["inside, from below"] = _segment_rays(tree, gaps + 0.5, np.full(gaps.size, far_fwd), yz0, yz1)
    # (in the kernels' form the walk goes from I_j straight into leaf j when the rest behind the origin is missed, without a push: their peak is j, not j + 1)
    special = [peak for L in LEVELS for peak in (L - 1, L, L + 1) if peak <= D - 2]
    gaps = np.asarray(list(range(-1, D - 1)) * 8 + [j for j in special for _ in range(64)], np.float64)
    yz0 = rng.uniform(lo, hi, (gaps.size, 2))
    yz1 = np.clip(yz0 + rng.uniform(-0.05, 0.05, yz0.shape), lo, hi)
    fam["inside, in the cross-section"] = _segment_rays(tree, gaps + 0.5, np.full(gaps.size, far_fwd), yz0, yz1)
    g = rng.integers(-1, D, 256).astype(np.float64)
    yz0 = rng.uniform(lo, hi, (256, 2))
    fam["inside, forward"] = _segment_rays(tree, g + 0.5, np.full(256, far_deep), yz0, np.clip(yz0 + rng.uniform(-0.05, 0.05, yz0.shape), lo, hi))
    # a finite t_max that ends between two slats (|d.x| = 1: t_max is a chain length); every box of the deep rays is still entered, the popped leaves beyond t_max are culled
    n = 512
    deep = np.arange(n) < n // 2
    s0 = np.where(deep, far_deep, far_fwd)
    s1 = np.where(deep, far_fwd, far_deep)
    stop = rng.integers(0, D - 1, n) + 0.5
    yz0 = rng.uniform(lo, hi, (n, 2))
    fam["finite t_max"] = _segment_rays(tree, s0, s1, yz0, np.clip(yz0 + rng.uniform(-0.05, 0.05, yz0.shape), lo, hi), np.abs(stop - s0).astype(f32))
    # d.x = +-0 and axis-parallel rays: 1 / d = Inf, and where the origin lies in a box plane the slab product is 0 * Inf = NaN
    n = 512
    o = np.empty((n, 3), f32)
    d = np.zeros((n, 3), f32)
    kind = np.arange(n) % 8
    ks = rng.integers(0, D, n)
    for j in range(n):
        box = tree.leaf_box(int(ks[j]))
        y, z = rng.uniform(lo, hi, 2)
        if kind[j] in (0, 1):  # along the chain, both ways; every fourth ray inside a box's y or z plane
            sgn = 1.0 if kind[j] == 0 else -1.0
            o[j] = [tree.x_of(far_fwd if sgn * tree.deep_sign < 0 else far_deep), y, z]
            if j % 32 < 8:  # y exactly in a plane of slat ks[j]'s box: the upper one (beside the slat), or — 4 rays, they run along the slat's edge A-C and are not "safe" — the lower one
                o[j, 1] = box[1] if j % 256 < 8 else box[4]
                o[j, 2] = rng.uniform(0.55, 0.7)
            d[j] = [sgn, 0.0, 0.0]
        elif kind[j] in (2, 3, 4, 5):  # across the chain along y or z: d.x = +0 or -0; x inside a slat's extent, in a gap, or exactly in a plane of a slat's box
            ax = 1 if kind[j] in (2, 3) else 2
            sgn = 1.0 if kind[j] in (2, 4) else -1.0
            where = (j // 8) % 3
            x = box[0] if where == 0 else (box[3] if where == 1 else f32(tree.x_of(ks[j] + rng.uniform(-0.7, 0.7))))
            o[j] = [x, y, z]
            o[j, ax] = -0.5 if sgn > 0 else 1.5
            d[j, ax] = sgn
            d[j, 0] = 0.0 if (j // 24) % 2 else -0.0
        else:  # d.x = +-0, both other components non-zero
            o[j] = [f32(tree.x_of(ks[j] + rng.uniform(-0.7, 0.7))), -0.5, rng.uniform(lo, hi)]
            d[j] = [0.0 if kind[j] == 6 else -0.0, 1.0, rng.uniform(-0.2, 0.2)]
    fam["d.x = 0 and axis-parallel"] = rays8(o, d)
    return fam


def all_rays(fams):
    return np.concatenate(list(fams.values()))


# ---- model A: the reference's loop -----------------------------------------------------------------------------------------------------------------------------------
def _check_direction(d):
    """-0 -> +0 (the reference normalises the direction's zeros before it takes 1 / d)."""
    d = np.array(d, f32)
    d[d == 0] = f32(0.0)
    return d


def _box_test32(b, o, inv, neg, tmax, tight=False):
    """bounds.jl:186-206 as written, in Float32, for rows of boxes and rays: the LARGER of the x and y exits, no robustness factor; a NaN fails every comparison.
    tight: with the two clauses that test lost (the z entry against the SMALLER of the x and y exits, and that exit not behind the origin), as the slab kernels add them."""
    near = np.where(neg, b[:, 3:], b[:, :3])
    far = np.where(neg, b[:, :3], b[:, 3:])
    with np.errstate(invalid="ignore", over="ignore"):
        tn = ((near - o) * inv).astype(f32)
        tf = ((far - o) * inv).astype(f32)
        tmin, tmx = tn[:, 0].copy(), tf[:, 0].copy()
        ok = ~((tmin > tf[:, 1]) | (tn[:, 1] > tmx))
        tmin = np.where(tn[:, 1] > tmin, tn[:, 1], tmin)
        tmx = np.where(tf[:, 1] > tmx, tf[:, 1], tmx)
        ok &= ~((tmin > tf[:, 2]) | (tn[:, 2] > tmx))
        tmin = np.where(tn[:, 2] > tmin, tn[:, 2], tmin)
        tmx = np.where(tf[:, 2] < tmx, tf[:, 2], tmx)
        ok &= (tmin < tmax) & (tmx > 0)
        if tight:
            exit_xy = np.fmin(tf[:, 0], tf[:, 1])
            ok &= ~(tn[:, 2] > exit_xy) & ~(exit_xy < 0)
        return ok


def model_a(arrays, rays, prim_test, any_hit=False, kernel_like=False, budget=None, budgeted_rounds=19):
    """accel/bvh.jl:212-258 (closest hit) and :260-299 (any hit) over the set_bvh arrays, all rays in lockstep: one node per ray and round.

    prim_test(rays8 (m, 8) with the rays' CURRENT t_max and normalised zeros, caller primitive indices (m,), any_hit) -> (hit (m,) bool, t (m,) Float32).
    Returns prim (caller index of the hit, -1), slot (its position in `order`: what the oracle and the kernels report), t_max at the end, occluded, peak (the most stack
    entries held at any time) and peak_fetch (the most entries held when an INTERIOR node is fetched — what a walk that is suspended at an interior fetch has to carry).

    kernel_like: the same walk as k_trace2 / k_trace3 keep its stack — the box test with the two lost clauses (no margin), both children tested at their parent, the far child
    pushed only if the ray enters its box, and taken at once, without a push, when the near child is missed.  Same hits; other stack counts.

    budget: the streaming wavefront's fetch budget (th_trace2.h): a ray is suspended before interior fetch number m * budget + 1, m = 1 ... budgeted_rounds (max_depth + 16
    budgeted rounds; after them a ray runs to its end), with the entries it holds; on resume those at level 16 and above go back into the overflow slab through the
    `lvl >= kStack2Lds` branch.  Returned then: suspended_at (the most entries held at a suspension) and hit_restored (the ray's closest hit was found in a leaf whose stack
    entry went through that branch at least once)."""
    bounds, a, flags, order = arrays
    a, flags, order = a.astype(np.int64), flags.astype(np.int64), order.astype(np.int64)
    slot_of = np.full(int(order.max()) + 1, -1, np.int64)
    slot_of[order] = np.arange(order.size)
    n = rays.shape[0]
    cur_rays = np.array(rays, f32)
    cur_rays[:, 4:7] = _check_direction(rays[:, 4:7])
    o, d = cur_rays[:, 0:3], cur_rays[:, 4:7]
    with np.errstate(divide="ignore"):
        inv = (f32(1.0) / d).astype(f32)
    neg = d < 0
    no_limit = np.full(n, np.inf, f32)
    cur = np.zeros(n, np.int64)
    sp = np.zeros(n, np.int64)
    stack = np.zeros((n, STACK_TOTAL), np.int64)
    peak, peak_fetch = np.zeros(n, np.int64), np.zeros(n, np.int64)
    prim = np.full(n, -1, np.int64)
    occluded = np.zeros(n, bool)
    active = np.ones(n, bool)
    fetches, suspended_at = np.zeros(n, np.int64), np.zeros(n, np.int64)
    restored = np.zeros((n, STACK_TOTAL), bool)  # per stack entry: it went through the resume copy above level 16
    cur_restored, hit_restored = np.zeros(n, bool), np.zeros(n, bool)
    while active.any():
        idx = np.nonzero(active)[0]
        node = cur[idx]
        inter = _box_test32(bounds[node], o[idx], inv[idx], neg[idx], cur_rays[idx, 3], kernel_like)
        is_leaf = (flags[node] & 3) == 3
        cnt = flags[node] >> 2
        assert not (is_leaf & (cnt == 0)).any(), "empty leaves are not modelled"
        leaf = inter & is_leaf
        for k in range(int(cnt[leaf].max()) if leaf.any() else 0):
            sel = leaf & (cnt > k) & ~occluded[idx]
            r = idx[sel]
            p = order[a[node[sel]] + k]
            hit, t = prim_test(cur_rays[r], p, any_hit)
            if any_hit:
                occluded[r[hit]] = True
            else:
                cur_rays[r[hit], 3] = t[hit]
                prim[r[hit]] = p[hit]
                hit_restored[r[hit]] = cur_restored[r[hit]]
        interior = inter & ~is_leaf
        ri, ni = idx[interior], node[interior]
        peak_fetch[ri] = np.maximum(peak_fetch[ri], sp[ri])
        if budget:
            stop = ri[(fetches[ri] > 0) & (fetches[ri] % budget == 0) & (fetches[ri] // budget <= budgeted_rounds)]
            suspended_at[stop] = np.maximum(suspended_at[stop], sp[stop])
            for r_ in stop[sp[stop] > 16]:
                restored[r_, 16:sp[r_]] = True
        fetches[ri] += 1
        cur_restored[ri] = False  # a node reached by descent was never a stack entry
        second_first = neg[ri, flags[ni] & 3]  # dir_is_neg[split_axis] == 2: the second child first, the first child waits
        near, far = np.where(second_first, a[ni], ni + 1), np.where(second_first, ni + 1, a[ni])
        if kernel_like:
            hn = _box_test32(bounds[near], o[ri], inv[ri], neg[ri], cur_rays[ri, 3], True)
            hf = _box_test32(bounds[far], o[ri], inv[ri], neg[ri], no_limit[ri], True)
            hf_t = _box_test32(bounds[far], o[ri], inv[ri], neg[ri], cur_rays[ri, 3], True)
            push, go = hn & hf, np.where(hn, near, far)
            dead = ~hn & ~hf_t  # neither child: the next stack entry
        else:
            push, go, dead = np.ones(ri.size, bool), near, np.zeros(ri.size, bool)
        if (sp[ri[push]] >= STACK_TOTAL).any():
            raise IndexError("the reference's 64-entry stack overflows (bvh.jl:222 throws a BoundsError)")
        stack[ri[push], sp[ri[push]]] = far[push]
        restored[ri[push], sp[ri[push]]] = False
        cur[ri] = go
        sp[ri[push]] += 1
        peak[ri] = np.maximum(peak[ri], sp[ri])
        pop = np.concatenate([idx[~interior], ri[dead]])
        done = (sp[pop] == 0) | occluded[pop]
        active[pop[done]] = False
        pop = pop[~done]
        sp[pop] -= 1
        cur[pop] = stack[pop, sp[pop]]
        cur_restored[pop] = restored[pop, sp[pop]]
    return {"suspended_at": suspended_at, "hit_restored": hit_restored & (prim >= 0), "prim": prim, "slot": np.where(prim >= 0, slot_of[np.maximum(prim, 0)], -1), "t": cur_rays[:, 3].copy(), "occluded": occluded, "peak": peak,
            "peak_fetch": peak_fetch}


def histogram(peak, top):
    return np.bincount(np.asarray(peak, np.int64), minlength=top + 1)


# ---- Float64 brute force ---------------------------------------------------------------------------------------------------------------------------------------------
def moller_trumbore64(tris, rays):
    """Every ray against every triangle in Float64: t, u, v, w (n, m) — NaN where the ray is parallel to the triangle's plane."""
    v = np.asarray(tris, np.float64)
    o, d = np.asarray(rays[:, 0:3], np.float64), np.asarray(rays[:, 4:7], np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    pv = np.cross(d[:, None, :], e2[None, :, :])
    det = np.einsum("mk,nmk->nm", e1, pv)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(det != 0, 1.0 / det, np.nan)
        tv = o[:, None, :] - v[None, :, 0, :]
        u = np.einsum("nmk,nmk->nm", tv, pv) * inv
        qv = np.cross(tv, e1[None, :, :])
        vv = np.einsum("nk,nmk->nm", d, qv) * inv
        t = np.einsum("mk,nmk->nm", e2, qv) * inv
    return t, u, vv, 1.0 - u - vv


def brute_force(tris, rays, extent):
    """Nearest hit, occlusion and the safe-ray predicate.  A ray is SAFE if, among the triangles it hits or nearly hits (all barycentrics > -1e-5), none has a barycentric within
    1e-5 of an edge, no t lies within 1e-5 (relative: of `extent` / |d| near 0, of t_max near t_max) of 0 or t_max, and the nearest and second-nearest hit differ by more than 1e-4
    relative.  A ray parallel to a triangle's plane and inside that plane's slab of the triangle is unsafe."""
    t, u, v, w = moller_trumbore64(tris, rays)
    tmax = np.asarray(rays[:, 3], np.float64)[:, None]
    dn = np.linalg.norm(np.asarray(rays[:, 4:7], np.float64), axis=1)[:, None]
    with np.errstate(invalid="ignore"):
        bmin = np.minimum(np.minimum(u, v), w)
        cand = bmin > -1e-5
        edge = cand & (bmin < 1e-5)
        eps0 = 1e-5 * extent / dn
        near_end = cand & ((np.abs(t) < eps0) | (np.abs(t - tmax) < 1e-5 * np.where(np.isfinite(tmax), tmax, 0.0)))
        hit = (bmin >= 0) & (t > 0) & (t <= tmax)
    parallel = np.isnan(t).any(axis=1)
    th = np.where(hit, t, np.inf)
    order = np.sort(th, axis=1)
    prim = np.where(hit.any(axis=1), np.argmin(th, axis=1), -1)
    t0 = order[:, 0]
    second = order[:, 1] if order.shape[1] > 1 else np.full(t0.shape, np.inf)
    both = np.isfinite(second)
    tie = both & ((np.where(both, second, 1.0) - np.where(both, t0, 0.0)) <= 1e-4 * np.where(both, second, 1.0))
    safe = ~(edge.any(axis=1) | near_end.any(axis=1) | tie | parallel)
    return {"prim": prim, "t": t0, "occluded": hit.any(axis=1), "safe": safe}


def prim_test64(tris):
    """A primitive test for model A in Float64 (for counting stack entries where the oracle is not at hand; its hits are the brute force's on safe rays)."""
    v = np.asarray(tris, np.float64)

    def test(r8, prims, any_hit):
        hit = np.zeros(len(prims), bool)
        t = np.zeros(len(prims), f32)
        for j in range(len(prims)):
            tt, u, vv, w = moller_trumbore64(v[prims[j]][None], r8[j:j + 1])
            if min(u[0, 0], vv[0, 0], w[0, 0]) >= 0 and 0 < tt[0, 0] <= r8[j, 3]:
                hit[j], t[j] = True, tt[0, 0]
        return hit, t

    return test


def oracle_prim_test(ob, osc):
    """The oracle's own primitive test (orc_prim_intersect / orc_prim_intersect_p on one caller primitive, no tree) as model A's callable."""
    import ctypes as C
    L = ob.lib()
    fptr = C.POINTER(C.c_float)
    t_out = C.c_float()
    geom = (C.c_float * 17)()

    def test(r8, prims, any_hit):
        r8 = np.ascontiguousarray(r8, f32)
        base = r8.ctypes.data
        hit = np.zeros(len(prims), bool)
        t = np.zeros(len(prims), f32)
        for j in range(len(prims)):
            ray = C.cast(base + 32 * j, fptr)
            if any_hit:
                hit[j] = bool(L.orc_prim_intersect_p(osc.h, int(prims[j]), ray))
            elif L.orc_prim_intersect(osc.h, int(prims[j]), ray, C.byref(t_out), geom):
                hit[j], t[j] = True, t_out.value
        return hit, t

    return test


def chain_scene(T, tris32, light=(0.5, 0.9, 0.5), power=2.0):
    """The triangles as one matte mesh (caller primitive i = triangle i) and one point light."""
    import attack_scenes as A
    mesh = A.mesh_prims(T, tris32)
    lights = [T.PointLight(T.translate([float(x) for x in light]), T.RGBSpectrum(float(power)))]
    return T.Scene(lights, T.BVHAccel([mesh], 1))


# ---- model B: the four-wide walk's stack -----------------------------------------------------------------------------------------------------------------------------
def fold4(bounds, a, flags):
    """The four-wide form of a binary tree in the get_bvh layout: starting from a node's two children, the interior child of largest surface area (Float32, the first of equals)
    is replaced by its two children until four slots are taken or only leaves are left.  Returns (nodes, levels): nodes[k] = list of (binary node index, four-wide index or
    -1 for a leaf); levels = the depth of the deepest four-wide node, the root being 1 — the library's count (it builds the four-wide form iff 3 * (levels + 1) <= 64), or 0
    when the root's children are all leaves."""
    b = np.asarray(bounds, f32)
    ext = (b[:, 3:] - b[:, :3]).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        area = (ext[:, 0] * ext[:, 1] + ext[:, 0] * ext[:, 2]).astype(f32) + (ext[:, 1] * ext[:, 2]).astype(f32)
    leaf = (np.asarray(flags) & 3) == 3
    assert not leaf[0], "a one-leaf tree has no four-wide form"
    nodes, depth, todo, levels = [None], [1], [(0, 0)], 0
    while todo:
        node, out = todo.pop()
        kids = [node + 1, int(a[node])]
        while len(kids) < 4:
            best, best_a = -1, f32(-1.0)
            for k, c in enumerate(kids):
                if not leaf[c] and area[c] > best_a:
                    best, best_a = k, area[c]
            if best < 0:
                break
            c = kids[best]
            kids[best] = c + 1
            kids.append(int(a[c]))
        rec = []
        for c in kids:
            if leaf[c]:
                rec.append((c, -1))
            else:
                nodes.append(None)
                depth.append(depth[out] + 1)
                levels = max(levels, depth[-1])
                rec.append((c, len(nodes) - 1))
                todo.append((c, len(nodes) - 1))
        nodes[out] = rec
    return nodes, levels


def model_b(arrays, tris, rays, cap=256):
    """The stack of the four-wide walk: at a node the children the ray enters (a plain slab test in Float64 against the current limit), nearest first; the walk goes into the
    nearest and pushes the other n_go - 1, the farthest deepest; an entry is dropped at pop time when its entry distance is no longer below the limit; a leaf's triangles (Float64
    Moeller-Trumbore) pull the limit in.  Only the order and the count of the pushes are modelled.  Returns levels, peak (n,) and marginal (n,): rays that pass within 1e-4
    (relative to the box size) of a face of a box they test — their count is not model B's to state."""
    bounds, a, flags, order = arrays
    a, flags, order = np.asarray(a, np.int64), np.asarray(flags, np.int64), np.asarray(order, np.int64)
    nodes, levels = fold4(bounds, a, flags)
    b64 = np.asarray(bounds, np.float64)
    kid_node = np.full((len(nodes), 4), -1, np.int64)
    kid_w4 = np.full((len(nodes), 4), -1, np.int64)
    for k, rec in enumerate(nodes):
        for j, (c, w) in enumerate(rec):
            kid_node[k, j], kid_w4[k, j] = c, w
    n = rays.shape[0]
    o, d = np.asarray(rays[:, 0:3], np.float64), np.asarray(rays[:, 4:7], np.float64)
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.where(d == 0, 0.0, d)
    dn = np.linalg.norm(d, axis=1)
    t_lim = np.asarray(rays[:, 3], np.float64).copy()
    v = np.asarray(tris, np.float64)
    # cur >= 0: four-wide node; cur <= -2: leaf (binary node -cur - 2); -1: nothing (pop)
    cur = np.zeros(n, np.int64)
    sp = np.zeros(n, np.int64)
    s_enc = np.zeros((n, cap), np.int64)
    s_t = np.zeros((n, cap), np.float64)
    peak = np.zeros(n, np.int64)
    marginal = np.zeros(n, bool)
    active = np.ones(n, bool)
    while active.any():
        idx = np.nonzero(active & (cur >= 0))[0]
        if idx.size:
            kn = kid_node[cur[idx]]  # (m, 4)
            bx = b64[np.maximum(kn, 0)]  # (m, 4, 6)
            with np.errstate(invalid="ignore"):
                t1 = (bx[:, :, :3] - o[idx, None, :]) * inv[idx, None, :]
                t2 = (bx[:, :, 3:] - o[idx, None, :]) * inv[idx, None, :]
                t_in = np.fmax.reduce(np.fmin(t1, t2), axis=2)
                t_out = np.fmin.reduce(np.fmax(t1, t2), axis=2)
                nan = np.isnan(t1).all(axis=2)
                enter = (kn >= 0) & ~nan & (t_in <= t_out) & (t_out > 0) & (t_in < t_lim[idx, None])
                eps = 1e-4 * np.linalg.norm(bx[:, :, 3:] - bx[:, :, :3], axis=2) / dn[idx, None]
                close = (kn >= 0) & ((np.abs(t_out - t_in) < eps) | (np.abs(t_out) < eps) | (np.abs(t_in - t_lim[idx, None]) < eps) | np.isnan(t1).any(axis=2))
            marginal[idx] |= close.any(axis=1)
            key = np.where(enter, t_in, np.inf)
            srt = np.argsort(key, axis=1, kind="stable")
            key_s = np.take_along_axis(key, srt, axis=1)
            kw = kid_w4[cur[idx]]
            enc = np.where(kw >= 0, kw, -kn - 2)
            enc_s = np.take_along_axis(enc, srt, axis=1)
            n_go = enter.sum(axis=1)
            for m in (3, 2, 1):  # the m-th nearest waits at sp + n_go - 1 - m: the farthest deepest
                sel = n_go > m
                r = idx[sel]
                pos = sp[r] + n_go[sel] - 1 - m
                if (pos >= cap).any():
                    raise IndexError("model B's stack overflows its own capacity")
                s_enc[r, pos] = enc_s[sel, m]
                s_t[r, pos] = key_s[sel, m]
            sp[idx] += np.maximum(n_go - 1, 0)
            peak[idx] = np.maximum(peak[idx], sp[idx])
            cur[idx] = np.where(n_go > 0, enc_s[:, 0], -1)
        lf = np.nonzero(active & (cur <= -2))[0]
        if lf.size:
            node = -cur[lf] - 2
            for k in range(int((flags[node] >> 2).max())):
                sel = (flags[node] >> 2) > k
                r = lf[sel]
                p = order[a[node[sel]] + k]
                e1, e2 = v[p, 1] - v[p, 0], v[p, 2] - v[p, 0]
                pv = np.cross(d[r], e2)
                with np.errstate(divide="ignore", invalid="ignore"):
                    invd = 1.0 / np.einsum("nk,nk->n", e1, pv)
                    tv = o[r] - v[p, 0]
                    u = np.einsum("nk,nk->n", tv, pv) * invd
                    qv = np.cross(tv, e1)
                    w = np.einsum("nk,nk->n", d[r], qv) * invd
                    t = np.einsum("nk,nk->n", e2, qv) * invd
                    hit = (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0) & (t <= t_lim[r])
                t_lim[r[hit]] = t[hit]
            cur[lf] = -1
        pp = np.nonzero(active & (cur == -1))[0]  # nothing entered, a leaf done, or an entry dropped: the next entry against the limit as it stands now
        empty = sp[pp] == 0
        active[pp[empty]] = False
        pp = pp[~empty]
        sp[pp] -= 1
        ok = s_t[pp, sp[pp]] < t_lim[pp]
        cur[pp] = np.where(ok, s_enc[pp, sp[pp]], -1)
    return {"levels": levels, "peak": peak, "marginal": marginal}


# ---- the geometric progression: scenes whose library and reference trees are deep ------------------------------------------------------------------------------------
def progression(n, base=1.45, s0=1e-8, seed=7):
    """n triangles whose sizes and positions grow geometrically (tests/test_gpu_hybrid.py: the scene whose reference construction fails): every builder peels them off a few per
    level.  Float64 (n, 3, 3); the first n of a longer progression are the same triangles."""
    rng = np.random.default_rng(seed)
    tris = np.empty((n, 3, 3), np.float64)
    for i in range(n):
        sc = s0 * base ** i
        tris[i] = np.array([sc, 0.37 * sc, -0.2 * sc]) + 0.05 * sc * rng.uniform(-1.0, 1.0, (3, 3))
    return tris


def prim_boxes(tris32):
    return np.concatenate([tris32.min(axis=1), tris32.max(axis=1)], axis=1).astype(f32)


def progression_rays(tris32, n, seed=3):
    """The chain families re-aimed at a progression scene: towards points on its triangles from a point off the chain ("forward": few boxes at a time) and from beyond its
    largest triangle, from inside the chain between two triangles, with a finite t_max, into empty space — and "reverse": from the small end outwards along the chain, where at
    every four-wide node the interior child (the smaller triangles) is the nearest and the three leaves wait on the stack, three entries per level."""
    rng = np.random.default_rng(seed)
    m = tris32.shape[0]
    t64 = tris32.astype(np.float64)
    size = float(np.abs(t64[-1]).max())
    k = rng.integers(0, m, n)
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = np.einsum("nk,nkc->nc", w, t64[k])
    kind = np.arange(n) % 6
    origin = np.empty((n, 3))
    out = kind == 5
    target[out] = np.einsum("nk,nkc->nc", w[out], t64[rng.integers(m - 4, m, int(out.sum()))])  # points on the four largest triangles …
    origin[out] = -np.array([1.0, 0.37, -0.2]) * np.abs(t64[0]).max() * rng.uniform(0.5, 2.0, (int(out.sum()), 1))  # … seen from just before the smallest
    origin[kind == 0] = (np.array([-0.3, 0.2, 0.5]) * size + rng.uniform(-0.1, 0.1, (int((kind == 0).sum()), 3)) * size)
    origin[kind == 1] = t64[-1].mean(axis=0) * 1.5 + rng.uniform(-0.01, 0.01, (int((kind == 1).sum()), 3)) * size  # beyond the largest triangle, looking down the chain
    k2 = rng.integers(0, m - 1, n)
    mid = 0.5 * (t64[k2].mean(axis=1) + t64[k2 + 1].mean(axis=1))  # between triangles k2 and k2 + 1
    inside = (kind >= 2) & (kind <= 4)
    origin[inside] = mid[inside]
    d = target - origin
    d[kind == 4] = rng.normal(size=(int((kind == 4).sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.full(n, np.inf)
    fin = kind == 3
    tmax[fin] = np.linalg.norm(target - origin, axis=1)[fin] * rng.uniform(0.3, 1.7, int(fin.sum()))
    return rays8(origin.astype(f32), d.astype(f32), tmax.astype(f32))


# sizes of the progression whose LIBRARY tree (binned SAH, trhip_build_bvh_host builder 0), folded four wide, has 19, 20 and 21 levels — the last size the four-wide walk accepts
# sits between the second and the third (tests/test_deep_trees.py asserts the level counts)
FOUR_WIDE_SIZES = (87, 93, 94)


def four_wide_rays(tris32):
    """The ray set of the four-wide tests: 4 000 progression rays and 2 000 of the certificate's attack rays (attack_scenes.attack_rays) aimed at the same triangles."""
    import attack_scenes as A
    pts = tris32.reshape(-1, 3)
    att = A.attack_rays(np.random.default_rng(5), 2000, pts.min(axis=0), pts.max(axis=0), tris32, [])
    return np.concatenate([progression_rays(tris32, 4000)] + list(att.values()))


def commit_edge_sizes(T):
    """(n, n + 1): the progression sizes whose REFERENCE tree (builder 2) is 64 and 65 levels deep — the deepest trhip_scene_commit accepts, and the first it refuses."""
    full = progression(200).astype(f32)
    depth = {}
    for n in range(100, 200):
        depth[n] = T._ffi.build_bvh_host(prim_boxes(full[:n]), 1, builder=2)[4]
        if depth[n] >= 65:
            assert depth[n] == 65 and depth[n - 1] == 64, (n, depth[n - 1], depth[n])
            return n - 1, n
    raise AssertionError("the progression never reaches a reference tree of 65 levels")


def stream_scene(T, which):
    """The lit scenes of the streaming tests: (tris, set_bvh arrays, camera, scene).  "one chain": caterpillar(40, "leaf_first"), the camera inside its deep end between
    slats 38 and 39, looking down the chain towards -x and a little downwards, so that the frame's rays cross the shared hypotenuse — meet their first slat — all along the chain.
    "twin chains": twin_chains(40), the camera on the plane y = 1 between them.  The point light sits beside the camera, in the open half: what a camera ray hits it also
    lights, through the same open halves the ray came through, so the frame's radiance depends on WHICH slat each ray hits first — a hit lost or moved by one slat changes it.
    fov 90 as every camera the oracle bridge describes (oracle_bridge.make_sensor); with the reference's perspective() (transformations.jl:119-130, kept as written) that is a narrow
    cone: the rays spread +- 0.02 around the axis.  Film 24 x 24."""
    film = T.Film([24, 24], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    window = T.Bounds2([-1.0, -1.0], [1.0, 1.0])
    if which == "one chain":
        tree = caterpillar(40, "leaf_first")
        tris, arrays = tree.tris, tree.arrays
        cam = T.PerspectiveCamera(T.look_at([38.5, 0.62, 0.62], [0.0, 0.45, 0.45], [0, 1, 0]), window, 0.0, 1.0, 0.0, 1e6, 90.0, film)
        light = (38.7, 0.7, 0.7)
    else:
        tris, arrays = twin_chains(40)
        cam = T.PerspectiveCamera(T.look_at([38.5, 1.0, 0.3], [0.0, 0.76, 0.13], [0, 0, 1]), window, 0.0, 1.0, 0.0, 1e6, 90.0, film)
        light = (38.7, 1.0, 0.45)
    return tris, arrays, cam, chain_scene(T, tris, light=light, power=40.0)
