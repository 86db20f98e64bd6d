"""The trees, rays and models of tests/deep_trees.py, checked on the CPU before tests/test_gpu_deep_trees.py hands them to the kernels.

* model A (the reference's loop over the set_bvh arrays, the oracle's own primitive test) returns the oracle's hits on every chain and every ray family — so its stack counts are
  the counts of the walk that produced those hits;
* the WITNESS: on every chain, every stack level from 0 to D - 1 is the peak of at least 16 rays, every level a kernel's LDS / slab boundary sits on (L - 1, L, L + 1 for the
  fast-level counts 10, 11, 12, 16, 32) of at least 64, the top of at least 64 — for the reference's loop, and (8 per level) for the stack as the slab kernels keep it;
* the oracle against a Float64 brute force on the rays that are safe to compare (no edge, no end point, no near-tie), of which every family has at least 98 %;
* model B (the four-wide fold and the push rule of the four-wide walk) on the progression scenes of the GPU file: 19, 20 and 21 levels, and what the stack holds there;
* what max_depth counts, and the entries the deepest accepted chain needs.
"""
import numpy as np
import pytest

import deep_trees as dt

# oracle t against Float64 Moeller-Trumbore on safe rays, max |t - t64| / t64 over all 26 chains x 9 families: measured 2.51e-7 (2.1 Float32 ulps).  The bound is 8 x that,
# and never less than 16 ulps (1.91e-6)
T_REL_MEASURED = 2.51e-7
T_REL_BOUND = max(8 * T_REL_MEASURED, 16 * 2.0 ** -23)

_cache = {}


def chain(T, ob, D, layout):
    """Everything the tests of one chain share, computed once: tree, scene, oracle, families, the oracle's answers, both models, the brute force."""
    key = (D, layout)
    if key not in _cache:
        tree = dt.caterpillar(D, layout)
        scene = dt.chain_scene(T, tree.tris)
        osc = ob.OracleScene.from_scene(scene, bvh=tree.arrays)
        fams = dt.ray_families(tree)
        test = dt.oracle_prim_test(ob, osc)
        res = {}
        for name, rays in fams.items():
            t_ref, slot_ref, _, _ = osc.trace_closest(rays)
            occ_ref, _ = osc.trace_any(rays)
            res[name] = {"rays": rays, "t": t_ref, "slot": slot_ref, "occ": occ_ref.astype(bool), "A": dt.model_a(tree.arrays, rays, test),
                         "A_any": dt.model_a(tree.arrays, rays, test, any_hit=True), "K": dt.model_a(tree.arrays, rays, test, kernel_like=True),
                         "bf": dt.brute_force(tree.tris, rays, float(D))}
        _cache[key] = (tree, res)
    return _cache[key]


CHAINS = [(D, layout) for D in dt.DEPTHS for layout in dt.LAYOUTS]


def test_the_depths_sit_on_either_side_of_every_fast_level_count():
    for L in dt.LEVELS:
        assert {L, L + 1, L + 2} <= set(dt.DEPTHS)  # D - 1 entries at most: the deepest entry at level L - 1, L, L + 1
    assert 40 in dt.DEPTHS and dt.DEEPEST in dt.DEPTHS and max(dt.DEPTHS) == dt.DEEPEST


@pytest.mark.parametrize("D,layout", CHAINS)
def test_the_chain_is_a_tree_set_bvh_lets_the_default_kernels_walk(D, layout):
    tree = dt.caterpillar(D, layout)
    b, a, f, order = tree.arrays
    assert a.size == 2 * D - 1 and sorted(order.tolist()) == list(range(D))
    assert dt.tree_depth(a, f) == D
    assert dt.nests(b, a, f)
    interior = (f & 3) != 3
    assert interior.sum() == D - 1 and np.all((f[interior] & 3) == 0) and np.all(f[~interior] == ((1 << 2) | 3))
    for i in np.nonzero(interior)[0]:  # {one leaf of one primitive, the rest}: the leaf first or second, as the layout says
        first_is_leaf, second_is_leaf = not interior[i + 1], not interior[a[i]]
        assert (first_is_leaf if layout == "leaf_first" else second_is_leaf)
        assert first_is_leaf != second_is_leaf or i == np.nonzero(interior)[0][-1]
        assert np.all(b[i + 1, :3] >= b[i, :3]) and np.all(b[a[i], 3:] <= b[i, 3:])
    for i in np.nonzero(~interior)[0]:  # every leaf box is the Float32 box of its triangle
        tri = tree.tris[order[a[i]]]
        assert np.array_equal(b[i, :3], tri.min(axis=0)) and np.array_equal(b[i, 3:], tri.max(axis=0))
    lb = np.array([tree.leaf_box(i) for i in range(D)])
    assert np.all(lb[1:, 1:3] > lb[:-1, 1:3]) and np.all(lb[1:, 4:6] < lb[:-1, 4:6])  # strictly nested in y and z


@pytest.mark.parametrize("D,layout", CHAINS)
def test_model_a_returns_the_oracles_hits(T, ob, D, layout):
    tree, res = chain(T, ob, D, layout)
    for name, r in res.items():
        what = f"{tree.name}, {name}"
        assert np.array_equal(r["A"]["slot"], r["slot"]), what
        hit = r["slot"] >= 0
        assert np.array_equal(r["A"]["t"].view(np.uint32)[hit], r["t"].view(np.uint32)[hit]), what
        assert np.array_equal(r["A_any"]["occluded"], r["occ"]), what
        # the same walk with the slab kernels' box test and push rule: other stack counts, the same hits
        assert np.array_equal(r["K"]["slot"], r["slot"]) and np.array_equal(r["K"]["t"].view(np.uint32)[hit], r["t"].view(np.uint32)[hit]), what
        assert r["A"]["peak"].max() <= D - 1 and r["K"]["peak"].max() <= D - 1


@pytest.mark.parametrize("D,layout", CHAINS)
def test_the_witness_every_stack_level_is_some_rays_peak(T, ob, D, layout, capsys):
    tree, res = chain(T, ob, D, layout)
    top = D - 1
    hist_a = sum(dt.histogram(r["A"]["peak"], top) for r in res.values())
    hist_k = sum(dt.histogram(r["K"]["peak"], top) for r in res.values())
    with capsys.disabled():
        print(f"\n{tree.name}: peak stack entries, reference loop  {hist_a.tolist()}\n{'':{len(tree.name)}}  slab kernels' stack             {hist_k.tolist()}")
    assert hist_a.size == D and np.all(hist_a >= 16), hist_a.tolist()
    assert np.all(hist_k >= 8), hist_k.tolist()
    for L in dt.LEVELS:
        for level in (L - 1, L, L + 1):
            if level <= top:
                assert hist_a[level] >= 64 and hist_k[level] >= 64, (L, level, int(hist_a[level]), int(hist_k[level]))
    assert hist_a[top] >= 64 and hist_k[top] >= 64
    # the families do what their names say: "reverse" fills the stack, "forward" never holds more than one entry
    for name, r in res.items():
        if name.startswith("reverse"):
            assert np.all(r["A"]["peak"] == top) and np.all(r["K"]["peak"] == top), name
        if name.startswith("forward") or name == "inside, forward":
            assert r["A"]["peak"].max() <= 1 and r["K"]["peak"].max() <= 1, name
    assert all(r["rays"].shape[0] >= 64 for r in res.values()) and 3000 <= sum(r["rays"].shape[0] for r in res.values()) <= 8000


@pytest.mark.parametrize("D,layout", CHAINS)
def test_the_oracle_equals_the_float64_brute_force_on_safe_rays(T, ob, D, layout):
    tree, res = chain(T, ob, D, layout)
    worst = 0.0
    for name, r in res.items():
        what = f"{tree.name}, {name}"
        bf = r["bf"]
        safe = bf["safe"]
        assert 1.0 - safe.mean() <= 0.02, f"{what}: {100 * (1 - safe.mean()):.2f} % of the rays are unsafe"
        assert np.array_equal(bf["prim"][safe], r["A"]["prim"][safe]), what  # (caller indices; r["A"]["slot"] is the oracle's, asserted above)
        assert np.array_equal(bf["occluded"][safe], r["occ"][safe]), what
        hit = safe & (r["slot"] >= 0)
        if hit.any():
            rel = np.abs(r["t"][hit].astype(np.float64) - bf["t"][hit]) / bf["t"][hit]
            worst = max(worst, float(rel.max()))
    print(f"{tree.name}: max |t - t64| / t64 = {worst:.3e}")
    assert worst <= T_REL_BOUND, f"{tree.name}: {worst:.3e} > {T_REL_BOUND:.3e}"
    hits = sum(int((r["slot"] >= 0).sum()) for r in res.values())
    assert hits >= 1500  # the families are not all misses


def test_the_families_hold_the_special_rays(T, ob):
    """d.x = +0 and -0, axis-parallel directions, origins exactly in box planes (0 * Inf in the slab products), and a finite t_max that ends between two slats."""
    tree, res = chain(T, ob, 40, "leaf_first")
    r = res["d.x = 0 and axis-parallel"]["rays"]
    dx = r[:, 4]
    assert ((dx == 0) & ~np.signbit(dx)).sum() >= 64 and ((dx == 0) & np.signbit(dx)).sum() >= 64
    assert ((r[:, 5] == 0) & (r[:, 6] == 0)).sum() >= 64 and ((dx == 0) & ((r[:, 5] == 0) | (r[:, 6] == 0))).sum() >= 64
    planes_x = np.unique(tree.bounds[:, [0, 3]])
    planes_y = np.unique(tree.bounds[:, [1, 4]])
    assert ((dx == 0) & np.isin(r[:, 0], planes_x)).sum() >= 32          # (plane - o.x) * (1 / d.x) = 0 * Inf
    assert ((r[:, 5] == 0) & np.isin(r[:, 1], planes_y)).sum() >= 16
    f = res["finite t_max"]["rays"]
    assert np.all(np.isfinite(f[:, 3])) and np.all(np.abs(np.abs(f[:, 4]) - 1.0) == 0)
    stop = f[:, 0].astype(np.float64) + f[:, 3] * f[:, 4]
    assert np.all(np.abs((stop % 1.0) - 0.5) < 1e-3)  # half way between two slats
    culled = res["finite t_max"]
    assert (culled["A"]["peak"] == 39).sum() >= 200 and (culled["slot"] < 0).sum() >= 50  # full stacks whose popped leaves lie beyond t_max


def test_what_max_depth_counts_and_what_the_deepest_accepted_chain_needs(T, ob):
    """trhip_scene_set_bvh and trhip_scene_commit refuse max_depth > 64; max_depth counts the NODES on the longest root-to-leaf path, the root being 1 (tu_scene.hip: the root span
    starts at depth 1).  A chain of D triangles has max_depth D.  The deepest accepted chain, D = 64, needs 63 stack entries in the reference's loop (one per interior node) — within
    the 64 the kernels hold.  The first refused, D = 65, would need 64: the reference's own array (bvh.jl:222) still holds that, so the library refuses one level early, not late.
    (The acceptance itself needs a scene, hence a device: tests/test_gpu_deep_trees.py.)"""
    tree, res = chain(T, ob, dt.DEEPEST, "leaf_first")
    assert dt.tree_depth(tree.a, tree.flags) == 64
    need = max(int(r["A"]["peak"].max()) for r in res.values())
    assert need == 63 and need <= dt.STACK_TOTAL
    assert max(int(r["K"]["peak"].max()) for r in res.values()) == 63 and max(int(r["A_any"]["peak"].max()) for r in res.values()) == 63
    deeper = dt.caterpillar(65, "leaf_first")
    assert dt.tree_depth(deeper.a, deeper.flags) == 65
    rays = dt.ray_families(deeper)["reverse, open"][:64]
    assert dt.model_a(deeper.arrays, rays, dt.prim_test64(deeper.tris))["peak"].max() == 64  # model A itself raises at a 65th entry, like bvh.jl:222
    # the host builders count the same way: two primitives -> root + two leaves = depth 2
    pb = np.float32([[2, 0, 0, 3, 1, 1], [0, 0, 0, 1, 1, 1]])
    assert T._ffi.build_bvh_host(pb, 1, builder=2)[4] == 2 and T._ffi.build_bvh_host(pb, 1, builder=0)[4] == 2


def test_the_commit_edge_sizes_of_the_progression(T):
    """The geometric progression whose reference tree grows a level every two triangles or so: the size whose reference tree is 64 deep, and the next, 65 deep (what
    tests/test_gpu_deep_trees.py commits with bvh_builder 2 and sees refused)."""
    n_ok, n_refused = dt.commit_edge_sizes(T)
    assert n_refused == n_ok + 1
    assert T._ffi.build_bvh_host(dt.prim_boxes(dt.progression(n_ok).astype(np.float32)), 1, builder=2)[4] == 64
    assert T._ffi.build_bvh_host(dt.prim_boxes(dt.progression(n_refused).astype(np.float32)), 1, builder=2)[4] == 65


@pytest.mark.parametrize("n,levels", list(zip(dt.FOUR_WIDE_SIZES, (19, 20, 21))))
def test_model_b_on_the_four_wide_acceptance_edge(T, n, levels, capsys):
    """The library's own tree (binned SAH, the host builder) of the first n triangles of the progression, folded four wide: 19, 20 and 21 levels by the library's count (the depth
    of the deepest four-wide node, the root being 1).  The library builds the four-wide form iff 3 * (levels + 1) <= 64, i.e. up to 20 levels.

    What the stack holds at 20 levels: no ray of the set needs more than 64 entries — the rule is sufficient.  The aim was 64 rays at 3 * 19 = 57 entries or more, the top of the slab; this family does
    not get there.  The binned SAH peels the progression off two or three triangles per binary level, and the fold (the largest interior child first) then makes four-wide nodes
    of two leaves and TWO interior children almost everywhere (16 of the 19 nodes that have an interior child at all); a node pushes three entries only where it has three leaves
    to enter and one interior child that is the nearest.  A ray that enters every box from the small end therefore pushes about two entries per level: the deepest stack of the
    set is 44 entries at 20 levels (42 at 19, 47 at 21), and what is asserted is 2 * (levels - 1) for at least 64 rays — far above k_trace3c4's 12 LDS levels, 20 short of the top
    of the slab."""
    tris = dt.progression(n).astype(np.float32)
    b, a, f, order, depth = T._ffi.build_bvh_host(dt.prim_boxes(tris), 1, builder=0)
    nodes, lv = dt.fold4(b, a, f)
    assert lv == levels
    assert (3 * (lv + 1) <= dt.STACK_TOTAL) == (levels <= 20)
    assert all(2 <= len(rec) <= 4 for rec in nodes)
    leaves = sorted(c for rec in nodes for c, w in rec if w < 0)
    assert leaves == sorted(np.nonzero((f & 3) == 3)[0].tolist())  # every binary leaf is some four-wide node's child, once
    rays = dt.four_wide_rays(tris)
    assert rays.shape[0] <= 8000
    got = dt.model_b((b, a, f, order), tris, rays)
    counted = ~got["marginal"]
    hist = np.bincount(got["peak"][counted])
    with capsys.disabled():
        print(f"\nprogression of {n}: binary depth {depth}, {lv} four-wide levels, {int(counted.sum())} of {rays.shape[0]} rays counted; peak stack entries {hist.tolist()}")
    assert got["levels"] == levels and counted.sum() >= 3000
    assert got["peak"].max() <= dt.STACK_TOTAL  # (marginal rays included: whatever side of a face they pass)
    assert got["peak"].max() <= 3 * (lv - 1) + 3
    assert (got["peak"][counted] >= 2 * (lv - 1)).sum() >= 64
    assert (got["peak"][counted] > 12).sum() >= 500  # k_trace3c4's 12 LDS levels: the slab is where these rays' stacks live


def test_the_twin_chains_are_one_nested_tree_of_41_levels():
    tris, (b, a, f, order) = dt.twin_chains(40)
    assert tris.shape == (80, 3, 3) and a.size == 1 + 2 * 79 and dt.tree_depth(a, f) == 41 and dt.nests(b, a, f)
    assert (f[0] & 3) == 1 and a[0] == 80 and sorted(order.tolist()) == list(range(80))
    one = dt.caterpillar(40, "leaf_first")
    assert np.array_equal(b[1:80], one.bounds) and np.array_equal(dt.caterpillar_arrays(one.tris)[1], one.a) and np.array_equal(dt.caterpillar_arrays(one.tris)[2], one.flags)
    leaf = (f & 3) == 3
    for i in np.nonzero(leaf)[0]:
        tri = tris[order[a[i]]]
        assert np.array_equal(b[i, :3], tri.min(axis=0)) and np.array_equal(b[i, 3:], tri.max(axis=0))


def test_the_streaming_frames_rays_are_suspended_deep_and_hit_in_restored_entries(T, ob):
    """The camera rays of the streaming scenes in model A, in k_trace2's form, with the streaming wavefront's suspension rule: at least 64 rays are suspended holding 17 entries or
    more under every budget the GPU test renders with; under budgets 3 and 7 at least 64 rays of the single chain find their closest hit in a leaf whose stack entry went back into
    the overflow slab through the `lvl >= kStack2Lds` resume branch.  Under budget 1 only levels 16 to 18 ever cross that branch (19 budgeted rounds): fewer rays hit there."""
    for which in ("one chain", "twin chains"):
        tris, arrays, cam, scene = dt.stream_scene(T, which)
        osc = ob.OracleScene.from_scene(scene, bvh=arrays)
        rays = ob.generate_rays(cam, T.scenes.camera_sample_grid(cam, 2, seed=21))
        test = dt.oracle_prim_test(ob, osc)
        plain = dt.model_a(arrays, rays, test, kernel_like=True)
        for b in (1, 3, 7):
            got = dt.model_a(arrays, rays, test, kernel_like=True, budget=b)
            assert np.array_equal(got["prim"], plain["prim"]) and np.array_equal(got["peak"], plain["peak"])  # the bookkeeping changes nothing
            print(f"{which}, budget {b}: deepest suspension max {int(got['suspended_at'].max())}, hits in restored entries {int(got['hit_restored'].sum())}")
            assert (got["suspended_at"] >= 17).sum() >= 64
            assert got["suspended_at"].max() <= (19 if b == 1 else 40)
            if which == "one chain":
                assert got["hit_restored"].sum() >= (64 if b > 1 else 16)
                assert np.all(got["prim"][got["hit_restored"]] >= 16)  # on the chain the entry of slat k sits at level k
