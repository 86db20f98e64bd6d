"""The traversal kernels on trees that fill their 64-entry stack (run with -m gpu; the trees, rays and models are tests/deep_trees.py, checked on the CPU in
tests/test_deep_trees.py).

Every kernel keeps the first levels of its per-ray stack in LDS and the rest in a global overflow slab (k_trace_closest / k_trace_any: in scratch) — 32, 16, 12 / 10, 11 and 12
fast levels for k_trace_closest, k_trace2, k_trace3 closest / any, k_trace3c and k_trace3c4.  The SAH trees of the other suites are shallow: nothing there holds more than a
dozen entries.  Here

* caterpillar chains of 10 ... 64 triangles go in through trhip_scene_set_bvh, one on either side of every fast-level count, and rays whose peak stack depth is every value from
  0 to D - 1 are traced by every binary walk under the options that change how it walks; hits are the oracle's bits on the same arrays, occlusion its booleans, and on safe
  rays both are the Float64 brute force's;
* the deepest chain set_bvh accepts (64) is walked, the next (65) refused; the same pair for trhip_scene_commit;
* the streaming wavefront renders a lit 40-level chain with fetch budgets 1, 3 and 7: rays are suspended with the entries they hold — up to 19 under budget 1 (19 budgeted
  rounds), up to 38 under 3 and 7 — and resumed through the copy that puts levels 16 and above back into the slab;
* the four-wide certified walk runs on library trees of 19, 20 and 21 four-wide levels: the last it accepts, and the first it leaves to the binary walk.
"""
import time

import numpy as np
import pytest

import deep_trees as dt
from conftest import supported
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

DEFAULTS = {"traversal": 3, "hybrid": 1, "wide4": 1, "any_on_accelerator": -1, "occluder_pretest": 1, "slab_margin_log2": 14, "count_visits": 0, "bvh_builder": -1, "streaming": 0,
            "stream_budget_min": 2048, "stream_list_cap": 0}


@pytest.fixture
def dctx(ctx):
    """The session's context with every option these tests touch at its default, before and after."""
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    yield ctx
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)


def configurations(ctx, accel_kernel):
    """(options, the closest-hit kernel the library must name).  `accel_kernel`: what the default configuration runs on this scene's accelerator."""
    cfg = [({}, accel_kernel),
           ({"traversal": 1}, "k_trace_closest"), ({"traversal": 1, "hybrid": 0}, "k_trace_closest"),
           ({"traversal": 2, "hybrid": 0}, "k_trace2"), ({"traversal": 3, "hybrid": 0}, "k_trace3"),
           ({"any_on_accelerator": 0}, accel_kernel), ({"any_on_accelerator": 1}, accel_kernel),
           ({"occluder_pretest": 0}, accel_kernel), ({"occluder_pretest": 1, "hybrid": 0}, "k_trace3"), ({"occluder_pretest": 0, "hybrid": 0}, "k_trace3"),
           ({"slab_margin_log2": 0}, "k_trace3"), ({"slab_margin_log2": 0, "traversal": 2}, "k_trace2"), ({"slab_margin_log2": 14}, accel_kernel),
           ({"count_visits": 1}, accel_kernel), ({"count_visits": 1, "hybrid": 0}, "k_trace3"), ({"count_visits": 1, "traversal": 2}, "k_trace2")]
    names = {7: ("k_trace7",), 6: ("k_trace4",), 4: ("k_trace8", "k_trace3")}  # the EXPERIMENTS build's kernels (k_trace8 only where the scene has an 8-wide form)
    for trav in supported(ctx, "traversal", (7, 6, 4)):
        cfg.append(({"traversal": trav}, names[trav]))
    return cfg


def run_configuration(ctx, flat, opts, kernel, fams, ref, what, fallback=None):
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        name = flat.closest_kernel_name()
        assert name in ((kernel,) if isinstance(kernel, str) else kernel), f"{what}, {opts}: the library names {name}, not {kernel}"
        for fam, rays in fams.items():
            tag = f"{what}, {opts or 'default'}, {fam}"
            got = flat.trace_closest(rays)
            if fallback is not None:
                fallback[fam] = flat.last_fallback()
            occ = flat.trace_any(rays)
            r = ref[fam]
            assert np.array_equal(got["prim"], r["slot"]), f"{tag}: primitives differ from the oracle's in {int((got['prim'] != r['slot']).sum())} rays"
            hit = r["slot"] >= 0
            assert_bits_equal(got["t"][hit], r["t"][hit], f"{tag}: t")
            assert_bits_equal(got["b1"][hit], r["b1"][hit], f"{tag}: b1")
            assert_bits_equal(got["b2"][hit], r["b2"][hit], f"{tag}: b2")
            # the interaction rebuilt from this configuration's hits (p = b0 p0 + b1 p1 + b2 p2, and the frame), against the oracle's
            assert_bits_equal(flat.hit_geometry(rays)[hit], r["geom"][hit], f"{tag}: hit geometry (p, n, ns, wo, ss)")
            assert np.array_equal(occ.astype(bool), r["occ"]), f"{tag}: occlusion differs from the oracle's in {int((occ.astype(bool) != r['occ']).sum())} rays"
            safe = r["bf"]["safe"]
            caller = np.where(got["prim"] >= 0, r["order"][np.maximum(got["prim"], 0)], -1)
            assert np.array_equal(caller[safe], r["bf"]["prim"][safe]), f"{tag}: primitives differ from the Float64 brute force on safe rays"
            assert np.array_equal(occ.astype(bool)[safe], r["bf"]["occluded"][safe]), f"{tag}: occlusion differs from the Float64 brute force on safe rays"
    finally:
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


def oracle_reference(ob, osc, order, tris, fams, extent):
    """The oracle on the same arrays, once per tree: t, slot, the interaction (p, n, ns, wo, ss) and occlusion; and the Float64 brute force."""
    ref = {}
    for fam, rays in fams.items():
        t, slot, geom, _ = osc.trace_closest(rays, want_geom=True)
        occ, _ = osc.trace_any(rays)
        ref[fam] = {"t": t, "slot": slot, "geom": geom, "occ": occ.astype(bool), "order": np.asarray(order, np.int64), "bf": dt.brute_force(tris, rays, extent)}
    return ref


def add_barycentrics(ref, flat, ctx, fams):
    """The oracle reports a hit's barycentrics only through the interaction it builds from them (p = b0 p0 + b1 p1 + b2 p2, and the frame).  So b1 / b2 are taken from the literal
    kernel (traversal 1, the reference's loop op for op) once its primitives and t equal the oracle's AND the interaction rebuilt from its hits (trhip_hit_geometry) equals the
    oracle's bit for bit; every other configuration is then held to those bits."""
    ctx.set_option("traversal", 1)
    try:
        for fam, rays in fams.items():
            got = flat.trace_closest(rays)
            assert np.array_equal(got["prim"], ref[fam]["slot"]), f"{fam}: the literal kernel's primitives differ from the oracle's"
            hit = ref[fam]["slot"] >= 0
            assert_bits_equal(got["t"][hit], ref[fam]["t"][hit], f"{fam}: the literal kernel's t")
            assert_bits_equal(flat.hit_geometry(rays)[hit], ref[fam]["geom"][hit], f"{fam}: the interaction rebuilt from the literal kernel's hits (p, n, ns, wo, ss)")
            ref[fam]["b1"], ref[fam]["b2"] = got["b1"].copy(), got["b2"].copy()
            w = 1.0 - got["b1"][hit].astype(np.float64) - got["b2"][hit]
            assert np.all(got["b1"][hit] >= 0) and np.all(got["b2"][hit] >= 0) and np.all(w >= -1e-6)
    finally:
        ctx.set_option("traversal", 3)


CHAINS = [(D, layout) for D in dt.DEPTHS for layout in dt.LAYOUTS]


@pytest.mark.parametrize("D,layout", CHAINS)
def test_every_binary_walk_equals_the_oracle_on_a_chain(T, ob, dctx, D, layout):
    ctx = dctx
    t0 = time.time()
    tree = dt.caterpillar(D, layout)
    scene = dt.chain_scene(T, tree.tris)
    flat = scene.flatten(ctx)
    try:
        flat.set_bvh(*tree.arrays)
        for x, y in zip(flat.bvh(), tree.arrays):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
        mode, acc_nodes, acc_depth = flat.bvh_mode()
        assert mode == 2 and flat.bvh_note() == "", (mode, flat.bvh_note())  # the chain is the canonical tree, the library's tree over the same slats the accelerator
        # at most tiny_scene_prims (16) primitives: the accelerator is one leaf (k_trace_leaf_c hands its ties to k_trace3 on the chain); above, a hierarchy, four wide
        assert (acc_nodes > 1) == (D > 16), (D, acc_nodes)
        accel_kernel = "k_trace3c4" if acc_nodes > 1 else "k_trace_leaf_c"
        osc = ob.OracleScene.from_scene(scene, bvh=tree.arrays)
        fams = dt.ray_families(tree)
        ref = oracle_reference(ob, osc, tree.order, tree.tris, fams, float(D))
        add_barycentrics(ref, flat, ctx, fams)
        fallback = {}
        for opts, kernel in configurations(ctx, accel_kernel):
            run_configuration(ctx, flat, opts, kernel, fams, ref, tree.name, fallback if not opts else None)
        # wide4 is read when the accelerator is uploaded: the same tree again, without the four-wide form
        ctx.set_option("wide4", 0)
        flat.set_bvh(*tree.arrays)
        assert flat.bvh_mode()[0] == 2
        run_configuration(ctx, flat, {}, "k_trace3c" if acc_nodes > 1 else "k_trace_leaf_c", fams, ref, tree.name + ", wide4 0")
        walked = sum(f[1] for f in fallback.values())
        print(f"{tree.name}: accelerator {acc_nodes} nodes, depth {acc_depth}, {accel_kernel}; rays handed back to k_trace3 on the chain (default configuration): "
              + ", ".join(f"{fam} {f[1]}/{f[0]}" for fam, f in fallback.items()) + f"; {time.time() - t0:.2f} s")
        # The handed-back rays walk the canonical chain with k_trace3, as the reference-order walk of the hybrid mode.  Every ray with a zero direction component is handed back
        # (the certificate does not cover 0 x Inf), so the whole axis family is — and it holds rays that run down the chain: by model A, in the form k_trace3 keeps its stack,
        # at least 32 of them peak beyond k_trace3's 12 LDS levels wherever the chain is long enough for that
        axis = "d.x = 0 and axis-parallel"
        assert fallback[axis] == (fams[axis].shape[0], fams[axis].shape[0]), fallback[axis]
        peak = dt.model_a(tree.arrays, fams[axis], dt.oracle_prim_test(ob, osc), kernel_like=True)["peak"]
        print(f"{tree.name}: handed-back axis family, peak stack entries in k_trace3's form: max {int(peak.max())}, {int((peak > 12).sum())} rays above 12")
        if D >= 14:
            assert (peak > 12).sum() >= 32, f"{tree.name}: only {int((peak > 12).sum())} handed-back rays leave k_trace3's LDS levels"
    finally:
        ctx.set_option("wide4", 1)
        scene._flat = None
        flat.free()


def test_set_bvh_accepts_a_chain_of_64_and_refuses_65(T, ob, dctx):
    """max_depth counts the nodes on the longest root-to-leaf path, the root being 1: a chain of D triangles has max_depth D.  64 is accepted — the reverse rays hold 63 entries
    on it, walked above by every configuration and once more here — and 65 is refused on the host, before any launch."""
    ctx = dctx
    for layout in dt.LAYOUTS:
        tree, deeper = dt.caterpillar(dt.DEEPEST, layout), dt.caterpillar(dt.DEEPEST + 1, layout)
        scene = dt.chain_scene(T, deeper.tris)
        flat = scene.flatten(ctx)
        try:
            with pytest.raises(T.TraceHipError, match="64-entry"):
                flat.set_bvh(*deeper.arrays)
        finally:
            scene._flat = None
            flat.free()
        scene = dt.chain_scene(T, tree.tris)
        flat = scene.flatten(ctx)
        try:
            flat.set_bvh(*tree.arrays)
            assert flat.bvh_mode()[0] == 2
            osc = ob.OracleScene.from_scene(scene, bvh=tree.arrays)
            fams = {k: v for k, v in dt.ray_families(tree).items() if k.startswith("reverse")}
            ref = oracle_reference(ob, osc, tree.order, tree.tris, fams, 64.0)
            add_barycentrics(ref, flat, ctx, fams)
            for opts, kernel in configurations(ctx, "k_trace3c4"):
                run_configuration(ctx, flat, opts, kernel, fams, ref, tree.name)
        finally:
            scene._flat = None
            flat.free()


def test_commit_accepts_a_reference_tree_of_64_levels_and_refuses_65(T, ob, dctx):
    """The geometric progression of tests/test_gpu_hybrid.py, cut where the reference's construction (bvh_builder 2) ends 64 levels deep, and one triangle later, at 65."""
    ctx = dctx
    n_ok, n_refused = dt.commit_edge_sizes(T)
    tris = {n: dt.progression(n).astype(np.float32) for n in (n_ok, n_refused)}
    assert T._ffi.build_bvh_host(dt.prim_boxes(tris[n_ok]), 1, builder=2)[4] == 64 and T._ffi.build_bvh_host(dt.prim_boxes(tris[n_refused]), 1, builder=2)[4] == 65
    ctx.set_option("bvh_builder", 2)
    scene = dt.chain_scene(T, tris[n_refused])
    with pytest.raises(T.TraceHipError, match="64-entry"):
        scene.flatten(ctx)
    scene._flat = None
    scene = dt.chain_scene(T, tris[n_ok])
    flat = scene.flatten(ctx)
    try:
        assert flat.bvh_mode()[0] == 1
        osc = ob.OracleScene.from_scene(scene)  # the oracle builds the reference's tree itself
        for x, y in zip(flat.bvh(), osc.get_bvh()):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
        assert dt.tree_depth(flat.bvh()[1], flat.bvh()[2]) == 64
        rays = dt.four_wide_rays(tris[n_ok])
        t_ref, slot_ref, _, _ = osc.trace_closest(rays)
        occ_ref, _ = osc.trace_any(rays)
        assert (slot_ref >= 0).sum() > 1000
        peak = dt.model_a(flat.bvh(), rays, dt.prim_test64(tris[n_ok]))["peak"]
        print(f"progression of {n_ok}: reference tree 64 levels; peak stack entries of the reference's loop: max {int(peak.max())}, {int((peak >= 33).sum())} rays above 32")
        assert (peak >= 33).sum() >= 64  # beyond the literal kernels' 32 LDS levels, far beyond the others'
        for trav in (3, 2, 1):
            ctx.set_option("traversal", trav)
            got = flat.trace_closest(rays)
            assert np.array_equal(got["prim"], slot_ref), f"traversal {trav}"
            assert_bits_equal(got["t"][slot_ref >= 0], t_ref[slot_ref >= 0], f"t, traversal {trav}")
            assert np.array_equal(flat.trace_any(rays).astype(bool), occ_ref.astype(bool)), f"traversal {trav}"
    finally:
        scene._flat = None
        flat.free()


STREAM_BUDGETS = (1, 3, 7, 2048)


@pytest.mark.parametrize("which", ["one chain", "twin chains"])
def test_streaming_wavefront_suspends_and_resumes_deep_stacks(T, ob, dctx, which):
    """A lit 40-level chain (matte slats, the camera inside the deep end looking along -x, one point light beside it), 24 x 24, 2 spp, depth 3, the tree through set_bvh
    (deep_trees.stream_scene).  With a fetch budget of b a ray is suspended before its interior fetches b + 1, 2 b + 1, ... with the entries it holds, and on resume those at
    level 16 and above go back into the overflow slab (th_trace2.h, the `lvl >= kStack2Lds` branches).  There are max_depth + 16 = 19 budgeted rounds: under budget 1 a
    suspended stack never exceeds 19 entries, so only levels 16 to 18 cross that branch, in three rounds; budgets 3 and 7 carry stacks of up to 38 entries across it.

    What must hold for every budget, and with a suspended-ray list of 64: film and per-sample radiance bit-equal to the classic wavefront and to the oracle on the same tree
    (the light makes every camera hit visible: the radiance says WHICH slat a ray hit first), the same ray counts, and — with the visit counters on — the same number of primitive
    tests whatever the budget: a ray that is suspended and resumed visits the leaves it would have visited uninterrupted, no leaf twice and none less.  (An entry written one slab
    row too high on resume passed the radiance comparison of an earlier form of this scene, whose light lit only the first dozen slats; it multiplies the primitive tests.)

    "twin chains": two such chains under one root, the camera between them: the rays of one wave hold different entries at the same level."""
    ctx = dctx
    tris, arrays, cam, scene = dt.stream_scene(T, which)
    flat = scene.flatten(ctx)
    try:
        flat.set_bvh(*arrays)
        assert flat.bvh_mode()[0] == 2
        osc = ob.OracleScene.from_scene(scene, bvh=arrays)
        # the witness: the frame's camera rays in model A, with the stack as k_trace2 keeps it
        rays = ob.generate_rays(cam, T.scenes.camera_sample_grid(cam, 2, seed=21))
        test = dt.oracle_prim_test(ob, osc)
        top = dt.tree_depth(arrays[1], arrays[2])
        for b in STREAM_BUDGETS[:3]:
            kern = dt.model_a(arrays, rays, test, kernel_like=True, budget=b)
            print(f"{which}, budget {b}: {rays.shape[0]} camera rays, {int((kern['prim'] >= 0).sum())} hits; entries held at the deepest suspension: "
                  f"{dt.histogram(kern['suspended_at'], top).tolist()}; closest hit in an entry restored above level 16: {int(kern['hit_restored'].sum())} rays")
            assert (kern["suspended_at"] >= 17).sum() >= 64
            if which == "one chain" and b > 1:
                assert kern["hit_restored"].sum() >= 64
        ref, ref_L, _ = osc.render(cam, "path", 2, 3, seed=21, want_samples=True)
        assert np.isfinite(ref).all() and (ref_L.sum(axis=-1) > 0).sum() >= (kern["prim"] >= 0).sum() // 2  # the camera hits are lit

        def render(**opts):
            for k, v in opts.items():
                ctx.set_option(k, v)
            try:
                integ = T.PathIntegrator(cam, T.SeededSampler(2, seed=21), 3)
                film = integ.render(scene, ctx).copy()
                return film, integ.sample_radiance(scene).copy(), integ.stats
            finally:
                for k in opts:
                    ctx.set_option(k, DEFAULTS[k])

        classic, classic_L, st0 = render(streaming=0)
        assert_bits_equal(classic_L, ref_L, "per-sample radiance, classic wavefront vs oracle")
        assert_bits_equal(classic, ref, "film, classic wavefront vs oracle")
        tested = {}
        for opts in [{"streaming": 1, "stream_budget_min": b} for b in STREAM_BUDGETS] + [{"streaming": 1, "stream_budget_min": 1, "stream_list_cap": 64}]:
            for count in (0, 1):
                film, L, st = render(count_visits=count, **opts)
                what = f"{which}, {opts}, count_visits {count}"
                assert_bits_equal(L, classic_L, f"per-sample radiance, {what} vs streaming 0")
                assert_bits_equal(L, ref_L, f"per-sample radiance, {what} vs oracle")
                assert_bits_equal(film, ref, f"film, {what} vs oracle")
                assert st.closest_rays == st0.closest_rays and st.shadow_rays == st0.shadow_rays, what
                if opts["stream_budget_min"] < 2048:
                    assert st.launches_shade > st0.launches_shade, f"{what}: the streaming wavefront shades in rounds, more of them than depths: it must not have declined the frame"
                if count and "stream_list_cap" not in opts:
                    tested[opts["stream_budget_min"]] = (int(st.prims_tested), int(st.prims_tested_shadow))
        print(f"{which}: primitive tests (closest, shadow) per budget: {tested}")
        assert tested[2048][0] > 0 and len(set(tested.values())) == 1, f"{which}: the budget changes the number of primitive tests: {tested}"
    finally:
        scene._flat = None
        flat.free()


@pytest.mark.parametrize("n,levels", list(zip(dt.FOUR_WIDE_SIZES, (19, 20, 21))))
def test_four_wide_walk_at_its_acceptance_edge(T, ob, dctx, n, levels):
    """A default commit (bvh_builder -1, no set_bvh) of the progression whose LIBRARY tree, folded four wide, has 19, 20 and 21 levels by the library's own count: the four-wide
    walk takes the first two (3 * (levels + 1) <= 64), the binary certified walk the third.  Results under the default: bit-equal to hybrid 0 and to traversal 1, and to the
    oracle on the reference tree it builds itself."""
    ctx = dctx
    tris = dt.progression(n).astype(np.float32)
    host = T._ffi.build_bvh_host(dt.prim_boxes(tris), 1, builder=0)
    assert dt.fold4(*host[:3])[1] == levels
    scene = dt.chain_scene(T, tris)
    flat = scene.flatten(ctx)
    try:
        mode = flat.bvh_mode()[0]
        assert mode in (2, 3), f"the scene is not certified: mode {mode}, {flat.bvh_note()}"
        for x, y, what in zip(flat.accelerator(), host[:4], ("bounds", "second children", "flags", "order")):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), f"the accelerator is not the host builder's tree: {what}"
        assert flat.bvh_mode()[2] == host[4]
        assert flat.closest_kernel_name() == ("k_trace3c4" if levels <= 20 else "k_trace3c"), (levels, flat.closest_kernel_name())
        rays = dt.four_wide_rays(tris)
        got = {}
        for name, opts in (("default", {}), ("hybrid 0", {"hybrid": 0}), ("traversal 1", {"traversal": 1})):
            for k, v in opts.items():
                ctx.set_option(k, v)
            try:
                assert flat.closest_kernel_name() == {"default": "k_trace3c4" if levels <= 20 else "k_trace3c", "hybrid 0": "k_trace3", "traversal 1": "k_trace_closest"}[name]
                hits = flat.trace_closest(rays)
                if name == "default":
                    fb = flat.last_fallback()
                got[name] = (hits, flat.trace_any(rays))
            finally:
                for k in opts:
                    ctx.set_option(k, DEFAULTS[k])
        print(f"progression of {n}: mode {mode}, accelerator depth {host[4]}, {levels} four-wide levels, {flat.closest_kernel_name()}; {fb[1]} of {fb[0]} rays handed back")
        assert (got["default"][0]["prim"] >= 0).sum() > 1000
        for name in ("hybrid 0", "traversal 1"):
            assert np.array_equal(got["default"][0]["prim"], got[name][0]["prim"]), f"default vs {name}: primitives"
            for f in ("t", "b1", "b2"):
                hit = got[name][0]["prim"] >= 0
                assert_bits_equal(got["default"][0][f][hit], got[name][0][f][hit], f"default vs {name}: {f}")
            assert np.array_equal(got["default"][1], got[name][1]), f"default vs {name}: occlusion"
        if mode == 2:  # the canonical tree is the reference's construction: the oracle builds the same one itself
            osc = ob.OracleScene.from_scene(scene)
            for x, y in zip(flat.bvh(), osc.get_bvh()):
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
        else:
            osc = ob.OracleScene.from_scene(scene, bvh=flat.bvh())
        sub = np.random.default_rng(9).choice(rays.shape[0], 600, replace=False)
        t_ref, slot_ref, _, _ = osc.trace_closest(rays[sub])
        occ_ref, _ = osc.trace_any(rays[sub])
        assert np.array_equal(got["default"][0]["prim"][sub], slot_ref)
        assert_bits_equal(got["default"][0]["t"][sub][slot_ref >= 0], t_ref[slot_ref >= 0], "t vs oracle")
        assert np.array_equal(got["default"][1][sub].astype(bool), occ_ref.astype(bool))
    finally:
        scene._flat = None
        flat.free()
