"""The preconditions of tests/shade_variants.py, from the oracle alone (no GPU): the scene that the GPU tests of the shading-kernel variants render must make every switch
matter, or a wrong index in a variant could hide behind samples that never reach it.  The floors are conditions the scene was tuned to meet; the achieved figures are printed
(-s) and recorded in docs/design/05-oracle-and-parity.md.  Also here: the oracle's SPPM renders a scene whose DirectionalLight no photon can pick."""
import numpy as np
import pytest

import directional_model as dm
import shade_variants as sv

_cache = {}


def radiance(T, ob, integrator, depth, **kw):
    """Per-sample radiance (n, 3) of the oracle on the reference's tree, computed once per configuration."""
    key = (integrator, depth, tuple(sorted(kw.items())))
    if key not in _cache:
        scene, _ = sv.build(T, **kw)
        _cache[key] = ob.OracleScene.from_scene(scene).render(sv.camera(T), integrator, sv.SPP, depth, seed=sv.SEED, want_samples=True)[1].reshape(-1, 3)
    return _cache[key]


@pytest.mark.parametrize("integrator,depth", [("path", sv.PATH_DEPTH), ("whitted", sv.WHITTED_DEPTH)])
def test_every_switch_matters_to_path_and_whitted(T, ob, integrator, depth):
    L = lambda **kw: radiance(T, ob, integrator, depth, **kw)  # noqa: E731
    tan, plain, tan_sun, sun, tan_raw = L(tangents=True), L(), L(tangents=True, sun="preprocessed"), L(sun="preprocessed"), L(tangents=True, sun="raw")
    assert tan.shape == (sv.SPP * 22 * 26, 3), "sample bounds 26 x 22: partial 16 x 16 tiles"
    non_black = float((np.nan_to_num(tan, nan=1.0) != 0).any(-1).mean())
    by_tangents, by_sun, by_tangents_under_sun = float(sv.differs(tan, plain).mean()), float(sv.differs(tan_sun, tan).mean()), float(sv.differs(tan_sun, sun).mean())
    by_raw_sun = int(sv.differs(tan_raw, tan).sum())
    scene, layout = sv.build(T, tangents=True)
    shares, caller = sv.first_hits(T, ob, ob.OracleScene.from_scene(scene), sv.camera(T), layout)
    print(f"{integrator} depth {depth}: non-black {non_black:.3f}; changed by tangents {by_tangents:.3f}, by the sun {by_sun:.3f}, by tangents under the sun {by_tangents_under_sun:.3f}, "
          f"by the raw sun {by_raw_sun} samples; first hits {({k: round(v, 3) for k, v in shares.items()})}")
    assert non_black >= 0.25
    assert by_tangents >= 0.05
    assert by_sun >= 0.10
    assert by_tangents_under_sun >= 0.05
    assert by_raw_sun >= 20
    for name in sv.MATERIALS:
        assert shares[name] >= 0.02, f"the {name} patch is the first hit of {shares[name]:.3f} of the camera samples"
    assert shares["sphere"] > 0 and shares["clipped_sphere"] > 0
    if integrator == "path":
        # the first vertex alone (depth 1) does not see the tangents, the whole path does: a second or later vertex on a tangent mesh, or the direction sampled at the first
        # with its frame, decided the sample.  Stricter: the camera ray did not even hit a patch.
        deep = sv.differs(tan, plain) & ~sv.differs(radiance(T, ob, "path", 1, tangents=True), radiance(T, ob, "path", 1))
        lo, hi = layout[next(iter(sv.MATERIALS))][0], layout[list(sv.MATERIALS)[-1]][1]
        off_patch = deep & ~((caller >= lo) & (caller < hi))
        print(f"path: tangents change {float(deep.mean()):.3f} of the samples beyond their first vertex, {float(off_patch.mean()):.3f} with a first hit off the patches")
        assert deep.mean() >= 0.05
        assert off_patch.sum() >= 20


def test_every_switch_matters_to_sppm(T, ob):
    P, cam = sv.SPPM, sv.camera(T)

    def run(**kw):
        scene, layout = sv.build(T, **kw)
        osc = ob.OracleScene.from_scene(scene)
        return osc.sppm(cam, P["radius"], P["depth"], P["iters"], P["photons"], seed=P["seed"]), osc, layout

    for kw in (dict(tangents=True), dict(tangents=True, sun="raw"), dict(tangents=True, sun="raw", crossing=True)):
        r, osc, layout = run(**kw)
        r0, _, _ = run(**{**kw, "tangents": False})
        lit = r["M"] > 0
        changed = float(sv.differs(r["phi"], r0["phi"])[lit].mean())
        print(f"SPPM {kw}: M.sum() {int(r['M'].sum())}, pixels with M > 0 {float(lit.mean()):.3f}, of which tangents change phi in {changed:.3f}; photon hits {r['info']['photon_hits']}")
        assert r["M"].sum() > 0
        assert changed >= 0.05
        if kw.get("crossing"):
            r1, _, _ = run(**{**kw, "crossing": False})
            shares, _ = sv.first_hits(T, ob, osc, cam, layout, spp=1)
            extra = int(r["stats"].closest_rays) - int(r1["stats"].closest_rays)
            print(f"  crossing: {extra} more closest-hit rays than without the quad; it is the first hit of {shares['crossing']:.3f} of the camera rays; Ld differs in "
                  f"{int(sv.differs(r['Ld'], r1['Ld']).sum())} pixels, M in {int((r['M'] != r1['M']).sum())}")
            assert extra > 0 and shares["crossing"] >= 0.02  # every crossing is one more closest-hit ray (tests/test_gpu_sppm_materialless.py)
            assert (r["M"] != r1["M"]).any(), "photons cross it too"
            assert sv.differs(r["Ld"], r1["Ld"]).any(), "and it casts a shadow"


def test_switches_are_read_back_from_the_scene(T, ob):
    for tangents in (False, True):
        for sun in sv.SUNS:
            for crossing in (False, True):
                scene, layout = sv.build(T, tangents, sun, crossing)
                assert sv.switches(T, scene) == (tangents, sun, crossing)
                n = max(hi for _, hi in layout.values())
                assert 16 < n <= 300, "more than tiny_scene_prims (a hierarchy), a few hundred at most"
                assert n == ob.OracleScene.from_scene(scene).n_prims


def test_oracle_sppm_renders_a_sun_no_photon_can_pick(T, ob):
    """A point light, then a sun that is not preprocessed (zero power): sample_discrete never picks it below 2^25 photons (api.sppm_directional_pick), so the reference would
    render the scene, the library renders it, and the oracle does.  Its iteration-1 Ld is the composite model's direct term, as test_gpu_directional_light asserts of the GPU."""
    scene = dm.floor_scene(T, "matte", "point_first", preprocessed=False)
    assert T.api.sppm_directional_pick(scene.lights, 48 * 48) == -1
    cam = T.scenes.shadows_camera(48)
    osc = ob.OracleScene.from_scene(scene)
    got = osc.sppm(cam, 0.05, 1, 1, seed=11)
    want, exact = dm.direct_terms(T, ob, scene, cam, 1, 11, "path", bvh=osc.get_bvh())
    sb = cam.film.get_sample_bounds()
    x0, y0 = -int(sb.p_min[0]) + 1, -int(sb.p_min[1]) + 1  # film pixel (1, 1) in the sample-pixel grid
    h, w = cam.film.size
    want, exact = want[0, y0:y0 + h, x0:x0 + w], np.broadcast_to(exact[0, y0:y0 + h, x0:x0 + w, None], (h, w, 3))
    assert exact.mean() > 0.9 and (want > 0).any()
    gi, wi = got["Ld"].view(np.int32).astype(np.int64), np.ascontiguousarray(want).view(np.int32).astype(np.int64)
    assert np.array_equal(gi[exact], wi[exact]), "Ld: bits differ where the model is exact"
    assert np.abs(gi - wi)[~exact].max(initial=0) <= 8
    assert np.isfinite(got["image"]).all()  # max_depth 1: no photon deposits, M stays 0
    # the same lights with the sun preprocessed: it has power, a photon picks it, and the oracle raises there as the reference would
    with pytest.raises(RuntimeError, match="picked a DirectionalLight"):
        ob.OracleScene.from_scene(dm.floor_scene(T, "matte", "point_first", True)).sppm(T.scenes.shadows_camera(16), 0.05, 2, 1, 100, seed=11)
