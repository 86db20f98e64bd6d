"""Scenes for tests/test_gpu_shade_specular.py: what the specular class of the path shading kernel (PRIM_SPEC, th_scene.h) must and must not take.
Every frame is 32 x 32 under the Cornell camera, 4 spp, depth 8; the oracle renders the same scene on the committed tree.
  s_cornell       the benchmark's box: a mirror and a smooth-glass sphere, both PRIM_SPEC
  mirror_wall     a mirror quad fills the view: every camera sample is PRIM_SPEC and parks, so full 64-entry batches run from the first iteration on; a matte floor in
                  front of the mirror (outside the view) catches the reflected paths
  spec_triangles  mirror and smooth-glass patches of 32 triangles each, with vertex normals, (u, v)s and tangents (tangents=True) or flat without any of them, beside the
                  two spheres; more than 16 primitives, so the commit builds a hierarchy and the streaming wavefront applies
  inside_glass    a matte ball (r = 0.17) inside the glass sphere (r = 0.2) with a light in the shell between them: diffuse bounces reach the glass from inside at up to
                  asin(0.17 / 0.2) = 58 degrees, beyond the critical 41.8 (total internal reflection), and refract out below it (eta_i and eta_t swapped); 2 lights
  mixed           matte, plastic, mirror and glass spheres side by side: PRIM_SPEC and general entries share the ring and its batches
  generic_kinds   rough glass (two microfacet lobes), a black mirror (an empty lobe set) and a black-reflectance glass: none of them PRIM_SPEC
  lights          `mixed` with no light, with two point lights, with a DirectionalLight behind the point light"""
import numpy as np

import directional_model as dm
import shade_variants as sv
from test_gpu_parity import MATERIALS

F = np.float32
RES, SPP, DEPTH, SEED = 32, 4, 8, 0x5BEC


def camera(T):
    return T.scenes.cornell_camera(RES)


def _sphere(T, centre, radius, material):
    return T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate(list(centre)), False), radius, 360.0), material)


def _matte(T, *rgb):
    return T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(*rgb)), T.ConstantTexture(0.0))


def _glass(T, r=1.0, t=1.0, rough=0.0):
    return T.GlassMaterial(T.ConstantTexture(T.RGBSpectrum(r)), T.ConstantTexture(T.RGBSpectrum(t)), T.ConstantTexture(rough), T.ConstantTexture(rough), T.ConstantTexture(1.5), True)


def _scene(T, prims, lights):
    return T.Scene(lights, T.BVHAccel(prims, 1))


def s_cornell(T):
    return T.scenes.cornell_scene()


def mirror_wall(T):
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    quad = lambda pts: T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, F(pts))
    mirror = T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.9)))
    prims = [T.GeometricPrimitive(t, mirror) for t in quad([[-6, -6, -2.5], [7, -6, -2.5], [7, 7, -2.5], [-6, 7, -2.5]])]
    prims += [T.GeometricPrimitive(t, _matte(T, 0.8, 0.7, 0.6)) for t in quad([[-6, -1.5, -2.5], [7, -1.5, -2.5], [7, -1.5, 14], [-6, -1.5, 14]])]
    return _scene(T, prims, [T.PointLight(T.translate([0.5, 1.0, 2.0]), T.RGBSpectrum(40.0))])


def spec_triangles(T, tangents):
    prims, _ = T.scenes.cornell_primitives(spheres=True)
    mats = [MATERIALS["mirror"](T), MATERIALS["glass"](T), T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.7, 0.9, 0.8))), _glass(T, 0.9, 0.8)]
    for k, m in enumerate(mats):
        v, nrm, uv, tg = sv.patch_arrays(k, tangents)
        core = T.ShapeCore(T.translate(list(sv.PATCHES[k][0])), False)
        smooth = k < 2  # patches 0 and 1 carry normals and (u, v)s (and tangents); 2 and 3 are flat triangles
        prims.append(T.create_mesh_primitives(core, np.arange(1, v.shape[0] + 1, dtype=np.uint32), v, nrm if smooth else None, m, tangents=tg if smooth else None, uv=uv if smooth else None))
    return _scene(T, prims, T.scenes.cornell_lights())


def inside_glass(T):
    prims, white = T.scenes.cornell_primitives(spheres=False)
    c = (0.6, 0.25, -2.4)
    prims += [_sphere(T, c, 0.2, _glass(T)), _sphere(T, c, 0.17, _matte(T, 0.9, 0.6, 0.3))]
    return _scene(T, prims, T.scenes.cornell_lights() + [T.PointLight(T.translate([c[0], c[1] + 0.185, c[2]]), T.RGBSpectrum(0.05))])


def _mixed_primitives(T):
    prims, white = T.scenes.cornell_primitives(spheres=True)
    prims += [_sphere(T, (0.15, 0.1, -2.25), 0.1, _matte(T, 0.3, 0.7, 0.4)), _sphere(T, (0.5, 0.12, -2.2), 0.12, MATERIALS["plastic"](T)),
              _sphere(T, (0.85, 0.6, -2.7), 0.14, MATERIALS["plastic_noremap"](T)), _sphere(T, (0.45, 0.7, -2.8), 0.15, MATERIALS["mirror"](T))]
    return prims


def mixed(T):
    return _scene(T, _mixed_primitives(T), T.scenes.cornell_lights())


def generic_kinds(T):
    prims, _ = T.scenes.cornell_primitives(spheres=True)
    black_mirror = T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.0)))
    prims += [_sphere(T, (0.15, 0.12, -2.25), 0.12, MATERIALS["rough_glass"](T)), _sphere(T, (0.5, 0.12, -2.2), 0.12, black_mirror), _sphere(T, (0.85, 0.6, -2.7), 0.14, _glass(T, 0.0, 0.9)),
              _sphere(T, (0.45, 0.7, -2.8), 0.15, _glass(T, 0.0, 0.0))]
    return _scene(T, prims, T.scenes.cornell_lights())


def lights(T, which):
    prims = _mixed_primitives(T)
    if which == "none":
        return _scene(T, prims, [])
    if which == "two":
        return _scene(T, prims, T.scenes.cornell_lights() + [T.PointLight(T.translate([0.2, 0.5, -2.1]), T.RGBSpectrum(0.8, 1.0, 1.2))])
    assert which == "directional"
    ls = T.scenes.cornell_lights() + [dm.sun(T)]
    scene = _scene(T, prims, ls)
    T.preprocess(ls[-1], scene)
    return scene


CASES = {
    "s_cornell": s_cornell,
    "mirror_wall": mirror_wall,
    "spec_triangles": lambda T: spec_triangles(T, False),
    "spec_triangles_tangents": lambda T: spec_triangles(T, True),
    "inside_glass": inside_glass,
    "mixed": mixed,
    "generic_kinds": generic_kinds,
    "lights_none": lambda T: lights(T, "none"),
    "lights_two": lambda T: lights(T, "two"),
    "lights_directional": lambda T: lights(T, "directional"),
}
