"""One scene family that drives every instantiation of the shading kernels (k_shade_path<STREAM, TAN, DIRL>, k_shade_whitted<0, DIRL>,
k_shade_sppm<TAN, DIRL, XING>, k_shade_photon<TAN, XING>), which the library picks from the scene's content alone:
  tangents   the seven material patches carry a tangent array (TAN)
  sun        "none", "preprocessed" or "raw": directional_model.sun behind the point and the spot light (DIRL); raw = not preprocessed, world_radius 0, zero power,
             which is the only sun SPPM accepts
  crossing   a material-less quad between the lights, the camera and the patches (XING; SPPM only: Whitted refuses such a scene)
The box walls are plain triangles.  Each entry of test_gpu_parity.MATERIALS sits on its own bumpy patch of 32 triangles with per-vertex normals and per-corner (u, v)s
whose ∂p/∂u is skewed against the patch's axes; the tangents are random directions (never parallel to ∂p/∂u), a few of them zero.  One full and one clipped sphere.
10 + 7 * 32 + 2 (+ 2) primitives: more than tiny_scene_prims, so the commit builds a hierarchy and the streaming wavefront applies.
Positions, lights and camera were tuned with the oracle alone (tests/test_shade_variants_scene.py asserts what they achieve)."""
import numpy as np

import directional_model as dm
from test_gpu_parity import MATERIALS
from test_gpu_sppm import spot_light

F = np.float32
GRID = 4  # quads per patch side: 2 * GRID^2 = 32 triangles
SPP, SEED = 3, 0x5AD
PATH_DEPTH, WHITTED_DEPTH = 6, 5
SPPM = dict(radius=0.08, depth=5, iters=3, photons=5000, seed=11)
SUNS = ("none", "preprocessed", "raw")
CAM_POS, CAM_TARGET = (0, 15, 50), (0, 0, -2)

# patch centre, side, (tilt about x, tilt about y) in degrees, bump phase — one per material, in MATERIALS' order
PATCHES = [
    ((0.20, 0.22, -2.55), 0.40, (-38.0, 20.0), 0.3),
    ((0.52, 0.16, -2.30), 0.38, (-55.0, -8.0), 1.1),
    ((0.82, 0.30, -2.60), 0.40, (-30.0, -28.0), 2.0),
    ((0.22, 0.62, -2.70), 0.40, (-12.0, 25.0), 2.9),
    ((0.55, 0.52, -2.80), 0.40, (-18.0, 4.0), 3.7),
    ((0.84, 0.70, -2.72), 0.38, (10.0, -26.0), 4.4),
    ((0.45, 0.86, -2.50), 0.36, (22.0, 10.0), 5.2),
]


def camera(T):
    """Film 24 x 20 under the default Lanczos filter: sample bounds 26 x 22, partial 16 x 16 tiles.  Inside the box's open side, looking at its back wall."""
    film = T.Film([24, 20], T.Bounds2([0.0, 0.0], [1.0, 1.0]), T.LanczosSincFilter([1.0, 1.0], 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at(list(CAM_POS), list(CAM_TARGET), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def _rot(ax_deg, ay_deg):
    ax, ay = np.deg2rad(ax_deg), np.deg2rad(ay_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return ry @ rx


def patch_arrays(k, tangents):
    """Unshared corners (3 per triangle): object-space vertices, normals of the smooth surface, (u, v)s, tangents or None."""
    (_, side, tilt, phase), g = PATCHES[k], GRID
    r = _rot(*tilt)

    def surf(a, b):
        z = 0.035 * np.sin(2 * np.pi * a + phase) * np.cos(1.5 * np.pi * b + 0.5 * phase)
        dza = 0.035 * 2 * np.pi * np.cos(2 * np.pi * a + phase) * np.cos(1.5 * np.pi * b + 0.5 * phase) / side
        dzb = -0.035 * 1.5 * np.pi * np.sin(2 * np.pi * a + phase) * np.sin(1.5 * np.pi * b + 0.5 * phase) / side
        p = np.stack([(a - 0.5) * side, (b - 0.5) * side, z], axis=-1)
        n = np.stack([-dza, -dzb, np.ones_like(a)], axis=-1)
        return p @ r.T, (n / np.linalg.norm(n, axis=-1, keepdims=True)) @ r.T

    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="xy")
    i, j = i.ravel(), j.ravel()
    corners = np.concatenate([np.stack([np.stack([i, j], 1), np.stack([i + 1, j], 1), np.stack([i + 1, j + 1], 1)], 1),
                              np.stack([np.stack([i, j], 1), np.stack([i + 1, j + 1], 1), np.stack([i, j + 1], 1)], 1)]).reshape(-1, 2) / g
    a, b = corners[:, 0], corners[:, 1]
    p, n = surf(a, b)
    uv = np.stack([0.8 * a + 0.45 * b, 0.9 * b - 0.2 * a], axis=1)  # ∂p/∂u is skewed against the patch's axes
    tg = None
    if tangents:
        rng = np.random.default_rng(100 + k)
        tg = rng.normal(size=p.shape).astype(F)
        tg[5::41] = 0.0  # a few zero tangents: the ts ⋅ ts > 0 branch
    return p.astype(F), n.astype(F), uv.astype(F), tg


def build(T, tangents=False, sun="none", crossing=False):
    """The scene and its layout: name -> (first, last + 1) caller-order primitive index of the walls, each material's patch, the spheres and the material-less quad."""
    assert sun in SUNS
    prims, white = T.scenes.cornell_primitives(spheres=False)
    layout = {"walls": (0, len(prims))}
    n = len(prims)
    for k, name in enumerate(MATERIALS):
        v, nrm, uv, tg = patch_arrays(k, tangents)
        core = T.ShapeCore(T.translate(list(PATCHES[k][0])), False)
        prims.append(T.create_mesh_primitives(core, np.arange(1, v.shape[0] + 1, dtype=np.uint32), v, nrm, MATERIALS[name](T), tangents=tg, uv=uv))
        layout[name] = (n, n + v.shape[0] // 3)
        n += v.shape[0] // 3
    mirror = T.MirrorMaterial(T.ConstantTexture(T.RGBSpectrum(0.95)))
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.14, 0.10, -2.22]), False), 0.10, 360.0), mirror))
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate([0.84, 0.13, -2.22]), False), 0.13, -0.05, 0.11, 270.0), white))
    layout["sphere"], layout["clipped_sphere"] = (n, n + 1), (n + 1, n + 2)
    n += 2
    if crossing:
        core = T.ShapeCore(T.translate([0, 0, 0]), False)
        quad = T.create_triangle_mesh(core, 2, np.uint32([1, 2, 3, 1, 3, 4]), 4, F([[0.1, 0.58, -2.05], [0.9, 0.58, -2.05], [0.9, 0.74, -2.75], [0.1, 0.74, -2.75]]))
        prims += [T.GeometricPrimitive(t, None) for t in quad]
        layout["crossing"] = (n, n + 2)
    lights = [T.PointLight(T.translate([0.5, 0.55, -1.75]), T.RGBSpectrum(1.6)), spot_light(T)]
    if sun != "none":
        lights.append(dm.sun(T))
    scene = T.Scene(lights, T.BVHAccel(prims, 1))
    if sun == "preprocessed":
        T.preprocess(lights[-1], scene)
    return scene, layout


def switches(T, scene):
    """(tangents, sun, crossing) read back from the scene description: what selects the kernels."""
    prims = T.api.splice_nested(scene.aggregate.primitives)
    tangents = any(isinstance(p, T.MeshPrimitives) and p.mesh.tangents is not None for p in prims)
    crossing = any(p.material is None for p in prims)
    suns = [l for l in scene.lights if isinstance(l, T.DirectionalLight)]
    sun = "none" if not suns else ("preprocessed" if float(suns[0].world_radius) > 0 else "raw")
    return tangents, sun, crossing


def first_hits(T, ob, osc, cam, layout, spp=SPP, seed=SEED):
    """Share of the camera samples whose first hit lies in each entry of the layout (from the oracle alone), and the per-sample caller-order primitive (-1: miss)."""
    rays = ob.generate_rays(cam, T.scenes.camera_sample_grid(cam, spp, seed))
    _, prim, _, _ = osc.trace_closest(rays)
    caller = np.where(prim >= 0, osc.get_bvh()[3][np.where(prim >= 0, prim, 0)].astype(np.int64), -1)
    return {name: float(((caller >= lo) & (caller < hi)).mean()) for name, (lo, hi) in layout.items()}, caller


def differs(a, b):
    """Per sample: do the radiances differ in their bits (a NaN against a number counts, NaN against NaN does not)?"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return (((a.view(np.uint32) != b.view(np.uint32)) & ~(na & nb)) | (na != nb)).any(axis=-1)
