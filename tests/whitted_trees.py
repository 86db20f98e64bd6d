"""Scenes whose Whitted ray trees are WIDE — several glass interfaces in a row, so that a level holds many times the rays of the camera level — and the
oracle's count of rays per tree level.  Shared by tests/test_gpu_whitted_trees.py; everything here runs on the CPU.

All scenes stand in the Cornell box without its spheres (scenes.cornell_primitives(spheres=False)) under scenes.cornell_camera.  A "pane face" is one quad of
clear glass across the whole raster; two faces make a pane, and every face a ray meets splits it into a reflected and a transmitted child."""
import numpy as np

SEED = 0x5EED0C12
PANE_CORNERS = ((-0.3, -0.6), (1.4, -0.6), (1.4, 1.2), (-0.3, 1.2))
SCENES = {
    "window": dict(panes=(-2.05, -2.10, -2.30, -2.35), radii=()),       # a double-glazed window: four interfaces in front of the box
    "pane_sphere": dict(panes=(-2.05, -2.10), radii=(0.38,)),            # one pane in front of a glass sphere
    "nested": dict(panes=(), radii=(0.38, 0.25, 0.12)),                  # three concentric glass spheres, no pane
}
SPHERE_CENTRE = [0.5, 0.3, -2.6]
LIGHT_SETS = ("point", "point_spot", "point_sun", "point_front")
# Shadow rays of the reference have no far end (Trace.jl:196-202: t_max = Inf), so whatever lies beyond a light occludes it: inside the closed box every surface is black
# under the Cornell and the spot light, and the sun lights only what its rays reach through the open front.  Those frames pin the trees (ray for ray) but carry almost no
# radiance through them.  "point_front" adds what does: a matte ground in front of the box, below every camera ray, lit by a point light above it with nothing beyond —
# the rays the glass faces reflect back out of the box end there, so lit leaves hang under the interior nodes of every level and the fold has real sums to get right.
# A ray that ends on the ground was a miss without it: the trees keep their shape.
GROUND_Y, FRONT_LIGHT = -0.7, [0.5, 3.0, 1.0]


def glass(T):
    one = T.ConstantTexture(T.RGBSpectrum(1.0))
    return T.GlassMaterial(one, one, T.ConstantTexture(0.0), T.ConstantTexture(0.0), T.ConstantTexture(1.5), True)


def pane_face(T, z, material):
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    return [T.GeometricPrimitive(t, material) for t in T.scenes._quad(core, *[[x, y, z] for x, y in PANE_CORNERS], [0, 0, 1])]


def lights_of(T, name):
    """The Cornell point light alone, or with test_gpu_sppm's spot light, a directional light (preprocessed by make_scene) or the light over the ground in front."""
    lights = T.scenes.cornell_lights()
    if name == "point_spot":
        from test_gpu_sppm import spot_light
        lights.append(spot_light(T))
    elif name == "point_sun":
        lights.append(T.DirectionalLight(T.translate([0, 0, 0]), T.RGBSpectrum(0.9, 0.8, 0.7), np.float32([0.3, 1.0, 0.8])))
    elif name == "point_front":
        lights.append(T.PointLight(T.translate(FRONT_LIGHT), T.RGBSpectrum(40.0, 36.0, 30.0)))
    else:
        assert name == "point", name
    return lights


def ground(T):
    grey = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.6, 0.7, 0.5)), T.ConstantTexture(0.0))
    core = T.ShapeCore(T.translate([0, 0, 0]), False)
    y = GROUND_Y
    return [T.GeometricPrimitive(t, grey) for t in T.scenes._quad(core, [-1.5, y, -1.9], [2.5, y, -1.9], [2.5, y, 6.0], [-1.5, y, 6.0], [0, 1, 0])]


def make_scene(T, name, lights="point"):
    spec = SCENES[name]
    g = glass(T)
    prims, _ = T.scenes.cornell_primitives(spheres=False)
    for z in spec["panes"]:
        prims += pane_face(T, z, g)
    for r in spec["radii"]:
        prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate(SPHERE_CENTRE), False), r, 360.0), g))
    if lights == "point_front":
        prims += ground(T)
    scene = T.Scene(lights_of(T, lights), T.BVHAccel(prims, 1))
    for l in scene.lights:
        T.preprocess(l, scene)  # the directional light takes the scene's bounding sphere: its shadow rays leave the box
    return scene


def sample_pixels(cam):
    sb = cam.film.get_sample_bounds()
    return (int(sb.p_max[0] - sb.p_min[0]) + 1) * (int(sb.p_max[1] - sb.p_min[1]) + 1)


class OracleFrames:
    """The oracle's Whitted renders of one scene, each computed once: `frame` for the comparisons, `rays_per_camera_ray` for the preconditions."""

    def __init__(self, T, osc):
        self.T, self.osc, self._frames = T, osc, {}

    def frame(self, res, spp, depth, seed=SEED, sample_offset=0):
        key = (res, spp, depth, seed, sample_offset)
        if key not in self._frames:
            xyzw, L, st = self.osc.render(self.T.scenes.cornell_camera(res), "whitted", spp, depth, seed=seed, sample_offset=sample_offset, want_samples=True)
            for a in (xyzw, L):
                a.setflags(write=False)
            self._frames[key] = (xyzw, L, st)
        return self._frames[key]

    def closest_rays(self, res, spp, depth, seed=SEED):
        return 0 if depth == 0 else int(self.frame(res, spp, depth, seed)[2].closest_rays)

    def rays_per_camera_ray(self, res, spp, depth, levels=None, seed=SEED):
        """{level: rays of that tree level / camera rays} for `levels` (default: every level 1 … depth) of the depth-`depth` tree.  Whitted consumes no random
        number below the camera sample, so the tree to depth d - 1 is a prefix of the tree to depth d: level d holds closest_rays(d) - closest_rays(d - 1) rays."""
        n1 = self.closest_rays(res, spp, 1, seed)
        assert n1 == sample_pixels(self.T.scenes.cornell_camera(res)) * spp
        return {d: (self.closest_rays(res, spp, d, seed) - self.closest_rays(res, spp, d - 1, seed)) / n1 for d in (levels or range(1, depth + 1))}


def queue_slots_per_camera_ray(n_camera_rays, k_seg=32, k_seg_gran=256):
    """What one level's queue holds per camera ray of a batch of `n_camera_rays` (render_whitted_impl: queue_cap(2 n) segments of k_seg)."""
    cap = ((2 * n_camera_rays + k_seg - 1) // k_seg + 2 * k_seg_gran + k_seg_gran - 1) // k_seg_gran * k_seg_gran
    return cap * k_seg / n_camera_rays
