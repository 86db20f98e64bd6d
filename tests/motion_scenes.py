"""Scenes, cameras and motions of the moving-geometry tests (tests/test_motion_api.py, tests/test_gpu_motion.py, tools/motion_probe.py).  Not a test."""
import math

import numpy as np

CENTRE = np.array([0.5, 0.4, -2.5])  # of the Cornell box: the cameras of a sequence turn about it
CUBE_CENTRE, CUBE_HALF = (0.68, 0.22, -2.35), 0.13
SPHERE_CENTRE, SPHERE_RADIUS = (0.3, 0.2, -2.6), 0.18
N_WALL_ENTRIES = 10  # cornell_primitives(spheres=False): ten top-level triangles
SPHERE_INDEX, CUBE_INDEX = N_WALL_ENTRIES, N_WALL_ENTRIES + 1  # top-level indices of the two bodies in moving_scene


def camera(T, resolution, degrees=0.0, crop=None, radius=(1.0, 1.0)):
    """The temporal tests' camera, turned about the vertical axis through the box's centre.  resolution: one number or [width, height]; radius: the film filter's."""
    a = math.radians(degrees)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    eye, target = CENTRE + R @ (np.array([0.0, 15.0, 50.0]) - CENTRE), CENTRE + R @ (np.array([0.0, 0.0, -2.0]) - CENTRE)
    res = [resolution, resolution] if np.isscalar(resolution) else list(resolution)
    film = T.Film(res, T.Bounds2(*(crop or ([0.0, 0.0], [1.0, 1.0]))), T.LanczosSincFilter(list(radius), 3.0), 1.0, 1.0, "")
    return T.PerspectiveCamera(T.look_at(eye.tolist(), target.tolist(), [0, 1, 0]), T.Bounds2([-1.0, -1.0], [1.0, 1.0]), 0.0, 1.0, 0.0, 1e6, 90.0, film)


def cube_mesh(centre=CUBE_CENTRE, half=CUBE_HALF):
    """A cube of 12 triangles with face normals (24 vertices, four per face): (vertices, 1-based indices, normals)."""
    verts, nrm, idx = [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            n = np.zeros(3)
            n[axis] = sign
            u, v = np.zeros(3), np.zeros(3)
            u[(axis + 1) % 3], v[(axis + 2) % 3] = 1.0, 1.0
            if sign < 0:
                u, v = v, u  # keep u x v = n
            base = len(verts)
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                verts.append(np.asarray(centre) + half * (n + a * u + b * v))
                nrm.append(n)
            idx += [base + 1, base + 2, base + 3, base + 1, base + 3, base + 4]
    return np.array(verts, np.float32), np.array(idx, np.uint32), np.array(nrm, np.float32)


def cube_primitives(T, material):
    verts, idx, nrm = cube_mesh()
    return T.create_mesh_primitives(T.ShapeCore(T.translate([0, 0, 0]), False), idx, verts, nrm, material)


def moving_scene(T):
    """The Cornell walls, one matte sphere (top-level entry SPHERE_INDEX) and one small matte cube as a MeshPrimitives (CUBE_INDEX): the bodies of the sequences."""
    prims, _ = T.scenes.cornell_primitives(spheres=False)
    assert len(prims) == N_WALL_ENTRIES
    green = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.3, 0.7, 0.35)), T.ConstantTexture(0.0))
    sand = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.75, 0.7, 0.6)), T.ConstantTexture(0.0))
    prims.append(T.GeometricPrimitive(T.Sphere(T.ShapeCore(T.translate(list(SPHERE_CENTRE)), False), SPHERE_RADIUS, 360.0), green))
    prims.append(cube_primitives(T, sand))
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims, 1))


def id_scene(T):
    """Cornell with its two spheres and the small cube: misses (the camera sees past the box), spheres and triangles all occur in its id plane."""
    prims, _ = T.scenes.cornell_primitives()
    sand = T.MatteMaterial(T.ConstantTexture(T.RGBSpectrum(0.75, 0.7, 0.6)), T.ConstantTexture(0.0))
    return T.Scene(T.scenes.cornell_lights(), T.BVHAccel(prims + [cube_primitives(T, sand)], 1))


def rotation_about(T, centre, axis, degrees):
    """The rigid turn by `degrees` about the line through `centre` along coordinate axis `axis`, as a Transformation whose inverse is the turn back, both built in Float64 and
    rounded once."""
    def matrix(deg):
        a = math.radians(deg)
        c, s = math.cos(a), math.sin(a)
        i, j = (axis + 1) % 3, (axis + 2) % 3
        R = np.eye(4)
        R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
        to, back = np.eye(4), np.eye(4)
        to[:3, 3], back[:3, 3] = centre, -np.asarray(centre, np.float64)
        return to @ R @ back
    return T.Transformation(matrix(degrees).astype(np.float32), matrix(-degrees).astype(np.float32))


def step_motion(T, frame):
    """{top-level index: Transformation} that carries moving_scene's bodies from their pose at frame - 1 to their pose at `frame` (frame >= 1): the sphere rises by
    (0.02, 0.07, -0.025) per frame — most of a sigma_plane, so that the pass which ignores the motion loses the history on its top and bottom —, the cube turns 12 degrees
    per frame about the vertical axis through its own centre.  Eight frames keep both inside the box and apart."""
    assert frame >= 1
    return {SPHERE_INDEX: T.translate([0.02, 0.07, -0.025]), CUBE_INDEX: rotation_about(T, CUBE_CENTRE, 1, 12.0)}


def scene_sequence(T, n_frames):
    """[(scene, motion)]: frame 0 is moving_scene with motion {} and every later frame the previous one moved by step_motion."""
    scene = moving_scene(T)
    out = [(scene, {})]
    for k in range(1, n_frames):
        motion = step_motion(T, k)
        scene = scene.moved(motion)
        out.append((scene, motion))
    return out
