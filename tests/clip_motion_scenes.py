"""The scene sequence of the clip-with-motion measurements (tests/test_clip_motion_api.py, tests/test_gpu_clip_motion.py, tools/clip_motion_probe.py): motion_scenes'
moving_scene with the sphere sliding mostly sideways over the floor, so that its shadow sweeps static surface, and the masks the figures are taken over.  Not a test."""
import numpy as np

import motion_scenes as ms

SPHERE_STEP = (0.03, 0.0, -0.015)  # per frame: 0.21 of the box's width in seven steps, from x = 0.3 to 0.51, and back to z = -2.705: clear of the turning cube (0.39 between the
                                   # centres, 0.364 the radii) and of the back wall, and still in front of the camera beside the cube
SWEPT_THRESHOLD = 0.10            # a swept pixel's 1024 spp luminance differs between the first and the last pose by more than this share of the larger


def step_motion(T, frame):
    """motion_scenes.step_motion with the sphere's step replaced by SPHERE_STEP; the cube turns as there."""
    motion = ms.step_motion(T, frame)
    motion[ms.SPHERE_INDEX] = T.translate(list(SPHERE_STEP))
    return motion


def scene_sequence(T, n_frames):
    """[(scene, motion)]: frame 0 is moving_scene with motion {} and every later frame the previous one moved by step_motion."""
    scene = ms.moving_scene(T)
    out = [(scene, {})]
    for k in range(1, n_frames):
        motion = step_motion(T, k)
        scene = scene.moved(motion)
        out.append((scene, motion))
    return out


def luminance(xyzw):
    """Y / w of a film, 0 where w is 0."""
    with np.errstate(all="ignore"):
        y = xyzw[..., 1].astype(np.float64) / xyzw[..., 3]
    return np.where(xyzw[..., 3] > 0, y, 0.0)


def swept_mask(static_surface, first_xyzw, last_xyzw):
    """Static surface pixels whose luminance differs between the two (1024 spp) films by more than SWEPT_THRESHOLD of the larger: where the shadow came or went."""
    a, b = luminance(first_xyzw), luminance(last_xyzw)
    larger = np.maximum(a, b)
    return static_surface & (larger > 0) & (np.abs(a - b) > SWEPT_THRESHOLD * larger)
