"""Host-side mirror of the part of Trace.jl's API that scene scripts touch, in Python.

The reference is Julia and no Julia runtime exists in this image, so the tested host above the C ABI is this module:
same names, same argument meaning, same (load-bearing) constructor bugs, Float32 arithmetic in the reference's
operation order.  Scene scripts written against ``Trace.X`` translate 1:1 to ``trace_jl_amd.X`` (see scenes.py, which
transcribes docs/src/shadows.md).  Everything numerically heavy happens behind ``libtracehip.so``; this module only
*constructs* (matrices, film geometry, filter table) and *flattens* the object graph through the C ABI.

Citations are file:line under /root/reference/src.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import TraceHipError

f32 = np.float32
_PI32 = f32(3.14159274101257324219)  # Float32(π)


def _deg2rad(x) -> np.float32:  # deg2rad(x::Float32) = x * (Float32(π) / 180f0)
    return f32(x) * (_PI32 / f32(180.0))


# ---- 4x4 Float32 matrices with StaticArrays' operation order --------------------------------------------------------------
def _mat(rows) -> np.ndarray:
    return np.array(rows, dtype=np.float32).reshape(4, 4)


def _mat_mul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    c = np.empty((4, 4), dtype=np.float32)
    for i in range(4):
        for j in range(4):
            c[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return c


def _det3(a, b, c, d, e, f, g, h, i):
    return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)


def _mat_inv(A: np.ndarray) -> np.ndarray:
    """inv(::Mat4f) as cofactor * (1/det) (StaticArrays' closed form; term order inside a cofactor is a documented
    tolerance source for general matrices)."""
    cof = np.empty((4, 4), dtype=np.float32)
    for r in range(4):
        for c in range(4):
            s = [A[i, j] for i in range(4) if i != r for j in range(4) if j != c]
            d = _det3(*s)
            cof[r, c] = -d if (r + c) & 1 else d
    det = ((A[0, 0] * cof[0, 0] + A[0, 1] * cof[0, 1]) + A[0, 2] * cof[0, 2]) + A[0, 3] * cof[0, 3]
    idet = f32(1.0) / det
    R = np.empty((4, 4), dtype=np.float32)
    for r in range(4):
        for c in range(4):
            R[r, c] = cof[c, r] * idet
    return R


class Transformation:
    """transformations.jl:1-22.  ``*`` multiplies the inverses in the same order (bug A.3, load-bearing)."""

    def __init__(self, m: Optional[np.ndarray] = None, inv_m: Optional[np.ndarray] = None):
        if m is None:
            m = np.eye(4, dtype=np.float32)
            inv_m = np.eye(4, dtype=np.float32)
        m = np.asarray(m, dtype=np.float32).reshape(4, 4)
        self.m = m
        self.inv_m = _mat_inv(m) if inv_m is None else np.asarray(inv_m, dtype=np.float32).reshape(4, 4)

    def __mul__(self, o: "Transformation") -> "Transformation":
        return Transformation(_mat_mul(self.m, o.m), _mat_mul(self.inv_m, o.inv_m))

    def inv(self) -> "Transformation":
        return Transformation(self.inv_m, self.m)

    def point(self, p) -> np.ndarray:  # :132-138
        m = self.m
        p = np.asarray(p, dtype=np.float32)
        one = f32(1.0)
        v = [((m[i, 0] * p[0] + m[i, 1] * p[1]) + m[i, 2] * p[2]) + m[i, 3] * one for i in range(4)]
        if v[3] == 1:
            return np.array(v[:3], dtype=np.float32)
        return np.array([v[0] / v[3], v[1] / v[3], v[2] / v[3]], dtype=np.float32)

    def vector(self, v) -> np.ndarray:  # :139
        m = self.m
        v = np.asarray(v, dtype=np.float32)
        return np.array([(m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2] for i in range(3)], dtype=np.float32)

    def swaps_handedness(self) -> bool:  # :161-163
        m = self.m
        return bool(_det3(m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2], m[2, 0], m[2, 1], m[2, 2]) < 0)


def inv(t: Transformation) -> Transformation:
    return t.inv()


def translate(d) -> Transformation:  # :24-38
    d = np.asarray(d, dtype=np.float32)
    return Transformation(_mat([[1, 0, 0, d[0]], [0, 1, 0, d[1]], [0, 0, 1, d[2]], [0, 0, 0, 1]]),
                          _mat([[1, 0, 0, -d[0]], [0, 1, 0, -d[1]], [0, 0, 1, -d[2]], [0, 0, 0, 1]]))


def scale(x, y, z) -> Transformation:  # :40-54
    x, y, z = f32(x), f32(y), f32(z)
    one = f32(1.0)
    return Transformation(_mat([[x, 0, 0, 0], [0, y, 0, 0], [0, 0, z, 0], [0, 0, 0, 1]]),
                          _mat([[one / x, 0, 0, 0], [0, one / y, 0, 0], [0, 0, one / z, 0], [0, 0, 0, 1]]))


def _norm3(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _normalize(v):
    v = np.asarray(v, dtype=np.float32)
    return (f32(1.0) / _norm3(v)) * v


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=np.float32)


def look_at(position, target, up) -> Transformation:  # :105-117
    position = np.asarray(position, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    up = np.asarray(up, dtype=np.float32)
    z = _normalize(position - target)
    x = _normalize(_cross(up, z))
    y = _cross(z, x)
    m = _mat([[x[0], y[0], z[0], 0], [x[1], y[1], z[1], 0], [x[2], y[2], z[2], 0], [0, 0, 0, 1]])
    return translate(position) * Transformation(m, m.T.copy())


def perspective(fov, near, far) -> Transformation:  # :119-130 — Mat4f literal filled column-major, no transpose (A.4)
    fov, near, far = f32(fov), f32(near), f32(far)
    p = np.zeros((4, 4), dtype=np.float32)
    p[0, 0] = 1
    p[1, 1] = 1
    p[2, 2] = far / (far - near)
    p[3, 2] = -far * near / (far - near)
    p[2, 3] = 1
    p[3, 3] = 0
    inv_tan = f32(1.0) / _ffi.detmath(2, _deg2rad(fov) / f32(2.0))[0]
    return scale(inv_tan, inv_tan, f32(1.0)) * Transformation(p)


def coordinate_system(v1):  # Trace.jl:139-146
    v1 = np.asarray(v1, dtype=np.float32)
    if abs(v1[0]) > abs(v1[1]):
        v2 = np.array([-v1[2], 0, v1[0]], dtype=np.float32) / np.sqrt(v1[0] * v1[0] + v1[2] * v1[2])
    else:
        v2 = np.array([0, v1[2], -v1[1]], dtype=np.float32) / np.sqrt(v1[1] * v1[1] + v1[2] * v1[2])
    return v1, v2, _cross(v1, v2)


# ---- spectrum / textures / materials -----------------------------------------------------------------------------------------
class RGBSpectrum:  # spectrum.jl:56-61
    def __init__(self, r=0.0, g=None, b=None):
        self.c = np.array([r, r, r] if g is None else [r, g, b], dtype=np.float32)


class ConstantTexture:  # textures/basic.jl:4-10
    def __init__(self, value):
        self.value = value


def _tex_rgb(t) -> List[float]:
    v = t.value if isinstance(t, ConstantTexture) else t
    return [float(x) for x in (v.c if isinstance(v, RGBSpectrum) else np.full(3, v, dtype=np.float32))]


def _tex_f(t) -> float:
    v = t.value if isinstance(t, ConstantTexture) else t
    return float(f32(v))


@dataclass(unsafe_hash=True)  # (hashable, by its fields as == compares them: Emitters takes {material: radiance})
class MatteMaterial:  # materials/material.jl:1-31
    Kd: ConstantTexture
    sigma: ConstantTexture

    def _flat(self):
        return 0, _tex_rgb(self.Kd) + [_tex_f(self.sigma)]


@dataclass(unsafe_hash=True)  # (hashable, by its fields as == compares them: Emitters takes {material: radiance})
class MirrorMaterial:  # :34-46
    Kr: ConstantTexture

    def _flat(self):
        return 1, _tex_rgb(self.Kr)


@dataclass(unsafe_hash=True)  # (hashable, by its fields as == compares them: Emitters takes {material: radiance})
class GlassMaterial:  # :49-116
    Kr: ConstantTexture
    Kt: ConstantTexture
    u_roughness: ConstantTexture
    v_roughness: ConstantTexture
    index: ConstantTexture
    remap_roughness: bool

    def _flat(self):
        return 2, _tex_rgb(self.Kr) + _tex_rgb(self.Kt) + [_tex_f(self.u_roughness), _tex_f(self.v_roughness), _tex_f(self.index), 1.0 if self.remap_roughness else 0.0]


@dataclass(unsafe_hash=True)  # (hashable, by its fields as == compares them: Emitters takes {material: radiance})
class PlasticMaterial:  # :119-151
    Kd: ConstantTexture
    Ks: ConstantTexture
    roughness: ConstantTexture
    remap_roughness: bool

    def _flat(self):
        return 3, _tex_rgb(self.Kd) + _tex_rgb(self.Ks) + [_tex_f(self.roughness), 1.0 if self.remap_roughness else 0.0]


# ---- shapes / primitives ---------------------------------------------------------------------------------------------------------
class ShapeCore:  # shapes/Shape.jl:1-15
    def __init__(self, object_to_world: Transformation, reverse_orientation: bool):
        self.object_to_world = object_to_world
        self.world_to_object = object_to_world.inv()
        self.reverse_orientation = bool(reverse_orientation)
        self.transform_swaps_handedness = object_to_world.swaps_handedness()


class Sphere:  # shapes/sphere.jl:1-30 (clamps and angles are derived inside the library, sphere.jl:13-26)
    def __init__(self, core: ShapeCore, radius, *args):
        self.core = core
        self.radius = f32(radius)
        if len(args) == 1:
            self.z_min, self.z_max, self.phi_max_deg = -self.radius, self.radius, f32(args[0])
        else:
            self.z_min, self.z_max, self.phi_max_deg = f32(args[0]), f32(args[1]), f32(args[2])


class TriangleMesh:  # shapes/triangle_mesh.jl:1-30: vertices go to world space here (:23), normals and tangents do not
    def __init__(self, core: ShapeCore, indices, vertices, normals=None, tangents=None, uv=None):
        self.core = core
        self.indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.object_vertices = v  # as passed by the caller (the oracle bridge re-derives world space from these)
        self.vertices = transform_points(core.object_to_world, v)
        self.normals = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        self.n_triangles = self.indices.size // 3
        # optional: one tangent per vertex (:11-12); (u, v)s, which the reference reads by CORNER position `mesh.uv[t.i + j]` (:82), i.e. 3 per triangle
        self.tangents = None if tangents is None else np.ascontiguousarray(tangents, dtype=np.float32).reshape(-1, 3)
        self.uv = None if uv is None else np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        if self.tangents is not None and self.tangents.shape[0] != v.shape[0]:
            raise ValueError("tangents: one per vertex")
        if self.uv is not None and self.uv.shape[0] < 3 * self.n_triangles:
            raise ValueError("uv: the reference indexes mesh.uv by corner position (triangle_mesh.jl:82): 3 * n_triangles entries are read")


def transform_points(t: Transformation, v: np.ndarray) -> np.ndarray:
    """(t::Transformation)(p::Point3f) for many points, Float32, left-to-right (transformations.jl:132-138)."""
    m = t.m
    one = f32(1.0)
    cols = [((m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]) + m[i, 2] * v[:, 2]) + m[i, 3] * one for i in range(4)]
    w = cols[3]
    out = np.stack(cols[:3], axis=1).astype(np.float32)
    div = w != 1
    if np.any(div):
        out[div] = out[div] / w[div, None]
    return np.ascontiguousarray(out, dtype=np.float32)


@dataclass
class Triangle:  # :32-43
    mesh: TriangleMesh
    k: int  # 0-based triangle number; the reference stores i = 3k + 1


def create_triangle_mesh(core: ShapeCore, n_triangles: int, indices, n_vertices: int, vertices, normals=None, tangents=None, uv=None) -> List[Triangle]:  # :45-58
    mesh = TriangleMesh(core, indices, vertices, normals, tangents, uv)
    assert mesh.n_triangles == n_triangles and mesh.vertices.shape[0] == n_vertices
    return [Triangle(mesh, k) for k in range(n_triangles)]


@dataclass
class GeometricPrimitive:  # primitive.jl:1-9
    shape: object
    material: object = None


@dataclass
class MeshPrimitives:
    """Bulk form of `[GeometricPrimitive(t, material) for t in create_triangle_mesh(...)]` for million-triangle meshes
    (one Python object instead of one per triangle); expands to exactly that list, in order."""
    mesh: "TriangleMesh"
    material: object = None


def create_mesh_primitives(core: ShapeCore, indices, vertices, normals=None, material=None, tangents=None, uv=None) -> MeshPrimitives:
    return MeshPrimitives(TriangleMesh(core, indices, vertices, normals, tangents, uv), material)


class BVHAccel:  # accel/bvh.jl:50-79: the tree itself is built inside the library at Scene flattening
    def __init__(self, primitives: Sequence[GeometricPrimitive], max_node_primitives: int = 1):
        self.primitives = list(primitives)
        self.max_node_primitives = min(255, int(max_node_primitives))


@dataclass
class PointLight:  # lights/point.jl:19-24
    light_to_world: Transformation
    i: RGBSpectrum


@dataclass
class SpotLight:  # lights/spot.jl:10-19
    light_to_world: Transformation
    i: RGBSpectrum
    total_width: float
    falloff_start: float


class DirectionalLight:  # lights/directional.jl:6-33 (mutable: preprocess! rewrites world_center / world_radius)
    def __init__(self, light_to_world: Transformation, l: RGBSpectrum, direction):
        self.light_to_world = light_to_world
        self.world_to_light = light_to_world.inv()
        self.i = l
        self.direction = _normalize(light_to_world.vector(direction))  # normalize(light_to_world(direction)) :29, a vector: no translation
        self.world_radius = f32(0.0)  # "To be computed in preprocessing stage" (:30): Scene never does (Trace.jl:184)
        self.world_center = np.zeros(3, dtype=np.float32)


# ---- bounds (bounds.jl) -------------------------------------------------------------------------------------------------------
# Julia's min / max on Float32: NaN wins, and -0 < +0 (so a union does not depend on the order of its operands).
def _jl_min(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    take_b = (b < a) | ((b == a) & np.signbit(b) & ~np.signbit(a)) | np.isnan(b)
    return np.where(take_b & ~np.isnan(a), b, a).astype(np.float32)


def _jl_max(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    take_b = (b > a) | ((b == a) & np.signbit(a) & ~np.signbit(b)) | np.isnan(b)
    return np.where(take_b & ~np.isnan(a), b, a).astype(np.float32)


def _jl_clamp(x, lo, hi):  # Base.clamp: ifelse(x > hi, hi, ifelse(x < lo, lo, x))
    return hi if x > hi else (lo if x < lo else x)


def _empty_bounds() -> np.ndarray:  # Bounds3() = Bounds3(Point3f(Inf32), Point3f(-Inf32))  bounds.jl:13
    return np.array([np.inf] * 3 + [-np.inf] * 3, dtype=np.float32)


def _union_points(b: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """b ∪ Bounds3(p) for every row p of pts (bounds.jl:59-61); min / max are exact, so the order is free."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    lo, hi = b[:3], b[3:]
    for p in pts:
        lo, hi = _jl_min(lo, p), _jl_max(hi, p)
    return np.concatenate([lo, hi]).astype(np.float32)


def _union_points_bulk(b: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """The same for many points at once (a million-triangle mesh): column extrema, with Julia's NaN and signed-zero rules."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    if pts.shape[0] == 0:
        return b
    lo, hi = b[:3].copy(), b[3:].copy()
    for a in range(3):
        col = pts[:, a]
        if np.isnan(col).any():
            lo[a] = hi[a] = np.float32(np.nan)
            continue
        mn, mx = col.min(), col.max()
        zs = np.signbit(col[col == 0])
        if mn == 0:
            mn = np.float32(-0.0) if zs.any() else np.float32(0.0)
        if mx == 0:
            mx = np.float32(0.0) if (~zs).any() else np.float32(-0.0)
        lo[a] = _jl_min(lo[a], mn)
        hi[a] = _jl_max(hi[a], mx)
    return np.concatenate([lo, hi]).astype(np.float32)


def _sphere_world_bound(s: "Sphere") -> np.ndarray:
    """world_bound(s) = object_to_world(object_bound(s)) (Shape.jl:17-19, sphere.jl:32-37): the 8 corners of the box over the CLAMPED
    z range of the constructor (sphere.jl:17-18), each through (t::Transformation)(p) (transformations.jl:141-143)."""
    r = s.radius
    z0 = _jl_clamp(min(s.z_min, s.z_max), -r, r)
    z1 = _jl_clamp(max(s.z_min, s.z_max), -r, r)
    lo, hi = (-r, -r, z0), (r, r, z1)
    corners = np.array([[(lo, hi)[c & 1][0], (lo, hi)[1 if c & 2 else 0][1], (lo, hi)[1 if c & 4 else 0][2]] for c in range(8)], dtype=np.float32)
    return _union_points(_empty_bounds(), np.stack([s.core.object_to_world.point(c) for c in corners]))


def _primitives_bound(prims) -> np.ndarray:
    b = _empty_bounds()
    for p in prims:
        if isinstance(p, BVHAccel):  # world_bound(bvh): its root box = the union of its primitives', Bounds3() when it has none (accel/bvh.jl:208-210)
            inner = _primitives_bound(p.primitives)
            b = np.concatenate([_jl_min(b[:3], inner[:3]), _jl_max(b[3:], inner[3:])]).astype(np.float32)
        elif isinstance(p, MeshPrimitives):
            m = p.mesh
            b = _union_points_bulk(b, m.vertices[m.indices.reshape(-1).astype(np.int64) - 1])  # 1-based indices (triangle_mesh.jl)
        elif isinstance(p.shape, Triangle):  # world_bound(t) = reduce(∪, Bounds3.(vertices(t)))  triangle_mesh.jl:97
            m, k = p.shape.mesh, p.shape.k
            b = _union_points(b, m.vertices[m.indices[3 * k:3 * k + 3].astype(np.int64) - 1])
        elif isinstance(p.shape, Sphere):
            sb = _sphere_world_bound(p.shape)
            b = np.concatenate([_jl_min(b[:3], sb[:3]), _jl_max(b[3:], sb[3:])]).astype(np.float32)
        else:
            raise TraceHipError(f"unsupported shape {type(p.shape).__name__}")
    return b


def _inside(b, p) -> bool:  # bounds.jl:71-73
    return bool(np.all(p >= b[:3]) and np.all(p <= b[3:]))


def bounding_sphere(b):
    """bounds.jl:145-149: (center, radius), center = (p_min + p_max) / 2f0, radius = distance(center, p_max) when the center is
    inside b, else 0f0.  ``b``: 6 floats (p_min, p_max), as Scene.bound returns."""
    b = np.asarray(b, np.float32).reshape(6)
    with np.errstate(invalid="ignore"):  # Bounds3(): Inf + -Inf = NaN, not inside
        center = ((b[:3] + b[3:]) / f32(2.0)).astype(np.float32)
    radius = _norm3(center - b[3:]) if _inside(b, center) else f32(0.0)  # distance(p1, p2) = norm(p1 - p2)  bounds.jl:127
    return center, f32(radius)


def preprocess(light, scene: "Scene") -> None:
    """preprocess!(light, scene): a DirectionalLight takes the scene's bounding sphere (directional.jl:35-37); Scene itself never
    calls it (Trace.jl:184), so an un-preprocessed light keeps world_radius = 0.  Other lights have nothing to preprocess."""
    if isinstance(light, DirectionalLight):
        light.world_center, light.world_radius = bounding_sphere(scene.bound)
        scene._flat = None  # the flattened scene holds the light's fields


def _light_key(l):
    return (id(l), bytes(np.asarray(l.direction, np.float32).tobytes()), float(l.world_radius), bytes(np.asarray(l.i.c, np.float32).tobytes())) if isinstance(l, DirectionalLight) else id(l)


class Scene:  # Trace.jl:176-187
    def __init__(self, lights, aggregate: BVHAccel):
        self.lights = list(lights)
        self.aggregate = aggregate
        self._flat = None
        self._bound = None
        self._base = None  # with_lights: the scene whose committed geometry this one shares

    def with_lights(self, lights) -> "Scene":
        """Scene(lights, self.aggregate) that shares this scene's committed geometry: its flatten() flattens this scene on the context if needed, then takes a relit view
        of it (trhip_scene_relight) and commits only the new lights.  Renders are bit for bit a fresh Scene(lights, self.aggregate)'s.  The geometry is the one this scene
        was committed with: primitives changed in place or options changed since do not apply to it (Scene(lights, aggregate) commits in full)."""
        s = Scene(lights, self.aggregate)
        s._base = self
        return s

    def moved(self, motion) -> "Scene":
        """The scene with some of its bodies carried to a new pose: `motion` is {index into self.aggregate.primitives: Transformation}, each the rigid motion of that
        top-level entry from its pose in this scene to the new one (a nested BVHAccel or a MeshPrimitives entry moves as a whole).  Returns a new Scene with the same lights,
        the same structure and the same material objects; entries without a motion are shared.  Host arithmetic only; the new scene commits in full when first rendered.
        A sphere gets the composed object_to_world (m = T.m o2w.m, inv_m = o2w.inv_m T.inv_m — the true inverse, not Transformation.__mul__'s).  A mesh's world-space
        vertices go through transform_points(T, .), its normals and tangents through T's linear part (the reference leaves both as the caller gave them, TriangleMesh above,
        so turning them is this helper's job); the moved mesh holds its vertices as given, under an identity object_to_world with the same effective orientation."""
        top = self.aggregate.primitives
        for k in motion:
            if not (isinstance(k, (int, np.integer)) and 0 <= k < len(top)):
                raise TraceHipError(f"Scene.moved: {k!r} is no index into the {len(top)} top-level primitives")
        meshes = {}

        def linear(T, v):
            m = T.m
            return np.ascontiguousarray(np.stack([(m[i, 0] * v[:, 0] + m[i, 1] * v[:, 1]) + m[i, 2] * v[:, 2] for i in range(3)], axis=1), dtype=np.float32)

        def moved_mesh(mesh, T):
            key = (id(mesh), id(T))
            if key not in meshes:
                new = TriangleMesh.__new__(TriangleMesh)
                new.core = ShapeCore(Transformation(), mesh.core.reverse_orientation != mesh.core.transform_swaps_handedness)
                new.indices, new.n_triangles, new.uv = mesh.indices, mesh.n_triangles, getattr(mesh, "uv", None)
                new.vertices = transform_points(T, mesh.vertices)
                new.object_vertices = new.vertices
                new.normals = None if mesh.normals is None else linear(T, mesh.normals)
                tangents = getattr(mesh, "tangents", None)
                new.tangents = None if tangents is None else linear(T, tangents)
                meshes[key] = new
            return meshes[key]

        def moved_primitive(p, T):
            if isinstance(p, BVHAccel):
                return BVHAccel([moved_primitive(q, T) for q in p.primitives], p.max_node_primitives)
            if isinstance(p, MeshPrimitives):
                return MeshPrimitives(moved_mesh(p.mesh, T), p.material)
            if isinstance(p.shape, Sphere):
                s, o2w = p.shape, p.shape.core.object_to_world
                core = ShapeCore(Transformation(_mat_mul(T.m, o2w.m), _mat_mul(o2w.inv_m, T.inv_m)), s.core.reverse_orientation)
                return GeometricPrimitive(Sphere(core, s.radius, s.z_min, s.z_max, s.phi_max_deg), p.material)
            if isinstance(p.shape, Triangle):
                return GeometricPrimitive(Triangle(moved_mesh(p.shape.mesh, T), p.shape.k), p.material)
            raise TraceHipError(f"Scene.moved: unsupported shape {type(p.shape).__name__}")

        prims = [moved_primitive(p, motion[i]) if i in motion else p for i, p in enumerate(top)]
        return Scene(self.lights, BVHAccel(prims, self.aggregate.max_node_primitives))

    @property
    def bound(self) -> np.ndarray:
        """scene.bound = world_bound(aggregate) (Trace.jl:183, accel/bvh.jl:208-210), as 6 Float32s p_min, p_max: the root box of the reference's BVH, i.e.
        the union of every primitive's world_bound (nested BVHs through their own root boxes), Bounds3() = (Inf, -Inf) without primitives."""
        if self._bound is None:
            self._bound = self._base.bound if self._base is not None else _primitives_bound(self.aggregate.primitives)
        return self._bound.copy()

    def flatten(self, ctx: Optional[_ffi.Context] = None) -> "FlatScene":
        # a light's fields may have changed since (preprocess, or a caller writing world_radius like Julia's mutable struct): the flat scene holds them
        if self._flat is not None and self._flat.light_keys != [_light_key(l) for l in self.lights]:
            self._flat = None
        if self._flat is None or (ctx is not None and self._flat.ctx is not ctx):
            if self._base is not None:  # with_lights: the base's committed geometry, this scene's lights (a light change relights again)
                self._flat = FlatScene.relight(self._base.flatten(ctx), self)
            else:
                self._flat = FlatScene(self, ctx or _ffi.default_context())
        return self._flat


# ---- sensor ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Bounds2:  # bounds.jl:1-4
    p_min: Sequence[float]
    p_max: Sequence[float]


@dataclass
class LanczosSincFilter:  # filter.jl:3-23
    radius: Sequence[float]
    tau: float

    def __call__(self, p) -> np.float32:
        return self._ws(f32(p[0]), f32(self.radius[0])) * self._ws(f32(p[1]), f32(self.radius[1]))

    def _sinc(self, x):
        x = abs(x)
        if x < f32(1e-5):
            return f32(1.0)
        x = x * _PI32
        return _ffi.detmath(0, x)[0] / x

    def _ws(self, x, r):
        x = abs(x)
        if x > r:
            return f32(0.0)
        return self._sinc(x) * self._sinc(x / f32(self.tau))


class Film:  # film.jl:7-62
    def __init__(self, resolution, crop_bounds: Bounds2, filter: LanczosSincFilter, diagonal, scale, filename: str):
        self.resolution = np.asarray(resolution, dtype=np.float32).reshape(2)
        res = self.resolution
        cmin = np.asarray(crop_bounds.p_min, dtype=np.float32)
        cmax = np.asarray(crop_bounds.p_max, dtype=np.float32)
        self.crop_window = (float(cmin[0]), float(cmin[1]), float(cmax[0]), float(cmax[1]))  # the constructor's fractional window (kept for hosts / tests)
        self.crop_bounds = Bounds2(np.ceil(res * cmin) + f32(1.0), np.ceil(res * cmax))  # :41-44
        self.filter = filter
        self.diagonal_mm = diagonal  # the constructor's argument (PerspectiveCamera.with_resolution)
        self.diagonal = f32(diagonal) * f32(0.001)
        self.scale = f32(scale)
        self.filename = filename
        w = int(abs(self.crop_bounds.p_max[0] - (self.crop_bounds.p_min[0] - f32(1.0))))  # inclusive_sides bounds.jl:100-102
        h = int(abs(self.crop_bounds.p_max[1] - (self.crop_bounds.p_min[1] - f32(1.0))))
        self.xyz = np.zeros((h, w, 3), dtype=np.float32)  # Pixel.xyz, (y, x)
        self.filter_weight_sum = np.zeros((h, w), dtype=np.float32)
        self.splat_xyz = np.zeros((h, w, 3), dtype=np.float32)
        self.filter_table_width = 16
        r = np.asarray(filter.radius, dtype=np.float32) / f32(16)
        self.filter_table = np.empty((16, 16), dtype=np.float32)  # (y, x) :55-59
        for y in range(16):
            for x in range(16):
                self.filter_table[y, x] = filter(((f32(x) + f32(0.5)) * r[0], (f32(y) + f32(0.5)) * r[1]))

    @property
    def size(self):
        return self.xyz.shape[:2]

    def get_sample_bounds(self) -> Bounds2:  # :68-73
        r = np.asarray(self.filter.radius, dtype=np.float32)
        return Bounds2(np.floor(np.asarray(self.crop_bounds.p_min) + f32(0.5) - r), np.ceil(np.asarray(self.crop_bounds.p_max) - f32(0.5) + r))

    def set_xyzw(self, xyzw: np.ndarray):
        self.xyz[...] = xyzw[..., :3]
        self.filter_weight_sum[...] = xyzw[..., 3]

    def to_rgb(self, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """save(film) up to the encoder (film.jl:204-222): linear RGB in [0,1], rows not flipped; computed on the GPU."""
        ctx = ctx or _ffi.default_context()
        h, w = self.size
        xyzw = np.ascontiguousarray(np.concatenate([self.xyz, self.filter_weight_sum[..., None]], axis=-1), dtype=np.float32)
        out = np.empty((h, w, 3), dtype=np.float32)
        ctx.check(_ffi.lib().trhip_film_to_rgb(ctx._h, _ffi.fptr(xyzw), w, h, float(self.scale), _ffi.fptr(out)))
        return out

    @staticmethod
    def add(a: np.ndarray, b: np.ndarray, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """a.xyz + b.xyz with a's weight lane, for two (H, W, 4) films (trhip_film_add; docs/design/23-direct-split.md): how a direct film goes back onto a filtered
        remainder."""
        a, b = _ffi.f32(a), _ffi.f32(b)
        if a.ndim != 3 or a.shape[2] != 4 or b.shape != a.shape:
            raise TraceHipError(f"Film.add: both films must be (H, W, 4), not {a.shape} and {b.shape}")
        ctx = ctx or _ffi.default_context()
        out = np.empty_like(a)
        ctx.check(_ffi.lib().trhip_film_add(ctx._h, _ffi.fptr(a), _ffi.fptr(b), a.shape[1], a.shape[0], _ffi.fptr(out), None))
        return out

    @staticmethod
    def add_device(d_a: int, d_b: int, width: int, height: int, d_out: int, ctx: Optional[_ffi.Context] = None) -> "_ffi.Stats":
        """The same on device pointers (d_out may equal d_a); nothing is copied to the host.  Returns the call's Stats."""
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        ctx.check(_ffi.lib().trhip_film_add_device(ctx._h, C.c_void_p(d_a), C.c_void_p(d_b), int(width), int(height), C.c_void_p(d_out), C.byref(st)))
        return st


def save(film: Film, ctx: Optional[_ffi.Context] = None) -> str:
    """film.jl:204-222: writes film.filename (8-bit PNG, rows flipped, no gamma)."""
    from PIL import Image
    rgb = film.to_rgb(ctx)
    img = np.clip(np.rint(rgb[::-1] * 255.0), 0, 255).astype(np.uint8)
    Image.fromarray(img, "RGB").save(film.filename)
    return film.filename


class PerspectiveCamera:  # camera/perspective.jl:11-40, 58-80
    def __init__(self, camera_to_world: Transformation, screen_window: Bounds2, shutter_open, shutter_close, lens_radius, focal_distance, fov, film: Film):
        self.camera_to_world = camera_to_world
        self.shutter_open, self.shutter_close = f32(shutter_open), f32(shutter_close)
        self.lens_radius, self.focal_distance = f32(lens_radius), f32(focal_distance)
        self.film = film
        self.fov, self.screen_window = fov, screen_window
        self.camera_to_screen = perspective(fov, 0.01, 1000.0)  # near / far hard-coded at :65
        smin = np.asarray(screen_window.p_min, dtype=np.float32)
        smax = np.asarray(screen_window.p_max, dtype=np.float32)
        one = f32(1.0)
        self.screen_to_raster = (scale(film.resolution[0], film.resolution[1], 1) * scale(one / (smax[0] - smin[0]), one / (smax[1] - smin[1]), 1)
                                 * translate([-smin[0], -smax[1], f32(0.0)]))
        self.raster_to_screen = self.screen_to_raster.inv()
        self.raster_to_camera = self.camera_to_screen.inv() * self.raster_to_screen

    def sensor(self) -> _ffi.Sensor:
        s = _ffi.Sensor()
        s.raster_to_camera[:] = self.raster_to_camera.m.reshape(-1).tolist()
        s.camera_to_world[:] = self.camera_to_world.m.reshape(-1).tolist()
        s.lens_radius, s.focal_distance = float(self.lens_radius), float(self.focal_distance)
        s.shutter_open, s.shutter_close = float(self.shutter_open), float(self.shutter_close)
        f = self.film
        s.crop_min[:] = [float(x) for x in f.crop_bounds.p_min]
        s.crop_max[:] = [float(x) for x in f.crop_bounds.p_max]
        s.filter_radius[:] = [float(x) for x in f.filter.radius]
        s.filter_table[:] = f.filter_table.reshape(-1).tolist()
        s.scale = float(f.scale)
        return s

    def with_resolution(self, resolution) -> "PerspectiveCamera":
        """The same camera on a Film of another resolution: the fractional crop window, the filter, the diagonal, the scale and the filename are the film's (the pixel bounds
        of the crop are derived again, as Film derives them)."""
        f = self.film
        film = Film(resolution, Bounds2(f.crop_window[:2], f.crop_window[2:]), f.filter, f.diagonal_mm, f.scale, f.filename)
        return PerspectiveCamera(self.camera_to_world, self.screen_window, self.shutter_open, self.shutter_close, self.lens_radius, self.focal_distance, self.fov, film)

    def world_to_pixel(self) -> np.ndarray:
        """The 3 x 4 Float32 matrix M of trhip_sensor_world_to_pixel: with h = M (p, 1) for a world point p, (h.x / h.z, h.y / h.z) is p's position in film-array pixel
        coordinates (0-based, integers at pixel centres, [y][x] as in xyzw), valid iff h.z > 0.  Host arithmetic: no context, no GPU."""
        out = np.empty(12, dtype=np.float32)
        sn = self.sensor()
        rc = _ffi.lib().trhip_sensor_world_to_pixel(C.byref(sn), _ffi.fptr(out))
        if rc:
            raise TraceHipError(_ffi.lib().trhip_last_error(None).decode() or f"trhip_sensor_world_to_pixel failed ({rc})")
        return out.reshape(3, 4)


def get_film(camera: PerspectiveCamera) -> Film:  # perspective.jl:83
    return camera.film


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
class SeededSampler:
    """The build's seeded counter-based sampler (include/trace_sampler.h) behind UniformSampler's protocol
    (sampler/sampler.jl:129-151).  The reference's UniformSampler draws from Julia's unseeded global RNG."""

    def __init__(self, samples_per_pixel: int, seed: int = 0x5EED0001, sample_offset: int = 0):
        self.samples_per_pixel = int(samples_per_pixel)
        self.seed = int(seed)
        self.sample_offset = int(sample_offset)
        self.current_sample = 1
        self._pixel = (0, 0)
        self._dim = 0

    # -- the AbstractSampler protocol the render loops call (sampler/sampler.jl:129-151); values from include/trace_sampler.h.
    #    The kernels address dimensions directly (camera 0-4, path vertex v at 5 + 8 v); a host that walks the protocol
    #    sequentially consumes the same stream as long as it positions itself with start_vertex(v) at every path vertex.
    def _u(self, dim: int) -> np.float32:
        from . import scenes
        key = scenes.ts_stream_key(self.seed, self._pixel[0], self._pixel[1], self.sample_offset + self.current_sample - 1)
        return np.float32(scenes.ts_uniform(key, dim))

    def start_pixel(self, p):  # start_pixel! :147-149
        self.current_sample = 1
        self._pixel = (int(p[0]), int(p[1]))
        self._dim = 0

    def has_next_sample(self) -> bool:  # :141-143
        return self.current_sample <= self.samples_per_pixel

    def start_next_sample(self):  # start_next_sample! :144-146
        self.current_sample += 1
        self._dim = 0

    def start_vertex(self, v: int):
        self._dim = 5 + 8 * int(v)

    def get_1d(self) -> np.float32:  # :131
        self._dim += 1
        return self._u(self._dim - 1)

    def get_2d(self) -> np.ndarray:  # :132-134
        return np.array([self.get_1d(), self.get_1d()], dtype=np.float32)

    def get_camera_sample(self, p_raster):  # :135-139: (p_film, p_lens, time)
        self._dim = 0
        p = np.asarray(p_raster, dtype=np.float32)
        film = p + self.get_2d()
        return film.astype(np.float32), self.get_2d(), self.get_1d()


def UniformSampler(samples_per_pixel: int) -> SeededSampler:
    return SeededSampler(samples_per_pixel)


# ---- flattening ---------------------------------------------------------------------------------------------------------------------
def splice_nested(prims):
    """A BVHAccel may itself be a primitive of another (accel/bvh.jl:50-53, test/test_intersection.jl:137-138): its primitives are
    spliced in place — the library builds ONE BVH over the flat list (any BVH over the same primitives gives the same hits except
    exact-t ties)."""
    out = []
    for p in prims:
        if isinstance(p, BVHAccel):
            out += splice_nested(p.primitives)
        else:
            out.append(p)
    return out


def top_level_counts(scene: "Scene"):
    """How many primitives of the flat list each top-level entry of scene.aggregate.primitives stands for (a MeshPrimitives its triangles, a nested BVHAccel everything
    in it): the scene's structure as FlatScene.body_table and PreviewSession's motion frames see it."""
    def count(p):
        if isinstance(p, BVHAccel):
            return sum(count(q) for q in p.primitives)
        return p.mesh.n_triangles if isinstance(p, MeshPrimitives) else 1
    return [count(p) for p in scene.aggregate.primitives]


class FlatScene:
    """Walk Scene -> BVHAccel -> GeometricPrimitive -> shape/material and push everything through the C ABI."""

    def __init__(self, scene: Scene, ctx: _ffi.Context):
        L = _ffi.lib()
        self.ctx = ctx
        self._h = C.c_void_p()
        ctx.check(L.trhip_scene_new(ctx._h, C.byref(self._h)))
        mat_ids = {}
        self.materials = []  # the material objects in id order (kept: Emitters resolves a material object to its id through material_id_of)

        def material_id(m):
            if m is None:
                return 0x00FFFFFF
            if id(m) not in mat_ids:
                kind, params = m._flat()
                p = np.array(params, dtype=np.float32)
                out = C.c_uint32()
                ctx.check(L.trhip_scene_add_material(self._h, kind, _ffi.fptr(p), p.size, C.byref(out)))
                mat_ids[id(m)] = out.value
                self.materials.append(m)
            return mat_ids[id(m)]

        prims = splice_nested(scene.aggregate.primitives)
        self.n_prims = len(prims)
        self.top_counts = top_level_counts(scene)
        i = 0
        while i < len(prims):
            p = prims[i]
            if not isinstance(p, MeshPrimitives) and isinstance(p.shape, Sphere):
                s = p.shape
                o2w = s.core.object_to_world
                m, im = _ffi.f32(o2w.m), _ffi.f32(o2w.inv_m)
                ctx.check(L.trhip_scene_add_sphere(self._h, _ffi.fptr(m), _ffi.fptr(im), int(s.core.reverse_orientation), float(s.radius), float(s.z_min), float(s.z_max),
                                                   float(s.phi_max_deg), material_id(p.material), None))
                i += 1
            elif isinstance(p, MeshPrimitives):
                mesh = p.mesh
                idx = np.ascontiguousarray(mesh.indices.reshape(-1, 3), dtype=np.uint32)
                mats = np.full(idx.shape[0], material_id(p.material), dtype=np.uint32)
                core = mesh.core
                flip = int(core.reverse_orientation != core.transform_swaps_handedness)
                self._add_triangles(ctx, mesh, idx, mats, flip, None)
                i += 1
            elif isinstance(p.shape, Triangle):
                # batch consecutive triangles of the same mesh into one call (caller order is preserved)
                mesh = p.shape.mesh
                j = i
                ks, mats = [], []
                while j < len(prims) and not isinstance(prims[j], MeshPrimitives) and isinstance(prims[j].shape, Triangle) and prims[j].shape.mesh is mesh:
                    ks.append(prims[j].shape.k)
                    mats.append(material_id(prims[j].material))
                    j += 1
                idx = np.ascontiguousarray(mesh.indices.reshape(-1, 3)[np.array(ks)], dtype=np.uint32)
                mats = np.array(mats, dtype=np.uint32)
                core = mesh.core
                flip = int(core.reverse_orientation != core.transform_swaps_handedness)
                self._add_triangles(ctx, mesh, idx, mats, flip, np.array(ks))
                i = j
            else:
                raise TraceHipError(f"unsupported shape {type(p.shape).__name__}")
        self._add_lights(scene)
        ctx.check(L.trhip_scene_commit(self._h, scene.aggregate.max_node_primitives))

    @classmethod
    def relight(cls, base: "FlatScene", scene: Scene) -> "FlatScene":
        """A relit view of the committed `base` (trhip_scene_relight) with `scene`'s lights: the light stage of a commit alone, the geometry shared."""
        L = _ffi.lib()
        self = cls.__new__(cls)
        self.ctx = base.ctx
        self._h = C.c_void_p()
        self.n_prims = base.n_prims
        self.top_counts = base.top_counts
        self.materials = base.materials
        self.ctx.check(L.trhip_scene_relight(base._h, C.byref(self._h)))
        self._add_lights(scene)
        self.ctx.check(L.trhip_scene_commit(self._h, scene.aggregate.max_node_primitives))
        return self

    def _add_lights(self, scene: Scene):
        L, ctx = _ffi.lib(), self.ctx
        self.light_keys = [_light_key(l) for l in scene.lights]
        for l in scene.lights:
            m, im = _ffi.f32(l.light_to_world.m), _ffi.f32(l.light_to_world.inv_m)
            I = _ffi.f32(l.i.c)
            if isinstance(l, PointLight):
                ctx.check(L.trhip_scene_add_point_light(self._h, _ffi.fptr(m), _ffi.fptr(im), _ffi.fptr(I)))
            elif isinstance(l, SpotLight):
                ctx.check(L.trhip_scene_add_spot_light(self._h, _ffi.fptr(m), _ffi.fptr(im), _ffi.fptr(I), float(l.total_width), float(l.falloff_start)))
            elif isinstance(l, DirectionalLight):  # the fields as the light holds them now (preprocessed or not)
                ctx.check(L.trhip_scene_add_directional_light(self._h, _ffi.fptr(I), _ffi.fptr(_ffi.f32(l.direction)), float(f32(l.world_radius))))
            else:
                raise TraceHipError(f"unsupported light {type(l).__name__}")

    def _add_triangles(self, ctx, mesh, idx, mats, flip, ks):
        """One trhip_scene_add_triangles(_ex) call; ks = the triangle numbers of `idx` inside the mesh (None: all, in order) — the corner uvs follow them."""
        L = _ffi.lib()
        nrm, tan, uv = mesh.normals, getattr(mesh, "tangents", None), getattr(mesh, "uv", None)
        if tan is None and uv is None:
            ctx.check(L.trhip_scene_add_triangles(self._h, _ffi.fptr(mesh.vertices), mesh.vertices.shape[0], _ffi.u32ptr(idx), idx.shape[0], _ffi.optr(nrm), _ffi.u32ptr(mats), flip,
                                                  None))
            return
        if uv is not None:
            uv = uv[:3 * mesh.n_triangles].reshape(-1, 3, 2)
            uv = np.ascontiguousarray(uv if ks is None else uv[ks], dtype=np.float32)
        ctx.check(L.trhip_scene_add_triangles_ex(self._h, _ffi.fptr(mesh.vertices), mesh.vertices.shape[0], _ffi.u32ptr(idx), idx.shape[0], _ffi.optr(nrm), _ffi.optr(tan),
                                                 _ffi.optr(uv), _ffi.u32ptr(mats), flip, None))

    def bvh(self):
        L = _ffi.lib()
        nn, npr = C.c_uint32(), C.c_uint32()
        self.ctx.check(L.trhip_scene_bvh_size(self._h, C.byref(nn), C.byref(npr)))
        bounds = np.empty((nn.value, 6), dtype=np.float32)
        a = np.empty(nn.value, dtype=np.uint32)
        flags = np.empty(nn.value, dtype=np.uint32)
        order = np.empty(npr.value, dtype=np.uint32)
        self.ctx.check(L.trhip_scene_get_bvh(self._h, _ffi.fptr(bounds), _ffi.u32ptr(a), _ffi.u32ptr(flags), _ffi.u32ptr(order)))
        return bounds, a, flags, order

    def prim_order(self) -> np.ndarray:
        """prim_order of bvh() alone (prim_order[slot] = caller primitive index), without copying the nodes."""
        nn, npr = C.c_uint32(), C.c_uint32()
        self.ctx.check(_ffi.lib().trhip_scene_bvh_size(self._h, C.byref(nn), C.byref(npr)))
        order = np.empty(npr.value, dtype=np.uint32)
        self.ctx.check(_ffi.lib().trhip_scene_get_bvh(self._h, None, None, None, _ffi.u32ptr(order)))
        return order

    def body_table(self, bodies) -> np.ndarray:
        """body_of_prim of trhip_temporal_motion, in ordered-primitive slot order (what trhip_hit.prim and the id plane's prim index): `bodies` gives the rigid-body index
        of every TOP-LEVEL entry of scene.aggregate.primitives — a MeshPrimitives entry or a nested BVHAccel is one body for everything in it —, None meaning static
        (the word 0xFFFFFFFF).  The caller-order table goes through this scene's prim_order (FlatScene.bvh()'s fourth array)."""
        bodies = list(bodies)
        if len(bodies) != len(self.top_counts):
            raise TraceHipError(f"FlatScene.body_table: {len(bodies)} entries for {len(self.top_counts)} top-level primitives")
        words = np.array([_ffi.STATIC_BODY if b is None else int(b) for b in bodies], dtype=np.uint32)
        per_prim = np.repeat(words, self.top_counts)
        order = self.prim_order()
        if order.size != per_prim.size:
            raise TraceHipError(f"FlatScene.body_table: the scene holds {order.size} primitives, its top-level entries {per_prim.size}")
        return np.ascontiguousarray(per_prim[order], dtype=np.uint32)

    def material_id_of(self, material) -> int:
        """The id this flat scene gave `material` (the object itself, not an equal one) when it was flattened."""
        for k, m in enumerate(self.materials):
            if m is material:
                return k
        raise TraceHipError(f"the scene has no primitive with this {type(material).__name__} object")

    @property
    def geometry_id(self) -> int:
        """Which committed geometry this flat scene holds (trhip_scene_geometry_id): equal for a scene and its relit views (Scene.with_lights), new for every full commit."""
        out = C.c_uint64()
        self.ctx.check(_ffi.lib().trhip_scene_geometry_id(self._h, C.byref(out)))
        return out.value

    def bvh_note(self) -> str:
        """Why a default commit holds one tree instead of two (trhip_scene_bvh_note); "" when it holds both."""
        buf = C.create_string_buffer(512)
        self.ctx.check(_ffi.lib().trhip_scene_bvh_note(self._h, buf, 512))
        return buf.value.decode()

    def closest_kernel_name(self) -> str:
        """The kernel a closest-hit launch on this scene runs under the context's current options (trhip_closest_kernel_name)."""
        buf = C.create_string_buffer(64)
        self.ctx.check(_ffi.lib().trhip_closest_kernel_name(self.ctx._h, self._h, buf, 64))
        return buf.value.decode()

    def bvh_mode(self):
        """(mode, accelerator nodes, accelerator depth): mode 0 = the library's tree alone, 1 = the canonical (reference / host) tree alone, 2 = hybrid: the canonical
        tree defines the answers, the library's tree accelerates the rays that carry the order-independence certificate (csrc/th_trace3c.h); 3 = the library's tree is the
        canonical one (the reference's construction fails on this scene) and, four children wide, its own accelerator."""
        mode, nn, dep = C.c_int(), C.c_uint32(), C.c_uint32()
        self.ctx.check(_ffi.lib().trhip_scene_bvh_mode(self._h, C.byref(mode), C.byref(nn), C.byref(dep)))
        return mode.value, nn.value, dep.value

    def accelerator(self):
        """The accelerator tree of a hybrid scene, in the layout of bvh() (order[accelerator slot] = caller primitive index)."""
        mode, nn, _ = self.bvh_mode()
        if mode not in (2, 3):
            raise _ffi.TraceHipError("the scene has no accelerator tree")
        L = _ffi.lib()
        npr = C.c_uint32()
        self.ctx.check(L.trhip_scene_bvh_size(self._h, None, C.byref(npr)))
        bounds = np.empty((nn, 6), dtype=np.float32)
        a = np.empty(nn, dtype=np.uint32)
        flags = np.empty(nn, dtype=np.uint32)
        order = np.empty(npr.value, dtype=np.uint32)
        self.ctx.check(L.trhip_scene_get_accelerator(self._h, _ffi.fptr(bounds), _ffi.u32ptr(a), _ffi.u32ptr(flags), _ffi.u32ptr(order)))
        return bounds, a, flags, order

    def set_bvh(self, bounds, a, flags, order):
        bounds, a, flags, order = _ffi.f32(bounds), np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(flags, np.uint32), np.ascontiguousarray(order, np.uint32)
        self.ctx.check(_ffi.lib().trhip_scene_set_bvh(self._h, _ffi.fptr(bounds), _ffi.u32ptr(a), _ffi.u32ptr(flags), a.size, _ffi.u32ptr(order), order.size))

    def trace_closest(self, rays: np.ndarray) -> np.ndarray:
        rays = _ffi.f32(rays).reshape(-1, 8)
        out = np.empty(rays.shape[0], dtype=_ffi.HIT_DTYPE)
        self.ctx.check(_ffi.lib().trhip_trace_closest(self.ctx._h, self._h, _ffi.fptr(rays), rays.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def accelerator_note(self) -> str:
        """Why this scene's accelerator is idle under the context's current options (trhip_accelerator_note); "" when it is used."""
        buf = C.create_string_buffer(512)
        self.ctx.check(_ffi.lib().trhip_accelerator_note(self.ctx._h, self._h, buf, 512))
        return buf.value.decode()

    def last_fallback(self):
        """(rays, rays re-walked on the canonical tree) of the last closest-hit trace call (hybrid mode: th_trace3c.h)."""
        out = np.zeros(2, np.uint64)
        self.ctx.check(_ffi.lib().trhip_last_fallback_counts(self.ctx._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return int(out[0]), int(out[1])

    def trace_any(self, rays: np.ndarray) -> np.ndarray:
        rays = _ffi.f32(rays).reshape(-1, 8)
        out = np.empty(rays.shape[0], dtype=np.uint8)
        self.ctx.check(_ffi.lib().trhip_trace_any(self.ctx._h, self._h, _ffi.fptr(rays), rays.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def hit_geometry(self, rays: np.ndarray) -> np.ndarray:
        rays = _ffi.f32(rays).reshape(-1, 8)
        out = np.empty((rays.shape[0], 15), dtype=np.float32)
        self.ctx.check(_ffi.lib().trhip_hit_geometry(self.ctx._h, self._h, _ffi.fptr(rays), rays.shape[0], _ffi.fptr(out)))
        return out

    def bsdf_query(self, material: int, allow_multiple_lobes: bool, mode: int, flags: int, frame9, dirs6) -> np.ndarray:
        frame9, dirs6 = _ffi.f32(frame9).reshape(-1, 9), _ffi.f32(dirs6).reshape(-1, 6)
        out = np.empty((frame9.shape[0], 8), dtype=np.float32)
        self.ctx.check(_ffi.lib().trhip_bsdf_query(self.ctx._h, self._h, material, int(allow_multiple_lobes), mode, flags, _ffi.fptr(frame9), _ffi.fptr(dirs6), frame9.shape[0], _ffi.fptr(out)))
        return out

    def free(self):
        if self._h:
            _ffi.lib().trhip_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- integrators -------------------------------------------------------------------------------------------------------------------
class _SamplerIntegrator:
    _entry = None

    def __init__(self, camera: PerspectiveCamera, sampler: SeededSampler, max_depth: int):
        self.camera, self.sampler, self.max_depth = camera, sampler, int(max_depth)
        self.stats: Optional[_ffi.Stats] = None

    def _render_film(self, flat: "FlatScene", entry: str, args, device_out: Optional[int]):
        """One film frame of the flattened scene through `entry`(ctx, scene, sensor, *args, out, stats) — `entry`_device with ``device_out``, a device pointer the film
        accumulators are then written to, nothing copied to the host and None returned; without it the film goes into camera.film and is returned."""
        ctx, sn, st, film = flat.ctx, self.camera.sensor(), _ffi.Stats(), self.camera.film
        if device_out is not None:
            entry, out, target = entry + "_device", None, C.c_void_p(device_out)
        else:
            out = np.empty(film.size + (4,), dtype=np.float32)
            target = _ffi.fptr(out)
        ctx.check(getattr(_ffi.lib(), entry)(ctx._h, flat._h, C.byref(sn), *args, target, C.byref(st)))
        self.stats = st
        if out is not None:
            film.set_xyzw(out)
        return out

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None, device_out: Optional[int] = None) -> np.ndarray:
        """Render into camera.film (and return xyzw, H x W x 4).  With ``device_out`` (a device pointer) the film
        accumulators are written there instead and nothing is copied to the host."""
        smp = self.sampler
        return self._render_film(scene.flatten(ctx), self._entry, (smp.samples_per_pixel, self.max_depth, smp.seed, smp.sample_offset), device_out)

    def sample_radiance(self, scene: Scene) -> np.ndarray:
        """Per-sample radiance of the last render: (spp, sb_h, sb_w, 3)."""
        flat = scene.flatten()
        sbh, sbw, _, _ = sample_bounds_shape(self.camera.film)
        out = np.empty((self.sampler.samples_per_pixel, sbh, sbw, 3), dtype=np.float32)
        flat.ctx.check(_ffi.lib().trhip_last_sample_radiance(flat.ctx._h, _ffi.fptr(out), out.size))
        return out

    def __call__(self, scene: Scene):
        """`integrator(scene)` / `scene |> integrator` (integrators/sampler.jl:12-56): render, then save(film)."""
        self.render(scene)
        if self.camera.film.filename:
            return save(self.camera.film)
        return None


class WhittedIntegrator(_SamplerIntegrator):  # integrators/sampler.jl:3-7
    _entry = "trhip_render_whitted"


class PathIntegrator(_SamplerIntegrator):
    """Not in the reference; defined in DESIGN.md from integrators/sppm.jl:208-266, 503-554."""
    _entry = "trhip_render_path"

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None, device_out: Optional[int] = None, sample_map: Optional["SampleMap"] = None,
               environment: Optional["Environment"] = None, env_scale: float = 1.0, hide_background: bool = False,
               emitters: Optional["Emitters"] = None, emit_scale: float = 1.0, emit_hits_only: bool = False, env_importance=None) -> np.ndarray:
        """_SamplerIntegrator.render; with ``sample_map`` a map frame (trhip_render_path_map): sample pixel p draws ``sample_map.counts[p]`` samples from the sampler's
        sample_offset on, and ``sampler.samples_per_pixel`` is not read.  With ``environment`` a path-env frame (trhip_render_path_env; docs/design/26-path-env.md): a path
        that leaves the scene brings back beta * E(dir) * env_scale — not at depth 1 with ``hide_background`` — and escapes() / relight() work on the frame afterwards.
        With ``env_importance`` as well — a mix in (0, 1), or True for 0.5 — the frame estimates the map's direct light at every non-specular vertex with one shadow ray,
        drawn from the map with that probability and from the BSDF otherwise (trhip_render_path_env_nee; docs/design/28-path-nee.md): far less noise under a small bright
        sun; escapes() and suppressed() work afterwards, relight() does not.  With ``emitters`` an emit frame (trhip_render_path_emit; docs/design/29-path-emit.md): the
        triangles of the set's materials shine with their radiance times ``emit_scale``, every non-specular vertex casts one shadow ray towards them, and emitted() works
        afterwards; ``emit_hits_only`` casts none and counts every hit on an emitter instead — plain path tracing, the reference estimator.  Without any of them it is
        trhip_render_path, the same call and the same bits."""
        smp = self.sampler
        if emitters is not None:
            if sample_map is not None or environment is not None or env_importance is not None:
                raise TraceHipError("PathIntegrator.render: emitters cannot be combined with sample_map or environment")
            prm = path_emit_params(emitters, emit_scale, emit_hits_only, "PathIntegrator.render")
            flat = scene.flatten(ctx)
            args = (smp.samples_per_pixel, self.max_depth, smp.seed, smp.sample_offset, emitters._handle_for(flat), C.byref(prm))
            return self._render_film(flat, "trhip_render_path_emit", args, device_out)
        if env_importance is not None:
            if sample_map is not None:
                raise TraceHipError("PathIntegrator.render: sample_map and env_importance cannot be combined (map frames have no environment term)")
            if environment is None:
                raise TraceHipError("PathIntegrator.render: env_importance needs an environment")
            prm = path_nee_params(environment, env_scale, hide_background, env_importance, "PathIntegrator.render")
            flat = scene.flatten(ctx)
            args = (smp.samples_per_pixel, self.max_depth, smp.seed, smp.sample_offset, environment._sampler_handle(flat.ctx), C.byref(prm))
            return self._render_film(flat, "trhip_render_path_env_nee", args, device_out)
        if environment is not None:
            if sample_map is not None:
                raise TraceHipError("PathIntegrator.render: sample_map and environment cannot be combined (map frames have no environment term)")
            prm = path_env_params(environment, env_scale, hide_background, "PathIntegrator.render")
            flat = scene.flatten(ctx)
            args = (smp.samples_per_pixel, self.max_depth, smp.seed, smp.sample_offset, environment._handle(flat.ctx), C.byref(prm))
            return self._render_film(flat, "trhip_render_path_env", args, device_out)
        if sample_map is None:
            return super().render(scene, ctx, device_out)
        flat = scene.flatten(ctx)
        counts = sample_map.for_film(self.camera.film)
        d_counts = _ffi.DeviceBuffer(counts.nbytes).from_host(counts) if device_out is not None else None  # a device frame reads its counts on the device
        try:
            args = (_ffi.u32ptr(counts) if d_counts is None else C.c_void_p(d_counts.ptr), sample_map.max_spp, self.max_depth, smp.seed, smp.sample_offset)
            return self._render_film(flat, "trhip_render_path_map", args, device_out)
        finally:
            if d_counts is not None:
                d_counts.free()

    def escapes(self, scene: Scene):
        """(beta, depth, dir) of the last render(environment=...) on the scene's context (trhip_last_escapes): beta and dir (spp, sb_h, sb_w, 3), depth (spp, sb_h, sb_w)
        int32 with 0 where the path did not escape; shaped like sample_radiance."""
        flat = scene.flatten()
        sbh, sbw, _, _ = sample_bounds_shape(self.camera.film)
        rec = np.empty((self.sampler.samples_per_pixel, sbh, sbw, 8), dtype=np.float32)
        flat.ctx.check(_ffi.lib().trhip_last_escapes(flat.ctx._h, _ffi.fptr(rec), rec.size))
        return rec[..., 0:3].copy(), rec[..., 3].astype(np.int32), rec[..., 4:7].copy()

    def emitted(self, scene: Scene):
        """(Lh, hits) of the last render(emitters=...) on the scene's context (trhip_last_emitted): the emitted light every camera sample collected, (spp, sb_h, sb_w, 3),
        and the number of hits on an emitter that counted, (spp, sb_h, sb_w) int32; shaped like sample_radiance."""
        flat = scene.flatten()
        sbh, sbw, _, _ = sample_bounds_shape(self.camera.film)
        rec = np.empty((self.sampler.samples_per_pixel, sbh, sbw, 4), dtype=np.float32)
        flat.ctx.check(_ffi.lib().trhip_last_emitted(flat.ctx._h, _ffi.fptr(rec), rec.size))
        return rec[..., 0:3].copy(), rec[..., 3].astype(np.int32)

    def suppressed(self, scene: Scene) -> np.ndarray:
        """Which escapes of the last render(environment=..., env_importance=...) do not count, because next-event estimation at the vertex before has already accounted for
        their light (the 8th float of trhip_last_escapes): (spp, sb_h, sb_w) bool, shaped like escapes()'s depth; all False after a frame without env_importance."""
        flat = scene.flatten()
        sbh, sbw, _, _ = sample_bounds_shape(self.camera.film)
        rec = np.empty((self.sampler.samples_per_pixel, sbh, sbw, 8), dtype=np.float32)
        flat.ctx.check(_ffi.lib().trhip_last_escapes(flat.ctx._h, _ffi.fptr(rec), rec.size))
        return rec[..., 7] != 0

    def relight(self, scene: Scene, environment: "Environment", env_scale: float = 1.0, hide_background: bool = False, device_out: Optional[int] = None) -> np.ndarray:
        """The film of the last render(environment=...) under another environment and / or other parameters, without tracing a ray (trhip_path_env_relight): film and
        sample_radiance equal a fresh render with these arguments bit for bit.  Valid only while that frame is the context's last; the counterpart of Scene.with_lights
        for the environment."""
        prm = path_env_params(environment, env_scale, hide_background, "PathIntegrator.relight")
        flat = scene.flatten()
        ctx, L = flat.ctx, _ffi.lib()
        if device_out is not None:
            ctx.check(L.trhip_path_env_relight_device(ctx._h, environment._handle(ctx), C.byref(prm), C.c_void_p(device_out)))
            return None
        h, w = self.camera.film.size
        out = np.empty((h, w, 4), dtype=np.float32)
        ctx.check(L.trhip_path_env_relight(ctx._h, environment._handle(ctx), C.byref(prm), _ffi.fptr(out)))
        self.camera.film.set_xyzw(out)
        return out


def path_env_params(environment, env_scale, hide_background, who: str) -> "_ffi.PathEnvParams":
    """trhip_path_env_params from the Python arguments, with the checks that need no library call answered here."""
    if not isinstance(environment, Environment):
        raise TraceHipError(f"{who}: environment must be an Environment, not {type(environment).__name__}")
    scale = float(env_scale)
    if not (scale >= 0.0 and math.isfinite(scale)):
        raise TraceHipError(f"{who}: env_scale must be finite and >= 0, not {env_scale}")
    p = _ffi.default_params(_ffi.PathEnvParams, "trhip_path_env_default_params")
    p.scale, p.flags = scale, _ffi.PATH_ENV_HIDE_BACKGROUND if hide_background else 0
    return p


def path_emit_params(emitters, emit_scale, emit_hits_only, who: str) -> "_ffi.PathEmitParams":
    """trhip_path_emit_params from the Python arguments, with the checks that need no library call answered here."""
    if not isinstance(emitters, Emitters):
        raise TraceHipError(f"{who}: emitters must be an Emitters, not {type(emitters).__name__}")
    scale = float(emit_scale)
    if not (scale >= 0.0 and math.isfinite(scale)):
        raise TraceHipError(f"{who}: emit_scale must be finite and >= 0, not {emit_scale}")
    p = _ffi.default_params(_ffi.PathEmitParams, "trhip_path_emit_default_params")
    p.scale, p.flags = scale, _ffi.PATH_EMIT_HITS_ONLY if emit_hits_only else 0
    return p


def path_nee_params(environment, env_scale, hide_background, env_importance, who: str) -> "_ffi.PathNeeParams":
    """trhip_path_nee_params from the Python arguments: path_env_params' checks, and env_importance — True (0.5) or a mix in (0, 1)."""
    e = path_env_params(environment, env_scale, hide_background, who)
    if env_importance is True:
        mix = 0.5
    elif isinstance(env_importance, bool) or not isinstance(env_importance, (int, float, np.floating)):
        raise TraceHipError(f"{who}: env_importance must be None, True or a mix in (0, 1), not {env_importance!r}")
    else:
        mix = float(env_importance)
    if not (0.0 < mix < 1.0) or not (0.0 < float(np.float32(mix)) < 1.0):
        raise TraceHipError(f"{who}: env_importance must lie in (0, 1), not {env_importance}")
    p = _ffi.default_params(_ffi.PathNeeParams, "trhip_path_nee_default_params")
    p.scale, p.flags, p.mix = e.scale, e.flags, mix
    return p


# ---- adaptive sampling (include/tracehip.h, trhip_render_path_map; docs/design/24-adaptive.md) ---------------------------------------------
def sample_bounds_shape(film: "Film"):
    """(sb_h, sb_w, x0, y0): the film's sample bounds — filter border included — as a shape and the raster pixel of its first entry."""
    sb = film.get_sample_bounds()
    return int(sb.p_max[1] - sb.p_min[1]) + 1, int(sb.p_max[0] - sb.p_min[0]) + 1, int(sb.p_min[0]), int(sb.p_min[1])


class SampleMap:
    """A per-pixel sample count for PathIntegrator.render(sample_map=...): ``counts`` is (sb_h, sb_w) uint32 over the film's SAMPLE pixels (get_sample_bounds, filter
    border included), every entry in 0 .. max_spp."""

    def __init__(self, counts, max_spp: int):
        c = np.asarray(counts)
        if c.ndim != 2 or c.size == 0:
            raise TraceHipError(f"SampleMap: counts must be (sb_h, sb_w), not {c.shape}")
        if np.any(c < 0) or np.any(c > int(max_spp)):
            raise TraceHipError(f"SampleMap: counts must lie in 0 .. max_spp = {int(max_spp)}")
        self.counts = np.ascontiguousarray(c, dtype=np.uint32)
        self.max_spp = int(max_spp)

    @property
    def total(self) -> int:
        return int(self.counts.sum(dtype=np.uint64))

    def for_film(self, film: "Film") -> np.ndarray:
        sbh, sbw, _, _ = sample_bounds_shape(film)
        if self.counts.shape != (sbh, sbw):
            raise TraceHipError(f"SampleMap: counts are {self.counts.shape}, the film's sample bounds {(sbh, sbw)}")
        return self.counts

    @classmethod
    def from_film(cls, film: "Film", counts_hw, max_spp: Optional[int] = None) -> "SampleMap":
        """From a count per FILM pixel, (H, W) in film.pixels order: every sample pixel takes the count of the nearest film pixel, clamped at the border."""
        c = np.asarray(counts_hw)
        h, w = film.size
        if c.shape != (h, w):
            raise TraceHipError(f"SampleMap.from_film: counts are {c.shape}, the film {(h, w)}")
        sbh, sbw, x0, y0 = sample_bounds_shape(film)
        fx0, fy0 = int(film.crop_bounds.p_min[0]), int(film.crop_bounds.p_min[1])  # raster pixel of film.pixels[0, 0]
        xs = np.clip(np.arange(sbw) + x0 - fx0, 0, w - 1)
        ys = np.clip(np.arange(sbh) + y0 - fy0, 0, h - 1)
        out = c[np.ix_(ys, xs)]
        return cls(out, int(out.max()) if max_spp is None else max_spp)

    @classmethod
    def region(cls, film: "Film", box, inside: int, outside: int) -> "SampleMap":
        """Region of interest: ``inside`` samples for the film pixels of box = (x0, y0, x1, y1) (film.pixels indices, x1 and y1 exclusive), ``outside`` elsewhere."""
        h, w = film.size
        x0, y0, x1, y1 = (int(v) for v in box)
        c = np.full((h, w), int(outside), dtype=np.int64)
        c[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = int(inside)
        return cls.from_film(film, c, max(int(inside), int(outside)))


def sample_map_model(mv, tau, eps, pilot: int, max_extra: int) -> np.ndarray:
    """trhip_sample_map in numpy, operation by operation in Float32 (include/tracehip.h): mv (sb_h, sb_w, 2) -> counts (sb_h, sb_w) uint32."""
    f = np.float32
    mv = np.asarray(mv, dtype=f)
    with np.errstate(all="ignore"):
        a = np.abs(mv[..., 0]) + f(eps)
        e = mv[..., 1] / (a * a)
        e = np.where(np.abs(e) < f(np.inf), e, f(np.inf)).astype(f)
        h, w = e.shape
        pad = np.full((h + 2, w + 2), f(0.0), dtype=f)  # +0 loses every `e > E`, like a pixel outside the bounds
        pad[1:-1, 1:-1] = e
        E = np.zeros((h, w), dtype=f)
        for dy in range(3):
            for dx in range(3):
                q = pad[dy:dy + h, dx:dx + w]
                E = np.where(q > E, q, E)
        x = (E / (f(tau) * f(tau))).astype(f)
        below = x < f(int(pilot) + int(max_extra))
        need = np.ceil(np.where(below, x, f(0.0))).astype(np.int64) - int(pilot)
    return np.where(below, np.maximum(need, 0), int(max_extra)).astype(np.uint32)


class AdaptivePathIntegrator:
    """Adaptive sampling on the public calls (docs/design/24-adaptive.md): a pilot trhip_render_path_device frame at n0 = sampler.samples_per_pixel >= 2,
    trhip_last_sample_stats_device and trhip_sample_map_device on its radiance records, then — when the map asks for any sample — a trhip_render_path_map_device frame at
    sample_offset + n0, and trhip_film_sum of the two films.  Every pixel keeps its pilot samples.  ``counts`` (sb_h, sb_w; the extra samples), ``total`` and ``stats``
    (the pilot's, and the map frame's or None) describe the last render."""

    def __init__(self, camera: PerspectiveCamera, sampler: SeededSampler, max_depth: int, tau: Optional[float] = None, max_extra: Optional[int] = None, eps: Optional[float] = None):
        if sampler.samples_per_pixel < 2:
            raise TraceHipError("AdaptivePathIntegrator: the pilot frame needs at least 2 samples per pixel (a variance)")
        self.camera, self.sampler, self.max_depth = camera, sampler, int(max_depth)
        p = _ffi.default_params(_ffi.SampleMapParams, "trhip_sample_map_default_params")
        p.pilot = sampler.samples_per_pixel
        if tau is not None:
            p.tau = tau
        if max_extra is not None:
            p.max_extra = int(max_extra)
        if eps is not None:
            p.eps = eps
        self.params = p
        self.counts: Optional[np.ndarray] = None
        self.total = 0
        self.mv: Optional[np.ndarray] = None
        self.stats = (None, None)

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        flat = scene.flatten(ctx)
        ctx = flat.ctx
        sn = self.camera.sensor()
        film = self.camera.film
        h, w = film.size
        sbh, sbw, _, _ = sample_bounds_shape(film)
        smp = self.sampler
        n0 = smp.samples_per_pixel
        L = _ffi.lib()
        bufs = [_ffi.DeviceBuffer(h * w * 16), _ffi.DeviceBuffer(h * w * 16), _ffi.DeviceBuffer(sbh * sbw * 8), _ffi.DeviceBuffer(sbh * sbw * 4), _ffi.DeviceBuffer(8)]
        d_pilot, d_extra, d_mv, d_counts, d_total = (C.c_void_p(b.ptr) for b in bufs)
        try:
            st0, st1 = _ffi.Stats(), None
            ctx.check(L.trhip_render_path_device(ctx._h, flat._h, C.byref(sn), n0, self.max_depth, smp.seed, smp.sample_offset, d_pilot, C.byref(st0)))
            ctx.check(L.trhip_last_sample_stats_device(ctx._h, d_mv))
            ctx.check(L.trhip_sample_map_device(ctx._h, d_mv, sbw, sbh, C.byref(self.params), d_counts, d_total))
            self.mv = bufs[2].to_host(np.float32, (sbh, sbw, 2))
            self.counts = bufs[3].to_host(np.uint32, (sbh, sbw))
            self.total = int(bufs[4].to_host(np.uint64, (1,))[0])
            if self.total:
                st1 = _ffi.Stats()
                ctx.check(L.trhip_render_path_map_device(ctx._h, flat._h, C.byref(sn), d_counts, self.params.max_extra, self.max_depth, smp.seed, smp.sample_offset + n0, d_extra,
                                                         C.byref(st1)))
                ctx.check(L.trhip_film_sum_device(ctx._h, d_pilot, d_extra, w, h, d_pilot))
            self.stats = (st0, st1)
            out = bufs[0].to_host(np.float32, (h, w, 4))
        finally:
            for b in bufs:
                b.free()
        film.set_xyzw(out)
        return out

    def tau_for_budget(self, mv, target_total: int, iterations: int = 60):
        """The tau whose map (sample_map_model: the kernel's arithmetic on the host, with this integrator's eps, pilot count and max_extra) totals closest to
        ``target_total`` extra samples: a bisection on log tau, for equal-ray comparisons.  Returns (tau, total); the total falls as tau grows and moves in steps, so
        it need not hit the target."""
        eps, pilot, max_extra = self.params.eps, self.params.pilot, self.params.max_extra
        total = lambda t: int(sample_map_model(mv, t, eps, pilot, max_extra).sum(dtype=np.uint64))
        lo, hi = np.float32(1e-6), np.float32(1e6)  # total(lo) >= target >= total(hi) wherever the target can be met
        best = min(((abs(total(t) - target_total), float(t)) for t in (lo, hi)))
        for _ in range(iterations):
            mid = np.float32(math.sqrt(float(lo) * float(hi)))
            if mid == lo or mid == hi:
                break
            n = total(mid)
            best = min(best, (abs(n - target_total), float(mid)))
            if n > target_total:
                lo = mid
            else:
                hi = mid
        return np.float32(best[1]), total(np.float32(best[1]))


# ---- first-hit feature buffers (include/tracehip.h, trhip_render_aov) -----------------------------------------------------------------
def base_colour(material) -> np.ndarray:
    """The base colour of a material as the feature buffers report it — a definition of this library (the reference has none): the constant texture the
    material's main lobe is built from, clamped like materials/material.jl clamps it before building the BSDF (clamp(spectrum), spectrum.jl:34-38):
    Matte Kd, Mirror Kr, Plastic Kd, Glass Kt unless it is black after the clamp (then Kr), no material zero."""
    def clamped(tex):
        return np.array([_jl_clamp(np.float32(x), np.float32(0.0), np.float32(np.inf)) for x in _tex_rgb(tex)], dtype=np.float32)
    if material is None:
        return np.zeros(3, np.float32)
    if isinstance(material, (MatteMaterial, PlasticMaterial)):
        return clamped(material.Kd)
    if isinstance(material, MirrorMaterial):
        return clamped(material.Kr)
    if isinstance(material, GlassMaterial):
        kt = clamped(material.Kt)
        return kt if not np.all(kt == 0) else clamped(material.Kr)
    raise TraceHipError(f"unsupported material {type(material).__name__}")


def primitive_materials(scene: "Scene"):
    """Per primitive in caller order (what prim_order of FlatScene.bvh() indexes): the material id FlatScene gives it (-1 without a material) and its base colour."""
    ids, cols, seen = [], [], {}
    for p in splice_nested(scene.aggregate.primitives):
        m = p.material
        if m is not None and id(m) not in seen:
            seen[id(m)] = len(seen)
        k = p.mesh.n_triangles if isinstance(p, MeshPrimitives) else 1
        ids += [-1 if m is None else seen[id(m)]] * k
        cols += [base_colour(m)] * k
    return np.array(ids, np.int32), np.array(cols, np.float32).reshape(-1, 3)


class AOVResult(dict):
    """What AOVIntegrator.render returns: a dict whose keys are also attributes."""
    __getattr__ = dict.__getitem__


class AOVIntegrator:
    """First-hit feature buffers of a frame (trhip_render_aov): depth, position, normals, base colour, ids — drawn with the camera samples of PathIntegrator for
    the same camera and sampler and filtered by the same film filter, so that they line up with the beauty frame at every antialiased edge.  No bounces, no
    lights, no BSDF: scenes without lights or with material-less primitives are fine."""

    def __init__(self, camera: PerspectiveCamera, sampler: SeededSampler):
        self.camera, self.sampler = camera, sampler
        self.stats: Optional[_ffi.Stats] = None

    def _sample_shape(self):
        return sample_bounds_shape(self.camera.film)[:2]

    def _call(self, scene, ctx, planes, samples, device, ids=None):
        """One frame through trhip_render_aov(_device), or, with an id plane asked for, through trhip_render_aov_ids(_device)."""
        flat = scene.flatten(ctx)
        ctx = flat.ctx
        sn, st, smp = self.camera.sensor(), _ffi.Stats(), self.sampler
        L = _ffi.lib()
        if ids is None:
            entry, outputs = (L.trhip_render_aov_device if device else L.trhip_render_aov), (planes, samples)
        else:
            entry, outputs = (L.trhip_render_aov_ids_device if device else L.trhip_render_aov_ids), (planes, samples, ids)
        ctx.check(entry(ctx._h, flat._h, C.byref(sn), smp.samples_per_pixel, smp.seed, smp.sample_offset, *outputs, C.byref(st)))
        self.stats = st

    def ids(self, scene: Scene, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """The id plane, (H, W) of _ffi.AOV_ID_DTYPE (trhip_render_aov_ids): per film pixel the nearest of its own spp camera samples — `prim` (the ordered-primitive
        slot, as in trhip_hit; FlatScene.bvh()'s prim_order[prim] is the caller's index), `material`, `t` — and `n_hit`, how many of them hit.  No hit: (-1, -1, inf, 0)."""
        h, w = self.camera.film.size
        out = np.empty((h, w), dtype=_ffi.AOV_ID_DTYPE)
        self._call(scene, ctx, None, None, False, ids=out.ctypes.data_as(C.c_void_p))
        return out

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None, device_out: Optional[int] = None, device_ids: Optional[int] = None):
        """The filtered planes.  Returns an AOVResult with `planes` (H, W, 3, 4: the raw, un-normalised sums of include/tracehip.h) and, each divided by its own
        weight where that weight is not zero (zero elsewhere), `albedo` (H, W, 3; by the weight of all samples), `normal`, `position` (H, W, 3) and `depth` (H, W)
        (by the weight of the hitting samples), and `alpha` = hit weight / total weight.  With ``device_out`` (a device pointer to H * W * 12 floats) the planes are
        written there, nothing is copied to the host and None is returned.  With ``device_ids`` (a device pointer to H * W 16-byte records; needs ``device_out``) the
        same call also writes the id plane there (trhip_render_aov_ids_device)."""
        if device_ids is not None:
            if device_out is None:
                raise TraceHipError("AOVIntegrator.render: device_ids needs device_out (for the id plane on the host use ids())")
            self._call(scene, ctx, C.c_void_p(device_out), None, True, ids=C.c_void_p(device_ids))
            return None
        if device_out is not None:
            self._call(scene, ctx, C.c_void_p(device_out), None, True)
            return None
        h, w = self.camera.film.size
        planes = np.empty((h, w, 3, 4), dtype=np.float32)
        self._call(scene, ctx, _ffi.fptr(planes), None, False)
        return self.normalise(planes)

    @staticmethod
    def normalise(planes: np.ndarray) -> AOVResult:
        planes = np.asarray(planes, np.float32)
        w_all, w_hit = planes[..., 0, 3], planes[..., 1, 3]

        def ratio(num, den):
            den = den[..., None] if num.ndim > den.ndim else den
            out = np.zeros(num.shape, np.float32)
            np.divide(num, den, out=out, where=np.broadcast_to(den != 0, num.shape))
            return out
        return AOVResult(planes=planes, albedo=ratio(planes[..., 0, :3], w_all), normal=ratio(planes[..., 1, :3], w_hit), position=ratio(planes[..., 2, :3], w_hit),
                         depth=ratio(planes[..., 2, 3], w_hit), alpha=ratio(w_hit, w_all))

    def samples(self, scene: Scene, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """The per-sample records, (spp, sb_h, sb_w) of _ffi.AOV_DTYPE: the trhip_hit of every camera ray, hit position, material id, geometric and shading normal, base colour."""
        sbh, sbw = self._sample_shape()
        out = np.empty((self.sampler.samples_per_pixel, sbh, sbw), dtype=_ffi.AOV_DTYPE)
        self._call(scene, ctx, None, out.ctypes.data_as(C.c_void_p), False)
        return out


# ---- ambient occlusion (include/tracehip.h, trhip_render_ao) ---------------------------------------------------------------------------
class AmbientOcclusionIntegrator(_SamplerIntegrator):
    """The picture of bare geometry (trhip_render_ao; docs/design/13-ao.md): the camera samples of PathIntegrator for the same camera and sampler, one cosine-distributed
    occlusion ray of reach `max_distance` from every first hit, radiance 1 where it escapes and 0 where it is stopped (times the base colour with ``albedo``), `background`
    where the camera ray misses.  No lights, no BSDF: a scene without lights or with material-less primitives renders.  One occlusion ray per camera sample: quality comes
    from the sampler's samples_per_pixel.  The film has the path frame's weights, so it goes through Denoiser.denoise with AOVIntegrator's planes."""

    def __init__(self, camera: PerspectiveCamera, sampler: SeededSampler, max_distance: float = math.inf, albedo: bool = False, background: float = 0.0):
        super().__init__(camera, sampler, 1)
        max_distance, background = float(max_distance), float(background)
        if not max_distance > 0.0:
            raise TraceHipError(f"AmbientOcclusionIntegrator: max_distance must be > 0 or inf, not {max_distance}")
        if not (background >= 0.0 and math.isfinite(background)):
            raise TraceHipError(f"AmbientOcclusionIntegrator: background must be finite and >= 0, not {background}")
        p = _ffi.default_params(_ffi.AoParams, "trhip_ao_default_params")
        p.max_distance, p.background, p.flags = max_distance, background, _ffi.AO_ALBEDO if albedo else 0
        self.params = p

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None, device_out: Optional[int] = None) -> np.ndarray:
        """Render into camera.film (and return xyzw, H x W x 4).  With ``device_out`` (a device pointer to H * W * 4 floats) the film accumulators are written there
        instead, nothing is copied to the host and None is returned."""
        smp = self.sampler
        return self._render_film(scene.flatten(ctx), "trhip_render_ao", (smp.samples_per_pixel, smp.seed, smp.sample_offset, C.byref(self.params)), device_out)


# ---- environment map and sky-lit frames (include/tracehip.h, trhip_env, trhip_render_sky) ----------------------------------------------------
def octahedral_directions(n: int) -> np.ndarray:
    """The unit direction (environment space) through the centre of every texel of an n x n octahedral map, (n, n, 3) Float64 indexed [j, i]: the inverse of the map
    the lookup applies (docs/design/25-sky.md).  Texel centre (i, j) is the point ((i + 0.5) / n * 2 - 1, (j + 0.5) / n * 2 - 1) of the square; outside the diamond
    |px| + |py| <= 1 lies the lower hemisphere, folded over the diamond's edges."""
    if not 1 <= n <= _ffi.ENV_MAX_N:
        raise TraceHipError(f"an environment map has n in [1, {_ffi.ENV_MAX_N}], not {n}")
    c = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0
    px, py = np.meshgrid(c, c, indexing="xy")
    z = 1.0 - np.abs(px) - np.abs(py)
    sgn = lambda v: np.where(v < 0, -1.0, 1.0)
    x = np.where(z < 0, (1.0 - np.abs(py)) * sgn(px), px)
    y = np.where(z < 0, (1.0 - np.abs(px)) * sgn(py), py)
    d = np.stack([x, y, z], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


class Environment:
    """An environment E(w), the radiance arriving from direction w: an octahedral map of n x n RGB texels (trhip_env; docs/design/25-sky.md).  `texels` is (n, n, 3),
    row j, column i, finite and >= 0, n in [1, 4096]; `world_to_env` a 3 x 3 matrix applied to every direction before the lookup (None: the identity).  The lookup
    itself is specified bit for bit; the texels are data, however they were made.  A device copy is created per context on first use and freed with this object."""

    def __init__(self, texels, world_to_env=None):
        t = np.asarray(texels)
        if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 3:
            raise TraceHipError(f"Environment: texels must be (n, n, 3), not {t.shape}")
        if not 1 <= t.shape[0] <= _ffi.ENV_MAX_N:
            raise TraceHipError(f"Environment: n must be in [1, {_ffi.ENV_MAX_N}], not {t.shape[0]}")
        t = np.ascontiguousarray(t, dtype=np.float32)
        if not np.isfinite(t).all() or (t < 0).any():
            raise TraceHipError("Environment: every texel must be finite and >= 0")
        r = np.eye(3, dtype=np.float32) if world_to_env is None else np.asarray(world_to_env)
        if r.shape != (3, 3):
            raise TraceHipError(f"Environment: world_to_env must be 3 x 3, not {r.shape}")
        r = np.ascontiguousarray(r, dtype=np.float32)
        if not np.isfinite(r).all():
            raise TraceHipError("Environment: every entry of world_to_env must be finite")
        self.texels, self.world_to_env = t, r
        self._handles = {}  # id(context) -> (context, trhip_env*)
        self._samplers = set()  # id(context) of the handles that have their sampling tables

    @property
    def n(self) -> int:
        return int(self.texels.shape[0])

    @classmethod
    def constant(cls, rgb) -> "Environment":
        """The same radiance from every direction: one texel."""
        return cls(np.asarray(rgb, dtype=np.float32).reshape(1, 1, 3))

    @classmethod
    def gradient(cls, zenith, horizon, ground, up=(0, 0, 1), n: int = 64) -> "Environment":
        """A sky that runs linearly in cos(angle to `up`) from `horizon` to `zenith` above the horizon and from `horizon` to `ground` below it."""
        u = np.asarray(up, dtype=np.float64)
        if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
            raise TraceHipError(f"Environment.gradient: up must be a non-zero vector of 3, not {up}")
        zenith, horizon, ground = (np.asarray(c, dtype=np.float64).reshape(3) for c in (zenith, horizon, ground))
        t = np.clip(octahedral_directions(int(n)) @ (u / np.linalg.norm(u)), -1.0, 1.0)[..., None]
        return cls(np.where(t >= 0, horizon + t * (zenith - horizon), horizon - t * (ground - horizon)))

    @classmethod
    def from_latlong(cls, image, n: Optional[int] = None) -> "Environment":
        """From a latitude-longitude image (H, W, 3), +z up: row 0 is the zenith, the last row the nadir, column 0 starts at azimuth 0 (the +x axis) and the azimuth
        grows towards +y.  Every texel centre's direction is found through the inverse octahedral map and the image is looked up there, bilinearly between pixel
        centres (wrapping in azimuth, clamped at the poles).  n defaults to the image's height, at most 4096."""
        img = np.asarray(image, dtype=np.float64)
        if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise TraceHipError(f"Environment.from_latlong: the image must be (H, W, 3), not {img.shape}")
        h, w = img.shape[:2]
        d = octahedral_directions(int(n) if n is not None else min(h, _ffi.ENV_MAX_N))
        v = np.arccos(np.clip(d[..., 2], -1.0, 1.0)) / np.pi * h - 0.5
        u = (np.arctan2(d[..., 1], d[..., 0]) / (2.0 * np.pi) % 1.0) * w - 0.5
        u0, v0 = np.floor(u), np.floor(v)
        tu, tv = (u - u0)[..., None], (v - v0)[..., None]
        c0, c1 = u0.astype(np.int64) % w, (u0.astype(np.int64) + 1) % w
        r0, r1 = np.clip(v0.astype(np.int64), 0, h - 1), np.clip(v0.astype(np.int64) + 1, 0, h - 1)
        top = img[r0, c0] * (1.0 - tu) + img[r0, c1] * tu
        bottom = img[r1, c0] * (1.0 - tu) + img[r1, c1] * tu
        return cls(top * (1.0 - tv) + bottom * tv)

    def _handle(self, ctx: _ffi.Context):
        """This map's trhip_env on `ctx`, created on first use."""
        if id(ctx) not in self._handles:
            h = C.c_void_p()
            ctx.check(_ffi.lib().trhip_env_create(ctx._h, _ffi.fptr(self.texels), self.n, _ffi.fptr(self.world_to_env), C.byref(h)))
            self._handles[id(ctx)] = (ctx, h)
        return self._handles[id(ctx)][1]

    def eval(self, dirs, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """E(w) for every direction of `dirs` (..., 3), evaluated on the device by the lookup the sky frame uses (trhip_env_eval)."""
        d = _ffi.f32(dirs)
        if d.ndim < 1 or d.shape[-1] != 3:
            raise TraceHipError(f"Environment.eval: directions must be (..., 3), not {d.shape}")
        ctx = ctx or _ffi.default_context()
        out = np.empty_like(d)
        ctx.check(_ffi.lib().trhip_env_eval(ctx._h, self._handle(ctx), _ffi.fptr(d), d.size // 3, _ffi.fptr(out)))
        return out

    def _sampler_handle(self, ctx: _ffi.Context):
        """This map's trhip_env on `ctx` with its sampling tables (trhip_env_make_sampler; docs/design/27-sky-importance.md), made on first use per context."""
        h = self._handle(ctx)
        if id(ctx) not in self._samplers:
            ctx.check(_ffi.lib().trhip_env_make_sampler(ctx._h, h))
            self._samplers.add(id(ctx))
        return h

    def sample(self, u, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """A unit direction for every point of `u` (..., 2) in [0, 1)^2, distributed like the map's radiance times solid angle: the device's deterministic sampler
        (trhip_env_sample).  The map's matrix must be orthonormal and the map not black."""
        p = _ffi.f32(u)
        if p.ndim < 1 or p.shape[-1] != 2:
            raise TraceHipError(f"Environment.sample: points must be (..., 2), not {p.shape}")
        if not ((p >= 0) & (p < 1)).all():
            raise TraceHipError("Environment.sample: every coordinate must lie in [0, 1)")
        ctx = ctx or _ffi.default_context()
        out = np.empty(p.shape[:-1] + (3,), dtype=np.float32)
        ctx.check(_ffi.lib().trhip_env_sample(ctx._h, self._sampler_handle(ctx), _ffi.fptr(p), p.size // 2, _ffi.fptr(out)))
        return out

    def pdf(self, dirs, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """The density, with respect to solid angle, with which sample() returns every direction of `dirs` (..., 3) (trhip_env_pdf)."""
        d = _ffi.f32(dirs)
        if d.ndim < 1 or d.shape[-1] != 3:
            raise TraceHipError(f"Environment.pdf: directions must be (..., 3), not {d.shape}")
        ctx = ctx or _ffi.default_context()
        out = np.empty(d.shape[:-1], dtype=np.float32)
        ctx.check(_ffi.lib().trhip_env_pdf(ctx._h, self._sampler_handle(ctx), _ffi.fptr(d), d.size // 3, _ffi.fptr(out)))
        return out

    def close(self):
        for ctx, h in self._handles.values():
            if ctx._h:  # (a context that was shut down took its device memory with it)
                _ffi.lib().trhip_env_free(h)
        self._handles = {}
        self._samplers = set()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Emitters:
    """The area lights of a scene (trhip_emitters; docs/design/29-path-emit.md): every triangle that carries one of the given material objects emits that material's
    radiance, on both sides.  ``radiance`` is {material object: RGBSpectrum}, each finite, >= 0.  The set is made from the scene's committed geometry — `scene` is flattened
    on `ctx` if it is not yet — and serves every relit view of it (Scene.with_lights); PathIntegrator.render(scene, emitters=...) renders with it."""

    def __init__(self, scene: Scene, radiance, ctx: Optional[_ffi.Context] = None):
        if not isinstance(radiance, dict) or not radiance:
            raise TraceHipError("Emitters: radiance must be a non-empty {material: RGBSpectrum}")
        mats, le = list(radiance.keys()), []
        for m in mats:
            v = radiance[m]
            c = np.asarray(v.c if isinstance(v, RGBSpectrum) else v, dtype=np.float32).reshape(-1)
            if c.shape != (3,) or not np.isfinite(c).all() or (c < 0).any():
                raise TraceHipError("Emitters: every radiance must be an RGBSpectrum with finite components >= 0")
            le.append(c)
        flat = scene.flatten(ctx)
        ids = np.array([flat.material_id_of(m) for m in mats], dtype=np.uint32)
        le = np.ascontiguousarray(np.stack(le), dtype=np.float32)
        self.ctx, self.geometry_id = flat.ctx, flat.geometry_id
        self._h = C.c_void_p()
        self.ctx.check(_ffi.lib().trhip_emitters_create(self.ctx._h, flat._h, _ffi.u32ptr(ids), _ffi.fptr(le), ids.size, C.byref(self._h)))
        n = C.c_uint32()
        self.ctx.check(_ffi.lib().trhip_emitters_size(self._h, C.byref(n)))
        self.n_triangles = int(n.value)

    def _handle_for(self, flat: "FlatScene"):
        if not self._h:
            raise TraceHipError("Emitters: closed")
        if flat.ctx is not self.ctx:
            raise TraceHipError("Emitters: made on another context than the scene's")
        return self._h

    def sample(self, u, ctx: Optional[_ffi.Context] = None):
        """(index, point, pdf_area) for every triple (xi, u0, u1) of `u` (..., 3) in [0, 1)^3: the emitter the device's sampler picks, the point on it and the density
        with respect to area (trhip_emitters_sample)."""
        p = _ffi.f32(u)
        if p.ndim < 1 or p.shape[-1] != 3:
            raise TraceHipError(f"Emitters.sample: points must be (..., 3), not {p.shape}")
        if not ((p >= 0) & (p < 1)).all():
            raise TraceHipError("Emitters.sample: every coordinate must lie in [0, 1)")
        if ctx is not None and ctx is not self.ctx:
            raise TraceHipError("Emitters.sample: made on another context")
        idx = np.empty(p.shape[:-1], dtype=np.uint32)
        pts = np.empty(p.shape[:-1] + (3,), dtype=np.float32)
        pdf = np.empty(p.shape[:-1], dtype=np.float32)
        self.ctx.check(_ffi.lib().trhip_emitters_sample(self.ctx._h, self._h, _ffi.fptr(p), p.size // 3, _ffi.u32ptr(idx), _ffi.fptr(pts), _ffi.fptr(pdf)))
        return idx, pts, pdf

    def close(self):
        if self._h and self.ctx._h:  # (a context that was shut down took its device memory with it)
            _ffi.lib().trhip_emitters_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SkyIntegrator(_SamplerIntegrator):
    """A sky-lit clay or albedo render (trhip_render_sky; docs/design/25-sky.md): AmbientOcclusionIntegrator's frame in which the occlusion ray that escapes brings
    back `environment`'s radiance from its direction, times `scale` (times the base colour with ``albedo``), and a camera ray that misses shows the environment (or 0
    with ``hide_background``).  No lights, no BSDF; one ray per camera sample, quality comes from the sampler's samples_per_pixel.  The film has the path frame's
    weights, so it goes through Denoiser.denoise with AOVIntegrator's planes, as an AO film does.

    ``importance`` (docs/design/27-sky-importance.md): None is that frame.  A float in (0, 1) — True is 0.5 — draws that share of the occlusion rays from the map's own
    distribution and weights every ray as the one-sample mixture estimator does (trhip_render_sky_is): unbiased as before, far less noise under a small bright sun."""

    def __init__(self, camera: PerspectiveCamera, sampler: SeededSampler, environment: Environment, max_distance: float = math.inf, albedo: bool = False, scale: float = 1.0,
                 hide_background: bool = False, importance=None):
        super().__init__(camera, sampler, 1)
        if not isinstance(environment, Environment):
            raise TraceHipError(f"SkyIntegrator: environment must be an Environment, not {type(environment).__name__}")
        if importance is not None and importance is not True:
            if isinstance(importance, bool) or not isinstance(importance, (int, float, np.floating)) or not 0.0 < float(importance) < 1.0:
                raise TraceHipError(f"SkyIntegrator: importance must be None, True or a float in (0, 1), not {importance}")
        max_distance, scale = float(max_distance), float(scale)
        if not max_distance > 0.0:
            raise TraceHipError(f"SkyIntegrator: max_distance must be > 0 or inf, not {max_distance}")
        if not (scale >= 0.0 and math.isfinite(scale)):
            raise TraceHipError(f"SkyIntegrator: scale must be finite and >= 0, not {scale}")
        p = _ffi.default_params(_ffi.SkyParams, "trhip_sky_default_params")
        p.max_distance, p.scale, p.flags = max_distance, scale, (_ffi.SKY_ALBEDO if albedo else 0) | (_ffi.SKY_HIDE_BACKGROUND if hide_background else 0)
        self.environment, self.params = environment, p
        self.is_params = None  # trhip_sky_is_params with `importance`: the frame is then trhip_render_sky_is
        if importance is not None:
            q = _ffi.default_params(_ffi.SkyIsParams, "trhip_sky_is_default_params")
            q.max_distance, q.scale, q.flags = p.max_distance, p.scale, p.flags
            if importance is not True:
                q.mix = float(importance)
            self.is_params = q

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None, device_out: Optional[int] = None) -> np.ndarray:
        """Render into camera.film (and return xyzw, H x W x 4).  With ``device_out`` (a device pointer to H * W * 4 floats) the film accumulators are written there
        instead, nothing is copied to the host and None is returned."""
        flat, smp = scene.flatten(ctx), self.sampler
        if self.is_params is not None:
            return self._render_is(flat, device_out)
        args = (smp.samples_per_pixel, smp.seed, smp.sample_offset, self.environment._handle(flat.ctx), C.byref(self.params))
        return self._render_film(flat, "trhip_render_sky", args, device_out)

    def _render_is(self, flat, device_out):
        """render() with `importance`: trhip_render_sky_is, the sampling tables made on first use."""
        smp = self.sampler
        args = (smp.samples_per_pixel, smp.seed, smp.sample_offset, self.environment._sampler_handle(flat.ctx), C.byref(self.is_params))
        return self._render_film(flat, "trhip_render_sky_is", args, device_out)


# ---- the inputs of the image-space passes: one check per kind, `who` the method named in the refusal -----------------------------------------
def _film_and_planes(who: str, xyzw, planes):
    """The (H, W, 4) film and the (H, W, 3, 4) planes of one frame, as contiguous Float32 arrays."""
    xyzw, planes = _ffi.f32(xyzw), _ffi.f32(planes)
    if xyzw.ndim != 3 or xyzw.shape[2] != 4 or planes.shape != xyzw.shape[:2] + (3, 4):
        raise TraceHipError(f"{who}: xyzw must be (H, W, 4) and planes (H, W, 3, 4), not {xyzw.shape} and {planes.shape}")
    return xyzw, planes


def _low_and_high(who: str, lo_xyzw, lo_planes, hi_planes):
    """The low-resolution film and planes and the full-size planes of an upscaling pass, as contiguous Float32 arrays."""
    lo_xyzw, lo_planes, hi_planes = _ffi.f32(lo_xyzw), _ffi.f32(lo_planes), _ffi.f32(hi_planes)
    if lo_xyzw.ndim != 3 or lo_xyzw.shape[2] != 4 or lo_planes.shape != lo_xyzw.shape[:2] + (3, 4) or hi_planes.ndim != 4 or hi_planes.shape[2:] != (3, 4):
        raise TraceHipError(f"{who}: lo_xyzw must be (h, w, 4), lo_planes (h, w, 3, 4) and hi_planes (H, W, 3, 4), not {lo_xyzw.shape}, {lo_planes.shape} and {hi_planes.shape}")
    return lo_xyzw, lo_planes, hi_planes


def _history_like(who: str, history, planes, planes_name: str = "planes"):
    """An optional history, shaped like the planes it is validated against."""
    if history is None:
        return None
    history = _ffi.f32(history)
    if history.shape != planes.shape:
        raise TraceHipError(f"{who}: history must be {planes.shape} like {planes_name}, not {history.shape}")
    return history


def _id_plane(who: str, ids, h: int, w: int, per: str = "pixel"):
    """An id plane: h * w 16-byte records (_ffi.AOV_ID_DTYPE), contiguous."""
    ids = np.ascontiguousarray(ids)
    if ids.nbytes != h * w * 16:
        raise TraceHipError(f"{who}: ids must hold one 16-byte record per {per}, not {ids.nbytes} bytes for {h} x {w}")
    return ids


def _body_tables(ids, body_of_prim, bodies):
    """(table, matrices) of a motion-aware pass: uint32 per ordered-primitive slot and (n_bodies, 12) Float32, each None when not given — and both None without an id
    plane, since every pixel is static then."""
    table = None if body_of_prim is None or ids is None else np.ascontiguousarray(body_of_prim, dtype=np.uint32).reshape(-1)
    mats = None if bodies is None or ids is None else _ffi.f32(bodies).reshape(-1, 12)
    return table, mats


def _pixel_map(who: str, pixel_map):
    """(ax, bx, ay, by) of Upscaler.pixel_map as four floats; `who` is the class named in the refusal."""
    m = [float(v) for v in pixel_map]
    if len(m) != 4:
        raise TraceHipError(f"{who}: pixel_map must be (ax, bx, ay, by), not {pixel_map!r}")
    return m


# ---- edge-avoiding denoiser (include/tracehip.h, trhip_denoise) ----------------------------------------------------------------------------
class Denoiser:
    """Edge-avoiding à-trous filter (Dammertz et al. 2010, Tukey's biweight as the edge-stopping function) for the film of a PathIntegrator or WhittedIntegrator render,
    guided by the planes of AOVIntegrator for the same camera and sampler (trhip_denoise; docs/design/12-denoise.md).  Fields left at None come from
    trhip_denoise_default_params.  Pixels that are no surface pixels — misses, silhouette pixels with less than min_coverage hit weight, NaNs — are returned untouched.

    `denoise_variance` is the variance-guided filter (trhip_denoise_var; docs/design/16-variance.md): a pixel's colour sigma is `variance_sigma` times the standard deviation
    of its luminance, from a variance plane such as TemporalAccumulator(moments=True) returns, plus `var_eps`; both default to trhip_denoise_var_default_params' and have
    no effect on `denoise`.  Everything else of its parameter block is this denoiser's."""

    def __init__(self, iterations: Optional[int] = None, demodulate: bool = True, sigma_colour: Optional[float] = None, sigma_normal: Optional[float] = None,
                 sigma_plane: Optional[float] = None, albedo_floor: Optional[float] = None, min_coverage: Optional[float] = None, variance_sigma: Optional[float] = None,
                 var_eps: Optional[float] = None):
        p = _ffi.default_params(_ffi.DenoiseParams, "trhip_denoise_default_params")
        for name, value in (("iterations", iterations), ("sigma_colour", sigma_colour), ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane), ("albedo_floor", albedo_floor),
                            ("min_coverage", min_coverage)):
            if value is not None:
                setattr(p, name, value)
        p.flags = _ffi.DENOISE_DEMODULATE if demodulate else 0
        self.params = p
        vp = _ffi.default_params(_ffi.DenoiseVarParams, "trhip_denoise_var_default_params")
        self.variance_sigma = float(vp.base.sigma_colour if variance_sigma is None else variance_sigma)
        self.var_eps = float(vp.var_eps if var_eps is None else var_eps)
        self.stats: Optional[_ffi.Stats] = None
        self.render_stats = None  # (path, aov, denoise) Stats of the last render(); (path, aov, moments, denoise) of a variance-guided one

    def _var_params(self) -> _ffi.DenoiseVarParams:
        vp = _ffi.DenoiseVarParams()
        vp.base = _ffi.DenoiseParams.from_buffer_copy(self.params)
        vp.base.sigma_colour = self.variance_sigma
        vp.var_eps = self.var_eps
        return vp

    def denoise_variance(self, xyzw: np.ndarray, planes: np.ndarray, variance: np.ndarray, ctx: Optional[_ffi.Context] = None):
        """As `denoise`, guided by `variance`, (H, W) as TemporalAccumulator(moments=True).accumulate_moments returns it.  Returns (xyzw, variance of the filtered colour)."""
        xyzw, planes, variance = _ffi.f32(xyzw), _ffi.f32(planes), _ffi.f32(variance)
        if xyzw.ndim != 3 or xyzw.shape[2] != 4 or planes.shape != xyzw.shape[:2] + (3, 4) or variance.shape != xyzw.shape[:2]:
            raise TraceHipError(f"denoise_variance: xyzw must be (H, W, 4), planes (H, W, 3, 4) and variance (H, W), not {xyzw.shape}, {planes.shape} and {variance.shape}")
        ctx = ctx or _ffi.default_context()
        h, w = xyzw.shape[:2]
        out, out_var, st, vp = np.empty_like(xyzw), np.empty_like(variance), _ffi.Stats(), self._var_params()
        ctx.check(_ffi.lib().trhip_denoise_var(ctx._h, _ffi.fptr(xyzw), _ffi.fptr(planes), _ffi.fptr(variance), w, h, C.byref(vp), _ffi.fptr(out), _ffi.fptr(out_var), C.byref(st)))
        self.stats = st
        return out, out_var

    def denoise_variance_device(self, d_xyzw: int, d_planes: int, d_variance: int, width: int, height: int, d_out: int, d_out_variance: Optional[int] = None,
                                ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out may equal d_xyzw, d_out_variance may equal d_variance or be None); nothing is copied to the host."""
        ctx = ctx or _ffi.default_context()
        st, vp = _ffi.Stats(), self._var_params()
        ctx.check(_ffi.lib().trhip_denoise_var_device(ctx._h, C.c_void_p(d_xyzw), C.c_void_p(d_planes), C.c_void_p(d_variance), int(width), int(height), C.byref(vp), C.c_void_p(d_out),
                                                      _ffi.dptr(d_out_variance), C.byref(st)))
        self.stats = st

    def denoise(self, xyzw: np.ndarray, planes: np.ndarray, ctx: Optional[_ffi.Context] = None) -> np.ndarray:
        """xyzw: (H, W, 4) as PathIntegrator.render returns it; planes: (H, W, 3, 4) as AOVIntegrator.render(...).planes.  Returns the denoised (H, W, 4)."""
        xyzw, planes = _film_and_planes("denoise", xyzw, planes)
        ctx = ctx or _ffi.default_context()
        h, w = xyzw.shape[:2]
        out, st = np.empty_like(xyzw), _ffi.Stats()
        ctx.check(_ffi.lib().trhip_denoise(ctx._h, _ffi.fptr(xyzw), _ffi.fptr(planes), w, h, C.byref(self.params), _ffi.fptr(out), C.byref(st)))
        self.stats = st
        return out

    def denoise_device(self, d_xyzw: int, d_planes: int, width: int, height: int, d_out: int, ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out may equal d_xyzw); nothing is copied to the host."""
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        ctx.check(_ffi.lib().trhip_denoise_device(ctx._h, C.c_void_p(d_xyzw), C.c_void_p(d_planes), int(width), int(height), C.byref(self.params), C.c_void_p(d_out), C.byref(st)))
        self.stats = st

    def render(self, scene: Scene, camera: PerspectiveCamera, sampler: SeededSampler, max_depth: int, ctx: Optional[_ffi.Context] = None, variance_guided: bool = False) -> np.ndarray:
        """Path frame and feature planes with the same sampler settings, both left on the device, denoised there; returns xyzw (H, W, 4), ready for film.set_xyzw / save.
        `variance_guided`: the frame's own bits through `denoise_variance`, guided by the spatial variance estimate of TemporalAccumulator(moments=True) without history."""
        ctx = scene.flatten(ctx).ctx
        h, w = camera.film.size
        if variance_guided:
            return self._render_variance_guided(scene, camera, sampler, max_depth, ctx, h, w)
        d_film, d_planes = _ffi.DeviceBuffer(h * w * 16), _ffi.DeviceBuffer(h * w * 48)
        try:
            path, aov = PathIntegrator(camera, sampler, max_depth), AOVIntegrator(camera, sampler)
            path.render(scene, ctx, device_out=d_film.ptr)
            aov.render(scene, ctx, device_out=d_planes.ptr)
            self.denoise_device(d_film.ptr, d_planes.ptr, w, h, d_film.ptr, ctx)
            self.render_stats = (path.stats, aov.stats, self.stats)
            return d_film.to_host(np.float32, (h, w, 4))
        finally:
            d_film.free()
            d_planes.free()

    def _render_variance_guided(self, scene, camera, sampler, max_depth, ctx, h, w) -> np.ndarray:
        bufs = [_ffi.DeviceBuffer(h * w * n) for n in (16, 48, 16, 48, 8, 4)]
        d_film, d_planes, d_acc, d_hist, d_mom, d_var = bufs
        try:
            path, aov = PathIntegrator(camera, sampler, max_depth), AOVIntegrator(camera, sampler)
            path.render(scene, ctx, device_out=d_film.ptr)
            aov.render(scene, ctx, device_out=d_planes.ptr)
            t = TemporalAccumulator(sigma_normal=self.params.sigma_normal, sigma_plane=self.params.sigma_plane, min_coverage=self.params.min_coverage, moments=True,
                                    demodulate=bool(self.params.flags & _ffi.DENOISE_DEMODULATE), albedo_floor=self.params.albedo_floor)
            t.accumulate_moments_device(d_film.ptr, d_planes.ptr, None, None, w, h, None, d_acc.ptr, d_hist.ptr, d_mom.ptr, d_var.ptr, ctx)
            self.denoise_variance_device(d_film.ptr, d_planes.ptr, d_var.ptr, w, h, d_film.ptr, None, ctx)
            self.render_stats = (path.stats, aov.stats, t.stats, self.stats)
            return d_film.to_host(np.float32, (h, w, 4))
        finally:
            for b in bufs:
                b.free()


# ---- edge-aware upscaling (include/tracehip.h, trhip_upscale) ----------------------------------------------------------------------------------
class Upscaler:
    """Joint bilateral upsampling of a low-resolution path film onto the feature planes of the full-size sensor (trhip_upscale; docs/design/17-upscale.md): the path frame
    is traced at 1 / factor of the resolution per axis, the cheap first-hit planes at both sizes, and the full-size film is reconstructed with the denoiser's normal and
    plane-distance edge tests.  Fields left at None come from trhip_upscale_default_params.  `upscale` returns (xyzw, mask): mask 1 guided, 2 unguided (no surface
    pixel), 3 orphan (a full-size surface no low pixel agreed with: filled bilinearly, the caller's to re-render), 0 nothing."""

    def __init__(self, radius: Optional[int] = None, demodulate: Optional[bool] = None, coverage: Optional[bool] = None, sigma_normal: Optional[float] = None, sigma_plane: Optional[float] = None,
                 albedo_floor: Optional[float] = None, min_coverage: Optional[float] = None):
        p = _ffi.default_params(_ffi.UpscaleParams, "trhip_upscale_default_params")
        if radius is not None:
            if int(radius) != radius or not 0 <= radius < 2 ** 32:
                raise TraceHipError(f"Upscaler: radius must be 1 or 2, not {radius!r}")
            p.radius = int(radius)
        for name, value in (("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane), ("albedo_floor", albedo_floor), ("min_coverage", min_coverage)):
            if value is not None:
                setattr(p, name, value)
        for flag, value in ((_ffi.UPSCALE_DEMODULATE, demodulate), (_ffi.UPSCALE_COVERAGE, coverage)):
            if value is not None:
                p.flags = (p.flags | flag) if value else (p.flags & ~flag)
        self.params = p
        self.stats: Optional[_ffi.Stats] = None
        self.render_stats = None  # (path, low planes, full planes, denoise or None, upscale) Stats of the last render()

    @staticmethod
    def pixel_map(hi_camera: PerspectiveCamera, lo_camera: PerspectiveCamera):
        """(ax, bx, ay, by) of trhip_upscale_params.lo_from_hi for two films of one camera: array pixel x of the full-size film lies at x * ax + bx in the low film's array
        coordinates.  Film pixel X (1-based) has its centre at raster position X + 0.5 and array index X - crop_min (docs/design/14-temporal.md); the two rasters share the
        optical axis, which pierces them at o = -m03 / m00 of raster_to_camera (y: -m13 / m11), and differ by the ratio of the resolutions about it:
        ax = res_lo.x / res_hi.x, bx = (crop_min_hi.x + 0.5 - o_hi.x) * ax + o_lo.x - 0.5 - crop_min_lo.x.  Float64, rounded once (docs/design/17-upscale.md derives it)."""
        out = []
        for k in (0, 1):
            o = []
            for cam in (hi_camera, lo_camera):
                m = np.asarray(cam.raster_to_camera.m, np.float64)
                if m[k, 1 - k] != 0.0 or m[k, k] == 0.0:
                    raise TraceHipError("Upscaler.pixel_map: raster_to_camera must be axis-aligned (maps that are not axis-aligned affine are out of scope)")
                o.append(-m[k, 3] / m[k, k])
            a = float(lo_camera.film.resolution[k]) / float(hi_camera.film.resolution[k])
            b = (float(hi_camera.film.crop_bounds.p_min[k]) + 0.5 - o[0]) * a + o[1] - 0.5 - float(lo_camera.film.crop_bounds.p_min[k])
            out += [float(np.float32(a)), float(np.float32(b))]
        return tuple(out)

    @staticmethod
    def low_camera(camera: PerspectiveCamera, factor, jitter=(0.0, 0.0)) -> PerspectiveCamera:
        """`camera` at 1 / factor of its resolution per axis (rounded to whole pixels, at least one).  `jitter` = (jx, jy), in LOW-pixel units, is defined by its effect:
        pixel_map(camera, low_camera(camera, factor, jitter)) is the unjittered map with bx + jx and by + jy.  The optical axis pierces every raster of these cameras at
        (-screen_window.p_min.x, -screen_window.p_max.y) raster pixels, whatever the resolution (docs/design/17-upscale.md), so the jittered camera is the same camera with
        both corners of its screen window moved by (-jx, -jy): the extent, hence the field of view, stays (docs/design/19-temporal-upsample.md)."""
        if not 1.0 <= float(factor) <= 4.0:
            raise TraceHipError(f"Upscaler: factor must lie in [1, 4], not {factor!r}")
        res = [max(1, int(round(float(r) / float(factor)))) for r in camera.film.resolution]
        lo = camera.with_resolution(res)
        jx, jy = (float(v) for v in jitter)
        if jx == 0.0 and jy == 0.0:
            return lo
        if not (math.isfinite(jx) and math.isfinite(jy)):
            raise TraceHipError(f"Upscaler.low_camera: jitter must be finite, not {jitter!r}")
        sw = camera.screen_window
        window = Bounds2([f32(sw.p_min[0]) - f32(jx), f32(sw.p_min[1]) - f32(jy)], [f32(sw.p_max[0]) - f32(jx), f32(sw.p_max[1]) - f32(jy)])
        return PerspectiveCamera(lo.camera_to_world, window, lo.shutter_open, lo.shutter_close, lo.lens_radius, lo.focal_distance, lo.fov, lo.film)

    def _params_for(self, pixel_map) -> _ffi.UpscaleParams:
        p = _ffi.UpscaleParams.from_buffer_copy(self.params)
        p.lo_from_hi[:] = _pixel_map("Upscaler", pixel_map)
        return p

    def upscale(self, lo_xyzw: np.ndarray, lo_planes: np.ndarray, hi_planes: np.ndarray, pixel_map, ctx: Optional[_ffi.Context] = None):
        """lo_xyzw (h, w, 4) and lo_planes (h, w, 3, 4) of the low-resolution camera, hi_planes (H, W, 3, 4) of the full-size one, pixel_map as `pixel_map` returns it.
        Returns (xyzw (H, W, 4), mask (H, W) uint8)."""
        lo_xyzw, lo_planes, hi_planes = _low_and_high("upscale", lo_xyzw, lo_planes, hi_planes)
        p = self._params_for(pixel_map)
        ctx = ctx or _ffi.default_context()
        (lh, lw), (h, w) = lo_xyzw.shape[:2], hi_planes.shape[:2]
        out, mask, st = np.empty((h, w, 4), np.float32), np.empty((h, w), np.uint8), _ffi.Stats()
        ctx.check(_ffi.lib().trhip_upscale(ctx._h, _ffi.fptr(lo_xyzw), _ffi.fptr(lo_planes), lw, lh, _ffi.fptr(hi_planes), w, h, C.byref(p), _ffi.fptr(out),
                                           mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)))
        self.stats = st
        return out, mask

    def upscale_device(self, d_lo_xyzw: int, d_lo_planes: int, lo_width: int, lo_height: int, d_hi_planes: int, width: int, height: int, pixel_map, d_out: int,
                       d_out_mask: Optional[int] = None, ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out_mask may be None); nothing is copied to the host."""
        p = self._params_for(pixel_map)
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        ctx.check(_ffi.lib().trhip_upscale_device(ctx._h, C.c_void_p(d_lo_xyzw), C.c_void_p(d_lo_planes), int(lo_width), int(lo_height), C.c_void_p(d_hi_planes), int(width), int(height),
                                                  C.byref(p), C.c_void_p(d_out), _ffi.dptr(d_out_mask), C.byref(st)))
        self.stats = st

    def render(self, scene: Scene, camera: PerspectiveCamera, sampler: SeededSampler, max_depth: int, factor=2, guide_spp: Optional[int] = None,
               denoiser: Optional["Denoiser"] = None, denoise_at: Optional[str] = "high", ctx: Optional[_ffi.Context] = None, want_mask: bool = False):
        """The one-shot frame, everything on the device: the path frame and its planes through `camera` at 1 / factor of the resolution with `sampler`, the full-size planes
        with `guide_spp` samples per pixel (default: the sampler's; same seed and offset), `denoiser` on the upscaled frame with the full-size planes (denoise_at "high", the
        default: it measured better in every swept cell, profiles/r14/upscale.txt), on the low frame ("low") or not at all (None, or no denoiser).  Returns xyzw (H, W, 4), ready for film.set_xyzw / save; with want_mask (xyzw, mask)."""
        if denoise_at not in ("low", "high", None):
            raise TraceHipError(f"Upscaler.render: denoise_at must be 'low', 'high' or None, not {denoise_at!r}")
        ctx = scene.flatten(ctx).ctx
        lo_cam = self.low_camera(camera, factor)
        (h, w), (lh, lw) = camera.film.size, lo_cam.film.size
        guide = SeededSampler(sampler.samples_per_pixel if guide_spp is None else int(guide_spp), seed=sampler.seed, sample_offset=sampler.sample_offset)
        bufs = [_ffi.DeviceBuffer(n) for n in (lh * lw * 16, lh * lw * 48, h * w * 48, h * w * 16, h * w)]
        d_lo, d_lo_planes, d_hi_planes, d_out, d_mask = bufs
        try:
            path, aov_lo, aov_hi = PathIntegrator(lo_cam, sampler, max_depth), AOVIntegrator(lo_cam, sampler), AOVIntegrator(camera, guide)
            path.render(scene, ctx, device_out=d_lo.ptr)
            aov_lo.render(scene, ctx, device_out=d_lo_planes.ptr)
            aov_hi.render(scene, ctx, device_out=d_hi_planes.ptr)
            dn_stats = None
            if denoiser is not None and denoise_at == "low":
                denoiser.denoise_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_lo.ptr, ctx)
                dn_stats = denoiser.stats
            self.upscale_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_hi_planes.ptr, w, h, self.pixel_map(camera, lo_cam), d_out.ptr, d_mask.ptr if want_mask else None, ctx)
            if denoiser is not None and denoise_at == "high":
                denoiser.denoise_device(d_out.ptr, d_hi_planes.ptr, w, h, d_out.ptr, ctx)
                dn_stats = denoiser.stats
            self.render_stats = (path.stats, aov_lo.stats, aov_hi.stats, dn_stats, self.stats)
            out = d_out.to_host(np.float32, (h, w, 4))
            return (out, d_mask.to_host(np.uint8, (h, w))) if want_mask else out
        finally:
            for b in bufs:
                b.free()


# ---- display pass (include/tracehip.h, trhip_display) ---------------------------------------------------------------------------------------
class Display:
    """The last stage of a preview, on the device: meter the film's luminance, expose, apply a tone curve and encode to 8-bit RGBA (trhip_display;
    docs/design/18-display.md).  curve "clamp" | "reinhard" | "aces", transfer "linear" | "srgb" (or the header's numbers); `percentile` in (0, 1] is the metered quantile that
    is mapped to `key`.  Fields left at None come from trhip_display_default_params.  `state` is the 16-byte exposure state carried from frame to frame: a
    _ffi.DisplayState for `encode` (host), a device address for `encode_device`."""

    def __init__(self, curve=None, transfer=None, auto_exposure: Optional[bool] = None, flip_rows: Optional[bool] = None, exposure: Optional[float] = None, key: Optional[float] = None,
                 percentile: Optional[float] = None, adapt_rate: Optional[float] = None, min_exposure: Optional[float] = None, max_exposure: Optional[float] = None,
                 white: Optional[float] = None):
        p = _ffi.default_params(_ffi.DisplayParams, "trhip_display_default_params")
        for name, value, names in (("curve", curve, _ffi.DISPLAY_CURVES), ("transfer", transfer, _ffi.DISPLAY_TRANSFERS)):
            if value is not None:
                number = names.get(value.lower()) if isinstance(value, str) else value
                if number is None or int(number) != number or not 0 <= number < 2 ** 32:
                    raise TraceHipError(f"Display: {name} must be one of {sorted(names)}, not {value!r}")
                setattr(p, name, int(number))
        if percentile is not None:
            permille = int(round(float(percentile) * 1000.0)) if math.isfinite(percentile) else -1
            if not 0 <= permille < 2 ** 32:
                raise TraceHipError(f"Display: percentile must lie in (0, 1], not {percentile!r}")
            p.percentile_permille = permille
        for name, value in (("exposure", exposure), ("key", key), ("adapt_rate", adapt_rate), ("min_exposure", min_exposure), ("max_exposure", max_exposure), ("white", white)):
            if value is not None:
                setattr(p, name, value)
        for flag, value in ((_ffi.DISPLAY_AUTO_EXPOSURE, auto_exposure), (_ffi.DISPLAY_FLIP_ROWS, flip_rows)):
            if value is not None:
                p.flags = (p.flags | flag) if value else (p.flags & ~flag)
        self.params = p
        self.stats: Optional[_ffi.Stats] = None

    @staticmethod
    def reference() -> "Display":
        """The look of `save`: linear clamp, no transfer function, exposure 1, rows flipped.  Its RGB bytes are the ones save(film) writes for every pixel free of NaN."""
        return Display(curve="clamp", transfer="linear", auto_exposure=False, flip_rows=True, exposure=1.0)

    @staticmethod
    def srgb_table() -> np.ndarray:
        """(256,) Float32: [0] = 0, [k] = T[k], the sRGB encode's thresholds (trhip_display_srgb_table; no GPU)."""
        out = np.empty(256, np.float32)
        rc = _ffi.lib().trhip_display_srgb_table(_ffi.fptr(out))
        if rc:
            raise TraceHipError(f"trhip_display_srgb_table failed ({rc})")
        return out

    def encode(self, xyzw: np.ndarray, scale=1.0, state: Optional[_ffi.DisplayState] = None, ctx: Optional[_ffi.Context] = None, want_histogram: bool = False):
        """xyzw (H, W, 4) -> uint8 (H, W, 4).  With a `state` (a _ffi.DisplayState; DisplayState() = none yet) returns (rgba, state), the state a new object; with
        want_histogram (rgba, state, histogram (256,) uint32), the state None when none was given."""
        xyzw = _ffi.f32(xyzw)
        if xyzw.ndim != 3 or xyzw.shape[2] != 4:
            raise TraceHipError(f"Display.encode: xyzw must be (H, W, 4), not {xyzw.shape}")
        ctx = ctx or _ffi.default_context()
        h, w = xyzw.shape[:2]
        out, st = np.empty((h, w, 4), np.uint8), _ffi.Stats()
        hist = np.empty(256, np.uint32) if want_histogram else None
        new_state = _ffi.DisplayState.from_buffer_copy(state) if state is not None else None
        ctx.check(_ffi.lib().trhip_display(ctx._h, _ffi.fptr(xyzw), w, h, float(scale), C.byref(self.params), C.byref(new_state) if new_state is not None else None,
                                           out.ctypes.data_as(C.POINTER(C.c_uint8)), _ffi.optr(hist), C.byref(st)))
        self.stats = st
        if want_histogram:
            return out, new_state, hist
        return (out, new_state) if state is not None else out

    def encode_device(self, d_xyzw: int, width: int, height: int, scale, d_out_rgba: int, d_state: Optional[int] = None, d_histogram: Optional[int] = None,
                      ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers: d_out_rgba height * width * 4 bytes, d_state 16 bytes (zeroed = no state yet) or None, d_histogram 1024 bytes or None; nothing is
        copied to the host."""
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        ctx.check(_ffi.lib().trhip_display_device(ctx._h, C.c_void_p(d_xyzw), int(width), int(height), float(scale), C.byref(self.params), _ffi.dptr(d_state),
                                                  C.c_void_p(d_out_rgba), _ffi.dptr(d_histogram), C.byref(st)))
        self.stats = st

    def save(self, film: "Film", ctx: Optional[_ffi.Context] = None) -> str:
        """Writes film.filename (8-bit PNG) through the pass: the rows come out in the order the parameters say (flipped by default, as `save` writes them) and the bytes are
        the device's; nothing is flipped or rounded on the host."""
        from PIL import Image
        xyzw = np.concatenate([film.xyz, film.filter_weight_sum[..., None]], axis=-1)
        rgba = self.encode(xyzw, film.scale, ctx=ctx)
        Image.fromarray(np.ascontiguousarray(rgba[..., :3]), "RGB").save(film.filename)
        return film.filename


# ---- temporal reprojection (include/tracehip.h, trhip_temporal) ------------------------------------------------------------------------------
class TemporalAccumulator:
    """Blends a path frame with the previous frame's accumulated colour, fetched through the previous camera and validated against the feature planes (trhip_temporal;
    docs/design/14-temporal.md).  Fields left at None come from trhip_temporal_default_params (max_history 8, sigma_normal 0.25, sigma_plane 0.1, min_coverage 0.5).
    The history is a (H, W, 3, 4) array: (c.rgb, N), (n, surface flag), (p, 0).  Scenes are static and lighting changes are not detected: pass history=None after one.

    `clip_gamma` / `clip_radius`: with either given, the reprojected history colour is first confined to mean +- clip_gamma * sd of the new frame's colours in a window of
    (2 clip_radius + 1)^2 pixels (trhip_temporal_clip; docs/design/15-temporal-clip.md), the other coming from trhip_temporal_clip_default_params; a history that no longer
    fits the frame, as after a change of lights, is then cut back within a frame.  clip_gamma = inf gives the unclipped result bit for bit.  With both None nothing changes:
    `params` is a TemporalParams and the calls go through trhip_temporal.

    `moments=True`: `accumulate_moments` / `accumulate_moments_device` also carry the two luminance moments along the reprojection and return a variance plane for
    Denoiser.denoise_variance (trhip_temporal_moments; docs/design/16-variance.md); their colour and history are `accumulate`'s bit for bit.  `spatial_below`, `albedo_floor`
    left at None come from trhip_temporal_moments_default_params; `demodulate` must be the denoiser's.  Not combinable with clipping: a clipped moments pass does not exist.

    `accumulate_motion` / `accumulate_motion_device` (a plain accumulator only): `accumulate` for a scene whose rigid bodies moved between the frames — with the frame's id
    plane, a body per primitive and a prev_from_cur matrix per body each pixel's surface is carried back to where its body was before the history is looked up
    (trhip_temporal_motion; docs/design/20-motion.md).  The history arrays are `accumulate`'s; with no table and no matrices the result is `accumulate`'s bit for bit.

    `carry_bodies=True` (needs `clip_gamma`): the clipping accumulator whose every call goes through trhip_temporal_clip_motion (docs/design/21-clip-motion.md) —
    `accumulate` / `accumulate_device` without an id plane (every pixel static), `accumulate_motion` / `accumulate_motion_device` with the tables —, so that a moving body
    keeps its history AND the shadow it drags over static surfaces is cut back to the new frame's colours.  `clip_max_history` (default:
    trhip_temporal_clip_motion_default_params'): a pixel whose history colour was clipped has its history length cut to this before the blend; inf never cuts it, and with
    inf and no moving pixel the result is the clipping accumulator's bit for bit.  Not combinable with moments=True: a moments pass that carries bodies does not exist.

    `accumulate_split` / `accumulate_split_device` (a plain accumulator only): `accumulate_motion` on the film minus a direct film, so that the history holds the indirect
    light alone (trhip_temporal_split; docs/design/23-direct-split.md).  With direct=None the result is `accumulate_motion`'s bit for bit."""

    def __init__(self, max_history: Optional[float] = None, sigma_normal: Optional[float] = None, sigma_plane: Optional[float] = None, min_coverage: Optional[float] = None,
                 clip_gamma: Optional[float] = None, clip_radius: Optional[int] = None, moments: bool = False, spatial_below: Optional[float] = None, demodulate: bool = True,
                 albedo_floor: Optional[float] = None, carry_bodies: bool = False, clip_max_history: Optional[float] = None):
        self.clip_params: Optional[_ffi.TemporalClipParams] = None
        self.moments_params: Optional[_ffi.TemporalMomentsParams] = None
        self.clip_motion_params: Optional[_ffi.TemporalClipMotionParams] = None
        if carry_bodies and moments:
            raise TraceHipError("TemporalAccumulator: moments=True cannot be combined with carry_bodies=True (trhip_temporal_moments does not carry bodies back)")
        if carry_bodies and clip_gamma is None:
            raise TraceHipError("TemporalAccumulator: carry_bodies=True needs clip_gamma (it selects trhip_temporal_clip_motion; without clipping, accumulate_motion of a "
                                "plain accumulator carries the bodies)")
        if clip_max_history is not None and not carry_bodies:
            raise TraceHipError("TemporalAccumulator: clip_max_history belongs to carry_bodies=True (trhip_temporal_clip_motion alone shortens the history)")
        if moments and (clip_gamma is not None or clip_radius is not None):
            raise TraceHipError("TemporalAccumulator: moments=True cannot be combined with clip_gamma / clip_radius (there is no clipped variant of trhip_temporal_moments)")
        if not moments and (spatial_below is not None or albedo_floor is not None):
            raise TraceHipError("TemporalAccumulator: spatial_below and albedo_floor belong to moments=True")
        if moments:
            mp = _ffi.default_params(_ffi.TemporalMomentsParams, "trhip_temporal_moments_default_params")
            if spatial_below is not None:
                mp.spatial_below = spatial_below
            if albedo_floor is not None:
                mp.albedo_floor = albedo_floor
            mp.flags = _ffi.DENOISE_DEMODULATE if demodulate else 0
            self.moments_params, p = mp, mp.base  # a view, as below
        elif clip_gamma is None and clip_radius is None:
            p = _ffi.default_params(_ffi.TemporalParams, "trhip_temporal_default_params")
        else:
            cp = _ffi.default_params(_ffi.TemporalClipParams, "trhip_temporal_clip_default_params")
            if clip_gamma is not None:
                cp.clip_gamma = clip_gamma
            if clip_radius is not None:
                if int(clip_radius) != clip_radius or not 0 <= clip_radius < 2 ** 32:
                    raise TraceHipError(f"TemporalAccumulator: clip_radius must be 1, 2 or 3, not {clip_radius!r}")
                cp.clip_radius = int(clip_radius)
            self.clip_params, p = cp, cp.base  # p is a view of cp.base: the fields set below land in the block that is passed
            if carry_bodies:
                cm = _ffi.default_params(_ffi.TemporalClipMotionParams, "trhip_temporal_clip_motion_default_params")
                if clip_max_history is not None:
                    cm.clip_max_history = clip_max_history
                self.clip_motion_params = cm  # gamma, radius and the base are taken from clip_params / params when a call is made
        for name, value in (("max_history", max_history), ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane), ("min_coverage", min_coverage)):
            if value is not None:
                setattr(p, name, value)
        self.params = p
        self.stats: Optional[_ffi.Stats] = None

    def _params_for(self, prev_camera) -> _ffi.TemporalParams:
        """`prev_camera`: the previous frame's PerspectiveCamera, its world_to_pixel() matrix, or None (zeros: nothing is found through it)."""
        p = _ffi.TemporalParams.from_buffer_copy(self.params)
        if prev_camera is not None:
            m = prev_camera.world_to_pixel() if hasattr(prev_camera, "world_to_pixel") else _ffi.f32(prev_camera)
            if m.size != 12:
                raise TraceHipError(f"TemporalAccumulator: the previous camera's matrix must be 3 x 4, not {m.shape}")
            p.prev_world_to_pixel[:] = m.reshape(-1).tolist()
        return p

    def _clip_params_for(self, prev_camera) -> _ffi.TemporalClipParams:
        cp = _ffi.TemporalClipParams.from_buffer_copy(self.clip_params)
        cp.base = self._params_for(prev_camera)
        return cp

    def _clip_motion_params_for(self, prev_camera, n_prims: int, n_bodies: int) -> _ffi.TemporalClipMotionParams:
        base, cm = self._params_for(prev_camera), _ffi.TemporalClipMotionParams.from_buffer_copy(self.clip_motion_params)
        mp = cm.base
        mp.prev_world_to_pixel[:] = list(base.prev_world_to_pixel)
        mp.max_history, mp.sigma_normal, mp.sigma_plane, mp.min_coverage = base.max_history, base.sigma_normal, base.sigma_plane, base.min_coverage
        mp.n_prims, mp.n_bodies = int(n_prims), int(n_bodies)
        cm.clip_gamma, cm.clip_radius = self.clip_params.clip_gamma, self.clip_params.clip_radius
        return cm

    def _moments_params_for(self, prev_camera) -> _ffi.TemporalMomentsParams:
        if self.moments_params is None:
            raise TraceHipError("TemporalAccumulator: accumulate_moments needs TemporalAccumulator(moments=True)")
        mp = _ffi.TemporalMomentsParams.from_buffer_copy(self.moments_params)
        mp.base = self._params_for(prev_camera)
        return mp

    def _motion_params_for(self, prev_camera, n_prims: int, n_bodies: int) -> _ffi.TemporalMotionParams:
        if self.clip_params is not None or self.moments_params is not None:
            raise TraceHipError("TemporalAccumulator: accumulate_motion needs a plain accumulator, or a clipping one built with carry_bodies=True (there is no moments "
                                "variant of trhip_temporal_motion, and a clipping accumulator without carry_bodies goes through trhip_temporal_clip)")
        base, mp = self._params_for(prev_camera), _ffi.TemporalMotionParams()
        mp.prev_world_to_pixel[:] = list(base.prev_world_to_pixel)
        mp.max_history, mp.sigma_normal, mp.sigma_plane, mp.min_coverage = base.max_history, base.sigma_normal, base.sigma_plane, base.min_coverage
        mp.n_prims, mp.n_bodies = int(n_prims), int(n_bodies)
        return mp

    def _split_params_for(self, prev_camera, n_prims: int, n_bodies: int) -> _ffi.TemporalMotionParams:
        if self.clip_params is not None or self.moments_params is not None:
            raise TraceHipError("TemporalAccumulator: accumulate_split needs a plain accumulator (trhip_temporal_split neither clips nor carries moments)")
        return self._motion_params_for(prev_camera, n_prims, n_bodies)

    @staticmethod
    def prev_from_cur(motion) -> np.ndarray:
        """The (3, 4) Float32 matrix trhip_temporal_motion wants for a body that `motion` (a Transformation) carried from the previous frame's pose to this one: the first
        three rows of its inv_m, each entry rounded to Float32 once."""
        return np.ascontiguousarray(np.asarray(motion.inv_m, np.float64)[:3, :4], dtype=np.float32)

    # The calls.  Five entries serve the colour passes, their argument lists extensions of one another: trhip_temporal and trhip_temporal_clip take (film, planes, history);
    # trhip_temporal_motion and trhip_temporal_clip_motion the id plane, the body table and the body matrices after them; trhip_temporal_split those and the direct film
    # after the film.  Each public method names its entry; _accumulate / _accumulate_device make the call.
    def _accumulate_entry(self) -> str:
        """What accumulate / accumulate_device call: with carry_bodies trhip_temporal_clip_motion (no id plane: every pixel static), with clipping trhip_temporal_clip."""
        if self.clip_motion_params is not None:
            return "trhip_temporal_clip_motion"
        return "trhip_temporal_clip" if self.clip_params is not None else "trhip_temporal"

    def _motion_entry(self) -> str:
        """What accumulate_motion / accumulate_motion_device call."""
        return "trhip_temporal_clip_motion" if self.clip_motion_params is not None else "trhip_temporal_motion"

    def _block_for(self, entry: str, prev_camera, n_prims: int, n_bodies: int):
        """The parameter block `entry` takes (and the refusal of an accumulator of the wrong kind)."""
        if entry == "trhip_temporal":
            return self._params_for(prev_camera)
        if entry == "trhip_temporal_clip":
            return self._clip_params_for(prev_camera)
        if entry == "trhip_temporal_clip_motion":
            return self._clip_motion_params_for(prev_camera, n_prims, n_bodies)
        if entry == "trhip_temporal_split":
            return self._split_params_for(prev_camera, n_prims, n_bodies)
        return self._motion_params_for(prev_camera, n_prims, n_bodies)

    def _accumulate(self, who: str, entry: str, xyzw, direct, planes, history, ids, body_of_prim, bodies, prev_camera, ctx):
        """The host call of accumulate, accumulate_motion and accumulate_split (`who`, for the refusals) through `entry`: (xyzw, history) of this frame."""
        xyzw, planes = _film_and_planes(who, xyzw, planes)
        if direct is not None:
            direct = _ffi.f32(direct)
            if direct.shape != xyzw.shape:
                raise TraceHipError(f"{who}: direct must be {xyzw.shape} like xyzw, not {direct.shape}")
        history = _history_like(who, history, planes)
        h, w = xyzw.shape[:2]
        if ids is not None or entry == "trhip_temporal_motion":  # the one entry whose id plane is not optional
            ids = _id_plane(who, ids, h, w)
        table, mats = _body_tables(ids, body_of_prim, bodies)
        p = self._block_for(entry, prev_camera, 0 if table is None else table.size, 0 if mats is None else mats.shape[0])
        ctx = ctx or _ffi.default_context()
        out, out_history, st = np.empty_like(xyzw), np.empty_like(planes), _ffi.Stats()
        args = [_ffi.fptr(xyzw)] + ([_ffi.optr(direct)] if entry == "trhip_temporal_split" else []) + [_ffi.fptr(planes), _ffi.optr(history)]
        if entry not in ("trhip_temporal", "trhip_temporal_clip"):
            args += [_ffi.optr(ids), _ffi.optr(table), _ffi.optr(mats)]
        ctx.check(getattr(_ffi.lib(), entry)(ctx._h, *args, w, h, C.byref(p), _ffi.fptr(out), _ffi.fptr(out_history), C.byref(st)))
        self.stats = st
        return out, out_history

    def _accumulate_device(self, entry: str, d_xyzw, d_direct, d_planes, d_history, d_ids, d_body_of_prim, n_prims, d_bodies, n_bodies, width, height, prev_camera, d_out,
                           d_out_history, ctx) -> None:
        """The same through `entry`_device, on device pointers; a table that is not given counts no entries."""
        p = self._block_for(entry, prev_camera, n_prims if d_body_of_prim else 0, n_bodies if d_bodies else 0)
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        args = [C.c_void_p(d_xyzw)] + ([_ffi.dptr(d_direct)] if entry == "trhip_temporal_split" else []) + [C.c_void_p(d_planes), _ffi.dptr(d_history)]
        if entry not in ("trhip_temporal", "trhip_temporal_clip"):
            args += [_ffi.dptr(d_ids), _ffi.dptr(d_body_of_prim), _ffi.dptr(d_bodies)]
        ctx.check(getattr(_ffi.lib(), entry + "_device")(ctx._h, *args, int(width), int(height), C.byref(p), C.c_void_p(d_out), C.c_void_p(d_out_history), C.byref(st)))
        self.stats = st

    def accumulate(self, xyzw: np.ndarray, planes: np.ndarray, history: Optional[np.ndarray], prev_camera, ctx: Optional[_ffi.Context] = None):
        """xyzw: (H, W, 4) as PathIntegrator.render returns it; planes: (H, W, 3, 4) as AOVIntegrator.render(...).planes; history: the second result of the previous
        frame's call, or None.  Returns (xyzw, history) of this frame; the xyzw goes into Denoiser.denoise with the same planes."""
        return self._accumulate("accumulate", self._accumulate_entry(), xyzw, None, planes, history, None, None, None, prev_camera, ctx)

    def accumulate_device(self, d_xyzw: int, d_planes: int, d_history: Optional[int], width: int, height: int, prev_camera, d_out: int, d_out_history: int,
                          ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out may equal d_xyzw, d_history may be None); nothing is copied to the host."""
        self._accumulate_device(self._accumulate_entry(), d_xyzw, None, d_planes, d_history, None, None, 0, None, 0, width, height, prev_camera, d_out, d_out_history, ctx)

    def accumulate_motion(self, xyzw: np.ndarray, planes: np.ndarray, history: Optional[np.ndarray], ids: np.ndarray, body_of_prim: Optional[np.ndarray],
                          bodies: Optional[np.ndarray], prev_camera, ctx: Optional[_ffi.Context] = None):
        """`accumulate` for a scene with moving rigid bodies (trhip_temporal_motion; docs/design/20-motion.md).  ids: (H, W) of _ffi.AOV_ID_DTYPE, this frame's
        AOVIntegrator.ids; body_of_prim: uint32 per ordered-primitive slot (FlatScene.body_table) or None; bodies: (n_bodies, 3, 4) prev_from_cur matrices or None.
        Returns (xyzw, history) of this frame.  An accumulator built with carry_bodies=True makes the same call through trhip_temporal_clip_motion."""
        return self._accumulate("accumulate_motion", self._motion_entry(), xyzw, None, planes, history, ids, body_of_prim, bodies, prev_camera, ctx)

    def accumulate_motion_device(self, d_xyzw: int, d_planes: int, d_history: Optional[int], d_ids: int, d_body_of_prim: Optional[int], n_prims: int, d_bodies: Optional[int],
                                 n_bodies: int, width: int, height: int, prev_camera, d_out: int, d_out_history: int, ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out may equal d_xyzw; d_history, d_body_of_prim and d_bodies may be None); nothing is copied to the host."""
        self._accumulate_device(self._motion_entry(), d_xyzw, None, d_planes, d_history, d_ids, d_body_of_prim, n_prims, d_bodies, n_bodies, width, height, prev_camera, d_out,
                                d_out_history, ctx)

    def accumulate_split(self, xyzw: np.ndarray, direct: Optional[np.ndarray], planes: np.ndarray, history: Optional[np.ndarray], ids: Optional[np.ndarray],
                         body_of_prim: Optional[np.ndarray], bodies: Optional[np.ndarray], prev_camera, ctx: Optional[_ffi.Context] = None):
        """`accumulate_motion` on xyzw.xyz - direct.xyz (a plain accumulator only; trhip_temporal_split, docs/design/23-direct-split.md): `direct` is the (H, W, 4) film of the
        frame's first-hit direct light, or None (then `accumulate_motion`'s result bit for bit).  ids may be None when there is no table: every pixel is static.  The returned
        film and history hold the indirect remainder; Film.add puts `direct` back after the filter."""
        return self._accumulate("accumulate_split", "trhip_temporal_split", xyzw, direct, planes, history, ids, body_of_prim, bodies, prev_camera, ctx)

    def accumulate_split_device(self, d_xyzw: int, d_direct: Optional[int], d_planes: int, d_history: Optional[int], d_ids: Optional[int], d_body_of_prim: Optional[int], n_prims: int,
                                d_bodies: Optional[int], n_bodies: int, width: int, height: int, prev_camera, d_out: int, d_out_history: int,
                                ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out may equal d_xyzw; d_direct, d_history, d_body_of_prim, d_bodies and, without a table, d_ids may be None); nothing is copied to
        the host."""
        if not d_ids:  # every pixel is static: the tables count no entries
            n_prims = n_bodies = 0
        self._accumulate_device("trhip_temporal_split", d_xyzw, d_direct, d_planes, d_history, d_ids, d_body_of_prim, n_prims, d_bodies, n_bodies, width, height, prev_camera, d_out,
                                d_out_history, ctx)

    def accumulate_moments(self, xyzw: np.ndarray, planes: np.ndarray, history: Optional[np.ndarray], moments: Optional[np.ndarray], prev_camera,
                           ctx: Optional[_ffi.Context] = None):
        """`accumulate` with the moments: `moments` is (H, W, 2), the third result of the previous frame's call, None exactly when `history` is.  Returns (xyzw, history,
        moments, variance (H, W)) of this frame; the variance goes into Denoiser.denoise_variance with the returned xyzw and the same planes."""
        mp = self._moments_params_for(prev_camera)
        xyzw, planes = _film_and_planes("accumulate_moments", xyzw, planes)
        if (history is None) != (moments is None):
            raise TraceHipError("accumulate_moments: moments must be None exactly when history is")
        if history is not None:
            history, moments = _ffi.f32(history), _ffi.f32(moments)
            if history.shape != planes.shape or moments.shape != xyzw.shape[:2] + (2,):
                raise TraceHipError(f"accumulate_moments: history must be {planes.shape} and moments {xyzw.shape[:2] + (2,)}, not {history.shape} and {moments.shape}")
        ctx = ctx or _ffi.default_context()
        h, w = xyzw.shape[:2]
        out, out_history, out_moments, out_var, st = np.empty_like(xyzw), np.empty_like(planes), np.empty((h, w, 2), np.float32), np.empty((h, w), np.float32), _ffi.Stats()
        ctx.check(_ffi.lib().trhip_temporal_moments(ctx._h, _ffi.fptr(xyzw), _ffi.fptr(planes), _ffi.optr(history), _ffi.optr(moments), w, h, C.byref(mp), _ffi.fptr(out),
                                                    _ffi.fptr(out_history), _ffi.fptr(out_moments), _ffi.fptr(out_var), C.byref(st)))
        self.stats = st
        return out, out_history, out_moments, out_var

    def accumulate_moments_device(self, d_xyzw: int, d_planes: int, d_history: Optional[int], d_moments: Optional[int], width: int, height: int, prev_camera, d_out: int,
                                  d_out_history: int, d_out_moments: int, d_out_variance: int, ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_out may equal d_xyzw; d_history and d_moments may both be None); nothing is copied to the host."""
        mp = self._moments_params_for(prev_camera)
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        ctx.check(_ffi.lib().trhip_temporal_moments_device(ctx._h, C.c_void_p(d_xyzw), C.c_void_p(d_planes), _ffi.dptr(d_history), _ffi.dptr(d_moments), int(width), int(height),
                                                           C.byref(mp), C.c_void_p(d_out), C.c_void_p(d_out_history), C.c_void_p(d_out_moments), C.c_void_p(d_out_variance),
                                                           C.byref(st)))
        self.stats = st


# ---- temporal upsampling (include/tracehip.h, trhip_temporal_upsample) -------------------------------------------------------------------------
class TemporalUpsampler:
    """Upscales a jittered low-resolution path film onto the full-size planes and blends it into a full-size history in one pass (trhip_temporal_upsample;
    docs/design/19-temporal-upsample.md): each full-size pixel trusts the new frame in proportion to how directly a low sample observed it.  Fields left at None come from
    trhip_temporal_upsample_default_params.  The history is a (H, W, 3, 4) array in TemporalAccumulator's layout whose word 0 holds (c.rgb, Omega), Omega an accumulated
    weight.  `jitter`: "grid" (factor 2 only: four offsets of a quarter low pixel that put every full-size pixel centre on a low pixel centre once in four frames),
    "halton" (bases 2 and 3, any factor) or None.  `accumulate` returns (xyzw, history, mask): mask is Upscaler's class + 4 where history was found.

    `carry_bodies=True`: every call goes through trhip_temporal_upsample_motion (docs/design/22-upsample-motion.md) — `accumulate` / `accumulate_device` without an id
    plane (every pixel static: trhip_temporal_upsample's bits), `accumulate_motion` / `accumulate_motion_device` with the FULL-SIZE frame's id plane, a body per primitive
    and a prev_from_cur matrix per body, so that a moving body's surface is carried back to where it was before the full-size history is looked up."""

    GRID = ((0.25, 0.25), (-0.25, -0.25), (-0.25, 0.25), (0.25, -0.25))

    def __init__(self, radius: Optional[int] = None, max_history: Optional[float] = None, sigma_normal: Optional[float] = None, sigma_plane: Optional[float] = None,
                 guide_sigma_normal: Optional[float] = None, guide_sigma_plane: Optional[float] = None, confidence_floor: Optional[float] = None,
                 confidence_sharpness: Optional[float] = None, min_coverage: Optional[float] = None, jitter: Optional[str] = "grid", carry_bodies: bool = False):
        if jitter not in ("grid", "halton", None):
            raise TraceHipError(f"TemporalUpsampler: jitter must be 'grid', 'halton' or None, not {jitter!r}")
        p = _ffi.default_params(_ffi.TemporalUpsampleParams, "trhip_temporal_upsample_default_params")
        if radius is not None:
            if int(radius) != radius or not 0 <= radius < 2 ** 32:
                raise TraceHipError(f"TemporalUpsampler: radius must be 1 or 2, not {radius!r}")
            p.radius = int(radius)
        for name, value in (("max_history", max_history), ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane), ("guide_sigma_normal", guide_sigma_normal),
                            ("guide_sigma_plane", guide_sigma_plane), ("confidence_floor", confidence_floor), ("confidence_sharpness", confidence_sharpness),
                            ("min_coverage", min_coverage)):
            if value is not None:
                setattr(p, name, value)
        self.params, self.jitter = p, jitter
        self.carry_bodies = bool(carry_bodies)
        self.stats: Optional[_ffi.Stats] = None

    def jitter_for(self, frame: int, factor=2):
        """(jx, jy) of frame `frame`, in low-pixel units, for Upscaler.low_camera."""
        frame = int(frame)
        if frame < 0:
            raise TraceHipError(f"TemporalUpsampler.jitter_for: frame must be >= 0, not {frame}")
        if self.jitter is None:
            return (0.0, 0.0)
        if self.jitter == "grid":
            if float(factor) != 2.0:
                raise TraceHipError(f"TemporalUpsampler: jitter 'grid' needs factor 2, not {factor!r} (use 'halton')")
            return self.GRID[frame % 4]

        def radical_inverse(base, i):
            f, r = 1.0, 0.0
            while i > 0:
                f /= base
                r += f * (i % base)
                i //= base
            return r
        return (radical_inverse(2, frame + 1) - 0.5, radical_inverse(3, frame + 1) - 0.5)

    def _params_for(self, pixel_map, prev_camera) -> _ffi.TemporalUpsampleParams:
        """`pixel_map`: Upscaler.pixel_map of this frame's cameras; `prev_camera`: the previous frame's FULL-SIZE PerspectiveCamera, its world_to_pixel() matrix, or None."""
        p = _ffi.TemporalUpsampleParams.from_buffer_copy(self.params)
        p.lo_from_hi[:] = _pixel_map("TemporalUpsampler", pixel_map)
        if prev_camera is not None:
            w2p = prev_camera.world_to_pixel() if hasattr(prev_camera, "world_to_pixel") else _ffi.f32(prev_camera)
            if w2p.size != 12:
                raise TraceHipError(f"TemporalUpsampler: the previous camera's matrix must be 3 x 4, not {w2p.shape}")
            p.prev_world_to_pixel[:] = w2p.reshape(-1).tolist()
        return p

    def _require_carry_bodies(self) -> None:
        if not self.carry_bodies:
            raise TraceHipError("TemporalUpsampler: accumulate_motion needs an upsampler built with carry_bodies=True (trhip_temporal_upsample does not carry bodies back)")

    def _motion_params_for(self, pixel_map, prev_camera, n_prims: int, n_bodies: int) -> _ffi.TemporalUpsampleMotionParams:
        self._require_carry_bodies()
        mp = _ffi.TemporalUpsampleMotionParams()
        mp.base = self._params_for(pixel_map, prev_camera)
        mp.n_prims, mp.n_bodies = int(n_prims), int(n_bodies)
        return mp

    # The calls.  trhip_temporal_upsample_motion takes trhip_temporal_upsample's arguments with the id plane, the body table and the body matrices after the history.
    def _accumulate(self, who: str, motion: bool, lo_xyzw, lo_planes, hi_planes, history, ids, body_of_prim, bodies, pixel_map, prev_camera, ctx):
        """The host call of accumulate (trhip_temporal_upsample) and, with `motion`, of accumulate_motion (trhip_temporal_upsample_motion); `who` for the refusals."""
        lo_xyzw, lo_planes, hi_planes = _low_and_high(who, lo_xyzw, lo_planes, hi_planes)
        history = _history_like(who, history, hi_planes, "hi_planes")
        (lh, lw), (h, w) = lo_xyzw.shape[:2], hi_planes.shape[:2]
        if ids is not None:
            ids = _id_plane(who, ids, h, w, "FULL-SIZE pixel")
        table, mats = _body_tables(ids, body_of_prim, bodies)
        if motion:
            entry, p = "trhip_temporal_upsample_motion", self._motion_params_for(pixel_map, prev_camera, 0 if table is None else table.size, 0 if mats is None else mats.shape[0])
            tables = [_ffi.optr(ids), _ffi.optr(table), _ffi.optr(mats)]
        else:
            entry, p, tables = "trhip_temporal_upsample", self._params_for(pixel_map, prev_camera), []
        ctx = ctx or _ffi.default_context()
        out, out_history, mask, st = np.empty((h, w, 4), np.float32), np.empty((h, w, 3, 4), np.float32), np.empty((h, w), np.uint8), _ffi.Stats()
        ctx.check(getattr(_ffi.lib(), entry)(ctx._h, _ffi.fptr(lo_xyzw), _ffi.fptr(lo_planes), lw, lh, _ffi.fptr(hi_planes), _ffi.optr(history), *tables, w, h, C.byref(p),
                                             _ffi.fptr(out), _ffi.fptr(out_history), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)))
        self.stats = st
        return out, out_history, mask

    def _accumulate_device(self, motion: bool, d_lo_xyzw, d_lo_planes, lo_width, lo_height, d_hi_planes, d_history, d_ids, d_body_of_prim, n_prims, d_bodies, n_bodies, width, height,
                           pixel_map, prev_camera, d_out, d_out_history, d_out_mask, ctx) -> None:
        """The same on device pointers; a table that is not given, or any table without an id plane, counts no entries."""
        if motion:
            entry, p = "trhip_temporal_upsample_motion_device", self._motion_params_for(pixel_map, prev_camera, n_prims if d_body_of_prim and d_ids else 0,
                                                                                        n_bodies if d_bodies and d_ids else 0)
            tables = [_ffi.dptr(d_ids), _ffi.dptr(d_body_of_prim), _ffi.dptr(d_bodies)]
        else:
            entry, p, tables = "trhip_temporal_upsample_device", self._params_for(pixel_map, prev_camera), []
        ctx = ctx or _ffi.default_context()
        st = _ffi.Stats()
        ctx.check(getattr(_ffi.lib(), entry)(ctx._h, C.c_void_p(d_lo_xyzw), C.c_void_p(d_lo_planes), int(lo_width), int(lo_height), C.c_void_p(d_hi_planes), _ffi.dptr(d_history),
                                             *tables, int(width), int(height), C.byref(p), C.c_void_p(d_out), C.c_void_p(d_out_history), _ffi.dptr(d_out_mask), C.byref(st)))
        self.stats = st

    def accumulate_motion(self, lo_xyzw: np.ndarray, lo_planes: np.ndarray, hi_planes: np.ndarray, history: Optional[np.ndarray], ids: Optional[np.ndarray],
                          body_of_prim: Optional[np.ndarray], bodies: Optional[np.ndarray], pixel_map, prev_camera, ctx: Optional[_ffi.Context] = None):
        """`accumulate` for a scene with moving rigid bodies (trhip_temporal_upsample_motion; docs/design/22-upsample-motion.md).  ids: (H, W) of _ffi.AOV_ID_DTYPE, the
        FULL-SIZE frame's AOVIntegrator.ids, or None (every pixel static); body_of_prim: uint32 per ordered-primitive slot (FlatScene.body_table) or None; bodies:
        (n_bodies, 3, 4) prev_from_cur matrices or None.  Returns (xyzw, history, mask) of this frame."""
        self._require_carry_bodies()
        return self._accumulate("accumulate_motion", True, lo_xyzw, lo_planes, hi_planes, history, ids, body_of_prim, bodies, pixel_map, prev_camera, ctx)

    def accumulate_motion_device(self, d_lo_xyzw: int, d_lo_planes: int, lo_width: int, lo_height: int, d_hi_planes: int, d_history: Optional[int], d_ids: Optional[int],
                                 d_body_of_prim: Optional[int], n_prims: int, d_bodies: Optional[int], n_bodies: int, width: int, height: int, pixel_map, prev_camera,
                                 d_out: int, d_out_history: int, d_out_mask: Optional[int] = None, ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_history, d_ids, d_body_of_prim, d_bodies and d_out_mask may be None); nothing is copied to the host."""
        self._accumulate_device(True, d_lo_xyzw, d_lo_planes, lo_width, lo_height, d_hi_planes, d_history, d_ids, d_body_of_prim, n_prims, d_bodies, n_bodies, width, height, pixel_map,
                                prev_camera, d_out, d_out_history, d_out_mask, ctx)

    def accumulate(self, lo_xyzw: np.ndarray, lo_planes: np.ndarray, hi_planes: np.ndarray, history: Optional[np.ndarray], pixel_map, prev_camera,
                   ctx: Optional[_ffi.Context] = None):
        """lo_xyzw (h, w, 4) and lo_planes (h, w, 3, 4) of this frame's jittered low camera, hi_planes (H, W, 3, 4) of the full-size one, history the second result of the
        previous frame's call, or None.  Returns (xyzw (H, W, 4), history (H, W, 3, 4), mask (H, W) uint8)."""
        if self.carry_bodies:  # no id plane: every pixel is static
            return self.accumulate_motion(lo_xyzw, lo_planes, hi_planes, history, None, None, None, pixel_map, prev_camera, ctx)
        return self._accumulate("accumulate", False, lo_xyzw, lo_planes, hi_planes, history, None, None, None, pixel_map, prev_camera, ctx)

    def accumulate_device(self, d_lo_xyzw: int, d_lo_planes: int, lo_width: int, lo_height: int, d_hi_planes: int, d_history: Optional[int], width: int, height: int, pixel_map,
                          prev_camera, d_out: int, d_out_history: int, d_out_mask: Optional[int] = None, ctx: Optional[_ffi.Context] = None) -> None:
        """The same on device pointers (d_history and d_out_mask may be None); nothing is copied to the host."""
        # (with carry_bodies no id plane: every pixel is static)
        self._accumulate_device(self.carry_bodies, d_lo_xyzw, d_lo_planes, lo_width, lo_height, d_hi_planes, d_history, None, None, 0, None, 0, width, height, pixel_map, prev_camera,
                                d_out, d_out_history, d_out_mask, ctx)


class PreviewSession:
    """A moving-camera preview of a static scene: frame k is the path film and the feature planes at sample_offset = sampler.sample_offset + k * spp, temporal accumulation
    against the previous frame's history and camera, then the à-trous filter with this frame's planes — all on the device, the buffers kept between frames.
    `reset()` drops the history (the frame counter goes on, so the next frame's noise is new): call it after Scene.with_lights, since the unclipped pass does not detect
    lighting changes; a film of another size resets as well.  A frame without history is filtered as Denoiser.render filters it, bit for bit.
    With `temporal=TemporalAccumulator(clip_gamma=...)` the history is clipped to the new frame's neighbourhood colours, and `session.scene = scene.with_lights(...)` between
    frames needs no reset(): render() flattens `self.scene` every frame, and a history lit the old way is cut back to the new frame's colours within a frame.
    `variance_guided=True`: the accumulator carries the luminance moments (TemporalAccumulator(moments=True), the default then; demodulation and albedo floor the
    denoiser's) and the filter is Denoiser.denoise_variance with the variance plane of the frame; a frame without history is filtered from its own bits with the spatial
    estimate, as Denoiser.render(variance_guided=True) filters it.  The default, False, is the session described above, call for call.
    `upscaler=Upscaler(...)`: path frame, planes, temporal pass and filter run through `camera.with_resolution(resolution / factor)` and the history is held at that size;
    the full-size planes are drawn with `guide_spp` samples per pixel (default: the sampler's) and the filtered frame is upscaled last (trhip_upscale;
    docs/design/17-upscale.md).  With None, the default, the session is the one described above, call for call.
    `display=Display(...)`: `render_display(camera)` renders the frame as `render` does and encodes the final device buffer to 8-bit RGBA (trhip_display;
    docs/design/18-display.md): only the bytes are downloaded, and the exposure state stays on the device from frame to frame (reset() and a film of another size clear it).
    `render` itself makes the calls it always made, with or without a display.
    `temporal_upsample=TemporalUpsampler(...)`, with an `upscaler` (whose presence, `factor` and `guide_spp` select the low camera and the guides; its own parameters are
    not consulted, the TemporalUpsampler's are): frame k traces the path frame and its planes through the low camera shifted by `jitter_for(k, factor)`, the full-size
    planes with `guide_spp`, upscales and blends into a FULL-SIZE history through the previous full-size camera in one pass (trhip_temporal_upsample;
    docs/design/19-temporal-upsample.md) and filters the result with the full-size planes.  Not combinable with variance_guided=True or a clipping / moments accumulator.
    With None, the default, the session makes the calls described above.
    `render(camera, motion={...})` / `render_display(camera, motion={...})`: a frame of a scene whose rigid bodies moved (docs/design/20-motion.md).  The caller has
    assigned the moved scene (Scene.moved) to `session.scene`; the dict maps top-level indices of scene.aggregate.primitives to the Transformation that carried that body
    from the previous frame's pose to this one.  The frame then also draws the id plane (trhip_render_aov_ids) and reprojects through trhip_temporal_motion, so a moving
    body keeps its history; an empty dict runs the same two calls with every pixel static.  With motion=None, the default, the session makes exactly the calls described
    above and draws no id plane — a body that moved then restarts its history every frame.  A motion frame needs the plain session: no upscaler, variance_guided,
    and no moments accumulator; `temporal_upsample` serves when the TemporalUpsampler was built with carry_bodies=True (trhip_temporal_upsample_motion;
    docs/design/22-upsample-motion.md: the id plane is drawn at full size with the guide sampler); a clipping accumulator serves when it was built with carry_bodies=True (trhip_temporal_clip_motion; docs/design/21-clip-motion.md:
    the shadow a moving body drags over static surfaces is then cut back within a frame, buffers passed apart, no copy paid).  The scene's top-level structure and primitive count must be the previous frame's (else: reset()).
    `split_direct=True` (docs/design/23-direct-split.md): the first-hit direct light stays out of the history.  Every light is a delta light, so that term has no noise
    to average and, kept apart, cannot lag: each frame also renders PathIntegrator(camera, sampler, 1) — path_li's first vertex with the frame's own samples —, the
    temporal pass is trhip_temporal_split on frame - direct (with a `motion` dict the bodies are carried, without one every pixel is static), the filter runs on the pass's
    output on every frame, and trhip_film_add puts the direct film back last: with one light the depth-1 path film, with more WhittedIntegrator(camera, sampler, 1), which
    sums every light instead of picking one.  A scene without lights renders no direct film.  render_stats then ends with the direct renders' and the addition's Stats.
    Not combinable with an upscaler, temporal_upsample, variance_guided=True or a clipping / moments accumulator.  The default, False, makes exactly the calls described
    above."""

    def __init__(self, scene: Scene, sampler: SeededSampler, max_depth: int, denoiser: Optional["Denoiser"] = None, temporal: Optional[TemporalAccumulator] = None,
                 variance_guided: bool = False, upscaler: Optional["Upscaler"] = None, factor=2, guide_spp: Optional[int] = None, display: Optional["Display"] = None,
                 temporal_upsample: Optional["TemporalUpsampler"] = None, split_direct: bool = False):
        if split_direct:
            if upscaler is not None and temporal_upsample is None:
                raise TraceHipError("PreviewSession: split_direct cannot be combined with an upscaler (the direct film would have to be upscaled beside the remainder)")
            if temporal_upsample is not None:
                raise TraceHipError("PreviewSession: split_direct cannot be combined with temporal_upsample (trhip_temporal_upsample takes no direct film)")
            if variance_guided:
                raise TraceHipError("PreviewSession: split_direct cannot be combined with variance_guided=True (trhip_temporal_moments takes no direct film)")
            if temporal is not None and (temporal.clip_params is not None or temporal.moments_params is not None):
                raise TraceHipError("PreviewSession: split_direct cannot be combined with a clipping or moments TemporalAccumulator (trhip_temporal_split neither clips "
                                    "nor carries moments)")
        self.split_direct = bool(split_direct)
        self._split_buffers = None  # split_direct: the depth-1 path film and the depth-1 Whitted film
        self._split_whitted = True  # with more than one light the film added back is Whitted's; False adds the depth-1 path film back (docs/design/23-direct-split.md)
        if temporal_upsample is not None:
            if upscaler is None:
                raise TraceHipError("PreviewSession: temporal_upsample needs an upscaler (upscaler=Upscaler(), with factor and guide_spp)")
            if variance_guided:
                raise TraceHipError("PreviewSession: temporal_upsample cannot be combined with variance_guided=True (there are no moments on the full-size history)")
            if temporal is not None and (temporal.clip_params is not None or temporal.moments_params is not None):
                raise TraceHipError("PreviewSession: temporal_upsample cannot be combined with a clipping or moments TemporalAccumulator")
            temporal_upsample.jitter_for(0, factor)  # 'grid' with another factor is refused here, not at the first frame
        self.temporal_upsample = temporal_upsample
        self._tu_buffers, self._tu_size = None, None  # low film, low planes; full planes, film, history x 2
        self.scene, self.sampler, self.max_depth = scene, sampler, int(max_depth)
        self.display = display
        self._display_buffers, self._display_size = None, None  # RGBA bytes and the 16-byte exposure state
        self.upscaler, self.factor, self.guide_spp = upscaler, factor, guide_spp
        self._up_buffers, self._up_size = None, None  # full-size planes and the upscaled film
        self.denoiser = denoiser if denoiser is not None else Denoiser()
        self.variance_guided = bool(variance_guided)
        if self.variance_guided and temporal is None:
            temporal = TemporalAccumulator(moments=True, demodulate=bool(self.denoiser.params.flags & _ffi.DENOISE_DEMODULATE), albedo_floor=self.denoiser.params.albedo_floor)
        if self.variance_guided and temporal.moments_params is None:
            raise TraceHipError("PreviewSession: variance_guided=True needs a TemporalAccumulator(moments=True)")
        self.temporal = temporal if temporal is not None else TemporalAccumulator()
        self.frame = 0
        self._size = None
        self._buffers = None     # film, planes, accumulated film, history x 2
        self._prev_matrix = None  # world_to_pixel of the camera whose history is held; None: no history
        self._prev_structure = None  # top_level_counts of the scene whose history is held (motion frames compare it)
        self._motion_buffers = None  # motion frames: the id plane, the body table, the body matrices
        self.render_stats = None  # (path, aov, temporal, denoise) Stats of the last render()

    def reset(self) -> None:
        """Drops the history.  Not needed after a change of lights when the session's accumulator clips (TemporalAccumulator(clip_gamma=...))."""
        self._prev_matrix = None
        if self._display_buffers:
            self._display_buffers[1].zero()

    def close(self) -> None:
        for b in self._buffers or ():
            b.free()
        self._buffers, self._size, self._prev_matrix = None, None, None
        for b in self._motion_buffers or ():
            b.free()
        self._motion_buffers = None
        for b in self._split_buffers or ():
            b.free()
        self._split_buffers = None
        for b in self._up_buffers or ():
            b.free()
        self._up_buffers, self._up_size = None, None
        for b in self._tu_buffers or ():
            b.free()
        self._tu_buffers, self._tu_size = None, None
        for b in self._display_buffers or ():
            b.free()
        self._display_buffers, self._display_size = None, None

    def render(self, camera: PerspectiveCamera, ctx: Optional[_ffi.Context] = None, motion=None) -> np.ndarray:
        """The next frame through `camera`; returns xyzw (H, W, 4), ready for film.set_xyzw / save.  `motion`: see the class text."""
        d_out, (h, w), _ = self._render_device(camera, ctx, motion)
        return d_out.to_host(np.float32, (h, w, 4))

    def render_display(self, camera: PerspectiveCamera, ctx: Optional[_ffi.Context] = None, motion=None) -> np.ndarray:
        """The next frame through `camera`, rendered exactly as `render` renders it and encoded by the session's Display with scale = camera.film.scale; returns uint8
        (H, W, 4).  Only these bytes leave the device."""
        if self.display is None:
            raise TraceHipError("PreviewSession.render_display: the session was constructed without display=Display(...)")
        d_out, (h, w), ctx = self._render_device(camera, ctx, motion)
        if self._display_size != (h, w):
            for b in self._display_buffers or ():
                b.free()
            self._display_size, self._display_buffers = (h, w), [_ffi.DeviceBuffer(h * w * 4), _ffi.DeviceBuffer(16).zero()]
        d_rgba, d_state = self._display_buffers
        self.display.encode_device(d_out.ptr, w, h, camera.film.scale, d_rgba.ptr, d_state.ptr, None, ctx)
        self.render_stats = self.render_stats + (self.display.stats,)
        return d_rgba.to_host(np.uint8, (h, w, 4))

    def _check_motion(self, motion) -> None:
        if not isinstance(motion, dict):
            raise TraceHipError("PreviewSession: motion must be a dict {top-level primitive index: Transformation} or None")
        if self.upscaler is not None and self.temporal_upsample is None:
            raise TraceHipError("PreviewSession: motion cannot be combined with an upscaler (the low-resolution history has no motion-aware pass)")
        if self.variance_guided:
            raise TraceHipError("PreviewSession: motion cannot be combined with variance_guided=True (trhip_temporal_moments does not carry bodies back)")
        if self.temporal_upsample is not None:
            if not self.temporal_upsample.carry_bodies:
                raise TraceHipError("PreviewSession: motion cannot be combined with temporal_upsample unless the TemporalUpsampler was built with carry_bodies=True "
                                    "(trhip_temporal_upsample does not carry bodies back)")
            return  # the accumulator is not used in this mode
        if (self.temporal.clip_params is not None and self.temporal.clip_motion_params is None) or self.temporal.moments_params is not None:
            raise TraceHipError("PreviewSession: motion cannot be combined with a clipping or moments TemporalAccumulator, unless the clipping one was built with "
                                "carry_bodies=True (trhip_temporal_clip and trhip_temporal_moments do not carry bodies back)")

    def _motion_tables(self, flat, motion, h, w):
        """(id plane, body table or None, matrices or None, n_prims, n_bodies) on the device for this frame's motion dict."""
        keys = sorted(motion)
        for k in keys:
            if not (isinstance(k, (int, np.integer)) and 0 <= k < len(flat.top_counts)):
                raise TraceHipError(f"PreviewSession: motion key {k!r} is no index into the {len(flat.top_counts)} top-level primitives of the scene")
        old = self._motion_buffers or []
        keep = bool(old) and old[0].nbytes == h * w * 16  # the id plane's buffer stays from frame to frame; the tables are this frame's
        for b in old[1 if keep else 0:]:
            b.free()
        self._motion_buffers = [old[0] if keep else _ffi.DeviceBuffer(h * w * 16)]
        if not keys:
            return self._motion_buffers[0], None, None, 0, 0
        body_of_top = [None] * len(flat.top_counts)
        for i, k in enumerate(keys):
            body_of_top[k] = i
        table = flat.body_table(body_of_top)
        mats = np.ascontiguousarray(np.stack([TemporalAccumulator.prev_from_cur(motion[k]) for k in keys]), dtype=np.float32)
        self._motion_buffers += [_ffi.DeviceBuffer(table.nbytes).from_host(table), _ffi.DeviceBuffer(mats.nbytes).from_host(mats)]
        return self._motion_buffers[0], self._motion_buffers[1], self._motion_buffers[2], table.size, len(keys)

    def _render_device(self, camera: PerspectiveCamera, ctx: Optional[_ffi.Context], motion=None):
        """The frame of `render`, left on the device: (buffer, (H, W), context)."""
        if motion is not None:
            self._check_motion(motion)
        flat = self.scene.flatten(ctx)
        ctx = flat.ctx
        if self.temporal_upsample is not None:
            return self._render_temporal_upsample(camera, ctx, motion, flat)
        hi_camera = camera
        if self.upscaler is not None:
            camera = Upscaler.low_camera(hi_camera, self.factor)
        h, w = camera.film.size
        if self._size != (h, w):
            self.close()
            self._size = (h, w)
            self._buffers = [_ffi.DeviceBuffer(h * w * n) for n in (16, 48, 16, 48, 48) + ((8, 8, 4) if self.variance_guided else ())]
        d_film, d_planes, d_acc = self._buffers[:3]
        d_prev, d_next = self._buffers[3 + (self.frame & 1)], self._buffers[3 + ((self.frame & 1) ^ 1)]
        spp = self.sampler.samples_per_pixel
        sampler = SeededSampler(spp, seed=self.sampler.seed, sample_offset=self.sampler.sample_offset + self.frame * spp)
        path, aov = PathIntegrator(camera, sampler, self.max_depth), AOVIntegrator(camera, sampler)
        structure = list(flat.top_counts)
        if motion is not None:
            if self._prev_matrix is not None and self._prev_structure is not None and structure != self._prev_structure:
                raise TraceHipError("PreviewSession: the scene's top-level structure or primitive count differs from the previous frame's, so its bodies cannot be "
                                    "matched with the history: call reset() before rendering it")
            d_ids, d_table, d_bodies, n_prims, n_bodies = self._motion_tables(flat, motion, h, w)
        path.render(self.scene, ctx, device_out=d_film.ptr)
        d_direct = d_direct_all = None  # split_direct: the film taken out before the history, the film put back after the filter
        direct_stats = ()
        if self.split_direct and self.scene.lights:
            if self._split_buffers is None:
                self._split_buffers = [_ffi.DeviceBuffer(h * w * 16) for _ in range(2)]
            d_direct, d_direct_all = self._split_buffers[0], self._split_buffers[0]
            first = PathIntegrator(camera, sampler, 1)  # path_li's first vertex: the same samples, film weights and light picks as `path`
            first.render(self.scene, ctx, device_out=d_direct.ptr)
            direct_stats = (first.stats,)
            if len(self.scene.lights) > 1 and self._split_whitted:  # every light summed at the first hit: no light-picking noise comes back
                every = WhittedIntegrator(camera, sampler, 1)
                d_direct_all = self._split_buffers[1]
                every.render(self.scene, ctx, device_out=d_direct_all.ptr)
                direct_stats += (every.stats,)
        if motion is not None:
            aov.render(self.scene, ctx, device_out=d_planes.ptr, device_ids=d_ids.ptr)
        else:
            aov.render(self.scene, ctx, device_out=d_planes.ptr)
        prev_matrix, matrix = self._prev_matrix, camera.world_to_pixel()
        had_history = prev_matrix is not None
        self._prev_matrix = None  # (until this frame's history is complete)
        if self.split_direct:
            if motion is None:
                d_ids, d_table, d_bodies, n_prims, n_bodies = None, None, None, 0, 0
            self.temporal.accumulate_split_device(d_film.ptr, d_direct.ptr if d_direct else None, d_planes.ptr, d_prev.ptr if had_history else None, d_ids.ptr if d_ids else None,
                                                  d_table.ptr if d_table else None, n_prims, d_bodies.ptr if d_bodies else None, n_bodies, w, h, prev_matrix, d_acc.ptr, d_next.ptr, ctx)
            # always the pass's output, the first frame too: the filter's input is the remainder, not the frame
            self.denoiser.denoise_device(d_acc.ptr, d_planes.ptr, w, h, d_acc.ptr, ctx)
            if d_direct_all:
                direct_stats += (Film.add_device(d_acc.ptr, d_direct_all.ptr, w, h, d_acc.ptr, ctx),)
        elif motion is not None:
            self.temporal.accumulate_motion_device(d_film.ptr, d_planes.ptr, d_prev.ptr if had_history else None, d_ids.ptr, d_table.ptr if d_table else None, n_prims,
                                                   d_bodies.ptr if d_bodies else None, n_bodies, w, h, prev_matrix, d_acc.ptr, d_next.ptr, ctx)
            self.denoiser.denoise_device((d_acc if had_history else d_film).ptr, d_planes.ptr, w, h, d_acc.ptr, ctx)
        elif self.variance_guided:
            m_prev, m_next, d_var = self._buffers[5 + (self.frame & 1)], self._buffers[5 + ((self.frame & 1) ^ 1)], self._buffers[7]
            self.temporal.accumulate_moments_device(d_film.ptr, d_planes.ptr, d_prev.ptr if had_history else None, m_prev.ptr if had_history else None, w, h, prev_matrix, d_acc.ptr,
                                                    d_next.ptr, m_next.ptr, d_var.ptr, ctx)
            self.denoiser.denoise_variance_device((d_acc if had_history else d_film).ptr, d_planes.ptr, d_var.ptr, w, h, d_acc.ptr, None, ctx)
        else:
            self.temporal.accumulate_device(d_film.ptr, d_planes.ptr, d_prev.ptr if had_history else None, w, h, prev_matrix, d_acc.ptr, d_next.ptr, ctx)
            # without history the accumulated film is the frame itself up to the rounding of XYZ -> RGB -> XYZ: the frame's own bits are filtered then
            self.denoiser.denoise_device((d_acc if had_history else d_film).ptr, d_planes.ptr, w, h, d_acc.ptr, ctx)
        self.render_stats = (path.stats, aov.stats, self.temporal.stats, self.denoiser.stats) + direct_stats
        if self.upscaler is not None:
            out = self._upscale(hi_camera, camera, sampler, d_acc, d_planes, ctx), hi_camera.film.size, ctx
        else:
            out = d_acc, (h, w), ctx
        self._prev_matrix = matrix
        self._prev_structure = structure
        self.frame += 1
        return out

    def _upscale(self, hi_camera, lo_camera, sampler, d_lo, d_lo_planes, ctx) -> "_ffi.DeviceBuffer":
        """The session's filtered low-resolution frame onto the full-size planes of this frame (left on the device)."""
        (hh, hw), (lh, lw) = hi_camera.film.size, lo_camera.film.size
        if self._up_size != (hh, hw):
            for b in self._up_buffers or ():
                b.free()
            self._up_size, self._up_buffers = (hh, hw), [_ffi.DeviceBuffer(hh * hw * n) for n in (48, 16)]
        d_hi_planes, d_out = self._up_buffers
        guide = SeededSampler(sampler.samples_per_pixel if self.guide_spp is None else int(self.guide_spp), seed=sampler.seed, sample_offset=sampler.sample_offset)
        aov = AOVIntegrator(hi_camera, guide)
        aov.render(self.scene, ctx, device_out=d_hi_planes.ptr)
        self.upscaler.upscale_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_hi_planes.ptr, hw, hh, Upscaler.pixel_map(hi_camera, lo_camera), d_out.ptr, None, ctx)
        self.render_stats = self.render_stats + (aov.stats, self.upscaler.stats)
        return d_out

    def _render_temporal_upsample(self, hi_camera: PerspectiveCamera, ctx, motion=None, flat=None):
        """The frame of the temporal-upsampling mode, left on the device: (buffer, (H, W), context).  With a motion dict (an upsampler built with carry_bodies=True) the
        full-size planes and the full-size id plane are drawn in one call and the pass is trhip_temporal_upsample_motion; with None the calls are what they were."""
        tu = self.temporal_upsample
        lo_camera = Upscaler.low_camera(hi_camera, self.factor, jitter=tu.jitter_for(self.frame, self.factor))
        (hh, hw), (lh, lw) = hi_camera.film.size, lo_camera.film.size
        if self._tu_size != ((hh, hw), (lh, lw)):
            self.close()
            self._tu_size = ((hh, hw), (lh, lw))
            self._tu_buffers = [_ffi.DeviceBuffer(n) for n in (lh * lw * 16, lh * lw * 48, hh * hw * 48, hh * hw * 16, hh * hw * 48, hh * hw * 48)]
        d_lo, d_lo_planes, d_hi_planes, d_out = self._tu_buffers[:4]
        d_prev, d_next = self._tu_buffers[4 + (self.frame & 1)], self._tu_buffers[4 + ((self.frame & 1) ^ 1)]
        spp = self.sampler.samples_per_pixel
        sampler = SeededSampler(spp, seed=self.sampler.seed, sample_offset=self.sampler.sample_offset + self.frame * spp)
        guide = SeededSampler(spp if self.guide_spp is None else int(self.guide_spp), seed=sampler.seed, sample_offset=sampler.sample_offset)
        path, aov_lo, aov_hi = PathIntegrator(lo_camera, sampler, self.max_depth), AOVIntegrator(lo_camera, sampler), AOVIntegrator(hi_camera, guide)
        structure = list(flat.top_counts) if flat is not None else None
        if motion is not None:
            if self._prev_matrix is not None and self._prev_structure is not None and structure != self._prev_structure:
                raise TraceHipError("PreviewSession: the scene's top-level structure or primitive count differs from the previous frame's, so its bodies cannot be "
                                    "matched with the history: call reset() before rendering it")
            d_ids, d_table, d_bodies, n_prims, n_bodies = self._motion_tables(flat, motion, hh, hw)
        path.render(self.scene, ctx, device_out=d_lo.ptr)
        aov_lo.render(self.scene, ctx, device_out=d_lo_planes.ptr)
        if motion is not None:
            aov_hi.render(self.scene, ctx, device_out=d_hi_planes.ptr, device_ids=d_ids.ptr)
        else:
            aov_hi.render(self.scene, ctx, device_out=d_hi_planes.ptr)
        prev_matrix, matrix = self._prev_matrix, hi_camera.world_to_pixel()
        self._prev_matrix = None  # (until this frame's history is complete)
        if motion is not None:
            tu.accumulate_motion_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_hi_planes.ptr, d_prev.ptr if prev_matrix is not None else None, d_ids.ptr,
                                        d_table.ptr if d_table else None, n_prims, d_bodies.ptr if d_bodies else None, n_bodies, hw, hh,
                                        Upscaler.pixel_map(hi_camera, lo_camera), prev_matrix, d_out.ptr, d_next.ptr, None, ctx)
        else:
            tu.accumulate_device(d_lo.ptr, d_lo_planes.ptr, lw, lh, d_hi_planes.ptr, d_prev.ptr if prev_matrix is not None else None, hw, hh,
                                 Upscaler.pixel_map(hi_camera, lo_camera), prev_matrix, d_out.ptr, d_next.ptr, None, ctx)
        self.denoiser.denoise_device(d_out.ptr, d_hi_planes.ptr, hw, hh, d_out.ptr, ctx)
        self.render_stats = (path.stats, aov_lo.stats, aov_hi.stats, tu.stats, self.denoiser.stats)
        self._prev_matrix = matrix
        self._prev_structure = structure
        self.frame += 1
        return d_out, (hh, hw), ctx


# ---- SPPM and the DirectionalLight -------------------------------------------------------------------------------------------------
def _to_Y(c) -> np.float32:  # spectrum.jl:64-66
    c = np.asarray(c, np.float32)
    return f32(f32(f32(0.212671) * c[0]) + f32(f32(0.715160) * c[1])) + f32(f32(0.072169) * c[2])


def light_power_y(light) -> np.float32:
    """to_Y(power(light)) as the library's SPPM host code forms it (point.jl:74-76, spot.jl:42-44, directional.jl:54-56); a SpotLight's cosines through
    the library's deterministic cosine, as its constructor (spot.jl:17)."""
    I = np.asarray(light.i.c, np.float32)
    if isinstance(light, PointLight):
        return _to_Y(f32(f32(4.0) * _PI32) * I)
    if isinstance(light, SpotLight):
        ct, cf = _ffi.detmath(1, [_deg2rad(light.total_width), _deg2rad(light.falloff_start)])
        return _to_Y(((I * f32(2.0)) * _PI32) * f32(f32(1.0) - f32(f32(0.5) * f32(cf + ct))))
    if isinstance(light, DirectionalLight):
        r = f32(f32(0.5) * f32(f32(2.0) * f32(light.world_radius)))
        return _to_Y((I * _PI32) * f32(r * r))
    raise TraceHipError(f"unsupported light {type(light).__name__}")


def _light_cdf(func) -> np.ndarray:
    """Distribution1D(func).cdf (sampling.jl:8-29) in Float32; a zero integral falls back to cdf[i] = i / n (1-based)."""
    n = len(func)
    cdf = np.zeros(n + 1, np.float32)
    for i in range(1, n + 1):
        cdf[i] = f32(cdf[i - 1] + f32(f32(func[i - 1]) / f32(n)))
    func_int = cdf[n]
    for i in range(1, n + 1):
        cdf[i] = f32((i + 1) / n) if func_int == 0 else f32(cdf[i] / func_int)
    return cdf


def radical_inverse_is_one(lo: int, hi: int) -> bool:
    """Is radical_inverse(0, i) == 1f0 (sampling.jl:45: reverse_bits(i) * 2^-64 in Float64, then Float32) for some Halton index lo <= i < hi?  It is
    exactly when the reversed index is >= 2^64 - 2^39 - 2^10 (the Float64 and Float32 roundings to nearest even), i.e. when the low 25 bits of i are all
    ones, or the low 24 are, bit 24 is not and bits 25..53 are."""
    for m, v in ((25, (1 << 25) - 1), (54, ((1 << 24) - 1) | (((1 << 54) - 1) ^ ((1 << 25) - 1)))):
        i = lo + ((v - lo) % (1 << m))  # the first i >= lo with i mod 2^m == v
        if i < hi:
            return True
    return False


def sppm_directional_pick(lights, n_photons: int, first_index: int = 0) -> int:
    """The light (0-based) of ``lights`` that is a DirectionalLight and that sample_discrete over the light power (sampling.jl:32-41) could pick for a
    photon of Halton index first_index .. first_index + n_photons - 1, or -1.  The reference has no sample_le for the light (sppm.jl:361), so the
    library's SPPMIntegrator refuses exactly such a call (csrc/tu_sppm.hip, sppm_directional_pick; the range there is 0 .. n_iterations * photons - 1):
    a light's interval [cdf[k], cdf[k+1]) of nonzero width counts as pickable; the last light, taken for u >= cdf[n], with cdf[n] == 1 only when some
    index of the range has radical_inverse(0, index) == 1f0."""
    if not lights:
        return -1
    cdf = _light_cdf([light_power_y(l) for l in lights])
    n = len(lights)
    for k, l in enumerate(lights):
        if not isinstance(l, DirectionalLight):
            continue
        if k + 1 < n:
            if not (cdf[k + 1] <= cdf[k]):
                return k
        elif not (cdf[k] >= 1) or (cdf[k] == 1 and radical_inverse_is_one(first_index, first_index + n_photons)):
            return k
    return -1


class SPPMIntegrator:  # integrators/sppm.jl:108-130
    """SPPMIntegrator(camera, initial_search_radius, max_depth, n_iterations, photons_per_iteration = -1, write_frequency = 1).

    ``seed`` selects the seeded sampler stream of the camera pass (the reference draws from the global RNG there).
    ``write_frequency`` (sppm.jl:166-171): ``__call__`` stores and saves the film after every iteration it divides and after the
    last one, as the reference does; ``render(on_write=...)`` hands those intermediate images to a callback instead.  Note the
    reference's default of 1: an image per iteration (the library then runs one iteration per batch, about 3x slower)."""

    def __init__(self, camera: PerspectiveCamera, initial_search_radius, max_depth: int, n_iterations: int, photons_per_iteration: int = -1, write_frequency: int = 1,
                 seed: int = 0x5EED0001):
        self.camera = camera
        self.initial_search_radius = f32(initial_search_radius)
        self.max_depth, self.n_iterations = int(max_depth), int(n_iterations)
        crop = camera.film.crop_bounds
        area = int((f32(crop.p_max[0]) - f32(crop.p_min[0])) * (f32(crop.p_max[1]) - f32(crop.p_min[1])))  # area(crop_bounds) bounds.jl:87-90
        self.photons_per_iteration = int(photons_per_iteration) if photons_per_iteration > 0 else area  # :121-124
        self.write_frequency = int(write_frequency)
        self.seed = int(seed)
        self.stats: Optional[_ffi.Stats] = None
        self._ctx = None

    def render(self, scene: Scene, ctx: Optional[_ffi.Context] = None, on_write=None) -> np.ndarray:
        """The film after ``n_iterations``.  ``on_write(iteration, xyzw)``: called with the image of the first ``iteration`` iterations after every iteration
        below the last that ``write_frequency`` divides (sppm.jl:166-171); the array is only valid during the call."""
        flat = scene.flatten(ctx)
        ctx = flat.ctx
        self._ctx = ctx  # (before the call: the periodic-image callback asks it for this process's rank in the job)
        sn = self.camera.sensor()
        st = _ffi.Stats()
        film = self.camera.film
        h, w = film.size
        out = np.empty((h, w, 4), dtype=np.float32)
        if on_write is not None and self.write_frequency > 0:
            failure = []

            def _cb(_user, iteration, ptr):
                try:
                    on_write(int(iteration), np.ctypeslib.as_array(ptr, shape=(h, w, 4)))
                    return 0
                except Exception as e:  # nothing may propagate through the C frames
                    failure.append(e)
                    return 1
            cb = _ffi.SPPM_WRITE_FN(_cb)
            rc = _ffi.lib().trhip_render_sppm_ex(ctx._h, flat._h, C.byref(sn), float(self.initial_search_radius), self.max_depth, self.n_iterations, self.photons_per_iteration, self.seed,
                                                 _ffi.fptr(out), C.byref(st), self.write_frequency, cb, None)
            if failure:
                raise failure[0]
            ctx.check(rc)
        else:
            ctx.check(_ffi.lib().trhip_render_sppm(ctx._h, flat._h, C.byref(sn), float(self.initial_search_radius), self.max_depth, self.n_iterations, self.photons_per_iteration, self.seed,
                                                   _ffi.fptr(out), C.byref(st)))
        self.stats = st
        self._ctx = ctx
        film.set_xyzw(out)  # set_image!(film, image) film.jl:195-202
        film.splat_xyz[...] = 0
        return out

    def state(self) -> dict:
        """SPPMPixel fields after the last render (see trhip_sppm_state)."""
        ctx = self._ctx
        h, w = self.camera.film.size
        out = {"Ld": np.empty((h, w, 3), np.float32), "tau": np.empty((h, w, 3), np.float32), "radius": np.empty((h, w), np.float32), "N": np.empty((h, w), np.float64),
               "M": np.empty((h, w), np.int64), "phi": np.empty((h, w, 3), np.float32), "vp_p": np.empty((h, w, 3), np.float32), "vp_beta": np.empty((h, w, 3), np.float32)}
        info = np.zeros(6, np.int64)
        i64 = C.POINTER(C.c_int64)
        ctx.check(_ffi.lib().trhip_sppm_state(ctx._h, _ffi.fptr(out["Ld"]), _ffi.fptr(out["tau"]), _ffi.fptr(out["radius"]), out["N"].ctypes.data_as(C.POINTER(C.c_double)),
                                              out["M"].ctypes.data_as(i64), _ffi.fptr(out["phi"]), _ffi.fptr(out["vp_p"]), _ffi.fptr(out["vp_beta"]), info.ctypes.data_as(i64)))
        out["info"] = {"grid_res": info[:3].copy(), "grid_entries": int(info[3]), "photon_hits": int(info[4]), "photons_per_iteration": int(info[5])}
        return out

    def __call__(self, scene: Scene):
        film = self.camera.film

        def periodic(iteration, xyzw):  # sppm.jl:166-171: set_image!(film, image); save(film)
            if self._job_rank() != 0:  # in a multi-GPU job every rank holds the whole image after the iteration's all-reduce: rank 0 writes it (as julia/TraceHIP.jl does)
                return
            film.set_xyzw(xyzw.copy())
            film.splat_xyz[...] = 0
            save(film)
        self.render(scene, on_write=periodic if film.filename and 0 < self.write_frequency < self.n_iterations else None)
        if film.filename and self._job_rank() == 0:
            return save(film)
        return None

    def _job_rank(self) -> int:
        """This process's rank in the library's multi-GPU job (0 without a communicator)."""
        return self._ctx.comm_rank()[0] if self._ctx is not None else 0  # (no render yet on a context: nothing to ask)


# ---- model_loader.jl:1-11 without Assimp: a minimal PLY reader ---------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4",
              "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path: str):
    """(vertices (n, 3) Float32, normals (n, 3) Float32 or None, faces (m, 3) 0-based UInt32) of an ascii / binary PLY with
    triangle faces (a list property on the face element) — the subset docs/src/assets/models needs."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: truncated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] == "comment" or tok[0] == "obj_info":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append({"name": tok[1], "count": int(tok[2]), "props": []})
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1]["props"].append(("list", tok[2], tok[3], tok[4]))
                else:
                    elements[-1]["props"].append(("scalar", tok[1], tok[2]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unsupported PLY format {fmt}")
        end = ">" if fmt == "binary_big_endian" else "<"
        verts = normals = faces = None
        for el in elements:
            n, props = el["count"], el["props"]
            if all(p[0] == "scalar" for p in props):
                names = [p[2] for p in props]
                if fmt == "ascii":
                    rows = np.array([f.readline().split() for _ in range(n)], dtype=np.float64).reshape(n, len(props))
                    cols = {nm: rows[:, i] for i, nm in enumerate(names)}
                else:
                    dt = np.dtype([(p[2], end + _PLY_TYPES[p[1]]) for p in props])
                    rec = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
                    cols = {nm: rec[nm] for nm in names}
                if el["name"] == "vertex":
                    verts = np.stack([cols["x"], cols["y"], cols["z"]], axis=1).astype(np.float32)
                    if all(k in cols for k in ("nx", "ny", "nz")):
                        normals = np.stack([cols["nx"], cols["ny"], cols["nz"]], axis=1).astype(np.float32)
            else:
                if len(props) != 1:
                    raise ValueError(f"{path}: element {el['name']}: only a single list property is supported")
                _, ct, it, _ = props[0]
                if fmt == "ascii":
                    rows = [f.readline().split() for _ in range(n)]
                    if any(int(r[0]) != 3 for r in rows):
                        raise ValueError("Only triangles supported.")  # model_loader.jl:29
                    idx = np.array([r[1:4] for r in rows], dtype=np.int64).reshape(n, 3)
                else:
                    dt = np.dtype([("n", end + _PLY_TYPES[ct]), ("i", end + _PLY_TYPES[it], (3,))])
                    rec = np.frombuffer(f.read(dt.itemsize * n), dtype=dt, count=n)
                    if n and np.any(rec["n"] != 3):
                        raise ValueError("Only triangles supported.")
                    idx = rec["i"].astype(np.int64)
                if el["name"] == "face":
                    faces = idx.astype(np.uint32)
        if verts is None or faces is None:
            raise ValueError(f"{path}: no vertex / face element")
        if faces.size and int(faces.max()) >= verts.shape[0]:
            raise ValueError(f"{path}: face index out of range")
        return verts, normals, faces


def load_triangle_mesh(model_file: str, core: Optional[ShapeCore] = None):
    """model_loader.jl:1-11: (triangle_meshes, triangles).  The reference goes through Assimp; PLY is read directly here.
    Like the reference it requires one normal per vertex (model_loader.jl:30)."""
    core = core or ShapeCore(Transformation(), False)
    verts, normals, faces = read_ply(model_file)
    if normals is None or normals.shape[0] != verts.shape[0]:
        raise ValueError("Number of normals is different from the number of vertices")
    indices = (faces.reshape(-1) + 1).astype(np.uint32)  # 1-based (model_loader.jl:36)
    triangles = create_triangle_mesh(core, faces.shape[0], indices, verts.shape[0], verts, normals)
    return [triangles[0].mesh] if triangles else [], triangles
