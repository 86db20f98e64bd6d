"""First-hit feature buffers, the part that needs no GPU: the per-sample record's layout (header text == ctypes mirror == numpy dtype) and the base-colour table.

The record is 80 bytes, not the 64 its first specification named: that text listed t, prim, b1, b2, p[3], material, n[3], ns[3], albedo[3] — seventeen 32-bit values, each to be
returned bit for bit — which four 16-byte words cannot hold.  Every listed field is kept, in five 16-byte words; this test pins that size to the header text."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = {"float": 4, "int32_t": 4, "uint32_t": 4}


def header_fields():
    """(name, C type, count, offset) of every member of trhip_aov_sample, from the text of include/tracehip.h (all members are 4-byte scalars or arrays of them: no padding)."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tracehip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*trhip_aov_sample\s*;", src).group(1)
    out, off = [], 0
    for ctype, names in re.findall(r"(\w+)\s+([^;]+);", body):
        for name in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            count = int(m.group(2) or 1)
            out.append((m.group(1), ctype, count, off))
            off += WIDTH[ctype] * count
    return out, off


def test_record_mirror_matches_the_header(T):
    fields, size = header_fields()
    assert [f[0] for f in fields] == ["t", "prim", "b1", "b2", "p", "material", "n", "pad0", "ns", "pad1", "albedo", "pad2"]
    assert size == 80 and size % 16 == 0
    S = T._ffi.AovSample
    assert C.sizeof(S) == size == T._ffi.AOV_DTYPE.itemsize
    ctypes_of = {"float": C.c_float, "int32_t": C.c_int32, "uint32_t": C.c_uint32}
    numpy_of = {"float": np.float32, "int32_t": np.int32, "uint32_t": np.uint32}
    assert [n for n, _ in S._fields_] == [f[0] for f in fields] == list(T._ffi.AOV_DTYPE.names)
    for (name, ctype, count, off), (_, ct) in zip(fields, S._fields_):
        assert getattr(S, name).offset == off, name
        assert ct is (ctypes_of[ctype] if count == 1 else ctypes_of[ctype] * count), name
        dt, doff = T._ffi.AOV_DTYPE.fields[name][:2]
        assert doff == off and dt.base == np.dtype(numpy_of[ctype]) and dt.shape == (() if count == 1 else (count,)), name
    # the 16-byte words the resolve kernel stores: hit | p, material | n, 0 | ns, 0 | albedo, 0
    assert [S.t.offset, S.p.offset, S.n.offset, S.ns.offset, S.albedo.offset] == [0, 16, 32, 48, 64]
    assert [S.material.offset, S.pad0.offset, S.pad1.offset, S.pad2.offset] == [28, 44, 60, 76]


def test_entry_points_are_declared_and_bound(T):
    header = open(os.path.join(ROOT, "include", "tracehip.h")).read()
    for name in ("trhip_render_aov", "trhip_render_aov_device"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in T._ffi.SIGNATURES and len(T._ffi.SIGNATURES[name][1]) == 9
        assert getattr(T.lib(), name) is not None
    assert T.lib().trhip_version() == 3001


def test_base_colour_table(T):
    rgb = lambda *c: T.ConstantTexture(T.RGBSpectrum(*c))  # noqa: E731
    f = T.ConstantTexture
    bits = lambda a: np.asarray(a, np.float32).view(np.uint32).tolist()  # noqa: E731
    kd, ks, kr, kt = (0.796, 0.235, 0.2), (0.3, 0.4, 0.5), (0.9, 0.8, 0.7), (0.25, 0.5, 0.75)
    assert bits(T.api.base_colour(T.MatteMaterial(rgb(*kd), f(0.0)))) == bits(kd)
    assert bits(T.api.base_colour(T.MirrorMaterial(rgb(*kr)))) == bits(kr)
    assert bits(T.api.base_colour(T.PlasticMaterial(rgb(*kd), rgb(*ks), f(0.1), True))) == bits(kd)
    assert bits(T.api.base_colour(T.GlassMaterial(rgb(*kr), rgb(*kt), f(0.0), f(0.0), f(1.5), True))) == bits(kt)
    # a glass whose Kt is black — as given, or only after the clamp — reports Kr
    assert bits(T.api.base_colour(T.GlassMaterial(rgb(*kr), rgb(0.0), f(0.0), f(0.0), f(1.5), True))) == bits(kr)
    assert bits(T.api.base_colour(T.GlassMaterial(rgb(*kr), rgb(-1.0, -0.5, 0.0), f(0.0), f(0.0), f(1.5), True))) == bits(kr)
    # the clamp of materials/material.jl: to [0, +Inf) per channel — negative channels go to 0, values above 1 stay
    assert bits(T.api.base_colour(T.MatteMaterial(rgb(-0.5, 2.5, 0.25), f(0.0)))) == bits((0.0, 2.5, 0.25))
    assert bits(T.api.base_colour(None)) == bits((0.0, 0.0, 0.0))


def test_primitive_materials_follow_the_flattening_order(T):
    """Material ids are handed out in the order FlatScene meets the materials (caller order of the primitives); a bulk mesh counts once per triangle."""
    scene = T.scenes.mesh_scene(4)
    ids, cols = T.api.primitive_materials(scene)
    assert ids.shape == (12 + 32,) and cols.shape == (12 + 32, 3)
    assert ids[:12].tolist() == [0] * 6 + [1, 1, 2, 2, 3, 4] and set(ids[12:].tolist()) == {5}
    assert np.array_equal(cols[12:], np.full((32, 3), np.float32(0.8)))
    prims, _ = T.scenes.cornell_primitives()
    prims[0] = T.GeometricPrimitive(prims[0].shape, None)
    ids, cols = T.api.primitive_materials(T.Scene([], T.BVHAccel(prims, 1)))
    assert ids[0] == -1 and ids[1] == 0 and not cols[0].any()


def test_normalise_divides_only_where_the_weight_is_not_zero(T):
    planes = np.zeros((1, 3, 3, 4), np.float32)
    planes[0, 0] = [[2, 4, 6, 4], [1, 2, 3, 2], [8, 6, 4, 10]]  # covered: total weight 4, hit weight 2
    planes[0, 1, 0] = [0, 0, 0, 4]                                # all misses: only plane 0's weight
    r = T.AOVIntegrator.normalise(planes)                          # pixel 2: nothing reached it
    assert r.albedo[0, 0].tolist() == [0.5, 1.0, 1.5] and r.normal[0, 0].tolist() == [0.5, 1.0, 1.5] and r.position[0, 0].tolist() == [4.0, 3.0, 2.0]
    assert r.depth[0, 0] == 5.0 and r.alpha[0].tolist() == [0.5, 0.0, 0.0]
    assert not r.albedo[0, 1:].any() and not r.normal[0, 1:].any() and not r.depth[0, 1:].any()
    assert r["planes"] is r.planes and r.planes.shape == (1, 3, 3, 4)
