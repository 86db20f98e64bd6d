"""A numpy Float32 model of the two kernels of docs/design/23-direct-split.md, written from that specification: it imports nothing from the library.  `accumulate` is
trhip_temporal_split — step 0, then tests/motion_model.py's pass on B' —, `film_add` is trhip_film_add.  Every line is one Float32 operation, in the order the text gives.

Not a test: tests/test_direct_split_api.py (CPU) checks the model's own properties, tests/test_gpu_direct_split.py compares the kernels with it bit for bit."""
import numpy as np

import motion_model as mm

F = np.float32
Params = mm.Params
ID_DTYPE = mm.ID_DTYPE


def remainder(B, direct):
    """Step 0: B' = (B.x - D.x, B.y - D.y, B.z - D.z, B.w); without a direct film B' is B, the same bits.  D.w is not read."""
    B = np.ascontiguousarray(B, F)
    if direct is None:
        return B
    D = np.ascontiguousarray(direct, F)
    assert D.shape == B.shape
    out = B.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = B[..., :3] - D[..., :3]
    return out


def accumulate(B, direct, P, history, M, ids, body_of_prim, bodies, prm, tally=None):
    """(out_xyzw (H, W, 4), out_history (H, W, 3, 4)): motion_model.accumulate on the remainder.  ids None (allowed when there is no table): every pixel is static."""
    B1 = remainder(B, direct)
    if ids is None:
        assert body_of_prim is None or len(body_of_prim) == 0
        ids = np.zeros(B1.shape[:2], ID_DTYPE)
        ids["prim"] = -1
        body_of_prim = None
    return mm.accumulate(B1, P, history, M, ids, body_of_prim, bodies, prm, tally)


def film_add(a, b):
    """out.xyz = a.xyz + b.xyz, out.w = a.w."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape and a.shape[-1] == 4
    out = a.copy()
    with np.errstate(all="ignore"):
        out[..., :3] = a[..., :3] + b[..., :3]
    return out


def synthetic_direct(B, seed, kind):
    """A direct film for the frame B: 'finite' — between 0 and 1.2 of the film's own xyz, so that the remainder is mostly a colour and sometimes negative, with a .w of garbage;
    'special' — the same with NaN, +Inf, -Inf and -0 entries sprinkled over a fifth of the values; 'zero' — all +0."""
    rng = np.random.default_rng(seed + 23)
    if kind == "zero":
        return np.zeros(B.shape, F)
    D = np.empty(B.shape, F)
    with np.errstate(all="ignore"):
        D[..., :3] = (np.nan_to_num(B[..., :3], nan=0.25, posinf=1.0, neginf=-1.0) * rng.uniform(0.0, 1.2, B.shape[:2] + (3,))).astype(F)
    D[..., 3] = rng.integers(0, 1 << 32, B.shape[:2]).astype(np.uint32).view(F)
    if kind == "special":
        u = rng.random(B.shape[:2] + (3,))
        xyz = D[..., :3]
        xyz[u < 0.20] = F(-0.0)
        xyz[u < 0.15] = -np.inf
        xyz[u < 0.10] = np.inf
        xyz[u < 0.05] = np.nan
        # Inf - Inf MAKES a NaN, and its sign is the processor's (x86 sets it, the GPU does not): where the film itself is not finite the direct film stays finite, so
        # that every NaN of the remainder is one that came in and both sides pass it on
        D[..., :3] = np.where(np.isfinite(B[..., :3]), xyz, D[..., :3])
    else:
        assert kind == "finite"
        assert np.isfinite(D[..., :3]).all()
    return D
