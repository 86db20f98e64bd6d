"""State shared between kinds of path frame on one context (docs/design/30-path-terms.md): the shadow lane serves the NEE term and the emit term, its note bytes carry
opposite meanings in the two, and the base records serve the environment terms and the emit term.  Five kinds of frame — path, path-env, path-env with next-event
estimation, emit, emit with HITS_ONLY — are rendered once each for reference and then in a tour in which every ordered pair of kinds occurs adjacently, a kind followed by
itself included; after every frame the film, the per-sample radiance, the shadow-ray count, the escape records (the two environment kinds) and the emitted sums (the two
emit kinds) equal the references bit for bit.  The tour runs again on three batches over two pipelines without overlap.

Shape: tests/path_emit_model.py's strip4 scene through tests/path_env_model.py's 37 x 29 camera at 3 spp, depth 4 — the shape of
tests/test_gpu_path_emit.py::test_frames_around_an_emit_frame_keep_their_bits, which shows that every kind renders on this scene.  The references are the library's own
first frames: what the frames contain is pinned to the models by the three terms' own test files; this one asks only that a frame does not depend on the frame before it."""
import numpy as np
import pytest

import path_emit_model as em
import path_env_model as pm
import path_nee_model as nm

pytestmark = pytest.mark.gpu

SEED = em.SEED
KINDS = ("path", "env", "env-nee", "emit", "emit-hits-only")


def tour(n):
    """A closed walk over n kinds that takes every ordered pair (a, b), a == b included, exactly once: an Euler circuit of the complete digraph with loops (Hierholzer).
    n * n + 1 entries."""
    unused = {a: list(range(n)) for a in range(n)}
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if unused[a]:
            stack.append(unused[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def frames(T, ob, ctx):
    """render(kind) -> everything the frame leaves behind, as a list of (name, array); and the references, one render per kind."""
    scene = em.scene_of(T, "strip4", committed=True)[0]
    texels, _, R = nm.env_of(7, True)
    env = T.Environment(texels, R)
    lights = T.Emitters(scene, {m: T.RGBSpectrum(*rgb) for m, rgb in em.scene_of(T, "strip4", committed=True)[2].items()})
    integ = T.PathIntegrator(pm.camera(T), T.SeededSampler(3, seed=SEED), 4)
    how = {"path": {}, "env": dict(environment=env, env_scale=0.5), "env-nee": dict(environment=env, env_scale=0.5, env_importance=0.25),
           "emit": dict(emitters=lights, emit_scale=0.5), "emit-hits-only": dict(emitters=lights, emit_scale=0.5, emit_hits_only=True)}

    def render(kind):
        out = [("film", integ.render(scene, **how[kind]).copy()), ("sample radiance", integ.sample_radiance(scene)),
               ("shadow rays", np.array([integ.stats.shadow_rays], np.uint64)), ("batches", np.array([integ.stats.n_batches], np.uint64))]
        if kind.startswith("env"):
            out += [(f"escapes[{k}]", a) for k, a in enumerate(integ.escapes(scene))]
        if kind.startswith("emit"):
            out += [(f"emitted[{k}]", a) for k, a in enumerate(integ.emitted(scene))]
        return out

    refs = {kind: render(kind) for kind in KINDS}
    yield render, refs
    lights.close()
    env.close()


def run_tour(render, refs, n_batches, what):
    order = tour(len(KINDS))
    assert len(order) == 26 and {(a, b) for a, b in zip(order, order[1:])} == {(a, b) for a in range(5) for b in range(5)}, "every ordered pair of kinds is adjacent"
    before = "nothing"
    for step, k in enumerate(order):
        kind = KINDS[k]
        for (name, got), (_, ref) in zip(render(kind), refs[kind]):
            where = f"{what}, frame {step}: {name} of a {kind} frame after {before}"
            if name == "batches":
                assert int(got[0]) == n_batches, where
            elif got.dtype == np.float32:
                assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref)), f"{where}: {int((bits(got) != bits(ref)).sum())} of {got.size} values differ"
            else:
                assert np.array_equal(got, ref), where
        before = kind


def test_the_references_are_frames_of_their_kind(frames):
    """The references differ from one another where the kinds do: a tour that compared equal frames would prove nothing."""
    _, refs = frames
    film = {k: bits(dict(v)["film"]) for k, v in refs.items()}
    rays = {k: int(dict(v)["shadow rays"][0]) for k, v in refs.items()}
    for a in range(len(KINDS)):
        for b in range(a + 1, len(KINDS)):
            assert not np.array_equal(film[KINDS[a]], film[KINDS[b]]), (KINDS[a], KINDS[b])
    assert rays["env"] == rays["path"] == rays["emit-hits-only"], "no lane rays"
    assert rays["env-nee"] > rays["path"] + 500 and rays["emit"] > rays["path"] + 500, "the lane carries rays in both kinds that use it"
    assert (dict(refs["env"])["escapes[1]"] > 0).any() and dict(refs["emit"])["emitted[1]"].sum() > 0 and dict(refs["emit-hits-only"])["emitted[1]"].sum() > 0


def test_every_ordered_pair_of_kinds_on_one_context(frames):
    render, refs = frames
    run_tour(render, refs, 1, "defaults")


def test_every_ordered_pair_of_kinds_on_three_batches_and_two_pipes(frames, ctx):
    """pipelines = 2, batch_paths = 1209 (one sample pass of the 39 x 31 sample pixels), overlap = 0: three batches on two pipes; the films and the records are the same."""
    render, refs = frames
    try:
        for k, v in dict(pipelines=2, batch_paths=1209, overlap=0).items():
            ctx.set_option(k, v)
        run_tour(render, refs, 3, "pipelines=2, batch_paths=1209, overlap=0")
    finally:
        for k, v in dict(pipelines=1, batch_paths=0, overlap=1).items():
            ctx.set_option(k, v)
