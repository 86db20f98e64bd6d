"""trhip_set_option on the MI355X: every option takes its default, every refusal keeps its text and its code, and Context.has_option agrees with trhip_option_in_build.
The module has a context of its own, so the session context's options stay as they are; nothing here launches a kernel."""

import pytest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
NEEDS = "needs the EXPERIMENTS build of the library (-DTRHIP_EXPERIMENTS): not in the default binary"

# every option with the value a new context holds for it (csrc/th_options.h; INTEGRATION.md's tables for the ones listed there)
DEFAULTS = {
    "count_visits": 0, "timing": 1, "batch_paths": 0, "pipelines": 1, "debug_trace_budget": 0, "bvh_builder": -1, "occluder_pretest": 1,
    "stream2_priority": -1, "leaf_kernel": 1, "slab_margin_log2": 14, "band_tile_rows": 0, "tiny_scene_prims": 16, "film_relayout": 1,
    "any_on_accelerator": -1, "wide4": 1, "leaf_queue": 0, "node_layout": 0, "overlap": 1, "compose_spheres": -1, "traversal": 3,
    "leaf_sorted": 0, "film_fused": 1, "trace3_spec": 1, "hybrid": 1, "trace7_cheap": 1, "streaming": 0, "stream_budget_shift": 12, "stream_list_cap": 0,
    "stream_budget_min": 2048, "sppm_batch": 0, "denoise_lds": 3, "temporal_patch": 1, "denoise_var_lds": 3,
}
# the values only the EXPERIMENTS build carries, with the start of the default binary's answer
EXPERIMENTS = [("traversal", 4, "traversal 4 "), ("traversal", 6, "traversal 6 "), ("traversal", 7, "traversal 7 "), ("leaf_queue", 1, "leaf_queue "), ("leaf_sorted", 1, "leaf_sorted "),
               ("bvh_builder", 1, "bvh_builder = 1 (the linear BVH) ")]
REFUSALS = [
    ("node_layout", -1, "node_layout: 0 (depth-first) or 1 (sibling pairs per 128-byte line)"),
    ("node_layout", 2, "node_layout: 0 (depth-first) or 1 (sibling pairs per 128-byte line)"),
    ("pipelines", 0, "pipelines must be in 1..8"),
    ("pipelines", 9, "pipelines must be in 1..8"),
    ("batch_paths", -1, "batch_paths must be >= 0 (0 = auto)"),
    ("traversal", 0, "traversal must be 1, 2, 3, 4, 6 or 7"),
    ("traversal", 5, "traversal must be 1, 2, 3, 4, 6 or 7"),
    ("traversal", 8, "traversal must be 1, 2, 3, 4, 6 or 7"),
    ("no_such_option", 1, "unknown option no_such_option"),
]


@pytest.fixture(scope="module")
def own(T):
    c = T.Context(0)
    yield c
    c.close()


def set_raw(T, c, name, value):
    lib = T.lib()
    rc = lib.trhip_set_option(c._h, name.encode(), int(value))
    return rc, lib.trhip_last_error(c._h).decode()


def test_every_option_accepts_its_default(T, own):
    for name, value in DEFAULTS.items():
        rc, msg = set_raw(T, own, name, value)
        assert rc == 0, (name, value, rc, msg)


@pytest.mark.parametrize("name,value,text", REFUSALS)
def test_refusals_keep_text_and_code(T, own, name, value, text):
    rc, msg = set_raw(T, own, name, value)
    assert (rc, msg) == (INVALID, text)


def test_null_arguments(T, own):
    lib = T.lib()
    assert lib.trhip_set_option(own._h, None, 1) == INVALID
    assert lib.trhip_last_error(own._h).decode() == "null argument"
    assert lib.trhip_set_option(None, b"timing", 1) == INVALID


@pytest.mark.parametrize("name,value,start", EXPERIMENTS)
def test_experiments_values(T, own, name, value, start):
    """A value of the EXPERIMENTS build: has_option is trhip_option_in_build's answer, and the default binary refuses it as UNSUPPORTED with its own sentence."""
    lib = T.lib()
    in_build = bool(lib.trhip_option_in_build(name.encode(), value))
    try:
        assert own.has_option(name, value) == in_build
        rc, msg = set_raw(T, own, name, value)
        if in_build:
            assert rc == 0, msg
        else:
            assert (rc, msg) == (UNSUPPORTED, start + NEEDS)
    finally:
        own.set_option(name, DEFAULTS[name])
    # the same options' other values exist in every build
    assert lib.trhip_option_in_build(name.encode(), DEFAULTS[name]) == 1
    assert own.has_option(name, DEFAULTS[name])
