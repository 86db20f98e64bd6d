"""csrc/th_options.h on the CPU: the option table and apply_option, driven through tests/host/options_main.cpp, against the rules of trhip_set_option written down here
once more, independently: every option, a ladder of values around every bound and past 32 bits, in the default and in the EXPERIMENTS build."""

import os
import re
import subprocess

import pytest

import host_programs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
NEEDS = "needs the EXPERIMENTS build of the library (-DTRHIP_EXPERIMENTS): not in the default binary"
VALUES = [-2**40, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 20, 21, 31, 32, 255, 256, 2**31, 2**32 + 5]
NO_MAX = 2**63 - 1


def i32(v):  # (int)v
    v &= 0xFFFFFFFF
    return v - 2**32 if v >= 2**31 else v


def u32(v):  # (uint32_t)v
    return v & 0xFFFFFFFF


def same(v):  # (uint64_t) of a value >= 0
    return v


def ok(v):
    return (0, v, "")


def flag(v, exp):
    return ok(int(v != 0))


def tri(v, exp):
    return ok(-1 if v < 0 else int(v != 0))


def clamp(lo, hi, cast):
    return lambda v, exp: ok(cast(max(lo, min(hi, v))))


def mask3(v, exp):
    return ok(v & 3)


def experiments_flag(name):
    return lambda v, exp: (UNSUPPORTED, None, f"{name} {NEEDS}") if v != 0 and not exp else ok(int(v != 0))


def bvh_builder(v, exp):
    if v == 1 and not exp:
        return (UNSUPPORTED, None, f"bvh_builder = 1 (the linear BVH) {NEEDS}")
    return ok(-1 if v < 0 else 4 if v > 4 else v)


def node_layout(v, exp):
    return ok(v) if 0 <= v <= 1 else (INVALID, None, "node_layout: 0 (depth-first) or 1 (sibling pairs per 128-byte line)")


def pipelines(v, exp):
    return ok(v) if 1 <= v <= 8 else (INVALID, None, "pipelines must be in 1..8")


def batch_paths(v, exp):
    return ok(v) if v >= 0 else (INVALID, None, "batch_paths must be >= 0 (0 = auto)")


def traversal(v, exp):
    if v < 1 or v > 7 or v == 5:
        return (INVALID, None, "traversal must be 1, 2, 3, 4, 6 or 7")
    if v in (4, 6, 7) and not exp:
        return (UNSUPPORTED, None, f"traversal {v} {NEEDS}")
    return ok(v)


# name -> (rule, a value the option takes that is not its default: what the field holds before the value under test is applied)
RULES = {
    **{n: (flag, p) for n, p in (("count_visits", 1), ("timing", 0), ("hybrid", 0), ("occluder_pretest", 0), ("film_fused", 0), ("trace3_spec", 0),
                                 ("trace7_cheap", 0), ("leaf_kernel", 0), ("film_relayout", 0), ("wide4", 0), ("overlap", 0),
                                 ("temporal_patch", 0))},
    "leaf_sorted": (experiments_flag("leaf_sorted"), 1),
    "leaf_queue": (experiments_flag("leaf_queue"), 1),
    "streaming": (tri, 1), "compose_spheres": (tri, 1), "any_on_accelerator": (tri, 1),
    "stream_budget_shift": (clamp(0, 31, u32), 3), "slab_margin_log2": (clamp(0, 20, i32), 3), "tiny_scene_prims": (clamp(0, 255, u32), 3),
    "bvh_builder": (bvh_builder, 2),
    "stream_list_cap": (clamp(0, NO_MAX, u32), 77), "sppm_batch": (clamp(0, NO_MAX, same), 77), "band_tile_rows": (clamp(0, NO_MAX, i32), 77),
    "stream_budget_min": (clamp(1, NO_MAX, u32), 77),
    "denoise_lds": (mask3, 1), "denoise_var_lds": (mask3, 1),
    "debug_trace_budget": (lambda v, exp: ok(u32(v)), 77), "stream2_priority": (lambda v, exp: ok(i32(v)), 77),
    "node_layout": (node_layout, 1), "pipelines": (pipelines, 2), "batch_paths": (batch_paths, 77), "traversal": (traversal, 2),
}
# names the table does not hold: one that never was an option, and the film-pass variants that lost their measurements and went with their kernels (docs/design/04-kernels.md)
UNKNOWN = ("no_such_option", "film_block", "film_tiled", "film_transpose", "film_swizzle")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_programs.build("options_main.cpp", tmp_path_factory.mktemp("options"))


def test_rows_are_the_documented_options(program):
    """The table's names: the first column of INTEGRATION.md's two option tables and the four options those tables leave out."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("| name | default | meaning |"):text.index("## Building")]
    documented = set()
    for line in section.splitlines():
        if line.startswith("| `"):
            documented.update(re.findall(r"`(\w+)`", line.split("|")[1]))
    documented |= {"trace3_spec", "denoise_lds", "denoise_var_lds", "temporal_patch"}
    names = subprocess.run([program, "names"], capture_output=True, text=True, check=True).stdout.split()
    assert len(names) == len(set(names))
    assert set(names) == documented
    assert set(names) == set(RULES)


@pytest.mark.parametrize("experiments", [False, True])
def test_every_option_follows_its_rule(program, experiments):
    cases = [(name, prime, v) for name, (_, prime) in RULES.items() for v in VALUES]
    cases += [(name, 0, v) for name in UNKNOWN for v in (0, 1)]
    fed = "".join(f"{n} {p} {v}\n" for n, p, v in cases)
    done = subprocess.run([program, str(int(experiments))], input=fed, capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr
    lines = done.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for (name, prime, v), line in zip(cases, lines):
        rc, before, after, msg = line.split("\t")
        if name in UNKNOWN:
            assert (int(rc), before, after, msg) == (INVALID, "-", "-", f"unknown option {name}")
            continue
        want_rc, want, want_msg = RULES[name][0](v, experiments)
        assert int(before) == RULES[name][0](prime, True)[1], (name, prime)
        assert int(rc) == want_rc and msg == want_msg, (name, v, line)
        if want_rc == 0:
            assert int(after) == want, (name, v, line)
        else:
            assert after == before, f"{name} = {v}: a refused call changed the field ({line})"
