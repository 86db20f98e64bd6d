"""The library calls of the Python binding, pinned call for call without a GPU: tests/golden/make_api_calls.py drives every public host and `_device` method of the
integrators and the image-space passes behind a stand-in for the loaded library, and what it records — entry, argument order, NULL against a pointer, the bytes of every
parameter block, the text of every refusal — must be tests/golden/api_calls.json, which was written from the binding as it stood before its call paths were shared and is
not regenerated from the code under test (see the generator's docstring)."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("make_api_calls", os.path.join(HERE, "golden", "make_api_calls.py"))
make = importlib.util.module_from_spec(spec)
spec.loader.exec_module(make)

with open(make.GOLDEN) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def recorded(T):
    real_lib, real_buffer = T._ffi.lib, T._ffi.DeviceBuffer
    rec = make.record(T)
    assert T._ffi.lib is real_lib and T._ffi.DeviceBuffer is real_buffer, "the stand-ins stayed behind"
    return rec


def test_the_cases_are_the_golden_files(recorded):
    assert sorted(recorded["calls"]) == sorted(GOLDEN["calls"]) == sorted(make.CASES)
    assert sorted(recorded["refusals"]) == sorted(GOLDEN["refusals"])
    assert all(GOLDEN["calls"].values()) and all(GOLDEN["refusals"].values())


@pytest.mark.parametrize("case", sorted(GOLDEN["calls"]))
def test_calls_are_the_parents(recorded, case):
    got, want = recorded["calls"][case], GOLDEN["calls"][case]
    assert [c[0] for c in got] == [c[0] for c in want], "the entries, in order"
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), f"call {k}, {w[0]}: {len(g) - 1} arguments for {len(w) - 1}"
        for j, (a, b) in enumerate(zip(g[1:], w[1:])):
            assert type(a) is type(b) and a == b, f"call {k}, {w[0]}, argument {j}: {a!r}, not {b!r}"


@pytest.mark.parametrize("case", sorted(GOLDEN["refusals"]))
def test_refusals_are_the_parents(recorded, case):
    """Each raised TraceHipError before any call was recorded (make_api_calls.record asserts both); the text is the parent's."""
    assert recorded["refusals"][case] == GOLDEN["refusals"][case]


def test_the_record_covers_host_and_device_entries_and_null_and_given_pointers():
    """What the golden file must hold to pin anything: for every pass both the host entry and its _device twin, and every nullable argument once NULL and once given."""
    entries = {c[0] for calls in GOLDEN["calls"].values() for c in calls}
    for base in ("trhip_render_whitted", "trhip_render_path", "trhip_render_path_map", "trhip_render_path_env", "trhip_path_env_relight", "trhip_render_ao", "trhip_render_sky",
                 "trhip_render_sky_is", "trhip_render_aov", "trhip_render_aov_ids", "trhip_denoise", "trhip_denoise_var", "trhip_upscale", "trhip_display", "trhip_temporal",
                 "trhip_temporal_clip", "trhip_temporal_moments", "trhip_temporal_motion", "trhip_temporal_clip_motion", "trhip_temporal_split", "trhip_temporal_upsample",
                 "trhip_temporal_upsample_motion", "trhip_film_add"):
        assert base in entries and base + "_device" in entries, base
    nullable = {"trhip_temporal": [3], "trhip_temporal_device": [3], "trhip_temporal_clip": [3], "trhip_temporal_clip_device": [3], "trhip_temporal_moments": [3, 4],
                "trhip_temporal_moments_device": [3, 4], "trhip_temporal_motion": [3, 5, 6], "trhip_temporal_motion_device": [3, 5, 6], "trhip_temporal_clip_motion": [3, 4, 5, 6],
                "trhip_temporal_clip_motion_device": [3, 4, 5, 6], "trhip_temporal_split": [2, 4, 5, 6, 7], "trhip_temporal_split_device": [2, 4, 5, 6, 7],
                "trhip_temporal_upsample": [6], "trhip_temporal_upsample_device": [6, 12], "trhip_temporal_upsample_motion": [6, 7, 8, 9],
                "trhip_temporal_upsample_motion_device": [6, 7, 8, 9, 15], "trhip_upscale_device": [10], "trhip_display": [6, 8], "trhip_display_device": [6, 8],
                "trhip_denoise_var_device": [8]}
    for entry, positions in nullable.items():
        calls = [c for cs in GOLDEN["calls"].values() for c in cs if c[0] == entry]
        for p in positions:  # (c[0] is the entry: argument k of the C call is c[k + 1])
            seen = {c[p + 1] is None for c in calls}
            assert seen == {True, False}, f"{entry}: argument {p} is {'always' if seen == {True} else 'never'} NULL in the record"
