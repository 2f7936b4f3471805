"""The history rectification queries' ABI and Python surface: the two structs against their ctypes mirrors and numpy dtype, the symbols
in the right library only, the appended option, rt.rectify as a public submodule whose names stay off the top level and whose numpy
path never loads torch, History.push's new keywords, and the header's pointers where the blocks used to say "not covered"."""
import ctypes as C
import inspect
import re
import subprocess
import sys
import types

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, rectify, temporal

AMD_NAMES = ("rt_temporal_bounds", "rt_temporal_accumulate_bounded", "rt_temporal_feedback", "rt_temporal_bounds_host",
             "rt_temporal_accumulate_bounded_host", "rt_temporal_feedback_host")
HOST_NAMES = ("rt_temporal_bounds_cpu", "rt_temporal_accumulate_bounded_cpu", "rt_temporal_feedback_cpu")
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
OPTION = "RT_AMD_DIAG_RECTIFY_MAX_GROUPS"


def _struct_fields(name):
    """(type, field, array length or None) of every member of `typedef struct name { ... } name;` in the header, comments removed"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    return [(m.group(1).strip(), m.group(2), int(m.group(3)) if m.group(3) else None) for m in re.finditer(r"([\w ]+?[ \*])(\w+)(?:\[(\d+)\])?;", body)]


def test_struct_sizes_and_offsets_match_the_header():
    assert _struct_fields("rt_temporal_box") == [("float", "lo", 4), ("float", "hi", 4)]
    assert [(f, t._length_) for f, t in _capi.TemporalBox._fields_] == [("lo", 4), ("hi", 4)]
    assert (_capi.TemporalBox.lo.offset, _capi.TemporalBox.hi.offset, C.sizeof(_capi.TemporalBox)) == (0, 16, 32)
    assert rectify.BOX_DTYPE.itemsize == 32 and rectify.BOX_DTYPE.names == ("lo", "hi") and rectify.BOX_DTYPE.fields["hi"][1] == 16
    assert _struct_fields("rt_bounds_params") == [("float", "gamma", None), ("uint32_t", "radius", None), ("uint32_t", "flags", None)]
    assert [f for f, _ in _capi.BoundsParams._fields_] == ["gamma", "radius", "flags"]
    assert [getattr(_capi.BoundsParams, f).offset for f, _ in _capi.BoundsParams._fields_] == [0, 4, 8] and C.sizeof(_capi.BoundsParams) == 12
    assert C.sizeof(_capi.TemporalPixel) == 32 and C.sizeof(_capi.TemporalGuides) == 48 and C.sizeof(_capi.TemporalParams) == 20  # reused as they are


def test_symbols_are_exported_and_listed_in_the_right_library_only():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and name not in _capi.HOST_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and name not in _capi.AMD_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays
    host_header = (_capi.REPO_ROOT / "include" / "rt_host.h").read_text()
    assert all(name in host_header for name in HOST_NAMES)


def test_the_option_is_appended_accepted_and_documented():
    amd = _capi.amd_lib()
    assert OPTION in HEADER and OPTION in (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
    assert amd.rt_set_option(OPTION.encode(), b"1") == 0 and amd.rt_set_option(OPTION.encode(), None) == 0
    kernels_h = (_capi.REPO_ROOT / "homework-18-graphics-raytracer_amd" / "csrc" / "rt_kernels.h").read_text()
    names = re.findall(r'X\(OPT_\w+, "(RT_AMD_\w+)"\)', kernels_h)
    assert names[-1] == OPTION and names[-2] == "RT_AMD_DIAG_MOTION_MAX_GROUPS"  # no existing enumerator moved


def test_the_header_states_the_block_and_points_to_it():
    start = HEADER.index("---- history rectification queries:")
    assert HEADER.index("---- temporal queries:") < start < HEADER.index("---- variance-guided filter queries:")
    block = HEADER[start:HEADER.index("---- variance-guided filter queries:")]
    for words in AMD_NAMES + ("rtdm::f_sqrt", "vpos", "-inf", "a NaN bound compares false", "M2' = M2 + (M1' * M1' - M1 * M1)", "clamped_length > max_length",
                              "radius outside 1 .. 3", "Not covered:", OPTION):
        assert words in block, words
    temporal_block = HEADER[HEADER.index("---- temporal queries:"):start]
    svgf_block = HEADER[HEADER.index("---- variance-guided filter queries:"):HEADER.index("---- diagnostics")]
    for text in (temporal_block, svgf_block):
        not_covered = text[text.rindex("Not covered"):]
        assert "colour box" not in not_covered and "feedback" not in not_covered
        assert "history rectification queries" in text


def test_rectify_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.rectify, types.ModuleType) and rt.rectify is rectify
    assert sorted(rectify.__all__) == sorted(["bounds", "bounds_numpy", "accumulate_bounded", "accumulate_bounded_numpy", "feedback", "feedback_numpy",
                                              "BOX_DTYPE", "GAMMA", "RADIUS", "CLAMPED_LENGTH", "filter_frame"])
    for name in rectify.__all__:
        assert hasattr(rectify, name) and name not in rt.__all__ and not hasattr(rt, name), name
    assert "rectify" not in rt.__all__
    assert rectify.RADIUS in (1, 2, 3) and rectify.GAMMA >= 0 and 0 < rectify.CLAMPED_LENGTH <= temporal.MAX_LENGTH
    push = inspect.signature(temporal.History.push).parameters
    assert (push["box"].default, push["clamped_length"].default, push["clamped"].default) == (None, 0, None)


def test_filter_frame_refuses_demodulation_before_it_does_anything():
    """the records' moments are of the colour as accumulated; a level 0 that is fed back cannot leave the filter demodulated"""
    import pytest

    with pytest.raises(ValueError, match="demodulate"):
        rectify.filter_frame(None, None, None, None, None, demodulate=True)
    assert "demodulate" in rectify.filter_frame.__doc__


def test_the_numpy_path_leaves_torch_and_hip_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import _capi, rectify, temporal\n"
            "c = np.full((6, 5, 3), 0.5, dtype=np.float32)\n"
            "box = rectify.bounds_numpy(c, 6, 5)\n"
            "assert (box['lo'] == 0.5).all() and (box['hi'] == 0.5).all()\n"
            "m = np.stack(np.meshgrid(np.arange(5), np.arange(6)), axis=-1).astype(np.float32)\n"
            "h = np.zeros(30, dtype=temporal.HISTORY_DTYPE)\n"
            "h['color'], h['moment1'], h['moment2'], h['length'] = 0.75, 0.75, 0.5625, 3\n"
            "out, var, clamped = rectify.accumulate_bounded_numpy(c, m, 6, 5, h, box)\n"
            "assert (clamped == 4).all() and (out['length'] == 4).all() and (out['color'] == 0.5).all()\n"
            "fed = rectify.feedback_numpy(c * 2, out, 6, 5)\n"
            "assert (fed['color'] == 1.0).all() and (fed['length'] == 4).all()\n"
            "assert 'torch' not in sys.modules and _capi._amd is None\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
