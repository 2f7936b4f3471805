"""The temporal queries' ABI and Python surface: the three structs against their ctypes mirrors and the header text, the symbols, the
option, rt.temporal as a public submodule whose names stay off the top level and whose numpy path never loads torch, and every refusal
of the one argument check, in the stated order, behind all six entry points."""
import ctypes as C
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, temporal

AMD_NAMES = ("rt_temporal_motion", "rt_temporal_accumulate", "rt_temporal_motion_host", "rt_temporal_accumulate_host")
HOST_NAMES = ("rt_temporal_motion_cpu", "rt_temporal_accumulate_cpu")
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
OPTION = "RT_AMD_DIAG_TEMPORAL_MAX_GROUPS"


def _struct_fields(name):
    """(type, field, count) of every member of `typedef struct name { ... } name;` in the header, comments removed"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    return [(m.group(1).strip(), m.group(2), int(m.group(3) or 1)) for m in re.finditer(r"([\w ]+?[ \*])(\w+)(?:\[(\d+)\])?;", body)]


def _check_layout(name, mirror, total):
    fields = _struct_fields(name)
    assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_]
    offset = 0
    for ctype, field, count in fields:
        size = (C.sizeof(C.c_void_p) if ctype.endswith("*") else 4) * count
        assert ctype.endswith("*") or ctype in ("float", "uint32_t"), ctype
        assert getattr(mirror, field).offset == offset and getattr(mirror, field).size == size, field
        offset += size
    assert C.sizeof(mirror) == offset == total
    return fields


def test_struct_sizes_and_offsets_match_the_header():
    fields = _check_layout("rt_temporal_pixel", _capi.TemporalPixel, 32)
    assert [(t, f, c) for t, f, c in fields] == [("float", "color", 3), ("float", "moment1", 1), ("float", "moment2", 1), ("uint32_t", "length", 1),
                                                 ("uint32_t", "reserved", 2)]
    _check_layout("rt_temporal_guides", _capi.TemporalGuides, 48)
    fields = _check_layout("rt_temporal_params", _capi.TemporalParams, 20)
    assert [f for _, f, _ in fields] == ["normal_min", "position_max", "alpha_min", "max_length", "flags"]
    assert temporal.HISTORY_DTYPE.itemsize == 32
    for name in ("color", "moment1", "moment2", "length", "reserved"):
        assert temporal.HISTORY_DTYPE.fields[name][1] == getattr(_capi.TemporalPixel, name).offset, name


def test_symbols_are_exported_and_listed_in_the_right_library_only():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and name not in _capi.HOST_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and name not in _capi.AMD_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays


def test_the_option_is_accepted_and_documented():
    amd = _capi.amd_lib()
    assert OPTION in HEADER and OPTION in (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
    assert amd.rt_set_option(OPTION.encode(), b"1") == 0 and amd.rt_set_option(OPTION.encode(), None) == 0


def test_temporal_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.temporal, types.ModuleType) and rt.temporal is temporal
    assert sorted(temporal.__all__) == sorted(["motion", "motion_numpy", "accumulate", "accumulate_numpy", "HISTORY_DTYPE", "Guides", "History",
                                               "accumulate_frame"])
    for name in temporal.__all__:
        assert hasattr(temporal, name) and name not in rt.__all__ and not hasattr(rt, name), name
    assert "temporal" not in rt.__all__


def test_the_numpy_path_leaves_torch_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import temporal\n"
            "frame = rt.Frame.full(5, 6, 3)\n"
            "position = np.full((30, 3), 0.5, dtype=np.float32)\n"
            "m = temporal.motion_numpy(position, rt.reference_camera(), frame)\n"
            "image = np.full((6, 5, 3), 0.5, dtype=np.float32)\n"
            "h, v = temporal.accumulate_numpy(image, m, 6, 5, np.zeros(30, dtype=temporal.HISTORY_DTYPE))\n"
            "assert (h['length'] == 1).all() and not v.any() and np.array_equal(h['color'], image)\n"
            "assert 'torch' not in sys.modules\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr


# ---- refusals: the one check of rt_temporal.h behind the CPU forms and, before any device work, the four entry points of librt_amd.so ----

A, B, M, H0, H1 = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4, 5))  # never dereferenced: every call below is refused on its arguments
INVALID, UNSUPPORTED = -1, -5


def _good():
    return _capi.TemporalGuides(), _capi.TemporalGuides(), _capi.TemporalParams(0.9, 0.1, 0.05, 32, 0)


def _accumulate(entry, color, motion, cur, prev, p, rows, cols, h_in, h_out):
    ref = lambda s: C.byref(s) if s is not None else None
    args = (color, motion, ref(cur), ref(prev), ref(p), rows, cols, h_in, h_out, None)
    if entry == "cpu":
        lib = _capi.host_lib()
        return lib.rt_temporal_accumulate_cpu(*args), lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    if entry == "device":
        return lib.rt_temporal_accumulate(*args, None), lib.rt_last_error().decode()
    return lib.rt_temporal_accumulate_host(*args), lib.rt_last_error().decode()


def _accumulate_cases():
    def with_(which, **kw):
        cur, prev, p = _good()
        for k, v in kw.items():
            setattr({"cur": cur, "prev": prev, "p": p}[which], k, v)
        return cur, prev, p

    # in the stated order: each case also carries every LATER fault it can, so the message shows which check came first
    late = dict(max_length=0, alpha_min=2.0, flags=1)
    yield "2^32 pixels", UNSUPPORTED, (None, None, None, None, None, 1 << 16, 1 << 16, None, None), "rows * cols"
    yield "null current", INVALID, (A, M, None, _good()[1], _good()[2], 4, 4, H0, H1), "current"
    yield "null previous", INVALID, (A, M, _good()[0], None, _good()[2], 4, 4, H0, H1), "previous"
    yield "null params", INVALID, (A, M, _good()[0], _good()[1], None, 4, 4, H0, H1), "params"
    yield "null color", INVALID, (None, M, *with_("p", **late), 4, 4, H0, H0), "color"
    yield "null motion", INVALID, (A, None, *with_("p", **late), 4, 4, H0, H0), "motion"
    yield "null history_in", INVALID, (A, M, *with_("p", **late), 4, 4, None, H1), "history_in"
    yield "null history_out", INVALID, (A, M, *with_("p", **late), 4, 4, H0, None), "history_out"
    yield "normal stride", INVALID, (A, M, *with_("cur", normal=4096, normal_stride=2), 4, 4, H0, H0), "current: normal_stride"
    yield "position stride", INVALID, (A, M, *with_("prev", position=4096, position_stride=0), 4, 4, H0, H0), "previous: position_stride"
    yield "object stride", INVALID, (A, M, *with_("cur", object=4096, object_stride=0), 4, 4, H0, H0), "current: object_stride"
    yield "valid stride", INVALID, (A, M, *with_("prev", valid=4096, valid_stride=0), 4, 4, H0, H0), "previous: valid_stride"
    yield "out is in", INVALID, (A, M, *with_("p", **late), 4, 4, H0, H0), "history_out must not be history_in"
    yield "max_length", INVALID, (A, M, *with_("p", **late), 4, 4, H0, H1), "max_length"
    yield "alpha_min above", INVALID, (A, M, *with_("p", alpha_min=1.5, position_max=-1.0, flags=1), 4, 4, H0, H1), "alpha_min"
    yield "alpha_min nan", INVALID, (A, M, *with_("p", alpha_min=float("nan")), 4, 4, H0, H1), "alpha_min"
    yield "position_max", INVALID, (A, M, *with_("p", position_max=-1.0, flags=1), 4, 4, H0, H1), "position_max"
    yield "position_max nan", INVALID, (A, M, *with_("p", position_max=float("nan")), 4, 4, H0, H1), "position_max"
    yield "flags", INVALID, (A, M, *with_("p", flags=1), 4, 4, H0, H1), "flags"
    yield "normal in one set", INVALID, (A, M, *with_("cur", normal=4096, normal_stride=3), 4, 4, H0, H1), "normal: a plane in one"
    yield "position in one set", INVALID, (A, M, *with_("prev", position=4096, position_stride=3), 4, 4, H0, H1), "position: a plane in one"
    yield "object in one set", INVALID, (A, M, *with_("cur", object=4096, object_stride=1), 4, 4, H0, H1), "object: a plane in one"


ACCUMULATE_CASES = [(e, c) for e in ("cpu", "device", "host") for c in _accumulate_cases()]


@pytest.mark.parametrize("entry,case", ACCUMULATE_CASES, ids=[f"{e}-{c[0]}" for e, c in ACCUMULATE_CASES])
def test_accumulate_refusals_return_their_status_and_message_in_order(entry, case):
    _, want, args, word = case
    status, text = _accumulate(entry, *args)
    who = {"cpu": "rt_temporal_accumulate_cpu", "device": "rt_temporal_accumulate", "host": "rt_temporal_accumulate_host"}[entry]
    assert status == want and text.startswith(who + ": ") and word in text, (status, text)


def test_the_device_form_alone_refuses_an_unaligned_history():
    cur, prev, p = _good()
    status, text = _accumulate("device", A, M, cur, prev, p, 4, 4, C.c_void_p(4096 + 8), H1)
    assert status == INVALID and "16-byte aligned" in text


def _motion(entry, position, p_stride, valid, v_stride, camera, frame, out):
    ref = lambda s: C.byref(s) if s is not None else None
    args = (position, p_stride, valid, v_stride, ref(camera), ref(frame), out)
    if entry == "cpu":
        lib = _capi.host_lib()
        return lib.rt_temporal_motion_cpu(*args), lib.rt_host_last_error().decode()
    lib = _capi.amd_lib()
    if entry == "device":
        return lib.rt_temporal_motion(*args, None), lib.rt_last_error().decode()
    return lib.rt_temporal_motion_host(*args), lib.rt_last_error().decode()


def _motion_cases():
    cam, full = rt.reference_camera(), rt.Frame.full(8, 6, 3)
    tile, stepped, huge = rt.Frame.full(8, 6, 3), rt.Frame.full(8, 6, 3), rt.Frame.full(1 << 16, 1 << 16, 3)
    tile.x0 = 1
    stepped.y_step = 2
    yield "null camera", INVALID, (A, 3, None, 0, None, full, M), "prev_camera"
    yield "null frame", INVALID, (A, 3, None, 0, cam, None, M), "prev_frame"
    yield "a tile", INVALID, (None, 3, None, 0, cam, tile, M), "full frame"
    yield "a stepped frame", INVALID, (None, 3, None, 0, cam, stepped, M), "full frame"
    yield "2^32 pixels", UNSUPPORTED, (None, 3, None, 0, cam, huge, None), "rows * cols"
    yield "null position", INVALID, (None, 2, None, 0, cam, full, None), "position pointer"
    yield "null motion", INVALID, (A, 2, None, 0, cam, full, None), "motion pointer"
    yield "position stride", INVALID, (A, 2, B, 0, cam, full, M), "position_stride"
    yield "valid stride", INVALID, (A, 3, B, 0, cam, full, M), "valid_stride"


MOTION_CASES = [(e, c) for e in ("cpu", "device", "host") for c in _motion_cases()]


@pytest.mark.parametrize("entry,case", MOTION_CASES, ids=[f"{e}-{c[0]}" for e, c in MOTION_CASES])
def test_motion_refusals_return_their_status_and_message_in_order(entry, case):
    _, want, args, word = case
    status, text = _motion(entry, *args)
    who = {"cpu": "rt_temporal_motion_cpu", "device": "rt_temporal_motion", "host": "rt_temporal_motion_host"}[entry]
    assert status == want and text.startswith(who + ": ") and word in text, (status, text)


def test_an_empty_image_is_ok_and_the_wrappers_raise():
    cur, prev, p = _good()
    empty = rt.Frame.full(0, 7, 3)
    for entry in ("cpu", "device", "host"):
        assert _accumulate(entry, None, None, None, None, None, 0, 7, None, None)[0] == 0
        assert _motion(entry, None, 0, None, 0, rt.reference_camera(), empty, None)[0] == 0
    image = np.full((6, 5, 3), 0.5, dtype=np.float32)
    m = np.zeros((6, 5, 2), dtype=np.float32)
    h = np.zeros(30, dtype=temporal.HISTORY_DTYPE)
    with pytest.raises(rt.RtError, match="max_length"):
        temporal.accumulate_numpy(image, m, 6, 5, h, max_length=0)
    with pytest.raises(rt.RtError, match="normal: a plane in one"):
        temporal.accumulate_numpy(image, m, 6, 5, h, current=temporal.Guides(normal=image))
    with pytest.raises(ValueError, match="history"):
        temporal.accumulate_numpy(image, m, 6, 5, h[:29])
    with pytest.raises(ValueError, match="motion"):
        temporal.accumulate_numpy(image, image, 6, 5, h)
    with pytest.raises(ValueError, match="full frame"):
        tile = rt.Frame.full(5, 6, 3)
        tile.y0 = 2
        temporal.motion_numpy(image, rt.reference_camera(), tile)
