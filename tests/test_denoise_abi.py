"""The denoise queries' ABI and Python surface: the two structs against their ctypes mirrors, the symbols, and rt.denoise as a public
submodule whose names stay off the top level and whose numpy path never loads torch."""
import ctypes as C
import re
import subprocess
import sys
import types

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, denoise

AMD_NAMES = ("rt_denoise_temp_bytes", "rt_denoise_atrous", "rt_denoise_atrous_host")
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()


def _struct_fields(name):
    """(type, field) of every member of `typedef struct name { ... } name;` in the header, comments removed"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w ]+?[ \*])(\w+);", body)]


def test_struct_sizes_and_offsets_match_the_header():
    pointer, word = C.sizeof(C.c_void_p), 4
    fields = _struct_fields("rt_denoise_guides")
    assert [f for _, f in fields] == [f for f, _ in _capi.DenoiseGuides._fields_]
    offset = 0
    for ctype, field in fields:
        size = pointer if ctype.endswith("*") else word
        assert getattr(_capi.DenoiseGuides, field).offset == offset and getattr(_capi.DenoiseGuides, field).size == size, field
        offset += size
    assert C.sizeof(_capi.DenoiseGuides) == offset == 48
    fields = _struct_fields("rt_denoise_params")
    assert [f for _, f in fields] == [f for f, _ in _capi.DenoiseParams._fields_] == ["sigma_color", "sigma_normal", "sigma_position", "first_level",
                                                                                     "n_levels", "flags"]
    assert [t for t, _ in fields] == ["float"] * 3 + ["uint32_t"] * 3
    for k, (_, field) in enumerate(fields):
        assert getattr(_capi.DenoiseParams, field).offset == 4 * k
    assert C.sizeof(_capi.DenoiseParams) == 24
    assert "#define RT_DENOISE_DEMODULATE_IN 1u" in HEADER and "#define RT_DENOISE_DEMODULATE_OUT 2u" in HEADER and "#define RT_DENOISE_DEMODULATE 3u" in HEADER


def test_symbols_are_exported_and_listed():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and not hasattr(host, name), name
    assert hasattr(host, "rt_denoise_atrous_cpu") and "rt_denoise_atrous_cpu" in _capi.HOST_SYMBOLS and not hasattr(amd, "rt_denoise_atrous_cpu")
    assert amd.rt_abi_version() == 1  # additive: the version stays
    assert amd.rt_denoise_temp_bytes(1080, 1920) == 1080 * 1920 * 12
    for option in ("RT_AMD_DENOISE_FORM", "RT_AMD_DIAG_DENOISE_MAX_GROUPS"):
        assert option in HEADER and option in (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
        assert amd.rt_set_option(option.encode(), b"1") == 0 and amd.rt_set_option(option.encode(), None) == 0


def test_denoise_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.denoise, types.ModuleType) and rt.denoise is denoise
    assert sorted(denoise.__all__) == sorted(["atrous", "atrous_numpy", "temp_bytes", "denoise_frame"])
    for name in denoise.__all__:
        assert callable(getattr(denoise, name)) and name not in rt.__all__ and not hasattr(rt, name), name


def test_the_numpy_path_leaves_torch_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import denoise\n"
            "a = np.full((6, 5, 3), 0.5, dtype=np.float32)\n"
            "out = denoise.atrous_numpy(a, 6, 5, levels=3)\n"
            "assert np.array_equal(out, a)\n"
            "assert 'torch' not in sys.modules\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
