"""The variance-guided filter queries' ABI and Python surface: the two structs against their ctypes mirrors, the symbols, the two options,
and rt.svgf as a public submodule whose names stay off the top level and whose numpy path never loads torch."""
import ctypes as C
import re
import subprocess
import sys
import types

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, svgf

AMD_NAMES = ("rt_svgf_variance", "rt_svgf_temp_bytes", "rt_svgf_atrous", "rt_svgf_variance_host", "rt_svgf_atrous_host")
HOST_NAMES = ("rt_svgf_variance_cpu", "rt_svgf_atrous_cpu")
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()


def _struct_fields(name):
    """(type, field) of every member of `typedef struct name { ... } name;` in the header, comments removed"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    return [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w ]+?[ \*])(\w+);", body)]


def _check(name, mirror, names, types_, size):
    fields = _struct_fields(name)
    assert [f for _, f in fields] == [f for f, _ in mirror._fields_] == names
    assert [t for t, _ in fields] == types_
    for k, (_, field) in enumerate(fields):
        assert getattr(mirror, field).offset == 4 * k and getattr(mirror, field).size == 4, field
    assert C.sizeof(mirror) == size == 4 * len(fields)


def test_struct_sizes_and_offsets_match_the_header():
    _check("rt_svgf_variance_params", _capi.SvgfVarianceParams, ["sigma_normal", "sigma_position", "min_length", "flags"], ["float"] * 2 + ["uint32_t"] * 2, 16)
    _check("rt_svgf_atrous_params", _capi.SvgfAtrousParams, ["sigma_luminance", "sigma_normal", "sigma_position", "first_level", "n_levels", "flags"],
           ["float"] * 3 + ["uint32_t"] * 3, 24)
    assert C.sizeof(_capi.DenoiseGuides) == 48 and C.sizeof(_capi.TemporalPixel) == 32  # reused as they are


def test_symbols_are_exported_and_listed():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays
    assert [amd.rt_svgf_temp_bytes(1080, 1920, k) for k in (1, 2, 5)] == [0, 1080 * 1920 * 16, 1080 * 1920 * 20]
    for option in ("RT_AMD_SVGF_FORM", "RT_AMD_DIAG_SVGF_MAX_GROUPS"):
        assert option in HEADER and option in (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
        assert amd.rt_set_option(option.encode(), b"1") == 0 and amd.rt_set_option(option.encode(), None) == 0


def test_svgf_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.svgf, types.ModuleType) and rt.svgf is svgf
    assert sorted(svgf.__all__) == sorted(["variance", "atrous", "variance_numpy", "atrous_numpy", "temp_bytes", "filter_frame"])
    for name in svgf.__all__:
        assert callable(getattr(svgf, name)) and name not in rt.__all__ and not hasattr(rt, name), name
    assert svgf.SIGMA_LUMINANCE == 4.0 and svgf.MIN_LENGTH == 4


def test_the_numpy_path_leaves_torch_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import svgf, temporal\n"
            "a = np.full((6, 5, 3), 0.5, dtype=np.float32)\n"
            "h = np.zeros(30, dtype=temporal.HISTORY_DTYPE)\n"
            "h['color'], h['moment1'], h['moment2'], h['length'] = 0.5, 0.5, 0.25, 1\n"
            "v = svgf.variance_numpy(h, 6, 5)\n"
            "assert not v.any()\n"
            "out, var = svgf.atrous_numpy(h['color'], v, 6, 5, levels=3)\n"
            "assert np.array_equal(out, a) and not var.any()\n"
            "assert 'torch' not in sys.modules\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
