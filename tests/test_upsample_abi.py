"""The guided upsampling queries' ABI and Python surface: the parameter struct against its ctypes mirror, the prototypes, the symbols in the
right library only, the status codes, the appended options, _host / _cpu argument parity, rt.upsample as a public submodule whose names
stay off the top level and whose numpy path never loads torch, and what the header says is not covered."""
import ctypes as C
import re
import subprocess
import sys
import types

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, upsample

AMD_NAMES = ("rt_upsample_guided", "rt_upsample_guided_host")
HOST_NAMES = ("rt_upsample_guided_cpu",)
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
HOST_HEADER = (_capi.REPO_ROOT / "include" / "rt_host.h").read_text()
OPTIONS = ("RT_AMD_UPSAMPLE_FORM", "RT_AMD_DIAG_UPSAMPLE_MAX_GROUPS")
PLAIN = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_struct_size_and_offsets_match_the_header():
    body = re.search(r"typedef struct rt_upsample_params \{(.*?)\} rt_upsample_params;", PLAIN, flags=re.S).group(1)
    fields = [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w ]+?[ \*])(\w+);", body)]
    assert fields == [("float", "sigma_normal"), ("float", "sigma_position"), ("uint32_t", "scale"), ("uint32_t", "radius"), ("uint32_t", "flags")]
    P = _capi.UpsampleParams
    assert [f for f, _ in P._fields_] == [name for _, name in fields]
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16] and C.sizeof(P) == 20


def prototype(text, name):
    args = re.search(r"\bint " + name + r"\((.*?)\);", text, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def test_prototypes_and_host_cpu_parity():
    device, host, cpu = prototype(PLAIN, "rt_upsample_guided"), prototype(PLAIN, "rt_upsample_guided_host"), prototype(HOST_HEADER, "rt_upsample_guided_cpu")
    types_of = lambda p: [re.sub(r"\w+$", "", a).strip() for a in p]
    assert types_of(device) == ["const float *", "uint32_t", "const rt_denoise_guides *", "const uint32_t *", "uint32_t", "const rt_denoise_guides *",
                                "const uint32_t *", "uint32_t", "const rt_upsample_params *", "uint32_t", "uint32_t", "float *", "void *"]
    assert device[-1] == "void *hip_stream" and types_of(host) == types_of(device)[:-1] == types_of(cpu)  # the device form without the stream
    strip = lambda p: [re.sub(r"\b[dh]_", "", a) for a in p]
    assert strip(host) == strip(device)[:-1] == strip(cpu)  # and the same names
    amd, hostlib = _capi.amd_lib(), _capi.host_lib()
    pointer, word = C.c_void_p, C.c_uint32
    guides, params = C.POINTER(_capi.DenoiseGuides), C.POINTER(_capi.UpsampleParams)
    expected = [pointer, word, guides, pointer, word, guides, pointer, word, params, word, word, pointer]
    assert amd.rt_upsample_guided.argtypes == expected + [pointer]
    assert amd.rt_upsample_guided_host.argtypes == expected and hostlib.rt_upsample_guided_cpu.argtypes == expected


def test_symbols_are_exported_and_listed_in_the_right_library_only():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and name not in _capi.HOST_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and name not in _capi.AMD_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays
    assert all(name in HOST_HEADER for name in HOST_NAMES)


def test_status_codes_without_a_device():
    """the argument check runs before any device work: the device form and the _host form refuse with the CPU form's code and text"""
    amd, host = _capi.amd_lib(), _capi.host_lib()
    lo, hi, p = _capi.DenoiseGuides(), _capi.DenoiseGuides(), _capi.UpsampleParams(1.0, 1.0, 5, 1, 0)
    args = (None, 3, C.byref(lo), None, 0, C.byref(hi), None, 0, C.byref(p), 4, 4, None)
    assert host.rt_upsample_guided_cpu(*args) == -1 and amd.rt_upsample_guided_host(*args) == -1 and amd.rt_upsample_guided(*args, None) == -1
    assert host.rt_host_last_error().decode() == "rt_upsample_guided_cpu: scale must be 2, 3 or 4"
    assert amd.rt_last_error().decode() == "rt_upsample_guided: scale must be 2, 3 or 4"
    p.scale = 2
    empty = args[:9] + (0, 4, None)
    assert host.rt_upsample_guided_cpu(*empty) == 0 and amd.rt_upsample_guided_host(*empty) == 0 and amd.rt_upsample_guided(*empty, None) == 0


def test_the_options_are_appended_accepted_and_documented():
    amd = _capi.amd_lib()
    integration = (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
    for option in OPTIONS:
        assert option in HEADER and option in integration
        assert amd.rt_set_option(option.encode(), b"1") == 0 and amd.rt_set_option(option.encode(), None) == 0
    kernels_h = (_capi.REPO_ROOT / "homework-18-graphics-raytracer_amd" / "csrc" / "rt_kernels.h").read_text()
    table = re.sub(r"/\*.*?\*/", "", kernels_h[kernels_h.index("#define RT_OPTIONS(X)"):kernels_h.index("#define RT_OPTION_ID")], flags=re.S)
    names = re.findall(r'X\(\s*OPT_\w+\s*,[\s\\]*"(RT_AMD_\w+)"\s*\)', table)
    at = names.index("RT_AMD_DIAG_ADAPTIVE_MAX_GROUPS")  # the last enumerator before this block: nothing moved, these two come after it
    assert names[at + 1:at + 3] == list(OPTIONS) and names[0] == "RT_AMD_RNG_LOOKAHEAD" and at == 25


def test_the_header_states_the_block_and_what_it_does_not_cover():
    start = HEADER.index("---- guided upsampling queries:")
    assert HEADER.index("---- variance-guided filter queries:") < start < HEADER.index("---- diagnostics")
    block = HEADER[start:HEADER.index("---- diagnostics")]
    for words in AMD_NAMES + OPTIONS + ("a = 2 r + 1 - s", "floor(a / 2 s)", "t_y = 1 - fabsf((float)dr - f_y) / (float)R", "w = (t_y * t_x) * e(x)",
                                        "C - C == 0", "a NaN keeps its payload", "rows_lo = ceil(rows / s)", "scale outside 2 .. 4", "radius outside 1 .. 2",
                                        "out == color_lo", "RT_DENOISE_DEMODULATE_IN without low->albedo"):
        assert words in block, words
    not_covered = block[block.rindex("Not covered"):]
    for words in ("rt_multi_*", "ractional", "variance plane", "jitter"):
        assert words in not_covered, words


def test_upsample_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.upsample, types.ModuleType) and rt.upsample is upsample
    assert sorted(upsample.__all__) == sorted(["guided", "guided_numpy", "Guides", "low_frame", "low_rays", "render_upsampled"])
    for name in upsample.__all__:
        assert hasattr(upsample, name) and name not in rt.__all__ and not hasattr(rt, name), name
    assert "upsample" not in rt.__all__
    for other in (rt.film, rt.denoise, rt.temporal, rt.svgf, rt.moving, rt.rectify, rt.materials, rt.adaptive):
        assert "upsample" not in other.__all__


def test_the_numpy_path_leaves_torch_and_hip_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import _capi, upsample\n"
            "low = upsample.low_frame(rt.Frame.full(7, 5, 2), 2)\n"
            "assert (low.width, low.height) == (4, 3)\n"
            "out = upsample.guided_numpy(np.full((12, 3), 0.5, dtype=np.float32), 5, 7, demodulate=False)\n"
            "assert out.shape == (5, 7, 3) and (out == 0.5).all()\n"
            "assert 'torch' not in sys.modules and _capi._amd is None\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
