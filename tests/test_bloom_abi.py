"""The bloom queries' ABI and Python surface: the parameter struct against its ctypes mirror, the prototypes, the symbols in the right
library only, every refusal in the order the header states with the same code and text from all three forms, the empty image, the
temp-size helper, the appended options, the header block's position and what it says is not covered, rt.bloom as a public submodule
whose names stay off the top level and whose numpy path never loads torch or the device library."""
import ctypes as C
import math
import re
import subprocess
import sys
import types

import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, bloom
import _bloom_support as S

AMD_NAMES = ("rt_bloom_temp_bytes", "rt_bloom", "rt_bloom_host")
HOST_NAMES = ("rt_bloom_cpu",)
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
HOST_HEADER = (_capi.REPO_ROOT / "include" / "rt_host.h").read_text()
OPTIONS = ("RT_AMD_BLOOM_FORM", "RT_AMD_DIAG_BLOOM_MAX_GROUPS")
PLAIN = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
INVALID = -1


def test_struct_size_and_offsets_match_the_header():
    body = re.search(r"typedef struct rt_bloom_params \{(.*?)\} rt_bloom_params;", PLAIN, flags=re.S).group(1)
    fields = [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w ]+?[ \*])(\w+);", body)]
    assert fields == [("float", "threshold"), ("float", "knee"), ("float", "intensity"), ("uint32_t", "n_levels")]
    P = _capi.BloomParams
    assert [f for f, _ in P._fields_] == [name for _, name in fields]
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12] and C.sizeof(P) == 16
    assert re.search(r"#define RT_BLOOM_MAX_LEVELS 8u\b", PLAIN)


def prototype(text, name, returns="int"):
    args = re.search(r"\b" + returns + " " + name + r"\((.*?)\);", text, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def test_prototypes_and_host_cpu_parity():
    device, host, cpu = prototype(PLAIN, "rt_bloom"), prototype(PLAIN, "rt_bloom_host"), prototype(HOST_HEADER, "rt_bloom_cpu")
    types_of = lambda p: [re.sub(r"\w+$", "", a).strip() for a in p]
    assert types_of(device) == ["const float *", "uint32_t", "const rt_bloom_params *", "uint32_t", "uint32_t", "float *", "float *", "void *"]
    assert device[-1] == "void *hip_stream" and types_of(host) == types_of(device)[:-1] == types_of(cpu)  # the device form without the stream
    strip = lambda p: [re.sub(r"\b[dh]_", "", a) for a in p]
    assert strip(host) == strip(device)[:-1] == strip(cpu)  # and the same names
    assert prototype(PLAIN, "rt_bloom_temp_bytes", "size_t") == ["uint32_t rows", "uint32_t cols", "uint32_t n_levels"]
    amd, hostlib = _capi.amd_lib(), _capi.host_lib()
    pointer, word = C.c_void_p, C.c_uint32
    expected = [pointer, word, C.POINTER(_capi.BloomParams), word, word, pointer, pointer]
    assert amd.rt_bloom.argtypes == expected + [pointer]
    assert amd.rt_bloom_host.argtypes == expected and hostlib.rt_bloom_cpu.argtypes == expected
    assert amd.rt_bloom_temp_bytes.argtypes == [word, word, word] and amd.rt_bloom_temp_bytes.restype is C.c_size_t


def test_symbols_are_exported_and_listed_in_the_right_library_only():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and name not in _capi.HOST_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and name not in _capi.AMD_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays
    assert all(name in HOST_HEADER for name in HOST_NAMES)


# ---- the refusals: never read, every case ends in a check ----
BUF = (C.c_float * 64)()
OTHER = (C.c_float * 64)()
P, Q = C.cast(BUF, C.c_void_p), C.cast(OTHER, C.c_void_p)
VALID = dict(color=P, stride=3, threshold=1.0, knee=0.5, intensity=0.5, levels=3, rows=2, cols=2, temp=Q, out=Q)
# (what is wrong, the text), in the order of include/rt_amd.h; a case breaks its own item AND every later one that can be broken with it
REFUSALS = [
    (dict(params=None), "null params"),
    (dict(levels=0), "n_levels must be 1 .. 8"),
    (dict(threshold=-1.0), "threshold must be >= 0 (+inf: nothing glows)"),
    (dict(knee=math.inf), "knee must be finite and >= 0"),
    (dict(intensity=math.nan), "intensity must be finite and >= 0"),
    (dict(stride=2), "color_stride must be at least 3 words"),
    (dict(rows=65536, cols=65536), "rows * cols: 2^32 pixels or more"),
    (dict(color=None, out=None, temp=None), "null color pointer"),
]
ALONE = [
    (dict(levels=9), "n_levels must be 1 .. 8"),
    (dict(threshold=math.nan), "threshold must be >= 0 (+inf: nothing glows)"),
    (dict(knee=-0.5), "knee must be finite and >= 0"),
    (dict(knee=math.nan), "knee must be finite and >= 0"),
    (dict(intensity=-1.0), "intensity must be finite and >= 0"),
    (dict(intensity=math.inf), "intensity must be finite and >= 0"),
    (dict(stride=0), "color_stride must be at least 3 words"),
    (dict(out=None, temp=None), "null out pointer"),
    (dict(color=P, out=P, stride=4), "out may be color only with color_stride 3"),
]


def call_all_forms(**changes):
    """[(status, last error)] of rt_bloom_cpu, rt_bloom_host and rt_bloom on VALID with ``changes``"""
    a = dict(VALID, **changes)
    params = _capi.BloomParams(a["threshold"], a["knee"], a["intensity"], a["levels"])
    p = None if "params" in changes else C.byref(params)
    args = (a["color"], a["stride"], p, a["rows"], a["cols"], a["temp"], a["out"])
    amd, host = _capi.amd_lib(), _capi.host_lib()
    results = [(host.rt_bloom_cpu(*args), host.rt_host_last_error().decode())]
    results.append((amd.rt_bloom_host(*args), amd.rt_last_error().decode()))
    results.append((amd.rt_bloom(*args, None), amd.rt_last_error().decode()))
    return results


def expect_refused(results, text):
    for (status, message), who in zip(results, ("rt_bloom_cpu", "rt_bloom_host", "rt_bloom")):
        assert status == INVALID and message == f"{who}: {text}", (who, status, message)


@pytest.mark.parametrize("first", range(len(REFUSALS)))
def test_every_refusal_in_the_order_of_the_header(first):
    """item `first` broken together with every later one: the first refusal is its own"""
    changes = {}
    for wrong, _ in reversed(REFUSALS[first:]):
        changes.update(wrong)
    expect_refused(call_all_forms(**changes), REFUSALS[first][1])


@pytest.mark.parametrize("wrong,text", ALONE, ids=[f"{'-'.join(w)}-{k}" for k, (w, _) in enumerate(ALONE)])
def test_the_other_values_each_check_refuses(wrong, text):
    expect_refused(call_all_forms(**wrong), text)


def test_a_null_temp_is_refused_where_the_form_takes_it():
    """rt_bloom_cpu and rt_bloom take the caller's scratch; rt_bloom_host makes its own, so a null h_temp is not its refusal"""
    a = dict(VALID, temp=None)
    params = _capi.BloomParams(a["threshold"], a["knee"], a["intensity"], a["levels"])
    args = (a["color"], a["stride"], C.byref(params), a["rows"], a["cols"], None, a["out"])
    amd, host = _capi.amd_lib(), _capi.host_lib()
    assert host.rt_bloom_cpu(*args) == INVALID and host.rt_host_last_error().decode() == "rt_bloom_cpu: null temp pointer"
    assert amd.rt_bloom(*args, None) == INVALID and amd.rt_last_error().decode() == "rt_bloom: null temp pointer"
    # out == color with another stride comes after the pointers
    both = (P, 4, C.byref(params), 2, 2, None, P)
    assert host.rt_bloom_cpu(*both) == INVALID and host.rt_host_last_error().decode() == "rt_bloom_cpu: null temp pointer"


def test_an_empty_image_is_accepted_and_plus_infinity_is_a_threshold():
    for rows, cols in ((0, 4), (4, 0), (0, 0)):
        assert [status for status, _ in call_all_forms(rows=rows, cols=cols, color=None, out=None, temp=None)] == [0, 0, 0]
    # an empty image is still checked for what comes before it
    expect_refused(call_all_forms(rows=0, cols=4, stride=2), "color_stride must be at least 3 words")
    params = _capi.BloomParams(math.inf, 0.0, 0.0, 8)
    out, temp = (C.c_float * 12)(), (C.c_float * 64)()
    color = (C.c_float * 12)(*[2.0] * 12)
    assert _capi.host_lib().rt_bloom_cpu(color, 3, C.byref(params), 2, 2, temp, out) == 0 and list(out) == [2.0] * 12


@pytest.mark.parametrize("rows,cols", [(1, 1), (17, 13), (1080, 1920)])
def test_temp_bytes_is_the_sum_of_the_levels(rows, cols):
    amd = _capi.amd_lib()
    for levels in (1, 5, 8):
        sizes = S.level_sizes(rows, cols, levels)
        want = sum(r * c * 12 for r, c in sizes)
        assert amd.rt_bloom_temp_bytes(rows, cols, levels) == want == bloom.temp_bytes(rows, cols, levels) == 4 * bloom._temp_floats(rows, cols, levels)
    assert S.level_sizes(17, 17, 5) == [(9, 9), (5, 5), (3, 3), (2, 2), (1, 1)] and S.level_sizes(1, 1, 2) == [(1, 1), (1, 1)]
    assert amd.rt_bloom_temp_bytes(rows, cols, 0) == 0 and amd.rt_bloom_temp_bytes(rows, cols, 9) == 0


def test_the_options_are_appended_accepted_and_documented():
    amd = _capi.amd_lib()
    integration = (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
    for option in OPTIONS:
        assert option in HEADER and option in integration
        assert amd.rt_set_option(option.encode(), b"1") == 0 and amd.rt_set_option(option.encode(), None) == 0
    kernels_h = (_capi.REPO_ROOT / "homework-18-graphics-raytracer_amd" / "csrc" / "rt_kernels.h").read_text()
    table = re.sub(r"/\*.*?\*/", "", kernels_h[kernels_h.index("#define RT_OPTIONS(X)"):kernels_h.index("#define RT_OPTION_ID")], flags=re.S)
    names = re.findall(r'X\(\s*OPT_\w+\s*,[\s\\]*"(RT_AMD_\w+)"\s*\)', table)
    at = names.index("RT_AMD_DIAG_UPSAMPLE_MAX_GROUPS")  # the last enumerator before this block: nothing moved, these two come after it
    assert names[at + 1:] == list(OPTIONS) and names[0] == "RT_AMD_RNG_LOOKAHEAD" and at == 27


def test_the_header_states_the_block_its_place_and_what_it_does_not_cover():
    titles = re.findall(r"^/\* (---- [^\n]*?) -{4,}", HEADER, flags=re.M)
    at = next(k for k, t in enumerate(titles) if t.startswith("---- bloom queries:"))
    assert titles[at - 1].startswith("---- the step after the path, on the device") and titles[at + 1].startswith("---- film queries:")
    start = HEADER.index("---- bloom queries:")
    block = HEADER[start:HEADER.index("---- film queries:")]
    for words in AMD_NAMES + OPTIONS + ("l = (w0 * c_r + w1 * c_g) + w2 * c_b", "c - c != 0", "t = fminf(fmaxf(s + knee, 0), 2 * knee)", "q = (t * t) / (4 * knee)",
                                        "m = fmaxf(s, q)", "B_k = c_k * (m / l)", "h_kr = (s_0 + 3 * s_1) + (3 * s_2 + s_3)", "(1 / 64)",
                                        "far_r = clamp(near_r + (r odd ? 1 : -1))", "up = (3 * h_near + h_far) * (1 / 16)", "g = intensity / (float)L",
                                        "out_k = c_k + g * up(U_1)_k", "rows_j * cols_j * 12", "n_levels outside 1 .. RT_BLOOM_MAX_LEVELS",
                                        "out == color with color_stride != 3", "rt_bloom_cpu"):
        assert words in block, words
    not_covered = block[block.rindex("Not covered"):]
    for words in ("rt_multi_*", "neighbours' rows", "lens dirt", "anamorphic", "tone", "rt_render"):
        assert words in not_covered, words


def test_bloom_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.bloom, types.ModuleType) and rt.bloom is bloom
    assert list(bloom.__all__) == ["bloom", "bloom_numpy", "temp_bytes", "finish_frame"]
    for name in bloom.__all__:
        assert hasattr(bloom, name) and name not in rt.__all__, name
        assert name == "bloom" or not hasattr(rt, name), name  # rt.bloom is the module, never the function
    assert "bloom" not in rt.__all__ and callable(bloom.bloom)
    for other in (rt.film, rt.denoise, rt.temporal, rt.svgf, rt.moving, rt.rectify, rt.materials, rt.adaptive, rt.upsample):
        assert "bloom" not in other.__all__ and "finish_frame" not in other.__all__


def test_the_numpy_path_leaves_torch_and_hip_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import _capi, bloom\n"
            "img = np.full((5, 7, 3), 4.0, dtype=np.float32)\n"
            "out = bloom.bloom_numpy(img, levels=3)\n"
            "assert out.shape == (5, 7, 3) and out.dtype == np.float32 and (out > 4.0).all()\n"
            "assert 'torch' not in sys.modules and _capi._amd is None\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
