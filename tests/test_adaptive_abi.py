"""The adaptive sampling queries' ABI and Python surface: the parameter struct against its ctypes mirror, the symbols in the right library
only, the appended option, rt.adaptive as a public submodule whose names stay off the top level and whose numpy path never loads torch,
and what the header says is not covered."""
import ctypes as C
import re
import subprocess
import sys
import types

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, adaptive

AMD_NAMES = ("rt_sample_budget", "rt_sample_list_temp_bytes", "rt_sample_list", "rt_film_offsets_listed", "rt_camera_rays_listed", "rt_film_splat_listed")
HOST_NAMES = ("rt_sample_budget_cpu", "rt_sample_list_cpu", "rt_film_offsets_listed_cpu", "rt_camera_rays_listed_cpu", "rt_film_splat_listed_cpu")
HEADER = (_capi.REPO_ROOT / "include" / "rt_amd.h").read_text()
OPTION = "RT_AMD_DIAG_ADAPTIVE_MAX_GROUPS"


def test_struct_size_and_offsets_match_the_header():
    body = re.search(r"typedef struct rt_sample_budget_params \{(.*?)\} rt_sample_budget_params;", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), flags=re.S).group(1)
    fields = [(m.group(1).strip(), m.group(2)) for m in re.finditer(r"([\w ]+?[ \*])(\w+);", body)]
    assert fields == [("float", "gain"), ("float", "epsilon"), ("uint32_t", "min_count"), ("uint32_t", "max_count"), ("uint32_t", "flags")]
    P = _capi.SampleBudgetParams
    assert [f for f, _ in P._fields_] == [name for _, name in fields]
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 4, 8, 12, 16] and C.sizeof(P) == 20
    assert re.search(r"#define RT_SAMPLE_MAX 64u", HEADER) and adaptive.SAMPLE_MAX == 64


def test_symbols_are_exported_and_listed_in_the_right_library_only():
    amd, host = _capi.amd_lib(), _capi.host_lib()
    for name in AMD_NAMES:
        assert hasattr(amd, name) and name in _capi.AMD_SYMBOLS and name not in _capi.HOST_SYMBOLS and not hasattr(host, name), name
    for name in HOST_NAMES:
        assert hasattr(host, name) and name in _capi.HOST_SYMBOLS and name not in _capi.AMD_SYMBOLS and not hasattr(amd, name), name
    assert amd.rt_abi_version() == 1  # additive: the version stays
    host_header = (_capi.REPO_ROOT / "include" / "rt_host.h").read_text()
    assert all(name in host_header for name in HOST_NAMES)
    assert not any(name + "_host" in HEADER for name in AMD_NAMES)  # no _host forms in this block


def test_temp_bytes_is_host_arithmetic():
    amd = _capi.amd_lib()
    sizes = [amd.rt_sample_list_temp_bytes(n) for n in (0, 1, 256, 257, 70001, (1 << 26) - 1, 1 << 26)]
    assert sizes == [0, 8, 8, 12, 4 * 275, 4 * ((1 << 18) + 1), 0]


def test_the_option_is_appended_accepted_and_documented():
    amd = _capi.amd_lib()
    assert OPTION in HEADER and OPTION in (_capi.REPO_ROOT / "INTEGRATION.md").read_text()
    assert amd.rt_set_option(OPTION.encode(), b"1") == 0 and amd.rt_set_option(OPTION.encode(), None) == 0
    kernels_h = (_capi.REPO_ROOT / "homework-18-graphics-raytracer_amd" / "csrc" / "rt_kernels.h").read_text()
    names = re.findall(r'X\(OPT_\w+,[\s\\]*"(RT_AMD_\w+)"\)', kernels_h)
    assert names[-1] == OPTION and names[-2] == "RT_AMD_DIAG_RECTIFY_MAX_GROUPS"  # no existing enumerator moved


def test_the_header_states_the_block_and_what_it_does_not_cover():
    start = HEADER.index("---- adaptive sampling queries:")
    assert HEADER.index("---- film queries:") < start < HEADER.index("---- denoise queries:")
    block = HEADER[start:HEADER.index("---- denoise queries:")]
    for words in AMD_NAMES + ("t < (float)range ? (uint32_t)t : range", "A negative variance", "start_i = min(S_i, capacity)", "first_i += start_(i+1) - start_i",
                              "pixel-major", "all-zero ray", "RT_FILM_STRATIFIED is RT_ERR_INVALID_ARGUMENT", "never causes a read outside [0, capacity)",
                              "rt_film_splat's bit for bit", "rt_accumulate_device's", OPTION):
        assert words in block, words
    not_covered = block[block.rindex("Not covered"):]
    for words in ("rt_multi_*", "tratified", "fixed total", "_host forms", "depth-of-field"):
        assert words in not_covered, words


def test_adaptive_is_a_public_submodule_off_the_top_level():
    assert isinstance(rt.adaptive, types.ModuleType) and rt.adaptive is adaptive
    assert sorted(adaptive.__all__) == sorted(["SAMPLE_MAX", "GAIN", "EPSILON", "SampleList", "budget", "budget_numpy", "list_temp_bytes", "sample_list",
                                               "sample_list_numpy", "offsets_listed", "offsets_listed_numpy", "camera_rays_listed", "camera_rays_listed_numpy",
                                               "splat_listed", "splat_listed_numpy", "render_pass", "render_adaptive"])
    for name in adaptive.__all__:
        assert hasattr(adaptive, name) and name not in rt.__all__ and not hasattr(rt, name), name
    assert "adaptive" not in rt.__all__
    for other in (rt.film, rt.denoise, rt.temporal, rt.svgf, rt.moving, rt.rectify, rt.materials):  # no submodule's public name is this module's
        assert "adaptive" not in other.__all__


def test_the_numpy_path_leaves_torch_and_hip_unloaded():
    code = (f"import sys\nsys.path.insert(0, {str(_capi.REPO_ROOT)!r})\nimport numpy as np\n"
            "import homework_18_graphics_raytracer_amd as rt\n"
            "from homework_18_graphics_raytracer_amd import _capi, adaptive, film\n"
            "frame = rt.Frame.full(5, 4, 2)\n"
            "counts = adaptive.budget_numpy(np.full(20, 0.5, dtype=np.float32), np.full(20, 0.25, dtype=np.float32), gain=4.0, epsilon=0.5, max_count=8)\n"
            "assert (counts == 1 + 2).all()\n"
            "sl = adaptive.sample_list_numpy(counts)\n"
            "assert sl.total.tolist() == [60, 60]\n"
            "off = adaptive.offsets_listed_numpy(frame, sl, 'uniform', 1)\n"
            "rays = adaptive.camera_rays_listed_numpy(rt.reference_camera(), frame, off, sl)\n"
            "f = film.Film(4, 5, 'tent', 1.0)\n"
            "adaptive.splat_listed(f, np.ones((60, 3), dtype=np.float32), off, sl, max_count=3)\n"
            "assert (f.weight > 0).all() and rays.shape == (60,)\n"
            "assert 'torch' not in sys.modules and _capi._amd is None\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr
