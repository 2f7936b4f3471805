"""The scene-update ABI (include/rt_amd.h rt_scene_update_vertices / _spheres / _lights / _materials) without a GPU: the four symbols are
exported with the header's signatures and listed, a null scene is refused first — whatever the other arguments are, an empty range
included — and writes nothing, and the Python methods exist.  (A scene cannot be created without a device, so the checks that read
it — the range, the empty range, the null data pointer, the validation of lights and materials — are in tests/test_gpu_scene_update.py.)"""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_scene_update_vertices", "rt_scene_update_spheres", "rt_scene_update_lights", "rt_scene_update_materials")
HEADER = Path(__file__).resolve().parent.parent / "include" / "rt_amd.h"


def test_update_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("update_vertices", "update_spheres", "update_lights", "update_materials"):
        assert callable(getattr(rt.Scene, name)), name
        assert list(inspect.signature(getattr(rt.Scene, name)).parameters)[:3] == ["self", "first", name[len("update_"):]], name


def test_header_signatures():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    want = {
        "rt_scene_update_vertices": "const rt_vertex *d_vertices",
        "rt_scene_update_spheres": "const rt_sphere *d_spheres",
        "rt_scene_update_lights": "const rt_light *h_lights",
        "rt_scene_update_materials": "const rt_material *h_materials",
    }
    for name, data in want.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert args == ["rt_scene *scene", "uint32_t first", "uint32_t count", data, "void *hip_stream"], (name, args)
    # ... and the bindings pass exactly those five arguments
    lib = _capi.amd_lib()
    for name in NAMES:
        assert len(getattr(lib, name).argtypes) == 5, name


def test_a_null_scene_is_refused_first_and_writes_nothing():
    lib = _capi.amd_lib()
    lights = (_capi.Light * 2)()
    lights[0].kind = 99  # would be refused later: the null scene comes first
    materials = (_capi.Material * 2)()
    before_l, before_m = bytes(lights), bytes(materials)
    device_ptr = C.c_void_p(16)  # never dereferenced
    calls = {
        "rt_scene_update_vertices": device_ptr, "rt_scene_update_spheres": device_ptr,
        "rt_scene_update_lights": lights, "rt_scene_update_materials": materials,
    }
    for name, data in calls.items():
        fn = getattr(lib, name)
        for first, count, ptr in ((0, 2, data), (0, 0, data), (0, 0, None), (0xFFFFFFFF, 0xFFFFFFFF, data), (5, 1, None)):
            assert fn(None, first, count, ptr, None) == -1, (name, first, count)
            msg = lib.rt_last_error()
            assert b"null scene" in msg and name.encode() in msg, (name, msg)
    assert bytes(lights) == before_l and bytes(materials) == before_m


def test_python_methods_check_their_arguments_before_the_library():
    import pytest

    scene = rt.Scene.__new__(rt.Scene)  # no device: never reaches the library
    scene._h = None
    with pytest.raises(ValueError):
        scene.update_vertices(0, _cpu_tensor())
    with pytest.raises(ValueError):
        scene.update_spheres(0, _cpu_tensor())
    with pytest.raises(ValueError):
        scene.update_vertices(0, np.zeros(25, dtype=np.float32))  # not whole triangles (24 floats each)
    with pytest.raises(ValueError):
        scene.update_spheres(0, np.zeros(7, dtype=np.float32))  # not whole rt_sphere records (5 words each)


def _cpu_tensor():
    import torch

    return torch.zeros((3, 8), dtype=torch.float32)  # not on the device
