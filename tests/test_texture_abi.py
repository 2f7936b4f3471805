"""The texture ABI (include/rt_amd.h "texture queries"; include/rt_texture_host.h the CPU forms) without a GPU: the symbols exist and
are listed, the size functions are host arithmetic, every status of the documented check order is returned with its message before any
device work, an empty batch is RT_OK, and the Python wrappers check their arguments."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, textures

INCLUDE = Path(__file__).resolve().parent.parent / "include"
NAMES = ("rt_texture_levels", "rt_texture_pyramid_floats", "rt_texture_pyramid", "rt_texture_footprint", "rt_texture_sample", "rt_texture_surfaces",
         "rt_light_terms_surfaces")
HOST_NAMES = ("rt_texture_pyramid_cpu", "rt_texture_footprint_cpu", "rt_texture_sample_cpu", "rt_texture_surfaces_cpu")
P = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do


def desc(width=8, height=4, texels=16, n_levels=1, filter=0, wrap_u=0, wrap_v=0):
    return _capi.TextureDesc(texels, width, height, n_levels, filter, wrap_u, wrap_v, (C.c_float * 2)(1.0, 1.0), (C.c_float * 2)(0.0, 0.0))


def declaration(header, name):
    text = re.sub(r"/\*.*?\*/", "", (INCLUDE / header).read_text(), flags=re.S)
    found = re.findall(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", text)
    assert len(found) == 1, name
    return [" ".join(p.split()) for p in found[0].split(",")]


def test_texture_symbols_are_exported_and_listed():
    lib, host = _capi.amd_lib(), _capi.host_lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in _capi.AMD_SYMBOLS and not hasattr(host, name), name
    header = (INCLUDE / "rt_texture_host.h").read_text()
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == sorted(HOST_NAMES) == sorted(_capi.TEXTURE_HOST_SYMBOLS)
    for name in HOST_NAMES:
        assert hasattr(host, name) and not hasattr(lib, name) and name not in _capi.HOST_SYMBOLS, name
    assert '#include "rt_texture_host.h"' in (INCLUDE / "rt_host.h").read_text()
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("Texture", "HostTexture", "Binding", "pyramid", "footprint", "sample", "apply", "light_terms_surfaces", "pyramid_numpy", "footprint_numpy",
                 "sample_numpy", "apply_numpy", "levels", "pyramid_floats", "workspace", "shade_hits_textured", "trace_rays_levels"):
        assert callable(getattr(textures, name)), name
    assert rt.textures is textures and "textures" not in rt.__all__  # a submodule: the top-level surface gains no name
    text = (INCLUDE / "rt_amd.h").read_text()
    for name, value in (("NEAREST", 0), ("BILINEAR", 1), ("TRILINEAR", 2), ("REPEAT", 0), ("CLAMP", 1), ("MODULATE", 1), ("NORMALIZE", 2), ("MAX_SIDE", 16384)):
        assert getattr(textures, name) == value and re.search(rf"#define RT_TEX_{name} {value}u", text), name
    assert textures.ALL_OBJECTS == 0xFFFFFFFF and "#define RT_TEX_ALL_OBJECTS 0xffffffffu" in text
    assert C.sizeof(_capi.TextureDesc) == 48


def test_the_declared_signatures():
    assert declaration("rt_amd.h", "rt_texture_pyramid") == ["const rt_texture *tex", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_texture_footprint") == [
        "const rt_scene *scene", "const rt_hit *d_hits", "const rt_ray *d_incoming", "size_t n", "float spread", "const float *d_width0", "float *d_footprint",
        "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_texture_sample") == [
        "const rt_texture *tex", "const float *d_uv", "size_t uv_stride_words", "const float *d_footprint", "size_t n", "float *d_out",
        "size_t out_stride_words", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_texture_surfaces") == [
        "const rt_texture *diffuse_tex", "const rt_texture *normal_tex", "const rt_hit *d_hits", "const float *d_footprint", "size_t n",
        "uint32_t object_index", "uint32_t flags", "rt_surface *d_surfaces", "void *hip_stream"]
    assert declaration("rt_amd.h", "rt_light_terms_surfaces") == [
        "const rt_scene *scene", "const rt_surface *d_surfaces", "const rt_hit *d_hits", "const rt_ray *d_incoming", "size_t n", "uint32_t light_first",
        "uint32_t light_count", "const unsigned char *d_asks", "const rt_hit *d_shadow_hits", "unsigned char *d_lit", "float *d_diffuse",
        "float *d_specular", "void *hip_stream"]
    lib = _capi.amd_lib()
    for name, device, cpu in (("pyramid", 2, 1), ("footprint", 8, 7), ("sample", 8, 7), ("surfaces", 9, 8)):
        assert len(getattr(lib, "rt_texture_" + name).argtypes) == device
        assert len(declaration("rt_texture_host.h", f"rt_texture_{name}_cpu")) == cpu  # the device form's arguments without the stream
    assert len(lib.rt_light_terms_surfaces.argtypes) == 13
    assert declaration("rt_texture_host.h", "rt_texture_footprint_cpu")[0] == "const rt_scene_desc *scene"  # as rt_previous_positions_cpu takes it


def test_the_size_functions():
    assert textures.levels(5, 3) == 3 and textures.levels(1, 1) == 1 and textures.levels(7, 1) == 3 and textures.levels(33, 65) == 7
    assert textures.levels(16384, 16384) == 15 and textures.levels(0, 4) == 0 and textures.levels(4, 0) == 0
    assert textures.pyramid_floats(1, 1, 1) == 3 and textures.pyramid_floats(5, 3, 1) == 45
    assert textures.pyramid_floats(5, 3, 3) == 3 * (15 + 2 * 1 + 1)  # 5x3, 2x1, 1x1
    assert textures.pyramid_floats(7, 1, 3) == 3 * (7 + 3 + 1) and textures.pyramid_floats(64, 64, 7) == 3 * sum(4 ** k for k in range(7))
    assert textures.pyramid_floats(16384, 16384, 15) == 3 * sum(4 ** k for k in range(15))
    for over in ((16385, 1, 1), (1, 16385, 1), (0, 1, 1), (1, 0, 1), (5, 3, 0), (5, 3, 4), (1, 1, 2), (1 << 32, 1, 1)):
        assert textures.pyramid_floats(*over) == 0, over


def test_the_descriptor_is_checked_first_and_in_order():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    pyramid = lambda d: lib.rt_texture_pyramid(None if d is None else C.byref(d), None)
    cases = ((None, -1, b"null texture"), (desc(texels=None), -1, b"null texture texels"), (desc(width=0), -1, b"width or height 0"),
             (desc(height=0, width=20000), -1, b"width or height 0"), (desc(width=16385), -5, b"16384"), (desc(height=16385, n_levels=0), -5, b"16384"),
             (desc(n_levels=0), -1, b"n_levels"), (desc(n_levels=5), -1, b"n_levels"), (desc(filter=3, wrap_u=2), -1, b"unknown filter"),
             (desc(wrap_u=2), -1, b"unknown wrap"), (desc(wrap_v=7), -1, b"unknown wrap"))
    for d, status, text in cases:
        assert pyramid(d) == status and text in err() and err().startswith(b"rt_texture_pyramid: "), text
        host = _capi.host_lib()
        assert host.rt_texture_pyramid_cpu(None if d is None else C.byref(d)) == status and text in host.rt_host_last_error(), text
        assert host.rt_host_last_error().decode().split(": ", 1)[1] == err().decode().split(": ", 1)[1]  # the same texts
    assert pyramid(desc(n_levels=1)) == 0  # level 0 only: nothing to launch


def test_footprint_sample_and_surfaces_check_their_arguments():
    lib = _capi.amd_lib()
    err = lib.rt_last_error
    foot = lambda n, scene=P, a=P, b=P, c=P: lib.rt_texture_footprint(scene, a, b, n, 0.5, None, c, None)
    assert foot(1 << 32) == -5 and b"2^32" in err() and foot(1 << 32, scene=None, a=None) == -5  # the count, first
    assert foot(2, scene=None) == -1 and b"null scene" in err() and foot(0, scene=None) == -1  # before the empty batch
    assert foot(0) == 0 and foot(0, a=None, b=None, c=None) == 0
    for bad in ({"a": None}, {"b": None}, {"c": None}):
        assert foot(2, **bad) == -1 and b"null hit, incoming-ray or footprint pointer" in err(), bad

    good = desc()
    sample = lambda n, d=good, uv=P, out=P, us=13, os=3: lib.rt_texture_sample(None if d is None else C.byref(d), uv, us, None, n, out, os, None)
    assert sample(1 << 32, d=None) == -5 and b"2^32" in err()
    assert sample(0, d=None) == -1 and b"null texture" in err()  # the descriptor before the empty batch
    assert sample(2, d=desc(filter=9), uv=None) == -1 and b"unknown filter" in err()
    assert sample(0) == 0 and sample(0, uv=None, out=None, us=0, os=0) == 0
    for bad in ({"uv": None}, {"out": None}):
        assert sample(2, us=0, **bad) == -1 and b"null uv or output pointer" in err(), bad  # the pointers before the strides
    assert sample(2, us=1) == -1 and b"uv_stride_words" in err() and sample(2, os=2) == -1 and b"out_stride_words" in err()

    surf = lambda n, d=good, m=None, hits=P, out=P, flags=0: lib.rt_texture_surfaces(None if d is None else C.byref(d), None if m is None else C.byref(m),
                                                                                     hits, None, n, 0xFFFFFFFF, flags, out, None)
    assert surf(1 << 32, d=desc(width=0)) == -5 and b"2^32" in err()
    assert surf(0, d=desc(width=0)) == -1 and b"width or height 0" in err()
    assert surf(0, m=desc(wrap_v=3)) == -1 and b"unknown wrap" in err()
    assert surf(0) == 0 and surf(0, hits=None, out=None, flags=99) == 0
    for bad in ({"hits": None}, {"out": None}):
        assert surf(2, flags=4, **bad) == -1 and b"null hit or surface pointer" in err(), bad
    assert surf(2, flags=4) == -1 and b"unknown flags" in err()
    assert surf(2, d=None) == 0 and surf(2, d=None, flags=8) == -1  # no texture: nothing to do, once the arguments are in order

    terms = lambda n, count=1, scene=P, s=P, a=P: lib.rt_light_terms_surfaces(scene, s, a, P, n, 0, count, P, P, P, P, P, None)
    light = lambda n, count=1, scene=P, a=P: lib.rt_light_terms(scene, a, P, n, 0, count, P, P, P, P, P, None)
    for args in ({"n": 1 << 32}, {"n": 1 << 20, "count": 1 << 12}, {"n": 2, "scene": None}, {"n": 0, "scene": None}):
        status = terms(**args)
        mine = err().decode()
        assert light(**args) == status < 0
        assert mine.split(": ", 1)[1] == err().decode().split(": ", 1)[1] and mine.startswith("rt_light_terms_surfaces: ")  # the neighbour's messages
    assert terms(0) == 0 and terms(3, count=0, s=None) == 0
    assert terms(2, s=None) == -1 and b"null surface, hit" in err() and terms(2, a=None) == -1 and b"pointer" in err()


def test_the_cpu_forms_check_like_the_device_forms():
    host = _capi.host_lib()
    err = host.rt_host_last_error
    good = desc()
    assert host.rt_texture_sample_cpu(None, P, 2, None, 1 << 32, P, 3) == -5 and b"2^32" in err()
    assert host.rt_texture_sample_cpu(None, P, 2, None, 0, P, 3) == -1 and b"null texture" in err()
    assert host.rt_texture_sample_cpu(C.byref(good), None, 2, None, 0, None, 3) == 0
    assert host.rt_texture_sample_cpu(C.byref(good), None, 2, None, 2, P, 3) == -1 and b"null uv or output pointer" in err()
    assert host.rt_texture_sample_cpu(C.byref(good), P, 1, None, 2, P, 3) == -1 and b"uv_stride_words" in err()
    assert host.rt_texture_surfaces_cpu(C.byref(good), None, None, None, 2, 0, 0, P) == -1 and b"null hit or surface pointer" in err()
    assert host.rt_texture_surfaces_cpu(C.byref(good), None, P, None, 2, 0, 4, P) == -1 and b"unknown flags" in err()
    assert host.rt_texture_surfaces_cpu(None, None, P, None, 2, 0, 0, P) == 0
    assert host.rt_texture_footprint_cpu(None, P, P, 1 << 32, 0.0, None, P) == -5 and b"2^32" in err()
    assert host.rt_texture_footprint_cpu(None, P, P, 2, 0.0, None, P) == -1 and b"null scene" in err()
    scene = rt.reference_world().desc()
    assert host.rt_texture_footprint_cpu(C.byref(scene), None, None, 0, 0.0, None, None) == 0
    assert host.rt_texture_footprint_cpu(C.byref(scene), None, P, 2, 0.0, None, P) == -1 and b"null hit, incoming-ray or footprint pointer" in err()


def test_the_python_wrappers_check_their_arguments():
    image = np.zeros((3, 5, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        textures.HostTexture(image[..., :2])
    with pytest.raises(ValueError):
        textures.HostTexture(image, n_levels=4)
    tex = textures.HostTexture(image)
    assert (tex.n_levels, tex.floats, tex.level(1).shape, tex.level(2).shape) == (3, 54, (1, 2, 3), (1, 1, 3))
    with pytest.raises(ValueError):
        tex.level(3)
    with pytest.raises(ValueError):
        textures.HostTexture.over(np.zeros(53, dtype=np.float32), 5, 3)
    with pytest.raises(ValueError):
        textures.sample_numpy(image, np.zeros((2, 2), dtype=np.float32))  # a HostTexture is wanted
    with pytest.raises(ValueError):
        textures.sample_numpy(tex, np.zeros((2, 2), dtype=np.float32), footprint=np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError):
        textures.apply_numpy(np.zeros((2, 18), dtype=np.uint32), np.zeros((3, 13), dtype=np.uint32), tex)
    with pytest.raises(ValueError):
        textures.Binding(diffuse=tex)  # a device Texture is wanted
    with pytest.raises(_capi.RtError):
        tex.filter = 5
        textures.sample_numpy(tex, np.zeros((2, 2), dtype=np.float32))
