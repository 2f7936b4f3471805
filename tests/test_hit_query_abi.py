"""The hit-query ABI (include/rt_amd.h rt_shade_hits / rt_reflect_rays / rt_refract_rays and the two _host forms) without a GPU: the
symbols exist and are listed, every status of the documented check order is returned with its message before any device work, an
empty batch is RT_OK, the records have the documented sizes, and without a device the host calls fail with a status and leave
their output buffers untouched."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_shade_hits", "rt_reflect_rays", "rt_refract_rays", "rt_shade_hits_host", "rt_refract_rays_host")


def test_hit_query_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays


def test_record_sizes():
    assert C.sizeof(_capi.Hit) == 52 and C.sizeof(_capi.Ray) == 44
    assert rt.HIT_DTYPE.itemsize == 52 and rt.RAY_DTYPE.itemsize == 44
    assert _capi.HIT_WORDS == 13 and _capi.RAY_WORDS == 11
    assert _capi.RT_HIT_NONE == 0xFFFFFFFF


def test_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    hits = (_capi.Hit * 2)()
    rays = (_capi.Ray * 2)()
    rgb = (C.c_float * 6)()
    out = (_capi.Ray * 2)()
    kind = (C.c_uint32 * 2)()
    travel = (C.c_float * 2)()
    cnt = C.c_ulonglong(5)
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do

    def shade(n, scene=fake, h=hits, r=rays, o=rgb):
        return lib.rt_shade_hits(scene, h, r, n, o, None, None)

    def shade_host(n, scene=fake, h=hits, r=rays, o=rgb):
        return lib.rt_shade_hits_host(scene, h, r, n, o, C.byref(cnt))

    def refract(n, scene=fake, h=hits, r=rays, o=out, k=kind, t=travel):
        return lib.rt_refract_rays(scene, h, r, n, 100.0, k, t, o, None, None)

    def refract_host(n, scene=fake, h=hits, r=rays, o=out, k=kind, t=travel):
        return lib.rt_refract_rays_host(scene, h, r, n, 100.0, k, t, o, C.byref(cnt))

    def reflect(n, scene=None, h=hits, r=rays, o=out):
        return lib.rt_reflect_rays(h, r, n, o, None)

    for fn in (shade, shade_host, refract, refract_host, reflect):
        with_scene = fn is not reflect
        # 1. 2^32 records or more: unsupported, named as such, and checked first
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error(), fn.__name__
        assert fn((1 << 32) + 7) == -5 and b"2^32" in lib.rt_last_error()
        assert fn(1 << 32, scene=None, h=None, r=None, o=None) == -5
        # 2. a null scene
        if with_scene:
            assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error(), fn.__name__
            assert fn(2, scene=None, h=None) == -1 and b"null scene" in lib.rt_last_error()
            assert fn(0, scene=None) == -1 and b"null scene" in lib.rt_last_error()  # before the empty batch
        # 3. nothing to do: status 0 and no device work (the fake scene is never read)
        assert fn(0) == 0, fn.__name__
        assert fn(0, h=None, r=None, o=None) == 0
        # 4. null hits, incoming or required output pointer with records to work on
        for bad in ({"h": None}, {"r": None}, {"o": None}):
            assert fn(2, **bad) == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (fn.__name__, bad)
    for fn in (refract, refract_host):
        assert fn(2, k=None) == -1 and b"pointer" in lib.rt_last_error()
        assert fn(0, t=None) == 0  # the travel output is optional
    assert cnt.value == 0  # the host calls' count of an empty batch
    assert all(v == 0.0 for v in rgb) and all(v == 0 for v in kind) and all(v == 0.0 for v in travel)
    assert bytes(out) == bytes(C.sizeof(out))


def test_band_hook_and_names_are_known():
    """the test hook that shortens the bands of a batch is an option of the library, and what a caller of rt.refract_rays needs to read
    `.kind` is exported"""
    lib = _capi.amd_lib()
    assert lib.rt_set_option(b"RT_AMD_DIAG_HIT_BAND_RECORDS", b"64") == 0
    assert lib.rt_set_option(b"RT_AMD_DIAG_HIT_BAND_RECORDS", None) == 0
    assert (rt.ESCAPED, rt.INFINITE, rt.TRAPPED, rt.HIT_NONE) == (0, 1, 2, -1)
    for name in ("ESCAPED", "INFINITE", "TRAPPED", "HIT_NONE", "Refractions", "shade_hits", "reflect_rays", "refract_rays"):
        assert name in rt.__all__, name


def test_python_wrappers_check_their_arguments():
    with pytest.raises(ValueError):
        rt.shade_hits(None, np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32))  # not CUDA tensors
    with pytest.raises(ValueError):
        rt.reflect_rays(np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32))
    with pytest.raises(ValueError):
        rt.refract_rays(None, np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32))
    with pytest.raises(ValueError):
        rt.shade_hits_numpy(None, np.zeros((3, 12), dtype=np.int32), np.zeros((3, 11), dtype=np.int32))
    with pytest.raises(ValueError):
        rt.refract_rays_numpy(None, np.zeros((3, 13), dtype=np.int32), np.zeros((2, 11), dtype=np.int32))  # one ray per hit


def test_no_device_fails_loudly_without_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_hit_queries.py covers the device path)")
    lib = _capi.amd_lib()
    hits = np.zeros(4, dtype=rt.HIT_DTYPE)
    hits["kind"] = 1
    hits["normal"] = (0.0, 1.0, 0.0)
    rays = np.zeros(4, dtype=rt.RAY_DTYPE)
    rays["direction"] = (0.0, -1.0, 0.0)
    rgb = np.full((4, 3), 7.0, dtype=np.float32)
    kind = np.full(4, 9, dtype=np.uint32)
    travel = np.full(4, 7.0, dtype=np.float32)
    escape = np.full((4, 11), 3, dtype=np.uint32)
    cnt = C.c_ulonglong(99)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # the arguments are fine, so the calls go on to the device, which is not there: a status, nothing computed on the host
    rc = lib.rt_shade_hits_host(C.c_void_p(16), p(hits), p(rays), 4, p(rgb), C.byref(cnt))
    assert rc in (-2, -3), rc
    assert (rgb == 7.0).all() and cnt.value == 99
    rc = lib.rt_refract_rays_host(C.c_void_p(16), p(hits), p(rays), 4, 100.0, p(kind), p(travel), p(escape), C.byref(cnt))
    assert rc in (-2, -3), rc
    assert (kind == 9).all() and (travel == 7.0).all() and (escape == 3).all() and cnt.value == 99
    assert lib.rt_shade_hits_host(None, p(hits), p(rays), 4, p(rgb), None) == -1
    assert (rgb == 7.0).all()
