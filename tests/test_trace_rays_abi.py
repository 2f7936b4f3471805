"""The radiance-query ABI (include/rt_amd.h rt_trace_rays / rt_trace_rays_host) without a GPU: the symbols exist and are listed,
arguments are refused with their status and message before any device work, and without a device the host call fails with a
status and computes nothing on the host."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_trace_rays", "rt_trace_rays_host")


def test_trace_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays


def test_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    rays = (_capi.Ray * 2)()
    rgb = (C.c_float * 6)()
    cnt = C.c_ulonglong(5)
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do

    def dev(n, scene=fake, r=rays, out=rgb, depth=5, contribution=1.0):
        return lib.rt_trace_rays(scene, r, n, depth, contribution, out, None, None)

    def host(n, scene=fake, r=rays, out=rgb, depth=5, contribution=1.0):
        return lib.rt_trace_rays_host(scene, r, n, depth, contribution, out, C.byref(cnt))

    for fn in (dev, host):
        # 2^32 rays or more: unsupported, named as such, and checked first
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error()
        assert fn((1 << 32) + 7) == -5 and b"2^32" in lib.rt_last_error()
        assert fn(1 << 32, scene=None, r=None, out=None, depth=33) == -5
        # a null scene
        assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error()
        # nothing to trace: status 0 and no device work (the fake scene is never read)
        assert fn(0) == 0
        assert fn(0, r=None, out=None, contribution=float("nan")) == 0
        # null ray / rgb pointers with rays to trace
        assert fn(2, r=None) == -1 and b"null ray or rgb pointer" in lib.rt_last_error()
        assert fn(2, out=None) == -1 and b"null ray or rgb pointer" in lib.rt_last_error()
        # max_depth above RT_MAX_DEPTH
        assert fn(2, depth=33) == -5 and b"RT_MAX_DEPTH" in lib.rt_last_error()
        assert fn(2, depth=1 << 30) == -5
    assert cnt.value == 0  # the host call's count of an empty batch
    assert all(v == 0.0 for v in rgb)


def test_python_wrappers_check_their_arguments():
    with pytest.raises(ValueError):
        rt.trace_rays_numpy(None, np.zeros((3, 10), dtype=np.int32), 5)
    with pytest.raises(ValueError):
        rt.trace_rays(None, np.zeros((3, 11), dtype=np.int32), 5)  # not a CUDA tensor


def test_no_device_fails_loudly_without_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_trace_rays.py covers the device path)")
    lib = _capi.amd_lib()
    rays = np.zeros(4, dtype=rt.RAY_DTYPE)
    rays["direction"] = (0.0, 0.0, -1.0)
    rgb = np.full((4, 3), 7.0, dtype=np.float32)
    cnt = C.c_ulonglong(99)
    # the arguments are fine, so the call goes on to the device, which is not there: a status, nothing computed on the host
    rc = lib.rt_trace_rays_host(C.c_void_p(16), rays.ctypes.data_as(C.c_void_p), 4, 5, 1.0, rgb.ctypes.data_as(C.c_void_p), C.byref(cnt))
    assert rc in (-2, -3, -4), rc
    assert (rgb == 7.0).all() and cnt.value == 99
    assert lib.rt_trace_rays_host(None, rays.ctypes.data_as(C.c_void_p), 4, 5, 1.0, rgb.ctypes.data_as(C.c_void_p), None) == -1
    assert (rgb == 7.0).all()
