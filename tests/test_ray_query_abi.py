"""The ray-query ABI (include/rt_amd.h rt_cast_rays / rt_cast_rays_host / rt_camera_rays) without a GPU: the symbols exist, the
records have the oracle's layout, arguments are checked before any device work, and without a device there is no CPU path."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi
import _oracle

NAMES = ("rt_cast_rays", "rt_cast_rays_host", "rt_camera_rays")


def test_query_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays


def test_records_have_the_oracle_layout():
    assert C.sizeof(_capi.Ray) == 44 and C.sizeof(_capi.Hit) == 52
    for ours, theirs in ((_capi.Ray, _oracle.OrcRay), (_capi.Hit, _oracle.OrcHit)):
        assert C.sizeof(ours) == C.sizeof(theirs)
        assert [f[0] for f in ours._fields_] == [f[0] for f in theirs._fields_]
        for name, _ in ours._fields_:
            assert getattr(ours, name).offset == getattr(theirs, name).offset, name
            assert getattr(ours, name).size == getattr(theirs, name).size, name
    # the numpy views of the same records
    assert rt.RAY_DTYPE.itemsize == 44 and rt.HIT_DTYPE.itemsize == 52
    for dt, st in ((rt.RAY_DTYPE, _capi.Ray), (rt.HIT_DTYPE, _capi.Hit)):
        for name, _ in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset, name
    assert _capi.RT_HIT_NONE == 0xFFFFFFFF and rt.HIT_NONE == -1


def test_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    rays = (_capi.Ray * 2)()
    hits = (_capi.Hit * 2)()
    fake = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first
    # null scene
    assert lib.rt_cast_rays(None, rays, 2, hits, None) == -1 and b"null" in lib.rt_last_error()
    assert lib.rt_cast_rays_host(None, rays, 2, hits) == -1
    # null ray / hit pointers with rays to cast
    assert lib.rt_cast_rays(fake, None, 2, hits, None) == -1
    assert lib.rt_cast_rays(fake, rays, 2, None, None) == -1
    assert lib.rt_cast_rays_host(fake, None, 2, hits) == -1
    assert lib.rt_cast_rays_host(fake, rays, 2, None) == -1
    # 2^32 rays or more: unsupported, named as such
    for fn in (lambda n: lib.rt_cast_rays(fake, rays, n, hits, None), lambda n: lib.rt_cast_rays_host(fake, rays, n, hits)):
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error()
        assert fn((1 << 32) + 7) == -5
    # camera rays: null camera / frame / output, invalid frames, a tile of 2^32 pixels
    cam = rt.reference_camera()
    good = rt.Frame.full(16, 8, 5)
    assert lib.rt_camera_rays(None, C.byref(good), fake, None) == -1
    assert lib.rt_camera_rays(C.byref(cam), None, fake, None) == -1
    assert lib.rt_camera_rays(C.byref(cam), C.byref(good), None, None) == -1
    for bad in (rt.Frame(10, 10, 5, 0, 0, 11, 10, 1), rt.Frame(10, 10, 5, 0, 0, 10, 10, 0), rt.Frame(10, 10, 5, 4, 0, 4, 10, 1),
                rt.Frame(0, 10, 5, 0, 0, 0, 10, 1)):
        assert lib.rt_camera_rays(C.byref(cam), C.byref(bad), fake, None) == -1 and b"frame" in lib.rt_last_error()
    huge = rt.Frame.full(65536, 65536, 5)
    assert lib.rt_camera_rays(C.byref(cam), C.byref(huge), fake, None) == -5 and b"2^32" in lib.rt_last_error()


def test_python_packing_checks_its_arguments():
    with pytest.raises(ValueError):
        rt.cast_rays_numpy(None, np.zeros((3, 10), dtype=np.int32))
    with pytest.raises(ValueError):
        rt.make_rays(np.zeros((2, 3), dtype=np.float32), np.zeros((2, 3), dtype=np.float32))  # not CUDA tensors


def test_no_device_fails_loudly_without_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_ray_query.py covers the device path)")
    lib = _capi.amd_lib()
    # no scene can exist without a device, so there is nothing to cast against; the host call fails with a status
    with pytest.raises(rt.RtError) as ei:
        rt.Scene(rt.reference_world())
    assert ei.value.code in (-2, -3)
    rays = np.zeros(4, dtype=rt.RAY_DTYPE)
    rays["direction"] = (0.0, 0.0, -1.0)
    hits = np.zeros(4, dtype=rt.HIT_DTYPE)
    assert lib.rt_cast_rays_host(None, rays.ctypes.data_as(C.c_void_p), 4, hits.ctypes.data_as(C.c_void_p)) == -1
    assert (hits.view(np.uint32) == 0).all()  # nothing was computed on the host instead
