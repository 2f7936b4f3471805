"""The stochastic radiance-query ABI (include/rt_amd.h rt_rng_create_seeded / rt_rng_upload / rt_trace_rays_distributed /
rt_trace_rays_distributed_host / rt_focus_rays) without a GPU: the symbols exist and are listed, arguments are refused with their
status and message before any device work and in the documented order, and without a device the host call fails with a status and
computes nothing on the host.

The checks that follow "n_rays differs from the rng's count" need an rt_rng whose count equals a non-zero n_rays, which only a
device can hold; up to there the order is pinned here, with an EMPTY seeded rt_rng (made without a device), and the rest of it in
tests/test_gpu_trace_rays_distributed.py::test_argument_order_with_a_live_rng."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_rng_create_seeded", "rt_rng_upload", "rt_trace_rays_distributed", "rt_trace_rays_distributed_host", "rt_focus_rays")
INVALID, UNSUPPORTED = -1, -5


def test_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays


def test_seeded_rng_arguments_and_the_empty_object():
    lib = _capi.amd_lib()
    h = C.c_void_p(77)
    # 2^32 generators or more: unsupported, checked first (the seed pointer is never read, the out pointer not written)
    assert lib.rt_rng_create_seeded(None, 1 << 32, None) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
    assert lib.rt_rng_create_seeded(C.c_void_p(16), (1 << 32) + 5, C.byref(h)) == UNSUPPORTED and h.value == 77
    assert lib.rt_rng_create_seeded(C.c_void_p(16), 3, None) == INVALID
    assert lib.rt_rng_create_seeded(None, 3, C.byref(h)) == INVALID and b"null seed pointer" in lib.rt_last_error()
    assert not h.value  # cleared before anything can fail
    # n == 0: a valid empty object, made without a device; it downloads and uploads nothing
    assert lib.rt_rng_create_seeded(None, 0, C.byref(h)) == 0 and h.value
    word = (C.c_uint32 * 1)(123)
    assert lib.rt_rng_download(h, word) == 0 and lib.rt_rng_upload(h, word) == 0 and word[0] == 123
    assert lib.rt_rng_upload(None, word) == INVALID and lib.rt_rng_upload(h, None) == INVALID
    assert lib.rt_rng_destroy(h) == 0
    empty = rt.Rng.seeded([])
    assert empty.count == 0 and empty.download().shape == (0, lib.rt_rng_state_words())
    empty.close()


def test_arguments_are_checked_before_device_work_and_in_order():
    lib = _capi.amd_lib()
    rays = (_capi.Ray * 2)()
    acc = (C.c_float * 6)()
    cnt = C.c_ulonglong(5)
    fake = C.c_void_p(16)  # a scene that is never dereferenced: every call below is refused on its arguments first, or has nothing to do
    empty = C.c_void_p()
    assert lib.rt_rng_create_seeded(None, 0, C.byref(empty)) == 0

    def dev(n, scene=fake, r=rays, rng=empty, epochs=1, out=acc, depth=5):
        return lib.rt_trace_rays_distributed(scene, r, n, depth, rng, epochs, out, None, None, None, None)

    def host(n, scene=fake, r=rays, rng=empty, epochs=1, out=acc, depth=5):
        return lib.rt_trace_rays_distributed_host(scene, r, n, depth, rng, epochs, out, C.byref(cnt))

    for fn in (dev, host):
        # 2^32 rays or more: unsupported, named as such, and checked first — before the null scene, the null rng, everything
        assert fn(1 << 32) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
        assert fn((1 << 32) + 7, scene=None, r=None, rng=None, out=None, depth=33) == UNSUPPORTED and b"2^32" in lib.rt_last_error()
        # a null scene, then a null rng
        assert fn(2, scene=None, rng=None) == INVALID and b"null scene" in lib.rt_last_error()
        assert fn(2, rng=None) == INVALID and b"null rng" in lib.rt_last_error()
        assert fn(0, rng=None) == INVALID and b"null rng" in lib.rt_last_error()  # even with nothing to trace
        # the count: two rays, no generators — before the null ray pointer, the missing outputs and max_depth
        assert fn(2) == INVALID and b"different number of generators" in lib.rt_last_error()
        assert fn(2, r=None, out=None, depth=33, epochs=0) == INVALID and b"different number of generators" in lib.rt_last_error()
        # nothing to trace: status 0 and no device work (the fake scene is never read), whatever else is missing
        assert fn(0) == 0
        assert fn(0, r=None, out=None, depth=33) == 0
    assert cnt.value == 0  # the host call's count of an empty batch
    assert all(v == 0.0 for v in acc)
    assert lib.rt_rng_destroy(empty) == 0


def test_focus_rays_arguments():
    lib = _capi.amd_lib()
    cam = rt.reference_camera()
    frame = rt.Frame.full(8, 4, 5)
    empty = C.c_void_p()
    assert lib.rt_rng_create_seeded(None, 0, C.byref(empty)) == 0
    out = C.c_void_p(16)  # never written: every call is refused first
    assert lib.rt_focus_rays(None, C.byref(frame), 3.0, 0.04, empty, out, None) == INVALID
    assert lib.rt_focus_rays(C.byref(cam), None, 3.0, 0.04, empty, out, None) == INVALID
    assert lib.rt_focus_rays(C.byref(cam), C.byref(frame), 3.0, 0.04, None, out, None) == INVALID
    bad = rt.Frame(8, 4, 5, 0, 0, 8, 4, 0)
    assert lib.rt_focus_rays(C.byref(cam), C.byref(bad), 3.0, 0.04, empty, out, None) == INVALID and b"bad frame" in lib.rt_last_error()
    assert lib.rt_focus_rays(C.byref(cam), C.byref(frame), 3.0, 0.04, empty, None, None) == INVALID and b"null ray pointer" in lib.rt_last_error()
    # 32 pixels, no generators
    assert lib.rt_focus_rays(C.byref(cam), C.byref(frame), 3.0, 0.04, empty, out, None) == INVALID and b"different" in lib.rt_last_error()
    assert lib.rt_rng_destroy(empty) == 0


def test_render_distributed_refuses_a_seeded_rng():
    """A seeded rt_rng has no frame geometry: rt_render_distributed refuses it on its arguments, before any device work."""
    lib = _capi.amd_lib()
    cam = rt.reference_camera()
    frame = rt.Frame.full(8, 4, 5)
    empty = C.c_void_p()
    assert lib.rt_rng_create_seeded(None, 0, C.byref(empty)) == 0
    rc = lib.rt_render_distributed(C.c_void_p(16), C.byref(cam), C.byref(frame), 3.0, 0.04, empty, 1, C.c_void_p(16), None, None, None, None)
    assert rc == INVALID and b"different tile" in lib.rt_last_error()
    assert lib.rt_rng_destroy(empty) == 0


def test_python_wrappers_check_their_arguments():
    with pytest.raises(ValueError):
        rt.trace_rays_distributed_numpy(None, np.zeros((3, 10), dtype=np.int32), 5, None, 1, np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        rt.trace_rays_distributed_numpy(None, np.zeros((3, 11), dtype=np.int32), 5, None, 1, np.zeros((2, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        rt.trace_rays_distributed(None, np.zeros((3, 11), dtype=np.int32), 5, None)  # not a CUDA tensor
    empty = rt.Rng.seeded([])
    with pytest.raises(ValueError):
        empty.upload(np.zeros((1, 516), dtype=np.uint32))
    empty.close()


def test_no_device_fails_loudly_without_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_gpu_trace_rays_distributed.py covers the device path)")
    lib = _capi.amd_lib()
    # generators need device memory: a status, and no object
    seeds = np.arange(4, dtype=np.uint64)
    h = C.c_void_p(77)
    rc = lib.rt_rng_create_seeded(seeds.ctypes.data_as(C.c_void_p), 4, C.byref(h))
    assert rc in (-2, -3, -4), rc
    assert not h.value
    with pytest.raises(rt.RtError):
        rt.Rng.seeded([1, 2, 3])
    # so no host call can get past the count check with rays to trace; with the empty object it has nothing to do and says so
    empty = C.c_void_p()
    assert lib.rt_rng_create_seeded(None, 0, C.byref(empty)) == 0
    rays = np.zeros(4, dtype=rt.RAY_DTYPE)
    rays["direction"] = (0.0, 0.0, -1.0)
    acc = np.full((4, 3), 7.0, dtype=np.float32)
    cnt = C.c_ulonglong(99)
    rc = lib.rt_trace_rays_distributed_host(C.c_void_p(16), rays.ctypes.data_as(C.c_void_p), 4, 5, empty, 1, acc.ctypes.data_as(C.c_void_p), C.byref(cnt))
    assert rc == INVALID
    assert (acc == 7.0).all() and cnt.value == 99
    assert lib.rt_trace_rays_distributed_host(None, rays.ctypes.data_as(C.c_void_p), 4, 5, empty, 1, acc.ctypes.data_as(C.c_void_p), None) == INVALID
    assert (acc == 7.0).all()
    assert lib.rt_rng_destroy(empty) == 0
