"""The light-query ABI (include/rt_amd.h rt_light_rays, rt_light_terms, rt_light_fold) without a GPU: the symbols exist and are listed,
every status of the documented check order is returned with its message before any device work and before the scene is read, an empty
batch is RT_OK, and the Python wrappers check their arguments."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_light_rays", "rt_light_terms", "rt_light_fold")


def test_light_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("light_rays", "light_terms", "light_fold", "shade_hits_by_light"):
        assert name in rt.__all__ and callable(getattr(rt, name)), name


def test_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    p = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    fake = C.c_void_p(16)  # a scene that is never read: the range of lights is checked last, after every refusal made here

    def rays(n, lights=1, scene=fake, a=p, b=p, c=p):
        return lib.rt_light_rays(scene, a, p, n, 0, lights, b, p, c, None)

    def terms(n, lights=1, scene=fake, a=p, b=p, c=p):
        return lib.rt_light_terms(scene, a, p, n, 0, lights, p, c, p, p, b, None)

    def fold(n, lights=1, scene=fake, a=p, b=p, c=p):
        return lib.rt_light_fold(scene, a, n, lights, c, p, p, b, None)

    for fn in (rays, terms, fold):
        name = fn.__name__
        # 1. the limits: unsupported, named as such, and checked first — before the null scene, the empty batch and the pointers
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn((1 << 32) + 7, scene=None, a=None, b=None) == -5, name
        assert fn(1 << 32, lights=0) == -5 and b"2^32" in lib.rt_last_error(), name  # n alone, whatever the lights
        assert fn(1 << 16, lights=1 << 16) == -5 and b"2^32" in lib.rt_last_error(), name  # n * light_count
        assert fn(1 << 31, lights=2, scene=None, a=None) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn((1 << 32) - 1, a=None) == -1, name  # just below it: the next checks
        assert fn((1 << 16) - 1, lights=1 << 16, a=None) == -1 and b"pointer" in lib.rt_last_error(), name
        # 2. a null scene, before the empty batch
        assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(2, scene=None, a=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(2, lights=0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        # 3. nothing to do: status 0, no device work, and the scene is not read
        assert fn(0) == 0, name
        assert fn(0, a=None, b=None) == 0, name
        assert fn(5, lights=0) == 0, name
        assert fn(5, lights=0, a=None, b=None) == 0, name
        assert fn(0, lights=0xFFFFFFFF) == 0, name
        # 4. a null required pointer with pairs to work on
        for bad in ({"a": None}, {"b": None}) + (({"c": None},) if fn is not rays else ()):
            assert fn(2, **bad) == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, bad)


def test_the_pair_limit_is_exact():
    """n * light_count is formed in 64 bits: 3 * (2^32 - 1) does not wrap below the limit"""
    lib = _capi.amd_lib()
    p, fake = C.c_void_p(16), C.c_void_p(16)
    assert lib.rt_light_rays(fake, None, p, 3, 0, 0xFFFFFFFF, p, p, None, None) == -5 and b"2^32" in lib.rt_last_error()
    assert lib.rt_light_fold(fake, None, 3, 0xFFFFFFFF, p, p, p, p, None) == -5 and b"2^32" in lib.rt_last_error()
    assert lib.rt_light_terms(fake, None, p, 65537, 0, 65535, p, p, p, p, p, None) == -1 and b"pointer" in lib.rt_last_error()  # 2^32 - 1 pairs


def test_a_null_light_distance_is_accepted():
    """d_light_distance may be NULL: with every other pointer given the call gets past the pointer check — here on an empty batch, so
    that nothing is launched; with a required pointer missing it is that pointer the message names"""
    lib = _capi.amd_lib()
    p, fake = C.c_void_p(16), C.c_void_p(16)
    assert lib.rt_light_rays(fake, p, p, 0, 0, 3, p, p, None, None) == 0
    assert lib.rt_light_rays(fake, p, p, 4, 0, 0, p, p, None, None) == 0
    for missing in range(4):
        args = [p, p, p, p]
        args[missing] = None
        rc = lib.rt_light_rays(fake, args[0], args[1], 4, 0, 1, args[2], args[3], None, None)
        assert rc == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), missing


def test_python_wrappers_check_their_arguments():
    hits, rays = np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32)
    with pytest.raises(ValueError):
        rt.light_rays(None, hits, rays)  # not CUDA tensors
    with pytest.raises(ValueError):
        rt.light_terms(None, hits, rays, np.zeros(3, dtype=np.uint8), hits)
    with pytest.raises(ValueError):
        rt.light_fold(None, hits, np.zeros(3, dtype=np.uint8), np.zeros((3, 3), dtype=np.float32), np.zeros((3, 3), dtype=np.float32),
                      np.zeros((3, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        rt.shade_hits_by_light(None, hits, rays)
    torch = pytest.importorskip("torch")
    # CPU tensors of the right shape are refused as well, and so are wrong shapes and dtypes before anything else is looked at
    t_hits, t_rays = torch.zeros((3, 13), dtype=torch.int32), torch.zeros((3, 11), dtype=torch.int32)
    with pytest.raises(ValueError):
        rt.light_rays(None, t_hits, t_rays)
    with pytest.raises(ValueError):
        rt.light_rays(None, t_hits, t_rays[:2])
    with pytest.raises(ValueError):
        rt.light_terms(None, t_hits.to(torch.float32), t_rays, torch.zeros(3, dtype=torch.uint8), t_hits)
    with pytest.raises(ValueError):
        rt.light_fold(None, t_hits[:, :12], torch.zeros(3, dtype=torch.uint8), torch.zeros((3, 3)), torch.zeros((3, 3)), torch.zeros((3, 3)))
    with pytest.raises(ValueError):
        rt.shade_hits_by_light(None, t_hits, torch.zeros((3, 10), dtype=torch.int32))
