"""The area-light ABI (include/rt_amd.h rt_area_light_rays, rt_area_light_terms, rt_area_light_fold; include/rt_host.h
rt_area_light_samples_cpu) without a GPU: the symbols exist and are listed, every status of the documented check order is returned with
its message before any device work and before the scene is read, an empty batch is RT_OK, and the Python wrappers check their
arguments."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, arealights

NAMES = ("rt_area_light_rays", "rt_area_light_terms", "rt_area_light_fold")
CENTER, UNIFORM, STRATIFIED = 0, 1, 2


def test_area_light_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert hasattr(_capi.host_lib(), "rt_area_light_samples_cpu") and "rt_area_light_samples_cpu" in _capi.HOST_SYMBOLS
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("rays", "terms", "fold", "samples_numpy", "shade_hits_soft", "workspace", "Workspace"):
        assert callable(getattr(arealights, name)), name
    assert rt.arealights is arealights and "arealights" not in rt.__all__  # a submodule: the top-level surface gains no name
    assert (arealights.UNIFORM, arealights.STRATIFIED) == (UNIFORM, STRATIFIED)


def calls():
    lib = _capi.amd_lib()
    p = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    fake = C.c_void_p(16)  # a scene that is never read: the range of lights is checked last, after every refusal made here

    def rays(n, lights=1, spp=1, pattern=UNIFORM, scene=fake, a=p, b=p, c=p):
        return lib.rt_area_light_rays(scene, a, p, n, 0, lights, c, None, spp, pattern, 0, b, p, p, None)

    def terms(n, lights=1, spp=1, pattern=None, scene=fake, a=p, b=p, c=p):
        return lib.rt_area_light_terms(scene, a, p, n, 0, lights, spp, p, c, p, p, p, b, None)

    def fold(n, lights=1, spp=1, pattern=None, scene=fake, a=p, b=p, c=p):
        return lib.rt_area_light_fold(scene, a, n, lights, spp, c, p, p, b, None, None)

    return lib, (rays, terms, fold)


def test_arguments_are_checked_before_device_work():
    lib, fns = calls()
    for fn in fns:
        name = fn.__name__
        # 1. the limits: unsupported, named as such, and checked first — before the null scene, the empty batch, the pointers and spp
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn((1 << 32) + 7, scene=None, a=None, b=None) == -5, name
        assert fn(1 << 32, lights=0) == -5 and b"2^32" in lib.rt_last_error(), name  # n alone, whatever the lights
        assert fn(1 << 16, lights=1 << 16) == -5 and b"2^32" in lib.rt_last_error(), name  # n * light_count
        assert fn(1 << 16, lights=1 << 10, spp=64) == -5 and b"2^32" in lib.rt_last_error(), name  # n * light_count * spp
        assert fn(1 << 16, lights=1 << 10, spp=64, scene=None, a=None) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn(1 << 31, lights=1, spp=2, scene=None) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn(1 << 16, lights=1 << 16, spp=0) == -5 and b"2^32" in lib.rt_last_error(), name  # the pairs, whatever spp
        assert fn((1 << 32) - 1, a=None) == -1, name  # just below it: the next checks
        assert fn((1 << 16) - 1, lights=1 << 10, spp=64, a=None) == -1 and b"pointer" in lib.rt_last_error(), name
        # 2. a null scene, before the empty batch
        assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(2, lights=0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(2, spp=0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name  # before spp
        # 3. nothing to do: status 0, no device work, the scene is not read — and spp is not looked at
        assert fn(0) == 0, name
        assert fn(0, a=None, b=None) == 0, name
        assert fn(5, lights=0) == 0, name
        assert fn(0, spp=0) == 0 and fn(0, spp=65) == 0, name
        assert fn(0, lights=0xFFFFFFFF, spp=0xFFFFFFFF) == 0, name
        # 4. a null required pointer with entries to work on, before spp
        for bad in ({"a": None}, {"b": None}, {"c": None}):
            assert fn(2, **bad) == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, bad)
            assert fn(2, spp=0, **bad) == -1 and b"pointer" in lib.rt_last_error(), (name, bad)
        # 5. spp, with a message that names the limit; before the scene is read
        for spp in (0, 65, 1 << 20):
            assert fn(2, spp=spp) == -1 and b"1 .. 64" in lib.rt_last_error(), (name, spp)
    # ... and the pattern, which rt_area_light_rays alone takes
    rays = fns[0]
    assert rays(2, spp=4, pattern=CENTER) == -1 and b"RT_FILM_CENTER" in lib.rt_last_error()
    assert rays(2, spp=4, pattern=3) == -1 and b"unknown pattern" in lib.rt_last_error()
    assert rays(2, spp=5, pattern=STRATIFIED) == -1 and b"k * k" in lib.rt_last_error()
    assert rays(2, spp=0, pattern=CENTER) == -1 and b"1 .. 64" in lib.rt_last_error()  # spp before the pattern
    assert rays(0, spp=5, pattern=STRATIFIED) == 0 and rays(0, pattern=CENTER) == 0  # n == 0 is RT_OK


def test_optional_pointers_are_optional():
    """d_ids and d_visibility may be NULL; with a required pointer missing it is that pointer the message names"""
    lib, _ = calls()
    p, fake = C.c_void_p(16), C.c_void_p(16)
    for missing in range(6):
        args = [p] * 6
        args[missing] = None
        rc = lib.rt_area_light_rays(fake, args[0], args[1], 4, 0, 1, args[2], None, 1, UNIFORM, 0, args[3], args[4], args[5], None)
        assert rc == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), missing
    assert lib.rt_area_light_rays(fake, p, p, 0, 0, 1, p, None, 1, UNIFORM, 0, p, p, p, None) == 0
    assert lib.rt_area_light_fold(fake, p, 0, 1, 1, p, p, p, p, None, None) == 0


def test_the_cpu_sampler_checks_its_arguments():
    lib = _capi.host_lib()
    light = (_capi.Light * 1)()
    radii, out = (C.c_float * 1)(0.5), (C.c_float * (3 * 64 * 4))()
    call = lambda n=4, count=1, spp=1, pattern=UNIFORM, lights=light, r=radii, o=out: lib.rt_area_light_samples_cpu(lights, 0, count, r, None, n, spp, pattern, 7, o)
    assert call() == 0
    assert call(n=1 << 32) == -5 and b"2^32" in lib.rt_host_last_error()
    assert call(n=1 << 16, count=1 << 10, spp=64, lights=None) == -5
    assert call(n=0, spp=0) == 0 and call(count=0, lights=None) == 0
    assert call(lights=None) == -1 and b"pointer" in lib.rt_host_last_error()
    assert call(r=None) == -1 and call(o=None) == -1
    for spp in (0, 65):
        assert call(spp=spp) == -1 and b"1 .. 64" in lib.rt_host_last_error()
    assert call(pattern=CENTER) == -1 and b"RT_FILM_CENTER" in lib.rt_host_last_error()
    assert call(spp=5, pattern=STRATIFIED) == -1 and b"k * k" in lib.rt_host_last_error()
    assert call(spp=64, pattern=STRATIFIED) == 0
    with pytest.raises(rt.RtError):
        arealights.samples_numpy([light[0]], [0.5], 4, 5, STRATIFIED)
    with pytest.raises(ValueError):
        arealights.samples_numpy([light[0]], [0.5, 0.5], 4, 4)


def test_python_wrappers_check_their_arguments():
    hits, rays = np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32)
    f3 = np.zeros((3, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        arealights.rays(None, hits, rays, np.zeros(1, dtype=np.float32), 1)  # not CUDA tensors
    with pytest.raises(ValueError):
        arealights.terms(None, hits, rays, np.zeros(3, dtype=np.uint8), f3, hits, 1)
    with pytest.raises(ValueError):
        arealights.fold(None, hits, np.zeros(3, dtype=np.uint8), f3, f3, f3, 1)
    with pytest.raises(ValueError):
        arealights.shade_hits_soft(None, hits, rays, np.zeros(1, dtype=np.float32))
    torch = pytest.importorskip("torch")
    t_hits, t_rays = torch.zeros((3, 13), dtype=torch.int32), torch.zeros((3, 11), dtype=torch.int32)
    with pytest.raises(ValueError):
        arealights.rays(None, t_hits, t_rays, torch.zeros(1), 1)  # CPU tensors
    with pytest.raises(ValueError):
        arealights.shade_hits_soft(None, t_hits, t_rays[:2], torch.zeros(1))
