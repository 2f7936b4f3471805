"""The hemisphere ABI (include/rt_amd.h rt_hemisphere_rays, rt_hemisphere_fold; include/rt_host.h rt_hemisphere_dirs_cpu,
rt_hemisphere_fold_cpu) without a GPU: the symbols exist and are listed, every status of the documented check order is returned with
its message before any device work and before the scene is read, an empty batch is RT_OK, d_rgb and d_radiance go together, and the
Python wrappers check their arguments."""
import ctypes as C

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi, hemisphere

NAMES = ("rt_hemisphere_rays", "rt_hemisphere_fold")
HOST_NAMES = ("rt_hemisphere_dirs_cpu", "rt_hemisphere_fold_cpu")
CENTER, UNIFORM, STRATIFIED = 0, 1, 2
INF = float("inf")


def test_hemisphere_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    for name in HOST_NAMES:
        assert hasattr(_capi.host_lib(), name) and name in _capi.HOST_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("rays", "fold", "dirs_numpy", "fold_numpy", "ambient_hits", "indirect_hits", "workspace", "Workspace"):
        assert callable(getattr(hemisphere, name)), name
    assert rt.hemisphere is hemisphere and "hemisphere" not in rt.__all__  # a submodule: the top-level surface gains no name
    assert (hemisphere.UNIFORM, hemisphere.STRATIFIED) == (UNIFORM, STRATIFIED)
    assert (hemisphere.SHADING, hemisphere.GEOMETRIC) == (0, 1)


def calls():
    lib = _capi.amd_lib()
    p = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    fake = C.c_void_p(16)  # a scene that is never read

    def rays(n, spp=1, pattern=UNIFORM, kind=0, scene=fake, a=p, b=p, c=p):
        return lib.rt_hemisphere_rays(scene, a, n, None, spp, pattern, 0, kind, b, c, p, None)

    def fold(n, spp=1, pattern=None, kind=None, scene=fake, a=p, b=p, c=p):
        return lib.rt_hemisphere_fold(scene, a, n, spp, b, None, INF, None, c, None, None, None)  # c: d_open, optional

    return lib, (rays, fold)


def test_arguments_are_checked_before_device_work():
    lib, fns = calls()
    for fn in fns:
        name = fn.__name__
        # 1. the limits: unsupported, named as such, and checked first — before the null scene, the empty batch, the pointers and spp
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn((1 << 32) + 7, scene=None, a=None, b=None) == -5, name
        assert fn(1 << 32, spp=0) == -5 and b"2^32" in lib.rt_last_error(), name  # n alone, whatever spp
        assert fn(1 << 26, spp=64) == -5 and b"2^32" in lib.rt_last_error(), name  # n * spp
        assert fn(1 << 26, spp=64, scene=None, a=None) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn(1 << 31, spp=2, scene=None) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn(3, spp=0xFFFFFFFF) == -5 and b"2^32" in lib.rt_last_error(), name  # before spp's own limit
        assert fn((1 << 32) - 1, a=None) == -1, name  # just below it: the next checks
        assert fn((1 << 26) - 1, spp=64, a=None) == -1 and b"pointer" in lib.rt_last_error(), name
        # 2. a null scene, before the empty batch
        assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(2, spp=0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name  # before spp
        # 3. nothing to do: status 0, no device work, the scene is not read — and spp is not looked at
        assert fn(0) == 0, name
        assert fn(0, a=None, b=None) == 0, name
        assert fn(0, spp=0) == 0 and fn(0, spp=65) == 0 and fn(0, spp=0xFFFFFFFF) == 0, name
        # 4. a null required pointer with entries to work on, before spp
        for bad in ({"a": None}, {"b": None}):
            assert fn(2, **bad) == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, bad)
            assert fn(2, spp=0, **bad) == -1 and b"pointer" in lib.rt_last_error(), (name, bad)
        # 5. spp, with a message that names the limit; before the scene is read
        for spp in (0, 65, 1 << 20):
            assert fn(2, spp=spp) == -1 and b"1 .. 64" in lib.rt_last_error(), (name, spp)
    # ... and the pattern and the normal kind, which rt_hemisphere_rays alone takes: the area lights' texts
    rays, fold = fns
    assert rays(2, c=None) == -1 and b"pointer" in lib.rt_last_error()  # d_asks is required there
    assert rays(2, spp=4, pattern=CENTER) == -1 and b"RT_FILM_CENTER" in lib.rt_last_error()
    assert rays(2, spp=4, pattern=3) == -1 and b"unknown pattern" in lib.rt_last_error()
    assert rays(2, spp=5, pattern=STRATIFIED) == -1 and b"k * k" in lib.rt_last_error()
    assert rays(2, spp=0, pattern=CENTER) == -1 and b"1 .. 64" in lib.rt_last_error()  # spp before the pattern
    assert rays(2, spp=4, kind=2) == -1 and b"normal_kind" in lib.rt_last_error() and b"RT_HEMISPHERE_GEOMETRIC" in lib.rt_last_error()
    assert rays(2, spp=4, pattern=CENTER, kind=2) == -1 and b"RT_FILM_CENTER" in lib.rt_last_error()  # the pattern before the kind
    assert rays(0, spp=5, pattern=STRATIFIED) == 0 and rays(0, pattern=CENTER) == 0 and rays(0, kind=7) == 0  # n == 0 is RT_OK


def test_optional_pointers_and_the_pair_of_the_bounce():
    """d_ids, d_shadow_hits, d_open, d_ambient may be NULL; d_rgb and d_radiance are given together or not at all"""
    lib, _ = calls()
    p, fake = C.c_void_p(16), C.c_void_p(16)
    for missing in range(4):
        args = [p] * 4
        args[missing] = None
        rc = lib.rt_hemisphere_rays(fake, args[0], 4, None, 1, UNIFORM, 0, 0, args[1], args[2], args[3], None)
        assert rc == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), missing
    fold = lambda radiance, rgb, n=4, spp=1: lib.rt_hemisphere_fold(fake, p, n, spp, p, None, INF, radiance, None, None, rgb, None)
    assert fold(p, None) == -1 and b"radiance or rgb" in lib.rt_last_error() and b"pointer" in lib.rt_last_error()
    assert fold(None, p) == -1 and b"radiance or rgb" in lib.rt_last_error()
    assert fold(p, None, spp=0) == -1 and b"radiance or rgb" in lib.rt_last_error()  # a pointer check: before spp
    assert fold(p, None, n=0) == 0 and fold(None, p, n=0) == 0  # ... and after the empty batch
    assert fold(p, p, spp=65) == -1 and b"1 .. 64" in lib.rt_last_error()  # both given: on to the next check
    assert fold(None, None, spp=65) == -1 and b"1 .. 64" in lib.rt_last_error()


def test_the_cpu_forms_check_their_arguments():
    lib = _capi.host_lib()
    normals, out = (C.c_float * 12)(*([0.0, 0.0, 1.0] * 4)), (C.c_float * (3 * 64 * 4))()
    dirs = lambda n=4, spp=1, pattern=UNIFORM, a=normals, o=out: lib.rt_hemisphere_dirs_cpu(a, None, n, spp, pattern, 7, o)
    assert dirs() == 0
    assert dirs(n=1 << 32) == -5 and b"2^32" in lib.rt_host_last_error()
    assert dirs(n=1 << 26, spp=64, a=None) == -5
    assert dirs(n=0, spp=0) == 0 and dirs(n=0, a=None, o=None) == 0
    assert dirs(a=None) == -1 and b"pointer" in lib.rt_host_last_error()
    assert dirs(o=None) == -1
    for spp in (0, 65):
        assert dirs(spp=spp) == -1 and b"1 .. 64" in lib.rt_host_last_error()
    assert dirs(pattern=CENTER) == -1 and b"RT_FILM_CENTER" in lib.rt_host_last_error()
    assert dirs(spp=5, pattern=STRATIFIED) == -1 and b"k * k" in lib.rt_host_last_error()
    assert dirs(spp=64, pattern=STRATIFIED) == 0
    hits, valid, asks = (C.c_uint32 * (13 * 4))(), (C.c_ubyte * 4)(), (C.c_ubyte * 8)()
    colour, shiness, radiance, rgb = (C.c_float * 12)(), (C.c_float * 4)(), (C.c_float * 24)(), (C.c_float * 12)()
    fold = lambda n=4, spp=2, h=hits, v=valid, a=asks, rad=None, out=None: lib.rt_hemisphere_fold_cpu(h, v, colour, shiness, n, spp, a, None, INF, rad, None,
                                                                                                 None, out)
    assert fold() == 0 and fold(rad=radiance, out=rgb) == 0
    assert fold(n=1 << 32) == -5 and fold(n=1 << 31, spp=2, h=None) == -5 and b"2^32" in lib.rt_host_last_error()
    assert fold(n=0, spp=0, h=None) == 0
    assert fold(h=None) == -1 and fold(v=None) == -1 and fold(a=None) == -1 and b"pointer" in lib.rt_host_last_error()
    assert fold(rad=radiance) == -1 and b"radiance or rgb" in lib.rt_host_last_error()
    assert fold(out=rgb) == -1 and b"radiance or rgb" in lib.rt_host_last_error()
    assert fold(spp=0) == -1 and b"1 .. 64" in lib.rt_host_last_error()
    with pytest.raises(rt.RtError):
        hemisphere.dirs_numpy(np.zeros((4, 3), dtype=np.float32), 5, STRATIFIED)
    with pytest.raises(ValueError):
        hemisphere.dirs_numpy(np.zeros((4, 2), dtype=np.float32), 4)
    with pytest.raises(ValueError):
        hemisphere.fold_numpy(np.zeros((4, 13), dtype=np.uint32), np.ones(4), np.zeros((4, 3)), np.zeros(4), np.zeros(7), 2)  # asks: 8 entries
    with pytest.raises(ValueError):
        hemisphere.fold_numpy(np.zeros((4, 13), dtype=np.uint32), np.ones(4), np.zeros((4, 3)), np.zeros(4), np.zeros(8), 2, radiance=np.zeros((8, 3)))


def test_python_wrappers_check_their_arguments():
    hits = np.zeros((3, 13), dtype=np.int32)
    with pytest.raises(ValueError):
        hemisphere.rays(None, hits, 1)  # not CUDA tensors
    with pytest.raises(ValueError):
        hemisphere.fold(None, hits, np.zeros(3, dtype=np.uint8), 1)
    with pytest.raises(ValueError):
        hemisphere.ambient_hits(None, hits, 4)
    with pytest.raises(ValueError):
        hemisphere.indirect_hits(None, hits, 4, 2)
    with pytest.raises(ValueError):
        hemisphere.workspace(-1, "cpu", 4)
    torch = pytest.importorskip("torch")
    t_hits = torch.zeros((3, 13), dtype=torch.int32)
    with pytest.raises(ValueError):
        hemisphere.rays(None, t_hits, 1)  # CPU tensors
    with pytest.raises(ValueError):
        hemisphere.fold(None, t_hits, torch.zeros(3, dtype=torch.uint8), 1)
    with pytest.raises(ValueError):
        hemisphere.rays(None, t_hits, -1)
