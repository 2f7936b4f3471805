"""The refraction-query ABI (include/rt_amd.h rt_refract_enter, rt_refract_step) without a GPU: the symbols exist and are listed, every
status of the documented check order is returned with its message before any device work and before the scene is read, an empty batch
is RT_OK, the Python wrappers check their arguments, and both level loops take the keyword that opens their casts."""
import ctypes as C
import inspect

import numpy as np
import pytest

import homework_18_graphics_raytracer_amd as rt
from homework_18_graphics_raytracer_amd import _capi

NAMES = ("rt_refract_enter", "rt_refract_step")


def test_refract_symbols_are_exported_and_listed():
    lib = _capi.amd_lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _capi.AMD_SYMBOLS, name
    assert lib.rt_abi_version() == 1  # additive: the version stays
    for name in ("refract_enter", "refract_step", "refract_rays_by_bounce", "refract_workspace"):
        assert name in rt.__all__ and callable(getattr(rt, name)), name
    assert rt.WALKING == 3 and "WALKING" in rt.__all__
    assert len({rt.ESCAPED, rt.INFINITE, rt.TRAPPED, rt.WALKING, _capi.RT_HIT_NONE}) == 5


def test_arguments_are_checked_before_device_work():
    lib = _capi.amd_lib()
    p = C.c_void_p(16)  # never dereferenced: every call below is refused on its arguments first, or has nothing to do
    fake = C.c_void_p(16)  # a scene that is never read

    def enter(n, scene=fake, ptrs=None):
        a = [p] * 7 if ptrs is None else ptrs
        return lib.rt_refract_enter(scene, a[0], a[1], n, a[2], a[3], a[4], a[5], a[6], None)

    def step(n, scene=fake, ptrs=None):
        a = [p] * 8 if ptrs is None else ptrs
        return lib.rt_refract_step(scene, a[0], n, 100.0, a[1], a[2], a[3], a[4], a[5], a[6], a[7], None)

    for fn, n_ptrs in ((enter, 7), (step, 8)):
        name = fn.__name__
        none = [None] * n_ptrs
        # 1. the limit: unsupported, named as such, and checked first — before the null scene, the empty batch and the pointers
        assert fn(1 << 32) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn((1 << 32) + 7, scene=None, ptrs=none) == -5 and b"2^32" in lib.rt_last_error(), name
        assert fn((1 << 32) - 1, ptrs=none) == -1 and b"pointer" in lib.rt_last_error(), name  # just below it: the next checks
        # 2. a null scene, before the empty batch and the pointers
        assert fn(2, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(2, scene=None, ptrs=none) == -1 and b"null scene" in lib.rt_last_error(), name
        assert fn(0, scene=None) == -1 and b"null scene" in lib.rt_last_error(), name
        # 3. nothing to do: status 0, no device work, and neither the scene nor a pointer is looked at
        assert fn(0) == 0, name
        assert fn(0, ptrs=none) == 0, name
        # 4. every pointer is required
        for missing in range(n_ptrs):
            ptrs = [p] * n_ptrs
            ptrs[missing] = None
            assert fn(2, ptrs=ptrs) == -1 and b"null" in lib.rt_last_error() and b"pointer" in lib.rt_last_error(), (name, missing)
        assert name[:5].encode() in lib.rt_last_error()  # the message names the call


def test_python_wrappers_check_their_arguments():
    hits, rays = np.zeros((3, 13), dtype=np.int32), np.zeros((3, 11), dtype=np.int32)
    with pytest.raises(ValueError):
        rt.refract_enter(None, hits, rays)  # not CUDA tensors
    with pytest.raises(ValueError):
        rt.refract_step(None, hits, hits, rays, np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.int32),
                        np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError):
        rt.refract_rays_by_bounce(None, hits, rays)
    torch = pytest.importorskip("torch")
    # CPU tensors of the right shape are refused as well, and so are wrong shapes and dtypes before anything else is looked at
    t_hits, t_rays = torch.zeros((3, 13), dtype=torch.int32), torch.zeros((3, 11), dtype=torch.int32)
    col = lambda dt: torch.zeros(3, dtype=dt)
    with pytest.raises(ValueError):
        rt.refract_enter(None, t_hits, t_rays)
    with pytest.raises(ValueError):
        rt.refract_enter(None, t_hits, t_rays[:2])
    with pytest.raises(ValueError):
        rt.refract_enter(None, t_hits.to(torch.float32), t_rays)
    with pytest.raises(ValueError):
        rt.refract_step(None, t_hits, t_hits, t_rays, col(torch.int32), col(torch.float32), col(torch.int32), col(torch.uint8))
    with pytest.raises(ValueError):
        rt.refract_step(None, t_hits, t_hits[:, :12], t_rays, col(torch.int32), col(torch.float32), col(torch.int32), col(torch.uint8))
    with pytest.raises(ValueError):
        rt.refract_rays_by_bounce(None, t_hits, torch.zeros((3, 10), dtype=torch.int32))
    with pytest.raises(ValueError):
        rt.refract_rays_by_bounce(None, t_hits, t_rays, rounds=-1)
    with pytest.raises(ValueError):
        rt.refract_rays_by_bounce(None, t_hits, t_rays, resume=True)  # nothing to resume from
    with pytest.raises(ValueError):
        rt.refract_rays_by_bounce(None, t_hits, t_rays, workspace=object())
    with pytest.raises(ValueError):
        rt.shade_hits_by_light(None, t_hits, torch.zeros((3, 10), dtype=torch.int32), workspace=object())


def test_open_casts_is_a_keyword_of_both_loops():
    for fn in (rt.trace_rays_levels, rt.trace_rays_distributed_levels):
        p = inspect.signature(fn).parameters
        assert "open_casts" in p and p["open_casts"].default is False, fn.__name__
    p = inspect.signature(rt.refract_rays_by_bounce).parameters
    assert list(p)[:9] == ["scene", "hits", "rays", "max_distance", "ray_count", "stream", "out", "rounds", "workspace"]
    assert p["max_distance"].default == 100.0 and p["rounds"].default == 11
    assert "workspace" in inspect.signature(rt.shade_hits_by_light).parameters
